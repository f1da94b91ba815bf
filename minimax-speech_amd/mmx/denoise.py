"""Spectral-gate noise reduction of reference clips on the device: the reference's SpectralGate
(dac-vae/audiotools/ml/layers/spectral_gate.py, which audiotools' transforms.NoiseReduce wraps), the Audacity-style gate, over a
ragged batch of mono clips in five launches of csrc/denoise.hip (mmx_gate_threshold, mmx_gate_analyze, mmx_gate_synthesize),
without a host sync.  The synthesis half is an inverse STFT on the spectral tile of csrc/spec_tile.h.

Definitions (spectral_gate.py:90-127 and AudioSignal.stft / istft restated; audiotools is not a dependency, DESIGN.md §2, restated
seams).  Window length n, hop n // 4, w = sqrt of the periodic Hann window held in fp32 (AudioSignal.get_window("sqrt_hann")):
    X = torch.stft(x, n, hop, window=w, center=True)            [n // 2 + 1, 1 + len // hop]; reflection by n // 2: len > n // 2
    N = the same of the noise clip;   dB(.) = 20 log10 max(|.|, 1e-4)
    thresh[k] = mean_t dB(N)[k, t] + n_std * std_t dB(N)[k, t]   (unbiased std, torch's default)
    m = dB(X) < thresh                                          (strict)
    smooth = conv2d(m, outer(tri(n_freq), tri(n_time)) / sum, zero padding), tri(p) = (1 .. p + 1 .. 1) / (p + 1): 7 x 11 taps by default
    y = torch.istft(X * (1 - denoise_amount * smooth), n, hop, window=w, center=True, length=len)
Every clip is gated on its own [bins, frames] grid: a shorter member of a batch sees zeros, not its neighbour or the padding, past
its last frame.  In integer units (1 .. p + 1 .. 1) the taps sum to (n_freq + 1)^2 (n_time + 1)^2, so smooth is an integer count
over that number: the device evaluates it exactly.

The noise statistics come from a noise clip the caller names: one shared clip, one per member, or a span (start, stop) of each clip
itself (the Audacity workflow: point at the room tone before the speaker starts).  There is deliberately no "statistics of the whole
clip" default: mean + 3 std of a clip's own dB lies above nearly every bin of that clip, every bin is masked and the output is
silence.

Tables are float64 -> three bf16 planes (mel.packed3), built once per (n, device).  There is no CPU fallback: a CPU tensor raises
MmxError."""
import math

import torch

from . import clips as CL
from . import mel as MEL
from . import ops
from ._lib import MmxError, call, stream, _p

LDS_BYTES = 160 * 1024
FRAMES_PER_TILE, GAP, CHUNK = 32, 16, 17                 # csrc/denoise.hip: GT_ROWS (two 16-frame tiles of spec_tile.h), GT_GAP, GT_CHUNK
MAX_WINDOW = 2048                                        # csrc/denoise.hip: GT_MAX_N, up to where the LDS carve-ups are stated and tested
MAX_SMOOTH = 14                                          # n_freq, n_time: the time-smoothed counts (<= (n_time + 1)^2) are bytes in LDS
FLOOR = 1e-4                                             # spectral_gate.py:99 magnitude.clamp(1e-4)


def frames_of(n, win_length):
    """Frames of a clip of n samples: torch.stft(center=True) with hop win_length // 4."""
    return 1 + n // (win_length // 4)


def padded_bins(win_length):
    return ops.round_up(win_length // 2 + 1, 32)


def lds_bytes(win_length, kernel="synth"):
    """Dynamic LDS of csrc/denoise.hip's kernels, which take 32 frames per workgroup.  "synth" (gt_synth_lds): the time-smoothed
    mask counts uint8 [32][padded_bins] plus ONE K chunk - at most 17 steps of 32 of the 2 * padded_bins columns (real parts, then
    imaginary parts) - of the gated frames as three bf16 planes [3][32][32 * steps + 8]; the chunks pass through the same planes in
    turn, their products added in chunk order.  "stft" (gt_stft_lds): the sample planes of 32 frames."""
    nbp = padded_bins(win_length)
    if kernel == "synth":
        return FRAMES_PER_TILE * nbp + 3 * FRAMES_PER_TILE * (32 * min(CHUNK, 2 * nbp // 32) + 8) * 2
    hop = win_length // 4
    span = (FRAMES_PER_TILE - 1) * hop + win_length
    return 3 * 2 * (span + GAP * -(-span // hop))


def refusal(lens, win_length, hop_length=None, n_freq=3, n_time=5):
    """Why the gate refuses these clip (or noise clip) lengths in this form (nothing is launched then), or None."""
    n = int(win_length)
    if n < 32 or n % 32:
        return f"win_length {n} is not a positive multiple of 32"
    if hop_length is not None and int(hop_length) * 4 != n:
        return f"hop_length {hop_length} is not win_length // 4 = {n // 4}"
    if max(lds_bytes(n), lds_bytes(n, "stft")) > LDS_BYTES:
        return f"the planes of win_length {n} need {max(lds_bytes(n), lds_bytes(n, 'stft'))} bytes of LDS"
    if n > MAX_WINDOW:
        return f"win_length {n} is above {MAX_WINDOW}, the largest window the kernels are built and tested for"
    if not (0 <= int(n_freq) <= MAX_SMOOTH and 0 <= int(n_time) <= MAX_SMOOTH):
        return f"n_freq {n_freq} / n_time {n_time} outside [0, {MAX_SMOOTH}]"
    short = [v for v in lens if v <= n // 2]
    if short:
        return f"a clip of {short[0]} samples cannot be reflected by {n // 2}"
    return None


# ------------------------------------------------------------------------------------------------ tables (float64)
def window(win_length):
    """sqrt of the periodic Hann window, fp32 as AudioSignal.get_window("sqrt_hann") holds it (computed in float64, rounded once)."""
    k = torch.arange(win_length, dtype=torch.float64)
    return torch.sqrt(0.5 - 0.5 * torch.cos(k * (2 * math.pi / win_length))).float()


def forward_basis(win_length):
    """float64 [2 * padded_bins, n]: mel.dft_basis over all bins with the fp32 sqrt-Hann window's values folded in."""
    return MEL.dft_basis(win_length, 0, win_length // 2 + 1, window=window(win_length))


def inverse_table(win_length):
    """(real half, imaginary half), float64 [n, padded_bins] each: irfft as a product.  Sample s of a frame is
    real[s] . Re X + imag[s] . Im X with real[s, k] = c_k cos(2 pi k s / n) / n, imag[s, k] = -c_k sin(2 pi k s / n) / n,
    c_0 = c_{n/2} = 1 and 2 between; the imaginary entries of DC and Nyquist are zero (irfft ignores them), padded bins are zero.
    The phase is reduced exactly in integers."""
    n, nb = win_length, win_length // 2 + 1
    s = torch.arange(n, dtype=torch.int64)
    k = torch.arange(nb, dtype=torch.int64)
    ang = ((s[:, None] * k[None, :]) % n).double() * (2 * math.pi / n)
    c = torch.full((nb,), 2.0 / n, dtype=torch.float64)
    c[0] = c[-1] = 1.0 / n
    re = torch.zeros(n, padded_bins(n), dtype=torch.float64)
    im = torch.zeros_like(re)
    re[:, :nb] = c * torch.cos(ang)
    im[:, :nb] = -c * torch.sin(ang)
    im[:, 0] = 0.0
    im[:, nb - 1] = 0.0
    return re, im


def triangle(p):
    """The integer triangle 1 .. p + 1 .. 1 (2 p + 1 taps): (p + 1) times the reference's linspace construction."""
    return [p + 1 - abs(i) for i in range(-p, p + 1)]


def smoothing_taps(n_freq=3, n_time=5):
    """float64 [2 n_freq + 1, 2 n_time + 1]: spectral_gate.py:40-54's filter, the outer product of the two triangles over its sum
    (n_freq + 1)^2 (n_time + 1)^2 in integer units."""
    f = torch.tensor(triangle(n_freq), dtype=torch.float64)
    t = torch.tensor(triangle(n_time), dtype=torch.float64)
    return torch.outer(f, t) / float((n_freq + 1) ** 2 * (n_time + 1) ** 2)


def _device_tables(n, dev):
    """(forward basis planes, inverse planes of [n, real columns | imaginary columns], fp32 window) on `dev`, built once per
    (n, device)."""
    return CL.device_tables(("denoise", int(n), str(dev)), lambda: (
        MEL.packed3(forward_basis(n), dev), MEL.packed3(torch.cat(inverse_table(n), dim=1), dev), window(n).to(dev)))


# ------------------------------------------------------------------------------------------------ launches
def _refuse(what, lens, n, hop, n_freq=3, n_time=5):
    why = refusal(lens, n, hop, n_freq, n_time)
    if why:
        raise MmxError(f"{what}: {why}")


def _threshold(x, lens, n_std, n):
    """x fp32 [B, L] on the device (rows may be views into longer rows) -> fp32 [B, bins]."""
    B, L = x.shape
    basis, _, _ = _device_tables(n, x.device)
    d_lens, h_lens = CL.lens_args(lens, L, x.device)
    cap = -(-frames_of(L, n) // FRAMES_PER_TILE)
    work = torch.empty(B, cap, padded_bins(n), 2, dtype=torch.float64, device=x.device)
    out = torch.empty(B, n // 2 + 1, dtype=torch.float32, device=x.device)
    call("mmx_gate_threshold", _p(x), CL.row_stride(x), L, B, _p(d_lens), h_lens, _p(basis), n, float(n_std), _p(work), cap, _p(out),
         out.shape[1], stream())
    return out


@torch.no_grad()
def gate_threshold(noise, lens=None, n_std=3.0, win_length=2048, hop_length=512):
    """The gate's per-bin threshold in dB of noise clips (a list of mono clips, one clip [n], or a padded batch [B, L] with `lens`):
    mean + n_std * unbiased std over each clip's own frames of 20 log10 max(|STFT|, 1e-4) -> fp32 [B, win_length // 2 + 1] on the
    device.  Sums and finish are fp64 in a fixed order: a clip's row is that of its solo run, bit for bit."""
    CL.on_device("gate_threshold", noise)
    x, lens = CL.pack(noise, lens, "gate_threshold")
    _refuse("gate_threshold", lens, win_length, hop_length)
    return _threshold(x, lens, n_std, int(win_length))


def _is_span(noise):
    return isinstance(noise, tuple) and len(noise) == 2 and all(isinstance(v, int) for v in noise)


@torch.no_grad()
def spectral_gate(clips, noise, lens=None, denoise_amount=1.0, n_std=3.0, win_length=2048, hop_length=512, n_freq=3, n_time=5,
                  return_mask=False):
    """SpectralGate.forward for a ragged batch.  clips: a list of mono clips ([n] / [1, n]) or a padded batch [B, L] / [B, 1, L] with
    `lens`.  noise, where the statistics come from: one clip (shared by all), a list with one clip per member, or a tuple
    (start, stop) in samples meaning that span OF EACH CLIP ITSELF - the room tone before the speaker starts.  (A clip's own whole
    length is no sensible default: mean + 3 std of its own dB masks nearly every bin and returns silence.)  denoise_amount: a float
    or one per clip.  Returns the gated clips: a list of [n] views for a list, a tensor of the input's shape (zero past `lens`) for a
    tensor; with return_mask also the list of the binary masks, bool [bins, frames] per clip (True: gated).  MmxError where refusal()
    gives a reason: nothing is launched then.  Nothing is read back; a clip's result is that of its solo run, bit for bit."""
    CL.on_device("spectral_gate", clips, noise)
    x, lens = CL.pack(clips, lens, "spectral_gate")
    B, L = x.shape
    n, dev = int(win_length), x.device
    _refuse("spectral_gate", lens, n, hop_length, n_freq, n_time)
    if _is_span(noise):
        a, b = noise
        if not 0 <= a < b <= min(lens):
            raise MmxError(f"spectral_gate: the noise span ({a}, {b}) does not lie inside a clip of {min(lens)} samples")
        _refuse("spectral_gate (noise span)", [b - a], n, hop_length)
        thresh = _threshold(x[:, a:b], None, n_std, n)
    else:
        nz, nlens = CL.pack(noise, None, "spectral_gate (noise)")
        if nz.shape[0] != (1 if isinstance(noise, torch.Tensor) else B):
            raise ValueError(f"spectral_gate: noise is one clip, one per clip ({B}) or a (start, stop) span, got {nz.shape[0]} clips")
        _refuse("spectral_gate (noise)", nlens, n, hop_length)
        thresh = _threshold(nz, nlens, n_std, n)
    amt = torch.tensor(CL.per_clip(denoise_amount, B, "spectral_gate: denoise_amount"), dtype=torch.float32, device=dev)

    basis, inv, win = _device_tables(n, dev)
    d_lens, h_lens = CL.lens_args(lens, L, dev)
    nbp, fcap = padded_bins(n), frames_of(L, n)
    spec = torch.empty(B, fcap, 2 * nbp, dtype=torch.float32, device=dev)
    mask = torch.empty(B, fcap, nbp, dtype=torch.uint8, device=dev)
    frames = torch.empty(B, fcap, n, dtype=torch.float32, device=dev)
    out = torch.empty(B, L, dtype=torch.float32, device=dev)
    call("mmx_gate_analyze", _p(x), CL.row_stride(x), L, B, _p(d_lens), h_lens, _p(basis), n, _p(thresh),
         thresh.shape[1] if thresh.shape[0] > 1 else 0, _p(spec), _p(mask), fcap, stream())
    call("mmx_gate_synthesize", _p(spec), _p(mask), fcap, L, B, _p(d_lens), h_lens, _p(inv), _p(win), n, int(n_freq), int(n_time),
         _p(amt), _p(frames), _p(out), L, stream())
    res = CL.unpack(out, lens, clips)
    if not return_mask:
        return res
    return res, [mask[b, :frames_of(v, n), :n // 2 + 1].t().bool() for b, v in enumerate(lens)]


class SpectralGate(torch.nn.Module):
    """The reference's module (spectral_gate.py) with tensors in place of AudioSignal: forward(audio, noise, ...) -> the gated audio
    of the same shape ([n], [B, L] or [B, 1, L]) or the list of gated clips; `noise` as spectral_gate takes it."""

    def __init__(self, n_freq: int = 3, n_time: int = 5):
        super().__init__()
        self.n_freq, self.n_time = int(n_freq), int(n_time)
        self.register_buffer("smoothing_filter", smoothing_taps(n_freq, n_time).float()[None, None])

    def forward(self, audio, noise, denoise_amount=1.0, n_std=3.0, win_length=2048, hop_length=512, lens=None):
        return spectral_gate(audio, noise, lens=lens, denoise_amount=denoise_amount, n_std=n_std, win_length=win_length,
                             hop_length=hop_length, n_freq=self.n_freq, n_time=self.n_time)
