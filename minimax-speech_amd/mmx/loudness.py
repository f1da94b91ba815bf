"""Integrated loudness and level matching on the device: what the reference's codec layer asks of
`audiotools.core.loudness.Meter` / `LoudnessMixin.loudness` (dac-vae/audiotools/core/loudness.py) and of `normalize` /
`ensure_max_of_audio` (core/effects.py:181-220; DACVAE.compress / decompress, dac-vae/base.py:166-180,285), as
mmx_kweight_blocks -> mmx_loudness_gate -> mmx_scale_rows (csrc/loudness.hip) over a ragged batch, without a host sync.

The definition is ITU-R BS.1770-4 as pyloudnorm and audiotools implement it, restated here (pyloudnorm, julius and torchaudio are
not dependencies; DESIGN.md §2, restated seams).

K-weighting for `rate`: two biquads in series, both with passband gain 1, coefficients in float64 as pyloudnorm's IIRfilter
computes them.  With A = 10^(G/40), w0 = 2 pi fc / rate, alpha = sin(w0) / (2 Q):
    high shelf (G = 4.0, Q = 1/sqrt 2, fc = 1500):
        b = [A((A+1) + (A-1) cos w0 + 2 sqrt A alpha), -2A((A-1) + (A+1) cos w0), A((A+1) + (A-1) cos w0 - 2 sqrt A alpha)]
        a = [(A+1) - (A-1) cos w0 + 2 sqrt A alpha,     2((A-1) - (A+1) cos w0),   (A+1) - (A-1) cos w0 - 2 sqrt A alpha]
    high pass (G = 0, Q = 0.5, fc = 38):
        b = [(1 + cos w0) / 2, -(1 + cos w0), (1 + cos w0) / 2],   a = [1 + alpha, -2 cos w0, 1 - alpha]
    both b and a divided by a[0].
Blocks: K = int(0.4 rate) samples every S = int(0.4 rate 0.25).  partial = "pad" (the default; audiotools through
julius.core.unfold): F = ceil((max(n, K) - K) / S) + 1 blocks, the tail zero padded; partial = "drop" (BS.1770, pyloudnorm):
F = (n - K) // S + 1.  z[c][j] = (sum of squares of block j of filtered channel c) / (0.4 rate), and
    l[j] = -0.691 + 10 log10 sum_c G[c] z[c][j],   G = [1, 1, 1, 1.41, 1.41].
Gating (Meter.integrated_loudness): the blocks with l > -70 give Gamma_r = -0.691 + 10 log10 sum_c G[c] mean z[c] - 10; the blocks
above both thresholds give LUFS = -0.691 + 10 log10 sum_c G[c] mean z[c].  No block kept: -70; the result is floored at -70
(MIN_LOUDNESS).  A clip shorter than 0.5 s is first zero padded by int((0.5 - n / rate) rate) samples (LoudnessMixin.loudness).
normalize(db): gain = exp((db - LUFS) ln 10 / 20); then ensure_max_of_audio(max_peak): where gain * peak > max_peak the gain is
max_peak / peak.
Supported rates are those with K == 4 S (16 000, 22 050, 24 000, 44 100 and 48 000 among them) whose S splits into at most 127
segments of at most 64 samples: a block is then the sum of four 100 ms sub-block energies.  Any other rate raises ValueError.

This module computes the coefficients and the state-transition tables in float64; the arithmetic is the kernels' (the filters
themselves, exactly, in fp64: not the reference's 512-tap FIR truncation, and not a sequential lfilter).  There is no CPU
fallback: a CPU tensor raises MmxError."""
import ctypes as C
import math

import numpy as np
import torch

from . import clips as CL
from ._lib import MmxError, call, stream, _p

MIN_LOUDNESS = -70.0
G_BS1770 = (1.0, 1.0, 1.0, 1.41, 1.41)
PARTIAL = {"pad": 0, "drop": 1}                         # include/mmx_hip.h MMX_LOUD_PAD / MMX_LOUD_DROP
MAX_CH = 5                                               # MMX_LOUD_MAX_CH
SEG_MAX, NSEG_MAX, STEPS = 64, 127, 7                    # csrc/loudness.hip KW_SEG_MAX, KW_NSEG_MAX, KW_STEPS


def k_weighting(rate):
    """((b, a) of the high shelf, (b, a) of the high pass): float64 arrays of 3, a[0] = 1."""
    rate = int(rate)
    if rate <= 0:
        raise ValueError(f"sample rate must be positive: {rate}")

    def shelf(G, Q, fc):
        A = 10.0 ** (G / 40.0)
        w0 = 2.0 * math.pi * (fc / rate)
        al = math.sin(w0) / (2.0 * Q)
        c, r = math.cos(w0), 2.0 * math.sqrt(A) * al
        b = [A * ((A + 1) + (A - 1) * c + r), -2 * A * ((A - 1) + (A + 1) * c), A * ((A + 1) + (A - 1) * c - r)]
        a = [(A + 1) - (A - 1) * c + r, 2 * ((A - 1) - (A + 1) * c), (A + 1) - (A - 1) * c - r]
        return np.array(b) / a[0], np.array(a) / a[0]

    def high_pass(Q, fc):
        w0 = 2.0 * math.pi * (fc / rate)
        al = math.sin(w0) / (2.0 * Q)
        c = math.cos(w0)
        b, a = [(1 + c) / 2, -(1 + c), (1 + c) / 2], [1 + al, -2 * c, 1 - al]
        return np.array(b) / a[0], np.array(a) / a[0]

    return shelf(4.0, 1.0 / math.sqrt(2.0), 1500.0), high_pass(0.5, 38.0)


def block_sizes(rate):
    """(K, S) = (int(0.4 rate), int(0.4 rate 0.25)), the reference Meter's arithmetic; ValueError unless K == 4 S."""
    rate = int(rate)
    K, S = int(0.4 * rate), int(0.4 * rate * 0.25)
    if rate <= 0 or S <= 0 or K != 4 * S:
        raise ValueError(f"loudness: sample rate {rate} is not supported (a 400 ms block of {K} samples is not four steps of {S})")
    return K, S


def padded_len(n, rate):
    """Samples of a clip of n after LoudnessMixin.loudness's rule: shorter than 0.5 s, int((0.5 - n / rate) * rate) zeros follow."""
    dur = n / rate
    return n + int((0.5 - dur) * rate) if dur < 0.5 else n


def n_blocks(n, rate, partial="pad"):
    """Blocks of a clip of n samples (before the 0.5 s rule; apply padded_len first where it holds)."""
    K, S = block_sizes(rate)
    return (n - K) // S + 1 if PARTIAL[partial] else -(-(max(n, K) - K) // S) + 1


def segment(rate):
    """Samples per lane: the smallest divisor of S that leaves at most 127 segments (ValueError when it would exceed 64)."""
    _, S = block_sizes(rate)
    for seg in range(1, SEG_MAX + 1):
        if S % seg == 0 and S // seg <= NSEG_MAX:
            return seg
    raise ValueError(f"loudness: sample rate {rate} is not supported (its {S}-sample step does not split into <= {NSEG_MAX} segments "
                     f"of <= {SEG_MAX} samples)")


def transition(rate):
    """A float64 [4, 4]: one sample of zero input moves the cascade's transposed-direct-form-II state s = (shelf s0, s1, high
    pass s0, s1) to A s.  (With input: y1 = b0 x + s0, s0 <- b1 x - a1 y1 + s1, s1 <- b2 x - a2 y1 per section, the high pass
    fed y1: scipy.signal.lfilter's zi / zf of the two sections.)"""
    (b1, a1), (b2, a2) = k_weighting(rate)
    return np.array([[-a1[1], 1.0, 0.0, 0.0],
                     [-a1[2], 0.0, 0.0, 0.0],
                     [b2[1] - a2[1] * b2[0], 0.0, -a2[1], 1.0],
                     [b2[2] - a2[2] * b2[0], 0.0, -a2[2], 0.0]])


def tables(rate):
    """What mmx_kweight_blocks takes as `tab` (float64 [10 + 16 * 8]) and `seg`: the 2 x 5 coefficients (b0, b1, b2, a1, a2;
    shelf first), A^(seg 2^k) for k = 0 .. 6 (the scan over a sub-block's lanes) and A^S (the carry across sub-blocks), row major."""
    _, S = block_sizes(rate)
    seg = segment(rate)
    (b1, a1), (b2, a2) = k_weighting(rate)
    A = transition(rate)
    P = np.linalg.matrix_power(A, seg)
    mats = []
    for _ in range(STEPS):
        mats.append(P)
        P = P @ P
    mats.append(np.linalg.matrix_power(A, S))
    tab = np.concatenate([b1, a1[1:], b2, a2[1:]] + [m.reshape(-1) for m in mats]).astype(np.float64)
    assert tab.shape == (10 + 16 * (STEPS + 1),)
    return tab, seg


def _cap(L, rate, S):
    return -(-max(int(L), rate // 2 + 1) // S)


def _device_tables(rate, dev):
    def build():
        tab, seg = tables(rate)
        return torch.from_numpy(tab).to(dev), seg
    return CL.device_tables(("loudness", int(rate), str(dev)), build)


def _run(wave, lens, rate, nch=1, partial="pad", G=None, db=None, max_peak=1.0, want_mask=False, scale=False):
    """The one place that launches.  wave fp32 [rows, L] on the device (unit stride along L; a clip is `nch` adjacent rows),
    lens a list of ints per row or None -> dict(lufs fp32 [clips], peak fp32 [rows], energy f64 [rows, cap], and, with db,
    gain fp32 [clips]; with want_mask, mask uint8 [clips, cap - 3]; with scale, out fp32 [rows, L], written within lens only)."""
    CL.on_device("loudness", wave)
    rate = int(rate)
    _, S = block_sizes(rate)
    tab, seg = _device_tables(rate, wave.device)
    rows, L = wave.shape
    if rows % nch or not 1 <= nch <= MAX_CH:
        raise ValueError(f"loudness: {rows} rows are not clips of {nch} channels (at most {MAX_CH})")
    if L < 1:
        raise ValueError("loudness: empty clips")
    clips, dev, code = rows // nch, wave.device, PARTIAL[partial]
    d_lens, _ = CL.lens_args(lens, L, dev)
    cap = _cap(L, rate, S)
    work = torch.empty(rows, cap, 5, dtype=torch.float64, device=dev)
    energy = torch.empty(rows, cap, dtype=torch.float64, device=dev)
    peak = torch.empty(rows, dtype=torch.float32, device=dev)
    lufs = torch.empty(clips, dtype=torch.float32, device=dev)
    gain = torch.empty(clips, dtype=torch.float32, device=dev) if db is not None else None
    mask = torch.zeros(clips, max(1, cap - 3), dtype=torch.uint8, device=dev) if want_mask else None
    bs = CL.row_stride(wave)
    call("mmx_kweight_blocks", _p(wave), bs, L, rows, _p(d_lens), rate, code, _p(tab), seg, _p(work), cap, _p(energy), cap, _p(peak),
         stream())
    Gh = None if G is None else (C.c_double * nch)(*[float(g) for g in G][:nch])
    call("mmx_loudness_gate", _p(energy), cap, cap, _p(peak), _p(d_lens), L, clips, nch, Gh, rate, code, _p(lufs), int(db is not None),
         0.0 if db is None else float(db), float(max_peak), _p(gain), _p(mask), mask.shape[1] if want_mask else 0, stream())
    out = None
    if scale:
        out = torch.empty(rows, L, dtype=torch.float32, device=dev)
        call("mmx_scale_rows", _p(wave), bs, L, rows, _p(d_lens), _p(gain), nch, _p(out), L, stream())
    return dict(lufs=lufs, peak=peak, energy=energy, gain=gain, mask=mask, out=out)


@torch.no_grad()
def integrated_loudness(waves, rate, lens=None, partial="pad"):
    """Integrated loudness (LUFS) of mono clips: a ragged list of [n] / [1, n] tensors, one clip [n], or a padded batch [B, L]
    with `lens` valid samples per row -> fp32 [B] on the device.  Every clip is metered alone: its value is that of its solo run,
    bit for bit."""
    CL.on_device("integrated_loudness", waves)
    w, lens = CL.pack(waves, lens, "integrated_loudness")
    return _run(w, lens, rate, partial=partial)["lufs"]


@torch.no_grad()
def normalize(waves, rate, db, max_peak=1.0, partial="pad"):
    """audiotools' normalize(db) followed by ensure_max_of_audio(max_peak) for a ragged list of mono clips ([n] / [1, n]) ->
    (the list of scaled clips [n], views of one buffer; the measured LUFS fp32 [B] of the inputs).  No host sync."""
    waves = list(waves)
    CL.on_device("normalize", waves)
    w, lens = CL.pack(waves, None, "normalize")
    r = _run(w, lens, rate, partial=partial, db=db, max_peak=max_peak, scale=True)
    return CL.unpack(r["out"], lens, waves), r["lufs"]


class Meter:
    """`audiotools.core.loudness.Meter(rate, ...)` on device memory, the reference constructor's keywords: K-weighting and 400 ms
    blocks only; `zeros` and `use_fir` are accepted and ignored (the exact filters run, not an FIR truncation).  partial: "pad"
    (audiotools' block rule) or "drop" (BS.1770 / pyloudnorm)."""

    def __init__(self, rate, filter_class="K-weighting", block_size=0.400, zeros=512, use_fir=False, partial="pad"):
        if filter_class != "K-weighting":
            raise NotImplementedError(f"filter_class {filter_class!r}: only K-weighting is built")
        if block_size != 0.400:
            raise NotImplementedError(f"block_size {block_size!r}: only 400 ms blocks are built")
        if partial not in PARTIAL:
            raise ValueError(f"partial {partial!r}: 'pad' or 'drop'")
        self.rate, self.filter_class, self.block_size, self.partial = int(rate), filter_class, block_size, partial
        self.zeros, self.use_fir = zeros, use_fir
        block_sizes(self.rate)
        segment(self.rate)
        self.G = list(G_BS1770)

    @torch.no_grad()
    def integrated_loudness(self, data, detail=False):
        """data [nb, nt, nch] (nch <= 5) or [nt] on the device -> LUFS fp32 [nb].  detail=True: the whole result of the launches
        (the kept-block mask among it) instead."""
        CL.on_device("Meter.integrated_loudness", data)
        if data.dim() == 1:
            data = data[None, :, None]
        if data.dim() != 3 or data.shape[2] > MAX_CH:
            raise ValueError(f"Meter.integrated_loudness takes [nb, nt, nch <= {MAX_CH}] or [nt], got {tuple(data.shape)}")
        nb, nt, nch = data.shape
        rows = data.to(torch.float32).transpose(1, 2).contiguous().reshape(nb * nch, nt)
        r = _run(rows, None, self.rate, nch=nch, partial=self.partial, G=self.G, want_mask=detail)
        return r if detail else r["lufs"]
