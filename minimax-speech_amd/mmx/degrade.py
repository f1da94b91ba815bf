"""Room and noise simulation on the device: the reference's EffectMixin.convolve, apply_ir, alter_drr, measure_drr and mix
(dac-vae/audiotools/core/effects.py:27-179, 540-647), which its RoomImpulseResponse, BackgroundNoise and CrossTalk transforms wrap
(data/transforms.py:707-900), over a ragged batch of mono clips in the launches of csrc/degrade.hip (mmx_ir_prepare, mmx_fir_rows,
mmx_row_absmax, mmx_mix_rows), without a host sync.  The long FIR is a framed product at hop 16 on the spectral tile's arithmetic
(csrc/spec_tile.h); there is no FFT.

Definitions (effects.py restated; audiotools is not a dependency, DESIGN.md §2, restated seams).  For a clip x of N samples and an
impulse response h of L samples, cut to L' = min(L, N) taps (effects.py:85-90):
    p    = the first index of max |h[0 .. L')| if start_at_max else 0
    s    = 1 / max(max |h[0 .. L')|, 1e-5)                   (effects.py:113-119: the delta's response peaks at the IR's own peak)
    y[n] = s * sum_{t < L'} h[t] X(n + p - t),   0 <= n < N
    X(i) = x[i mod N]                       wrap=True  (the reference: a circular product of length N, effects.py:105-111)
         = x[i] if 0 <= i < N else 0        wrap=False (a room: nothing arrives before the clip starts)
apply_ir (effects.py:160-177): y * max(max |x|, 1e-8) / max(max |y|, 1e-8), after alter_drr where `drr` is given.
alter_drr (effects.py:540-574, 591-647), on the WHOLE IR: td = argmax h (signed), t0 = int(rate * 0.0025), the early response is h on
[td - t0, td + t0] within [0, L), the late field the rest, w the periodic Hann window (scipy.signal.get_window("hann", count)) over
the early indices; alpha is the larger root of a alpha^2 + b alpha + c = 0 with a = sum w^2 e^2, b = sum 2 (1 - w) w e^2,
c = sum (1 - w)^2 e^2 - 10^(drr / 10) sum l^2, floored at max |l| / max |e|; h' = alpha w e + (1 - w) e + l, divided by its peak where
that is above 1 (ensure_max_of_audio).  The sums are fp64 here (the reference takes them in fp32).  A negative discriminant gives NaN
taps, as the reference's sqrt does: nothing is read back to check for it.  Where the floor engages, the target is NOT reached; that,
too, is the reference's behaviour.  measure_drr (effects.py:576-589): 10 log10(sum e^2 / sum l^2).
mix (effects.py:52-63, 200-220): the noise zero padded or cut to its clip's length FIRST, then
    out = x + exp(((Lx - snr) - Ln) ln 10 / 20) * noise,    Lx, Ln = mmx.loudness.integrated_loudness (partial="pad"), each clip alone.

`ir_eq` (apply_ir; effects.py:155-156) and `noise_eq` (mix; the reference's `other_eq`, effects.py:57-58) are mel-band equalizer
curves for the impulse response and for the fitted noise: mmx.channel.equalizer, before alter_drr and before the metering.

Deliberately left out: `use_original_phase`, multi-channel clips, and looping a short noise clip (it is zero padded, as
EffectMixin.mix itself does; the looping is the reference's file loader's).

The one host table is the set of Hann windows (float64).  There is no CPU fallback: a CPU tensor raises MmxError before any device
work."""
import math

import numpy as np
import torch

from . import clips as CL
from . import ops
from ._lib import MmxError, call, stream, _p

LDS_BYTES = 160 * 1024
WAVES, ROW_TILES = 4, 4                                  # csrc/degrade.hip: FIR_WAVES, FIR_RT (a row tile: 16 frames x 16 columns)
NOUT = WAVES * ROW_TILES * 256                           # FIR_NOUT: consecutive outputs of one clip a workgroup owns
CHUNK_TAPS = 4096                                        # FIR_CHUNK: K columns (taps) staged in LDS at a time
MAX_TAPS = 65536                                         # FIR_MAX_TAPS: one second at 48 kHz is 48000; the table is 96 bytes per tap
GAIN_FACTOR = math.log(10.0) / 20.0                      # effects.py:12


def padded_taps(taps):
    """K of the product: taps + 15 columns (output column j of a frame starts j samples later), rounded up to the MFMA's 32."""
    return ops.round_up(int(taps) + 15, 32)


def lds_bytes(taps):
    """Dynamic LDS of fir_rows_kernel (fir_lds of csrc/degrade.hip): the sample span under the workgroup's NOUT / 16 frames at hop 16
    for ONE K chunk - NOUT - 16 + min(CHUNK_TAPS, padded taps) samples - as three bf16 planes.  The chunks pass through the same
    planes in turn; the accumulators stay in registers."""
    return 3 * 2 * (NOUT - 16 + min(CHUNK_TAPS, padded_taps(taps)))


def refusal(lens, ir_lens):
    """Why convolve refuses clips of these lengths with impulse responses of these (one, or one per clip), or None.  Nothing is
    launched then."""
    lens, ir_lens = [int(v) for v in lens], [int(v) for v in ir_lens]
    if not lens or len(ir_lens) not in (1, len(lens)):
        return f"{len(ir_lens)} impulse responses for {len(lens)} clips (one, or one per clip)"
    if min(lens) < 1:
        return "an empty clip"
    if min(ir_lens) < 1:
        return "an empty impulse response"
    ir_lens = ir_lens * len(lens) if len(ir_lens) == 1 else ir_lens
    most = max(min(a, b) for a, b in zip(lens, ir_lens))
    if most > MAX_TAPS:
        return f"{most} taps are above {MAX_TAPS}, the longest impulse response the kernel is built and tested for"
    if lds_bytes(most) > LDS_BYTES:
        return f"{most} taps need {lds_bytes(most)} bytes of LDS"
    return None


# ------------------------------------------------------------------------------------------------ host side (float64)
def hann_windows(t0):
    """float64 [2 t0 + 1, 2 t0 + 1]: row c - 1 holds scipy.signal.get_window("hann", c) (periodic: 0.5 - 0.5 cos(2 pi i / c)) in its
    first c columns.  The early window of alter_drr has between 1 and 2 t0 + 1 points, depending on where the IR peaks."""
    W = 2 * int(t0) + 1
    c = np.arange(1, W + 1, dtype=np.float64)[:, None]
    i = np.arange(W, dtype=np.float64)[None, :]
    return np.where(i < c, 0.5 - 0.5 * np.cos(2.0 * math.pi * i / c), 0.0)


def early_bounds(h, rate):
    """(lo, hi) of the early response of IR h (float array): [td - t0, td + t0] within the IR, td the signed argmax."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    td, t0 = int(np.argmax(h)), int(rate * 0.0025)
    return max(td - t0, 0), min(td + t0, h.size - 1)


def measure_drr_host(h, rate):
    """measure_drr in float64 on the host: 10 log10(sum early^2 / sum late^2)."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    lo, hi = early_bounds(h, rate)
    e2 = float(np.sum(h[lo:hi + 1] ** 2))
    return 10.0 * math.log10(e2 / (float(np.sum(h ** 2)) - e2)) if h.size > hi - lo + 1 else math.inf


def alter_drr_host(h, rate, drr):
    """alter_drr in float64 on the host (the arithmetic of ir_prepare_kernel up to summation order) -> float64 [L]."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    lo, hi = early_bounds(h, rate)
    w = np.zeros_like(h)
    w[lo:hi + 1] = hann_windows(int(rate * 0.0025))[hi - lo, :hi - lo + 1]
    early = np.zeros_like(h)
    early[lo:hi + 1] = h[lo:hi + 1]
    late = h - early
    a = np.sum(w ** 2 * early ** 2)
    b = np.sum(2.0 * (1.0 - w) * w * early ** 2)
    c = np.sum((1.0 - w) ** 2 * early ** 2) - 10.0 ** (float(drr) / 10.0) * np.sum(late ** 2)
    disc = b * b - 4.0 * a * c
    if not disc >= 0.0:
        return np.full_like(h, np.nan)
    e = math.sqrt(disc)
    alpha = max((-b - e) / (2.0 * a), (-b + e) / (2.0 * a), np.abs(late).max() / np.abs(early).max())
    out = alpha * w * early + (1.0 - w) * early + late
    peak = np.abs(out).max()
    return out / peak if peak > 1.0 else out


def prepare_host(h, n, start_at_max=True):
    """(L', p, s) of IR h applied to a clip of n samples."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    taps = min(h.size, int(n))
    a = np.abs(h[:taps])
    return taps, (int(np.argmax(a)) if start_at_max else 0), 1.0 / max(float(a.max()), 1e-5)


def convolve_host(x, h, start_at_max=True, wrap=True):
    """The index definition at the top in float64 on the host, literally -> float64 [N].  O(N L'): for tests and small checks."""
    x, h = np.asarray(x, dtype=np.float64).reshape(-1), np.asarray(h, dtype=np.float64).reshape(-1)
    N = x.size
    taps, p, s = prepare_host(h, N, start_at_max)
    y = np.zeros(N)
    n = np.arange(N)
    for t in range(taps):
        i = n + p - t
        if wrap:
            y += h[t] * x[i % N]
        else:
            ok = (i >= 0) & (i < N)
            y[ok] += h[t] * x[i[ok]]
    return y * s


def toeplitz(h, taps):
    """float64 [16, padded taps]: row j, column u = g[u - j] with g[v] = h[taps - 1 - v], zero outside [0, taps): the B operand
    (one 16-column tile, stored column-major as the packer takes weights [N = 16, K])."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    kp = padded_taps(taps)
    v = np.arange(kp)[None, :] - np.arange(16)[:, None]
    ok = (v >= 0) & (v < taps)
    return np.where(ok, h[np.clip(taps - 1 - v, 0, h.size - 1)], 0.0)


def pack_table(h, taps, kcap=None):
    """The table ir_table_kernel writes for one IR, built on the host: bf16 [3, kcap // 32, 64, 8], the three bf16 terms of
    toeplitz(h, taps) in mmx_pack_skinny order (lane = 16 g + j holds columns 32 kt + 8 g .. + 7 of row j); columns from the padded
    taps to kcap are zero."""
    from .mel import planes3
    kp = padded_taps(taps)
    kcap = kp if kcap is None else int(kcap)
    assert kcap % 32 == 0 and kcap >= kp
    full = np.zeros((16, kcap))
    full[:, :kp] = toeplitz(np.asarray(h, dtype=np.float32), taps)
    out = []
    for pl in planes3(torch.from_numpy(full)):           # [16, kcap] -> [kt][g][j][e] -> lane = 16 g + j
        out.append(pl.reshape(16, kcap // 32, 4, 8).permute(1, 2, 0, 3).reshape(kcap // 32, 64, 8))
    return torch.stack(out)


def unpack_table(table):
    """pack_table's inverse: bf16 [3, K // 32, 64, 8] (or flat) -> float64 [16, K], the sum of the three planes."""
    t = table.reshape(3, -1, 4, 16, 8).double().sum(0)   # [kt][g][j][e]
    return t.permute(2, 0, 1, 3).reshape(16, -1).numpy()


# ------------------------------------------------------------------------------------------------ launches
def _hann(t0, dev):
    return CL.device_tables(("degrade", int(t0), str(dev)), lambda: torch.from_numpy(hann_windows(t0)).to(dev))


def _prepare(irs, ir_lens, sig_lens, rate, drr, start_at_max, what):
    """irs: one IR [n], a list (one, or one per clip) or a padded batch [B, Lir] with ir_lens; sig_lens: the clips' lengths ->
    dict(ir fp32 [B, Lir], p, s, taps, drr, table, kcap), everything on the device."""
    B = len(sig_lens)
    h, hl = CL.pack(irs, ir_lens, f"{what} (impulse response)")
    why = refusal(sig_lens, hl)
    if why:
        raise MmxError(f"{what}: {why}")
    shared = h.shape[0] == 1 and B > 1
    hl = hl * B if shared else hl
    dev, Lir, Lsig = h.device, h.shape[1], max(sig_lens)
    kcap = padded_taps(max(min(a, b) for a, b in zip(sig_lens, hl)))
    t0 = int(rate * 0.0025) if rate is not None else 0
    d_drr = None
    if drr is not None:
        vals = CL.per_clip(drr, B, f"{what}: drr", none=float("nan"))
        if any(v == v for v in vals):
            d_drr = torch.tensor(vals, dtype=torch.float32, device=dev)
    d_il, h_il = CL.lens_args(hl, Lir, dev)
    d_sl, h_sl = CL.lens_args(sig_lens, Lsig, dev)
    r = dict(ir=torch.empty(B, Lir, dtype=torch.float32, device=dev), p=torch.empty(B, dtype=torch.int32, device=dev),
             s=torch.empty(B, dtype=torch.float32, device=dev), taps=torch.empty(B, dtype=torch.int32, device=dev),
             drr=torch.empty(B, dtype=torch.float32, device=dev), table=torch.empty(B, 3, kcap * 16, dtype=torch.bfloat16, device=dev),
             kcap=kcap, ir_lens=hl)
    call("mmx_ir_prepare", _p(h), 0 if shared else CL.row_stride(h), Lir, B, _p(d_il), h_il, Lsig, _p(d_sl), h_sl, _p(d_drr), t0,
         _p(_hann(t0, dev)), int(bool(start_at_max)), _p(r["ir"]), Lir, _p(r["p"]), _p(r["s"]), _p(r["taps"]), _p(r["drr"]),
         _p(r["table"]), kcap, stream())
    return r


def _fir(x, lens, prep, wrap):
    """x fp32 [B, L] -> (out fp32 [B, L], zero past lens; peak fp32 [B] = max |out|)."""
    B, L = x.shape
    d_lens, h_lens = CL.lens_args(lens, L, x.device)
    out = torch.empty(B, L, dtype=torch.float32, device=x.device)
    peak = torch.empty(B, dtype=torch.float32, device=x.device)
    call("mmx_fir_rows", _p(x), CL.row_stride(x), L, B, _p(d_lens), h_lens, _p(prep["table"]), prep["kcap"], _p(prep["p"]), _p(prep["s"]),
         _p(prep["taps"]), int(bool(wrap)), _p(out), L, _p(peak), stream())
    return out, peak


def row_absmax(x, lens=None):
    """max |x[b, :lens[b]]| of fp32 rows [B, L] on the device -> fp32 [B] (mmx_row_absmax)."""
    CL.on_device("row_absmax", x)
    B, L = x.shape
    d_lens, _ = CL.lens_args(lens, L, x.device)
    peak = torch.empty(B, dtype=torch.float32, device=x.device)
    call("mmx_row_absmax", _p(x), CL.row_stride(x), L, B, _p(d_lens), _p(peak), stream())
    return peak


@torch.no_grad()
def convolve(clips, irs, lens=None, ir_lens=None, start_at_max=True, wrap=True):
    """EffectMixin.convolve for a ragged batch.  clips: a list of mono clips ([n] / [1, n]), one clip [n], or a padded batch [B, L] /
    [B, 1, L] with `lens`.  irs: one impulse response [n] for all clips, a list with one per clip, or a padded batch [B, Lir] with
    `ir_lens`.  wrap=True is the reference's circular product; wrap=False lets nothing arrive from before the clip's start.
    Returns the convolved clips: a list of [n] views for a list, a tensor of the input's shape (zero past `lens`) for a tensor.
    MmxError where refusal() gives a reason, or for a CPU tensor: nothing is launched then.  Nothing is read back; a clip's result
    is that of its solo call, bit for bit."""
    CL.on_device("convolve", clips, irs)
    x, lens = CL.pack(clips, lens, "convolve")
    prep = _prepare(irs, ir_lens, lens, None, None, start_at_max, "convolve")
    return CL.unpack(_fir(x, lens, prep, wrap)[0], lens, clips)


@torch.no_grad()
def apply_ir(clips, irs, rate, drr=None, start_at_max=True, wrap=True, lens=None, ir_lens=None, ir_eq=None):
    """EffectMixin.apply_ir for a ragged batch: alter_drr where `drr` (one value, or one per clip with None entries) names a target,
    convolve, then the rescale to the input's peak (effects.py:160-177, clamps of 1e-8).  ir_eq: an equalizer curve [n_bands] (or one
    per impulse response) applied to the impulse responses first (mmx.channel.equalizer; effects.py:155-156).  Arguments and result as
    convolve."""
    CL.on_device("apply_ir", clips, irs)
    x, lens = CL.pack(clips, lens, "apply_ir")
    if ir_eq is not None:
        from .channel import equalizer
        irs = equalizer(irs, ir_eq, rate, lens=ir_lens)
    prep = _prepare(irs, ir_lens, lens, rate, drr, start_at_max, "apply_ir")
    B, L = x.shape
    d_lens, _ = CL.lens_args(lens, L, x.device)
    before = row_absmax(x, lens)
    y, after = _fir(x, lens, prep, wrap)
    gain = before.clamp(min=1e-8) / after.clamp(min=1e-8)
    out = torch.zeros(B, L, dtype=torch.float32, device=x.device) if d_lens is not None else torch.empty_like(y)
    call("mmx_scale_rows", _p(y), L, L, B, _p(d_lens), _p(gain), 1, _p(out), L, stream())
    return CL.unpack(out, lens, clips)


@torch.no_grad()
def alter_drr(irs, rate, drr, ir_lens=None):
    """EffectMixin.alter_drr for a ragged batch of impulse responses (a list, one IR, or [B, Lir] with `ir_lens`): drr is one target
    in dB or one per IR (None entries copy the IR) -> the altered IRs, a list of [n] views or a tensor of the input's shape."""
    CL.on_device("alter_drr", irs)
    h, hl = CL.pack(irs, ir_lens, "alter_drr")
    prep = _prepare(h, hl, hl, rate, drr, True, "alter_drr")
    return CL.unpack(prep["ir"], hl, irs)


@torch.no_grad()
def measure_drr(irs, rate, ir_lens=None):
    """EffectMixin.measure_drr: the direct-to-reverberant ratio in dB of each impulse response -> fp32 [B] on the device.  (It and
    alter_drr go through mmx_ir_prepare whole, table included, so they refuse what convolve refuses: more than MAX_TAPS taps.)"""
    CL.on_device("measure_drr", irs)
    h, hl = CL.pack(irs, ir_lens, "measure_drr")
    return _prepare(h, hl, hl, rate, None, True, "measure_drr")["drr"]


@torch.no_grad()
def mix(clips, noises, rate, snr=10.0, lens=None, noise_lens=None, noise_eq=None):
    """EffectMixin.mix for a ragged batch: clips as convolve takes them; noises one clip [n] for all, a list with one per clip, or a
    padded batch with `noise_lens`.  Each noise is zero padded or cut to its clip's length, both are metered (BS.1770 integrated
    loudness, mmx.loudness with partial="pad", each clip alone) and the noise is added at `snr` dB (one value, or one per clip)
    below the clip.  noise_eq: an equalizer curve [n_bands] (or one per clip) applied to the fitted noise before it is metered
    (mmx.channel.equalizer; the reference's other_eq, effects.py:57-58).  `rate` must be one the meter supports.  Result as convolve."""
    from . import loudness as LOUD
    CL.on_device("mix", clips, noises)
    x, lens = CL.pack(clips, lens, "mix")
    B, L = x.shape
    nz, nl = CL.pack(noises, noise_lens, "mix (noise)")
    if min(lens + nl) < 1:
        raise MmxError("mix: an empty clip")
    if nz.shape[0] not in (1, B):
        raise ValueError(f"mix: one noise clip, or one per clip ({B}), got {nz.shape[0]}")
    snrs = torch.tensor(CL.per_clip(snr, B, "mix: snr"), dtype=torch.float32, device=x.device)
    fit = torch.zeros(B, L, dtype=torch.float32, device=x.device)                # effects.py:54-56: pad, then truncate
    for b in range(B):
        src = 0 if nz.shape[0] == 1 else b
        m = min(nl[src], lens[b])
        fit[b, :m] = nz[src, :m]
    if noise_eq is not None:
        from .channel import equalizer
        fit = equalizer(fit, noise_eq, rate, lens=lens)
    lx = LOUD._run(x, lens, rate, partial="pad")["lufs"]
    ln = LOUD._run(fit, lens, rate, partial="pad")["lufs"]
    return CL.unpack(mix_rows(x, fit, lx, ln, snrs, lens), lens, clips)


def mix_rows(x, noise, lx, ln, snr, lens=None, noise_lens=None):
    """mmx_mix_rows: x, noise fp32 [B, L] / [B, Ln], lx, ln, snr fp32 [B], all on the device -> fp32 [B, L], zero past lens."""
    CL.on_device("mix_rows", x, noise, lx, ln, snr)
    B, L = x.shape
    dev = x.device
    d_lens, _ = CL.lens_args(lens, L, dev)
    d_nl, _ = CL.lens_args(noise_lens, noise.shape[1], dev)
    out = torch.empty(B, L, dtype=torch.float32, device=dev)
    call("mmx_mix_rows", _p(x), CL.row_stride(x), L, B, _p(d_lens), _p(noise), CL.row_stride(noise), noise.shape[1], _p(d_nl), _p(lx),
         _p(ln), _p(snr), _p(out), L, stream())
    return out


class RoomImpulseResponse(torch.nn.Module):
    """The reference's transform (data/transforms.py RoomImpulseResponse) with tensors in place of AudioSignal and explicit parameters
    in place of sampled ones: forward(audio, ir, drr=None) -> apply_ir(audio, ir, rate, drr).  No file loading, no sampling."""

    def __init__(self, sample_rate: int, start_at_max: bool = True, wrap: bool = True):
        super().__init__()
        self.sample_rate, self.start_at_max, self.wrap = int(sample_rate), bool(start_at_max), bool(wrap)

    def forward(self, audio, ir, drr=None, lens=None, ir_lens=None, eq=None):
        return apply_ir(audio, ir, self.sample_rate, drr=drr, start_at_max=self.start_at_max, wrap=self.wrap, lens=lens, ir_lens=ir_lens,
                        ir_eq=eq)


class BackgroundNoise(torch.nn.Module):
    """The reference's transform (data/transforms.py BackgroundNoise; CrossTalk is the same mix with speech as the noise) with
    tensors and explicit parameters: forward(audio, noise, snr=10.0) -> mix(audio, noise, rate, snr)."""

    def __init__(self, sample_rate: int):
        super().__init__()
        self.sample_rate = int(sample_rate)

    def forward(self, audio, noise, snr=10.0, lens=None, noise_lens=None, eq=None):
        return mix(audio, noise, self.sample_rate, snr=snr, lens=lens, noise_lens=noise_lens, noise_eq=eq)
