"""Channel degradations on the device: the reference's low_pass / high_pass (dac-vae/audiotools/core/dsp.py:153-215), mel_filterbank,
equalizer, clip_distortion, quantization and mulaw_quantization (core/effects.py:386-523), which its LowPass, HighPass, Equalizer,
ClippingDistortion, Quantization and MuLawQuantization transforms wrap (data/transforms.py:531-666, 1095-1170), over a ragged batch
of mono clips, without a host sync.  The filters run on the long FIR of csrc/degrade.hip (mmx_ir_prepare, mmx_fir_rows) behind the
replicate padding of csrc/channel.hip (mmx_pad_edge_rows); the quantile is an exact radix select (mmx_row_select, mmx_clip_rows);
the quantizers are fp64 per sample (mmx_quantize_rows).

Definitions.  The filters are julius' (LowPassFilters, HighPassFilters, SplitBands), RESTATED, NOT COMPARED AGAINST julius, which is
not a dependency (restated seams; tests/test_channel_host.py pins the restatement by its invariants).  `rate` in Hz;
the design arithmetic is float64 on the host, rounded once to fp32.
  low-pass bank, cutoffs f_k, c_k = f_k / rate in (0, 0.5]:  half = int(zeros / min_k c_k / 2), T = 2 half + 1 taps, t = -half .. half,
      win[i] = 0.5 - 0.5 cos(2 pi i / (2 half))  (the symmetric Hann window, end points 0),
      lp_k[t] = 2 c_k win sinc(2 pi c_k t), sinc(0) = 1, divided by its own sum;
      y[n] = sum_t lp[t] x[clamp(n + t, 0, N - 1)]: replicate padding, N samples out.   zeros = 51 (dsp.py:153, 185).
  high-pass: x - lowpass(x), taps delta[t == 0] - lp[t].
  band split, n_bands >= 2: mel(f) = 2595 log10(1 + f / 700); the cutoffs are the n_bands - 1 interior points of n_bands + 1 points
      evenly spaced in mel over [0, rate / 2]; zeros = 8, one half for the bank; band_0 = lp_0, band_k = lp_k - lp_{k-1},
      band_{n-1} = x - lp_{n-2}.
  equalizer (effects.py:405-433): sum_k 10**db_k * band_k.  The exponent is db, NOT db / 20: that is the reference's arithmetic
      (`weights = 10**db`) and it is kept.  Here the whole equalizer is ONE filter per clip, h = sum_k 10**db_k * taps of band_k,
      summed in float64 and rounded once (the reference filters n_bands times in fp32 and sums the bands).
  clip_distortion (effects.py:435-461), percentile q in [0, 1]: clamp to [Q(q / 2), Q(1 - q / 2)], Q torch.quantile's linear
      interpolation over the clip's own N samples: pos = r (N - 1), lo = floor(pos), hi = ceil(pos), w = pos - lo, and
      v[lo] + (v[hi] - v[lo]) w over the ascending order statistics v.  Deviation: pos and w are float64 on the host and the lerp is
      fp64 on the device, rounded once; torch takes pos in fp32, which at N = 1 440 000 is already off by 1.5e-3 of a rank.  A row
      that holds a NaN gets NaN thresholds and an all-NaN result (torch.quantile propagates the NaN too); -0 and +0 compare equal.
  quantization(Q) (effects.py:463-490): 2 floor((x + 1) / 2 Q) / Q - 1.
  mulaw_quantization(Q) (effects.py:492-523), mu = Q - 1: c = trunc((sign(x) log1p(mu |x|) / log1p(mu) + 1) / 2 mu + 0.5),
      z = c / mu * 2 - 1, out = sign(z) (exp(|z| log1p(mu)) - 1) / mu.
      Both in fp64 per sample, rounded once: in fp32 (the reference's arithmetic) codes flip - between 1 and 19 per clip at Q = 65536
      on the test clips.  The reference returns x - (x - quantized) in fp32 (a straight-through estimator); the value is stated here.

The filter on the device: the clip goes into a row of N + 2 half samples with its ends repeated, the row through mmx_ir_prepare
(start_at_max = 0) and mmx_fir_rows (wrap = 0) with the taps reversed, and output n is sample n + 2 half of that product times
max(max |h|, 1e-5), which undoes prepare's scale (mmx_scale_rows on the shifted rows).  Clips whose parameters give different `half`
run as separate launch sequences.  Host tables: the tap sets (float64, cached per setting).  There is no CPU fallback: a CPU tensor
raises MmxError before any device work.  Nothing is read back; a clip's result is that of its solo call, bit for bit."""
import ctypes as C
import math

import numpy as np
import torch

from . import clips as CL
from . import degrade as D
from ._lib import MmxError, call, stream, _p

ZEROS = 51                                               # dsp.py:153, 185
BAND_ZEROS = 8                                           # julius.SplitBands
SELECT_SPAN = 8192                                       # csrc/channel.hip SEL_SPAN: samples of one row a workgroup of the select counts
SELECT_RANKS = 4                                         # SEL_RANKS: order statistics per row and call
SELECT_WORK = 4 * 256 + 8                                # SEL_WORK: int32 of scratch per row and rank


# ------------------------------------------------------------------------------------------------ host side (float64)
def half_size(cutoffs, rate, zeros=ZEROS):
    """half of a low-pass bank: int(zeros / min_k (f_k / rate) / 2)."""
    return int(zeros / min(float(f) / rate for f in np.atleast_1d(cutoffs)) / 2)


def lowpass_taps(cutoffs, rate, zeros=ZEROS):
    """float64 [T] for one cutoff in Hz, [K, T] for K of them (one half for the bank): index i holds lp[t = i - half]."""
    fs = np.atleast_1d(np.asarray(cutoffs, dtype=np.float64))
    half = half_size(fs, rate, zeros)
    t = np.arange(-half, half + 1, dtype=np.float64)
    i = np.arange(2 * half + 1, dtype=np.float64)
    win = 0.5 - 0.5 * np.cos(2.0 * math.pi * i / (2 * half)) if half > 0 else np.ones(1)
    out = []
    for f in fs:
        c = float(f) / rate
        a = 2.0 * math.pi * c * t
        lp = 2.0 * c * win * np.where(t == 0, 1.0, np.sin(a) / np.where(t == 0, 1.0, a))
        out.append(lp / lp.sum())
    return out[0] if np.ndim(cutoffs) == 0 else np.stack(out)


def highpass_taps(cutoffs, rate, zeros=ZEROS):
    """delta[t == 0] - lowpass_taps, same shapes."""
    lp = lowpass_taps(cutoffs, rate, zeros)
    hp = -lp
    hp[..., lp.shape[-1] // 2] += 1.0
    return hp


def band_cutoffs(rate, n_bands):
    """float64 [n_bands - 1]: the interior points in Hz of n_bands + 1 points evenly spaced in mel over [0, rate / 2]."""
    top = 2595.0 * math.log10(1.0 + (rate / 2.0) / 700.0)
    mels = np.linspace(0.0, top, int(n_bands) + 1)
    return (700.0 * (10.0 ** (mels / 2595.0) - 1.0))[1:-1]


_banks = {}


def band_taps(rate, n_bands, zeros=BAND_ZEROS):
    """float64 [n_bands, T]: the taps of julius.SplitBands(rate, n_bands) - lp_0, lp_k - lp_{k-1}, delta - lp_{n-2}.  Cached."""
    key = (float(rate), int(n_bands), int(zeros))
    if key not in _banks:
        lp = lowpass_taps(band_cutoffs(rate, n_bands), rate, zeros)
        delta = np.zeros(lp.shape[1])
        delta[lp.shape[1] // 2] = 1.0
        bank = np.concatenate([lp[:1], lp[1:] - lp[:-1], (delta - lp[-1])[None]])
        bank.setflags(write=False)
        _banks[key] = bank
    return _banks[key]


def equalizer_taps(rate, db, zeros=BAND_ZEROS):
    """float64 [T] for one curve db [n_bands], [B, T] for curves [B, n_bands]: sum_k 10**db_k * band_taps[k] (the exponent is db)."""
    db = np.asarray(db, dtype=np.float64)
    bank, w = band_taps(rate, db.shape[-1], zeros), 10.0 ** db
    h = np.zeros(db.shape[:-1] + bank.shape[1:])
    for k in range(bank.shape[0]):                       # bands ascending, each curve alone: a curve's taps do not depend on its companions
        h += w[..., k, None] * bank[k]
    return h


def quantile_ranks(n, r):
    """(lo, hi, w) of torch.quantile's linear interpolation at fraction r over n samples, float64."""
    pos = float(r) * (int(n) - 1)
    lo = math.floor(pos)
    return int(lo), int(math.ceil(pos)), pos - lo


def clip_ranks(n, q):
    """([lo, hi, lo', hi'], [w, w']) of the two quantiles q / 2 and 1 - q / 2 of clip_distortion."""
    a, b = quantile_ranks(n, float(q) / 2.0), quantile_ranks(n, 1.0 - float(q) / 2.0)
    return [a[0], a[1], b[0], b[1]], [a[2], b[2]]


def quantization_host(x, Q):
    """The uniform quantizer in float64 on the host -> float64."""
    x = np.asarray(x, dtype=np.float64)
    return 2.0 * (np.floor((x + 1.0) / 2.0 * Q) / Q) - 1.0


def mulaw_host(x, Q, codes=False):
    """The mu-law quantizer in float64 on the host -> float64 (codes=True: the value before truncation as well)."""
    x = np.asarray(x, dtype=np.float64)
    mu = float(Q) - 1.0
    pre = (np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu) + 1.0) / 2.0 * mu + 0.5
    z = np.trunc(pre) / mu * 2.0 - 1.0
    out = np.sign(z) * (np.exp(np.abs(z) * np.log1p(mu)) - 1.0) / mu
    return (out, pre) if codes else out


def refusal(lens, rate=None, cutoffs=None, zeros=None, n_bands=None, q=None, channels=None):
    """Why a call on clips of these lengths refuses, or None: an empty clip; a cutoff (Hz; a band filter) outside (0, rate / 2];
    n_bands < 2 (the equalizer and the band split); more than degrade.MAX_TAPS taps; a percentile q outside [0, 1]; fewer than 2
    quantization channels.  zeros: None is 51 for a band filter, 8 for the band split.  Nothing is launched then."""
    lens = [int(v) for v in lens]
    if not lens or min(lens) < 1:
        return "an empty clip"
    if cutoffs is not None:
        fs = [float(f) for f in np.atleast_1d(cutoffs)]
        if not all(0.0 < f <= rate / 2.0 for f in fs):
            return f"a cutoff outside (0, {rate / 2.0}] Hz"
        taps = 2 * half_size(fs, rate, ZEROS if zeros is None else zeros) + 1
        if taps > D.MAX_TAPS:
            return f"{taps} taps are above {D.MAX_TAPS}, the longest filter the FIR is built and tested for"
    if n_bands is not None:
        if int(n_bands) < 2:
            return f"{int(n_bands)} bands (at least 2)"
        taps = 2 * half_size(band_cutoffs(rate, n_bands), rate, BAND_ZEROS if zeros is None else zeros) + 1
        if taps > D.MAX_TAPS:
            return f"{taps} taps are above {D.MAX_TAPS}, the longest filter the FIR is built and tested for"
    if q is not None and not all(0.0 <= float(v) <= 1.0 for v in np.atleast_1d(q)):
        return "a clip percentile outside [0, 1]"
    if channels is not None and not all(float(v) >= 2 and float(v) == int(v) and float(v) < 2 ** 31 for v in np.atleast_1d(channels)):
        return "fewer than 2 quantization channels (a whole number, at least 2)"
    return None


def _refuse(what, why):
    if why:
        raise MmxError(f"{what}: {why}")


# ------------------------------------------------------------------------------------------------ launches
def _host_i32(vals):
    return (C.c_int32 * len(vals))(*vals)


def pad_edge(x, lens, half):
    """mmx_pad_edge_rows: x fp32 [B, L] -> (fp32 [B, L + 2 half], the padded rows' lengths)."""
    B, L = x.shape
    d_lens, h_lens = CL.lens_args(lens, L, x.device)
    out = torch.empty(B, L + 2 * half, dtype=torch.float32, device=x.device)
    call("mmx_pad_edge_rows", _p(x), CL.row_stride(x), L, B, _p(d_lens), h_lens, int(half), _p(out), L + 2 * half, stream())
    return out, [v + 2 * half for v in lens]


def _fir_padded(xp, plens, lens, L, taps, what):
    """xp: the padded rows of pad_edge; taps float64 [T] (one filter for all rows) or [B, T] -> fp32 [B, L], zero past lens."""
    B = xp.shape[0]
    taps = np.asarray(taps, dtype=np.float64)
    half = (taps.shape[-1] - 1) // 2
    h = np.ascontiguousarray(taps[..., ::-1]).astype(np.float32)        # y[n] = sum_t f[t] x[n + t]: the FIR's taps are f reversed
    peak = np.maximum(np.abs(h.reshape(-1, h.shape[-1])).max(axis=1), np.float32(1e-5)).astype(np.float32)
    gain = torch.from_numpy(np.broadcast_to(peak, (B,)).copy() if peak.size == 1 else peak).to(xp.device)
    prep = D._prepare(torch.from_numpy(h).to(xp.device), None, plens, None, None, False, what)
    y, _ = D._fir(xp, plens, prep, False)
    out = torch.zeros(B, L, dtype=torch.float32, device=xp.device)
    d_lens, _ = CL.lens_args(lens, L, xp.device)
    # the slice and prepare's scale undone in one launch: rows start 2 half samples into the product
    call("mmx_scale_rows", _p(y.data_ptr() + 4 * 2 * half), y.shape[1], L, B, _p(d_lens), _p(gain), 1, _p(out), L, stream())
    return out


def _filter(x, lens, taps, what):
    """x fp32 [B, L]; taps: a list of B float64 tap sets (rows whose sets differ in length run as separate launch sequences, rows
    that share one array object as one shared filter) -> fp32 [B, L], zero past lens."""
    B, L = x.shape
    groups = {}
    for b, t in enumerate(taps):
        groups.setdefault(t.shape[-1], []).append(b)
    out = None
    for T, rows in groups.items():
        sub, sl = (x, lens) if len(rows) == B else (x[rows], [lens[b] for b in rows])
        Ls = sub.shape[1] if len(rows) == B else max(sl)
        sub = sub if len(rows) == B else sub[:, :Ls]
        xp, plens = pad_edge(sub, sl, (T - 1) // 2)
        same = all(taps[b] is taps[rows[0]] for b in rows)
        res = _fir_padded(xp, plens, sl, Ls, taps[rows[0]] if same else np.stack([taps[b] for b in rows]), what)
        if len(rows) == B:
            return res
        if out is None:
            out = torch.zeros(B, L, dtype=torch.float32, device=x.device)
        out[rows, :Ls] = res
    return out


def _cutoffs(cutoff, B, what):
    return CL.per_clip(cutoff, B, f"{what}: cutoff")


def _band_filter(clips, cutoff, rate, zeros, lens, what, design):
    CL.on_device(what, clips)
    x, lens = CL.pack(clips, lens, what)
    fs = _cutoffs(cutoff, len(lens), what)
    for f in sorted(set(fs)):                            # each clip's filter is its own: half comes from its own cutoff
        _refuse(what, refusal(lens, rate, [f], zeros))
    made = {f: design(f, rate, zeros) for f in set(fs)}
    return CL.unpack(_filter(x, lens, [made[f] for f in fs], what), lens, clips)


@torch.no_grad()
def low_pass(clips, cutoff, rate, zeros=ZEROS, lens=None):
    """low_pass (dsp.py:153-183) for a ragged batch.  clips: a list of mono clips ([n] / [1, n]), one clip [n], or a padded batch
    [B, L] / [B, 1, L] with `lens`; cutoff in Hz, one value or one per clip (each clip's filter is designed from its own cutoff, as
    the reference's loop does).  Returns a list of [n] views for a list, a tensor of the input's shape (zero past `lens`) for a
    tensor.  MmxError where refusal() gives a reason, or for a CPU tensor: nothing is launched then."""
    return _band_filter(clips, cutoff, rate, zeros, lens, "low_pass", lowpass_taps)


@torch.no_grad()
def high_pass(clips, cutoff, rate, zeros=ZEROS, lens=None):
    """high_pass (dsp.py:185-215): x - low_pass(x) as one filter, delta - lp.  Arguments and result as low_pass."""
    return _band_filter(clips, cutoff, rate, zeros, lens, "high_pass", highpass_taps)


def _curves(db, B, what):
    """db: one curve [n_bands] or one per clip [B, n_bands] (host values) -> float64 [B or 1, n_bands]."""
    if isinstance(db, torch.Tensor):
        if db.is_cuda:
            raise ValueError(f"{what}: pass the curve as host values, not a device tensor")
        db = db.double().numpy()
    db = np.asarray(db, dtype=np.float64)
    if db.ndim == 1:
        db = db[None]
    if db.ndim != 2 or db.shape[0] not in (1, B):
        raise ValueError(f"{what}: one curve [n_bands], or one per clip ({B}), got {tuple(db.shape)}")
    return db


def _equalize(x, lens, db, rate, what):
    db = _curves(db, len(lens), what)
    _refuse(what, refusal(lens, rate, n_bands=db.shape[1]))
    h = equalizer_taps(rate, db)
    return _filter(x, lens, [h[0]] * len(lens) if h.shape[0] == 1 else [h[b] for b in range(len(lens))], what)


@torch.no_grad()
def equalizer(clips, db, rate, lens=None):
    """equalizer (effects.py:405-433): the bands of julius.SplitBands(rate, n_bands) weighted by 10**db (sic) and summed, as ONE
    filter per clip.  db: one curve [n_bands] or one per clip [B, n_bands], host values.  Clips and result as low_pass."""
    CL.on_device("equalizer", clips)
    x, lens = CL.pack(clips, lens, "equalizer")
    return CL.unpack(_equalize(x, lens, db, rate, "equalizer"), lens, clips)


@torch.no_grad()
def mel_filterbank(clips, n_bands, rate, lens=None):
    """mel_filterbank (effects.py:386-403): the clip split into n_bands mel-spaced bands, one launch sequence per band over the once
    padded rows -> the last axis is the band: [B, L, n_bands] for [B, L] (zero past `lens`), [n, n_bands] for one clip, a list of
    [n, n_bands] for a list."""
    CL.on_device("mel_filterbank", clips)
    x, lens = CL.pack(clips, lens, "mel_filterbank")
    _refuse("mel_filterbank", refusal(lens, rate, n_bands=n_bands))
    bank = band_taps(rate, n_bands)
    xp, plens = pad_edge(x, lens, (bank.shape[1] - 1) // 2)
    out = torch.stack([_fir_padded(xp, plens, lens, x.shape[1], bank[k], "mel_filterbank") for k in range(bank.shape[0])], dim=-1)
    if isinstance(clips, torch.Tensor):
        return out.reshape(*clips.shape, bank.shape[0])
    return [out[b, :v] for b, v in enumerate(lens)]


def order_statistics(x, ranks, lens=None):
    """mmx_row_select: x fp32 [B, L] on the device, ranks a list of B lists of R <= SELECT_RANKS ints (0 = the smallest) ->
    (fp32 [B, R] the order statistics of each row's first lens[b] samples, int32 [B] 1 where the row holds a NaN)."""
    CL.on_device("order_statistics", x)
    B, L = x.shape
    lens = [L] * B if lens is None else [int(v) for v in lens]
    flat = [int(v) for row in ranks for v in row]
    R = len(flat) // B
    if len(ranks) != B or any(len(row) != R for row in ranks) or not 1 <= R <= SELECT_RANKS:
        raise ValueError(f"order_statistics: between 1 and {SELECT_RANKS} ranks for each of the {B} rows")
    if min(lens) < 1 or any(not 0 <= v < lens[b] for b, row in enumerate(ranks) for v in row):
        raise MmxError("order_statistics: an empty clip, or a rank outside the clip")
    d_lens, h_lens = CL.lens_args(lens, L, x.device)
    d_ranks = torch.tensor(flat, dtype=torch.int32, device=x.device)
    vals = torch.empty(B, R, dtype=torch.float32, device=x.device)
    flag = torch.empty(B, dtype=torch.int32, device=x.device)
    work = torch.empty(B * R * SELECT_WORK, dtype=torch.int32, device=x.device)
    call("mmx_row_select", _p(x), CL.row_stride(x), L, B, _p(d_lens), h_lens, _p(d_ranks), _host_i32(flat), R, _p(vals), _p(flag),
         _p(work), stream())
    return vals, flag


def _clip(x, lens, q, what):
    """-> (thresholds fp32 [B, 2], clipped fp32 [B, L] zero past lens)."""
    B, L = x.shape
    qs = CL.per_clip(q, B, f"{what}: clip_percentile")
    _refuse(what, refusal(lens, q=qs))
    plan = [clip_ranks(n, v) for n, v in zip(lens, qs)]
    stats, flag = order_statistics(x, [r for r, _ in plan], lens)
    w = torch.tensor([w for _, w in plan], dtype=torch.float64, device=x.device)
    d_lens, h_lens = CL.lens_args(lens, L, x.device)
    thr = torch.empty(B, 2, dtype=torch.float32, device=x.device)
    out = torch.empty(B, L, dtype=torch.float32, device=x.device)
    call("mmx_clip_rows", _p(x), CL.row_stride(x), L, B, _p(d_lens), h_lens, _p(stats), _p(w), _p(flag), _p(thr), _p(out), L, stream())
    return thr, out


@torch.no_grad()
def clip_distortion(clips, clip_percentile, lens=None):
    """clip_distortion (effects.py:435-461): each clip clamped to its own quantiles q / 2 and 1 - q / 2 (q one value or one per
    clip, in [0, 1]).  Clips and result as low_pass."""
    CL.on_device("clip_distortion", clips)
    x, lens = CL.pack(clips, lens, "clip_distortion")
    return CL.unpack(_clip(x, lens, clip_percentile, "clip_distortion")[1], lens, clips)


@torch.no_grad()
def clip_thresholds(clips, clip_percentile, lens=None):
    """The two thresholds clip_distortion clamps to -> fp32 [B, 2] on the device (NaN for a clip that holds a NaN)."""
    CL.on_device("clip_thresholds", clips)
    x, lens = CL.pack(clips, lens, "clip_thresholds")
    return _clip(x, lens, clip_percentile, "clip_thresholds")[0]


def _quantize(clips, channels, lens, mode, what):
    CL.on_device(what, clips)
    x, lens = CL.pack(clips, lens, what)
    B, L = x.shape
    qs = CL.per_clip(channels, B, f"{what}: quantization_channels")
    _refuse(what, refusal(lens, channels=qs))
    qs = [int(v) for v in qs]
    d_lens, h_lens = CL.lens_args(lens, L, x.device)
    out = torch.empty(B, L, dtype=torch.float32, device=x.device)
    call("mmx_quantize_rows", _p(x), CL.row_stride(x), L, B, _p(d_lens), h_lens, mode, _p(torch.tensor(qs, dtype=torch.int32, device=x.device)),
         _host_i32(qs), _p(out), L, stream())
    return CL.unpack(out, lens, clips)


@torch.no_grad()
def quantization(clips, quantization_channels, lens=None):
    """quantization (effects.py:463-490): 2 floor((x + 1) / 2 Q) / Q - 1, Q one whole number >= 2 or one per clip.  Clips and result
    as low_pass."""
    return _quantize(clips, quantization_channels, lens, 0, "quantization")


@torch.no_grad()
def mulaw_quantization(clips, quantization_channels, lens=None):
    """mulaw_quantization (effects.py:492-523) with mu = Q - 1.  Arguments and result as quantization."""
    return _quantize(clips, quantization_channels, lens, 1, "mulaw_quantization")


# ------------------------------------------------------------------------------------------------ modules
class LowPass(torch.nn.Module):
    """The reference's transform (data/transforms.py LowPass) with tensors in place of AudioSignal and an explicit cutoff in place of
    a sampled one: forward(audio, cutoff) -> low_pass(audio, cutoff, rate, zeros)."""

    def __init__(self, sample_rate: int, zeros: int = ZEROS):
        super().__init__()
        self.sample_rate, self.zeros = int(sample_rate), int(zeros)

    def forward(self, audio, cutoff, lens=None):
        return low_pass(audio, cutoff, self.sample_rate, zeros=self.zeros, lens=lens)


class HighPass(LowPass):
    """data/transforms.py HighPass: forward(audio, cutoff) -> high_pass(audio, cutoff, rate, zeros)."""

    def forward(self, audio, cutoff, lens=None):
        return high_pass(audio, cutoff, self.sample_rate, zeros=self.zeros, lens=lens)


class Equalizer(torch.nn.Module):
    """data/transforms.py Equalizer: forward(audio, eq) -> equalizer(audio, eq, rate); eq is the curve itself (the reference samples
    -eq_amount * rand(n_bands))."""

    def __init__(self, sample_rate: int):
        super().__init__()
        self.sample_rate = int(sample_rate)

    def forward(self, audio, eq, lens=None):
        return equalizer(audio, eq, self.sample_rate, lens=lens)


class ClippingDistortion(torch.nn.Module):
    """data/transforms.py ClippingDistortion: forward(audio, perc) -> clip_distortion(audio, perc)."""

    def forward(self, audio, perc, lens=None):
        return clip_distortion(audio, perc, lens=lens)


class Quantization(torch.nn.Module):
    """data/transforms.py Quantization: forward(audio, channels) -> quantization(audio, channels)."""

    def forward(self, audio, channels, lens=None):
        return quantization(audio, channels, lens=lens)


class MuLawQuantization(torch.nn.Module):
    """data/transforms.py MuLawQuantization: forward(audio, channels) -> mulaw_quantization(audio, channels)."""

    def forward(self, audio, channels, lens=None):
        return mulaw_quantization(audio, channels, lens=lens)
