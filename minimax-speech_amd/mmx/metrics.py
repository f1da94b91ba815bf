"""Distances between an estimate and a reference waveform on the device, in the units the reference's codec is trained and
validated in: what dac-vae/train.py:706-709 reports (`stft/loss`, `mel/loss`, `waveform/loss`, through dac-vae/loss.py
MultiScaleSTFTLoss, MelSpectrogramLoss, L1Loss) plus SISDRLoss of the same file, and the `mse` / `snr` that
dac-vae/extract_dac_latents.py:89-95 writes per decoded sample.  One launch pair of mmx_spec_dist per scale and one of
mmx_wave_sums (csrc/metrics.hip) over a ragged batch, without a host sync and without a spectrogram in memory.

Definitions (audiotools/core/audio_signal.py:1185-1212, 1354-1369 restated; audiotools, scipy and librosa are not dependencies,
DESIGN.md §2, restated seams).  One scale with window length n:
    S = |torch.stft(x, n_fft=n, hop_length=n // 4, window=periodic Hann(n), center=True)|      [n // 2 + 1, 1 + len // (n // 4)]
    (center=True reflects the clip by n // 2 samples on each side; a clip needs more than n // 2 samples)
    mel mode: M = F S with F = mel_filterbank(rate, n, n_mels, fmin, fmax) in fp32 (Slaney scale and norm, librosa's defaults)
    d_log = mean |log10(max(a, clamp_eps)^pow) - log10(max(b, clamp_eps)^pow)|,   d_mag = mean |a - b|
    over the clip's own frames and the n // 2 + 1 bins (or n_mels mels); a, b the values of the estimate and the reference.
    distance = sum over the scales of log_weight * d_log + mag_weight * d_mag.
For a batch of equal-length clips the reference's L1Loss(reduction="mean") over the batched spectrogram is the mean over the
clips of these per-clip values.
Waveform, from the seven sums of mmx_wave_sums (n samples, x the estimate, y the reference):
    l1 = sum |x - y| / n,   mse = sum (x - y)^2 / n,   snr_db = 10 log10(var(y) / (mse + 1e-10)),  var = mean y^2 - (mean y)^2;
    sisdr_db = 10 log10(|alpha y0|^2 / |x0 - alpha y0|^2 + 1e-8) with x0, y0 the zero-mean signals and
    alpha = (<x0, y0> + 1e-8) / (|y0|^2 + 1e-8): SISDRLoss's formula with zero_mean, scaling and eps = 1e-8.  The residual is
    evaluated as |d0|^2 + 2 (1 - alpha) <d0, y0> + (1 - alpha)^2 |y0|^2 with d0 = x0 - y0, whose leading term is summed directly
    (no cancellation between |x0|^2 and |y0|^2 when the two signals are close).

mmx/mel.py builds the tables (float64; the window folded into the DFT basis); this module states the arithmetic around the launches.
There is no CPU fallback: a CPU tensor raises MmxError."""
import numpy as np
import torch

from . import clips as CL
from . import mel as MEL
from . import ops
from ._lib import MmxError, call, stream, _p

MEL_N_MELS = (5, 10, 20, 40, 80, 160, 320)               # dac-vae/loss.py:261-262
MEL_WINDOWS = (32, 64, 128, 256, 512, 1024, 2048)
STFT_WINDOWS = (2048, 512)                               # loss.py:176
VALIDATION_STFT_WINDOWS = (1024, 2048)                   # what train.py's validation step builds its stft_loss with
MAX_MELS = 384                                           # csrc/metrics.hip: SD_MT = 3 mel tiles per wave, 8 waves
LDS_BYTES = 160 * 1024
FRAMES_PER_TILE, SAMPLES_PER_CHUNK, GAP = 16, 4096, 16   # csrc/spec_tile.h: frame tile, GAP as csrc/metrics.hip sets it; its WS_CHUNK


def frames_of(n, n_fft):
    """Frames of a clip of n samples: torch.stft(center=True) with hop n_fft // 4."""
    return 1 + n // (n_fft // 4)


def padded_bins(n_fft):
    return ops.round_up(n_fft // 2 + 1, 32)


def lds_bytes(n_fft, n_mels=0):
    """Dynamic LDS of mmx_spec_dist's kernel (sd_lds of csrc/metrics.hip over spec_plane of csrc/spec_tile.h): sample planes of both
    signals (STFT mode) or of one signal and its magnitude planes (mel mode), plus the reduction buffer."""
    hop = n_fft // 4
    span = 15 * hop + n_fft
    planes = 3 * 2 * (span + GAP * -(-span // hop))
    return (planes + 3 * 16 * (padded_bins(n_fft) + 8) * 2 if n_mels else 2 * planes) + 128


def refusal(lens, n_fft, n_mels=0):
    """Why mmx_spec_dist refuses these clip lengths at this scale (the entry point returns MMX_EARG before any launch), or None."""
    if n_fft < 32 or n_fft % 32:
        return f"n_fft {n_fft} is not a positive multiple of 32"
    if not 0 <= n_mels <= MAX_MELS:
        return f"n_mels {n_mels} is outside [0, {MAX_MELS}]"
    if lds_bytes(n_fft, n_mels) > LDS_BYTES:
        return f"the planes of n_fft {n_fft} need {lds_bytes(n_fft, n_mels)} bytes of LDS"
    short = [n for n in lens if n <= n_fft // 2]
    if short:
        return f"a clip of {short[0]} samples cannot be reflected by {n_fft // 2}"
    return None


def dft_basis(n_fft):
    """float64 [2 * padded_bins, n_fft]: mel.dft_basis over all n_fft // 2 + 1 bins."""
    return MEL.dft_basis(n_fft, 0, n_fft // 2 + 1)


def mel_table(rate, n_fft, n_mels, fmin=0.0, fmax=None):
    """float64 [n_mels rounded up to 16, padded_bins]: the fp32 filterbank the reference holds, zero padded."""
    return MEL.filter_table(MEL.mel_filterbank(rate, n_fft, n_mels, fmin, fmax), 0, n_fft // 2 + 1)


def _device_tables(rate, n_fft, n_mels, fmin, fmax, dev):
    """(basis planes, filter planes or None) on `dev`, built once per (n_fft) and per (rate, n_fft, n_mels, fmin, fmax)."""
    basis = CL.device_tables(("metrics", int(n_fft), str(dev)), lambda: MEL.packed3(dft_basis(n_fft), dev))
    if not n_mels:
        return basis, None
    kf = ("metrics", int(rate), int(n_fft), int(n_mels), float(fmin), None if fmax is None else float(fmax), str(dev))
    return basis, CL.device_tables(kf, lambda: MEL.packed3(mel_table(rate, n_fft, n_mels, fmin, fmax), dev))


def spec_dist(x, y, lens, rate, n_fft, n_mels=0, fmin=0.0, fmax=None, pow=1.0, clamp_eps=1e-5, d_lens=None, h_lens=None):
    """One scale: x, y fp32 [B, L] on the device (unit stride along L), lens a list of ints or None -> f64 [B, 2] on the device
    (d_log, d_mag).  n_mels = 0: the STFT bins themselves.  MmxError where refusal() gives a reason: nothing is launched then."""
    CL.on_device("mmx_spec_dist", x, y)
    B, L = x.shape
    why = refusal(lens or [L], n_fft, n_mels)            # the entry point's own conditions, with a reason; nothing is launched
    if why:
        raise MmxError(f"mmx_spec_dist: {why}")
    basis, filt = _device_tables(rate, n_fft, n_mels, fmin, fmax, x.device)
    if d_lens is None:
        d_lens, h_lens = CL.lens_args(lens, L, x.device)
    cap = -(-frames_of(L, n_fft) // FRAMES_PER_TILE)
    work = torch.empty(B, cap, 2, dtype=torch.float64, device=x.device)
    out = torch.empty(B, 2, dtype=torch.float64, device=x.device)
    call("mmx_spec_dist", _p(x), CL.row_stride(x), _p(y), CL.row_stride(y), L, B, _p(d_lens), h_lens, _p(basis), _p(filt), int(n_fft),
         int(n_mels), float(clamp_eps), float(pow), _p(work), cap, _p(out), stream())
    return out


def wave_sums(x, y, lens=None, clip=None, d_lens=None):
    """x, y fp32 [B, L] on the device -> f64 [B, 7]: sum x, y, x^2, y^2, x y, |x - y|, (x - y)^2 over each clip's own samples,
    x limited to [-clip, clip] first when clip is given."""
    CL.on_device("mmx_wave_sums", x, y)
    B, L = x.shape
    if d_lens is None:
        d_lens, _ = CL.lens_args(lens, L, x.device)
    cap = -(-L // SAMPLES_PER_CHUNK)
    work = torch.empty(B, cap, 7, dtype=torch.float64, device=x.device)
    out = torch.empty(B, 7, dtype=torch.float64, device=x.device)
    call("mmx_wave_sums", _p(x), CL.row_stride(x), _p(y), CL.row_stride(y), L, B, _p(d_lens), 0.0 if clip is None else float(clip),
         _p(work), cap, _p(out), stream())
    return out


def sisdr_from_sums(s, n, scaling=True, zero_mean=True, eps=1e-8):
    """SISDRLoss's ratio in dB (positive: the loss is its negative) from mmx_wave_sums' sums s [B, 7] (x the estimate, y the
    reference) and the sample counts n [B]; tensors (any device) or numpy arrays, float64."""
    lib = torch if isinstance(s, torch.Tensor) else np
    sx, sy, sxx, syy, sxy, _, sdd = (s[..., k] for k in range(7))
    if zero_mean:
        yy, xy, dd = syy - sy * sy / n, sxy - sx * sy / n, sdd - (sx - sy) * (sx - sy) / n
    else:
        yy, xy, dd = syy, sxy, sdd
    alpha = (xy + eps) / (yy + eps) if scaling else 1.0
    dy = xy - yy                                           # <d0, y0>
    noise = dd + 2.0 * (1.0 - alpha) * dy + (1.0 - alpha) * (1.0 - alpha) * yy
    return 10.0 * lib.log10(alpha * alpha * yy / noise + eps)


def metrics_from_sums(s, n):
    """dict(l1, mse, snr_db, sisdr_db) from the seven sums s [B, 7] and the sample counts n [B] (float64; tensors or numpy)."""
    lib = torch if isinstance(s, torch.Tensor) else np
    mse = s[..., 6] / n
    var = s[..., 3] / n - (s[..., 1] / n) * (s[..., 1] / n)
    return dict(l1=s[..., 5] / n, mse=mse, snr_db=10.0 * lib.log10(var / (mse + 1e-10)), sisdr_db=sisdr_from_sums(s, n))


def _intake(est, ref, lens, what):
    """(x, y, lens, device lengths, host lengths) of a public call: CL.pack_pair, whose ValueErrors come before the device-only
    refusal, and one upload of the lengths for all the launches."""
    x, y, lens = CL.pack_pair(est, ref, lens, what)
    CL.on_device(what, x, y)
    return (x, y, lens) + CL.lens_args(lens, x.shape[1], x.device)


def _counts(x, d_lens):
    if d_lens is None:
        return torch.full((x.shape[0],), float(x.shape[1]), dtype=torch.float64, device=x.device)
    return d_lens.double()


def _multi_scale(x, y, lens, d_lens, h_lens, rate, windows, n_mels, fmin, fmax, pow, clamp_eps, log_weight, mag_weight):
    total = None
    for i, w in enumerate(windows):
        d = spec_dist(x, y, lens, rate, int(w), n_mels[i] if n_mels else 0, fmin[i] if n_mels else 0.0, fmax[i] if n_mels else None,
                      pow, clamp_eps, d_lens, h_lens)
        v = log_weight * d[:, 0] + mag_weight * d[:, 1]
        total = v if total is None else total + v
    return total


def _per_scale(v, n, name):
    v = list(v) if isinstance(v, (list, tuple)) else [v] * n
    if len(v) != n:
        raise ValueError(f"{name} needs one entry per window length ({n}), got {len(v)}")
    return v


@torch.no_grad()
def mel_distance(est, ref, rate, lens=None, n_mels=MEL_N_MELS, window_lengths=MEL_WINDOWS, pow=1.0, clamp_eps=1e-5, log_weight=1.0,
                 mag_weight=0.0, mel_fmin=0.0, mel_fmax=None):
    """MelSpectrogramLoss (dac-vae/loss.py:231-327, its defaults) per clip: est / ref two lists of mono clips or two padded
    tensors [B, L] / [B, 1, L] with `lens` -> f64 [B] on the device.  Nothing is read back."""
    x, y, lens, d_lens, h_lens = _intake(est, ref, lens, "mel_distance")
    nw = len(window_lengths)
    return _multi_scale(x, y, lens, d_lens, h_lens, rate, window_lengths, _per_scale(n_mels, nw, "n_mels"), _per_scale(mel_fmin, nw, "mel_fmin"),
                        _per_scale(mel_fmax, nw, "mel_fmax"), pow, clamp_eps, log_weight, mag_weight)


@torch.no_grad()
def stft_distance(est, ref, rate=None, lens=None, window_lengths=STFT_WINDOWS, pow=2.0, clamp_eps=1e-5, log_weight=1.0, mag_weight=1.0):
    """MultiScaleSTFTLoss (dac-vae/loss.py:142-228, its defaults) per clip -> f64 [B] on the device.  `rate` plays no part."""
    x, y, lens, d_lens, h_lens = _intake(est, ref, lens, "stft_distance")
    return _multi_scale(x, y, lens, d_lens, h_lens, rate, window_lengths, None, None, None, pow, clamp_eps, log_weight, mag_weight)


@torch.no_grad()
def waveform_distance(est, ref, lens=None, clip=None):
    """dict of f64 [B] device tensors: l1 (L1Loss), mse and snr_db = 10 log10(var(ref) / (mse + 1e-10)) (extract_dac_latents.py:94-95)
    and sisdr_db, SISDRLoss's ratio with its defaults (zero mean, scaling, eps 1e-8) as a POSITIVE number of dB: the reference's
    loss is its negative.  clip: the estimate is limited to [-clip, clip] first (the extractor clips its reconstruction to 1)."""
    x, y, lens, d_lens, h_lens = _intake(est, ref, lens, "waveform_distance")
    return metrics_from_sums(wave_sums(x, y, lens, clip, d_lens), _counts(x, d_lens))


@torch.no_grad()
def audio_distance(est, ref, rate, lens=None, clip=None):
    """What the reference's validation step and extractor say about a reconstruction, per clip: dict of f64 [B] device tensors
    mel (MelSpectrogramLoss as train.py configures it: pow 1, mag_weight 0, seven scales), stft (MultiScaleSTFTLoss with
    train.py's windows [1024, 2048]), l1, mse, snr_db, sisdr_db.  No value is read back."""
    x, y, lens, d_lens, h_lens = _intake(est, ref, lens, "audio_distance")
    nw = len(MEL_WINDOWS)
    out = dict(mel=_multi_scale(x, y, lens, d_lens, h_lens, rate, MEL_WINDOWS, list(MEL_N_MELS), [0.0] * nw, [None] * nw, 1.0, 1e-5, 1.0, 0.0),
               stft=_multi_scale(x, y, lens, d_lens, h_lens, rate, VALIDATION_STFT_WINDOWS, None, None, None, 2.0, 1e-5, 1.0, 1.0))
    out.update(metrics_from_sums(wave_sums(x, y, lens, clip, d_lens), _counts(x, d_lens)))
    return out
