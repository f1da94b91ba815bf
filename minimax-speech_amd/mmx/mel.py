"""Reference audio -> log-mel frames on the device (the `feat_extractor` of speech/config.yaml:183-191).

Reference: speech/matcha/utils/audio.py:45-82 (mel_spectrogram, center=False) and the inference branch of
cosyvoice/dataset/processor.py:339-392 (extract_reference_mel_from_speech: centre crop, peak normalisation).  The arithmetic is
one launch of mmx_logmel (csrc/mel.hip).  This module builds the tables of every spectral front end (that one, s3tok.LogMelW,
mmx/metrics.py): the windowed DFT basis and the mel filterbank in float64, both as three bf16 planes of their exact values.
There is no CPU fallback: a CPU tensor raises.

mel_filterbank restates what `librosa.filters.mel` builds with its defaults (htk=False, norm="slaney") from that function's
published definition; librosa itself is not a dependency (restated seams)."""
import math

import numpy as np
import torch

from . import clips as CL
from . import ops
from ._lib import BF16, F32, MmxError, TORCH_DT, call, stream, _p

LOG_CLIP = 1e-5                                          # audio.py:23 dynamic_range_compression_torch


def _hz_to_mel(f):
    """Slaney's auditory-toolbox scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor 6.4)."""
    f = np.asarray(f, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp, min_log_hz = 200.0 / 3, 1000.0
    min_log_mel, logstep = min_log_hz / f_sp, math.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def mel_filterbank(sr, n_fft, n_mels, fmin=0.0, fmax=None, dtype=np.float32):
    """[n_mels, n_fft // 2 + 1] triangular filters, centres equally spaced on the Slaney mel scale between fmin and fmax
    (None: sr / 2), each scaled by 2 / (its band's width in Hz) so that every filter has about unit area.  Computed in float64;
    the result is rounded to `dtype` where the published implementation rounds (the ramps, then the scaled rows)."""
    fmax = float(sr) / 2 if fmax is None else float(fmax)
    fft_f = np.fft.rfftfreq(n_fft, 1.0 / sr)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(fmin), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fft_f[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    w = np.maximum(0.0, np.minimum(lower, upper)).astype(dtype)
    enorm = 2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels])
    return (w.astype(np.float64) * enorm[:, None]).astype(dtype)


def nonzero_bins(fb):
    """(first bin, count) of the columns of a filterbank that carry a non-zero weight."""
    nz = np.flatnonzero(np.asarray(fb).any(axis=0))
    return int(nz[0]), int(nz[-1] - nz[0] + 1)


def frames_of(n, n_fft, hop):
    """Frames of a clip of n samples (audio.py:57-75: reflect padding by (n_fft - hop) / 2, center=False)."""
    pad = (n_fft - hop) // 2
    return (n + 2 * pad - n_fft) // hop + 1 if (n > pad and n + 2 * pad >= n_fft) else 0


def planes3(v64):
    """float64 -> three bf16 terms hi + mid + lo (24 significant bits), round to nearest each."""
    out, r = [], v64
    for _ in range(3):
        t = r.to(torch.bfloat16)
        out.append(t)
        r = r - t.double()
    return out


_planes3 = planes3


def dft_basis(n_fft, bin0=0, n_bins=None, kp=None, window=None):
    """float64 [2 * (n_bins rounded up to 32), kp] for bins bin0 .. bin0 + n_bins - 1 (None: up to n_fft // 2): bin bin0 + i ->
    row 32 * (i // 16) + i % 16 = hann[k] cos(2 pi (bin0 + i) k / n_fft), that row + 16 the sine (a 16-row tile pair per 16 bins);
    the phase reduced exactly in integers; periodic Hann window (torch.hann_window's default) folded in, or `window` [n_fft] (its
    values taken as float64) in its place.  kp (None: n_fft) pads the K dimension: columns at and beyond n_fft are zero."""
    n_bins = n_fft // 2 + 1 - bin0 if n_bins is None else n_bins
    k = torch.arange(n_fft, dtype=torch.int64)
    bins = torch.arange(bin0, bin0 + n_bins, dtype=torch.int64)
    ang = ((bins[:, None] * k[None, :]) % n_fft).double() * (2 * math.pi / n_fft)
    if window is None:
        hann = 0.5 - 0.5 * torch.cos(k.double() * (2 * math.pi / n_fft))
    else:
        hann = torch.as_tensor(window).double().reshape(n_fft)
    i = torch.arange(n_bins)
    rows = 32 * (i // 16) + i % 16
    basis = torch.zeros(2 * ops.round_up(n_bins, 32), n_fft if kp is None else kp, dtype=torch.float64)
    basis[rows, :n_fft] = hann * torch.cos(ang)
    basis[rows + 16, :n_fft] = hann * torch.sin(ang)
    return basis


def filter_table(fb, bin0, n_bins):
    """float64 [n_mels rounded up to 16, n_bins rounded up to 32]: columns bin0 .. bin0 + n_bins - 1 of the fp32 filterbank the
    reference holds, zero padded."""
    filt = torch.zeros(ops.round_up(fb.shape[0], 16), ops.round_up(n_bins, 32), dtype=torch.float64)
    filt[:fb.shape[0], :n_bins] = torch.from_numpy(fb[:, bin0:bin0 + n_bins].astype(np.float64))
    return filt


def packed3(m64, dev):
    """A float64 table -> its three bf16 planes on `dev`, each in mmx_pack_skinny order, one after the other."""
    return torch.cat([ops.pack_skinny(p.to(dev).contiguous(), dtype=BF16) for p in planes3(m64)])


def crop_bounds(n, sample_rate, min_length=0.5, max_length=4.0):
    """processor.py:345-376 with training=False: (start, stop) of the segment a clip of n samples contributes."""
    min_samples, max_samples = int(min_length * sample_rate), int(max_length * sample_rate)
    if n < min_samples:
        raise ValueError(f"reference clip is too short: {n / sample_rate:.2f} s < {min_length} s")
    if n > max_samples:
        start = (n - max_samples) // 2
        return start, start + max_samples
    return 0, n


def prepare_reference(wave, sample_rate, min_length=0.5, max_length=4.0):
    """The inference branch of extract_reference_mel_from_speech (processor.py:339-392): wave [n] or [1, n] on the device ->
    (segment [1, n'] fp32 (a view: centre crop to max_length), gain [1] fp32 = 1 / max|segment| computed on the device, 1 for
    silence).  The normalised clip of processor.py:387 is segment * gain; mmx_logmel applies the gain itself."""
    if not wave.is_cuda:
        raise MmxError("prepare_reference works on device memory only (no CPU fallback)")
    w = wave.reshape(1, -1).to(torch.float32)
    a, b = crop_bounds(w.shape[1], sample_rate, min_length, max_length)
    seg = w[:, a:b]
    peak = seg.abs().amax(dim=1)
    gain = torch.where(peak > 0, 1.0 / peak, torch.ones_like(peak))
    return seg, gain


class _LogMelTables:
    """What LogMel and s3tok.LogMelW share: one instance per (setting, device) holding the device tables (DFT basis planes,
    filter planes, bin range), and the plumbing of a call.  A subclass gives _build, frames, its entry point's name, whether that
    takes a per-member gain, and whether a bf16 result needs the fp32 channel-major one beside it."""

    _entry, _takes_gain, _fp32_cm = None, False, False

    def __init_subclass__(cls):
        cls._cache = {}

    @classmethod
    def _cached(cls, device, *setting):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise MmxError(f"{cls.__name__} works on device memory only (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self = cls._cache.get((*setting, dev))
        if self is None:
            self = object.__new__(cls)
            self._build(*setting, dev)
            cls._cache[(*setting, dev)] = self
        return self

    def _tables(self, fb, kp=None):
        self.filterbank = fb                             # fp32, as the reference holds it
        self.bin0, self.n_bins = nonzero_bins(fb)
        self.basis = packed3(dft_basis(self.n_fft, self.bin0, self.n_bins, kp), self.dev)
        self.filt = packed3(filter_table(fb, self.bin0, self.n_bins), self.dev)

    def _run(self, wave, lens, gain, time_major, dtype, out):
        CL.on_device(self._entry, wave)
        wave, lens = CL.pack(wave, lens, self._entry)
        B, L = wave.shape
        d_lens, h_lens = CL.lens_args(lens, L, wave.device)
        T = max(1, max(self.frames(n) for n in lens))                # a member without a frame: the entry point refuses it
        if time_major:
            if out is None:
                out = torch.empty(B, T, self.n_mels, dtype=TORCH_DT[dtype], device=wave.device)
            assert out.is_contiguous() and tuple(out.shape) == (B, T, self.n_mels) and out.dtype == TORCH_DT[dtype]
            cm, tm = None, out
            if self._fp32_cm and out.dtype != torch.float32:
                cm = torch.empty(B, self.n_mels, T, device=wave.device)
        else:
            cm, tm = torch.empty(B, self.n_mels, T, device=wave.device), None
        if gain is not None:
            gain = gain.to(torch.float32).reshape(B).contiguous()
        if self._takes_gain:
            call("mmx_logmel", _p(wave), CL.row_stride(wave), L, B, _p(gain), _p(d_lens), h_lens, _p(self.basis), _p(self.filt),
                 self.n_fft, self.hop, self.bin0, self.n_bins, self.n_mels, _p(cm), T, _p(tm), T, dtype, stream())
        else:
            call("mmx_logmel_w", _p(wave), CL.row_stride(wave), L, B, _p(d_lens), h_lens, _p(self.basis), _p(self.filt),
                 self.n_fft, self.hop, self.bin0, self.n_bins, self.n_mels, _p(cm), T, _p(tm), T, dtype, stream())
        return tm if time_major else cm


class LogMel(_LogMelTables):
    """The device tables of one mel setting and the launch of mmx_logmel."""

    _entry, _takes_gain = "mmx_logmel", True

    def __new__(cls, n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0, fmax=8000, device="cuda"):
        return cls._cached(device, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax)

    def _build(self, n_fft, num_mels, sr, hop, win, fmin, fmax, dev):
        if win != n_fft:
            raise NotImplementedError("win_size == n_fft only: the window is folded into the DFT basis")
        if n_fft % 32 or num_mels > 128 or hop % 8 or (n_fft - hop) % 2 or not 0 < hop <= n_fft:
            raise MmxError(f"mmx_logmel: unsupported setting n_fft {n_fft} hop {hop} n_mels {num_mels}")
        self.n_fft, self.hop, self.n_mels, self.dev = n_fft, hop, num_mels, dev
        self.pad = (n_fft - hop) // 2
        self._tables(mel_filterbank(sr, n_fft, num_mels, fmin, fmax))

    def frames(self, n):
        return frames_of(n, self.n_fft, self.hop)

    @torch.no_grad()
    def __call__(self, wave, lens=None, gain=None, time_major=False, dtype=F32, out=None):
        """wave fp32 [B, L] on the device (zero padded where `lens`, a list of ints, gives fewer valid samples per member);
        gain fp32 [B] on the device or None -> log-mel [B, n_mels, T] fp32 (the reference function's result), or with
        time_major=True [B, T, n_mels] in the activation type of `dtype` (written into `out` when given).  T = the frames of the
        longest member; a shorter member's remaining frames are 0."""
        return self._run(wave, lens, gain, time_major, dtype, out)
