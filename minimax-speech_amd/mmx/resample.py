"""Sample-rate conversion on the device: what the reference asks of `torchaudio.transforms.Resample`
(cosyvoice/utils/file_utils.py:44-50 load_wav, cli/frontend.py:157-162, tools/extract_speech_token.py:30,
tools/extract_embedding.py:30) as one launch of mmx_resample_sinc (csrc/resample.hip) over a ragged batch of mono clips.

The filter is the polyphase windowed sinc torchaudio documents as `sinc_interp_hann`, restated here from that description
(torchaudio is not a dependency; DESIGN.md §2, restated seams): with the rates reduced by their gcd to o -> n,
base = min(o, n) * rolloff and width = ceil(lowpass_filter_width * o / base), output j of a clip x[0 .. L) is

    y[j] = (base / o) * sum_m x[m] * sinc(pi t) * cos^2(pi t / (2 lowpass_filter_width)),   t = base * (m / o - j / n),

over the m with |t| < lowpass_filter_width, x = 0 outside the clip, ceil(n * L / o) outputs.  This module builds the taps in
float64, rounds them once to fp32 and packs the live ones per phase; the arithmetic is the kernel's.  There is no CPU fallback:
a CPU tensor raises MmxError."""
import math

import numpy as np
import torch

from . import clips as CL
from ._lib import MmxError, call, stream, _p

NOUT = 1024                                              # include/mmx_hip.h MMX_RESAMPLE_NOUT: outputs per workgroup


def _reduced(orig, new):
    orig, new = int(orig), int(new)
    if orig <= 0 or new <= 0:
        raise ValueError(f"sample rates must be positive: {orig} -> {new}")
    g = math.gcd(orig, new)
    return orig // g, new // g


def _width(o, n, lowpass_filter_width, rolloff):
    return int(math.ceil(int(lowpass_filter_width) * o / (min(o, n) * float(rolloff))))


def _taps64(o, n, lowpass_filter_width, rolloff, k):
    """(float64 taps, their mask |t| < lowpass_filter_width) at the dense tap indices k [n, K] (int64; row p = phase p); the taps
    outside the mask are 0."""
    lpw = int(lowpass_filter_width)
    base = min(o, n) * float(rolloff)
    width = _width(o, n, lpw, rolloff)
    p = np.arange(n, dtype=np.int64)
    # t = base * (m / o - j / n) with the difference taken exactly in integers: m n - j o = (k - width) n - p o in every frame
    t = base * ((k - width) * n - p[:, None] * o).astype(np.float64) / (o * n)
    live = np.abs(t) < lpw
    pt = np.pi * t
    sinc = np.where(t == 0, 1.0, np.sin(pt) / np.where(t == 0, 1.0, pt))
    h = sinc * np.cos(pt / (2 * lpw)) ** 2 * (base / o)
    return np.where(live, h, 0.0), live


def sinc_kernel(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """(dense fp32 bank [n, 2 * width + o], width): tap k of phase p multiplies x[f * o + k - width] of frame f = j // n,
    p = j % n.  Evaluated in float64 and rounded once; the taps with |t| >= lowpass_filter_width are exactly 0."""
    o, n = _reduced(orig, new)
    width = _width(o, n, lowpass_filter_width, rolloff)
    h, _ = _taps64(o, n, lowpass_filter_width, rolloff, np.broadcast_to(np.arange(2 * width + o, dtype=np.int64), (n, 2 * width + o)))
    return h.astype(np.float32), width


def out_len(L, orig, new):
    """Outputs of a clip of L samples: ceil(new * L / orig) in integers."""
    o, n = _reduced(orig, new)
    return (n * int(L) + o - 1) // o


def _packed(orig, new, lowpass_filter_width=6, rolloff=0.99):
    """The device form of sinc_kernel's bank: (taps fp32 [cmax, n] tap-major, first int32 [n], count int32 [n], width).  Phase p's
    live taps are the dense columns first[p] .. first[p] + count[p] - 1 (|t| < lowpass_filter_width is an interval of k);
    taps[c, p] = dense[p, first[p] + c], zero for c >= count[p].  Only the window of the dense row that can be live is evaluated
    (the samples within width + 1 of o p / n), so a pair whose dense bank would be huge still packs, and the entry point, not
    the host's memory, decides whether the kernel takes it."""
    o, n = _reduced(orig, new)
    width = _width(o, n, lowpass_filter_width, rolloff)
    k0 = (np.arange(n, dtype=np.int64) * o) // n - 1     # dense index of the sample width + 1 before o p / n
    h, live = _taps64(o, n, lowpass_filter_width, rolloff, k0[:, None] + np.arange(2 * width + 3, dtype=np.int64)[None, :])
    lead = live.argmax(axis=1)
    first, count = (k0 + lead).astype(np.int32), live.sum(axis=1).astype(np.int32)
    assert first.min() >= 0 and count.min() >= 1 and count.max() <= 2 * width and (first + count).max() <= 2 * width + o
    taps = np.zeros((int(count.max()), n), dtype=np.float32)
    for c in range(taps.shape[0]):                       # beyond a phase's count the window holds zeros (or ends)
        col = np.minimum(lead + c, h.shape[1] - 1)
        taps[c] = np.where(c < count, h[np.arange(n), col], 0.0).astype(np.float32)
    return taps, first, count, width


class Resample:
    """`torchaudio.transforms.Resample(orig_freq, new_freq)` on device memory: the packed bank of one setting and the launch.
    One object per setting (cached, like mel.LogMel); its tables are uploaded to a device the first time a clip on it arrives."""

    _cache = {}

    def __new__(cls, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99,
                device="cuda"):
        if resampling_method != "sinc_interp_hann":
            raise NotImplementedError(f"resampling_method {resampling_method!r}: only sinc_interp_hann (the reference's default) is built")
        if torch.device(device).type != "cuda":
            raise MmxError("Resample works on device memory only (no CPU fallback)")
        key = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), str(device))
        self = cls._cache.get(key)
        if self is None:
            self = super().__new__(cls)
            self.orig_freq, self.new_freq = key[0], key[1]
            self.lowpass_filter_width, self.rolloff = key[2], key[3]
            self.o, self.n = _reduced(*key[:2])
            self._host, self._tables = None, {}
            cls._cache[key] = self
        return self

    def out_len(self, L):
        return out_len(L, self.o, self.n)

    def _device_tables(self, dev):
        if dev not in self._tables:
            if self._host is None:
                self._host = _packed(self.o, self.n, self.lowpass_filter_width, self.rolloff)
            taps, first, count, _ = self._host
            self._tables[dev] = tuple(torch.from_numpy(a).to(dev) for a in (taps, first, count))
        return self._tables[dev]

    def _run(self, wave, lens):
        """wave fp32 [B, L] on the device (unit stride along L), lens a list of B ints -> [B, out_len(longest)]: the one place that
        launches."""
        B, L = wave.shape
        taps, first, count = self._device_tables(wave.device)
        d_lens, h_lens = CL.lens_args(lens, L, wave.device)
        cols = max(1, self.out_len(max(lens)))
        if cols > 2 ** 31 - 1 - NOUT:
            raise MmxError(f"mmx_resample_sinc: {cols} output samples per clip do not fit the entry point's 32-bit column count")
        out = torch.empty(B, cols, dtype=torch.float32, device=wave.device)
        call("mmx_resample_sinc", _p(wave), CL.row_stride(wave), L, B, _p(d_lens), h_lens, self.o, self.n, self._host[3], _p(taps),
             _p(first), _p(count), taps.shape[0], _p(out), cols, cols, stream())
        return out

    @torch.no_grad()
    def __call__(self, wave, lens=None):
        """wave [n] or [B, L] on the device (zero padded where `lens`, a list of ints, gives fewer valid samples per clip) ->
        fp32 [out_len(n)] or [B, out_len(longest)], a shorter clip's remaining columns 0.  Equal rates: the input itself."""
        if self.orig_freq == self.new_freq:
            return wave
        CL.on_device("Resample", wave)
        out = self._run(*CL.pack(wave, lens, "Resample"))
        return out[0] if wave.dim() == 1 else out


def resample(waves, orig, new):
    """A ragged list of mono clips ([n] or [1, n], on one device) -> the list of their resampled clips, one launch: views of one
    buffer, each cut to its clip's output length.  A clip's values are those of its own solo run, bit for bit."""
    waves = list(waves)
    if int(orig) == int(new) or not waves:
        return [w.reshape(-1) for w in waves]
    CL.on_device("resample", waves)
    rs = Resample(orig, new)
    x, lens = CL.pack(waves, None, "resample")
    return CL.unpack(rs._run(x, lens), [rs.out_len(n) for n in lens], waves)
