"""Float64 numpy restatement of the STOI definition in mmx/stoi.py (rules 1 - 7), written from that text in the order the host
library computes, and the fixtures of tests/test_stoi_host.py and tests/test_gpu_stoi.py.  It is the yardstick of both; it has not
been compared against pystoi, which is not available here."""
import functools

import numpy as np

FS, FRAME, HOP, NFFT, BANDS, SEG = 10000, 256, 128, 512, 15, 30
BETA, DYN_RANGE, EPS = -15.0, 40.0, np.finfo(np.float64).eps
EDGES = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109), (109, 138),
         (138, 174), (174, 219)]


def window():
    return np.hanning(FRAME + 2)[1:-1]


def starts(n):
    return list(range(0, n - FRAME, HOP))                # i < n - 256, strict


def band_matrix():
    f = np.linspace(0, FS, NFFT + 1)[:NFFT // 2 + 1]
    obm = np.zeros((BANDS, NFFT // 2 + 1))
    edges = []
    for k in range(BANDS):
        lo, hi = 150.0 * 2.0 ** ((2 * k - 1) / 6), 150.0 * 2.0 ** ((2 * k + 1) / 6)
        a, b = int(np.argmin((f - lo) ** 2)), int(np.argmin((f - hi) ** 2))
        obm[k, a:b] = 1.0
        edges.append((a, b))
    return obm, edges


def energies(x):
    w = window()
    return np.array([20 * np.log10(np.linalg.norm(w * x[i:i + FRAME]) + EPS) for i in starts(len(x))])


def select(x):
    """(energies, keep mask, source frames of the kept frames) of the reference x."""
    e = energies(x)
    keep = (np.max(e) - DYN_RANGE - e) < 0
    return e, keep, np.flatnonzero(keep)


def rebuild(sig, kept):
    w = window()
    out = np.zeros((len(kept) - 1) * HOP + FRAME)
    for k, f in enumerate(kept):
        out[k * HOP:k * HOP + FRAME] += w * sig[f * HOP:f * HOP + FRAME]
    return out


def envelopes(sig):
    """[15, frames]: sqrt of the band sums of |rfft(w frame, 512)|^2 over the frames of sig."""
    w = window()
    obm, _ = band_matrix()
    spec = np.array([np.fft.rfft(w * sig[i:i + FRAME], NFFT) for i in starts(len(sig))]).reshape(-1, NFFT // 2 + 1).T
    return np.sqrt(obm @ (np.abs(spec) ** 2))


def segments(e):
    return np.array([e[:, m - SEG:m] for m in range(SEG, e.shape[1] + 1)])       # [J, 15, 30]


def score(xb, yb, extended=False):
    """Rules 5 - 7 from the band envelopes [15, frames] of the reference (xb) and the estimate (yb)."""
    if xb.shape[1] < SEG:
        return 1e-5
    xs, ys = segments(xb), segments(yb)
    J = xs.shape[0]
    if extended:
        def rowcol(s):
            s = s - s.mean(axis=2, keepdims=True)
            s = s / (np.linalg.norm(s, axis=2, keepdims=True) + EPS)
            s = s - s.mean(axis=1, keepdims=True)
            return s / (np.linalg.norm(s, axis=1, keepdims=True) + EPS)
        return float(np.sum(rowcol(xs) * rowcol(ys) / SEG) / J)
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    yp = np.minimum(ys * c, xs * (1 + 10 ** (-BETA / 20)))
    yp = yp - yp.mean(axis=2, keepdims=True)
    xc = xs - xs.mean(axis=2, keepdims=True)
    yp = yp / (np.linalg.norm(yp, axis=2, keepdims=True) + EPS)
    xc = xc / (np.linalg.norm(xc, axis=2, keepdims=True) + EPS)
    return float(np.sum(yp * xc) / (J * BANDS))


def clipped_share(xb, yb):
    """Share of the (segment, band, frame) values at which rule 6's min takes its clip branch."""
    xs, ys = segments(xb), segments(yb)
    c = np.linalg.norm(xs, axis=2, keepdims=True) / (np.linalg.norm(ys, axis=2, keepdims=True) + EPS)
    return float(np.mean(ys * c > xs * (1 + 10 ** (-BETA / 20))))


def stoi(x, y, extended=False, detail=False):
    """x the reference, y the estimate: float arrays of equal length at 10 kHz.  detail: also dict(energy, keep, map, frames)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert x.shape == y.shape and x.ndim == 1
    e, keep, kept = select(x)
    xb, yb = envelopes(rebuild(x, kept)), envelopes(rebuild(y, kept))
    d = score(xb, yb, extended)
    if not detail:
        return d
    return d, dict(energy=e, keep=keep, map=kept, frames=xb.shape[1], xb=xb, yb=yb)


# ------------------------------------------------------------------------------------------------ fixtures (fp32 clips at 10 kHz)
GAPS = {4096: (), 4097: (), 4225: (), 4353: (), 4481: (), 6000: ((2000, 3200),), 12000: ((0, 1500), (5000, 7430), (11200, 12000))}
LENGTHS = tuple(GAPS)
KEPT = {4096: 30, 4097: 31, 4225: 32, 4353: 33, 4481: 34, 6000: 37, 12000: 60}     # of 30, 31, 32, 33, 34, 45 and 92 frames
ESTIMATES = ("same", "zero", "snr20", "snr0", "noise", "loud")


def _noise(n, seed):
    return np.random.default_rng(seed).standard_normal(n)


@functools.lru_cache(maxsize=None)
def reference(n):
    """Harmonics at 180 .. 4100 Hz with weights 1 / (k + 1), 2 % vibrato, a 3.1 Hz envelope, scale 0.2, white noise of standard
    deviation 0.02; the spans of GAPS[n] scaled by 1e-4.  fp32, as the device sees it."""
    t = np.arange(n) / FS
    vib = 1.0 + 0.02 * np.sin(2 * np.pi * 5.0 * t)
    x = np.zeros(n)
    for k, f in enumerate((180, 360, 540, 900, 1500, 2300, 3100, 4100)):
        x += np.sin(2 * np.pi * np.cumsum(f * vib) / FS) / (k + 1)
    x *= 0.2 * (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t))
    x += 0.02 * _noise(n, 1000 + n)
    for a, b in GAPS[n]:
        x[a:b] *= 1e-4
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def estimate(n, kind):
    x = reference(n).astype(np.float64)
    if kind == "same":
        y = x
    elif kind == "zero":
        y = np.zeros(n)
    elif kind in ("snr20", "snr0"):
        v = _noise(n, 2000 + n)
        y = x + v * np.sqrt(np.mean(x ** 2) / np.mean(v ** 2)) * 10.0 ** (-(20.0 if kind == "snr20" else 0.0) / 20)
    elif kind == "noise":
        y = 0.1 * _noise(n, 3000 + n)
    elif kind == "loud":                                 # the +20 dB SNR estimate, 30 dB louder
        y = estimate(n, "snr20").astype(np.float64) * 10.0 ** (30.0 / 20)
    else:
        raise KeyError(kind)
    return y.astype(np.float32)


@functools.lru_cache(maxsize=None)
def expected(n, kind, extended):
    """(d, detail) of the fixture pair in float64: computed once, shared by the tests."""
    return stoi(reference(n), estimate(n, kind), extended, detail=True)
