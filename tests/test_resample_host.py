"""Host side of the sinc resampler (mmx/resample.py): the bank, the output length, the packed device form and the guards, without a
GPU.  The yardstick is the closed-form sum of `sinc_interp_hann`, evaluated here in float64 straight from its definition

    y[j] = (base / o) * sum_m x[m] * sinc(pi t) * cos^2(pi t / (2 lpw)),   t = base * (m / o - j / n),   |t| < lpw,

with m / o - j / n taken as the exact integer m n - j o over o n, so it knows nothing of frames, phases or the packed layout.
tests/test_gpu_resample.py measures the kernel against `resample_f64` of this file."""
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(16000, 24000), (48000, 16000), (48000, 24000), (44100, 16000), (44100, 24000), (22050, 24000), (8000, 16000)]
WIDTHS = [7, 19, 13, 17, 12, 7, 7]
LPW, ROLLOFF = 6, 0.99


def reduced(orig, new):
    g = math.gcd(orig, new)
    return orig // g, new // g


def tap_f64(m, j, o, n):
    """(h, live) in float64 of input sample m for output j (integer arrays that broadcast).  As the documented algorithm does, t is
    clamped to [-lpw, lpw] before the window, which turns the taps outside the sum into cos^2(pi / 2) ~ 4e-33 times a sinc zero."""
    base = min(o, n) * ROLLOFF
    t = base * (np.asarray(m, dtype=np.int64) * n - np.asarray(j, dtype=np.int64) * o).astype(np.float64) / (o * n)
    live = np.abs(t) < LPW
    t = np.clip(t, -LPW, LPW)
    pt = np.pi * t
    sinc = np.where(t == 0, 1.0, np.sin(pt) / np.where(t == 0, 1.0, pt))
    return sinc * np.cos(pt / (2 * LPW)) ** 2 * (base / o), live


def width_of(o, n):
    return int(math.ceil(LPW * o / (min(o, n) * ROLLOFF)))


def resample_f64(x, orig, new):
    """x [L] (any float type, read as float64) -> (y64 [ceil(n L / o)], sum_m |h x| per output, live taps per output): the closed form,
    every output from the samples around o j / n that can be live."""
    o, n = reduced(orig, new)
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    J = (n * L + o - 1) // o
    j = np.arange(J, dtype=np.int64)[:, None]
    W = width_of(o, n)
    m = (j * o) // n + np.arange(-W - 1, W + 2, dtype=np.int64)[None, :]
    h, live = tap_f64(m, j, o, n)
    h = np.where(live, h, 0.0)
    xm = np.where((m >= 0) & (m < L), x[np.clip(m, 0, L - 1)], 0.0)
    return (h * xm).sum(axis=1), np.abs(h * xm).sum(axis=1), live.sum(axis=1)


@pytest.mark.parametrize("pair,width", list(zip(PAIRS, WIDTHS)))
def test_sinc_kernel_equals_the_formula(pair, width):
    """Shape, width, every entry = fp32(float64 formula), dead taps exactly 0, at most 2 width live taps and unit DC gain per phase."""
    from mmx.resample import sinc_kernel
    o, n = reduced(*pair)
    h, w = sinc_kernel(*pair)
    assert w == width == width_of(o, n) and h.dtype == np.float32 and h.shape == (n, 2 * width + o)
    k, p = np.arange(2 * width + o)[None, :], np.arange(n)[:, None]
    h64, live = tap_f64(k - width, p, o, n)                 # frame 0: m = k - width, j = p
    assert np.abs(h64[~live]).max(initial=0.0) < 2e-49        # what the formula itself gives at |t| >= lpw: 0 in fp32
    assert np.array_equal(h, h64.astype(np.float32))
    assert (h[~live] == 0.0).all()
    assert live.sum(axis=1).max() <= 2 * width
    gain = np.abs(h.astype(np.float64).sum(axis=1) - 1.0).max()
    print(f"\n{pair}: width {width}, live <= {live.sum(axis=1).max()}, DC gain error {gain:.2e}")
    assert gain <= 1e-3


def test_bank_is_the_same_in_every_frame():
    """The frame / phase form: the taps of output j = f n + p on samples f o + k - width are the bank's row p, whatever f."""
    for pair in PAIRS:
        o, n = reduced(*pair)
        w = width_of(o, n)
        k, p = np.arange(2 * w + o)[None, :], np.arange(n)[:, None]
        h0, _ = tap_f64(k - w, p, o, n)
        h9, _ = tap_f64(977 * o + k - w, 977 * n + p, o, n)
        assert np.array_equal(h0, h9)


@pytest.mark.parametrize("pair", PAIRS)
def test_out_len(pair):
    from mmx.resample import out_len
    o, n = reduced(*pair)
    for L in sorted({1, max(1, o - 1), o, o + 1, 1000}):
        want = -((-n * L) // o)
        assert out_len(L, *pair) == want == math.ceil(n * L / o)
        assert len(resample_f64(np.zeros(L), *pair)[0]) == want
    assert out_len(2 ** 31 - 1, 8000, 16000) == 2 ** 32 - 2       # beyond 32 bits


@pytest.mark.parametrize("pair", PAIRS)
def test_packed_form_expands_to_the_dense_bank(pair):
    from mmx.resample import _packed, sinc_kernel
    h, width = sinc_kernel(*pair)
    taps, first, count, w = _packed(*pair)
    n = h.shape[0]
    assert w == width and taps.dtype == np.float32 and taps.shape == (int(count.max()), n) and count.max() <= 2 * width
    assert first.dtype == count.dtype == np.int32 and first.shape == count.shape == (n,)
    assert {(16000, 24000): 13, (48000, 16000): 37, (44100, 16000): 34}.get(pair, count.max()) == count.max()
    dense = np.zeros_like(h)
    for p in range(n):
        assert first[p] >= 0 and first[p] + count[p] <= h.shape[1]
        dense[p, first[p]:first[p] + count[p]] = taps[:count[p], p]
        assert (taps[count[p]:, p] == 0).all()
    assert np.array_equal(dense, h)
    if pair == (44100, 16000):
        assert h.nbytes == 160 * 475 * 4 and taps.nbytes == 160 * 34 * 4


def test_guards():
    from mmx._lib import MmxError
    from mmx.resample import Resample, resample
    with pytest.raises(NotImplementedError):
        Resample(16000, 24000, resampling_method="sinc_interp_kaiser")
    with pytest.raises(MmxError):
        Resample(16000, 24000)(torch.zeros(100))
    with pytest.raises(MmxError):
        Resample(16000, 24000, device="cpu")
    with pytest.raises(MmxError):
        resample([torch.zeros(100)], 16000, 24000)
    x = torch.zeros(100)
    assert Resample(16000, 16000)(x) is x
    assert Resample(16000, 24000) is Resample(16000, 24000)          # one object per setting


def test_symbol_is_declared_bound_and_documented():
    from mmx import _lib, resample
    s = "mmx_resample_sinc"
    hdr = open(os.path.join(ROOT, "include", "mmx_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert re.search(r"\bint\s+" + s + r"\s*\(", hdr) and s in _lib.SYMBOLS and f"`{s}`" in doc and hasattr(_lib.load(), s)
    assert int(re.search(r"#define MMX_RESAMPLE_NOUT (\d+)", hdr).group(1)) == resample.NOUT
    assert _lib.load().mmx_abi_version() == 10
