"""Channel degradations (mmx/channel.py, csrc/channel.hip), the part that needs no GPU: a restatement of julius' LowPassFilters /
HighPassFilters / SplitBands and of the reference's equalizer, clip_distortion, quantization and mulaw_quantization
(dac-vae/audiotools/core/effects.py:386-523) as julius and the reference write them - replicate pad, conv1d, band differences, the
sum over weighted bands - against the module's host tables; the quantile ranks against torch.quantile; refusals; the wiring of the
new entry points.

julius is not a dependency and is not compared against: the invariants below pin the restatement (tap sets that sum to 1, a
constant clip that stays constant, low + high = x, bands that sum to x, a flat equalizer that is the identity)."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mmx import _lib
from mmx import channel as CH
from mmx import degrade as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement
def ref_sinc(t):
    return torch.where(t == 0, torch.ones_like(t), torch.sin(t) / torch.where(t == 0, torch.ones_like(t), t))


def ref_lowpass_filters(cutoffs, zeros, dtype=torch.float64):
    """julius.LowPassFilters.__init__ for normalised cutoffs (all > 0) -> (filters [K, 2 half + 1], half)."""
    half = int(zeros / min(cutoffs) / 2)
    window = torch.hann_window(2 * half + 1, periodic=False, dtype=dtype)
    time = torch.arange(-half, half + 1, dtype=dtype)
    filters = []
    for c in cutoffs:
        f = 2 * c * window * ref_sinc(2 * c * math.pi * time)
        filters.append(f / f.sum())
    return torch.stack(filters), half


def ref_lowpass(x, cutoffs, zeros, dtype=torch.float64):
    """julius.LowPassFilters.forward (pad='replicate', stride 1) for one mono clip -> [K, N]."""
    filters, half = ref_lowpass_filters(cutoffs, zeros, dtype)
    xp = F.pad(torch.as_tensor(x).to(dtype).reshape(1, 1, -1), (half, half), mode="replicate")
    return F.conv1d(xp, filters[:, None])[0]


def ref_low_pass(x, cutoff_hz, rate, zeros=51, dtype=torch.float64):
    return ref_lowpass(x, [cutoff_hz / rate], zeros, dtype)[0]


def ref_high_pass(x, cutoff_hz, rate, zeros=51, dtype=torch.float64):
    return torch.as_tensor(x).to(dtype).reshape(-1) - ref_low_pass(x, cutoff_hz, rate, zeros, dtype)


def ref_mel_cutoffs(rate, n_bands):
    """julius.bands.mel_frequencies(n_bands + 1, 0, rate / 2)[1:-1], in Hz."""
    hz_to_mel = lambda f: 2595 * math.log10(1 + f / 700)
    mels = torch.linspace(hz_to_mel(0.0), hz_to_mel(rate / 2), n_bands + 1, dtype=torch.float64)
    return [float(v) for v in (700 * (10 ** (mels / 2595) - 1))[1:-1]]


def ref_split_bands(x, rate, n_bands, dtype=torch.float64):
    """julius.SplitBands.forward -> [n_bands, N]."""
    lows = ref_lowpass(x, [f / rate for f in ref_mel_cutoffs(rate, n_bands)], 8, dtype)
    low, bands = lows[0], [lows[0]]
    for low_and_band in lows[1:]:
        bands.append(low_and_band - low)
        low = low_and_band
    bands.append(torch.as_tensor(x).to(dtype).reshape(-1) - low)
    return torch.stack(bands)


def ref_equalizer(x, db, rate, dtype=torch.float64):
    """effects.py:418-431: fbank * 10**db, summed over the bands."""
    db = torch.as_tensor(db, dtype=torch.float64)
    fbank = ref_split_bands(x, rate, db.numel(), dtype)
    return (fbank * (10 ** db).to(dtype)[:, None]).sum(0)


def ref_quantile(v, n, r):
    """v[lo] + (v[hi] - v[lo]) w over the ascending float64 order statistics v, ranks from the module."""
    lo, hi, w = CH.quantile_ranks(n, r)
    return v[lo] + (v[hi] - v[lo]) * w


def ref_clip(x, q):
    """effects.py:451-459 for one clip in float64 (ranks in float64) -> (lo, hi, clamped)."""
    x = torch.as_tensor(x).double().reshape(-1)
    v = torch.sort(x).values
    lo, hi = ref_quantile(v, x.numel(), q / 2), ref_quantile(v, x.numel(), 1 - q / 2)
    return lo, hi, x.clamp(lo, hi)


def ref_quantization(x, Q, dtype=torch.float64):
    """effects.py:481-486 -> (quantized, the value before floor)."""
    x = torch.as_tensor(x).to(dtype)
    pre = (x + 1) / 2 * Q
    return 2 * (pre.floor() / Q) - 1, pre


def ref_mulaw(x, Q, dtype=torch.float64):
    """effects.py:508-519 -> (quantized, the value before truncation)."""
    x = torch.as_tensor(x).to(dtype)
    mu = torch.tensor(Q - 1.0, dtype=dtype)
    y = torch.sign(x) * torch.log1p(mu * torch.abs(x)) / torch.log1p(mu)
    pre = (y + 1) / 2 * mu + 0.5
    z = (pre.to(torch.int64) / mu) * 2 - 1.0
    return torch.sign(z) * (torch.exp(torch.abs(z) * torch.log1p(mu)) - 1.0) / mu, pre


def rel_err(a, b):
    a, b = torch.as_tensor(a).double().reshape(-1), torch.as_tensor(b).double().reshape(-1)
    return float((a - b).abs().max() / b.abs().max())


def clip(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    return 0.2 * torch.randn(n, generator=g, dtype=torch.float64) * (1.0 + 0.5 * torch.sin(2 * np.pi * t / 700.0))


def host_filter(x, taps):
    """y[n] = sum_t taps[t + half] x[clamp(n + t)] in float64 on the host, literally."""
    x, taps = np.asarray(x, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    half = (taps.size - 1) // 2
    return np.correlate(np.pad(x, half, mode="edge"), taps, mode="valid")


# ------------------------------------------------------------------------------------------------ the tap designer
def test_half_sizes_and_cutoffs():
    assert CH.half_size(4000, 24000) == 153 and CH.lowpass_taps(4000, 24000).shape == (307,)
    assert CH.half_size(100, 24000) == 6120 and CH.highpass_taps(100, 24000).shape == (12241,)
    assert CH.half_size(8000, 24000, 8) == 12 and CH.lowpass_taps(8000, 24000, zeros=8).shape == (25,)
    fc = CH.band_cutoffs(24000, 6)
    assert fc.shape == (5,) and abs(fc[0] - 434.7) < 0.1 and np.all(np.diff(fc) > 0) and fc[-1] < 12000
    assert np.allclose(fc, ref_mel_cutoffs(24000, 6), rtol=1e-12)
    assert CH.band_taps(24000, 6).shape == (6, 2 * CH.half_size(fc, 24000, 8) + 1)
    assert CH.band_taps(24000, 6) is CH.band_taps(24000, 6)              # cached


@pytest.mark.parametrize("rate,cutoffs,zeros", [(24000, [4000.0], 51), (24000, [100.0], 51), (16000, [8000.0], 8), (24000, [300.0, 3400.0, 7000.0], 8)])
def test_lowpass_taps_are_the_restatement_and_sum_to_one(rate, cutoffs, zeros):
    mine = CH.lowpass_taps(cutoffs, rate, zeros)
    ref, half = ref_lowpass_filters([f / rate for f in cutoffs], zeros)
    assert mine.shape == tuple(ref.shape) and mine.shape[1] == 2 * half + 1
    assert np.abs(mine - ref.numpy()).max() < 1e-15
    assert np.abs(mine.sum(axis=1) - 1.0).max() < 1e-14
    assert mine[0, 0] == 0.0 or abs(mine[0, 0]) < 1e-20                   # the symmetric window ends in 0
    assert np.abs(mine - mine[:, ::-1]).max() < 1e-15                     # symmetric up to the cosine's rounding
    hp = CH.highpass_taps(cutoffs, rate, zeros)
    assert np.abs(hp + mine - np.eye(1, mine.shape[1], half)).max() < 1e-15
    one = CH.lowpass_taps(cutoffs[0], rate, zeros)                        # a scalar: one tap set, designed from its own cutoff
    assert one.ndim == 1 and one.size == 2 * CH.half_size(cutoffs[0], rate, zeros) + 1


def test_filters_match_the_restatement_and_keep_their_invariants():
    rate = 24000
    for n, seed in ((1000, 1), (37, 2)):                 # the second: margins longer than the clip
        x = clip(n, seed)
        lo = host_filter(x, CH.lowpass_taps(4000, rate))
        hi = host_filter(x, CH.highpass_taps(4000, rate))
        assert rel_err(lo, ref_low_pass(x, 4000, rate)) < 1e-12 and rel_err(hi, ref_high_pass(x, 4000, rate)) < 1e-12
        assert np.abs(lo + hi - x.numpy()).max() < 1e-12                  # low_pass + high_pass == x
        const = np.full(n, 0.37)
        assert np.abs(host_filter(const, CH.lowpass_taps(4000, rate)) - 0.37).max() < 1e-14      # the edge rule
        assert np.abs(host_filter(const, CH.highpass_taps(4000, rate))).max() < 1e-14
        for nb in (3, 6):
            bank = CH.band_taps(rate, nb)
            bands = np.stack([host_filter(x, bank[k]) for k in range(nb)])
            assert rel_err(bands, ref_split_bands(x, rate, nb)) < 1e-12
            assert np.abs(bands.sum(0) - x.numpy()).max() < 1e-12         # the bands sum to x
            db = -np.linspace(0.0, 1.0, nb)
            assert rel_err(host_filter(x, CH.equalizer_taps(rate, db)), ref_equalizer(x, db, rate)) < 1e-12
            flat = CH.equalizer_taps(rate, np.zeros(nb))
            assert np.abs(flat - np.eye(1, flat.size, flat.size // 2)[0]).max() < 1e-12
            assert np.abs(host_filter(x, flat) - x.numpy()).max() < 1e-12 and rel_err(ref_equalizer(x, np.zeros(nb), rate), x) < 1e-12
    both = CH.equalizer_taps(rate, np.array([[-0.5, -1.0, 0.0], [-0.2, 0.0, -0.7]]))
    assert both.shape == (2, CH.band_taps(rate, 3).shape[1]) and np.array_equal(both[1], CH.equalizer_taps(rate, [-0.2, 0.0, -0.7]))
    assert abs(both[0].sum() - 10.0 ** -0.5) < 1e-12                      # DC sees the first band alone, times 10**db (sic), not 10**(db / 20)


# ------------------------------------------------------------------------------------------------ quantile, quantizers
def test_quantile_ranks_agree_with_torch_quantile():
    for n, seed in ((1, 3), (2, 4), (1000, 5), (4099, 6)):
        x = clip(n, seed)
        v = torch.sort(x).values
        for r in (0.0, 0.05, 0.5, 0.95, 1.0, 1.0 / 3.0):
            lo, hi, w = CH.quantile_ranks(n, r)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= w < 1.0
            assert abs(float(ref_quantile(v, n, r)) - float(torch.quantile(x, r))) <= 1e-15
    assert CH.clip_ranks(1000, 0.1) == ([49, 50, 949, 950], [CH.quantile_ranks(1000, 0.05)[2], CH.quantile_ranks(1000, 0.95)[2]])
    assert CH.clip_ranks(1000, 0.0)[0] == [0, 0, 999, 999] and CH.clip_ranks(1001, 1.0) == ([500, 500, 500, 500], [0.0, 0.0])
    lo, hi, y = ref_clip(clip(1000, 5), 0.1)
    assert lo < 0 < hi and float(y.min()) == float(lo) and float(y.max()) == float(hi)


def test_host_quantizers_are_the_restatement():
    x = clip(4099, 11).float()
    for Q in (8, 256, 65536):
        assert np.array_equal(CH.quantization_host(x.numpy(), Q), ref_quantization(x, Q)[0].numpy())
        out, pre = CH.mulaw_host(x.numpy(), Q, codes=True)
        want, wpre = ref_mulaw(x, Q)
        assert np.abs(out - want.numpy()).max() <= 1e-15 and np.abs(pre - wpre.numpy()).max() <= 1e-9
        levels = np.unique(CH.quantization_host(x.numpy(), Q))
        assert np.all(np.abs((levels + 1) / 2 * Q - np.round((levels + 1) / 2 * Q)) < 1e-9)       # on the grid k * 2 / Q - 1


# ------------------------------------------------------------------------------------------------ refusals, wiring
def test_refusals():
    assert CH.refusal([1000], 24000, cutoffs=[4000.0]) is None and CH.refusal([1000], 24000, cutoffs=[12000.0]) is None
    assert CH.refusal([5], 24000, cutoffs=[100.0]) is None                 # a margin longer than the clip is fine
    assert "cutoff" in CH.refusal([1000], 24000, cutoffs=[0.0]) and "cutoff" in CH.refusal([1000], 24000, cutoffs=[12000.5])
    assert "cutoff" in CH.refusal([1000], 24000, cutoffs=[4000.0, -1.0])
    assert "taps" in CH.refusal([1000], 24000, cutoffs=[10.0])              # 2 * 61200 + 1 taps
    assert 2 * CH.half_size(10.0, 24000) + 1 > D.MAX_TAPS
    assert CH.refusal([1000], 24000, n_bands=2) is None and "bands" in CH.refusal([1000], 24000, n_bands=1)
    assert CH.refusal([1000], q=[0.0, 1.0]) is None and "percentile" in CH.refusal([1000], q=1.5)
    assert "percentile" in CH.refusal([1000], q=-0.1) and "percentile" in CH.refusal([1000], q=float("nan"))
    assert CH.refusal([1000], channels=[2, 65536]) is None and "channels" in CH.refusal([1000], channels=1)
    assert "channels" in CH.refusal([1000], channels=[256, 0])
    assert "empty clip" in CH.refusal([5, 0]) and "empty clip" in CH.refusal([])
    x = torch.randn(100)
    for call in (lambda: CH.low_pass(x, 4000, 24000), lambda: CH.high_pass([x], 100, 24000), lambda: CH.equalizer(x, [0.0, -1.0], 24000),
                 lambda: CH.mel_filterbank(x, 4, 24000), lambda: CH.clip_distortion(x, 0.1), lambda: CH.clip_thresholds(x, 0.1),
                 lambda: CH.quantization(x, 256), lambda: CH.mulaw_quantization(x, 256), lambda: CH.order_statistics(x[None], [[0]]),
                 lambda: CH.LowPass(24000)(x, 4000), lambda: CH.MuLawQuantization()(x, 256),
                 lambda: D.apply_ir(x, x[:10], 24000, ir_eq=[0.0, -1.0]), lambda: D.mix(x, x, 24000, noise_eq=[0.0, -1.0])):
        with pytest.raises(_lib.MmxError, match="no CPU fallback"):
            call()


def test_entry_points_are_declared_bound_and_documented():
    hdr = open(os.path.join(ROOT, "include", "mmx_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for s in ("mmx_pad_edge_rows", "mmx_row_select", "mmx_clip_rows", "mmx_quantize_rows"):
        assert s in _lib.SYMBOLS and re.search(r"\bint\s+" + s + r"\s*\(", hdr) and f"`{s}`" in doc and hasattr(lib, s)
    assert _lib.ABI_VERSION == 10
    assert "channel.hip" in open(os.path.join(ROOT, "minimax-speech_amd", "csrc", "Makefile")).read()
    assert f"{len(_lib.SYMBOLS)} entry points" in open(os.path.join(ROOT, "README.md")).read()
    gate = open(os.path.join(ROOT, "tools", "check_resources.py")).read()
    for k in ("pad_edge_kernel", "row_select_kernel", "clip_rows_kernel", "quantize_rows_kernel"):
        assert f'"{k}"' in gate
    src = open(os.path.join(ROOT, "minimax-speech_amd", "csrc", "channel.hip")).read()
    for name, v in (("SEL_SPAN", CH.SELECT_SPAN), ("SEL_RANKS", CH.SELECT_RANKS)):
        assert re.search(r"\b" + name + r" = " + str(v) + r"\b", src), name
    assert CH.SELECT_WORK == 4 * 256 + 8 and "SEL_WORK = SEL_PASSES * SEL_BINS + 8" in src
    assert "restated, not compared against julius" in CH.__doc__.lower() and "10**db" in CH.__doc__
    for fn, name in ((D.apply_ir, "ir_eq"), (D.mix, "noise_eq")):
        assert inspect.signature(fn).parameters[name].default is None
    assert "needs julius" not in D.__doc__
    from mmx.pipeline import TtsEngine
    for key in ("ir_eq", "noise_eq", "low_pass", "high_pass", "eq", "clip", "quantize", "mulaw"):
        assert f"`{key}`" in TtsEngine._degrade.__doc__
