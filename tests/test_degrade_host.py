"""Room and noise simulation (mmx/degrade.py, csrc/degrade.hip), the part that needs no GPU: a float64 restatement of the reference's
EffectMixin (dac-vae/audiotools/core/effects.py) - convolve lines 85-121, apply_ir lines 160-177, decompose_ir / measure_drr /
solve_alpha / alter_drr lines 540-647, mix lines 52-63 with normalize lines 214-219 - against the module's index definition and its
fp64 host path; the Toeplitz table builder; the LDS formula; refusals; and the wiring of the new entry points.

audiotools is not a dependency: the restatement works on plain float64 tensors and keeps the reference's operations and their order
(the zero padding / truncation of the IR, torch.roll over the peak, rfft / irfft of the signal's length, the delta trick)."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

from mmx import _lib
from mmx import degrade as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAIN_FACTOR = np.log(10) / 20                            # effects.py:12


# ------------------------------------------------------------------------------------------------ the restatement
def ref_convolve(x, h, start_at_max=True, dtype=torch.float64):
    """effects.py:85-121 for one mono clip x [N] and one IR h [L], literally, in `dtype`."""
    x, h = torch.as_tensor(x).to(dtype).reshape(1, 1, -1), torch.as_tensor(h).to(dtype).reshape(1, 1, -1)
    pad_len = x.shape[-1] - h.shape[-1]                  # :85
    if pad_len > 0:
        h = torch.nn.functional.pad(h, (0, pad_len))     # :88 zero_pad(0, pad_len)
    else:
        h = h[..., :x.shape[-1]]                         # :90 truncate_samples
    if start_at_max:
        idx = h.abs().argmax(axis=-1)                    # :96
        irs = torch.zeros_like(h)
        for i in range(h.shape[0]):
            irs[i] = torch.roll(h[i], -idx[i].item(), -1)   # :99
        h = irs
    delta = torch.zeros_like(h)
    delta[..., 0] = 1                                    # :102-103
    length = x.shape[-1]                                 # :105
    delta_fft = torch.fft.rfft(delta, length)
    other_fft = torch.fft.rfft(h, length)
    self_fft = torch.fft.rfft(x, length)
    convolved_audio = torch.fft.irfft(other_fft * self_fft, length)          # :110-111
    delta_audio = torch.fft.irfft(other_fft * delta_fft, length)             # :113-114
    delta_max = delta_audio.abs().max(dim=-1, keepdims=True)[0]              # :117
    scale = 1 / delta_max.clamp(1e-5)                    # :118
    return (convolved_audio * scale).reshape(-1)         # :119


def ref_decompose_ir(h, rate):
    """effects.py:540-574 for one IR [L] in float64 -> (early_response, late_field, window)."""
    h = torch.as_tensor(h).double().reshape(-1)
    td = int(torch.argmax(h))                            # :549
    t0 = int(rate * 0.0025)                              # :550
    idx = torch.arange(h.numel())
    early_idx = (idx >= td - t0) * (idx <= td + t0)      # :554
    early = torch.zeros_like(h)
    early[early_idx] = h[early_idx]
    late = torch.zeros_like(h)
    late[~early_idx] = h[~early_idx]
    window = torch.zeros_like(h)
    count = int(early_idx.sum())
    # :571 get_window("hann", count) = scipy.signal.get_window: periodic (fftbins=True)
    window[early_idx] = 0.5 - 0.5 * torch.cos(2 * math.pi * torch.arange(count, dtype=torch.float64) / count)
    return early, late, window


def ref_measure_drr(h, rate):
    early, late, _ = ref_decompose_ir(h, rate)           # :585-589
    return float(10 * torch.log10((early ** 2).sum() / (late ** 2).sum()))


def ref_alter_drr(h, rate, drr, detail=False):
    """effects.py:591-647 (solve_alpha, the floor, the recombination, ensure_max_of_audio lines 194-197) in float64."""
    early, late, wd = ref_decompose_ir(h, rate)
    e_sq, l_sq = early ** 2, late ** 2
    a = (wd ** 2 * e_sq).sum()                           # :604
    b = (2 * (1 - wd) * wd * e_sq).sum()                 # :605
    c = ((1 - wd) ** 2 * e_sq).sum() - torch.pow(torch.tensor(10.0, dtype=torch.float64), drr / 10) * l_sq.sum()      # :606
    expr = ((b ** 2) - 4 * a * c).sqrt()                 # :610
    alpha = torch.maximum((-b - expr) / (2 * a), (-b + expr) / (2 * a))      # :611-614
    min_alpha = late.abs().max() / early.abs().max()     # :635-637
    floored = bool(min_alpha > alpha)
    alpha = torch.maximum(alpha, min_alpha)              # :638
    out = alpha * wd * early + (1 - wd) * early + late   # :640-644
    peak = out.abs().max()                               # :194-197
    if peak > 1.0:
        out = out * (1.0 / peak)
    return (out, float(alpha), floored) if detail else out


def ref_apply_ir(x, h, rate, drr=None, dtype=torch.float64):
    """effects.py:157-177 without ir_eq and use_original_phase."""
    if drr is not None:
        h = ref_alter_drr(h, rate, drr)
    x = torch.as_tensor(x).to(dtype).reshape(-1)
    max_spk = x.abs().max()                              # :161
    y = ref_convolve(x, h, dtype=dtype)                  # :166
    max_transformed = y.abs().max()                      # :175
    return y * (max_spk.clamp(1e-8) / max_transformed.clamp(1e-8))          # :176-177


def ref_fit_noise(noise, n):
    """effects.py:54-56: zero_pad(0, max(0, n - len)) then truncate_samples(n)."""
    noise = torch.as_tensor(noise).double().reshape(-1)
    return torch.nn.functional.pad(noise, (0, max(0, n - noise.numel())))[:n]


def ref_mix(x, noise, snr, loud_x, loud_n):
    """effects.py:52-63 with normalize (lines 214-219); the two loudness values (of x and of the fitted noise) are given."""
    x = torch.as_tensor(x).double().reshape(-1)
    other = ref_fit_noise(noise, x.numel())
    tgt_loudness = loud_x - snr                          # :60
    gain = math.exp((tgt_loudness - loud_n) * GAIN_FACTOR)                   # :216-217
    return x + other * gain                              # :63, :219


def make_ir(rate, L, peak, seed=0):
    """Decaying noise (exp(-0.75 t / L)) x 0.3, pre-peak samples x 0.05, peak 1.0."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64)
    h = torch.randn(L, generator=g, dtype=torch.float64) * torch.exp(-0.75 * t / L) * 0.3
    h[:peak] *= 0.05
    h[peak] = 1.0
    return h


def rel_err(y, ref):
    y, ref = torch.as_tensor(y).double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    return float((y - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("start_at_max", [True, False])
@pytest.mark.parametrize("N,L", [(500, 77), (300, 300), (200, 450), (257, 1)])
def test_index_definition_equals_the_reference_fft_route(N, L, start_at_max):
    g = torch.Generator().manual_seed(N + L)
    x = torch.randn(N, generator=g, dtype=torch.float64)
    h = torch.randn(L, generator=g, dtype=torch.float64) * torch.exp(-torch.arange(L, dtype=torch.float64) / max(L / 4, 1))
    ref = ref_convolve(x, h, start_at_max)
    got = D.convolve_host(x.numpy(), h.numpy(), start_at_max=start_at_max, wrap=True)
    assert rel_err(got, ref) < 1e-12
    taps, p, s = D.prepare_host(h.numpy(), N, start_at_max)
    assert taps == min(L, N) and (p == int(h[:taps].abs().argmax()) if start_at_max else p == 0)
    assert s == 1.0 / max(float(h[:taps].abs().max()), 1e-5)


def test_wrap_false_is_the_causal_part():
    """wrap=False: the same sum with zeros outside the clip; where no tap reaches outside, both agree exactly."""
    g = torch.Generator().manual_seed(5)
    x, h = torch.randn(120, generator=g, dtype=torch.float64).numpy(), torch.randn(9, generator=g, dtype=torch.float64).numpy()
    h[3] = 4.0
    a, b = D.convolve_host(x, h, wrap=True), D.convolve_host(x, h, wrap=False)
    assert np.array_equal(a[5:117], b[5:117]) and not np.allclose(a[:5], b[:5])
    direct = np.convolve(x, h)[3:123] / 4.0              # y[n] = s * sum h[t] x[n + 3 - t]
    assert np.abs(direct - b).max() < 1e-13


@pytest.mark.parametrize("taps,kcap", [(1, None), (31, None), (33, 96), (300, None)])
def test_toeplitz_table_unpacks_to_g(taps, kcap):
    h = torch.randn(taps + 5, generator=torch.Generator().manual_seed(taps)).numpy()     # fp32 taps; 5 beyond L' never enter
    tab = D.pack_table(h, taps, kcap)
    kp = D.padded_taps(taps)
    assert kp % 32 == 0 and kp >= taps + 15 and tab.dtype == torch.bfloat16 and tab.shape == (3, (kcap or kp) // 32, 64, 8)
    got = D.unpack_table(tab)
    want = np.zeros_like(got)
    for j in range(16):
        for u in range(got.shape[1]):
            v = u - j
            if 0 <= v < taps:
                want[j, u] = float(h[taps - 1 - v])      # g[u - j], g[v] = h[L' - 1 - v]
    assert np.array_equal(got.astype(np.float32), want.astype(np.float32))   # three bf16 terms hold an fp32 value exactly
    assert not got[:, taps + 15:].any()                 # the K padding
    assert np.array_equal(D.toeplitz(h, taps), want[:, :kp])


@pytest.mark.parametrize("rate,L,peak", [(16000, 2000, 40), (24000, 5000, 137)])
@pytest.mark.parametrize("target", [0.0, 10.0, 20.0])
def test_alter_drr_reaches_the_target(rate, L, peak, target):
    h = make_ir(rate, L, peak)
    out, alpha, floored = ref_alter_drr(h, rate, target, detail=True)
    assert math.isfinite(alpha) and not floored         # a real alpha above its floor
    assert abs(ref_measure_drr(out, rate) - target) < 1e-3
    mine = D.alter_drr_host(h.numpy(), rate, target)
    assert rel_err(mine, out) < 1e-12
    assert abs(D.measure_drr_host(mine, rate) - target) < 1e-3
    assert abs(D.measure_drr_host(h.numpy(), rate) - ref_measure_drr(h, rate)) < 1e-9


def test_alter_drr_floor_engages():
    """(16000, 300, 25) with target -5 dB: alpha is floored at max|late| / max|early| and the result is not -5 dB (-4.26 with this IR)."""
    rate, h = 16000, make_ir(16000, 300, 25)
    out, alpha, floored = ref_alter_drr(h, rate, -5.0, detail=True)
    got = ref_measure_drr(out, rate)
    assert floored and abs(got + 5.0) > 0.1 and abs(got + 4.2625) < 1e-3
    mine = D.alter_drr_host(h.numpy(), rate, -5.0)
    assert rel_err(mine, out) < 1e-12 and abs(D.measure_drr_host(mine, rate) - got) < 1e-9


def test_alter_drr_negative_discriminant_is_nan():
    """A target far above what the early window can give has no real root: NaN, as the reference's sqrt gives (documented)."""
    h = make_ir(16000, 2000, 40)
    assert torch.isnan(ref_alter_drr(h, 16000, -60.0)).all() and np.isnan(D.alter_drr_host(h.numpy(), 16000, -60.0)).all()


def test_hann_windows_are_periodic():
    W = D.hann_windows(40)
    assert W.shape == (81, 81) and W[0, 0] == 0.0 and not W[4, 5:].any()
    for c in (1, 2, 41, 81):
        assert np.allclose(W[c - 1, :c], 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(c) / c), atol=1e-16)


def test_lds_bytes_under_the_budget_for_every_chunk_form():
    forms = [1, 17, 18, 31, 33, D.CHUNK_TAPS - 15, D.CHUNK_TAPS - 14, D.CHUNK_TAPS, D.CHUNK_TAPS + 17, 24000, 48000, D.MAX_TAPS]
    for taps in forms:
        n = D.lds_bytes(taps)
        assert n == 6 * (D.NOUT - 16 + min(D.CHUNK_TAPS, D.padded_taps(taps))) and n <= D.LDS_BYTES
    assert D.lds_bytes(D.MAX_TAPS) == D.lds_bytes(D.CHUNK_TAPS) == 6 * (D.NOUT - 16 + D.CHUNK_TAPS)
    assert D.NOUT == D.WAVES * D.ROW_TILES * 256 and D.CHUNK_TAPS % 32 == 0
    src = open(os.path.join(ROOT, "minimax-speech_amd", "csrc", "degrade.hip")).read()
    for name, v in (("FIR_WAVES", D.WAVES), ("FIR_RT", D.ROW_TILES), ("FIR_CHUNK", D.CHUNK_TAPS), ("FIR_MAX_TAPS", D.MAX_TAPS)):
        assert re.search(r"\b" + name + r" = " + str(v) + r"\b", src), name


def test_refusals():
    assert D.refusal([1000], [77]) is None and D.refusal([100000, 90000], [D.MAX_TAPS]) is None
    assert "taps" in D.refusal([100000], [D.MAX_TAPS + 1])
    assert D.refusal([D.MAX_TAPS], [D.MAX_TAPS + 1]) is None         # an IR longer than the clip is truncated first
    assert "empty clip" in D.refusal([5, 0], [3]) and "empty impulse" in D.refusal([5], [0])
    assert D.refusal([5, 6, 7], [3, 3]) is not None
    x, h = torch.randn(100), torch.randn(10)
    for call in (lambda: D.convolve([x], h), lambda: D.apply_ir(x, h, 16000), lambda: D.mix([x], [x], 16000),
                 lambda: D.alter_drr([h], 16000, 3.0), lambda: D.measure_drr(h, 16000), lambda: D.row_absmax(x[None])):
        with pytest.raises(_lib.MmxError, match="no CPU fallback"):
            call()


def test_entry_points_are_declared_bound_and_documented():
    hdr = open(os.path.join(ROOT, "include", "mmx_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _lib.load()
    for s in ("mmx_ir_prepare", "mmx_fir_rows", "mmx_row_absmax", "mmx_mix_rows"):
        assert s in _lib.SYMBOLS and re.search(r"\bint\s+" + s + r"\s*\(", hdr) and f"`{s}`" in doc and hasattr(lib, s)
    assert _lib.ABI_VERSION == 10
    assert "degrade.hip" in open(os.path.join(ROOT, "minimax-speech_amd", "csrc", "Makefile")).read()
    gate = open(os.path.join(ROOT, "tools", "check_resources.py")).read()
    for k in ("ir_prepare_kernel", "ir_table_kernel", "fir_rows_kernel", "row_absmax_kernel", "mix_rows_kernel"):
        assert f'"{k}"' in gate
    from mmx.pipeline import TtsEngine
    for fn in (TtsEngine.prompt_from_clip, TtsEngine.prompts_from_clips):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "degrade" and params["degrade"].default is None
    for name in ("ir_eq", "use_original_phase", "Multi-channel", "looping"):
        assert name.lower() in D.__doc__.lower()
