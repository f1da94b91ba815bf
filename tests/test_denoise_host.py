"""Spectral-gate noise reduction (mmx/denoise.py, csrc/denoise.hip), host side: a float64 restatement of the reference's SpectralGate
written from its definition - torch.stft / conv2d / torch.istft; it knows nothing of tiles, planes or tables - the seeded fixtures it
shares with tests/test_gpu_denoise.py with the conditions the device test leans on, and the host logic: taps, frame counts, tables,
refusals, the LDS budget.  No GPU.

Fixtures are synthetic: a noise-only lead-in of a quarter of the clip, then 24 harmonics of a gliding 120 Hz tone under a 1.7 Hz
envelope (peak 0.2), all under white noise of 0.01 rms (-40 dBFS); noise clips are that noise alone.  A noise clip of
exactly 2 frames, the unbiased std's smallest case, does not exist: 1 + len // hop = 2 needs len < n / 2, which the reflection by
n / 2 (torch.stft's too) refuses; the smallest legal clip, n / 2 + 1 samples, has 3 frames and stands in for it."""
import functools
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

from mmx import denoise as D
from mmx import mel as MEL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 24000
WINDOWS = (32, 128, 512, 2048)      # the smallest window: one K step; 65 bins: a last bin tile of padding; two K chunks; the default
LONG = {32: 400, 128: 1500, 512: 9000, 2048: 24000}
# seeds of the batch members and of the lead-in clip, chosen so that EVERY fixture meets the conditions asserted below on its own
SEEDS = {32: (1, 0, 0, 0, 1), 128: (1, 0, 2, 0, 0), 512: (9, 2, 8, 0, 1), 2048: (0, 0, 0, 0, 0)}
LEAD_SEED = {32: 2, 128: 1, 512: 0, 2048: 0}
NEAR_DB = 0.05                                           # the widest band in which the device's decision may differ (test_gpu_denoise)


def lengths(n):
    """The ragged batch of one window: the shortest legal clip (3 frames), 15 / 16 / 17 frames (a frame-tile boundary), a long one."""
    hop = n // 4
    return (n // 2 + 1, 14 * hop + 3, 15 * hop, 16 * hop + hop - 1, LONG[n])


def noise_lengths(n):
    """The smallest legal noise clip (3 frames: the unbiased std's smallest case that exists) and one of 13 frames."""
    return (n // 2 + 1, 12 * (n // 4) + 5)


# ------------------------------------------------------------------------------------------------ fixtures (seeded, read-only)
@functools.lru_cache(None)
def clip(n_samples, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    t = torch.arange(n_samples, dtype=torch.float64) / RATE
    phase = 2 * math.pi * (120.0 * t + 15.0 * t * t)      # 120 Hz gliding up by 30 Hz per second
    voiced = sum(torch.sin(h * phase) / h for h in range(1, 25)) * (0.5 + 0.5 * torch.sin(2 * math.pi * 1.7 * t))
    voiced[:n_samples // 4] = 0.0
    voiced = voiced * (0.2 / float(voiced.abs().max()))
    x = (voiced + 0.01 * torch.randn(n_samples, generator=g, dtype=torch.float64)).float()
    return x.requires_grad_(False)


@functools.lru_cache(None)
def noise_clip(n_samples, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return (0.01 * torch.randn(n_samples, generator=g, dtype=torch.float64)).float().requires_grad_(False)


def lead_clip(n):
    """The long clip whose own lead-in (its first quarter) is the noise reference."""
    return clip(LONG[n], LEAD_SEED[n])


def noise_clips(n):
    """The 3-frame and the 13-frame noise clip of window n."""
    return [noise_clip(v) for v in noise_lengths(n)]


def batch(n):
    """(clips, their noise clips) of window n: the 3-frame member takes the 3-frame noise clip, the others the 13-frame one.  (A
    threshold from 3 frames sits in the bulk of a bin's dB distribution, not in its tail, so near ties are about 1.5e-3 of any grid
    it gates; only the smallest grid has seeds that meet 1e-3 with it.  The threshold itself is checked on every window.)"""
    short, long = noise_clips(n)
    xs = [clip(v, SEEDS[n][i]) for i, v in enumerate(lengths(n))]
    return xs, [short if i == 0 else long for i in range(len(xs))]


# ------------------------------------------------------------------------------------------------ the restatement
def stft(x, n, dtype=torch.float64):
    return torch.stft(x.to(dtype), n, hop_length=n // 4, win_length=n, window=D.window(n).to(dtype), center=True, pad_mode="reflect",
                      return_complex=True)


def db(X):
    return 20 * X.abs().clamp(min=1e-4).log10()


def threshold_ref(noise, n, n_std=3.0, dtype=torch.float64):
    d = db(stft(noise, n, dtype))
    return d.mean(dim=-1) + n_std * d.std(dim=-1)


def reference_taps(n_freq, n_time, dtype=torch.float64):
    """spectral_gate.py:40-54, the reference's construction, in `dtype`."""
    tri = lambda p: torch.cat([torch.linspace(0, 1, p + 2, dtype=dtype)[:-1], torch.linspace(1, 0, p + 2, dtype=dtype)])[1:-1]
    f = torch.outer(tri(n_freq), tri(n_time))
    return f / f.sum()


def gate_ref(x, noise, n=2048, n_std=3.0, denoise_amount=1.0, n_freq=3, n_time=5, dtype=torch.float64, force_mask=None):
    """(waveform, margins dB - thresh [bins, frames], mask bool [bins, frames]) of SpectralGate.forward(x, noise) in `dtype`;
    force_mask: the decisions to apply in place of the restatement's own (the margins stay its own)."""
    X = stft(x, n, dtype)
    margin = db(X) - threshold_ref(noise, n, n_std, dtype)[:, None]
    m = (margin < 0) if force_mask is None else force_mask.to(torch.bool)
    sm = F.conv2d(m.to(dtype)[None, None], reference_taps(n_freq, n_time, dtype)[None, None], padding=(n_freq, n_time))[0, 0]
    Y = X * (1 - denoise_amount * sm)
    y = torch.istft(Y, n, hop_length=n // 4, win_length=n, window=D.window(n).to(dtype), center=True, length=x.numel())
    return y, margin, m


@functools.lru_cache(None)
def batch_ref(n):
    """gate_ref in float64 of every member of batch(n) with its own noise clip (computed once, shared by the tests)."""
    xs, nz = batch(n)
    return [gate_ref(x, z, n) for x, z in zip(xs, nz)]


def rms(v):
    return float(v.double().pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------ the fixtures' conditions
@pytest.mark.parametrize("n", WINDOWS)
def test_fixture_conditions(n):
    """What tests/test_gpu_denoise.py leans on, so that a bad fixture fails here: few near ties (the device may decide those either
    way), a mask that is neither empty nor full, a peak at 0.2 - for every member of every batch on its own."""
    xs, _ = batch(n)
    for x, (y, margin, m) in zip(xs, batch_ref(n)):
        near, share = int((margin.abs() < NEAR_DB).sum()), float(m.double().mean())
        print(f"n {n} len {x.numel()}: near ties {near} of {margin.numel()} ({near / margin.numel():.2e}), masked {share:.3f}, "
              f"peak {float(x.abs().max()):.3f}")
        assert near / margin.numel() <= 1e-3, (n, x.numel(), near, margin.numel())      # every fixture on its own grid
        assert 0.05 <= share <= 0.99, (n, x.numel(), share)
        assert float(x.abs().max()) <= 0.25 and tuple(y.shape) == tuple(x.shape)


@pytest.mark.parametrize("n", WINDOWS)
def test_the_gate_does_something(n):
    """The long clip gated by its own lead-in (the Audacity workflow): the lead-in's RMS falls to a quarter or less."""
    x = lead_clip(n)
    lead = x.numel() // 4
    y, margin, m = gate_ref(x, x[:lead], n)
    before, after = rms(x[:lead]), rms(y[:lead])
    print(f"n {n}: lead-in rms {before:.4f} -> {after:.4f}; near ties {float((margin.abs() < NEAR_DB).double().mean()):.2e}")
    assert abs(before - 0.01) < 1e-3 and after <= before / 4
    assert float((margin.abs() < NEAR_DB).double().mean()) <= 1e-3 and 0.05 <= float(m.double().mean()) <= 0.99
    # speech survives: the voiced part keeps more than half of its level
    assert rms(y[lead:]) >= 0.5 * rms(x[lead:])


def test_whole_clip_statistics_would_return_silence():
    """Why there is no "statistics of the clip itself" default: mean + 3 std of a clip's own dB masks nearly every bin."""
    x = clip(24000, 4)
    y, _, m = gate_ref(x, x, 2048)
    assert float(m.double().mean()) > 0.97 and rms(y) < 0.1 * rms(x)


@pytest.mark.parametrize("n", WINDOWS)
def test_fp32_restatement_agrees_with_float64(n):
    """What the reference computes (fp32 stft, conv2d, istft) against float64: the floor under any device tolerance."""
    worst, flips, worst_margin = 0.0, 0, 0.0
    xs, nz = batch(n)
    for x, z, (y, margin, m) in zip(xs, nz, batch_ref(n)):
        y32, margin32, m32 = gate_ref(x, z, n, dtype=torch.float32)
        worst = max(worst, float((y32.double() - y).abs().max()))
        flips += int((m32 != m).sum())
        worst_margin = max(worst_margin, float((margin32.double() - margin)[margin.abs() < 40].abs().max()))
    print(f"n {n}: fp32 against float64 max |dy| {worst:.2e}, mask flips {flips}, max |d margin| {worst_margin:.2e} dB")
    assert worst <= 5.1e-8 and flips == 0


# ------------------------------------------------------------------------------------------------ host logic
def test_smoothing_taps_equal_the_reference_formula():
    for nf, nt in ((3, 5), (0, 0), (1, 7), (15, 15)):
        taps = D.smoothing_taps(nf, nt)
        assert tuple(taps.shape) == (2 * nf + 1, 2 * nt + 1) and abs(float(taps.sum()) - 1.0) < 1e-15
        assert float((taps - reference_taps(nf, nt)).abs().max()) < 1e-15
    assert D.triangle(3) == [1, 2, 3, 4, 3, 2, 1] and sum(D.triangle(5)) == 36
    g = D.SpectralGate()
    assert (g.n_freq, g.n_time) == (3, 5) and tuple(g.smoothing_filter.shape) == (1, 1, 7, 11)
    assert float((g.smoothing_filter[0, 0] - reference_taps(3, 5, torch.float32)).abs().max()) < 1e-7


def test_frame_counts_match_torch_stft():
    for n in WINDOWS:
        for v in lengths(n) + noise_lengths(n):
            assert D.frames_of(v, n) == stft(torch.zeros(v), n).shape[1] == 1 + v // (n // 4)
        assert [D.frames_of(v, n) for v in lengths(n)[:4]] == [3, 15, 16, 17] and [D.frames_of(v, n) for v in noise_lengths(n)] == [3, 13]
    with pytest.raises(RuntimeError):                     # the 2-frame clip: torch refuses the reflection as the gate does
        stft(torch.zeros(2048 // 4 + 1), 2048)


def test_window_and_dft_basis_window_keyword():
    w = D.window(2048)
    assert w.dtype == torch.float32 and float(w[0]) == 0.0 and float(w[1024]) == 1.0
    assert float((w.double() ** 2 - torch.hann_window(2048, periodic=True, dtype=torch.float64)).abs().max()) < 2e-7
    # the default keeps today's Hann table bit for bit; a window given as float64 Hann reproduces it
    a = MEL.dft_basis(128, 0, 65)
    hann = 0.5 - 0.5 * torch.cos(torch.arange(128, dtype=torch.float64) * (2 * math.pi / 128))
    assert torch.equal(a, MEL.dft_basis(128, 0, 65, window=None)) and torch.equal(a, MEL.dft_basis(128, 0, 65, window=hann))
    assert not torch.equal(a, D.forward_basis(128)) and D.forward_basis(128).dtype == torch.float64


def test_inverse_of_forward_is_the_squared_window_times_the_frame():
    for n in (32, 128, 2048):
        nb, nbp = n // 2 + 1, D.padded_bins(n)
        fwd, (ire, iim) = D.forward_basis(n), D.inverse_table(n)
        assert tuple(fwd.shape) == (2 * nbp, n) and tuple(ire.shape) == tuple(iim.shape) == (n, nbp) and ire.dtype == torch.float64
        assert float(ire[:, nb:].abs().max()) == 0.0 and float(iim[:, nb:].abs().max()) == 0.0
        assert float(iim[:, 0].abs().max()) == 0.0 and float(iim[:, nb - 1].abs().max()) == 0.0
        frame = torch.randn(n, generator=torch.Generator().manual_seed(n), dtype=torch.float64)
        i = torch.arange(nb)
        rows = 32 * (i // 16) + i % 16
        re, im = fwd[rows] @ frame, -(fwd[rows + 16] @ frame)        # the basis holds +sin
        want = torch.fft.rfft(frame * D.window(n).double())
        assert float((re - want.real).abs().max()) < 1e-10 and float((im - want.imag).abs().max()) < 1e-10
        y = (ire[:, :nb] @ re + iim[:, :nb] @ im) * D.window(n).double()
        assert float((y - D.window(n).double() ** 2 * frame).abs().max()) < 1e-12
        # irfft ignores the imaginary parts of DC and Nyquist
        spec = torch.complex(re, im + 1.0)
        assert float((ire[:, :nb] @ spec.real + iim[:, :nb] @ spec.imag - torch.fft.irfft(spec, n=n)).abs().max()) < 1e-12


def test_refusals_and_lds_budget():
    for n in range(32, 2049, 32):
        assert D.lds_bytes(n) <= D.LDS_BYTES and D.lds_bytes(n, "stft") <= D.LDS_BYTES and D.refusal([RATE], n, n // 4) is None
    assert D.lds_bytes(2048) == 32 * 1056 + 3 * 32 * (32 * 17 + 8) * 2 == 139776      # 66 K steps in chunks of 17, 17, 17, 15
    assert 3 * 16 * (2 * 1056 + 8) * 2 == 203520 > D.LDS_BYTES          # all of K at once does not fit even for 16 frames: hence the chunks
    assert D.lds_bytes(128) == 32 * 96 + 3 * 32 * (32 * 6 + 8) * 2      # 6 K steps: one chunk
    assert D.lds_bytes(2048, "stft") == 3 * 2 * (17920 + 16 * 35) == 110880
    assert D.lds_bytes(4096) > D.LDS_BYTES and "LDS" in D.refusal([RATE], 4096, 1024)
    assert "above 2048" in D.refusal([RATE], 2080, 520)
    assert "win_length // 4" in D.refusal([RATE], 2048, 256) and D.refusal([RATE], 2048, None) is None
    assert "multiple of 32" in D.refusal([RATE], 48, 12) and "multiple of 32" in D.refusal([RATE], 0, 0)
    assert "reflected" in D.refusal([RATE, 1024], 2048, 512) and D.refusal([1025], 2048, 512) is None
    assert "n_time" in D.refusal([RATE], 2048, 512, 3, 15) and D.refusal([RATE], 2048, 512, 14, 14) is None


def test_a_cpu_tensor_is_refused_before_any_device_work():
    x = clip(1500)
    with pytest.raises(D.MmxError, match="no CPU fallback"):
        D.spectral_gate([x], x[:375], win_length=128, hop_length=32)
    with pytest.raises(D.MmxError, match="no CPU fallback"):
        D.gate_threshold(x[:375], win_length=128, hop_length=32)
    with pytest.raises(D.MmxError, match="no CPU fallback"):
        D.SpectralGate()(x[None], (0, 375), win_length=128, hop_length=32)


def test_entry_points_are_declared_bound_and_documented():
    from mmx import _lib
    hdr = open(os.path.join(ROOT, "include", "mmx_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in ("mmx_gate_threshold", "mmx_gate_analyze", "mmx_gate_synthesize"):
        assert s in _lib.SYMBOLS and re.search(r"\bint\s+" + s + r"\s*\(", hdr) and f"`{s}`" in doc
    assert _lib.ABI_VERSION == 10
    assert "denoise.hip" in open(os.path.join(ROOT, "minimax-speech_amd", "csrc", "Makefile")).read()
    gate = open(os.path.join(ROOT, "tools", "check_resources.py")).read()
    for k in ("gate_stft_kernel", "gate_thresh_kernel", "gate_synth_kernel", "gate_ola_kernel"):
        assert f'"{k}"' in gate
    import inspect
    from mmx.pipeline import TtsEngine
    assert inspect.signature(TtsEngine.prompt_from_clip).parameters["denoise"].default is None
    assert inspect.signature(TtsEngine.prompts_from_clips).parameters["denoise"].default is None
