"""Audio distances (mmx/metrics.py, dac-vae/loss.py), host side: a float64 yardstick written from the definitions - torch.stft in
float64, the filterbank, plain means; it knows nothing of tiles or planes - the fixtures it shares with tests/test_gpu_metrics.py,
and the host logic: frame counts, table shapes, the refusals, the drop-in classes' arguments.  No GPU."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from mmx import metrics as M
from mmx.mel import mel_filterbank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 24000
EDGE_LENGTHS = (1025, 4095, 4096, 4097, 20000)           # shortest legal at 2048; a frame-count boundary; 40 frames at hop 512: 2.5 tiles


# ------------------------------------------------------------------------------------------------ fixtures (seeded, read-only)
@functools.lru_cache(None)
def clips():
    g = torch.Generator().manual_seed(20)
    t = torch.arange(RATE, dtype=torch.float64) / RATE
    ref = 0.3 * torch.sin(2 * math.pi * 220.0 * t) * (1.0 + 0.5 * torch.sin(2 * math.pi * 3.0 * t))
    ref = (ref + 0.05 * torch.randn(RATE, generator=g, dtype=torch.float64)).float()
    codec = (ref.double() + 3e-3 * torch.randn(RATE, generator=g, dtype=torch.float64)).float()
    codec[:2000] = 0.0
    near = (ref.double() + 1e-5 * torch.randn(RATE, generator=g, dtype=torch.float64)).float()
    out = dict(ref=ref, codec=codec, half=0.5 * ref, near=near, silent=torch.zeros(RATE))
    for v in out.values():
        v.requires_grad_(False)
    return out


def clip(name):
    return clips()[name]


# ------------------------------------------------------------------------------------------------ the yardstick
def spectrum(x, n_fft, dtype=torch.float64):
    win = torch.hann_window(n_fft, periodic=True, dtype=dtype)
    return torch.stft(x.to(dtype), n_fft, hop_length=n_fft // 4, window=win, center=True, pad_mode="reflect", return_complex=True).abs()


def spec_ref(x, y, n_fft, n_mels=0, pow=1.0, eps=1e-5, fmin=0.0, fmax=None, dtype=torch.float64):
    """(d_log, d_mag) of one scale, as python floats."""
    a, b = spectrum(x, n_fft, dtype), spectrum(y, n_fft, dtype)
    if n_mels:
        fb = torch.from_numpy(mel_filterbank(RATE, n_fft, n_mels, fmin, fmax)).to(dtype)
        a, b = fb @ a, fb @ b
    d_log = (a.clamp(min=eps).pow(pow).log10() - b.clamp(min=eps).pow(pow).log10()).abs().mean()
    return float(d_log), float((a - b).abs().mean())


@functools.lru_cache(None)
def mel_ref(xn, yn, n=RATE, dtype=torch.float64):
    """MelSpectrogramLoss with train.py's settings on the first n samples of two fixtures."""
    return sum(spec_ref(clip(xn)[:n], clip(yn)[:n], w, m, dtype=dtype)[0] for w, m in zip(M.MEL_WINDOWS, M.MEL_N_MELS))


@functools.lru_cache(None)
def stft_ref(xn, yn, n=RATE, windows=M.VALIDATION_STFT_WINDOWS, dtype=torch.float64):
    """MultiScaleSTFTLoss (pow 2, both weights 1)."""
    return sum(sum(spec_ref(clip(xn)[:n], clip(yn)[:n], w, 0, pow=2.0, dtype=dtype)) for w in windows)


def wave_ref(x, y, clipv=None):
    """l1, mse, snr_db, sisdr_db in float64 numpy, two-pass, from the definitions."""
    x, y = x.double().numpy(), y.double().numpy()
    if clipv is not None:
        x = np.clip(x, -clipv, clipv)
    mse = np.mean((x - y) ** 2)
    x0, y0 = x - x.mean(), y - y.mean()
    alpha = ((x0 * y0).sum() + 1e-8) / ((y0 ** 2).sum() + 1e-8)
    sisdr = 10 * np.log10(((alpha * y0) ** 2).sum() / ((x0 - alpha * y0) ** 2).sum() + 1e-8)
    return dict(l1=np.mean(np.abs(x - y)), mse=mse, snr_db=10 * np.log10(np.var(y) / (mse + 1e-10)), sisdr_db=sisdr)


def sums_np(x, y):
    x, y = x.double().numpy(), y.double().numpy()
    d = x - y
    return np.array([x.sum(), y.sum(), (x * x).sum(), (y * y).sum(), (x * y).sum(), np.abs(d).sum(), (d * d).sum()])


# ------------------------------------------------------------------------------------------------ the yardstick itself
def test_half_amplitude_has_the_analytic_mel_distance():
    """0.5 x scales every mel value by 0.5, so each of the seven scales contributes log10 2 as long as no value is at the clamp:
    the noise floor of `ref` keeps every mel value above 1e-5, and this result confirms it."""
    assert abs(mel_ref("half", "ref") - 7 * math.log10(2.0)) < 1e-12
    assert abs(7 * math.log10(2.0) - 2.10721) < 1e-5
    for w, m in zip(M.MEL_WINDOWS, M.MEL_N_MELS):
        fb = torch.from_numpy(mel_filterbank(RATE, w, m)).double()
        assert float((fb @ spectrum(clip("half"), w)).min()) > 1e-5


def test_fp32_restatement_agrees_with_float64():
    """What the reference computes (fp32 torch.stft, fp32 matmul) against the float64 yardstick: fp32's own error, a few 1e-7
    relative per magnitude and averaged over thousands of terms, is far below the 1e-4 the device is held to, so the device
    tolerance cannot be derived from it (tests/test_gpu_metrics.py states where it comes from)."""
    for xn in ("codec", "half"):
        a, b = mel_ref(xn, "ref"), mel_ref(xn, "ref", dtype=torch.float32)
        assert abs(a - b) <= 1e-5 * a, (xn, a, b)
        a, b = stft_ref(xn, "ref"), stft_ref(xn, "ref", dtype=torch.float32)
        assert abs(a - b) <= 1e-5 * a, (xn, a, b)


def test_fixture_distances_are_where_the_tolerances_assume():
    assert mel_ref("codec", "ref") >= 0.1 and stft_ref("codec", "ref") >= 0.1 and stft_ref("half", "ref") >= 0.1
    assert 1e-4 < mel_ref("near", "ref") < 1e-3 and 1e-4 < stft_ref("near", "ref") < 2e-3
    assert abs(wave_ref(clip("near"), clip("ref"))["sisdr_db"] - 87.27) < 0.2


def test_one_pass_sums_give_the_two_pass_waveform_metrics():
    """metrics_from_sums on float64 numpy sums against the two-pass definitions: what the device evaluates from its seven sums."""
    for xn in ("codec", "half", "near"):
        x, y = clip(xn), clip("ref")
        got, want = M.metrics_from_sums(sums_np(x, y), float(RATE)), wave_ref(x, y)
        for k in ("l1", "mse", "snr_db"):
            assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (xn, k)
        if xn != "half":                                  # 0.5 y has no residual after scaling: both formulas return rounding noise
            assert abs(got["sisdr_db"] - want["sisdr_db"]) < 1e-6, xn
    got = M.sisdr_from_sums(sums_np(clip("codec"), clip("ref")), float(RATE), scaling=False, zero_mean=False)
    x, y = clip("codec").double().numpy(), clip("ref").double().numpy()
    assert abs(got - 10 * np.log10((y ** 2).sum() / ((x - y) ** 2).sum() + 1e-8)) < 1e-9


# ------------------------------------------------------------------------------------------------ host logic
def test_frame_counts_match_torch_stft():
    for n in EDGE_LENGTHS + (RATE,):
        for w in (32, 1024, 2048):
            assert M.frames_of(n, w) == spectrum(torch.zeros(n), w).shape[1] == 1 + n // (w // 4)
    assert M.frames_of(4095, 2048) == 8 and M.frames_of(4096, 2048) == 9 and M.frames_of(4097, 2048) == 9
    assert M.frames_of(1025, 2048) == 3 and M.frames_of(20000, 2048) == 40 and 40 % 16 != 0


def test_table_shapes_and_values():
    for w, m in ((32, 5), (2048, 320)):
        nb, nbp = w // 2 + 1, M.padded_bins(w)
        basis, filt = M.dft_basis(w), M.mel_table(RATE, w, m)
        assert nbp % 32 == 0 and nbp >= nb and tuple(basis.shape) == (2 * nbp, w) and basis.dtype == torch.float64
        assert tuple(filt.shape) == ((m + 15) // 16 * 16, nbp) and filt.dtype == torch.float64
        assert float(filt[m:].abs().max() if filt.shape[0] > m else 0.0) == 0.0 and float(filt[:, nb:].abs().max()) == 0.0
        # the basis rows are the windowed DFT: bin i of a frame is (row . frame) - i (row + 16 . frame)
        g = torch.Generator().manual_seed(1)
        frame = torch.randn(w, generator=g, dtype=torch.float64)
        want = torch.fft.rfft(frame * torch.hann_window(w, periodic=True, dtype=torch.float64))
        i = torch.arange(nb)
        rows = 32 * (i // 16) + i % 16
        assert float((basis[rows] @ frame - want.real).abs().max()) < 1e-10
        assert float((basis[rows + 16] @ frame + want.imag).abs().max()) < 1e-10
        pad_rows = sorted(set(range(2 * nbp)) - set(rows.tolist()) - set((rows + 16).tolist()))
        assert float(basis[pad_rows].abs().max()) == 0.0
    assert (1 + 17 // 1, M.padded_bins(32)) == (18, 32) and M.padded_bins(2048) == 1056        # 17 bins in one tile pair; 1025 in 66


def test_refusals_and_lds_budget():
    for w, m in zip(M.MEL_WINDOWS, M.MEL_N_MELS):
        assert M.lds_bytes(w, m) <= M.LDS_BYTES and M.refusal([RATE], w, m) is None
    for w in (512, 1024, 2048):
        assert M.lds_bytes(w) <= M.LDS_BYTES and M.refusal([RATE], w) is None
    assert M.lds_bytes(2048, 320) == 3 * 2 * (9728 + 16 * 19) + 3 * 16 * 1064 * 2 + 128
    assert M.lds_bytes(4096) > M.LDS_BYTES and "LDS" in M.refusal([RATE], 4096)
    assert "reflected" in M.refusal([RATE, 1024], 2048) and M.refusal([1025], 2048) is None
    assert "multiple of 32" in M.refusal([RATE], 48) and "multiple of 32" in M.refusal([RATE], 0)
    assert "n_mels" in M.refusal([RATE], 2048, 400)


def test_mismatched_pairs_raise_value_error_before_any_device_work():
    a, b = torch.zeros(3000), torch.zeros(2999)
    with pytest.raises(ValueError):
        M.mel_distance([a], [b], RATE)
    with pytest.raises(ValueError):
        M.waveform_distance(torch.zeros(2, 3000), torch.zeros(2, 2999))
    with pytest.raises(ValueError):
        M.stft_distance([a, a], [a])
    with pytest.raises(M.MmxError):                       # equal lengths, but host memory: no CPU fallback
        M.waveform_distance([a], [a])


def test_dropin_loss_classes_take_the_reference_arguments():
    import loss as DL
    from torch import nn
    m = DL.MelSpectrogramLoss()
    assert m.n_mels == list(M.MEL_N_MELS) and m.window_lengths == list(M.MEL_WINDOWS)
    assert (m.pow, m.mag_weight, m.log_weight, m.clamp_eps) == (1.0, 0.0, 1.0, 1e-5)
    s = DL.MultiScaleSTFTLoss()
    assert s.window_lengths == [2048, 512] and (s.pow, s.mag_weight, s.log_weight, s.clamp_eps) == (2.0, 1.0, 1.0, 1e-5)
    assert DL.MultiScaleSTFTLoss(window_lengths=[1024, 2048]).window_lengths == [1024, 2048]
    d = DL.SISDRLoss()
    assert (d.scaling, d.reduction, d.zero_mean, d.clip_min) == (True, "mean", True, None)
    assert DL.L1Loss().attribute == "audio_data"
    for cls in (DL.MultiScaleSTFTLoss, DL.MelSpectrogramLoss):
        with pytest.raises(NotImplementedError):
            cls(loss_fn=nn.MSELoss())
        with pytest.raises(NotImplementedError):
            cls(match_stride=True)
    with pytest.raises(ValueError):                       # a bare tensor carries no rate
        DL.MelSpectrogramLoss()(torch.zeros(1, 1, 3000), torch.zeros(1, 1, 3000))

    class Sig:
        def __init__(self, a):
            self.audio_data, self.sample_rate = a, RATE
    a, r = DL._audio(Sig(torch.zeros(2, 1, 3000)))
    assert tuple(a.shape) == (2, 3000) and r == RATE
    assert not hasattr(DL, "GANLoss") and not hasattr(DL, "kl_loss")


def test_entry_points_are_declared_bound_and_documented():
    from mmx import _lib
    hdr = open(os.path.join(ROOT, "include", "mmx_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for s in ("mmx_spec_dist", "mmx_wave_sums"):
        assert s in _lib.SYMBOLS and re.search(r"\bint\s+" + s + r"\s*\(", hdr) and f"`{s}`" in doc
    assert _lib.ABI_VERSION == 10
    src = open(os.path.join(ROOT, "minimax-speech_amd", "csrc", "Makefile")).read()
    assert "metrics.hip" in src
    gate = open(os.path.join(ROOT, "tools", "check_resources.py")).read()
    for k in ("spec_dist_kernel", "spec_finish_kernel", "wave_sums_kernel", "wave_finish_kernel"):
        assert f'"{k}"' in gate
