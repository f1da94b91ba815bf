"""Host side of the reference-audio front end (mmx/mel.py), no GPU: the Slaney filterbank restated from librosa's published
definition, the crop rule of cosyvoice/dataset/processor.py:370-373, and the mel fixture's own consistency."""
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "mel.npz"))


@pytest.mark.parametrize("fmax", [8000, None])
def test_filterbank_structure(fmax):
    """[80][961], non-negative, every row one rising and one falling ramp, about unit area: sum * 12.5 Hz within 2 % of 1 for
    filters wider than four bins (12.5 Hz = 24000 / 1920, the bin spacing: a Slaney-normalised triangle of width w Hz has area
    1 in Hz, and sampling it every 12.5 Hz integrates it to O((12.5 / w)^2))."""
    from mmx import mel as M
    fb = M.mel_filterbank(24000, 1920, 80, 0, fmax)
    assert fb.shape == (80, 961) and fb.dtype == np.float32 and (fb >= 0).all()
    for i, row in enumerate(fb):
        nz = np.flatnonzero(row)
        assert nz.size > 0, i
        assert (np.diff(nz) == 1).all(), i                       # one contiguous support
        seg = row[nz[0] - 1:nz[-1] + 2].astype(np.float64)
        d = np.sign(np.diff(seg))
        k = int(np.argmax(seg))
        assert (d[:k] > 0).all() and (d[k:] < 0).all(), i        # rising, then falling
        if nz.size > 4:
            assert abs(row.astype(np.float64).sum() * 12.5 - 1) < 0.02, (i, row.sum() * 12.5)
    # centres rise with the channel
    assert (np.diff(fb.argmax(axis=1)) > 0).all()


def test_nonzero_bin_range():
    """fmax = 8000 at 24 kHz: bin 640 sits on fmax and bin 0 on fmin, so bins 1 .. 639 of 961 carry weight."""
    from mmx import mel as M
    assert M.nonzero_bins(M.mel_filterbank(24000, 1920, 80, 0, 8000)) == (1, 639)
    b0, n = M.nonzero_bins(M.mel_filterbank(24000, 1920, 80, 0, None))
    assert b0 == 1 and b0 + n <= 961 and n > 900


def test_filterbank_is_the_fixture_one(gold):
    from mmx import mel as M
    assert np.array_equal(M.mel_filterbank(24000, 1920, 80, 0, 8000), gold["fb_8000"])
    assert np.array_equal(M.mel_filterbank(24000, 1920, 80, 0, None), gold["fb_full"])


@pytest.mark.parametrize("n", [12000, 50000, 96000, 96001, 120000, 131313])
def test_crop_indices_follow_the_processor(n):
    """processor.py:370-376 (training=False): longer than max_length -> centre crop, else the whole clip."""
    from mmx import mel as M
    sr, max_samples = 24000, int(4.0 * 24000)
    a, b = M.crop_bounds(n, sr, 0.5, 4.0)
    if n > max_samples:
        start = (n - max_samples) // 2
        assert (a, b) == (start, start + max_samples)
    else:
        assert (a, b) == (0, n)
    assert torch.equal(torch.arange(n)[a:b], torch.arange(n)[None][:, a:b][0])


def test_too_short_reference_raises():
    from mmx import mel as M
    with pytest.raises(ValueError):
        M.crop_bounds(11999, 24000, 0.5, 4.0)
    assert M.crop_bounds(12000, 24000, 0.5, 4.0) == (0, 12000)


def test_frame_counts():
    from mmx import mel as M
    assert [M.frames_of(n, 1920, 480) for n in (4800, 2400, 1440, 96000, 721, 720)] == [10, 5, 3, 200, 1, 0]


def test_front_end_has_no_cpu_fallback():
    from mmx import mel as M
    from mmx._lib import MmxError
    from matcha.utils.audio import mel_spectrogram
    with pytest.raises(MmxError):
        mel_spectrogram(torch.zeros(1, 4800), 1920, 80, 24000, 480, 1920, 0, 8000)
    with pytest.raises(MmxError):
        M.prepare_reference(torch.zeros(24000), 24000)
    with pytest.raises(NotImplementedError):
        mel_spectrogram(torch.zeros(1, 4800), 1920, 80, 24000, 480, 1920, 0, 8000, center=True)


@pytest.mark.parametrize("name,frames", [("noise", 10), ("tone", 5), ("short", 3), ("noise_full", 10)])
def test_fixture_fp32_agrees_with_float64(gold, name, frames):
    """Guards the fixture, not the code: the reference function's fp32 output and the float64 evaluation of the same formula
    agree to the bound recorded beside them."""
    r32, r64, tol = gold[f"ref32_{name}"], gold[f"ref64_{name}"], float(gold[f"tol_{name}"])
    assert r32.shape == r64.shape == (80, frames) and r32.dtype == np.float32 and r64.dtype == np.float64
    assert np.abs(r32 - r64).max() <= tol
    w = gold["wave_" + name.split("_")[0]]
    assert w.dtype == np.float32 and abs(np.abs(w).max() - 1) < 1e-6


@pytest.mark.parametrize("n", [32, 96])
def test_metrics_basis_is_the_shared_builder(n):
    from mmx import mel as M, metrics as MT
    assert torch.equal(MT.dft_basis(n), M.dft_basis(n, 0, n // 2 + 1)) and torch.equal(MT.dft_basis(n), M.dft_basis(n))


def test_basis_k_padding_is_exactly_zero():
    from mmx import mel as M
    plain, padded = M.dft_basis(48, 2, 20), M.dft_basis(48, 2, 20, kp=64)
    assert plain.shape == (64, 48) and padded.shape == (64, 64) and padded.dtype == torch.float64
    assert torch.equal(padded[:, :48], plain) and not padded[:, 48:].any() and plain.any()


def test_basis_row_map_crosses_a_tile():
    """n_bins 17: bin 16 opens the second 16-row tile pair (rows 32 and 48); rows of no bin are zero."""
    from mmx import mel as M
    n_fft, bin0, n_bins = 64, 3, 17
    t = M.dft_basis(n_fft, bin0, n_bins)
    assert t.shape == (64, n_fft)
    k = np.arange(n_fft)
    hann = 0.5 - 0.5 * np.cos(2 * np.pi * k / n_fft)
    used = []
    for i in range(n_bins):
        row = 32 * (i // 16) + i % 16
        used += [row, row + 16]
        ph = 2 * np.pi * (((bin0 + i) * k) % n_fft) / n_fft
        assert np.abs(t[row].numpy() - hann * np.cos(ph)).max() < 1e-15, i
        assert np.abs(t[row + 16].numpy() - hann * np.sin(ph)).max() < 1e-15, i
    assert used[-2:] == [32, 48]
    assert not t[[r for r in range(64) if r not in used]].any()


def test_planes3_sum_back_to_24_bits():
    from mmx import mel as M
    t = M.dft_basis(96)
    p = M.planes3(t)
    assert M._planes3 is M.planes3 and len(p) == 3 and all(q.dtype == torch.bfloat16 and q.shape == t.shape for q in p)
    s = p[0].double() + p[1].double() + p[2].double()
    assert ((s - t).abs() <= 2.0 ** -24 * t.abs()).all()
    f = M.filter_table(M.mel_filterbank(16000, 96, 20), 1, 40)
    assert f.shape == (32, 64) and f.dtype == torch.float64 and not f[20:].any() and not f[:, 40:].any()
    assert torch.equal(torch.stack(M.planes3(f)).double().sum(0), f)      # fp32 values: three bf16 terms hold them exactly
