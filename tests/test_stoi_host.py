"""The host side of STOI (mmx/stoi.py: tables, shape rules, refusals) and the float64 yardstick of tests/stoi_f64.py with its
fixtures.  Two properties of the fixtures are CONDITIONS of the GPU tests, asserted here: no reference frame's energy lies within
0.05 dB of its clip's threshold (the mask must be decided alike in fp32 and float64), and every (segment, band) of every reference
keeps a mean-removed norm of at least 1e-3 of its norm (below that the division by norm + EPS turns rounding into the answer, in
float64 as well).  Where a fixture misses one, the fixture changes, not the bound."""
import numpy as np
import pytest
import torch

import stoi_f64 as R
from mmx import stoi as S
from mmx._lib import MmxError

BAND_LIST = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87), (87, 109),
             (109, 138), (138, 174), (174, 219)]


def test_band_edges_and_table():
    assert S.band_edges() == BAND_LIST == list(S.BAND_EDGES) == R.band_matrix()[1]
    t = S.third_octave_table()
    assert t.dtype == torch.float64 and tuple(t.shape) == (16, 288) and S.padded_bins() == 288
    assert set(t.unique().tolist()) == {0.0, 1.0}
    assert t.sum(dim=1).tolist() == [float(b - a) for a, b in BAND_LIST] + [0.0]
    assert torch.equal(t[:15, :257], torch.from_numpy(R.band_matrix()[0]))
    assert BAND_LIST[-1][1] <= 16 * S.BIN_TILES                       # the bin tiles the kernel computes hold every band


def test_basis_is_the_zero_padded_window():
    b = S.dft_basis()
    assert tuple(b.shape) == (576, 256)
    w = S.window()
    assert np.array_equal(w, np.hanning(258)[1:-1]) and len(w) == 256
    k = np.arange(256)
    for bin_ in (0, 7, 100, 218, 256):
        row = 32 * (bin_ // 16) + bin_ % 16
        np.testing.assert_allclose(b[row].numpy(), w * np.cos(2 * np.pi * bin_ * k / 512), atol=1e-12)
        np.testing.assert_allclose(b[row + 16].numpy(), w * np.sin(2 * np.pi * bin_ * k / 512), atol=1e-12)


def test_frames_of():
    assert [S.frames_of(n) for n in (0, 256, 257, 384, 385, 3969, 4096, 4097)] == [0, 0, 1, 1, 2, 30, 30, 31]
    for n in (257, 300, 384, 385, 4096, 4097, 6000):
        assert S.frames_of(n) == len(R.starts(n))
    assert [S.spectral_frames(k) for k in (0, 1, 2, 31)] == [0, 0, 1, 30]
    assert S.lds_bytes() == 2 * 3 * 2 * 2448 + 2 * 3 * 16 * 232 * 2 and S.lds_bytes() <= 160 * 1024


def test_the_strict_bound_applies_twice():
    """3969 and 4096 samples: 30 energy frames, all kept, rebuild 3968 + 128 samples, which hold 29 frames -> 1e-5.  4097 is the
    shortest clip with one segment."""
    for n, frames in ((3969, 29), (4096, 29), (4097, 30)):
        x = R.reference(4481)[:n]
        d, det = R.stoi(x, x, detail=True)
        assert det["keep"].all() and len(det["keep"]) == frames + 1 and det["frames"] == frames
        assert (d == 1e-5) == (frames < 30)
        if frames >= 30:
            assert abs(d - 1.0) <= 1e-12


@pytest.mark.parametrize("n", R.LENGTHS)
def test_fixture_conditions(n):
    e, keep, kept = R.select(R.reference(n).astype(np.float64))
    assert len(e) == S.frames_of(n) and int(keep.sum()) == R.KEPT[n] == len(kept)
    assert np.abs(e - (e.max() - 40.0)).min() >= 0.05, "a frame energy within 0.05 dB of the threshold"
    _, det = R.expected(n, "same", False)
    assert det["frames"] == R.KEPT[n] - 1
    if det["frames"] >= 30:
        s = R.segments(det["xb"])
        c = s - s.mean(axis=2, keepdims=True)
        ratio = np.linalg.norm(c, axis=2) / np.linalg.norm(s, axis=2)
        assert ratio.min() >= 1e-3, ratio.min()


def test_the_compaction_crosses_tiles():
    _, det = R.expected(6000, "same", False)
    assert len(det["keep"]) == 45 and det["map"].tolist() != list(range(37)) and det["map"][-1] == 44
    _, det = R.expected(12000, "same", False)
    assert len(det["keep"]) == 92 and not det["keep"][0] and not det["keep"][-1] and len(det["map"]) == 60


@pytest.mark.parametrize("n", [n for n in R.LENGTHS if n > 4096])
def test_values_of_the_yardstick(n):
    for ext in (False, True):
        assert abs(R.expected(n, "same", ext)[0] - 1.0) <= 1e-12
        assert R.expected(n, "zero", ext)[0] == 0.0
        assert 0.8 < R.expected(n, "snr20", ext)[0] < 1.0
        assert R.expected(n, "snr0", ext)[0] < R.expected(n, "snr20", ext)[0]
        # scale invariance: 30 dB louder, to the rounding of the louder fp32 samples
        assert abs(R.expected(n, "loud", ext)[0] - R.expected(n, "snr20", ext)[0]) <= 1e-6
    assert abs(R.expected(n, "noise", True)[0]) <= 0.1
    assert abs(R.expected(n, "noise", False)[0]) <= 0.1


def test_both_sides_of_the_clip_are_exercised():
    shares = [R.clipped_share(R.expected(n, k, False)[1]["xb"], R.expected(n, k, False)[1]["yb"]) for n in (6000, 12000) for k in ("snr0", "noise")]
    assert all(0.0 < s < 0.5 for s in shares), shares


def test_refusals():
    assert S.refusal([4097]) is None and S.refusal([257], 24000) is None
    assert "holds no frame" in S.refusal([4097, 256])
    assert "holds no frame" in S.refusal([0])
    assert "sample rate" in S.refusal([4097], 0)
    assert "sample rate" in S.refusal([4097], 22050.5)
    assert "differ in length" in S.refusal([4097, 5000], S.FS, [4097, 4999])
    x = torch.zeros(4097)
    with pytest.raises(ValueError, match="differ in length"):            # clips.pack_pair, before anything touches a device
        S.stoi([x], [x[:4000]], 10000)
    with pytest.raises(MmxError, match="no CPU fallback"):
        S.stoi([x], [x], 10000)
    with pytest.raises(MmxError, match="sample rate"):
        S.stoi([x], [x], 0)


def test_symbols_are_bound():
    from mmx import _lib
    assert {"mmx_stoi_select", "mmx_stoi_bands", "mmx_stoi_score"} <= set(_lib.SYMBOLS) and _lib.ABI_VERSION == 10
