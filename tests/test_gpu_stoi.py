"""STOI and extended STOI on the device (csrc/stoi.hip mmx_stoi_select / mmx_stoi_bands / mmx_stoi_score, mmx/stoi.py) against the
float64 yardstick and fixtures of tests/stoi_f64.py (whose two conditions tests/test_stoi_host.py asserts on the CPU).

Lengths: 4096 (29 spectral frames: 1e-5 with the count), 4097 (one segment), 4225 (two), 4353 / 4481 (32 / 33 frames: the second
16-frame tile begins), 6000 with a gap (37 of 45 frames kept: the compaction crosses a tile), 12000 with three gaps (60 of 92).
Estimates: the reference itself, zeros, +20 dB and 0 dB SNR noise, independent noise, and the +20 dB one 30 dB louder.

Bound.  The cap is a condition of use: STOI is quoted to 0.01, the device value has to be two decimal places better, 1e-4.  The
kernel is deterministic; the constant below is 4 x the worst |device - float64| measured on an MI355X over every case here, per
mode (DESIGN.md lists them), the margin being for clips other than these, and never above the cap."""
import ctypes as C

import numpy as np
import pytest
import torch

import stoi_f64 as R
from mmx import stoi as S
from mmx._lib import MmxError, _p, i64, load, stream

pytestmark = pytest.mark.gpu

CAP = 1e-4
# worst |device - float64| measured on an MI355X over test_scores_against_float64: standard 4.00e-8 (4225 samples, 0 dB SNR), extended
# 8.49e-8 (4097 samples, the +20 dB estimate 30 dB louder)
TOL = {False: min(CAP, 4 * 4.00e-8), True: min(CAP, 4 * 8.49e-8)}
ENERGY_TOL_DB = 1e-5      # fp32 products: |d norm| / norm <= 2^-24, that is 20 / ln 10 * 6e-8 = 5.2e-7 dB; the gate's margin is 0.05 dB
WORST = {False: 0.0, True: 0.0}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pair(n, kind):
    return dev(R.estimate(n, kind)), dev(R.reference(n))


@pytest.mark.parametrize("n", R.LENGTHS)
def test_select_matches_float64(n):
    """Keep mask, F and the frame map are the float64 ones exactly; the energies to fp32 rounding."""
    ref = dev(R.reference(n))[None]
    sel = S.select(ref)
    _, det = R.expected(n, "same", False)
    F = R.KEPT[n]
    assert sel["cap"] == S.frames_of(n) == len(det["keep"])
    assert sel["kept"].tolist() == [F]
    assert sel["mask"][0].cpu().numpy().astype(bool).tolist() == det["keep"].tolist()
    m = sel["map"][0].cpu().numpy()
    assert m[:F].tolist() == det["map"].tolist() and (m[F:] == -1).all()
    err = np.abs(sel["energy"][0].cpu().numpy() - det["energy"]).max()
    print(f"n {n}: energy max |device - float64| {err:.2e} dB")
    assert err <= ENERGY_TOL_DB


@pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
@pytest.mark.parametrize("n", R.LENGTHS)
def test_scores_against_float64(n, extended):
    """The six estimates of one reference as one batch; the spectral frame count is the float64 one exactly."""
    est = [dev(R.estimate(n, k)) for k in R.ESTIMATES]
    ref = [dev(R.reference(n))] * len(est)
    d, frames = S.stoi(est, ref, S.FS, extended=extended, return_frames=True)
    d, frames = d.cpu().tolist(), frames.cpu().tolist()
    for i, k in enumerate(R.ESTIMATES):
        want, det = R.expected(n, k, extended)
        err = abs(d[i] - want)
        WORST[extended] = max(WORST[extended], err)
        print(f"n {n} {k:6s} {'extended' if extended else 'standard'}: device {d[i]:.12f} float64 {want:.12f} |diff| {err:.2e}   "
              f"(worst so far {WORST[extended]:.2e})")
        assert frames[i] == det["frames"] == R.KEPT[n] - 1
        if det["frames"] < 30:
            assert d[i] == want == 1e-5
        else:
            assert err <= TOL[extended], (n, k, d[i], want)
    if n > 4096:
        assert abs(d[0] - 1.0) <= 1e-12 and d[1] == 0.0                 # the identical pair, the zero estimate
        assert abs(d[5] - d[2]) <= 2 * TOL[extended]                    # 30 dB louder: scale invariance


def test_envelopes_against_float64():
    """The one intermediate in memory: band envelopes of the 6000-sample pair (two and a quarter tiles, through the compaction)."""
    est, ref = pair(6000, "snr0")
    sel = S.select(ref[None])
    env = S.bands(est[None], ref[None], None, sel)[0].cpu().double().numpy()       # [2, cap, 16]
    _, det = R.expected(6000, "snr0", False)
    T = det["frames"]
    for s, want in ((0, det["xb"]), (1, det["yb"])):
        got = env[s, :T, :15].T
        rel = np.abs(got - want).max() / want.max()
        print(f"envelope {s}: max |device - float64| / max {rel:.2e}")
        assert rel <= 1e-5                                              # fp32 throughout; 2^-24 = 6e-8 per operation
        assert (env[s, T:] == 0).all() and (env[s, :, 15] == 0).all()


RAGGED = ((4097, "snr20"), (12000, "snr0"), (6000, "noise"), (4353, "loud"))


@pytest.mark.parametrize("extended", [False, True], ids=["standard", "extended"])
def test_ragged_batch_equals_solo_runs_bit_for_bit(extended):
    """Four clips as one padded batch whose rows hold NaN beyond `lens`: every clip has its solo bits, also with the rows reversed."""
    lens = [n for n, _ in RAGGED]
    L = max(lens) + 77
    x = torch.full((len(lens), L), float("nan"), device="cuda")
    y = torch.full((len(lens), L), float("nan"), device="cuda")
    for b, (n, k) in enumerate(RAGGED):
        x[b, :n], y[b, :n] = pair(n, k)
    batch, fb = S.stoi(x, y, S.FS, extended=extended, lens=lens, return_frames=True)
    rev, fr = S.stoi(x.flip(0).contiguous(), y.flip(0).contiguous(), S.FS, extended=extended, lens=lens[::-1], return_frames=True)
    assert torch.isfinite(batch).all()
    for b, (n, k) in enumerate(RAGGED):
        e, r = pair(n, k)
        solo, fs = S.stoi([e], [r], S.FS, extended=extended, return_frames=True)
        assert torch.equal(batch[b], solo[0]) and torch.equal(rev[len(lens) - 1 - b], solo[0]), (n, k)
        assert int(fb[b]) == int(fs[0]) == int(fr[len(lens) - 1 - b]) == R.KEPT[n] - 1


# ----------------------------------------------------------------------------------------------------- the entry points themselves
class Raw:
    """The three entry points on buffers that are longer than the header asks for and filled with a sentinel, each cloned before
    the launch: what a launch may write is named in include/mmx_hip.h, everything else keeps its bits."""

    SLACK = 64

    def __init__(self, est, ref, lens, L):
        self.est, self.ref, self.lens, self.L = est, ref, lens, L
        self.B = ref.shape[0]
        self.cap = S.frames_of(L)
        self.wcap = max(1, -(-(self.cap - S.SEG) // S.SEGMENTS_PER_TILE))
        B, cap, k = self.B, self.cap, self.SLACK
        self.basis, self.filt, self.win = S._device_tables(ref.device)
        self.d_lens = None if lens is None else torch.tensor(lens, dtype=torch.int32, device="cuda")
        self.h_lens = None if lens is None else (C.c_int32 * B)(*lens)
        self.buf = dict(energy=torch.full((B * cap + k,), -7.0, dtype=torch.float64, device="cuda"),
                        mask=torch.full((B * cap + k,), 9, dtype=torch.uint8, device="cuda"),
                        map=torch.full((B * cap + k,), -9, dtype=torch.int32, device="cuda"),
                        kept=torch.full((B + k,), -9, dtype=torch.int32, device="cuda"),
                        env=torch.full((B * 2 * cap * 16 + k,), -7.0, dtype=torch.float32, device="cuda"),
                        work=torch.full((B * self.wcap + k,), -7.0, dtype=torch.float64, device="cuda"),
                        out=torch.full((B + k,), -7.0, dtype=torch.float64, device="cuda"),
                        frames=torch.full((B + k,), -9, dtype=torch.int32, device="cuda"))
        self.before = {}

    def snap(self):
        torch.cuda.synchronize()
        self.before = {k: v.clone() for k, v in self.buf.items()}

    def changed(self):
        torch.cuda.synchronize()
        return {k for k, v in self.buf.items() if not torch.equal(v.view(torch.uint8), self.before[k].view(torch.uint8))}

    def select(self, ref=True, lens=True, h_lens=True, cap=None, L=None):
        b = self.buf
        return load().mmx_stoi_select(_p(self.ref) if ref else None, i64(self.ref.shape[1]), self.L if L is None else L, self.B,
                                      _p(self.d_lens) if lens else None, self.h_lens if h_lens else None, _p(self.win), _p(b["energy"]),
                                      _p(b["mask"]), _p(b["map"]), _p(b["kept"]), self.cap if cap is None else cap, stream())

    def bands(self, filt=True, h_lens=True, cap=None):
        b = self.buf
        return load().mmx_stoi_bands(_p(self.est), i64(self.est.shape[1]), _p(self.ref), i64(self.ref.shape[1]), self.L, self.B,
                                     _p(self.d_lens), self.h_lens if h_lens else None, _p(self.win), _p(b["map"]), _p(b["kept"]),
                                     _p(self.basis), _p(self.filt) if filt else None, _p(b["env"]), self.cap if cap is None else cap, stream())

    def score(self, extended=0, wcap=None, out=True):
        b = self.buf
        return load().mmx_stoi_score(_p(b["env"]), self.cap, self.B, _p(b["kept"]), extended, _p(b["work"]),
                                     self.wcap if wcap is None else wcap, _p(b["out"]) if out else None, _p(b["frames"]), stream())


def ragged_raw():
    lens = [6000, 4097, 12000]
    L = 12000
    x = torch.full((3, L), float("nan"), device="cuda")
    y = torch.full((3, L), float("nan"), device="cuda")
    for b, (n, k) in enumerate(zip(lens, ("snr0", "snr20", "noise"))):
        x[b, :n], y[b, :n] = pair(n, k)
    return Raw(x, y, lens, L), lens


def test_outputs_not_named_are_unchanged():
    """Each entry point writes the buffers the header names, inside the extents it names, and nothing else."""
    raw, lens = ragged_raw()
    B, cap, wcap, k = raw.B, raw.cap, raw.wcap, raw.SLACK
    nf = [S.frames_of(n) for n in lens]
    F = [R.KEPT[n] for n in lens]

    raw.snap()
    assert raw.select() == 0
    assert raw.changed() == {"energy", "mask", "map", "kept"}
    b, old = raw.buf, raw.before
    assert b["kept"][:B].tolist() == F
    for name, n in (("energy", B * cap), ("mask", B * cap), ("map", B * cap), ("kept", B)):
        assert torch.equal(b[name][n:], old[name][n:]), name              # the slack past the stated extent
    e, eo = b["energy"][:B * cap].view(B, cap), old["energy"][:B * cap].view(B, cap)
    for i in range(B):
        assert torch.equal(e[i, nf[i]:], eo[i, nf[i]:])                   # energies past the clip's own frames are not written
    assert set(b["mask"][:B * cap].unique().tolist()) <= {0, 1}            # every byte of mask and map is

    raw.snap()
    old = raw.before
    assert raw.bands() == 0
    assert raw.changed() == {"env"}
    env, envo = b["env"][:B * 2 * cap * 16].view(B, 2, cap, 16), old["env"][:B * 2 * cap * 16].view(B, 2, cap, 16)
    assert torch.equal(b["env"][B * 2 * cap * 16:], old["env"][B * 2 * cap * 16:])
    for i in range(B):
        assert torch.equal(env[i, :, F[i] - 1:], envo[i, :, F[i] - 1:])    # rows at and past F - 1
        assert torch.isfinite(env[i, :, :F[i] - 1]).all()

    for ext in (0, 1):
        b["work"].fill_(-7.0), b["out"].fill_(-7.0), b["frames"].fill_(-9)
        raw.snap()
        old = raw.before
        assert raw.score(ext) == 0
        assert raw.changed() == {"work", "out", "frames"}
        assert b["frames"][:B].tolist() == [f - 1 for f in F]
        for name, n in (("work", B * wcap), ("out", B), ("frames", B)):
            assert torch.equal(b[name][n:], old[name][n:]), name
        w, wo = b["work"][:B * wcap].view(B, wcap), old["work"][:B * wcap].view(B, wcap)
        for i in range(B):
            tiles = -(-(F[i] - 30) // S.SEGMENTS_PER_TILE)
            assert torch.equal(w[i, tiles:], wo[i, tiles:])
        # the raw path is the wrapper's path: the same bits
        est = [raw.est[i, :n] for i, n in enumerate(lens)]
        ref = [raw.ref[i, :n] for i, n in enumerate(lens)]
        assert torch.equal(b["out"][:B], S.stoi(est, ref, S.FS, extended=bool(ext)))


def test_every_earg_path_launches_nothing():
    raw, lens = ragged_raw()
    assert raw.select() == 0 and raw.bands() == 0 and raw.score(0) == 0     # a good state to damage
    raw.snap()
    short, long_ = Raw(raw.est, raw.ref, [6000, 256, 12000], raw.L), Raw(raw.est, raw.ref, [6000, 4097, 12001], raw.L)
    short.buf = long_.buf = raw.buf                      # the same outputs behind other lengths
    calls = [raw.select(ref=False),                      # a missing pointer
             raw.select(h_lens=False),                   # device lens without their host copy
             raw.select(lens=False),                     # and the other way round
             raw.select(cap=raw.cap - 1),                # a capacity below frames_of(L)
             raw.select(L=256),                          # no frame at all
             short.select(), short.bands(),              # one member of 256 samples
             long_.select(), long_.bands(),              # one member longer than L
             raw.bands(filt=False), raw.bands(h_lens=False), raw.bands(cap=raw.cap - 1),
             raw.score(2), raw.score(-1), raw.score(0, wcap=raw.wcap - 1), raw.score(0, out=False)]
    assert calls == [-1] * len(calls), calls
    assert raw.changed() == set()
    with pytest.raises(MmxError, match="holds no frame"):
        S.stoi([raw.est[0, :256]], [raw.ref[0, :256]], S.FS)
    with pytest.raises(MmxError, match="holds no frame"):                 # 600 samples at 24 kHz are 250 at 10 kHz
        S.stoi([raw.est[0, :600]], [raw.ref[0, :600]], 24000)
    with pytest.raises(ValueError, match="differ in length"):
        S.stoi([raw.est[0, :6000]], [raw.ref[0, :5999]], S.FS)
    with pytest.raises(MmxError, match="no CPU fallback"):
        S.stoi([raw.est[0, :6000].cpu()], [raw.ref[0, :6000].cpu()], S.FS)
    assert raw.changed() == set()


def test_other_rates_go_through_the_projects_resampler():
    """A 24 kHz pair equals the same pair resampled by mmx.resample by hand, bit for bit: the number is STOI on this project's
    10 kHz rendering."""
    from mmx.resample import resample
    est = [pair(4353, "snr0")[0].repeat(3)[:12000], pair(4481, "snr20")[0].repeat(4)[:14400]]      # fixtures without a gap
    ref = [pair(4353, "snr0")[1].repeat(3)[:12000], pair(4481, "snr20")[1].repeat(4)[:14400]]
    for ext in (False, True):
        got, frames = S.stoi(est, ref, 24000, extended=ext, return_frames=True)
        want = S.stoi(resample(est, 24000, S.FS), resample(ref, 24000, S.FS), S.FS, extended=ext)
        assert torch.equal(got, want) and got.dtype == torch.float64 and got.is_cuda
        assert frames.tolist() == [S.frames_of(5000) - 1, S.frames_of(6000) - 1]      # nothing is silent in these renderings
        assert torch.isfinite(got).all() and (got < 1.0).all()
    # a padded tensor with equal lengths takes the same path
    both = S.stoi(torch.stack([est[0], est[0]]), torch.stack([ref[0], ref[0]]), 24000)
    assert torch.equal(both[0], both[1]) and torch.equal(both[0], S.stoi(est[:1], ref[:1], 24000)[0])


def test_module_and_input_forms():
    e, r = pair(6000, "snr0")
    want = S.stoi([e], [r], S.FS)
    assert torch.equal(S.STOI()(e[None], r[None]), want)
    assert torch.equal(S.STOI(extended=True)(e[None, None], r[None, None]), S.stoi([e], [r], S.FS, extended=True))
    assert torch.equal(S.stoi(e[None], r[None], 10000.0), want)
