"""Channel degradations on the device (csrc/channel.hip mmx_pad_edge_rows / mmx_row_select / mmx_clip_rows / mmx_quantize_rows and the
FIR of csrc/degrade.hip behind them, mmx/channel.py) against the float64 restatement of tests/test_channel_host.py, then the
`ir_eq` / `noise_eq` arguments of mmx.degrade and the engine keyword (TtsEngine.prompt_from_clip / prompts_from_clips, degrade=).

Inputs: B = 3 ragged clips of 1000, NOUT + 3 and 2 NOUT + 517 samples (tests/test_gpu_degrade.py's), as a padded batch whose
columns past each clip's length hold NaN: a finite result proves that nothing past `lens` was read.

Filters: low_pass(8000, zeros=8) at 24 kHz (25 taps), low_pass(4000) (307 taps), high_pass(100) (12 241 taps: three K chunks of the
FIR, and a margin longer than the shortest clip), the equalizer with 3 and 6 bands and per-clip curves in [-1, 0], mel_filterbank(6).
Bound (the convention of tests/test_gpu_degrade.py): per clip max |y - y64| / max |y64| <= max(4 * base, 1e-6), y64 the float64
restatement, base the same restatement run in float32 against it.

Order statistics equal torch.sort of the row on the CPU, by value, exactly.  Thresholds: within 2^-23 * max(|v_lo|, |v_hi|) of the
float64 lerp (one fp32 rounding of a value between the two is 2^-24 of the larger).  Clipping: torch.clamp with the device's own
thresholds, bit for bit.  Quantizers, Q in {8, 256, 65536}: within 2^-23 relative of the float64 restatement (one fp32 rounding is
2^-24; the device's log1p / exp differ from the host's in the last fp64 bits only) and the same codes wherever the restatement's
value before truncation is further than 1e-9 from a whole number - an fp32 implementation flips codes at Q = 65536 and fails."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_channel_host as H
import test_gpu_degrade as GD
from test_gpu_degrade import eng                         # noqa: F401  (the module-scoped engine fixture)
from mmx import channel as CH, clips, degrade as D
from mmx._lib import MmxError, check, i64, load, stream, _p

pytestmark = pytest.mark.gpu

RATE = 24000
NS = GD.NS
bits, padded = GD.bits, GD.padded
CURVES = {3: [[0.0, -1.0, -0.5], [-0.3, 0.0, -0.9], [-1.0, -0.25, 0.0]],
          6: [[0.0, -0.2, -0.4, -0.6, -0.8, -1.0], [-1.0, 0.0, -0.7, -0.1, -0.5, -0.3], [-0.45, -0.9, 0.0, -1.0, -0.15, -0.6]]}
FILTERS = {
    "lp8k": (lambda x, lens: CH.low_pass(x, 8000, RATE, zeros=8, lens=lens), lambda x, b, dt: H.ref_low_pass(x, 8000, RATE, 8, dt), 25),
    "lp4k": (lambda x, lens: CH.low_pass(x, 4000, RATE, lens=lens), lambda x, b, dt: H.ref_low_pass(x, 4000, RATE, 51, dt), 307),
    "hp100": (lambda x, lens: CH.high_pass(x, 100, RATE, lens=lens), lambda x, b, dt: H.ref_high_pass(x, 100, RATE, 51, dt), 12241),
    "eq3": (lambda x, lens: CH.equalizer(x, CURVES[3], RATE, lens=lens), lambda x, b, dt: H.ref_equalizer(x, CURVES[3][b], RATE, dt), None),
    "eq6": (lambda x, lens: CH.equalizer(x, CURVES[6], RATE, lens=lens), lambda x, b, dt: H.ref_equalizer(x, CURVES[6][b], RATE, dt), None),
    "mel6": (lambda x, lens: CH.mel_filterbank(x, 6, RATE, lens=lens), lambda x, b, dt: H.ref_split_bands(x, RATE, 6, dt).T, None),
}


@functools.lru_cache(None)
def inputs():
    return [GD.clip(n, 10 + i) for i, n in enumerate(NS)]


@functools.lru_cache(None)
def batch():
    return padded(inputs())


@functools.lru_cache(None)
def device(name):
    x, lens = batch()
    out = FILTERS[name][0](x, lens)
    torch.cuda.synchronize()
    return out


@functools.lru_cache(None)
def reference(name):
    """(y64, base) per clip, computed once."""
    out = []
    for b, x in enumerate(inputs()):
        y64 = FILTERS[name][1](x, b, torch.float64)
        out.append((y64, H.rel_err(FILTERS[name][1](x, b, torch.float32), y64)))
    return out


# ------------------------------------------------------------------------------------------------ filters
@pytest.mark.parametrize("name", list(FILTERS))
def test_filter_parity(name):
    x, lens = batch()
    out = device(name)
    assert out.shape == ((3, x.shape[1], 6) if name == "mel6" else x.shape)
    if FILTERS[name][2]:
        cut, zeros = {"lp8k": (8000, 8), "lp4k": (4000, 51), "hp100": (100, 51)}[name]
        assert 2 * CH.half_size(cut, RATE, zeros) + 1 == FILTERS[name][2]
    for b, (y64, base) in enumerate(reference(name)):
        y = out[b, :lens[b]].cpu()
        assert torch.isfinite(y).all()
        err, bound = H.rel_err(y, y64), max(4 * base, 1e-6)
        print(f"{name} clip {b}: N {lens[b]} err {err:.3e} base {base:.3e} bound {bound:.3e}")
        assert err <= bound, (name, b, err, bound)
        assert not out[b, lens[b]:].any()                # tail columns are zeros


def test_filters_keep_their_invariants_on_the_device():
    x, lens = batch()
    for b in range(3):
        n = lens[b]
        s = device("lp4k")[b, :n] + CH.high_pass(x, 4000, RATE, lens=lens)[b, :n]
        # each filter's output is within the parity bound's floor, 1e-6 of a peak that is at most the input's: k outputs, k * 1e-6
        assert H.rel_err(s.cpu(), inputs()[b]) <= 2e-6                    # low_pass + high_pass == x
        assert H.rel_err(device("mel6")[b, :n].sum(-1).cpu(), inputs()[b]) <= 6e-6      # the bands sum to x
    const = torch.full((5000,), 0.37, device="cuda")
    assert (CH.low_pass(const, 4000, RATE) - 0.37).abs().max() <= 1e-6 * 0.37           # the edge rule
    flat = CH.equalizer(x, [0.0] * 6, RATE, lens=lens)
    assert H.rel_err(flat[1, :lens[1]].cpu(), inputs()[1]) <= 1e-6


def test_batched_equals_solo_bit_for_bit():
    xs = [x.cuda() for x in inputs()]
    _, lens = batch()
    listed = {"lp4k": CH.low_pass(xs, 4000, RATE), "eq6": CH.equalizer(xs, CURVES[6], RATE), "mel6": CH.mel_filterbank(xs, 6, RATE)}
    solo = {"lp8k": lambda b: CH.low_pass(xs[b], 8000, RATE, zeros=8), "lp4k": lambda b: CH.low_pass(xs[b], 4000, RATE),
            "hp100": lambda b: CH.high_pass(xs[b], 100, RATE), "eq3": lambda b: CH.equalizer(xs[b], CURVES[3][b], RATE),
            "eq6": lambda b: CH.equalizer(xs[b], CURVES[6][b], RATE), "mel6": lambda b: CH.mel_filterbank(xs[b], 6, RATE)}
    for name, fn in solo.items():
        for b in range(3):
            one = fn(b)
            assert one.shape[0] == lens[b] and torch.equal(bits(one), bits(device(name)[b, :lens[b]])), (name, b)
            if name in listed:
                assert torch.equal(bits(one), bits(listed[name][b])), (name, b)
    # one cutoff per clip: every clip's filter is designed from its own cutoff, so clips of different `half` share a call
    mixed = CH.low_pass(xs, [4000.0, 8000.0, 4000.0], RATE)
    for b, f in enumerate((4000, 8000, 4000)):
        assert torch.equal(bits(mixed[b]), bits(CH.low_pass(xs[b], f, RATE)))
    assert torch.equal(bits(CH.LowPass(RATE)(xs[1], 4000)), bits(listed["lp4k"][1]))
    assert torch.equal(bits(CH.HighPass(RATE)(xs[0], 100)), bits(device("hp100")[0, :lens[0]]))
    assert torch.equal(bits(CH.Equalizer(RATE)(xs[2], CURVES[6][2])), bits(listed["eq6"][2]))


# ------------------------------------------------------------------------------------------------ order statistics, clipping
def select_rows():
    g = torch.Generator().manual_seed(5)
    tiny = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 3.0, -3.0, float("inf"),
                         -float("inf"), 0.0, -0.0, 2.5e-39, 1.0], dtype=torch.float32)
    rows = [torch.tensor([0.25]), torch.tensor([0.5, -0.75]),
            (torch.randint(0, 8, (3001,), generator=g).float() - 3.5) / 4,               # eight levels: heavy ties
            tiny[torch.randperm(tiny.numel(), generator=g)],
            GD.clip(CH.SELECT_SPAN + 77, 21),                                             # two workgroups, the second with 77 samples
            GD.clip(3 * CH.SELECT_SPAN, 22)]                                              # three full workgroups
    return rows


def test_order_statistics_are_exact():
    rows = select_rows()
    x, lens = padded(rows, extra=5)
    sorts = [torch.sort(r).values for r in rows]
    for pick in (lambda n: [0, n // 2, n - 1], lambda n: [n - 1, 0, (n - 1) // 3, min(n - 1, n // 2 + 1)], lambda n: [n // 2]):
        ranks = [pick(n) for n in lens]
        vals, flag = CH.order_statistics(x, ranks, lens)
        assert not flag.any()
        for b, n in enumerate(lens):
            want = sorts[b][ranks[b]]
            assert (vals[b].cpu() == want).all(), (b, ranks[b], vals[b].cpu().tolist(), want.tolist())
    # every rank of the row of zeros, denormals and infinities
    n = lens[3]
    for k0 in range(0, n, 4):
        vals, _ = CH.order_statistics(x[3:4], [list(range(k0, k0 + 4))], [n])
        assert (vals[0].cpu() == sorts[3][k0:k0 + 4]).all()
    solo, _ = CH.order_statistics(rows[4].cuda()[None], [[0, lens[4] // 2, lens[4] - 1]])
    assert torch.equal(solo[0].cpu(), sorts[4][[0, lens[4] // 2, lens[4] - 1]])
    with pytest.raises(MmxError):
        CH.order_statistics(x, [[n] for n in lens], lens)


@pytest.mark.parametrize("q", [0.0, 0.1, 1.0])
def test_thresholds_and_clipping(q):
    x, lens = batch()
    thr = CH.clip_thresholds(x, q, lens=lens)
    out = CH.clip_distortion(x, q, lens=lens)
    assert thr.shape == (3, 2) and out.shape == x.shape
    for b, w in enumerate(inputs()):
        n, v = lens[b], torch.sort(w.double()).values
        for side, r in enumerate((q / 2, 1 - q / 2)):
            lo, hi, _ = CH.quantile_ranks(n, r)
            want, tol = float(H.ref_quantile(v, n, r)), 2.0 ** -23 * max(abs(float(v[lo])), abs(float(v[hi])))
            print(f"q {q} clip {b} side {side}: device {float(thr[b, side]):.9e} float64 {want:.9e} tol {tol:.2e}")
            assert abs(float(thr[b, side]) - want) <= tol
        t = thr[b].cpu()
        assert torch.equal(bits(out[b, :n].cpu()), bits(w.clamp(t[0], t[1]))) and not out[b, n:].any()
        assert torch.equal(bits(CH.clip_distortion(w.cuda(), q)), bits(out[b, :n]))         # solo
        assert torch.equal(bits(CH.clip_thresholds(w.cuda(), q)[0]), bits(thr[b]))
    if q == 0.0:
        assert torch.equal(bits(out[1, :lens[1]].cpu()), bits(inputs()[1]))
    if q == 0.1:
        per = CH.clip_distortion(x, [0.1, 0.0, 1.0], lens=lens)
        assert torch.equal(bits(per[0]), bits(out[0])) and torch.equal(bits(CH.ClippingDistortion()(inputs()[2].cuda(), 0.1)), bits(out[2, :lens[2]]))


def test_a_nan_row_is_nan_and_its_neighbours_are_untouched():
    x, lens = batch()
    bad = x.clone()
    bad[1, 4000] = float("nan")
    thr, out = CH.clip_thresholds(bad, 0.1, lens=lens), CH.clip_distortion(bad, 0.1, lens=lens)
    good_thr, good = CH.clip_thresholds(x, 0.1, lens=lens), CH.clip_distortion(x, 0.1, lens=lens)
    assert torch.isnan(thr[1]).all() and torch.isnan(out[1, :lens[1]]).all() and not out[1, lens[1]:].any()
    for b in (0, 2):
        assert torch.equal(bits(thr[b]), bits(good_thr[b])) and torch.equal(bits(out[b]), bits(good[b]))
    vals, flag = CH.order_statistics(bad, [[0, 5], [0, 5], [0, 5]], lens)
    assert flag.tolist() == [0, 1, 0] and torch.isnan(vals[1]).all() and torch.isfinite(vals[[0, 2]]).all()


# ------------------------------------------------------------------------------------------------ quantizers
@pytest.mark.parametrize("Q", [8, 256, 65536])
def test_quantizers(Q):
    x, lens = batch()
    uni, mul = CH.quantization(x, Q, lens=lens), CH.mulaw_quantization(x, Q, lens=lens)
    mu, lmu = Q - 1.0, np.log1p(Q - 1.0)
    for b, w in enumerate(inputs()):
        n = lens[b]
        for name, got, (want, pre) in (("uniform", uni[b, :n].cpu().double(), H.ref_quantization(w, Q)),
                                       ("mulaw", mul[b, :n].cpu().double(), H.ref_mulaw(w, Q))):
            err = ((got - want).abs() / want.abs().clamp(min=1e-300)).max()
            far = (pre - pre.round()).abs() > 1e-9       # the restatement's code is not a matter of its own last bits
            if name == "uniform":
                code, back = pre.floor(), (got + 1) / 2 * Q
            else:
                code, back = pre.trunc(), (torch.sign(got) * torch.log1p(mu * got.abs()) / lmu + 1) / 2 * mu
            print(f"{name} Q {Q} clip {b}: max rel err {float(err):.3e}; {int((~far).sum())} values within 1e-9 of a whole number; "
                  f"codes recovered to {float((back - back.round()).abs().max()):.2e}")
            assert float(err) <= 2.0 ** -23
            assert (back - back.round()).abs().max() < 1e-2 and torch.equal(back.round()[far], code[far])
            if name == "mulaw":
                assert far.all()                         # measured on the CPU: at least 4.6e-6 from a whole number for these clips
            else:
                assert torch.equal(back, code)           # Q is a power of two: every step of the uniform quantizer is exact in fp64
        assert not uni[b, n:].any() and not mul[b, n:].any()
        assert torch.equal(bits(CH.quantization(w.cuda(), Q)), bits(uni[b, :n]))             # solo
        assert torch.equal(bits(CH.mulaw_quantization(w.cuda(), Q)), bits(mul[b, :n]))
    per = CH.mulaw_quantization(x, [Q, 8, 256], lens=lens)
    assert torch.equal(bits(per[0]), bits(mul[0])) and torch.equal(bits(per[1, :lens[1]]), bits(CH.MuLawQuantization()(inputs()[1].cuda(), 8)))
    assert torch.equal(bits(CH.Quantization()(inputs()[2].cuda(), Q)), bits(uni[2, :lens[2]]))


# ------------------------------------------------------------------------------------------------ the entry points themselves
def test_entry_points_keep_the_sentinel_outside_the_written_region():
    lib = load()
    x, lens = padded(inputs()[:2], extra=0)
    B, L = x.shape
    d_lens, h_lens = clips.lens_args(lens, L, x.device)
    half = 1200                                          # longer than the first clip
    pad = torch.full((B, L + 2 * half + 6), 5.0, device="cuda")
    check(lib.mmx_pad_edge_rows(_p(x), i64(L), L, B, _p(d_lens), h_lens, half, _p(pad), i64(pad.shape[1]), stream()), "mmx_pad_edge_rows")
    assert (pad[:, L + 2 * half:] == 5.0).all()
    for b, w in enumerate(inputs()[:2]):
        n = lens[b]
        want = torch.cat([w[:1].expand(half), w, w[-1:].expand(half)])
        assert torch.equal(bits(pad[b, :n + 2 * half].cpu()), bits(want)) and not pad[b, n + 2 * half:L + 2 * half].any()
    R = 3
    ranks = [0, lens[0] - 1, 7, 1, lens[1] // 2, lens[1] - 1]
    vals, flag = torch.full((B * R + 2,), 5.0, device="cuda"), torch.full((B + 1,), 5, dtype=torch.int32, device="cuda")
    work = torch.full((B * R * CH.SELECT_WORK + 4,), 5, dtype=torch.int32, device="cuda")
    check(lib.mmx_row_select(_p(x), i64(L), L, B, _p(d_lens), h_lens, _p(torch.tensor(ranks, dtype=torch.int32, device="cuda")),
                             (C.c_int32 * 6)(*ranks), R, _p(vals), _p(flag), _p(work), stream()), "mmx_row_select")
    assert (vals[B * R:] == 5.0).all() and flag.tolist() == [0, 0, 5] and (work[B * R * CH.SELECT_WORK:] == 5).all()
    for b, w in enumerate(inputs()[:2]):
        assert torch.equal(vals[b * R:(b + 1) * R].cpu(), torch.sort(w).values[ranks[b * R:(b + 1) * R]])
    hist = work[:B * R * CH.SELECT_WORK].reshape(B, R, CH.SELECT_WORK)[:, :, :1024].reshape(B, R, 4, 256).sum(-1)
    assert (hist[:, :, 0].cpu() == torch.tensor(lens)[:, None]).all() and (hist[:, :, 3] >= 1).all()      # pass 0 counts every sample
    stats = torch.tensor([[-0.1, -0.1, 0.2, 0.3], [-0.3, -0.2, 0.1, 0.1]], device="cuda")
    w = torch.tensor([[0.0, 0.5], [0.25, 0.0]], dtype=torch.float64, device="cuda")
    thr, out = torch.full((B * 2 + 2,), 5.0, device="cuda"), torch.full((B, L + 3), 5.0, device="cuda")
    check(lib.mmx_clip_rows(_p(x), i64(L), L, B, _p(d_lens), h_lens, _p(stats), _p(w), _p(flag), _p(thr), _p(out), i64(L + 3), stream()),
          "mmx_clip_rows")
    s64 = stats.cpu().double().numpy()
    want = [float(np.float32(s64[b, 2 * k] + (s64[b, 2 * k + 1] - s64[b, 2 * k]) * float(w[b, k]))) for b in range(B) for k in range(2)]
    assert thr.tolist() == want + [5.0, 5.0] and (out[:, L:] == 5.0).all()
    for b, wv in enumerate(inputs()[:2]):
        assert torch.equal(bits(out[b, :lens[b]].cpu()), bits(wv.clamp(thr[2 * b].cpu(), thr[2 * b + 1].cpu()))) and not out[b, lens[b]:L].any()
    q = [256, 8]
    out = torch.full((B, L + 3), 5.0, device="cuda")
    for mode, fn in ((0, CH.quantization), (1, CH.mulaw_quantization)):
        check(lib.mmx_quantize_rows(_p(x), i64(L), L, B, _p(d_lens), h_lens, mode, _p(torch.tensor(q, dtype=torch.int32, device="cuda")),
                                    (C.c_int32 * 2)(*q), _p(out), i64(L + 3), stream()), "mmx_quantize_rows")
        assert (out[:, L:] == 5.0).all() and not out[0, lens[0]:L].any()
        assert torch.equal(bits(out[1, :lens[1]]), bits(fn(inputs()[1].cuda(), 8)))


def test_refusals_leave_the_outputs_untouched():
    lib, dev = load(), "cuda"
    L = 600
    x = GD.clip(L, 3).cuda()[None]
    out = torch.full((1, L + 200), 5.0, device=dev)
    one = lambda v: (torch.tensor([v], dtype=torch.int32, device=dev), (C.c_int32 * 1)(v))
    pad = lambda half, lens=None, h_lens=None, o_bs=L + 200: lib.mmx_pad_edge_rows(_p(x), i64(L), L, 1, _p(lens), h_lens, half, _p(out), i64(o_bs), stream())
    assert pad(-1) == -1 and pad(101) == -1 and pad(4, *one(0)) == -1 and pad(4, *one(L + 1)) == -1 and pad(4, one(5)[0], None) == -1
    vals, flag = torch.full((4,), 5.0, device=dev), torch.full((1,), 5, dtype=torch.int32, device=dev)
    work = torch.full((4 * CH.SELECT_WORK,), 5, dtype=torch.int32, device=dev)
    sel = lambda ranks, R, lens=None, h_lens=None: lib.mmx_row_select(
        _p(x), i64(L), L, 1, _p(lens), h_lens, _p(torch.tensor(ranks, dtype=torch.int32, device=dev)), (C.c_int32 * len(ranks))(*ranks), R,
        _p(vals), _p(flag), _p(work), stream())
    assert sel([0, L], 2) == -1 and sel([-1], 1) == -1 and sel([0] * 5, 5) == -1 and sel([0], 0) == -1 and sel([7], 1, *one(7)) == -1
    assert sel([0], 1, *one(0)) == -1
    stats, w = torch.zeros(1, 4, device=dev), torch.zeros(1, 2, dtype=torch.float64, device=dev)
    thr, zero = torch.full((2,), 5.0, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    clp = lambda lens=None, h_lens=None, o_bs=L + 200: lib.mmx_clip_rows(_p(x), i64(L), L, 1, _p(lens), h_lens, _p(stats), _p(w), _p(zero), _p(thr),
                                                                         _p(out), i64(o_bs), stream())
    assert clp(*one(0)) == -1 and clp(one(5)[0], None) == -1 and clp(o_bs=L - 1) == -1
    qz = lambda mode, q, o_bs=L + 200: lib.mmx_quantize_rows(_p(x), i64(L), L, 1, None, None, mode, _p(one(q)[0]), one(q)[1], _p(out), i64(o_bs), stream())
    assert qz(0, 1) == -1 and qz(1, 0) == -1 and qz(2, 256) == -1 and qz(0, 256, o_bs=L - 1) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 and float(vals.min()) == 5.0 and int(flag) == 5 and int(work.min()) == 5 and float(thr.min()) == 5.0
    w = x[0]
    for call, word in ((lambda: CH.low_pass(w, 12001, RATE), "cutoff"), (lambda: CH.high_pass(w, 0.0, RATE), "cutoff"),
                       (lambda: CH.low_pass(w, 10.0, RATE), "taps"), (lambda: CH.equalizer(w, [0.0], RATE), "bands"),
                       (lambda: CH.mel_filterbank(w, 1, RATE), "bands"), (lambda: CH.clip_distortion(w, 1.01), "percentile"),
                       (lambda: CH.quantization(w, 1), "channels"), (lambda: CH.mulaw_quantization([w, w], [256, 1]), "channels"),
                       (lambda: CH.low_pass([w, w[:0]], 4000, RATE), "empty clip")):
        with pytest.raises(MmxError, match=word):
            call()


# ------------------------------------------------------------------------------------------------ mmx.degrade, the engine keyword
def test_ir_eq_and_noise_eq_are_equalize_then_call():
    xs = [GD.clip(n, 20 + i).cuda() for i, n in enumerate((9000, 12000))]
    hs = [GD.ir(900, 40, 1).cuda(), GD.ir(1500, 0, 2).cuda()]
    ns = [(0.05 * GD.clip(n, 30 + i)).cuda() for i, n in enumerate((5000, 20000))]          # shorter, longer
    curves = CURVES[3][:2]
    got = D.apply_ir(xs, hs, RATE, drr=[None, 5.0], ir_eq=curves)
    want = D.apply_ir(xs, CH.equalizer(hs, curves, RATE), RATE, drr=[None, 5.0])
    plain = D.apply_ir(xs, hs, RATE, drr=[None, 5.0])
    for b in range(2):
        assert torch.equal(bits(got[b]), bits(want[b])) and not torch.equal(bits(got[b]), bits(plain[b]))
        assert torch.equal(bits(D.apply_ir(xs[b], hs[b], RATE, drr=[None, 5.0][b], ir_eq=curves[b])), bits(got[b]))
    assert torch.equal(bits(D.RoomImpulseResponse(RATE)(xs[0], hs[0], eq=curves[0])), bits(got[0]))
    got = D.mix(xs, ns, RATE, snr=[5.0, 12.0], noise_eq=curves)
    fitted = []
    for x, n in zip(xs, ns):
        f = torch.zeros_like(x)
        m = min(x.numel(), n.numel())
        f[:m] = n[:m]
        fitted.append(f)
    want = D.mix(xs, CH.equalizer(fitted, curves, RATE), RATE, snr=[5.0, 12.0])
    plain = D.mix(xs, ns, RATE, snr=[5.0, 12.0])
    for b in range(2):
        assert torch.equal(bits(got[b]), bits(want[b])) and not torch.equal(bits(got[b]), bits(plain[b]))
    assert torch.equal(bits(D.BackgroundNoise(RATE)(xs[1], ns[1], snr=12.0, eq=curves[1])), bits(got[1]))


def everything():
    room, fan = GD.ir(3000, 40, 1).cuda(), (0.1 * GD.clip(20000, 8)).cuda()
    return {"ir": room, "drr": 5.0, "wrap": False, "ir_eq": CURVES[3][0], "noise": fan, "snr": 12.0, "noise_eq": CURVES[6][1],
            "low_pass": 7000.0, "high_pass": 100.0, "eq": CURVES[6][0], "clip": 0.05, "quantize": 4096, "mulaw": 256}


def by_hand(w, o):
    y = D.apply_ir(w, o["ir"], RATE, drr=o["drr"], wrap=o["wrap"], ir_eq=o["ir_eq"])
    y = D.mix(y, o["noise"], RATE, snr=o["snr"], noise_eq=o["noise_eq"])
    y = CH.high_pass(CH.low_pass(y, o["low_pass"], RATE), o["high_pass"], RATE)
    y = CH.clip_distortion(CH.equalizer(y, o["eq"], RATE), o["clip"])
    return CH.mulaw_quantization(CH.quantization(y, o["quantize"]), o["mulaw"])


def test_prompt_from_clip_degrade_with_every_key(eng):
    w = GD.clip(31200, 7).cuda()                          # 1.3 s at 24 kHz
    ptext = torch.randint(0, 151936, (1, 4), generator=torch.Generator().manual_seed(1)).cuda()
    opts = everything()
    got = eng.prompt_from_clip(w, RATE, ptext, generator=GD._gen(), degrade=opts)
    GD._same(got, eng.prompt_from_clip(by_hand(w, opts), RATE, ptext, generator=GD._gen()))
    plain = eng.prompt_from_clip(w, RATE, ptext, generator=GD._gen())
    assert not torch.equal(got["prompt_speech_feat"], plain["prompt_speech_feat"])
    only = eng.prompt_from_clip(w, RATE, ptext, generator=GD._gen(), degrade={"mulaw": 256})
    GD._same(only, eng.prompt_from_clip(CH.mulaw_quantization(w, 256), RATE, ptext, generator=GD._gen()))
    for bad in ({"snr": 3.0}, {"ir_eq": [0.0, -1.0], "low_pass": 4000.0}, {"noise_eq": [0.0, -1.0], "clip": 0.1}, {"low_pass": 4000.0, "order": 3}):
        with pytest.raises(ValueError, match="degrade"):
            eng.prompt_from_clip(w, RATE, ptext, degrade=bad)


def test_prompts_from_clips_degrade_with_every_key(eng):
    from mmx.resample import Resample
    ws = [GD.clip(31200, 7).cuda(), GD.clip(28800, 8).cuda(), GD.clip(36000, 9).cuda()]
    rates = [RATE] * 3
    full = everything()
    other = dict(full, low_pass=3400.0, eq=CURVES[6][2], clip=0.2, mulaw=64)                  # same keys, other values: one group
    dg = [full, {"low_pass": 3400.0, "quantize": 256}, other]
    g = torch.Generator().manual_seed(4)
    n24 = [Resample(16000, RATE).out_len(Resample(r, 16000).out_len(c.numel())) for c, r in zip(ws, rates)]
    noises = [torch.randn(80, eng.dacenc.frames(v), generator=g).cuda() for v in n24]
    bulk = eng.prompts_from_clips(ws, rates, noises=noises, degrade=dg)
    hand = [by_hand(ws[0], full), CH.quantization(CH.low_pass(ws[1], 3400.0, RATE), 256), by_hand(ws[2], other)]
    for i in range(3):
        GD._same(bulk[i], eng.prompt_from_clip(ws[i], rates[i], noise=noises[i][None], degrade=dg[i]))
        GD._same(bulk[i], eng.prompt_from_clip(hand[i], rates[i], noise=noises[i][None]))
