"""Room and noise simulation on the device (csrc/degrade.hip mmx_ir_prepare / mmx_fir_rows / mmx_row_absmax / mmx_mix_rows,
mmx/degrade.py) against the float64 restatement of tests/test_degrade_host.py, then the engine keyword built on it
(TtsEngine.prompt_from_clip / prompts_from_clips, degrade=).

Shapes, B = 3 ragged, chosen to cross every boundary fir_rows_kernel has: clips of 1000 samples (4 of a workgroup's 16 row tiles
live, one per wave, the last partial), NOUT + 3 (a second workgroup with 3 outputs) and 2 NOUT + 517 (three workgroups, the last
with three row tiles: one wave idle); impulse responses of 1 tap (K = 32: one step, the prefetch runs past the end at once), 31 and
33 taps (46 / 48 columns: one and two steps), CHUNK_TAPS + 17 (two K chunks, the second of two steps) and 1500 and CHUNK_TAPS + 17
taps against the 1000-sample clip (L > N: truncated, once with the IR's own peak cut away); the peak at tap 0, in the middle and at
the last tap; wrap and no wrap.  The batch goes in as a padded tensor whose columns past each clip's length hold NaN: a finite
result proves that nothing past `lens` was read.

Parity bound (the convention of tests/test_gpu_kv_parity.py for fp32-grade kernels): per clip
    max |y - y64| / max |y64| <= max(4 * base, 1e-6),
y64 the float64 restatement, base the same restatement run in float32 against float64 on the same inputs.  Measured on an MI355X:
see DESIGN.md (room and noise simulation)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import test_degrade_host as H
import test_s3tok_host as S3
from mmx import clips, degrade as D

pytestmark = pytest.mark.gpu

NS = (1000, D.NOUT + 3, 2 * D.NOUT + 517)
LONG = D.CHUNK_TAPS + 17
# name -> per clip (taps, peak index)
CASES = {
    "short": ((1, 0), (31, 15), (33, 32)),
    "chunks": ((LONG, 500), (LONG, 0), (LONG, LONG - 1)),
    "mixed": ((1500, 1200), (33, 0), (LONG, 2000)),
}


def bits(t):
    return t.contiguous().view(torch.int32)


def clip(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    return (0.2 * torch.randn(n, generator=g, dtype=torch.float64) * (1.0 + 0.5 * torch.sin(2 * np.pi * t / 700.0))).float()


def ir(taps, peak, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    h = 0.3 * torch.randn(taps, generator=g, dtype=torch.float64) * torch.exp(-3.0 * torch.arange(taps, dtype=torch.float64) / taps)
    h[peak] = 1.0 if seed % 2 else -1.0
    return h.float()


@functools.lru_cache(None)
def inputs(case):
    return [clip(n, 10 + i) for i, n in enumerate(NS)], [ir(t, p, i) for i, (t, p) in enumerate(CASES[case])]


def padded(xs, extra=7):
    lens = [int(x.numel()) for x in xs]
    t = torch.full((len(xs), max(lens) + extra), float("nan"))
    for b, x in enumerate(xs):
        t[b, :lens[b]] = x
    return t.cuda(), lens


def ref_causal(x, h, start_at_max=True, dtype=torch.float64):
    """The restatement's route (test_degrade_host.ref_convolve: truncate, rfft / irfft, the delta's scale) for wrap=False: the
    product taken at a length that holds the whole linear convolution, read from the peak on."""
    x, h = torch.as_tensor(x).to(dtype).reshape(-1), torch.as_tensor(h).to(dtype).reshape(-1)[:x.numel()]
    N, p = x.numel(), (int(h.abs().argmax()) if start_at_max else 0)
    length = N + h.numel()
    full = torch.fft.irfft(torch.fft.rfft(h, length) * torch.fft.rfft(x, length), length)
    return full[p:p + N] * (1 / h.abs().max().clamp(1e-5))


@functools.lru_cache(None)
def reference(case, wrap, start_at_max=True):
    """(y64, base) per clip, computed once."""
    xs, hs = inputs(case)
    fn = H.ref_convolve if wrap else ref_causal
    out = []
    for x, h in zip(xs, hs):
        y64 = fn(x, h, start_at_max)
        out.append((y64, H.rel_err(fn(x, h, start_at_max, dtype=torch.float32), y64)))
    return out


@functools.lru_cache(None)
def device(case, wrap, start_at_max=True):
    xs, hs = inputs(case)
    batch, lens = padded(xs)
    hb, hl = padded(hs, extra=3)
    out = D.convolve(batch, hb, lens=lens, ir_lens=hl, start_at_max=start_at_max, wrap=wrap)
    torch.cuda.synchronize()
    return out, lens


def test_restatement_of_the_causal_route_is_the_index_definition():
    x, h = clip(300, 1), ir(77, 20, 1)
    assert H.rel_err(ref_causal(x, h), D.convolve_host(x.numpy(), h.numpy(), wrap=False)) < 1e-12
    assert H.rel_err(ref_causal(x[:50], h), D.convolve_host(x[:50].numpy(), h.numpy(), wrap=False)) < 1e-12


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("case", list(CASES))
def test_convolve_parity(case, wrap):
    out, lens = device(case, wrap)
    assert out.shape == (3, max(lens) + 7)
    worst = 0.0
    for b, (y64, base) in enumerate(reference(case, wrap)):
        y = out[b, :lens[b]].cpu()
        assert torch.isfinite(y).all()
        err, bound = H.rel_err(y, y64), max(4 * base, 1e-6)
        worst = max(worst, err / bound)
        print(f"{case} wrap={wrap} clip {b}: N {lens[b]} taps {CASES[case][b][0]} err {err:.3e} base {base:.3e} bound {bound:.3e}")
        assert err <= bound, (case, wrap, b, err, bound)
        assert not out[b, lens[b]:].any()                # tail columns are zeros
    print(f"{case} wrap={wrap}: worst err / bound {worst:.3f}")


def test_convolve_without_start_at_max():
    out, lens = device("mixed", True, False)
    for b, (y64, base) in enumerate(reference("mixed", True, False)):
        err = H.rel_err(out[b, :lens[b]].cpu(), y64)
        print(f"start_at_max=False clip {b}: err {err:.3e} base {base:.3e}")
        assert err <= max(4 * base, 1e-6)


@pytest.mark.parametrize("wrap", [True, False])
def test_batched_equals_solo_bit_for_bit(wrap):
    xs, hs = inputs("mixed")
    out, lens = device("mixed", wrap)
    listed = D.convolve([x.cuda() for x in xs], [h.cuda() for h in hs], wrap=wrap)
    for b in range(3):
        solo = D.convolve(xs[b].cuda(), hs[b].cuda(), wrap=wrap)
        assert solo.shape == (lens[b],)
        assert torch.equal(bits(solo), bits(out[b, :lens[b]])) and torch.equal(bits(solo), bits(listed[b]))
    # one IR for all clips: each row is that clip's solo call with it
    shared = D.convolve([x.cuda() for x in xs], hs[2].cuda(), wrap=wrap)
    for b in range(3):
        assert torch.equal(bits(shared[b]), bits(D.convolve(xs[b].cuda(), hs[2].cuda(), wrap=wrap)))


def test_entry_points_keep_the_sentinel_outside_the_written_region():
    from mmx._lib import check, i64, load, stream, _p
    xs, hs = inputs("short")
    x, lens = padded(xs, extra=0)
    B, L = x.shape
    prep = D._prepare([h.cuda() for h in hs], None, lens, None, None, True, "test")
    out = torch.full((B, L + 9), 5.0, device="cuda")
    peak = torch.full((B + 2,), 5.0, device="cuda")
    d_lens, h_lens = clips.lens_args(lens, L, x.device)
    check(load().mmx_fir_rows(_p(x), i64(L), L, B, _p(d_lens), h_lens, _p(prep["table"]), prep["kcap"], _p(prep["p"]), _p(prep["s"]),
                              _p(prep["taps"]), 1, _p(out), i64(L + 9), _p(peak), stream()), "mmx_fir_rows")
    torch.cuda.synchronize()
    want, _ = device("short", True)
    assert (out[:, L:] == 5.0).all() and (peak[B:] == 5.0).all()
    for b in range(B):
        assert torch.equal(bits(out[b, :lens[b]]), bits(want[b, :lens[b]])) and not out[b, lens[b]:L].any()
        assert float(peak[b]) == float(out[b, :lens[b]].abs().max())
    before = torch.full((B + 1,), 5.0, device="cuda")
    check(load().mmx_row_absmax(_p(x), i64(L), L, B, _p(d_lens), _p(before), stream()), "mmx_row_absmax")
    assert [float(v) for v in before[:B]] == [float(v.abs().max()) for v in xs] and float(before[B]) == 5.0
    assert [int(v) for v in prep["taps"]] == [1, 31, 33] and [int(v) for v in prep["p"]] == [0, 15, 32]
    for b, h in enumerate(hs):                           # the device's table is the host builder's
        got = prep["table"][b].reshape(3, -1, 64, 8).cpu()
        assert torch.equal(got.view(torch.int16), D.pack_table(h.numpy(), h.numel(), prep["kcap"]).view(torch.int16))


def test_entry_points_refuse_before_any_launch():
    """The C entry points' own checks (MMX_EARG = -1) with valid pointers: outputs stay untouched."""
    from mmx._lib import i64, load, stream, _p
    lib, dev = load(), "cuda"
    L, Lir = 600, D.MAX_TAPS + 1
    x = clip(L, 3).cuda()[None]
    prep = D._prepare([ir(40, 3, 1).cuda()], None, [L], None, None, True, "test")
    out, peak = torch.full((1, L), 5.0, device=dev), torch.full((1,), 5.0, device=dev)
    one = lambda v: (torch.tensor([v], dtype=torch.int32, device=dev), (C.c_int32 * 1)(v))
    fir = lambda kcap, wrap, lens=None, h_lens=None, o_bs=L: lib.mmx_fir_rows(
        _p(x), i64(L), L, 1, _p(lens), h_lens, _p(prep["table"]), kcap, _p(prep["p"]), _p(prep["s"]), _p(prep["taps"]), wrap, _p(out),
        i64(o_bs), _p(peak), stream())
    k = prep["kcap"]
    assert fir(k + 1, 1) == -1 and fir(0, 1) == -1 and fir(D.padded_taps(D.MAX_TAPS) + 32, 1) == -1 and fir(k, 2) == -1
    assert fir(k, 1, *one(0)) == -1 and fir(k, 1, *one(L + 1)) == -1 and fir(k, 1, one(5)[0], None) == -1 and fir(k, 1, o_bs=L - 1) == -1
    big = torch.zeros(1, Lir, device=dev)
    hann = torch.zeros(1, 1, dtype=torch.float64, device=dev)
    h_out = torch.full((1, Lir), 5.0, device=dev)
    p, s, taps, drr = (torch.full((1,), 5, dtype=torch.int32, device=dev), torch.full((1,), 5.0, device=dev),
                       torch.full((1,), 5, dtype=torch.int32, device=dev), torch.full((1,), 5.0, device=dev))
    table = torch.full((3 * 16 * D.padded_taps(Lir),), 5.0, dtype=torch.bfloat16, device=dev)
    prepare = lambda Lsig, kcap, il=None, h_il=None: lib.mmx_ir_prepare(
        _p(big), i64(Lir), Lir, 1, _p(il), h_il, Lsig, None, None, None, 0, _p(hann), 1, _p(h_out), i64(Lir), _p(p), _p(s), _p(taps),
        _p(drr), _p(table), kcap, stream())
    assert prepare(Lir + 5, D.padded_taps(Lir)) == -1                   # more than MAX_TAPS taps
    assert prepare(100, 64) == -1 and prepare(100, 130) == -1            # a table too small for 100 taps; not a multiple of 32
    assert prepare(100, 128, *one(0)) == -1                              # an empty impulse response
    torch.cuda.synchronize()
    assert float(out.min()) == 5.0 and float(peak) == 5.0 and float(h_out.min()) == 5.0 and float(table.float().min()) == 5.0
    assert int(p) == 5 and float(s) == 5.0 and int(taps) == 5 and float(drr) == 5.0
    with pytest.raises(D.MmxError, match="taps"):
        D.convolve(torch.zeros(D.MAX_TAPS + 8, device=dev), big[0])


# ------------------------------------------------------------------------------------------------ apply_ir, DRR
DRR_CASES = ((16000, 2000, 40, 10.0), (24000, 5000, 137, 0.0), (16000, 300, 25, -5.0))       # the last: the floor on alpha engages


def test_alter_and_measure_drr():
    """The device's alter_drr / measure_drr against the restatement.  IR taps: the parity bound above with base = one fp32 rounding
    (2^-24) -> 1e-6 of the IR's peak.  dB values: the fp32 result's half ulp below 32 dB (9.5e-7) plus what the fp32 rounding of the
    altered taps can move the energy ratio by (at most 4 * 2^-24 relative: 1.1e-6 dB) -> 1e-5 dB."""
    for rate in (16000, 24000):
        sel = [c for c in DRR_CASES if c[0] == rate]
        hs = [H.make_ir(r, L, pk).float() for r, L, pk, _ in sel]
        targets = [t for *_, t in sel]
        got = D.alter_drr([h.cuda() for h in hs], rate, targets)
        for h, t, g in zip(hs, targets, got):
            want = H.ref_alter_drr(h.double(), rate, t)
            err = H.rel_err(g.cpu(), want)
            m_dev, m_ref = float(D.measure_drr(g, rate)[0]), H.ref_measure_drr(g.cpu().double(), rate)
            print(f"alter_drr rate {rate} L {h.numel()} target {t}: taps err {err:.3e}; measured {m_dev:.6f} dB, restated {m_ref:.6f}, "
                  f"float64 IR {H.ref_measure_drr(want, rate):.6f}")
            assert err <= 1e-6
            assert abs(m_dev - m_ref) <= 1e-5 and abs(m_dev - H.ref_measure_drr(want, rate)) <= 1e-5
            assert (abs(m_dev - t) > 0.1) if t < 0 else (abs(m_dev - t) < 1e-3)
        plain = D.measure_drr([h.cuda() for h in hs], rate).cpu()
        for h, v in zip(hs, plain):
            assert abs(float(v) - H.ref_measure_drr(h.double(), rate)) <= 1e-5
    # None entries leave an IR as it is; a target with no real root gives NaN taps (documented, not checked on the device)
    h = H.make_ir(16000, 2000, 40).float().cuda()
    a, b = D.alter_drr([h, h], 16000, [None, -60.0])
    assert torch.equal(bits(a), bits(h)) and torch.isnan(b).all()


def test_apply_ir_keeps_the_input_peak():
    xs, hs = inputs("mixed")
    rate = 16000
    got = D.apply_ir([x.cuda() for x in xs], [h.cuda() for h in hs], rate, drr=[None, None, 10.0])
    for b, (x, h, y) in enumerate(zip(xs, hs, got)):
        want = H.ref_apply_ir(x, h.double(), rate, drr=(10.0 if b == 2 else None))
        peak_in, peak_out = float(x.abs().max()), float(y.abs().max())
        err = H.rel_err(y.cpu(), want)
        base = H.rel_err(H.ref_apply_ir(x, h.double(), rate, drr=(10.0 if b == 2 else None), dtype=torch.float32), want)
        print(f"apply_ir clip {b}: peak in {peak_in:.8f} out {peak_out:.8f}; err {err:.3e} base {base:.3e}")
        assert abs(peak_out - peak_in) <= 2.0 ** -22 * peak_in          # the quotient and the product: one fp32 rounding each
        assert err <= max(4 * base, 1e-6)
        solo = D.apply_ir(x.cuda(), h.cuda(), rate, drr=(10.0 if b == 2 else None))
        assert torch.equal(bits(solo), bits(y))
    mod = D.RoomImpulseResponse(rate)
    assert torch.equal(bits(mod(xs[1].cuda(), hs[1].cuda())), bits(got[1]))


# ------------------------------------------------------------------------------------------------ mix
def test_mix_against_the_restatement_and_the_snr():
    """The gain is exp(((Lx - snr) - Ln) ln 10 / 20) from the device's own loudness values, so the meter's tolerance is not counted
    again.  Bound: the two fp32 differences of values below 64 dB move the exponent by at most 2 * 2^-24 * 64 * 0.1151 = 8.8e-7,
    the fp32 gain and the fp32 product and sum add 3 * 2^-24 -> 1.1e-6 of the louder of clip and scaled noise; 2e-6 of max |mix|."""
    from mmx import loudness, metrics
    rate = 16000
    xs = [clip(n, 20 + i) for i, n in enumerate((9000, 12000, 16500))]
    ns = [0.05 * clip(n, 30 + i) for i, n in enumerate((5000, 20000, 16500))]         # shorter, longer, equal
    snrs = [5.0, 10.0, 20.0]
    dx, dn = [x.cuda() for x in xs], [n.cuda() for n in ns]
    got = D.mix(dx, dn, rate, snr=snrs)
    fitted = [H.ref_fit_noise(n, x.numel()).float().cuda() for x, n in zip(xs, ns)]
    lx, ln = loudness.integrated_loudness(dx, rate).cpu(), loudness.integrated_loudness(fitted, rate).cpu()
    for b in range(3):
        want = H.ref_mix(xs[b], ns[b], snrs[b], float(lx[b]), float(ln[b]))
        err = H.rel_err(got[b].cpu(), want)
        print(f"mix clip {b}: Lx {float(lx[b]):.3f} Ln {float(ln[b]):.3f} snr {snrs[b]} err {err:.3e}")
        assert got[b].shape == xs[b].shape and err <= 2e-6
        assert torch.equal(bits(D.mix(dx[b], dn[b], rate, snr=snrs[b])), bits(got[b]))          # solo
    assert torch.equal(got[0][5000:].cpu(), xs[0][5000:])                # past the short noise the clip is untouched
    lo, hi = D.mix(dx, dn, rate, snr=5.0), D.mix(dx, dn, rate, snr=15.0)
    d_lo, d_hi = metrics.waveform_distance(lo, dx)["snr_db"], metrics.waveform_distance(hi, dx)["snr_db"]
    print("snr_db at 5 / 15:", d_lo.tolist(), d_hi.tolist())
    assert ((d_hi - d_lo - 10.0).abs() <= 0.05).all()
    assert torch.equal(bits(D.BackgroundNoise(rate)(dx[1], dn[1], snr=10.0)), bits(got[1]))
    # the raw launch: noise lengths of its own, sentinel past the row
    from mmx._lib import check, i64, load, stream, _p
    x, lens = padded(xs[:2], extra=0)
    nz, nl = padded(ns[:2], extra=0)
    out = torch.full((2, x.shape[1] + 4), 5.0, device="cuda")
    d_lens, d_nl = torch.tensor(lens, dtype=torch.int32, device="cuda"), torch.tensor(nl, dtype=torch.int32, device="cuda")
    lx, ln, snr = (torch.tensor([v, v], dtype=torch.float32, device="cuda") for v in (-20.0, -30.0, 10.0))
    check(load().mmx_mix_rows(_p(x), i64(x.shape[1]), x.shape[1], 2, _p(d_lens), _p(nz), i64(nz.shape[1]), nz.shape[1], _p(d_nl), _p(lx),
                              _p(ln), _p(snr), _p(out), i64(out.shape[1]), stream()), "mmx_mix_rows")
    assert (out[:, x.shape[1]:] == 5.0).all() and not out[0, lens[0]:x.shape[1]].any() and torch.isfinite(out).all()
    assert torch.equal(out[0, :5000].cpu(), xs[0][:5000] + ns[0])        # gain exp(0) = 1
    assert torch.equal(out[1, :12000].cpu(), xs[1] + ns[1][:12000])


# ------------------------------------------------------------------------------------------------ the engine keyword
@pytest.fixture(scope="module")
def eng(golden_dir):
    """As tests/test_gpu_denoise.py: 2-layer LM, 1 mid block, synthetic DAC, the S3 fixture state, split build."""
    from mmx import shapes, synth
    from mmx.pipeline import TtsEngine
    z, _ = S3.load_fixture(golden_dir)
    llm_sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    flow_sd = synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1, use_speaker_encoder=True), 0)
    dac_sd = synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0)
    enc_sd = synth.synth_state_dict(shapes.dac_encoder_manifest(80), 0)
    e = TtsEngine(llm_sd, flow_sd, dac_sd, dtype=2, max_batch=1, max_ctx=256, s3tok_sd=S3.fixture_state(z, "bf16"), dacenc_sd=enc_sd)
    yield e
    e.close()


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k


def _gen():
    return torch.Generator(device="cuda").manual_seed(9)


def test_prompt_from_clip_degrade(eng, monkeypatch):
    w = clip(31200, 7).cuda()                             # 1.3 s at 24 kHz
    room, fan = ir(3000, 40, 1).cuda(), (0.1 * clip(20000, 8)).cuda()
    ptext = torch.randint(0, 151936, (1, 4), generator=torch.Generator().manual_seed(1)).cuda()
    plain = eng.prompt_from_clip(w, 24000, ptext, generator=_gen())
    with monkeypatch.context() as mp:                     # None: today's bits, nothing of this module is launched
        for name in ("apply_ir", "mix", "convolve"):
            mp.setattr(D, name, lambda *a, **k: pytest.fail("degrade=None reached mmx.degrade"))
        _same(eng.prompt_from_clip(w, 24000, ptext, generator=_gen(), degrade=None), plain)
    by_hand = D.mix([D.apply_ir(w, room, 24000, drr=5.0, wrap=False)], [fan], 24000, snr=12.0)[0]
    opts = {"ir": room, "drr": 5.0, "wrap": False, "noise": fan, "snr": 12.0}
    got = eng.prompt_from_clip(w, 24000, ptext, generator=_gen(), degrade=opts)
    _same(got, eng.prompt_from_clip(by_hand, 24000, ptext, generator=_gen()))
    assert not torch.equal(got["prompt_speech_feat"], plain["prompt_speech_feat"])
    # degrade first, then denoise, then level
    dn = {"noise": fan[:8000]}
    _same(eng.prompt_from_clip(w, 24000, ptext, generator=_gen(), degrade={"noise": fan}, denoise=dn, normalize_db=-20.0),
          eng.prompt_from_clip(D.mix(w, fan, 24000), 24000, ptext, generator=_gen(), denoise=dn, normalize_db=-20.0))
    with pytest.raises(ValueError, match="degrade"):
        eng.prompt_from_clip(w, 24000, ptext, degrade={"snr": 3.0})


def test_prompts_from_clips_degrade(eng):
    from mmx.resample import Resample
    clips = [clip(31200, 7).cuda(), clip(28800, 8).cuda(), clip(36000, 9).cuda().reshape(1, -1)]
    rates = [24000, 24000, 24000]
    room, fan = ir(3000, 40, 1).cuda(), (0.1 * clip(20000, 8)).cuda()
    dg = [{"ir": room, "drr": 5.0}, None, {"ir": room, "noise": fan, "snr": 8.0}]
    g = torch.Generator().manual_seed(4)
    n24 = [Resample(16000, 24000).out_len(Resample(r, 16000).out_len(c.numel())) for c, r in zip(clips, rates)]
    noises = [torch.randn(80, eng.dacenc.frames(v), generator=g).cuda() for v in n24]
    bulk = eng.prompts_from_clips(clips, rates, noises=noises, degrade=dg)
    for i in range(3):
        _same(bulk[i], eng.prompt_from_clip(clips[i], rates[i], noise=noises[i][None], degrade=dg[i]))
    one = eng.prompts_from_clips(clips[:2], rates[:2], noises=noises[:2], degrade={"noise": fan})
    for i in range(2):
        _same(one[i], eng.prompt_from_clip(clips[i], rates[i], noise=noises[i][None], degrade={"noise": fan}))
    with pytest.raises(ValueError):
        eng.prompts_from_clips(clips, rates, degrade=[None])
