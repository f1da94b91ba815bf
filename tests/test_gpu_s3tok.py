"""The S3 speech tokenizer on the device (csrc/s3tok.hip, mmx_logmel_w of csrc/mel.hip, mmx/s3tok.py) against float64: the
three kernels on their own, then the engine by the token rule (tests/test_s3tok_host.py).

Outputs sit in sentinel-guarded buffers, inputs that must not be read hold NaN, and whatever lies outside the written window is
compared bit for bit with a clone taken before the launch.  Every bound comes from the reference's own error, the number formats
or a CPU statement of the chain in fp32 - never from what the kernels return."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_s3tok_host as R

pytestmark = pytest.mark.gpu

GUARD = 64
NAN = float("nan")


def guarded(shape, dtype=torch.float32, fill=NAN):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), fill if dtype.is_floating_point else -12345, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def assert_guards(buf, what=""):
    b = buf.cpu()
    for g in (b[:GUARD], b[-GUARD:]):
        assert bool(torch.isnan(g).all() if g.is_floating_point() else (g == -12345).all()), f"{what}: wrote outside its output"


def bits(t):
    return t.contiguous().view(torch.int32)


def row_rel(got, ref):
    """Worst per-row relative error: max|got - ref| over a row / max|ref| of that row (rows of zeros: absolute)."""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    den = ref.abs().amax(dim=1)
    return float(((got - ref).abs().amax(dim=1) / torch.where(den > 0, den, torch.ones_like(den))).max())


@pytest.fixture(scope="module")
def fix(golden_dir):
    z, names = R.load_fixture(golden_dir)
    return z, names


# ------------------------------------------------------------------------------------------------ mmx_logmel_w
def test_logmel_w_parity_with_float64(fix):
    """Per clip max|kernel - f64| <= 4 * max(e_ref, 1e-6), e_ref = max|reference fp32 - f64| (the rule of test_gpu_mel.py).
    Measured on an MI355X, e_gpu / e_ref: noise 3.1e-6 / 4.3e-6, tiny 1.7e-6 / 9.8e-7, voiced 8.7e-6 / 5.0e-6,
    gap 2.6e-6 / 2.9e-6."""
    from mmx.s3tok import LogMelW
    z, names = fix
    m = LogMelW()
    assert (m.bin0, m.n_bins) == (1, 199)
    for n in names:
        w = torch.from_numpy(z["wave_" + n]).cuda()
        got = m(w)
        r64 = z["mel64_" + n]
        assert got.dtype == torch.float32 and tuple(got.shape) == (1,) + r64.shape
        e_gpu = np.abs(got[0].cpu().numpy().astype(np.float64) - r64).max()
        e_ref = np.abs(z["mel32_" + n].astype(np.float64) - r64).max()
        print(f"\nlogmel_w {n}: e_gpu {e_gpu:.3e}  e_ref {e_ref:.3e}  ratio {e_gpu / max(e_ref, 1e-6):.2f}")
        assert e_gpu <= 4 * max(e_ref, 1e-6), (n, e_gpu, e_ref)
        assert torch.equal(m(w, time_major=True)[0], got[0].t())


def test_logmel_w_zero_padded_batch_equals_solo_runs(fix):
    """All fixture clips (the 360-sample one and the floor-binding one among them) in one launch, NaN behind every member's
    samples: each member bit-identical to its solo run, frames past its length exactly 0, nothing written outside the outputs."""
    from mmx import _lib as L
    from mmx.s3tok import LogMelW
    import ctypes as C
    z, names = fix
    assert "tiny" in names and "gap" in names
    m = LogMelW()
    waves = [torch.from_numpy(z["wave_" + n]).cuda() for n in names]
    lens = [w.numel() for w in waves]
    B, Lm = len(waves), max(lens)
    batch = torch.full((B, Lm), NAN, device="cuda")
    for i, w in enumerate(waves):
        batch[i, :lens[i]] = w
    T = max(n // 160 for n in lens)
    ldo = T + 3
    bcm, cm = guarded((B, 128, ldo))
    btm, tm = guarded((B, T, 128))
    before = cm.clone()
    d_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
    L.check(L.load().mmx_logmel_w(L._p(batch), L.i64(Lm), Lm, B, L._p(d_lens), (C.c_int32 * B)(*lens), L._p(m.basis), L._p(m.filt), 400, 160,
                                  m.bin0, m.n_bins, 128, L._p(cm), L.i64(ldo), L._p(tm), T, 0, L.stream()), "mmx_logmel_w")
    torch.cuda.synchronize()
    assert_guards(bcm, "out_cm")
    assert_guards(btm, "out_tm")
    assert torch.equal(bits(cm[:, :, T:]), bits(before[:, :, T:]))                  # the pitch's tail is not touched
    for i, w in enumerate(waves):
        Tb = lens[i] // 160
        solo = m(w)
        assert torch.equal(cm[i, :, :Tb], solo[0]), names[i]
        assert bool((cm[i, :, Tb:T] == 0).all()) and bool((tm[i, Tb:] == 0).all()), names[i]
        assert torch.equal(tm[i], cm[i, :, :T].t()), names[i]
    got = m(torch.nan_to_num(batch), lens=lens)
    assert torch.equal(got, cm[:, :, :T])


def test_logmel_w_refuses_a_member_without_reflection():
    from mmx._lib import MmxError
    from mmx.s3tok import LogMelW
    m = LogMelW()
    with pytest.raises(MmxError, match="code -1"):
        m(torch.zeros(1, 200, device="cuda"))
    assert tuple(m(torch.zeros(1, 201, device="cuda")).shape) == (1, 128, 1)


# ------------------------------------------------------------------------------------------------ mmx_s3_rope_fsmn
def _rope_fsmn_case(C_, B, T, lens, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3 * C_, generator=g)
    x = torch.randn(B, T, C_, generator=g)
    w = torch.randn(C_, 1, 31, generator=g) * 0.2
    return qkv, x, w


def _rope_fsmn_ref(qkv, x, w, lens, dtype):
    B, T, C3 = qkv.shape
    C_, H = C3 // 3, C3 // 192
    cos, sin = (t[:T].to(dtype) for t in R.rope_tables())
    q, k, v = (t.to(dtype) for t in qkv.split(C_, dim=-1))
    m = R.valid_rows(lens, T).to(dtype)[:, :, None]
    v = torch.nan_to_num(v) * m                                                     # a padding row's v is never read
    qo = R.rope_ref(q.view(B, T, H, 64), cos, sin).reshape(B, T, C_) * m
    ko = R.rope_ref(k.view(B, T, H, 64), cos, sin).reshape(B, T, C_) * m
    return qo, ko, x.to(dtype) + R.fsmn_ref(v, m, w.to(dtype))


def _run_rope_fsmn(qkv, x, w, lens):
    from mmx import s3tok
    B, T, C3 = qkv.shape
    C_ = C3 // 3
    bq, dq = guarded((B, T, C3))
    br, dr = guarded((B, T, C_))
    dq.copy_(qkv)
    cos, sin = (t.cuda() for t in s3tok.rope_tables())
    s3tok.s3_rope_fsmn(dq, x.cuda(), dr, w[:, 0, :].t().contiguous().cuda(), cos, sin, B=B, T=T, C_=C_,
                       lens=torch.tensor(lens, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert_guards(bq, "qkv")
    assert_guards(br, "r")
    return dq.cpu(), dr.cpu()


@pytest.mark.parametrize("C_", [128, 1280])
@pytest.mark.parametrize("B,T,lens", [(1, 1, [1]), (1, 14, [14]), (1, 33, [33]), (3, 50, [50, 14, 25])])
def test_rope_fsmn_parity_with_float64(C_, B, T, lens):
    """q, k, r against float64 on the operands as read, per row relative: max(4 * the fp32 torch statement's error, 1e-6).
    Padding rows: r is the residual row bit for bit, q / k are zero; v is left alone; a member equals its solo bits; NaN in a
    padding row's v changes nothing.  Measured on an MI355X (C 1280, (3, 50)): q 7.3e-8, k 7.1e-8, r 1.6e-7; the fp32 torch
    statement 7.8e-8 / 7.4e-8 / 1.6e-7."""
    qkv, x, w = _rope_fsmn_case(C_, B, T, lens, 100 + C_ + T)
    ref = _rope_fsmn_ref(qkv, x, w, lens, torch.float64)
    st = _rope_fsmn_ref(qkv, x, w, lens, torch.float32)
    got_qkv, got_r = _run_rope_fsmn(qkv, x, w, lens)
    assert torch.equal(bits(got_qkv[:, :, 2 * C_:]), bits(qkv[:, :, 2 * C_:]))      # v is not written
    valid = R.valid_rows(lens, T)
    for name, got, r64, s32 in (("q", got_qkv[:, :, :C_], ref[0], st[0]), ("k", got_qkv[:, :, C_:2 * C_], ref[1], st[1]), ("r", got_r, ref[2], st[2])):
        e, e32 = row_rel(got[valid], r64[valid]), row_rel(s32[valid], r64[valid])
        print(f"\nrope_fsmn C {C_} ({B}, {T}) {name}: e_gpu {e:.3e}  fp32 statement {e32:.3e}")
        assert e <= max(4 * e32, 1e-6), (name, e, e32)
    assert torch.equal(bits(got_r[~valid]), bits(x[~valid]))
    assert bool((got_qkv[:, :, :2 * C_][~valid] == 0).all())
    if B > 1:
        nan_qkv = qkv.clone()
        nan_qkv[:, :, 2 * C_:][~valid] = NAN
        q2, r2 = _run_rope_fsmn(nan_qkv, x, w, lens)
        assert torch.equal(bits(q2[:, :, :2 * C_]), bits(got_qkv[:, :, :2 * C_])) and torch.equal(bits(r2), bits(got_r))
        for i, n in enumerate(lens):
            qs, rs = _run_rope_fsmn(qkv[i:i + 1, :n].contiguous(), x[i:i + 1, :n].contiguous(), w, [n])
            assert torch.equal(bits(qs[0]), bits(got_qkv[i, :n])) and torch.equal(bits(rs[0]), bits(got_r[i, :n])), i


# ------------------------------------------------------------------------------------------------ mmx_fsq_encode
def _run_fsq(x, W, b, lens):
    from mmx import s3tok
    B, T, C_ = x.shape
    bi, ids = guarded((B, T), torch.int32)
    bp, pre = guarded((B, T, 8))
    s3tok.fsq_encode(x.cuda(), W.cuda(), b.cuda(), ids, B=B, T=T, C_=C_, lens=torch.tensor(lens, dtype=torch.int32, device="cuda"), pre=pre)
    torch.cuda.synchronize()
    assert_guards(bi, "ids")
    assert_guards(bp, "pre")
    return ids.cpu(), pre.cpu()


@pytest.mark.parametrize("C_", [256, 1280])
@pytest.mark.parametrize("B,T,lens", [(1, 1, [1]), (1, 14, [14]), (3, 50, [50, 14, 25])])
def test_fsq_encode_token_rule(C_, B, T, lens):
    """Digits by the token rule against float64, pre-round values within the bound, ids past code_len 0.  bound =
    max(4 * (torch's fp32 statement against float64), 4e-6): the fp32 floor of the token rule with nothing but the number format.
    Measured on an MI355X (C 1280, (3, 50)): pre-round error 2.7e-7, the fp32 statement 8.5e-7, bound 4e-6, 0 undecided digits."""
    g = torch.Generator().manual_seed(7 + C_ + T)
    x = torch.randn(B, T, C_, generator=g)
    W = torch.randn(8, C_, generator=g) / C_ ** 0.5
    b = torch.randn(8, generator=g) * 0.2
    v64 = torch.tanh(F.linear(x.double(), W.double(), b.double())) * R.FSQ_SCALE
    v32 = torch.tanh(F.linear(x, W, b)) * R.FSQ_SCALE
    valid = R.valid_rows(lens, T)
    base = float((v32.double() - v64).abs()[valid].max())
    bound = max(4 * base, 4e-6)
    assert bound <= 1e-3
    ids, pre = _run_fsq(x, W, b, lens)
    e = float((pre.double() - v64).abs()[valid].max())
    wrong, undecided = R.token_rule(R.id_digits(ids), v64, bound, valid)
    print(f"\nfsq C {C_} ({B}, {T}): e_gpu {e:.3e}  fp32 statement {base:.3e}  bound {bound:.1e}  undecided {undecided:.2%}")
    assert e <= bound and wrong == 0 and undecided <= 0.02
    assert torch.equal(R.ids_of(R.digits_of(pre)).int()[valid], ids[valid])         # the ids are the kernel's own values, rounded
    assert bool((ids[~valid] == 0).all()) and bool((pre[~valid] == 0).all())
    assert int(ids.min()) >= 0 and int(ids.max()) < 6561


def test_fsq_encode_rounds_half_to_even():
    """A sweep of fp32 neighbours of h = +-atanh(0.5 / 0.999) through digit 0 (W = e_0, no bias): wherever the kernel's own
    v = tanh(h) * 0.999 is exactly +-0.5 the digit is 1 (round half to even; half away from zero would give 2 / 0), and every
    digit is rint of the value the kernel reports."""
    C_ = 256
    h0 = torch.tensor(np.arctanh(0.5 / R.FSQ_SCALE), dtype=torch.float32)
    steps = torch.arange(-1024, 1024, dtype=torch.int32)
    h = (h0.view(torch.int32) + steps).view(torch.float32)
    h = torch.cat([h, -h])
    x = torch.zeros(1, h.numel(), C_)
    x[0, :, 0] = h
    W = torch.zeros(8, C_)
    W[0, 0] = 1.0
    ids, pre = _run_fsq(x, W, torch.zeros(8), [h.numel()])
    v = pre[0, :, 0]
    d0 = R.id_digits(ids)[0, :, 0]
    assert torch.equal(d0, R.digits_of(v)) and bool((R.id_digits(ids)[0, :, 1:] == 1).all())
    half = v.abs() == 0.5
    print(f"\nfsq half-to-even: {int(half.sum())} values exactly +-0.5 ({int((v == 0.5).sum())} positive)")
    assert int((v == 0.5).sum()) > 0 and int((v == -0.5).sum()) > 0
    assert bool((d0[half] == 1).all())
    assert set(d0.tolist()) == {0, 1, 2}


# ------------------------------------------------------------------------------------------------ engine
def _bound(sd, mel, lens, v64, h64, valid, build, e_ref, planes):
    """The token rule's bound for a build: max(4 * base, floor); base = a CPU statement of the chain in torch fp32 with the
    build's rounding wherever an activation (and, with weight planes, a weight) becomes a GEMM / attention operand, against
    float64; floor = 4 * max(e_ref, 1e-6) (fp32 build) or 4 * 2^-17 * max|h| (split build)."""
    with torch.no_grad():
        if build == "fp32":
            v32 = R.encode_ref(sd, mel, lens, torch.float32)[0]
            floor = 4 * max(e_ref, 1e-6)
        else:
            v32 = R.encode_ref(sd, mel, lens, torch.float32, rnd=R.split2, wrnd=R.split2 if planes else None)[0]
            floor = 4 * 2.0 ** -17 * float(h64.abs()[valid].max())
    base = float((v32.double() - v64).abs()[valid].max())
    return max(4 * base, floor), base


BUILDS = [("fp32", 0, "fp32", None), ("split_bf16_state", 2, "bf16", None), ("split_planes", 2, "fp32", None)]


@pytest.mark.parametrize("build,dt,kind,wplanes", BUILDS, ids=[b[0] for b in BUILDS])
def test_engine_token_rule_on_the_fixture(fix, build, dt, kind, wplanes):
    """(256, 4, 2) on the fixture's mel: code_len exact; every decided digit equals the float64 digit (and, on the fp32-kind
    state the reference ran, the reference's); pre-round values within the bound per row; batched equals solo, id for id.
    Measured on an MI355X, worst pre-round error / base / bound: fp32 3.1e-6 / 1.1e-6 / 5.9e-6; split on a bf16-kind state
    1.2e-5 / 1.1e-5 / 8.3e-5; split with weight planes 2.0e-5 / 1.3e-5 / 8.3e-5; undecided digits 0 %, 0 %, 0.14 %."""
    from mmx import shapes, synth
    from mmx.s3tok import SpeechTokenizerEngine
    z, names = fix
    sd = R.fixture_state(z, kind)
    mel, lens = R.padded_mel(z, names)
    with torch.no_grad():
        v64, h64, _, l2 = R.encode_ref(sd, mel, lens)
    valid = R.valid_rows(l2, v64.shape[1])
    eng = SpeechTokenizerEngine(sd, dtype=dt, n_head=4)
    assert eng.wplanes == (build == "split_planes")
    bound, base = _bound(sd, mel, lens, v64, h64, valid, "fp32" if dt == 0 else "split", float(z["e_ref"]), eng.wplanes)
    codes, cl, pre = eng.quantize(mel.cuda(), lens, want_pre=True)
    assert codes.dtype == torch.int32 and tuple(codes.shape) == tuple(v64.shape[:2]) and cl.tolist() == l2 == z["code_len"].tolist()
    codes, pre = codes.cpu(), pre.cpu()
    e = float((pre.double() - v64).abs()[valid].max())
    wrong, undecided = R.token_rule(R.id_digits(codes), v64, bound, valid)
    print(f"\ns3tok engine {build}: e_gpu {e:.3e}  base {base:.3e}  bound {bound:.3e}  undecided {undecided:.2%}  wrong {wrong}")
    assert bound <= 1e-3
    assert e <= bound and wrong == 0 and undecided <= 0.02
    assert bool((codes[~valid] == 0).all())
    if kind == "fp32":
        ref_d = R.id_digits(torch.from_numpy(z["codes"]))
        decided = ((v64.abs() - 0.5).abs() > bound) & valid[..., None]
        assert bool((R.id_digits(codes) == ref_d)[decided].all())
    for i, n in enumerate(lens):
        solo, scl = eng.quantize(mel[i:i + 1, :, :n].contiguous().cuda(), [n])
        assert scl.tolist() == [l2[i]] and torch.equal(solo[0, :l2[i]].cpu(), codes[i, :l2[i]]), names[i]


def test_engine_without_planes_on_an_fp32_state_is_reported(fix):
    """The same fp32-kind state with wplanes=False (weights rounded to bf16 at load): reported, not asserted.  Measured on an
    MI355X: pre-round error 9.9e-3, 2 of 720 digits differ from float64."""
    from mmx.s3tok import SpeechTokenizerEngine
    z, names = fix
    sd = R.fixture_state(z, "fp32")
    mel, lens = R.padded_mel(z, names)
    with torch.no_grad():
        v64, _, _, l2 = R.encode_ref(sd, mel, lens)
    valid = R.valid_rows(l2, v64.shape[1])
    eng = SpeechTokenizerEngine(sd, dtype=2, wplanes=False)
    codes, cl, pre = eng.quantize(mel.cuda(), lens, want_pre=True)
    d = (R.id_digits(codes.cpu()) != R.digits_of(v64))[valid]
    print(f"\ns3tok engine split, fp32-kind state, no planes: pre-round error {float((pre.cpu().double() - v64).abs()[valid].max()):.3e}, "
          f"{int(d.sum())} of {d.numel()} digits differ from float64")
    assert cl.tolist() == l2


def test_engine_bf16_request_builds_the_split_build_and_cpu_raises(fix):
    from mmx._lib import MmxError, X2
    from mmx.s3tok import SpeechTokenizerEngine
    z, _ = fix
    eng = SpeechTokenizerEngine(R.fixture_state(z, "bf16"), dtype=1)
    assert eng.dtype == X2 and not eng.wplanes
    with pytest.raises(MmxError):
        eng.quantize(torch.zeros(1, 128, 8), [8])
    with pytest.raises(MmxError):
        eng.tokenize([torch.zeros(400)])


@pytest.mark.parametrize("dt", [0, 2], ids=["fp32", "split"])
def test_tokenize_clips_batched_equals_solo(fix, dt):
    """Clip -> mel -> tokens in one zero-padded batch: every clip's ids equal its solo run and quantize() on its own device
    mel, and obey the token rule against float64 on that mel."""
    from mmx.s3tok import LogMelW, SpeechTokenizerEngine
    z, names = fix
    sd = R.fixture_state(z, "fp32")
    eng = SpeechTokenizerEngine(sd, dtype=dt)
    waves = [torch.from_numpy(z["wave_" + n]).cuda() for n in names]
    toks = eng.tokenize(waves)
    assert [t.numel() for t in toks] == z["code_len"].tolist() and all(t.dtype == torch.int32 for t in toks)
    m = LogMelW()
    for i, w in enumerate(waves):
        solo = eng.tokenize([w])[0]
        assert torch.equal(solo, toks[i]), names[i]
        mel = m(w)
        q, cl = eng.quantize(mel, [mel.shape[2]])
        assert torch.equal(q[0, :int(cl[0])], toks[i]), names[i]
        with torch.no_grad():
            v64, h64, _, l2 = R.encode_ref(sd, mel.cpu(), [mel.shape[2]])
        valid = R.valid_rows(l2, v64.shape[1])
        bound, _ = _bound(sd, mel.cpu(), [mel.shape[2]], v64, h64, valid, "fp32" if dt == 0 else "split", float(z["e_ref"]), eng.wplanes)
        assert bound <= 1e-3 and R.token_rule(R.id_digits(toks[i].cpu())[None], v64, bound, valid)[0] == 0, names[i]


def _clip(n, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n, dtype=torch.float64)
    env = 0.6 + 0.4 * torch.sin(2 * np.pi * 2.5 * t / 16000)
    return ((0.4 * torch.sin(2 * np.pi * 180.0 * t / 16000) * env).float() + 0.05 * torch.randn(n, generator=g))


def test_engine_full_size_token_rule():
    """(1280, 20, 6), synthetic weights, one 2 s clip (50 tokens), split build: the token rule against the float64 restatement.
    Measured on an MI355X: pre-round error 2.4e-5, base 2.3e-5, bound 1.2e-4, 0.25 % undecided."""
    from mmx import shapes, synth
    from mmx.s3tok import LogMelW, SpeechTokenizerEngine
    sd = synth.synth_state_dict(shapes.s3tok_manifest(), 1)
    eng = SpeechTokenizerEngine(sd, dtype=2, n_head=20)
    assert (eng.C, eng.H, eng.layers) == (1280, 20, 6) and not eng.wplanes
    mel = LogMelW()(_clip(32000, 11).cuda())
    codes, cl, pre = eng.quantize(mel, [200], want_pre=True)
    assert cl.tolist() == [50]
    with torch.no_grad():
        v64, h64, _, l2 = R.encode_ref(sd, mel.cpu(), [200])
    valid = R.valid_rows(l2, 50)
    bound, base = _bound(sd, mel.cpu(), [200], v64, h64, valid, "split", 0.0, False)
    e = float((pre.cpu().double() - v64).abs().max())
    wrong, undecided = R.token_rule(R.id_digits(codes.cpu()), v64, bound, valid)
    print(f"\ns3tok full size: e_gpu {e:.3e}  base {base:.3e}  bound {bound:.3e}  undecided {undecided:.2%}  wrong {wrong}")
    assert bound <= 1e-3 and e <= bound and wrong == 0 and undecided <= 0.02


def test_long_audio_windows_and_merge(fix):
    """A 31 s clip (3100 frames: two windows, 750 rows each) at (256, 4, 2): ids equal the float64 restatement applied per window
    under the CPU-tested plan and merged, by the token rule; the mel (and its clip maximum) is taken once over the whole clip."""
    from mmx import s3tok
    z, _ = fix
    sd = R.fixture_state(z, "fp32")
    eng = s3tok.SpeechTokenizerEngine(sd, dtype=2)
    w = _clip(31 * 16000, 23).cuda()
    toks = eng.tokenize([w])[0].cpu()
    mel = s3tok.LogMelW()(w).cpu()
    assert mel.shape[2] == 3100
    with pytest.raises(s3tok.MmxError, match="want_pre"):
        eng.quantize(mel.cuda(), [3100], want_pre=True)
    plan = s3tok.segment_plan(3100)
    assert plan == [(0, 3000), (2600, 500)]
    segs = torch.zeros(len(plan), 128, 3000)
    for i, (s, n) in enumerate(plan):
        segs[i, :, :n] = mel[0, :, s:s + n]
    lens = [n for _, n in plan]
    with torch.no_grad():
        v64, h64, _, l2 = R.encode_ref(sd, segs, lens)
    valid = R.valid_rows(l2, v64.shape[1])
    bound, _ = _bound(sd, segs, lens, v64, h64, valid, "split", 0.0, eng.wplanes)
    rows = s3tok.merge_segments([[(i, j) for j in range(l2[i])] for i in range(len(plan))])
    assert toks.numel() == len(rows) == 750 + 125 - 100
    vm = torch.stack([v64[i, j] for i, j in rows])
    wrong, undecided = R.token_rule(R.id_digits(toks), vm, bound, torch.ones(len(rows), dtype=torch.bool))
    print(f"\ns3tok long audio: bound {bound:.3e}  undecided {undecided:.2%}  wrong {wrong}")
    assert bound <= 1e-3 and wrong == 0 and undecided <= 0.02


# ------------------------------------------------------------------------------------------------ pipeline, drop-in, LayerNorm width
def test_prompt_from_audio_splats_into_tts(fix):
    """A 1.3 s clip pair -> prompt dict: tokens and latents trimmed to token_len and 2 * token_len (frontend_zero_shot), the flow
    embedding from the same clip; tts(**dict) runs on a 2-layer LM and equals passing the same tensors by hand."""
    from mmx import shapes, synth
    from mmx.pipeline import TtsEngine
    z, _ = fix
    llm_sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    flow_sd = synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1, use_speaker_encoder=True), 0)
    dac_sd = synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0)
    enc_sd = synth.synth_state_dict(shapes.dac_encoder_manifest(80), 0)
    text = torch.randint(0, 151936, (1, 8), generator=torch.Generator().manual_seed(0)).cuda()
    ptext = torch.randint(0, 151936, (1, 4), generator=torch.Generator().manual_seed(1)).cuda()
    w16, w24 = _clip(20800, 3).cuda(), _clip(31200, 4).cuda()
    eng = TtsEngine(llm_sd, flow_sd, dac_sd, dtype=2, max_batch=1, max_ctx=256, s3tok_sd=R.fixture_state(z, "bf16"), dacenc_sd=enc_sd)
    try:
        g = torch.Generator(device="cuda").manual_seed(9)
        p = eng.prompt_from_audio(w16, w24, ptext, generator=g)
        assert set(p) == {"llm_prompt_speech_token", "flow_prompt_speech_token", "prompt_speech_feat", "prompt_text", "flow_embedding"}
        n_tok, n_lat = (20800 // 160 - 1) // 2 // 2 + 1, eng.dacenc.frames(31200)
        token_len = min(n_lat // 2, n_tok)
        assert n_tok == 33 and n_lat == 65 and token_len == 32                  # the latents decide: one token is cut
        assert tuple(p["llm_prompt_speech_token"].shape) == (1, token_len) and p["llm_prompt_speech_token"].dtype == torch.long
        assert tuple(p["prompt_speech_feat"].shape) == (1, 2 * token_len, 80) and tuple(p["flow_embedding"].shape) == (1, 192)
        assert torch.equal(p["llm_prompt_speech_token"][0], eng.s3tok.tokenize([w16])[0][:token_len].long())
        assert int(p["llm_prompt_speech_token"].max()) < 6561
        a = eng.tts(text, seed=0, exact_steps=12, **p).clone()
        b = eng.tts(text, p["flow_embedding"], ptext, p["llm_prompt_speech_token"], p["flow_prompt_speech_token"], p["prompt_speech_feat"],
                    seed=0, exact_steps=12)
        assert a.shape[-1] == 24 * eng.hop and torch.isfinite(a).all() and torch.equal(a, b)
    finally:
        eng.close()
    bare = TtsEngine(llm_sd, flow_sd, dac_sd, dtype=2, max_batch=1, max_ctx=256)
    try:
        with pytest.raises(RuntimeError, match="s3tok_sd"):
            bare.prompt_from_audio(w16, w24)
    finally:
        bare.close()


def test_dropin_package_layouts_and_agreement(fix):
    """s3tokenizer.S3TokenizerV2.quantize / log_mel_spectrogram: the reference's layouts and dtypes, the engine's values."""
    import sys
    sys.path.insert(0, os.path.join(R.ROOT, "minimax-speech_amd", "speech", "tools", "S3Tokenizer"))
    import s3tokenizer
    from mmx.s3tok import LogMelW, SpeechTokenizerEngine
    z, names = fix
    sd = R.fixture_state(z, "fp32")
    tok = s3tokenizer.S3TokenizerV2("speech_tokenizer_v2_25hz", s3tokenizer.ModelConfig(n_audio_state=256, n_audio_head=4, n_audio_layer=2))
    tok.load_state_dict(sd, strict=True)
    tok.freeze()
    tok = tok.to("cuda")
    assert tok.device.type == "cuda" and not any(p.requires_grad for p in tok.parameters())
    mels = [s3tokenizer.log_mel_spectrogram(torch.from_numpy(z["wave_" + n]), device="cuda") for n in names]
    for n, m in zip(names, mels):
        assert m.dtype == torch.float32 and tuple(m.shape) == z["mel32_" + n].shape
        assert torch.equal(m, LogMelW()(torch.from_numpy(z["wave_" + n]).cuda())[0])
    feats, lens = s3tokenizer.padding(mels)
    assert tuple(feats.shape) == (4, 128, 200) and lens.dtype == torch.int32 and lens.tolist() == [200, 2, 56, 100]
    codes, code_len = tok(feats, lens.cuda())
    assert codes.dtype == torch.int32 and tuple(codes.shape) == tuple(z["codes"].shape) and code_len.tolist() == z["code_len"].tolist()
    eng = SpeechTokenizerEngine(sd, dtype=2)
    assert torch.equal(codes, eng.quantize(feats, lens.tolist())[0])
    tok.float_parity()
    c32, _ = tok.quantize(feats, lens.cuda())
    assert torch.equal(c32, SpeechTokenizerEngine(sd, dtype=0).quantize(feats, lens.tolist())[0])
    with pytest.raises(RuntimeError, match="init_from_pt"):
        s3tokenizer.load_model("speech_tokenizer_v2_25hz")
    with pytest.raises(RuntimeError, match="init_from_pt"):
        tok.init_from_onnx("x.onnx")


@pytest.mark.parametrize("dt", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C_,eps", [(1280, 1e-6), (2048, 1e-5), (1025, 1e-5)])
def test_rownorm_beyond_1024_channels(C_, eps, dt):
    """mmx_rownorm at the tokenizer's width (rows of more than 1024 channels take the 32-values-per-lane form, in both output
    types): LayerNorm against float64, per row relative <= max(4 * the torch fp32 statement's error, 1e-6), the statement being
    torch's fp32 LayerNorm, rounded to bf16 for the bf16 output; guards intact.  Measured on an MI355X: fp32 1.4e-7 ... 1.8e-7
    (statement 1.3e-7 ... 2.1e-7); bf16 2.5e-3 ... 3.1e-3, equal to the statement's (the rounding of the output)."""
    from mmx import ops
    g = torch.Generator().manual_seed(C_)
    B, T = 2, 7
    tdt = torch.bfloat16 if dt == 1 else torch.float32
    x = torch.randn(B, T, C_, generator=g) * 3 + 0.5
    ga, be = torch.randn(C_, generator=g) * 0.1 + 1, torch.randn(C_, generator=g) * 0.05
    ref = F.layer_norm(x.double(), (C_,), ga.double(), be.double(), eps)
    st = F.layer_norm(x, (C_,), ga, be, eps).to(tdt)
    buf, out = guarded((B, T, C_), tdt)
    ops.rownorm(x.cuda(), ga.cuda(), be.cuda(), eps, rows=T, C_=C_, batch=B, dtype=dt, **({"out_act": out} if dt == 1 else {"out_f32": out}))
    torch.cuda.synchronize()
    assert_guards(buf, "rownorm")
    e, e32 = row_rel(out.cpu(), ref), row_rel(st, ref)
    print(f"\nrownorm C {C_} dtype {dt}: e_gpu {e:.3e}  torch statement {e32:.3e}")
    assert e <= max(4 * e32, 1e-6)


@pytest.mark.parametrize("build,dt,kind,wplanes", BUILDS, ids=[b[0] for b in BUILDS])
def test_engine_odd_frame_count_solo(fix, build, dt, kind, wplanes):
    """57 mel frames (29 rows after the first stride-2 convolution, 15 tokens): at an odd length the last window of each
    convolution reads one row past the end, which is zero padding.  A solo quantize against float64 by the token rule.
    Measured on an MI355X, pre-round error / base / bound: fp32 1.6e-6 / 1.0e-6 / 5.9e-6; split on a bf16-kind state
    5.9e-6 / 8.9e-6 / 8.0e-5; split with weight planes 1.9e-5 / 1.1e-5 / 8.0e-5; no undecided digit."""
    from mmx.s3tok import SpeechTokenizerEngine
    z, _ = fix
    sd = R.fixture_state(z, kind)
    mel = torch.from_numpy(z["mel32_noise"][:, 20:77]).contiguous()[None]
    with torch.no_grad():
        v64, h64, _, l2 = R.encode_ref(sd, mel, [57])
    assert l2 == [15]
    valid = R.valid_rows(l2, 15)
    eng = SpeechTokenizerEngine(sd, dtype=dt)
    bound, base = _bound(sd, mel, [57], v64, h64, valid, "fp32" if dt == 0 else "split", float(z["e_ref"]), eng.wplanes)
    codes, cl, pre = eng.quantize(mel.cuda(), [57], want_pre=True)
    assert cl.tolist() == [15] and tuple(codes.shape) == (1, 15)
    e = float((pre.cpu().double() - v64).abs().max())
    wrong, undecided = R.token_rule(R.id_digits(codes.cpu()), v64, bound, valid)
    print(f"\ns3tok engine {build}, 57 frames: e_gpu {e:.3e}  base {base:.3e}  bound {bound:.3e}  undecided {undecided:.2%}  wrong {wrong}")
    assert bound <= 1e-3 and e <= bound and wrong == 0 and undecided <= 0.02
    # the same clip inside a longer zero-padded buffer (T = 60: the rows past 57 are masked, not read)
    pad = torch.zeros(1, 128, 60)
    pad[:, :, :57] = mel
    pad[:, :, 57:] = 3.0
    c2, cl2 = eng.quantize(pad.cuda(), [57])
    assert cl2.tolist() == [15] and torch.equal(c2[0, :15], codes[0])
