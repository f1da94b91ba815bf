"""The LM decode step on fp16 planes (MMX_H2 / MMX_H2W; csrc/decode.hip, csrc/act_layout.h, the decode attention's MMX_DA_H2
output) over the activation range, with the three-bf16-plane form (MMX_X3) on the same inputs as the control.

Inputs.  One launch holds rows 2^32 apart: row r of a batch is randn * 2^e, e walking the ladder 2^-20 .. 2^12 of
tests/test_lm_planes_host.py (a batch of one takes the ladder launch by launch).  A second set sits at scale 1 with two
massive-activation channels (columns * 2^11, |x * gamma| up to ~1e4).  Error is per row throughout: max |got - ref| over the
row / max |ref| of that row, so a defect confined to one row or one scale cannot hide behind the largest row of the launch.

Bounds (all derived on the host, none from what the kernels give):
  * planes a kernel writes: per element max(2^-22 |v|, 2^-25) + 2^-24 |v| against v recomputed in fp32 (the format's bound of
    test_lm_planes_host.py plus one fp32 rounding of v).  mmx_decode_prep is NOT bit for bit split_planes(x * gamma): the
    gfx950 build contracts the product into both conversions (v_fma_mixlo_f16: hi = fp16 of the exact product x * gamma, lo =
    fp16 of the exact product minus hi), one rounding each where the host statement rounds the product to fp32 first - so the
    contracted form's bound is the one asserted, and the planes are also checked against the exact product, which they hold
    to the format's max(2^-22 |v|, 2^-25) alone;
  * mmx_skinny2: float64 on the operands AS THE PLANES HOLD THEM (merged input planes, the weights as packed); bound per row
    max(4 * e32, 1e-6), e32 = the same statement evaluated in fp32 on the CPU against float64; never above 1e-5.  It does not
    depend on the row's scale: it stays tight at 2^-20, where the format itself is coarse, and a matrix unit that read
    subnormal fp16 operands as zero would miss it by the factors of the host file's table (>= 16 x the format's own error
    from 2^-3 down, 1.0 at 2^-20);
  * engine: the suite's fp32 log-prob bound 2e-3 (tests/test_gpu_llm.py) against the CPU oracle's teacher-forced record.

Measured on the MI355X (test_kernel_scale_table prints the table; DESIGN.md section 2 keeps it): the kernels follow the format's
no-flush column at every scale (MMX_H2 2.6e-2 at 2^-20, 1.5e-6 at 2^-6, 2.8e-7 at 2^-3, 1.6e-7 .. 1.9e-7 from 2^0 up; flushed
operands would give 1.0, 3.2e-4, 2.7e-4) - v_mfma_f32_16x16x32_f16 keeps subnormal fp16 operands; the largest row bound of any
case is 4.2e-6; engine log-probs 2.4e-4 (fp16 planes) / 2.0e-5 (bf16 planes) on the 2^-6 checkpoint, 1.7e-5 on the massive one."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops_parity import assert_guards, guarded
from test_lm_planes_host import (EPS, LADDER, format_table, gain, h2_elem_bound, h2_store_bound, ladder_rows, massive_rows,
                                 row_err, scale_table, weights)

pytestmark = pytest.mark.gpu

X3, H2, H2W = 3, 4, 0x14
DT_NAME = {X3: "x3", H2: "h2", H2W: "h2w"}
N = 64
ROW_FLOOR, ROW_CAP = 1e-6, 1e-5
LOGP_TOL = 2e-3                                           # tests/test_gpu_llm.py, fp32 build
SENTINEL16 = int(torch.tensor(7.0, dtype=torch.bfloat16).view(torch.int16))      # the guard value of a 16-bit buffer, as bits


@pytest.fixture(scope="module")
def ops():
    from mmx import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    _lib.load()
    return ops


def input_sets(B, K, seed):
    """[(name, x [B, K], the rows' exponents)]: the ladder in one launch (B = 1: one launch per ladder scale) and the
    massive-activation set."""
    if B >= len(LADDER):
        sets = [("ladder",) + ladder_rows(B, K, seed)]
    else:
        sets = [(f"2^{e}",) + ladder_rows(B, K, seed + 50 + e, exps=(e,)) for e in LADDER]
    return sets + [("massive", massive_rows(B, K, seed + 1), [0] * B)]


def ssq_table(x):
    """[32][64] per-16-column-tile sums of squares of the rows of x, as a producer of the residual stream writes them."""
    B, K = x.shape
    t = torch.zeros(32, 64)
    t[:B, :K // 16] = x.double().pow(2).reshape(B, K // 16, 16).sum(-1).float()
    return t


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def plane_rows(ops, view, B, K, nplanes):
    """A guarded plane buffer -> ([nplanes, B, K] rows the kernel owns, [nplanes, pad rows, K] rows of the last tile it must not
    write), 16-bit patterns."""
    R = ops.packed_rows(B)
    un = torch.stack([ops.unpack_act(view.cpu().reshape(nplanes, -1)[s], R, K, 1) for s in range(nplanes)])
    un = un.contiguous().view(torch.int16)
    return un[:, :B], un[:, B:]


def merged(rows, f16):
    """[planes, B, K] 16-bit patterns -> float64 [B, K]."""
    return sum(rows[s].contiguous().view(torch.float16 if f16 else torch.bfloat16).double() for s in range(rows.shape[0]))


def assert_pad_untouched(pad, what):
    assert bool((pad == SENTINEL16).all()), f"{what}: rows >= B of the planes were written"


# ------------------------------------------------------------------------------------------------ 1. mmx_decode_prep
@pytest.mark.parametrize("B,K", [(19, 128), (1, 128), (19, 896)])
def test_decode_prep_fp16_planes_over_the_range(ops, B, K):
    """h = x bit for bit; the planes hold x * gamma (contracted form, see the module docstring); ssq per row within 1e-6, slots
    past K / 16 zero; rows >= B and the guards around every output untouched."""
    gam = gain(K, 3)
    exact_bits = 0
    for name, x, _ in input_sets(B, K, 20):
        xs_buf, xs = guarded(2 * ops.plane_elems(B, K), torch.bfloat16)
        ssq_buf, ssq = guarded(32 * 64, torch.float32)
        h_buf, h = guarded(B * K, torch.float32)
        ops.decode_prep(x.cuda(), xs, ssq, B=B, K=K, gamma=gam.cuda(), h=h.view(B, K), dtype=H2)
        torch.cuda.synchronize()
        for buf, n in ((xs_buf, xs.numel()), (ssq_buf, ssq.numel()), (h_buf, h.numel())):
            assert_guards(buf, n, f"decode_prep {name}")
        assert torch.equal(bits(h.cpu().view(B, K)), bits(x)), name
        rows, pad = plane_rows(ops, xs, B, K, 2)
        assert_pad_untouched(pad, name)
        v = x * gam                                        # the fp32 product, as the host statement of the format forms it
        got = merged(rows, True)
        assert bool(torch.isfinite(got).all()), name
        err = (got - v.double()).abs()
        assert bool((err <= h2_store_bound(v)).all()), (name, float((err / h2_store_bound(v)).max()))
        p = x.double() * gam.double()                      # the exact product: what the contracted conversions round
        assert bool(((got - p).abs() <= h2_elem_bound(p.float())).all()), name
        want, _ = plane_rows(ops, ops.split_planes(v, f16=True), B, K, 2)
        exact_bits += int(torch.equal(rows, want))
        sq = ssq.cpu().view(32, 64)
        ref = ssq_table(x)
        assert float(row_err(sq[:B, :K // 16], ref[:B, :K // 16]).max()) <= 1e-6, name
        assert float(sq[:B, K // 16:].abs().sum()) == 0.0 and bool(torch.isnan(sq[B:]).all()), name
    print(f"decode_prep B {B} K {K}: {exact_bits} input sets bit for bit split_planes(x * gamma), the others within the contracted bound")


# ------------------------------------------------------------------------------------------------ 2. / 3. mmx_skinny2
def packed_weights(ops, w, dt, epi):
    """-> (the pack, the weights as the pack holds them, float64)."""
    ih = N if epi == 1 else 0
    if dt == X3:
        assert torch.equal(w.to(torch.bfloat16).float(), w)
        return ops.pack_skinny(w.to(torch.bfloat16).cuda().contiguous(), dtype=X3, interleave_half=ih), w.double()
    wp = ops.pack_skinny_h2(w.cuda().contiguous(), planes=(2 if dt == H2W else 1), interleave_half=ih)
    assert isinstance(wp, ops.Planed) == (dt == H2W)
    ws, wq, r = w * ops.H2_WSCALE, 0, w * ops.H2_WSCALE
    for _ in range(2 if dt == H2W else 1):
        t = r.to(torch.float16)
        wq, r = wq + t.double(), r - t.float()
    if dt == H2:
        assert torch.equal(wq, ws.double())               # a bf16-representable weight * 2^8 is an fp16 number
    return wp, wq / ops.H2_WSCALE


def statement(xm, wq, ssq, K, epi, bias, res, dtype):
    """The projection and its epilogue on the operands as given, evaluated in `dtype` (float64: the reference; float32: e32)."""
    acc = xm.to(dtype) @ wq.to(dtype).t()
    if ssq is not None:
        acc = acc * torch.rsqrt(ssq.to(dtype).sum(-1, keepdim=True) / K + torch.tensor(EPS, dtype=dtype))
    if epi == 0:
        return acc if bias is None else acc + bias.to(dtype)
    if epi == 1:
        return F.silu(acc[:, :N]) * acc[:, N:]
    return res.to(dtype) + acc


def run_skinny2(ops, dt, x, exps, K, epi, rs, tw, J, seed, with_bias=True):
    """One launch on x.  -> dict of what the kernel left (CPU tensors) and of the references."""
    B = x.shape[0]
    f16 = dt != X3
    ns = 2 if f16 else 3
    w = weights(2 * N if epi == 1 else N, K, seed, bf16=(dt != H2W))
    gam, gnext = (gain(K, seed + 1) if rs else None), gain(N, seed + 2)
    g = torch.Generator().manual_seed(seed + 3)
    bias = torch.randn(N, generator=g) if epi == 0 and with_bias else None
    res = torch.randn(B, N, generator=g) * torch.exp2(torch.tensor(exps, dtype=torch.float32))[:, None] if epi == 2 else None
    xg = x * gam if rs else x
    xs = ops.split_planes(xg, f16=f16)
    xm = ops.merge_planes(xs, B, K, f16=f16).double()     # the operand as the planes hold it
    wp, wq = packed_weights(ops, w, dt, epi)
    ssq = ssq_table(x) if rs else None
    r64 = statement(xm, wq, None if ssq is None else ssq[:B], K, epi, bias, res, torch.float64)
    r32 = statement(xm, wq, None if ssq is None else ssq[:B], K, epi, bias, res, torch.float32)
    exact = statement(xg, w, None if ssq is None else ssq[:B], K, epi, bias, res, torch.float64)
    R, nt = ops.packed_rows(B), (N + 15) // 16
    out_buf, out = guarded(R * N, torch.float32) if epi != 1 else (None, None)
    if epi == 2:
        out.view(R, N)[:B] = res.cuda()
    xo_buf, xo = guarded(ns * ops.plane_elems(B, N), torch.bfloat16) if epi != 0 else (None, None)
    so_buf = torch.full((32 * 64 + 128,), float("nan"), device="cuda")
    so = so_buf[64:64 + 32 * 64]
    so.zero_()                                            # the table's contract: allocated zeroed (include/mmx_hip.h)
    groups = (nt + tw - 1) // tw
    part_buf, part = guarded(J * groups * tw * (R // 16) * 4 * 64, torch.float32) if J > 1 else (None, None)
    tickets = torch.zeros(nt, dtype=torch.int32, device="cuda") if J > 1 else None
    ops.skinny2(xs.cuda(), wp, B=B, K=K, N=N, dtype=(H2 if f16 else X3), bias=(bias.cuda() if bias is not None else None),
                ssq_in=(ssq.cuda() if rs else None), eps=EPS, epi=epi, out=(out.view(R, N) if epi != 1 else None), xs_out=xo,
                gamma_next=(gnext.cuda() if epi == 2 else None), ssq_out=(so.view(32, 64) if epi == 2 else None), tiles_per_wg=tw,
                ksplit=J, part=part, tickets=tickets)
    torch.cuda.synchronize()
    what = f"skinny2 {DT_NAME[dt]} epi {epi}"
    if epi != 1:
        assert_guards(out_buf, R * N, what)
        assert bool(torch.isnan(out.view(R, N)[B:]).all()), f"{what}: rows >= B of out were written"
    if epi != 0:
        assert_guards(xo_buf, xo.numel(), what)
    if J > 1:
        assert_guards(part_buf, part.numel(), what)
        assert int(tickets.abs().sum()) == 0
    sb = so_buf.cpu()
    assert bool(torch.isnan(sb[:64]).all()) and bool(torch.isnan(sb[64 + 32 * 64:]).all()), f"{what}: wrote outside ssq_out"
    rows = pad = None
    if epi != 0:
        rows, pad = plane_rows(ops, xo, B, N, ns)
        assert_pad_untouched(pad, what)
    return dict(out=(out.cpu().view(R, N)[:B] if epi != 1 else None), rows=rows, ssq_out=so.cpu().view(32, 64), r64=r64, r32=r32,
                exact=exact, gnext=gnext, f16=f16)


def row_bound(r):
    """max(4 * e32, 1e-6) per row, from the CPU's fp32 evaluation of the statement; never above 1e-5."""
    b = torch.clamp(4 * row_err(r["r32"], r["r64"]), min=ROW_FLOOR)
    assert float(b.max()) <= ROW_CAP, float(b.max())
    return b


def check_skinny2(r, epi, tag):
    rb = row_bound(r)
    ref = r["r64"]
    if epi == 1:
        # the SwiGLU leaves planes only: the row bound on the fp32 value plus what the planes of that value may be off by
        got = merged(r["rows"], r["f16"])
        tol = (rb * ref.abs().amax(-1))[:, None] + (h2_store_bound(ref.float()) if r["f16"] else ref.abs() * 2.0 ** -23)
        # without the RMSNorm statistic the product of a row at 2^9 or 2^12 leaves the fp16 range (the engine's gate / up always
        # carries the statistic): an element past 65520 must show as non-finite planes, one below 65504 must hold the bound
        safe = ref.abs() < 6.0e4 if r["f16"] else torch.ones_like(ref, dtype=torch.bool)
        past = (ref.abs() > 7.0e4) & ~safe
        assert bool(torch.isfinite(got[safe]).all()) and not bool(torch.isfinite(got[past]).any()), tag
        over = ((got - ref).abs() / tol)[safe].max()
        assert float(over) <= 1.0, (tag, float(over))
        return
    got = r["out"]
    assert bool(torch.isfinite(got).all()), tag
    e = row_err(got, ref)
    assert bool((e <= rb).all()), (tag, [f"{float(a):.2e}/{float(b):.2e}" for a, b in zip(e, rb) if a > b])
    if epi == 2:
        # planes of out * gamma_next against the kernel's own fp32 `out`; per-tile sums of squares of it; rows >= B zero as allocated
        v = got.double() * r["gnext"].double()
        pe = (merged(r["rows"], r["f16"]) - v).abs()
        tol = h2_store_bound(v.float()) if r["f16"] else v.abs() * 2.0 ** -23
        assert bool((pe <= tol).all()), (tag, float((pe / tol.clamp_min(1e-300)).max()))
        B, nt = got.shape[0], N // 16
        assert float(row_err(r["ssq_out"][:B, :nt], ssq_table(got)[:B, :nt]).max()) <= 1e-6, tag
        assert float(r["ssq_out"][B:].abs().sum()) == 0.0 and float(r["ssq_out"][:, nt:].abs().sum()) == 0.0, tag


@pytest.mark.parametrize("tw", [1, 2])
@pytest.mark.parametrize("B", [19, 1])
@pytest.mark.parametrize("epi,rs,K,J", [(0, True, 128, 1), (0, False, 128, 1), (1, True, 128, 1), (1, False, 128, 1), (2, True, 128, 1),
                                       (2, False, 128, 1), (2, False, 256, 2), (2, True, 256, 2)])
@pytest.mark.parametrize("dt", [H2, H2W, X3], ids=["h2", "h2w", "x3"])
def test_skinny2_over_the_range(ops, dt, epi, rs, K, J, B, tw):
    """Every epilogue, with and without the RMSNorm statistic, one and two tiles per workgroup, one and two row tiles, K cut over
    two workgroups for the residual projections: each row within its own bound, the epilogue's planes and statistics against the
    kernel's own fp32 output, rows >= B and every guard untouched."""
    for name, x, exps in input_sets(B, K, 40 + epi):
        r = run_skinny2(ops, dt, x, exps, K, epi, rs, tw, J, seed=7 * epi + K)
        check_skinny2(r, epi, (DT_NAME[dt], name, epi, rs, K, J, B, tw))


def test_kernel_scale_table(ops, capsys):
    """The host file's table with the kernels beside it: 19 rows at one scale per launch, q/k/v-like projection (epilogue 0, RMSNorm
    statistic), the kernel's per-row error against float64 on the EXACT operands.  It is the format's error plus the kernel's
    own: bounded by the table's no-flush column plus the row bound.  (The flushed column is what a matrix unit that zeroes
    subnormal fp16 operands would show instead.)"""
    tab = scale_table()
    cols = {DT_NAME[dt]: {} for dt in (H2, H2W, X3)}
    for dt in (H2, H2W, X3):
        for e in LADDER:
            x, exps = ladder_rows(19, 128, 100 + e, exps=(e,))      # the inputs of scale_table()
            r = run_skinny2(ops, dt, x, exps, 128, 0, True, 1, 1, seed=1, with_bias=False)
            cols[DT_NAME[dt]][e] = float(row_err(r["out"], r["exact"]).max())
            # the format's share plus the kernel's own
            fmt = float(row_err(r["r64"], r["exact"]).max())
            assert cols[DT_NAME[dt]][e] <= fmt + float(row_bound(r).max()), (DT_NAME[dt], e, cols[DT_NAME[dt]][e], fmt)
    with capsys.disabled():
        print("\nper-row relative error against float64 on exact operands: the plane formats (host) and mmx_skinny2 (this GPU)")
        print(format_table(tab, cols))


# ------------------------------------------------------------------------------------------------ 4. decode attention
@pytest.mark.parametrize("Hq,Hkv,B", [(14, 2, 6), (14, 2, 19), (4, 2, 6)])
def test_decode_attn_fp16_planes_over_the_v_range(ops, Hq, Hkv, B):
    """V cache (and the step's own V row) at scales 2^-12, 1 and 2^12, with 0 and 40 cached keys, all in one launch: the two fp16
    planes equal split_planes(o, f16=True) of the row-major fp32 output of the same launch arguments bit for bit (B = 19 at 14
    heads: two heads per workgroup)."""
    D, page, P = 64, 16, 4
    g = torch.Generator().manual_seed(17 + Hq)
    combos = [(e, n) for e in (-12, 0, 12) for n in (0, 40)]
    scale = torch.tensor([2.0 ** combos[b % 6][0] for b in range(B)])
    pos = torch.tensor([combos[b % 6][1] for b in range(B)], dtype=torch.int32)
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g)
    qkv[:, (Hq + Hkv) * D:] *= scale[:, None]
    kc = torch.randn(B * P + 1, Hkv, page, D, generator=g)
    vc = torch.randn(B * P + 1, Hkv, page, D, generator=g)
    vc[:B * P] *= scale.repeat_interleave(P)[:, None, None, None]
    bt = torch.arange(B * P, dtype=torch.int32).reshape(B, P)
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2).float() / D))
    W = Hq * D
    o_buf, o = guarded(B * W, torch.float32)
    p_buf, p = guarded(2 * ops.plane_elems(B, W), torch.bfloat16)
    kw = dict(B=B, Hq=Hq, Hkv=Hkv, page=page, dtype=0, per_head=True)
    ops.decode_attn(qkv.cuda(), inv.cuda(), pos.cuda(), kc.cuda(), vc.cuda(), bt.cuda(), o.view(B, W), **kw)
    ops.decode_attn(qkv.cuda(), inv.cuda(), pos.cuda(), kc.cuda(), vc.cuda(), bt.cuda(), p, out_split="f16", **kw)
    torch.cuda.synchronize()
    assert_guards(o_buf, B * W, "decode_attn fp32")
    assert_guards(p_buf, p.numel(), "decode_attn planes")
    o32 = o.cpu().view(B, W)
    assert bool(torch.isfinite(o32).all())
    # the rows are at the scale of their V: the launch does hold outputs 2^24 apart
    amax = o32.abs().amax(-1)
    assert float(amax[scale == 2.0 ** 12].min()) > 2.0 ** 8 and float(amax[scale == 2.0 ** -12].max()) < 2.0 ** -8
    rows, pad = plane_rows(ops, p, B, W, 2)
    assert_pad_untouched(pad, "decode_attn planes")
    want, _ = plane_rows(ops, ops.split_planes(o32, f16=True), B, W, 2)
    assert torch.equal(rows, want), int((rows != want).sum())


# ------------------------------------------------------------------------------------------------ 5. engine
STEPS, NSEQ = 6, 17


def derived_checkpoint(kind):
    from mmx import shapes, synth
    sd = dict(synth.synth_state_dict(shapes.llm_manifest(layers=2), 0))
    for k in ("llm.model.model.embed_tokens.weight", "speech_embedding.weight"):
        t = sd[k].clone()
        if kind == "small":
            t *= 2.0 ** -6                                # embedding rows at 2^-10: below the fp16 planes' documented lower edge
        else:
            t[:, 100] = 2.0 ** 11                         # one massive residual channel in every row
        sd[k] = t
    return sd


@pytest.fixture(scope="module", params=["small", "massive"])
def forced_case(request):
    """A derived checkpoint, 17 prompts, the ids forced on them and the CPU oracle's log-probs of every step (computed once)."""
    from oracle import llm as OL
    sd = derived_checkpoint(request.param)
    g = torch.Generator().manual_seed(23)
    z = torch.zeros(1, 0, dtype=torch.long)
    texts = [torch.randint(0, 151936, (1, 6 + b % 5), generator=g) for b in range(NSEQ)]
    forced = torch.randint(0, 6561, (NSEQ, STEPS), generator=g)
    ref = []
    with torch.no_grad():
        for b in range(NSEQ):
            rec = []
            OL.lm_inference(sd, OL.QwenCfg(layers=2), texts[b], z, z, seed=0, seq=b, forced=forced[b].tolist(), max_steps=STEPS, record=rec)
            assert len(rec) == STEPS
            ref.append(torch.stack(rec))
    return request.param, sd, texts, forced, torch.stack(ref)     # ref [NSEQ, STEPS, V]


@pytest.mark.parametrize("B", [1, NSEQ])
@pytest.mark.parametrize("planes", ["f16x2", "bf16x3"])
def test_engine_teacher_forced_logp_on_derived_checkpoints(forced_case, planes, B):
    """2-layer split build, 6 teacher-forced steps: every step's log-probs within the fp32 bound of the CPU oracle's, on a
    checkpoint whose embeddings sit below the fp16 planes' lower edge and on one with a massive residual channel."""
    from mmx.llm import LlmEngine
    kind, sd, texts, forced, ref = forced_case
    eng = LlmEngine(sd, dtype=X3, max_batch=B, max_ctx=128, use_graphs=False, lm_planes=planes)
    assert eng.h2 == (planes == "f16x2")
    z = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    xs = [eng.build_lm_input(t.cuda(), z, z) for t in texts[:B]]
    eng.start(xs, [100] * B, [100] * B, seed=0, forced=forced[:B].cuda(), want_logp=True)
    errs = []
    for i in range(STEPS):
        if i:
            eng.step()
        lp = eng.logp.cpu()
        assert bool(torch.isfinite(lp).all()), (kind, planes, B, i)
        errs.append(float((lp - ref[:B, i]).abs().max()))
    eng.close()
    print(f"{kind} checkpoint, {planes}, batch {B}: max |dlogp| over {STEPS} steps = {max(errs):.3e} (bound {LOGP_TOL:.0e})")
    assert max(errs) < LOGP_TOL, (kind, planes, B, errs)
