"""Float64 parity of the LM's paged KV-cache kernels: mmx_rope_kv_store, mmx_paged_attn and the three kernels behind
mmx_decode_attn (one and two query heads per workgroup, GQA-shared), plus the launches of mmx_paged_attn / mmx_attn_dense that
need more than 64 KB of dynamic LDS.

One reference, kv_ref(): plain torch on the CPU.  It gathers every sequence's cached keys / values through the block table as
stored (bf16 widened exactly), ropes the new rows, rounds the new K / V to the storage type as the kernels do, appends and runs
causal GQA softmax attention - all in float64, except the RoPE angle, which is the model's fp32 product float32(p) * inv_freq[d]
(what HF computes and what the engine's rope_tab holds) widened to float64.  test_kv_ref_matches_dense_restatement checks it on
the CPU against a dense [n, n] causal attention over the concatenated history.

Metric: per (sequence, query row, head) max |got - ref| over the 64 channels / max |ref| over those 64 channels; every row passes.
Bounds: bf16 kernels 1e-2 (decode_attn) and 2e-2 (rope_kv_store + paged_attn); fp32 kernels 4 x the error of the SAME statement
in plain torch fp32 on the CPU (same inputs, same metric), at least 1e-6 and never above the suite's 2e-5 (figures below).

Caches: shuffled block tables, more pages than the tables name, a leading and a trailing guard page, unused table entries point
at a trash page.  Every cache row that is not part of a sequence's history holds NaN, so a read of a wrong row shows in the
output; after every launch all cache elements but the rows written are compared bit for bit with a clone taken before it."""
import functools

import pytest
import torch

from test_gpu_ops_parity import ATOL, GUARD, _attn, assert_guards, attn64, guarded, is_sentinel

gpu = pytest.mark.gpu

D, HALF, PAGE, SCALE = 64, 32, 16, 0.125
INV = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))          # fp32, as LmModel builds it
BF16_DECODE, BF16_PAGED, FP32_CAP, FP32_FLOOR, FP32_K = 1e-2, 2e-2, 2e-5, 1e-6, 1e-6

# fp32 bounds = max(4 * base, 1e-6) <= 2e-5 with base = worst row of kv_ref(dtype=float32) against kv_ref(dtype=float64), computed
# by every fp32 test on its own inputs (fp32_bound(), printed).  torch's fp32 matmul on the CPU sums in an order that depends on
# the host and its thread count, so base moves by some 30 % between hosts; measured on the host of the MI355X run (base -> bound):
#   A  (19, 14, 2) 1.00e-6 -> 4.0e-6   (17, 16, 8) 1.07e-6 -> 4.3e-6   (17, 16, 16) 1.35e-6 -> 5.4e-6
#   B  ctx 0: 2.0e-7 -> 1e-6 (the floor)   16: 2.7e-7 -> 1.1e-6   511: 1.12e-6 -> 4.5e-6   700: 1.29e-6 -> 5.2e-6   1015: 1.22e-6 -> 4.9e-6
#   E  (14, 2): 20 + 1 + 1 rows 6.7e-7 -> 2.7e-6, 3 + 1 rows 9.0e-7 -> 3.6e-6   (4, 4): 7.4e-7 -> 3.0e-6, 5.3e-7 -> 2.1e-6
#   F  paged_attn at max_pages 1040: 2.1e-7 -> 1e-6 (the floor)
# (the kernels' own worst rows in that run: fp32 decode_attn 4.6e-7, fp32 rope_kv_store + paged_attn 7.2e-7)

@pytest.fixture(scope="module")
def env():
    from mmx import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    _lib.load()
    return _lib, ops


def tdt(dt):
    return torch.bfloat16 if dt == 1 else torch.float32


def bits(t):
    """The elements as integers: comparisons that hold for NaN too."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ================================================================================================ the reference
def rope(x, p, dtype):
    """x [..., 64] of `dtype`, p integer positions broadcastable to x.shape[:-1]."""
    ang = (p.to(torch.float32)[..., None] * INV).to(dtype)                          # the fp32 product, then widened
    c, s = ang.cos(), ang.sin()
    x0, x1 = x[..., :HALF], x[..., HALF:]
    return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], -1)


def kv_ref(qkv, pos, kc, vc, bt, *, Hq, Hkv, st, dtype=torch.float64, round_q=False):
    """qkv [B, R, (Hq + 2 Hkv) * 64] fp32: R new rows per sequence from position pos[b] on; kc / vc [pages, Hkv, 16, 64] of the
    storage type `st` hold keys 0 .. pos[b] - 1 of sequence b at (bt[b, j // 16], :, j % 16).  All on the CPU.
    -> out [B, R, Hq * 64], q [B, R, Hq, 64] (roped), k_new [B, R, Hkv, 64] (roped, NOT yet rounded to st), all `dtype`;
       v_new [B, R, Hkv, 64] of st.  round_q: the queries go through st first (mmx_paged_attn reads rope_kv_store's q_out)."""
    B, R, _ = qkv.shape
    G = Hq // Hkv
    x = qkv.to(dtype)
    out = torch.zeros(B, R, Hq * D, dtype=dtype)
    qs, ks, vs = [], [], []
    for b in range(B):
        p0 = int(pos[b])
        pp = torch.arange(p0, p0 + R)[:, None]
        q = rope(x[b, :, :Hq * D].reshape(R, Hq, D), pp, dtype)
        ku = rope(x[b, :, Hq * D:(Hq + Hkv) * D].reshape(R, Hkv, D), pp, dtype)
        vn = qkv[b, :, (Hq + Hkv) * D:].reshape(R, Hkv, D).to(st)
        qs.append(q)
        ks.append(ku)
        vs.append(vn)
        if round_q:
            q = q.to(st).to(dtype)
        j = torch.arange(p0)
        pg, sl = bt[b, j // PAGE].long(), j % PAGE
        K = torch.cat([kc[pg, :, sl].to(dtype), ku.to(st).to(dtype)], 0)          # [p0 + R, Hkv, 64]
        V = torch.cat([vc[pg, :, sl].to(dtype), vn.to(dtype)], 0)
        Kh, Vh = (t.transpose(0, 1).repeat_interleave(G, 0) for t in (K, V))        # [Hq, p0 + R, 64]
        s = torch.einsum("rhd,hnd->hrn", q, Kh) * SCALE
        vis = torch.arange(p0 + R)[None, :] <= pp                                   # row r sees keys 0 .. p0 + r
        s = s.masked_fill(~vis[None], float("-inf"))
        out[b] = torch.einsum("hrn,hnd->rhd", torch.softmax(s, -1), Vh).reshape(R, Hq * D)
    return out, torch.stack(qs), torch.stack(ks), torch.stack(vs)


def row_ratio(got, ref):
    """[..., H * 64] -> [..., H]: max |got - ref| over a head's 64 channels / max |ref| over them."""
    g, r = got.double().reshape(*got.shape[:-1], -1, D), ref.double().reshape(*ref.shape[:-1], -1, D)
    den = r.abs().amax(-1)
    assert float(den.min()) > 0
    return (g - r).abs().amax(-1) / den


def assert_rows(got, ref, bound, what, report=True):
    assert bool(torch.isfinite(got.float()).all()), f"{what}: output not finite (a row outside the context was read, or nothing was written)"
    r = row_ratio(got, ref)
    worst = float(r.max())
    if report:
        print(f"{what}: worst row {worst:.3e} (bound {bound:.2e})")
    assert worst < bound, f"{what}: row {tuple(int(i) for i in (r == r.max()).nonzero()[0])} at {worst:.3e} >= {bound:.2e}"


def fp32_bound(key, ref32, ref64):
    base = float(row_ratio(ref32, ref64).max())
    bound = max(4 * base, FP32_FLOOR)
    print(f"{key}: fp32 torch statement vs float64, worst row {base:.3e} -> bound {bound:.3e}")
    assert 0 < base and bound <= FP32_CAP
    return bound


def bf16_ulp(x):
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 7)


def assert_roped(got, ref64, dt, what):
    """A roped row as stored (q_out, appended K): fp32 1e-6 per (row, head); bf16 the float64 value rounded to bf16 within one ulp."""
    if dt == 0:
        assert_rows(got.reshape(*got.shape[:-2], -1), ref64.reshape(*ref64.shape[:-2], -1), FP32_K, what, report=False)
    else:
        want = ref64.to(torch.bfloat16).double()
        ulp = bf16_ulp(torch.maximum(want.abs(), got.double().abs()))
        assert bool(((got.double() - want).abs() <= ulp).all()), f"{what}: more than one bf16 ulp from the float64 RoPE"


# ================================================================================================ caches
def make_cache(g, st, Hkv, lens, grow, maxp, extra=3):
    """lens[b] keys cached per sequence, room for `grow` more.  -> kc, vc [pages, Hkv, 16, 64] (CPU), bt [B, maxp] int32."""
    B = len(lens)
    need = [max(1, -(-(n + grow) // PAGE)) for n in lens]
    assert max(need) <= maxp
    NP = 2 + sum(need) + extra + 1                                  # guard, sequences, unused, trash, guard
    ids = 1 + torch.randperm(NP - 2, generator=g)
    bt = torch.full((B, maxp), int(ids[-1]), dtype=torch.int32)     # unused entries: the trash page
    valid = torch.zeros(NP, PAGE, dtype=torch.bool)
    o = 0
    for b in range(B):
        bt[b, :need[b]] = ids[o:o + need[b]].to(torch.int32)
        o += need[b]
        j = torch.arange(lens[b])
        valid[bt[b, j // PAGE].long(), j % PAGE] = True
    nan = torch.tensor(float("nan"))
    m = valid[:, None, :, None]
    kc = torch.where(m, torch.randn(NP, Hkv, PAGE, D, generator=g) * 0.7, nan).to(st)
    vc = torch.where(m, torch.randn(NP, Hkv, PAGE, D, generator=g), nan).to(st)
    return kc, vc, bt


def assert_cache(kc1, vc1, kc0, vc0, bt, written, what):
    """kc1 / vc1 after, kc0 / vc0 before (CPU); written = [(b, position)].  Everything but those rows is bit-identical."""
    keep = torch.ones(kc0.shape[0], PAGE, dtype=torch.bool)
    for b, p in written:
        keep[int(bt[b, p // PAGE]), p % PAGE] = False
    assert int((~keep).sum()) == len(written)
    for a, z, n in ((kc1, kc0, "kc"), (vc1, vc0, "vc")):
        same = (bits(a) == bits(z)).all(-1).all(1)                  # [pages, 16]
        assert bool(same[keep].all()), f"{what}: {n} changed outside the appended rows, at (page, slot) {(~same & keep).nonzero()[:4].tolist()}"


def assert_appended(kc1, vc1, bt, b, p, k64, v_st, dt, what):
    pg, sl = int(bt[b, p // PAGE]), p % PAGE
    assert torch.equal(bits(vc1[pg, :, sl]), bits(v_st)), f"{what}: appended V is not bit-exact"
    assert_roped(kc1[pg, :, sl], k64, dt, f"{what} appended K")


def padded_rows(x, ld):
    """[B, R, W] fp32 -> the same rows at pitch ld and batch stride R * ld + 40, NaN everywhere else (device)."""
    B, R, W = x.shape
    bs = R * ld + 40
    buf = torch.full((B * bs,), float("nan"))
    for b in range(B):
        buf[b * bs:b * bs + R * ld].view(R, ld)[:, :W] = x[b]
    return buf.cuda(), bs


def unpad(buf, n, B, R, ld, bs, W, what):
    """The guarded output buffer (device) -> [B, R, W] (CPU); guards, slack columns and the gaps between batch items keep the sentinel."""
    assert_guards(buf, n, what)
    body = buf.cpu()[GUARD:GUARD + n]
    wrote = torch.zeros(n, dtype=torch.bool)
    rows = []
    for b in range(B):
        v = body[b * bs:b * bs + R * ld].view(R, ld)
        wrote[b * bs:b * bs + R * ld].view(R, ld)[:, :W] = True
        rows.append(v[:, :W])
    assert bool(is_sentinel(body[~wrote]).all()), f"{what}: a slack element was written"
    return torch.stack(rows)


# ================================================================================================ decode_attn
@functools.lru_cache(maxsize=None)
def decode_case(B, Hq, Hkv, dt, lens, maxp, seed):
    """One decode step of B sequences with lens[b] cached keys: inputs and the reference, built once and left unchanged."""
    g = torch.Generator().manual_seed(seed)
    st = tdt(dt)
    kc, vc, bt = make_cache(g, st, Hkv, lens, 1, maxp)
    qkv = torch.randn(B, 1, (Hq + 2 * Hkv) * D, generator=g)
    ref, _, k64, v_st = kv_ref(qkv, lens, kc, vc, bt, Hq=Hq, Hkv=Hkv, st=st)
    c = dict(B=B, Hq=Hq, Hkv=Hkv, dt=dt, lens=lens, kc=kc, vc=vc, bt=bt, qkv=qkv, ref=ref[:, 0], k64=k64[:, 0], v_st=v_st[:, 0])
    if dt == 0:
        c["ref32"] = kv_ref(qkv, lens, kc, vc, bt, Hq=Hq, Hkv=Hkv, st=st, dtype=torch.float32)[0][:, 0]
    return c


def rope_table(n):
    ang = torch.arange(n, dtype=torch.float32)[:, None] * INV[None, :]
    return torch.cat([ang.cos(), ang.sin()], dim=1).contiguous()                    # as LmModel builds it


def run_decode(ops, c, what, *, tab=True, packed=False, split=False, **kw):
    """One mmx_decode_attn launch on fresh device copies.  -> (out [B, Hq * 64] CPU, whole output buffer, kc, vc after (CPU)).
    Checks the output's guards / slack / padding rows, the appended rows and that the rest of the cache is untouched."""
    B, Hq, Hkv, dt = c["B"], c["Hq"], c["Hkv"], c["dt"]
    K, W = Hq * D, (Hq + 2 * Hkv) * D
    ldqkv, ldo = W + 24, K + 8
    qkv = torch.full((B, ldqkv), float("nan"))
    qkv[:, :W] = c["qkv"][:, 0]
    R = ops.packed_rows(B)
    if split:
        n = (2 if split == "f16" else 3) * R * K
        buf, view = guarded(n, torch.bfloat16)
    elif packed:
        n = R * K
        buf, view = guarded(n, tdt(dt))
    else:
        n = B * ldo
        buf, view = guarded(n, tdt(dt))
    kc, vc = c["kc"].cuda(), c["vc"].cuda()
    ops.decode_attn(qkv.cuda(), INV.cuda(), torch.tensor(c["lens"], dtype=torch.int32).cuda(), kc, vc, c["bt"].cuda(), view, B=B, Hq=Hq,
                    Hkv=Hkv, page=PAGE, dtype=dt, rope_tab=(rope_table(c["bt"].shape[1] * PAGE).cuda() if tab else None),
                    out_packed=packed, out_split=split, ldqkv=ldqkv, ldo=ldo, **kw)
    torch.cuda.synchronize()
    assert_guards(buf, n, what)
    body = buf.cpu()[GUARD:GUARD + n]
    if split:
        planes = body.view(-1, R * K)
        for pl in planes:
            assert bool(is_sentinel(ops.unpack_act(pl, R, K, 1)[B:]).all()), f"{what}: a padding row of a plane was written"
        out = ops.merge_planes(planes, B, K, f16=(split == "f16"))
    elif packed:
        full = ops.unpack_act(body, R, K, dt)
        assert bool(is_sentinel(full[B:]).all()), f"{what}: a padding row of the packed output was written"
        out = full[:B]
    else:
        full = body.view(B, ldo)
        assert bool(is_sentinel(full[:, K:]).all()), f"{what}: a slack column was written"
        out = full[:, :K]
    kc, vc = kc.cpu(), vc.cpu()
    assert_cache(kc, vc, c["kc"], c["vc"], c["bt"], [(b, c["lens"][b]) for b in range(B)], what)
    for b in range(B):
        assert_appended(kc, vc, c["bt"], b, c["lens"][b], c["k64"][b], c["v_st"][b], dt, f"{what} seq {b}")
    return out.contiguous(), body, kc, vc


def decode_bound(c, key):
    return fp32_bound(key, c["ref32"], c["ref"]) if c["dt"] == 0 else BF16_DECODE


# ---- A. two query heads per workgroup against one head per workgroup and against float64
A_SHAPES = [(19, 14, 2), (17, 16, 8), (17, 16, 16)]
A_CTX = [0, 1, 15, 16, 17, 31, 32, 33, 319, 320, 321, 383, 384, 385, 700]          # 320 / 384: keys per pass (fp32 / bf16 cache)
A_MODES = {"f32": (0, {}), "f32-packed": (0, dict(packed=True)), "f32-planes": (0, dict(split=True)),
           "f32-f16planes": (0, dict(split="f16")), "bf16": (1, {}), "bf16-packed": (1, dict(packed=True))}


def a_case(shape, dt):
    B, Hq, Hkv = shape
    g = torch.Generator().manual_seed(B * Hq + Hkv)
    ctx = A_CTX + [A_CTX[int(i)] for i in torch.randperm(len(A_CTX), generator=g)[:B - len(A_CTX)]]
    lens = tuple(ctx[int(i)] for i in torch.randperm(B, generator=g))
    return decode_case(B, Hq, Hkv, dt, lens, 48, 100 + Hkv)


@gpu
@pytest.mark.parametrize("mode", list(A_MODES))
@pytest.mark.parametrize("shape", A_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_decode_attn_two_heads_per_workgroup(env, shape, mode):
    """B * Hq > 256, where mmx_decode_attn picks decode_attn_kernel<T, OM, 2>: the default launch equals one_head=True bit for
    bit (whole output buffer, kc, vc) and both meet the bound against float64, every context of A_CTX in one launch.
    (19, 14, 2): 7 heads over 4 workgroups (the last serves one) and 38 (sequence, kv head) pairs on a grid of 40;
    (17, 16, 16): one head per kv head, so the second head slot of every workgroup is the clamped repeat.
    Planes: the merged bf16 planes equal the row-major fp32 output; the two fp16 planes are within 3e-7 of it (the bounds of
    test_gpu_split.py) and, per element, within 2^-22 |v| + 2^-25 (hi and lo are round-to-nearest fp16 of v and of v - hi, which
    fp32 holds exactly; 2^-25 is half the fp16 subnormal spacing)."""
    L, ops = env
    dt, kw = A_MODES[mode]
    B, Hq, Hkv = shape
    assert B * Hq > 256
    c = a_case(shape, dt)
    tag = f"A {shape} {mode}"
    bound = decode_bound(c, f"A {shape}")
    two = run_decode(ops, c, tag + " default", per_head=True, **kw)
    one = run_decode(ops, c, tag + " one_head", per_head=True, one_head=True, **kw)
    for a, b, n in zip(two[1:], one[1:], ("output", "kc", "vc")):
        assert torch.equal(bits(a), bits(b)), f"{tag}: {n} differs between two heads and one head per workgroup"
    if not kw.get("split"):
        assert_rows(two[0], c["ref"], bound, tag)
        return
    flat = run_decode(ops, c, tag + " row-major", per_head=True)[0]
    assert_rows(flat, c["ref"], bound, tag + " row-major")
    if kw["split"] is True:
        assert torch.equal(two[0], flat), f"{tag}: hi + mid + lo is not the fp32 output"
    else:
        d = (two[0].double() - flat.double()).abs()
        assert float(d.max() / flat.double().abs().max()) < 3e-7
        assert bool((d <= 2.0 ** -22 * flat.double().abs() + 2.0 ** -25).all()), f"{tag}: fp16 hi + lo loses more than the format does"


# ---- B. RoPE computed in the kernel (rope_tab = NULL)
def b_lens(ctx, maxp):
    return (ctx, max(ctx - 7, 0), ctx // 2, ctx, min(ctx + 9, maxp * PAGE - 1))      # as test_decode_attn_one_token


@gpu
@pytest.mark.parametrize("dt,per_head", [(0, False), (1, True), (1, False)], ids=["f32", "bf16-per-head", "bf16-gqa"])
@pytest.mark.parametrize("ctx", [0, 16, 511, 700, 1015])
def test_decode_attn_rope_in_kernel(env, dt, per_head, ctx):
    """cosf / sinf of float32(p) * inv_freq[d] in the kernel (no table) and the table launch, each against float64; positions
    up to 1024, where an angle error of one fp32 ulp (6e-5) would move K by more than the 1e-6 the appended row is held to."""
    L, ops = env
    c = decode_case(5, 14, 2, dt, b_lens(ctx, 66), 66, 200 + ctx)
    bound = decode_bound(c, f"B ctx {ctx}")
    for tab in (False, True):
        for packed in (False, True):
            tag = f"B ctx {ctx} dt {dt} per_head {per_head} tab {tab} packed {packed}"
            out = run_decode(ops, c, tag, tab=tab, packed=packed, per_head=per_head)[0]
            assert_rows(out, c["ref"], bound, tag)


# ---- C. the GQA-shared kernel around its own units
C_CTX = [63, 64, 65, 127, 128, 511, 512, 513, 1023, 1024, 1025]   # a page per wave / two / a full round of 32 pages / the second


@gpu
@pytest.mark.parametrize("B", [1, 5, 19])
@pytest.mark.parametrize("Hkv", [1, 2, 4])
def test_decode_attn_gqa_shared_edges(env, Hkv, B):
    """decode_attn_gqa_kernel (bf16, Hq = 7 Hkv), every context of C_CTX, B per launch, row-major and packed."""
    L, ops = env
    n = len(C_CTX)
    groups = [[C_CTX[(i + k) % n] for k in range(B)] for i in range(0, n, B)]       # every context, B per launch
    for gi, lens in enumerate(groups):
        c = decode_case(B, 7 * Hkv, Hkv, 1, tuple(lens), 66, 300 + 10 * Hkv + gi)
        for packed in (False, True):
            tag = f"C Hkv {Hkv} B {B} ctx {lens} packed {packed}"
            assert_rows(run_decode(ops, c, tag, packed=packed)[0], c["ref"], BF16_DECODE, tag)


# ================================================================================================ E. rope_kv_store + paged_attn
def prefill_case(dt, Hq, Hkv, pos0, steps, maxp, seed, key):
    """Inputs, reference and bound of run_prefill (CPU)."""
    st = tdt(dt)
    g = torch.Generator().manual_seed(seed)
    kc0, vc0, bt = make_cache(g, st, Hkv, pos0, sum(steps), maxp)
    qkv = torch.randn(len(pos0), sum(steps), (Hq + 2 * Hkv) * D, generator=g)
    ref, q64, k64, v_st = kv_ref(qkv, pos0, kc0, vc0, bt, Hq=Hq, Hkv=Hkv, st=st)
    if dt == 0:
        bound = fp32_bound(key, kv_ref(qkv, pos0, kc0, vc0, bt, Hq=Hq, Hkv=Hkv, st=st, dtype=torch.float32)[0], ref)
    else:
        bound = BF16_PAGED
    return kc0, vc0, bt, qkv, ref, q64, k64, v_st, bound


def run_prefill(ops, dt, Hq, Hkv, pos0, steps, maxp, seed, key):
    """Launches of `steps[i]` rows per sequence, one after the other, from positions pos0 on an existing history of pos0[b] keys.
    Reference: kv_ref over all rows at once (causal, so a later launch does not change an earlier row)."""
    st = tdt(dt)
    B, K, W = len(pos0), Hq * D, (Hq + 2 * Hkv) * D
    kc0, vc0, bt, qkv, ref, q64, k64, v_st, bound = prefill_case(dt, Hq, Hkv, pos0, steps, maxp, seed, key)
    kc, vc, btd, inv = kc0.cuda(), vc0.cuda(), bt.cuda(), INV.cuda()
    ldqkv, ldq, ldo = W + 24, K + 8, K + 16
    r0 = 0
    for rows in steps:
        tag = f"{key} dt {dt} rows {r0}..{r0 + rows - 1}"
        pos = torch.tensor([p + r0 for p in pos0], dtype=torch.int32).cuda()
        x, qkv_bs = padded_rows(qkv[:, r0:r0 + rows], ldqkv)
        q_bs, o_bs = rows * ldq + 16, rows * ldo + 24
        qb, qv = guarded(B * q_bs, st)
        ob, ov = guarded(B * o_bs, st)
        ops.rope_kv_store(x, inv, pos, qv, kc, vc, btd, B=B, rows=rows, Hq=Hq, Hkv=Hkv, page=PAGE, dtype=dt, ldqkv=ldqkv, qkv_bs=qkv_bs,
                          ldq=ldq, q_bs=q_bs)
        ops.paged_attn(qv, pos, kc, vc, btd, ov, B=B, rows=rows, Hq=Hq, Hkv=Hkv, page=PAGE, dtype=dt, ldq=ldq, q_bs=q_bs, ldo=ldo, o_bs=o_bs)
        torch.cuda.synchronize()
        q = unpad(qb, B * q_bs, B, rows, ldq, q_bs, K, tag + " q_out")
        out = unpad(ob, B * o_bs, B, rows, ldo, o_bs, K, tag + " out")
        assert_roped(q.reshape(B, rows, Hq, D), q64[:, r0:r0 + rows], dt, tag + " q_out")
        assert_rows(out, ref[:, r0:r0 + rows], bound, tag)
        kc1, vc1 = kc.cpu(), vc.cpu()
        assert_cache(kc1, vc1, kc0, vc0, bt, [(b, pos0[b] + r0 + t) for b in range(B) for t in range(rows)], tag)
        for b in range(B):
            for t in range(rows):
                assert_appended(kc1, vc1, bt, b, pos0[b] + r0 + t, k64[b, r0 + t], v_st[b, r0 + t], dt, f"{tag} seq {b} row {t}")
        kc0, vc0 = kc1, vc1
        r0 += rows


@gpu
@pytest.mark.parametrize("Hq,Hkv", [(14, 2), (4, 4)])
@pytest.mark.parametrize("dt", [0, 1])
def test_rope_kv_store_paged_attn_batched(env, dt, Hq, Hkv):
    """The batched prompt path: B = 3, another pos[b] per sequence, q_out / out / qkv with slack columns and batch gaps.
    20 rows from positions 0 / 13 / 250 (a prefill from empty, pages 0 -> 1 -> 2, contexts 251 .. 270 across paged_attn's
    256-thread stride), then two single rows; 3 rows from 0 / 14 / 254 (contexts 1 .. 3: three of the four waves empty), then one."""
    L, ops = env
    run_prefill(ops, dt, Hq, Hkv, [0, 13, 250], [20, 1, 1], 20, 400 + Hq, f"E ({Hq}, {Hkv}) 20+1+1")
    run_prefill(ops, dt, Hq, Hkv, [0, 14, 254], [3, 1], 20, 500 + Hq, f"E ({Hq}, {Hkv}) 3+1")


# ================================================================================================ F. more than 64 KB of LDS
@gpu
@pytest.mark.parametrize("dt", [0, 1])
def test_paged_attn_above_64k_lds(env, dt):
    """max_pages = 1040: the score row of 16640 positions makes 67.9 KB of dynamic LDS whatever the context (here 6 and 7 keys,
    every table entry but the first names the trash page)."""
    L, ops = env
    run_prefill(ops, dt, 14, 2, [5], [2], 1040, 600, "F paged_attn max_pages 1040")


@gpu
@pytest.mark.parametrize("Tq,Tk,chunk,q_begin", [(8, 1920, 0, 0), (2500, 2500, 50, 2496)])
@pytest.mark.parametrize("dt", [0, 1])
def test_attn_dense_above_64k_lds(env, dt, Tq, Tk, chunk, q_begin):
    """mmx_attn_dense keeps 8 score rows of Tk floats: 64.1 KB at Tk = 1920, 82 KB at 2500.  Per (query row, head) against float64."""
    L, ops = env
    B, H = 1, 2
    g = torch.Generator().manual_seed(Tk)
    q = torch.randn(B, Tq, H * D, generator=g).to(tdt(dt))
    k, v = (torch.randn(B, Tk, H * D, generator=g).to(tdt(dt)) for _ in range(2))
    km = torch.ones(B, Tk)
    km[:, Tk - 9:] = 0
    got = _attn(ops, dt, q.cuda(), k.cuda(), v.cuda(), B=B, H=H, Tq=Tq, Tk=Tk, ldq=H * D, ldk=H * D, ldv=H * D, q_bs=Tq * H * D,
                k_bs=Tk * H * D, v_bs=Tk * H * D, keymask=km.cuda(), chunk=chunk, q_begin=q_begin)
    ref = attn64(q.double(), k.double(), v.double(), H, SCALE, km, chunk)
    assert bool(is_sentinel(got[:, :q_begin]).all())
    assert_rows(got[:, q_begin:], ref[:, q_begin:], ATOL[dt], f"F attn_dense Tk {Tk} dt {dt}")


# ================================================================================================ on the CPU
def dense_ref(qkv, Hq, Hkv, st):
    """The second statement: one sequence from an empty cache, [n, n] causal attention over all its rows, RoPE as cos / sin of
    cat(f, f) and rotate_half (the oracle's form).  qkv [n, (Hq + 2 Hkv) * 64] fp32 -> [n, Hq * 64] float64."""
    n = qkv.shape[0]
    x = qkv.double()
    q = x[:, :Hq * D].view(n, Hq, D).transpose(0, 1)
    k = x[:, Hq * D:(Hq + Hkv) * D].view(n, Hkv, D).transpose(0, 1)
    v = qkv[:, (Hq + Hkv) * D:].view(n, Hkv, D).transpose(0, 1).to(st).double()
    f = (torch.arange(n).float()[:, None] * INV[None, :]).double()
    e = torch.cat([f, f], -1)
    rot = lambda t: torch.cat([-t[..., HALF:], t[..., :HALF]], -1)
    q = q * e.cos() + rot(q) * e.sin()
    k = (k * e.cos() + rot(k) * e.sin()).to(st).double()
    kr, vr = k.repeat_interleave(Hq // Hkv, 0), v.repeat_interleave(Hq // Hkv, 0)
    s = (q @ kr.transpose(-2, -1)) * D ** -0.5
    s = s.masked_fill(~torch.tril(torch.ones(n, n, dtype=torch.bool)), float("-inf"))
    return (torch.softmax(s, -1) @ vr).transpose(0, 1).reshape(n, Hq * D)


@pytest.mark.parametrize("Hq,Hkv", [(14, 2), (4, 4)])
@pytest.mark.parametrize("dt", [0, 1])
def test_kv_ref_matches_dense_restatement(dt, Hq, Hkv):
    """kv_ref in three launches (37 rows from empty, 1 row, 9 rows - each reading the rows before it from a shuffled paged cache
    it was written to) against the dense statement over the 47 rows: 1e-12 per row."""
    st = tdt(dt)
    g = torch.Generator().manual_seed(7 + Hq)
    B, steps = 2, [37, 1, 9]
    kc, vc, bt = make_cache(g, st, Hkv, [0] * B, sum(steps), 5)
    qkv = torch.randn(B, sum(steps), (Hq + 2 * Hkv) * D, generator=g)
    r0 = 0
    for rows in steps:
        out, _, k64, v_st = kv_ref(qkv[:, r0:r0 + rows], [r0] * B, kc, vc, bt, Hq=Hq, Hkv=Hkv, st=st)
        for b in range(B):
            want = dense_ref(qkv[b, :r0 + rows], Hq, Hkv, st)[r0:]
            assert float(row_ratio(out[b], want).max()) < 1e-12
            for t in range(rows):
                p = r0 + t
                kc[int(bt[b, p // PAGE]), :, p % PAGE] = k64[b, t].to(st)
                vc[int(bt[b, p // PAGE]), :, p % PAGE] = v_st[b, t]
        r0 += rows
    whole = kv_ref(qkv, [0] * B, kc, vc, bt, Hq=Hq, Hkv=Hkv, st=st)[0]             # and all rows in one call
    for b in range(B):
        assert float(row_ratio(whole[b], dense_ref(qkv[b], Hq, Hkv, st)).max()) < 1e-12


def test_bf16_rounding_points_fit_the_bounds():
    """The inputs of the bf16 cases (K of scale 0.7, unit V) leave no row whose reference is so small that the kernels' documented
    rounding points alone break its bound: float64 arithmetic with the output rounded to bf16 (decode_attn), and with the
    queries rounded to bf16 as well (rope_kv_store's q_out feeds paged_attn), stays within half of 1e-2 / 2e-2 on every row."""
    for shape in A_SHAPES:
        c = a_case(shape, 1)
        assert float(row_ratio(c["ref"].to(torch.bfloat16), c["ref"]).max()) < BF16_DECODE / 2
    for Hkv in (1, 4):
        c = decode_case(19, 7 * Hkv, Hkv, 1, tuple(C_CTX[k % len(C_CTX)] for k in range(19)), 66, 300 + 10 * Hkv)
        assert float(row_ratio(c["ref"].to(torch.bfloat16), c["ref"]).max()) < BF16_DECODE / 2
    g = torch.Generator().manual_seed(414)
    Hq, Hkv, pos0 = 14, 2, [0, 13, 250]
    kc, vc, bt = make_cache(g, torch.bfloat16, Hkv, pos0, 22, 20)
    qkv = torch.randn(3, 22, (Hq + 2 * Hkv) * D, generator=g)
    ref = kv_ref(qkv, pos0, kc, vc, bt, Hq=Hq, Hkv=Hkv, st=torch.bfloat16)[0]
    emu = kv_ref(qkv, pos0, kc, vc, bt, Hq=Hq, Hkv=Hkv, st=torch.bfloat16, round_q=True)[0].to(torch.bfloat16)
    assert float(row_ratio(emu, ref).max()) < BF16_PAGED / 2
