"""Which requests the LM decode entry points accept, and that every form they can launch computes the right thing.

mmx_skinny_gemm, mmx_skinny2 and mmx_decode_attn_fin each select one kernel instantiation from a table (csrc/llm.hip, csrc/decode.hip).
Every sweep below walks the whole request space at a small shape.  Whether a request is accepted is written here as the rule
include/mmx_hip.h documents (skinny_accepts, skinny2_accepts, decode_attn_accepts) - it is not read back from the library.  An
accepted request must match float64 math on the same values within the bound the existing test of that kernel and dtype uses
(named beside each table of bounds); a refused one must raise MmxError and leave every output, NaN-filled beforehand, as it was.

sweep_*() yield (case id, accepted, run); run() launches on fresh outputs and returns (outputs, reference) - tools that compare
two builds of the library bit for bit walk the same generators."""
import ctypes
import functools
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, BF16, X2, X3, X3W, H2, H2W = 0, 1, 2, 3, 0x13, 4, 0x14
NAN = float("nan")


@pytest.fixture(scope="module")
def env():
    from mmx import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    _lib.load()
    return _lib, ops


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


def bits(t):
    """The elements as integers: comparisons that hold for NaN too."""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def check_sweep(L, cases):
    """-> (accepted, refused) counts.  cases: (id, accepted, run) with run() -> ([(name, got, ref, bound)], [output buffers])."""
    n = [0, 0]
    for cid, accepted, run in cases:
        if accepted:
            checks, _ = run()
            for name, got, ref, bound in checks:
                assert bool(torch.isfinite(got.float()).all()), (cid, name, "not finite")
                err = rel_err(got, ref)
                assert err < bound, (cid, name, err, bound)
        else:
            state = {}
            with pytest.raises(L.MmxError):
                run(state)
            for before, after in state["kept"]:
                assert torch.equal(bits(before), bits(after)), (cid, "a refused request wrote to an output")
        n[0 if accepted else 1] += 1
    torch.cuda.synchronize()
    return tuple(n)


# ================================================================================================ mmx_skinny_gemm
SK_K, SK_N = 96, 64
SK_B = (1, 17, 33, 49, 65)                                  # MT 1..4, and one row tile too many
# tests/test_gpu_kernels.py::test_skinny_gemm (F32, BF16), tests/test_gpu_split.py::test_skinny_gemm_split (X2, X3)
SK_TOL = {F32: 3e-5, BF16: 1.5e-2, X2: 4e-5, X3: 3e-6}


def skinny_accepts(dtype, xdt, flags, epi, kgamma, B):
    """include/mmx_hip.h, mmx_skinny_gemm: B <= 64, epi 0..2; the split builds take fp32 row-major x (kgamma optional); the packed
    layouts are for x of the weights' type T, as X_PACKED alone or with OUT_PACKED; x is fp32 or T; MMX_BF16 with fp32 row-major x
    also takes kgamma, with epi 0 / 1."""
    if B > 64 or epi not in (0, 1, 2):
        return False
    if dtype in (X2, X3):
        return xdt == F32 and flags == 0
    if kgamma:
        return dtype == BF16 and xdt == F32 and flags == 0 and epi in (0, 1)
    if flags not in (0, 1, 3) or (flags and xdt != dtype):
        return False
    return xdt == F32 or (dtype == BF16 and xdt == BF16)


@functools.lru_cache(maxsize=None)
def skinny_data(B):
    g = torch.Generator().manual_seed(1000 + B)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=(r(B, SK_K) * 3).cuda(), w=(r(SK_N, SK_K) / math.sqrt(SK_K)).bfloat16().float().cuda(),
                w2=(r(2 * SK_N, SK_K) / math.sqrt(SK_K)).bfloat16().float().cuda(), gam=(1 + 0.1 * r(SK_K)).cuda(),
                bias=r(SK_N).cuda(), res=r(B, SK_N).cuda())


@functools.lru_cache(maxsize=None)
def skinny_pack(B, dtype, glu):
    from mmx import _lib, ops
    d = skinny_data(B)
    w = d["w2"] if glu else d["w"]                           # bf16-representable: every build holds the same values
    return ops.pack_skinny(w.to(_lib.WEIGHT_DT[dtype]).contiguous(), dtype=dtype, interleave_half=(SK_N if glu else 0))


def sweep_skinny_gemm(ops):
    K, N = SK_K, SK_N
    for dtype, xdt, flags, epi, kg, B in itertools.product((F32, BF16, X2, X3), (F32, BF16), (0, 1, 3, 2), range(4), (False, True), SK_B):
        def run(state=None, dtype=dtype, xdt=xdt, flags=flags, epi=epi, kg=kg, B=B):
            d, split = skinny_data(B), dtype in (X2, X3)
            tdt = torch.bfloat16 if dtype == BF16 else torch.float32
            xv = d["x"].bfloat16() if xdt == BF16 else d["x"]
            of = d["res"].clone() if epi == 2 else torch.full((B, N), NAN, device="cuda")
            oa = torch.full((ops.packed_rows(B) * N,), NAN, device="cuda", dtype=tdt)
            outs = dict(out_f32=of) if split else dict(out_act=oa) if epi == 1 else dict(out_f32=of, out_act=oa)
            if state is not None:
                state["kept"] = [(t.clone(), t) for t in outs.values()]
            ops.skinny_gemm(ops.pack_act(xv, dtype) if flags & 1 else xv, skinny_pack(B, dtype, epi == 1), B=B, K=K, N=N, dtype=dtype,
                            bias=(d["bias"] if epi == 0 else None), rs=(epi != 2), eps=1e-6, epi=epi, x_packed=bool(flags & 1),
                            out_packed=bool(flags & 2), kgamma=(d["gam"] if kg else None), **outs)
            acc = (xv.double() * (d["gam"].double() if kg else 1.0)) @ (d["w2"] if epi == 1 else d["w"]).double().t()
            if epi != 2:
                acc = acc * torch.rsqrt(xv.double().pow(2).mean(-1, keepdim=True) + 1e-6)
            ref = acc + d["bias"].double() if epi == 0 else F.silu(acc[:, :N]) * acc[:, N:] if epi == 1 else d["res"].double() + acc
            got = {k: (v if k == "out_f32" else ops.unpack_act(v, B, N, dtype) if flags & 2 else v[:B * N].view(B, N)) for k, v in outs.items()}
            return [(k, v, ref, SK_TOL[dtype]) for k, v in got.items()], list(outs.values())
        yield f"skinny_gemm dtype {dtype} x {xdt} flags {flags} epi {epi} kgamma {int(kg)} B {B}", skinny_accepts(dtype, xdt, flags, epi, kg, B), run


def test_skinny_gemm_requests(env):
    """Every (dtype, x_dtype, flags, epi, kgamma) at B = 1, 17, 33, 49 (MT 1..4) and 65, K = 96, N = 64: the accepted set is the
    documented one, and every accepted request - each of the 108 instantiations is one - matches float64."""
    L, ops = env
    ok, no = check_sweep(L, sweep_skinny_gemm(ops))
    # 27 table rows x 4 MT, + kgamma on the 6 split rows and on 2 of the bf16 / fp32-x rows
    assert (ok, ok + no) == ((27 + 6 + 2) * 4, 4 * 2 * 4 * 4 * 2 * 5)


# ================================================================================================ mmx_skinny2
S2_K, S2_N = 128, 64
# tests/test_gpu_split.py::test_skinny2_vs_float64 (X3), ::test_weight_planes_skinny2_vs_float64 (X3W),
# ::test_skinny2_fp16_planes_vs_float64 (H2, H2W); one bf16 plane x bf16 weights is the arithmetic of the bf16 skinny GEMM:
# tests/test_gpu_kernels.py::test_skinny_gemm
S2_TOL = {X3: 3e-6, X3W: 3e-6, H2: 3e-6, H2W: 3e-6, BF16: 1.5e-2}


def skinny2_accepts(dtype, B, tw, epi, ksplit):
    """include/mmx_hip.h, mmx_skinny2: B <= 32; tiles_per_wg 1 | 2 (three weight planes in registers, MMX_X3W: 1 only);
    ksplit > 1 with epi 2 only."""
    return B <= 32 and tw in ((1,) if dtype == X3W else (1, 2)) and (ksplit == 1 or epi == 2)


@functools.lru_cache(maxsize=None)
def skinny2_data(B, dtype, glu):
    from mmx import ops
    g = torch.Generator().manual_seed(2000 + B)
    r = lambda *s: torch.randn(*s, generator=g)
    x, gam, gnext, bias, res = (r(B, S2_K) * 3).cuda(), (1 + 0.1 * r(S2_K)).cuda(), (1 + 0.1 * r(S2_N)).cuda(), r(S2_N).cuda(), r(B, S2_N).cuda()
    w = (r(2 * S2_N if glu else S2_N, S2_K) / math.sqrt(S2_K)).bfloat16().float().cuda()
    half = S2_N if glu else 0
    if dtype in (H2, H2W):
        wp = ops.pack_skinny_h2(w, planes=(2 if dtype == H2W else 1), interleave_half=half)
    elif dtype == X3W:
        wp = ops.pack_skinny(w, dtype=X3W, interleave_half=half)
    else:
        wp = ops.pack_skinny(w.bfloat16().contiguous(), dtype=dtype, interleave_half=half)
    ssq = torch.zeros(32, 64, device="cuda")
    ssq[:B, :S2_K // 16] = x.double().pow(2).reshape(B, S2_K // 16, 16).sum(-1).float()[:32]        # (B = 33 is refused before it is read)
    return dict(x=x, gam=gam, gnext=gnext, bias=bias, res=res, w=w, wp=wp, ssq=ssq)


def planes_of(ops, x, dtype):
    if dtype == BF16:
        return ops.pack_act(x.bfloat16(), BF16)[None]
    return ops.split_planes(x, f16=dtype in (H2, H2W))


def merged(ops, xs, B, N, dtype):
    if dtype == BF16:
        return ops.unpack_act(xs[0], B, N, BF16).float()
    return ops.merge_planes(xs, B, N, f16=dtype in (H2, H2W))


def sweep_skinny2(ops):
    K, N = S2_K, S2_N
    for dtype, B, tw, epi, J in itertools.product((X3, X3W, BF16, H2, H2W), (1, 17, 33), (1, 2, 3), range(3), (1, 2)):
        def run(state=None, dtype=dtype, B=B, tw=tw, epi=epi, J=J):
            d = skinny2_data(B, dtype, epi == 1)
            rs, nt, R = epi != 2, (N + 15) // 16, ops.packed_rows(B)
            xs = planes_of(ops, d["x"] * d["gam"] if rs else d["x"], dtype)
            out = d["res"].clone() if epi == 2 else torch.full((B, N), NAN, device="cuda") if epi == 0 else None
            xs_out = torch.full((xs.shape[0], R * N), NAN, dtype=torch.bfloat16, device="cuda") if epi else None
            ssq_out = torch.zeros(32, 64, device="cuda") if epi == 2 else None
            part = torch.full((J * ((nt + 2) // 3 * 3) * (R // 4) * 64,), NAN, device="cuda") if J > 1 else None
            tickets = torch.zeros(nt, dtype=torch.int32, device="cuda") if J > 1 else None
            if state is not None:
                state["kept"] = [(t.clone(), t) for t in (out, xs_out, ssq_out) if t is not None]
            # (ops.skinny2 turns X3 / H2 into X3W / H2W for a weight-plane pack)
            ops.skinny2(xs, d["wp"], B=B, K=K, N=N, dtype={X3W: X3, H2W: H2}.get(dtype, dtype), bias=(d["bias"] if epi == 0 else None),
                        ssq_in=(d["ssq"] if rs else None), eps=1e-6, epi=epi, out=out, xs_out=xs_out, gamma_next=(d["gnext"] if epi == 2 else None),
                        ssq_out=ssq_out, tiles_per_wg=tw, ksplit=J, part=part, tickets=tickets)
            acc = (d["x"].double() * (d["gam"].double() if rs else 1.0)) @ d["w"].double().t()
            if rs:
                acc = acc * torch.rsqrt(d["x"].double().pow(2).mean(-1, keepdim=True) + 1e-6)
            ref = acc + d["bias"].double() if epi == 0 else F.silu(acc[:, :N]) * acc[:, N:] if epi == 1 else d["res"].double() + acc
            checks = [("out", merged(ops, xs_out, B, N, dtype) if epi == 1 else out, ref, S2_TOL[dtype])]
            if epi == 2:
                checks.append(("planes of out * gamma_next", merged(ops, xs_out, B, N, dtype), ref * d["gnext"].double(), S2_TOL[dtype]))
            return checks, [t for t in (out, xs_out, ssq_out) if t is not None]
        yield f"skinny2 dtype {dtype} B {B} tiles_per_wg {tw} epi {epi} ksplit {J}", skinny2_accepts(dtype, B, tw, epi, J), run


def test_skinny2_requests(env):
    """The five dtypes at B = 1, 17 (MT 1, 2) and 33, tiles_per_wg 1..3, epi 0..2, ksplit 1 | 2, K = 128, N = 64: the accepted
    set is the documented one and every accepted request - each of the 54 instantiations is one - matches float64."""
    L, ops = env
    ok, no = check_sweep(L, sweep_skinny2(ops))
    assert (ok, ok + no) == (54 + 54 // 3, 5 * 3 * 3 * 3 * 2)              # every form, and its epi 2 once more with ksplit 2


# ================================================================================================ mmx_decode_attn_fin
DA_B, DA_POS, D = 3, (0, 16, 40), 64
DA_TOL = {F32: 2e-5, BF16: 1e-2}                            # tests/test_gpu_kernels.py::test_decode_attn_one_token


def decode_attn_accepts(L, dt, b):
    """include/mmx_hip.h, MMX_DA_*: the plane outputs are for dtype MMX_F32, without MMX_DA_PACKED, one kind at a time."""
    planes = b & (L.DA_SPLIT | L.DA_H2)
    return not planes or (dt == F32 and not b & L.DA_PACKED and planes != (L.DA_SPLIT | L.DA_H2))


@functools.lru_cache(maxsize=None)
def decode_attn_data(dt, Hq, Hkv, page):
    """One decode step of DA_B sequences with DA_POS cached keys; the float64 reference (RoPE angle: the fp32 product
    float32(p) * inv_freq, as the model's table holds it), the new K / V rounded to the cache's type."""
    g = torch.Generator().manual_seed(3000 + Hq + page)
    st = torch.bfloat16 if dt == BF16 else torch.float32
    maxp = 4
    bt = torch.randperm(DA_B * maxp, generator=g).to(torch.int32).reshape(DA_B, maxp)
    kc = (torch.randn(DA_B * maxp, Hkv, page, D, generator=g) * 0.7).to(st)
    vc = torch.randn(DA_B * maxp, Hkv, page, D, generator=g).to(st)
    qkv = torch.randn(DA_B, (Hq + 2 * Hkv) * D, generator=g)
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.int64).float() / D))
    ang = torch.arange(maxp * page, dtype=torch.float32)[:, None] * inv[None, :]
    ref = torch.zeros(DA_B, Hq * D, dtype=torch.float64)
    for b, p in enumerate(DA_POS):
        c, s = ang[p].double().cos(), ang[p].double().sin()
        rope = lambda x: torch.cat([x[..., :32] * c - x[..., 32:] * s, x[..., 32:] * c + x[..., :32] * s], -1)
        x = qkv[b].double()
        q = rope(x[:Hq * D].view(Hq, D))
        kn = rope(x[Hq * D:(Hq + Hkv) * D].view(Hkv, D)).to(st).double()
        vn = qkv[b, (Hq + Hkv) * D:].view(Hkv, D).to(st).double()
        j = torch.arange(p)
        kk = torch.cat([kc[bt[b, j // page].long(), :, j % page].double(), kn[None]], 0)      # [p + 1, Hkv, D]
        vv = torch.cat([vc[bt[b, j // page].long(), :, j % page].double(), vn[None]], 0)
        kk, vv = (t.transpose(0, 1).repeat_interleave(Hq // Hkv, 0) for t in (kk, vv))          # [Hq, p + 1, D]
        sc = torch.einsum("hd,hnd->hn", q, kk) * 0.125
        ref[b] = torch.einsum("hn,hnd->hd", torch.softmax(sc, -1), vv).reshape(Hq * D)
    return dict(bt=bt.cuda(), kc=kc.cuda(), vc=vc.cuda(), qkv=qkv.cuda(), inv=inv.cuda(), tab=torch.cat([ang.cos(), ang.sin()], 1).contiguous().cuda(),
                pos=torch.tensor(DA_POS, dtype=torch.int32).cuda(), ref=ref.cuda())


def sweep_decode_attn(L, ops):
    for b, dt, (Hq, Hkv), page in itertools.product(range(32), (F32, BF16), ((14, 2), (4, 2)), (16, 32)):
        def run(state=None, b=b, dt=dt, Hq=Hq, Hkv=Hkv, page=page):
            d = decode_attn_data(dt, Hq, Hkv, page)
            B, K, R = DA_B, Hq * D, ops.packed_rows(DA_B)
            split = "f16" if b & L.DA_H2 else bool(b & L.DA_SPLIT)
            # (a refused request names no single output form: room for the largest, three planes)
            out = torch.full((3, R * K), NAN, dtype=(torch.bfloat16 if split or dt == BF16 else torch.float32), device="cuda")
            kc, vc = d["kc"].clone(), d["vc"].clone()
            if state is not None:
                state["kept"] = [(out.clone(), out), (d["kc"], kc), (d["vc"], vc)]
            # (straight through the C ABI: ops.decode_attn has no spelling for both kinds of planes at once)
            p = L._p
            L.check(L.load().mmx_decode_attn_fin(p(d["qkv"]), L.i64((Hq + 2 * Hkv) * D), B, Hq, Hkv, D, p(d["inv"]), p(d["tab"]), p(d["pos"]), None,
                                                 p(kc), p(vc), p(d["bt"]), d["bt"].shape[1], page, ctypes.c_float(0.125), p(out), L.i64(K), dt, b,
                                                 L.stream()), "mmx_decode_attn_fin")
            flat = out.view(-1)
            got = (ops.merge_planes(out[:2 if split == "f16" else 3], B, K, f16=(split == "f16")) if split else
                   ops.unpack_act(flat[:R * K], B, K, dt) if b & L.DA_PACKED else flat[:B * K].view(B, K))
            return [("out", got, d["ref"], DA_TOL[dt])], [out, kc, vc]
        yield f"decode_attn bits {b} dtype {dt} heads {Hq}/{Hkv} page {page}", decode_attn_accepts(L, dt, b), run


def test_decode_attn_requests(env):
    """The 32 patterns of the MMX_DA_* bits for fp32 and bf16 caches, 14 / 2 and 4 / 2 heads, pages of 16 and 32 keys, three
    sequences with 0, 16 and 40 cached keys: the accepted set is the documented one (the bits ops.decode_attn_bits builds are the
    header's) and every accepted request matches float64; a refused one leaves the output and the cache alone."""
    L, ops = env
    assert [ops.decode_attn_bits(out_packed=b & 1, per_head=b & 2, out_split=("f16" if b & 8 else bool(b & 4)), one_head=b & 16)
            for b in range(32) if b & 12 != 12] == [b for b in range(32) if b & 12 != 12]
    ok, no = check_sweep(L, sweep_decode_attn(L, ops))
    # fp32: 8 patterns of (PACKED, PER_HEAD, ONE_HEAD) without planes + 4 + 4 with one kind of planes and no PACKED; bf16: the 8
    assert (ok, ok + no) == ((16 + 8) * 4, 32 * 2 * 2 * 2)
