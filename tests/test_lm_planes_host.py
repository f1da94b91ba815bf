"""The plane formats of the LM decode step, stated on the host (no GPU): ops.split_planes / ops.merge_planes ARE the format
(two fp16 planes hi + lo of MMX_H2, three bf16 planes of MMX_X3; include/mmx_hip.h), and everything the GPU parity tests of
tests/test_gpu_lm_planes.py bound is derived here from the number formats alone.

fp16 has 5 exponent bits: hi = fp16(v) leaves a remainder r = v - hi (exact in fp32) with |r| <= 2^-11 |v|, and lo = fp16(r)
is off by 2^-11 |r| <= 2^-22 |v| while lo is a normal number, by half the subnormal spacing 2^-25 once it is not.  Two planes
therefore hold v to max(2^-22 |v|, 2^-25) - 22 bits only where |v| is well above 2^-3 - and overflow at |v| >= 65520 (the
midpoint between fp16's largest number 65504 and 2^16 rounds to infinity).  Three bf16 planes carry fp32's 8 exponent bits
and hold every fp32 value exactly.

The scale table (printed by test_scale_table; the source of the range sentence in DESIGN.md section 2) is the per-row relative
error of an RMSNorm-consuming projection, float64 on the exact operands against float64 on the operands as the planes hold
them, with the rows at one scale 2^e.  `flush=True` is the same statement for a matrix unit that would read subnormal fp16
operands as zero: the GPU tests use it to tell which of the two the hardware does."""
import math

import torch

from mmx import ops

LADDER = (-20, -14, -10, -6, -3, 0, 3, 6, 9, 12)     # row scales 2^e of the range tests
K, N, ROWS = 128, 64, 19
EPS = 1e-6
H2_BOUND, X3_BOUND = 3e-6, 1e-6                       # per-row bounds of the scale table (H2: at scales >= 2^H2_LOW_EDGE)
H2_LOW_EDGE = -6
F16_MIN_NORMAL = 2.0 ** -14


def h2_elem_bound(v):
    """What two fp16 planes may be off by, per element (see the module docstring)."""
    return torch.maximum(v.double().abs() * 2.0 ** -22, torch.full_like(v, 2.0 ** -25, dtype=torch.float64))


def h2_store_bound(v):
    """h2_elem_bound plus one fp32 rounding of v: planes of a product a kernel formed in fp32, against that product recomputed."""
    return h2_elem_bound(v) + v.double().abs() * 2.0 ** -24


def held(v, f16=True, flush=False):
    """fp32 [B, K] -> float64 [B, K]: the value the planes of ops.split_planes hold.  flush: every subnormal fp16 term reads as
    zero."""
    B, Kv = v.shape
    xs = ops.split_planes(v, f16=f16)
    if flush:
        assert f16
        h = xs.view(torch.float16)
        xs = torch.where(h.abs() < F16_MIN_NORMAL, torch.zeros_like(h), h).view(torch.bfloat16)
    return ops.merge_planes(xs, B, Kv, f16=f16).double()


def row_err(got, ref):
    """Per row: max |got - ref| over the row / max |ref| of that row."""
    got, ref = got.double(), ref.double()
    return (got - ref).abs().amax(-1) / ref.abs().amax(-1)


def ladder_rows(B, Kv, seed, exps=LADDER):
    """[B, Kv] fp32: row r is randn * 2^exps[r % len(exps)] - one matrix whose rows lie 2^32 apart - and the exponent of each row."""
    g = torch.Generator().manual_seed(seed)
    e = torch.tensor([exps[r % len(exps)] for r in range(B)], dtype=torch.float64)
    x = (torch.randn(B, Kv, generator=g, dtype=torch.float64) * torch.exp2(e)[:, None]).float()
    return x, [int(v) for v in e]


def massive_rows(B, Kv, seed, cols=(5, 77)):
    """[B, Kv] fp32 at scale 1 with two massive-activation channels (columns * 2^11; |x * gamma| peaks near 6e3)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Kv, generator=g)
    for c in cols:
        x[:, c % Kv] *= 2.0 ** 11
    return x


def weights(Nw, Kv, seed, bf16=True):
    """[Nw, Kv] projection weights ~ 1/sqrt(K); bf16-representable (what MMX_H2 packs exactly) or general fp32 (MMX_H2W)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(Nw, Kv, generator=g) / math.sqrt(Kv)
    return w.to(torch.bfloat16).float() if bf16 else w


def gain(Kv, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.1 * torch.randn(Kv, generator=g)


def proj64(v, x, w):
    """float64 of the RMSNorm-consuming projection: (v @ w^T) * rsqrt(mean(x^2) + eps), v = the operand x * gamma (as held)."""
    return (v.double() @ w.double().t()) * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + EPS)


def scale_table(seed=0):
    """{e: (two fp16 planes, the same with subnormal terms flushed, three bf16 planes)}: the largest per-row error of ROWS rows at
    scale 2^e."""
    w, gam = weights(N, K, seed + 1), gain(K, seed + 2)
    out = {}
    for e in LADDER:
        x, _ = ladder_rows(ROWS, K, seed + 100 + e, exps=(e,))
        v = x * gam
        ref = proj64(v, x, w)
        out[e] = tuple(float(row_err(proj64(held(v, **kw), x, w), ref).max())
                       for kw in (dict(f16=True), dict(f16=True, flush=True), dict(f16=False)))
    return out


def format_table(tab, extra=None):
    """The scale table as text; extra: {name: {e: value}} columns measured elsewhere (the kernels)."""
    names = ["2 fp16 planes", "  ... flushed", "3 bf16 planes"] + list(extra or {})
    lines = ["row scale " + " ".join(f"{n:>14s}" for n in names)]
    for e in LADDER:
        vals = list(tab[e]) + [extra[n].get(e, float("nan")) for n in (extra or {})]
        lines.append(f"2^{e:<7d} " + " ".join(f"{v:14.2e}" for v in vals))
    return "\n".join(lines)


def test_element_bound():
    """|merge(split(v)) - v| over 2^-30 .. 2^15.99, both signs, zeros: two fp16 planes within max(2^-22 |v|, 2^-25), three bf16
    planes exact."""
    mag = torch.exp2(torch.linspace(-30.0, 15.99, 4064, dtype=torch.float64))
    v = torch.cat([mag, -mag, torch.zeros(64, dtype=torch.float64)]).float().reshape(64, 128)
    assert float(v.abs().max()) < 65504.0 and int((v == 0).sum()) == 64
    err = (held(v, f16=True) - v.double()).abs()
    assert bool((err <= h2_elem_bound(v)).all()), float((err / h2_elem_bound(v)).max())
    # the bound is attained to within 4x at both ends: it is the format's, not a loose one
    big, small = v.abs() >= 1.0, (v != 0) & (v.abs() < 2.0 ** -16)
    assert float((err / h2_elem_bound(v))[big].max()) > 0.25 and float((err / h2_elem_bound(v))[small].max()) > 0.25
    assert torch.equal(held(v, f16=False), v.double())
    assert float(held(v, f16=True)[v == 0].abs().max()) == 0.0


def test_overflow_edges():
    """|v| >= 65520 makes the fp16 planes non-finite (hi = inf, lo = v - inf = -inf: their sum is NaN), 65519 does not; three bf16
    planes stay finite (and exact) at 2^17."""
    v = torch.zeros(16, 32)
    v[0, 0], v[1, 1], v[2, 2], v[3, 3], v[4, 4] = 65519.0, -65519.0, 65520.0, -65520.0, 2.0 ** 17
    ok = ops.split_planes(v[:2].clone(), f16=True).view(torch.float16)
    assert bool(torch.isfinite(ok).all())
    assert bool(((held(v[:2].clone()) - v[:2].double()).abs() <= h2_elem_bound(v[:2])).all())
    for r in (2, 3, 4):
        one = torch.zeros(16, 32)
        one[r, r] = v[r, r]
        planes = ops.split_planes(one, f16=True).view(torch.float16)
        assert int((~torch.isfinite(planes)).sum()) == 2, r                  # hi and lo of that one element
        assert bool(torch.isnan(ops.merge_planes(planes.view(torch.bfloat16), 16, 32, f16=True)[r, r]))
    x3 = ops.split_planes(v, f16=False)
    assert bool(torch.isfinite(x3.float()).all()) and torch.equal(ops.merge_planes(x3, 16, 32), v)


def test_scale_table(capsys):
    """The table of the module docstring.  Two fp16 planes meet 3e-6 per row at every scale >= 2^-6 and lose it below; three bf16
    planes meet 1e-6 at every scale; the flushed form is more than 16x worse at every scale <= 2^-3, which is what lets the GPU
    test tell a flushing matrix unit from one that keeps subnormal operands."""
    tab = scale_table()
    with capsys.disabled():
        print("\nper-row relative error of a K = 128 projection from the plane formats alone (float64, 19 rows per scale):")
        print(format_table(tab))
    for e in LADDER:
        h2, flushed, x3 = tab[e]
        assert x3 <= X3_BOUND, (e, x3)
        if e >= H2_LOW_EDGE:
            assert h2 <= H2_BOUND, (e, h2)
        if e <= -3:
            assert flushed > 16 * h2, (e, flushed, h2)
    # the lower edge is an edge: the next ladder scale below it misses the bound
    assert tab[-10][0] > H2_BOUND
