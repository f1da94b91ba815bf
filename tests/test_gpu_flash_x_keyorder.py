"""Key order of the P V product of attn_flash_x_kernel (csrc/attention_x.hip): the kernel takes the P operand straight from the S^T
accumulators, so k-slot (g, j) of k-step ks is key 32 ks + 16 (j >> 2) + 4g + (j & 3), and the V^T image in LDS is stored in that order.
A P element multiplied with the wrong key's V row is an error that bounded random data can hide; a one-hot P cannot.

Inputs, exact in bf16 (so both entry points, fp32 operands and pre-split planes, see the same numbers and every lo plane is zero):
  K[j]    64 pseudo-random +-1 (generator seeded with T), the same for every batch member and head
  tgt     a target key per (batch member, head, query), uniform over the keys visible to the query
  Q[q]    8 K[tgt[q]]                    V[j][d] = ((7 j + 3 d) mod 251) - 125                    scale = 0.125
The target's score is 64, every other key's is K[j] . K[tgt] <= 32 (test_inputs_are_one_hot, CPU: the gap is 32 .. 38 at the T used
here), so P is one-hot to e^-32 and the output row is V[tgt[q]]: the float64 softmax is within 3e-12 of it.  A wrong key changes
at least one of the 64 channels by >= 1 (7 j mod 251 is injective for j < 251).

Tolerance 1e-3 absolute.  The kernel's only inexact step on these inputs is o * (1 / l) with l = 1 + (T - 1) e^-32 at most and
|V| <= 125: about 1e-5.  1e-3 is two orders above that and three below the smallest error of a misplaced key.

Cases: both entry points; T = 72 (one full tile and one of 8 keys), 130 and 250 (several tiles, the last ragged); klen ragged across the
batch with lengths that are no multiple of 16; chunk = 50 and q_begin = 64 at T = 130; forms 0 .. 3 of mmx_attn_flash_xs with B from the
dispatch rule (restated in kernel_of) so that <1,true,4>, <1,true,8> and <2,true,8> all run.  Form 0 is launched at the small grid
and at the two grids (B = 24, T = 130; B = 12, T = 250) between which the former per-launch rule switched to the 256-query form; it
now reaches <1,true,8> at both, and <2,true,8> is reached through form 2 only.
Judged: every row q_begin <= q < klen[b]; rows from klen[b] on are padding (under a quarter of the rows of every case)."""
import functools
from collections import namedtuple

import pytest
import torch

gpu = pytest.mark.gpu

H, D, SCALE, TOL = 8, 64, 0.125, 1e-3
W = H * D
Case = namedtuple("Case", "entry form B T mode kernel")


def ceil_div(a, b):
    return (a + b - 1) // b


def kernel_of(entry, form, B, T, qb):
    """mmx_attn_flash_x / mmx_attn_flash_xs of csrc/attention_x.hip, restated."""
    npairs, Tq = H * B, T - qb
    small = npairs * ceil_div(Tq, 128) < 192
    if entry == "x":
        return "<1,false,4>" if small else "<1,false,8>"
    if small or form == 3:
        return "<1,true,4>"
    return "<2,true,8>" if form == 2 else "<1,true,8>"


def spec(c):
    """-> (chunk, q_begin, klen list or None)."""
    klen = None
    if c.mode == "klen":
        klen = [c.T] * c.B
        klen[1] = c.T - 29                                 # 43 / 101 / 221: no multiple of 16
        if c.B > 2:
            klen[4], klen[7] = c.T - 53, c.T - 16
    return (50 if c.mode == "chunk" else 0), (64 if c.mode == "qbegin" else 0), klen


MODES = [(72, "none"), (130, "klen"), (130, "chunk"), (130, "qbegin"), (250, "klen")]


def mk(entry, form, B, T, mode):
    qb = 64 if mode == "qbegin" else 0
    return Case(entry, form, B, T, mode, kernel_of(entry, form, B, T, qb))


def cases_for(entry, form, want):
    """One case per mode with the smallest B of 2, 12, 24 whose launch reaches `want`."""
    out = []
    for T, mode in MODES:
        hit = [c for c in (mk(entry, form, B, T, mode) for B in (2, 12, 24)) if c.kernel == want]
        assert hit, (entry, form, want, T, mode)
        out.append(hit[0])
    return out


CASES = cases_for("x", 0, "<1,false,4>") + cases_for("x", 0, "<1,false,8>") + \
    cases_for("xs", 3, "<1,true,4>") + cases_for("xs", 1, "<1,true,8>") + cases_for("xs", 2, "<2,true,8>") + \
    [mk("xs", 0, 2, 130, "klen"), mk("xs", 0, 12, 250, "klen"), mk("xs", 0, 24, 130, "chunk"), mk("xs", 0, 24, 130, "klen")]


def cid(c):
    return f"{c.entry}{c.kernel}-B{c.B}-T{c.T}-{c.mode}" + (f"-form{c.form}" if c.entry == "xs" else "")


def test_cases_reach_every_instantiation():
    assert {c.kernel for c in CASES if c.entry == "x"} == {"<1,false,4>", "<1,false,8>"}
    for form, want in ((0, {"<1,true,4>", "<1,true,8>"}), (1, {"<1,true,8>"}), (2, {"<2,true,8>"}), (3, {"<1,true,4>"})):
        assert {c.kernel for c in CASES if c.entry == "xs" and c.form == form} == want, form
    assert len({cid(c) for c in CASES}) == len(CASES)
    for c in CASES:                                        # padding rows: under a quarter of the rows
        klen = spec(c)[2]
        if klen:
            assert any(n % 16 for n in klen) and sum(c.T - n for n in klen) * 4 < c.B * c.T


@functools.lru_cache(maxsize=None)
def keys_values(T):
    g = torch.Generator().manual_seed(T)
    k = (torch.randint(0, 2, (T, D), generator=g) * 2 - 1).float()
    j, d = torch.arange(T)[:, None], torch.arange(D)[None, :]
    return k, ((7 * j + 3 * d) % 251 - 125).float()


@functools.lru_cache(maxsize=None)
def targets(B, T, mode):
    """-> (tgt [B, H, T] long, nvis [B, T]: the keys 0 .. nvis - 1 are the ones visible to the query; 0 for a padding row)."""
    c = Case("", 0, B, T, mode, "")
    chunk, _, klen = spec(c)
    q = torch.arange(T)
    tk = torch.tensor(klen if klen else [T] * B)
    nvis = tk[:, None].expand(B, T).clone()
    if chunk:
        nvis = torch.minimum(nvis, ((q // chunk + 1) * chunk)[None, :])
    nvis = torch.where(q[None, :] < tk[:, None], nvis, torch.zeros_like(nvis))
    g = torch.Generator().manual_seed(T * 100 + B)
    u = torch.rand(B, H, T, generator=g, dtype=torch.float64)
    tgt = (u * nvis[:, None, :]).long().clamp(max=T - 1)
    return torch.minimum(tgt, (nvis[:, None, :] - 1).clamp(min=0)), nvis


def operands(c):
    """-> q, k, v [B, T, H * D] fp32 (exact in bf16), want [B, T, H * D] = V[tgt], judged [B, T] bool."""
    k1, v1 = keys_values(c.T)
    tgt, nvis = targets(c.B, c.T, c.mode)
    q = (8.0 * k1[tgt]).permute(0, 2, 1, 3).reshape(c.B, c.T, W)               # [B, H, T, D] -> [B, T, H * D]
    want = v1[tgt].permute(0, 2, 1, 3).reshape(c.B, c.T, W)
    k = k1[None, :, None, :].expand(c.B, c.T, H, D).reshape(c.B, c.T, W).contiguous()
    v = v1[None, :, None, :].expand(c.B, c.T, H, D).reshape(c.B, c.T, W).contiguous()
    judged = (nvis > 0) & (torch.arange(c.T)[None, :] >= spec(c)[1])
    return q.contiguous(), k, v, want, judged


@pytest.mark.parametrize("T", sorted({T for T, _ in MODES}))
def test_inputs_are_one_hot(T):
    """The score gap of the key set (exact: +-1 integers), the float64 softmax against V[tgt], and the bf16 exactness of the operands."""
    k1, v1 = keys_values(T)
    gram = k1 @ k1.t()
    gram.fill_diagonal_(-64.0)
    assert 64.0 - float(gram.max()) >= 32.0
    for x in (8.0 * k1, k1, v1):
        assert bool((x.bfloat16().float() == x).all())
    assert len({tuple(r) for r in v1.long().tolist()}) == T                       # no two keys share a V row
    for mode in sorted({m for t, m in MODES if t == T}):
        c = Case("", 0, 2, T, mode, "")
        q, k, v, want, judged = operands(c)
        _, nvis = targets(2, T, mode)
        s = torch.einsum("bihd,bjhd->bhij", q.view(2, T, H, D).double(), k.view(2, T, H, D).double()) * SCALE
        vis = torch.arange(T)[None, None, :] < nvis[:, :, None]
        p = torch.softmax(s.masked_fill(~vis[:, None], float("-inf")), -1)
        ref = torch.einsum("bhij,bjhd->bihd", p, v.view(2, T, H, D).double()).reshape(2, T, W)
        assert float((ref - want.double())[judged].abs().max()) < 1e-9


@pytest.mark.parametrize("B,T,mode", sorted({(c.B, c.T, c.mode) for c in CASES if c.T >= 130}))
def test_targets_cover_every_slot(B, T, mode):
    """Keys 4g + r and 16 + 4g + r of both k-steps: every residue of tgt mod 64 occurs among the judged rows."""
    c = Case("", 0, B, T, mode, "")
    tgt, _ = targets(B, T, mode)
    judged = operands(c)[4]
    assert set((tgt.permute(0, 2, 1)[judged] % 64).flatten().tolist()) == set(range(64))


@pytest.fixture(scope="module")
def env():
    from mmx import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    _lib.load()
    return ops


def split2(x):
    hi = x.bfloat16()
    return hi, (x - hi.float()).bfloat16()


@gpu
@pytest.mark.parametrize("c", CASES, ids=cid)
def test_output_row_is_the_target_keys_value_row(env, c):
    ops = env
    B, T = c.B, c.T
    chunk, qb, klen = spec(c)
    q, k, v, want, judged = operands(c)
    out = torch.full((B, T, W), float("nan"), device="cuda")
    kl = torch.tensor(klen, dtype=torch.int32).cuda() if klen else None
    common = dict(B=B, H=H, T=T, scale=SCALE, chunk=chunk, q_begin=qb, klen=kl, ldo=W, o_bs=T * W)
    if c.entry == "x":
        ops.attn_flash_x(q.cuda(), k.cuda(), v.cuda(), out, ldq=W, ldk=W, ldv=W, q_bs=T * W, k_bs=T * W, v_bs=T * W, **common)
    else:
        Tp = (T + 7) // 8 * 8
        (qh, ql), (kh, kl2), (vh, vl) = split2(q), split2(k), split2(v)
        qk = torch.cat([qh, kh, ql, kl2], -1).contiguous()                     # [hi Q | hi K | lo Q | lo K]
        vt = torch.zeros(B, 2, W, Tp, dtype=torch.bfloat16)
        vt[:, 0, :, :T], vt[:, 1, :, :T] = vh.transpose(1, 2), vl.transpose(1, 2)
        ops.attn_flash_xs(qk.cuda(), vt.cuda(), out, ldqk=4 * W, ldvt=Tp, qk_bs=T * 4 * W, vt_bs=2 * W * Tp, form=c.form, **common)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool(torch.isfinite(got[judged]).all()), f"{cid(c)}: a judged row is not finite"
    err = (got - want).abs().view(B, T, H, D).amax(-1)                         # [B, T, H]
    err[~judged] = 0
    worst = float(err.max())
    b, row, h = (int(i) for i in (err == err.max()).nonzero()[0])
    tgt = int(targets(B, T, c.mode)[0][b, h, row])
    print(f"{cid(c)}: worst |out - V[tgt]| {worst:.3e} at (b, row, head) {(b, row, h)}, target key {tgt} (tile {tgt // 64}, slot {tgt % 64})")
    assert worst < TOL, f"{cid(c)}: {worst:.3e} at (b, row, head) {(b, row, h)}, target key {tgt} (mod 64: {tgt % 64})"
