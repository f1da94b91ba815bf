"""Float64 per-row parity of the MFMA attention kernels: attn_flash_kernel (bf16 and fp8, every instantiation the dispatch reaches),
attn_flash_splitk_kernel and attn_relpos_kernel of csrc/attention.hip, attn_flash_x_kernel (fp32 and pre-split operands) and
attn_relpos_x_kernel of csrc/attention_x.hip, on inputs that make the online-softmax rescale run with live accumulators.

References (plain torch float64 on the CPU, no rounding inside), fed the operands as the kernel reads them from memory (bf16 tensors
widened exactly for the bf16 and fp8 kernels, fp32 for the split kernels, hi + lo of the two bf16 planes for mmx_attn_flash_xs):
  flash_ref   softmax(q k^T * scale, masked) v;  key j is visible to query i when j < klen[b], keymask[b, j] != 0 and, with
              chunk > 0, j < (i // chunk + 1) * chunk;  a row with no visible key is zero and must come out exactly zero
  relpos_ref  score(i, j) = ((q_i + u) . k_j + (q_i + v) . p[T - 1 - i + j]) * scale, the same masks
A CPU test holds both to 1e-12 against the statement built from oracle.flow.rel_shift and oracle.flow.subsequent_chunk_mask.

Inputs: randn (the split kernels keep their x 1.5) plus a per-head pattern in channel 0 of q and k, exact in bf16 and in e4m3 (multiples
of 8 up to 120, small integers), so that with scale 1/8 head h's scores get the term q0 * k0(j) / 8:
  flat   nothing             up8   q0 = 8, k0 = 8 min(j // 48, 15): + 8 nats per 48 keys, every tile moves the maximum by more than 2^6
  up2    q0 = 2, the same k0: + 2.9 log2 units per step, the maximum stays for a tile or two, then moves
  down8  q0 = -8, the same k0: the maximum is in the first tile          saw  q0 = 8, k0 = 8 ((j // 48) % 3)
  spike  q0 = 8, k0 = 16 where j % 97 == 96: one key per two tiles 16 nats up
and, for the rel-pos kernels, through the position table (q0 = 0, pos_v[h, 0] = the constant, so (q + v)0 is exact):
  rel-up    p0[m] = 8 (m // step), (q + v)0 = 8, step = max(12, ceil((2T - 1) / 16)): at most 15 steps, and one 64-key tile further is at
            least one step at every T used here (at T = 77 the k0 staircase has no step between the two tiles; this head has)
  rel-up2   the same table, (q + v)0 = 2          rel-peak  p0 = 8 max(0, 4 - |m - (T - 4)|), (q + v)0 = 8: 32 nats on j - i = -3
In the rel-pos cases the random part of k and of the table is randn x 0.5: the input change the bf16 cap asked for.  With x 1 the
rounding of q + u and q + v to bf16 (2^-9 of each of 64 channels, twice) puts 1.7e-3 nats rms on every score, the MODEL's bases were
7.2e-3 .. 9.0e-3 and 4 base passed 3e-2 in five of the six cases; with x 0.5 they are 5.1e-3 .. 6.2e-3.  The patterns are untouched.
Flash heads cycle flat up8 up2 down8 saw spike flat up8; rel-pos heads are flat up8 up2 saw rel-up rel-peak down8 rel-up2 (down8 and
rel-up2 added so that every launch has a head that never rescales and, at T = 77, one with increments between 1 and 6).
test_patterns_drive_the_rescale (CPU) walks the reference scores of every launch in 64-key tiles and asserts these conditions.

Metric: per (batch member, query row, head) max |got - ref| over the head's 64 channels / max |ref| over them; every row passes; rows
with a visible key have a denominator > 0.  A failure names the worst (b, row, head, pattern).  With klen, rows >= klen[b] are padding:
the kernel either computes them or, where they fill a workgroup, writes zeros; such a row passes as either.

Bounds come from a second CPU statement, the MODEL: the same math with the build's rounding points, key tiles of 64 and the true
running maximum per tile.
  bf16   P rounded to bf16 before P V, the denominator sums the unrounded p, output rounded to bf16; rel-pos rounds q + u, q + v too
  fp8    Q, K, V and 4 P rounded to e4m3, the denominator sums the rounded P, output rounded to bf16
  split  float32 arithmetic; each operand as bf16(x) + bf16(x - bf16(x)), the lo x lo term dropped, for Q K and P V; fp32 output
base = the MODEL's worst row against float64 on the case's own inputs.  bf16: bound = max(4 base, 4 * 2^-9), never above 3e-2; split:
max(4 base, 4 * 2^-17), never above 5e-4 (test_model_bounds_fit_the_caps, CPU, every case; the rel-pos cases' inputs changed for it, see
above).  fp8: every row within 2 base, and the RMS ratio of each (batch member, head) under 7e-2.

Guards: every output lives in a guarded() buffer with Tcap > T rows, slack columns and gaps between batch members; everything but rows
q_begin .. T - 1 of the 512 columns keeps the bits of a clone taken before.  NaN: q rows before q_begin and from T on, K rows from T (or
klen[b]) on, V rows / V^T columns from T (or round_up(klen[b], 8)) on, position rows past 2T - 2; V^T columns T .. round_up(T, 8) - 1
are zero.  Keys hidden by keymask are loaded and meet p = 0: their K rows are 4 q_j (score + 32 nats for their own query), their V
rows +-1000 (+-256 in the fp8 cases: e4m3 ends at 448 and the conversion of a larger value is not a number), so an ignored mask shows.

FIGURES  per kernel, over its cases: MODEL base -> bound on the host of the MI355X run (16 threads) | the kernel's worst row in that run
  attn_flash_kernel<1,false,4>   bf16   4.9e-3 .. 6.1e-3 -> 2.0e-2 .. 2.4e-2 | 5.3e-3 .. 6.6e-3
  attn_flash_kernel<1,false,8>   bf16   5.8e-3 .. 6.3e-3 -> 2.3e-2 .. 2.5e-2 | 6.8e-3 .. 7.2e-3
  attn_flash_splitk_kernel       bf16   4.6e-3 .. 5.5e-3 -> 1.9e-2 .. 2.2e-2 | 4.8e-3 .. 5.8e-3
  attn_relpos_kernel<4>          bf16   5.1e-3 .. 6.2e-3 -> 2.0e-2 .. 2.5e-2 | 5.2e-3 .. 7.2e-3
  attn_flash_kernel<1,true>      fp8    0.133 .. 0.155 -> 0.265 .. 0.310 | 0.142 .. 0.175 (at most 0.63 of its case's bound); (b, head) RMS <= 5.8e-2
  attn_flash_kernel<2,true>      fp8    0.162 .. 0.194 -> 0.324 .. 0.388 | 0.188 .. 0.201 (0.58);                          (b, head) RMS <= 5.6e-2
  attn_flash_x_kernel<1,false,4> split  3.3e-5 .. 5.0e-5 -> 1.3e-4 .. 2.0e-4 | 3.6e-5 .. 5.0e-5
  attn_flash_x_kernel<1,false,8> split  4.7e-5 .. 6.7e-5 -> 1.9e-4 .. 2.7e-4 | 4.3e-5 .. 6.6e-5
  attn_flash_x_kernel<1,true,4>  split  2.6e-5 .. 3.0e-5 -> 1.0e-4 .. 1.2e-4 | 2.6e-5 .. 3.0e-5
  attn_flash_x_kernel<1,true,8>  split  2.9e-5 .. 3.2e-5 -> 1.2e-4 .. 1.3e-4 | 3.2e-5 .. 3.5e-5      <2,true,8>: the same figures
  attn_relpos_x_kernel           split  2.9e-5 .. 4.8e-5 -> 1.2e-4 .. 1.9e-4 | 2.1e-5 .. 3.2e-5
Every kernel's worst row sits at its MODEL's base: no kernel needed a fix, and the fp8 rule of 2 base held with the lazy maximum.
Mutation check (a scratch build of attention.hip without `l_run[mf] *= alpha;` in attn_flash_kernel, run once): all 15 bf16 and all 18
fp8 flash cases of this file fail, worst rows 0.98 on the up2 head; of the 16 cases of test_attn_flash_bf16 14 still pass and the two
at T = 1000, chunk 0, q_begin 0 fail at 0.976 (over 16 000 randn rows one does rescale: the premise "randn never rescales" holds at
T <= 700, not at 1000; the old test then sees it only through its global maximum)."""
import functools
from collections import namedtuple

import pytest
import torch

from test_gpu_fused_parity import Out, bf, round_up, strided, two
from test_gpu_ops_parity import GUARD, assert_guards, guarded, is_sentinel  # noqa: F401  (Out is built on them)

gpu = pytest.mark.gpu

H, D, SCALE, KT = 8, 64, 0.125, 64
LOG2E = 1.4426950408889634
NEG = float("-inf")
FLOOR = {"bf16": 4 * 2.0 ** -9, "split": 4 * 2.0 ** -17}
CAP = {"bf16": 3e-2, "split": 5e-4}
RMS_FP8 = 7e-2
PATS = ("flat", "up8", "up2", "down8", "saw", "spike", "flat", "up8")
REL_PATS = ("flat", "up8", "up2", "saw", "rel-up", "rel-peak", "down8", "rel-up2")
REL_MULT = 0.5                                             # the random part of k and of the position table in the rel-pos cases (docstring)
Q0 = {"up8": 8.0, "up2": 2.0, "down8": -8.0, "saw": 8.0, "spike": 8.0}

# kind -> the build whose rounding points the MODEL has
BUILD = {"bf16": "bf16", "fp8": "fp8", "x": "split", "xs": "split", "rel": "bf16", "relx": "split"}
Case = namedtuple("Case", "kind B T mode qb form kernel")


def f8(x):
    return x.float().to(torch.float8_e4m3fn).to(x.dtype)


# ================================================================================================ the dispatch rules, restated
def ceil_div(a, b):
    return (a + b - 1) // b


def kernel_of(kind, B, T, qb, klen, form=0):
    """The instantiation a launch reaches (mmx_attn_flash_bf16 / _fp8 in csrc/attention.hip, mmx_attn_flash_x / _xs in
    csrc/attention_x.hip), restated:
      bf16: npairs * ceil(Tq / 64) < 96 and T >= 512 and no klen -> split-key kernel; else small = npairs * ceil(Tq / 128) < 192:
            small -> <1,false,4> (64 queries per workgroup), else <1,false,8> (128)
      fp8:  small -> <1,true> (64), else <2,true> (128)          x: small -> <1,false,4>, else <1,false,8>
      xs:   small = form 3 or the rule above -> <1,true,4>; else form 1 -> <1,true,8>, form 2 -> <2,true,8> (256 queries)"""
    npairs, Tq = H * B, T - qb
    small = npairs * ceil_div(Tq, 128) < 192
    if kind == "bf16":
        if npairs * ceil_div(Tq, 64) < 96 and T >= 512 and not klen:
            return "splitk", 16
        return ("flash<1,false,4>", 64) if small else ("flash<1,false,8>", 128)
    if kind == "fp8":
        return ("flash<1,true>", 64) if small else ("flash<2,true>", 128)
    if kind == "x":
        return ("flash_x<1,false,4>", 64) if small else ("flash_x<1,false,8>", 128)
    if kind == "xs":
        if small or form == 3:
            return "flash_x<1,true,4>", 64
        assert form in (1, 2), "form 0 picks by the rounds of the grid: not restated here"
        return ("flash_x<1,true,8>", 128) if form == 1 else ("flash_x<2,true,8>", 256)
    return ("relpos<4>", 64) if kind == "rel" else ("relpos_x", 64)


# ================================================================================================ cases
def spec(c):
    """-> dict(chunk, klen list or None, km [B, T] float or None)."""
    B, T, mode = c.B, c.T, c.mode
    chunk = 50 if "chunk" in mode else 0
    klen = None
    if "klen" in mode:
        if c.kind in ("rel", "relx"):
            klen = [T, T - 45]
        elif B == 2:
            klen = [T, 190]
        else:                                              # member 1: its second workgroup is all padding and writes zeros
            klen = [T] * B
            klen[1], klen[2], klen[5] = 40, 137, 193
    km = None
    if "holes" in mode:                                    # the last member: tile 0 (and 7 more keys) and tile 2 hidden, holes elsewhere
        km = torch.ones(B, T)
        j = torch.arange(T)
        km[B - 1, (j <= 70) | ((j >= 128) & (j < 192)) | (j % 7 == 3)] = 0
    if "dead" in mode:                                     # member 0 sees nothing at all
        km = torch.ones(B, T)
        km[0] = 0
    if "mask4" in mode:                                    # every tile jt % 4 == 2: one wave of the split-key kernel sees nothing
        km = torch.ones(B, T)
        km[:, (torch.arange(T) // KT) % 4 == 2] = 0
    return dict(chunk=chunk, klen=klen, km=km)


def mk(kind, B, T, mode, qb=0, form=0):
    klen = spec(Case(kind, B, T, mode, qb, form, ""))["klen"]
    return Case(kind, B, T, mode, qb, form, kernel_of(kind, B, T, qb, klen, form)[0])


def flash_cases(kind):
    small = [mk(kind, 1, 333, m) for m in ("none", "chunk")] + [mk(kind, 1, 333, "qbegin", 48)]
    small += [mk(kind, 2, 333, m) for m in ("none", "chunk", "klen", "holes", "chunk+holes", "dead")] + [mk(kind, 2, 333, "qbegin", 48)]
    wide = [mk(kind, 24, 200, m) for m in ("none", "chunk", "holes", "klen")] + [mk(kind, 24, 200, "qbegin", 16)]
    return small, wide


BF_S, BF_W = flash_cases("bf16")
F8_S, F8_W = flash_cases("fp8")
F8_S = F8_S + [mk("fp8", 1, 600, "chunk")]
X_S, X_W = flash_cases("x")
X_S = [c for c in X_S if c.B == 2]
SPLITK = [mk("bf16", 1, 600, m, 0) for m in ("none", "chunk", "mask4", "chunk+mask4")] + \
         [mk("bf16", 2, 700, m, 656) for m in ("none", "chunk", "mask4", "chunk+mask4")]
XS = [mk("xs", 2, 333, m, 0, f) for f in (0, 1, 2, 3) for m in ("none", "chunk", "klen")] + \
     [mk("xs", 24, 200, m, 0, f) for f in (1, 2) for m in ("none", "chunk", "klen")]
REL = [mk("rel", 2, T, m) for T in (333, 77) for m in ("none", "chunk", "klen")]
RELX = [mk("relx", 2, T, m) for T in (333, 77) for m in ("none", "chunk", "klen")]
ALL = BF_S + BF_W + SPLITK + F8_S + F8_W + REL + X_S + X_W + XS + RELX


def cid(c):
    return f"{c.kernel}-B{c.B}-T{c.T}-{c.mode}" + (f"-qb{c.qb}" if c.qb else "") + (f"-form{c.form}" if c.kind == "xs" else "")


def test_cases_reach_the_instantiations_they_name():
    """The shapes against the dispatch rules restated in kernel_of (nothing is probed in the library)."""
    assert {c.kernel for c in BF_S} == {"flash<1,false,4>"} and {c.kernel for c in BF_W} == {"flash<1,false,8>"}
    assert {c.kernel for c in F8_S} == {"flash<1,true>"} and {c.kernel for c in F8_W} == {"flash<2,true>"}
    assert {c.kernel for c in X_S} == {"flash_x<1,false,4>"} and {c.kernel for c in X_W} == {"flash_x<1,false,8>"}
    assert {c.kernel for c in XS} == {"flash_x<1,true,4>", "flash_x<1,true,8>", "flash_x<2,true,8>"}
    for c in SPLITK:                                       # npairs * ceil(Tq / 64) < 96 and T >= 512
        assert c.kernel == "splitk" and H * c.B * ceil_div(c.T - c.qb, 64) < 96 and c.T >= 512
    assert len({cid(c) for c in ALL}) == len(ALL)


# ================================================================================================ inputs
def opclass(kind):
    return {"bf16": "b", "fp8": "b", "rel": "rb", "x": "f", "xs": "s", "relx": "rf"}[kind]


@functools.lru_cache(maxsize=None)
def raw_inputs(rel, B, T, mult, plain=False):
    """-> dict(q, k, v [B, T, H, D] fp32, pats, and for rel-pos pos [2T - 1, H, D], pu, pv [H, D]) with the patterns written."""
    g = torch.Generator().manual_seed(B * 1000 + T + (7 if rel else 0))
    q, k, v = (torch.randn(B, T, H, D, generator=g) * mult for _ in range(3))
    if rel:
        k *= REL_MULT
    d = dict(q=q, k=k, v=v, pats=(("flat",) * H if plain else (REL_PATS if rel else PATS)))
    if rel:
        d["pos"] = torch.randn(2 * T - 1, H, D, generator=g) * REL_MULT
        d["pu"], d["pv"] = torch.randn(H, D, generator=g) * 0.2, torch.randn(H, D, generator=g) * 0.2
    j = torch.arange(T)
    stair = 8.0 * (j // 48).clamp(max=15).float()
    for h, p in enumerate(d["pats"]):
        if p == "flat":
            continue
        if rel:
            d["pu"][h, 0] = d["pv"][h, 0] = 0.0
        if p in Q0:
            q[:, :, h, 0] = Q0[p]
            k[:, :, h, 0] = {"saw": 8.0 * ((j // 48) % 3).float(), "spike": torch.where(j % 97 == 96, 16.0, 0.0)}.get(p, stair)
        else:
            m = torch.arange(2 * T - 1)
            step = max(12, ceil_div(2 * T - 1, 16))
            q[:, :, h, 0] = 0.0
            d["pv"][h, 0] = 2.0 if p == "rel-up2" else 8.0
            d["pos"][:, h, 0] = 8.0 * (4 - (m - (T - 4)).abs()).clamp(min=0).float() if p == "rel-peak" else 8.0 * (m // step).float()
            assert float(d["pos"][:, h, 0].max()) <= 120
    return d


def inputs(c, plain=False):
    """The operands as the kernel reads them (fp32 tensors holding the exact values), cached per (operand class, shape)."""
    return _inputs(opclass(c.kind), c.B, c.T, plain)


@functools.lru_cache(maxsize=None)
def _inputs(oc, B, T, plain):
    rel = oc[0] == "r"
    raw = raw_inputs(rel, B, T, 1.5 if oc in ("f", "s") else 1.0, plain)
    rd = {"b": bf, "rb": bf, "f": lambda x: x, "rf": lambda x: x, "s": two}[oc]
    d = dict(raw)
    for n in ("q", "k", "v") + (("pos",) if rel else ()):
        d[n] = rd(raw[n])
    return d


# ================================================================================================ references
def visible(B, T, *, keymask=None, klen=None, chunk=0):
    """-> [B, T queries, T keys] bool."""
    j = torch.arange(T)
    vis = torch.ones(B, T, T, dtype=torch.bool)
    if klen is not None:
        vis &= j[None, None, :] < torch.as_tensor(klen)[:, None, None]
    if keymask is not None:
        vis &= (keymask != 0)[:, None, :]
    if chunk > 0:
        vis &= (j[None, :] < (j[:, None] // chunk + 1) * chunk)[None]
    return vis


def flash_scores(q, k, scale):
    return torch.einsum("bihd,bjhd->bhij", q, k) * scale


def relpos_scores(q, k, pos, pu, pv, scale):
    B, T = q.shape[:2]
    i = torch.arange(T)
    idx = (T - 1 - i[:, None] + i[None, :]).expand(B, H, T, T)
    bd = torch.einsum("bihd,mhd->bhim", q + pv, pos).gather(-1, idx)
    return (torch.einsum("bihd,bjhd->bhij", q + pu, k) + bd) * scale


def attend(s, vis, v):
    """s [B, H, T, T], vis [B, T, T], v [B, T, H, D] -> [B, T, H, D]; a row with no visible key is zero."""
    s = s.masked_fill(~vis[:, None], NEG)
    m = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(m), m, torch.zeros_like(m)))
    l = p.sum(-1, keepdim=True)
    return torch.einsum("bhij,bjhd->bihd", p / torch.where(l > 0, l, torch.ones_like(l)), v)


def flash_ref(q, k, v, *, scale, keymask=None, klen=None, chunk=0):
    return attend(flash_scores(q, k, scale), visible(q.shape[0], q.shape[1], keymask=keymask, klen=klen, chunk=chunk), v)


def relpos_ref(q, k, v, pos, pu, pv, *, scale, keymask=None, klen=None, chunk=0):
    return attend(relpos_scores(q, k, pos, pu, pv, scale), visible(q.shape[0], q.shape[1], keymask=keymask, klen=klen, chunk=chunk), v)


def ref_scores(c, plain=False):
    x = inputs(c, plain)
    q, k = x["q"].double(), x["k"].double()
    if "pos" in x:
        return relpos_scores(q, k, x["pos"].double(), x["pu"].double(), x["pv"].double(), SCALE)
    return flash_scores(q, k, SCALE)


def vis_of(c):
    sp = spec(c)
    return visible(c.B, c.T, keymask=sp["km"], klen=sp["klen"], chunk=sp["chunk"])


@functools.lru_cache(maxsize=None)
def _ref(oc, B, T, mode, kind):
    c = Case(kind, B, T, mode, 0, 0, "")
    return attend(ref_scores(c), vis_of(c), inputs(c)["v"].double())


def ref_of(c):
    """The float64 reference of the launch, all rows: computed once per (operands, shape, masks), shared and left unchanged."""
    return _ref(opclass(c.kind), c.B, c.T, c.mode, {"fp8": "bf16"}.get(c.kind, c.kind))


# ================================================================================================ the tile walk
def tile_max(s, vis):
    """s [B, H, T, T] -> the maximum of each 64-key tile [B, H, T, ntile] (masked keys -inf)."""
    B, _, T, _ = s.shape
    nt = ceil_div(T, KT)
    sp = torch.full((B, H, T, nt * KT), NEG, dtype=s.dtype)
    sp[..., :T] = s.masked_fill(~vis[:, None], NEG)
    return sp.view(B, H, T, nt, KT).amax(-1)


def tile_walk(s, vis):
    """-> (rescales, mids) [B, H, T]: per row the tiles whose maximum is more than 6 / between 1 and 6 log2 units above a FINITE
    running maximum (the true one, moved by every tile)."""
    tm = tile_max(s, vis) * LOG2E
    run = tm.cummax(-1).values
    prev = torch.cat([torch.full_like(run[..., :1], NEG), run[..., :-1]], -1)
    fin = torch.isfinite(prev) & torch.isfinite(tm)
    inc = torch.where(fin, tm - prev, torch.zeros_like(tm))
    return (fin & (inc > 6)).sum(-1), (fin & (inc > 1) & (inc <= 6)).sum(-1)


# ================================================================================================ the MODEL
def run_max(s):
    """s [B, H, T, T] masked -> (the running tile maximum at each key [B, H, T, T], the final one [B, H, T, 1]); rows / tiles that
    have seen nothing yet get 0."""
    T = s.shape[-1]
    tm = tile_max(s, torch.ones(s.shape[0], T, T, dtype=torch.bool))
    run = tm.cummax(-1).values
    run = torch.where(torch.isfinite(run), run, torch.zeros_like(run))
    return run.repeat_interleave(KT, -1)[..., :T], run[..., -1:]


def soft_model(s, vis, mul_pv, *, prnd, pscale=1.0, den_rounded=False):
    """Tile-wise softmax with P rounded relative to the running maximum of its tile.  mul_pv(P [B, H, T, T]) -> P V [B, T, H, D]."""
    s = s.masked_fill(~vis[:, None], NEG)
    run, M = run_max(s)
    p = torch.exp(s - run) * pscale
    w = torch.exp(run - M)
    pr = prnd(p)
    den = ((pr if den_rounded else p) * w).sum(-1).transpose(1, 2)[..., None]
    return mul_pv(pr, w) / torch.where(den > 0, den, torch.ones_like(den))


def split2(x):
    h = bf(x)
    return h, bf(x - h)


def mm3(eq, a, b):
    """a b with both operands as bf16 hi + lo, the lo x lo term dropped (float32)."""
    (ah, al), (bh, bl) = split2(a), split2(b)
    return torch.einsum(eq, ah, bh) + torch.einsum(eq, al, bh) + torch.einsum(eq, ah, bl)


def model_of(c):
    """The MODEL's output of the launch [B, T, H, D] (float64 for bf16 / fp8, float32 for the split build)."""
    x, vis, build = inputs(c), vis_of(c), BUILD[c.kind]
    rel = "pos" in x
    if build == "split":
        q, k, v = x["q"], x["k"], x["v"]
        if rel:
            B, T = q.shape[:2]
            i = torch.arange(T)
            idx = (T - 1 - i[:, None] + i[None, :]).expand(B, H, T, T)
            s = (mm3("bihd,bjhd->bhij", q + x["pu"], k) + mm3("bihd,mhd->bhim", q + x["pv"], x["pos"]).gather(-1, idx)) * SCALE
        else:
            s = mm3("bihd,bjhd->bhij", q, k) * SCALE
        vh, vl = split2(v)

        def mul_pv(p, w):
            ph, pl = split2(p)
            return torch.einsum("bhij,bjhd->bihd", ph * w, vh) + torch.einsum("bhij,bjhd->bihd", pl * w, vh) + torch.einsum("bhij,bjhd->bihd", ph * w, vl)
        return soft_model(s, vis, mul_pv, prnd=lambda p: p)
    rq = f8 if build == "fp8" else (lambda t: t)
    q, k, v = rq(x["q"]).double(), rq(x["k"]).double(), rq(x["v"]).double()
    if rel:
        s = relpos_scores(torch.zeros_like(q), k, x["pos"].double(), bf(x["q"] + x["pu"]).double(), bf(x["q"] + x["pv"]).double(), SCALE)
    else:
        s = flash_scores(q, k, SCALE)
    mul_pv = lambda p, w: torch.einsum("bhij,bjhd->bihd", p * w, v)
    if build == "fp8":
        return bf(soft_model(s, vis, mul_pv, prnd=f8, pscale=4.0, den_rounded=True))
    return bf(soft_model(s, vis, mul_pv, prnd=bf))


# ================================================================================================ metric
def judged_rows(c):
    """-> (strict [B, T - qb] bool: rows held to the reference; has_key [B, T - qb]: rows with a visible key)."""
    sp = spec(c)
    t = torch.arange(c.qb, c.T)
    strict = torch.ones(c.B, c.T - c.qb, dtype=torch.bool) if sp["klen"] is None else t[None, :] < torch.tensor(sp["klen"])[:, None]
    return strict, vis_of(c)[:, c.qb:].any(-1)


def row_stats(got, ref, strict, has_key, pats, what):
    """got, ref [B, R, H, D] -> (worst ratio, (b, row, head, pattern), ratios [B, R, H])."""
    g, r = got.double(), ref.double()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    assert bool(torch.isfinite(g).all()), f"{what}: output not finite (something that must not be read was read, or a row was not written), " \
                                          f"first at (b, row, head) {(~torch.isfinite(g)).any(-1).nonzero()[:3].tolist()}"
    den, err = r.abs().amax(-1), (g - r).abs().amax(-1)
    assert bool((den[has_key] > 0).all()) and bool((den[~has_key] == 0).all()), f"{what}: the reference's denominator"
    z = den == 0
    assert bool((err[z] == 0).all()), f"{what}: a row whose reference is exactly zero is not zero, at (b, row, head) {(z & (err != 0)).nonzero()[:4].tolist()}"
    ratio = torch.where(z, torch.zeros_like(err), err / den.clamp_min(1e-300))
    ratio = torch.where(~strict[..., None] & (g.abs().amax(-1) == 0), torch.zeros_like(ratio), ratio)     # a padding row written as zeros
    b, row, h = (int(i) for i in (ratio == ratio.max()).nonzero()[0])
    return float(ratio.max()), (b, row, h, pats[h]), ratio


def head_rms(got, ref, strict):
    """RMS(got - ref) / RMS(ref) per (batch member, head) over the strict rows -> [B, H]."""
    w = strict[:, :, None, None].double()
    return (((got.double() - ref) ** 2 * w).sum((1, 3)) / ((ref ** 2) * w).sum((1, 3)).clamp_min(1e-300)).sqrt()


@functools.lru_cache(maxsize=None)
def _base(c):
    strict, has_key = judged_rows(c)
    ref, mod = ref_of(c)[:, c.qb:], model_of(c)[:, c.qb:]
    base, at, _ = row_stats(mod, ref, strict, has_key, inputs(c)["pats"], "model " + cid(c))
    return base, at, float(head_rms(mod, ref, strict).max())


def bound_of(c):
    """-> (base, bound) of the case from the MODEL on this host."""
    base = _base(c._replace(kernel="", form=0))[0]
    build = BUILD[c.kind]
    return base, (2 * base if build == "fp8" else max(4 * base, FLOOR[build]))


# ================================================================================================ CPU tests
@pytest.mark.parametrize("T,chunk", [(77, 0), (100, 50), (130, 25)])
def test_refs_match_the_oracle_statement(T, chunk):
    """flash_ref / relpos_ref against softmax(masked_fill(scores)) built from oracle.flow.rel_shift and subsequent_chunk_mask, 1e-12."""
    from oracle import flow as OF
    g = torch.Generator().manual_seed(T)
    B = 2
    q, k, v = (torch.randn(B, T, H, D, generator=g, dtype=torch.float64) for _ in range(3))
    pos = torch.randn(2 * T - 1, H, D, generator=g, dtype=torch.float64)
    pu, pv = torch.randn(H, D, generator=g, dtype=torch.float64) * 0.2, torch.randn(H, D, generator=g, dtype=torch.float64) * 0.2
    km = (torch.rand(B, T, generator=g) > 0.3).float()
    klen = [T, T - 9]
    vis = km.bool()[:, None, :].expand(B, T, T).clone()
    vis[1, :, klen[1]:] = False
    if chunk:
        vis &= OF.subsequent_chunk_mask(T, chunk)[None]
    qh, kh, vh = q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)
    ac = (q + pu).transpose(1, 2) @ kh.transpose(-2, -1)
    bd = OF.rel_shift((q + pv).transpose(1, 2) @ pos[None].transpose(1, 2).transpose(-2, -1))
    for got, s in ((flash_ref(q, k, v, scale=SCALE, keymask=km, klen=klen, chunk=chunk), qh @ kh.transpose(-2, -1) * SCALE),
                   (relpos_ref(q, k, v, pos, pu, pv, scale=SCALE, keymask=km, klen=klen, chunk=chunk), (ac + bd) * SCALE)):
        want = (torch.softmax(s.masked_fill(~vis[:, None], NEG), -1) @ vh).transpose(1, 2)
        assert float((got - want).abs().max() / want.abs().max()) < 1e-12
    dead = flash_ref(q, k, v, scale=SCALE, keymask=torch.zeros(B, T))
    assert float(dead.abs().max()) == 0.0


LAUNCHES = sorted({(opclass(c.kind), c.B, c.T, c.mode): c for c in ALL}.values(), key=ALL.index)


@pytest.mark.parametrize("c", LAUNCHES, ids=lambda c: f"{opclass(c.kind)}-B{c.B}-T{c.T}-{c.mode}")
def test_patterns_drive_the_rescale(c):
    """Conditions on the reference alone: the 64-key tile walk (threshold 6 log2 units, true running maximum) of every launch's
    float64 scores has a head in which EVERY row that sees more than 64 keys rescales with live accumulators, a head with tile-to-tile
    increments between 1 and 6, and a down8 head that never rescales; plain randn of the same shape never rescales."""
    vis, pats = vis_of(c), inputs(c)["pats"]
    resc, mid = tile_walk(ref_scores(c), vis)               # [B, H, T]
    # the bf16 flash operands: every row that sees more than one tile.  Where the randn term is wider (rel-pos: two random terms, 2.0 log2
    # units; the x 1.5 operands: 3.2) a step of 11.5 log2 units seen through a sliver of keys (chunk 50 shows rows 50 .. 99 keys 96 .. 99
    # of the next step) does not always clear 6 above the maximum over 48 keys: there, at T >= 128, 999 in 1000 of the rows that see
    # more than two tiles
    wide = opclass(c.kind) != "b" and c.T >= 2 * KT
    many = (vis.sum(-1) > (2 * KT if wide else KT))[:, None, :].expand_as(resc)
    assert bool(many.any())
    every = [pats[h] for h in range(H) if float((resc[:, h][many[:, h]] > 0).double().mean()) >= (0.999 if wide else 1.0)]
    assert every and ("up8" in every or c.T < 97), (every, "no head rescales on every row that sees more than one tile")
    assert any(int(mid[:, h].sum()) > 0 for h in range(H) if pats[h] in ("up2", "rel-up2")), "no head with increments between 1 and 6"
    # randn alone: none at all on the bf16 flash operands (score spread 1.44 log2 units); the rel-pos scores (two random terms, 2.0) and
    # the split kernels' x 1.5 operands (3.2) are wider and a rare row does rescale: fewer than one row in fifty
    few = 0 if opclass(c.kind) == "b" else c.B * c.T // 50
    assert int(resc[:, pats.index("down8")].sum()) == 0 and all(int(resc[:, h].sum()) <= few for h in range(H) if pats[h] == "flat")
    for p in ("up8", "up2", "saw", "spike"):
        if p in pats:
            assert int(resc[:, pats.index(p)].sum()) > 0 or c.T < 97, p
    plain = tile_walk(ref_scores(c, plain=True), vis)[0]
    assert all(int(plain[:, h].sum()) <= few for h in range(H)), "plain randn rescales: the premise of this file does not hold"
    den = ref_of(c).abs().amax(-1)
    print(f"{cid(c)}: rescales per head {[int(resc[:, h].sum()) for h in range(H)]}, of plain randn {int(plain.sum())}, smallest per-row max |ref| {float(den[den > 0].min()):.3f}")


@pytest.mark.parametrize("c", ALL, ids=cid)
def test_model_bounds_fit_the_caps(c):
    base, bound = bound_of(c)
    _, at, rms = _base(c._replace(kernel="", form=0))
    print(f"{cid(c)}: MODEL base {base:.3e} at {at} -> bound {bound:.3e}" + (f", worst (b, head) RMS {rms:.3e}" if c.kind == "fp8" else ""))
    if c.kind == "fp8":
        assert rms < RMS_FP8
    else:
        assert bound <= CAP[BUILD[c.kind]], (base, bound)


# ================================================================================================ GPU side
@pytest.fixture(scope="module")
def env():
    from mmx import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    _lib.load()
    return _lib, ops


def fill_rows(flat, x, bs, ld, live, off=0):
    """x [B, T, W] into member b row t at off + b * bs + t * ld of the flat buffer, rows where live [B, T]."""
    B, T, W = x.shape
    view = strided(flat, B, bs, T, ld, W, off)
    view[live] = x[live].to(flat.dtype)


def nan_flat(n, dtype):
    return torch.full((n,), float("nan"), dtype=dtype)


WORST = {}


def run_case(env, c):
    """One launch with guards and poison -> the kernel's rows q_begin .. T - 1 [B, T - qb, H, D] (CPU)."""
    _, ops = env
    sp, x = spec(c), inputs(c)
    B, T, qb, kind = c.B, c.T, c.qb, c.kind
    chunk, klen, km = sp["chunk"], sp["klen"], sp["km"]
    Tcap, W = T + 5, H * D
    t = torch.arange(T)
    tk = torch.tensor(klen if klen else [T] * B)
    q_live = ((t >= qb)[None, :]).expand(B, T)
    k_live = t[None, :] < tk[:, None]
    q, k, v = (x[n].reshape(B, T, W).clone() for n in ("q", "k", "v"))
    if km is not None:                                     # hidden keys: loaded, p = 0
        hid = km == 0
        k[hid] = (4 * x["q"].reshape(B, T, W))[hid]
        big = (256.0 if kind == "fp8" else 1000.0) * (1 - 2 * (torch.arange(W) % 2).float())
        v[hid] = big.expand(B, T, W)[hid]
    wide = kind in ("x", "xs", "relx")                     # fp32 output
    dt = torch.float32 if kind in ("x", "relx") else torch.bfloat16
    al = 4 if dt == torch.float32 else 8
    ld = W + al
    bs = Tcap * ld + al
    ldo, o_bs = (W + 4, Tcap * (W + 4) + 4) if wide else (ld, bs)
    out = Out(B * o_bs, torch.float32 if wide else torch.bfloat16)
    kmd = km.cuda() if km is not None else None
    kl = torch.tensor(klen, dtype=torch.int32).cuda() if klen else None
    common = dict(B=B, H=H, T=T, scale=SCALE, chunk=chunk, klen=kl)

    def vt_planes(planes):
        """V^T planes [B][len(planes)][512][ldvt]: columns < round_up(klen[b] or T, 8) written, those from T on as zeros."""
        ldvt = round_up(Tcap, 8) + 8
        vt_bs = len(planes) * W * ldvt + 16
        flat = nan_flat(B * vt_bs, torch.bfloat16)
        for b in range(B):
            n = round_up(int(tk[b]), 8)
            for pi, pl in enumerate(planes):
                dst = flat[b * vt_bs + pi * W * ldvt:][:W * ldvt].view(W, ldvt)
                dst[:, :n] = 0
                dst[:, :min(n, T)] = pl[b, :min(n, T)].t().to(torch.bfloat16)
        return flat.cuda(), ldvt, vt_bs

    if kind in ("bf16", "fp8", "rel"):
        qf, kf = nan_flat(B * bs, dt), nan_flat(B * bs, dt)
        fill_rows(qf, q, bs, ld, q_live)
        fill_rows(kf, k, bs, ld, k_live)
        vt, ldvt, vt_bs = vt_planes([v])
        args = dict(ldq=ld, ldk=ld, ldvt=ldvt, ldo=ldo, q_bs=bs, k_bs=bs, vt_bs=vt_bs, o_bs=o_bs, **common)
        qd, kd = qf.cuda(), kf.cuda()
        if kind == "rel":
            pf = nan_flat((2 * T + 3) * ld, dt)
            fill_rows(pf, x["pos"].reshape(1, 2 * T - 1, W), 0, ld, torch.ones(1, 2 * T - 1, dtype=torch.bool))
            pd, pu, pv = pf.cuda(), x["pu"].cuda(), x["pv"].cuda()
            launch = lambda: ops.attn_relpos_bf16(qd, kd, vt, pd, pu, pv, out.view, ldp=ld, **args)
        else:
            launch = lambda: ops.attn_flash_bf16(qd, kd, vt, out.view, keymask=kmd, q_begin=qb, fp8=(kind == "fp8"), **args)
    elif kind in ("x", "relx"):
        qf, kf, vf = nan_flat(B * bs, dt), nan_flat(B * bs, dt), nan_flat(B * bs, dt)
        fill_rows(qf, q, bs, ld, q_live)
        fill_rows(kf, k, bs, ld, k_live)
        fill_rows(vf, v, bs, ld, k_live)
        qd, kd, vd = qf.cuda(), kf.cuda(), vf.cuda()
        args = dict(ldq=ld, ldk=ld, ldv=ld, ldo=ldo, q_bs=bs, k_bs=bs, v_bs=bs, o_bs=o_bs, **common)
        if kind == "relx":
            pf = nan_flat((2 * T + 3) * ld, dt)
            fill_rows(pf, x["pos"].reshape(1, 2 * T - 1, W), 0, ld, torch.ones(1, 2 * T - 1, dtype=torch.bool))
            pd, pu, pv = pf.cuda(), x["pu"].cuda(), x["pv"].cuda()
            launch = lambda: ops.attn_relpos_x(qd, kd, vd, pd, pu, pv, out.view, ldp=ld, **args)
        else:
            launch = lambda: ops.attn_flash_x(qd, kd, vd, out.view, keymask=kmd, q_begin=qb, **args)
    else:                                                  # xs: rows [hi Q | hi K | lo Q | lo K], V^T as two planes
        assert qb == 0 and km is None
        ldqk = 2048 + 8
        qk_bs = Tcap * ldqk + 8
        f = nan_flat(B * qk_bs, dt)
        for src, live, cols in ((q, q_live, (0, 1024)), (k, k_live, (512, 1536))):
            hi, lo = split2(src)
            fill_rows(f, hi, qk_bs, ldqk, live, cols[0])
            fill_rows(f, lo, qk_bs, ldqk, live, cols[1])
        vt, ldvt, vt_bs = vt_planes(list(split2(v)))
        qkd = f.cuda()
        launch = lambda: ops.attn_flash_xs(qkd, vt, out.view, ldqk=ldqk, ldvt=ldvt, ldo=ldo, qk_bs=qk_bs, vt_bs=vt_bs, o_bs=o_bs, form=c.form, **common)
    out.snap()
    launch()
    torch.cuda.synchronize()
    body = out.check([(B, o_bs, ldo, 0, qb, T, 0, W)], cid(c))
    rows = strided(body, B, o_bs, T, ldo, W)[:, qb:]
    assert not bool(is_sentinel(rows).reshape(B, T - qb, H, D).all(-1).any()), f"{cid(c)}: a row of the window was not written"
    return rows.reshape(B, T - qb, H, D).clone()


def check_case(env, c, group):
    base, bound = bound_of(c)
    got = run_case(env, c)
    strict, has_key = judged_rows(c)
    ref = ref_of(c)[:, c.qb:]
    pats = inputs(c)["pats"]
    worst, at, _ = row_stats(got, ref, strict, has_key, pats, cid(c))
    w = WORST.setdefault(group, [0.0, 0.0, 0.0])
    w[0], w[1], w[2] = max(w[0], base), max(w[1], bound), max(w[2], worst)
    msg = f"{cid(c)}: MODEL base {base:.3e} -> bound {bound:.3e} | kernel worst row {worst:.3e} at (b, row - q_begin, head, pattern) {at}"
    if c.kind == "fp8":
        rms = head_rms(got, ref, strict)
        b, h = (int(i) for i in (rms == rms.max()).nonzero()[0])
        msg += f"; worst (b, head) RMS {float(rms.max()):.3e} at ({b}, {h}, {pats[h]})"
    print(msg + f"   [group {group} so far: base {w[0]:.3e} bound {w[1]:.3e} kernel {w[2]:.3e}]")
    assert worst < bound, msg
    if c.kind == "fp8":
        assert float(rms.max()) < RMS_FP8, msg
    if spec(c)["klen"]:                                    # a workgroup of pure padding writes zeros (kernel_of gives its height)
        qt = kernel_of(c.kind, c.B, c.T, c.qb, spec(c)["klen"], c.form)[1]
        for b, n in enumerate(spec(c)["klen"]):
            first = ceil_div(max(n - c.qb, 0), qt) * qt
            if c.kind not in ("rel", "relx"):
                assert float(got[b, first:].abs().max() if first < c.T - c.qb else 0.0) == 0.0, f"{cid(c)}: padding workgroup of member {b} not zero"


@gpu
@pytest.mark.parametrize("c", BF_S + BF_W, ids=cid)
def test_flash_bf16_rows(env, c):
    check_case(env, c, "flash bf16")


@gpu
@pytest.mark.parametrize("c", SPLITK, ids=cid)
def test_flash_splitk_rows(env, c):
    check_case(env, c, "splitk bf16")


@gpu
@pytest.mark.parametrize("c", F8_S + F8_W, ids=cid)
def test_flash_fp8_rows(env, c):
    check_case(env, c, "flash fp8")


@gpu
@pytest.mark.parametrize("c", REL, ids=cid)
def test_relpos_bf16_rows(env, c):
    check_case(env, c, "relpos bf16")


@gpu
@pytest.mark.parametrize("c", X_S + X_W, ids=cid)
def test_flash_x_rows(env, c):
    check_case(env, c, "flash_x split")


@gpu
@pytest.mark.parametrize("c", XS, ids=cid)
def test_flash_xs_rows(env, c):
    check_case(env, c, "flash_xs split")


@gpu
@pytest.mark.parametrize("c", RELX, ids=cid)
def test_relpos_x_rows(env, c):
    check_case(env, c, "relpos_x split")
