"""Float64 per-row parity of the three row-tile kernels of csrc/fused.hip: mmx_est_tail, mmx_est_resnet and mmx_dac_ru, every
instantiation their dispatch reaches, in the bf16, fp32, split (MMX_X2) and weight-plane (MMX_X2W) builds.

References (plain torch float64 on the CPU, no rounding inside), fed the operands as the kernel reads them from memory (dtype 1:
bf16-rounded ao / a_in and weights; dtype 2: fp32 activations, bf16-rounded weights; X2W and dtype 0: everything fp32):
  tail_ref    x1 = x + ao wo^T + bo;  x2 = (x1 + W2 gelu(W1 LN3(x1) + b1) + b2) * mask;  qkv = LN1(x2) wqkv^T;  act = x2
  resnet_ref  h = mish(LN(conv3(a) + b1)) * m;  h = (h + tv) * m;  h = mish(LN(conv3(h) + b2)) * m;  x = h + conv1(a) + br;  qkv as above
              (both convolutions pad with two zero rows of their own input)
  ru_ref      x_out = x + lrelu(conv1(snake_a2(lrelu(conv7_dil(snake_a0(x)) + b7))) + b1);  act = snake_next(x_out);  rows >= lens[b]
              are read as zero and written as zero
The CPU tests (not marked gpu) hold them to 1e-12 against oracle.flow.causal_resnet, oracle.flow.basic_transformer_block (its
post-attention half, and through a second block the Q | K | V) and oracle.dac.residual_unit.

Metric: per row (batch member, frame) max |got - ref| over the row's channels / max |ref| over them; every row passes.  x, act_out,
Q, K, V (vt_out transposed back) are judged separately; a row whose reference is exactly zero must be exactly zero.

Bounds come from a second CPU statement, the MODEL: the same chain in torch float32 with the build's rounding wherever the kernel
makes an activation a GEMM operand or stores it (dtype 0 nothing, dtype 1 bf16, split builds bf16(x) + bf16(x - bf16(x)), X2W the
weights split alike).  base = the model's worst row against float64; bound = max(4 * base, floor), floor = 1e-6 (dtype 0),
4 * 2^-17 (split), 4 * 2^-9 (bf16); never above the suite's 5e-5 / 3e-2 / 5e-4 (est kernels) and 4e-2 / 2e-4 (dac_ru), which
test_model_bounds_fit_the_caps checks on the CPU for every case.

Guards: every output lives in a guarded() buffer full of the sentinel, every input element the kernel must not read (rows
T .. Tcap - 1, slack columns of ao / a_in, rows >= lens[b], the gaps between batch members) holds NaN, and after each launch all
bits outside the written window (rows t_begin .. T - 1, the named columns; vt_out frames t_begin .. the next multiple of 8 after T,
those from T on as zeros) equal a clone taken before.  A wrong read shows as NaN in the output, a wrong write as a changed guard.

Figures (FIGURES below): base -> bound per case group as the CPU statement gave them on the host of the MI355X run (16 threads), and
the kernels' worst rows in that run.  torch's fp32 matmul sums in an order that depends on the host and its thread count, so the
fp32 bases move (a 4-thread development host gave 1.3e-6 / 1.1e-6 where the table says 6.6e-7 / 7.1e-7); the floors and the bf16
and split bases, which rounding points dominate, do not."""
import functools

import pytest
import torch
import torch.nn.functional as F

from test_gpu_ops_parity import GUARD, assert_guards, guarded, is_sentinel, snake64

gpu = pytest.mark.gpu

X2, X2W = 2, 0x12
DTS = [0, 1, X2, X2W]
DT_NAME = {0: "f32", 1: "bf16", X2: "x2", X2W: "x2w"}
CODE = {0: 0, 1: 1, X2: 2, X2W: 2}            # the dtype an entry point is called with (Planed weights make it X2W)
FLOOR = {0: 1e-6, 1: 4 * 2.0 ** -9, X2: 4 * 2.0 ** -17, X2W: 4 * 2.0 ** -17}
CAP_EST = {0: 5e-5, 1: 3e-2, X2: 5e-4, X2W: 5e-4}
CAP_RU = {1: 4e-2, X2: 2e-4, X2W: 2e-4}
EPS, SLOPE = 1e-5, 0.1

# FIGURES   worst case of the group: base -> bound = max(4 * base, floor) | the kernels' worst row, every instantiation and output
#   est_tail    f32   6.6e-7 -> 2.6e-6 | 1.9e-6    residual rows of mean 100: 7.5e-6 -> 3.0e-5 | 7.7e-6
#               bf16  5.7e-3 -> 2.3e-2 | 5.7e-3    x2  9.4e-6 -> 3.8e-5 | 1.1e-5    x2w  1.3e-5 -> 5.1e-5 | 1.4e-5
#   est_resnet  f32   7.1e-7 -> 2.8e-6 | 1.6e-6    bf16  5.1e-3 -> 2.0e-2 | 4.7e-3    x2  9.2e-6 -> 3.7e-5 | 9.4e-6    x2w  1.1e-5 -> 4.4e-5 | 1.2e-5
#   dac_ru      bf16  7.7e-3 -> 3.1e-2 | 7.4e-3    x2  1.2e-5 -> 4.7e-5 | 1.1e-5    x2w  1.5e-5 -> 5.9e-5 | 1.6e-5
# (every case is held to the bound of its own base, which is at most the group's; the fp32 MFMA sums K in one sequential FMA chain
#  where torch sums in blocks, which is why the fp32 kernels sit at two to three times the torch statement's error)


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


def round_up(x, m):
    return (x + m - 1) // m * m


# ================================================================================================ rounding of the model
def ident(x):
    return x


def bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def two(x):
    """bf16(x) + bf16(x - bf16(x)): what two bf16 planes hold."""
    h = bf(x)
    return h + bf(x - h)


def act_rnd(dt):
    return {0: ident, 1: bf}.get(dt, two)


def store_rnd(dt, planes=False):
    return bf if dt == 1 else (two if planes else ident)


def w_read(w, dt):
    """A weight matrix as the kernel reads it from memory (fp32 tensor)."""
    return w if dt in (0, X2W) else bf(w)


def w_model(w, dt):
    return two(w) if dt == X2W else w_read(w, dt)


def cast_w(W, dt, fn, dtype, mats):
    return {k: (fn(v, dt) if k in mats else v).to(dtype) for k, v in W.items()}


# ================================================================================================ the three chains
def ln(x, g, b):
    return F.layer_norm(x, x.shape[-1:], g, b, EPS)


def tail_chain(ao, x, W, mask, nxt, r=ident, rs_act=ident, rs_qkv=ident):
    """ao [B, T, 512], x [B, T, 256], mask [B, T] or None -> (x2, act, qkv or None).  r: rounding of a GEMM operand; rs_*: of a
    stored output.  With the identities in float64 this is tail_ref."""
    x1 = x + r(ao) @ W["wo"].t() + W["bo"]
    h = r(ln(x1, W["n3g"], W["n3b"]))
    f = r(F.gelu(h @ W["w1"].t() + W["b1"]))
    x2 = x1 + f @ W["w2"].t() + W["b2"]
    if mask is not None:
        x2 = x2 * mask[..., None]
    qkv = rs_qkv(r(ln(x2, W["n1g"], W["n1b"])) @ W["wqkv"].t()) if nxt else None
    return x2, rs_act(x2), qkv


def conv_causal(z, w, b):
    """z [B, T, Cin], w [Cout, Cin, k]: k - 1 zero rows of z in front."""
    return F.conv1d(F.pad(z.transpose(1, 2), (w.shape[2] - 1, 0)), w, b).transpose(1, 2)


def resnet_chain(a, R, tv, mask, r=ident, rs_qkv=ident):
    """a [B, T, cin] (already masked), tv [B, 256], mask [B, T] or None -> (x, qkv)."""
    m = 1.0 if mask is None else mask[..., None]
    a = r(a)
    h = F.mish(ln(conv_causal(a, R["w1"], R["b1"]), R["g1"], R["be1"])) * m
    h = r((h + tv[:, None, :]) * m)
    h = F.mish(ln(conv_causal(h, R["w2"], R["b2"]), R["g2"], R["be2"])) * m
    x = h + conv_causal(a, R["wr"], R["br"])
    return x, rs_qkv(r(ln(x, R["n1g"], R["n1b"])) @ R["wqkv"].t())


def snake(v, alpha):
    return v + (alpha + 1e-9).reciprocal() * torch.sin(alpha * v) ** 2


def ru_chain(x, U, dil, lens, r=ident, rs_act=ident, snk=snake):
    """x [B, T, C] (rows >= lens[b] may hold anything), lens list or None -> (x_out, act)."""
    B, T, _ = x.shape
    live = torch.ones(B, T, 1, dtype=torch.bool) if lens is None else (torch.arange(T)[None, :] < torch.tensor(lens)[:, None])[..., None]
    xz = torch.where(live, x, torch.zeros((), dtype=x.dtype))
    s0 = r(snk(xz, U["a0"]))
    c7 = F.conv1d(s0.transpose(1, 2), U["w7"], U["b7"], dilation=dil, padding=3 * dil).transpose(1, 2)
    mid = r(snk(F.leaky_relu(c7, SLOPE), U["a2"]))
    y = F.leaky_relu(mid @ U["w1"][:, :, 0].t() + U["b1"], SLOPE)
    xo = torch.where(live, xz + y, torch.zeros((), dtype=x.dtype))
    return xo, rs_act(snk(xo, U["an"]))


# ================================================================================================ metric
def row_stats(got, ref, what):
    """-> (worst ratio over the rows whose reference is not zero, its index); a row whose reference is exactly zero must be exactly zero."""
    g, r = got.double(), ref.double()
    assert g.shape == r.shape, (what, g.shape, r.shape)
    if g.numel() == 0:
        return 0.0, ()
    assert bool(torch.isfinite(g).all()), f"{what}: output not finite (something that must not be read was read, or a row was not written)"
    den, err = r.abs().amax(-1), (g - r).abs().amax(-1)
    z = den == 0
    assert bool((err[z] == 0).all()), f"{what}: a row whose reference is exactly zero is not zero, at {(z & (err != 0)).nonzero()[:4].tolist()}"
    ratio = torch.where(z, torch.zeros_like(err), err / den.clamp_min(1e-300))
    return float(ratio.max()), tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])


WORST = {}


def assert_rows(got, ref, bound, what, group=None):
    worst, at = row_stats(got, ref, what)
    if group is not None:
        WORST[group] = max(WORST.get(group, 0.0), worst)
    assert worst < bound, f"{what}: row {at} at {worst:.3e} >= {bound:.2e}"
    return worst


def model_base(model, ref):
    """dicts of outputs -> the model's worst row against the reference."""
    base = 0.0
    for k, r in ref.items():
        base = max(base, row_stats(model[k], r, "model " + k)[0])
    return base


def bound_of(base, dt):
    return max(4 * base, FLOOR[dt])


def qkv_parts(d, qkv):
    if qkv is not None:
        d["q"], d["k"], d["v"] = qkv[..., :512], qkv[..., 512:1024], qkv[..., 1024:]
    return d


# ================================================================================================ buffers
def strided(flat, B, bs, R, ld, width, off=0):
    """[B, R, width] view of a flat buffer: member b row t column c at off + b * bs + t * ld + c."""
    return flat.as_strided((B, R, width), (bs, ld, 1), flat.storage_offset() + off)


class Out:
    """A guarded output buffer: windows are given as (B, bs, R, ld, off) + row / column ranges."""

    def __init__(self, n, dtype, fill=None):
        self.n, self.dtype = n, dtype
        self.buf, self.view = guarded(n, dtype)
        if fill is not None:
            fill(self.view)
        self.before = None

    def snap(self):
        self.before = self.buf.cpu()

    def check(self, wins, what):
        """wins: [(B, bs, ld, off, r0, r1, c0, c1)] - everything else keeps the bits of the last snap().  -> body after (CPU)."""
        assert_guards(self.buf, self.n, what)
        after = self.buf.cpu()
        win = torch.zeros(self.n + 2 * GUARD, dtype=torch.bool)
        body = win[GUARD:GUARD + self.n]
        for B, bs, ld, off, r0, r1, c0, c1 in wins:
            if r1 > r0 and c1 > c0:
                strided(body, B, bs, r1, ld, c1, off)[:, r0:, c0:] = True
        same = bits(after) == bits(self.before)
        assert bool(same[~win].all()), f"{what}: written outside its window, at element {((~same) & ~win).nonzero().flatten()[:4].tolist()} of the guarded buffer"
        return after[GUARD:GUARD + self.n]


def poisoned(shape, dtype, fill):
    """An input buffer full of NaN with fill(buffer) applied (device)."""
    t = torch.full(shape, float("nan"), dtype=dtype)
    fill(t)
    return t.cuda()


_PACKS = {}


def pack_mats(env, key, dt, mats):
    """{name: [N, K] fp32 CPU} -> fragment-ordered device packs of build dt, once per module."""
    L, ops = env
    if (key, dt) not in _PACKS:
        wd = torch.float32 if dt == X2W else L.WEIGHT_DT[dt]
        _PACKS[(key, dt)] = {k + "_p": ops.pack_skinny(w.cuda().to(wd).contiguous(), dtype=dt) for k, w in mats.items()}
        torch.cuda.synchronize()
    return _PACKS[(key, dt)]


# ================================================================================================ the Q | K | V forms
QW = {"bf16": 1024, "f32": 1536, "planes": 2048}


def form_of(dt, form=None):
    return form or {0: "f32", 1: "bf16"}.get(dt, "planes")


class Next:
    """q_out / vt_out of one launch family (MmxEstNext) with slack columns, batch gaps and guards."""

    def __init__(self, ops, B, Tcap, form, wqkv_p, n1g, n1b):
        self.B, self.Tcap, self.form = B, Tcap, form
        self.W = QW[form]
        self.ldq, self.q_bs = self.W + 8, Tcap * (self.W + 8) + 8
        self.q = Out(B * self.q_bs, torch.float32 if form == "f32" else torch.bfloat16)
        self.NP = {"bf16": 1, "planes": 2, "f32": 0}[form]
        self.vt = None
        if self.NP:
            self.ldvt = round_up(Tcap, 8) + 8
            self.vt_bs = self.NP * 512 * self.ldvt + 16
            self.vt = Out(B * self.vt_bs, torch.bfloat16)
        self.struct = ops.est_next(wqkv=wqkv_p, n1g=n1g, n1b=n1b, q_out=self.q.view, ldq=self.ldq, q_bs=self.q_bs,
                                   vt_out=(self.vt.view if self.vt else None), ldvt=(self.ldvt if self.vt else 0), vt_bs=(self.vt_bs if self.vt else 0))

    def snap(self):
        self.q.snap()
        if self.vt:
            self.vt.snap()

    def check(self, T, tb, what):
        """-> ({q, k, v} [B, T - tb, 512] float32, raw bodies): the windows hold everything that changed; V^T frames T .. are zeros."""
        B = self.B
        qb = self.q.check([(B, self.q_bs, self.ldq, 0, tb, T, 0, self.W)], what + " q_out")
        rows = strided(qb, B, self.q_bs, T, self.ldq, self.W)[:, tb:].float()
        raw = [qb]
        if self.form == "f32":
            return qkv_parts({}, rows), raw
        T8 = round_up(T, 8)
        vb = self.vt.check([(B, self.vt_bs, self.ldvt, 0, 0, self.NP * 512, tb, T8)], what + " vt_out")
        raw.append(vb)
        vt = strided(vb, B, self.vt_bs, self.NP * 512, self.ldvt, T8).float()
        assert bool((vt[:, :, T:] == 0).all()), f"{what}: vt_out frames T .. are not zeros"
        if self.form == "bf16":
            return dict(q=rows[..., :512], k=rows[..., 512:], v=vt[:, :, tb:T].transpose(1, 2)), raw
        v = (vt[:, :512, tb:T] + vt[:, 512:, tb:T]).transpose(1, 2)
        return dict(q=rows[..., :512] + rows[..., 1024:1536], k=rows[..., 512:1024] + rows[..., 1536:], v=v), raw


# ================================================================================================ est_tail
TAIL_MATS = ("wo", "w1", "w2", "wqkv")


@functools.lru_cache(maxsize=None)
def tail_weights(kind="plain"):
    g = torch.Generator().manual_seed(11)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    W = dict(wo=rn(256, 512, sc=512 ** -0.5), w1=rn(1024, 256, sc=1 / 16), w2=rn(256, 1024, sc=1 / 32), wqkv=rn(1536, 256, sc=1 / 16),
             bo=rn(256, sc=0.1), b1=rn(1024, sc=0.1), b2=rn(256, sc=0.1), n3g=1 + rn(256, sc=0.1), n3b=rn(256, sc=0.1),
             n1g=1 + rn(256, sc=0.1), n1b=rn(256, sc=0.1))
    if kind == "wide":                       # FF1 pre-activations of spread 2.7: the GELU tails out to about +-8
        W["n3g"] = W["n3g"] * 2.7
    return W


def make_mask(g, B, T, kind):
    if kind is None:
        return None
    m = (torch.rand(B, T, generator=g) > 0.3).float()
    if kind == "tile":                       # the last member: a whole 64-row tile masked
        m[-1, :64] = 0
    if kind == "f0":                         # frame 0 masked, frame 1 not
        m[:, 0], m[:, 1:2] = 0, 1
    return m


@functools.lru_cache(maxsize=None)
def tail_case(dt, B, T, Tcap, mkind, nxt, form, rng="plain"):
    """Inputs, reference, model and bound of one est_tail case (CPU), built once and left unchanged."""
    g = torch.Generator().manual_seed(1000 * B + T)
    ao = torch.randn(B, T, 512, generator=g)
    if dt == 1:
        ao = bf(ao)
    x0 = torch.randn(B, T, 256, generator=g) + (100.0 if rng == "mean100" else 0.0)
    mask = make_mask(g, B, T, mkind)
    W = tail_weights("wide" if rng == "wide" else "plain")
    x2, act, qkv = tail_chain(ao.double(), x0.double(), cast_w(W, dt, w_read, torch.float64, TAIL_MATS), None if mask is None else mask.double(), nxt)
    ref = qkv_parts(dict(x=x2, act=act), qkv)
    mx, ma, mq = tail_chain(ao, x0, cast_w(W, dt, w_model, torch.float32, TAIL_MATS), mask, nxt, act_rnd(dt), store_rnd(dt), store_rnd(dt, form == "planes"))
    base = model_base(qkv_parts(dict(x=mx, act=ma), mq), ref)
    return dict(dt=dt, B=B, T=T, Tcap=Tcap, nxt=nxt, form=form, rng=rng, ao=ao, x0=x0, mask=mask, ref=ref, base=base,
                bound=bound_of(base, dt), cap=CAP_EST[dt], key=f"est_tail {DT_NAME[dt]} ({B}, {T}) {mkind} nxt {nxt} {form} {rng}")


class TailRun:
    """Device buffers of one est_tail case; launch() may be called hop after hop."""

    def __init__(self, env, c):
        L, ops = env
        self.env, self.c = env, c
        dt, B, T, Tc = c["dt"], c["B"], c["T"], c["Tcap"]
        self.ldao = 512 if T == 130 else 528
        W = tail_weights("wide" if c["rng"] == "wide" else "plain")
        self.w = dict(pack_mats(env, "tail", dt, {k: W[k] for k in TAIL_MATS}), **{k: v.cuda() for k, v in W.items() if k not in TAIL_MATS})
        self.ao = poisoned((B, Tc, self.ldao), tdt(dt), lambda t: t[:, :T, :512].copy_(c["ao"]))
        self.rm = None if c["mask"] is None else poisoned((B, Tc), torch.float32, lambda t: t[:, :T].copy_(c["mask"]))
        self.x = Out(B * Tc * 256, torch.float32, lambda v: v.view(B, Tc, 256)[:, :T].copy_(c["x0"]))
        self.act = Out(B * Tc * 512, tdt(dt))
        self.nx = Next(ops, B, Tc, c["form"], self.w["wqkv_p"], self.w["n1g"], self.w["n1b"]) if c["nxt"] else None

    def launch(self, bm, cfg, T=None, tb=0, what=""):
        """-> (outputs of rows tb .. T - 1 as float32 [B, T - tb, .], raw bodies of every output buffer)."""
        L, ops = self.env
        c = self.c
        B, Tc = c["B"], c["Tcap"]
        T = c["T"] if T is None else T
        for o in (self.x, self.act):
            o.snap()
        if self.nx:
            self.nx.snap()
        ops.est_tail(self.ao, self.x.view, self.w, B=B, T=T, dtype=CODE[c["dt"]], bm=bm, rowmask=self.rm, act_out=self.act.view[256:], act_ld=512,
                     nxt=(self.nx.struct if self.nx else None), t_begin=tb, Tcap=Tc, ldao=self.ldao, **cfg)
        torch.cuda.synchronize()
        xb = self.x.check([(B, Tc * 256, 256, 0, tb, T, 0, 256)], what + " x")
        ab = self.act.check([(B, Tc * 512, 512, 256, tb, T, 0, 256)], what + " act_out")
        out = dict(x=strided(xb, B, Tc * 256, T, 256, 256)[:, tb:], act=strided(ab, B, Tc * 512, T, 512, 256, 256)[:, tb:].float())
        raw = [xb, ab]
        if self.nx:
            parts, r2 = self.nx.check(T, tb, what)
            out.update(parts)
            raw += r2
        return out, raw


def judge(out, c, tb, T, what, group):
    assert c["bound"] <= c["cap"], f"{what}: the model's bound {c['bound']:.2e} is above the suite's {c['cap']:.1e}"
    for k, r in c["ref"].items():
        assert_rows(out[k], r[:, tb:T], c["bound"], f"{what} {k}", group)


# (dtype, form, bm, cfg): every instantiation mmx_est_tail dispatches to (the rows of TAIL_FORMS in csrc/fused.hip)
TAIL_VARIANTS = (
    [(0, None, bm, {}) for bm in (16, 32)]
    + [(1, None, bm, {}) for bm in (16, 32, 64)]
    + [(1, None, 64, dict(waves=4, pf=2)), (1, None, 64, dict(waves=4, pf=4)), (1, None, 32, dict(waves=4, pf=4)), (1, None, 32, dict(waves=8, pf=2)),
       (1, None, 16, dict(waves=8)), (1, None, 32, dict(narrow=True, pf=4)), (1, None, 32, dict(waves=4, pf=2)), (1, None, 32, dict(waves=8, pf=4))]
    + [(X2, None, 32, {}), (X2, None, 32, dict(waves=4)), (X2, None, 16, {}), (X2, None, 16, dict(waves=4)), (X2, None, 32, dict(narrow=True, pf=2)),
       (X2, None, 32, dict(narrow=True, pf=4)), (X2, None, 64, {}), (X2, None, 64, dict(pf=4))]
    + [(X2W, None, bm, {}) for bm in (16, 32, 64)]
    + [(X2, "f32", bm, {}) for bm in (16, 32, 64)] + [(X2W, "f32", 64, {})])
# (B, T, Tcap, mask): one row; a random mask inside a larger Tcap; a last tile of one row; two 64-row tiles and a bit; a masked tile
TAIL_SHAPES = [(2, 1, 1, None), (3, 37, 48, "rand"), (2, 65, 65, None), (1, 130, 130, None), (2, 70, 72, "tile")]
TAIL_RANGES = [(2, 37, 40, "rand", "mean100"), (2, 37, 40, None, "wide")]


def var_id(v):
    dt, form, bm, cfg = v
    return "-".join([DT_NAME[dt], form or "dflt", str(bm)] + [f"{k}{int(x)}" for k, x in cfg.items()])


def tail_cases(dt, form, with_plain_nxt_false=True):
    f = form_of(dt, form)
    cs = [tail_case(dt, *s, True, f) for s in TAIL_SHAPES] + [tail_case(dt, *s[:4], True, f, s[4]) for s in TAIL_RANGES]
    if with_plain_nxt_false:
        cs += [tail_case(dt, *s, False, f) for s in TAIL_SHAPES]
    return cs


@gpu
@pytest.mark.parametrize("var", TAIL_VARIANTS, ids=var_id)
def test_est_tail_rows(env, var):
    """Every shape of TAIL_SHAPES with and without the next block's LayerNorm + Q/K/V, and the two input ranges of TAIL_RANGES
    (residual rows of mean 100: a one-pass variance would lose them; FF1 pre-activations out to +-8: the GELU tails), per row
    against float64.  ao has 16 slack columns of NaN (ldao = 528) except at T = 130."""
    dt, form, bm, cfg = var
    for c in tail_cases(dt, form, form is None):
        out, _ = TailRun(env, c).launch(bm, cfg, what=c["key"])
        judge(out, c, 0, c["T"], c["key"], ("est_tail", DT_NAME[dt]) + (("mean100",) if c["rng"] == "mean100" else ()))
    print(f"est_tail {var_id(var)}: worst rows so far " + ", ".join(f"{' '.join(k[2:]) or 'all others'} {v:.3e}" for k, v in WORST.items() if k[:2] == ("est_tail", DT_NAME[dt])))


STREAM_VARIANTS = [(0, None, 32, {}), (1, None, 32, {}), (1, None, 64, {}), (X2, None, 32, {}), (X2, None, 64, {}), (X2, "f32", 16, {}), (X2W, None, 64, {})]


@gpu
@pytest.mark.parametrize("tb", [16, 48])
@pytest.mark.parametrize("var", STREAM_VARIANTS, ids=var_id)
def test_est_tail_streaming_hop(env, var, tb):
    """(B, T) = (2, 70), t_begin = 16 / 48 after a hop that computed rows 0 .. t_begin - 1: the rows of the earlier hop keep their
    bits in x, act_out, q_out and vt_out (the windows of launch()), the rows from t_begin on equal a t_begin = 0 launch bit for
    bit and meet the float64 bound."""
    dt, form, bm, cfg = var
    c = tail_case(dt, 2, 70, 80, "rand", True, form_of(dt, form))
    full, _ = TailRun(env, c).launch(bm, cfg, what=c["key"] + " whole")
    run = TailRun(env, c)
    run.launch(bm, cfg, T=tb, what=c["key"] + f" hop 0 .. {tb - 1}")
    hop, _ = run.launch(bm, cfg, tb=tb, what=c["key"] + f" hop {tb} ..")
    judge(hop, c, tb, 70, c["key"] + f" t_begin {tb}", ("est_tail", DT_NAME[dt]))
    for k in full:
        assert torch.equal(bits(full[k][:, tb:].float()), bits(hop[k].float())), f"{c['key']} t_begin {tb}: {k} differs from the t_begin = 0 launch"


# ================================================================================================ est_resnet
RES_MATS = ("w1", "w2", "wr", "wqkv")
RES_CIN = [(256, 256), (256, 512), (320, 320), (512, 512)]


@functools.lru_cache(maxsize=None)
def res_weights(cin):
    g = torch.Generator().manual_seed(20 + cin)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    return dict(w1=rn(256, cin, 3, sc=(3 * cin) ** -0.5), w2=rn(256, 256, 3, sc=768 ** -0.5), wr=rn(256, cin, 1, sc=cin ** -0.5),
                wqkv=rn(1536, 256, sc=1 / 16), b1=rn(256, sc=0.1), b2=rn(256, sc=0.1), br=rn(256, sc=0.1), g1=1 + rn(256, sc=0.1),
                be1=rn(256, sc=0.1), g2=1 + rn(256, sc=0.1), be2=rn(256, sc=0.1), n1g=1 + rn(256, sc=0.1), n1b=rn(256, sc=0.1))


@functools.lru_cache(maxsize=None)
def res_case(dt, cin, T, Tcap, mkind, form):
    B = 2
    g = torch.Generator().manual_seed(3000 + 7 * cin + T)
    mask = make_mask(g, B, T, mkind)
    a = torch.randn(B, T, cin, generator=g) * (1.0 if mask is None else mask[..., None])
    if dt == 1:
        a = bf(a)
    tv_all = torch.randn(B, 3 * 256, generator=g)
    tv = tv_all[:, 256:512]
    R = res_weights(cin)
    x, qkv = resnet_chain(a.double(), cast_w(R, dt, w_read, torch.float64, RES_MATS), tv.double(), None if mask is None else mask.double())
    ref = qkv_parts(dict(x=x), qkv)
    mx, mq = resnet_chain(a, cast_w(R, dt, w_model, torch.float32, RES_MATS), tv, mask, act_rnd(dt), store_rnd(dt, form == "planes"))
    base = model_base(qkv_parts(dict(x=mx), mq), ref)
    return dict(dt=dt, B=B, T=T, Tcap=Tcap, cin=cin, form=form, a=a, tv_all=tv_all, mask=mask, ref=ref, base=base, bound=bound_of(base, dt),
                cap=CAP_EST[dt], key=f"est_resnet {DT_NAME[dt]} cin {cin} T {T} {mkind} {form}")


def conv_mat(w):
    """Conv1d weight [Cout, Cin, k] -> [Cout, k * Cin], tap-major (ops.conv1d_matrix)."""
    return w.permute(0, 2, 1).reshape(w.shape[0], -1)


class ResRun:
    def __init__(self, env, c, lda, a=None):
        L, ops = env
        self.env, self.c, self.lda = env, c, lda
        dt, B, T, Tc, cin = c["dt"], c["B"], c["T"], c["Tcap"], c["cin"]
        R = res_weights(cin)
        self.r = dict(pack_mats(env, ("res", cin), dt, {k: (R[k] if k == "wqkv" else conv_mat(R[k])) for k in RES_MATS}),
                      **{k: v.cuda() for k, v in R.items() if k not in RES_MATS})
        a = c["a"] if a is None else a
        self.a = poisoned((B, Tc, lda), tdt(dt), lambda t: t[:, :T, :cin].copy_(a))
        self.rm = None if c["mask"] is None else poisoned((B, Tc), torch.float32, lambda t: t[:, :T].copy_(c["mask"]))
        self.tv = c["tv_all"].cuda()
        self.x = Out(B * Tc * 256, torch.float32)
        self.nx = Next(ops, B, Tc, c["form"], self.r["wqkv_p"], self.r["n1g"], self.r["n1b"])

    def launch(self, bm, waves, T=None, tb=0, what=""):
        L, ops = self.env
        c = self.c
        B, Tc = c["B"], c["Tcap"]
        T = c["T"] if T is None else T
        self.x.snap()
        self.nx.snap()
        ops.est_resnet(self.a, self.lda, c["cin"], self.x.view, self.r, self.tv[:, 256:], 3 * 256, B=B, T=T, dtype=CODE[c["dt"]], bm=bm, rowmask=self.rm,
                       nxt=self.nx.struct, t_begin=tb, Tcap=Tc, waves=waves)
        torch.cuda.synchronize()
        xb = self.x.check([(B, Tc * 256, 256, 0, tb, T, 0, 256)], what + " x")
        out = dict(x=strided(xb, B, Tc * 256, T, 256, 256)[:, tb:])
        parts, raw = self.nx.check(T, tb, what)
        out.update(parts)
        return out, [xb] + raw


def res_bms(dt, cin):
    """Every tile height the dispatch accepts for this build and cin."""
    if dt == 0:
        return [16]
    if dt == 1:
        return [16, 32, 64]
    return [16] if cin == 512 else [16, 32]


RES_T = [(1, None), (2, "rand"), (3, None), (16, "f0"), (17, "rand"), (33, None), (50, "rand")]


def res_cases(dt, cin, form=None):
    return [res_case(dt, cin, T, T + 5, mk, form_of(dt, form)) for T, mk in RES_T]


@gpu
@pytest.mark.parametrize("dt", DTS, ids=lambda d: DT_NAME[d])
@pytest.mark.parametrize("cin,lda", RES_CIN, ids=lambda v: str(v))
def test_est_resnet_rows(env, cin, lda, dt):
    """B = 2, T = 1 / 2 / 3 (shorter than the halo) / 16 / 17 / 33 / 50, with and without a row mask (once with frame 0 masked), tv
    taken from a wider row; every tile height the dispatch accepts for (build, cin) with the default wave count and with
    waves = 4; a_in with NaN slack columns when lda > cin and 5 NaN rows behind T.  The split builds write the pre-split planes;
    the fp32 Q | K | V form (vt_out = NULL) runs once per tile height."""
    for bm in res_bms(dt, cin):
        for waves in (0, 4):
            for c in res_cases(dt, cin):
                out, _ = ResRun(env, c, lda).launch(bm, waves, what=c["key"] + f" bm {bm} waves {waves}")
                judge(out, c, 0, c["T"], c["key"] + f" bm {bm} waves {waves}", ("est_resnet", DT_NAME[dt]))
        if dt == X2:
            for c in res_cases(dt, cin, "f32")[3:]:
                out, _ = ResRun(env, c, lda).launch(bm, 0, what=c["key"] + f" bm {bm}")
                judge(out, c, 0, c["T"], c["key"] + f" bm {bm}", ("est_resnet", DT_NAME[dt]))
    print(f"est_resnet {DT_NAME[dt]} cin {cin} lda {lda}: worst row so far {WORST[('est_resnet', DT_NAME[dt])]:.3e}")


@gpu
@pytest.mark.parametrize("dt", [X2, X2W], ids=lambda d: DT_NAME[d])
def test_est_resnet_split_512_channels_32_rows_is_refused(env, dt):
    """Two bf16 planes of 50 rows x 512 channels do not fit LDS beside h1: the host returns the argument error, nothing launches."""
    L, ops = env
    c = res_case(dt, 512, 33, 38, None, "planes")
    run = ResRun(env, c, 512)
    run.x.snap()
    run.nx.snap()
    with pytest.raises(L.MmxError, match="argument"):
        ops.est_resnet(run.a, 512, 512, run.x.view, run.r, run.tv[:, 256:], 768, B=2, T=33, dtype=2, bm=32, nxt=run.nx.struct, Tcap=38)
    torch.cuda.synchronize()
    assert bool(is_sentinel(run.x.check([], "refused launch x")).all())
    run.nx.q.check([], "refused launch q_out")


@gpu
@pytest.mark.parametrize("tb", [16, 32])
@pytest.mark.parametrize("dt,bm", [(0, 16), (1, 64), (1, 16), (X2, 32), (X2, 16), (X2W, 32)], ids=lambda v: str(v))
def test_est_resnet_streaming_hop(env, dt, bm, tb):
    """T = 50 in Tcap = 64, t_begin = 16 / 32 after a hop over rows 0 .. t_begin - 1: the halo rows come from a_in, the earlier
    hop's rows of x / q_out / vt_out keep their bits, the new rows equal the t_begin = 0 launch bit for bit."""
    c = res_case(dt, 256, 50, 64, "rand", form_of(dt))
    full, _ = ResRun(env, c, 256).launch(bm, 0, what=c["key"] + " whole")
    run = ResRun(env, c, 256)
    run.launch(bm, 0, T=tb, what=c["key"] + f" hop 0 .. {tb - 1}")
    hop, _ = run.launch(bm, 0, tb=tb, what=c["key"] + f" hop {tb} ..")
    judge(hop, c, tb, 50, c["key"] + f" t_begin {tb}", ("est_resnet", DT_NAME[dt]))
    for k in full:
        assert torch.equal(bits(full[k][:, tb:].float()), bits(hop[k].float())), f"{c['key']} t_begin {tb}: {k} differs from the t_begin = 0 launch"


@gpu
@pytest.mark.parametrize("dt,bm", [(0, 16), (1, 64), (1, 32), (X2, 32), (X2, 16), (X2W, 16)], ids=lambda v: str(v))
def test_est_resnet_is_causal_with_a_five_frame_field(env, dt, bm):
    """a_in changed at frame t = 20 (of 50; 19 for the 16-row tiles, the last row of a tile's halo): rows < t and rows > t + 4 of
    every output keep their bits - two causal k3 convolutions see 5 frames - and row t itself changes."""
    c = res_case(dt, 256, 50, 55, None, form_of(dt))
    t = 19 if bm == 16 else 20
    a2 = c["a"].clone()
    a2[:, t] += 1.0
    if dt == 1:
        a2 = bf(a2)
    one, _ = ResRun(env, c, 256).launch(bm, 0, what=c["key"])
    two_, _ = ResRun(env, c, 256, a=a2).launch(bm, 0, what=c["key"] + " changed")
    for k in one:
        a, b = bits(one[k].float()), bits(two_[k].float())
        assert torch.equal(a[:, :t], b[:, :t]), f"{c['key']} bm {bm}: {k} changed before the changed frame"
        assert torch.equal(a[:, t + 5:], b[:, t + 5:]), f"{c['key']} bm {bm}: {k} changed more than 4 frames after the changed frame"
        assert not torch.equal(a[:, t], b[:, t])


# ================================================================================================ dac_ru
RU_BMS = {1: {48: [64, 128, 256], 96: [64, 128, 256], 192: [32, 64, 128]}, X2: {48: [64, 128], 96: [32, 64, 128], 192: [16, 32]}}
RU_DEFAULT = {1: lambda C, d: {48: 128, 96: 256, 192: 32 if d > 3 else 64}[C], X2: lambda C, d: {48: 64, 96: 128 if d > 3 else 64, 192: 32}[C],
              X2W: lambda C, d: {48: 64, 96: 128 if d > 3 else 64, 192: 32}[C]}
RU_DTS = [1, X2, X2W]


@functools.lru_cache(maxsize=None)
def ru_weights(C, dil):
    g = torch.Generator().manual_seed(40 + C + dil)
    rn = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    al = lambda: 0.1 + 2.9 * torch.rand(C, generator=g)
    return dict(w7=rn(C, C, 7, sc=(7 * C) ** -0.5), w1=rn(C, C, 1, sc=C ** -0.5), b7=rn(C, sc=0.1), b1=rn(C, sc=0.1), a0=al(), a2=al(), an=al())


@functools.lru_cache(maxsize=None)
def ru_case(dt, C, dil, T, lens):
    B = 3 if lens else 2
    g = torch.Generator().manual_seed(5000 + C + 31 * dil + T)
    x = torch.randn(B, T, C, generator=g)
    U = ru_weights(C, dil)
    mats = ("w7", "w1")
    U64 = cast_w(U, dt, w_read, torch.float64, mats)
    xo, act = ru_chain(x.double(), U64, dil, lens, snk=snake64)
    ref = dict(x=xo, act=act)
    mx, ma = ru_chain(x, cast_w(U, dt, w_model, torch.float32, mats), dil, lens, act_rnd(dt), store_rnd(dt))
    base = model_base(dict(x=mx, act=ma), ref)
    return dict(dt=dt, B=B, C=C, dil=dil, T=T, lens=lens, x=x, ref=ref, base=base, bound=bound_of(base, dt), cap=CAP_RU[dt],
                key=f"dac_ru {DT_NAME[dt]} C {C} dil {dil} T {T} lens {lens}")


def ru_lens(T):
    return (T, 1, 0)


def ru_Ts(bm):
    return sorted({1, 3, bm - 1, bm, bm + 1, 2 * bm + 5})


def ru_pack(env, dt, C, dil):
    L, ops = env
    key = ("ru", C, dil, dt)
    if key not in _PACKS:
        U = ru_weights(C, dil)
        w7p, w1p = ops.pack_dac_ru(U["w7"].cuda(), U["w1"].cuda(), dt)
        _PACKS[key] = dict(w7_p=w7p, w1_p=w1p, b7=U["b7"].cuda(), b1=U["b1"].cuda(), a0=U["a0"].cuda(), a2=U["a2"].cuda(), an=U["an"].cuda())
        torch.cuda.synchronize()
    return _PACKS[key]


def run_ru(env, c, bm, with_act, what, B=None, x=None, lens="case"):
    """One mmx_dac_ru launch: x with NaN in rows >= lens[b] and in the 8-element gap behind every member.  -> (outputs, raw bodies)."""
    L, ops = env
    dt, C, dil, T = c["dt"], c["C"], c["dil"], c["T"]
    x = c["x"] if x is None else x
    lens = c["lens"] if lens == "case" else lens
    B, T = x.shape[0], x.shape[1]
    ru = ru_pack(env, dt, C, dil)
    bs = T * C + 8

    def fill(t):
        for b in range(B):
            n = T if lens is None else lens[b]
            t[b * bs:b * bs + n * C].view(n, C).copy_(x[b, :n])
    xd = poisoned((B * bs,), torch.float32, fill)
    xo, ao = Out(B * bs, torch.float32), (Out(B * bs, tdt(dt)) if with_act else None)
    xo.snap()
    if ao:
        ao.snap()
    ops.dac_ru(xd, xo.view, ru, B=B, T=T, C_=C, dil=dil, dtype=CODE[dt], act_out=(ao.view if ao else None), alpha_next=(ru["an"] if ao else None),
               lens=(None if lens is None else torch.tensor(lens, dtype=torch.int32).cuda()), bm=bm, x_bs=bs)
    torch.cuda.synchronize()
    win = [(B, bs, C, 0, 0, T, 0, C)]
    xb = xo.check(win, what + " x_out")
    out, raw = dict(x=strided(xb, B, bs, T, C, C)), [xb]
    if ao:
        ab = ao.check(win, what + " act_out")
        out["act"] = strided(ab, B, bs, T, C, C).float()
        raw.append(ab)
    return out, raw


RU_TILES = [(dt, C, bm) for dt in (1, X2) for C in (48, 96, 192) for bm in RU_BMS[dt][C]] + [(X2W, C, 0) for C in (48, 96, 192)]


@gpu
@pytest.mark.parametrize("dt,C,bm", RU_TILES, ids=[f"{DT_NAME[d]}-{C}-{bm}" for d, C, bm in RU_TILES])
def test_dac_ru_rows(env, dt, C, bm):
    """Every tile the dispatch instantiates (the weight-plane build has one per (C, dil)), dil 1 / 3 / 9, T = 1, 3 (shorter than
    the halo), bm - 1, bm, bm + 1, 2 bm + 5: B = 3 with lens = [T, 1, 0] and act_out, B = 2 without lens and without act_out,
    x_bs = T C + 8.  Members 0 and 1 of the lens launch equal B = 1 launches of T and 1 rows bit for bit."""
    for dil in (1, 3, 9):
        tile = bm or RU_DEFAULT[dt](C, dil)
        for T in ru_Ts(tile):
            c, c2 = ru_case(dt, C, dil, T, ru_lens(T)), ru_case(dt, C, dil, T, None)
            tag = c["key"] + f" bm {bm}"
            out, _ = run_ru(env, c, bm, True, tag)
            assert max(c["bound"], c2["bound"]) <= c["cap"], f"{tag}: the model's bound is above the suite's {c['cap']:.1e}"
            for k, r in c["ref"].items():
                assert_rows(out[k], r, c["bound"], f"{tag} {k}", ("dac_ru", DT_NAME[dt]))
            for b, n in ((0, T), (1, 1)):
                solo, _ = run_ru(env, c, bm, True, tag + f" member {b} alone", x=c["x"][b:b + 1, :n].contiguous(), lens=None)
                for k in solo:
                    assert torch.equal(bits(solo[k][0].float()), bits(out[k][b, :n].float())), f"{tag}: {k} of member {b} differs from its B = 1 launch"
            out2, _ = run_ru(env, c2, bm, False, c2["key"] + f" bm {bm}")
            assert_rows(out2["x"], c2["ref"]["x"], c2["bound"], f"{c2['key']} bm {bm} x", ("dac_ru", DT_NAME[dt]))
    print(f"dac_ru {DT_NAME[dt]} C {C} bm {bm}: worst row so far {WORST[('dac_ru', DT_NAME[dt])]:.3e}")


@gpu
@pytest.mark.parametrize("dt", RU_DTS, ids=lambda d: DT_NAME[d])
def test_dac_ru_refuses_other_tiles(env, dt):
    """A tile height the dispatch has no instantiation for is the argument error (a host check: nothing is written)."""
    L, ops = env
    for C in (48, 96, 192):
        ok = set(RU_BMS[dt][C]) if dt in RU_BMS else {RU_DEFAULT[dt](C, 1)}
        for bm in sorted({16, 32, 48, 64, 128, 256, 512} - ok):
            c = ru_case(dt, C, 1, 3, None)
            with pytest.raises(L.MmxError, match="argument"):
                run_ru(env, c, bm, True, f"{c['key']} bm {bm}")


# ================================================================================================ on the CPU
def all_cases():
    for dt in DTS:
        for form in ((None, "f32") if dt in (X2, X2W) else (None,)):
            yield from tail_cases(dt, form, form is None)
        yield tail_case(dt, 2, 70, 80, "rand", True, form_of(dt))
        if dt == X2:
            yield tail_case(dt, 2, 70, 80, "rand", True, "f32")
        for cin, _ in RES_CIN[1:]:
            yield from res_cases(dt, cin)
        if dt == X2:
            yield from res_cases(dt, 256, "f32")[3:]
        yield res_case(dt, 256, 50, 64, "rand", form_of(dt))
        yield res_case(dt, 256, 50, 55, None, form_of(dt))
    for dt in RU_DTS:
        for C in (48, 96, 192):
            for dil in (1, 3, 9):
                tiles = RU_BMS[dt][C] if dt in RU_BMS else [RU_DEFAULT[dt](C, dil)]
                for T in sorted({T for bm in tiles for T in ru_Ts(bm)}):
                    yield ru_case(dt, C, dil, T, ru_lens(T))
                    yield ru_case(dt, C, dil, T, None)


def test_model_bounds_fit_the_caps():
    """Every case of this file: base > 0 (the model is not the reference) and max(4 * base, floor) stays under the tolerance the
    suite already states for the kernel and build - the inputs were chosen so; nothing here comes from a kernel."""
    groups = {}
    for c in all_cases():
        assert c["base"] > 0 and c["bound"] <= c["cap"], f"{c['key']}: base {c['base']:.3e} -> bound {c['bound']:.3e} above the cap {c['cap']:.1e}"
        k = (c["key"].split()[0], DT_NAME[c["dt"]]) + (("mean100",) if c.get("rng") == "mean100" else ())
        groups[k] = max(groups.get(k, 0.0), c["base"])
    for k, base in groups.items():
        print(f"{' '.join(k)}: base {base:.3e} -> bound {max(4 * base, FLOOR[{v: d for d, v in DT_NAME.items()}[k[1]]]):.3e}")


def rand_sd(g, shapes):
    return {k: torch.randn(*s, generator=g, dtype=torch.float64) * (0.1 if len(s) == 1 else (s[-1] * (s[1] if len(s) == 3 else 1)) ** -0.5) for k, s in shapes.items()}


def attention64(q, k, v, bias):
    B, T, _ = q.shape
    h = lambda t: t.view(B, T, 8, 64).transpose(1, 2)
    s = (h(q) @ h(k).transpose(-2, -1)) * 64 ** -0.5 + bias[:, None]
    return (torch.softmax(s, dim=-1) @ h(v)).transpose(1, 2).reshape(B, T, 512)


def block_w(sd, p, pn):
    return dict(wo=sd[p + ".attn1.to_out.0.weight"], bo=sd[p + ".attn1.to_out.0.bias"], n3g=sd[p + ".norm3.weight"], n3b=sd[p + ".norm3.bias"],
                w1=sd[p + ".ff.net.0.proj.weight"], b1=sd[p + ".ff.net.0.proj.bias"], w2=sd[p + ".ff.net.2.weight"], b2=sd[p + ".ff.net.2.bias"],
                n1g=sd[pn + ".norm1.weight"], n1b=sd[pn + ".norm1.bias"],
                wqkv=torch.cat([sd[pn + ".attn1.to_q.weight"], sd[pn + ".attn1.to_k.weight"], sd[pn + ".attn1.to_v.weight"]]))


def test_tail_ref_matches_the_oracle_block():
    """Two oracle.flow.basic_transformer_block in a row on a synthetic float64 state dict.  Block 0: its attention output restated
    here, then tail_ref = the oracle's block output (x) and LayerNorm + Q | K | V of block 1; block 1: attention over exactly
    those Q | K | V, then tail_ref again = the oracle's second output - which pins the Q | K | V part too.  1e-12 per row."""
    from oracle import flow as OF
    g = torch.Generator().manual_seed(5)
    shapes = {}
    for p in ("b0", "b1"):
        shapes.update({p + ".norm1.weight": (256,), p + ".norm1.bias": (256,), p + ".norm3.weight": (256,), p + ".norm3.bias": (256,),
                       p + ".attn1.to_q.weight": (512, 256), p + ".attn1.to_k.weight": (512, 256), p + ".attn1.to_v.weight": (512, 256),
                       p + ".attn1.to_out.0.weight": (256, 512), p + ".attn1.to_out.0.bias": (256,), p + ".ff.net.0.proj.weight": (1024, 256),
                       p + ".ff.net.0.proj.bias": (1024,), p + ".ff.net.2.weight": (256, 1024), p + ".ff.net.2.bias": (256,)})
    sd = rand_sd(g, shapes)
    for p in ("b0", "b1"):
        sd[p + ".norm1.weight"] += 1
        sd[p + ".norm3.weight"] += 1
    B, T = 2, 23
    x = torch.randn(B, T, 256, generator=g, dtype=torch.float64)
    bias = torch.zeros(B, T, T, dtype=torch.float64)
    bias[1, :, 17:] = -1.0e10
    y0 = OF.basic_transformer_block(sd, "b0", x, bias)
    y1 = OF.basic_transformer_block(sd, "b1", y0, bias)
    qkv0 = ln(x, sd["b0.norm1.weight"], sd["b0.norm1.bias"]) @ block_w(sd, "b0", "b0")["wqkv"].t()
    ao0 = attention64(qkv0[..., :512], qkv0[..., 512:1024], qkv0[..., 1024:], bias)
    x2, act, qkv1 = tail_chain(ao0, x, block_w(sd, "b0", "b1"), None, True)
    assert row_stats(x2, y0, "tail_ref x")[0] < 1e-12 and torch.equal(act, x2)
    ao1 = attention64(qkv1[..., :512], qkv1[..., 512:1024], qkv1[..., 1024:], bias)
    x3, _, _ = tail_chain(ao1, x2, block_w(sd, "b1", "b1"), None, False)
    assert row_stats(x3, y1, "tail_ref through Q | K | V")[0] < 1e-12
    mask = (torch.rand(B, T, generator=g) > 0.3).double()
    xm, am, _ = tail_chain(ao0, x, block_w(sd, "b0", "b1"), mask, False)
    assert torch.equal(xm, x2 * mask[..., None]) and torch.equal(am, xm)


@pytest.mark.parametrize("cin", [256, 320])
def test_resnet_ref_matches_the_oracle(cin):
    """oracle.flow.causal_resnet on a synthetic float64 state dict, with and without a mask (frame 0 masked once): 1e-12 per row."""
    from oracle import flow as OF
    g = torch.Generator().manual_seed(6 + cin)
    sd = rand_sd(g, {"r.block1.block.0.weight": (256, cin, 3), "r.block1.block.0.bias": (256,), "r.block1.block.2.weight": (256,),
                     "r.block1.block.2.bias": (256,), "r.block2.block.0.weight": (256, 256, 3), "r.block2.block.0.bias": (256,),
                     "r.block2.block.2.weight": (256,), "r.block2.block.2.bias": (256,), "r.mlp.1.weight": (256, 1024), "r.mlp.1.bias": (256,),
                     "r.res_conv.weight": (256, cin, 1), "r.res_conv.bias": (256,)})
    sd["r.block1.block.2.weight"] += 1
    sd["r.block2.block.2.weight"] += 1
    R = dict(w1=sd["r.block1.block.0.weight"], b1=sd["r.block1.block.0.bias"], g1=sd["r.block1.block.2.weight"], be1=sd["r.block1.block.2.bias"],
             w2=sd["r.block2.block.0.weight"], b2=sd["r.block2.block.0.bias"], g2=sd["r.block2.block.2.weight"], be2=sd["r.block2.block.2.bias"],
             wr=sd["r.res_conv.weight"], br=sd["r.res_conv.bias"], n1g=torch.ones(256, dtype=torch.float64), n1b=torch.zeros(256, dtype=torch.float64),
             wqkv=torch.zeros(1536, 256, dtype=torch.float64))
    B, T = 2, 19
    a = torch.randn(B, T, cin, generator=g, dtype=torch.float64)
    temb = torch.randn(B, 1024, generator=g, dtype=torch.float64)
    tv = F.linear(F.mish(temb), sd["r.mlp.1.weight"], sd["r.mlp.1.bias"])
    for mkind in (None, "rand", "f0"):
        mask = make_mask(g, B, T, mkind)
        m = torch.ones(B, T, 1, dtype=torch.float64) if mask is None else mask.double()[..., None]
        want = OF.causal_resnet(sd, "r", a, m, temb)
        got, _ = resnet_chain(a * m, R, tv, None if mask is None else mask.double())
        assert row_stats(got, want, f"resnet_ref {mkind}")[0] < 1e-12


@pytest.mark.parametrize("C,dil", [(48, 1), (96, 3), (192, 9)])
def test_ru_ref_matches_the_oracle(C, dil):
    """oracle.dac.residual_unit (weight norm folded by the oracle's own fold) on a synthetic float64 state dict: the whole batch
    without lens, and with lens every member's live rows = the oracle on that member alone, its other rows zero.  1e-12 per row."""
    from oracle import dac as OD
    g = torch.Generator().manual_seed(8 + C)
    rd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {"u.block.0.alpha": 0.1 + 2.9 * torch.rand(1, C, 1, generator=g, dtype=torch.float64), "u.block.2.alpha": 0.1 + 2.9 * torch.rand(1, C, 1, generator=g, dtype=torch.float64),
          "u.block.1.0.weight_g": 1 + 0.1 * rd(C, 1, 1), "u.block.1.0.weight_v": rd(C, C, 7), "u.block.1.0.bias": 0.1 * rd(C),
          "u.block.3.0.weight_g": 1 + 0.1 * rd(C, 1, 1), "u.block.3.0.weight_v": rd(C, C, 1), "u.block.3.0.bias": 0.1 * rd(C)}
    U = dict(w7=OD.fold_weight_norm(sd["u.block.1.0.weight_g"], sd["u.block.1.0.weight_v"]), b7=sd["u.block.1.0.bias"],
             w1=OD.fold_weight_norm(sd["u.block.3.0.weight_g"], sd["u.block.3.0.weight_v"]), b1=sd["u.block.3.0.bias"],
             a0=sd["u.block.0.alpha"].reshape(C), a2=sd["u.block.2.alpha"].reshape(C), an=0.1 + 2.9 * torch.rand(C, generator=g, dtype=torch.float64))
    B, T = 3, 40
    x = rd(B, T, C)
    orc = lambda z: OD.residual_unit(sd, "u", z.transpose(1, 2), dil).transpose(1, 2)
    xo, act = ru_chain(x, U, dil, None, snk=snake64)
    assert row_stats(xo, orc(x), "ru_ref")[0] < 1e-12
    assert row_stats(act, OD.snake(xo.transpose(1, 2), U["an"].reshape(1, C, 1)).transpose(1, 2), "ru_ref act")[0] < 1e-12
    lens = (T, 7, 0)
    xp = x.clone()
    for b, n in enumerate(lens):
        xp[b, n:] = float("nan")
    xl, al = ru_chain(xp, U, dil, lens, snk=snake64)
    for b, n in enumerate(lens):
        assert bool((xl[b, n:] == 0).all()) and bool((al[b, n:] == 0).all())
        if n:
            assert row_stats(xl[b:b + 1, :n], orc(x[b:b + 1, :n]), f"ru_ref member {b}")[0] < 1e-12
