"""Float64 parity of the windowed GEMM (every block tile x dtype x MmxGemmParams path) and of the elementwise / glue kernels
and mmx_attn_dense options that only the whole-model goldens exercised.

Every reference is the same operation in plain torch float64 on the CPU, on the values as the kernel reads them: bf16-rounded
weights and activations for dtype 1, bf16-rounded weights only for dtypes 2 / 3, the fp32 weights themselves for the
weight-plane dtypes.  Outputs are allocated with guard elements in front, behind and in every slack column, filled with a
sentinel (NaN; 7.0 for bf16): an element the kernel must not write has to keep it, an element it must write has to lose it.

GEMM bounds are the table of test_gpu_kernels.py (relative to max |ref|; 1e-2 for a bf16 out_act) and, for the weight
planes, the bounds of test_gpu_split.py::test_weight_planes_gemm_vs_float64."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

X2W, X3W = 0x12, 0x13
TOL = {0: 2e-5, 1: 2e-2, 2: 4e-5, 3: 2e-5, X2W: 4e-5, X3W: 3e-6}
DT_NAME = {0: "f32", 1: "bf16", 2: "x2", 3: "x3", X2W: "x2w", X3W: "x3w"}
BASE = {0: 0, 1: 1, 2: 2, 3: 3, X2W: 2, X3W: 3}              # the dtype code the entry point is called with
TILES = ["128x128", "128x64", "64x64", "32x64"]
CFGS = [(t, d) for t in TILES for d in (0, 1, 2, 3)] + [(t, d) for t in ("64x64", "32x64") for d in (X2W, X3W)]
PLAIN_CFGS = [c for c in CFGS if c[1] < 4]
cfg_id = lambda c: f"{c[0]}-{DT_NAME[c[1]]}"
# M, N: no multiple of any tile, a second block in both directions (128x64 also at its own N <= 64 shape)
SHAPES = {"128x128": [(150, 136)], "128x64": [(300, 48), (150, 136)], "64x64": [(150, 136)], "32x64": [(150, 136)]}
KS = (96, 40)                                                 # 40: the zero-padded K tail of the last k-tile is read
GUARD = 64                                                    # sentinel elements in front of and behind every output


@pytest.fixture(scope="module")
def env():
    from mmx import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    _lib.load()
    return _lib, ops


def tol_f(dt):
    return TOL[dt]


def tol_a(dt):
    return 1e-2 if dt == 1 else TOL[dt]


def tdt(dt):
    return torch.bfloat16 if dt == 1 else torch.float32


def sentinel(dtype):
    return 7.0 if dtype == torch.bfloat16 else float("nan")


def is_sentinel(t):
    return (t == 7.0) if t.dtype == torch.bfloat16 else torch.isnan(t)


def guarded(n, dtype):
    """A device buffer of n elements between two guards: (whole buffer, the n-element view a kernel is handed)."""
    buf = torch.full((n + 2 * GUARD,), sentinel(dtype), dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def assert_guards(buf, n, what=""):
    b = buf.cpu()
    assert bool(is_sentinel(b[:GUARD]).all()) and bool(is_sentinel(b[GUARD + n:]).all()), f"{what}: wrote outside its output"


def rel_err(got, ref):
    return float((got.double() - ref.double()).abs().max() / (ref.double().abs().max() + 1e-300))


def act64(y, act, slope=0.1):
    if act == "lrelu":
        return F.leaky_relu(y, slope)
    if act == "gelu":
        return F.gelu(y)
    if act == "silu":
        return F.silu(y)
    if act == "mish":
        return F.mish(y)
    if act == "tanh":
        return torch.tanh(y)
    return y


def snake64(v, alpha):
    return v + (alpha.double() + 1e-9).reciprocal() * torch.sin(alpha.double() * v) ** 2


def rnd(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


# ================================================================================================ A. windowed GEMM
def operands(env, dt, x, w):
    """x: activations (fp32, CPU, any shape), w: weight matrix [N, K] (fp32, CPU) -> the device operands of dtype dt and both
    as float64 as the kernel reads them."""
    L, ops = env
    xa = x.to(tdt(dt)).cuda()
    wp = ops.pack_linear(w.cuda(), dt)
    wr = w.double() if dt in (X2W, X3W) else w.to(L.WEIGHT_DT[dt]).double()
    return xa, wp, xa.cpu().double(), wr


def place(ref, ld, bstride, out_off=0, out_len=None):
    """Where mmx_gemm_win puts ref [batch, M, N]: element (b, m, n) at b * bstride + m * ld + n + out_off if that lies in
    [0, out_len) of its batch item.  -> (expected flat values, written mask) over batch * bstride elements."""
    batch, M, N = ref.shape
    exp = torch.zeros(batch * bstride, dtype=torch.float64)
    mask = torch.zeros(batch * bstride, dtype=torch.bool)
    lin = torch.arange(M)[:, None] * ld + torch.arange(N)[None, :] + out_off
    ok = (lin >= 0) & (lin < (out_len if out_len is not None else bstride))
    for b in range(batch):
        exp[b * bstride + lin[ok]] = ref[b][ok]
        mask[b * bstride + lin[ok]] = True
    return exp, mask


def check_flat(got, exp, mask, tol, what):
    """got: the whole guarded buffer (CPU).  Written elements within tol of max |exp|, all others still the sentinel."""
    n = exp.numel()
    body = got[GUARD:GUARD + n]
    keep = torch.ones(got.numel(), dtype=torch.bool)
    keep[GUARD:GUARD + n] = ~mask
    assert bool(is_sentinel(got[keep]).all()), f"{what}: an element outside the output window was written"
    w = body[mask].double()
    assert bool(torch.isfinite(w).all()), f"{what}: an element of the output window was not written (or is not finite)"
    err = float((w - exp[mask]).abs().max() / (exp[mask].abs().max() + 1e-300))
    assert err < tol, f"{what}: {err:.3e} >= {tol:.1e}"


def run_gemm(env, cfg, A, W, M, N, *, exp_f=None, exp_a=None, ld=None, bstride=None, tag="", **kw):
    """Launches the problem with the forced tile and with tile = 0 into sentinel-filled outputs, checks both against the
    expected (values, mask) pairs and against each other.  -> {tile: (out_f32 body, out_act body)} (CPU)."""
    L, ops = env
    tile, dt = cfg
    n = (exp_f or exp_a)[0].numel()
    outs = {}
    for tl in (L.TILES[tile], 0):
        bf, vf = guarded(n, torch.float32) if exp_f else (None, None)
        ba, va = guarded(n, tdt(dt)) if exp_a else (None, None)
        ops.gemm(A, W, M, N, dtype=BASE[dt], tile=tl, out_f32=vf, ldo_f=ld, of_bstride=bstride, out_act=va, ldo_a=ld,
                 oa_bstride=bstride, **kw)
        torch.cuda.synchronize()
        what = f"{tag} {cfg_id(cfg)} tile={tl}"
        got = []
        for buf, exp, tol, name in ((bf, exp_f, tol_f(dt), "out_f32"), (ba, exp_a, tol_a(dt), "out_act")):
            if exp is None:
                got.append(None)
                continue
            c = buf.cpu()
            check_flat(c, exp[0], exp[1], tol, f"{what} {name}")
            got.append(c[GUARD:GUARD + n])
        outs[tl] = got
    for i, (exp, tol) in enumerate(((exp_f, tol_f(dt)), (exp_a, tol_a(dt)))):      # the forced tile and the heuristic's agree
        if exp is not None:
            a, b = outs[L.TILES[tile]][i][exp[1]].double(), outs[0][i][exp[1]].double()
            d = float((a - b).abs().max() / (exp[0][exp[1]].abs().max() + 1e-300))
            assert d < tol, f"{tag} {cfg_id(cfg)}: forced tile vs tile=0 differ by {d:.3e}"
    return outs


ACTS = [("none", "none"), ("lrelu", "none"), ("gelu", "none"), ("silu", "none"), ("mish", "none"), ("tanh", "none"), ("none", "mish")]


@pytest.mark.parametrize("act,act2", ACTS, ids=[f"{a}+{b}" for a, b in ACTS])
@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_gemm_linear_every_activation(env, cfg, act, act2):
    """Bias + every activation code; act2 = mish writes out_f32 before and out_act after it."""
    for M, N in SHAPES[cfg[0]]:
        for K in KS:
            g = torch.Generator().manual_seed(M + N + K)
            x, w, b = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N)
            xa, wp, xr, wr = operands(env, cfg[1], x, w)
            f = act64(xr @ wr.t() + b.double(), act)
            a = act64(f, act2)
            run_gemm(env, cfg, xa, wp, M, N, exp_f=place(f[None], N, M * N), exp_a=place(a[None], N, M * N), ld=N, bstride=M * N,
                     lda=K, cin=K, bias=b.cuda(), act=act, act2=act2, tag=f"linear {M}x{N}x{K} {act}+{act2}")


@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_gemm_snake_and_bias_modulus(env, cfg):
    """N = 3 * 48 output phases sharing 48 biases and 48 Snake alphas (the ConvTranspose1d's bias_mod / alpha_mod)."""
    M, N, mod = SHAPES[cfg[0]][0][0], 144, 48
    for K in KS:
        g = torch.Generator().manual_seed(K)
        x, w, b = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, mod)
        alpha = 1 + 0.1 * rnd(g, mod)
        xa, wp, xr, wr = operands(env, cfg[1], x, w)
        f = xr @ wr.t() + b.double().repeat(3)
        a = snake64(f, alpha.repeat(3))
        run_gemm(env, cfg, xa, wp, M, N, exp_f=place(f[None], N, M * N), exp_a=place(a[None], N, M * N), ld=N, bstride=M * N,
                 lda=K, cin=K, bias=b.cuda(), bias_mod=mod, alpha=alpha.cuda(), alpha_mod=mod, tag=f"snake K={K}")


@pytest.mark.parametrize("s", [2, 5])
@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_gemm_strided_conv(env, cfg, s):
    """The DAC encoder's down-sampling Conv1d(k = 2s, stride s, padding ceil(s / 2)) through row_stride."""
    L, ops = env
    T, B, pad = 77, 2, math.ceil(s / 2)
    To = (T + 2 * pad - 2 * s) // s + 1
    N = SHAPES[cfg[0]][0][1]
    for Cin in (24, 8):
        g = torch.Generator().manual_seed(s * 100 + Cin)
        x, w, b = rnd(g, B, T, Cin), rnd(g, N, Cin, 2 * s, scale=(2 * s * Cin) ** -0.5), rnd(g, N)
        xa, wp, xr, wr = operands(env, cfg[1], x, ops.conv1d_matrix(w))
        wq = wr.reshape(N, 2 * s, Cin).permute(0, 2, 1)
        ref = F.conv1d(xr.transpose(1, 2), wq, b.double(), stride=s, padding=pad).transpose(1, 2)
        assert ref.shape == (B, To, N)
        e = place(ref, N, To * N)
        run_gemm(env, cfg, xa, wp, To, N, exp_f=e, exp_a=e, ld=N, bstride=To * N, lda=Cin, cin=Cin, ntaps=2 * s, row_stride=s,
                 row_off=-pad, row_lo=0, row_hi=T, batch=B, a_bstride=T * Cin, bias=b.cuda(), tag=f"strided conv s={s} Cin={Cin}")


@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_gemm_dilated_conv_column_and_row_window(env, cfg):
    """3 taps, dilation 2, cin < lda and rows outside [row_lo, row_hi) read as zero: the columns cin .. lda - 1 and the rows
    outside the window hold NaN, so that any read of them shows."""
    L, ops = env
    B, T, lo, hi = 2, 150, 3, 146
    N = SHAPES[cfg[0]][0][1]
    for lda, Cin in ((128, 96), (64, 40)):
        g = torch.Generator().manual_seed(lda)
        x, w, b = rnd(g, B, T, Cin), rnd(g, N, Cin, 3, scale=(3 * Cin) ** -0.5), rnd(g, N)
        buf = torch.full((B, T, lda), float("nan"))
        buf[:, lo:hi, :Cin] = x[:, lo:hi]
        xa, wp, _, wr = operands(env, cfg[1], buf, ops.conv1d_matrix(w))
        xr = torch.zeros(B, T, Cin, dtype=torch.float64)
        xr[:, lo:hi] = x[:, lo:hi].to(tdt(cfg[1])).double()
        wq = wr.reshape(N, 3, Cin).permute(0, 2, 1)
        ref = F.conv1d(xr.transpose(1, 2), wq, b.double(), dilation=2, padding=2).transpose(1, 2)
        e = place(ref, N, T * N)
        run_gemm(env, cfg, xa, wp, T, N, exp_f=e, exp_a=e, ld=N, bstride=T * N, lda=lda, cin=Cin, ntaps=3, dil=2, row_off=-2,
                 row_lo=lo, row_hi=hi, batch=B, a_bstride=T * lda, bias=b.cuda(), tag=f"dilated conv lda={lda} cin={Cin}")


@pytest.mark.parametrize("T", [45, 130])
@pytest.mark.parametrize("cfg", PLAIN_CFGS, ids=cfg_id)
def test_gemm_swapped_operands_batched(env, cfg, T):
    """V^T[b] = W_v X_b^T as the flow encoder launches it: A = the weight (a_bstride = 0), W = the activations of batch item b
    (w_bstride), one bias per ROW, out_act rows of Tp = round_up(T, 8) elements whose columns T .. Tp - 1 are not written."""
    L, ops = env
    B, M, dt = 3, 150, cfg[1]
    Tp = ops.round_up(T, 8)
    for K in KS:
        Kp = ops.round_up(K, 32)
        g = torch.Generator().manual_seed(T + K)
        wv, x, b = rnd(g, M, K, scale=K ** -0.5), rnd(g, B, T, K), rnd(g, M)
        A = wv.to(tdt(dt)).cuda()                                          # the A operand has the activation storage type
        W = torch.zeros(B * T, Kp, dtype=L.WEIGHT_DT[dt], device="cuda")   # the W operand the weight storage type, K zero padded
        W[:, :K] = x.reshape(B * T, K)
        ref = A.cpu().double() @ W.cpu().double()[:, :K].reshape(B, T, K).transpose(1, 2) + b.double()[None, :, None]
        run_gemm(env, cfg, A, W, M, T, exp_a=place(ref, Tp, M * Tp), ld=Tp, bstride=M * Tp, lda=K, cin=K, batch=B, a_bstride=0,
                 w_bstride=T * Kp, bias=b.cuda(), bias_per_row=True, tag=f"swapped T={T} K={K}")


@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_gemm_vector_and_scalar_epilogue_bit_identical(env, cfg):
    """ldo_f = ldo_a = ldr = N (16-byte stores and residual loads) against N + 1 and N + 3 (element-wise ones): the same bits,
    and the slack columns keep their sentinel."""
    L, ops = env
    M, N, K = 150, 136, 96
    g = torch.Generator().manual_seed(11)
    x, w, b, res = rnd(g, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N), rnd(g, M, N)
    xa, wp, xr, wr = operands(env, cfg[1], x, w)
    f = F.gelu(xr @ wr.t() + b.double()) + res.double()
    got = {}
    for ld in (N, N + 1, N + 3):
        r = torch.zeros(M, ld)
        r[:, :N] = res
        e = place(f[None], ld, M * ld)
        o = run_gemm(env, cfg, xa, wp, M, N, exp_f=e, exp_a=e, ld=ld, bstride=M * ld, lda=K, cin=K, bias=b.cuda(), act="gelu",
                     residual=r.cuda(), ldr=ld, tag=f"epilogue ld={ld}")
        got[ld] = [t.reshape(M, ld)[:, :N] for t in o[L.TILES[cfg[0]]]]
    for ld in (N + 1, N + 3):
        assert torch.equal(got[ld][0], got[N][0]) and torch.equal(got[ld][1], got[N][1]), f"ld={ld} differs from the vector epilogue"


@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_gemm_output_window_convtranspose_clip(env, cfg):
    """ConvTranspose1d(kernel 10, stride 5, padding 3, output_padding 1) with Cout = 20: out_off = -60 (no multiple of 8) cuts
    the first GEMM row, out_len = T * 100 the last one; nothing outside [0, out_len) of a batch item may be written."""
    L, ops = env
    B, T, s, Cout = 2, 149, 5, 20
    for Cin in (48, 8):
        g = torch.Generator().manual_seed(Cin)
        x, w, b = rnd(g, B, T, Cin), rnd(g, Cin, Cout, 2 * s, scale=(2 * Cin) ** -0.5), rnd(g, Cout)
        dt = cfg[1]
        xa = x.to(tdt(dt)).cuda()
        wp = ops.pack_convtranspose1d(w.cuda(), s, dt)
        wr = w.double() if dt in (X2W, X3W) else w.to(L.WEIGHT_DT[dt]).double()
        ref = F.conv_transpose1d(xa.cpu().double().transpose(1, 2), wr, b.double(), stride=s, padding=3, output_padding=1)
        assert ref.shape == (B, Cout, T * s)
        n = T * s * Cout
        e = (ref.transpose(1, 2).reshape(-1), torch.ones(B * n, dtype=torch.bool))
        run_gemm(env, cfg, xa, wp, T + 1, s * Cout, exp_f=e, exp_a=e, ld=s * Cout, bstride=n, lda=Cin, cin=Cin, ntaps=2, row_off=-1,
                 row_lo=0, row_hi=T, batch=B, a_bstride=T * Cin, bias=b.cuda(), bias_mod=Cout, out_off=-3 * Cout, out_len=n,
                 tag=f"convtranspose clip Cin={Cin}")


@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_gemm_rowmask_and_residual_batched(env, cfg):
    """Row mask and residual together, batch 2, with batch strides that are not the dense ones."""
    for M, N in SHAPES[cfg[0]]:
        for K in KS:
            g = torch.Generator().manual_seed(M + K)
            B, rbs, mbs = 2, M * N + 8, M + 3
            x, w, b = rnd(g, B, M, K), rnd(g, N, K, scale=K ** -0.5), rnd(g, N)
            res, mask = rnd(g, B, rbs), (torch.rand(B, mbs, generator=g) > 0.3).float()
            alpha = 1 + 0.1 * rnd(g, N)
            xa, wp, xr, wr = operands(env, cfg[1], x, w)
            f = (F.leaky_relu(xr @ wr.t() + b.double(), 0.1) + res[:, :M * N].reshape(B, M, N).double()) * mask[:, :M, None].double()
            a = snake64(f, alpha)
            run_gemm(env, cfg, xa, wp, M, N, exp_f=place(f, N, M * N), exp_a=place(a, N, M * N), ld=N, bstride=M * N, lda=K, cin=K,
                     batch=B, a_bstride=M * K, bias=b.cuda(), act="lrelu", slope=0.1, residual=res.cuda(), ldr=N, r_bstride=rbs,
                     rowmask=mask.cuda(), rm_bstride=mbs, alpha=alpha.cuda(), tag=f"mask+residual {M}x{N}x{K}")


def test_gemm_weight_planes_refuse_the_128_row_tiles(env):
    """MMX_X2W / MMX_X3W exist for the 64x64 and 32x64 tiles only: the other two are an argument error, not another kernel."""
    L, ops = env
    x = torch.randn(150, 96).cuda()
    out = torch.zeros(150, 136, device="cuda")
    for pdt in (X2W, X3W):
        wp = ops.pack_linear(torch.randn(136, 96).cuda(), pdt)
        for tile in ("128x128", "128x64"):
            with pytest.raises(L.MmxError, match="code -1"):
                ops.gemm(x, wp, 150, 136, dtype=BASE[pdt], lda=96, cin=96, out_f32=out, ldo_f=136, tile=L.TILES[tile])
    with pytest.raises(L.MmxError):                                 # and a plane dtype code without planes is refused up front
        ops.gemm(x, torch.zeros(136, 96, device="cuda", dtype=torch.bfloat16), 150, 136, dtype=X2W, lda=96, cin=96, out_f32=out, ldo_f=136)


# ================================================================================================ activations on a deliberate grid
def act_grid():
    """Crosses mish's softplus threshold (20), the erf clamp of the fused kernels (3 * sqrt(2)) and the exp overflow range."""
    sp = [0.0, -0.0, 1e-6, -1e-6, 19.999, -19.999, 20.0, 20.001, 50.0, -50.0, 88.0, -88.0, 100.0, -100.0]
    return torch.cat([torch.linspace(-30, 30, 4001), torch.tensor(sp)])


ACT_CODES = ["none", "lrelu", "gelu", "silu", "mish", "tanh"]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("act", ACT_CODES)
@pytest.mark.parametrize("dt", [0, 1])
def test_act_rows_grid(env, dt, act, masked):
    """mmx_act_rows per element: |got - ref| <= tol * (1 + |ref|), tol 1e-5 for fp32 results and 1e-2 for the bf16 copy."""
    L, ops = env
    x = act_grid()
    C_ = 41
    rows = x.numel() // C_ + 1                                     # 4015 grid values, zero padded to 98 ragged rows of 41
    x = torch.cat([x, torch.zeros(rows * C_ - x.numel())])
    mask = (torch.rand(rows, generator=torch.Generator().manual_seed(1)) > 0.3).float() if masked else None
    ref = act64(x.double(), act).reshape(rows, C_) * (mask.double()[:, None] if masked else 1.0)
    bf, vf = guarded(rows * C_, torch.float32)
    ba, va = guarded(rows * C_, tdt(dt))
    ops.act_rows(x.cuda(), rows=rows, C_=C_, act=act, rowmask=(mask.cuda() if masked else None), out_f32=vf, out_act=va, dtype=dt)
    torch.cuda.synchronize()
    assert_guards(bf, rows * C_, "out_f32")
    assert_guards(ba, rows * C_, "out_act")
    for got, tol in ((vf, 1e-5), (va, 1e-2 if dt else 1e-5)):
        got = got.cpu().double().reshape(rows, C_)
        assert bool(torch.isfinite(got).all())
        d = (got - ref).abs() - tol * (1 + ref.abs())
        i = int(d.argmax())
        assert float(d.max()) <= 0, (act, float(x[i]), float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]))


@pytest.mark.parametrize("dt", [0, 1])
def test_rownorm_mish_wide_range(env, dt):
    """mmx_rownorm's compile-time mish with gains of 10: normalised values beyond +-30 cross the softplus threshold.  Per
    element as test_act_rows_grid (rows of zero mean, so that the fp32 mean costs nothing next to the bound)."""
    L, ops = env
    C_, rows = 256, 37
    g = torch.Generator().manual_seed(2)
    x = rnd(g, rows, C_)
    gamma, beta = torch.full((C_,), 10.0), rnd(g, C_, scale=0.1)
    ref = F.mish(F.layer_norm(x.double(), (C_,), gamma.double(), beta.double(), 1e-5))
    assert float(ref.max()) > 25
    bf, vf = guarded(rows * C_, torch.float32)
    ba, va = guarded(rows * C_, tdt(dt))
    ops.rownorm(x.cuda(), gamma.cuda(), beta.cuda(), 1e-5, rows=rows, C_=C_, act="mish", out_f32=vf, out_act=va, dtype=dt)
    torch.cuda.synchronize()
    assert_guards(bf, rows * C_)
    assert_guards(ba, rows * C_)
    for got, tol in ((vf, 1e-5), (va, 1e-2 if dt else 1e-5)):
        got = got.cpu().double().reshape(rows, C_)
        assert bool(torch.isfinite(got).all()) and float(((got - ref).abs() - tol * (1 + ref.abs())).max()) <= 0


@pytest.mark.parametrize("act", ACT_CODES)
@pytest.mark.parametrize("dt", [0, 1, 2, 3])
def test_gemm_epilogue_activations_grid(env, dt, act):
    """The same grid through the GEMM epilogue's compile-time activations: an identity weight (K = N = 64)."""
    L, ops = env
    x = act_grid()
    x = torch.cat([x, torch.zeros(64 * 64 - x.numel())]).reshape(64, 64)
    xa, wp, xr, wr = operands(env, dt, x, torch.eye(64))
    ref = act64(xr @ wr.t(), act)
    bf, vf = guarded(64 * 64, torch.float32)
    ba, va = guarded(64 * 64, tdt(dt))
    ops.linear(xa, wp, 64, dtype=dt, act=act, out_f32=vf.view(64, 64), out_act=va.view(64, 64))
    torch.cuda.synchronize()
    assert_guards(bf, 64 * 64)
    assert_guards(ba, 64 * 64)
    assert bool(torch.isfinite(vf).all()) and bool(torch.isfinite(va.float()).all())
    assert rel_err(vf.cpu().reshape(64, 64), ref) < tol_f(dt)
    assert rel_err(va.cpu().reshape(64, 64), ref) < tol_a(dt)


# ================================================================================================ B. elementwise and glue kernels
def _copy2d_case(ops, sdt, ddt, B, rows, cols, rep, ibs, irs, ics, obs, ors, ocs, g):
    tin = (rows + rep - 1) // rep
    n_in = (B - 1) * ibs + (tin - 1) * irs + (cols - 1) * ics + 1
    n_out = (B - 1) * obs + (rows - 1) * ors + (cols - 1) * ocs + 1
    src = torch.randn(n_in, generator=g).to(tdt(sdt))
    buf, view = guarded(n_out, tdt(ddt))
    ops.copy2d(src.cuda(), sdt, ibs, irs, ics, view, ddt, obs, ors, ocs, rows=rows, cols=cols, batch=B, rep=rep)
    torch.cuda.synchronize()
    b, r, c = torch.meshgrid(torch.arange(B), torch.arange(rows), torch.arange(cols), indexing="ij")
    o = (b * obs + r * ors + c * ocs).reshape(-1)
    exp = src[(b * ibs + (r // rep) * irs + c * ics).reshape(-1)].to(tdt(ddt))
    got = buf.cpu()
    keep = torch.ones(got.numel(), dtype=torch.bool)
    keep[GUARD + o] = False
    assert bool(is_sentinel(got[keep]).all()), "copy2d wrote outside rows x cols"
    assert torch.equal(got[GUARD + o], exp), "copy2d is not bit-exact"


@pytest.mark.parametrize("rows,cols", [(37, 80), (33, 65), (1, 100)])
@pytest.mark.parametrize("sdt,ddt", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_copy2d(env, sdt, ddt, rows, cols):
    """[B, C, T] -> [B, T, C], back, and row copies; padded strides on both sides, batch 2; rep = nearest-neighbour upsampling
    (rows = rep * Tin).  Bit-exact against tensor.to(dtype)."""
    L, ops = env
    g = torch.Generator().manual_seed(rows + cols)
    B = 2
    for rep in (1, 2, 3):
        R = rows * rep
        tin = rows
        # channels-first in (column stride = padded T), time-major out
        _copy2d_case(ops, sdt, ddt, B, R, cols, rep, cols * (tin + 5) + 3, 1, tin + 5, R * (cols + 3) + 7, cols + 3, 1, g)
        # time-major in, channels-first out
        _copy2d_case(ops, sdt, ddt, B, R, cols, rep, tin * (cols + 2) + 1, cols + 2, 1, cols * (R + 4) + 5, 1, R + 4, g)
        # no transpose
        _copy2d_case(ops, sdt, ddt, B, R, cols, rep, tin * (cols + 1) + 9, cols + 1, 1, R * (cols + 6) + 2, cols + 6, 1, g)


@pytest.mark.parametrize("C_", [80, 896, 100])
@pytest.mark.parametrize("dt", [0, 1])
def test_gather_rows(env, dt, C_):
    L, ops = env
    g = torch.Generator().manual_seed(C_)
    V = 50
    ids = torch.tensor([0, V - 1, 7, 7, -1, 3, V - 1, -1, 12, 0, 31], dtype=torch.int64)
    n = ids.numel()
    table = rnd(g, V, C_)
    mask = torch.tensor([1, 1, 0, 1, 1, 0, 1, 1, 1, 0, 1], dtype=torch.float32)
    scale = math.sqrt(C_)
    for ld, rm in ((C_, None), (C_ + 5, mask)):
        m = torch.tensor(scale, dtype=torch.float32) * (rm if rm is not None else torch.ones(n))     # the kernel's one fp32 factor
        ref = table[ids.clamp(min=0)] * m[:, None]                                               # one fp32 product: exact
        bf, vf = guarded(n * ld, torch.float32)
        ba, va = guarded(n * ld, tdt(dt))
        ops.gather_rows(ids.cuda(), table.cuda(), scale=scale, rowmask=(rm.cuda() if rm is not None else None), out_f32=vf,
                        out_act=va, dtype=dt, ldo_f=ld, ldo_a=ld)
        torch.cuda.synchronize()
        for buf, want in ((bf, ref), (ba, ref.to(tdt(dt)))):
            assert_guards(buf, n * ld)
            got = buf.cpu()[GUARD:GUARD + n * ld].reshape(n, ld)
            assert torch.equal(got[:, :C_], want) and bool(is_sentinel(got[:, C_:]).all())


@pytest.mark.parametrize("C_", [8, 48, 96])
@pytest.mark.parametrize("dt", [0, 1])
def test_mask_rows(env, dt, C_):
    """In place: masked rows exactly zero, all others bit-identical; the last 256-thread block is partly empty."""
    L, ops = env
    rows = 333
    assert (rows * C_ // (8 if dt else 4)) % 256 != 0
    g = torch.Generator().manual_seed(C_)
    x = rnd(g, rows, C_).to(tdt(dt))
    mask = (torch.rand(rows, generator=g) > 0.4).float()
    mask[-1] = 0
    buf, view = guarded(rows * C_, tdt(dt))
    view.copy_(x.reshape(-1))
    ops.mask_rows(view, mask.cuda(), rows=rows, C_=C_, dtype=dt)
    torch.cuda.synchronize()
    assert_guards(buf, rows * C_)
    got = view.cpu().reshape(rows, C_)
    assert torch.equal(got[mask != 0], x[mask != 0])
    assert bool((got[mask == 0] == 0).all()) and int((mask == 0).sum()) > 50


@pytest.mark.parametrize("ldh", [320, 512])
@pytest.mark.parametrize("T", [1, 37])
@pytest.mark.parametrize("dt", [0, 1])
def test_est_pack(env, dt, T, ldh):
    """h[b][t] = [x[b % x_mod] | mu | spks | cond]; NULL parts read as zero; columns 320 .. ldh - 1 are not written."""
    L, ops = env
    B = 4
    g = torch.Generator().manual_seed(T + ldh)
    mu, spks, cond = rnd(g, B, T, 80), rnd(g, B, 80), rnd(g, B, T, 80)
    for x_mod in (2, B):
        x = rnd(g, x_mod, T, 80)
        for null in (None, "mu", "spks", "cond"):
            parts = dict(mu=mu, spks=spks, cond=cond)
            if null:
                parts[null] = None
            dev = {k: (v.cuda() if v is not None else None) for k, v in parts.items()}
            buf, view = guarded(B * T * ldh, tdt(dt))
            ops.est_pack(x.cuda(), dev["mu"], dev["spks"], dev["cond"], view.view(B, T, ldh), B=B, T=T, dtype=dt, x_mod=x_mod)
            torch.cuda.synchronize()
            z = torch.zeros(B, T, 80)
            ref = torch.cat([x[torch.arange(B) % x_mod], z if parts["mu"] is None else mu,
                             z if parts["spks"] is None else spks[:, None, :].expand(B, T, 80), z if parts["cond"] is None else cond], -1)
            assert_guards(buf, B * T * ldh)
            got = view.cpu().reshape(B, T, ldh)
            assert torch.equal(got[..., :320], ref.to(tdt(dt))), (x_mod, null)
            assert bool(is_sentinel(got[..., 320:]).all())


@pytest.mark.parametrize("dim", [320, 256, 6])
@pytest.mark.parametrize("dt", [0, 1])
def test_sinusoidal_emb(env, dt, dim):
    """The bound comes from the reference: the distance of the fp32 torch statement (oracle.flow.sinusoidal_pos_emb on the CPU)
    from the float64 evaluation on the same t, times 4 - the argument 1000 * t * freq is rounded to fp32 (ulp 6e-5 at 1000) in
    both, anything tighter would test rounding order.  bf16: half an ulp of the stored value on top (<= 2^-8 relative)."""
    from oracle import flow as OF
    L, ops = env
    g = torch.Generator().manual_seed(dim)
    t = torch.cat([torch.tensor([0.0, 1e-3, 0.25, 0.5, 1.0]), torch.rand(11, generator=g)])
    half = dim // 2
    fr = torch.exp(torch.arange(half, dtype=torch.float64) * -(math.log(10000) / (half - 1)))
    e = 1000.0 * t.double()[:, None] * fr[None, :]
    ref = torch.cat([e.sin(), e.cos()], -1)
    d_ref = float((OF.sinusoidal_pos_emb(t, dim).double() - ref).abs().max())
    buf, view = guarded(t.numel() * dim, tdt(dt))
    ops.sinusoidal_emb(t.cuda(), view, dim=dim, dtype=dt)
    torch.cuda.synchronize()
    assert_guards(buf, t.numel() * dim)
    got = view.cpu().double().reshape(t.numel(), dim)
    d = (got - ref).abs()
    print(f"sinusoidal_emb dim={dim} dtype={dt}: fp32 torch statement vs float64 {d_ref:.3e}, kernel vs float64 {float(d.max()):.3e}")
    assert d_ref > 0
    bound = 4 * d_ref + ((ref.abs() + 4 * d_ref) * 2.0 ** -8 if dt else 0.0)
    assert bool((d <= bound).all()), float(d.max())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 80 * 37 * 2])
def test_cfg_euler(env, n):
    import numpy as np
    L, ops = env
    g = torch.Generator().manual_seed(n)
    for cfg, dt_ in ((0.7, 0.1), (0.0, 0.1)):
        x, dc, du = rnd(g, n), rnd(g, n), rnd(g, n)
        c, h = float(np.float32(cfg)), float(np.float32(dt_))          # the scalars as the entry point receives them
        ref = x.double() + h * ((1.0 + c) * dc.double() - c * du.double())
        buf, view = guarded(n, torch.float32)
        view.copy_(x)
        ops.cfg_euler(view, dc.cuda(), du.cuda(), cfg, dt_, n)
        torch.cuda.synchronize()
        assert_guards(buf, n)
        assert rel_err(view.cpu(), ref) < 1e-6


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("act", ["none", "mish"])
@pytest.mark.parametrize("B,T,C_,groups", [(2, 37, 512, 32), (1, 300, 256, 8), (3, 5, 64, 64), (2, 1, 80, 1)])
@pytest.mark.parametrize("dt", [0, 1])
def test_groupnorm(env, dt, B, T, C_, groups, act, masked):
    """16 channels per group, 1 channel per group, one group, fewer than 256 elements per group; mean offset +3 (a one-pass
    variance would lose it).  Against F.group_norm in float64."""
    L, ops = env
    g = torch.Generator().manual_seed(T + C_)
    x = rnd(g, B, T, C_) + 3
    gamma, beta = 1 + 0.1 * rnd(g, C_), 0.1 * rnd(g, C_)
    mask = (torch.rand(B, T, generator=g) > 0.3).float() if masked else None
    ref = F.group_norm(x.double().transpose(1, 2), groups, gamma.double(), beta.double(), 1e-5).transpose(1, 2)
    ref = act64(ref, act) * (mask.double()[..., None] if masked else 1.0)
    buf, view = guarded(B * T * C_, tdt(dt))
    ops.groupnorm(x.cuda(), gamma.cuda(), beta.cuda(), view, B=B, T=T, C_=C_, groups=groups, dtype=dt, act=act,
                  rowmask=(mask.cuda() if masked else None))
    torch.cuda.synchronize()
    assert_guards(buf, B * T * C_)
    got = view.cpu().reshape(B, T, C_)
    assert bool(torch.isfinite(got.float()).all())
    assert rel_err(got, ref) < (1e-2 if dt else 1e-5)


@pytest.mark.parametrize("I", [4864, 100])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("dt", [0, 1])
def test_swiglu(env, dt, rows, I):
    """silu(gate) * up with inputs of scale 8 (the sigmoid saturates on both sides), row pitches above 2I and I.  Per element:
    |got - ref| <= tol * (1 + |ref|) with the suite's fp32 elementwise bound 1e-5, 1e-2 for bf16 (2^-9 rounding)."""
    L, ops = env
    g = torch.Generator().manual_seed(rows + I)
    ldgu, ldo = 2 * I + 12, I + 7
    gu = torch.full((rows, ldgu), float("nan"))
    gu[:, :2 * I] = rnd(g, rows, 2 * I, scale=8.0)
    ref = F.silu(gu[:, :I].double()) * gu[:, I:2 * I].double()
    buf, view = guarded(rows * ldo, tdt(dt))
    ops.swiglu(gu.cuda(), view, rows=rows, I=I, dtype=dt, ldgu=ldgu, ldo=ldo)
    torch.cuda.synchronize()
    assert_guards(buf, rows * ldo)
    got = view.cpu().reshape(rows, ldo)
    assert bool(is_sentinel(got[:, I:]).all())
    tol = 1e-2 if dt else 1e-5
    assert float(((got[:, :I].double() - ref).abs() - tol * (1 + ref.abs())).max()) <= 0


@pytest.mark.parametrize("D", [80, 128])
def test_vae_sample(env, D):
    L, ops = env
    rows = 37
    g = torch.Generator().manual_seed(D)
    ml = rnd(g, rows, 2 * D)
    ml[:, D:] = torch.linspace(-20, 20, rows * D)[torch.randperm(rows * D, generator=g)].reshape(rows, D)
    noise = rnd(g, rows, D)
    lg = ml[:, D:].clamp(-14, 14)
    assert int((ml[:, D:] < -14).sum()) > 0 and int((ml[:, D:] > 14).sum()) > 0
    ref = ml[:, :D].double() + noise.double() * lg.double().exp()
    bufs = [guarded(rows * D, torch.float32) for _ in range(3)]
    ops.vae_sample(ml.cuda(), noise.cuda(), bufs[0][1], bufs[1][1], bufs[2][1], rows=rows, D=D)
    torch.cuda.synchronize()
    for b, _ in bufs:
        assert_guards(b, rows * D)
    z, m, logs = (v.cpu().reshape(rows, D) for _, v in bufs)
    assert torch.equal(m, ml[:, :D]) and torch.equal(logs, lg)
    assert rel_err(z, ref) < 1e-6


@pytest.mark.parametrize("snake", [False, True])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("C_", [8, 96])
@pytest.mark.parametrize("dt", [0, 1])
def test_conv_cin1(env, dt, C_, T, snake):
    """Conv1d(1 -> C, 7) + LeakyReLU (+ Snake into out_act) against F.conv1d in float64; the Snake argument reaches ~30."""
    L, ops = env
    B, k, slope = 2, 7, 0.1
    g = torch.Generator().manual_seed(C_ + T)
    x, w, b = rnd(g, B, T, scale=1.3), rnd(g, C_, k), rnd(g, C_)
    alpha = (0.5 + 1.5 * torch.rand(C_, generator=g)) if snake else None
    f = F.leaky_relu(F.conv1d(x.double()[:, None, :], w.double()[:, None, :], b.double(), padding=3), slope).transpose(1, 2)
    a = snake64(f, alpha) if snake else f
    bf, vf = guarded(B * T * C_, torch.float32)
    ba, va = guarded(B * T * C_, tdt(dt))
    ops.conv_cin1(x.cuda(), w.cuda(), b.cuda(), T=T, C_=C_, k=k, batch=B, dtype=dt, slope=slope,
                  alpha=(alpha.cuda() if snake else None), out_f32=vf, out_act=va)
    torch.cuda.synchronize()
    assert_guards(bf, B * T * C_)
    assert_guards(ba, B * T * C_)
    assert bool(torch.isfinite(vf).all()) and bool(torch.isfinite(va.float()).all())
    assert rel_err(vf.cpu().reshape(B, T, C_), f) < 2e-5
    assert rel_err(va.cpu().reshape(B, T, C_), a) < (1e-2 if dt else 2e-5)


def _conv_cout1(ops, dt, C_, T, use_tanh, seed):
    B, k, slope = 2, 7, 0.1
    g = torch.Generator().manual_seed(seed)
    x = rnd(g, B, T, C_).to(tdt(dt))
    w, b = rnd(g, k, C_, scale=1.0 / math.sqrt(k * C_)), rnd(g, 1, scale=0.1)             # pre-activation of unit variance
    acc = F.leaky_relu(F.conv1d(x.double().transpose(1, 2), w.double().t()[None], b.double(), padding=3), slope)[:, 0]
    ref = torch.tanh(acc) if use_tanh else acc.clamp(-1, 1)
    buf, view = guarded(B * T, torch.float32)
    ops.conv_cout1_tanh(x.cuda(), w.cuda(), b.cuda(), view, T=T, C_=C_, k=k, batch=B, dtype=dt, slope=slope, use_tanh=use_tanh)
    torch.cuda.synchronize()
    assert_guards(buf, B * T)
    return view.cpu().reshape(B, T), ref, acc


@pytest.mark.parametrize("use_tanh", [True, False])
@pytest.mark.parametrize("T", [1, 255, 256, 257, 700])
@pytest.mark.parametrize("dt", [0, 1])
def test_conv_cout1_tanh(env, dt, T, use_tanh):
    """The DAC tail Conv1d(48 -> 1, 7) + LeakyReLU + tanh / clamp.  The output is fp32 from fp32 sums of 336 exact products of
    O(1) partial sums: the suite's fp32 GEMM bound, 2e-5 of max |ref| <= 1."""
    L, ops = env
    got, ref, acc = _conv_cout1(ops, dt, 48, T, use_tanh, T)
    if T > 1:
        assert float(acc.max()) > 1.0                                 # the clamp branch is taken
    assert bool(torch.isfinite(got).all()) and rel_err(got, ref) < 2e-5


def test_conv_cout1_tanh_above_64k_lds(env):
    """fp32, C = 96, k = 7: 103 KB of dynamic LDS - inside the 160 KB the argument check admits, and the launch opts in."""
    L, ops = env
    got, ref, _ = _conv_cout1(ops, 0, 96, 300, True, 5)
    assert bool(torch.isfinite(got).all()) and rel_err(got, ref) < 2e-5


# ================================================================================================ C. mmx_attn_dense options
def attn64(q, k, v, H, scale, keymask=None, chunk=0):
    """q [B, Tq, H*64], k / v [B, Tk, H*64] float64 -> [B, Tq, H*64]; rows without a visible key are zero."""
    B, Tq, Tk, D = q.shape[0], q.shape[1], k.shape[1], 64
    qh, kh, vh = (t.reshape(B, -1, H, D).transpose(1, 2) for t in (q, k, v))
    s = (qh @ kh.transpose(-2, -1)) * scale
    vis = torch.ones(B, Tq, Tk, dtype=torch.bool)
    if keymask is not None:
        vis &= keymask.bool()[:, None, :]
    if chunk:
        i, j = torch.arange(Tq)[:, None], torch.arange(Tk)[None, :]
        vis &= (j < (i // chunk + 1) * chunk)[None]
    s = s.masked_fill(~vis[:, None], float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(vis[:, None].any(-1, keepdim=True), p, torch.zeros_like(p))
    return (p @ vh).transpose(1, 2).reshape(B, Tq, H * D)


def _attn(ops, dt, q, k, v, *, B, H, Tq, Tk, ldq, ldk, ldv, q_bs, k_bs, v_bs, **kw):
    ldo = H * 64 + 8                                                   # 8 slack columns per output row
    buf, view = guarded(B * Tq * ldo, tdt(dt))
    ops.attn_dense(q, k, v, view, B=B, H=H, Tq=Tq, Tk=Tk, ldq=ldq, ldk=ldk, ldv=ldv, ldo=ldo, q_bs=q_bs, k_bs=k_bs, v_bs=v_bs,
                   o_bs=Tq * ldo, scale=0.125, dtype=dt, **kw)
    torch.cuda.synchronize()
    assert_guards(buf, B * Tq * ldo)
    got = view.cpu().reshape(B, Tq, ldo)
    assert bool(is_sentinel(got[..., H * 64:]).all())
    return got[..., :H * 64]


ATOL = {0: 2e-5, 1: 2e-2}


@pytest.mark.parametrize("dt", [0, 1])
def test_attn_dense_head_stride(env, dt):
    """q / k / v interleaved per head in one [B][T][H * 3 * 64] buffer (the speaker encoder's QKVAttentionLegacy layout)."""
    L, ops = env
    B, H, T, D = 2, 4, 50, 64
    g = torch.Generator().manual_seed(4)
    qkv = rnd(g, B, T, H, 3, D).to(tdt(dt))
    dev = qkv.reshape(B, T, H * 3 * D).cuda()
    ld = H * 3 * D
    got = _attn(ops, dt, dev, dev[:, :, D:], dev[:, :, 2 * D:], B=B, H=H, Tq=T, Tk=T, ldq=ld, ldk=ld, ldv=ld, q_bs=T * ld, k_bs=T * ld,
                v_bs=T * ld, head_stride=3 * D)
    q, k, v = (qkv[:, :, :, i].reshape(B, T, H * D).contiguous() for i in range(3))
    ref = attn64(q.double(), k.double(), v.double(), H, 0.125)
    assert rel_err(got, ref) < ATOL[dt]
    sep = _attn(ops, dt, q.cuda(), k.cuda(), v.cuda(), B=B, H=H, Tq=T, Tk=T, ldq=H * D, ldk=H * D, ldv=H * D, q_bs=T * H * D,
                k_bs=T * H * D, v_bs=T * H * D)
    assert torch.equal(got, sep)                                       # the same arithmetic on the same values


@pytest.mark.parametrize("chunk", [0, 25])
@pytest.mark.parametrize("q_begin", [16, 48])
@pytest.mark.parametrize("dt", [0, 1])
def test_attn_dense_q_begin(env, dt, q_begin, chunk):
    """Only queries q_begin .. T - 1 are computed (over all keys): the rows before keep their sentinel, the others equal the
    full computation."""
    L, ops = env
    B, H, T, D = 2, 4, 77, 64
    g = torch.Generator().manual_seed(q_begin + chunk)
    q, k, v = (rnd(g, B, T, H * D).to(tdt(dt)) for _ in range(3))
    km = torch.ones(B, T)
    km[1, T - 9:] = 0
    ref = attn64(q.double(), k.double(), v.double(), H, 0.125, km, chunk)
    kw = dict(B=B, H=H, Tq=T, Tk=T, ldq=H * D, ldk=H * D, ldv=H * D, q_bs=T * H * D, k_bs=T * H * D, v_bs=T * H * D, keymask=km.cuda(),
              chunk=chunk)
    got = _attn(ops, dt, q.cuda(), k.cuda(), v.cuda(), q_begin=q_begin, **kw)
    assert bool(is_sentinel(got[:, :q_begin]).all())
    assert rel_err(got[:, q_begin:], ref[:, q_begin:]) < ATOL[dt]
    full = _attn(ops, dt, q.cuda(), k.cuda(), v.cuda(), **kw)
    assert torch.equal(got[:, q_begin:], full[:, q_begin:]) and rel_err(full, ref) < ATOL[dt]


@pytest.mark.parametrize("dt", [0, 1])
def test_attn_dense_cross_lengths_and_fully_masked_row(env, dt):
    """Tq = 20 queries over Tk = 77 keys with a key mask; a batch row whose keys are all masked outputs exact zeros."""
    L, ops = env
    B, H, Tq, Tk, D = 3, 4, 20, 77, 64
    g = torch.Generator().manual_seed(9)
    q = rnd(g, B, Tq, H * D).to(tdt(dt))
    k, v = (rnd(g, B, Tk, H * D).to(tdt(dt)) for _ in range(2))
    km = (torch.rand(B, Tk, generator=g) > 0.3).float()
    km[1] = 0
    got = _attn(ops, dt, q.cuda(), k.cuda(), v.cuda(), B=B, H=H, Tq=Tq, Tk=Tk, ldq=H * D, ldk=H * D, ldv=H * D, q_bs=Tq * H * D,
                k_bs=Tk * H * D, v_bs=Tk * H * D, keymask=km.cuda())
    ref = attn64(q.double(), k.double(), v.double(), H, 0.125, km)
    assert bool((got[1] == 0).all()) and float(ref[1].abs().max()) == 0.0
    assert rel_err(got, ref) < ATOL[dt]
