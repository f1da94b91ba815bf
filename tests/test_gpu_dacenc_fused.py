"""mmx_dac_ru at the encoder's widths, C = 64 and 128 (csrc/fused.hip: 4 n-fragments per wave, 16 columns per lane in the
epilogues), in the bf16 and split builds, dilation 1 / 3 / 9, every tile height that has an instantiation - with the method of
tests/test_gpu_fused_parity.py, imported from there and not restated: the float64 reference ru_ref (ru_chain with snake64), the
rounding MODEL whose worst row is a case's base, bound = max(4 * base, floor), the per-row metric in which a row whose reference is
exactly zero must be exactly zero, inputs with NaN in everything the kernel must not read and outputs in guarded buffers whose bits
outside the written window must not change.

Shapes: B = 3, T = 2 bm + 5 (two whole tiles and a 5-row one), two launches per (tile, dilation) whose lens put a member's end
  A  mid-tile (bm + bm / 2), exactly on a tile edge (bm), at 0;
  B  at T (5 rows into the last tile), inside the halo behind a tile edge (bm + 2 dil <= bm + 3 dil), on the second edge (2 bm).
One launch per tile (dilation 9, lens B) runs again with x_out = NULL: act_out must keep its bits and the x_out buffer all of its.

The CPU tests (not marked gpu) hold ru_ref at these widths to oracle.dac.residual_unit at 1e-12 (that file's own statement, called
with C = 64 / 128) and every case's bound under the dac_ru caps of that file (4e-2 bf16, 2e-4 split)."""
import pytest
import torch

import test_gpu_fused_parity as P
from test_gpu_fused_parity import CODE, DT_NAME, X2, X2W, Out, assert_rows, bits, env, poisoned, ru_case, ru_pack, strided, tdt  # noqa: F401

gpu = pytest.mark.gpu

# the instantiations of DAC_RU_FORMS for C = 64 / 128 and the defaults of dac_ru_select (static_asserts in csrc/fused.hip)
ENC_BMS = {1: {64: [64, 128, 256], 128: [64, 128]}, X2: {64: [64, 128], 128: [32, 64]}}
ENC_DEFAULT = {1: {64: 128, 128: 128}, X2: {64: 64, 128: 64}}
DILS = (1, 3, 9)
ENC_TILES = [(dt, C, bm) for dt in (1, X2) for C in (64, 128) for bm in ENC_BMS[dt][C]]

# FIGURES   worst case of the group: base -> bound = max(4 * base, floor) | the kernel's worst row, every tile, dilation and output
#   dac_ru C 64 / 128   bf16  8.2e-3 -> 3.3e-2 | 8.2e-3    x2  1.0e-5 -> 4.1e-5 | 1.0e-5
# (as in the parity file: every case is held to the bound of its own base, at most the group's; the bases are the CPU statement's,
#  the worst rows those of the nine tiles on an MI355X)


def enc_T(bm):
    return 2 * bm + 5


def enc_lens(bm, dil):
    T = enc_T(bm)
    return (bm + bm // 2, bm, 0), (T, bm + 2 * dil, 2 * bm)


def enc_cases(dt, C, bm):
    for dil in DILS:
        for lens in enc_lens(bm, dil):
            yield ru_case(dt, C, dil, enc_T(bm), lens)


def run_enc(env, c, bm, what, with_x=True):
    """One mmx_dac_ru launch with act_out, as run_ru of the parity file (NaN in rows >= lens[b] and in the 8-element gap behind
    every member, guarded outputs); with_x=False passes x_out = NULL, and the x_out buffer must keep every bit."""
    L, ops = env
    dt, C, dil, T, lens, x = c["dt"], c["C"], c["dil"], c["T"], c["lens"], c["x"]
    B = x.shape[0]
    ru = ru_pack(env, dt, C, dil)
    bs = T * C + 8

    def fill(t):
        for b in range(B):
            t[b * bs:b * bs + lens[b] * C].view(lens[b], C).copy_(x[b, :lens[b]])
    xd = poisoned((B * bs,), torch.float32, fill)
    xo, ao = Out(B * bs, torch.float32), Out(B * bs, tdt(dt))
    xo.snap()
    ao.snap()
    ops.dac_ru(xd, (xo.view if with_x else None), ru, B=B, T=T, C_=C, dil=dil, dtype=CODE[dt], act_out=ao.view, alpha_next=ru["an"],
               lens=torch.tensor(lens, dtype=torch.int32).cuda(), bm=bm, x_bs=bs)
    torch.cuda.synchronize()
    win = [(B, bs, C, 0, 0, T, 0, C)]
    xb = xo.check(win if with_x else [], what + " x_out")
    ab = ao.check(win, what + " act_out")
    return dict(x=strided(xb, B, bs, T, C, C), act=strided(ab, B, bs, T, C, C).float()), ab


@gpu
@pytest.mark.parametrize("dt,C,bm", ENC_TILES, ids=[f"{DT_NAME[d]}-{C}-{bm}" for d, C, bm in ENC_TILES])
def test_dac_ru_encoder_rows(env, dt, C, bm):
    grp = ("dac_ru enc", DT_NAME[dt])
    for c in enc_cases(dt, C, bm):
        tag = c["key"] + f" bm {bm}"
        print(f"{tag}: base {c['base']:.3e} -> bound {c['bound']:.3e}")
        assert c["bound"] <= c["cap"], f"{tag}: the model's bound is above the suite's {c['cap']:.1e}"
        out, ab = run_enc(env, c, bm, tag)
        for k, r in c["ref"].items():
            w = assert_rows(out[k], r, c["bound"], f"{tag} {k}", grp)
            print(f"    {k}: worst row {w:.3e}")
        if c["dil"] == 9 and c["lens"][0] == c["T"]:
            out2, ab2 = run_enc(env, c, bm, tag + " x_out NULL", with_x=False)
            assert torch.equal(bits(ab), bits(ab2)), f"{tag}: act_out differs without x_out"
    # the default request (bm = 0) launches the default tile: the same bits
    if bm == ENC_DEFAULT[dt][C]:
        c = ru_case(dt, C, 3, enc_T(bm), enc_lens(bm, 3)[1])
        _, a0 = run_enc(env, c, 0, c["key"] + " bm 0")
        _, a1 = run_enc(env, c, bm, c["key"] + f" bm {bm}")
        assert torch.equal(bits(a0), bits(a1))
    print(f"dac_ru {DT_NAME[dt]} C {C} bm {bm}: worst row so far {P.WORST[grp]:.3e}")


@gpu
def test_dac_ru_encoder_refusals(env):
    """No weight-plane forms at C = 64 / 128, no other tile heights, and neither output: the argument error, nothing written."""
    L, ops = env
    for C in (64, 128):
        for dt in (1, X2):
            for bm in sorted({16, 32, 64, 128, 256, 512} - set(ENC_BMS[dt][C])):
                with pytest.raises(L.MmxError, match="argument"):
                    run_enc(env, ru_case(dt, C, 1, 37, (37, 5, 0)), bm, f"C {C} bm {bm}")
        ru = ru_pack(env, 1, C, 1)
        x = torch.zeros(1, 37, C, device="cuda")
        with pytest.raises(L.MmxError, match="argument"):
            ops.dac_ru(x, None, ru, B=1, T=37, C_=C, dil=1, dtype=1)
        with pytest.raises(L.MmxError, match="argument"):
            P.run_ru(env, ru_case(X2W, C, 1, 37, None), 0, True, f"x2w C {C}")


# ================================================================================================ on the CPU
@pytest.mark.parametrize("C,dil", [(64, 1), (64, 9), (128, 3)])
def test_ru_ref_matches_the_oracle_at_the_encoder_widths(C, dil):
    """ru_ref (the float64 statement every case above is judged against) = oracle.dac.residual_unit at 1e-12 per row, with and
    without lens: the parity file's own check, run at C = 64 / 128."""
    P.test_ru_ref_matches_the_oracle(C, dil)


def test_encoder_model_bounds_fit_the_caps():
    """Every case of this file: base > 0 and max(4 * base, floor) under the dac_ru caps of the parity file."""
    worst = {}
    for dt, C, bm in ENC_TILES:
        for c in enc_cases(dt, C, bm):
            assert c["cap"] == P.CAP_RU[dt]
            assert c["base"] > 0 and c["bound"] <= c["cap"], f"{c['key']}: base {c['base']:.3e} -> bound {c['bound']:.3e} above the cap {c['cap']:.1e}"
            worst[DT_NAME[dt]] = max(worst.get(DT_NAME[dt], 0.0), c["base"])
    for k, b in worst.items():
        print(f"dac_ru C 64 / 128 {k}: base {b:.3e} -> bound {max(4 * b, P.FLOOR[{'bf16': 1, 'x2': X2}[k]]):.3e}")
