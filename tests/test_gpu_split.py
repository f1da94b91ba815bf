"""The split build (MMX_X2 / MMX_X3, include/mmx_hip.h): bf16 weight stream, fp32 activations carried as 2 / 3 bf16
terms inside every MFMA product.  It is the build that has to meet the north star on the headline path — FSQ token ids
bit-exact and waveform within 1e-3 abs of the CPU path on identical inputs (BASELINE.json) — at the bf16 build's weight
bytes.  The weights are bf16-representable (mmx/synth.py), so both sides hold them exactly; what differs from the fp32
oracle is the activation rounding: 2^-17 per GEMM input in the flow / DAC (X2), fp32-level in the LM (X3).

Bounds (stated before measuring; each is derived, none is fitted):
  * kernels: X3 = the fp32 build's tolerance; X2 = 2^-17 relative per operand -> 4e-5 of the output range;
  * LM log-probs (17 steps, 24 layers): the fp32 build's 2e-3;
  * DAC waveform / estimator / flow goldens: 16 significant bits against bf16's 8 is 2^-8 of the bf16 build's measured
    error (3e-2 / 6e-2 / 0.25) -> 1.2e-4 / 2.4e-4 / 1e-3; the stated bounds leave 2x: 2.5e-4 / 5e-4 / 2e-3;
  * composed path: ids identical, waveform <= 1e-3 (the north star itself).
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

X2, X3 = 2, 3
SEED = 7


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-12))


@pytest.mark.parametrize("dt,tol", [(X2, 4e-5), (X3, 3e-6)])
@pytest.mark.parametrize("B,K,N,epi,rs", [(1, 896, 1152, 0, True), (3, 896, 896, 2, False), (17, 4864, 896, 2, False),
                                          (1, 896, 4864, 1, True), (32, 896, 4864, 1, True), (33, 896, 6564, 0, True)])
def test_skinny_gemm_split(dt, tol, B, K, N, epi, rs):
    """fp32 activations x bf16 weights with the RMSNorm gain riding as kgamma, against float64 math on the same values.
    X3 must be at fp32 level: 3e-6 of the output range is ~25 ulp of fp32 at K = 4864."""
    from mmx import ops
    g = torch.Generator().manual_seed(B * 31 + N)
    x = (torch.randn(B, K, generator=g) * 3).cuda()
    w = (torch.randn((2 * N if epi == 1 else N), K, generator=g) / math.sqrt(K)).to(torch.bfloat16).cuda()
    gam = (1 + 0.1 * torch.randn(K, generator=g)).cuda() if rs else None
    bias = torch.randn(N, generator=g).cuda() if epi == 0 else None
    wp = ops.pack_skinny(w.contiguous(), dtype=dt, interleave_half=(N if epi == 1 else 0))
    xd = x.double()
    acc = (xd * (gam.double() if rs else 1.0)) @ w.double().t()
    if rs:
        acc = acc * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6)
    if epi == 0:
        out = torch.zeros(B, N, device="cuda")
        ops.skinny_gemm(x, wp, B=B, K=K, N=N, dtype=dt, bias=bias, rs=rs, eps=1e-6, epi=0, out_f32=out, kgamma=gam)
        ref = acc + bias.double()
    elif epi == 1:
        out = torch.zeros(B, N, device="cuda")
        ops.skinny_gemm(x, wp, B=B, K=K, N=N, dtype=dt, rs=rs, eps=1e-6, epi=1, out_f32=out, kgamma=gam)
        ref = F.silu(acc[:, :N]) * acc[:, N:]
    else:
        res = torch.randn(B, N, generator=g).cuda()
        out = res.clone()
        ops.skinny_gemm(x, wp, B=B, K=K, N=N, dtype=dt, epi=2, out_f32=out)
        ref = res.double() + acc
    assert rel_err(out, ref) < tol


def test_gemm_split_is_fp32_grade_on_bf16_weights():
    """X3 on the windowed GEMM: error against float64 of the order of an fp32 dot product's own rounding."""
    from mmx import ops
    g = torch.Generator().manual_seed(5)
    M, N, K = 300, 256, 1024
    x = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(torch.bfloat16).cuda()
    ref = x.double() @ w.double().t()
    errs = {}
    for dt in (0, X2, X3):
        out = torch.zeros(M, N, device="cuda")
        ops.linear(x, ops.pack_linear(w.float(), dt), K, dtype=dt, out_f32=out)
        errs[dt] = rel_err(out, ref)
    print(f"gemm vs float64: fp32 build {errs[0]:.2e}, X2 {errs[X2]:.2e}, X3 {errs[X3]:.2e}")
    assert errs[X3] < 2e-6 and errs[X2] < 2e-5 and errs[0] < 2e-6


@pytest.mark.parametrize("B,T,chunk,mode", [(2, 200, 0, "none"), (16, 333, 0, "klen"), (2, 130, 50, "none"), (3, 97, 0, "mask"),
                                            (2, 1000, 50, "none"), (4, 257, 0, "qbegin")])
def test_attn_flash_x_vs_float64(B, T, chunk, mode):
    """fp32 q / k / v with hi + lo bf16 splits of both operands (3 MFMAs per product) against float64 softmax attention:
    2^-17 per operand -> 4e-5 of the output range (stated in the module docstring)."""
    from mmx import ops
    g = torch.Generator().manual_seed(B * 1000 + T)
    H, D = 8, 64
    qkv = (torch.randn(B, T, 3 * H * D, generator=g) * 1.5).cuda()
    lens = [T - (i * 37) % (T // 2) for i in range(B)] if mode in ("klen", "mask") else [T] * B
    lens[0] = T
    mask = torch.zeros(B, T)
    for i, n in enumerate(lens):
        mask[i, :n] = 1
    mask = mask.cuda()
    q_begin = 64 if mode == "qbegin" else 0
    out = torch.full((B, T, H * D), float("nan"), device="cuda")
    ops.attn_flash_x(qkv, qkv[:, :, 512:], qkv[:, :, 1024:], out, B=B, H=H, T=T, ldq=1536, ldk=1536, ldv=1536, ldo=512,
                     q_bs=T * 1536, k_bs=T * 1536, v_bs=T * 1536, o_bs=T * 512, scale=0.125, chunk=chunk, q_begin=q_begin,
                     keymask=(mask if mode == "mask" else None),
                     klen=(torch.tensor(lens, dtype=torch.int32, device="cuda") if mode == "klen" else None))
    x = qkv.double().reshape(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    s = (x[0] @ x[1].transpose(-1, -2)) * 0.125
    vis = mask.bool()[:, None, None, :].expand(B, H, T, T).clone()
    if chunk:
        i = torch.arange(T, device="cuda")
        vis &= (i[None, :] < ((i[:, None] // chunk + 1) * chunk))[None, None]
    ref = (torch.softmax(s.masked_fill(~vis, float("-inf")), -1) @ x[2]).permute(0, 2, 1, 3).reshape(B, T, H * D)
    for i, n in enumerate(lens):                            # padding query rows are don't-care (zeros or finite)
        a, r = out[i, q_begin:n], ref[i, q_begin:n]
        assert torch.isfinite(a).all()
        assert rel_err(a, r) < 4e-5, (i, rel_err(a, r))


def test_lm_teacher_forced_logp_split(golden_dir):
    """24-layer LM, teacher-forced log-probs against the reference golden: X3 is held to the fp32 build's bound."""
    from mmx.llm import LlmEngine
    from oracle import weights as W
    gold = dict(np.load(os.path.join(golden_dir, "llm.npz")))
    sd = W.synth_state_dict(W.load_manifest(os.path.join(golden_dir, "manifest_llm.json")), SEED)
    import test_gpu_llm as TL
    TL.test_teacher_forced_logp_vs_reference_golden(sd, gold, X3, 2e-3)


@pytest.mark.parametrize("lat", [80, 128])
def test_dac_decode_split_vs_reference_golden(golden_dir, lat):
    import test_gpu_dac as TD
    TD.test_dac_decode_vs_reference_golden(golden_dir, lat, X2, 2.5e-4)


def test_flow_split_vs_reference_golden(golden_dir):
    """Estimator seam, conformer encoder and the whole flow.inference (10 Euler steps) against the reference goldens."""
    from mmx.flow import FlowEngine
    from oracle import weights as W
    sd = W.synth_state_dict(W.load_manifest(os.path.join(golden_dir, "manifest_flow.json")), SEED)
    gold = dict(np.load(os.path.join(golden_dir, "flow.npz")))
    import test_gpu_flow as TF
    TF.EST_TOL[X2], TF.FLOW_TOL[X2] = 5e-4, 2e-3
    for fused in (True, False):                              # the row-tile fused kernels and the one-launch-per-op path
        eng = {X2: FlowEngine(sd, dtype=X2, fused=fused)}
        TF.test_estimator_seam(eng, gold, X2)
        TF.test_flow_inference_vs_reference_golden(eng, gold, X2)


# ------------------------------------------------------------------------------------------------ composed, config-3 size
from test_gpu_pipeline import case  # noqa: E402,F401  (the config-3 inputs and the oracle's composed outputs)


def test_composed_pipeline_split_ids_identical_waveform_1e3(case):
    """The north star on the split build, free running: the same 250 ids as the CPU path, the waveform within 1e-3 abs."""
    import test_gpu_pipeline as TP
    eng = TP._engine(case, X2)
    for rep in range(2):                                   # eager pass, then the recorded graphs
        wav = eng.tts(case["text"].cuda(), case["emb"].cuda(), seed=TP.SEED, exact_steps=TP.N_STEPS)
        got = eng.llm.tokens()[0]
        assert got == case["toks"], ("token ids differ from the oracle", rep,
                                     next(i for i, (a, b) in enumerate(zip(got, case["toks"])) if a != b))
        err = (wav.cpu() - case["wav"]).abs().max().item()
        print(f"split build composed: {len(got)} ids identical, waveform max abs err {err:.3e} "
              f"(std {case['wav'].std().item():.3f}, SNR {TP._snr_db(case['wav'], wav.cpu()):.1f} dB)")
        assert wav.shape == case["wav"].shape and err <= TP.WAV_TOL_F32, err


def _ssq_table(x):
    """[32][64] per-16-column-tile sums of squares of the rows of x (the producer side of the RMSNorm statistic)."""
    B, K = x.shape
    t = torch.zeros(32, 64, device=x.device)
    t[:B, :K // 16] = x.double().pow(2).reshape(B, K // 16, 16).sum(-1).float()
    return t


@pytest.mark.parametrize("B,K,N,epi,rs,tw,J", [(1, 896, 1152, 0, True, 1, 1), (32, 896, 1152, 0, True, 1, 1), (17, 896, 896, 2, False, 1, 1),
                                               (32, 896, 4864, 1, True, 2, 1), (9, 896, 4864, 1, True, 1, 1), (32, 4864, 896, 2, False, 2, 8),
                                               (3, 4864, 896, 2, False, 1, 8), (32, 896, 6564, 0, True, 2, 1), (16, 896, 6564, 0, True, 1, 1)])
def test_skinny2_vs_float64(B, K, N, epi, rs, tw, J):
    """The decode-step projection kernel (csrc/decode.hip) on split-plane activations against float64 on the same values,
    fp32 level; with the k split across workgroups (J = 8) it is launched 20 times back to back on the same tickets /
    partial buffers: every launch must return the same bits (slice-order summation, tickets left at zero).  The epilogue
    outputs of the residual projections (planes of out * gamma_next, per-tile sums of squares) and of the SwiGLU (planes)
    are checked too."""
    from mmx import ops
    g = torch.Generator().manual_seed(B * 31 + N + J)
    x = (torch.randn(B, K, generator=g) * 3).cuda()
    w = (torch.randn((2 * N if epi == 1 else N), K, generator=g) / math.sqrt(K)).to(torch.bfloat16).cuda()
    gam = (1 + 0.1 * torch.randn(K, generator=g)).cuda() if rs else None
    gnext = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
    bias = torch.randn(N, generator=g).cuda() if epi == 0 else None
    wp = ops.pack_skinny(w.contiguous(), dtype=X3, interleave_half=(N if epi == 1 else 0))
    xg = x * gam if rs else x
    xs = ops.split_planes(xg)
    assert (ops.merge_planes(xs, B, K) - xg).abs().max().item() == 0.0        # 3 bf16 terms hold an fp32 value exactly
    ssq = _ssq_table(x) if rs else None
    xd = x.double()
    acc = xg.double() @ w.double().t()
    if rs:
        acc = acc * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + 1e-6)
    res = torch.randn(B, N, generator=g).cuda()
    ref = acc + bias.double() if epi == 0 else (F.silu(acc[:, :N]) * acc[:, N:] if epi == 1 else res.double() + acc)
    nt = (N + 15) // 16
    part = torch.full((J * nt * ops.packed_rows(B) // 4 * 64,), float("nan"), device="cuda") if J > 1 else None
    tickets = torch.zeros(nt, dtype=torch.int32, device="cuda") if J > 1 else None
    outs = []
    for rep in range(20 if J > 1 else 2):
        out = res.clone() if epi == 2 else (torch.full((B, N), float("nan"), device="cuda") if epi == 0 else None)
        xs_out = torch.zeros(3, ops.plane_elems(B, N), dtype=torch.bfloat16, device="cuda") if epi != 0 and N % 32 == 0 else None
        ssq_out = torch.zeros(32, 64, device="cuda") if epi == 2 else None
        ops.skinny2(xs, wp, B=B, K=K, N=N, dtype=X3, bias=bias, ssq_in=ssq, eps=1e-6, epi=epi, out=out, xs_out=xs_out,
                    gamma_next=(gnext if epi == 2 else None), ssq_out=ssq_out, tiles_per_wg=tw, ksplit=J, part=part, tickets=tickets)
        got = ops.merge_planes(xs_out, B, N) if epi == 1 else out
        outs.append((got, xs_out, ssq_out))
    torch.cuda.synchronize()
    assert rel_err(outs[0][0], ref) < 3e-6, rel_err(outs[0][0], ref)
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0])
    if epi == 2:
        got, xs_out, ssq_out = outs[0]
        # planes hold out * gamma_next to fp32 rounding (the kernel subtracts the hi term from the UNROUNDED product with one
        # fma, so hi + mid + lo can be one ulp closer to the exact product than the rounded fp32 product is)
        assert rel_err(ops.merge_planes(xs_out, B, N), got.double() * gnext.double()) < 1e-7
        assert rel_err(ssq_out[:B, :nt], _ssq_table(got)[:B, :nt]) < 1e-6 and float(ssq_out[B:].abs().sum()) == 0.0
    if J > 1:
        assert int(tickets.abs().sum()) == 0


def test_decode_prep_and_attention_split_planes():
    """mmx_decode_prep (x -> h copy, planes of x * gamma, per-tile sums of squares) and the decode attention's split-plane
    output against the same kernels' fp32 outputs."""
    from mmx import ops
    g = torch.Generator().manual_seed(9)
    B, K = 19, 896
    x = torch.randn(B, K, generator=g).cuda()
    gam = (1 + 0.1 * torch.randn(K, generator=g)).cuda()
    xs = torch.zeros(3, ops.plane_elems(B, K), dtype=torch.bfloat16, device="cuda")
    ssq, h = torch.zeros(32, 64, device="cuda"), torch.zeros(B, K, device="cuda")
    ops.decode_prep(x, xs, ssq, B=B, K=K, gamma=gam, h=h)
    assert torch.equal(h, x) and rel_err(ops.merge_planes(xs, B, K), x.double() * gam.double()) < 1e-7
    assert rel_err(ssq[:B, :56], _ssq_table(x)[:B, :56]) < 1e-6 and float(ssq[:, 56:].abs().sum()) == 0.0
    # decode attention: row-major fp32 output vs split-plane output of the same launch arguments
    Hq, Hkv, D, page, P = 14, 2, 64, 16, 8
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).cuda()
    pos = torch.randint(1, page * P - 1, (B,), generator=g).to(torch.int32).cuda()
    kc = torch.randn(B * P + 1, Hkv, page, D, generator=g).cuda()
    vc = torch.randn(B * P + 1, Hkv, page, D, generator=g).cuda()
    bt = torch.arange(B * P, dtype=torch.int32).reshape(B, P).cuda()
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2).float() / D))).cuda()
    o1 = torch.zeros(B, Hq * D, device="cuda")
    o2 = torch.zeros(3, ops.plane_elems(B, Hq * D), dtype=torch.bfloat16, device="cuda")
    ops.decode_attn(qkv, inv, pos, kc.clone(), vc.clone(), bt, o1, B=B, Hq=Hq, Hkv=Hkv, page=page, dtype=0, per_head=True)
    ops.decode_attn(qkv, inv, pos, kc.clone(), vc.clone(), bt, o2, B=B, Hq=Hq, Hkv=Hkv, page=page, dtype=0, per_head=True, out_split=True)
    assert torch.equal(ops.merge_planes(o2, B, Hq * D), o1)


def test_lm_split_decode_v2_equals_round2_kernel(golden_dir):
    """The decode step on csrc/decode.hip produces the log-probs of the same step on the round-2 kernel (NS = 3) to fp32
    rounding (different summation trees), at batch 1 and at batch 32 (two 16-row tiles, k split across workgroups)."""
    from mmx import shapes, synth
    from mmx.llm import LlmEngine
    sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    z = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    g = torch.Generator().manual_seed(4)
    for B in (1, 32):
        texts = [torch.randint(0, 151936, (1, 6 + b % 5), generator=g).cuda() for b in range(B)]
        lp = {}
        for v2 in (False, True):
            eng = LlmEngine(sd, dtype=X3, max_batch=B, max_ctx=128, use_graphs=False, lm_planes="bf16x3",
                            decode_on=("planes" if v2 else "skinny"))
            xs = [eng.build_lm_input(t, z, z) for t in texts]
            eng.start(xs, [12] * B, [12] * B, seed=3, want_logp=True)
            for _ in range(6):
                eng.step()
            lp[v2] = (eng.logp.clone(), eng.tokens())
        d = (lp[True][0] - lp[False][0]).abs().max().item()
        print(f"decode v2 vs round-2 kernel, batch {B}: max |dlogp| {d:.3e}")
        assert d < 2e-4 and lp[True][1] == lp[False][1]


def test_zero_shot_batch_vs_oracle():
    """Prompt-conditioned (zero-shot) synthesis through the throughput path: TtsEngine.tts_batch with per-utterance prompt
    text + LM prompt speech tokens (llm.py:691-703) and flow prompt tokens + prompt latents (flow.py:472-498), one of the
    three utterances without a prompt, against the oracle's composed path — ids identical, waveform <= 1e-3 (split build)."""
    from mmx import shapes, synth
    from mmx.pipeline import TtsEngine
    from oracle import dac as ODAC, flow as OFLOW, llm as OLLM
    llm_sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    flow_sd = synth.synth_state_dict(shapes.flow_manifest(), 0)
    dac_sd = synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0)
    g = torch.Generator().manual_seed(21)
    B, lens = 3, [40, 61, 33]
    texts = [torch.randint(0, 151936, (1, 12), generator=g) for _ in range(B)]
    ptext = [torch.randint(0, 151936, (1, 4), generator=g), None, torch.randint(0, 151936, (1, 7), generator=g)]
    lps = [torch.randint(0, 6561, (1, 18), generator=g), None, torch.randint(0, 6561, (1, 26), generator=g)]
    fpt = [torch.randint(0, 6561, (1, 18), generator=g), None, torch.randint(0, 6561, (1, 26), generator=g)]
    feat = [torch.randn(1, 36, 80, generator=g) * 0.5, None, torch.randn(1, 52, 80, generator=g) * 0.5]
    emb = [torch.randn(1, 192, generator=g) for _ in range(B)]
    c = lambda t: None if t is None else t.cuda()
    eng = TtsEngine(llm_sd, flow_sd, dac_sd, dtype=X2, max_batch=B, max_ctx=256)
    z, zf = torch.zeros(1, 0, dtype=torch.long), torch.zeros(1, 0, 80)
    for overlap in (False, True):
        wavs = eng.tts_batch([c(t) for t in texts], [c(e) for e in emb], seed=4, exact_steps=lens, overlap=overlap, group_size=2,
                             prompt_texts=[c(t) for t in ptext], llm_prompt_speech_tokens=[c(t) for t in lps],
                             flow_prompt_speech_tokens=[c(t) for t in fpt], prompt_speech_feats=[c(t) for t in feat])
        torch.cuda.synchronize()
        for b in range(B):
            pt, ls, fp, ff = (ptext[b] if ptext[b] is not None else z), (lps[b] if lps[b] is not None else z), \
                (fpt[b] if fpt[b] is not None else z), (feat[b] if feat[b] is not None else zf)
            with torch.no_grad():
                toks = OLLM.lm_inference(llm_sd, OLLM.QwenCfg(layers=2), texts[b], pt, ls, seed=4, seq=b, max_steps=lens[b], ignore_eos_always=True)
                lat = OFLOW.flow_inference(flow_sd, torch.tensor(toks).reshape(1, -1), fp, ff, emb[b])
                wav = ODAC.decode(dac_sd, lat, [5, 4, 4, 3, 2])
            assert eng.last_tokens[b].tolist() == toks, (overlap, b)
            err = (wavs[b].cpu() - wav).abs().max().item()
            print(f"zero-shot batch (overlap={overlap}) utterance {b}: {len(toks)} ids identical, waveform max abs err {err:.3e}")
            assert wavs[b].shape == wav.shape and err <= 1e-3, (b, err)


@pytest.mark.parametrize("B,T,masked,with_next", [(3, 150, False, True), (2, 64, True, True), (1, 333, True, False), (5, 97, False, True)])
def test_est_tail_64_row_split_tile_equals_32_row_tile(B, T, masked, with_next):
    """mmx_est_tail, split build, 64-row tile (attention tile in two K halves, 256-wide FF chunks, one-fragment patches, A fragments
    read per plane) == the 32-row tile, bit for bit: the same per-row arithmetic in the same order (ragged last tiles, row mask,
    with and without the next block's LayerNorm + Q/K/V, both ring depths)."""
    from mmx import ops, shapes, synth
    from mmx.flow import FlowEngine
    fl = FlowEngine(synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1), 0), dtype=X2, use_graphs=False)
    blocks = [w for st in fl.mid for w in st["blocks"]]
    g = torch.Generator().manual_seed(11 + T)
    Tp = ops.round_up(T, 8)
    ao = torch.randn(B, T, 512, generator=g).cuda()
    x0 = torch.randn(B, T, 256, generator=g).cuda()
    mask = (torch.rand(B, T, generator=g) > 0.3).float().cuda() if masked else None
    outs = []
    for bm, pf in ((32, 0), (64, 0), (64, 4)):
        x = x0.clone()
        qk = torch.zeros(B, T, 2048, dtype=torch.bfloat16, device="cuda")
        vt = torch.zeros(B, 2, 512, Tp, dtype=torch.bfloat16, device="cuda")
        act = torch.zeros(B, T, 512, device="cuda")
        w, wn = blocks[0], blocks[1]
        nxt = ops.est_next(wqkv=wn["wqkv_p"], n1g=wn["n1g"], n1b=wn["n1b"], q_out=qk, ldq=2048, q_bs=T * 2048, vt_out=vt, ldvt=Tp,
                           vt_bs=2 * 512 * Tp) if with_next else None
        ops.est_tail(ao, x, w, B=B, T=T, dtype=X2, bm=bm, nxt=nxt, pf=pf, rowmask=mask, act_out=act[:, :, 256:], act_ld=512)
        torch.cuda.synchronize()
        outs.append((x, qk, vt, act))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("wp", [False, True])
def test_split_tiles_of_every_height_agree_bit_for_bit(wp):
    """Which tile height a fused estimator kernel runs with depends on the size of the flow group an utterance lands in; the split
    build's result must not.  est_tail on 16- / 32- / 64-row tiles (all 8 waves) and est_resnet (cin = 256) on 16- / 32-row tiles
    (both 8 waves): identical bits, with and without weight planes."""
    from mmx import ops, shapes, synth
    from mmx.flow import FlowEngine
    fl = FlowEngine(synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1), 0, kind=("fp32" if wp else "bf16")), dtype=X2, use_graphs=False,
                    wplanes=wp)
    blocks = [w for st in fl.mid for w in st["blocks"]]
    res = [st["res"] for st in fl.mid]
    g = torch.Generator().manual_seed(31)
    B, T = 2, 173
    Tp = ops.round_up(T, 8)
    ao = torch.randn(B, T, 512, generator=g).cuda()
    a_in = torch.randn(B, T, 256, generator=g).cuda()
    x0 = torch.randn(B, T, 256, generator=g).cuda()
    tv = torch.randn(B, 14 * 256, generator=g).cuda()
    mask = (torch.rand(B, T, generator=g) > 0.3).float().cuda()
    w, wn = blocks[0], blocks[1]

    def run(fn):
        x = x0.clone()
        qk = torch.zeros(B, T, 2048, dtype=torch.bfloat16, device="cuda")
        vt = torch.zeros(B, 2, 512, Tp, dtype=torch.bfloat16, device="cuda")
        nxt = ops.est_next(wqkv=wn["wqkv_p"], n1g=wn["n1g"], n1b=wn["n1b"], q_out=qk, ldq=2048, q_bs=T * 2048, vt_out=vt, ldvt=Tp, vt_bs=2 * 512 * Tp)
        fn(x, nxt)
        torch.cuda.synchronize()
        assert torch.isfinite(x).all() and float(x.abs().max()) > 0
        return x, qk, vt

    tails = [run(lambda x, nxt, bm=bm: ops.est_tail(ao, x, w, B=B, T=T, dtype=X2, bm=bm, nxt=nxt, rowmask=mask)) for bm in (16, 32, 64)]
    resn = [run(lambda x, nxt, bm=bm: ops.est_resnet(a_in, 256, 256, x, res[0], tv, 14 * 256, B=B, T=T, dtype=X2, bm=bm, rowmask=mask, nxt=nxt))
            for bm in (16, 32)]
    for outs in (tails, resn):
        for other in outs[1:]:
            for a, b in zip(outs[0], other):
                assert torch.equal(a, b)


def test_est_tail_64_row_split_tile_equals_32_row_tile_with_weight_planes():
    """The same with weight planes (an fp32-kind checkpoint: every packed weight as hi + lo bf16 packs, MMX_X2W): the 64-row tile and
    the 32-row tile meet hi and lo packs in the same order (per 256 columns of the FF intermediate) and agree bit for bit."""
    from mmx import ops, shapes, synth
    from mmx.flow import FlowEngine
    fl = FlowEngine(synth.synth_state_dict(shapes.flow_manifest(num_mid_blocks=1), 0, kind="fp32"), dtype=X2, use_graphs=False, wplanes=True)
    blocks = [w for st in fl.mid for w in st["blocks"]]
    assert isinstance(blocks[0]["wo_p"], ops.Planed)
    g = torch.Generator().manual_seed(23)
    B, T = 3, 150
    Tp = ops.round_up(T, 8)
    ao = torch.randn(B, T, 512, generator=g).cuda()
    x0 = torch.randn(B, T, 256, generator=g).cuda()
    mask = (torch.rand(B, T, generator=g) > 0.3).float().cuda()
    outs = []
    for bm in (32, 64):
        x = x0.clone()
        qk = torch.zeros(B, T, 2048, dtype=torch.bfloat16, device="cuda")
        vt = torch.zeros(B, 2, 512, Tp, dtype=torch.bfloat16, device="cuda")
        w, wn = blocks[0], blocks[1]
        nxt = ops.est_next(wqkv=wn["wqkv_p"], n1g=wn["n1g"], n1b=wn["n1b"], q_out=qk, ldq=2048, q_bs=T * 2048, vt_out=vt, ldvt=Tp, vt_bs=2 * 512 * Tp)
        ops.est_tail(ao, x, w, B=B, T=T, dtype=X2, bm=bm, nxt=nxt, rowmask=mask)
        torch.cuda.synchronize()
        outs.append((x, qk, vt))
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 0
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ full-size configs 4 and 5
def test_config4_rank_share_full_size_split_vs_oracle(case):
    """BASELINE config 4, one rank's share at FULL size on the split build — the shape `bench.py` times: 32 utterances, lengths
    U{50..500} tokens (seed 3), 24-layer LM, the overlapped schedule (decode loop with two 16-row MFMA tiles and the ticketed
    split-K down projection, compaction into the 16-slot engine, ragged zero-padded flow groups with the batched encoder,
    64-row est_tail tiles beside the decode loop).  The two shortest and the longest utterance against the CPU oracle's
    composed path: ids identical, waveform within 1e-3 (the north star; sequence id = position in the batch keys the Philox
    stream on both sides).  The back-to-back schedule must give the same ids for all 32."""
    from mmx.pipeline import TtsEngine
    from oracle import dac as ODAC, flow as OFLOW, llm as OLLM
    lens = torch.randint(50, 501, (32,), generator=torch.Generator().manual_seed(3)).tolist()
    g = torch.Generator().manual_seed(2)
    texts = [torch.randint(0, 151936, (1, 48), generator=g) for _ in range(32)]
    emb = case["emb"].cuda()
    tc = [t.cuda() for t in texts]
    eng = TtsEngine(case["llm_sd"], case["flow_sd"], case["dac_sd"], dtype=X2, max_batch=32, max_ctx=640)
    for rep in range(2):                                   # eager pass, then the recorded graphs
        wavs = eng.tts_batch(tc, [emb] * 32, seed=0, exact_steps=lens, overlap=True)
        torch.cuda.synchronize()
        ids = [t.tolist() for t in eng.last_tokens]
        if rep == 0:
            first = ([w.clone() for w in wavs], ids)
    assert ids == first[1]
    for b in range(32):                                    # other flow groups / graphs: rounding of the fp32 activations only
        assert wavs[b].shape == first[0][b].shape == (1, 1, 2 * len(ids[b]) * 480)
        assert (wavs[b] - first[0][b]).abs().max().item() < 2e-4, b
    eng.tts_batch(tc, [emb] * 32, seed=0, exact_steps=lens, overlap=False)
    assert [t.tolist() for t in eng.last_tokens] == ids
    z = torch.zeros(1, 0, dtype=torch.long)
    order = sorted(range(32), key=lambda i: lens[i])
    for b in order[:2] + order[-1:]:
        with torch.no_grad():
            toks = OLLM.lm_inference(case["llm_sd"], OLLM.QwenCfg(), texts[b], z, z, seed=0, seq=b, max_steps=lens[b], ignore_eos_always=True)
            lat = OFLOW.flow_inference(case["flow_sd"], torch.tensor(toks).reshape(1, -1), z, torch.zeros(1, 0, 80), case["emb"])
            wav = ODAC.decode(case["dac_sd"], lat, [5, 4, 4, 3, 2])
        assert ids[b] == toks, (b, next(i for i, (x, y) in enumerate(zip(ids[b], toks)) if x != y))
        err = (wavs[b].cpu() - wav).abs().max().item()
        print(f"config-4 share on the split build, utterance {b} ({lens[b]} steps): {len(toks)} ids identical, waveform max abs err {err:.3e}")
        assert wavs[b].shape == wav.shape and err <= 1e-3, (b, err)


def test_config5_long_form_streaming_full_size_split_vs_oracle(case, capsys):
    """BASELINE config 5 at FULL size on the split build: ONE 60 s utterance (290 text ids, 1500 decode steps, 24-layer LM,
    captured decode graph), streamed in 25-token hops with the estimator state cache, against the oracle.
      (a) Token ids.  Any two fp32 evaluations of the LM differ by ~1e-5 in log-prob (this build: 2e-5 against the oracle,
          tools/long_ctx_diag.py; the reference on another BLAS likewise), and the reference's sampler hands its multinomial noise
          out by SORTED POSITION, so two candidates closer than that swap noise and the draw changes: over 1500 steps of a flat
          distribution such near-ties occur (measured: step 1143, two ids 2.1e-5 apart).  oracle.llm.decision_unstable marks the
          steps whose draw a 6e-5 perturbation can flip.  Required: free running, the ids are identical up to the first such
          step; teacher forced along the oracle's ids, EVERY draw equals the oracle's except at such steps.
      (b) The first four chunks of the stream (teacher forced: the oracle's ids) within 1e-3 of oracle/stream.py's first four
          hops (a hop sees only the tokens before it, so the prefix of the oracle's schedule is the schedule of the prefix).
      (c) The closing chunk (cross-faded seam included) within 1e-3 of the oracle's, on a 10 s utterance of the same schedule (a
          3000-frame oracle pass takes minutes on the host cores).  The oracle side is two flow passes instead of twenty: the
          LAST streaming pass and the closing pass - streaming passes agree on finished frames (the flow is chunk causal), so
          the last streaming pass alone holds every latent frame the earlier ones rendered."""
    from mmx.pipeline import TtsEngine
    from oracle import flow as OFLOW, llm as OLLM, stream as OS
    import time
    N = 1500
    t_start = time.time()

    def tick(msg):                                         # a heartbeat past pytest's capture: minutes of CPU oracle follow
        with capsys.disabled():
            print(f"  [config 5, {time.time() - t_start:5.0f} s] {msg}", flush=True)

    text = torch.randint(0, 151936, (1, 290), generator=torch.Generator().manual_seed(6))
    emb = case["emb"]
    z, zf = torch.zeros(1, 0, dtype=torch.long), torch.zeros(1, 0, 80)
    unstable, drawn = [], []
    tick("oracle LM, 1500 steps ...")
    with torch.no_grad():
        toks = OLLM.lm_inference(case["llm_sd"], OLLM.QwenCfg(), text, z, z, seed=1, seq=0, max_steps=N, ignore_eos_always=True,
                                 unstable=unstable, sampled_out=drawn)
    tick("GPU: free-running ids, then the teacher-forced 60 s stream ...")
    assert len(drawn) == N
    eng = TtsEngine(case["llm_sd"], case["flow_sd"], case["dac_sd"], dtype=X2, max_batch=1, max_ctx=2048)
    free = eng.generate_tokens([text.cuda()], seed=1, exact_steps=N)[0].tolist()
    first = unstable[0] if unstable else N
    k = sum(1 for t in drawn[:first] if t < 6561)          # ids accepted before the first unstable step
    assert free[:k] == toks[:k], ("free-running ids leave the oracle's before its first unstable step", first,
                                  next(i for i, (a, b) in enumerate(zip(free, toks)) if a != b))
    forced = torch.tensor(drawn).reshape(1, -1).cuda()
    chunks = [c.reshape(-1).cpu() for c in eng.tts_stream(text.cuda(), emb.cuda(), seed=1, exact_steps=N, cache=True, forced=forced)]
    n_out = int(eng.llm.state[2, 0])
    got, mine = eng.llm.out_tokens[0, :n_out].tolist(), eng.llm.sampled[0, :N].tolist()
    CL, CR = eng.dac.ctx_left, eng.dac.ctx_right
    del eng
    torch.cuda.empty_cache()
    diff = [i for i in range(N) if mine[i] != drawn[i]]
    print(f"config 5 on the split build: {N} steps, {len(toks)} ids; steps the oracle marks unstable (6e-5): {unstable}; free-running ids "
          f"identical for the first {next((i for i, (a, b) in enumerate(zip(free, toks)) if a != b), len(toks))}; teacher-forced draws that differ: {diff}")
    assert got == toks and set(diff) <= set(unstable), (diff, unstable)
    tk = torch.tensor(toks).reshape(1, -1)
    sched = OS.hop_schedule(len(toks), 0)
    assert len(chunks) == len(sched) and sum(c.shape[0] for c in chunks) == len(toks) * 960
    tick("oracle: first four hops ...")
    with torch.no_grad():
        head = [(off * 2, OFLOW.flow_inference(case["flow_sd"], tk[:, :vis], z, zf, emb, streaming=True, finalize=False)[0].t().contiguous(), False)
                for vis, off, _ in sched[:4]]
        want = OS.render_passes(case["dac_sd"], [5, 4, 4, 3, 2], head, CL, CR)
        errs = [(g - w).abs().max().item() for g, w in zip(chunks[:4], want)]
        assert [g.shape for g in chunks[:4]] == [w.shape for w in want]
        print(f"config 5 on the split build ({len(chunks)} chunks): first four chunks vs the oracle's hops {[f'{e:.2e}' for e in errs]}")
        assert max(errs) <= 1e-3, errs
    # (c) the closing seam at 10 s (250 steps, ten hops): the same schedule, the oracle's last streaming pass and closing pass (a 60 s
    # oracle pass over 3000 frames takes minutes on the host cores; the seam arithmetic does not depend on the length)
    N2 = 250
    drawn2 = []
    with torch.no_grad():
        toks2 = OLLM.lm_inference(case["llm_sd"], OLLM.QwenCfg(), text, z, z, seed=2, seq=0, max_steps=N2, ignore_eos_always=True, sampled_out=drawn2)
    tick(f"closing seam at {len(toks2)} tokens: GPU stream, then two oracle flow passes ...")
    eng = TtsEngine(case["llm_sd"], case["flow_sd"], case["dac_sd"], dtype=X2, max_batch=1, max_ctx=2048)
    chunks2 = [c.reshape(-1).cpu() for c in eng.tts_stream(text.cuda(), emb.cuda(), seed=2, exact_steps=N2, cache=True,
                                                           forced=torch.tensor(drawn2).reshape(1, -1).cuda())]
    assert eng.llm.out_tokens[0, :int(eng.llm.state[2, 0])].tolist() == toks2
    del eng
    torch.cuda.empty_cache()
    tk2 = torch.tensor(toks2).reshape(1, -1)
    sched2 = OS.hop_schedule(len(toks2), 0)
    assert len(chunks2) == len(sched2)
    with torch.no_grad():
        vis, off, _ = sched2[-2]
        last = OFLOW.flow_inference(case["flow_sd"], tk2[:, :vis], z, zf, emb, streaming=True, finalize=False)[0].t().contiguous()
        tick("oracle: last streaming pass done")
        fin = OFLOW.flow_inference(case["flow_sd"], tk2, z, zf, emb, streaming=False, finalize=True)[0].t().contiguous()
        tick("oracle: closing pass done")
        tail = OS.render_passes(case["dac_sd"], [5, 4, 4, 3, 2], [(off * 2, last, False), (sched2[-1][1] * 2, fin, True)], CL, CR)[-1]
    err = (chunks2[-1] - tail).abs().max().item()
    print(f"config 5 on the split build: closing chunk ({tail.shape[0]} samples, cross-faded seam included) vs the oracle {err:.3e}")
    assert chunks2[-1].shape == tail.shape and err <= 1e-3, err


# ------------------------------------------------------------------------------------------------ fp32 checkpoints
def test_dac_trained_weight_norm_vs_reference_golden(golden_dir):
    """weight_g != ||weight_v|| (tests/golden/dac80_fp32.npz: the reference's Decoder on the "fp32" checkpoint kind of
    mmx/synth.py, per-channel weight_g / ||weight_v|| in [0.6, 1.5], ConvTranspose1d gains per dim-0 slice).  fp32 build: the
    fold (ops.fold_weight_norm) must reproduce the reference within 1e-4.  The split and bf16 builds ROUND the folded weights
    to bf16 at load (2^-9 relative per weight): their distance is reported and held to the bf16-weight bound below."""
    from mmx.dac import DacDecoderEngine
    from oracle import weights as W
    sd = W.synth_state_dict(W.load_manifest(os.path.join(golden_dir, "manifest_dac80.json")), SEED, kind="fp32")
    g = np.load(os.path.join(golden_dir, "dac80_fp32.npz"))
    for dt, tol in ((0, 1e-4), (X2, 3e-2), (1, 6e-2)):
        eng = DacDecoderEngine(sd, [5, 4, 4, 3, 2], dtype=dt)
        for T in (8, 50):
            wav = eng.decode(torch.from_numpy(g[f"z_T{T}"]).cuda()).cpu()
            ref = torch.from_numpy(g[f"wav_T{T}"])
            err = (wav - ref).abs().max().item()
            print(f"DAC on a trained-like weight norm, dtype {dt}, T={T}: max abs err {err:.3e}")
            assert wav.shape == ref.shape and err < tol, (dt, T, err)


@pytest.fixture(scope="module")
def case_fp32():
    """Config-3 inputs on the "fp32" checkpoint kind (general fp32 weights, trained-like weight norms: what the reference's
    loaders hand over, cli/model.py:67-75, dac-vae/inference.py:42-46) and the oracle's composed outputs on them."""
    import test_gpu_pipeline as TP
    from mmx import shapes, synth
    from oracle import dac as ODAC, flow as OFLOW, llm as OLLM
    llm_sd = synth.synth_state_dict(shapes.llm_manifest(), 0, kind="fp32")
    flow_sd = synth.synth_state_dict(shapes.flow_manifest(), 0, kind="fp32")
    dac_sd = synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0, kind="fp32")
    text = torch.randint(0, 151936, (1, TP.N_TEXT), generator=torch.Generator().manual_seed(2))
    emb = torch.randn(1, 192, generator=torch.Generator().manual_seed(1))
    z = torch.zeros(1, 0, dtype=torch.long)
    with torch.no_grad():
        toks = OLLM.lm_inference(llm_sd, OLLM.QwenCfg(), text, z, z, seed=TP.SEED, seq=0, max_steps=TP.N_STEPS, ignore_eos_always=True)
        lat = OFLOW.flow_inference(flow_sd, torch.tensor(toks).reshape(1, -1), z, torch.zeros(1, 0, 80), emb)
        wav = ODAC.decode(dac_sd, lat, [5, 4, 4, 3, 2])
    return dict(llm_sd=llm_sd, flow_sd=flow_sd, dac_sd=dac_sd, text=text, emb=emb, toks=toks, lat=lat, wav=wav)


def test_split_build_on_an_fp32_checkpoint_measured(case_fp32):
    """What the split build WITHOUT weight planes does on a checkpoint whose weights are not bf16-representable (it rounds
    them to bf16 at load): measured against the oracle on the unrounded weights and printed for DESIGN.md — free-running id
    agreement, teacher-forced draw agreement, and the waveform error of flow + DAC on the oracle's ids.  The requirement here
    is only the bf16-WEIGHT bound (8 significant bits of every weight, 16 / 24 of every activation): teacher-forced agreement
    >= 60 % and SNR >= 25 dB, the bf16 build's own bounds; the north star on such checkpoints is the job of the weight-plane
    mode (test_weight_planes_*)."""
    import test_gpu_pipeline as TP
    case = case_fp32
    eng = TP._engine(case, X2)
    eng.tts(case["text"].cuda(), case["emb"].cuda(), seed=TP.SEED, exact_steps=TP.N_STEPS)
    got, want = eng.llm.tokens()[0], case["toks"]
    n = min(len(got), len(want))
    first = next((i for i in range(n) if got[i] != want[i]), n)
    mism = sum(1 for i in range(n) if got[i] != want[i]) + abs(len(got) - len(want))
    z0 = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    x = eng.llm.build_lm_input(case["text"].cuda(), z0, z0)
    eng.llm.start([x], [TP.N_STEPS], [TP.N_STEPS], seed=TP.SEED, forced=torch.tensor(want).reshape(1, -1))
    eng.llm.run(TP.N_STEPS)
    drawn = eng.llm.sampled[0, :len(want)].tolist()
    agree = sum(1 for a, b in zip(drawn, want) if a == b) / len(want)
    tok = torch.tensor(want, device="cuda").reshape(1, -1)
    wav = eng.token2wav(tok, z0, torch.zeros(1, 0, 80, device="cuda"), case["emb"].cuda()).cpu()
    err, snr = (wav - case["wav"]).abs().max().item(), TP._snr_db(case["wav"], wav)
    print(f"split build, weights ROUNDED to bf16 at load, vs the oracle on the fp32 checkpoint: free running {mism}/{n} ids differ "
          f"(first divergence at step {first}); teacher forced {agree * 100:.1f} % of the draws equal; same-ids waveform max abs err "
          f"{err:.3e}, SNR {snr:.1f} dB")
    assert agree >= TP.BF16_MIN_TF_AGREEMENT and snr >= TP.BF16_MIN_SNR_DB, (agree, snr)


# ------------------------------------------------------------------------------------------------ weight planes (fp32 checkpoints)
def test_weight_planes_gemm_vs_float64():
    """mmx_gemm_win with MMX_X2W / MMX_X3W: GENERAL fp32 weights as 2 / 3 bf16 planes, every term above the last kept bit
    (3 / 6 MFMAs per fragment pair) against float64 on the same values.  Bounds as for bf16-exact weights: 2^-17 per operand
    (X2W: 4e-5 of the output range stated, half of it expected), fp32 level (X3W).  The plain X2 / X3 codes on the same weights
    ROUND them to bf16: their error (printed) is the 2^-9 the weight planes remove.  Also a 3-tap dilated conv (windowed rows)."""
    from mmx import ops
    from mmx._lib import X2W, X3W
    g = torch.Generator().manual_seed(15)
    M, N, K = 300, 200, 1000                              # ragged tiles, K padded to 1024 inside every plane
    x = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda()
    ref = x.double() @ w.double().t()
    errs = {}
    for name, dt, pdt in (("X2", X2, X2), ("X3", X3, X3), ("X2W", X2, X2W), ("X3W", X3, X3W)):
        out = torch.zeros(M, N, device="cuda")
        wp = ops.pack_linear(w, pdt)
        assert isinstance(wp, ops.Planed) == (pdt in (X2W, X3W)) and wp.shape == (N, 1024 * (1 if pdt in (X2, X3) else (2 if pdt == X2W else 3)))
        ops.linear(x, wp, K, dtype=dt, out_f32=out)
        errs[name] = rel_err(out, ref)
    print("gemm on general fp32 weights vs float64: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["X2W"] < 4e-5 and errs["X3W"] < 3e-6 and errs["X2"] > 20 * errs["X2W"]
    B, T, C = 2, 77, 96
    xc = torch.randn(B, T, C, generator=g).cuda()
    wc = (torch.randn(64, C, 3, generator=g) / math.sqrt(3 * C)).cuda()
    bias = torch.randn(64, generator=g).cuda()
    want = F.conv1d(F.pad(xc.double().transpose(1, 2), (2, 2)), wc.double(), bias.double(), dilation=2).transpose(1, 2)
    out = torch.zeros(B, T, 64, device="cuda")
    ops.conv1d(xc, ops.pack_conv1d(wc, X2W), T=T, Cin=C, k=3, dil=2, pad_left=2, dtype=X2, batch=B, bias=bias, out_f32=out)
    assert rel_err(out, want) < 4e-5


@pytest.mark.parametrize("B,K,N,epi,rs,J", [(1, 896, 1152, 0, True, 1), (32, 896, 1152, 0, True, 1), (17, 896, 896, 2, False, 1),
                                            (32, 896, 4864, 1, True, 1), (32, 4864, 896, 2, False, 8), (3, 4864, 896, 2, False, 8),
                                            (16, 896, 6564, 0, True, 1)])
def test_weight_planes_skinny2_vs_float64(B, K, N, epi, rs, J):
    """The decode-step projection with MMX_X3W: general fp32 weights as three bf16 planes, six MFMAs per fragment, against
    float64 on the same values - fp32 level, as for bf16-exact weights (test_skinny2_vs_float64)."""
    from mmx import ops
    from mmx._lib import X3W
    g = torch.Generator().manual_seed(B * 31 + N + J)
    x = (torch.randn(B, K, generator=g) * 3).cuda()
    w = (torch.randn((2 * N if epi == 1 else N), K, generator=g) / math.sqrt(K)).cuda()
    gam = (1 + 0.1 * torch.randn(K, generator=g)).cuda() if rs else None
    bias = torch.randn(N, generator=g).cuda() if epi == 0 else None
    wp = ops.pack_skinny(w.contiguous(), dtype=X3W, interleave_half=(N if epi == 1 else 0))
    assert isinstance(wp, ops.Planed)
    xg = x * gam if rs else x
    xs = ops.split_planes(xg)
    ssq = _ssq_table(x) if rs else None
    acc = xg.double() @ w.double().t()
    if rs:
        acc = acc * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + 1e-6)
    res = torch.randn(B, N, generator=g).cuda()
    ref = acc + bias.double() if epi == 0 else (F.silu(acc[:, :N]) * acc[:, N:] if epi == 1 else res.double() + acc)
    nt = (N + 15) // 16
    part = torch.full((J * nt * ops.packed_rows(B) // 4 * 64,), float("nan"), device="cuda") if J > 1 else None
    tickets = torch.zeros(nt, dtype=torch.int32, device="cuda") if J > 1 else None
    out = res.clone() if epi == 2 else (torch.full((B, N), float("nan"), device="cuda") if epi == 0 else None)
    xs_out = torch.zeros(3, ops.plane_elems(B, N), dtype=torch.bfloat16, device="cuda") if epi != 0 and N % 32 == 0 else None
    ops.skinny2(xs, wp, B=B, K=K, N=N, dtype=X3, bias=bias, ssq_in=ssq, eps=1e-6, epi=epi, out=out, xs_out=xs_out,
                ssq_out=(torch.zeros(32, 64, device="cuda") if epi == 2 else None), tiles_per_wg=1, ksplit=J, part=part, tickets=tickets)
    got = ops.merge_planes(xs_out, B, N) if epi == 1 else out
    assert rel_err(got, ref) < 3e-6, rel_err(got, ref)


def test_weight_planes_dac_trained_weight_norm_vs_reference_golden(golden_dir):
    """The DAC decoder on a trained-like weight norm (dac80_fp32.npz, folded weights that are general fp32 values) in the
    weight-plane mode: the split build's own bound for bf16-exact weights (2.5e-4), where rounding the weights gave 1.8e-2."""
    from mmx.dac import DacDecoderEngine
    from oracle import weights as W
    sd = W.synth_state_dict(W.load_manifest(os.path.join(golden_dir, "manifest_dac80.json")), SEED, kind="fp32")
    g = np.load(os.path.join(golden_dir, "dac80_fp32.npz"))
    eng = DacDecoderEngine(sd, [5, 4, 4, 3, 2], dtype=X2, wplanes=True)
    for T in (8, 50):
        wav = eng.decode(torch.from_numpy(g[f"z_T{T}"]).cuda()).cpu()
        err = (wav - torch.from_numpy(g[f"wav_T{T}"])).abs().max().item()
        print(f"DAC on a trained-like weight norm, weight planes, T={T}: max abs err {err:.3e}")
        assert err < 2.5e-4, (T, err)


def test_weight_planes_composed_pipeline_on_an_fp32_checkpoint(case_fp32):
    """The north star on a checkpoint whose weights are NOT bf16-representable (general fp32 LM / flow weights, trained-like DAC
    weight norms): TtsEngine(dtype=split, wplanes=True) at config-3 size, free running, against the oracle on the same
    unrounded weights - the same 250 ids, the waveform within 1e-3."""
    import test_gpu_pipeline as TP
    from mmx.pipeline import TtsEngine
    case = case_fp32
    eng = TtsEngine(case["llm_sd"], case["flow_sd"], case["dac_sd"], dtype=X2, max_batch=1, max_ctx=640, wplanes=True)
    for rep in range(2):
        wav = eng.tts(case["text"].cuda(), case["emb"].cuda(), seed=TP.SEED, exact_steps=TP.N_STEPS)
        got = eng.llm.tokens()[0]
        assert got == case["toks"], ("token ids differ from the oracle", rep, next(i for i, (a, b) in enumerate(zip(got, case["toks"])) if a != b))
        err = (wav.cpu() - case["wav"]).abs().max().item()
        print(f"weight planes, fp32 checkpoint, composed: {len(got)} ids identical, waveform max abs err {err:.3e} "
              f"(SNR {TP._snr_db(case['wav'], wav.cpu()):.1f} dB)")
        assert wav.shape == case["wav"].shape and err <= 1e-3, err


def test_weight_planes_flow_fused_and_per_op_vs_oracle():
    """flow.inference on an fp32 checkpoint (general fp32 weights) in the weight-plane mode, on the fused row-tile kernels (the hi
    pack against both activation planes, then the lo pack against the hi plane: csrc/fused.hip stage_run_w) and on the one-launch-
    per-op path (csrc/gemm.hip, NWP = 2), against the oracle on the same unrounded weights: the split build's bound for
    bf16-exact weights (2e-3; latents of std ~1.2).  Without weight planes the same build lands at the bf16-weight level."""
    from mmx import shapes, synth
    from mmx.flow import FlowEngine
    from oracle import flow as OFLOW
    sd = synth.synth_state_dict(shapes.flow_manifest(), 0, kind="fp32")
    g = torch.Generator().manual_seed(33)
    tok = torch.randint(0, 6561, (1, 60), generator=g)
    ptok = torch.randint(0, 6561, (1, 11), generator=g)
    pfeat = torch.randn(1, 22, 80, generator=g) * 0.5
    emb = torch.randn(1, 192, generator=g)
    with torch.no_grad():
        ref = OFLOW.flow_inference(sd, tok, ptok, pfeat, emb)[0].t().contiguous()
    errs = {}
    for name, kw in (("fused, planes", dict(wplanes=True, fused=True)), ("per op, planes", dict(wplanes=True, fused=False)),
                     ("fused, rounded", dict(wplanes=False, fused=True))):
        eng = FlowEngine(sd, dtype=X2, use_graphs=False, **kw)
        lat = eng.inference_time_major(tok.cuda(), ptok.cuda(), pfeat.cuda(), emb.cuda(), False, True).cpu()
        assert lat.shape == ref.shape
        errs[name] = (lat - ref).abs().max().item()
    print("flow.inference on an fp32 checkpoint vs the oracle: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["fused, planes"] < 2e-3 and errs["per op, planes"] < 2e-3 and errs["fused, rounded"] > 5 * errs["fused, planes"]


@pytest.mark.parametrize("B,T,chunk,ragged,form", [(6, 980, 0, False, 0), (6, 980, 0, True, 0), (10, 420, 50, False, 0), (2, 300, 0, False, 0), (16, 896, 0, True, 0),
                                                    (6, 980, 0, True, 1), (10, 420, 50, False, 1), (6, 980, 0, True, 2), (10, 420, 50, True, 3), (2, 300, 0, False, 2)])
def test_attn_flash_xs_presplit_vs_float64(B, T, chunk, ragged, form):
    """mmx_attn_flash_xs (operands split by the producer: bf16 rows [hi Q | hi K | lo Q | lo K], V transposed as two planes) against
    float64 attention of hi + lo, over launch shapes that take each of its three forms: 4 waves x 16 queries (small launches),
    8 x 16 and 8 x 32 queries (256 per workgroup, chosen when that grid needs fewer rounds of the 256 CUs: 6 x 980 and 10 x 420
    here), and with the form given by the caller (1: the 128-query workgroups of the groups beside the decode loop, 2 / 3: the
    256-query and the 4-wave 64-query workgroups).  2^-17 per operand -> 4e-5 of the output range."""
    from mmx import ops
    g = torch.Generator().manual_seed(B * 1000 + T)
    H, D = 8, 64
    qkv = (torch.randn(B, T, 3 * H * D, generator=g) * 1.5).cuda()
    hi = qkv.to(torch.bfloat16)
    lo = (qkv - hi.float()).to(torch.bfloat16)
    Tp = ops.round_up(T, 8)
    qk = torch.cat([hi[:, :, :1024], lo[:, :, :1024]], dim=2).contiguous()                  # [hi Q | hi K | lo Q | lo K]
    vt = torch.zeros(B, 2, 512, Tp, dtype=torch.bfloat16, device="cuda")
    vt[:, 0, :, :T], vt[:, 1, :, :T] = hi[:, :, 1024:].transpose(1, 2), lo[:, :, 1024:].transpose(1, 2)
    lens = [T - (i * 53) % (T // 2) for i in range(B)] if ragged else [T] * B
    lens[0] = T
    out = torch.full((B, T, H * D), float("nan"), device="cuda")
    ops.attn_flash_xs(qk, vt, out, B=B, H=H, T=T, ldqk=2048, ldvt=Tp, ldo=512, qk_bs=T * 2048, vt_bs=2 * 512 * Tp, o_bs=T * 512, scale=0.125,
                      chunk=chunk, klen=(torch.tensor(lens, dtype=torch.int32, device="cuda") if ragged else None), form=form)
    x = (hi.double() + lo.double()).reshape(B, T, 3, H, D).permute(2, 0, 3, 1, 4)
    for b0 in range(0, B, 4):                                # float64 scores in slices of 4 batch rows (memory)
        xb = x[:, b0:b0 + 4]
        s = (xb[0] @ xb[1].transpose(-1, -2)) * 0.125
        i = torch.arange(T, device="cuda")
        vis = torch.ones(T, T, dtype=torch.bool, device="cuda")
        if chunk:
            vis &= i[None, :] < ((i[:, None] // chunk + 1) * chunk)
        vis = vis[None, None].expand(s.shape[0], H, T, T).clone()
        for j in range(s.shape[0]):
            vis[j, :, :, lens[b0 + j]:] = False
        ref = (torch.softmax(s.masked_fill(~vis, float("-inf")), -1) @ xb[2]).permute(0, 2, 1, 3).reshape(-1, T, H * D)
        for j in range(ref.shape[0]):
            n = lens[b0 + j]
            a, r = out[b0 + j, :n], ref[j, :n]
            assert torch.isfinite(a).all() and rel_err(a, r) < 4e-5, (b0 + j, rel_err(a, r))


# ------------------------------------------------------------------------------------------------ fp16 planes of the LM decode step
@pytest.mark.parametrize("wp", [1, 2])
@pytest.mark.parametrize("B,K,N,epi,rs,tw,J", [(1, 896, 1152, 0, True, 1, 1), (32, 896, 1152, 0, True, 1, 1), (17, 896, 896, 2, False, 1, 1),
                                               (32, 896, 4864, 1, True, 2, 1), (32, 4864, 896, 2, False, 2, 8), (3, 4864, 896, 2, False, 1, 8),
                                               (32, 896, 6564, 0, True, 2, 1)])
def test_skinny2_fp16_planes_vs_float64(B, K, N, epi, rs, tw, J, wp):
    """mmx_skinny2 with MMX_H2 / MMX_H2W: activations as TWO fp16 planes (22 significant bits), fp16 weights stored * 2^8 - one
    plane for bf16-representable weights (exact), hi + lo for general fp32 weights - on v_mfma_f32_16x16x32_f16, against float64
    on the same values.  Stated: 3e-6 of the output range (the three-bf16-plane form's bound; 22 bits against 24 is 2.4e-7
    relative per operand).  The epilogue's plane outputs (fp16 hi + lo of out * gamma_next, of the SwiGLU) are checked too."""
    from mmx import ops
    from mmx._lib import H2
    g = torch.Generator().manual_seed(B * 31 + N + J + wp)
    x = (torch.randn(B, K, generator=g) * 3).cuda()
    w = (torch.randn((2 * N if epi == 1 else N), K, generator=g) / math.sqrt(K))
    w = (w.to(torch.bfloat16).float() if wp == 1 else w).cuda()
    gam = (1 + 0.1 * torch.randn(K, generator=g)).cuda() if rs else None
    gnext = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
    bias = torch.randn(N, generator=g).cuda() if epi == 0 else None
    wpk = ops.pack_skinny_h2(w.contiguous(), planes=wp, interleave_half=(N if epi == 1 else 0))
    assert isinstance(wpk, ops.Planed) == (wp == 2)
    xg = x * gam if rs else x
    xs = ops.split_planes(xg, f16=True)
    assert rel_err(ops.merge_planes(xs, B, K, f16=True), xg) < 3e-7            # two fp16 terms: 22 bits
    ssq = _ssq_table(x) if rs else None
    acc = xg.double() @ w.double().t()
    if rs:
        acc = acc * torch.rsqrt(x.double().pow(2).mean(-1, keepdim=True) + 1e-6)
    res = torch.randn(B, N, generator=g).cuda()
    ref = acc + bias.double() if epi == 0 else (F.silu(acc[:, :N]) * acc[:, N:] if epi == 1 else res.double() + acc)
    nt = (N + 15) // 16
    part = torch.full((J * nt * ops.packed_rows(B) // 4 * 64,), float("nan"), device="cuda") if J > 1 else None
    tickets = torch.zeros(nt, dtype=torch.int32, device="cuda") if J > 1 else None
    out = res.clone() if epi == 2 else (torch.full((B, N), float("nan"), device="cuda") if epi == 0 else None)
    xs_out = torch.zeros(2, ops.plane_elems(B, N), dtype=torch.bfloat16, device="cuda") if epi != 0 and N % 32 == 0 else None
    ops.skinny2(xs, wpk, B=B, K=K, N=N, dtype=H2, bias=bias, ssq_in=ssq, eps=1e-6, epi=epi, out=out, xs_out=xs_out,
                gamma_next=(gnext if epi == 2 else None), ssq_out=(torch.zeros(32, 64, device="cuda") if epi == 2 else None),
                tiles_per_wg=tw, ksplit=J, part=part, tickets=tickets)
    got = ops.merge_planes(xs_out, B, N, f16=True) if epi == 1 else out
    assert rel_err(got, ref) < 3e-6, rel_err(got, ref)
    if epi == 2:
        assert rel_err(ops.merge_planes(xs_out, B, N, f16=True), got.double() * gnext.double()) < 3e-7


def test_decode_prep_and_attention_fp16_planes():
    """mmx_decode_prep and the decode attention's output as two fp16 planes (MMX_H2) against the same kernels' fp32 outputs."""
    from mmx import ops
    from mmx._lib import H2
    g = torch.Generator().manual_seed(9)
    B, K = 19, 896
    x = torch.randn(B, K, generator=g).cuda()
    gam = (1 + 0.1 * torch.randn(K, generator=g)).cuda()
    xs = torch.zeros(2, ops.plane_elems(B, K), dtype=torch.bfloat16, device="cuda")
    ssq, h = torch.zeros(32, 64, device="cuda"), torch.zeros(B, K, device="cuda")
    ops.decode_prep(x, xs, ssq, B=B, K=K, gamma=gam, h=h, dtype=H2)
    assert torch.equal(h, x) and rel_err(ops.merge_planes(xs, B, K, f16=True), x.double() * gam.double()) < 3e-7
    assert rel_err(ssq[:B, :56], _ssq_table(x)[:B, :56]) < 1e-6
    Hq, Hkv, D, page, P = 14, 2, 64, 16, 8
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).cuda()
    pos = torch.randint(1, page * P - 1, (B,), generator=g).to(torch.int32).cuda()
    kc = torch.randn(B * P + 1, Hkv, page, D, generator=g).cuda()
    vc = torch.randn(B * P + 1, Hkv, page, D, generator=g).cuda()
    bt = torch.arange(B * P, dtype=torch.int32).reshape(B, P).cuda()
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2).float() / D))).cuda()
    o1 = torch.zeros(B, Hq * D, device="cuda")
    o2 = torch.zeros(2, ops.plane_elems(B, Hq * D), dtype=torch.bfloat16, device="cuda")
    ops.decode_attn(qkv, inv, pos, kc.clone(), vc.clone(), bt, o1, B=B, Hq=Hq, Hkv=Hkv, page=page, dtype=0, per_head=True)
    ops.decode_attn(qkv, inv, pos, kc.clone(), vc.clone(), bt, o2, B=B, Hq=Hq, Hkv=Hkv, page=page, dtype=0, per_head=True, out_split="f16")
    assert rel_err(ops.merge_planes(o2, B, Hq * D, f16=True), o1) < 3e-7


def test_lm_decode_fp16_planes_equals_bf16_planes():
    """The decode step on two fp16 planes (LlmEngine.lm_planes = "f16x2", the default) produces the log-probs of the same steps on
    three bf16 planes to fp32-level rounding and the same ids, at batch 1 and batch 32, on a bf16-representable and on an fp32
    checkpoint (weight planes: two fp16 planes against three bf16 planes)."""
    from mmx import shapes, synth
    from mmx.llm import LlmEngine
    z = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    g = torch.Generator().manual_seed(4)
    for kind in ("bf16", "fp32"):
        sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0, kind=kind)
        for B in (1, 32):
            texts = [torch.randint(0, 151936, (1, 6 + b % 5), generator=g).cuda() for b in range(B)]
            lp = {}
            for planes in ("bf16x3", "f16x2"):
                eng = LlmEngine(sd, dtype=X3, max_batch=B, max_ctx=128, use_graphs=False, lm_planes=planes, wplanes="auto")
                assert eng.h2 == (planes == "f16x2") and eng.wplanes == (kind == "fp32")
                xs = [eng.build_lm_input(t, z, z) for t in texts]
                eng.start(xs, [12] * B, [12] * B, seed=3, want_logp=True)
                for _ in range(6):
                    eng.step()
                lp[planes] = (eng.logp.clone(), eng.tokens())
            d = (lp["f16x2"][0] - lp["bf16x3"][0]).abs().max().item()
            print(f"decode step, fp16 planes vs bf16 planes, {kind} checkpoint, batch {B}: max |dlogp| {d:.3e}")
            assert d < 2e-4 and lp["f16x2"][1] == lp["bf16x3"][1]


@pytest.mark.parametrize("T,chunk,ragged", [(50, 0, False), (100, 25, False), (173, 0, True), (300, 50, True)])
def test_attn_relpos_x_vs_float64(T, chunk, ragged):
    """Conformer rel-pos attention of the split build on the MFMA (mmx_attn_relpos_x: fp32 operands, every product as bf16
    hi*hi + lo*hi + hi*lo) against the float64 statement of RelPositionMultiHeadedAttention (attention.py:215-330): (q + u) k^T +
    rel_shift((q + v) p^T), chunk mask, prefix lengths of a padded batch, softmax, P V.  2^-17 per operand -> 4e-5 of the range."""
    from mmx import ops
    from oracle import flow as OF
    g = torch.Generator().manual_seed(T + 3)
    B, H, D = 3, 8, 64
    qkv = torch.randn(B, T, 3 * H * D, generator=g).cuda()
    pos = torch.randn(2 * T - 1, H * D, generator=g).cuda()
    pu, pv = (torch.randn(H, D, generator=g) * 0.2).cuda(), (torch.randn(H, D, generator=g) * 0.2).cuda()
    lens = [T, T - 9, T // 2 + 5] if ragged else [T] * B
    out = torch.full((B, T, H * D), float("nan"), device="cuda")
    ops.attn_relpos_x(qkv, qkv[:, :, 512:], qkv[:, :, 1024:], pos, pu, pv, out, B=B, H=H, T=T, ldq=1536, ldk=1536, ldv=1536, ldp=512, ldo=512,
                      q_bs=T * 1536, k_bs=T * 1536, v_bs=T * 1536, o_bs=T * 512, scale=D ** -0.5, chunk=chunk,
                      klen=(torch.tensor(lens, dtype=torch.int32, device="cuda") if ragged else None))
    x = qkv.double().cpu().reshape(B, T, 3, H, D)
    qh = x[:, :, 0]
    kh, vh = x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    ph = pos.double().cpu().view(1, 2 * T - 1, H, D).transpose(1, 2)
    ac = (qh + pu.double().cpu()).transpose(1, 2) @ kh.transpose(-2, -1)
    bd = OF.rel_shift((qh + pv.double().cpu()).transpose(1, 2) @ ph.transpose(-2, -1))
    s = (ac + bd) * D ** -0.5
    if chunk:
        s = s.masked_fill(~OF.subsequent_chunk_mask(T, chunk)[None, None], float("-inf"))
    for b in range(B):
        s[b, :, :, lens[b]:] = float("-inf")
    ref = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(B, T, H * D)
    for b in range(B):
        a, r = out[b, :lens[b]].cpu().double(), ref[b, :lens[b]]
        assert torch.isfinite(a).all() and rel_err(a, r) < 4e-5, (b, rel_err(a, r))
