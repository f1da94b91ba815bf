"""Decode attention with the loop's `finished` flags (mmx_decode_attn_fin, csrc/llm.hip): the workgroups of an ended sequence
return before they touch the cache or the output; every live sequence gets the bits it gets without the flags.

Kernel level: 3 sequences with 1, 33 and 321 cached keys (321: a second pass of the 320-key loop of the fp32 cache), the middle one
finished; one head per workgroup (14 heads) and two (98 heads: 3 x 98 > 256, where the entry point pairs them); row-major fp32
output and two fp16 planes (MMX_H2).  K / V pages live inside larger buffers whose margins hold a pattern.
Engine level: a 2-layer LM, 4 sequences of which one ends early, stepped with and without LlmEngine.skip_finished: ids and
log-probs bit for bit the same at every step.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

CTX = (1, 33, 321)
FIN = 1                          # the finished slot


def _guarded(n, gen, guard=4096):
    """n random floats between two margins of NaN-pattern words -> (whole buffer, view of the n floats)."""
    buf = torch.full((n + 2 * guard,), float("nan"), device="cuda")
    buf[guard:guard + n] = torch.randn(n, generator=gen).cuda()
    return buf, buf[guard:guard + n]


@pytest.mark.parametrize("out_split", [False, "f16"])
@pytest.mark.parametrize("Hq", [14, 98])
def test_finished_slot_is_skipped_live_slots_bit_equal(Hq, out_split):
    from mmx import ops
    g = torch.Generator().manual_seed(Hq + 5)
    B, Hkv, D, page = 3, 2, 64, 16
    P = (max(CTX) + page) // page                           # pages per sequence: keys 0 .. pos
    qkv = torch.randn(B, (Hq + 2 * Hkv) * D, generator=g).cuda()
    pos = torch.tensor(CTX, dtype=torch.int32).cuda()
    fin = torch.tensor([int(b == FIN) for b in range(B)], dtype=torch.int32).cuda()
    npg = B * P + 1
    kbuf, kc0 = _guarded(npg * Hkv * page * D, g)
    vbuf, vc0 = _guarded(npg * Hkv * page * D, g)
    bt = torch.arange(B * P, dtype=torch.int32).reshape(B, P).cuda()
    inv = (1.0 / (1e6 ** (torch.arange(0, D, 2).float() / D))).cuda()
    K = Hq * D
    if out_split:
        sentinel = torch.full((2, ops.plane_elems(B, K)), 1.5, dtype=torch.bfloat16, device="cuda")
        rowid = ops.pack_act(torch.arange(16, device="cuda", dtype=torch.float32)[:, None].expand(16, K).to(torch.bfloat16).contiguous(), 1)
        is_fin = (rowid == FIN)[None].expand(2, -1)
    else:
        sentinel = torch.full((B, K), 1.5, device="cuda")
        is_fin = torch.zeros(B, K, dtype=torch.bool, device="cuda")
        is_fin[FIN] = True

    def run(flags):
        kb, vb, out = kbuf.clone(), vbuf.clone(), sentinel.clone()
        kc = kb[4096:4096 + kc0.numel()].view(npg, Hkv, page, D)
        vc = vb[4096:4096 + vc0.numel()].view(npg, Hkv, page, D)
        ops.decode_attn(qkv, inv, pos, kc, vc, bt, out, B=B, Hq=Hq, Hkv=Hkv, page=page, dtype=0, per_head=True, out_split=out_split,
                        finished=flags)
        torch.cuda.synchronize()
        return kb, vb, out

    k_ref, v_ref, o_ref = run(None)
    k_got, v_got, o_got = run(fin)
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)
    # without the flags every slot's rows are written; with them the finished slot's row keeps the sentinel, the others' bits agree
    assert bool((bits(o_ref) != bits(sentinel))[is_fin].any())
    assert torch.equal(bits(o_got)[is_fin], bits(sentinel)[is_fin])
    assert torch.equal(bits(o_got)[~is_fin], bits(o_ref)[~is_fin])
    # caches: the finished slot's pages are byte for byte what they were before the call, everything else (the live slots' new
    # rows, the untouched pages, both margins) what the call without the flags leaves
    pages = torch.zeros(npg, dtype=torch.bool, device="cuda")
    pages[FIN * P:(FIN + 1) * P] = True
    for before, ref, got in ((kbuf, k_ref, k_got), (vbuf, v_ref, v_got)):
        mask = torch.zeros(before.numel(), dtype=torch.bool, device="cuda")
        mask[4096:4096 + kc0.numel()] = pages[:, None].expand(npg, Hkv * page * D).reshape(-1)
        assert torch.equal(bits(got)[mask], bits(before)[mask])
        assert torch.equal(bits(got)[~mask], bits(ref)[~mask])
        assert bool((bits(ref)[mask] != bits(before)[mask]).any())          # (the unflagged call did append the slot's row)
        assert torch.equal(bits(got)[:4096], bits(before)[:4096]) and torch.equal(bits(got)[-4096:], bits(before)[-4096:])


def test_engine_loop_with_an_early_end_same_ids_and_logprobs():
    from mmx import shapes, synth
    from mmx.llm import LlmEngine, ST_FIN
    sd = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)
    z = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    g = torch.Generator().manual_seed(6)
    B, steps = 4, 14
    lens = [steps, 4, steps, 9]                              # slots 1 and 3 end early (max_len = min_len: no eos needed)
    eng = LlmEngine(sd, dtype=3, max_batch=B, max_ctx=128)
    assert eng.decode_on == "planes"
    xs = [eng.build_lm_input(torch.randint(0, 151936, (1, 5 + b), generator=g).cuda(), z, z) for b in range(B)]
    runs = {}
    old = LlmEngine.skip_finished
    try:
        for skip in (False, True):
            LlmEngine.skip_finished = skip
            eng.close()                                      # the recorded step holds the pointer argument: record again
            eng.start(xs, lens, lens, seed=3, want_logp=True)
            logps, fins = [], []
            for _ in range(steps):
                eng.step()
                logps.append(eng.logp.clone())
                fins.append(eng.state[ST_FIN].tolist())
            runs[skip] = (eng.tokens(), logps, fins)
    finally:
        LlmEngine.skip_finished = old
    (t0, l0, f0), (t1, l1, f1) = runs[False], runs[True]
    assert [len(t) for t in t0] == lens and f0[-1] == [1] * B and f0[5][1] == 1 and f0[5][0] == 0      # slot 1 ended early
    assert t0 == t1 and f0 == f1
    for a, b in zip(l0, l1):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
