"""The LM engine's own structure (mmx/llm.py): which (build, planes, batch) combinations an engine accepts, the one prompt
entry at the 64-row chunk edge, and what two engines over one LmModel share.  2-layer model, contexts <= 256."""
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, BF16, X3 = 0, 1, 3


@pytest.fixture(scope="module")
def sd():
    from mmx import shapes, synth
    return synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)


def test_engine_refuses_what_no_kernel_serves(sd):
    """fp16 / weight-plane decode packs are read by csrc/decode.hip only (<= 32 sequences, not the round-2 kernel): an engine that
    would hand them to mmx_skinny_gemm - which reads them as one bf16 pack, garbage without an error - is refused at
    construction.  bf16 and fp32 engines of 33..64 sequences run on that kernel as before."""
    from mmx.llm import LlmEngine
    with pytest.raises(ValueError):
        LlmEngine(sd, dtype=X3, max_batch=33)
    with pytest.raises(ValueError):
        LlmEngine(sd, dtype=X3, max_batch=33, lm_planes="bf16x3", wplanes=True)
    with pytest.raises(ValueError):
        LlmEngine(sd, dtype=X3, max_batch=2, wplanes=True, decode_on="skinny")
    LlmEngine.use_v2 = False                           # the same through the class knob the tools set
    try:
        with pytest.raises(ValueError):
            LlmEngine(sd, dtype=X3, max_batch=2, wplanes=True)
    finally:
        LlmEngine.use_v2 = True
    LlmEngine(sd, dtype=F32, max_batch=33, max_ctx=64)
    eng = LlmEngine(sd, dtype=BF16, max_batch=33, max_ctx=64)
    g = torch.Generator().manual_seed(1)
    z = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    xs = [eng.build_lm_input(torch.randint(0, 151936, (1, 3 + b % 4), generator=g).cuda(), z, z) for b in range(33)]
    eng.start(xs, [8] * 33, [8] * 33, seed=2)
    for _ in range(4):
        eng.step()
    drawn = eng.sampled[:, :5]
    assert bool(((drawn >= 0) & (drawn < eng.V)).all()), drawn
    assert all(0 <= t < eng.V for toks in eng.tokens() for t in toks)


def test_prompt_entry_at_the_chunk_edge(sd):
    """Prompts of 2, 64, 65, 66 and 129 rows (one chunk, exactly one, one + a one-row remainder, two + one; fp32 build): the ids
    of 8 steps after start() at batch 1 (prefills L rows) equal those of the same request admit()-ted into slot 1 of a running
    2-slot engine (prefills L - 1 rows, the last row is the next decode step's input), same seed and sequence id."""
    from mmx.llm import LlmEngine
    g = torch.Generator().manual_seed(13)
    z = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    e1 = LlmEngine(sd, dtype=F32, max_batch=1, max_ctx=256)
    e2 = LlmEngine(sd, dtype=F32, max_batch=2, max_ctx=256)
    rows = e1.build_lm_input(torch.randint(0, 151936, (1, 127), generator=g).cuda(), z, z)
    assert rows.shape[0] == 129
    y = e2.build_lm_input(torch.randint(0, 151936, (1, 6), generator=g).cuda(), z, z)
    e2.start([y, y], [100, 1], [100, 1], seed=5)       # slot 0 keeps decoding, slot 1 is idle after its one step
    for L in (2, 64, 65, 66, 129):
        e1.start([rows[:L]], [8], [8], seed=5, seq_ids=[7])
        want = e1.run(8)[0]
        e2.admit(1, rows[:L], 8, 8, seq_id=7)
        for _ in range(8):
            e2.step()
        got = e2.tokens()[1]
        print(f"L = {L}: {want} / {got}")
        assert got == want and 6 <= len(want) <= 8, L


def test_sharing_is_sharing(sd):
    """An engine built with share_from runs on the other engine's model: one KV cache, one page allocator, one set of packs."""
    from mmx.llm import LlmEngine
    big = LlmEngine(sd, dtype=BF16, max_batch=20, max_ctx=128)
    small = LlmEngine(None, dtype=BF16, max_batch=16, max_ctx=128, share_from=big)
    assert small.kc is big.kc and small.vc is big.vc and small.pages is big.pages
    for k, w in big.layers[0].items():
        assert small.layers[0][k].data_ptr() == w.data_ptr(), k
