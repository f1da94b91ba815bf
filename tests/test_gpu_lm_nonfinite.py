"""Logits that are not finite end their sequence loudly (sampler error 3, include/mmx_hip.h) instead of yielding an arbitrary id.

An activation of 65520 or more overflows the fp16 planes of the decode step (hi = inf, lo = -inf, tests/test_lm_planes_host.py),
the MFMA turns that into NaN and the NaN reaches every logit of the sequence.  Ranking NaNs finds no threshold and no candidate;
before error 3 the sampler then read an id out of uninitialised LDS.  Now csrc/sampler.hip tests the log-sum-exp it already
holds: the sequence is marked finished with error 3, nothing is drawn or written, and LlmEngine raises wherever it reads the
finished flags back.  -inf among finite logits stays legal (probability zero)."""
import pytest
import torch

from test_gpu_sampler_table import (DEFAULT, E, EOS, MAX_OUT, Seq, buffers, cases, check_against_oracle, emb, env,  # noqa: F401
                                    launch_tab, standard_seq)

pytestmark = pytest.mark.gpu
V = 6564
NORMAL, FLAGGED, LEGAL = "normal", "flagged", "legal"


def rows_of_every_kind(cases):
    """[(kind, Seq)]: normal rows around an all-NaN row, one +inf, one NaN among finite logits, all -inf, and the legal row with a
    few -inf (its arg-max among them) among finite logits."""
    sp = dict(seed=1234)
    seqs = [(NORMAL, standard_seq(cases, 1, V, sp))]
    q = standard_seq(cases, 2, V, sp)
    q.logits = torch.full((V,), float("nan"))
    seqs.append((FLAGGED, q))
    q = standard_seq(cases, 3, V, sp)
    q.logits[777] = float("inf")
    seqs.append((FLAGGED, q))
    seqs.append((NORMAL, standard_seq(cases, 4, V, sp)))
    q = standard_seq(cases, 6, V, sp)
    q.logits[V - 1] = float("nan")                        # the last id: one thread's last element
    seqs.append((FLAGGED, q))
    q = standard_seq(cases, 7, V, sp)
    q.logits = torch.full((V,), float("-inf"))
    seqs.append((FLAGGED, q))
    q = standard_seq(cases, 8, V, sp)
    q.logits[[int(q.logits.argmax()), 0, 4000, V - 2]] = float("-inf")
    seqs.append((LEGAL, q))
    seqs.append((NORMAL, standard_seq(cases, 9, V, sp)))
    return seqs


def launch_scalar_batch(ops, emb, seqs):
    bf = buffers(seqs, V)
    sp = dict(DEFAULT, seed=1234)
    ops.sample_step(bf["logits"], bf["state"], bf["out_tokens"], emb, bf["next_x"], V=V, B=len(seqs), eos_id=EOS, seed=sp["seed"],
                    top_k=sp["top_k"], top_p=sp["top_p"], win_size=sp["win_size"], tau_r=sp["tau_r"], sampled=bf["sampled"])
    torch.cuda.synchronize()
    return [(int(bf["sampled"][b, s.step]), bf["state"][:, b].tolist(), bf["out_tokens"][b].cpu(), bf["next_x"][b].cpu())
            for b, s in enumerate(seqs)], bf


@pytest.mark.parametrize("entry", ["scalar", "table"])
def test_nonfinite_logits_end_their_own_sequence_only(env, cases, emb, entry):
    """One launch of each entry point over rows of every kind: a flagged row shows finished = 1 and error 3 with pos / step / n_out,
    sampled, out_tokens and next_x untouched; the normal rows and the legal row with -inf logits match the oracle composition and
    carry no error."""
    _, ops = env
    kinds, seqs = zip(*rows_of_every_kind(cases))
    got, bf = launch_tab(ops, emb, list(seqs), V) if entry == "table" else launch_scalar_batch(ops, emb, list(seqs))
    assert kinds.count(FLAGGED) == 4 and kinds.count(LEGAL) == 1
    for b, (kind, s) in enumerate(zip(kinds, seqs)):
        if kind == FLAGGED:
            st = s.state()
            st[3], st[7] = 1, 3
            assert got[b][1] == st, (b, got[b][1])
            assert bool((bf["sampled"][b] == -1).all()) and bool((got[b][3] == -3.0).all()), b
            want_row = torch.full((MAX_OUT,), -7, dtype=torch.int32)
            want_row[:len(s.hist)] = torch.tensor(s.hist, dtype=torch.int32)
            assert torch.equal(got[b][2], want_row), b
        else:
            check_against_oracle(s, got[b], emb, (entry, b))
            assert got[b][1][7] == 0, (b, got[b][1])


# ----------------------------------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def overflow_sd():
    """A checkpoint whose speech embedding carries 2^17 in one channel of every row: past the fp16 planes, well inside fp32."""
    from mmx import shapes, synth
    sd = dict(synth.synth_state_dict(shapes.llm_manifest(layers=2), 0))
    t = sd["speech_embedding.weight"].clone()
    t[:, 200] = 2.0 ** 17
    sd["speech_embedding.weight"] = t
    return sd


def _start(sd, planes, B=2):
    from mmx.llm import LlmEngine
    eng = LlmEngine(sd, dtype=3, max_batch=B, max_ctx=128, use_graphs=False, lm_planes=planes)
    g = torch.Generator().manual_seed(8)
    z = torch.zeros(1, 0, dtype=torch.long, device="cuda")
    xs = [eng.build_lm_input(torch.randint(0, 151936, (1, 6 + b), generator=g).cuda(), z, z) for b in range(B)]
    eng.start(xs, [12] * B, [12] * B, seed=3, want_logp=True)
    return eng


def test_engine_raises_on_fp16_plane_overflow(overflow_sd):
    """lm_planes = "f16x2": the first decode step feeds an embedding row with 2^17 to the planes; run() raises the error that names
    the slot and the way out instead of returning ids.  lm_planes = "bf16x3" decodes the same checkpoint to finite log-probs."""
    from mmx.llm import ST_ERR, ST_FIN
    eng = _start(overflow_sd, "f16x2")
    with pytest.raises(RuntimeError, match=r"slot 0: non-finite logits \(fp16 plane range: lm_planes='bf16x3'\)"):
        eng.run(12)
    assert eng.state[ST_ERR].tolist() == [3, 3] and eng.state[ST_FIN].tolist() == [1, 1]
    eng.close()
    eng = _start(overflow_sd, "bf16x3")
    for _ in range(5):
        eng.step()
        assert bool(torch.isfinite(eng.logp).all())
    toks = eng.run(12)
    assert eng.state[ST_ERR].tolist() == [0, 0] and all(len(t) >= 10 and all(0 <= i < EOS for i in t) for t in toks), toks
    eng.close()
