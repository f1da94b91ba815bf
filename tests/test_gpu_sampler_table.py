"""Per-sequence samplers and seeds: the sampler kernel's table entry point (mmx_sample_step_tab, csrc/sampler.hip) against the
scalar entry point and against compositions of the CPU oracle's sampling primitives on the same Philox noise (ids IDENTICAL, no
tolerance), then the engine (LlmEngine.start / set_sampler / compact_from / run_queue) and the drop-in (Qwen2LM.sampling) on top
of it."""
import struct
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu
E, EOS, MAX_OUT = 896, 6561, 128
DEFAULT = dict(mode=0, top_p=0.8, top_k=25, win_size=10, tau_r=0.1)


@pytest.fixture(scope="module")
def env():
    from mmx import _lib, ops
    assert torch.cuda.is_available(), "GPU tests need a real MI355X"
    _lib.load()
    return _lib, ops


@pytest.fixture(scope="module")
def cases():
    from oracle import weights as W
    return W.sampler_cases(64)


@pytest.fixture(scope="module")
def emb():
    return torch.randn(6656, E, generator=torch.Generator().manual_seed(5)).cuda()


# ----------------------------------------------------------------------------- helpers
def column(mode=0, top_p=0.8, top_k=25, win_size=10, tau_r=0.1, seed=0):
    """One column of the sampler table as the header defines it, built here without any range check."""
    bits = lambda v: struct.unpack("<i", struct.pack("<f", float(v)))[0]
    i32 = lambda u: u - (1 << 32) if u >= (1 << 31) else u
    return [mode, top_k, win_size, bits(top_p), bits(tau_r), i32(seed & 0xffffffff), i32((seed >> 32) & 0xffffffff), 0]


class Seq:
    """One sequence of a sampler launch: its logits, history, loop state and sampler."""

    def __init__(self, logits, hist, step, ignore_eos, seq, sampler, pos=40, eos=EOS):
        self.logits, self.hist, self.step, self.seq, self.pos, self.eos = logits, list(hist), step, seq, pos, eos
        self.min_len = step + 1 if ignore_eos else 0
        self.sp = dict(DEFAULT, seed=0)
        self.sp.update(sampler)

    def state(self):
        return [self.pos, self.step, len(self.hist), 0, self.min_len, 999, self.seq, 0]

    def oracle(self):
        """llm.py:259-274 around the sequence's own sampler, composed from the oracle's primitives."""
        from oracle import llm as OL
        sp, logp = self.sp, self.logits.log_softmax(-1)
        for trial in range(101):
            noise = OL.philox_noise(sp["seed"], self.seq, self.step, trial)
            if sp["mode"] == 0:
                top = OL.ras_sampling_e(logp, self.hist, noise, sp["top_p"], sp["top_k"], sp["win_size"], sp["tau_r"])
            elif sp["mode"] == 1:
                prob, idx = OL.nucleus_candidates(logp, sp["top_p"], sp["top_k"])
                top = int(idx[OL.multinomial_e(prob, noise(0, prob.numel()))])
            else:
                p = logp.softmax(dim=0)
                top = OL.multinomial_e(p, noise(1, p.numel()))
            if self.step >= self.min_len or top != self.eos:
                return top
        raise AssertionError("the oracle ran out of trials")

    def expected_state(self, top):
        st = self.state()
        if top == self.eos:
            st[1], st[3] = self.step + 1, 1
        else:
            st[0], st[1] = self.pos + 1, self.step + 1
            if top < self.eos:
                st[2] = len(self.hist) + 1
        return st


GUARD = 256                                               # sentinel words on either side of every output buffer


def guarded(shape, dtype, fill):
    """(whole buffer, the view of `shape` in its middle): the style of tests/test_gpu_s3tok.py, with the launch's own fill."""
    n = 1
    for d in shape:
        n *= d
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def buffers(seqs, V, E=E, ldl=None, ldx=None, pad=float("nan"), logp=False):
    """The launch's buffers.  Outputs sit between sentinel words; logits may have a pitch ldl > V (columns V..ldl hold `pad`),
    next_x a pitch ldx > E; logp: a [B, V] logp_out buffer as well."""
    B = len(seqs)
    ldl, ldx = ldl or V, ldx or E
    logits = torch.full((B, ldl), pad)
    logits[:, :V] = torch.stack([s.logits for s in seqs])
    assert logits.shape == (B, ldl) and seqs[0].logits.numel() == V
    raw = {}
    raw["state"], state = guarded((8, B), torch.int32, -12345)
    state.copy_(torch.tensor([s.state() for s in seqs], dtype=torch.int32).t())
    raw["out_tokens"], out_tokens = guarded((B, MAX_OUT), torch.int32, -7)
    for b, s in enumerate(seqs):
        out_tokens[b, :len(s.hist)] = torch.tensor(s.hist, dtype=torch.int32).cuda()
    raw["sampled"], sampled = guarded((B, MAX_OUT), torch.int32, -1)
    raw["next_x"], next_x = guarded((B, ldx), torch.float32, -3.0)
    bf = dict(logits=logits.cuda(), state=state, out_tokens=out_tokens, sampled=sampled, next_x=next_x, logp_out=None, raw=raw,
              dims=(V, E))
    if logp:
        raw["logp_out"], bf["logp_out"] = guarded((B, V), torch.float32, -5.0)
    bf["before"] = {k: v.clone() for k, v in raw.items()}
    return bf


def assert_only_named_words_written(bf, seqs):
    """Every word of every output buffer, its sentinels included, holds the bits it held before the launch - except the words
    include/mmx_hip.h says a step may write: sampled[b][step], out_tokens[b][n_out], next_x[b][:E], logp_out[b][:V] and the
    sequence's 8 state words."""
    V, E = bf["dims"]
    for name, buf in bf["raw"].items():
        may = torch.zeros(buf.numel(), dtype=torch.bool)
        inner = may[GUARD:buf.numel() - GUARD].view(bf[name].shape)
        for b, s in enumerate(seqs):
            if name == "state":
                inner[:, b] = True
            elif name == "sampled":
                inner[b, s.step] = True
            elif name == "out_tokens":
                inner[b, len(s.hist)] = True
            elif name == "next_x":
                inner[b, :E] = True
            else:
                inner[b, :V] = True
        now, was = buf.cpu().view(torch.int32), bf["before"][name].cpu().view(torch.int32)
        bad = (now != was) & ~may
        assert not bool(bad.any()), (name, "written outside its words at", bad.nonzero().flatten()[:8].tolist())


def rows_of(bf, seqs):
    E_ = bf["dims"][1]
    return [(int(bf["sampled"][b, s.step]), bf["state"][:, b].tolist(), bf["out_tokens"][b].cpu(), bf["next_x"][b, :E_].cpu())
            for b, s in enumerate(seqs)]


def launch_tab(ops, emb, seqs, V, cols=None, **kw):
    """One launch of the table entry point over `seqs` -> (sampled id, state column, out_tokens row, next_x row) per sequence.
    kw: the layout arguments of buffers()."""
    B = len(seqs)
    bf = buffers(seqs, V, E=emb.shape[1], **kw)
    cols = [column(**s.sp) for s in seqs] if cols is None else cols
    samp = torch.tensor(cols, dtype=torch.int32).t().contiguous().cuda()
    ops.sample_step_tab(bf["logits"], bf["state"], bf["out_tokens"], emb, bf["next_x"], samp, V=V, B=B, eos_id=seqs[0].eos,
                        sampled=bf["sampled"], logp_out=bf["logp_out"])
    torch.cuda.synchronize()
    assert_only_named_words_written(bf, seqs)
    return rows_of(bf, seqs), bf


def launch_scalar(ops, emb, s, V, **kw):
    bf = buffers([s], V, E=emb.shape[1], **kw)
    sp = s.sp
    ops.sample_step(bf["logits"], bf["state"], bf["out_tokens"], emb, bf["next_x"], V=V, B=1, eos_id=s.eos, seed=sp["seed"],
                    top_k=sp["top_k"], top_p=sp["top_p"], win_size=sp["win_size"], tau_r=sp["tau_r"], sampled=bf["sampled"],
                    logp_out=bf["logp_out"])
    torch.cuda.synchronize()
    assert_only_named_words_written(bf, [s])
    return rows_of(bf, [s])[0]


def check_against_oracle(s, got, emb, tag):
    top, st, out_row, nx = got
    want = s.oracle()
    assert top == want, (tag, top, want)
    assert st == s.expected_state(want), (tag, st)
    if want < s.eos:
        assert int(out_row[len(s.hist)]) == want and torch.equal(nx, emb[want].cpu()), tag
    else:
        assert int(out_row[len(s.hist)]) == -7 and bool((nx == -3.0).all()), tag


def logp_error(got, logits, tag=""):
    """(max|got - f64|, its bound) of one logp_out row against float64 log_softmax of the same fp32 logits.  The bound is the rule of
    the parity tests here, 4 * max(e_ref, 2^-23 * max|logp64|): e_ref is what torch's own fp32 log_softmax misses float64 by on this
    row, the second term one fp32 rounding of the row's largest output (half an ulp of a value below 2^k is at most 2^-24 * 2^k
    < 2^-23 |value|), which is the floor for any fp32 result.  Printed for the record."""
    ref = logits.double().log_softmax(-1)
    e_ref = float((logits.log_softmax(-1).double() - ref).abs().max())
    bound = 4.0 * max(e_ref, 2.0 ** -23 * float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    print(f"logp_out {tag}: err {err:.3e}  e_ref {e_ref:.3e}  bound {bound:.3e}  ratio {err / bound:.3f}")
    return err, bound


def widen(logits, V, s):
    """The case's 6564 logits padded with further random ones up to V (ids above EOS, which the loop skips)."""
    if V == logits.numel():
        return logits
    extra = torch.randn(V - logits.numel(), generator=torch.Generator().manual_seed(100 + s)) * float(logits.std()) + float(logits.mean())
    return torch.cat([logits, extra])


def standard_seq(cases, s, V, sampler):
    """Case s as tests/test_gpu_kernels.py::test_sampler_matches_oracle runs it: EOS dominant on every fifth, ignore_eos on even ones."""
    logp, hist = cases[s]
    logits = widen(logp + 3.7, V, s).clone()
    if s % 5 == 0:
        logits[EOS] = logits.max() + 2.0
    return Seq(logits, hist, step=s, ignore_eos=(s % 2 == 0), seq=3, sampler=sampler)


# ----------------------------------------------------------------------------- 1. table == scalars
@pytest.mark.parametrize("V", [6564, 6656])
def test_table_of_defaults_equals_scalar_launches(env, cases, emb, V):
    """B = 4, every column the engine defaults: sampled, state, out_tokens and next_x bit for bit what four launches of the
    scalar entry point leave (V = 6656 is the kernel's limit: 13 logits for every thread)."""
    _, ops = env
    for s0 in (0, 8, 20, 33):                            # s0 = 0 / 20: EOS-dominant re-draws; 33: repetition history
        seqs = [standard_seq(cases, s0 + i, V, dict(seed=1234)) for i in range(4)]
        got, _ = launch_tab(ops, emb, seqs, V)
        for b, s in enumerate(seqs):
            ref = launch_scalar(ops, emb, s, V)
            assert got[b][0] == ref[0] and got[b][1] == ref[1], (s0, b)
            assert torch.equal(got[b][2], ref[2]) and torch.equal(got[b][3], ref[3]), (s0, b)


# ----------------------------------------------------------------------------- 2. mixed batch
def mixed_batch(cases, V):
    from oracle import llm as OL
    g = torch.Generator().manual_seed(77)

    def eos_dominant(s, sampler):
        # EOS is the most likely id and must be re-drawn (ignore_eos), yet the nucleus holds another candidate to re-draw
        logits = widen(cases[s][0] + 3.7, V, s).clone()
        logits[EOS] = logits.max() + 3.5
        q = Seq(logits, cases[s][1], step=s, ignore_eos=True, seq=20 + s, sampler=sampler)
        prob, idx = OL.nucleus_candidates(logits.log_softmax(-1), q.sp["top_p"], q.sp["top_k"])
        assert int(idx[0]) == EOS and idx.numel() > 1, "case must keep a non-EOS nucleus candidate"
        return q

    seqs = []
    # RAS, defaults, a history that ends in the very id the nucleus draw yields: the repetition fallback fires
    logp, hist = cases[3]
    q = Seq(widen(logp + 3.7, V, 3), hist, step=3, ignore_eos=False, seq=3, sampler=dict(seed=1234))
    prob, idx = OL.nucleus_candidates(q.logits.log_softmax(-1), 0.8, 25)
    q.hist[-1] = int(idx[OL.multinomial_e(prob, OL.philox_noise(1234, 3, 3, 0)(0, prob.numel()))])
    seqs.append(q)
    # nucleus only, the widest one: top_p 1.0, top_k 64, a 64-bit seed
    seqs.append(Seq(widen(cases[4][0], V, 4), cases[4][1], step=11, ignore_eos=False, seq=1,
                    sampler=dict(mode=1, top_p=1.0, top_k=64, seed=(0xDEADBEEF << 32) | 5)))
    # random only, seed with the top bit set
    seqs.append(Seq(widen(cases[9][0], V, 9), cases[9][1], step=2, ignore_eos=False, seq=7, sampler=dict(mode=2, seed=(1 << 63) + 12345)))
    # RAS with top_k 1 and the longest window over a 70-token history that ends in the arg-max id
    h70 = torch.randint(0, 6561, (70,), generator=g).tolist()
    h70[-40] = int(cases[6][0].argmax())
    seqs.append(Seq(widen(cases[6][0], V, 6), h70, step=70, ignore_eos=False, seq=2,
                    sampler=dict(top_p=0.3, top_k=1, win_size=64, tau_r=0.015625, seed=99)))
    # RAS with an empty window (the fallback always fires: 0 >= 0) and 64 candidates
    seqs.append(Seq(widen(cases[12][0], V, 12), cases[12][1], step=5, ignore_eos=False, seq=4,
                    sampler=dict(top_p=0.95, top_k=64, win_size=0, tau_r=0.5, seed=(7 << 32) | 7)))
    # EOS dominant under ignore_eos, one per mode
    seqs.append(eos_dominant(5, dict(mode=1, top_p=0.99, top_k=10, seed=(3 << 32) | 1)))
    seqs.append(eos_dominant(13, dict(mode=2, seed=4321)))
    seqs.append(eos_dominant(21, dict(mode=0, top_p=0.9, top_k=40, win_size=5, tau_r=0.25, seed=(1 << 40) + 3)))
    return seqs


@pytest.mark.parametrize("V", [6564, 6656])
def test_mixed_batch_matches_oracle_in_any_order(env, cases, emb, V):
    """8 sequences in ONE launch, each with its own mode, top_p, top_k, win_size, tau_r and seed: every column equals the oracle
    composition for its own parameters, whatever its neighbours are (two orders)."""
    _, ops = env
    seqs = mixed_batch(cases, V)
    assert len({(s.sp["mode"], s.sp["top_p"], s.sp["top_k"], s.sp["win_size"], s.sp["tau_r"], s.sp["seed"]) for s in seqs}) == len(seqs)
    for order in (list(range(len(seqs))), [5, 2, 7, 0, 3, 6, 1, 4]):
        run = [seqs[i] for i in order]
        got, _ = launch_tab(ops, emb, run, V)
        for b, s in enumerate(run):
            check_against_oracle(s, got[b], emb, (order[b], "slot", b))


def test_candidate_list_longer_than_512_entries(env, emb):
    """top_k = 64 makes the list threshold the SMALLEST of the 64 group maxima (group = (id % 512) // 8).  Here the 600 largest
    logits all sit in 63 of the groups, so more than 512 elements lie above the 64th group's maximum - more than the kernel's
    candidate list once held.  Table (nucleus, RAS) and scalar entry point all equal the oracle."""
    _, ops = env
    V = 6564
    g = torch.Generator().manual_seed(41)
    logits = torch.randn(V, generator=g) * 0.5
    ids = torch.arange(V)
    outside = ids[(ids % 512) // 8 != 63]
    top = outside[torch.randperm(outside.numel(), generator=g)[:600]]
    logits[top] = 3.0 + torch.randn(600, generator=g) * 0.3
    p = logits.log_softmax(-1).softmax(0)
    gmax = torch.full((64,), -1.0).scatter_reduce(0, (ids % 512) // 8, p, "amax")
    assert int((p >= gmax.min()).sum()) > 512
    wide = dict(top_p=1.0, top_k=64, seed=(5 << 32) | 17)
    seqs = [Seq(logits, [], step=k, ignore_eos=False, seq=k, sampler=dict(wide, mode=1)) for k in range(6)] + \
           [Seq(logits, [], step=k, ignore_eos=False, seq=k, sampler=dict(wide, mode=0)) for k in range(6, 8)]
    got, _ = launch_tab(ops, emb, seqs, V)
    for b, q in enumerate(seqs):
        check_against_oracle(q, got[b], emb, b)
    assert len({g_[0] for g_ in got}) > 1                # (different draws: the 64 candidates are nearly equally likely)
    check_against_oracle(seqs[-1], launch_scalar(ops, emb, seqs[-1], V), emb, "scalar")


# ----------------------------------------------------------------------------- 3. modes through the scalar entry point
def test_modes_equal_scalar_ras_limits(env, cases, emb):
    """Mode 1 (nucleus only) is scalar RAS whose repetition threshold is never reached (tau_r = 1e30), mode 2 (random only) is
    scalar RAS with an empty window (win_size = 0: 0 >= 0, the fallback always fires and draws stream 1): identical ids, 64 cases."""
    _, ops = env
    V = 6564
    for mode, limit in ((1, dict(tau_r=1e30)), (2, dict(win_size=0))):
        seqs = [standard_seq(cases, s, V, dict(mode=mode, seed=1234)) for s in range(64)]
        got = launch_tab(ops, emb, seqs[:32], V)[0] + launch_tab(ops, emb, seqs[32:], V)[0]
        for s in range(64):
            ref = launch_scalar(ops, emb, standard_seq(cases, s, V, dict(seed=1234, **limit)), V)
            assert got[s][0] == ref[0] and got[s][1] == ref[1], (mode, s)
            assert torch.equal(got[s][2], ref[2]) and torch.equal(got[s][3], ref[3]), (mode, s)


# ----------------------------------------------------------------------------- 4. bad columns
def test_bad_column_stops_its_own_sequence_only(env, cases, emb):
    """A column out of range (top_k = 0; mode = 7) gets error 2 and `finished`, and nothing of it is drawn or written; the good
    columns of the same launch still match the oracle."""
    _, ops = env
    V = 6564
    seqs = [standard_seq(cases, s, V, dict(seed=50 + s)) for s in (1, 2, 3, 4, 7)]
    cols = [column(**s.sp) for s in seqs]
    cols[1] = column(**dict(seqs[1].sp, top_k=0))
    cols[3] = column(**dict(seqs[3].sp, mode=7))
    got, bf = launch_tab(ops, emb, seqs, V, cols=cols)
    for b, s in enumerate(seqs):
        if b in (1, 3):
            st = s.state()
            st[3], st[7] = 1, 2
            assert got[b][1] == st, (b, got[b][1])
            assert bool((bf["sampled"][b] == -1).all()) and bool((got[b][3] == -3.0).all())
            want_row = torch.full((MAX_OUT,), -7, dtype=torch.int32)
            want_row[:len(s.hist)] = torch.tensor(s.hist, dtype=torch.int32)
            assert torch.equal(got[b][2], want_row)
        else:
            check_against_oracle(s, got[b], emb, b)
    for bad in (dict(top_k=65), dict(win_size=65), dict(win_size=-1), dict(mode=-1), dict(mode=3)):
        col = column(**dict(seqs[0].sp, **bad))
        got, _ = launch_tab(ops, emb, seqs[:1], V, cols=[col])
        assert got[0][1][3] == 1 and got[0][1][7] == 2, bad
    with pytest.raises(ValueError):
        ops.sampler_column(top_k=0)
    assert ops.sampler_column(mode="nucleus", top_p=0.7, top_k=12, win_size=3, tau_r=0.2, seed=(1 << 63) + 5) == \
        column(mode=1, top_p=0.7, top_k=12, win_size=3, tau_r=0.2, seed=(1 << 63) + 5)


# ----------------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def lm_sd():
    from mmx import shapes, synth
    return synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)


def _texts(n, length, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 151936, (1, length), generator=g) for _ in range(n)]


Z = torch.zeros(1, 0, dtype=torch.long)


def _oracle_ids(lm_sd, text, seed, seq, steps):
    from oracle import llm as OL
    return OL.lm_inference(lm_sd, OL.QwenCfg(layers=2), text, Z, Z, seed=seed, seq=seq, max_steps=steps)


def test_engine_per_sequence_seeds_match_oracle(lm_sd):
    """B = 4, four seeds (one 64-bit): every sequence's free-running ids are the CPU oracle's under ITS seed (fp32 build)."""
    from mmx.llm import LlmEngine
    texts, seeds, steps = _texts(4, 8, 31), [11, 5, (9 << 32) | 2, 1234567], 14
    eng = LlmEngine(lm_sd, dtype=0, max_batch=4, max_ctx=256)
    xs = [eng.build_lm_input(t.cuda(), Z.cuda(), Z.cuda()) for t in texts]
    eng.start(xs, [16] * 4, [160] * 4, seeds=seeds)
    got = eng.run(steps)
    for b in range(4):
        assert got[b] == _oracle_ids(lm_sd, texts[b], seeds[b], b, steps), b
    eng.close()


def test_new_seed_and_new_parameters_reuse_the_captured_step(lm_sd):
    """Two start() calls with different seeds replay the SAME recorded decode step and both match the oracle; after capture,
    set_sampler(slot, top_k=1) takes effect on the very next step: the id is the arg-max of that step's log-probs (where RAS's
    repetition rule fires on the arg-max id, common.py:113-115, it is the oracle's full-vocabulary draw)."""
    from mmx.llm import LlmEngine
    from oracle import llm as OL
    text, steps = _texts(1, 8, 32)[0], 12
    eng = LlmEngine(lm_sd, dtype=0, max_batch=1, max_ctx=256)
    x = eng.build_lm_input(text.cuda(), Z.cuda(), Z.cuda())
    eng.start([x], [16], [160], seed=3, want_logp=True)
    assert eng.run(steps)[0] == _oracle_ids(lm_sd, text, 3, 0, steps)
    recorded = eng._decode
    assert recorded is not None
    eng.start([x], [16], [160], seed=(1 << 40) + 9, want_logp=True)
    assert eng._decode is recorded
    assert eng.run(steps)[0] == _oracle_ids(lm_sd, text, (1 << 40) + 9, 0, steps)
    assert eng._decode is recorded
    eng.start([x], [40], [160], seed=5, want_logp=True)
    for _ in range(3):
        eng.step()
    eng.set_sampler(0, top_k=1)
    greedy = 0
    for i in range(4, 20):
        hist = eng.tokens()[0]
        eng.step()
        logp = eng.logp[0].cpu()
        top, got = int(logp.argmax()), int(eng.sampled[0, i])
        assert top != EOS
        if top in hist[-10:]:
            assert got == OL.ras_sampling_e(logp, hist, OL.philox_noise(5, 0, i, 0), 0.8, 1, 10, 0.1), i
        else:
            assert got == top, (i, got, top)
            greedy += 1
    assert greedy >= 4 and eng._decode is recorded
    with pytest.raises(ValueError):
        eng.set_sampler(0, top_k=0)
    eng.close()


MIXED = [None, dict(mode=1, top_p=0.9, top_k=40), dict(mode=2), dict(top_k=3, win_size=4, tau_r=0.25), dict(mode="nucleus", top_k=1),
         dict(top_p=0.5)]


def test_compaction_keeps_every_survivors_sampler(lm_sd):
    """A 6-sequence batch with six samplers and six seeds continues in a 4-slot engine once <= 4 are active: the same tokens as
    without compaction (the pattern of tests/test_gpu_llm.py::test_compaction_to_smaller_batch_preserves_tokens)."""
    from mmx.llm import LlmEngine, ST_FIN, ST_NOUT
    B = 6
    lens = [5, 19, 9, 23, 14, 21]
    seeds = [4, 40, (5 << 32) | 1, 7, 7, 1 << 35]
    big = LlmEngine(lm_sd, dtype=1, max_batch=B, max_ctx=128)
    small = LlmEngine(None, dtype=1, max_batch=4, max_ctx=128, share_from=big)
    xs = [big.build_lm_input(t.cuda(), Z.cuda(), Z.cuda()) for t in _texts(B, 5, 33)]
    big.start(xs, lens, lens, samplers=MIXED, seeds=seeds)
    ref = big.run(max(lens))
    big.start(xs, lens, lens, samplers=MIXED, seeds=seeds)
    out = [None] * B
    eng, slots, done = big, list(range(B)), 1
    while done < max(lens):
        eng.step()
        done += 1
        fin, n = eng.state[ST_FIN].tolist(), eng.state[ST_NOUT].tolist()
        for s_, b in enumerate(slots):
            if fin[s_] and out[b] is None:
                out[b] = eng.out_tokens[s_, :n[s_]].tolist()
        active = [s_ for s_, b in enumerate(slots) if out[b] is None]
        if eng is big and 0 < len(active) <= 4:
            small.compact_from(big, active)
            eng, slots = small, [slots[s_] for s_ in active]
    n = eng.state[ST_NOUT].tolist()
    for s_, b in enumerate(slots):
        if out[b] is None:
            out[b] = eng.out_tokens[s_, :n[s_]].tolist()
    assert eng is small and out == ref
    assert len({tuple(t) for t in ref}) == B
    big.close()
    small.close()


def test_run_queue_with_per_request_samplers_and_seeds(lm_sd):
    """6 requests through a 2-slot engine, each with its own seed and sampler: per request, what it yields alone at B = 1 with
    that seed, sampler and sequence id (fp32 build)."""
    from mmx.llm import LlmEngine
    lens = [9, 20, 6, 15, 12, 8]
    seeds = [6, 60, (2 << 32) | 6, None, 8, 1 << 33]
    texts = _texts(6, 5, 34)
    e1 = LlmEngine(lm_sd, dtype=0, max_batch=1, max_ctx=128)
    want = []
    for i, (t, n) in enumerate(zip(texts, lens)):
        e1.start([e1.build_lm_input(t.cuda(), Z.cuda(), Z.cuda())], [n], [n], seed=(21 if seeds[i] is None else seeds[i]), seq_ids=[i],
                 samplers=[MIXED[i]])
        want.append(e1.run(n)[0])
    e1.close()
    eng = LlmEngine(lm_sd, dtype=0, max_batch=2, max_ctx=128)
    reqs = [(eng.build_lm_input(t.cuda(), Z.cuda(), Z.cuda()), n, n, MIXED[i], seeds[i]) for i, (t, n) in enumerate(zip(texts, lens))]
    for rep in range(2):
        assert eng.run_queue(reqs, seed=21, poll_every=4, ahead=8) == want, rep
    eng.close()


# ----------------------------------------------------------------------------- drop-in
def _dropin_lm(lm_sd, sampling):
    from cosyvoice.llm.llm import Qwen2Encoder, Qwen2LM
    lm = Qwen2LM(896, 896, 6561, Qwen2Encoder({"num_hidden_layers": 2}), sampling)
    lm.load_state_dict(lm_sd, strict=True)
    lm = lm.to("cuda")
    lm.compute_dtype = 0
    lm.seed = 4
    return lm


def _inference(lm, text):
    z = Z.cuda()
    i32 = lambda n: torch.tensor([n], dtype=torch.int32, device="cuda")
    return list(lm.inference(text=text.cuda(), text_len=i32(text.shape[1]), prompt_text=z, prompt_text_len=i32(0), prompt_speech_token=z,
                             prompt_speech_token_len=i32(0), embedding=torch.zeros(1, 192, device="cuda")))


def test_dropin_nucleus_sampling_runs_mode_1(lm_sd):
    """Qwen2LM(sampling=nucleus_sampling).inference yields the ids of the engine run in mode 1 - not RAS's."""
    from cosyvoice.utils.common import nucleus_sampling
    from mmx.llm import LlmEngine
    text = _texts(1, 7, 35)[0]
    lm = _dropin_lm(lm_sd, partial(nucleus_sampling, top_p=0.9, top_k=12))
    got = _inference(lm, text)
    eng = LlmEngine(lm_sd, dtype=0, max_batch=1, max_ctx=2048)
    x = eng.build_lm_input(text.cuda(), Z.cuda(), Z.cuda())
    eng.start([x], [14], [140], seed=4, samplers=[dict(mode=1, top_p=0.9, top_k=12)])
    want = eng.run(140)[0]
    eng.close()
    assert got == want and 12 <= len(got) <= 140
    col = lm.engine(1)._samp_host[0]
    assert (col["mode"], col["top_p"], col["top_k"]) == (1, 0.9, 12)


class Recording:
    """A `sampling` callable the device does not know: records what it is called with and returns a scripted id."""

    def __init__(self, script):
        self.script, self.calls = script, []

    def __call__(self, weighted_scores, decoded_tokens, sampling):
        self.calls.append((weighted_scores.detach().float().cpu().clone(), list(decoded_tokens), sampling))
        return torch.tensor(self.script[len(self.calls) - 1])


@pytest.fixture(scope="module")
def scripted(lm_sd):
    """(text, the ids the callable returns call by call, the id every step settles on, the oracle's log-probs of every step when
    those ids are fed back).  Step 0 and step 6 settle on ids above EOS (llm.py:755-756: not yielded, the same input is fed
    again - at step 0 that is the whole prompt); at step 3 (< min_len = 14) the callable first returns EOS and is asked again."""
    from oracle import llm as OL
    text = _texts(1, 7, 36)[0]
    steps = torch.randint(0, 6561, (18,), generator=torch.Generator().manual_seed(9)).tolist() + [EOS]
    steps[0], steps[6] = 6563, 6562
    calls = steps[:3] + [EOS] + steps[3:]
    ref = []
    OL.lm_inference(lm_sd, OL.QwenCfg(layers=2), text, Z, Z, seed=0, seq=0, forced=steps, max_steps=len(steps), record=ref)
    assert len(ref) == len(steps)
    return text, calls, steps, ref


@pytest.mark.parametrize("entry", ["inference", "inference_wrapper"])
def test_dropin_calls_an_unknown_sampler_on_the_host(lm_sd, scripted, entry):
    """Any other callable is called at every step, as llm.py:745-760 with :259-274 calls it: with the step's log-probs (the CPU
    oracle's teacher-forced ones, to the fp32 log-prob tolerance of tests/test_gpu_llm.py) and the ids yielded so far; once per
    step, and once more where it returns EOS under ignore_eos; what it returns is what the generator yields, ids above EOS
    left out, up to the EOS it returns at the end."""
    text, calls, steps, ref = scripted
    rec = Recording(calls)
    lm = _dropin_lm(lm_sd, rec)
    if entry == "inference":
        got = _inference(lm, text)
    else:
        x = lm.engine(1).build_lm_input(text.cuda(), Z.cuda(), Z.cuda()).unsqueeze(0)
        got = list(lm.inference_wrapper(x, 25, 14, 140, "u"))
    assert got == [t for t in steps if t < EOS]
    assert len(rec.calls) == len(calls)
    step_of_call = [0, 1, 2, 3] + list(range(3, len(steps)))
    for c, (logp, decoded, sampling) in enumerate(rec.calls):
        i = step_of_call[c]
        assert decoded == [t for t in steps[:i] if t < EOS] and sampling == 25, c
        assert (logp - ref[i]).abs().max().item() < 2e-3, (c, i)
