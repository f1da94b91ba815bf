"""The sampler kernel (csrc/sampler.hip) where Gaussian logits at V = 6564 never take it: exact ties in value (the stable sort's
index order decides), tied group maxima, probabilities that underflow to 0, small and odd vocabularies, pitched buffers, error 1,
and a candidate list with more takers than it holds.  Expectation everywhere: the oracle composition of Seq.oracle() on the same
Philox noise - ids, state column, out_tokens row and next_x row IDENTICAL, and (through launch_tab / launch_scalar) every word of
every output buffer outside the ones include/mmx_hip.h names bit for bit what it was before the launch.

Every case is first shown DECISIVE in the reference alone (oracle/llm.py draw_undecided, with the case's own mode, top_p, top_k,
win_size and tau_r): no case is skipped, an undecided one fails the test.  Random logits are drawn on a grid of 2^-6 or coarser,
so two log-probs are equal or at least 0.0156 apart by construction; the seeds are such that no running sum passes within 1e-4 of
top_p and no race is closer than 1e-3."""
import pytest
import torch

from test_gpu_sampler_table import (EOS, Seq, check_against_oracle, emb, env, launch_scalar, launch_tab,  # noqa: F401
                                    logp_error)

pytestmark = pytest.mark.gpu
V0 = 6564
RAS = dict(mode=0)
NUCLEUS_WIDE = dict(mode=1, top_p=1.0, top_k=64)
RANDOM = dict(mode=2)
IDS = torch.arange(6656)


# ----------------------------------------------------------------------------------------------------- helpers
def undecided(s):
    from oracle import llm as OL
    sp = s.sp
    return OL.draw_undecided(s.logits.log_softmax(-1), s.hist, lambda k: OL.philox_noise(sp["seed"], s.seq, s.step, k),
                             s.step < s.min_len, s.eos, mode=sp["mode"], top_p=sp["top_p"], top_k=sp["top_k"],
                             win_size=sp["win_size"], tau_r=sp["tau_r"])


def run(ops, emb, seqs, V, scalar=(), **kw):
    """Asserts every case decisive, then runs them through the table entry point (<= 32 per launch) and the RAS ones listed in
    `scalar` through the scalar entry point as well; everything against the oracle."""
    why = [(i, undecided(s)) for i, s in enumerate(seqs)]
    assert all(w is None for _, w in why), [x for x in why if x[1] is not None]
    got = []
    for b0 in range(0, len(seqs), 32):
        got += launch_tab(ops, emb, seqs[b0:b0 + 32], V, **kw)[0]
    for i, s in enumerate(seqs):
        check_against_oracle(s, got[i], emb, ("table", i))
    for i in scalar:
        assert seqs[i].sp["mode"] == 0
        check_against_oracle(seqs[i], launch_scalar(ops, emb, seqs[i], V, **kw), emb, ("scalar", i))
    return got


def on_grid(V, seed, scale, grid):
    return ((torch.randn(V, generator=torch.Generator().manual_seed(seed)) * scale) / grid).round() * grid


def history(s, logits, eos):
    """As oracle/weights.py sampler_cases: s % 13 accepted ids, every third history ending in the arg-max id (the repetition rule
    then sends RAS to the full-vocabulary draw)."""
    g = torch.Generator().manual_seed(500 + s)
    hist = torch.randint(0, eos, (s % 13,), generator=g).tolist() if eos > 0 else []
    if s % 3 == 0 and hist and int(logits.argmax()) < eos:
        hist[-1] = int(logits.argmax())
    return hist


def prefix(s):
    from oracle import llm as OL
    return OL.nucleus_candidates(s.logits.log_softmax(-1), s.sp["top_p"], s.sp["top_k"])


def takers(logits, top_k):
    """How many elements the kernel's list has to take: those at or above the top_k-th largest of the 64 group maxima
    (group = (id % 512) // 8), as tests/test_gpu_sampler_table.py::test_candidate_list_longer_than_512_entries states it."""
    p = logits.log_softmax(-1).softmax(0)
    ids = IDS[:p.numel()]
    gmax = torch.full((64,), -1.0).scatter_reduce(0, (ids % 512) // 8, p, "amax")
    return int((p >= gmax.sort(descending=True).values[top_k - 1]).sum())


# ----------------------------------------------------------------------------------------------------- ties
GRIDS = {"grid 1": (1.0, 2.0), "grid 1/4": (0.25, 4.0)}       # name -> (grid, scale of the Gaussian before rounding)


def tie_cases(grid, scale, sampler):
    seqs = []
    for s in range(32):
        logits = on_grid(V0, 900 + s, scale, grid)
        seqs.append(Seq(logits, history(s, logits, EOS), step=s, ignore_eos=(s % 2 == 0), seq=3, sampler=dict(sampler, seed=77)))
    return seqs


@pytest.mark.parametrize("sampler", [RAS, NUCLEUS_WIDE, RANDOM], ids=["ras", "nucleus64", "random"])
@pytest.mark.parametrize("name", list(GRIDS))
def test_ties_inside_the_nucleus(env, emb, name, sampler):
    """32 rows of logits rounded to a grid, V = 6564: equal probabilities inside the candidate prefix (asserted here: in every row
    of grid 1, in most of grid 1/4), and over the whole row for the full-vocabulary draw that every third history asks for."""
    _, ops = env
    grid, scale = GRIDS[name]
    seqs = tie_cases(grid, scale, sampler)
    if sampler["mode"] != 2:
        tied = sum(bool((prefix(s)[0].diff() == 0).any()) for s in seqs)
        assert tied >= (32 if grid == 1.0 else 24), tied
    run(ops, emb, seqs, V0, scalar=(0, 3, 9) if sampler["mode"] == 0 else ())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", list(GRIDS))
def test_tie_across_the_top_k_cut(env, emb, name, mode):
    """By hand: 27 ids share the largest value, everything else (on the grid) lies far below; top_k = 25, top_p = 1.0.  Sorted
    positions 24, 25 and 26 are equal: index order alone puts a in and b, c out, and a is drawn only through the noise of
    position 24.  The (seq, step) pairs are the first four whose oracle draw IS a and the first four whose draw is not."""
    _, ops = env
    grid = GRIDS[name][0]
    a, b, c = 6143, 6144, 6500                            # a: the last id of round 11, b: the first of round 12
    tied = [5, 64, 199, 511, 512, 1030, 1500, 2047, 2048, 2600, 3010, 3012, 3583, 3584, 4100, 4607, 4608, 5119, 5120, 5700, 5701,
            5900, 6000, 6100, a, b, c]
    logits = on_grid(V0, 950, 1.0, grid).clamp(max=3.0) - 12.0
    logits[tied] = 0.0
    sampler = dict(mode=mode, top_p=1.0, top_k=25, seed=77)
    sv, si = logits.log_softmax(-1).softmax(0).sort(descending=True, stable=True)
    assert float(sv[0]) == float(sv[24]) == float(sv[25]) == float(sv[26]) > float(sv[27]) and si[24:27].tolist() == [a, b, c]
    hit, miss = [], []
    for k in range(300):
        q = Seq(logits, [], step=k % 100, ignore_eos=False, seq=k // 100, sampler=sampler)
        (hit if q.oracle() == a else miss).append(q)
    assert len(hit) >= 4
    got = run(ops, emb, hit[:4] + miss[:4], V0, scalar=(0, 5) if mode == 0 else ())
    assert [g[0] for g in got[:4]] == [a] * 4


def seventy_maxima():
    """The largest value 70 times: one in each of the 64 groups (lane and round drawn at random) and six more."""
    g = torch.Generator().manual_seed(61)
    ids = [8 * grp + int(torch.randint(0, 8, (1,), generator=g)) + 512 * int(torch.randint(0, 12, (1,), generator=g)) for grp in range(64)]
    rest = [i for i in torch.randperm(6144, generator=g).tolist() if i not in ids and i != EOS][:6]
    logits = on_grid(V0, 951, 1.0, 0.25).clamp(max=3.0) - 4.0
    logits[ids + rest] = 0.0
    assert int((logits == logits.max()).sum()) == 70 and len({(i % 512) // 8 for i in ids}) == 64
    return logits


@pytest.mark.parametrize("top_k", [25, 64])
def test_tied_group_maxima(env, emb, top_k):
    """Every group maximum is the same value: the threshold is chosen among equal maxima by index, and the candidates are the
    top_k smallest ids of the 70.  Nucleus and RAS, eight (seq, step) pairs each."""
    _, ops = env
    logits = seventy_maxima()
    seqs = [Seq(logits, history(k, logits, EOS), step=k, ignore_eos=False, seq=5, sampler=dict(mode=k % 2, top_p=1.0, top_k=top_k, seed=77))
            for k in range(16)]
    want = sorted((logits == 0.0).nonzero().flatten().tolist())[:top_k]
    assert prefix(seqs[0])[1].tolist() == want
    run(ops, emb, seqs, V0, scalar=(0, 6))


@pytest.mark.parametrize("V", [6564, 6656])
def test_uniform_row(env, emb, V):
    """All logits equal: every comparison of the selection is a tie, the prefix is ids 0 .. n-1, the full draw runs over V equal p."""
    _, ops = env
    logits = torch.zeros(V)
    seqs = []
    for k in range(12):
        sampler = [RAS, dict(mode=1, top_p=0.8, top_k=25), RANDOM, NUCLEUS_WIDE][k % 4]
        hist = [3, 1, 0, 2] if k % 8 == 0 else []        # RAS, 25 candidates among ids 0..24: a repetition now and then
        seqs.append(Seq(logits, hist, step=k, ignore_eos=(k % 2 == 0), seq=6, sampler=dict(sampler, seed=77)))
    assert prefix(seqs[0])[1].tolist() == list(range(25)) and prefix(seqs[3])[1].tolist() == list(range(64))
    run(ops, emb, seqs, V, scalar=(0, 4, 8))


# ----------------------------------------------------------------------------------------------------- underflow
@pytest.mark.parametrize("peak_on_eos", [False, True])
def test_underflow_to_zero_probability(env, emb, peak_on_eos):
    """Three finite peaks, every other logit 120 below the lowest: their p is exactly 0 and, with top_p = 1.0 and top_k = 25, they
    fill the prefix behind the peaks (the fp32 running sum of the peaks may or may not reach 1.0).  A zero-probability candidate
    is never drawn: every id is one of the peaks."""
    _, ops = env
    peaks = [EOS if peak_on_eos else 4097, 13, 6200]
    logits = torch.full((V0,), -121.25)
    logits[peaks] = torch.tensor([0.0, -0.5, -1.25])
    p = logits.log_softmax(-1).softmax(0)
    assert int((p > 0).sum()) == 3 and float(p[0]) == 0.0
    seqs = []
    for k in range(24):
        hist = [peaks[1 + k % 2]] * 3 if k % 3 == 0 else [17]       # RAS: a repeated peak sends the draw to the full vocabulary
        seqs.append(Seq(logits, hist, step=k, ignore_eos=(not peak_on_eos and k % 2 == 0), seq=7,
                        sampler=dict(mode=k % 3, top_p=1.0, top_k=25, seed=77)))
    got = run(ops, emb, seqs, V0, scalar=(0, 3, 6))
    assert {g[0] for g in got} <= set(peaks) and len({g[0] for g in got}) == 3


# ----------------------------------------------------------------------------------------------------- small and odd V
SMALL_SAMPLERS = [dict(mode=0, top_p=0.8), dict(mode=1, top_p=1.0, top_k=64), RANDOM, dict(mode=0, top_p=0.95, top_k=3, win_size=4, tau_r=0.25),
                  dict(mode=1, top_p=0.9, top_k=5), dict(mode=0, top_p=1.0, top_k=64, win_size=0)]


@pytest.mark.parametrize("V", [1, 2, 7, 8, 63, 64, 65, 100, 511, 512, 513, 1000, 6563])
def test_small_and_odd_vocabularies(env, V):
    """eos_id = V - 1, an embedding of V rows, 18 rows per V in one launch: samplers whose top_k is below V and above V (then
    lim = the number of takers binds and the threshold may be a padding entry), ignore_eos on every other row (V = 1: the only
    id is EOS, ignore_eos stays off)."""
    _, ops = env
    eos = V - 1
    emb_v = torch.randn(V, 896, generator=torch.Generator().manual_seed(6)).cuda()
    seqs = []
    for s in range(18):
        sampler = SMALL_SAMPLERS[s % 6]                   # (top_p = 1.0 takes every id of a small V: keep the last one's p above 1e-4)
        logits = on_grid(V, 900 + s, 0.5 if sampler.get("top_p") == 1.0 else [0.5, 1.0, 2.0][s % 3], 2.0 ** -6)
        seqs.append(Seq(logits, history(s, logits, eos), step=s, ignore_eos=(V > 1 and s % 2 == 0), seq=4, eos=eos,
                        sampler=dict(sampler, seed=77)))
    assert any(q.sp["top_k"] < V for q in seqs) or V <= 3
    assert any(q.sp["top_k"] > V for q in seqs) or V >= 64
    run(ops, emb_v, seqs, V, scalar=(0, 3, 6))


# ----------------------------------------------------------------------------------------------------- pitch and width
def plain_cases(n=8, sampler=RAS):
    seqs = []
    for s in range(n):
        logits = on_grid(V0, 900 + s, [0.5, 2.0, 4.0, 8.0][s % 4], 2.0 ** -6)
        seqs.append(Seq(logits, history(s, logits, EOS), step=s, ignore_eos=(s % 2 == 0), seq=2, sampler=dict(sampler, seed=77)))
    return seqs


@pytest.mark.parametrize("pad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_logits_pitch_above_V(env, emb, pad):
    """V = 6564 logits in rows of 6656: the 92 columns past V hold NaN / +inf and are never read - ids, rows and logp_out are those of
    the contiguous launch bit for bit (a pad value that reached the softmax would end the row with error 3 or show in logp_out)."""
    _, ops = env
    seqs = plain_cases(8) + plain_cases(4, NUCLEUS_WIDE) + plain_cases(4, RANDOM)
    why = [undecided(s) for s in seqs]
    assert why == [None] * len(seqs), why
    ref, bf0 = launch_tab(ops, emb, seqs, V0, logp=True)
    got, bf1 = launch_tab(ops, emb, seqs, V0, logp=True, ldl=6656, pad=pad)
    assert bf1["logits"].shape == (16, 6656) and not bool(torch.isfinite(bf1["logits"][:, V0:]).any())
    for b, s in enumerate(seqs):
        check_against_oracle(s, got[b], emb, b)
        assert got[b][0] == ref[b][0] and got[b][1] == ref[b][1] and got[b][1][7] == 0, b
    assert torch.equal(bf0["logp_out"], bf1["logp_out"]) and bool(torch.isfinite(bf1["logp_out"]).all())
    check_against_oracle(seqs[1], launch_scalar(ops, emb, seqs[1], V0, ldl=6656, pad=pad), emb, "scalar")


@pytest.mark.parametrize("E", [70, 512, 1000])
def test_embedding_width_and_next_x_pitch(env, E):
    """E off 896 - below one pass of the 512-thread embedding copy, exactly one, one and a tail - into next_x rows of pitch E + 24:
    the row is the embedding's, the 24 words behind it keep their bits."""
    _, ops = env
    emb_e = torch.randn(V0, E, generator=torch.Generator().manual_seed(7)).cuda()
    seqs = plain_cases(8)
    got = run(ops, emb_e, seqs, V0, scalar=(1,), ldx=E + 24)
    assert sum(g[0] < EOS for g in got) >= 4              # (rows that did copy an embedding)


# ----------------------------------------------------------------------------------------------------- error 1
def test_error_1_after_101_eos_draws(env, emb):
    """EOS is the only id with non-zero probability and ignore_eos is on: 101 draws give EOS, which llm.py:271-273 answers by
    raising.  The kernel flags error 1 and accepts the id: finished = 1, step + 1, sampled[b][step] = EOS, nothing appended, pos
    and n_out as they were.  All three modes, between neighbours that match the oracle."""
    _, ops = env
    only_eos = torch.full((V0,), -120.0)
    only_eos[EOS] = 0.0
    assert int((only_eos.log_softmax(-1).softmax(0) > 0).sum()) == 1
    stuck = {1: 0, 3: 1, 4: 2}                            # slot -> mode
    plain = plain_cases(8)
    seqs = [Seq(only_eos, [9, 8], step=20 + b, ignore_eos=True, seq=9, sampler=dict(mode=stuck[b], seed=77)) if b in stuck else plain[b]
            for b in range(6)]
    assert all(undecided(s) is None for s in seqs)
    got, bf = launch_tab(ops, emb, seqs, V0)
    for b, s in enumerate(seqs):
        if b in stuck:
            st = s.state()
            st[1], st[3], st[7] = s.step + 1, 1, 1
            assert got[b][0] == EOS and got[b][1] == st, (b, got[b][:2])
            assert got[b][2].tolist() == [9, 8] + [-7] * 126 and bool((got[b][3] == -3.0).all()), b
        else:
            check_against_oracle(s, got[b], emb, b)
            assert got[b][1][7] == 0
    top, st, out_row, nx = launch_scalar(ops, emb, seqs[1], V0)
    assert top == EOS and st[7] == 1 and st[3] == 1 and st[1] == seqs[1].step + 1 and st[0] == seqs[1].pos and st[2] == 2


# ----------------------------------------------------------------------------------------------------- full candidate list
def full_list_row():
    """V = 6564, top_k = 25: the 2496 ids of groups 0..23 ((id % 512) // 8 < 24, i.e. id % 512 < 192) above every other id, so the
    25th group maximum is small and all 2496 are at or above it - 448 more than the list holds.  The 25 largest lie in all 13
    rounds id // 512 and all three waves id % 512 // 64 (every (round, wave) of the last three rounds: whichever takers a
    truncated list drops, nucleus members are among them); the other 2471 share one value."""
    logits = on_grid(V0, 952, 0.5, 2.0 ** -6).clamp(max=1.5) - 3.0
    ids = IDS[:V0]
    logits[ids % 512 < 192] = 2.0
    top = [512 * r + 64 * w + off for r, w, off in
           [(12, 0, 7), (12, 1, 20), (12, 2, 63), (11, 0, 0), (11, 1, 33), (11, 2, 5), (10, 0, 41), (10, 1, 1), (10, 2, 30),
            (9, 0, 9), (9, 1, 50), (9, 2, 12), (8, 2, 2), (8, 0, 60), (8, 1, 17), (7, 1, 8), (7, 2, 44), (6, 0, 3), (5, 2, 21),
            (4, 1, 62), (3, 0, 15), (2, 2, 39), (1, 1, 4), (0, 0, 11), (7, 0, 26)]]
    assert len(set(top)) == 25 and all(i % 512 < 192 for i in top) and {i // 512 for i in top} == set(range(13))
    assert {i % 512 // 64 for i in top} == {0, 1, 2}
    logits[top] = 5.0 + 0.0625 * torch.randperm(25, generator=torch.Generator().manual_seed(8)).float()
    return logits, top


def tied_6000_row():
    """6000 ids of one value above everything else, none of them in group 63: with top_k = 64 the threshold is group 63's small
    maximum and the list would have to hold 6000 entries, nearly the whole vocabulary.  (With top_k = 25 no row can do that: a
    list longer than 2496 needs large values in 25 groups, which lifts the threshold to them.)  The candidates are the 64
    smallest of the 6000 ids."""
    logits = on_grid(V0, 953, 0.5, 2.0 ** -6).clamp(max=1.5) - 3.0
    ids = IDS[:V0]
    free = ids[((ids % 512) // 8 != 63) & (ids != EOS)]
    tied = free[torch.randperm(free.numel(), generator=torch.Generator().manual_seed(9))[:6000]]
    logits[tied] = 2.0
    return logits, sorted(tied.tolist())


@pytest.mark.parametrize("row", ["2496 above", "6000 tied"])
def test_more_takers_than_the_candidate_list_holds(env, emb, row):
    """A valid distribution with more than 2048 elements at or above the top_k-th group maximum (asserted here).  The kernel
    selects the top_k best of the row exactly in that case: the oracle's ids - no error code - for nucleus and RAS, eight (seq,
    step) pairs each, and through the scalar entry point.  Ranking a truncated list instead draws from the wrong set."""
    _, ops = env
    if row == "2496 above":
        (logits, top), top_k = full_list_row(), 25
        assert takers(logits, top_k) >= 2496               # (and the few that tie with the 25th group maximum)
        assert sorted(prefix(Seq(logits, [], 0, False, 0, dict(mode=1, top_p=1.0, top_k=25)))[1].tolist()) == sorted(top)
    else:
        (logits, tied), top_k = tied_6000_row(), 64
        assert takers(logits, top_k) >= 6000
        assert prefix(Seq(logits, [], 0, False, 0, dict(mode=1, top_p=1.0, top_k=64)))[1].tolist() == tied[:64]
    assert takers(logits, top_k) > 2048
    best = int(logits.argmax())
    seqs = [Seq(logits, [], step=k, ignore_eos=False, seq=k, sampler=dict(mode=1, top_p=1.0, top_k=top_k, seed=(5 << 32) | 17))
            for k in range(8)]
    seqs += [Seq(logits, [best if k % 4 == 3 else 17] * 2, step=k, ignore_eos=False, seq=8 + k,    # (k = 3, 7: a repetition may fire)
                 sampler=dict(mode=0, top_p=1.0, top_k=top_k, seed=(5 << 32) | 17)) for k in range(8)]
    got = run(ops, emb, seqs, V0, scalar=(8, 11))
    assert len({g[0] for g in got}) > 4 and all(g[1][7] == 0 for g in got)


# ----------------------------------------------------------------------------------------------------- logp_out
def test_logp_out_against_float64(env, emb):
    """logp_out row by row against float64 log_softmax of the same fp32 logits: rows of the four peakedness levels of
    oracle/weights.py sampler_cases, a tied row (grid 1) and an underflow row.  Rule of the other parity tests here:
    max|logp - f64| <= 4 * max(e_ref, 2^-23 * max|logp64|), e_ref = max|torch fp32 log_softmax - f64| on that row; the second term
    is one fp32 rounding of the row's largest output (test_gpu_sampler_table.py logp_error).
    Measured on MI355X, err / bound per row: 0.074, 0.101, 0.098, 0.111 (peakedness 0.5, 2, 4, 8), 0.127 (tied), 0.034 (underflow);
    errors 3.9e-7 .. 3.1e-6, in four of the six rows the very figure torch's fp32 log_softmax has (e_ref).  The 64 rows of
    tests/test_gpu_kernels.py::test_sampler_matches_oracle under the same rule: at most 0.199."""
    from oracle import weights as W
    _, ops = env
    rows = [lp + 3.7 for lp, _ in W.sampler_cases(4)] + [on_grid(V0, 900, 2.0, 1.0)]
    under = torch.full((V0,), -121.25)
    under[[4097, 13, 6200]] = torch.tensor([0.0, -0.5, -1.25])
    rows.append(under)
    seqs = [Seq(r, [], step=b, ignore_eos=False, seq=1, sampler=dict(seed=77)) for b, r in enumerate(rows)]
    _, bf = launch_tab(ops, emb, seqs, V0, logp=True)
    got = bf["logp_out"].cpu()
    worst = [logp_error(got[b], r, f"row {b}") for b, r in enumerate(rows)]
    assert all(err <= bound for err, bound in worst), worst
