"""mmx/sched.py, tts_batch's flow-group scheduler, on the CPU: recorded calls replayed (tests/golden/sched.json: the polls of
tts_batch calls and the groups they issued, recorded from the closure the scheduler replaced) and the rules one at a time."""
import json
import os

import pytest

from mmx.sched import GroupScheduler, groups

COST = {"step_ms": 1.0, "group_ms": 40.0, "frame_ms": 0.01}


def load_cases(golden_dir):
    with open(os.path.join(golden_dir, "sched.json")) as f:
        return {c["name"]: c for c in json.load(f)}


def as_lists(log):
    return [[step, wi, pol, list(grp)] for step, wi, pol, grp in log]


def scheduler_of(case):
    a = case["args"]
    return GroupScheduler(a["group_size"], a["max_pad_ratio"], a["frame_quantum"], a["hold_steps"], a["tail_active"], a["flow_workers"],
                          case["sched"], a["B"], a["B"] == a["NS"], a["polite"])


def test_recorded_schedules_replay_exactly(golden_dir):
    """Every recorded call: the polls (step, final, [(utterance, tokens)], still decoding) fed to a fresh scheduler issue exactly
    the recorded (step, worker, polite, group) list - what each issue() returns and the log it leaves."""
    cases = load_cases(golden_dir)
    assert sorted(cases) == ["config4_bf16", "config4_split", "overlapped6", "prompts3", "queue3on1", "queue7on3", "ramp_rush_split"]
    for name, case in cases.items():
        s, plen, got = scheduler_of(case), case["args"]["plen"], []
        for step, final, arrivals, remaining in case["trace"]:
            for b, n_tokens in arrivals:
                s.arrive(b, 2 * (n_tokens + plen[b]), step)
            got += s.issue(step, remaining, final)
        assert as_lists(got) == case["issued"], name
        assert as_lists(s.log) == case["issued"] and not s.pending, name
        assert sorted(b for e in case["issued"] for b in e[3]) == list(range(case["args"]["B"])), name


def test_recorded_cases_cover_the_rules(golden_dir):
    """The fixture is not vacuous: the config-4 share holds partial groups, compares both builds' cost models and ends on the
    last-arrival split or a final flush; the ramp case issues a pair first; the queue cases never use the polite tiling."""
    cases = load_cases(golden_dir)
    c4 = cases["config4_split"]
    assert c4["args"]["B"] == c4["args"]["NS"] == 32 and c4["sched"] != cases["config4_bf16"]["sched"]
    assert any(e[2] for e in c4["issued"]) and not c4["issued"][-1][2]                       # polite beside the loop, not at the end
    assert {e[1] for e in c4["issued"]} == {0, 1}
    assert len(cases["ramp_rush_split"]["issued"][0][3]) <= 2
    assert not any(e[2] for n in ("queue7on3", "queue3on1") for e in cases[n]["issued"])
    assert cases["prompts3"]["args"]["plen"] == [18, 0, 26]


@pytest.mark.parametrize("order,frames,group_size,first,want", [
    ([0, 1, 2, 3], {0: 100, 1: 150, 2: 210, 3: 500}, 8, 0, [[0, 1], [2], [3]]),             # pad ratio 2.0, quantum 32
    ([0, 1], {0: 10, 1: 40}, 8, 0, [[0, 1]]),                                                # the quantum wins over the ratio
    (list(range(7)), {b: 100 for b in range(7)}, [2, 2, 4, 8], 1, [[0, 1], [2, 3, 4, 5], [6]]),   # the ramp, counted from `first`
])
def test_groups(order, frames, group_size, first, want):
    assert groups(order, frames, group_size, 2.0, 32, first=first) == want


def test_hold_then_final():
    """group_size 4, hold 60, 2 workers, every utterance in a slot: a partial group waits until its first member has waited
    hold_steps; the final poll issues what is left, and two groups (the pad ratio keeps 130 and 300 frames apart) are not split."""
    s = GroupScheduler(4, 2.0, 32, 60, 0, 2, COST, 4, True)
    s.arrive(0, 100, 9)
    assert s.issue(9, 3, False) == []
    s.arrive(1, 120, 17)
    for step in range(17, 66, 8):
        assert s.issue(step, 2, False) == [], step
    assert s.issue(73, 2, False) == [(73, 0, True, [0, 1])]                                  # waited 64 >= 60
    assert s.free_at == [73 + 40 + 0.01 * 220, 0.0] and abs(s.free_at[0] - 115.2) < 1e-9
    s.arrive(2, 130, 81)
    assert s.issue(81, 1, False) == []
    s.arrive(3, 300, 90)
    assert s.issue(90, 0, True) == [(90, 1, False, [2]), (90, 0, False, [3])]
    assert s.issued == 3 and s.pending == [] and len(s.log) == 3


def test_final_split_longest_first():
    """One final group of three, both workers free: the longest alone on worker 0, the other two on worker 1."""
    s = GroupScheduler(4, 2.0, 32, 60, 0, 2, COST, 7, True)
    for b, f in ((4, 200), (5, 220), (6, 240)):
        s.arrive(b, f, 100)
    assert s.issue(100, 0, True) == [(100, 0, False, [6]), (100, 1, False, [4, 5])]
    # hold_steps = 0 switches the split off with the hold
    s = GroupScheduler(4, 2.0, 32, 0, 0, 2, COST, 7, True)
    for b, f in ((4, 200), (5, 220), (6, 240)):
        s.arrive(b, f, 100)
    assert s.issue(100, 0, True) == [(100, 0, False, [4, 5, 6])]


@pytest.mark.parametrize("remaining,want", [(3, [(9, 0, True, [0])]), (5, [])])
def test_rush(remaining, want):
    """tail_active 4: with at most 4 utterances still decoding and a worker predicted free, a partial group goes at once."""
    s = GroupScheduler(4, 2.0, 32, 60, 4, 2, COST, 8, True)
    s.arrive(0, 100, 9)
    assert s.issue(9, remaining, False) == want


def test_rush_needs_a_free_worker_and_polite_needs_full_slots():
    s = GroupScheduler(1, 2.0, 32, 60, 4, 1, COST, 8, False)         # B != NS: never polite
    s.arrive(0, 100, 9)
    assert s.issue(9, 7, False) == [(9, 0, False, [0])]              # a full group (size 1); worker busy until 9 + 40 + 1
    s = GroupScheduler(4, 2.0, 32, 60, 4, 1, COST, 8, True)
    s.free_at[0] = 50.0
    s.arrive(1, 100, 17)
    assert s.issue(17, 3, False) == []                               # rush rule: no worker predicted free at 17 ms
    assert s.issue(57, 3, False) == [(57, 0, True, [1])]
