"""tts_batch's flow-group scheduler as a plain object: which finished utterances form a flow group, how long a partial group stays
open, which flow worker solves it.  Integers in, groups out (no torch, no streams, no engine): decode steps are the clock, so the
same arrivals give the same schedule - and every worker the same set of captured plans - from run to run (tests/test_sched.py)."""


def groups(order, frames, group_size, max_pad_ratio, frame_quantum, first=0):
    """Consecutive runs of `order` (sorted by length) whose lengths are within the padding budget.
    group_size may be a list: the size limit of the k-th group issued (k counted from `first`); the last entry
    repeats.  A ramp such as [2, 2, 4, 8] lets the flow stage start as soon as the two shortest utterances are
    decoded instead of waiting for eight."""
    sizes = group_size if isinstance(group_size, (list, tuple)) else [group_size]
    out, i = [], 0
    while i < len(order):
        gs = sizes[min(first + len(out), len(sizes) - 1)]
        j, t0 = i + 1, frames[order[i]]
        while j < len(order) and j - i < gs and frames[order[j]] <= max(t0 * max_pad_ratio, t0 + frame_quantum):
            j += 1
        out.append(order[i:j])
        i = j
    return out


class GroupScheduler:
    """One per tts_batch call.  cost: the engine's cost model (ms): a decode step step_ms; a flow group group_ms + frame_ms per frame.
    full_slots: every utterance has a decode slot from the start (B == NS); otherwise the flow stage is the bottleneck: never polite."""

    def __init__(self, group_size, max_pad_ratio, frame_quantum, hold_steps, tail_active, flow_workers, cost, B, full_slots, polite=True):
        self.sizes = group_size if isinstance(group_size, (list, tuple)) else [group_size]
        self.max_pad_ratio, self.frame_quantum = max_pad_ratio, frame_quantum
        self.hold_steps, self.tail_active, self.workers = hold_steps, tail_active, range(flow_workers)
        self.step_ms, self.group_ms, self.frame_ms = cost["step_ms"], cost["group_ms"], cost["frame_ms"]
        self.B, self.polite = B, bool(polite and full_slots)
        self.pending = []                     # finished, not yet issued: in arrival order (never re-sorted across polls)
        self.frames, self.arrived = {}, {}    # per utterance: flow frames, decode step of the poll that saw it finished
        self.issued = 0                       # groups issued so far
        self.free_at = [0.0] * flow_workers   # predicted time (ms on the decode-step clock) each worker finishes its queue
        self.log = []                         # (step, worker, polite, [utterances]) of every group issued

    def arrive(self, b, frames, step):
        """Utterance b has finished with `frames` flow frames (callers keep one poll's arrivals sorted by (tokens, index))."""
        self.pending.append(b)
        self.frames[b], self.arrived[b] = frames, step

    def issue(self, step, remaining, final):
        """The groups to enqueue now, in order, as their log entries (step, worker, polite, [utterances]).  remaining: utterances
        still decoding (or queued); final: the decode loop has ended, nothing is held back."""
        frames, free_at = self.frames, self.free_at
        grps = groups(self.pending, frames, self.sizes, self.max_pad_ratio, self.frame_quantum, first=self.issued)
        now = step * self.step_ms
        if not final and grps:
            want = self.sizes[min(self.issued + len(grps) - 1, len(self.sizes) - 1)]
            waited = step - min(self.arrived[b] for b in grps[-1])
            rush = 0 < remaining <= self.tail_active and any(free_at[w] <= now for w in self.workers)
            if len(grps[-1]) < want and not (self.hold_steps > 0 and waited >= self.hold_steps) and not rush:
                grps = grps[:-1]                             # keep a partial group open for later arrivals
        assign = None
        if final and self.hold_steps > 0 and len(grps) == 1 and len(grps[0]) >= 2:
            # last arrivals: longest first, each to the worker predicted to finish it first (the other worker may
            # still be busy with an earlier group, then splitting only delays the end)
            fa = [max(free_at[w], now) for w in self.workers]
            parts = [[] for _ in self.workers]
            for b in sorted(grps[0], key=lambda b: -frames[b]):
                w = min(self.workers, key=lambda w: (fa[w] + (0.0 if parts[w] else self.group_ms) + self.frame_ms * frames[b], w))
                fa[w] += (0.0 if parts[w] else self.group_ms) + self.frame_ms * frames[b]
                parts[w].append(b)
            assign = [w for w in self.workers if parts[w]]
            grps = [sorted(parts[w], key=lambda b: (frames[b], b)) for w in assign]
        n0 = len(self.log)
        for grp in grps:
            # the worker predicted to be free first.  Prediction, not wall time: decode steps are the clock and a
            # group costs group_ms + frame_ms per frame (fitted to MMX_TIMING=2 traces), so the assignment - and
            # with it every worker's set of captured plans - repeats from run to run
            wi = assign.pop(0) if assign else min(self.workers, key=lambda w: (max(free_at[w], now), w))
            free_at[wi] = max(free_at[wi], now) + self.group_ms + self.frame_ms * sum(frames[b] for b in grp)
            # groups issued while the decode loop is running use the flow kernels' polite tiling (FlowEngine.polite);
            # the last arrivals, issued when it has ended, the fastest one
            self.log.append((step, wi, self.polite and not final, grp))
            self.issued += 1
            for b in grp:
                self.pending.remove(b)
        return self.log[n0:]
