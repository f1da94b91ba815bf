"""Log-probs and token ids of the LM engine over a fixed matrix of builds, batch sizes and modes of operation, as one .npz:
the before / after record of a change that must not alter what the engine computes (same launches, same arguments, same
order -> every array bit-identical).  Only API that has been stable is used: the constructor keywords, build_lm_input,
start(want_logp=True), step, logp, tokens(), run_queue, admit (through run_queue), compact_from, forward_rows,
open_stream / feed / commit.

    python tools/lm_dump.py OUT.npz
    python tools/lm_dump.py --compare A.npz B.npz        # exit status 1 unless every array of A equals its namesake in B

Matrix (2-layer model, max_ctx 256): builds F32, BF16, X3 / f16x2, X3 / bf16x3, X3 with wplanes="auto" on an fp32-kind
checkpoint; batch sizes 1, 3, 20; per (build, batch size) on one engine of that many slots:
  fixed    start + 6 steps, log-probs of every step and the accepted ids
  compact  the same batch, continued from step 3 in a share_from engine of min(B, 16) slots (at 20, four sequences have ended)
  queue    run_queue of 5 requests through the B slots, and once per build through a 2-slot engine (queue2)
  rows     forward_rows of 70 rows, then 5 more behind them
  feed     (one slot) three feed passes: 70 rows, the committed token alone, 3 rows
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimax-speech_amd"))

BUILDS = [("f32", 0, {}, "bf16"), ("bf16", 1, {}, "bf16"), ("x3_f16x2", 3, dict(lm_planes="f16x2"), "bf16"),
          ("x3_bf16x3", 3, dict(lm_planes="bf16x3"), "bf16"), ("x3_fp32ckpt", 3, dict(wplanes="auto"), "fp32")]
BATCHES = (1, 3, 20)
VOCAB = 151936


def ragged(toks):
    out = np.full((len(toks), max([len(t) for t in toks] + [1])), -1, dtype=np.int64)
    for i, t in enumerate(toks):
        out[i, :len(t)] = t
    return out


def dump(dev="cuda"):
    from mmx import shapes, synth
    from mmx.llm import LlmEngine, ST_FIN
    out = {}
    z = torch.zeros(1, 0, dtype=torch.long, device=dev)
    sds = {}
    for name, dt, kw, kind in BUILDS:
        if kind not in sds:
            sds[kind] = synth.synth_state_dict(shapes.llm_manifest(layers=2, vocab=VOCAB), 0, kind=kind)
        g = torch.Generator().manual_seed(5)
        ids = lambda n, hi=VOCAB: torch.randint(0, hi, (1, n), generator=g).to(dev)      # text ids; hi = 6561: speech token ids
        for B in BATCHES:
            eng = LlmEngine(sds[kind], dtype=dt, device=dev, max_batch=B, max_ctx=256, **kw)
            key = f"{name}/B{B}/"
            xs = [eng.build_lm_input(ids(5 + (3 * b) % 7), z, ids(b % 3, 6561)) for b in range(B)]
            lens = [2 if b % 5 == 4 else 12 for b in range(B)]                # at B = 20 four sequences end at step 2

            def fixed(tag, switch):
                eng.start(xs, lens, lens, seed=4, want_logp=True)
                lp, cur = [eng.logp.clone()], eng
                for i in range(6):
                    if switch and i == 2:
                        active = [s_ for s_, f in enumerate(eng.state[ST_FIN].tolist()) if not f]
                        cur = LlmEngine(None, dtype=dt, device=dev, max_batch=min(B, 16), max_ctx=256, share_from=eng)
                        cur.compact_from(eng, active)
                    cur.step()
                    lp.append(cur.logp.clone() if cur is eng else cur.x_in.clone())     # (a compacted engine records no log-probs)
                out[key + tag + "/trace"] = torch.cat([t.reshape(-1) for t in lp]).cpu().numpy()
                out[key + tag + "/ids"] = ragged(cur.tokens())
                if cur is not eng:
                    cur.close()

            fixed("fixed", False)
            fixed("compact", True)
            reqs = [(eng.build_lm_input(ids(4 + i), z, z), n, n) for i, n in enumerate((9, 14, 6, 11, 8))]
            out[key + "queue/ids"] = ragged(eng.run_queue(reqs, seed=6, poll_every=4, ahead=8))
            if B == 1:
                e2 = LlmEngine(sds[kind], dtype=dt, device=dev, max_batch=2, max_ctx=256, **kw)
                out[f"{name}/queue2/ids"] = ragged(e2.run_queue([(e2.build_lm_input(ids(4 + i), z, z), n, n) for i, n in enumerate((9, 14, 6, 11, 8))],
                                                                seed=6, poll_every=4, ahead=8))
                e2.close()
            rows = eng.build_lm_input(ids(73), z, z)
            out[key + "rows/h"] = torch.cat([eng.forward_rows(rows[:70], 0), eng.forward_rows(rows[70:], 70)]).cpu().numpy()
            if B == 1:
                eng.open_stream(seed=3, seq_id=1, want_logp=True)
                lp, toks = [], []
                for x in (rows[:70], None, rows[70:73]):
                    toks.append(eng.feed(x, ignore_eos=True))
                    eng.commit(toks[-1])
                    lp.append(eng.logp.clone())
                out[key + "feed/logp"] = torch.cat(lp).cpu().numpy()
                out[key + "feed/ids"] = np.array(toks, dtype=np.int64)
            eng.close()
            print(f"{key}: done", flush=True)
    return out


def compare(a, b):
    A, B_ = np.load(a), np.load(b)
    bad = [k for k in sorted(set(A.files) | set(B_.files))
           if k not in A.files or k not in B_.files or not torch.equal(torch.from_numpy(A[k]), torch.from_numpy(B_[k]))]
    for k in bad:
        print("DIFFERS" if k in A.files and k in B_.files else "MISSING", k)
    print(f"{len(set(A.files) | set(B_.files))} arrays, {len(bad)} differing")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    ap.add_argument("out", nargs="?")
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    with torch.no_grad():
        np.savez(a.out, **dump())
    print(f"wrote {a.out}")
