"""How far are the faster builds from the split build, in the codec's own metrics?  (README.)

The benchmark's synthetic checkpoint (bench.build_weights), a handful of utterances of the headline workload's length range.  The
split build generates each utterance's token ids and its audio; the bf16 build, and the bf16 build with fp8 attention in the flow
estimator, then render the SAME ids (token2wav: the flow and the DAC see the tokens the split build drew, so the audio differs by
the build's arithmetic alone).  Printed: mmx.metrics.audio_distance of each build's audio against the split build's, per utterance
and as the mean - mel and stft are the distances the reference's DAC-VAE validation reports, snr_db / sisdr_db the waveform ratios,
stoi / estoi mmx.stoi.stoi (standard and extended) of the same pair: intelligibility on this project's 10 kHz rendering of the 24 kHz
audio (mmx/stoi.py, rule 8), with the split build's audio as the clean signal.

    python tools/build_quality.py [--tokens 75,150,250,400]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "minimax-speech_amd")):
    sys.path.insert(0, p)
import torch
import bench
from mmx import metrics, shapes, stoi, synth
from mmx.pipeline import TtsEngine

KEYS = ("mel", "stft", "l1", "mse", "snr_db", "sisdr_db", "stoi", "estoi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="75,150,250,400", help="decode steps per utterance (25 tokens = 1 s of audio)")
    a = ap.parse_args()
    steps = [int(v) for v in a.tokens.split(",")]
    torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
    llm_sd, flow_sd, dac_sd = bench.build_weights(0)
    g = torch.Generator().manual_seed(2)
    texts = [torch.randint(0, 151936, (1, 48), generator=g).cuda() for _ in steps]
    emb = torch.randn(1, 192, generator=torch.Generator().manual_seed(1)).cuda()

    split = TtsEngine(llm_sd, flow_sd, dac_sd, dtype=2, max_batch=1, max_ctx=640, wplanes="auto")
    ids, ref = [], []
    for t, n in zip(texts, steps):
        ref.append(split.tts(t, emb, seed=0, exact_steps=n).reshape(-1).clone())
        ids.append(torch.tensor(split.llm.tokens()[0], dtype=torch.long).reshape(1, -1).cuda())
    again = [split.token2wav(i, split._prompt(None), split._prompt(None, feat=True), emb).reshape(-1) for i in ids]
    rows = [("split build, the same ids again", again)]
    small_lm = synth.synth_state_dict(shapes.llm_manifest(layers=2), 0)          # these engines only render: their LM is not run
    for name, attn in (("bf16 build", "bf16"), ("bf16 build, fp8 attention", "fp8")):
        eng = TtsEngine(small_lm, flow_sd, dac_sd, dtype=1, max_batch=1, max_ctx=640, attn=attn)
        rows.append((name, [eng.token2wav(i, eng._prompt(None), eng._prompt(None, feat=True), emb).reshape(-1).clone() for i in ids]))
        eng.close()
    print(f"audio_distance and stoi against the split build's audio, {len(steps)} utterances of {steps} tokens ({sum(steps) / 25:.0f} s), teacher-forced ids")
    for name, wavs in rows:
        d = {k: v.cpu() for k, v in metrics.audio_distance(wavs, ref, 24000).items()}
        d["stoi"], d["estoi"] = stoi.stoi(wavs, ref, 24000).cpu(), stoi.stoi(wavs, ref, 24000, extended=True).cpu()
        for i, n in enumerate(steps):
            print(f"  {name:34s} {n:4d} tokens  " + "  ".join(f"{k} {float(d[k][i]):.4g}" for k in KEYS))
        print(f"{name:36s} mean         " + "  ".join(f"{k} {float(d[k].mean()):.4g}" for k in KEYS))
    split.close()


if __name__ == "__main__":
    main()
