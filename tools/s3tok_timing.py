"""One timing of the speech tokenizer: a 4 s clip -> tokens at full size (1280, 20, 6) on the split build
(SpeechTokenizerEngine.tokenize), against the same encoder written with torch ops in fp32 on the same GPU (torch.stft, the
restatement of tests/test_s3tok_host.py run on the device).  Synthetic weights (mmx.synth, seed 1), a fixed noise clip.

    python tools/s3tok_timing.py

Each figure is the least of 20 calls after 3 warm-up calls; a call's window ends in a device synchronise.  The two versions
are timed one after the other, not alternated.  Not a speed item: a record beside the parity numbers."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "minimax-speech_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch
import test_s3tok_host as R
from mmx import shapes, synth
from mmx.s3tok import LogMelW, SpeechTokenizerEngine

torch.set_num_threads(max(1, min(len(os.sched_getaffinity(0)), 16)))
sd = synth.synth_state_dict(shapes.s3tok_manifest(), 1)
g = torch.Generator().manual_seed(3)
w = (0.3 * torch.randn(64000, generator=g)).cuda()
eng = SpeechTokenizerEngine(sd, dtype=2)
sd_gpu = {k: v.cuda() for k, v in sd.items()}
fb = torch.from_numpy(LogMelW().filterbank).cuda()
win = torch.hann_window(400).cuda()

def ours():
    return eng.tokenize([w])[0]

def torch_ops():
    st = torch.stft(w, 400, 160, window=win, return_complex=True)
    mel = fb @ (st[..., :-1].abs() ** 2)
    ls = torch.clamp(mel, min=1e-10).log10()
    ls = (torch.maximum(ls, ls.max() - 8.0) + 4.0) / 4.0
    v = R.encode_ref(sd_gpu, ls[None], [ls.shape[1]], torch.float32)[0]
    return (R.digits_of(v) * (3 ** torch.arange(8, device=v.device))).sum(-1)[0]

def least(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(n):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3

with torch.no_grad():
    a, b = ours(), torch_ops()
    print("tokens", a.numel(), "ids differing from the torch-op encoder:", int((a.cpu().long() != b.cpu()).sum()))
    print(f"engine (split build) {least(ours):.3f} ms   torch ops (fp32) {least(torch_ops):.3f} ms")
    def mel_only():
        return LogMelW()(w)
    print(f"mmx_logmel_w alone {least(mel_only):.3f} ms")
