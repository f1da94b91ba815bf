"""One timing of the audio distances: mmx.metrics.audio_distance - seven mel scales, two STFT scales, the waveform
sums, 20 launches - on the headline batch's 32 mixed-length utterances (2 .. 20 s at 24 kHz, bench.py's seed) as ONE ragged batch,
against the same quantities written with torch.stft / torch.matmul in fp32 on the same GPU (clip by clip: the lengths differ, and a
padded torch.stft would reflect at the wrong sample).  Fixed noise clips; the estimate is the reference plus 3e-3 noise.

    python tools/metrics_timing.py

Each figure is the least of 5 windows of 3 calls after 2 warm-up calls, timed with device events; the two versions are timed one
after the other, not alternated.  Not a speed item: a record beside the parity numbers."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "minimax-speech_amd")):
    sys.path.insert(0, p)
import torch
from mmx import metrics as M
from mmx.mel import mel_filterbank

RATE = 24000
lens = [int(v) * 960 for v in torch.randint(50, 501, (32,), generator=torch.Generator().manual_seed(3))]
g = torch.Generator().manual_seed(5)
ref = [(0.2 * torch.randn(n, generator=g)).cuda() for n in lens]
est = [r + 3e-3 * torch.randn(r.numel(), generator=g).cuda() for r in ref]
L = max(lens)
x, y = torch.zeros(32, L, device="cuda"), torch.zeros(32, L, device="cuda")
for b, n in enumerate(lens):
    x[b, :n], y[b, :n] = est[b], ref[b]
win = {w: torch.hann_window(w, device="cuda") for w in M.MEL_WINDOWS}
fbs = {w: torch.from_numpy(mel_filterbank(RATE, w, m)).cuda() for w, m in zip(M.MEL_WINDOWS, M.MEL_N_MELS)}


def ours():
    return M.audio_distance(x, y, RATE, lens=lens)


def mag(a, w):
    return torch.stft(a, w, w // 4, window=win[w], center=True, return_complex=True).abs()


def torch_ops():
    out = []
    for a, b in zip(est, ref):
        mel = stft = 0.0
        for w in M.MEL_WINDOWS:
            ma, mb = mag(a, w), mag(b, w)
            if w in M.VALIDATION_STFT_WINDOWS:
                stft = stft + (ma.clamp(1e-5).pow(2).log10() - mb.clamp(1e-5).pow(2).log10()).abs().mean() + (ma - mb).abs().mean()
            mel = mel + ((fbs[w] @ ma).clamp(1e-5).log10() - (fbs[w] @ mb).clamp(1e-5).log10()).abs().mean()
        d = a - b
        out.append(torch.stack([mel, stft, d.abs().mean(), (d * d).mean()]))
    return torch.stack(out)


def least(fn, windows=5, calls=3, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) / calls)
    return best


with torch.no_grad():
    a, b = ours(), torch_ops()
    for k, col in (("mel", 0), ("stft", 1), ("l1", 2), ("mse", 3)):
        rel = ((a[k] - b[:, col].double()).abs() / b[:, col].double()).max().item()
        print(f"{k}: largest relative difference from the fp32 torch ops over the 32 clips {rel:.2e}")
    print(f"32 clips, {sum(lens) / RATE:.0f} s of audio ({min(lens) / RATE:.1f} .. {max(lens) / RATE:.1f} s)")
    print(f"audio_distance (one ragged batch, 20 launches) {least(ours):.3f} ms   torch ops (fp32, clip by clip) {least(torch_ops):.3f} ms")
    print(f"mel_distance alone {least(lambda: M.mel_distance(x, y, RATE, lens=lens)):.3f} ms   "
          f"stft [1024, 2048] alone {least(lambda: M.stft_distance(x, y, lens=lens, window_lengths=M.VALIDATION_STFT_WINDOWS)):.3f} ms   "
          f"waveform sums alone {least(lambda: M.waveform_distance(x, y, lens=lens)):.3f} ms")
