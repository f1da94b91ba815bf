"""One timing of STOI: mmx.stoi.stoi - two resample launches, then select, bands, score: six launches - on the
headline batch's 32 mixed-length utterances (2 .. 20 s at 24 kHz, bench.py's seed) as ONE ragged batch, against the same arithmetic
written with torch ops in fp32 / fp64 on the same GPU, clip by clip (the kept frames differ per clip) from the SAME 10 kHz
renderings: frames by unfold, the mask, index_select, overlap-add by index_add_, torch.fft.rfft, the band matrix, the segment
statistics of the standard measure.  Fixed noise clips under a 3 Hz envelope with a silent second; the estimate is the reference plus
noise at a tenth of its level.

    python tools/stoi_timing.py

Each figure is the least of 5 windows of 3 calls after 2 warm-up calls, timed with device events; the two versions are timed one
after the other, not alternated.  Not a speed item: a record beside the parity numbers."""
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "minimax-speech_amd")):
    sys.path.insert(0, p)
import torch
from mmx import stoi as S
from mmx.resample import resample

RATE = 24000
lens = [int(v) * 960 for v in torch.randint(50, 501, (32,), generator=torch.Generator().manual_seed(3))]
g = torch.Generator().manual_seed(5)
ref = []
for n in lens:
    t = torch.arange(n) / RATE
    r = 0.2 * torch.randn(n, generator=g) * (0.55 + 0.45 * torch.sin(2 * math.pi * 3.0 * t))
    r[RATE // 2:RATE // 2 + RATE] *= 1e-4                # a silent second
    ref.append(r.cuda())
est = [r + 0.02 * torch.randn(r.numel(), generator=g).cuda() for r in ref]
L = max(lens)
x, y = torch.zeros(32, L, device="cuda"), torch.zeros(32, L, device="cuda")
for b, n in enumerate(lens):
    x[b, :n], y[b, :n] = est[b], ref[b]
est10, ref10 = resample(est, RATE, S.FS), resample(ref, RATE, S.FS)
win = torch.from_numpy(S.window()).float().cuda()
obm = S.third_octave_table()[:15, :257].float().cuda()


def ours():
    return S.stoi(x, y, RATE, lens=lens)


def ours_10k():
    return S.stoi(est10, ref10, S.FS)


def rebuilt(a, kept):
    fr = a.unfold(0, S.FRAME, S.HOP)[:S.frames_of(a.numel())].index_select(0, kept) * win
    out = torch.zeros((kept.numel() - 1) * S.HOP + S.FRAME, device=a.device)
    idx = (torch.arange(kept.numel(), device=a.device)[:, None] * S.HOP + torch.arange(S.FRAME, device=a.device)[None, :]).reshape(-1)
    return out.index_add_(0, idx, fr.reshape(-1))


def env_of(a):
    fr = a.unfold(0, S.FRAME, S.HOP)[:S.frames_of(a.numel())] * win
    return (obm @ torch.fft.rfft(fr, S.NFFT, dim=1).abs().pow(2).t()).sqrt().double()          # [15, frames]


def torch_ops():
    out = []
    for a, b in zip(est10, ref10):
        fr = b.unfold(0, S.FRAME, S.HOP)[:S.frames_of(b.numel())] * win
        e = 20 * torch.log10(fr.double().norm(dim=1) + S.EPS)
        kept = torch.nonzero(e.max() - S.DYN_RANGE - e < 0).reshape(-1)                       # a host sync per clip: nonzero
        xb, yb = env_of(rebuilt(b, kept)), env_of(rebuilt(a, kept))
        xs, ys = xb.unfold(1, S.SEG, 1), yb.unfold(1, S.SEG, 1)                               # [15, J, 30]
        c = xs.norm(dim=2, keepdim=True) / (ys.norm(dim=2, keepdim=True) + S.EPS)
        yp = torch.minimum(ys * c, xs * (1 + 10 ** (-S.BETA / 20)))
        yp, xc = yp - yp.mean(dim=2, keepdim=True), xs - xs.mean(dim=2, keepdim=True)
        yp, xc = yp / (yp.norm(dim=2, keepdim=True) + S.EPS), xc / (xc.norm(dim=2, keepdim=True) + S.EPS)
        out.append((yp * xc).sum() / (xs.shape[0] * xs.shape[1]))
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
    assert torch.equal(a, ours_10k())
    d, frames = S.stoi(x, y, RATE, lens=lens, return_frames=True)
    print(f"stoi over the 32 clips: {a.min().item():.4f} .. {a.max().item():.4f}; spectral frames {int(frames.min())} .. {int(frames.max())} "
          f"of {min(S.frames_of(v.numel()) for v in ref10)} .. {max(S.frames_of(v.numel()) for v in ref10)}; "
          f"largest |difference| from the torch ops {(a - b).abs().max().item():.2e}")
    print(f"32 clips, {sum(lens) / RATE:.0f} s of audio ({min(lens) / RATE:.1f} .. {max(lens) / RATE:.1f} s)")
    print(f"stoi from 24 kHz (one ragged batch, 6 launches) {least(ours):.3f} ms   from the 10 kHz renderings (4 launches) {least(ours_10k):.3f} ms   "
          f"torch ops from the 10 kHz renderings (clip by clip) {least(torch_ops):.3f} ms")
    print(f"extended, from 24 kHz {least(lambda: S.stoi(x, y, RATE, lens=lens, extended=True)):.3f} ms")
