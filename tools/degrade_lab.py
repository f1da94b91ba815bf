"""Timing of the long FIR of mmx.degrade: convolve for a batch of eight 10 s clips at 24 kHz against a 1 s impulse
response (24000 taps), beside the reference's own formulation run by torch on the same device - torch.fft.rfft / irfft of the
signal's length for signal, IR and delta, as dac-vae/audiotools/core/effects.py:105-119 - and the same pair at shorter impulse
responses, which is where the two forms cross.

    python tools/degrade_lab.py [--out FILE]

Three timings per tap count, alternated window by window (ours, ours without mmx_ir_prepare, torch) so that drift hits all alike:
each figure is the least of 7 windows, a window long enough to hold at least 50 ms of work, after 3 warm-up calls, timed with device
events.  The MFMA figures beside them are computed from the shapes: useful MACs N * L' per clip, and the six bf16 products per MAC the
kernel issues (over K = L' + 15 rounded up to 32, and whole 256-output row tiles).  Before timing, the device result at each size is
compared with the reference formulation in float64 (one clip), so that no time is reported for a wrong result.  No GPU: it fails."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "minimax-speech_amd")):
    sys.path.insert(0, p)
import torch
from mmx import degrade as D

RATE, B, SECONDS = 24000, 8, 10
TAPS = (750, 1500, 3000, 6000, 12000, 24000)


def torch_convolve(x, h):
    """effects.py:85-119 on a batch [B, N] with one IR [L] (L <= N), fp32 on the device."""
    N = x.shape[-1]
    hp = torch.nn.functional.pad(h, (0, N - h.numel()))[None]
    idx = hp.abs().argmax(dim=-1)                        # stays on the device: the roll as a gather, no .item()
    hp = torch.gather(hp, 1, (torch.arange(N, device=x.device)[None] + idx[:, None]) % N)
    delta = torch.zeros_like(hp)
    delta[..., 0] = 1
    other_fft = torch.fft.rfft(hp, N)
    y = torch.fft.irfft(other_fft * torch.fft.rfft(x, N), N)
    d = torch.fft.irfft(other_fft * torch.fft.rfft(delta, N), N)
    return y * (1 / d.abs().max(dim=-1, keepdim=True)[0].clamp(1e-5))


def window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternated(fns, windows=7, warm=3, least_ms=50.0):
    calls = []
    for fn in fns:
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        calls.append(max(1, int(least_ms / max(window(fn, 1), 1e-3)) + 1))
    best = [1e9] * len(fns)
    for _ in range(windows):
        for i, fn in enumerate(fns):
            best[i] = min(best[i], window(fn, calls[i]))
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "degrade_lab needs an MI355X: a timing taken elsewhere says nothing"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = RATE * SECONDS
    g = torch.Generator().manual_seed(3)
    x = (0.2 * torch.randn(B, N, generator=g)).cuda()
    lens = [N] * B
    say(f"{B} clips of {SECONDS} s at {RATE} Hz ({N} samples each), one impulse response for all; wrap=True (the reference's circular product)")
    say(f"{'taps':>6} {'convolve ms':>12} {'fir only ms':>12} {'torch fft ms':>13} {'fir/torch':>10} {'useful TMAC/s':>14} {'MFMA TFLOP/s':>13} {'err vs f64':>11}")
    with torch.no_grad():
        for taps in TAPS:
            t = torch.arange(taps, dtype=torch.float64)
            h = (0.2 * torch.randn(taps, generator=g, dtype=torch.float64) * torch.exp(-6.0 * t / taps))
            h[taps // 50] = 1.0
            hd = h.float().cuda()
            prep = D._prepare(hd, None, lens, None, None, True, "degrade_lab")
            ours = lambda: D.convolve(x, hd)
            fir = lambda: D._fir(x, lens, prep, True)
            ref = lambda: torch_convolve(x, hd)
            y, yt = ours(), ref()
            hp = torch.roll(torch.nn.functional.pad(h, (0, N - taps)), -(taps // 50))
            y64 = torch.fft.irfft(torch.fft.rfft(hp, N) * torch.fft.rfft(x[0].double().cpu(), N), N)
            err = float((y[0].double().cpu() - y64).abs().max() / y64.abs().max())
            err_t = float((yt[0].double().cpu() - y64).abs().max() / y64.abs().max())
            assert err < 1e-5 and err_t < 1e-5, (taps, err, err_t)
            t_all, t_fir, t_ref = alternated([ours, fir, ref])
            kp = D.padded_taps(taps)
            tiles = B * -(-N // 256)
            say(f"{taps:6d} {t_all:12.3f} {t_fir:12.3f} {t_ref:13.3f} {t_fir / t_ref:10.2f} {B * N * taps / t_fir / 1e9:14.2f} "
                f"{tiles * 256 * kp * 6 * 2 / t_fir / 1e9:13.1f} {err:11.2e}   (torch route vs f64 {err_t:.2e})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
