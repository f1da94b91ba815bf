"""Timing of the channel degradations of mmx.channel: eight clips of 10 s at 24 kHz, each effect alone, beside what a
user would write without the module on the same device tensors - F.pad(mode="replicate") + F.conv1d with the same taps for the
filters, torch.quantile + clamp for the clipping, the reference's own tensor expressions (effects.py:481-486, 514-519, in fp32) for
the quantizers.

    python tools/channel_lab.py [--out FILE]

Two timings per effect, alternated window by window so that drift hits both alike: each figure is the least of 7 windows, a window
long enough to hold at least 50 ms of work, after 3 warm-up calls, timed with device events (the method of tools/degrade_lab.py).
Before timing, the device result of each filter is compared with the torch route in float64 on the CPU (one clip), and the clipping
thresholds with torch.quantile, so that no time is reported for a wrong result.  No GPU: it fails."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "minimax-speech_amd"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np
import torch
import torch.nn.functional as F
from degrade_lab import alternated
from mmx import channel as CH

RATE, B, SECONDS = 24000, 8, 10


def torch_filter(x, taps):
    """Replicate padding and conv1d (a correlation, as julius applies its filters) on a batch [B, N], fp32 or fp64."""
    half = (taps.numel() - 1) // 2
    return F.conv1d(F.pad(x[:, None], (half, half), mode="replicate"), taps[None, None])[:, 0]


def torch_clip(x, q):
    lo, hi = torch.quantile(x, q / 2, dim=-1, keepdim=True), torch.quantile(x, 1 - q / 2, dim=-1, keepdim=True)
    return x.clamp(lo, hi)


def torch_quantization(x, Q):
    return 2 * (((x + 1) / 2 * Q).floor() / Q) - 1


def torch_mulaw(x, Q):
    mu = torch.tensor(Q - 1.0, device=x.device)
    y = torch.sign(x) * torch.log1p(mu * torch.abs(x)) / torch.log1p(mu)
    z = (((y + 1) / 2 * mu + 0.5).to(torch.int64) / mu) * 2 - 1.0
    return torch.sign(z) * (torch.exp(torch.abs(z) * torch.log1p(mu)) - 1.0) / mu


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "channel_lab needs an MI355X: a timing taken elsewhere says nothing"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    N = RATE * SECONDS
    g = torch.Generator().manual_seed(3)
    x = (0.2 * torch.randn(B, N, generator=g)).cuda()
    curve = -np.linspace(0.0, 1.0, 6)
    say(f"{B} clips of {SECONDS} s at {RATE} Hz ({N} samples each), one setting for all")
    say(f"{'effect':<28} {'taps':>6} {'mmx.channel ms':>15} {'torch ms':>10} {'ours/torch':>11} {'check':>10}")
    filters = [("low_pass(8000, zeros=8)", lambda: CH.low_pass(x, 8000, RATE, zeros=8), CH.lowpass_taps(8000, RATE, 8)),
               ("low_pass(4000)", lambda: CH.low_pass(x, 4000, RATE), CH.lowpass_taps(4000, RATE)),
               ("high_pass(100)", lambda: CH.high_pass(x, 100, RATE), CH.highpass_taps(100, RATE)),
               ("equalizer(6 bands)", lambda: CH.equalizer(x, curve, RATE), CH.equalizer_taps(RATE, curve))]
    with torch.no_grad():
        for name, ours, taps in filters:
            td = torch.from_numpy(taps).float().cuda()
            ref = lambda: torch_filter(x, td)
            y64 = torch_filter(x[:1].double().cpu(), torch.from_numpy(taps))
            err = float((ours()[0].double().cpu() - y64[0]).abs().max() / y64.abs().max())
            assert err < 1e-5, (name, err)
            t_ours, t_ref = alternated([ours, ref])
            say(f"{name:<28} {taps.size:6d} {t_ours:15.3f} {t_ref:10.3f} {t_ours / t_ref:11.2f} {err:10.2e}")
        bank = CH.band_taps(RATE, 6)
        bd = torch.from_numpy(bank).float().cuda()
        ours = lambda: CH.mel_filterbank(x, 6, RATE)
        ref = lambda: F.conv1d(F.pad(x[:, None], (bank.shape[1] // 2,) * 2, mode="replicate"), bd[:, None]).permute(0, 2, 1)
        err = float((ours() - ref()).abs().max() / ref().abs().max())
        assert err < 1e-5, err
        t_ours, t_ref = alternated([ours, ref])
        say(f"{'mel_filterbank(6)':<28} {bank.shape[1]:6d} {t_ours:15.3f} {t_ref:10.3f} {t_ours / t_ref:11.2f} {err:10.2e}")
        for q in (0.1,):
            ours, ref = (lambda: CH.clip_distortion(x, q)), (lambda: torch_clip(x, q))
            thr = CH.clip_thresholds(x, q).cpu()
            want = torch.stack([torch.quantile(x.cpu().double(), r, dim=-1) for r in (q / 2, 1 - q / 2)], dim=-1)
            err = float((thr.double() - want).abs().max())
            assert err < 1e-6, err
            t_ours, t_ref = alternated([ours, ref])
            say(f"{f'clip_distortion({q})':<28} {'':>6} {t_ours:15.3f} {t_ref:10.3f} {t_ours / t_ref:11.2f} {err:10.2e}")
        for name, ours, ref in (("quantization(256)", lambda: CH.quantization(x, 256), lambda: torch_quantization(x, 256)),
                                ("mulaw_quantization(256)", lambda: CH.mulaw_quantization(x, 256), lambda: torch_mulaw(x, 256))):
            err = float((ours() - ref()).abs().max())
            t_ours, t_ref = alternated([ours, ref])
            say(f"{name:<28} {'':>6} {t_ours:15.3f} {t_ref:10.3f} {t_ours / t_ref:11.2f} {err:10.2e}   (torch route in fp32)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
