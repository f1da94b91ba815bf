"""Times the DAC-VAE encoder and decoder engines on synthetic weights: ms per call and audio-s/s.

    python tools/time_dac.py            encoder + decoder, bf16 build (B = 1 and 8 clips of 10 s)
    python tools/time_dac.py encoder    the encoder leg: one 10 s clip (encode) and a ragged batch of 16 clips of 3 - 10 s
                                        (encode_ragged), fuse_ru off and on, bf16 and split builds

The encoder leg alternates the unfused and the fused engine inside every repeat (other work shares the machine: a drift hits
both), warms every shape first, times device-synchronised windows of `inner` calls and reports the median and the min .. max of
`reps` windows.  Beside the times it prints what the two forms launch and, from dac_ru_lds of csrc/fused.hip, the LDS a fused
workgroup holds - the numbers DESIGN.md 4.3 and profiles/README.md quote."""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimax-speech_amd"))
from mmx import shapes, synth  # noqa: E402
from mmx.dac import DacDecoderEngine, DacEncoderEngine  # noqa: E402

ENC_RATES = [2, 3, 4, 4, 5]
# default tiles of mmx_dac_ru for the encoder's fused stages (dac_ru_select in csrc/fused.hip): {dtype: {C: rows}}
FUSED_BM = {1: {64: 128, 128: 128}, 2: {64: 64, 128: 64}}


def timeit(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def dac_ru_lds(C, bm, ns, dil):
    """csrc/fused.hip dac_ru_lds: bytes of LDS of one fused workgroup (ns = 2: the split build's hi + lo planes)."""
    cp = (C + 31) // 32 * 32
    pa = (((cp * 2 + 31) // 32) | 1) * 32
    patch = 16 * ((48 if C % 48 == 0 else 64) + 4)
    return ns * ((bm + 6 * dil) * pa + bm * pa) + 4 * patch * 4 + 8 * cp * 4


def encoder_launches(fused):
    """Kernel launches of one encode: head, 3 units per block (2 GEMMs, or 1 fused kernel at C = 64 / 128), 5 strided convs, the two
    closing convs, the VAE sampling kernel and 3 layout copies (+ 1 noise copy when the draw is given)."""
    units = sum(3 * (1 if fused and c in DacEncoderEngine.FUSED_RU_C else 2) for c in (64, 128, 256, 512, 1024))
    return 1 + units + 5 + 2 + 1 + 3


def windows(fns, reps, inner):
    """fns: {name: callable}.  Every repeat times each name's window of `inner` calls in turn -> {name: [ms per call]}."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t0) / inner * 1e3)
    return out


def encoder_leg(reps=7, inner=10):
    sd = synth.synth_state_dict(shapes.dac_encoder_manifest(80), 0)
    g = torch.Generator().manual_seed(0)
    one = (0.3 * torch.randn(1, 1, 240000, generator=g)).cuda()
    secs = [3.0 + 7.0 * i / 15 for i in range(16)]                       # 16 clips, 3 .. 10 s
    clips = [(0.3 * torch.randn(int(s * 24000), generator=g)).cuda() for s in secs]
    print(f"launches per encode: unfused {encoder_launches(False)}, fused {encoder_launches(True)}")
    for dt, name in ((1, "bf16"), (2, "split")):
        ns = 2 if dt == 2 else 1
        for C in (64, 128):
            bm = FUSED_BM[dt][C]
            print(f"{name} C {C}: {bm}-row tile, LDS per workgroup " + ", ".join(f"dil {d}: {dac_ru_lds(C, bm, ns, d)} B" for d in (1, 3, 9)))
        engs = {f: DacEncoderEngine(sd, ENC_RATES, dtype=dt, fuse_ru=f) for f in (False, True)}
        for what, total, mk in (("1 x 10 s (encode)", 10.0, lambda e: (lambda: e.encode(one))),
                                (f"16 x 3-10 s ragged, {sum(secs):.0f} s (encode_ragged)", sum(secs), lambda e: (lambda: e.encode_ragged(clips)))):
            res = windows({"unfused": mk(engs[False]), "fused": mk(engs[True])}, reps, inner)
            med = {k: statistics.median(v) for k, v in res.items()}
            print(f"{name} {what}: " + "  ".join(f"{k} {med[k]:.3f} ms (min {min(v):.3f} max {max(v):.3f}; {total / med[k] * 1e3:.0f} audio-s/s)"
                                                    for k, v in res.items()) + f"  fused / unfused {med['fused'] / med['unfused']:.3f}", flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "encoder":
        return encoder_leg()
    enc = DacEncoderEngine(synth.synth_state_dict(shapes.dac_encoder_manifest(80), 0), ENC_RATES)
    dec = DacDecoderEngine(synth.synth_state_dict(shapes.dac_decoder_manifest(80), 0), [5, 4, 4, 3, 2])
    for B in (1, 8):
        wav = 0.3 * torch.randn(B, 1, 240000, device="cuda")
        z = torch.randn(B, 80, 500, device="cuda")
        te = timeit(lambda: enc.encode(wav))
        td = timeit(lambda: dec.decode(z))
        print(f"B={B} 10 s each: encode {te:.2f} ms ({B * 10 / te * 1e3:.0f} audio-s/s)  decode {td:.2f} ms "
              f"({B * 10 / td * 1e3:.0f} audio-s/s)", flush=True)


if __name__ == "__main__":
    main()
