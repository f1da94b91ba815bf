"""One timing of the loudness meter and the gain on the headline benchmark's 32 mixed-length utterances: the
waveform lengths bench.py's default workload produces (50 .. 500 speech tokens each, seed 3; 960 samples per token at 24 kHz),
filled with noise, as one ragged batch through what tts_batch(loudness_db=-16) adds behind the DAC decode:

    mmx_kweight_blocks (3 launches) -> mmx_loudness_gate -> mmx_scale_rows

    python tools/loudness_timing.py [--calls 50]

A figure is the device-event time of `--calls` back-to-back sequences into preallocated buffers, divided by their number; the
median and the least of 7 such windows after a warm-up window are printed, for the whole sequence and for each entry point
alone, beside the bytes the sequence has to move (every sample read twice by the filter walks and once by the gain, written
once).  Not a speed item: nothing of it runs unless a caller asks for a level."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimax-speech_amd"))
import torch
from mmx import _lib as L
from mmx import loudness as LD

HBM_ACHIEVABLE = 6.3e12                                  # bytes / s (MI355X)
RATE = 24000

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=50)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run gives no time"

lens = [960 * t for t in torch.randint(50, 501, (32,), generator=torch.Generator().manual_seed(3)).tolist()]
B, Lm = len(lens), max(lens)
g = torch.Generator().manual_seed(0)
wave = torch.zeros(B, Lm)
for b, n in enumerate(lens):
    wave[b, :n] = 0.1 * torch.randn(n, generator=g)
wave = wave.cuda()
outs, lufs = LD.normalize([wave[b, :n] for b, n in enumerate(lens)], RATE, -16.0)      # uploads the tables
again = LD.integrated_loudness(outs, RATE)
print(f"{B} utterances, {sum(lens)} samples ({sum(lens) / RATE:.1f} s, longest {Lm / RATE:.1f} s): measured "
      f"{lufs.min().item():.3f} .. {lufs.max().item():.3f} LUFS, after normalize(-16) {again.min().item():.4f} .. {again.max().item():.4f}")

_, S = LD.block_sizes(RATE)
tab, seg = LD._device_tables(RATE, wave.device)
cap = LD._cap(Lm, RATE, S)
d_lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
work = torch.empty(B, cap, 5, dtype=torch.float64, device="cuda")
energy = torch.empty(B, cap, dtype=torch.float64, device="cuda")
peak, lu, gain = (torch.empty(B, device="cuda") for _ in range(3))
out = torch.empty(B, Lm, device="cuda")
lib, st = L.load(), L.stream()


def blocks():
    return lib.mmx_kweight_blocks(L._p(wave), L.i64(Lm), Lm, B, L._p(d_lens), RATE, 0, L._p(tab), seg, L._p(work), cap, L._p(energy),
                                  L.i64(cap), L._p(peak), st)


def gate():
    return lib.mmx_loudness_gate(L._p(energy), L.i64(cap), cap, L._p(peak), L._p(d_lens), Lm, B, 1, None, RATE, 0, L._p(lu), 1,
                                 C.c_float(-16.0), C.c_float(1.0), L._p(gain), None, L.i64(0), st)


def scale():
    return lib.mmx_scale_rows(L._p(wave), L.i64(Lm), Lm, B, L._p(d_lens), L._p(gain), 1, L._p(out), L.i64(Lm), st)


def timed(fns):
    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            for f in fns:
                assert f() == 0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls    # us per sequence
    window()
    ws = [window() for _ in range(7)]
    return statistics.median(ws), min(ws)


for name, fns in (("meter + gain (5 launches)", (blocks, gate, scale)), ("mmx_kweight_blocks (3 launches)", (blocks,)),
                  ("mmx_loudness_gate", (gate,)), ("mmx_scale_rows", (scale,))):
    med, least = timed(fns)
    print(f"{name:32s} median {med:8.2f} us   least {least:8.2f} us")
assert torch.equal(lu, lufs) and all(torch.equal(out[b, :n], outs[b]) for b, n in enumerate(lens))
nbytes = 4 * sum(lens) * 4
print(f"bytes: 3 reads + 1 write of {sum(lens)} fp32 samples = {nbytes / 1e6:.1f} MB = {nbytes / HBM_ACHIEVABLE * 1e6:.2f} us at 6.3 TB/s")
