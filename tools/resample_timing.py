"""One timing of the sinc resampler: a 30 s mono clip, 48 kHz -> 16 kHz and 16 kHz -> 24 kHz, one launch of
mmx_resample_sinc each, beside its byte floor (input + output bytes over the HBM rate).

    python tools/resample_timing.py [--calls 200]

A figure is the device-event time of `--calls` back-to-back launches into one preallocated output, divided by their number, the
least of 5 such windows after a warm-up window; back to back, a launch shorter than the launch overhead measures that overhead.
For the kernel's own duration run the same command under `rocprofv3 --kernel-trace --stats`.  Not a speed item: a once-per-voice
cost, recorded beside the parity numbers."""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimax-speech_amd"))
import torch
from mmx import _lib as L
from mmx.resample import Resample, out_len

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12                # bytes / s (MI355X)

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a CPU run gives no time"

for orig, new in ((48000, 16000), (16000, 24000)):
    n_in = 30 * orig
    x = torch.rand(n_in, generator=torch.Generator().manual_seed(0)).mul(2).sub(1).cuda()
    rs = Resample(orig, new)
    y = rs(x)                                            # uploads the tables; the timed loop below reuses them
    n_out = out_len(n_in, orig, new)
    assert y.shape[0] == n_out and torch.isfinite(y).all()
    taps, first, count = rs._device_tables(x.device)
    out = torch.empty(n_out, device="cuda")
    lib, st = L.load(), L.stream()

    def window():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            rc = lib.mmx_resample_sinc(L._p(x), L.i64(n_in), n_in, 1, None, None, rs.o, rs.n, rs._host[3], L._p(taps), L._p(first),
                                       L._p(count), taps.shape[0], L._p(out), L.i64(n_out), n_out, st)
            assert rc == 0
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls    # us per launch

    window()
    us = min(window() for _ in range(5))
    assert torch.equal(out, y)
    nbytes = 4 * (n_in + n_out)
    print(f"{orig} -> {new}: 30 s = {n_in} samples in, {n_out} out, {taps.shape[0]} taps x {rs.n} phases; {us:.2f} us per launch; "
          f"byte floor {nbytes / 1e6:.2f} MB = {nbytes / HBM_PEAK * 1e6:.2f} us at 8 TB/s ({nbytes / HBM_ACHIEVABLE * 1e6:.2f} us at 6.3 TB/s)")
