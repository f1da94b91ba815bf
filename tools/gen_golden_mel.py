"""Writes tests/golden/mel.npz: log-mel fixtures for tests/test_mel_host.py and tests/test_gpu_mel.py.  Runs on the CPU.

    python tools/gen_golden_mel.py [path of the reference's speech/matcha/utils/audio.py; default: under oracle.ref_shims.REF]

The reference's mel_spectrogram (audio.py:45-82) is loaded from the given file and run as it is.  Its two imports that are not
installed here get stand-ins before the load: `librosa.filters.mel` calls mmx.mel.mel_filterbank (the Slaney filterbank restated
from librosa's published definition), `scipy.io.wavfile.read` is never called on this path.  Recorded per waveform: the samples,
the reference function's fp32 output, a float64 evaluation of the same formula (direct, numpy rfft in float64 on the fp32
samples and the fp32 filterbank), and the bound the two must agree to; plus the filterbanks.  Arrays only."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimax-speech_amd"))
from mmx import mel as M  # noqa: E402

SETTING = dict(n_fft=1920, num_mels=80, sampling_rate=24000, hop_size=480, win_size=1920, fmin=0)


def load_reference(path):
    lib, filt = types.ModuleType("librosa"), types.ModuleType("librosa.filters")
    filt.mel = lambda sr, n_fft, n_mels, fmin, fmax: M.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    lib.filters = filt
    sys.modules.setdefault("librosa", lib)
    sys.modules.setdefault("librosa.filters", filt)
    try:
        import scipy.io.wavfile  # noqa: F401
    except ImportError:
        sp, io, wf = types.ModuleType("scipy"), types.ModuleType("scipy.io"), types.ModuleType("scipy.io.wavfile")
        wf.read = None
        sys.modules.update({"scipy": sp, "scipy.io": io, "scipy.io.wavfile": wf})
    spec = importlib.util.spec_from_file_location("ref_audio", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def logmel_f64(x, fb, n_fft, hop):
    """audio.py:57-82 in float64 on the fp32 samples x [n] and the fp32 filterbank fb."""
    pad = (n_fft - hop) // 2
    y = np.pad(x.astype(np.float64), (pad, pad), mode="reflect")
    T = (len(y) - n_fft) // hop + 1
    k = np.arange(n_fft)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * k / n_fft)
    frames = np.stack([y[t * hop:t * hop + n_fft] for t in range(T)]) * win
    spec = np.fft.rfft(frames, axis=1)
    mag = np.sqrt(spec.real ** 2 + spec.imag ** 2 + 1e-9)
    return np.log(np.maximum(fb.astype(np.float64) @ mag.T, 1e-5))


def waveforms():
    g = torch.Generator().manual_seed(20240)
    rnd = lambda n: torch.randn(n, generator=g, dtype=torch.float32)
    t = torch.arange(2400, dtype=torch.float64)
    out = {"noise": rnd(4800), "tone": (0.9 * torch.sin(2 * np.pi * 440.0 * t / 24000)).float() + 1e-3 * rnd(2400),
           "short": rnd(1440)}
    return {k: (v / v.abs().max()).numpy() for k, v in out.items()}


# |fp32 reference - float64| allowed per case: the fp32 spectrum of a frame is off by a few eps32 * ||frame|| per bin (~1e-6 at
# these frame norms); a log-mel value moves by that over its mel energy: >= 1 for noise at full scale (bound 1e-5), ~1e-3 for the
# leakage channels of the tone above its 1e-3 noise floor (bound 1e-2)
TOL = {"noise": 1e-5, "tone": 1e-2, "short": 1e-5, "noise_full": 1e-5}


def main():
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        sys.path.insert(0, ROOT)
        from oracle.ref_shims import REF
        path = os.path.join(REF, "speech", "matcha", "utils", "audio.py")
    ref = load_reference(path)
    out = {}
    for fmax, tag in ((8000, "8000"), (None, "full")):
        out[f"fb_{tag}"] = M.mel_filterbank(24000, 1920, 80, 0, fmax)
    for name, x in waveforms().items():
        for fmax, tag in ((8000, ""), (None, "_full")):
            if tag and name != "noise":
                continue
            ref.mel_basis.clear()
            ref.hann_window.clear()
            with torch.no_grad():
                y32 = ref.mel_spectrogram(torch.from_numpy(x)[None], fmax=fmax, center=False, **SETTING)[0].numpy()
            y64 = logmel_f64(x, out["fb_full" if tag else "fb_8000"], 1920, 480)
            assert y32.shape == y64.shape and y32.dtype == np.float32
            key = name + tag
            out[f"ref32_{key}"], out[f"ref64_{key}"], out[f"tol_{key}"] = y32, y64, np.float64(TOL[key])
            print(f"{key:12s} frames {y32.shape[1]:3d}  max|fp32 - f64| {np.abs(y32 - y64).max():.3e}  (bound {TOL[key]:.0e})")
        out[f"wave_{name}"] = x
    path = os.path.join(ROOT, "tests", "golden", "mel.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
