"""Writes the S3 speech tokenizer fixtures of tests/test_s3tok_host.py and tests/test_gpu_s3tok.py.  Runs on the CPU.

    python tools/gen_golden_s3tok.py [directory that holds the reference's s3tokenizer package;
                                      default: speech/tools/S3Tokenizer under oracle.ref_shims.REF]

The reference's modules (s3tokenizer/utils.py, model.py, model_v2.py) are loaded from their files and run as they are; `onnx`,
`torchaudio` and `tqdm`, which they import and this path never calls, get empty stand-ins.  Arrays, shapes and index lists only:

  tests/golden/manifest_s3tok.json   key -> shape of S3TokenizerV2 at full size
  tests/golden/s3tok.npz             mel_128 (the filterbank the reference reads from assets/mel_filters.npz); per clip the samples,
                                     the reference's fp32 log-mel, the float64 evaluation (tests/test_s3tok_host.py logmel_ref) and
                                     their bound; at (256, 4, 2) with mmx.synth weights of the recorded seed: the reference's
                                     quantize output for the zero-padded batch and per clip, its fp32 pre-round values, and e_ref
  tests/golden/s3tok_plan.json       windows and merged index list of the > 3000-frame path, from the reference's own
                                     _quantize_mixed_batch driven with a stub encoder whose tokens are frame indices

The float64 side (logmel_ref, encode_ref) is imported from tests/test_s3tok_host.py, so that the generator and the tests share one
yardstick: an edit to that restatement changes what this tool records as e_ref and what it accepts under the 2 % cap - regenerate
the fixtures and re-read the printed figures after one.

A token fixture in which more than 2 % of the digits lie within 1e-3 of a rounding boundary in float64 is refused: pick another seed."""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimax-speech_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mmx import shapes, synth  # noqa: E402
import test_s3tok_host as R  # noqa: E402

SEED = 0
PLAN_FRAMES = (2999, 3000, 3001, 5600, 5601, 8200, 9000)


def load_reference(pkg_dir):
    for name in ("onnx", "torchaudio", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        sys.modules["tqdm"].tqdm = lambda it, *a, **k: it
    sys.path.insert(0, pkg_dir)
    return importlib.import_module("s3tokenizer.model_v2"), importlib.import_module("s3tokenizer.utils")


def clips():
    g = torch.Generator().manual_seed(20251)
    rnd = lambda n: torch.randn(n, generator=g, dtype=torch.float32)
    t = torch.arange(20800, dtype=torch.float64)
    speechy = (0.5 * torch.sin(2 * np.pi * 220.0 * t / 16000) * (0.6 + 0.4 * torch.sin(2 * np.pi * 3.0 * t / 16000))).float() + 0.05 * rnd(20800)
    gap = 0.3 * rnd(16000)
    gap[5000:11000] *= 1e-6                              # a near-silent stretch: the max - 8 floor binds there
    out = {"noise": 0.3 * rnd(32000), "tiny": 0.3 * rnd(360), "voiced": speechy[:8960], "gap": gap}     # 8960 samples: 56 frames, no multiple of 16
    return {k: v.numpy() for k, v in out.items()}


# |fp32 reference - float64| allowed on the final (v + 4) / 4 values: the fp32 spectrum of a frame is off by a few eps32 * ||frame||
# per bin; a log10 value moves by that over its mel power's square root, divided by 4 ln 10 by the affine map.  Full-scale noise:
# 1e-5; channels that sit up to 8 decades below the clip maximum (the tone's leakage, the silent stretch above its floor): 1e-2.
TOL = {"noise": 1e-5, "tiny": 1e-5, "voiced": 1e-2, "gap": 1e-2}


def plan_fixture(M):
    tok = M.S3TokenizerV2("speech_tokenizer_v2_25hz", M.ModelConfig(n_audio_state=64, n_audio_head=1, n_audio_layer=1))
    seen = []

    class Enc(torch.nn.Module):                          # tokens = the absolute index of the frame a token row starts at
        def forward(self, mel, mel_len):
            seen.append([(int(mel[i, 0, 0]), int(mel_len[i])) for i in range(mel.shape[0])])
            return mel[:, 0, ::4], ((mel_len - 1) // 2 + 1 - 1) // 2 + 1

    class Quant(torch.nn.Module):
        def encode(self, h):
            return h.long()

    tok.encoder, tok.quantizer = Enc(), Quant()
    out = {}
    for n in PLAN_FRAMES:
        mel = torch.zeros(1, 128, n)
        mel[0, 0] = torch.arange(n, dtype=torch.float32)
        ln = torch.tensor([n])
        seen.clear()
        codes, cl = tok._quantize_mixed_batch(mel, ln, ln > 3000, 3000)
        out[str(n)] = {"windows": [list(w) for w in seen[0]], "merged": codes[0, :int(cl[0])].tolist()}
    return out


def main():
    if len(sys.argv) > 1:
        pkg = sys.argv[1]
    else:
        sys.path.insert(0, ROOT)
        from oracle.ref_shims import REF
        pkg = os.path.join(REF, "speech", "tools", "S3Tokenizer")
    M, U = load_reference(pkg)
    gold = os.path.join(ROOT, "tests", "golden")

    full = M.S3TokenizerV2("speech_tokenizer_v2_25hz", M.ModelConfig())
    json.dump({k: list(v.shape) for k, v in full.state_dict().items()}, open(os.path.join(gold, "manifest_s3tok.json"), "w"), indent=0)
    del full

    out = {"mel_128": U._mel_filters("cpu", 128).numpy(), "seed": np.int64(SEED)}
    names, mels = [], []
    for name, x in clips().items():
        with torch.no_grad():
            y32 = U.log_mel_spectrogram(torch.from_numpy(x)).numpy()
        y64 = R.logmel_ref(x, out["mel_128"])
        assert y32.shape == y64.shape == (128, len(x) // 160) and y32.dtype == np.float32
        err = np.abs(y32 - y64).max()
        assert err <= TOL[name], (name, err)
        print(f"{name:8s} samples {len(x):6d} frames {y32.shape[1]:3d}  max|fp32 - f64| {err:.3e}  (bound {TOL[name]:.0e})  "
              f"on the floor: {(y64 == y64.min()).mean():.2%}")
        out["wave_" + name], out["mel32_" + name], out["mel64_" + name], out["tol_mel_" + name] = x, y32, y64, np.float64(TOL[name])
        names.append(name)
        mels.append(torch.from_numpy(y32))
    out["names"] = np.array(names)

    cfg = R.FIX_CFG
    sd = synth.synth_state_dict(shapes.s3tok_manifest(**cfg), SEED, "fp32")
    tok = M.S3TokenizerV2("speech_tokenizer_v2_25hz", M.ModelConfig(n_audio_state=cfg["C"], n_audio_head=cfg["heads"], n_audio_layer=cfg["layers"]))
    tok.load_state_dict(sd, strict=True)
    tok.eval()
    feats, feat_lens = U.padding(mels)
    pre = {}
    hook = tok.quantizer._codebook.project_down.register_forward_hook(lambda m, i, o: pre.__setitem__("h", o.detach().clone()))
    with torch.no_grad():
        codes, code_len = tok.quantize(feats, feat_lens)
        pre32 = (pre["h"].float().tanh() * 0.9990000128746033).reshape(codes.shape[0], codes.shape[1], 8)
        for i, n in enumerate(names):
            c, cl = tok.quantize(mels[i][None], torch.tensor([mels[i].shape[1]]))
            out["codes_" + n] = c[:, :int(cl[0])].numpy().astype(np.int32)
        v64, h64, x64, l2 = R.encode_ref(sd, feats, feat_lens.tolist())
    hook.remove()
    valid = R.valid_rows(l2, v64.shape[1])
    assert l2 == code_len.tolist()
    e_ref = float((pre32.double() - v64).abs()[valid].max())
    near = float((((v64.abs() - 0.5).abs() < 1e-3) & valid[..., None]).sum()) / (int(valid.sum()) * 8)
    d = R.digits_of(v64)[valid]
    print(f"tokens {l2}  e_ref {e_ref:.3e}  digits within 1e-3 of a boundary {near:.2%}  min margin {float((v64.abs() - 0.5).abs()[valid].min()):.2e}  "
          f"digit shares {[round(float((d == k).float().mean()), 3) for k in range(3)]}  max|h| {float(h64.abs()[valid].max()):.2f}  "
          f"hidden rms {float(x64[valid].pow(2).mean().sqrt()):.2f}")
    if near > 0.02:
        raise SystemExit("more than 2 % of the digits are undecided in float64: pick another seed")
    out.update(codes=codes.numpy().astype(np.int32), code_len=code_len.numpy().astype(np.int32), pre32=pre32.numpy(), e_ref=np.float64(e_ref),
               hmax=np.float64(h64.abs()[valid].max()))
    path = os.path.join(gold, "s3tok.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")

    json.dump(plan_fixture(M), open(os.path.join(gold, "s3tok_plan.json"), "w"))
    print(os.path.getsize(os.path.join(gold, "s3tok_plan.json")), "bytes of plan")


if __name__ == "__main__":
    main()
