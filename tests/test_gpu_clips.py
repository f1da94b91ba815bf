"""Every audio module through the one intake (mmx/clips.py) on the device: a clip's result is the same bits whether it arrives in a
list, in a padded tensor with `lens`, or alone - the promise of each function's docstring - and a padded tensor whose rows are all
whole gives the same bits with lens=[L, L, L] as with lens=None (clips.lens_args passes NULL for both).

Three clips of 1500, 1031 and 700 samples of seeded noise at 16 kHz: above every module's minimum at the settings below, with one
exception.  audio_distance's scales go up to a 2048-sample window, which reflects by 1024 samples, so it refuses the 700-sample
clip (asserted below, in both forms); it runs on the other two clips, and the scales that take all three (windows up to 1024) and
the waveform sums run on all three through mel_distance, stft_distance and waveform_distance."""
import functools

import pytest
import torch

from mmx import degrade, denoise, loudness, mel, metrics, resample, stoi
from mmx._lib import MmxError

pytestmark = pytest.mark.gpu

RATE = 16000
LENS = [1500, 1031, 700]


@functools.cache
def inputs():
    """(clips, a second signal per clip, equal-length batch, second equal-length batch, impulse response), on the device."""
    g = torch.Generator().manual_seed(11)
    a = [0.1 * torch.randn(n, generator=g) for n in LENS]
    b = [x + 0.03 * torch.randn(x.numel(), generator=g) for x in a]
    eq = 0.1 * torch.randn(3, 1500, generator=g)
    eq2 = eq + 0.03 * torch.randn(3, 1500, generator=g)
    ir = torch.randn(300, generator=g) * torch.exp(-torch.arange(300) / 60.0)
    return [x.cuda() for x in a], [x.cuda() for x in b], eq.cuda(), eq2.cuda(), ir.cuda()


def padded(ws):
    x = torch.zeros(len(ws), max(w.numel() for w in ws), device="cuda")
    for i, w in enumerate(ws):
        x[i, :w.numel()] = w
    return x


def cut(out, ns):
    """Per clip, its own part of a result: the last dimension cut to ns[b] (None: the whole entry).  One clip passed as [n] comes
    back without a batch dimension."""
    if isinstance(out, dict):
        out = torch.stack([out[k] for k in sorted(out)], dim=1)
    if ns is None:
        return [out[b] for b in range(len(out))]
    if isinstance(out, torch.Tensor) and out.dim() == 1:
        out = out[None]
    if isinstance(out, torch.Tensor) and out.dim() == 3 and out.shape[1] == 1:      # [B, 1, L] in, [B, 1, L] back
        out = out[:, 0]
    return [out[b][..., :n] for b, n in enumerate(ns)]


LOGMEL = dict(n_fft=512, num_mels=80, sampling_rate=RATE, hop_size=128, win_size=512, fmin=0, fmax=8000)


def _logmel(x, y, lens, ns):
    m = mel.LogMel(**LOGMEL)
    return cut(m(x, lens=lens), [m.frames(n) for n in ns])


def _resample(x, y, lens, ns):
    rs = resample.Resample(RATE, 24000)
    return cut(rs(x, lens) if isinstance(x, torch.Tensor) else resample.resample(x, RATE, 24000), [rs.out_len(n) for n in ns])


def _normalize(x, y, lens, ns):
    """normalize takes a list only: a padded batch goes in as the views of its rows."""
    out, lufs = loudness.normalize(x if isinstance(x, list) else [x.reshape(len(ns), -1)[b, :n] for b, n in enumerate(ns)], RATE, -20.0)
    return [torch.cat([o, l[None]]) for o, l in zip(out, lufs)]


def _distance(fn, **kw):
    return lambda x, y, lens, ns: cut(fn(x, y, lens=lens, **kw), None)


CASES = {
    "logmel": _logmel,
    "resample": _resample,
    "integrated_loudness": lambda x, y, lens, ns: cut(loudness.integrated_loudness(x, RATE, lens=lens), None),
    "normalize": _normalize,
    "mel_distance": _distance(metrics.mel_distance, rate=RATE, n_mels=metrics.MEL_N_MELS[:6], window_lengths=metrics.MEL_WINDOWS[:6]),
    "stft_distance": _distance(metrics.stft_distance, window_lengths=(1024, 512)),
    "waveform_distance": _distance(metrics.waveform_distance, clip=1.0),
    "spectral_gate": lambda x, y, lens, ns: cut(denoise.spectral_gate(x, (0, 400), lens=lens, win_length=256, hop_length=64), ns),
    "stoi": lambda x, y, lens, ns: cut(stoi.stoi(y, x, RATE, lens=lens), None),
    "convolve": lambda x, y, lens, ns: cut(degrade.convolve(x, inputs()[4], lens=lens), ns),
    "mix": lambda x, y, lens, ns: cut(degrade.mix(x, y, RATE, snr=7.0, lens=lens, noise_lens=lens), ns),
}


def same(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and torch.equal(g, w), f"{what}: clip {b}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_form_gives_a_clip_the_same_bits(name):
    run = CASES[name]
    a, b, eq, eq2, _ = inputs()
    want = run(a, b, None, LENS)
    assert all(bool(torch.isfinite(w).all()) for w in want)
    same(run(padded(a), padded(b), LENS, LENS), want, f"{name}, padded tensor with lens")
    same(run(padded(a)[:, None], padded(b)[:, None], torch.tensor(LENS), LENS), want, f"{name}, [B, 1, L] with lens as a tensor")
    for i, n in enumerate(LENS):
        same(run([a[i]], [b[i]], None, [n]), want[i:i + 1], f"{name}, clip {i} in a list of one")
        same(run(a[i], b[i], None, [n]), want[i:i + 1], f"{name}, clip {i} alone")
    same(run(eq, eq2, [1500] * 3, [1500] * 3), run(eq, eq2, None, [1500] * 3), f"{name}, whole rows with lens against lens=None")


def test_audio_distance():
    """The two clips its 2048-sample scale takes, in every form; the 700-sample clip refuses the batch in every form."""
    a, b, eq, eq2, _ = inputs()
    run = _distance(metrics.audio_distance, rate=RATE, clip=1.0)
    want = run(a[:2], b[:2], None, None)
    assert all(bool(torch.isfinite(w).all()) for w in want)
    same(run(padded(a[:2]), padded(b[:2]), LENS[:2], None), want, "padded tensor with lens")
    for i in range(2):
        same(run(a[i], b[i], None, None), want[i:i + 1], f"clip {i} alone")
    same(run(eq, eq2, [1500] * 3, None), run(eq, eq2, None, None), "whole rows with lens against lens=None")
    for x, y, lens in ((a, b, None), (padded(a), padded(b), LENS), (a[2], b[2], None)):
        with pytest.raises(MmxError, match="reflected"):
            metrics.audio_distance(x, y, RATE, lens=lens)
