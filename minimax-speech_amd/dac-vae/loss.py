"""Drop-in for the inference side of dac-vae/loss.py: L1Loss (:11-48), SISDRLoss (:51-139), MultiScaleSTFTLoss (:142-228) and
MelSpectrogramLoss (:231-327) with the reference's constructor arguments, evaluated by mmx.metrics (mmx_spec_dist, mmx_wave_sums)
on device tensors.  `forward(x, y)` takes tensors [B, 1, T] (or [B, T]) or any two objects with `.audio_data` and `.sample_rate`
(an AudioSignal), x the estimate and y the reference, and returns the scalar the reference returns: the mean over an equal-length
batch, as a float64 device scalar.  No autograd: these are measurements, not training losses; GANLoss and kl_loss are training only and not part of this.
A `loss_fn` other than L1, `match_stride=True` or a window other than Hann raise NotImplementedError."""
import torch
from torch import nn

import _mmx_path  # noqa: F401
from mmx import clips, metrics


def _audio(v):
    """(tensor [B, T], sample rate or None) of a tensor [B, 1, T] / [B, T] / [T] or of an object with .audio_data / .sample_rate."""
    rate = getattr(v, "sample_rate", None)
    a = getattr(v, "audio_data", v)
    if not torch.is_tensor(a):
        raise TypeError(f"expected a tensor or an object with .audio_data, got {type(v).__name__}")
    if a.dim() == 3:
        if a.shape[1] != 1:
            raise NotImplementedError(f"mono audio only, got {a.shape[1]} channels")
        a = a[:, 0]
    elif a.dim() == 1:
        a = a[None]
    return a, rate


def _l1_only(loss_fn, match_stride, window_type):
    if not isinstance(loss_fn, nn.L1Loss) or getattr(loss_fn, "reduction", "mean") != "mean":
        raise NotImplementedError("loss_fn: only nn.L1Loss() is built")
    if match_stride:
        raise NotImplementedError("match_stride=True is not built")
    if window_type not in (None, "hann"):
        raise NotImplementedError(f"window_type {window_type!r}: only the Hann window is built")


class L1Loss(nn.Module):
    def __init__(self, attribute: str = "audio_data", weight: float = 1.0, **kwargs):
        super().__init__()
        if attribute != "audio_data" or kwargs.get("reduction", "mean") != "mean":
            raise NotImplementedError("only the mean L1 distance of audio_data is built")
        self.attribute, self.weight = attribute, weight

    @torch.no_grad()
    def forward(self, x, y):
        (xa, _), (ya, _) = _audio(x), _audio(y)
        return metrics.waveform_distance(xa, ya)["l1"].mean()


class SISDRLoss(nn.Module):
    """loss.py:91-139.  As there, forward(x, y) takes x as the REFERENCES and y as the estimates, and the result is the negative
    ratio in dB."""

    def __init__(self, scaling: int = True, reduction: str = "mean", zero_mean: int = True, clip_min: int = None, weight: float = 1.0):
        super().__init__()
        self.scaling, self.reduction, self.zero_mean, self.clip_min, self.weight = scaling, reduction, zero_mean, clip_min, weight

    @torch.no_grad()
    def forward(self, x, y):
        (ref, _), (est, _) = _audio(x), _audio(y)
        e, r, lens = clips.pack_pair(est, ref, None, "SISDRLoss")
        s = metrics.wave_sums(e, r, lens)
        sdr = -metrics.sisdr_from_sums(s, float(e.shape[1]), bool(self.scaling), bool(self.zero_mean))
        if self.clip_min is not None:
            sdr = torch.clamp(sdr, min=self.clip_min)
        if self.reduction == "mean":
            sdr = sdr.mean()
        elif self.reduction == "sum":
            sdr = sdr.sum()
        return sdr


class MultiScaleSTFTLoss(nn.Module):
    def __init__(self, window_lengths=[2048, 512], loss_fn=nn.L1Loss(), clamp_eps: float = 1e-5, mag_weight: float = 1.0,
                 log_weight: float = 1.0, pow: float = 2.0, weight: float = 1.0, match_stride: bool = False, window_type: str = None):
        super().__init__()
        _l1_only(loss_fn, match_stride, window_type)
        self.window_lengths = [int(w) for w in window_lengths]
        self.loss_fn, self.clamp_eps, self.mag_weight, self.log_weight, self.pow, self.weight = loss_fn, clamp_eps, mag_weight, log_weight, pow, weight

    @torch.no_grad()
    def forward(self, x, y):
        (xa, _), (ya, _) = _audio(x), _audio(y)
        return metrics.stft_distance(xa, ya, window_lengths=self.window_lengths, pow=self.pow, clamp_eps=self.clamp_eps,
                                     log_weight=self.log_weight, mag_weight=self.mag_weight).mean()


class MelSpectrogramLoss(nn.Module):
    """`sample_rate` (not a reference argument) is the rate of bare tensors; an AudioSignal brings its own."""

    def __init__(self, n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048], loss_fn=nn.L1Loss(),
                 clamp_eps: float = 1e-5, mag_weight: float = 0.0, log_weight: float = 1.0, pow: float = 1.0, weight: float = 1.0,
                 match_stride: bool = False, mel_fmin=[0, 0, 0, 0, 0, 0, 0], mel_fmax=[None, None, None, None, None, None, None],
                 window_type: str = None, sample_rate: int = None):
        super().__init__()
        _l1_only(loss_fn, match_stride, window_type)
        self.window_lengths, self.n_mels = [int(w) for w in window_lengths], [int(m) for m in n_mels]
        nw = min(len(self.window_lengths), len(self.n_mels), len(mel_fmin), len(mel_fmax))        # the reference zips the four lists
        self.window_lengths, self.n_mels = self.window_lengths[:nw], self.n_mels[:nw]
        self.mel_fmin, self.mel_fmax = list(mel_fmin)[:nw], list(mel_fmax)[:nw]
        self.loss_fn, self.clamp_eps, self.mag_weight, self.log_weight, self.pow, self.weight = loss_fn, clamp_eps, mag_weight, log_weight, pow, weight
        self.sample_rate = sample_rate

    @torch.no_grad()
    def forward(self, x, y):
        (xa, rx), (ya, ry) = _audio(x), _audio(y)
        rate = rx or ry or self.sample_rate
        if rate is None:
            raise ValueError("MelSpectrogramLoss on bare tensors needs sample_rate= at construction")
        return metrics.mel_distance(xa, ya, int(rate), n_mels=self.n_mels, window_lengths=self.window_lengths, pow=self.pow,
                                    clamp_eps=self.clamp_eps, log_weight=self.log_weight, mag_weight=self.mag_weight,
                                    mel_fmin=self.mel_fmin, mel_fmax=self.mel_fmax).mean()
