"""Drop-in for speech/matcha/utils/audio.py:45-82: `mel_spectrogram`, the `feat_extractor` of speech/config.yaml:183-191
(and `mel_spec_transform1`, :143-151).  Same signature and result [B, num_mels, T]; the arithmetic is one launch of
mmx_logmel (mmx/mel.py), so `y` must live on a ROCm device."""
from .. import _paths  # noqa: F401
from mmx.mel import LogMel


def mel_spectrogram(y, n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, center=False):
    if center:
        raise NotImplementedError("center=True: no configuration of the reference uses it")
    return LogMel(n_fft, num_mels, sampling_rate, hop_size, win_size, fmin, fmax, device=y.device)(y)
