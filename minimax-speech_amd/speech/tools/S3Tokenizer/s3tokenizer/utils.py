"""Drop-in for s3tokenizer/utils.py: the functions the v2 tokenizer's callers use.  log_mel_spectrogram is one launch pair of
mmx_logmel_w (mmx/s3tok.py LogMelW), so the audio has to live on (or be moved to, with `device=`) a ROCm device."""
from typing import List, Optional, Union

import numpy as np
import torch
import torch.nn.functional as F

from . import _paths  # noqa: F401
from mmx import s3tok as _s3tok


def log_mel_spectrogram(audio: Union[np.ndarray, torch.Tensor], n_mels: int = 128, padding: int = 0,
                        device: Optional[Union[str, torch.device]] = None):
    """utils.py:220-267: audio [n] (or [B, n]) at 16 kHz -> [n_mels, n // 160] (or [B, n_mels, n // 160]) fp32.  A path is not
    accepted (decoding a file needs torchaudio)."""
    if isinstance(audio, str):
        raise RuntimeError("log_mel_spectrogram: pass the samples; reading a file needs torchaudio, which this build does not use")
    if not torch.is_tensor(audio):
        audio = torch.from_numpy(np.asarray(audio))
    if device is not None:
        audio = audio.to(device)
    if padding > 0:
        audio = F.pad(audio, (0, padding))
    if n_mels != 128:
        raise NotImplementedError("n_mels = 128 only: the v2 tokenizer's setting")
    out = _s3tok.LogMelW(n_mels, audio.device)(audio)
    return out[0] if audio.dim() == 1 else out


def make_non_pad_mask(lengths: torch.Tensor, max_len: int = 0) -> torch.Tensor:
    """utils.py:270-307: [B] lengths -> bool [B, max_len], True on the valid part."""
    max_len = max_len if max_len > 0 else int(lengths.max())
    return torch.arange(max_len, device=lengths.device)[None, :] < lengths[:, None]


def mask_to_bias(mask: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """utils.py:310-343: bool mask -> additive attention bias, -1e10 on the masked part."""
    assert mask.dtype == torch.bool and dtype in (torch.float32, torch.bfloat16, torch.float16)
    return (1.0 - mask.to(dtype)) * -1.0e10


def padding(data: List[torch.Tensor]):
    """utils.py:346-364: a list of [128, T_i] mels -> (zero-padded [B, 128, T_max], int32 lengths [B])."""
    assert isinstance(data, list)
    lens = torch.tensor([m.size(1) for m in data], dtype=torch.int32)
    out = data[0].new_zeros(len(data), data[0].size(0), int(lens.max()))
    for i, m in enumerate(data):
        out[i, :, :m.size(1)] = m
    return out, lens


def merge_tokenized_segments(tokenized_segments, overlap, token_rate):
    """utils.py:367-390."""
    return _s3tok.merge_segments(tokenized_segments, overlap, token_rate)
