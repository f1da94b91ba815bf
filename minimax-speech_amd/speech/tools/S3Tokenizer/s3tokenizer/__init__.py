"""Drop-in for speech/tools/S3Tokenizer/s3tokenizer (the v2 tokenizer): same names, signatures, state-dict keys and layouts; the
arithmetic runs in mmx.s3tok.SpeechTokenizerEngine on a ROCm device.  Put speech/tools/S3Tokenizer on sys.path as for the
reference package.

`load_model` and `S3TokenizerV2.init_from_onnx` download a checkpoint and read it with `onnx`; neither is available here, so they
raise and name `S3TokenizerV2.init_from_pt`.  The v1 `S3Tokenizer` class is out of scope."""
from . import _paths  # noqa: F401
from .model_v2 import ModelConfig, S3TokenizerV2
from .utils import log_mel_spectrogram, make_non_pad_mask, mask_to_bias, merge_tokenized_segments, padding

__all__ = ["ModelConfig", "S3TokenizerV2", "load_model", "log_mel_spectrogram", "make_non_pad_mask", "mask_to_bias",
           "merge_tokenized_segments", "padding"]


def load_model(name: str, download_root: str = None):
    raise RuntimeError(f"s3tokenizer.load_model({name!r}) downloads an ONNX checkpoint and converts it with `onnx`; neither a network "
                       "nor `onnx` is part of this build.  Convert the checkpoint once with the reference's onnx2torch, then "
                       "S3TokenizerV2(name).init_from_pt(path)")
