"""Drop-in for s3tokenizer/model_v2.py: `S3TokenizerV2` as a parameter shell with the reference's 4 + 16 * layers + 2
state-dict keys and attribute paths (encoder.conv1, encoder.blocks[i].attn.query, quantizer._codebook.project_down, ...);
forward / quantize run in mmx.s3tok.SpeechTokenizerEngine, built lazily from the module's current parameters."""
from dataclasses import dataclass
from typing import Tuple

import torch

from . import _paths  # noqa: F401
from mmx import shapes, shell
from mmx.s3tok import SpeechTokenizerEngine


@dataclass
class ModelConfig:
    n_mels: int = 128
    n_audio_ctx: int = 1500
    n_audio_state: int = 1280
    n_audio_head: int = 20
    n_audio_layer: int = 6
    n_codebook_size: int = 3 ** 8

    use_sdpa: bool = False


class S3TokenizerV2(shell.EngineHost):
    """model_v2.py:354-604, inference only.  The engine runs the split build by default (compute_dtype 2; float_parity() selects
    the fp32 build); it never runs the bf16 build: tokens are discrete."""

    compute_dtype = 2

    def __init__(self, name: str, config: ModelConfig = None):
        super().__init__()
        config = ModelConfig() if config is None else config
        self.name = name
        if "v1" not in name:
            assert "v2" in name
            config.n_codebook_size = 3 ** 8
        self.config = config
        shell.register(self, shapes.s3tok_manifest(config.n_audio_state, config.n_audio_head, config.n_audio_layer, config.n_mels))

    def _get_engine(self):
        if self._engine is None:
            wp = None if self.weight_planes == "auto" else self.weight_planes
            self._engine = SpeechTokenizerEngine(self.state_dict(), dtype=self.compute_dtype, device=self._device(),
                                                 n_head=self.config.n_audio_head, wplanes=wp)
        return self._engine

    def forward(self, mel: torch.Tensor, mel_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return self.quantize(mel, mel_len)

    @torch.inference_mode()
    def quantize(self, mel: torch.Tensor, mel_len: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """mel [B, n_mels, T], mel_len [B] -> (code int32 [B, T'] (int64 when a member exceeds 3000 frames, as in the reference),
        code_len [B] in mel_len's integer type)."""
        codes, code_len = self._get_engine().quantize(mel.to(self._device()), mel_len)
        long_path = bool((mel_len > 3000).any())
        return (codes.long() if long_path else codes), code_len.to(torch.long if long_path else mel_len.dtype)

    @property
    def device(self):
        return next(self.parameters()).device

    def init_from_onnx(self, onnx_path: str):
        raise RuntimeError("S3TokenizerV2.init_from_onnx reads the checkpoint with `onnx`, which is not part of this build; convert it "
                           "once with the reference's onnx2torch and use init_from_pt")

    def init_from_pt(self, ckpt_path: str):
        self.load_state_dict(torch.load(ckpt_path, map_location="cpu", mmap=True), strict=True)

    def freeze(self):
        self.requires_grad_(False)
