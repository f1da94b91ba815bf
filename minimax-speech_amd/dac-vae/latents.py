"""The `*_latent2x.pt` latent file format that connects DAC-VAE to the TTS flow model.

Writer side follows dac-vae/extract_dac_latents.py:20-46 (clamp to [-1, 1], encode UNPADDED audio) and :171-196
(the saved dict and the `<audio stem>_latent2x.pt` naming); reader side follows
speech/cosyvoice/dataset/processor.py:149-159 (`z` -> [T, D], trimmed so latents = token_latent_ratio * tokens).
The encoder itself runs on the HIP path (model.DACVAE.encode); file IO is torch.save / torch.load as in the reference,
so files written by either side load in the other.  Audio decoding / resampling (librosa in the reference) and the
multi-process driver of that script are outside the hot path: callers hand over a mono float waveform.
"""
import os
from typing import Dict, List, Tuple

import numpy as np
import torch

LATENT_SUFFIX = "_latent2x.pt"


def latent_path(audio_path: str) -> str:
    """a/b/c/d.wav -> a/b/c/d_latent2x.pt (extract_dac_latents.py:166-168)."""
    return os.path.splitext(audio_path)[0] + LATENT_SUFFIX


@torch.inference_mode()
def latent_record(model, audio, sample_rate: int, original_path: str = "") -> Dict:
    """Encodes one mono waveform (numpy or torch, [T]) and returns the reference's latent dict (CPU tensors)."""
    if sample_rate != model.sample_rate:
        raise ValueError(f"audio must be resampled to {model.sample_rate} Hz first (got {sample_rate})")
    audio = torch.as_tensor(np.asarray(audio) if not torch.is_tensor(audio) else audio).float().reshape(-1)
    dev = next(model.parameters()).device
    x = torch.clamp(audio.to(dev).reshape(1, 1, -1), -1.0, 1.0)
    z, mu, logs = model.encode(x, sample_rate)
    z, mu, logs = z.squeeze(0).cpu(), mu.squeeze(0).cpu(), logs.squeeze(0).cpu()
    n = audio.numel()
    return {
        "z": z, "mu": mu, "logs": logs,
        "sample_rate": sample_rate,
        "compression_ratio": x.shape[-1] // z.shape[-1],
        "original_duration": n / sample_rate,
        "original_samples": n,
        "latent_shape": list(z.shape),
        "original_path": original_path,
    }


@torch.inference_mode()
def latent_records(model, audios, sample_rate: int, original_paths: List[str] = None) -> List[Dict]:
    """latent_record for a list of mono waveforms of any lengths in ONE encode (model.encode_batch: a zero-padded batch whose
    members keep the values of their own unpadded encode): the dict of latent_record per clip, same clamp, same fields."""
    if sample_rate != model.sample_rate:
        raise ValueError(f"audio must be resampled to {model.sample_rate} Hz first (got {sample_rate})")
    if original_paths is not None and len(original_paths) != len(audios):
        raise ValueError(f"{len(original_paths)} paths for {len(audios)} clips")
    dev = next(model.parameters()).device
    clips = [torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).float().reshape(-1) for a in audios]
    outs = model.encode_batch([torch.clamp(c.to(dev), -1.0, 1.0) for c in clips])
    recs = []
    for i, (c, (z, mu, logs)) in enumerate(zip(clips, outs)):
        z, mu, logs = z.cpu(), mu.cpu(), logs.cpu()
        n = c.numel()
        recs.append({
            "z": z, "mu": mu, "logs": logs,
            "sample_rate": sample_rate,
            "compression_ratio": n // z.shape[-1],
            "original_duration": n / sample_rate,
            "original_samples": n,
            "latent_shape": list(z.shape),
            "original_path": original_paths[i] if original_paths is not None else "",
        })
    return recs


@torch.inference_mode()
def reconstruction_info(model, audio, sample_rate: int, original_path: str = "") -> Dict:
    """How well does this checkpoint reconstruct one mono waveform?  The comparison half of extract_dac_latents.py (:57-106
    decode_and_save_sample, without its file writes): the clip is clamped to [-1, 1] and encoded unpadded as latent_record does,
    decoded, the reconstruction limited to [-1, 1] and both trimmed to the shorter; returns the `info` dict of :98-106
    (`mse`, `snr` as numpy computes them there) plus mmx.metrics.audio_distance's values (mel, stft, l1, sisdr_db) and the
    reconstructed audio (`reconstructed`, a device tensor [n]).  One encode, one decode and one set of metric launches; the
    first host sync is the read-back of the six numbers at the end."""
    from mmx import metrics
    if sample_rate != model.sample_rate:
        raise ValueError(f"audio must be resampled to {model.sample_rate} Hz first (got {sample_rate})")
    audio = torch.as_tensor(np.asarray(audio) if not torch.is_tensor(audio) else audio).float().reshape(-1)
    dev = next(model.parameters()).device
    x = torch.clamp(audio.to(dev).reshape(1, 1, -1), -1.0, 1.0)
    z, _, _ = model.encode(x, sample_rate)
    rec = model.decode(z).reshape(-1)
    n = min(x.shape[-1], rec.numel())
    d = metrics.audio_distance(rec[None, :n], x.reshape(1, -1)[:, :n], sample_rate, clip=1.0)
    vals = torch.stack([d[k][0] for k in ("mse", "snr_db", "mel", "stft", "l1", "sisdr_db")]).cpu().tolist()     # the one sync
    return {
        "original_path": original_path,
        "original_duration": audio.numel() / sample_rate,
        "reconstructed_duration": rec.numel() / sample_rate,
        "latent_shape": list(z.squeeze(0).shape),
        "compression_ratio": x.shape[-1] // z.shape[-1],
        "mse": vals[0], "snr": vals[1], "mel": vals[2], "stft": vals[3], "l1": vals[4], "sisdr_db": vals[5],
        "reconstructed": torch.clamp(rec, -1.0, 1.0),
    }


def save_latents(model, audios, sample_rate: int, audio_paths: List[str]) -> List[str]:
    """latent_records, each written as `<audio stem>_latent2x.pt` next to its audio file; returns the paths written."""
    outs = []
    for rec, path in zip(latent_records(model, audios, sample_rate, audio_paths), audio_paths):
        out = latent_path(path)
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        torch.save(rec, out)
        outs.append(out)
    return outs


def save_latent(model, audio, sample_rate: int, audio_path: str) -> str:
    """Encodes and writes `<audio stem>_latent2x.pt` next to the audio file; returns the path written."""
    rec = latent_record(model, audio, sample_rate, audio_path)
    out = latent_path(audio_path)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    torch.save(rec, out)
    return out


def load_speech_latent(path: str, speech_token: List[int] = None, token_latent_ratio: int = 2) -> Tuple[torch.Tensor, List[int]]:
    """Reads a latent file as the TTS side does (processor.py:149-159): returns (speech_latent [T, D], speech_token),
    trimmed so that T == token_latent_ratio * len(speech_token) when a ratio and tokens are given."""
    rec = torch.load(path, map_location="cpu", weights_only=False)
    lat = rec["z"].transpose(0, 1)
    if token_latent_ratio != 0 and speech_token is not None:
        token_len = int(min(lat.shape[0] / token_latent_ratio, len(speech_token)))
        lat = lat[:token_latent_ratio * token_len]
        speech_token = speech_token[:token_len]
    return lat, speech_token
