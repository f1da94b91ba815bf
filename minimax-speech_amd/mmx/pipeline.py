"""End-to-end TTS hot path: text ids -> (LM) FSQ speech tokens -> (flow) DAC-VAE latents -> (DAC decoder) waveform.

This is the glue the reference leaves unwritten (speech/inference.py is empty): it follows
CosyVoice2Model.tts / token2wav (speech/cosyvoice/cli/model.py:285-386, non-streaming branch) with the HiFT
vocoder call (model.py:316) replaced by DACVAE.decode, as the README pipeline and the flow's training target
(speech_latent, flow.py:388-389) imply.
"""
import os
import queue
import threading
import time
from types import SimpleNamespace
from typing import Dict, List, Optional

import torch

from . import ops
from ._lib import BF16, F32, TORCH_DT, X2, X3, is_split
from .dac import DacDecoderEngine
from .flow import FlowEngine, Graphed
from .llm import ST_ERR, ST_FIN, ST_NOUT, ST_POS, LlmEngine
from .sched import GroupScheduler, groups

TOKEN_RATE = 25          # FSQ tokens per second (config.yaml:12)
SAMPLE_RATE = 24000


def step_bounds(n_text, exact_steps, min_ratio=2, max_ratio=20):
    """(min_len, max_len) of one decode: the text length times the ratios (llm.py:706-707), or exactly exact_steps with EOS ignored."""
    return (exact_steps, exact_steps) if exact_steps is not None else (int(n_text * min_ratio), int(n_text * max_ratio))


def _own(v, b):
    """Utterance b's value of an optional per-utterance argument: None, one value for all, or a list (entries may be None)."""
    return v[b] if isinstance(v, (list, tuple)) else v


def fade_in_out(fade_in, fade_out, window):
    """speech/cosyvoice/utils/common.py:142-150 on device tensors: the head of `fade_in` is mixed with the tail of
    `fade_out` over the two halves of `window`."""
    n = window.shape[0] // 2
    out = fade_in.clone()
    out[..., :n] = out[..., :n] * window[:n] + fade_out[..., -n:] * window[n:]
    return out


class TtsEngine:
    def __init__(self, llm_sd, flow_sd, dac_sd, dtype=BF16, device="cuda", max_batch=1, max_ctx=2048,
                 dac_rates=(5, 4, 4, 3, 2), use_graphs=True, attn="bf16", wplanes=False, s3tok_sd=None, dacenc_sd=None,
                 dacenc_rates=(2, 3, 4, 4, 5), dacenc_fused=False):
        """dacenc_fused: the DAC-VAE encoder runs the ResidualUnits of its 64- and 128-channel stages as one kernel each
        (DacEncoderEngine(fuse_ru=True)); off by default, which keeps the prompt latents' bits.
        wplanes (split build only): the weight-plane mode for checkpoints whose weights are NOT bf16-representable - what the
        reference's loaders hand over (fp32 llm.pt / flow.pt, cli/model.py:67-75; trained weight norms, dac-vae/inference.py:42-46).
        Every GEMM weight is carried as bf16 planes of its fp32 value (3 in the LM, 2 in the flow and the DAC: include/mmx_hip.h
        MMX_X3W / MMX_X2W) and the products keep every term above the last kept bit, so ids identical / waveform <= 1e-3 hold on
        such checkpoints too (tests/test_gpu_split.py::test_weight_planes_*)."""
        self.dtype, self.dev = dtype, torch.device(device)
        self.wplanes = wplanes if is_split(dtype) else False        # True / False / "auto" (per model: ops.resolve_wplanes)
        if self.dev.type == "cuda" and self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        device = self.dev
        # the split build: the flow and the DAC keep 16 significant bits of every activation (X2: waveform error ~1e-4),
        # the LM 24 (X3): its sampler turns a log-prob error into a different token id, and the AR loop feeds that back
        ldt = X3 if is_split(dtype) else dtype
        self.llm = LlmEngine(llm_sd, dtype=ldt, device=device, max_batch=max_batch, max_ctx=max_ctx, use_graphs=use_graphs,
                             wplanes=self.wplanes)
        # the decode step costs ~40 % more at 17..32 rows than at <= 16 (two MFMA row tiles): once at most 16
        # sequences are still running the batch continues in a 16-slot engine over the same weights and KV pages
        self.llm_small = (LlmEngine(None, dtype=ldt, device=device, max_batch=16, max_ctx=max_ctx, use_graphs=use_graphs,
                                    share_from=self.llm) if max_batch > 16 else None)
        self.flow = FlowEngine(flow_sd, dtype=dtype, device=device, use_graphs=use_graphs, attn=attn, wplanes=self.wplanes)
        self.dac = DacDecoderEngine(dac_sd, list(dac_rates), dtype=dtype, device=device, wplanes=self.wplanes)
        self.hop = self.dac.hop
        # zero-shot prompts from a raw clip (prompt_from_audio): the S3 speech tokenizer and the DAC-VAE encoder, built on first use
        self._s3tok_sd, self._dacenc_sd, self._dacenc_rates = s3tok_sd, dacenc_sd, list(dacenc_rates)
        self._s3tok = self._dacenc = None
        self.dacenc_fused = bool(dacenc_fused)
        # tts_batch's cost model of its own stages (ms): a decode step beside the flow; a flow group = group_ms + frame_ms per frame.
        # Initial values: what _refit_sched measures for this build on one MI355X on the config-4 share (it re-measures them in
        # every call: self.sched_fit; sched_adapt lets the model follow the fit)
        self.sched = ({"step_ms": 1.05, "group_ms": 47.0, "frame_ms": 0.026} if is_split(dtype) else
                      {"step_ms": 0.84, "group_ms": 35.0, "frame_ms": 0.009})
        self.sched_fit, self._sched_prev = None, None

    # auxiliary streams per flow group for its per-utterance stages (conformer encoder, DAC decode); 1 = off.  Off by default:
    # measured on the config-4 rank share, 2 / 3 / 4 streams cost 15 % / 13 % / 32 % of the step (more queues beside the decode
    # loop slow its launches more than the per-utterance stages gain); useful only without a decode loop alongside
    group_fan = 1
    batch_encoder = True      # the conformer encoder of a flow group runs as one zero-padded batch (FlowEngine.encode_batch)
    batch_dac = True          # ... and so does its DAC decode (DacDecoderEngine.decode_time_major with per-member lengths)

    flow_priority = 0      # HIP stream priority of the flow workers' streams (the decode loop runs at -1 = high)

    def _flow_stream(self):
        """A flow worker's stream.  Priorities outside torch's range (HIP has a low level, +1) go through
        hipStreamCreateWithPriority and torch.cuda.ExternalStream."""
        if self.flow_priority in (0, -1):
            return torch.cuda.Stream(device=self.dev, priority=self.flow_priority)
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        h = ctypes.c_void_p()
        with torch.cuda.device(self.dev):
            rc = hip.hipStreamCreateWithPriority(ctypes.byref(h), ctypes.c_uint(0), ctypes.c_int(self.flow_priority))
        if rc != 0:
            raise RuntimeError(f"hipStreamCreateWithPriority({self.flow_priority}) -> {rc}")
        self.__dict__.setdefault("_ext_streams", []).append(h)
        return torch.cuda.ExternalStream(h.value, device=self.dev)

    def _aux_streams(self, cur, n):
        """n auxiliary streams belonging to the stream `cur` (one set per flow worker stream; created once)."""
        pool = self.__dict__.setdefault("_aux", {})
        key = cur.cuda_stream
        if key not in pool or len(pool[key]) < n:
            pool[key] = [torch.cuda.Stream(device=self.dev, priority=0) for _ in range(n)]
        return pool[key][:n]

    def close(self):
        """Destroys every recorded hipGraph of the engines on the calling thread (deterministic teardown: nothing is left
        for Python's cyclic collector to finalise later on whatever thread it happens to run)."""
        self.llm.close()
        if self.llm_small is not None:
            self.llm_small.close()
        for fl in getattr(self, "_flows", [self.flow]):
            fl.close()
        self.flow.close()

    @torch.no_grad()
    def generate_tokens(self, texts: List[torch.Tensor], prompt_texts=None, prompt_speech=None, seed=0,
                        min_ratio=2, max_ratio=20, exact_steps=None, samplers=None, seeds=None) -> List[torch.Tensor]:
        """Batched AR decode (Qwen2LM.inference semantics per sequence). exact_steps (int or list) forces exactly
        that many sampling steps with EOS ignored (BASELINE config 3: 250 steps for a 10 s utterance).
        samplers / seeds: per utterance (LlmEngine.start); None = the LM engine's sampler attributes and the scalar `seed`."""
        assert len(texts) == self.llm.B
        xs = [self.llm.build_lm_input(t, self._prompt(_own(prompt_texts, b)), self._prompt(_own(prompt_speech, b)))
              for b, t in enumerate(texts)]
        mins, maxs = zip(*(step_bounds(t.numel(), _own(exact_steps, b), min_ratio, max_ratio) for b, t in enumerate(texts)))
        self.llm.start(xs, list(mins), list(maxs), seed=seed, samplers=samplers, seeds=seeds)
        self.llm.run(max(maxs))
        return self.llm.accepted()

    def _prompt(self, x, feat=False):
        """A prompt argument, None = no prompt: zero tokens [1, 0] (text, LM / flow speech tokens) or, feat=True, latents [1, 0, 80]."""
        if x is not None:
            return x
        return torch.zeros(1, 0, 80, device=self.dev) if feat else torch.zeros(1, 0, dtype=torch.long, device=self.dev)

    def _latents2wav(self, lat):
        """fp32 latents [T, 80] -> waveform [1, 1, T * hop]: copied into the compute dtype, then the DAC decoder.  A list of two or
        more: ONE decode of the zero-padded group (DacDecoderEngine.decode_time_major with per-member lengths: row masks in the
        GEMM epilogues, lengths in the fused ResidualUnits) instead of ~32 launches per utterance; member i of the result,
        wav[i, :, :T_i * hop], equals its own decode bit for bit.  (One utterance passes no lengths: they only add mask launches.)"""
        lats = list(lat) if isinstance(lat, (list, tuple)) else [lat]
        Ts = [int(l.shape[0]) for l in lats]
        alloc = torch.zeros if len(lats) > 1 else torch.empty            # padding rows are read: zero filled
        zt = alloc(len(lats), max(Ts), 80, dtype=TORCH_DT[self.dtype], device=self.dev)
        for i, l in enumerate(lats):
            ops.copy2d(l.contiguous(), F32, 0, 80, 1, zt[i], self.dtype, 0, 80, 1, rows=Ts[i], cols=80)
        return self.dac.decode_time_major(zt, len(lats), max(Ts), lens=(Ts if len(lats) > 1 else None))

    def _level(self, wavs, loudness_db, rate=SAMPLE_RATE):
        """Level matching of finished audio (mmx.loudness.normalize: BS.1770 integrated loudness brought to loudness_db LUFS, the
        peak kept at or below 1.0; DACVAE.decompress's last step, dac-vae/base.py:285).  wavs: one waveform or a list, each of any
        shape holding one mono clip; loudness_db: None (the input itself, nothing is launched), a float, or for a list one entry per
        waveform (None entries stay as they are).  Every clip is metered alone, so its result does not depend on its companions;
        the clips that share a target share one launch sequence.  No host sync."""
        if loudness_db is None or (isinstance(loudness_db, (list, tuple)) and all(d is None for d in loudness_db)):
            return wavs
        from .loudness import normalize
        if not isinstance(wavs, (list, tuple)):
            return normalize([wavs.reshape(-1)], rate, float(loudness_db))[0][0].reshape(wavs.shape)
        if isinstance(loudness_db, (list, tuple)) and len(loudness_db) != len(wavs):
            raise ValueError("loudness_db: one value, or one entry per utterance")
        dbs = [_own(loudness_db, b) for b in range(len(wavs))]
        out = list(wavs)
        for db in sorted({float(d) for d in dbs if d is not None}):
            idx = [b for b, d in enumerate(dbs) if d is not None and float(d) == db]
            for b, w in zip(idx, normalize([wavs[b].reshape(-1) for b in idx], rate, db)[0]):
                out[b] = w.reshape(wavs[b].shape)
        return out

    def _gate(self, wavs, rates, denoise):
        """Spectral-gate noise reduction of recordings before anything else sees them (mmx.denoise.spectral_gate, the reference's
        NoiseReduce / SpectralGate).  wavs: a list of mono clips [n] on the device at `rates`; denoise: per clip None (the clip as it
        is: nothing is launched) or a dict of spectral_gate's keywords, of which `noise` is required: a noise clip, or (start, stop)
        in samples of the clip itself.  The clips that share a rate and a gate setting form one launch sequence; each is gated on its
        own grid, so its result is that of its solo call, bit for bit.  No host sync."""
        from .denoise import _is_span, spectral_gate
        out, groups = list(wavs), {}
        for i, d in enumerate(denoise):
            if d is None:
                continue
            d = dict(d)
            if "noise" not in d:
                raise ValueError("denoise: the dict needs `noise` (a noise clip, or (start, stop) in samples of the clip itself)")
            if d.pop("return_mask", False) or "lens" in d:
                raise ValueError("denoise: return_mask and lens are not engine arguments")
            nz, amount = d.pop("noise"), d.pop("denoise_amount", 1.0)
            if _is_span(nz):
                a, b = nz
                if not 0 <= a < b <= wavs[i].numel():
                    raise ValueError(f"denoise: the noise span ({a}, {b}) does not lie inside a clip of {wavs[i].numel()} samples")
                nz = wavs[i][a:b]
            groups.setdefault((int(rates[i]), tuple(sorted(d.items()))), []).append((i, nz.to(self.dev, torch.float32).reshape(-1), float(amount)))
        for (_, setting), members in groups.items():
            gated = spectral_gate([wavs[i] for i, _, _ in members], [nz for _, nz, _ in members],
                                  denoise_amount=[a for _, _, a in members], **dict(setting))
            for (i, _, _), w in zip(members, gated):
                out[i] = w
        return out

    def _degrade(self, wavs, rates, degrade):
        """Room, noise and channel simulation of recordings before anything else sees them (mmx.degrade, mmx.channel: the
        reference's RoomImpulseResponse / BackgroundNoise / LowPass / HighPass / Equalizer / ClippingDistortion / Quantization /
        MuLawQuantization transforms).  wavs: a list of mono clips [n] on the device at `rates`; degrade: per clip None (the clip as
        it is: nothing is launched) or a dict with at least one effect: `ir` (an impulse response at the clip's rate; optional `drr`,
        `wrap`, `start_at_max`, `ir_eq`), `noise` (optional `snr`, default 10 dB, and `noise_eq`), `low_pass` / `high_pass` (a cutoff in
        Hz), `eq` (an equalizer curve [n_bands]), `clip` (a percentile in [0, 1]), `quantize` / `mulaw` (channels).  The order is
        room, noise, band limits (low pass, then high pass), equalizer, clipping, quantizer (uniform, then mu-law).  The clips that
        share a rate and a setting form one launch sequence; each clip's result is that of its solo call, bit for bit.  No host
        sync."""
        from . import channel as CH
        from .degrade import apply_ir, mix
        effects = ("ir", "noise", "low_pass", "high_pass", "eq", "clip", "quantize", "mulaw")
        out, groups = list(wavs), {}
        for i, d in enumerate(degrade):
            if d is None:
                continue
            d = dict(d)
            e = {k: d.pop(k, None) for k in effects + ("ir_eq", "noise_eq")}
            drr, snr = d.pop("drr", None), d.pop("snr", 10.0)
            wrap, at_max = bool(d.pop("wrap", True)), bool(d.pop("start_at_max", True))
            if d or all(e[k] is None for k in effects) or (e["ir_eq"] is not None and e["ir"] is None) or \
                    (e["noise_eq"] is not None and e["noise"] is None):
                raise ValueError(f"degrade: a dict with at least one of {', '.join(effects)} (and drr, wrap, start_at_max, ir_eq with "
                                 f"`ir`; snr, noise_eq with `noise`); got {sorted(k for k in e if e[k] is not None)} and {sorted(d)}")
            dev = lambda t: None if t is None else t.to(self.dev, torch.float32).reshape(-1)
            curve = lambda c: None if c is None else [float(v) for v in (c.reshape(-1).tolist() if hasattr(c, "reshape") else c)]
            e.update(ir=dev(e["ir"]), noise=dev(e["noise"]), drr=drr, snr=float(snr), **{k: curve(e[k]) for k in ("eq", "ir_eq", "noise_eq")})
            form = tuple(None if e[k] is None else len(e[k]) if isinstance(e[k], list) else True for k in effects + ("ir_eq", "noise_eq"))
            groups.setdefault((int(rates[i]), form, wrap, at_max), []).append((i, e))
        for (rate, _, wrap, at_max), members in groups.items():
            clips, first = [out[i] for i, _ in members], members[0][1]
            col = lambda k: [e[k] for _, e in members]
            if first["ir"] is not None:
                drrs = col("drr")
                clips = apply_ir(clips, col("ir"), rate, drr=None if all(v is None for v in drrs) else drrs, start_at_max=at_max,
                                 wrap=wrap, ir_eq=None if first["ir_eq"] is None else col("ir_eq"))
            if first["noise"] is not None:
                clips = mix(clips, col("noise"), rate, snr=col("snr"), noise_eq=None if first["noise_eq"] is None else col("noise_eq"))
            if first["low_pass"] is not None:
                clips = CH.low_pass(clips, col("low_pass"), rate)
            if first["high_pass"] is not None:
                clips = CH.high_pass(clips, col("high_pass"), rate)
            if first["eq"] is not None:
                clips = CH.equalizer(clips, col("eq"), rate)
            if first["clip"] is not None:
                clips = CH.clip_distortion(clips, col("clip"))
            if first["quantize"] is not None:
                clips = CH.quantization(clips, col("quantize"))
            if first["mulaw"] is not None:
                clips = CH.mulaw_quantization(clips, col("mulaw"))
            for (i, _), w in zip(members, clips):
                out[i] = w
        return out

    @torch.no_grad()
    def token2wav(self, token: torch.Tensor, prompt_token: torch.Tensor, prompt_feat: torch.Tensor,
                  embedding: torch.Tensor, streaming=False, finalize=True, loudness_db=None) -> torch.Tensor:
        """tokens [1,L] -> waveform [1, 1, 2*L*hop] (cli/model.py:285-319 with the vocoder swapped for DAC).
        loudness_db: the waveform is brought to that integrated loudness (LUFS, peak <= 1.0; _level); None leaves it as decoded."""
        wav = self._latents2wav(self.flow.inference_time_major(token, prompt_token, prompt_feat, embedding, streaming, finalize))
        return self._level(wav, loudness_db)

    @torch.no_grad()
    def reference_embedding(self, reference_audio, sample_rate=24000, cache=None, resample=False) -> torch.Tensor:
        """A reference recording (a mono clip [n] / [1, n] on the device at `sample_rate`, or a list of clips of one speaker)
        -> the speaker embedding [1, 192] the flow is conditioned on: crop + peak gain, mmx_logmel, the learnable speaker
        encoder (SpeakerEncoderEngine.embed_audio).  Needs a flow checkpoint with `speaker_encoder.*` (use_speaker_encoder: True).
        cache (a dict): one embedding per distinct clip object.
        resample=True: a recording at another rate is first brought to the mel tables' 24 kHz (mmx.resample, one launch for the
        list) and embedded at that rate; the default crops in seconds of `sample_rate` and analyses the samples as they are."""
        if self.flow.spk_enc is None:
            raise RuntimeError("reference_audio needs the learnable speaker encoder: the flow state dict has no speaker_encoder.* "
                               "weights (speech/config.yaml use_speaker_encoder: True)")
        key = id(reference_audio)
        if cache is not None and key in cache:
            return cache[key][1]
        clips = list(reference_audio) if isinstance(reference_audio, (list, tuple)) else [reference_audio]
        if resample and sample_rate != SAMPLE_RATE:
            from .resample import resample as resample_clips
            clips, sample_rate = resample_clips(clips, sample_rate, SAMPLE_RATE), SAMPLE_RATE
        e = self.flow.spk_enc.embed_audio(clips, sample_rate)
        if cache is not None:
            cache[key] = (reference_audio, e)              # the clip is kept alive with its id
        return e

    @property
    def s3tok(self):
        """The speech tokenizer engine of `s3tok_sd` (mmx/s3tok.py), built on first use."""
        if self._s3tok is None:
            if self._s3tok_sd is None:
                raise RuntimeError("prompt_from_audio needs the speech tokenizer: pass s3tok_sd (a state dict with S3TokenizerV2's keys)")
            from .s3tok import SpeechTokenizerEngine
            # weight planes are resolved from the tokenizer's own weights (its real checkpoint is fp32) unless they are forced on
            self._s3tok = SpeechTokenizerEngine(self._s3tok_sd, dtype=self.dtype, device=self.dev,
                                                wplanes=True if self.wplanes is True else None)
        return self._s3tok

    @property
    def dacenc(self):
        """The DAC-VAE encoder engine of `dacenc_sd`, built on first use."""
        if self._dacenc is None:
            if self._dacenc_sd is None:
                raise RuntimeError("prompt_from_audio needs the DAC-VAE encoder: pass dacenc_sd (encoder.* and en_conv_post.* weights)")
            from .dac import DacEncoderEngine
            self._dacenc = DacEncoderEngine(self._dacenc_sd, self._dacenc_rates, dtype=self.dtype, device=self.dev,
                                            fuse_ru=self.dacenc_fused)
        return self._dacenc

    @torch.no_grad()
    def prompt_from_audio(self, wave16k, wave24k, prompt_text=None, noise=None, generator=None) -> dict:
        """A zero-shot prompt from one recording given at both rates (mono [n] / [1, n] on the device; prompt_from_clip
        takes one clip and resamples it): frontend_zero_shot's speech part (cli/frontend.py:157-174).  wave16k -> speech tokens (the S3 tokenizer), wave24k
        -> prompt latents (DACVAE.encode's z, as processor.py:149-159 reads them; `noise` / `generator` as DacEncoderEngine.encode)
        and, where the flow has its speaker encoder, the embedding.  token_len = min(latent frames // 2, tokens); tokens are cut
        to token_len and the latents to 2 * token_len.  The result splats into tts / tts_stream:
        eng.tts(text, **eng.prompt_from_audio(w16, w24, prompt_text)) (pass flow_embedding= beside it when the flow has no
        speaker encoder)."""
        w24 = wave24k.to(self.dev, torch.float32).reshape(1, 1, -1)
        tok = self.s3tok.tokenize([wave16k.to(self.dev)])[0]
        z = self.dacenc.encode(torch.clamp(w24, -1.0, 1.0), noise=noise, generator=generator)[0]          # [1, 80, T']
        return self._prompt_dict(tok, z, w24, prompt_text)

    def _prompt_dict(self, tok, z, w24, prompt_text):
        """The dict of prompt_from_audio from a clip's speech tokens [n], prompt latents z [1, 80, T'] and 24 kHz samples."""
        token_len = min(z.shape[2] // 2, tok.numel())
        tok = tok[:token_len].to(torch.long).reshape(1, -1)
        out = {"llm_prompt_speech_token": tok, "flow_prompt_speech_token": tok,
               "prompt_speech_feat": z[:, :, :2 * token_len].transpose(1, 2).contiguous()}
        if prompt_text is not None:
            out["prompt_text"] = prompt_text
        if self.flow.spk_enc is not None:
            out["flow_embedding"] = self.reference_embedding(w24.reshape(-1), 24000)
        return out

    @torch.no_grad()
    def prompt_from_clip(self, wave, sample_rate, prompt_text=None, noise=None, generator=None, via_16k=True, normalize_db=None,
                         denoise=None, degrade=None) -> dict:
        """prompt_from_audio from ONE recording (mono [n] / [1, n]) at any rate: the two resamplings happen here, on the device
        (mmx.resample.Resample).  via_16k=True is the reference's inference route: the file is brought to 16 kHz
        (utils/file_utils.py:44-50 load_wav) and the features are taken from THAT clip brought to 24 kHz (cli/frontend.py:157-162);
        via_16k=False brings the source to each rate directly, as the dataset tools do (tools/extract_speech_token.py:30,
        tools/extract_embedding.py:30).  A rate that is already the wanted one is not resampled.
        normalize_db: the clip is first brought to that integrated loudness at its own rate (LUFS, peak <= 1.0; _level, as
        DACVAE.compress normalises to -16 before it encodes, dac-vae/base.py:166-180), so tokens, latents and embedding all see the
        same level-matched clip; None takes the clip at the level it has.
        denoise: None (the clip as recorded: nothing is launched), or a dict of mmx.denoise.spectral_gate's keywords of which
        `noise` is required (a noise clip, or (start, stop) in samples of this clip: the room tone before the speaker starts).  The
        gate runs at the clip's own rate BEFORE the level matching, so the meter hears the cleaned speech.
        degrade: None (nothing is launched), or a dict with `ir` (plus optional `drr`, `wrap`, `start_at_max`) and / or `noise` plus
        `snr`: the room and the noise of mmx.degrade (_degrade), at the clip's own rate, IR first and then noise, BEFORE denoise and
        the level matching - so a degraded and then cleaned prompt is expressible.  The dict also takes the channel effects of
        mmx.channel, applied after room and noise in this order: `low_pass`, `high_pass` (Hz), `eq` (a curve [n_bands]), `clip` (a
        percentile), `quantize`, `mulaw` (channels); and `ir_eq` / `noise_eq`, equalizer curves for the IR and the noise."""
        from .resample import Resample
        w = wave.to(self.dev, torch.float32).reshape(-1)
        if degrade is not None:
            w = self._degrade([w], [int(sample_rate)], [degrade])[0]
        if denoise is not None:
            w = self._gate([w], [int(sample_rate)], [denoise])[0]
        w = self._level(w, normalize_db, int(sample_rate))
        w16 = Resample(sample_rate, 16000)(w)
        w24 = Resample(16000, SAMPLE_RATE)(w16) if via_16k else Resample(sample_rate, SAMPLE_RATE)(w)
        return self.prompt_from_audio(w16, w24, prompt_text, noise, generator)

    @torch.no_grad()
    def prompts_from_clips(self, waves, sample_rates, prompt_texts=None, noises=None, generator=None, via_16k=True,
                           normalize_db=None, denoise=None, degrade=None) -> List[dict]:
        """prompt_from_clip for a list of recordings (mono [n] / [1, n]; sample_rates: one rate or one per clip) with the batched
        stages run once: the clips that share a rate go through ONE resample launch per target rate (mmx.resample.resample),
        all of them through ONE speech-tokenizer batch and ONE DAC-VAE encode (DacEncoderEngine.encode_ragged); the speaker
        embedding stays one reference_embedding per clip.  Entry i is the dict prompt_from_clip(waves[i], ...) returns, bit for
        bit where noises[i] [80, frames] is given (a `generator` instead gives one draw for the batch, each clip its own rows).
        normalize_db (one value, or one per clip with None entries): as prompt_from_clip, each clip metered alone at its own rate,
        the clips that share a rate and a target in one launch sequence.
        denoise (one dict for all, or one per clip with None entries left alone): as prompt_from_clip, before the level matching;
        the clips that share a rate and a gate setting in one launch sequence.
        degrade (one dict for all, or one per clip with None entries left alone): as prompt_from_clip, before denoise; the clips that
        share a rate and a setting in one launch sequence."""
        from .resample import resample as resample_clips
        n = len(waves)
        rates = [int(sample_rates)] * n if isinstance(sample_rates, (int, float)) else [int(r) for r in sample_rates]
        if len(rates) != n or (prompt_texts is not None and len(prompt_texts) != n) or (noises is not None and len(noises) != n):
            raise ValueError("prompts_from_clips: sample_rates, prompt_texts and noises are per clip")
        if n == 0:
            return []
        ws = [w.to(self.dev, torch.float32).reshape(-1) for w in waves]
        if isinstance(normalize_db, (list, tuple)) and len(normalize_db) != n:
            raise ValueError("prompts_from_clips: normalize_db is one value or per clip")
        if isinstance(denoise, (list, tuple)) and len(denoise) != n:
            raise ValueError("prompts_from_clips: denoise is one dict or per clip")
        if isinstance(degrade, (list, tuple)) and len(degrade) != n:
            raise ValueError("prompts_from_clips: degrade is one dict or per clip")
        if degrade is not None:
            ws = self._degrade(ws, rates, [_own(degrade, i) for i in range(n)])
        if denoise is not None:
            ws = self._gate(ws, rates, [_own(denoise, i) for i in range(n)])
        if normalize_db is not None:
            for r in sorted(set(rates)):
                idx = [i for i in range(n) if rates[i] == r]
                for i, w in zip(idx, self._level([ws[i] for i in idx], [_own(normalize_db, i) for i in idx], r)):
                    ws[i] = w

        def by_rate(clips, src_rates, new):
            out = [None] * n
            for r in sorted(set(src_rates)):
                idx = [i for i in range(n) if src_rates[i] == r]
                for i, o in zip(idx, resample_clips([clips[i] for i in idx], r, new)):
                    out[i] = o
            return out
        w16 = by_rate(ws, rates, 16000)
        w24 = by_rate(w16, [16000] * n, SAMPLE_RATE) if via_16k else by_rate(ws, rates, SAMPLE_RATE)
        toks = self.s3tok.tokenize(w16)
        lat = self.dacenc.encode_ragged([torch.clamp(w, -1.0, 1.0) for w in w24], noises=noises, generator=generator)
        return [self._prompt_dict(toks[i], lat[i][0][None], w24[i].reshape(1, 1, -1), _own(prompt_texts, i)) for i in range(n)]

    @staticmethod
    def batch_prompt_args(prompts) -> dict:
        """A list of prompt dicts (prompts_from_clips / prompt_from_clip / prompt_from_audio) -> the per-utterance keyword lists
        tts_batch takes: eng.tts_batch(texts, **eng.batch_prompt_args(ps)).  flow_embeddings is left out when no prompt has one
        (a flow without its speaker encoder: pass flow_embeddings= beside it)."""
        col = lambda k: [p.get(k) for p in prompts]
        out = {"prompt_texts": col("prompt_text"), "llm_prompt_speech_tokens": col("llm_prompt_speech_token"),
               "flow_prompt_speech_tokens": col("flow_prompt_speech_token"), "prompt_speech_feats": col("prompt_speech_feat")}
        if any("flow_embedding" in p for p in prompts):
            out["flow_embeddings"] = col("flow_embedding")
        return out

    @torch.no_grad()
    def voice_conversion(self, source_wave, source_rate, flow_prompt_speech_token, prompt_speech_feat, flow_embedding, speed=1.0,
                         prompt_text=None, llm_prompt_speech_token=None, loudness_db=None) -> torch.Tensor:
        """The words of `source_wave` (mono [n] / [1, n] at `source_rate`) in the prompt's voice, non-streaming: frontend_vc
        (cli/frontend.py:205-213) and CosyVoice2.inference_vc (cli/cosyvoice.py:132-139 -> cli/model.py:331-335, the source's speech
        tokens take the place of the LM's).  Source -> 16 kHz -> the S3 tokenizer -> token2wav with the prompt -> [1, 1, 2 * tokens *
        hop].  Takes the splat of a prompt_from_clip / prompt_from_audio dict: eng.voice_conversion(src, rate, **prompt); the LM's
        keys (prompt_text, llm_prompt_speech_token) are not used.  speed != 1: the latent frames are resampled linearly in time
        to int(frames / speed) before the decoder (cli/model.py:312-315).  loudness_db: as token2wav."""
        from .resample import Resample
        w16 = Resample(source_rate, 16000)(source_wave.to(self.dev, torch.float32).reshape(-1))
        tok = self.s3tok.tokenize([w16])[0].to(torch.long).reshape(1, -1)
        if speed == 1.0:
            return self.token2wav(tok, flow_prompt_speech_token, prompt_speech_feat, flow_embedding, loudness_db=loudness_db)
        lat = self.flow.inference_time_major(tok, flow_prompt_speech_token, prompt_speech_feat, flow_embedding, False, True)
        return self._level(self._latents2wav(ops.resample_linear(lat.float().t(), int(lat.shape[0] / speed)).t().contiguous()), loudness_db)

    def _embedding_arg(self, flow_embedding, reference_audio, sample_rate):
        if (flow_embedding is None) == (reference_audio is None):
            raise ValueError("give exactly one of flow_embedding and reference_audio")
        return flow_embedding if reference_audio is None else self.reference_embedding(reference_audio, sample_rate)

    @torch.no_grad()
    def tts(self, text, flow_embedding=None, prompt_text=None, llm_prompt_speech_token=None, flow_prompt_speech_token=None,
            prompt_speech_feat=None, seed=0, exact_steps=None, reference_audio=None, sample_rate=24000, loudness_db=None) -> torch.Tensor:
        """One utterance, non-streaming (cli/model.py:321-386 `stream=False` branch).  reference_audio (instead of
        flow_embedding): the voice as a recording, see reference_embedding.  loudness_db: as token2wav."""
        flow_embedding = self._embedding_arg(flow_embedding, reference_audio, sample_rate)
        toks = self.generate_tokens([text], [prompt_text], [llm_prompt_speech_token], seed=seed, exact_steps=exact_steps)[0]
        return self.token2wav(toks.reshape(1, -1), self._prompt(flow_prompt_speech_token), self._prompt(prompt_speech_feat, feat=True),
                              flow_embedding, loudness_db=loudness_db)

    MEL_CACHE = 8            # cli/model.py:258: frames of overlap between two passes

    @staticmethod
    def fade_window(n: int, device) -> torch.Tensor:
        """np.hamming(2n) (cli/model.py:262) with each pair (w[i], w[i + n]) scaled to sum to one: a cross-fade of two equal
        signals is then the identity (the raw halves sum to 1.08)."""
        import numpy as np
        w = torch.from_numpy(np.hamming(2 * n)).float()
        s_ = w[:n] + w[n:]
        return torch.cat([w[:n] / s_, w[n:] / s_]).to(device)

    @torch.no_grad()
    def tts_stream(self, text, flow_embedding=None, seed=0, exact_steps=None, token_hop=25, latents_out=None, forced=None,
                   cache=True, prompt_text=None, llm_prompt_speech_token=None, flow_prompt_speech_token=None,
                   prompt_speech_feat=None, reference_audio=None, sample_rate=24000):
        """Streaming synthesis of one (long) utterance: BASELINE config 5 / cli/model.py:336-378 (`stream=True`), zero-shot
        prompts included (prompt_text / llm_prompt_speech_token condition the LM, llm.py:691-703; flow_prompt_speech_token /
        prompt_speech_feat the flow, flow.py:472-498).
        The AR decode runs ahead on its own stream (captured decode step).  Hop schedule as the reference: the first hop takes
        token_hop + prompt_token_pad tokens (pad = ceil(Lp / 25) * 25 - Lp, model.py:338-341), later hops token_hop; a hop runs
        once `hop + look-ahead` tokens exist and solves the chunk-causal flow over the tokens so far; the closing pass solves
        everything WITHOUT chunk masks (model.py:371-378 leaves `stream` at False).
        Rendering (the DAC decoder replaces HiFT and its mel / source caches, model.py:298-311; rule restated in
        oracle/stream.py): the DAC is NOT causal — a sample depends on `dac.ctx_left` latent frames before and `dac.ctx_right`
        after its own frame — so a pass renders the frames whose right context is final, from a window with ctx_left frames of
        ALREADY RENDERED left context; streaming passes agree on finished frames, so their chunks equal the offline decode of
        the same latents sample for sample.  Like the reference (model.py:306-311) a streaming pass holds the samples of its
        last MEL_CACHE frames back: the next streaming pass emits them unchanged, the CLOSING pass — the one seam where two
        passes disagree about the frames around it — renders those frames again from its own latents and cross-fades the two
        renderings (utils/common.py:142-150 fade_in_out, window of model.py:262 normalised to unit sum).
        Yields waveform chunks [1, n] (device); `latents_out` (a list) receives the latent frames [n, 80] each chunk was
        rendered from; `forced` [1, steps] teacher-forces the accepted ids (LlmEngine.start).  cache=True: hops solve only
        their new frames (FlowEngine.StreamState); cache=False recomputes all frames at every hop, as the reference does.
        reference_audio (instead of flow_embedding): the voice as a recording (reference_embedding), embedded once before the
        first hop.
        There is no loudness_db here: integrated loudness (mmx.loudness) is a property of the whole utterance, which a stream has
        not seen when it emits its first chunk.  Level-match the prompt (prompt_from_clip(normalize_db=...)) or the joined chunks."""
        assert self.llm.B == 1
        flow_embedding = self._embedding_arg(flow_embedding, reference_audio, sample_rate)
        fpt, pf = self._prompt(flow_prompt_speech_token), self._prompt(prompt_speech_feat, feat=True)
        x = self.llm.build_lm_input(text, self._prompt(prompt_text), self._prompt(llm_prompt_speech_token))
        mn, mx = step_bounds(int(text.numel()), exact_steps)
        if not hasattr(self, "_lm_stream"):
            self._lm_stream = torch.cuda.Stream(device=self.dev, priority=-1)
        lm, caller = self._lm_stream, torch.cuda.current_stream()
        lm.wait_stream(caller)
        L = self.flow.L
        CL, CR, MC = self.dac.ctx_left, self.dac.ctx_right, self.MEL_CACHE
        Lp = int(fpt.numel())
        pad = -(-Lp // token_hop) * token_hop - Lp              # model.py:338
        with torch.cuda.stream(lm):
            self.llm.start([x], [mn], [mx], seed=seed, forced=forced)
        done, offset = 1, 0                                  # decode steps issued, tokens consumed by hops
        emitted = 0                                          # latent frames rendered
        sstate = self.flow.stream_open(2 * (mx + Lp)) if cache else None
        tail = None                                          # the last ctx_left + MEL_CACHE rendered latent frames
        held = None                                          # samples of the last MEL_CACHE rendered frames, not yet emitted
        held_lat = None

        def render(n_tok, finalize):
            nonlocal emitted, tail, held, held_lat
            ev = torch.cuda.Event()
            ev.record(lm)
            caller.wait_event(ev)                          # tokens [0, n_tok) are written
            tok = self.llm.out_tokens[0:1, :n_tok].to(torch.int64)
            lat = self.flow.inference_time_major(tok, fpt, pf, flow_embedding, streaming=not finalize, finalize=finalize,
                                                 stream_state=sstate)
            T2 = lat.shape[0]
            hi = T2 if finalize else T2 - CR               # frames whose right context is final
            if hi <= emitted:
                return None
            # the closing pass renders the held frames again (as many as the last streaming pass held back: MEL_CACHE, or all
            # it rendered when that was fewer)
            re = held.shape[1] // self.hop if (finalize and held is not None) else 0
            start = emitted - re
            ctx = None if tail is None else tail[:tail.shape[0] - re][-CL:]
            seg = lat[start:] if ctx is None or ctx.shape[0] == 0 else torch.cat([ctx, lat[start:]], dim=0)
            nctx = 0 if ctx is None else ctx.shape[0]
            wav = self._latents2wav(seg)[:, 0, nctx * self.hop:(nctx + hi - start) * self.hop]
            lat_used = lat[emitted:hi]
            if finalize:
                if re:
                    wav = fade_in_out(wav, held, self.fade_window(re * self.hop, self.dev))
                    lat_used = torch.cat([held_lat, lat_used], 0)
                out, held, held_lat = wav, None, None
            else:
                keep = min(MC, hi - emitted)
                out = wav[:, :wav.shape[1] - keep * self.hop]
                if held is not None:
                    out = torch.cat([held, out], dim=1)
                    lat_used = torch.cat([held_lat, lat_used], 0)
                held = wav[:, wav.shape[1] - keep * self.hop:].clone()
                held_lat, lat_used = lat_used[lat_used.shape[0] - keep:].clone(), lat_used[:lat_used.shape[0] - keep]
            if latents_out is not None and lat_used.shape[0]:
                latents_out.append(lat_used.clone())
            new = lat[emitted:hi]
            tail = (new if tail is None else torch.cat([tail, new], 0))[-(CL + MC):].clone()
            emitted = hi
            return out if out.shape[1] else None

        try:
            while True:
                with torch.cuda.stream(lm):
                    st = self.llm.state[:, 0].tolist()         # D2H copy on the LM stream: waits for the steps issued so far
                self.llm.raise_nonfinite([st[ST_ERR]])
                n_out, finished = st[ST_NOUT], bool(st[ST_FIN]) or done >= mx
                this_hop = token_hop + pad if offset == 0 else token_hop          # model.py:341
                while n_out - offset >= this_hop + L:
                    w = render(offset + this_hop + L, finalize=False)
                    offset += this_hop
                    this_hop = token_hop
                    if w is not None:
                        yield w
                if finished:
                    w = render(n_out, finalize=True)
                    if w is not None:
                        yield w
                    break
                # keep the decode a few ACCEPTED tokens ahead of the renderer.  The look-ahead is counted in tokens, not in
                # steps (ids above the EOS id advance the step counter without producing a token, llm.py:755-756), and at
                # least one step is issued per round, so the loop always makes progress.
                k = min(mx - done, max(1, offset + this_hop + L + 8 - n_out))
                with torch.cuda.stream(lm):
                    for _ in range(k):
                        self.llm.step()
                done += k
        finally:
            if sstate is not None:
                self.flow.stream_close(sstate)           # the state (and its hop graphs) goes back to the pool
        caller.wait_stream(lm)

    # ------------------------------------------------------------------ batch of independent utterances
    def _flow_dac_group(self, grp, toks, embs, wavs, frame_quantum, flow=None, prompts=None):
        """Flow + DAC for a group of finished utterances: per-utterance conformer encoder, one batched ODE solve, per-
        utterance DAC decode.  prompts: per utterance (flow_prompt_speech_token [1, Lp], prompt_speech_feat [1, Tp, 80]) or
        None (flow.py:472-498: the prompt's tokens go through the encoder in front of the utterance's, its latents are the
        `cond` rows of its frames, and its frames are dropped from the result).
        MMX_TIMING=3 prints the three stage times (with stream syncs between them)."""
        flow = flow or self.flow
        pr = [_own(prompts, b) or (self._prompt(None), self._prompt(None, feat=True)) for b in grp]
        trace = os.environ.get("MMX_TIMING") == "3"
        marks = []

        def mark():
            if trace:
                torch.cuda.current_stream().synchronize()
                marks.append(time.perf_counter())

        # The conformer encoder and the DAC decode are per utterance: chains of ~100 / ~30 launches, most of them too small to
        # fill the chip.  The utterances of a group are independent there, so each goes to one of `fan` auxiliary streams
        # (forked from / joined into the group's stream with events); the batched ODE solve between them stays on the group's
        # stream.  fan = 1: everything on the group's stream.
        cur = torch.cuda.current_stream()
        fan = min(self.group_fan, len(grp))
        aux = self._aux_streams(cur, fan) if fan > 1 else []

        def fanned(jobs):
            """jobs: callables, one per utterance; run on the auxiliary streams round robin, joined before returning."""
            if not aux:
                return [j() for j in jobs]
            ev0 = torch.cuda.Event()
            ev0.record(cur)
            out = []
            for i, j in enumerate(jobs):
                st = aux[i % fan]
                st.wait_event(ev0)
                with torch.cuda.stream(st):
                    out.append(j())
            for st in aux:
                ev = torch.cuda.Event()
                ev.record(st)
                cur.wait_event(ev)
            for o in out:                                    # results live on after this call, on other streams
                for t in (o if isinstance(o, tuple) else (o,)):
                    if isinstance(t, torch.Tensor):
                        t.record_stream(cur)
            return out

        mark()
        if self.batch_encoder and len(grp) > 1:
            # one encoder pass over the zero-padded group (FlowEngine.encode_batch)
            conds = flow.conditions_batch([toks[b].reshape(1, -1) for b in grp], [p[0] for p in pr], [p[1] for p in pr],
                                          [embs[b] for b in grp])
        else:
            conds = fanned([(lambda b=b, p=p: flow.conditions(toks[b].reshape(1, -1), p[0], p[1], embs[b])) for b, p in zip(grp, pr)])
        mark()
        xs = flow.cfm_batch([c[0] for c in conds], [c[1] for c in conds], [c[2] for c in conds], pad_to=frame_quantum)
        mark()
        lats = [lat[c[3]:] for lat, c in zip(xs, conds)]     # the prompt's frames are not rendered (flow.py:509)
        if self.batch_dac and len(grp) > 1 and not aux:
            wav = self._latents2wav(lats)                    # one decode of the zero-padded group
            for i, b in enumerate(grp):
                wavs[b] = wav[i:i + 1, :, :lats[i].shape[0] * self.hop]
        else:
            for b, w in zip(grp, fanned([(lambda l=l: self._latents2wav(l)) for l in lats])):
                wavs[b] = w
        if aux:
            # blocks the auxiliary streams allocated (and this function's temporaries freed there) go back to THEIR pools:
            # nothing on them may be reused before the group's stream has finished reading it
            ev = torch.cuda.Event()
            ev.record(cur)
            for st in aux:
                st.wait_event(ev)
        mark()
        if trace:
            e, c, d = ((marks[i + 1] - marks[i]) * 1e3 for i in range(3))
            print(f"[flow_dac_group] n={len(grp)} frames={[2 * toks[b].numel() for b in grp]}: encoder {e:.1f} ms, "
                  f"cfm {c:.1f} ms, dac {d:.1f} ms", flush=True)

    @torch.no_grad()
    def tts_batch(self, texts, flow_embeddings=None, seed=0, exact_steps=None, group_size=8, max_pad_ratio=2.0,
                  frame_quantum=32, overlap=True, poll_every=8, flow_workers=2, hold_steps=60, tail_active=0, polite=True,
                  prompt_texts=None, llm_prompt_speech_tokens=None, flow_prompt_speech_tokens=None,
                  prompt_speech_feats=None, samplers=None, seeds=None, reference_audio=None, sample_rate=24000,
                  loudness_db=None) -> List[torch.Tensor]:
        """Throughput path for a batch of independent utterances (BASELINE config 4, one rank's share): one batched
        AR decode for all of them; as sequences finish (shortest first) their flow + DAC work — per-utterance
        conformer encoder, ODE solves batched over groups of similar length (zero padded + masked), DAC decode — is
        issued by a second host thread on a second HIP stream, so the latency-bound decode loop and the MFMA-bound
        flow overlap on the chip (the reference overlaps the same two stages with its llm_job thread,
        cli/model.py:332-335).  overlap=False runs the stages back to back.
        Zero-shot prompts (cli/cosyvoice.py:92-104 -> cli/model.py:321-326), each a per-utterance list or None: prompt_texts
        and llm_prompt_speech_tokens condition the LM (llm.py:691-703), flow_prompt_speech_tokens / prompt_speech_feats the
        flow (flow.py:472-498).
        samplers / seeds: per utterance, the LM sampler (dict over mode / top_p / top_k / win_size / tau_r / seed, LlmEngine.start)
        and seed of its own; None (the list or an entry) = the LM engine's sampler attributes and the scalar `seed`.
        group_size / hold_steps: a finished utterance waits at most hold_steps decode steps for up to group_size companions
        of similar length.  Large groups pay twice: a launch of the fused flow kernels costs about the same from 500 to
        8 000 rows (it is bound by every workgroup streaming the block's weights), so fewer, fuller groups are less GPU
        work, and less flow work beside the decode loop makes the decode loop itself faster (measured, 32 utterances:
        ramp 2,2,4,8 / hold 40: 718 ms per step, decode loop 617 ms; groups of 8 / hold 60: 703 ms, decode loop 577 ms);
        then its (partial) group is issued, so the flow work of the long utterances is not left for after the last
        token (the rule counts decode steps, not wall time: the schedule, and with it the set of captured plans, is
        the same from run to run).
        reference_audio: per utterance, a recording of the voice (reference_embedding) used where flow_embeddings[b] would be
        (an entry of None keeps flow_embeddings[b]); every distinct clip object is embedded once, before the decode loop starts.
        polite: flow groups issued while the decode loop runs use FlowEngine.polite tiling (64-row tiles: fewer workgroups,
        more of the chip left to the decode loop's launches); the groups of the final poll use the fastest tiling.
        tail_active > 0: once at most that many sequences are still decoding, a finished utterance no longer waits for
        companions when a flow worker is (predicted) idle - the decode loop is the critical path, and whatever the last
        utterances still have to do after their last token is what the step ends on.
        loudness_db (one value, or one per utterance with None entries): every utterance is brought to that integrated loudness
        (LUFS, peak <= 1.0; _level) once all are decoded, each metered alone: the result does not depend on groups or schedule, and
        equals mmx.loudness.normalize of the loudness_db=None result.  None: nothing is measured or launched."""
        B = len(texts)
        if reference_audio is None and flow_embeddings is None:
            raise ValueError("give flow_embeddings or reference_audio")
        if reference_audio is not None:
            assert len(reference_audio) == B
            clips = {}                                    # one embedding per distinct clip object
            flow_embeddings = [self._embedding_arg(_own(flow_embeddings, b), None, sample_rate) if clip is None else
                               self.reference_embedding(clip, sample_rate, clips) for b, clip in enumerate(reference_audio)]
        NS = self.llm.B                                   # decode slots; more utterances than slots queue up and are admitted
        assert B >= NS and (overlap or B == NS)           # into slots as they free (continuous batching, LlmEngine.admit)
        assert (samplers is None or len(samplers) == B) and (seeds is None or len(seeds) == B)
        xs = [self.llm.build_lm_input(t, self._prompt(_own(prompt_texts, b)), self._prompt(_own(llm_prompt_speech_tokens, b)))
              for b, t in enumerate(texts)]
        prompts = flow_prompt_speech_tokens and [None if fp is None else (fp, self._prompt(_own(prompt_speech_feats, b), feat=True))
                                                 for b, fp in enumerate(flow_prompt_speech_tokens)]
        plen = [int(p[0].numel()) if p else 0 for p in prompts or [None] * B]                      # prompt tokens in the flow
        mins, maxs = (list(v) for v in zip(*(step_bounds(t.numel(), _own(exact_steps, b)) for b, t in enumerate(texts))))
        wavs: List[Optional[torch.Tensor]] = [None] * B
        toks: List[Optional[torch.Tensor]] = [None] * B
        self.last_tokens, self.last_schedule = toks, None    # accepted ids per utterance (device int64 tensors); GroupScheduler.log
        if not overlap:
            self.llm.start(xs, mins, maxs, seed=seed, samplers=samplers, seeds=seeds)
            self.llm.run(max(maxs), poll_every)
            n = self.llm.state[ST_NOUT].tolist()
            toks[:] = self.llm.accepted(n=n)
            order = sorted(range(B), key=lambda b: (n[b], b))
            for grp in groups(order, [2 * (v + plen[b]) for b, v in enumerate(n)], group_size, max_pad_ratio, frame_quantum):
                self._flow_dac_group(grp, toks, flow_embeddings, wavs, frame_quantum, prompts=prompts)
            return self._level(wavs, loudness_db)

        # ---- start: flow workers, scheduler, decode loop
        if not hasattr(self, "_sides") or len(self._sides) != flow_workers:
            # the decode loop is a chain of short latency-bound kernels: give it the high-priority queue so its
            # launches are not parked behind the flow's large grids.  The flow stage itself is a chain of short
            # kernels too, so `flow_workers` host threads, each with its own stream and its own plan buffers (the
            # weights are shared), solve different groups concurrently.
            # (CU-masked flow streams, hipExtStreamCreateWithCUMask, were tried to keep CUs free for the decode loop:
            # the mask is not honoured on this pool — an 8192^3 GEMM takes the same time with 1/4 and 4/4 of the CUs)
            self._sides = [self._flow_stream() for _ in range(flow_workers)]
            self._flows = [self.flow] + [self.flow.clone_shared() for _ in range(flow_workers - 1)]
            self._hi = torch.cuda.Stream(device=self.dev, priority=-1)
        qs, err = [queue.Queue() for _ in range(flow_workers)], []
        caller, main = torch.cuda.current_stream(), self._hi
        main.wait_stream(caller)
        trace = os.environ.get("MMX_TIMING") == "2"
        group_events: list = []
        cold0 = Graphed.cold_calls
        t0 = time.perf_counter()

        def worker(wi):
            side, flow = self._sides[wi], self._flows[wi]
            try:
                torch.cuda.set_device(self.dev)
                with torch.cuda.stream(side):
                    for grp, ev, flow.polite in iter(qs[wi].get, None):
                        side.wait_event(ev)                      # the group's token ids were written on the LM stream
                        t_in = time.perf_counter()
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(side)
                        self._flow_dac_group(grp, toks, flow_embeddings, wavs, frame_quantum, flow, prompts)
                        e1.record(side)                          # read after the call has drained: the scheduler's cost model
                        group_events.append((sum(2 * toks[b].numel() for b in grp), flow.polite, e0, e1))
                        if trace:
                            side.synchronize()
                            print(f"[tts_batch]   worker {wi}: group of {len(grp)} ({[2 * toks[b].numel() for b in grp]} frames) "
                                  f"{(t_in - t0) * 1e3:.0f} -> {(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)
            except BaseException as e:                           # surfaced by the caller
                err.append(e)

        ths = [threading.Thread(target=worker, args=(wi,), daemon=True) for wi in range(flow_workers)]
        for th in ths:
            th.start()
        sch = GroupScheduler(group_size, max_pad_ratio, frame_quantum, hold_steps, tail_active, flow_workers, self.sched, B, B == NS, polite)
        self.last_schedule = sch.log
        # eng, slots: the active engine and its slot -> utterance index; waiting: utterances without a slot yet
        call = SimpleNamespace(eng=self.llm, slots=list(range(NS)), waiting=list(range(NS, B)), harvested=set(), toks=toks, plen=plen,
                               sched=sch, qs=qs, main=main, B=B, poll_every=poll_every, xs=xs, mins=mins, maxs=maxs, samplers=samplers, seeds=seeds)
        with torch.cuda.stream(main):
            self.llm.start(xs[:NS], mins[:NS], maxs[:NS], seed=seed, samplers=samplers and samplers[:NS],
                           seeds=seeds and seeds[:NS])              # (captures serialise themselves: mmx/flow.py, Graphed)
            # without a queue max(maxs) steps end every sequence; with one, admissions happen only at polls, so the loop
            # runs until every utterance has been seen (the bound only stops a runaway: each admitted utterance can wait
            # up to poll_every steps for its slot on top of its own max_len)
            done, max_steps = 1, (max(maxs) if B == NS else sum(maxs) + (B + 1) * poll_every)
            issue_s = 0.0                                        # host time spent enqueueing decode steps (graph replays)
            while done < max_steps:                              # ---- loop: k decode steps, then a poll
                k = min(poll_every, max_steps - done)
                t_i = time.perf_counter()
                for _ in range(k):
                    call.eng.step()
                issue_s += time.perf_counter() - t_i
                done += k
                self._poll_slots(call, self._poll_finished(call, done, False))
                self._poll_issue(call, done, False)
                if len(call.harvested) == B:
                    break
            if call.waiting:
                raise RuntimeError(f"tts_batch: {len(call.waiting)} queued utterances were never admitted")
            self._poll_finished(call, done, True)                # ---- final poll: whatever is left arrives, nothing is held back
            self._poll_issue(call, done, True)
        # ---- drain.  The call returns finished audio, so it drains its streams on the host as well: the decode stream here, the
        # flow streams after the workers have issued everything.  Leaving the drain to stream waits (so that the next
        # call's decode loop is already queued behind them) measured 6 % slower per step: a blocked high-priority queue
        # ahead of the still running flow tail costs the tail more than the host round trip saves.
        main.synchronize()
        t_lm = time.perf_counter()
        for qq in qs:
            qq.put(None)
        for th in ths:
            th.join()
        if err:
            raise err[0]
        for sd in self._sides:
            sd.synchronize()
        for fl in self._flows:
            fl.polite = False
        if os.environ.get("MMX_TIMING"):
            print(f"[tts_batch] LM loop done at {(t_lm - t0) * 1e3:.0f} ms, flow/DAC tail until {(time.perf_counter() - t0) * 1e3:.0f} ms, "
                  f"decode steps {done}", flush=True)
        for sd in self._sides:
            caller.wait_stream(sd)
        caller.wait_stream(main)
        # host-side accounting of the call (bench.py puts it into its JSON line: a multi-GPU node runs N x (decode thread + flow
        # workers) on shared cores, and a slow host shows up here first)
        self.last_host = dict(decode_steps=done, lm_issue_ms=round(issue_s * 1e3, 2), lm_done_ms=round((t_lm - t0) * 1e3, 1),
                              call_ms=round((time.perf_counter() - t0) * 1e3, 1))
        self._refit_sched(done, (t_lm - t0) * 1e3, group_events, steady=(Graphed.cold_calls == cold0 and B == NS))
        return self._level(wavs, loudness_db)

    def _poll_finished(self, call, step, final):
        """A poll of tts_batch's decode loop (`call`: that call's state), step 1: reads the finished flags once; the utterances that
        finished since the last poll (at the final one: all that are left) arrive at the scheduler, shortest first.  Returns the flags."""
        eng, slots = call.eng, call.slots
        st = eng.host_state()                             # (raises for a slot whose logits were not finite)
        fin, n = st[ST_FIN], st[ST_NOUT]
        new = sorted([s_ for s_ in range(len(slots)) if (fin[s_] or final) and slots[s_] not in call.harvested],
                     key=lambda s_: (n[s_], slots[s_]))
        for s_, ids in zip(new, eng.accepted(new, n)):
            b = slots[s_]
            call.harvested.add(b)
            call.toks[b] = ids
            call.sched.arrive(b, 2 * (ids.numel() + call.plen[b]), step)
        return fin

    def _poll_slots(self, call, fin):
        """Step 2, the slots: queued utterances into freed slots, KV pages for the steps up to the next poll, and the move into
        the 16-slot engine once few enough sequences are left."""
        eng, slots, harvested = call.eng, call.slots, call.harvested
        for s_ in range(len(slots)):                            # a freed slot takes the next queued utterance
            if call.waiting and fin[s_] and slots[s_] in harvested:
                b = call.waiting.pop(0)
                eng.admit(s_, call.xs[b], call.mins[b], call.maxs[b], seq_id=b, sampler=_own(call.samplers, b),
                          seed=_own(call.seeds, b))             # reserves KV pages for the whole max_len
                slots[s_], fin[s_] = b, 0
        if eng is self.llm:
            # every running sequence must own the pages the steps up to the next poll will write (a no-op when admit /
            # start reserved the whole max_len; raises when the allocator is exhausted instead of decoding into the
            # shared scratch page)
            eng.ensure_capacity(call.poll_every + 1, pos=eng.state[ST_POS].tolist(), active=[s_ for s_ in range(len(slots)) if not fin[s_]])
        if not call.waiting and self.llm_small is not None and eng is self.llm and 0 < call.B - len(harvested) <= self.llm_small.B:
            act = [s_ for s_ in range(len(slots)) if slots[s_] not in harvested]
            self.llm_small.compact_from(self.llm, act)
            call.eng, call.slots = self.llm_small, [slots[s_] for s_ in act]

    def _poll_issue(self, call, step, final):
        """Step 3: the groups the scheduler issues now, each behind an event on the decode stream, onto their workers' queues."""
        for _, wi, pol, grp in call.sched.issue(step, call.B - len(call.harvested), final):
            ev = torch.cuda.Event()
            ev.record(call.main)
            call.qs[wi].put((grp, ev, pol))

    SCHED_HYSTERESIS = 0.25
    sched_adapt = False       # True: self.sched follows the measured fit (off by default: a change of the model moves groups between
                              # workers, and a worker that meets a new group shape spends two calls capturing a plan for it)

    def _refit_sched(self, steps, lm_ms, group_events, steady=True):
        """The scheduler's cost model from this call's own clock: decode step = loop time / steps; group cost = least squares of
        (frames, HIP-event duration) over the groups that ran beside the decode loop.  self.sched_fit always holds the latest fit;
        with sched_adapt, self.sched (what the next call uses) follows it past SCHED_HYSTERESIS when two steady calls in a row gave the
        same fit, one parameter at a time."""
        if not steady:                                   # a call that captured plans (or queued utterances) times something else
            self._sched_prev = None
            return
        fit = {"step_ms": lm_ms / max(1, steps)}
        pts = [(f, e0.elapsed_time(e1)) for f, pol, e0, e1 in group_events if pol]
        if len(pts) >= 3 and len({f for f, _ in pts}) >= 2:
            n = float(len(pts))
            sx, sy = sum(f for f, _ in pts), sum(t for _, t in pts)
            sxx, sxy = sum(f * f for f, _ in pts), sum(f * t for f, t in pts)
            den = n * sxx - sx * sx
            slope = (n * sxy - sx * sy) / den if den > 0 else 0.0
            if slope > 0 and (sy - slope * sx) / n > 0:
                fit["frame_ms"], fit["group_ms"] = slope, (sy - slope * sx) / n
        prev, self._sched_prev = self._sched_prev, fit
        self.sched_fit = {k: round(v, 5) for k, v in fit.items()}
        if not self.sched_adapt:
            return
        for k, v in fit.items():
            if prev and k in prev and abs(v - prev[k]) <= 0.1 * prev[k] and abs(v - self.sched[k]) > self.SCHED_HYSTERESIS * self.sched[k]:
                self.sched[k] = round(v, 5)
