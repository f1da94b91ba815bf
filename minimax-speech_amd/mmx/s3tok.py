"""S3 speech tokenizer engine: a 16 kHz clip -> the 25 Hz FSQ speech tokens of a zero-shot prompt
(`llm_prompt_speech_token` / `flow_prompt_speech_token`).

Reference: speech/tools/S3Tokenizer/s3tokenizer/model_v2.py (S3TokenizerV2: AudioEncoderV2, FSMNMultiHeadAttention, FSQCodebook),
utils.py:220-267 (log_mel_spectrogram), :367-390 (merge_tokenized_segments); called from cli/frontend.py:92-102.  Three kernels
are the tokenizer's own (mmx_logmel_w of csrc/mel.hip; csrc/s3tok.hip: mmx_s3_rope_fsmn, mmx_fsq_encode); the two stride-2 convolutions, the
LayerNorms, the fused Q | K | V projection (a zero bias segment for K), the out-projection, the MLP and the attention run on the
entry points every other engine uses.  There is no CPU fallback: a CPU tensor raises MmxError.

segment_plan and merge_segments are pure host functions (the > 30 s path of S3TokenizerV2._quantize_mixed_batch)."""
from typing import Dict, List

import torch

from . import mel as MEL
from . import ops
from ._lib import BF16, F32, X2, X2W, MmxError, call, is_split, stream, _p
from .clips import on_device, pack

SAMPLE_RATE, N_FFT, HOP, N_MELS = 16000, 400, 160, 128
MAX_FRAMES = 3000                                        # model_v2.py:401: more mel frames than this select the windowed path
WINDOW, STRIDE = 3000, 2600                              # :443-445: 30 s windows, 4 s overlap
OVERLAP_S, TOKEN_RATE = 4, 25                            # :440, :561
ROPE_ROWS = 2048                                         # :314 precompute_freqs_cis(64, 1024 * 2)


# ----------------------------------------------------------------------------- host side (no GPU)
def frames_of(n: int) -> int:
    """Mel frames of a clip of n samples (utils.py:258-259: center=True gives n // 160 + 1 frames, the last one is dropped)."""
    return n // HOP


def conv_len(n: int) -> int:
    """Length after one k3 / stride-2 / pad-1 convolution (model_v2.py:330,333)."""
    return (n - 1) // 2 + 1


def code_len_of(frames: int) -> int:
    return conv_len(conv_len(frames))


def segment_plan(n_frames: int):
    """[(start, length), ...] of the windows S3TokenizerV2._quantize_mixed_batch (model_v2.py:454-504) encodes for a member of
    n_frames mel frames: one window for up to 3000 frames, else 3000-frame windows every 2600 frames (the last one shorter;
    each is zero padded to 3000 frames)."""
    if n_frames <= MAX_FRAMES:
        return [(0, n_frames)]
    plan, start = [], 0
    while start < n_frames:
        plan.append((start, min(start + WINDOW, n_frames) - start))
        start += STRIDE
    return plan


def merge_segments(segments, overlap=OVERLAP_S, token_rate=TOKEN_RATE):
    """utils.py:367-390 merge_tokenized_segments: keeps the middle of every window, dropping (overlap // 2) * token_rate tokens
    on each inner side."""
    drop = (overlap // 2) * token_rate
    merged = []
    for i, toks in enumerate(segments):
        lo = 0 if i == 0 else drop
        hi = -drop if i != len(segments) - 1 else len(toks)
        merged.extend(toks[lo:hi])
    return merged


def rope_tables():
    """cos / sin fp32 [2048][32] with the reference's own torch CPU calls (model_v2.py:37-48 precompute_freqs_cis(64, 2048))."""
    freqs = 1.0 / (10000.0 ** (torch.arange(0, 64, 2)[:32].float() / 64))
    t = torch.arange(ROPE_ROWS)
    cis = torch.polar(torch.ones(ROPE_ROWS, 32), torch.outer(t, freqs).float())
    real = torch.view_as_real(cis)
    return real[..., 0].contiguous(), real[..., 1].contiguous()


# ----------------------------------------------------------------------------- log-mel tables and launch
class LogMelW(MEL._LogMelTables):
    """The device tables of the Whisper-convention log-mel (utils.py:220-267: n_fft 400, hop 160, 128 mels at 16 kHz) and the
    launch of mmx_logmel_w.  The DFT basis has its K dimension zero padded from 400 to 416 columns."""

    _entry, _fp32_cm = "mmx_logmel_w", True              # the clip maximum is taken over fp32 values

    def __new__(cls, n_mels=N_MELS, device="cuda"):
        return cls._cached(device, n_mels)

    def _build(self, n_mels, dev):
        self.n_fft, self.hop, self.n_mels, self.dev = N_FFT, HOP, n_mels, dev
        self._tables(MEL.mel_filterbank(SAMPLE_RATE, N_FFT, n_mels), kp=ops.round_up(N_FFT, 32))    # librosa.filters.mel's defaults

    def frames(self, n):
        return frames_of(n)

    @torch.no_grad()
    def __call__(self, wave, lens=None, time_major=False, dtype=F32, out=None):
        """wave fp32 [B, L] (or [L]) on the device, zero padded where `lens` (a list of ints) gives fewer valid samples per member
        -> log-mel [B, n_mels, T] fp32 (the reference function's layout), or with time_major=True [B, T, n_mels] in the activation
        type of `dtype` (into `out` when given).  T = the frames of the longest member; a shorter member's remaining frames are 0."""
        return self._run(wave, lens, None, time_major, dtype, out)


# ----------------------------------------------------------------------------- the two other kernels
def s3_rope_fsmn(qkv, x, r, wt, rope_cos, rope_sin, *, B, T, C_, lens=None):
    """mmx_s3_rope_fsmn: qkv fp32 [B, T, 3C] (q and k rotated in place), x / r fp32 [B, T, C], wt fp32 [31, C], lens int32 [B]."""
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.numel() >= B
    call("mmx_s3_rope_fsmn", _p(qkv), 3 * C_, T * 3 * C_, B, T, C_, _p(x), T * C_, _p(r), T * C_, _p(wt), _p(rope_cos), _p(rope_sin),
         rope_cos.shape[0], _p(lens), stream())


def fsq_encode(x, W, bias, ids, *, B, T, C_, lens=None, pre=None):
    """mmx_fsq_encode: x fp32 [B, T, C], W fp32 [8, C], bias fp32 [8] -> ids int32 [B, T] (and pre fp32 [B, T, 8])."""
    if lens is not None:
        assert lens.dtype == torch.int32 and lens.numel() >= B
    assert ids.dtype == torch.int32 and W.dtype == torch.float32 and tuple(W.shape) == (8, C_)
    call("mmx_fsq_encode", _p(x), C_, T * C_, B, T, C_, _p(W), _p(bias), _p(lens), _p(ids), T, _p(pre), stream())


# ----------------------------------------------------------------------------- engine
class SpeechTokenizerEngine:
    """S3TokenizerV2 on the device, built from a state dict with the reference's keys; C, the layer count and the mel count come
    from the shapes, the head dimension is 64 (n_head, when given, is only checked against C).

    dtype: MMX_F32 or the split build MMX_X2.  Asked for the bf16 build, the engine builds the split build: tokens are discrete,
    the model runs once per voice, and there is no speed to buy with wrong ids.  wplanes (split build): True / False / None =
    "auto": the weights go in as two bf16 planes when they are not bf16-representable (ops.resolve_wplanes) - the real tokenizer
    checkpoint is fp32."""

    def __init__(self, sd: Dict[str, torch.Tensor], dtype=X2, device="cuda", n_head=None, wplanes=None):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise MmxError("SpeechTokenizerEngine works on device memory only (no CPU fallback)")
        if dtype == BF16:
            dtype = X2
        if dtype not in (F32, X2):
            raise MmxError(f"SpeechTokenizerEngine: dtype {dtype} is not supported (MMX_F32 or MMX_X2)")
        self.dtype, self.dev, self.split = dtype, dev, is_split(dtype)
        self.C, self.n_mels = sd["encoder.conv1.weight"].shape[:2]
        C_ = self.C
        if C_ % 64 or (n_head is not None and n_head * 64 != C_):
            raise MmxError(f"SpeechTokenizerEngine: n_audio_state {C_} is not 64 * n_head (the rotary table fixes the head dimension)")
        self.H = C_ // 64
        self.layers = 0
        while f"encoder.blocks.{self.layers}.attn.query.weight" in sd:
            self.layers += 1
        mats = [k for k, v in sd.items() if v.dim() >= 2 and "fsmn_block" not in k and "project_down" not in k]
        self.wplanes = self.split and ops.resolve_wplanes("auto" if wplanes is None else wplanes, [sd[k] for k in mats])
        pd = X2W if self.wplanes else dtype
        f = lambda k: sd[k].detach().to(dev, torch.float32).contiguous()
        self.w1, self.b1 = ops.pack_conv1d(f("encoder.conv1.weight"), pd), f("encoder.conv1.bias")
        self.w2, self.b2 = ops.pack_conv1d(f("encoder.conv2.weight"), pd), f("encoder.conv2.bias")
        self.blocks = []
        for i in range(self.layers):
            p = f"encoder.blocks.{i}."
            wqkv = torch.cat([f(p + "attn.query.weight"), f(p + "attn.key.weight"), f(p + "attn.value.weight")])
            bqkv = torch.cat([f(p + "attn.query.bias"), torch.zeros(C_, device=dev), f(p + "attn.value.bias")])   # key has no bias
            self.blocks.append(dict(
                ln1g=f(p + "attn_ln.weight"), ln1b=f(p + "attn_ln.bias"), wqkv=ops.pack_linear(wqkv, pd), bqkv=bqkv,
                wo=ops.pack_linear(f(p + "attn.out.weight"), pd), bo=f(p + "attn.out.bias"),
                wt=f(p + "attn.fsmn_block.weight")[:, 0, :].t().contiguous(),                                   # [31, C] tap-major
                ln2g=f(p + "mlp_ln.weight"), ln2b=f(p + "mlp_ln.bias"),
                wm1=ops.pack_linear(f(p + "mlp.0.weight"), pd), bm1=f(p + "mlp.0.bias"),
                wm2=ops.pack_linear(f(p + "mlp.2.weight"), pd), bm2=f(p + "mlp.2.bias")))
        self.wpd, self.bpd = f("quantizer._codebook.project_down.weight"), f("quantizer._codebook.project_down.bias")
        cos, sin = rope_tables()
        self.rope_cos, self.rope_sin = cos.to(dev), sin.to(dev)
        self._bufs = {}
        self._mel = None

    # activation buffers per (B, T), reused
    def _buffers(self, B, T):
        b = self._bufs.get((B, T))
        if b is None:
            C_, T1 = self.C, conv_len(T)
            T2 = conv_len(T1)
            e = lambda *s: torch.empty(*s, dtype=torch.float32, device=self.dev)
            b = dict(mt=e(B, T, self.n_mels), h1=e(B, T1, C_), x=e(B, T2, C_), x2=e(B, T2, C_), r=e(B, T2, C_), hn=e(B, T2, C_),
                     qkv=e(B, T2, 3 * C_), att=e(B, T2, C_), ff=e(B, T2, 4 * C_), pre=e(B, T2, 8),
                     ids=torch.empty(B, T2, dtype=torch.int32, device=self.dev))
            if len(self._bufs) >= 8:
                self._bufs.clear()
            self._bufs[(B, T)] = b
        return b

    @torch.no_grad()
    def encode_time_major(self, mt, lens, want_pre=False):
        """mt fp32 [B, T, n_mels] on the device with the rows past a member's length zero; lens: list of ints ->
        (ids int32 [B, T2], code_len list[, pre fp32 [B, T2, 8]]).  The buffers returned are the engine's own: reused by the next
        call of the same shape."""
        dt, C_, H = self.dtype, self.C, self.H
        B, T, M = mt.shape
        assert M == self.n_mels and mt.is_contiguous() and mt.dtype == torch.float32 and len(lens) == B
        T1 = conv_len(T)
        T2 = conv_len(T1)
        if T2 > ROPE_ROWS:
            raise MmxError(f"SpeechTokenizerEngine: {T2} token rows exceed the rotary table's {ROPE_ROWS}")
        l1 = [conv_len(int(n)) for n in lens]
        l2 = [conv_len(n) for n in l1]
        ar = lambda n, Tn: (torch.arange(Tn, device=self.dev)[None, :] < torch.tensor(n, device=self.dev)[:, None]).float().contiguous()
        m1, m2 = ar(l1, T1), ar(l2, T2)
        klen = torch.tensor(l2, dtype=torch.int32, device=self.dev)
        b = self._buffers(B, T)
        ops.conv1d(mt, self.w1, T=T, Cin=M, k=3, pad_left=1, stride=2, T_out=T1, dtype=dt, batch=B, bias=self.b1, act="gelu",
                   rowmask=m1, out_act=b["h1"])
        x, x2 = b["x"], b["x2"]
        ops.conv1d(b["h1"], self.w2, T=T1, Cin=C_, k=3, pad_left=1, stride=2, T_out=T2, dtype=dt, batch=B, bias=self.b2, act="gelu",
                   rowmask=m2, out_f32=x)
        hn, qkv, att, r, ff = b["hn"], b["qkv"], b["att"], b["r"], b["ff"]
        for w in self.blocks:
            ops.rownorm(x, w["ln1g"], w["ln1b"], 1e-6, rows=T2, C_=C_, batch=B, out_act=hn, dtype=dt)
            ops.linear(hn, w["wqkv"], C_, dtype=dt, bias=w["bqkv"], out_f32=qkv)
            s3_rope_fsmn(qkv, x, r, w["wt"], self.rope_cos, self.rope_sin, B=B, T=T2, C_=C_, lens=klen)
            kw = dict(B=B, H=H, ldq=3 * C_, ldk=3 * C_, ldv=3 * C_, ldo=C_, q_bs=T2 * 3 * C_, k_bs=T2 * 3 * C_, v_bs=T2 * 3 * C_,
                      o_bs=T2 * C_, scale=0.125)         # (q D^-1/4) . (k D^-1/4), D = 64
            if self.split:
                ops.attn_flash_x(qkv, qkv[:, :, C_:], qkv[:, :, 2 * C_:], att, T=T2, klen=klen, **kw)
            else:
                ops.attn_dense(qkv, qkv[:, :, C_:], qkv[:, :, 2 * C_:], att, Tq=T2, Tk=T2, dtype=dt, keymask=m2, **kw)
            ops.linear(att, w["wo"], C_, dtype=dt, bias=w["bo"], residual=r, out_f32=x2)      # x + out(attn) + fsmn
            ops.rownorm(x2, w["ln2g"], w["ln2b"], 1e-5, rows=T2, C_=C_, batch=B, out_act=hn, dtype=dt)
            ops.linear(hn, w["wm1"], C_, dtype=dt, bias=w["bm1"], act="gelu", out_act=ff)
            ops.linear(ff, w["wm2"], 4 * C_, dtype=dt, bias=w["bm2"], residual=x2, out_f32=x)
        fsq_encode(x, self.wpd, self.bpd, b["ids"], B=B, T=T2, C_=C_, lens=klen, pre=b["pre"] if want_pre else None)
        return (b["ids"], l2, b["pre"]) if want_pre else (b["ids"], l2)

    @torch.no_grad()
    def quantize(self, mel, mel_len, want_pre=False):
        """S3TokenizerV2.quantize (model_v2.py:385-414): mel fp32 [B, n_mels, T] on the device, mel_len [B] ->
        (codes int32 [B, T'], code_len int32 [B]) with T' = the code length of T frames and 0 past a member's code_len; a member of more than 3000 frames takes the windowed path of
        _quantize_mixed_batch (all windows of all members as one batch, merged per member)."""
        if not mel.is_cuda:
            raise MmxError("SpeechTokenizerEngine works on device memory only (no CPU fallback)")
        B, M, T = mel.shape
        lens = [int(v) for v in (mel_len.tolist() if hasattr(mel_len, "tolist") else mel_len)]
        assert len(lens) == B and M == self.n_mels and max(lens) <= T
        mel = mel.to(torch.float32)
        if max(lens) <= MAX_FRAMES:
            mt = self._buffers(B, T)["mt"]
            ops.copy2d(mel.contiguous(), F32, M * T, 1, T, mt, F32, T * M, M, 1, rows=T, cols=M, batch=B)
            self._mask_input(mt, lens)
            out = self.encode_time_major(mt, lens, want_pre)
            cl = torch.tensor(out[1], dtype=torch.int32, device=self.dev)
            return (out[0].clone(), cl, out[2].clone()) if want_pre else (out[0].clone(), cl)
        # windowed path: every member contributes its windows (a short member: one), each zero padded to 3000 frames
        if want_pre:
            raise MmxError("SpeechTokenizerEngine.quantize: want_pre is for members of at most 3000 frames (the windowed path merges ids only)")
        plans = [segment_plan(n) for n in lens]
        owner = [(bi, s, n) for bi, pl in enumerate(plans) for (s, n) in pl]
        S = len(owner)
        mt = self._buffers(S, WINDOW)["mt"]
        mt.zero_()
        for si, (bi, s, n) in enumerate(owner):
            mt[si, :n] = mel[bi, :, s:s + n].t()
        seg_lens = [n for (_, _, n) in owner]
        ids, l2 = self.encode_time_major(mt, seg_lens)[:2]
        ids = ids.cpu()
        per = [[] for _ in range(B)]
        for si, (bi, _, _) in enumerate(owner):
            per[bi].append(ids[si, :l2[si]].tolist())
        merged = [merge_segments(p) if len(p) > 1 else p[0] for p in per]
        cl = [len(m) for m in merged]
        codes = torch.zeros(B, max(cl), dtype=torch.int32)
        for bi, m in enumerate(merged):
            codes[bi, :cl[bi]] = torch.tensor(m, dtype=torch.int32)
        return codes.to(self.dev), torch.tensor(cl, dtype=torch.int32, device=self.dev)

    def _mask_input(self, mt, lens):
        """model_v2.py:328-329 `x * mask`: the frames past a member's length are zero."""
        B, T, M = mt.shape
        if min(lens) < T:
            m = (torch.arange(T, device=self.dev)[None, :] < torch.tensor(lens, device=self.dev)[:, None]).float().contiguous()
            ops.mask_rows(mt, m, rows=B * T, C_=M, dtype=F32)

    @torch.no_grad()
    def tokenize(self, waves16k: List[torch.Tensor]) -> List[torch.Tensor]:
        """16 kHz clips (each [n] or [1, n] on the device) -> one int32 token tensor per clip: one zero-padded batch through
        mmx_logmel_w (the whole-clip mel, with its clip maximum, comes before any windowing), then quantize."""
        waves = list(waves16k)
        on_device("SpeechTokenizerEngine", waves)
        batch, lens = pack([w.to(self.dev) for w in waves], None, "SpeechTokenizerEngine.tokenize")
        if self._mel is None:
            self._mel = LogMelW(self.n_mels, self.dev)
        frames = [frames_of(n) for n in lens]
        if max(frames) <= MAX_FRAMES:
            mt = self._mel(batch, lens=lens, time_major=True, dtype=F32, out=self._buffers(len(waves), max(frames))["mt"])
            ids, l2 = self.encode_time_major(mt, frames)
            return [ids[i, :l2[i]].clone() for i in range(len(waves))]
        mel = self._mel(batch, lens=lens)
        codes, cl = self.quantize(mel, frames)
        return [codes[i, :int(cl[i])].clone() for i in range(len(waves))]
