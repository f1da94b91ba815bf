"""Autoregressive speech-token LM engine (Qwen2-0.5B-shaped backbone + CosyVoice2 heads) on libmmx_hip kernels.

Reference (speech/): cosyvoice/llm/llm.py:676-711 (Qwen2LM.inference), :745-760 (inference_wrapper AR loop),
:359-371 (forward_one_step -> HF Qwen2ForCausalLM hidden_states[-1]), :259-274 (sampling_ids),
cosyvoice/utils/common.py:111-139 (ras/nucleus/random sampling).

One decode step for a batch of B sequences is 6 launches per layer (RMSNorm-folded QKV projection, RoPE + paged KV
append, paged GQA attention, o_proj + residual, RMSNorm-folded gate/up + SwiGLU, down + residual) + logits + the
device-resident sampler; it is recorded once into a hipGraph and replayed per token, with all loop state
(positions, step counters, token history, next input embedding, finished flags) on the device — the host only
polls `finished` every few steps (the reference syncs on .item() every token, llm.py:752).
The sampler's parameters (mode, top_p, top_k, win_size, tau_r, seed) are device state too: one column per sequence of the
table `samp` (include/mmx_hip.h, mmx_sample_step_tab), so every request has its own and the recorded step holds none of them.
Attention is full causal over the KV cache (SURVEY.md §7 "version-drift trap").
LmModel holds what engines of different batch sizes share (packed weights, RoPE tables, paged KV cache, page allocator);
an LlmEngine is one batch size over it and decides at construction which kernel family runs its decode step and its prompt
rows (decode_on / prompt_on, LlmEngine._dispatch), refusing the combinations no kernel serves.
"""
import math
from typing import Dict, List, Optional

import torch

from . import ops
from ._lib import BF16, F32, H2, TORCH_DT, WEIGHT_DT, X3, X3W, is_split
from .flow import Graphed

ST_POS, ST_STEP, ST_NOUT, ST_FIN, ST_MINLEN, ST_MAXLEN, ST_SEQ, ST_ERR = range(8)


class PageAllocator:
    """Free list of physical KV pages (the vLLM seam of the reference, cli/model.py:274-283 / llm.py:715-743, keeps its KV
    cache in such pages).  A sequence holds pages for the rows it has written plus a look-ahead; pages return to the list
    when it finishes, and a queued request is admitted into the freed slot (LlmEngine.admit)."""

    def __init__(self, n_pages: int):
        self.free_pages = list(range(n_pages - 1, -1, -1))
        self.n_pages = n_pages

    @property
    def n_free(self) -> int:
        return len(self.free_pages)

    def alloc(self, n: int) -> List[int]:
        if n > len(self.free_pages):
            raise RuntimeError(f"KV cache exhausted: {n} pages wanted, {len(self.free_pages)} free of {self.n_pages}")
        out = self.free_pages[-n:][::-1]
        del self.free_pages[-n:]
        return out

    def free(self, pages: List[int]):
        self.free_pages.extend(reversed(pages))


class LmModel:
    """What every engine over one checkpoint shares, built once from the state dict: shapes and flags, the packed weights, the
    RoPE tables, the paged KV cache and its page allocator.  An LlmEngine adds what belongs to one batch size."""

    def __init__(self, sd: Dict[str, torch.Tensor], dtype, device, max_batch, max_ctx, page, heads, kv_heads, head_dim, rope_theta,
                 eps, speech_token_size, prefix, kv_pages, wplanes, h2, gemm_packs):
        """wplanes / h2: the decode packs are weight planes / fp16 (w * 2^8); gemm_packs: row-major copies for the windowed GEMM
        are packed too.  max_batch sizes the KV cache when kv_pages is None."""
        self.dtype, self.tdt, self.dev = dtype, TORCH_DT[dtype], torch.device(device)
        self.wplanes, self.h2 = wplanes, h2
        self.ddt = H2 if h2 else dtype                    # dtype code of the decode-step kernels (csrc/decode.hip)
        self.split = is_split(dtype)                      # bf16 weights, fp32 activations split inside the MFMA products
        self.Hq, self.Hkv, self.D, self.eps, self.page = heads, kv_heads, head_dim, eps, page
        self.eos, self.V = speech_token_size, speech_token_size + 3
        f = lambda k: sd[k].detach().to(self.dev, torch.float32).contiguous()
        c = (lambda t: t.float().contiguous()) if wplanes else (lambda t: t.to(WEIGHT_DT[dtype]).contiguous())
        dt = X3W if wplanes else dtype                    # the code the weights are packed for (X3W: ops.Planed packs)
        # The RMSNorm gain is folded into the packed weights only in the fp32 build.  The bf16 and split builds keep the
        # checkpoint's bf16 weights as they are and apply the gain to the activations: in the producer's epilogue on the
        # decode step (csrc/decode.hip), in the kernel for prompt chunks (kgamma).
        self.unfolded = dtype != F32
        ks = (lambda g: None) if self.unfolded else (lambda g: g)
        if h2:                                            # fp16 packs: one plane (bf16-representable checkpoint) or hi + lo
            pk = lambda w, g=None, ih=0: ops.pack_skinny_h2(w, planes=(2 if wplanes else 1), interleave_half=ih)
        else:
            pk = lambda w, g=None, ih=0: ops.pack_skinny(c(w), dtype=dt, kscale=ks(g), interleave_half=ih)
        self.n_layers = len({k.split(".")[4] for k in sd if k.startswith(prefix + ".layers.")})
        self.H = sd[prefix + ".norm.weight"].shape[0]
        self.I = sd[prefix + ".layers.0.mlp.gate_proj.weight"].shape[0]
        self.layers, self.pf_layers = [], []
        for l in range(self.n_layers):
            p = f"{prefix}.layers.{l}"
            a = p + ".self_attn"
            wqkv = torch.cat([f(a + ".q_proj.weight"), f(a + ".k_proj.weight"), f(a + ".v_proj.weight")], 0)
            bqkv = torch.cat([f(a + ".q_proj.bias"), f(a + ".k_proj.bias"), f(a + ".v_proj.bias")], 0).contiguous()
            wgu = torch.cat([f(p + ".mlp.gate_proj.weight"), f(p + ".mlp.up_proj.weight")], 0)
            g1, g2 = f(p + ".input_layernorm.weight"), f(p + ".post_attention_layernorm.weight")
            if gemm_packs:
                # row-major copies for the windowed GEMM (_gemm_layers): many prompt rows at once are an ordinary tall GEMM
                # over weights read once, not passes of the weight-streaming decode kernels
                self.pf_layers.append(dict(
                    wqkv=ops.pack_linear(c(wqkv), dt), wo=ops.pack_linear(c(f(a + ".o_proj.weight")), dt),
                    wgu=ops.pack_linear(c(wgu), dt), wdown=ops.pack_linear(c(f(p + ".mlp.down_proj.weight")), dt), g1=g1, g2=g2))
            self.layers.append(dict(wqkv=pk(wqkv, g1), bqkv=bqkv, wo=pk(f(a + ".o_proj.weight")), wgu=pk(wgu, g2, self.I),
                                    wdown=pk(f(p + ".mlp.down_proj.weight")), g1=g1, g2=g2))
            del wqkv, wgu
        self.norm_w = f(prefix + ".norm.weight")
        self.embed_tokens = f(prefix + ".embed_tokens.weight")
        if "llm_decoder.weight" in sd:
            self.wdec = pk(f("llm_decoder.weight"), self.norm_w)
            self.bdec = f("llm_decoder.bias")
            self.speech_emb = f("speech_embedding.weight")
            self.llm_emb = f("llm_embedding.weight")
        else:                                              # backbone only (Qwen2Encoder.forward_one_step)
            self.wdec = self.bdec = self.speech_emb = self.llm_emb = None
        # HF Qwen2RotaryEmbedding inv_freq (modeling_qwen2.py: 1 / theta^(arange(0,d,2)/d)), computed like HF in fp32
        self.inv_freq = (1.0 / (rope_theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))).to(self.dev)
        # cos/sin per position exactly as HF computes them (fp32 outer product, then cos/sin): [max_ctx][cos 32 | sin 32]
        # one capacity for the KV pages, the RoPE table, the token history and every guard: whole pages
        self.max_pages = (max_ctx + page - 1) // page
        self.max_out = self.max_pages * page
        ang = torch.arange(self.max_out, dtype=torch.float32)[:, None] * self.inv_freq.cpu()[None, :]
        self.rope_tab = torch.cat([ang.cos(), ang.sin()], dim=1).contiguous().to(self.dev)
        # paged KV cache: [layers][pages][Hkv][page][D]; pages are handed out by a free-list allocator, a slot's block
        # table row lists the pages of the sequence it currently runs (idle slots point at the scratch page)
        npages = max_batch * self.max_pages if kv_pages is None else int(kv_pages)
        self.trash_page = npages                  # scratch page: idle slots append their (ignored) KV here
        self.kc = torch.zeros(self.n_layers, npages + 1, kv_heads, page, head_dim, dtype=self.tdt, device=self.dev)
        self.vc = torch.zeros_like(self.kc)
        self.pages = PageAllocator(npages)


class LlmEngine:
    # decode attention: batches of at least this many sequences use the GQA-shared kernel (one workgroup per kv head serving
    # its 7 query heads), smaller ones the per-head kernel (more workgroups for the few sequences there are)
    gqa_min_batch = 1 << 30
    use_v2 = True            # bf16 / split builds: decode step on csrc/decode.hip (False: the round-2 projection kernel)
    # split build, decode step: "f16x2" = activations as two fp16 planes (22 bits) and fp16 weights (csrc/decode.hip MMX_H2 / H2W:
    # two thirds of the activation bytes and of the MFMAs of the three-bf16-plane form, 4 instead of 6 bytes per weight on an
    # fp32 checkpoint); "bf16x3" = three bf16 planes (MMX_X3 / X3W)
    lm_planes = "f16x2"
    # weight prefetch: a side stream of the (captured) decode step touches layer l + 1's packed weights while layer l computes
    # (csrc/elementwise.hip prefetch_kernel), so that the next projections read them from the Infinity Cache; 0 = off, else the
    # number of workgroups of the prefetch launch
    prefetch = 0
    # decode attention returns at once for a slot whose sequence has ended (mmx_decode_attn_fin); False: it recomputes the
    # slot's last step every step, as before (A/B measurements; the live slots' results are the same bit for bit)
    skip_finished = True

    def __init__(self, sd: Dict[str, torch.Tensor], dtype=BF16, device="cuda", max_batch=1, max_ctx=2048, page=16,
                 heads=14, kv_heads=2, head_dim=64, rope_theta=1e6, eps=1e-6, speech_token_size=6561, use_graphs=True,
                 prefix="llm.model.model", share_from=None, kv_pages=None, wplanes=False, lm_planes=None, decode_on=None,
                 prompt_on=None):
        """wplanes (split build X3 only): every projection weight is carried as THREE bf16 planes hi + mid + lo = the checkpoint's
        fp32 value (MMX_X3W: csrc/decode.hip for the decode step, csrc/gemm.hip for the prompt pass) instead of being rounded to
        bf16 - for checkpoints whose weights are not bf16-representable (the reference loads an fp32 llm.pt, cli/model.py:67-75).
        Costs 3 x the weight bytes and 2 x the MFMAs of the plain split build.
        share_from: a second engine of a different batch size over the SAME LmModel - packed weights and paged KV cache - as
        that engine (used to continue a partly finished batch at a smaller, cheaper batch size: see compact_from).
        decode_on / prompt_on: the kernel family of the decode step and of prompt rows (_dispatch; None = what the build and the
        batch size make best).  A combination whose packs no kernel can read raises ValueError."""
        if share_from is not None:
            m, v2 = share_from.model, share_from.v2 if decode_on is None else decode_on == "planes"
            dtype, h2, wplanes, gemm_packs = m.dtype, m.h2, m.wplanes, bool(m.pf_layers)
        else:
            wplanes = dtype == X3 and ops.resolve_wplanes(wplanes, (v for k, v in sd.items() if v.dim() >= 2 and ("proj" in k or k == "llm_decoder.weight")))
            planes = lm_planes or self.lm_planes
            if planes not in ("f16x2", "bf16x3"):
                raise ValueError(f"lm_planes {planes!r}: 'f16x2' or 'bf16x3'")
            v2, gemm_packs = self.use_v2 if decode_on is None else decode_on == "planes", True
            h2 = dtype == X3 and planes == "f16x2" and v2  # (the round-2 kernel takes the bf16 packs)
        self.decode_on, self.prompt_on = self._dispatch(dtype, h2, wplanes, v2, max_batch, decode_on, prompt_on, gemm_packs)
        if share_from is None:
            m = LmModel(sd, dtype, device, max_batch, max_ctx, page, heads, kv_heads, head_dim, rope_theta, eps, speech_token_size,
                        prefix, kv_pages, wplanes, h2, gemm_packs=self.prompt_on != "skinny")
        self.model, self.B, self.use_graphs, self.v2 = m, max_batch, use_graphs, v2      # (v2: decode step asked for on csrc/decode.hip)
        # the model's fields that tests, tools, bench.py and the drop-in read from an engine, under the names they always had
        self.dtype, self.tdt, self.ddt, self.dev, self.h2, self.wplanes = m.dtype, m.tdt, m.ddt, m.dev, m.h2, m.wplanes
        self.n_layers, self.H, self.I, self.Hq, self.Hkv, self.D, self.eps = m.n_layers, m.H, m.I, m.Hq, m.Hkv, m.D, m.eps
        self.page, self.max_pages, self.max_out, self.eos, self.V = m.page, m.max_pages, m.max_out, m.eos, m.V
        self.layers, self.llm_emb, self.speech_emb, self.embed_tokens = m.layers, m.llm_emb, m.speech_emb, m.embed_tokens
        self.kc, self.vc, self.pages = m.kc, m.vc, m.pages
        if m.wplanes and not m.h2:                        # three bf16 weight planes in registers: one output tile per workgroup
            self.v2_cfg = dict(qkv=(1, 1), o=(1, 1), gu=(1, 1), down=(1, 8), head=(1, 1))
        B = self.B
        self.block_table = torch.full((B, m.max_pages), m.trash_page, dtype=torch.int32, device=self.dev)
        self.slot_pages = [[] for _ in range(B)]
        self.state = torch.zeros(8, B, dtype=torch.int32, device=self.dev)
        self.out_tokens = torch.zeros(B, self.max_out, dtype=torch.int32, device=self.dev)
        self.sampled = torch.full((B, self.max_out), -1, dtype=torch.int32, device=self.dev)
        self.forced, self._forced_buf = None, None
        self.x_in = torch.zeros(B, self.H, device=self.dev)         # next input embedding (written by the sampler)
        self.h = torch.zeros(B, self.H, device=self.dev)            # residual stream of the step
        # its compute-dtype copy; at batch > 8 the decode step keeps it (and every other GEMM input) in the packed
        # MFMA-fragment order of include/mmx_hip.h (whole 16-row tiles)
        self.packed = B >= 4 and not m.unfolded
        self.h_act = torch.zeros(ops.packed_rows(B), self.H, dtype=self.tdt, device=self.dev)
        self.logits = torch.zeros(B, self.V, device=self.dev)
        self.logp = torch.zeros(B, self.V, device=self.dev)
        # the engine's default sampler (config.yaml:46-50): what a sequence gets that is started without one of its own
        self.seed, self.want_logp = 0, False
        self.mode, self.top_p, self.top_k, self.win_size, self.tau_r = 0, 0.8, 25, 10, 0.1
        # the sampler table the kernel reads (field-major, one column per slot) and its host mirror
        self._samp_host = [self._sampler_fields(None, None) for _ in range(B)]
        self.samp = torch.tensor([ops.sampler_column(**f) for f in self._samp_host], dtype=torch.int32).t().contiguous().to(self.dev)
        self._decode, self._graph_key = None, None
        self.reserve_ahead = 1 << 30               # start(): rows reserved past the prompt (default: the whole max_len)

    @staticmethod
    def _dispatch(dtype, h2, wplanes, v2, B, decode_on, prompt_on, gemm_packs):
        """-> (decode_on, prompt_on): the kernel family that serves B sequences over packs of (dtype, h2, wplanes).
        decode_on, the decode step: "planes" = csrc/decode.hip on split-plane activations (bf16 and split builds, <= 32
        sequences, v2: asked for), else "skinny" = mmx_skinny_gemm, the round-2 projection kernel.
        prompt_on, prompt rows: "gemm" = the windowed GEMM; "skinny" = mmx_skinny_gemm chunks of <= 64 rows over the decode
        packs; "gemm-batch" (>= 4 slots) = the prompts of a start() as one tall GEMM pass, weights read once for all of them,
        and rows entering a single slot (admit, feed, forward_rows) as skinny chunks.
        fp16 and weight-plane packs (h2 / wplanes) are read by csrc/decode.hip and, row-major, by the windowed GEMM only:
        whatever else is asked of them raises ValueError, as does a family named by keyword that cannot serve.
        gemm_packs: the model has, or will get, the row-major copies."""
        planes_only = h2 or wplanes
        packs = ("fp16" if h2 else "bf16") + (" weight-plane" if wplanes else "") + " decode packs"
        decode = "planes" if v2 and dtype != F32 and B <= 32 else "skinny"
        if decode_on not in (None, decode):
            raise ValueError(f"decode_on={decode_on!r}: 'planes' (csrc/decode.hip) serves the bf16 and split builds up to 32 sequences, "
                             f"'skinny' (mmx_skinny_gemm) the rest; this is dtype {dtype} at max_batch {B}")
        if planes_only and decode != "planes":
            raise ValueError(f"{packs} are read by csrc/decode.hip only, which does not serve " +
                             (f"max_batch {B} > 32" if v2 else "the round-2 kernel (use_v2 = False / decode_on='skinny')"))
        ok = ("gemm",) if planes_only else ("gemm", "gemm-batch", "skinny") if gemm_packs else ("skinny",)
        if prompt_on not in (None,) + ok:
            raise ValueError(f"prompt_on={prompt_on!r}: {packs}" + ("" if gemm_packs else ", shared model without row-major copies,") + f" take {ok}")
        return decode, prompt_on or ("gemm" if planes_only else "gemm-batch" if B >= 4 and gemm_packs else "skinny")

    @staticmethod
    def _attn_kw(split, h2, B, gqa_min_batch):
        """The decode attention form of the step on csrc/decode.hip (ops.decode_attn's switches; the static_asserts under
        decode_attn_select in csrc/llm.hip pin the kernels they resolve to): its output is the o projection's operand - one
        packed bf16 plane (bf16 build), three bf16 planes (split build) or two fp16 planes (h2)."""
        return dict(per_head=bool(split or B < gqa_min_batch), out_split=("f16" if h2 else bool(split)), out_packed=not split)

    # ------------------------------------------------------------------ one transformer pass over `rows` tokens/seq
    def _layers(self, h, ha, B, rows, pos, block_table, packed=False):
        """The layers on mmx_skinny_gemm (prompt chunks; the decode step where decode_on is "skinny").
        h fp32 [B*rows, H] residual stream (in place) and ha, its compute-dtype copy (kept in sync by the residual epilogues: it
        is the A operand of the next RMSNorm-folded projection; unused in the split build, whose GEMM inputs are the fp32
        tensors themselves).  bf16 and split builds: the RMSNorm gains ride as kgamma on the fp32 residual stream.
        pos int32 [B] device, block_table [B, max_pages].
        packed (decode step, batch > 8): ha / att / act live in the packed fragment order; the first projection
        reads the fp32 residual stream itself (row-major), so no packing pass is needed for the input embedding."""
        m = self.model
        dt, H, I = m.dtype, m.H, m.I
        n = B * rows
        assert n <= 64 and not (packed and rows != 1)
        nr = ops.packed_rows(n) if packed else n
        qkv = torch.empty(n, (m.Hq + 2 * m.Hkv) * m.D, device=self.dev)
        q = torch.empty(n, m.Hq * m.D, dtype=m.tdt, device=self.dev)
        att = torch.empty(nr, m.Hq * m.D, dtype=m.tdt, device=self.dev)
        act = torch.empty(nr, I, dtype=m.tdt, device=self.dev)
        kg = (lambda g: g) if m.unfolded else (lambda g: None)
        res = dict(out_f32=h) if m.split else dict(out_f32=h, out_act=ha)      # the residual epilogues' outputs
        gu = dict(out_f32=act) if m.split else dict(out_act=act)               # SwiGLU product in the activation dtype
        for l, w in enumerate(m.layers):
            first = (packed and l == 0) or m.unfolded
            ops.skinny_gemm(h if first else ha, w["wqkv"], B=n, K=H, N=qkv.shape[1], dtype=dt, bias=w["bqkv"], rs=True,
                            eps=m.eps, epi=0, out_f32=qkv, x_packed=packed and not first, kgamma=kg(w["g1"]))
            if rows == 1:
                ops.decode_attn(qkv, m.inv_freq, pos, m.kc[l], m.vc[l], block_table, att, B=B, Hq=m.Hq,
                                Hkv=m.Hkv, page=m.page, dtype=dt, rope_tab=m.rope_tab, out_packed=packed,
                                per_head=m.split or B < self.gqa_min_batch)
            else:
                ops.rope_kv_store(qkv, m.inv_freq, pos, q, m.kc[l], m.vc[l], block_table, B=B, rows=rows,
                                  Hq=m.Hq, Hkv=m.Hkv, page=m.page, dtype=dt)
                ops.paged_attn(q, pos, m.kc[l], m.vc[l], block_table, att, B=B, rows=rows, Hq=m.Hq,
                               Hkv=m.Hkv, page=m.page, dtype=dt)
            ops.skinny_gemm(att, w["wo"], B=n, K=m.Hq * m.D, N=H, dtype=dt, epi=2, x_packed=packed, out_packed=packed, **res)
            ops.skinny_gemm(h if m.unfolded else ha, w["wgu"], B=n, K=H, N=I, dtype=dt, rs=True, eps=m.eps, epi=1,
                            x_packed=packed, out_packed=packed, kgamma=kg(w["g2"]), **gu)
            ops.skinny_gemm(act, w["wdown"], B=n, K=I, N=H, dtype=dt, epi=2, x_packed=packed, out_packed=packed, **res)

    # decode-step projections of the split build (csrc/decode.hip): (output tiles per workgroup, k slices across workgroups)
    v2_cfg = dict(qkv=(1, 1), o=(1, 1), gu=(2, 1), down=(2, 8), head=(2, 1))

    def _planes(self):
        """Static buffers of the split-plane decode step (csrc/decode.hip): activation planes, sum-of-squares tables (zeroed:
        unused tile slots must read 0), partial tiles and tickets of the down projection's cross-workgroup k split."""
        if not hasattr(self, "_v2"):
            m = self.model
            H, I, R = m.H, m.I, ops.packed_rows(self.B)
            NQ = (m.Hq + 2 * m.Hkv) * m.D
            bf = lambda K: torch.zeros((2 if m.h2 else 3) if m.split else 1, R * K, dtype=torch.bfloat16, device=self.dev)
            J = self.v2_cfg["down"][1]
            self._v2 = dict(qkv=torch.empty(self.B, NQ, device=self.dev), xs_a=bf(H), xs_b=bf(H), xs_att=bf(m.Hq * m.D), xs_act=bf(I),
                            ssq_a=torch.zeros(32, ops.SSQ_SLOTS, device=self.dev), ssq_b=torch.zeros(32, ops.SSQ_SLOTS, device=self.dev),
                            part=torch.empty(J * ((H + 15) // 16) * (R // 4) * 64, device=self.dev),
                            tickets=torch.zeros((H + 15) // 16, dtype=torch.int32, device=self.dev))
        return self._v2

    def _prefetch(self, l=None):
        """The decode step's weight prefetch (LlmEngine.prefetch workgroups; 0 = off, the default: a measured negative, kept for
        bench.py --lm-prefetch).  l: fork - a side stream touches the packs of layer l + 1 (the head's after the last layer)
        while layer l computes; None: join - the side stream's last launch belongs to this step."""
        if not int(self.prefetch):
            return
        if not hasattr(self, "_pf_side"):
            self._pf_side = torch.cuda.Stream(device=self.dev)
            self._pf_sink = torch.zeros(4, dtype=torch.int32, device=self.dev)
        layers, ev = self.model.layers, torch.cuda.Event()
        src, dst = (torch.cuda.current_stream(), self._pf_side) if l is not None else (self._pf_side, torch.cuda.current_stream())
        ev.record(src)
        dst.wait_event(ev)
        if l is not None:
            with torch.cuda.stream(self._pf_side):
                ops.prefetch4([layers[l + 1][k] for k in ("wqkv", "wo", "wgu", "wdown")] if l + 1 < len(layers) else [self.model.wdec],
                              self._pf_sink, int(self.prefetch))

    def _layers_split_decode(self, x_in, h, B, pos, block_table):
        """One decode step of the bf16 and split builds on split-plane activations (csrc/decode.hip, B <= 32 sequences): one
        prep launch, then 5 launches per layer.  x_in -> h (residual stream, fp32) and the planes of h * gamma; every
        projection's epilogue writes the planes (and the RMSNorm partial sums) its consumer reads.  Leaves the planes of
        h * norm_w and the sums of squares of h in xs_a / ssq_a for the head."""
        m = self.model
        dt, H, I, c, S = m.ddt, m.H, m.I, self.v2_cfg, self._planes()
        NQ = (m.Hq + 2 * m.Hkv) * m.D
        qkv = S["qkv"][:B]
        # the attention of an ended slot is skipped: the sampler leaves such a slot's state and input alone and nothing reads its
        # rows (rows are independent in every projection), until admit / compact_from / _upload_state rewrite the whole column
        fin = self.state[ST_FIN] if self.skip_finished else None      # (pos is state[ST_POS]: _decode_step)
        ops.decode_prep(x_in, S["xs_a"], S["ssq_a"], B=B, K=H, gamma=m.layers[0]["g1"], h=h, dtype=dt)
        for l, w in enumerate(m.layers):
            self._prefetch(l)
            g_next = m.layers[l + 1]["g1"] if l + 1 < len(m.layers) else m.norm_w
            ops.skinny2(S["xs_a"], w["wqkv"], B=B, K=H, N=NQ, dtype=dt, bias=w["bqkv"], ssq_in=S["ssq_a"], eps=m.eps, epi=0, out=qkv,
                        tiles_per_wg=c["qkv"][0])
            # (bf16 build: one plane = the packed A-fragment order the attention kernels already write)
            ops.decode_attn(qkv, m.inv_freq, pos, m.kc[l], m.vc[l], block_table, S["xs_att"], B=B, Hq=m.Hq,
                            Hkv=m.Hkv, page=m.page, dtype=m.dtype, rope_tab=m.rope_tab, finished=fin,
                            **self._attn_kw(m.split, m.h2, B, self.gqa_min_batch))
            ops.skinny2(S["xs_att"], w["wo"], B=B, K=m.Hq * m.D, N=H, dtype=dt, epi=2, out=h, xs_out=S["xs_b"],
                        gamma_next=w["g2"], ssq_out=S["ssq_b"], tiles_per_wg=c["o"][0])
            ops.skinny2(S["xs_b"], w["wgu"], B=B, K=H, N=I, dtype=dt, ssq_in=S["ssq_b"], eps=m.eps, epi=1, xs_out=S["xs_act"],
                        tiles_per_wg=c["gu"][0])
            ops.skinny2(S["xs_act"], w["wdown"], B=B, K=I, N=H, dtype=dt, epi=2, out=h, xs_out=S["xs_a"], gamma_next=g_next,
                        ssq_out=S["ssq_a"], tiles_per_wg=c["down"][0], ksplit=c["down"][1], part=S["part"], tickets=S["tickets"])
        self._prefetch(None)

    def _tail(self, B, packed=False, planes_ready=False):
        """final RMSNorm (folded) + llm_decoder + log_softmax + sampler + loop bookkeeping for all B sequences.
        planes_ready (decode step on csrc/decode.hip): xs_a / ssq_a already hold the planes of h * norm_w (the step's last
        projection wrote them); otherwise they are made from self.h first."""
        m = self.model
        if self.decode_on == "planes":
            S = self._planes()
            if not planes_ready:
                ops.decode_prep(self.h, S["xs_a"], S["ssq_a"], B=B, K=m.H, gamma=m.norm_w, dtype=m.ddt)
            ops.skinny2(S["xs_a"], m.wdec, B=B, K=m.H, N=m.V, dtype=m.ddt, bias=m.bdec, ssq_in=S["ssq_a"],
                        eps=m.eps, epi=0, out=self.logits, tiles_per_wg=self.v2_cfg["head"][0])
        else:                                             # gain on the fp32 stream (kgamma), or folded into wdec (fp32 build)
            x, kw = (self.h, dict(kgamma=m.norm_w)) if m.unfolded else (self.h_act, dict(x_packed=packed))
            ops.skinny_gemm(x, m.wdec, B=B, K=m.H, N=m.V, dtype=m.dtype, bias=m.bdec, rs=True, eps=m.eps, epi=0, out_f32=self.logits, **kw)
        ops.sample_step_tab(self.logits, self.state, self.out_tokens, m.speech_emb, self.x_in, self.samp, V=m.V, B=B,
                            eos_id=m.eos, sampled=self.sampled, forced=self.forced,
                            logp_out=(self.logp if self.want_logp else None))

    # ------------------------------------------------------------------ per-sequence samplers
    SAMPLER_FIELDS = ("mode", "top_p", "top_k", "win_size", "tau_r", "seed")

    def _sampler_fields(self, sampler, seed, base=None):
        """`base` (default: the engine's default sampler) overridden by `sampler` (a dict over SAMPLER_FIELDS, or None) and `seed`
        (or None): an entry of the host mirror.  The one place where the mode becomes what the table holds."""
        f = dict(base) if base is not None else {k: getattr(self, k) for k in self.SAMPLER_FIELDS}
        if sampler:
            unknown = set(sampler) - set(self.SAMPLER_FIELDS)
            if unknown:
                raise ValueError(f"unknown sampler fields {sorted(unknown)}")
            f.update({k: v for k, v in sampler.items() if v is not None})
        if seed is not None:
            f["seed"] = int(seed)
        f["mode"] = ops.SAMPLER_MODES.get(f["mode"], f["mode"])      # the mirror holds the mode as the table does: 0 / 1 / 2
        return f

    def _write_samplers(self, fields):
        """fields: one dict per slot, len(fields) == B -> host mirror and device table, one copy."""
        assert len(fields) == self.B
        cols = [ops.sampler_column(**f) for f in fields]           # raises ValueError on a bad column: nothing written
        self._samp_host = [dict(f) for f in fields]
        self.samp.copy_(torch.tensor(cols, dtype=torch.int32).t().contiguous())

    def set_sampler(self, slot: int, *, mode=None, top_p=None, top_k=None, win_size=None, tau_r=None, seed=None):
        """Changes the sampler of one slot: the fields given (mode 0 / "ras", 1 / "nucleus", 2 / "random"; top_k 1..64; win_size
        0..64), the others stay as the slot has them.  Takes effect at the slot's next sampling step, recorded decode graph included:
        the kernel reads the column from device memory (csrc/sampler.hip)."""
        f = self._sampler_fields(dict(mode=mode, top_p=top_p, top_k=top_k, win_size=win_size, tau_r=tau_r, seed=seed), None,
                                 base=self._samp_host[slot])
        self._write_sampler(slot, f, ops.sampler_column(**f))

    def _write_sampler(self, slot, f, col):
        self._samp_host[slot] = f
        self.samp[:, slot].copy_(torch.tensor(col, dtype=torch.int32))

    def _decode_step(self):
        B = self.B
        if self.decode_on == "planes":
            self._layers_split_decode(self.x_in, self.h, B, self.state[ST_POS], self.block_table)
            return self._tail(B, planes_ready=True)
        self.h.copy_(self.x_in)
        if not self.packed:
            self.h_act[:B].copy_(self.x_in)
        self._layers(self.h, self.h_act, B, 1, self.state[ST_POS], self.block_table, packed=self.packed)
        self._tail(B, packed=self.packed)

    # ------------------------------------------------------------------ request setup
    def build_lm_input(self, text, prompt_text, prompt_speech_token, speaker_embed=None):
        """llm.py:691-703: [sos | embed(prompt_text ++ text) | task_id | speech_emb(prompt_speech)] fp32 [L, H];
        with speaker_embed ([1, H], inference_spk, llm.py:663): [sos | speaker_embed | text | task_id | prompt speech]."""
        tok = torch.cat([prompt_text.reshape(-1), text.reshape(-1)]).to(self.dev, torch.int64)
        s = 0 if speaker_embed is None else 1
        L = 2 + s + tok.numel() + prompt_speech_token.numel()
        x = torch.empty(L, self.H, device=self.dev)
        x[0].copy_(self.llm_emb[0])
        if s:
            x[1].copy_(speaker_embed.reshape(-1))
        ops.gather_rows(tok, self.embed_tokens, out_f32=x[1 + s:1 + s + tok.numel()], dtype=F32)
        x[1 + s + tok.numel()].copy_(self.llm_emb[1])
        if prompt_speech_token.numel():
            ops.gather_rows(prompt_speech_token.reshape(-1).to(self.dev, torch.int64), self.speech_emb,
                            out_f32=x[2 + s + tok.numel():], dtype=F32)
        return x

    def speaker_conditioning(self, sd_linear_w, sd_linear_b, emb192):
        """normalize -> spk_embed_affine_layer (llm.py:184-186 / :650-653): [1,192] -> [1,H] fp32."""
        d = emb192.shape[1]
        g = torch.full((d,), 1.0 / math.sqrt(d), device=self.dev)
        en = torch.empty(1, d, dtype=self.tdt, device=self.dev)
        ops.rownorm(emb192.to(self.dev, torch.float32).contiguous(), g, None, 1e-30, rows=1, C_=d, rms=True, out_act=en, dtype=self.dtype)
        out = torch.empty(1, self.H, device=self.dev)
        ops.linear(en, sd_linear_w, d, dtype=self.dtype, bias=sd_linear_b, out_f32=out)
        return out

    # ------------------------------------------------------------------ KV pages
    def _set_pages(self, slot: int, rows: int):
        """Makes sure slot `slot` owns pages for `rows` cache rows (allocating what is missing)."""
        need = min((rows + self.page - 1) // self.page, self.max_pages)
        have = self.slot_pages[slot]
        if need > len(have):
            new = self.pages.alloc(need - len(have))
            self.block_table[slot, len(have):need] = torch.tensor(new, dtype=torch.int32)
            have.extend(new)

    def release(self, slot: int):
        """Returns the slot's pages to the free list; the slot idles on the scratch page until the next admit."""
        if self.slot_pages[slot]:
            self.pages.free(self.slot_pages[slot])
            self.slot_pages[slot] = []
            self.block_table[slot].fill_(self.model.trash_page)

    def ensure_capacity(self, ahead: int, pos: Optional[List[int]] = None, active: Optional[List[int]] = None):
        """Called by the host loop between decode steps: every active slot must own pages for the next `ahead` rows
        (the loop polls every few steps, so it allocates that far ahead; a full page list raises)."""
        pos = self.state[ST_POS].tolist() if pos is None else pos
        for s_ in (range(self.B) if active is None else active):
            if self.slot_pages[s_]:
                self._set_pages(s_, pos[s_] + 1 + ahead)

    @torch.no_grad()
    def admit(self, slot: int, x: torch.Tensor, min_len: int, max_len: int, seq_id: int, ahead: Optional[int] = None,
              sampler: Optional[dict] = None, seed: Optional[int] = None):
        """Continuous batching: puts a new request into an idle slot while the other slots keep decoding.  All prompt
        rows but the last are prefetched into freshly allocated pages; the last row becomes the slot's next input, so the
        next ordinary decode step of the batch computes its logits and draws its first token (same Philox key (seed,
        seq id, step 0) as a fixed-batch start) — no separate sampling pass, nothing of the other sequences is touched.
        ahead: cache rows reserved past the prompt.  None reserves the whole max_len (what start() does); a caller that
        passes less MUST call ensure_capacity() between decode steps (run_queue does) — rows past the reservation map to
        the shared scratch page.
        sampler / seed: the request's own (see start); None = the engine's attributes."""
        fields = self._sampler_fields(sampler, seed)
        col = ops.sampler_column(**fields)                # a bad sampler is refused before the slot is touched
        L = x.shape[0]
        if L + max_len > self.max_pages * self.page:
            raise RuntimeError("sequence exceeds the KV cache")
        self.release(slot)
        self._set_pages(slot, L + (max_len if ahead is None else min(ahead, max_len)))
        x = x.to(self.dev, torch.float32).contiguous()
        self._prefill(x[:L - 1], 0, slot)
        self.x_in[slot].copy_(x[L - 1])
        st = torch.tensor([L - 1, 0, 0, 0, min_len, max_len, seq_id, 0], dtype=torch.int32)
        self.state[:, slot].copy_(st)
        self._write_sampler(slot, fields, col)
        self.sampled[slot].fill_(-1)

    def start(self, lm_inputs: List[torch.Tensor], min_lens: List[int], max_lens: List[int], seed=0, seq_ids=None,
              forced: Optional[torch.Tensor] = None, want_logp=False, samplers: Optional[list] = None,
              seeds: Optional[list] = None):
        """Prefills every sequence (prompt rows in chunks of <= 64 through the same kernels as decode) and samples
        the first token of each.  After this, call step()/run().
        samplers: per sequence, a dict over (mode, top_p, top_k, win_size, tau_r, seed) or None; fields left out, and None, mean
        the engine's attributes of those names.  seeds: per sequence, overrides the scalar `seed` (which becomes the engine's)."""
        B = self.B
        assert len(lm_inputs) == B and (samplers is None or len(samplers) == B) and (seeds is None or len(seeds) == B)
        self.seed, self.want_logp = int(seed), want_logp
        self._write_samplers([self._sampler_fields(samplers[b] if samplers else None, seeds[b] if seeds else None) for b in range(B)])
        if forced is not None:
            if self._forced_buf is None:
                self._forced_buf = torch.zeros(B, self.max_out, dtype=torch.int32, device=self.dev)
            self._forced_buf[:, :forced.shape[1]].copy_(forced.to(torch.int32))
            self.forced = self._forced_buf
        else:
            self.forced = None
        st = torch.zeros(8, B, dtype=torch.int32)
        for b in range(B):
            st[ST_MINLEN, b], st[ST_MAXLEN, b] = min_lens[b], max_lens[b]
            st[ST_SEQ, b] = b if seq_ids is None else seq_ids[b]
        self.state.copy_(st)
        self.sampled.fill_(-1)
        for b, x in enumerate(lm_inputs):
            assert x.shape[0] + max_lens[b] <= self.max_pages * self.page, "sequence exceeds the KV cache"
            self.release(b)
            self._set_pages(b, x.shape[0] + min(max_lens[b], self.reserve_ahead))
        if self.prompt_on != "skinny":
            self._prefill_batch(lm_inputs)
        else:
            for b, x in enumerate(lm_inputs):
                self._prefill(x, 0, b, head=True)
                self.state[ST_POS, b] = x.shape[0] - 1   # the sampler's +1 makes it L (= rows in the cache)
        self._tail(B)
        self._fresh_decode_graph()

    def _prefill_batch(self, lm_inputs):
        """All prompts in one pass per layer: rows = B x Lmax (shorter prompts are zero padded; a padded row only adds
        cache entries past its prompt, which the decode steps overwrite before they are read).  RMSNorm, projections
        on the windowed GEMM (weights read once for every prompt), RoPE + KV store + causal attention over the paged
        cache, SwiGLU: 9 launches per layer for the whole batch (32 prompts of 50 rows through the decode kernels cost
        ~58 ms of GPU time: the 1 GB of weights was streamed once per prompt)."""
        B, H = self.B, self.H
        Ls = [int(x.shape[0]) for x in lm_inputs]
        Lm = max(Ls)
        R = B * Lm
        h = torch.zeros(B, Lm, H, device=self.dev)
        for b, x in enumerate(lm_inputs):
            h[b, :Ls[b]].copy_(x)
        h = h.reshape(R, H)
        self._gemm_layers(h, B, Lm, torch.zeros(B, dtype=torch.int32, device=self.dev), self.block_table)
        last = torch.tensor([b * Lm + Ls[b] - 1 for b in range(B)], dtype=torch.long, device=self.dev)
        hl = h.index_select(0, last)
        self.h[:B].copy_(hl)
        self.h_act[:B].copy_(hl)
        self.state[ST_POS].copy_(torch.tensor([L - 1 for L in Ls], dtype=torch.int32))

    def _gemm_layers(self, h, B, Lm, pos, block_table):
        """The layers over B x Lm prompt rows h [B * Lm, H] (fp32, in place) on the windowed GEMM: RMSNorm, projections (weights read
        once for all rows; weight planes when the packs are ops.Planed), RoPE + KV store + causal attention over the paged cache
        from position pos[b], SwiGLU - 9 launches per layer."""
        m = self.model
        dt, H, I = m.dtype, m.H, m.I
        R = B * Lm
        a = torch.empty(R, H, dtype=m.tdt, device=self.dev)
        qkv = torch.empty(R, (m.Hq + 2 * m.Hkv) * m.D, device=self.dev)
        q = torch.empty(R, m.Hq * m.D, dtype=m.tdt, device=self.dev)
        att = torch.empty(R, m.Hq * m.D, dtype=m.tdt, device=self.dev)
        gu = torch.empty(R, 2 * I, device=self.dev)
        act = torch.empty(R, I, dtype=m.tdt, device=self.dev)
        for l, (w, ws) in enumerate(zip(m.pf_layers, m.layers)):
            ops.rownorm(h, w["g1"], None, m.eps, rows=R, C_=H, rms=True, out_act=a, dtype=dt)
            ops.linear(a, w["wqkv"], H, dtype=dt, bias=ws["bqkv"], out_f32=qkv)
            ops.rope_kv_store(qkv, m.inv_freq, pos, q, m.kc[l], m.vc[l], block_table, B=B, rows=Lm,
                              Hq=m.Hq, Hkv=m.Hkv, page=m.page, dtype=dt)
            ops.paged_attn(q, pos, m.kc[l], m.vc[l], block_table, att, B=B, rows=Lm, Hq=m.Hq,
                           Hkv=m.Hkv, page=m.page, dtype=dt)
            ops.linear(att, w["wo"], m.Hq * m.D, dtype=dt, residual=h, out_f32=h)
            ops.rownorm(h, w["g2"], None, m.eps, rows=R, C_=H, rms=True, out_act=a, dtype=dt)
            ops.linear(a, w["wgu"], H, dtype=dt, out_f32=gu)
            ops.swiglu(gu, act, rows=R, I=I, dtype=dt)
            ops.linear(act, w["wdown"], I, dtype=dt, residual=h, out_f32=h)

    def _prefill(self, x, pos0, slot, head=False, norm_out=None):
        """The one prompt entry: the rows x [n, H] go into `slot`'s cache at positions pos0.. in chunks of <= 64 through the
        engine's prompt family (_prefill_chunk; a chunk's hidden rows live in staging buffers the next chunk overwrites, so
        what a caller wants of them is taken here).
        head: the last row's hidden state becomes the slot's h / h_act, what _tail projects (start, feed).
        norm_out fp32 [n, H]: receives hidden_states[-1], the backbone's final RMSNorm of every row (forward_rows)."""
        m = self.model
        x = x.to(self.dev, torch.float32).contiguous()
        for c0 in range(0, x.shape[0], 64):
            hc, hca = self._prefill_chunk(x[c0:c0 + 64], pos0 + c0, slot)
            if norm_out is not None:
                ops.rownorm(hc, m.norm_w, None, m.eps, rows=hc.shape[0], C_=m.H, rms=True, out_f32=norm_out[c0:c0 + 64], dtype=F32)
        if head:
            self.h[slot].copy_(hc[-1])
            self.h_act[slot].copy_(hca[-1])

    def _prefill_chunk(self, xc, pos0, b):
        """<= 64 prompt rows of sequence b through the layers at cache position pos0.  One hipGraph per chunk length over
        static staging buffers: a 50-row prompt is 144 launches, which the host issues in ~1.5 ms eagerly (32 prompts
        in front of a batch: ~50 ms with the GPU mostly idle) and the graph replays in ~0.4 ms."""
        rows = xc.shape[0]
        if self.prompt_on == "gemm":
            hc = xc.to(self.dev, torch.float32).clone()
            self._gemm_layers(hc, 1, rows, torch.tensor([pos0], dtype=torch.int32, device=self.dev), self.block_table[b:b + 1].contiguous())
            return hc, hc.to(self.tdt)
        if not hasattr(self, "_pf"):
            self._pf = dict(h=torch.zeros(64, self.H, device=self.dev), ha=torch.zeros(64, self.H, dtype=self.tdt, device=self.dev),
                            pos=torch.zeros(1, dtype=torch.int32, device=self.dev),
                            bt=torch.zeros(1, self.max_pages, dtype=torch.int32, device=self.dev), graphs={})
        pf = self._pf
        pf["h"][:rows].copy_(xc)
        pf["ha"][:rows].copy_(xc)
        pf["pos"].fill_(pos0)
        pf["bt"].copy_(self.block_table[b:b + 1])
        if rows not in pf["graphs"]:
            pf["graphs"][rows] = Graphed(lambda r=rows: self._layers(pf["h"][:r], pf["ha"][:r], 1, r, pf["pos"], pf["bt"]), self.use_graphs)
        pf["graphs"][rows]()
        return pf["h"][:rows], pf["ha"][:rows]

    def step(self):
        self._decode()

    def close(self):
        """Deterministic teardown of the recorded graphs (decode step, prompt chunks) on the calling thread."""
        if self._decode is not None:
            self._decode.release()
            self._decode = None
        if hasattr(self, "_pf"):
            for g in self._pf["graphs"].values():
                g.release()
            del self._pf

    @torch.no_grad()
    def forward_rows(self, x: torch.Tensor, pos0: int) -> torch.Tensor:
        """Qwen2Encoder.forward_one_step (llm.py:359-371): appends the rows x [n, H] to sequence 0's KV cache at position
        pos0 (full causal attention over the cache) and returns hidden_states[-1] = the final RMSNorm of
        the backbone, fp32 [n, H]."""
        n = x.shape[0]
        if pos0 + n > self.max_pages * self.page:
            raise RuntimeError("sequence exceeds the KV cache")
        if pos0 == 0:
            self.release(0)
        self._set_pages(0, pos0 + n)
        out = torch.empty(n, self.H, device=self.dev)
        self._prefill(x, pos0, 0, norm_out=out)
        return out

    def compact_from(self, big: "LlmEngine", idx: List[int]):
        """Continue the still-active sequences `idx` of `big` in this (smaller-batch) engine: loop state, token
        history, next input embedding and block-table rows are gathered into slots 0..len(idx)-1; the KV pages
        themselves are shared and stay where they are.  Unused slots are marked finished."""
        n = len(idx)
        assert n <= self.B and big.kc is self.kc
        ii = torch.tensor(idx, dtype=torch.long, device=self.dev)
        st = torch.zeros(8, self.B, dtype=torch.int32, device=self.dev)
        st[ST_FIN, n:] = 1
        st[:, :n] = big.state[:, ii]
        self.state.copy_(st)
        self.out_tokens[:n].copy_(big.out_tokens[ii])
        self.sampled[:n].copy_(big.sampled[ii])
        self.x_in[:n].copy_(big.x_in[ii])
        self.block_table.fill_(self.model.trash_page)           # idle slots append their (ignored) KV to the scratch page
        self.block_table[:n].copy_(big.block_table[ii])
        self.seed, self.want_logp = big.seed, False
        self.mode, self.top_p, self.top_k, self.win_size, self.tau_r = big.mode, big.top_p, big.top_k, big.win_size, big.tau_r
        self.samp[:, :n] = big.samp[:, ii]                # every survivor keeps its own sampler and seed
        self._samp_host[:n] = [dict(big._samp_host[i]) for i in idx]
        self.forced = None
        self._fresh_decode_graph()

    def _fresh_decode_graph(self):
        # forced and logp_out are baked POINTER arguments of the sampler launch (seeds, sampler parameters: device data)
        key = (self.forced is None, self.want_logp)
        if self._decode is None or self._graph_key != key:
            if self._decode is not None:
                self._decode.release()
            self._decode = Graphed(self._decode_step, self.use_graphs)
        self._graph_key = key

    def raise_nonfinite(self, err):
        """err: state[ST_ERR] of the slots a caller has just read back.  Code 3 (include/mmx_hip.h): the sampler met logits that are
        not finite and ended the sequence without drawing - an activation left the range of the fp16 planes."""
        bad = [s_ for s_, e in enumerate(err) if e == 3]
        if bad:
            raise RuntimeError(f"slot {bad[0]}: non-finite logits (fp16 plane range: lm_planes='bf16x3')" +
                               (f"; also slots {bad[1:]}" if len(bad) > 1 else ""))

    def host_state(self) -> List[List[int]]:
        """The loop state as host lists [field][slot] in ONE device-to-host copy (the poll of a decode loop: finished flags,
        counts and error codes together); raises for a slot whose logits were not finite."""
        st = self.state.tolist()
        self.raise_nonfinite(st[ST_ERR])
        return st

    def run(self, max_steps: int, poll_every: int = 8) -> List[List[int]]:
        """Decode until every sequence finished or max_steps tokens were tried; returns accepted tokens per sequence."""
        done, st = 1, None                                # start() already sampled step 0
        while done < max_steps:
            n = min(poll_every, max_steps - done)
            if self.reserve_ahead < (1 << 30):
                self.ensure_capacity(n + 1)
            for _ in range(n):
                self._decode()
            done += n
            st = self.host_state()
            if all(st[ST_FIN]):
                break
        if st is None:                                    # max_steps <= 1: start()'s own draw is the only one to check
            st = self.host_state()
        return self.tokens(st[ST_NOUT])

    @torch.no_grad()
    def run_queue(self, requests, seed=0, poll_every: int = 8, ahead: int = 32):
        """Continuous batching over a queue of requests [(lm_input [L, H], min_len, max_len[, sampler[, seed]])]: up to B run at a
        time; when a sequence finishes its pages go back to the allocator and the next queued request is admitted into its slot
        between two decode steps.  Returns the accepted tokens per request (seq id = request index, so the result equals
        running every request alone under the same seed and sampler).  A request's sampler (dict, see start) and seed are
        optional; None / absent = the engine's sampler attributes and `seed`."""
        self.seed, self.want_logp, self.forced = int(seed), False, None
        self._fresh_decode_graph()
        st = torch.zeros(8, self.B, dtype=torch.int32)
        st[ST_FIN] = 1
        self.state.copy_(st)
        for s_ in range(self.B):
            self.release(s_)
        out: List[Optional[List[int]]] = [None] * len(requests)
        owner = [-1] * self.B
        nxt = 0
        while True:
            st = self.host_state()
            fin, nout = st[ST_FIN], st[ST_NOUT]
            for s_ in range(self.B):
                if owner[s_] >= 0 and fin[s_]:
                    out[owner[s_]] = self.out_tokens[s_, :nout[s_]].tolist()
                    owner[s_] = -1
                    self.release(s_)
                if owner[s_] < 0 and nxt < len(requests):
                    x, mn, mx, *own = requests[nxt]
                    self.admit(s_, x, mn, mx, seq_id=nxt, ahead=ahead + poll_every, sampler=(own[0] if own else None),
                               seed=(own[1] if len(own) > 1 else None))
                    owner[s_] = nxt
                    nxt += 1
            active = [s_ for s_ in range(self.B) if owner[s_] >= 0]
            if not active:
                return out
            self.ensure_capacity(ahead + poll_every, active=active)
            for _ in range(poll_every):
                self._decode()

    # ------------------------------------------------------------------ host-driven stream (bistream decode, llm.py:762-870)
    def open_stream(self, seed=0, seq_id=0, want_logp=False, sampler: Optional[dict] = None):
        """One sequence (slot 0) whose LM passes are issued one at a time by the host: text rows and speech-token rows
        arrive interleaved, so the loop of llm.py:786-870 stays on the host; every pass still runs on the HIP kernels and
        the sampler stays on the device.  The loop state (fields of include/mmx_hip.h) is mirrored on the host and
        uploaded before each pass."""
        assert self.B == 1, "bistream decode is single-sequence (cli/model.py:105-112)"
        self.release(0)
        self._set_pages(0, self.max_pages * self.page)        # the text arrives incrementally: reserve the whole context
        self.seed, self.want_logp, self.forced = int(seed), bool(want_logp), None
        self._write_samplers([self._sampler_fields(sampler, None)])
        self._st = dict(rows=0, calls=0, hist=0, seq=int(seq_id), last=None)
        self.sampled.fill_(-1)
        self._fresh_decode_graph()

    def embed_text(self, tok: torch.Tensor, table=None) -> torch.Tensor:
        """llm.model.model.embed_tokens rows (or `table`'s), fp32 [n, H]."""
        tok = tok.reshape(-1).to(self.dev, torch.int64)
        x = torch.empty(tok.numel(), self.H, device=self.dev)
        if tok.numel():
            ops.gather_rows(tok, self.embed_tokens if table is None else table, out_f32=x, dtype=F32)
        return x

    def embed_speech(self, tok: torch.Tensor) -> torch.Tensor:
        return self.embed_text(tok, self.speech_emb)

    def _upload_state(self, pos, ignore_eos):
        s = self._st
        st = torch.tensor([pos, s["calls"], s["hist"], 0, (1 << 30) if ignore_eos else 0, 1 << 30, s["seq"], 0],
                          dtype=torch.int32).reshape(8, 1)
        self.state.copy_(st)

    def feed(self, x: Optional[torch.Tensor], ignore_eos: bool) -> int:
        """One LM pass: appends the rows x [n, H] (None: the embedding of the last accepted token, graph replay) to
        the KV cache and samples from the last row's logits (RAS on the device; ignore_eos as llm.py:259-274).
        Returns the sampled id; call commit() with the id the caller settles on."""
        s = self._st
        n = 1 if x is None else x.shape[0]
        if s["rows"] + n > self.max_pages * self.page or s["calls"] >= self.max_out:
            raise RuntimeError("bistream: sequence exceeds the KV cache (no fill token / eos was produced)")
        if x is None:
            self._upload_state(s["rows"], ignore_eos)
            self._decode()
        else:
            self._prefill(x, s["rows"], 0, head=True)
            self._upload_state(s["rows"] + n - 1, ignore_eos)
            self._tail(1)
        tok = int(self.sampled[0, s["calls"]].item())
        err = int(self.state[ST_ERR, 0].item())
        if err == 2:
            raise RuntimeError("the sampler table's column is out of range (include/mmx_hip.h, mmx_sample_step_tab)")
        self.raise_nonfinite([err])
        if err:
            raise RuntimeError("sampling reaches max_trials 100 and still get eos when ignore_eos is True, check your input!")
        s["rows"] += n
        s["calls"] += 1
        self._last_sampled = tok
        return tok

    def commit(self, token: int):
        """Appends `token` to the decoded history the repetition window reads (bistream keeps fill / eos ids in it,
        llm.py:831) and makes its embedding the next single-row input when it is a speech id."""
        s = self._st
        if token != self._last_sampled or token >= self.eos:
            self.out_tokens[0, s["hist"]] = token
            if token < self.eos:
                self.x_in[0].copy_(self.speech_emb[token])
            elif self._last_sampled < self.eos and s["last"] is not None:
                self.x_in[0].copy_(self.speech_emb[s["last"]])     # the device draw that was overruled moved x_in
        if token < self.eos:
            s["last"] = token
        s["hist"] += 1

    def accepted(self, slots=None, n=None) -> List[torch.Tensor]:
        """The accepted ids of `slots` (default: every slot) as int64 device tensors; n: state[ST_NOUT] as a host list, for a
        caller that has read it already."""
        n = self.state[ST_NOUT].tolist() if n is None else n
        return [self.out_tokens[s_, :n[s_]].to(torch.int64) for s_ in (range(self.B) if slots is None else slots)]

    def tokens(self, n=None) -> List[List[int]]:
        """n: state[ST_NOUT] as a host list, for a caller that has read it already."""
        n = self.state[ST_NOUT].tolist() if n is None else n
        t = self.out_tokens.cpu()
        return [t[b, :n[b]].tolist() for b in range(self.B)]
