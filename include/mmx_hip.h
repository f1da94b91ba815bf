/* mmx_hip.h — C ABI of libmmx_hip.so: the MI355X (gfx950) kernels behind the TTS inference hot path
 * of ishine/minimax-speech (Qwen2 AR speech-token LM -> CosyVoice2 flow-matching decoder -> DAC-VAE
 * decoder).  SURVEY.md §8(b) "C-ABI underneath".
 *
 * The reference has no FFI for this path (it is torch.nn all the way down); each entry point below
 * replaces the torch operator sequence of the cited reference lines, and is what a ctypes binding in
 * the reference would call (INTEGRATION.md shows that stub).
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory unless named h_*;
 *  - the caller owns all buffers; the library keeps no pointer after a call returns and has no
 *    global mutable state -> re-entrant, one stream per caller thread
 *    (reference threading: speech/cosyvoice/cli/model.py:332-335, one llm_job thread per request);
 *  - every launch goes to the `hipStream_t` argument (NULL = legacy default stream), is asynchronous and
 *    capture-safe (no allocation, no synchronisation) so callers can record hipGraphs;
 *  - return 0 on success, MMX_EARG (-1) on an argument/shape error (nothing launched),
 *    <= -1000 for -(hipError_t) - 1000.  The Python host turns non-zero into RuntimeError, matching the
 *    reference's exception/assert convention (flow.py:453, llm.py:273);
 *  - `dtype`: MMX_F32 (parity build: fp32 storage, exact fp32 MFMA) or MMX_BF16 (bf16 storage of weights
 *    and GEMM-input activations, fp32 accumulation and fp32 residual streams).  "T" below means that type.
 *    MMX_X2 / MMX_X3 (the split build): weights are stored and streamed as bf16 exactly as in MMX_BF16, every
 *    activation is stored as fp32 ("T" = float for activations), and each product against an activation runs on the
 *    bf16 MFMA with the activation split into 2 (hi + lo: 16 significant bits) or 3 (24 bits) bf16 terms accumulated
 *    in fp32.  With bf16-representable weights the result is fp32-grade (X3) at the bf16 build's weight bytes.
 *    Entry points without a matrix product treat MMX_X2 / MMX_X3 as MMX_F32.
 *    MMX_X2W / MMX_X3W (the split build on an fp32 CHECKPOINT: mmx_gemm_win, mmx_skinny2): the weights too are carried as 2 / 3
 *    bf16 planes hi + [mid +] lo = w, and a product keeps every term (activation plane s) x (weight plane p) with
 *    s + p < 2 / 3 - three / six bf16 MFMAs per fragment pair, 16 / 24 significant bits of both operands.  Weight layout:
 *    mmx_gemm_win: the planes side by side in every row, W[n][p * (ldw / planes) + k]; mmx_skinny2: the planes' packs one
 *    after the other.  Every other argument as for MMX_X2 / MMX_X3.
 *  - activations are TIME-MAJOR: a [B,C,T] tensor of the reference is stored as rows of C channels.
 */
#ifndef MMX_HIP_H
#define MMX_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP__
typedef struct ihipStream_t* hipStream_t;
#endif

#define MMX_F32 0
#define MMX_BF16 1
#define MMX_X2 2
#define MMX_X3 3
#define MMX_X2W 0x12
#define MMX_X3W 0x13
/* fp16 planes of the LM decode step (mmx_skinny2, mmx_decode_prep, mmx_decode_attn's split output only): activations as TWO fp16
 * planes hi + lo (22 significant bits), weights fp16 and stored * 2^8 - one plane for a bf16-representable checkpoint (MMX_H2),
 * two planes hi + lo for an fp32 checkpoint (MMX_H2W); v_mfma_f32_16x16x32_f16.  Range: |weight| < 255, and for an activation
 * v (= x * gain of its consumer)
 *   |v| < 65520: at or past it the planes are inf / -inf, the products NaN, and mmx_sample_step* ends the sequence with error 3;
 *   the planes hold v to max(2^-22 |v|, 2^-25): 22 bits only where |v| is well above 2^-3.  Per row of a projection (max |err| over
 *   the row / max |ref| of the row, against float64 on exact operands) that is < 3e-6 for rows of scale >= 2^-6 and grows as
 *   2^-25 / scale below: 3.5e-5 at 2^-10, 3.2e-4 at 2^-14, 2.6e-2 at 2^-20 (measured on MI355X = the format's own figures: the MFMA
 *   keeps subnormal fp16 operands).  Nothing fails at the lower end; MMX_X3 has no such edge. */
#define MMX_H2 4
#define MMX_H2W 0x14

/* activation codes */
#define MMX_ACT_NONE 0
#define MMX_ACT_LRELU 1
#define MMX_ACT_GELU 2   /* exact erf gelu (diffusers 0.29 GELU) */
#define MMX_ACT_SILU 3
#define MMX_ACT_MISH 4
#define MMX_ACT_TANH 5

int mmx_abi_version(void);

/* ---------------------------------------------------------------------------------------------
 * Windowed GEMM:  C[b][m][n] = sum_tap sum_c A[b][m*row_stride + tap*dil + row_off][c] * W[b][n][tap*cin + c]
 * Replaces torch Linear / Conv1d / ConvTranspose1d (+ the elementwise ops fused in its epilogue):
 *   dac-vae/model.py:107-143,237-323,342-371 (WNConv1d+LeakyReLU, Snake, WNConvTranspose1d, residual add)
 *   speech/cosyvoice/flow/decoder.py:36-85 (CausalConv1d), speech/matcha/models/components/transformer.py:243-316
 *   (to_q/k/v, to_out, GELU proj, ff out), speech/cosyvoice/transformer Linear layers.
 * Epilogue, per element v:  v += bias;  v = act(v);  v += residual;  v *= rowmask[m];
 *   out_f32[lin] = v;   out_act[lin] = T( alpha ? snake(act2(v), alpha) : act2(v) )
 *   with lin = m*ldo + n + out_off, written only when 0 <= lin < out_len (ConvTranspose1d edge clip).
 */
typedef struct MmxGemmParams {
    const void* A;          /* T, rows of lda elements */
    const void* W;          /* T, [N][ldw], K contiguous, zero padded to a multiple of 32 */
    const float* bias;      /* [bias_mod] (or [M] when bias_per_row) or NULL */
    const float* residual;  /* fp32 [M][ldr] or NULL */
    const float* rowmask;   /* fp32 [M] or NULL */
    const float* alpha;     /* Snake alpha [alpha_mod] for the out_act copy, or NULL */
    float* out_f32;         /* fp32 output or NULL */
    void* out_act;          /* T output or NULL */
    int64_t lda, ldw, ldr, ldo_f, ldo_a;
    int64_t a_bstride, w_bstride, r_bstride, rm_bstride, of_bstride, oa_bstride;   /* per batch, in elements */
    int64_t row_off, row_lo, row_hi;   /* A row = m*row_stride + tap*dil + row_off, rows outside [row_lo,row_hi) read 0 */
    int64_t out_off, out_len;
    int32_t M, N, batch;
    int32_t ntaps, cin, dil;
    int32_t bias_mod, alpha_mod, bias_per_row;
    int32_t act, act2;
    float slope;
    int32_t row_stride;                /* 1 for Linear / stride-1 convs; s for a stride-s Conv1d (DAC-VAE encoder) */
} MmxGemmParams;
int mmx_gemm_win(const MmxGemmParams* p, int dtype, hipStream_t stream);
/* The same launch with the block tile forced (0 = the library's heuristic): a tuning entry for tools/microbench.py. */
#define MMX_TILE_128x128 1
#define MMX_TILE_128x64 2
#define MMX_TILE_64x64 3
#define MMX_TILE_32x64 4
int mmx_gemm_win_tile(const MmxGemmParams* p, int dtype, int tile, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row-wise normalisation (LayerNorm / RMSNorm) with fused tail:
 *   y = norm(x[b][t][:]) * gamma (+ beta);  y = act(y);  y = (y*rowmask + addvec[b][:]) * rowmask
 * written to out_f32 and/or out_act (T).  rms != 0 selects RMSNorm (no mean, beta ignored).  C <= 2048.
 * Replaces nn.LayerNorm (+Mish, + time-embedding add) of decoder.py:65-85 / matcha decoder.py:56-61,
 * transformer.py norm1/norm3, encoder_layer.py norm_mha/norm_ff, Qwen2 RMSNorm (prefill).
 */
int mmx_rownorm(const float* x, int64_t ldx, int64_t x_bstride, int rows, int C, int batch,
                const float* gamma, const float* beta, float eps, int rms, int act,
                const float* rowmask, int64_t rm_bstride, const float* addvec, int64_t av_bstride,
                float* out_f32, int64_t ldo_f, int64_t of_bstride,
                void* out_act, int64_t ldo_a, int64_t oa_bstride, int dtype, hipStream_t stream);

/* GroupNorm over a time-major fp32 tensor [B][T][C] (statistics per (batch, group) over C/groups channels x T),
 * then act (MMX_ACT_NONE / MMX_ACT_MISH) and * rowmask[b][t] (optional), output in T.  Replaces arch_util.py:21-38
 * GroupNorm32 inside LearnableSpeakerEncoder (llm.py:34-96) and GroupNorm + Mish of matcha Block1D (decoder.py:32-43). */
int mmx_groupnorm(const float* x, int B, int T, int C, int groups, const float* gamma, const float* beta, float eps,
                  int act, const float* rowmask, void* out, int dtype, hipStream_t stream);

/* out = act(x) * rowmask[row] on a fp32 [rows][C] tensor (fp32 and / or T output): the stand-alone Mish / SiLU / mask
 * multiplications of the matcha block classes (decoder.py:41-43,49,59; transformer.py) when they are called one by one. */
int mmx_act_rows(const float* x, int64_t rows, int C, int act, const float* rowmask, float* out_f32, void* out_act, int dtype,
                 hipStream_t stream);

/* out[i][:] = table[ids[i]][:] * scale * (rowmask ? rowmask[i] : 1)   (ids < 0 are clamped to 0,
 * flow.py:477).  Replaces nn.Embedding lookups (flow.py:477, llm.py:694-700). */
int mmx_gather_rows(const int64_t* ids, int n, const float* table, int C, float scale, const float* rowmask,
                    float* out_f32, int64_t ldo_f, void* out_act, int64_t ldo_a, int dtype, hipStream_t stream);

/* Strided copy/cast: out[b][r][c] = T(in[b*ibs + r*irs + c*ics]) for r<rows, c<cols; used for
 * [B,C,T] <-> time-major conversions at the API boundary and nearest-neighbour upsampling
 * (row r reads input row r / rep; upsample_encoder.py:60). in_dtype/out_dtype may differ. */
int mmx_copy2d(const void* in, int in_dtype, int64_t ibs, int64_t irs, int64_t ics, int rep,
               void* out, int out_dtype, int64_t obs, int64_t ors, int64_t ocs,
               int rows, int cols, int batch, hipStream_t stream);

/* Estimator input pack (decoder.py:424-432): h[b][t] = [x | mu | spks | cond] as T, + sinusoidal
 * timestep embedding (matcha decoder.py:14-29, scale 1000) emb[b][:] as T.
 * x/mu/cond are fp32 time-major [B][T][80]; batch b reads x[(b % x_mod) * x_bs ...] so the conditional and the
 * unconditional half of a CFG batch share one state tensor (x_mod = number of utterances);
 * spks [B][80]; NULL mu/spks/cond read as zero. */
int mmx_est_pack(const float* x, int64_t x_bs, int x_mod, const float* mu, const float* spks, const float* cond, int B, int T, int C,
                 void* h, int64_t ldh, int dtype, hipStream_t stream);
int mmx_sinusoidal_emb(const float* t, int B, int dim, float scale, void* out, int dtype, hipStream_t stream);

/* CFG + Euler update (flow_matching.py:118-120): x += dt * ((1+cfg)*d[0] - cfg*d[1]); n elements. */
int mmx_cfg_euler(float* x, const float* d_cond, const float* d_uncond, float cfg, float dt, int64_t n,
                  hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Attention.
 * mmx_attn_dense: softmax(q k^T * scale [+ rel-pos term] masked) v for [B][T][H*D] T-typed q/k/v
 *   (row strides ldq/ldk/ldv, head h at column h*D).  Key j is visible to query i iff
 *   j < Tk  and (keymask == NULL or keymask[b][j] != 0) and (chunk == 0 or j < (i/chunk + 1)*chunk);
 *   rows with no visible key output 0 (they are padding rows, masked by every consumer).
 *   rel-pos (pos != NULL): score = ((q+u).k + (q+v).pos[T-1-i+j]) * scale — attention.py:225-330 with
 *   rel_shift folded into the index; pos is [2T-1][H*D] T-typed, u/v fp32 [H][D].
 *   head_stride: column distance between heads inside q/k/v (0 = D; 3*D for the head-interleaved qkv of
 *   arch_util.py:58-77 QKVAttentionLegacy, whose q*s . k*s with s = D^-1/4 equals scale = D^-1/2).
 *   Replaces diffusers Attention (SDPA) of transformer.py:196-204 with the additive bias of
 *   decoder.py:441-445 / common.py:160-168, and RelPositionMultiHeadedAttention.
 * q_begin (multiple of 16; 0 = all): only queries q_begin .. T-1 are computed (keys still 0 .. T-1) — the streaming hop with
 *   cached K / V.
 * mmx_attn_flash_bf16: the MFMA flash-attention kernel for the same contract without rel-pos, bf16,
 *   D = 64, V given TRANSPOSED as vt[b][h*D + d][t] (ldvt elements per row, zero padded).
 *   klen (NULL = none): int32 [B], the number of valid keys of each batch row of a zero-padded batch whose key masks are
 *   prefixes (decoder.py:433-445 with a padding mask): keys j >= klen[b] are invisible, key tiles beyond klen[b] are not
 *   visited, query rows >= klen[b] (padding) that fill a whole workgroup are written as zeros.  Cheaper than the same
 *   mask given as keymask (which makes every tile a masked tile).
 */
int mmx_attn_dense(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs,
                   const void* v, int64_t ldv, int64_t v_bs, void* out, int64_t ldo, int64_t o_bs,
                   int B, int H, int D, int Tq, int Tk, float scale, const float* keymask, int64_t km_bs, int chunk,
                   const void* pos, int64_t ldp, const float* pos_u, const float* pos_v,
                   int head_stride, int q_begin, int dtype, hipStream_t stream);
int mmx_attn_flash_bf16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs,
                        const void* vt, int64_t ldvt, int64_t vt_bs, void* out, int64_t ldo, int64_t o_bs,
                        int B, int H, int T, float scale, const float* keymask, int64_t km_bs, int chunk, int q_begin,
                        const int32_t* klen, hipStream_t stream);
/* Conformer rel-pos attention of the split build (speech/cosyvoice/transformer/attention.py:215-330 incl. rel_shift): fp32
 * q / k / v rows, pos fp32 [2T - 1][ldp] = linear_pos(ESPnet table), pos_u / pos_v fp32 [H * 64]; every product as bf16
 * hi*hi + lo*hi + hi*lo on the MFMA (as mmx_attn_flash_x); klen int32 [B] valid rows per batch member or NULL; out fp32. */
int mmx_attn_relpos_x(const float* q, int64_t ldq, int64_t q_bs, const float* k, int64_t ldk, int64_t k_bs, const float* v,
                      int64_t ldv, int64_t v_bs, const float* pos, int64_t ldp, const float* pos_u, const float* pos_v,
                      float* out, int64_t ldo, int64_t o_bs, int B, int H, int T, float scale, int chunk, const int32_t* klen,
                      hipStream_t stream);
/* mmx_attn_flash_xs: the split build's attention on operands the PRODUCER has already split (MmxEstNext, MMX_X2 with
 * vt_out): qk bf16 [B][T][ldqk >= 2048] = [hi Q | hi K | lo Q | lo K], vt bf16 [B][2][512][ldvt], out fp32 [B][T][ldo].
 * form: 0 = the default workgroup shape (fastest alone: 64-query workgroups on a small grid, else 128-query ones); 1 = the shape that
 * leaves LDS and registers for a co-resident workgroup of another stream (launches beside the LM decode loop) - the same launch as 0
 * since P stays in registers; 2 / 3 = 256-query / 4-wave 64-query workgroups (measurements).  Every form holds 64 KB of LDS.
 * The forms agree to fp32 rounding (different query-tile heights accumulate the online softmax over the same key tiles).
 * mmx_attn_flash_x: the same contract on fp32 operands:
 * q / k / v / out fp32, V ROW-major (v[b][t][h*D + d], ldv elements per
 * row — the QKV projection's own output, no transposed copy), both operands of Q K^T and P V split into bf16 hi + lo
 * (3 MFMAs per product).  Replaces the same reference lines as mmx_attn_flash_bf16. */
int mmx_attn_flash_x(const float* q, int64_t ldq, int64_t q_bs, const float* k, int64_t ldk, int64_t k_bs,
                     const float* v, int64_t ldv, int64_t v_bs, float* out, int64_t ldo, int64_t o_bs,
                     int B, int H, int T, float scale, const float* keymask, int64_t km_bs, int chunk,
                     int q_begin, const int32_t* klen, hipStream_t stream);
int mmx_attn_flash_xs(const void* qk, int64_t ldqk, int64_t qk_bs, const void* vt, int64_t ldvt, int64_t vt_bs,
                      float* out, int64_t ldo, int64_t o_bs, int B, int H, int T, float scale, const float* keymask,
                      int64_t km_bs, int chunk, int q_begin, const int32_t* klen, int form, hipStream_t stream);
/* Conformer rel-pos attention on the MFMA (speech/cosyvoice/transformer/attention.py:215-330), bf16 build:
 *   score(i, j) = ((q_i + pos_u) . k_j + (q_i + pos_v) . pos[T - 1 - i + j]) * scale      (rel_shift folded into the index)
 * q, k: bf16 rows (head h at column h * 64), vt: V TRANSPOSED [B][H * 64][ldvt] (zero padded to ldvt >= round_up(T, 8)
 * columns), pos: bf16 [2T - 1][ldp] = linear_pos(pos_emb) (head h at column h * 64), pos_u / pos_v fp32 [H * 64];
 * chunk > 0: query i sees keys j < (i / chunk + 1) * chunk (streaming); klen (optional, int32 [B]): valid rows per member of
 * a zero-padded batch (keys beyond are masked; `pos` is the table of the padded length T).  Replaces mmx_attn_dense's VALU path for the
 * encoder's 10 layers in the bf16 build; the fp32 / split builds keep mmx_attn_dense. */
int mmx_attn_relpos_bf16(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs,
                         const void* vt, int64_t ldvt, int64_t vt_bs, const void* pos, int64_t ldp,
                         const float* pos_u, const float* pos_v, void* out, int64_t ldo, int64_t o_bs,
                         int B, int H, int T, float scale, int chunk, const int32_t* klen, hipStream_t stream);

/* The same contract (bf16 tensors in HBM) with Q, K, V^T and P quantised to OCP fp8 e4m3 inside the kernel and both
 * products on the fp8 MFMA (BASELINE config 5).  Accuracy: the bound stated in tests/test_gpu_kernels.py (<= 7 % of the output RMS). */
int mmx_attn_flash_fp8(const void* q, int64_t ldq, int64_t q_bs, const void* k, int64_t ldk, int64_t k_bs,
                       const void* vt, int64_t ldvt, int64_t vt_bs, void* out, int64_t ldo, int64_t o_bs,
                       int B, int H, int T, float scale, const float* keymask, int64_t km_bs, int chunk, int q_begin,
                       const int32_t* klen, hipStream_t stream);

/* DAC-VAE encoder head: Conv1d(1 -> C, k) + LeakyReLU (dac-vae/model.py:208 with :509-514) on a mono waveform
 * x fp32 [B][T]; w fp32 [C][k]; out_f32 [B][T][C] (optional) and out_act T [B][T][C] = snake(v, alpha) (alpha optional). */
int mmx_conv_cin1(const float* x, int64_t x_bs, int T, int C, int k, const float* w, const float* bias, float slope,
                  const float* alpha, float* out_f32, void* out_act, int batch, int dtype, hipStream_t stream);
/* VAE head (dac-vae/model.py:476-481): ml fp32 [rows][2D] = (m | logs); logs clamped to [-14, 14];
 * z = m + noise * exp(logs).  All outputs fp32 [rows][D]. */
int mmx_vae_sample(const float* ml, const float* noise, int64_t rows, int D, float* z, float* m, float* logs,
                   hipStream_t stream);
/* x[row][:] = 0 where rowmask[row] == 0, in place; x is T [rows][C] (C a multiple of 16 bytes).  The rows beyond a member's length
 * of a zero-padded batch behind a ConvTranspose1d (dac-vae/model.py:252-284), whose GEMM rows straddle that boundary. */
int mmx_mask_rows(void* x, int64_t rows, int C, const float* rowmask, int dtype, hipStream_t stream);
/* Masked mean over the rows of a time-major fp32 tensor (speech/cosyvoice/llm/llm.py:80-88, LearnableSpeakerEncoder's mean pooling):
 *   out[b][c] = sum_t x[b][t][c] * mask[b][t] / max(sum_t mask[b][t], 1);  mask fp32 [B][m_bs >= rows] or NULL (plain mean).
 * x [B][rows][C] with batch stride x_bs; out T [B][ldo].  Summation order is fixed (no atomics). */
int mmx_pool_rows(const float* x, int64_t x_bs, int rows, int C, int batch, const float* mask, int64_t m_bs, void* out,
                  int64_t ldo, int dtype, hipStream_t stream);
/* Cache prefetch: reads the byte ranges [p_i, p_i + n_i) (16-byte aligned, n_i multiples of 16; NULL = none) with default-policy
 * loads and keeps nothing, so the lines are left in L2 / the Infinity Cache for a later launch (the next LM layer's weights while
 * the current layer computes: a side stream of the captured decode step).  sink: 4 writable bytes (never written in practice). */
int mmx_prefetch4(const void* p0, int64_t n0, const void* p1, int64_t n1, const void* p2, int64_t n2, const void* p3, int64_t n3,
                  void* sink, int workgroups, hipStream_t stream);
/* Speed change (speech/cosyvoice/cli/model.py:312-314): x fp32 [rows][T] -> out fp32 [rows][T2], linear interpolation in time
 * with torch's F.interpolate(mode="linear", align_corners=False) sample positions. */
int mmx_resample_linear(const float* x, int64_t rows, int T, int T2, float* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * DAC tail: Conv1d(C -> 1, k) + LeakyReLU(0.1) + tanh (dac-vae/model.py:364-370,509-514).
 * act: T [B][T][C] (Snake already applied by the producer); w fp32 [k][C]; out fp32 [B][T]. */
int mmx_conv_cout1_tanh(const void* act, int64_t a_bs, int T, int C, int k, const float* w, const float* bias,
                        float slope, int use_tanh, float* out, int64_t o_bs, int batch, int dtype, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Autoregressive LM decode step (speech/cosyvoice/llm/llm.py:745-760 + HF Qwen2 layer).
 *
 * mmx_skinny_gemm: out[b][n] = (rs ? rstd[b] : 1) * sum_k x[b][k] * Wp[n][k] (+bias) for B <= 64 rows:
 *   weights are streamed once, straight to registers, in MFMA-fragment order (pack with mmx_pack_skinny).
 *   x is fp32 [B][ldx] (x_dtype MMX_F32) or T.  rs != 0: rstd[b] = rsqrt(mean_k x^2 + eps) is computed
 *   in-kernel (RMSNorm with its weight pre-folded into Wp).  epi: 0 store fp32 (+bias);
 *   1 SwiGLU: Wp rows are [gate tile | up tile] pairs, out_act[b][n] = T(silu(g)*u);
 *   2 residual: out_f32[b][n] += acc (in place).
 *   flags: MMX_X_PACKED — x (type T) is in MFMA A-fragment order xp[m][kb][lane][E] (lane = g*16 + l16 holds
 *   x[m*16 + l16][kb*KB + g*E + j]; E = 8 bf16 / 4 fp32, KB = 4E; ceil(B/16)*16 rows allocated, ldx ignored);
 *   MMX_OUT_PACKED — out_act is written in that order for a consumer whose K is this N (N % 32 == 0, ldo_a ignored).
 *   Pays at batch > 8, where every workgroup re-reads the whole activation matrix from L2.
 *   dtype MMX_X2 / MMX_X3 (split build): x fp32 row-major (flags 0), Wp the bf16 pack made WITHOUT kscale, kgamma [K] fp32
 *   (or NULL) = the RMSNorm gain applied to x before the split, results to out_f32 only (epi 1 writes silu(g)*u there).
 *   MMX_BF16 with fp32 x (flags 0) also takes kgamma (epi 0 / 1): the gain is applied to x before it is rounded to bf16, Wp
 *   packed without kscale (the form the bf16 build's prompt chunks use, its decode step running on mmx_skinny2).
 */
#define MMX_X_PACKED 1
#define MMX_OUT_PACKED 2
int mmx_pack_skinny(const void* w, int64_t ldw, int N, int K, const float* kscale, int interleave_half,
                    void* wp, int dtype, hipStream_t stream);
int mmx_skinny_gemm(const void* x, int x_dtype, int64_t ldx, int B, int K, int N, const void* wp,
                    const float* bias, int rs, float eps, int epi, float* out_f32, int64_t ldo_f,
                    void* out_act, int64_t ldo_a, int dtype, int flags, const float* kgamma, hipStream_t stream);

/* Decode-step projections, B <= 32 sequences, on SPLIT-PLANE activations (dtype MMX_X3: 3 planes as below; dtype MMX_BF16:
 * ONE plane = bf16(x), which is the packed A-fragment order of MMX_X_PACKED):
 *   an activation x [B][K] (already multiplied by the RMSNorm gain of its consumer) is stored as 3 bf16 planes
 *   hi + mid + lo = x, each in MFMA A-fragment order:
 *     xs[plane s][m][kb][lane = g*16 + l16][j] = term s of x[m*16 + l16][kb*32 + g*8 + j]      (ceil(B/16) row tiles m)
 *   The producer of an activation splits it once; consumers load fragments straight into MFMA operands.
 *   Sum-of-squares tables `ssq` [32 rows][64 tile slots] fp32 carry the RMSNorm statistic the same way: a producer of the
 *   residual stream writes, per 16-column output tile, each row's sum of squares over that tile's columns; the consumer
 *   adds a row's slots (unused slots must be zero: allocate zeroed).
 *
 * mmx_decode_prep: x fp32 [B][K] (K <= 1024) -> h (copy, optional), xs = planes of x * gamma, ssq of x.  The head of a
 *   decode step: the sampler's next input embedding becomes the residual stream and the first projection's operand.
 * mmx_skinny2:  acc[b][n] = rstd[b] * sum_k xs[b][k] * Wp[n][k],  rstd from ssq_in (NULL: 1), Wp the bf16 pack of
 *   mmx_pack_skinny (no kscale);
 *   epi 0: out[b][n] = acc + bias;
 *   epi 1: SwiGLU of [gate tile | up tile] pairs, written as planes xs_out of width N (the down projection's operand);
 *   epi 2: out[b][n] += acc (+ bias) in place (the residual stream); if xs_out: planes of out * gamma_next; if ssq_out:
 *          the per-tile sums of squares of out.
 *   tiles_per_wg (1 | 2; MMX_X3W, three weight planes in registers: 1 only): 16-column tiles a workgroup produces from ONE pass
 *   over xs (8 waves = 8 k slices).
 *   ksplit (1, or > 1 with epi 2): K is also cut into `ksplit` slices across workgroups; partial tiles go through
 *   `part` (>= ksplit * ceil(N/16) * ceil(B/16)*4 * 64 floats) and are summed in slice order by the workgroup that
 *   takes the last ticket of its tile (`tickets`: ceil(N/16) int32, zero before the first launch; left zero).  Launches
 *   that share part / tickets must be ordered on one stream.
 *   Replace the q/k/v, o, gate/up (+SiLU*up), down projections and the llm_decoder head of one decode step
 *   (speech/cosyvoice/llm/llm.py:359-371,749; HF Qwen2 MLP / attention projections / RMSNorm). */
int mmx_decode_prep(const float* x, int64_t ldx, int B, int K, const float* gamma, float* h, int64_t ldh, void* xs,
                    float* ssq, int dtype, hipStream_t stream);
int mmx_skinny2(const void* xs, int B, int K, int N, const void* wp, const float* bias, const float* ssq_in, float eps,
                int epi, float* out, int64_t ldo, void* xs_out, const float* gamma_next, float* ssq_out,
                int tiles_per_wg, int ksplit, float* part, int64_t part_floats, int32_t* tickets, int dtype,
                hipStream_t stream);

/* RoPE (HF rotate_half; inv_freq[D/2] fp32 = 1/theta^(2i/D) as HF computes it) on q/k of
 * qkv[b][t][: (Hq+2Hkv)*D] at position pos[b] + t, K/V appended to the paged cache, q written as T.  Cache layout:
 * kc/vc [n_pages][Hkv][page][D] T, block_table [B][max_pages] int32.  rows = tokens per sequence. */
int mmx_rope_kv_store(const float* qkv, int64_t ldqkv, int64_t qkv_bs, int B, int rows, int Hq, int Hkv, int D,
                      const float* inv_freq, const int32_t* pos, void* q_out, int64_t ldq, int64_t q_bs,
                      void* kc, void* vc, const int32_t* block_table, int max_pages, int page,
                      int dtype, hipStream_t stream);
/* Causal GQA attention over the paged cache: query row t of sequence b sees keys [0, pos[b] + t]. */
int mmx_paged_attn(const void* q, int64_t ldq, int64_t q_bs, int B, int rows, int Hq, int Hkv, int D, float scale,
                   const int32_t* pos, const void* kc, const void* vc, const int32_t* block_table, int max_pages,
                   int page, void* out, int64_t ldo, int64_t o_bs, int dtype, hipStream_t stream);
/* Single-token decode: RoPE(q), RoPE(k_new), KV append and causal GQA attention in ONE launch per layer
 * (same arithmetic as mmx_rope_kv_store + mmx_paged_attn with rows = 1).  qkv fp32 [B][ldqkv], out T [B][ldo].
 * rope_tab (optional, fp32 [max_pos][D] = cos | sin per position, as HF's rotary embedding computes them) replaces
 * the in-kernel cosf/sinf of pos * inv_freq.
 * out_packed: an OR of the MMX_DA_* switches below; any other bit is an error.
 *   MMX_DA_PACKED   out in the packed A-fragment order of T (MMX_OUT_PACKED, K = Hq*D) instead of row-major.
 *   MMX_DA_PER_HEAD the per-query-head kernel even where the GQA-shared one applies (bf16, page = 16, Hq = 7 Hkv: one workgroup per
 *                   kv head serves its 7 query heads, Q K^T on the MFMA with the queries split into bf16 hi + lo).
 *   MMX_DA_SPLIT    out as SPLIT PLANES, three bf16 terms (see mmx_skinny2); dtype MMX_F32 / the split builds only, without MMX_DA_PACKED.
 *   MMX_DA_H2       out as TWO fp16 planes (MMX_H2); same conditions, and not together with MMX_DA_SPLIT.
 *   MMX_DA_ONE_HEAD the per-head kernel with ONE query head per workgroup at every batch size (default: from B * Hq > 256 on, two
 *                   heads share a workgroup's K / V reads; same results bit for bit). */
#define MMX_DA_PACKED 1
#define MMX_DA_PER_HEAD 2
#define MMX_DA_SPLIT 4
#define MMX_DA_H2 8
#define MMX_DA_ONE_HEAD 16
int mmx_decode_attn(const float* qkv, int64_t ldqkv, int B, int Hq, int Hkv, int D, const float* inv_freq,
                    const float* rope_tab, const int32_t* pos, void* kc, void* vc, const int32_t* block_table, int max_pages, int page,
                    float scale, void* out, int64_t ldo, int dtype, int out_packed, hipStream_t stream);
/* mmx_decode_attn with the loop's `finished` flags (int32 [B], indexed like pos; NULL = mmx_decode_attn): the workgroups of a
 * sequence whose flag is non-zero return at once - no K/V append, no cache read, its output row keeps what it held.  For decode
 * loops that keep an ended sequence in its slot (pos frozen, its outputs ignored) until the slot is given to another one. */
int mmx_decode_attn_fin(const float* qkv, int64_t ldqkv, int B, int Hq, int Hkv, int D, const float* inv_freq,
                        const float* rope_tab, const int32_t* pos, const int32_t* finished, void* kc, void* vc,
                        const int32_t* block_table, int max_pages, int page, float scale, void* out, int64_t ldo, int dtype,
                        int out_packed, hipStream_t stream);
/* SwiGLU for prefill: out = T(silu(gu[:, :I]) * gu[:, I:2I]) */
int mmx_swiglu(const float* gu, int64_t ldgu, int rows, int I, void* out, int64_t ldo, int dtype, hipStream_t stream);

/* Sampler = log_softmax + ras_sampling + sampling_ids + the loop bookkeeping of inference_wrapper
 * (llm.py:259-274,751-760; utils/common.py:111-139), one workgroup per sequence, all state on device:
 *   state[field * B + b], fields {0 pos, 1 step, 2 n_out, 3 finished, 4 min_len, 5 max_len, 6 seq_id, 7 error}
 *   (int32, field-major so that &state[0] is the pos[] array the attention kernels read)
 * Draws follow oracle/philox.py (Philox4x32-10 keyed by seed; exponential race == torch.multinomial).
 * On an accepted token: appended to out_tokens[b][n_out++], next_x[b][:] = speech_emb[token][:].
 * EOS (== eos_id) sets finished; ids > eos_id leave next_x unchanged (llm.py:755-756).
 * Every call advances state.step and state.pos (+1) of unfinished sequences.
 * forced != NULL: teacher forcing, forced[b*max_out + step] replaces the accepted token (the sampled id is
 * still recorded in sampled[b][step]).  logp_out (optional, fp32 [B][V], pitch V) receives log_softmax(logits).
 * Shapes: any 0 < V <= 6656, any eos_id < V, any E > 0, any ldl >= V and ldx >= E are served; row b of the logits is
 *   logits[b * ldl .. b * ldl + V), columns V..ldl of a row are never read (they may hold anything, NaN included).
 * What a step writes, for an unfinished sequence b with valid logits and parameters: sampled[b][step] (if sampled != NULL),
 *   logp_out[b][0..V) (if logp_out != NULL), words of state column b, and - on an accepted token only - out_tokens[b][n_out] and
 *   next_x[b * ldx .. b * ldx + E).  No other word of any buffer is written: the rest of the rows, the words between E and ldx,
 *   and every other sequence's rows keep their bits (tests/test_gpu_sampler_edges.py checks this contract).
 * Candidates are the reference's for every valid distribution - exact ties are broken by index as its stable sort does, and a
 *   row with more elements at or above the selection threshold than the kernel's candidate list holds is selected exactly too
 *   (slower).  tau_r is taken as fp32: win_size * tau_r can differ from the reference's double product at an exact integer.
 * error (field 7): 0 none; 1 = 100 EOS re-draws under ignore_eos still gave EOS (llm.py:271-273 raises there; the id is accepted:
 *       sampled[b][step] = eos_id, finished = 1, step + 1, nothing appended);
 *   2 = the sequence's column of the sampler table is out of range (mmx_sample_step_tab only, see below);
 *   3 = the sequence's logits are not finite - a NaN, a +inf, or every one of them -inf, which is what an activation past the
 *       range of the fp16 planes (MMX_H2 above) turns into: state.finished = 1 for THAT sequence, nothing is drawn, its pos /
 *       step / n_out, out_tokens, sampled and next_x rows keep what they held (logp_out of the row is unspecified); the other
 *       sequences of the launch are not affected.  -inf among finite logits is legal (probability 0) and not flagged. */
int mmx_sample_step(const float* logits, int64_t ldl, int V, int B, int eos_id, int top_k, float top_p,
                    int win_size, float tau_r, uint64_t seed, int32_t* state, int32_t* out_tokens, int max_out,
                    int32_t* sampled, const int32_t* forced, const float* speech_emb, int E, float* next_x,
                    int64_t ldx, float* logp_out, hipStream_t stream);
/* The same step with the sampler's parameters PER SEQUENCE in device memory instead of launch scalars, so that a recorded decode
 * step holds none of them (a new seed or nucleus width needs no new hipGraph) and every request of a batch has its own:
 *   samp[field * B + b] (int32, field-major like `state`), fields
 *     {0 mode, 1 top_k, 2 win_size, 3 top_p (fp32 bits), 4 tau_r (fp32 bits), 5 seed low word, 6 seed high word, 7 reserved = 0}
 *   mode 0: ras_sampling (common.py:111-116) = what mmx_sample_step does;
 *   mode 1: nucleus_sampling alone (common.py:119-134): the candidate prefix and the draw from noise stream which = 0, no
 *           repetition window (win_size and tau_r are range-checked but unused);
 *   mode 2: random_sampling alone (common.py:137-139): the full-vocabulary draw from noise stream which = 1 (top_p unused).
 *   In every mode the EOS re-draw loop of llm.py:259-274 advances the trial index as in mode 0, and the noise is
 *   oracle/philox.py exp_noise(seed, seq_id, step, trial, which, .).
 * The kernel range-checks each column (the host cannot: the values are in device memory): mode outside 0..2, top_k outside 1..64 or
 * win_size outside 0..64 sets state.error = 2 and state.finished = 1 for THAT sequence and draws nothing (out_tokens, sampled and
 * next_x rows untouched); the other sequences of the launch are not affected.  Every other argument as for mmx_sample_step. */
int mmx_sample_step_tab(const float* logits, int64_t ldl, int V, int B, int eos_id, const int32_t* samp, int32_t* state,
                        int32_t* out_tokens, int max_out, int32_t* sampled, const int32_t* forced, const float* speech_emb,
                        int E, float* next_x, int64_t ldx, float* logp_out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Row-tile fused kernels of the CFM estimator (csrc/fused.hip).  One workgroup takes a tile of `bm` frames of one
 * sequence through every row-local op between two attentions, so a transformer block is 2 launches (this + attention).
 * Dimensions are those of speech/config.yaml:104-116: C = 256 channels, 8 heads x 64, FF 1024.
 * Weights are in MFMA fragment order (mmx_pack_skinny of the [N][K] matrix; Conv1d k3: K = tap*Cin + c).
 *
 * MmxEstNext (optional, wqkv != NULL): LayerNorm (n1g, n1b) of the result followed by the Q/K/V projection of the NEXT
 *   transformer block (matcha transformer.py:256-285: norm1 -> attn1.to_q/to_k/to_v, no bias).
 *   MMX_BF16: q_out = [B][T][ldq >= 1024] (Q | K) and vt_out = V transposed [B][512][ldvt] (frames >= T written as 0);
 *   MMX_F32 : q_out = [B][T][ldq >= 1536] (Q | K | V), vt_out unused.
 *   MMX_X2  : vt_out == NULL: fp32 q_out = [B][T][ldq >= 1536] (Q | K | V);  vt_out != NULL: the operands of
 *             mmx_attn_flash_xs, split here once: q_out bf16 [B][T][ldq >= 2048] = [hi Q | hi K | lo Q | lo K] and
 *             vt_out bf16 [B][2 planes][512][ldvt] (V transposed, hi then lo; vt_bs >= 2 * 512 * ldvt).
 * mmx_est_tail: x += attn1.to_out(ao) ; x += ff(norm3(x))  (transformer.py:286-313), x fp32 [B][T][256] in place;
 *   rowmask (optional) multiplies the result; act_out (optional) receives T(x) with row stride act_ld.
 * mmx_est_resnet: CausalResnetBlock1D (flow/decoder.py:65-85 + matcha decoder.py:56-61):
 *   h = mish(LN(conv3(a_in) + b1)) * m;  h = (h + tv[b]) * m;  h = mish(LN(conv3(h) + b2)) * m;
 *   x = h + conv1(a_in) + br.  a_in T [B][T][lda] (cin columns, already masked); tv = mlp(mish(t_emb)) fp32 [B][256].
 * bm: 16 / 32 / 64 (bf16), 16 / 32 (fp32 tail), 16 (fp32 resnet).
 * t_begin > 0 (streaming with cached state, config 5): only frames t_begin .. T-1 are computed; every buffer is indexed by
 * absolute frame with the batch strides given, so the rows of earlier hops (the conv halo, the K / V rows) are found
 * where those hops left them.
 */
typedef struct MmxEstNext {
    const void* wqkv;
    const float* n1g;
    const float* n1b;
    void* q_out;
    void* vt_out;
    int64_t q_bs, vt_bs;
    int32_t ldq, ldvt;
} MmxEstNext;
typedef struct MmxEstTailParams {
    const void* ao;         /* T [B][T][ldao], 512 columns: attention output */
    float* x;               /* fp32 [B][T][256] residual stream, in place */
    const void* wo;         /* packed [256][512] */
    const void* w1;         /* packed [1024][256] */
    const void* w2;         /* packed [256][1024] */
    const float* bo;
    const float* b1;
    const float* b2;
    const float* n3g;
    const float* n3b;
    const float* rowmask;   /* fp32 [B][T] or NULL */
    void* act_out;          /* T or NULL */
    int64_t ao_bs, x_bs, rm_bs, act_bs;
    int32_t ldao, act_ld, B, T;
    int32_t t_begin;        /* first frame to process (multiple of 16; 0 = all): frames before it are only read */
    float eps;
    MmxEstNext next;
} MmxEstTailParams;
typedef struct MmxEstResnetParams {
    const void* a_in;
    float* x;               /* fp32 [B][T][256] out */
    const void* w1;         /* packed [256][3*cin] */
    const void* w2;         /* packed [256][768] */
    const void* wr;         /* packed [256][cin] */
    const float* b1;
    const float* g1;
    const float* be1;
    const float* b2;
    const float* g2;
    const float* be2;
    const float* br;
    const float* tv;        /* fp32 [B][...], row stride tv_bs, this block's 256 values */
    const float* rowmask;
    int64_t a_bs, x_bs, tv_bs, rm_bs;
    int32_t lda, cin, B, T;
    int32_t t_begin;        /* as in MmxEstTailParams; the causal halo rows t_begin-18 .. are read from a_in */
    float eps;
    MmxEstNext next;
} MmxEstResnetParams;
/* cfg = pf + 16 * waves + 512 * narrow (0 = the library's defaults; mmx_est_tail only: narrow = 8 waves with 32-column passes,
 * the bf16 default for 64 / 32 rows and the form of the split build's 64-row tile): pf = k-steps of weight fragments a wave keeps in flight (2 / 4 / 8);
 * bm = rows per workgroup: 64 / 32 / 16 (MMX_BF16, MMX_X2, MMX_X2W), 32 / 16 (MMX_F32).  The split build's 64-row tile takes the
 * attention rows in two K halves and the FF intermediate in 256-wide chunks (two bf16 planes of 64 rows fit LDS that way) and is
 * bit-identical to its 32-row tile;
 * waves = 4 (one wave per SIMD, 64-column slices) or 8 (two per SIMD, 32-column slices: one wave's epilogue runs under the
 * other's MFMA stage; bf16 only).  Any other value of a field (pf = 3, waves = 5, a bit above these, 512 for mmx_est_resnet) is MMX_EARG, as is a
 * (dtype, bm, cfg) the build has no instantiation for; MMX_X2W takes the split build's default form, whatever cfg says. */
int mmx_est_tail(const MmxEstTailParams* p, int dtype, int bm, int cfg, hipStream_t stream);
int mmx_est_resnet(const MmxEstResnetParams* p, int dtype, int bm, int cfg, hipStream_t stream);
/* ---------------------------------------------------------------------------------------------
 * DAC-VAE ResidualUnit as one kernel (dac-vae/model.py:107-143; :509-514: LeakyReLU(slope) after every Conv1d):
 *     x_out = x + lrelu(conv1(snake_a2(lrelu(conv7, dilation dil (snake_a0(x))))))      [act_out = snake_alpha_next(x_out)]
 * for the narrow decoder stages, C = 48 / 96 / 192, and the encoder's first two, C = 64 / 128 (MMX_BF16 and MMX_X2 only: the
 * encoder has no weight planes, MMX_X2W with C = 64 / 128 is MMX_EARG); dtype MMX_BF16 or MMX_X2 (the fp32 build runs the unit as two
 * mmx_gemm_win launches).  x / x_out: fp32 [B][T][C] residual stream (batch stride x_bs elements; x_out must not alias x:
 * neighbouring tiles read each other's halo rows); act_out (optional): the next layer's input activation, bf16 (MMX_BF16) or
 * fp32 (MMX_X2), same strides.  x_out may be NULL when act_out is given (the last unit of an encoder block, whose residual
 * stream nobody reads): nothing is written for it and act_out keeps the bits it has with x_out; both NULL is MMX_EARG.  w7 / w1: mmx_pack_skinny packs of the weight matrices [C][7 * CP] (tap-major, each tap's
 * C input channels zero-padded to CP = 32 * ceil(C / 32)) and [C][CP].  lens (optional, int32 [B]): rows >= lens[b] of batch
 * member b are conv padding - read as zero, written as zero (utterances of different lengths decoded in one batch).
 * bm: rows per workgroup, 0 = the library's default for (C, dtype); a height the build has no instantiation for is MMX_EARG
 * (MMX_X2W has the default tile only). */
typedef struct {
    const float* x;
    float* x_out;
    void* act_out;
    const void* w7;
    const void* w1;
    const float* b7;
    const float* b1;
    const float* a0;
    const float* a2;
    const float* alpha_next;
    const int32_t* lens;
    int64_t x_bs;
    int32_t B, T, C, dil;
    float slope;
} MmxDacRuParams;
int mmx_dac_ru(const MmxDacRuParams* p, int dtype, int bm, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Reference audio -> log-mel frames in one launch (speech/matcha/utils/audio.py:45-82 with center=False: reflect padding by
 * pad = (n_fft - hop) / 2, torch.stft with a periodic Hann window of win_size == n_fft, sqrt(re^2 + im^2 + 1e-9), the mel
 * filterbank, log(max(v, 1e-5))); with `gain` also the peak normalisation of cosyvoice/dataset/processor.py:385-387.
 *   wave  fp32 [B][w_bs >= L] mono rows; gain fp32 [B] or NULL: sample * gain[b] (rounded to fp32) is what is analysed;
 *   lens  int32 [B] or NULL: valid samples per member of a zero-padded batch, each reflected at its OWN end; h_lens: the same
 *         values in HOST memory (given exactly when lens is), so that the call can refuse a member before anything is launched.
 *   Member b has frames(len) = (len + 2 * pad - n_fft) / hop + 1 frames (len / hop when hop divides len); frame t covers the
 *   padded samples t * hop .. t * hop + n_fft - 1.  The reflection is index arithmetic on the row: no padded copy exists.
 *   basis bf16 [3][2 * nbp][n_fft], nbp = n_bins rounded up to 32: three planes hi + mid + lo of the float64 values
 *         hann[k] * cos(2 pi (bin0 + i) k / n_fft) (row 32 * (i / 16) + i % 16) and hann[k] * sin(..) (that row + 16), rows of bins
 *         >= n_bins zero, each plane in mmx_pack_skinny order;
 *   filt  bf16 [3][mp][nbp], mp = n_mels rounded up to 16: three planes of the fp32 filterbank columns bin0 .. bin0 + n_bins - 1
 *         (zero padded), each plane in mmx_pack_skinny order.  Only bins with a non-zero filter weight need to be passed
 *         (fmax = 8000 at 24 kHz, n_fft 1920: bins 1 .. 639 of 961).
 *   Both products run on the bf16 MFMA with the samples / magnitudes split into three bf16 terms in the kernel and every term
 *   pair s + p < 3 kept, fp32 accumulation: one arithmetic for every `dtype`, which only selects the type T of out_tm.
 *   out_cm fp32 [B][n_mels][ldo >= T] (the reference function's layout) and / or out_tm T [B][T][n_mels] (time-major, the speaker
 *   encoder's input); frames t >= frames(lens[b]) are written as 0 (the collate's zero padding, processor.py:658).
 * MMX_EARG: n_fft % 32 != 0, n_mels > 128, hop % 8 != 0, n_fft - hop odd, a member (or L) with at most pad samples (the reflection
 *   is undefined; torch raises there too) or too few for one frame, T smaller than a member's frame count, or tables that do not fit 160 KB of LDS. */
int mmx_logmel(const float* wave, int64_t w_bs, int L, int B, const float* gain, const int32_t* lens, const int32_t* h_lens,
               const void* basis, const void* filt, int n_fft, int hop, int bin0, int n_bins, int n_mels, float* out_cm,
               int64_t ldo, void* out_tm, int T, int dtype, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The S3 speech tokenizer's own kernels (speech/tools/S3Tokenizer/s3tokenizer, class S3TokenizerV2; cli/frontend.py:92-102).  Its
 * convolutions, LayerNorms, projections, MLP and attention run on mmx_gemm_win (row_stride 2), mmx_rownorm and
 * mmx_attn_flash_x / mmx_attn_dense.
 *
 * mmx_logmel_w: 16 kHz clip -> Whisper-convention log-mel (s3tokenizer/utils.py:220-267 log_mel_spectrogram): torch.stft with
 * center=True (reflect padding by n_fft / 2 on each side) and a periodic Hann window, the last frame dropped (a member of len
 * samples has len / hop frames), the POWER spectrum re^2 + im^2, the mel filterbank, log10(max(v, 1e-10)), the floor at
 * (maximum over the whole clip) - 8, then (v + 4) / 4.  Arguments and tables as for mmx_logmel, except:
 *   n_fft needs to be a multiple of 16 only (400): the K dimension of the basis is zero padded to kp = n_fft rounded up to 32,
 *   basis bf16 [3][2 * nbp][kp]; the frame itself is not changed;
 *   there is no gain.
 * Two launches: the first writes the log10 values (and 0 for the frames t >= len / hop of a member), the second - one workgroup
 * per clip - takes the maximum over the clip's own valid frames and applies the floor and the affine map to them.  A maximum
 * has no order and a wave owns whole column tiles, so a member of a zero-padded batch gets the bits of its solo run.
 *   out_cm fp32 [B][n_mels][ldo >= T] and / or out_tm T [B][T][n_mels]; a bf16 out_tm needs out_cm beside it (the maximum is
 *   taken over the fp32 values).
 * MMX_EARG: as mmx_logmel; a member with at most n_fft / 2 samples (the reflection is undefined; torch raises there too).
 */
int mmx_logmel_w(const float* wave, int64_t w_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const void* basis,
                 const void* filt, int n_fft, int hop, int bin0, int n_bins, int n_mels, float* out_cm, int64_t ldo,
                 void* out_tm, int T, int dtype, hipStream_t stream);

/* mmx_s3_rope_fsmn: what FSMNMultiHeadAttention.qkv_attention does between the projections and the softmax
 * (s3tokenizer/model_v2.py:51-70 apply_rotary_emb, :177-189 forward_fsmn, :204-207), in one launch, fp32:
 *   qkv  fp32 [B][T][ldqkv >= 3C] = [Q | K | V] of the fused projection, heads of 64 channels (C a multiple of 64).  Q and K are
 *        rotated IN PLACE: y[d] = x[d] * cos[t][d % 32] + (d < 32 ? -x[d + 32] : x[d - 32]) * sin[t][d % 32], position t = the row
 *        index, evaluated unfused as torch does; the reference's two D^-1/4 factors are the attention's scale = D^-1/2.
 *   rope_cos / rope_sin fp32 [rope_rows >= T][32]: the real and imaginary parts of precompute_freqs_cis(64, 2048), built on the
 *        host with the reference's own torch calls (no device trigonometry);
 *   wt   fp32 [31][C]: fsmn_block.weight [C][1][31] transposed (tap-major);  x fp32 [B][T][C]: the block's input (residual);
 *   r    fp32 [B][T][C] = x + (depthwise31(v m) + v m) m, m = (t < lens[b]); zero padding 15 / 15, the 31 taps summed in tap
 *        order.  The out-projection's `residual` epilogue then finishes x + out(attn) + fsmn.
 *   lens int32 [B] or NULL (= T): rows t >= lens[b] get r = x (bit for bit) and zero q / k, and their v is read as zero.
 * One wave per (head, 32-row time tile): lane = channel, the RoPE partner is lane ^ 32, the tile's v rows and their halo in LDS. */
int mmx_s3_rope_fsmn(float* qkv, int64_t ldqkv, int64_t qkv_bs, int B, int T, int C, const float* x, int64_t x_bs, float* r,
                     int64_t r_bs, const float* wt, const float* rope_cos, const float* rope_sin, int rope_rows,
                     const int32_t* lens, hipStream_t stream);

/* mmx_fsq_encode: FSQCodebook.encode (s3tokenizer/model_v2.py:96-112): per row of x fp32 [B][T][ldx >= C]
 *   h = W x + bias (W fp32 [8][C] = project_down.weight as loaded, fp32 dot products);  v_i = tanhf(h_i) * 0.9990000128746033f;
 *   ids[b][t] = sum_i (rintf(v_i) + 1) * 3^i  (round half to even, digits in {0, 1, 2}, id in [0, 6561)), int32 [B][ld_ids >= T];
 *   pre (optional) fp32 [B][T][8] receives the v_i.  lens int32 [B] or NULL: rows t >= lens[b] get id 0 (and v = 0). */
int mmx_fsq_encode(const float* x, int64_t ldx, int64_t x_bs, int B, int T, int C, const float* W, const float* bias,
                   const int32_t* lens, int32_t* ids, int64_t ld_ids, float* pre, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * mmx_resample_sinc: sample-rate conversion of a ragged batch of mono clips in one launch, the polyphase windowed-sinc FIR that
 * torchaudio documents as `sinc_interp_hann` (what cosyvoice/utils/file_utils.py:44-50 and cli/frontend.py:157-162 call).
 *   orig -> neu: the two rates divided by their gcd (coprime, different).  With base = min(orig, neu) * rolloff and
 *   width = ceil(lpw * orig / base), output j = f * neu + p (frame f, phase p) of a clip x[0 .. len) is
 *       y[j] = sum_k h[p][k] * x[f * orig + k - width],   k in [0, 2 * width + orig),   x = 0 outside [0, len),
 *       h[p][k] = fp32((base / orig) * sinc(pi t) * cos^2(pi t / (2 lpw))),  t = base * ((k - width) / orig - p / neu) in float64,
 *   and a clip has ceil(neu * len / orig) outputs (64-bit arithmetic).  Taps with |t| >= lpw are exactly 0 in fp32, so the bank
 *   arrives packed (mmx/resample.py builds it):
 *   first int32 [neu]: the dense index k of a phase's first live tap;  count int32 [neu]: its live taps (<= cmax <= 2 * width);
 *   taps  fp32 [cmax][neu], tap-major: taps[c][p] = h[p][first[p] + c], zero beyond count[p].
 *   wave  fp32 [B][w_bs >= L];  lens int32 [B] or NULL (= L): valid samples per clip, each >= 1, h_lens the same values in HOST
 *         memory (given exactly when lens is); samples at or beyond lens[b] are never read.
 *   out   fp32 [B][o_bs >= out_cols]: columns [0, ceil(neu * lens[b] / orig)) hold the result, the columns from there to out_cols
 *         are written as 0, nothing else is written.
 * A workgroup owns MMX_RESAMPLE_NOUT consecutive outputs of one clip and holds the packed bank and the input span under them in
 * LDS.  Every output is one thread's fp32 sum over its live taps in ascending order (fmaf), so a clip's bits do not depend on the
 * batch, on its row or on the workgroup.
 * MMX_EARG: rates that are equal or not coprime, a length outside [1, L], out_cols smaller than a clip's output count, or a rate
 *   pair whose packed bank plus input span, (cmax * neu + ceil((MMX_RESAMPLE_NOUT - 1) * orig / neu) + 2 * width + 2) * 4 bytes,
 *   exceeds 64 KB of LDS (16001 -> 16000 does; every pair of the usual audio rates is far below).  Nothing is launched then. */
#define MMX_RESAMPLE_NOUT 1024
int mmx_resample_sinc(const float* wave, int64_t w_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, int orig, int neu,
                      int width, const float* taps, const int32_t* first, const int32_t* count, int cmax, float* out,
                      int64_t o_bs, int out_cols, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Loudness (csrc/loudness.hip; the definition is stated in mmx/loudness.py): ITU-R BS.1770-4 integrated loudness as
 * dac-vae/audiotools/core/loudness.py computes it (Meter.integrated_loudness, LoudnessMixin.loudness) and the gain of
 * core/effects.py:181-220 (normalize, ensure_max_of_audio), over a ragged batch, without a host sync.
 *   rate: one with int(0.4 rate) == 4 * S, S = int(0.4 rate 0.25) (16 000, 22 050, 24 000, 44 100, 48 000 among them): a 400 ms block
 *         is then four sub-blocks of S samples.  A row of len samples counts as n' = len + int((0.5 - len / rate) * rate) samples when it
 *         is shorter than 0.5 s (zeros), and has nsub = ceil(n' / S) sub-blocks with MMX_LOUD_PAD (julius.core.unfold: the tail zero
 *         padded), n' / S with MMX_LOUD_DROP (BS.1770 / pyloudnorm); its blocks are the nsub - 3 runs of four sub-blocks.
 *   cap:  columns of the per-sub-block arrays, >= ceil(max(L, rate / 2 + 1) / S).
 *   lens  int32 [rows] or NULL (= L), clamped to [0, L]; samples at or beyond lens[b] are never read.
 *
 * mmx_kweight_blocks: wave fp32 [B][w_bs >= L] mono rows ->
 *   energy f64 [B][e_bs >= cap]: energy[b][i] = sum of squares of the K-weighted row over the samples of sub-block i below n' (the
 *          tail block is padded AFTER the filter, as julius.core.unfold does), i < nsub; 0 from there to cap;
 *   peak   fp32 [B]: max |x| over the row's len samples.
 *   tab    f64 [10 + 16 * 8] in device memory (mmx/loudness.py tables): the two biquads (b0, b1, b2, a1, a2 each, a0 = 1; shelf first),
 *          then row-major 4 x 4 powers of the transition matrix A of the cascade's transposed-direct-form-II state: A^(seg 2^k) for
 *          k = 0 .. 6, then A^S.  seg: samples per lane, S % seg == 0, seg <= 64, S / seg <= 127.
 *   work   f64 [B][cap][5]: scratch (sub-block states and peaks).
 *   Three launches: zero-state segment walks and a scan over the lanes per sub-block; one wave per row carrying the state across
 *   sub-blocks; the walk from the true state that sums the squares.  State and sums are fp64.  A row's values depend on its own
 *   samples, length and rate only: solo and batched runs agree bit for bit.
 * mmx_loudness_gate: one wave per clip of nch <= MMX_LOUD_MAX_CH adjacent rows (lens[clip * nch] is the clip's length) ->
 *   lufs fp32 [nclips]: l_j = -0.691 + 10 log10 sum_c G[c] z[c][j], z = block energy / (0.4 rate); the blocks with l_j > -70 give
 *   Gamma_r = (loudness of their mean z) - 10; the blocks above both give the result; no block, or a result below -70: -70.
 *   G f64 [nch] in HOST memory or NULL (1, 1, 1, 1.41, 1.41).  want_gain: gain fp32 [nclips] = exp((target_db - lufs) ln10 / 20), or
 *   max_peak / peak where that gain would lift the clip's peak above max_peak (then gain * peak <= max_peak in fp32).
 *   mask uint8 [nclips][mask_bs >= cap - 3] or NULL: 1 for every block that passed both gates.
 * mmx_scale_rows: out[b][j] = x[b][j] * gain[b / nch] for j < lens[b]; nothing else is written; out may be x. */
#define MMX_LOUD_PAD 0
#define MMX_LOUD_DROP 1
#define MMX_LOUD_MAX_CH 5
int mmx_kweight_blocks(const float* wave, int64_t w_bs, int L, int B, const int32_t* lens, int rate, int partial, const double* tab,
                       int seg, double* work, int cap, double* energy, int64_t e_bs, float* peak, hipStream_t stream);
int mmx_loudness_gate(const double* energy, int64_t e_bs, int cap, const float* peak, const int32_t* lens, int L, int nclips, int nch,
                      const double* G, int rate, int partial, float* lufs, int want_gain, float target_db, float max_peak, float* gain,
                      uint8_t* mask, int64_t mask_bs, hipStream_t stream);
int mmx_scale_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const float* gain, int nch, float* out,
                   int64_t o_bs, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Audio distances (csrc/metrics.hip; the definitions are stated in mmx/metrics.py): what the reference's DAC-VAE validation step
 * reports (dac-vae/train.py:706-709 through dac-vae/loss.py MultiScaleSTFTLoss, MelSpectrogramLoss, L1Loss, SISDRLoss) and what its
 * latent extractor writes per decoded sample (extract_dac_latents.py:89-95), between an estimate x and a reference y: two ragged
 * batches of mono rows of equal per-clip length, without a host sync.
 *   x, y  fp32 [B][x_bs / y_bs >= L];  lens int32 [B] or NULL (= L): valid samples per clip, the same for x and y; samples at or
 *         beyond lens[b] are never read.
 *
 * mmx_spec_dist: ONE scale of the spectral distance, the arithmetic of AudioSignal.stft / mel_spectrogram
 * (audiotools/core/audio_signal.py:1185-1212, 1354-1369): torch.stft(center=True) - reflection by n_fft / 2 on each side, done as
 * index arithmetic on the row - with a periodic Hann window of n_fft samples, hop = n_fft / 4, frames(len) = 1 + len / hop frames,
 * magnitude sqrt(re^2 + im^2) of all n_fft / 2 + 1 bins, and with n_mels > 0 the mel projection of the magnitudes.
 *   h_lens: the values of lens in HOST memory (given exactly when lens is), so that the call can refuse a clip before a launch.
 *   basis bf16 [3][2 * nbp][n_fft], nbp = n_fft / 2 + 1 rounded up to 32: three planes hi + mid + lo of the float64 values
 *         hann[k] * cos(2 pi i k / n_fft) (row 32 * (i / 16) + i % 16) and hann[k] * sin(..) (that row + 16), rows of bins
 *         > n_fft / 2 zero, each plane in mmx_pack_skinny order (mmx_logmel's layout with bin0 = 0 and every bin);
 *   filt  bf16 [3][mp][nbp], mp = n_mels rounded up to 16: three planes of the fp32 filterbank [n_mels][n_fft / 2 + 1] (zero
 *         padded), each plane in mmx_pack_skinny order; NULL exactly when n_mels == 0 (STFT mode: the bins themselves).
 *   Both products run on the bf16 MFMA with samples and magnitudes split into three bf16 terms and every term pair s + p < 3
 *   kept, fp32 accumulation (mmx_logmel's arithmetic).  With a, b the values of x and y at one (frame, column), column = bin or mel:
 *   out   f64 [B][2]:  out[b][0] = mean |log10(max(a, eps)^pow) - log10(max(b, eps)^pow)|,   out[b][1] = mean |a - b|,
 *         both over the clip's own frames(lens[b]) frames x the true n_fft / 2 + 1 bins (or n_mels mels).  Every term from the
 *         subtraction on is fp64 and summed in a fixed order: per 16-frame tile into work, then per clip by the finishing launch.
 *   work  f64 [B][cap][2], cap >= ceil(frames(L) / 16): scratch.
 *   A workgroup takes 16 frames of one clip through both signals; no spectrogram is written.  A clip's two numbers depend on its
 *   own samples and length alone: solo and batched runs agree bit for bit, and x == y gives exactly 0.
 * MMX_EARG, before anything is launched: n_fft < 32 or not a multiple of 32; a clip (or L) with at most n_fft / 2 samples (the
 *   reflection is undefined; torch raises there too) or more than L; n_mels > 384; eps <= 0; tables that do not fit 160 KB of LDS
 *   (n_fft 2048 fits in both modes, 4096 in neither).
 *
 * mmx_wave_sums: one pass over the same pair ->
 *   out   f64 [B][7] = sum x, sum y, sum x^2, sum y^2, sum x y, sum |x - y|, sum (x - y)^2 over the clip's lens[b] samples, in fp64
 *         (4096 samples per workgroup in a fixed tree, then per clip in workgroup order by the finishing launch);
 *   clip  > 0: x is first limited to [-clip, clip] (the extractor clips its reconstruction to +-1); 0: x as it is;
 *   work  f64 [B][cap][7], cap >= ceil(L / 4096): scratch.
 *   L1, MSE, SNR and SI-SDR follow from the seven sums (mmx/metrics.py, on the device). */
int mmx_spec_dist(const float* x, int64_t x_bs, const float* y, int64_t y_bs, int L, int B, const int32_t* lens, const int32_t* h_lens,
                  const void* basis, const void* filt, int n_fft, int n_mels, double eps, double pow, double* work, int cap,
                  double* out, hipStream_t stream);
int mmx_wave_sums(const float* x, int64_t x_bs, const float* y, int64_t y_bs, int L, int B, const int32_t* lens, float clip, double* work,
                  int cap, double* out, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Spectral-gate noise reduction (csrc/denoise.hip; the definitions are stated in mmx/denoise.py): the reference's SpectralGate
 * (dac-vae/audiotools/ml/layers/spectral_gate.py, wrapped by transforms.NoiseReduce) on a ragged batch of mono rows, without a host
 * sync, and with it an inverse STFT.  One scale n_fft (a multiple of 32, 32 .. 2048), hop = n_fft / 4, torch.stft(center=True) /
 * torch.istft(center=True, length=len) with the square root of the periodic Hann window, frames(len) = 1 + len / hop,
 * bins = n_fft / 2 + 1, nbp = bins rounded up to 32.
 *   x      fp32 [B][x_bs >= L];  lens int32 [B] or NULL (= L), h_lens the same values in HOST memory (given exactly when lens is);
 *          samples at or beyond lens[b] are never read.
 *   basis  bf16 [3][2 * nbp][n_fft]: mmx_spec_dist's table with the sqrt-Hann window in place of the Hann window.
 *
 * mmx_gate_threshold: noise clips x -> thresh fp32 [B][t_bs >= bins]: per bin, mean + n_std * std (unbiased) over the clip's own
 *   frames of dB = 20 log10 max(|N|, 1e-4).  dB, its sums and the finish are fp64 in a fixed order (per 32-frame tile into work, then
 *   per clip in tile order); no atomics.   work f64 [B][cap][nbp][2], cap >= ceil(frames(L) / 32): scratch.
 * mmx_gate_analyze: clips x and their thresholds (row b at thresh + b * t_bs; t_bs = 0 shares one row) ->
 *   spec   fp32 [B][frames_cap][2 * nbp]: per frame the real parts of the nbp bins, then the imaginary parts (padded bins 0);
 *   mask   uint8 [B][frames_cap][nbp]: 1 where 20 log10 max(|X|, 1e-4) < thresh (strict, fp64 comparison of the fp32 magnitude), 0 at
 *          padded bins and at frames at or past frames(lens[b]); every byte is written.   frames_cap >= frames(L).
 * mmx_gate_synthesize: spec and mask as written above -> out fp32 [B][o_bs >= L]:
 *   gain = 1 - amount[b] * smooth(mask), smooth = conv2d with the normalised outer product of the triangles of 2 n_freq + 1 taps over
 *   bins and 2 n_time + 1 taps over frames (n_freq, n_time <= 14), zero padded at the edges of the clip's OWN [bins, frames(lens[b])]
 *   grid, evaluated exactly as an integer sum over (n_freq + 1)^2 (n_time + 1)^2;  spec * gain is inverted per frame as a product
 *   against inv, multiplied by the window, overlap-added as a gather (each sample adds its <= 4 frames in ascending order; no
 *   atomics), divided by the overlap-added window^2 and cropped by n_fft / 2.  Samples at or past lens[b] are written as 0.
 *   inv    bf16 [3][n_fft][2 * nbp]: the inverse DFT as three planes, each in mmx_pack_skinny order: c_k cos(2 pi k s / n) / n at
 *          [s][k] and -c_k sin(2 pi k s / n) / n at [s][nbp + k], c_k = 1 for k = 0 and n / 2 (whose imaginary entries are 0), 2
 *          between, 0 at padded bins;
 *   window fp32 [n_fft]: the synthesis window;   amount fp32 [B] on the device;
 *   frames fp32 [B][frames_cap][n_fft]: scratch (the windowed frames).
 *   The products run on the bf16 MFMA with both operands as three bf16 terms, fp32 accumulation; a workgroup takes 32 frames, whose
 *   2 * nbp gated columns pass through the same LDS in chunks of at most 544, one after the other; a chunk's product starts from
 *   zero in registers and is added, in chunk order, to what the earlier chunks left in `frames`, which is thus the accumulator
 *   across chunks (each element read and written by the one thread that owns it), and the last chunk applies the window.
 * A clip's threshold, mask and output depend on its own samples, length and arguments alone: solo and batched runs agree bit for bit.
 * MMX_EARG, before anything is launched: n_fft < 32, > 2048 or not a multiple of 32; a clip (or L) with at most n_fft / 2 samples or
 *   more than L; a capacity or stride below the stated one; n_freq or n_time outside [0, 14]. */
int mmx_gate_threshold(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const void* basis,
                       int n_fft, double n_std, double* work, int cap, float* thresh, int64_t t_bs, hipStream_t stream);
int mmx_gate_analyze(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const void* basis, int n_fft,
                     const float* thresh, int64_t t_bs, float* spec, uint8_t* mask, int frames_cap, hipStream_t stream);
int mmx_gate_synthesize(const float* spec, const uint8_t* mask, int frames_cap, int L, int B, const int32_t* lens, const int32_t* h_lens,
                        const void* inv, const float* window, int n_fft, int n_freq, int n_time, const float* amount, float* frames,
                        float* out, int64_t o_bs, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Intelligibility (csrc/stoi.hip; the definition is stated in mmx/stoi.py): STOI and extended STOI between a reference and an
 * estimate at 10 kHz, what the reference's audiotools.metrics.quality.stoi asks a host library for, on a ragged batch of mono rows
 * of equal per-clip length, without a host sync and without atomics.  Frames of 256 samples at hop 128 that start strictly below
 * len - 256: frames(len) = ceil((len - 256) / 128); a 512-point DFT of the windowed frame; 15 third-octave bands; segments of 30 frames.
 *   est, ref fp32 [B][e_bs / r_bs >= L];  lens int32 [B] or NULL (= L), h_lens the same values in HOST memory (given exactly when
 *            lens is); samples at or beyond lens[b] are never read.
 *   window   fp32 [256]: numpy.hanning(258)[1:-1];   cap >= frames(L): the row count of every per-frame buffer below.
 *
 * mmx_stoi_select: the silent-frame decision, on the reference alone ->
 *   energy f64 [B][cap]: 20 log10(|window * frame| + 2^-52) of the clip's frames(lens[b]) frames (fp32 products, fp64 sum in a fixed
 *          order); entries past them are not written;
 *   mask   uint8 [B][cap]: 1 where max(energy) - 40 - energy < 0, 0 elsewhere (every byte is written);
 *   map    int32 [B][cap]: the source frame of kept frame i for i < F, in order (the exclusive scan of mask), -1 from F on;
 *   kept   int32 [B]: F.
 * mmx_stoi_bands: both signals rebuilt from their kept frames (each sample the sum of at most two windowed source samples found
 *   through map: the overlap-add at hop 128 as a gather, never stored), the (F + 1) * 128 samples framed again into F - 1 frames,
 *   their spectra on the bf16 MFMA (samples and |X|^2 as three bf16 terms, fp32 accumulation: mmx_spec_dist's arithmetic), ->
 *   env    fp32 [B][2][cap][16]: sqrt of the band sums of |X|^2 per frame, signal 0 the reference, 1 the estimate, column 15 zero;
 *          rows at and past F - 1 are not written.  F and map are read from device memory; no spectrogram is stored.
 *   basis  bf16 [3][2 * 288][256]: mmx_spec_dist's table of n_fft = 512 with `window` followed by 256 zeros in place of the Hann
 *          window, cut to its 256 non-zero columns;   filt bf16 [3][16][288]: the 0 / 1 band table, both in mmx_pack_skinny order.
 * mmx_stoi_score: env and kept as written above -> out f64 [B]: the mean over the J = F - 30 segments (frames m - 30 .. m - 1 for
 *   m = 30 .. F - 1) and the 15 bands of the correlation of the mean-removed, normalised segment of the reference with that of the
 *   estimate scaled to the reference's norm and limited to (1 + 10^(15/20)) times the reference (extended = 0), or of the segments
 *   normalised over rows, then over columns, summed and divided by 30 J (extended = 1); 1e-5 where F - 1 < 30.
 *   frames int32 [B]: F - 1.   work f64 [B][wcap], wcap >= max(1, ceil((cap - 30) / 16)): scratch.
 *   Every term is fp64, summed in a fixed order: per 16 segments into work, then per clip by the finishing launch.
 * A clip's numbers depend on its own samples and length alone: solo and batched runs agree bit for bit.
 * MMX_EARG, before anything is launched: a clip (or L) with at most 256 samples or more than L; lens without h_lens; a capacity or
 *   stride below the stated one; extended outside {0, 1}. */
int mmx_stoi_select(const float* ref, int64_t r_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const float* window,
                    double* energy, uint8_t* mask, int32_t* map, int32_t* kept, int cap, hipStream_t stream);
int mmx_stoi_bands(const float* est, int64_t e_bs, const float* ref, int64_t r_bs, int L, int B, const int32_t* lens,
                   const int32_t* h_lens, const float* window, const int32_t* map, const int32_t* kept, const void* basis,
                   const void* filt, float* env, int cap, hipStream_t stream);
int mmx_stoi_score(const float* env, int cap, int B, const int32_t* kept, int extended, double* work, int wcap, double* out,
                   int32_t* frames, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Room and noise simulation (csrc/degrade.hip; the definitions are stated in mmx/degrade.py): the reference's EffectMixin.convolve,
 * apply_ir, alter_drr, measure_drr and mix (dac-vae/audiotools/core/effects.py:27-179, 540-647) on a ragged batch of mono fp32 rows,
 * without a host sync.  Every `lens` array (int32 [B] in device memory, or NULL = the full width) comes with the same values in HOST
 * memory (h_*; given exactly when the device array is); lengths lie in [1, width].
 *
 * mmx_ir_prepare: one impulse response per clip (ir fp32 [B][ir_bs >= Lir], or ir_bs = 0: one row shared by all), ir_lens / Lir its
 *   lengths, sig_lens / Lsig the lengths of the clips it will be applied to ->
 *   h_out fp32 [B][h_bs >= Lir]: the IR after alter_drr(drr[b]) (effects.py:617-647: early window of t0 = int(rate * 0.0025) samples
 *         either side of the signed argmax, fp64 sums, the larger root, alpha floored at max|late| / max|early|, then
 *         ensure_max_of_audio(1)); a NaN target, or drr = NULL, copies the IR.  A negative discriminant leaves NaNs, as the
 *         reference does.  Columns from ir_lens[b] to Lir are zero.  h_out may not alias ir.
 *   hann  f64 [2 t0 + 1][2 t0 + 1] (device): row c - 1 holds the periodic Hann window of c points.
 *   taps  int32 [B]: L' = min(ir_lens[b], sig_lens[b]) (effects.py:85-90);  p int32 [B]: the first index of max |h_out[0 .. L')| when
 *         start_at_max, else 0;  s fp32 [B]: 1 / max(max |h_out[0 .. L')|, 1e-5);  drr_out fp32 [B]: measure_drr of h_out,
 *         10 log10(sum early^2 / sum late^2);
 *   table bf16 [B][3][kcap / 32][64][8]: B[u][j] = g[u - j], g[v] = h_out[L' - 1 - v] (zero outside [0, L')), as three bf16 terms
 *         in mmx_pack_skinny order; kcap a multiple of 32, at least max_b L' + 15 rounded up to 32.
 * mmx_fir_rows: out[b][n] = s[b] * sum_{t < L'} h[t] X(n + p[b] - t) for n < lens[b], X(i) = x[b][i mod lens[b]] (wrap = 1) or x[b][i]
 *   inside the clip and 0 outside (wrap = 0); zeros from lens[b] to L.  A six-term bf16 MFMA product (fp32 accumulation, K ascending)
 *   of the clip's frames at hop 16 against `table`.  peak fp32 [B]: max |out[b]| (zeroed here, then an atomic max on the bit pattern).
 *   An output's bits depend on its clip, its prepared IR and its position alone.  out may not alias x.
 * mmx_row_absmax: peak fp32 [B] = max |x[b][0 .. lens[b])|, zeroed here.
 * mmx_mix_rows: out[b][j] = x[b][j] + exp(((lx[b] - snr[b]) - ln[b]) ln 10 / 20) * noise[b][j] for j < lens[b] (noise reads as zero
 *   from nlens[b] on), zeros from lens[b] to L;  lx, ln, snr fp32 [B] in device memory.
 * MMX_EARG, before anything is launched or written: more than 65536 taps (max_b L'), a length outside [1, width], lens without h_lens,
 *   a stride or capacity below the stated one, wrap outside {0, 1}. */
int mmx_ir_prepare(const float* ir, int64_t ir_bs, int Lir, int B, const int32_t* ir_lens, const int32_t* h_ir_lens, int Lsig,
                   const int32_t* sig_lens, const int32_t* h_sig_lens, const float* drr, int t0, const double* hann, int start_at_max,
                   float* h_out, int64_t h_bs, int32_t* p, float* s, int32_t* taps, float* drr_out, void* table, int kcap,
                   hipStream_t stream);
int mmx_fir_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const void* table, int kcap,
                 const int32_t* p, const float* s, const int32_t* taps, int wrap, float* out, int64_t o_bs, float* peak,
                 hipStream_t stream);
int mmx_row_absmax(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, float* peak, hipStream_t stream);
int mmx_mix_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const float* noise, int64_t n_bs, int Ln,
                 const int32_t* nlens, const float* lx, const float* ln, const float* snr, float* out, int64_t o_bs, hipStream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Channel degradations (csrc/channel.hip; the definitions are stated in mmx/channel.py): what the reference's low_pass / high_pass
 * (dac-vae/audiotools/core/dsp.py:153-215) and mel_filterbank / equalizer / clip_distortion / quantization / mulaw_quantization
 * (core/effects.py:386-523) need beside mmx_ir_prepare / mmx_fir_rows, on a ragged batch of mono fp32 rows, without a host sync.
 * lens / h_lens as above: int32 [B] in device memory with the same values in host memory, or both NULL; lengths lie in [1, L].
 *
 * mmx_pad_edge_rows: out[b][i] = x[b][clamp(i - half, 0, lens[b] - 1)] for i < lens[b] + 2 half (replicate padding; half may exceed
 *   the clip), zeros from there to L + 2 half; out fp32 [B][o_bs >= L + 2 half], not x.  Output n of a filter of 2 half + 1 taps with
 *   replicate padding is sample n + 2 half of mmx_fir_rows (wrap = 0, p = 0) over these rows.
 * mmx_row_select: out fp32 [B][R] = the order statistics ranks[b][r] (0 = the smallest; int32 [B][R] in device memory, h_ranks the
 *   same values in host memory; R <= 4) of x[b][0 .. lens[b]), exact: a radix select over the order-preserving integer image of the
 *   bits in four counting launches of 8 bits and a finishing launch, whatever the data; -0 counts as +0 and comes back as +0.
 *   nanflag int32 [B]: 1 where the row holds a NaN (its out values are NaN then), else 0.
 *   work int32 [B][R][1032]: scratch (four histograms of 256 bins, the chosen prefixes), zeroed here.  Integer atomics only.
 * mmx_clip_rows: stats fp32 [B][4] = (v[lo], v[hi]) of the lower and of the upper quantile, w f64 [B][2] the interpolation weights
 *   (device memory) -> thr fp32 [B][2] = v[lo] + (v[hi] - v[lo]) w in fp64, rounded once;
 *   out[b][j] = min(max(x[b][j], thr[b][0]), thr[b][1]) for j < lens[b], zeros from lens[b] to L.  Where nanflag[b] is set, thr and the
 *   row's samples are NaN.  out may be x.
 * mmx_quantize_rows: q int32 [B] channels per row (device; h_q the same values in host memory, each >= 2), mode 0:
 *   2 floor((x + 1) / 2 q) / q - 1; mode 1 (mu-law, mu = q - 1): c = trunc((sign(x) log1p(mu |x|) / log1p(mu) + 1) / 2 mu + 0.5),
 *   z = c / mu * 2 - 1, sign(z) (exp(|z| log1p(mu)) - 1) / mu.  fp64 per sample, rounded once; zeros from lens[b] to L.  out may be x.
 * MMX_EARG, before anything is launched or written: a length outside [1, L], lens without h_lens, a stride below the stated one,
 *   half < 0, a rank outside [0, lens[b]), R outside [1, 4], q < 2, a mode outside {0, 1}. */
int mmx_pad_edge_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, int half, float* out,
                      int64_t o_bs, hipStream_t stream);
int mmx_row_select(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const int32_t* ranks,
                   const int32_t* h_ranks, int R, float* out, int32_t* nanflag, int32_t* work, hipStream_t stream);
int mmx_clip_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const float* stats,
                  const double* w, const int32_t* nanflag, float* thr, float* out, int64_t o_bs, hipStream_t stream);
int mmx_quantize_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, int mode, const int32_t* q,
                      const int32_t* h_q, float* out, int64_t o_bs, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
