// The S3 speech tokenizer's own kernels (speech/tools/S3Tokenizer/s3tokenizer: utils.py:220-267, model_v2.py:51-70,83-112,
// 177-189) for gfx950; everything else of the tokenizer runs on mmx_gemm_win / mmx_rownorm / the attention entry points.
//   mmx_logmel_w      16 kHz clip -> Whisper-convention log-mel: csrc/mel.hip's design (samples as three bf16 planes in LDS, the
//                     windowed DFT and the mel projection as six-term bf16 MFMA products against three-plane float64 tables)
//                     with center=True reflection by n_fft / 2, the power spectrum, log10, and a finishing launch for the
//                     clip maximum: floor at max - 8, (v + 4) / 4
//   mmx_s3_rope_fsmn  rotate-half RoPE on q and k in place and r = x + (depthwise31(v m) + v m) m in one launch, one wave per head
//   mmx_fsq_encode    project_down -> tanh -> * 0.999 -> round half to even -> base-3 index, one wave per row
// One fp32 arithmetic for every build; every sum runs in a fixed order that depends on neither the tiling nor the batch.
#include "common.h"
#include "../../include/mmx_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------ log-mel
constexpr int LW_WAVES = 8;
constexpr float LW_LOG_CLIP = -10.f;                    // log10(max(v, 1e-10)) of every v <= 1e-10

struct Bf3 { bf16_t h, m, l; };
__device__ __forceinline__ Bf3 split3(float v) {        // the remainders are exact in fp32
    Bf3 o;
    o.h = f2bf(v);
    v -= bf2f(o.h);
    o.m = f2bf(v);
    v -= bf2f(o.m);
    o.l = f2bf(v);
    return o;
}

__device__ __forceinline__ short8_t ld8(const bf16_t* p) { return *reinterpret_cast<const short8_t*>(p); }

// six bf16 MFMAs = every term (a plane s) x (b plane p) with s + p < 3, smallest terms first
__device__ __forceinline__ float4_t mfma6(const short8_t (&a)[3], const short8_t (&b)[3], float4_t c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], c, 0, 0, 0);
    return c;
}

// basis: [3 planes][2 * nbp / 16 tiles][kp / 32][64][8], kp = n_fft rounded up to 32 (zero columns beyond n_fft);
//        tile 2j = window * cos of bins 16j .. 16j + 15, tile 2j + 1 = window * sin
// filt : [3 planes][mp / 16 tiles][nbp / 32][64][8]
// Writes log10(max(mel power, 1e-10)) for frames t < len / hop and 0 for the others; logmel_w_finish does the rest.
template <typename TO>
__global__ __launch_bounds__(LW_WAVES * 64) void logmel_w_kernel(const float* __restrict__ wave, long w_bs, int L,
                                                                 const int* __restrict__ lens, const bf16_t* __restrict__ basis,
                                                                 const bf16_t* __restrict__ filt, int n_fft, int kp, int hop, int nbp,
                                                                 int n_mels, int mp, float* __restrict__ out_cm, long ldo,
                                                                 TO* __restrict__ out_tm, int T) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = 15 * hop + kp;                        // samples under 16 frames plus the zero-weighted K padding (a multiple of 8)
    const int MS = nbp + 8;                             // power row stride: 16-byte aligned rows, 4 banks apart
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);       // [3][S]
    bf16_t* mg = xs + 3 * S;                            // [3][16][MS]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * 16;
    const int pad = n_fft / 2;
    const int len = lens ? min(lens[b], L) : L;
    const int Tb = len > pad ? len / hop : 0;
    const int mtiles = mp / 16;

    if (t0 >= Tb) {                                     // a tile of padding frames (uniform over the workgroup): zeros
        for (int i = tid; i < 16 * n_mels; i += LW_WAVES * 64) {
            const int t = t0 + i / n_mels, mel = i % n_mels;
            if (t < T) {
                if (out_cm) out_cm[((long)b * n_mels + mel) * ldo + t] = 0.f;
                if (out_tm) out_tm[((long)b * T + t) * n_mels + mel] = Cvt<TO>::from_f(0.f);
            }
        }
        return;
    }

    // ---- stage 0: samples -> planes (the K padding multiplies zero basis columns: it only has to be finite)
    const float* x = wave + (long)b * w_bs;
    for (int q = tid; q < S; q += LW_WAVES * 64) {
        long i = (long)t0 * hop + q - pad;
        if (i < 0) i = -i;
        if (i >= len) i = 2L * (len - 1) - i;
        // beyond one reflection: only frames >= Tb reach there, and those are written as zeros
        const float v = (q < 15 * hop + n_fft && i >= 0 && i < len) ? x[i] : 0.f;
        const Bf3 s = split3(v);
        xs[q] = s.h;
        xs[S + q] = s.m;
        xs[2 * S + q] = s.l;
    }
    __syncthreads();

    // ---- stage 1: DFT tiles -> power planes
    const int nkt = kp / 32;
    const long PB = (long)2 * nbp * kp;                 // elements per basis plane
    const bf16_t* xa = xs + l16 * hop + g * 8;
    for (int j = wv; j < nbp / 16; j += LW_WAVES) {
        float4_t re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
        const bf16_t* wc = basis + (long)(2 * j) * nkt * 512 + lane * 8;
        const bf16_t* ws = wc + (long)nkt * 512;
#pragma unroll 2
        for (int kt = 0; kt < nkt; ++kt) {
            short8_t a[3], c[3], s[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                a[p] = ld8(xa + p * S + kt * 32);
                c[p] = ld8(wc + p * PB + (long)kt * 512);
                s[p] = ld8(ws + p * PB + (long)kt * 512);
            }
            re = mfma6(a, c, re);
            im = mfma6(a, s, im);
        }
        // C layout: lane (g, l16) holds frames 4g .. 4g + 3 of bin 16j + l16
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const Bf3 m3 = split3(re[r] * re[r] + im[r] * im[r]);
            bf16_t* d = mg + (4 * g + r) * MS + j * 16 + l16;
            d[0] = m3.h;
            d[16 * MS] = m3.m;
            d[32 * MS] = m3.l;
        }
    }
    __syncthreads();

    // ---- stage 2: mel projection, log10, both layouts
    const int nk2 = nbp / 32;
    const long PF = (long)mp * nbp;
    const bf16_t* ma = mg + l16 * MS + g * 8;
    for (int mt = wv; mt < mtiles; mt += LW_WAVES) {
        float4_t acc = {0.f, 0.f, 0.f, 0.f};
        const bf16_t* wf = filt + (long)mt * nk2 * 512 + lane * 8;
#pragma unroll 2
        for (int kt = 0; kt < nk2; ++kt) {
            short8_t a[3], f[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                a[p] = ld8(ma + p * 16 * MS + kt * 32);
                f[p] = ld8(wf + p * PF + (long)kt * 512);
            }
            acc = mfma6(a, f, acc);
        }
        const int mel = mt * 16 + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = t0 + 4 * g + r;
            if (mel < n_mels && t < T) {
                const float v = acc[r];
                const float o = t < Tb ? (v > 1e-10f ? log10f(v) : LW_LOG_CLIP) : 0.f;
                if (out_cm) out_cm[((long)b * n_mels + mel) * ldo + t] = o;
                if (out_tm) out_tm[((long)b * T + t) * n_mels + mel] = Cvt<TO>::from_f(o);
            }
        }
    }
}

// One workgroup per clip: the maximum over the clip's valid frames (a maximum has no order), then
// v = (max(v, mx - 8) + 4) / 4 on those frames.  The fp32 log10 values are read from out_cm when it is given, else from out_tm
// (fp32 there: the entry point refuses a bf16 out_tm without out_cm).
constexpr int LF_THREADS = 1024;
template <typename TO>
__global__ __launch_bounds__(LF_THREADS) void logmel_w_finish(const int* __restrict__ lens, int L, int n_fft, int hop, int n_mels,
                                                              float* __restrict__ out_cm, long ldo, TO* __restrict__ out_tm, int T) {
    __shared__ float red[LF_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = lens ? min(lens[b], L) : L;
    const int Tb = min(len > n_fft / 2 ? len / hop : 0, T);
    const long n = (long)Tb * n_mels;
    if (n == 0) return;
    float* cm = out_cm ? out_cm + (long)b * n_mels * ldo : nullptr;
    TO* tm = out_tm ? out_tm + (long)b * T * n_mels : nullptr;
    float mx = -INFINITY;
    if (cm) {
        for (long i = tid; i < n; i += LF_THREADS) mx = fmaxf(mx, cm[(i / Tb) * ldo + i % Tb]);
    } else {
        for (long i = tid; i < n; i += LF_THREADS) mx = fmaxf(mx, Cvt<TO>::to_f(tm[i]));
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int w = 1; w < LF_THREADS / 64; ++w) mx = fmaxf(mx, red[w]);
    const float flo = mx - 8.0f;
    if (cm) {
        for (long i = tid; i < n; i += LF_THREADS) {
            const long mel = i / Tb, t = i % Tb;
            const float v = (fmaxf(cm[mel * ldo + t], flo) + 4.0f) / 4.0f;
            cm[mel * ldo + t] = v;
            if (tm) tm[t * n_mels + mel] = Cvt<TO>::from_f(v);
        }
    } else {
        for (long i = tid; i < n; i += LF_THREADS) tm[i] = Cvt<TO>::from_f((fmaxf(Cvt<TO>::to_f(tm[i]), flo) + 4.0f) / 4.0f);
    }
}

// ------------------------------------------------------------------------------------------------ RoPE + FSMN memory
constexpr int RF_TT = 32;                               // output rows per wave
constexpr int RF_TAPS = 31, RF_HALF = 15;

// grid (time tiles, heads, batch), one wave: lane = channel of the head.  q / k are rotated in place (lane d and lane d ^ 32
// of the same wave hold the pair, both read before either writes).
__global__ __launch_bounds__(64) void s3_rope_fsmn_kernel(float* __restrict__ qkv, long ldqkv, long qkv_bs, int C,
                                                          const float* __restrict__ x, long x_bs, float* __restrict__ r, long r_bs,
                                                          const float* __restrict__ wt, const float* __restrict__ cs,
                                                          const float* __restrict__ sn, const int* __restrict__ lens, int T) {
    __shared__ float vs[(RF_TT + RF_TAPS - 1) * 64];
    const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z, t0 = blockIdx.x * RF_TT;
    const int c = h * 64 + lane;
    const int len = lens ? min(lens[b], T) : T;
    float* row0 = qkv + (long)b * qkv_bs;
    // v m of rows t0 - 15 .. t0 + TT + 14: zero outside [0, len)
    for (int i = 0; i < RF_TT + RF_TAPS - 1; ++i) {
        const int t = t0 - RF_HALF + i;
        vs[i * 64 + lane] = (t >= 0 && t < len) ? row0[(long)t * ldqkv + 2 * C + c] : 0.f;
    }
    float w[RF_TAPS];
#pragma unroll
    for (int j = 0; j < RF_TAPS; ++j) w[j] = wt[(long)j * C + c];
    __syncthreads();
    const int d = lane & 31;
    const int tend = min(t0 + RF_TT, T);
    for (int t = t0; t < tend; ++t) {
        float* qr = row0 + (long)t * ldqkv + c;
        const float xr = x[(long)b * x_bs + (long)t * C + c];
        float* rr = r + (long)b * r_bs + (long)t * C + c;
        if (t >= len) {                                 // padding row (uniform over the wave)
            *rr = xr;
            qr[0] = 0.f;
            qr[C] = 0.f;
            continue;
        }
        const float* vw = vs + (t - t0) * 64 + lane;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < RF_TAPS; ++j) acc = __builtin_fmaf(w[j], vw[j * 64], acc);
        *rr = xr + (acc + vw[RF_HALF * 64]);
        const float co = cs[t * 32 + d], si = sn[t * 32 + d];
        const float q = qr[0], k = qr[C];
        const float qp = __shfl_xor(q, 32, 64), kp = __shfl_xor(k, 32, 64);
        const float qrot = lane < 32 ? -qp : qp, krot = lane < 32 ? -kp : kp;
        qr[0] = __fadd_rn(__fmul_rn(q, co), __fmul_rn(qrot, si));     // xq * cos + xq_r * sin, unfused as torch evaluates it
        qr[C] = __fadd_rn(__fmul_rn(k, co), __fmul_rn(krot, si));
    }
}

// ------------------------------------------------------------------------------------------------ FSQ head
constexpr int FQ_ROWS = 4;                              // rows (waves) per workgroup
constexpr float FQ_SCALE = 0.9990000128746033f;

__global__ __launch_bounds__(FQ_ROWS * 64) void fsq_encode_kernel(const float* __restrict__ x, long ldx, long x_bs, int T, int C, int B,
                                                                  const float* __restrict__ W, const float* __restrict__ bias,
                                                                  const int* __restrict__ lens, int* __restrict__ ids, long ld_ids,
                                                                  float* __restrict__ pre) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * FQ_ROWS + (threadIdx.x >> 6);
    if (row >= (long)B * T) return;                     // uniform over the wave
    const int b = (int)(row / T), t = (int)(row % T);
    const int len = lens ? min(lens[b], T) : T;
    int* idp = ids + (long)b * ld_ids + t;
    float* pp = pre ? pre + row * 8 : nullptr;
    if (t >= len) {
        if (lane == 0) *idp = 0;
        if (pp && lane < 8) pp[lane] = 0.f;
        return;
    }
    const float* xr = x + (long)b * x_bs + (long)t * ldx;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < C; c += 64) {
        const float xv = xr[c];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(xv, W[(long)i * C + c], acc[i]);
    }
    int id = 0, p3 = 1;
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float v = tanhf(wave_sum(acc[i]) + bias[i]) * FQ_SCALE;
        id += ((int)rintf(v) + 1) * p3;
        p3 *= 3;
        if (lane == i) mine = v;
    }
    if (lane == 0) *idp = id;
    if (pp && lane < 8) pp[lane] = mine;
}

}  // namespace

extern "C" int mmx_logmel_w(const float* wave, int64_t w_bs, int L, int B, const int32_t* lens, const int32_t* h_lens,
                            const void* basis, const void* filt, int n_fft, int hop, int bin0, int n_bins, int n_mels,
                            float* out_cm, int64_t ldo, void* out_tm, int T, int dtype, hipStream_t stream) {
    MMX_CHECK_ARG(wave && basis && filt && (out_cm || out_tm) && B > 0 && B <= 65535 && T > 0 && L > 0);
    MMX_CHECK_ARG(n_fft > 0 && n_fft % 16 == 0 && n_mels > 0 && n_mels <= 128);
    MMX_CHECK_ARG(hop > 0 && hop <= n_fft && hop % 8 == 0);
    MMX_CHECK_ARG(bin0 >= 0 && n_bins > 0 && bin0 + n_bins <= n_fft / 2 + 1);
    MMX_CHECK_ARG(w_bs >= L && (!out_cm || ldo >= T) && (!lens == !h_lens));
    const int act = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(act == MMX_F32 || (act == MMX_BF16 && (out_cm || !out_tm)));   // the clip maximum is taken over fp32 values
    const int pad = n_fft / 2;
    int tmax = 0;
    for (int b = 0; b < B; ++b) {
        const int len = h_lens ? h_lens[b] : L;
        MMX_CHECK_ARG(len > pad && len <= L && len / hop > 0);       // the reflection reads sample `pad`
        tmax = max(tmax, len / hop);
    }
    MMX_CHECK_ARG(T >= tmax);                           // every frame a member has fits the outputs
    const int kp = (n_fft + 31) / 32 * 32, nbp = (n_bins + 31) / 32 * 32, mp = (n_mels + 15) / 16 * 16;
    const size_t lds = ((size_t)3 * (15 * hop + kp) + (size_t)3 * 16 * (nbp + 8)) * sizeof(bf16_t);
    MMX_CHECK_ARG(lds <= 160 * 1024);
    const dim3 grid((T + 15) / 16, B), block(LW_WAVES * 64);
    if (act == MMX_BF16) {
        MMX_LDS_OPT_IN(logmel_w_kernel<bf16_t>, lds);
        hipLaunchKernelGGL(logmel_w_kernel<bf16_t>, grid, block, lds, stream, wave, (long)w_bs, L, lens, (const bf16_t*)basis,
                           (const bf16_t*)filt, n_fft, kp, hop, nbp, n_mels, mp, out_cm, (long)ldo, (bf16_t*)out_tm, T);
        MMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(logmel_w_finish<bf16_t>, dim3(B), dim3(LF_THREADS), 0, stream, lens, L, n_fft, hop, n_mels, out_cm, (long)ldo,
                           (bf16_t*)out_tm, T);
    } else {
        MMX_LDS_OPT_IN(logmel_w_kernel<float>, lds);
        hipLaunchKernelGGL(logmel_w_kernel<float>, grid, block, lds, stream, wave, (long)w_bs, L, lens, (const bf16_t*)basis,
                           (const bf16_t*)filt, n_fft, kp, hop, nbp, n_mels, mp, out_cm, (long)ldo, (float*)out_tm, T);
        MMX_LAUNCH_CHECK();
        hipLaunchKernelGGL(logmel_w_finish<float>, dim3(B), dim3(LF_THREADS), 0, stream, lens, L, n_fft, hop, n_mels, out_cm, (long)ldo,
                           (float*)out_tm, T);
    }
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_s3_rope_fsmn(float* qkv, int64_t ldqkv, int64_t qkv_bs, int B, int T, int C, const float* x, int64_t x_bs,
                                float* r, int64_t r_bs, const float* wt, const float* rope_cos, const float* rope_sin,
                                int rope_rows, const int32_t* lens, hipStream_t stream) {
    MMX_CHECK_ARG(qkv && x && r && wt && rope_cos && rope_sin && B > 0 && B <= 65535 && T > 0 && C > 0 && C % 64 == 0 && C / 64 <= 65535);
    MMX_CHECK_ARG(T <= rope_rows);                      // the position is the row index
    MMX_CHECK_ARG(ldqkv >= 3 * (int64_t)C && qkv_bs >= (int64_t)T * ldqkv && x_bs >= (int64_t)T * C && r_bs >= (int64_t)T * C);
    const dim3 grid((T + RF_TT - 1) / RF_TT, C / 64, B);
    hipLaunchKernelGGL(s3_rope_fsmn_kernel, grid, dim3(64), 0, stream, qkv, (long)ldqkv, (long)qkv_bs, C, x, (long)x_bs, r, (long)r_bs,
                       wt, rope_cos, rope_sin, lens, T);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_fsq_encode(const float* x, int64_t ldx, int64_t x_bs, int B, int T, int C, const float* W, const float* bias,
                              const int32_t* lens, int32_t* ids, int64_t ld_ids, float* pre, hipStream_t stream) {
    MMX_CHECK_ARG(x && W && bias && ids && B > 0 && T > 0 && C > 0 && ldx >= C && x_bs >= (int64_t)T * ldx && ld_ids >= T);
    const long rows = (long)B * T;
    MMX_CHECK_ARG((rows + FQ_ROWS - 1) / FQ_ROWS <= 0x7fffffffL);
    hipLaunchKernelGGL(fsq_encode_kernel, dim3((unsigned)((rows + FQ_ROWS - 1) / FQ_ROWS)), dim3(FQ_ROWS * 64), 0, stream, x, (long)ldx,
                       (long)x_bs, T, C, B, W, bias, lens, ids, (long)ld_ids, pre);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
