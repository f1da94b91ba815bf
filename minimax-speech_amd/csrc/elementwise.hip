// Row-wise and elementwise kernels of the hot path (all HBM-bound: coalesced rows, wave-shuffle
// reductions, one pass over the data).  See include/mmx_hip.h for the contracts.
#include "common.h"
#include <type_traits>

template <int V> using ic = std::integral_constant<int, V>;

// ---------------------------------------------------------------------------- rownorm
// one wave per row, the row in registers (C <= 64 * MAXV; 2048 at most: the speech tokenizer's 1280 channels take MAXV = 32).
// fp32 statistics (two-pass over registers).
template <typename T, int MAXV, int ACT>
__global__ __launch_bounds__(256) void rownorm_kernel(
    const float* __restrict__ x, long ldx, long x_bs, int rows, int C,
    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int rms, int act,
    const float* __restrict__ rowmask, long rm_bs, const float* __restrict__ addvec, long av_bs,
    float* __restrict__ outf, long ldo_f, long of_bs, T* __restrict__ outa, long ldo_a, long oa_bs) {
    constexpr bool PRECISE = sizeof(T) == 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int row = blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float* xr = x + (long)b * x_bs + (long)row * ldx;
    float v[MAXV];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = lane + i * 64;
        v[i] = c < C ? xr[c] : 0.f;
        s += v[i];
    }
    float mean = 0.f;
    if (!rms) mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = lane + i * 64;
        float d = c < C ? v[i] - mean : 0.f;
        q += d * d;
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
    const float rm = rowmask ? rowmask[(long)b * rm_bs + row] : 1.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        int c = lane + i * 64;
        if (c >= C) continue;
        float y = (v[i] - mean) * rstd * gamma[c];
        if (!rms && beta) y += beta[c];
        y = act_c<ACT, PRECISE>(y, 0.f);
        y *= rm;
        if (addvec) y = (y + addvec[(long)b * av_bs + c]) * rm;
        if (outf) outf[(long)b * of_bs + (long)row * ldo_f + c] = y;
        if (outa) outa[(long)b * oa_bs + (long)row * ldo_a + c] = Cvt<T>::from_f(y);
    }
}

extern "C" int mmx_rownorm(const float* x, int64_t ldx, int64_t x_bstride, int rows, int C, int batch,
                           const float* gamma, const float* beta, float eps, int rms, int act,
                           const float* rowmask, int64_t rm_bstride, const float* addvec, int64_t av_bstride,
                           float* out_f32, int64_t ldo_f, int64_t of_bstride,
                           void* out_act, int64_t ldo_a, int64_t oa_bstride, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(x && gamma && rows > 0 && C > 0 && C <= 2048 && batch > 0 && (out_f32 || out_act));
    dim3 grid((rows + 3) / 4, batch);
    MMX_CHECK_ARG(act == ACT_NONE || act == ACT_MISH);
    return dispatch_dtype(dtype, [&](auto el) {
        auto go = [&](auto mv, auto a) {               // MV: values a thread holds (C <= 64 * MV); A: the activation, compile time
            hipLaunchKernelGGL((rownorm_kernel<decltype(el), mv(), a()>), grid, dim3(256), 0, stream, x, ldx, x_bstride, rows, C, gamma, beta, eps, rms, act,
                               rowmask, rm_bstride, addvec, av_bstride, out_f32, ldo_f, of_bstride, (decltype(el)*)out_act, ldo_a, oa_bstride);
            return launch_status();
        };
        auto by_c = [&](auto a) { return C <= 256 ? go(ic<4>{}, a) : C <= 512 ? go(ic<8>{}, a) : C <= 1024 ? go(ic<16>{}, a) : go(ic<32>{}, a); };
        return act == ACT_MISH ? by_c(ic<ACT_MISH>{}) : by_c(ic<ACT_NONE>{});
    });
}

// ---------------------------------------------------------------------------- gather rows
template <typename T>
__global__ void gather_rows_kernel(const int64_t* __restrict__ ids, int n, const float* __restrict__ table, int C,
                                   float scale, const float* __restrict__ rowmask, float* __restrict__ outf, long ldo_f,
                                   T* __restrict__ outa, long ldo_a) {
    const int i = blockIdx.x;
    long id = ids[i];
    if (id < 0) id = 0;
    const float m = scale * (rowmask ? rowmask[i] : 1.f);
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        float v = table[id * C + c] * m;
        if (outf) outf[(long)i * ldo_f + c] = v;
        if (outa) outa[(long)i * ldo_a + c] = Cvt<T>::from_f(v);
    }
}
extern "C" int mmx_gather_rows(const int64_t* ids, int n, const float* table, int C, float scale, const float* rowmask,
                               float* out_f32, int64_t ldo_f, void* out_act, int64_t ldo_a, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(ids && table && n > 0 && C > 0 && (out_f32 || out_act));
    return dispatch_dtype(dtype, [&](auto el) {
        hipLaunchKernelGGL(gather_rows_kernel<decltype(el)>, dim3(n), dim3(256), 0, stream, ids, n, table, C, scale, rowmask, out_f32, ldo_f, (decltype(el)*)out_act, ldo_a);
        return launch_status();
    });
}

// ---------------------------------------------------------------------------- copy2d (transposing cast through LDS)
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void copy2d_kernel(const TI* __restrict__ in, long ibs, long irs, long ics, int rep,
                                                     TO* __restrict__ out, long obs, long ors, long ocs, int rows, int cols) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    in += (long)b * ibs;
    out += (long)b * obs;
    // read with the faster-varying INPUT index on tx
    const bool in_col_fast = (ics <= irs);
    for (int j = ty; j < 32; j += 8) {
        int r = in_col_fast ? r0 + j : r0 + tx;
        int c = in_col_fast ? c0 + tx : c0 + j;
        if (r < rows && c < cols) {
            float v = Cvt<TI>::to_f(in[(long)(r / rep) * irs + (long)c * ics]);
            tile[r - r0][c - c0] = v;
        }
    }
    __syncthreads();
    const bool out_col_fast = (ocs <= ors);
    for (int j = ty; j < 32; j += 8) {
        int r = out_col_fast ? r0 + j : r0 + tx;
        int c = out_col_fast ? c0 + tx : c0 + j;
        if (r < rows && c < cols) out[(long)r * ors + (long)c * ocs] = Cvt<TO>::from_f(tile[r - r0][c - c0]);
    }
}
extern "C" int mmx_copy2d(const void* in, int in_dtype, int64_t ibs, int64_t irs, int64_t ics, int rep,
                          void* out, int out_dtype, int64_t obs, int64_t ors, int64_t ocs,
                          int rows, int cols, int batch, hipStream_t stream) {
    in_dtype = MMX_ACT_DTYPE(in_dtype);
    out_dtype = MMX_ACT_DTYPE(out_dtype);
    MMX_CHECK_ARG(in && out && rows > 0 && cols > 0 && batch > 0 && rep >= 1);
    dim3 grid((cols + 31) / 32, (rows + 31) / 32, batch);
    return dispatch_dtype(in_dtype, [&](auto ti) {
        return dispatch_dtype(out_dtype, [&](auto to) {
            hipLaunchKernelGGL((copy2d_kernel<decltype(ti), decltype(to)>), grid, dim3(256), 0, stream, (const decltype(ti)*)in, ibs, irs, ics, rep,
                               (decltype(to)*)out, obs, ors, ocs, rows, cols);
            return launch_status();
        });
    });
}

// ---------------------------------------------------------------------------- estimator input pack / time embedding
template <typename T>
__global__ void est_pack_kernel(const float* __restrict__ x, long x_bs, int x_mod, const float* __restrict__ mu, const float* __restrict__ spks,
                                const float* __restrict__ cond, int Tn, int C, T* __restrict__ h, long ldh) {
    const int b = blockIdx.y;
    const long row = blockIdx.x;                   // frame
    const long o = ((long)b * Tn + row);
    for (int c = threadIdx.x; c < 4 * C; c += blockDim.x) {
        int part = c / C, cc = c % C;
        float v;
        if (part == 0) v = x[(long)(b % x_mod) * x_bs + row * C + cc];
        else if (part == 1) v = mu ? mu[o * C + cc] : 0.f;
        else if (part == 2) v = spks ? spks[(long)b * C + cc] : 0.f;
        else v = cond ? cond[o * C + cc] : 0.f;
        h[o * ldh + c] = Cvt<T>::from_f(v);
    }
}
extern "C" int mmx_est_pack(const float* x, int64_t x_bs, int x_mod, const float* mu, const float* spks, const float* cond, int B, int T_, int C,
                            void* h, int64_t ldh, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(x && h && B > 0 && T_ > 0 && C > 0 && ldh >= 4 * C && x_mod > 0);
    dim3 grid(T_, B);
    return dispatch_dtype(dtype, [&](auto el) {
        hipLaunchKernelGGL(est_pack_kernel<decltype(el)>, grid, dim3(128), 0, stream, x, x_bs, x_mod, mu, spks, cond, T_, C, (decltype(el)*)h, ldh);
        return launch_status();
    });
}

template <typename T>
__global__ void sinusoidal_kernel(const float* __restrict__ t, int dim, float scale, T* __restrict__ out) {
    const int b = blockIdx.x;
    const int half = dim / 2;
    const float k = logf(10000.f) / (float)(half - 1);
    for (int i = threadIdx.x; i < dim; i += blockDim.x) {
        int j = i < half ? i : i - half;
        float e = scale * t[b] * expf((float)j * -k);
        out[(long)b * dim + i] = Cvt<T>::from_f(i < half ? sinf(e) : cosf(e));
    }
}
extern "C" int mmx_sinusoidal_emb(const float* t, int B, int dim, float scale, void* out, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(t && out && B > 0 && dim >= 4 && dim % 2 == 0);
    return dispatch_dtype(dtype, [&](auto el) {
        hipLaunchKernelGGL(sinusoidal_kernel<decltype(el)>, dim3(B), dim3(128), 0, stream, t, dim, scale, (decltype(el)*)out);
        return launch_status();
    });
}

__global__ void cfg_euler_kernel(float* __restrict__ x, const float* __restrict__ dc, const float* __restrict__ du,
                                 float cfg, float dt, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = x[i] + dt * ((1.0f + cfg) * dc[i] - cfg * du[i]);
}
extern "C" int mmx_cfg_euler(float* x, const float* d_cond, const float* d_uncond, float cfg, float dt, int64_t n,
                             hipStream_t stream) {
    MMX_CHECK_ARG(x && d_cond && d_uncond && n > 0);
    hipLaunchKernelGGL(cfg_euler_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, d_cond, d_uncond, cfg, dt, (long)n);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

// ---------------------------------------------------------------------------- DAC tail conv (C -> 1) + LeakyReLU + tanh
// One thread per output sample; the k*C weights sit in LDS; a block's 256 consecutive samples read a
// (256 + k - 1) x C window of the activation, staged once through LDS (coalesced 16-byte rows).
template <typename T>
__global__ __launch_bounds__(256) void conv_cout1_kernel(const T* __restrict__ act, long a_bs, int Tn, int C, int k,
                                                         const float* __restrict__ w, const float* __restrict__ bias,
                                                         float slope, int use_tanh, float* __restrict__ out, long o_bs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* ws = reinterpret_cast<float*>(smem);              // [k*C]
    T* xs = reinterpret_cast<T*>(ws + k * C);                // [(256 + k - 1)][C]
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * 256;
    const int pad = (k - 1) / 2;
    const T* a = act + (long)b * a_bs;
    for (int i = threadIdx.x; i < k * C; i += 256) ws[i] = w[i];
    const int nrow = 256 + k - 1;
    for (int i = threadIdx.x; i < nrow * C; i += 256) {
        int r = i / C, c = i % C;
        long t = (long)t0 + r - pad;
        xs[i] = (t >= 0 && t < Tn) ? a[t * C + c] : Cvt<T>::from_f(0.f);
    }
    __syncthreads();
    const int t = t0 + threadIdx.x;
    if (t >= Tn) return;
    float acc = bias ? bias[0] : 0.f;
    const T* xr = xs + threadIdx.x * C;                      // window rows [tid, tid + k)
    for (int i = 0; i < k * C; ++i) acc += Cvt<T>::to_f(xr[i]) * ws[i];
    acc = acc > 0.f ? acc : acc * slope;
    out[(long)b * o_bs + t] = use_tanh ? tanhf(acc) : fminf(fmaxf(acc, -1.f), 1.f);
}
extern "C" int mmx_conv_cout1_tanh(const void* act, int64_t a_bs, int T_, int C, int k, const float* w, const float* bias,
                                   float slope, int use_tanh, float* out, int64_t o_bs, int batch, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(act && w && out && T_ > 0 && C > 0 && k > 0 && (k & 1) && batch > 0);
    dim3 grid((T_ + 255) / 256, batch);
    size_t esz = dtype == MMX_BF16 ? 2 : 4;
    size_t lds = (size_t)k * C * 4 + (size_t)(256 + k - 1) * C * esz;
    MMX_CHECK_ARG(lds <= 160 * 1024);
    // above 64 KB the launch needs the per-function opt-in, as the GEMM's larger tiles do (fp32 / split builds from C = 64 at k = 7)
    return dispatch_dtype(dtype, [&](auto el) {
        MMX_LDS_OPT_IN(conv_cout1_kernel<decltype(el)>, lds);
        hipLaunchKernelGGL(conv_cout1_kernel<decltype(el)>, grid, dim3(256), lds, stream, (const decltype(el)*)act, a_bs, T_, C, k, w, bias, slope, use_tanh, out, o_bs);
        return launch_status();
    });
}

// ---------------------------------------------------------------------------- DAC-VAE encoder head / VAE sampling
// Conv1d(1 -> C, k) + LeakyReLU: thread = (sample t, 8 channels); the k+255 input samples of a block sit in LDS.
template <typename T>
__global__ __launch_bounds__(256) void conv_cin1_kernel(const float* __restrict__ x, long x_bs, int Tn, int C, int k,
                                                        const float* __restrict__ w, const float* __restrict__ bias, float slope,
                                                        const float* __restrict__ alpha, float* __restrict__ outf, T* __restrict__ outa) {
    constexpr bool PRECISE = sizeof(T) == 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* xs = reinterpret_cast<float*>(smem);            // [TB + k - 1]
    float* ws = xs + (256 + k - 1);                        // [C][k]
    const int b = blockIdx.y, t0 = blockIdx.x * 256, pad = (k - 1) / 2;
    const float* xb = x + (long)b * x_bs;
    for (int i = threadIdx.x; i < 256 + k - 1; i += 256) {
        long t = (long)t0 + i - pad;
        xs[i] = (t >= 0 && t < Tn) ? xb[t] : 0.f;
    }
    for (int i = threadIdx.x; i < C * k; i += 256) ws[i] = w[i];
    __syncthreads();
    // 256 threads cover 256 samples x C channels in passes: thread -> (sample tid / (C/8) ..., 8 channels)
    const int cg = C / 8;                                  // channel groups of 8 per sample
    for (int item = threadIdx.x; item < 256 * cg; item += 256) {
        const int ts = item / cg, c0 = (item % cg) * 8;
        const int t = t0 + ts;
        if (t >= Tn) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = bias ? bias[c0 + e] : 0.f;
            for (int j = 0; j < k; ++j) a += ws[(c0 + e) * k + j] * xs[ts + j];
            a = a > 0.f ? a : a * slope;
            v[e] = a;
        }
        const long o = ((long)b * Tn + t) * C + c0;
        if (outf) {
#pragma unroll
            for (int e = 0; e < 8; ++e) outf[o + e] = v[e];
        }
        if (outa) {
#pragma unroll
            for (int e = 0; e < 8; ++e) outa[o + e] = Cvt<T>::from_f(alpha ? snake_apply<PRECISE>(v[e], alpha[c0 + e]) : v[e]);
        }
    }
}
extern "C" int mmx_conv_cin1(const float* x, int64_t x_bs, int T_, int C, int k, const float* w, const float* bias, float slope,
                             const float* alpha, float* out_f32, void* out_act, int batch, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(x && w && (out_f32 || out_act) && T_ > 0 && C > 0 && C % 8 == 0 && k > 0 && (k & 1) && batch > 0);
    dim3 grid((T_ + 255) / 256, batch);
    size_t lds = (size_t)(256 + k - 1 + C * k) * 4;
    return dispatch_dtype(dtype, [&](auto el) {
        hipLaunchKernelGGL(conv_cin1_kernel<decltype(el)>, grid, dim3(256), lds, stream, x, x_bs, T_, C, k, w, bias, slope, alpha, out_f32, (decltype(el)*)out_act);
        return launch_status();
    });
}

__global__ void vae_sample_kernel(const float* __restrict__ ml, const float* __restrict__ noise, long n, int D,
                                  float* __restrict__ z, float* __restrict__ m, float* __restrict__ logs) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long r = i / D;
    const int c = i % D;
    const float mu = ml[r * 2 * D + c];
    float lg = ml[r * 2 * D + D + c];
    lg = fminf(fmaxf(lg, -14.f), 14.f);
    m[i] = mu;
    logs[i] = lg;
    z[i] = mu + noise[i] * expf(lg);
}
extern "C" int mmx_vae_sample(const float* ml, const float* noise, int64_t rows, int D, float* z, float* m, float* logs,
                              hipStream_t stream) {
    MMX_CHECK_ARG(ml && noise && z && m && logs && rows > 0 && D > 0);
    const long n = rows * D;
    hipLaunchKernelGGL(vae_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, ml, noise, n, D, z, m, logs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

// ---------------------------------------------------------------------------- row mask in place
// x[row][:] = 0 where rowmask[row] == 0 (T = fp32 or bf16, 16-byte chunks): the rows beyond a member's length in a zero-padded
// batch after a ConvTranspose1d, whose GEMM rows straddle the boundary (mmx/dac.py: batched DAC decode of a flow group).
template <typename T>
__global__ void mask_rows_kernel(T* __restrict__ x, long rows, int C, const float* __restrict__ rowmask) {
    constexpr int E = 16 / sizeof(T);
    const long cpr = C / E, i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * cpr) return;
    const long r = i / cpr;
    if (rowmask[r] == 0.f) reinterpret_cast<uint4*>(x)[i] = make_uint4(0, 0, 0, 0);
}
extern "C" int mmx_mask_rows(void* x, int64_t rows, int C, const float* rowmask, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(x && rowmask && rows > 0 && C > 0 && ((uintptr_t)x % 16) == 0 && C % (dtype == MMX_BF16 ? 8 : 4) == 0);
    const long n = rows * (C / (dtype == MMX_BF16 ? 8 : 4));
    if (dtype == MMX_BF16) hipLaunchKernelGGL(mask_rows_kernel<bf16_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (bf16_t*)x, (long)rows, C, rowmask);
    else hipLaunchKernelGGL(mask_rows_kernel<float>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (float*)x, (long)rows, C, rowmask);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

// ---------------------------------------------------------------------------- masked mean over rows
// out[b][c] = sum_t x[b][t][c] * mask[b][t] / max(sum_t mask[b][t], 1)   (mask NULL: the plain mean over T rows):
// LearnableSpeakerEncoder's mean pooling (speech/cosyvoice/llm/llm.py:80-88).  A workgroup takes 64 channels of one batch member:
// 4 row groups x 64 channels, each thread sums rows rg, rg + 4, ... in order, the four partial sums are added in group order
// (deterministic: no atomics).
template <typename T>
__global__ __launch_bounds__(256) void pool_rows_kernel(const float* __restrict__ x, long x_bs, int rows, int C,
                                                        const float* __restrict__ mask, long m_bs, T* __restrict__ out, long ldo) {
    __shared__ float part[4][64], cnt[4];
    const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6, c = blockIdx.x * 64 + cl, b = blockIdx.y;
    float s = 0.f, n = 0.f;
    for (int t = rg; t < rows; t += 4) {
        const float m = mask ? mask[(long)b * m_bs + t] : 1.f;
        n += m;
        if (c < C) s += x[(long)b * x_bs + (long)t * C + c] * m;
    }
    part[rg][cl] = s;
    if (cl == 0) cnt[rg] = n;
    __syncthreads();
    if (rg == 0 && c < C) {
        const float tot = ((part[0][cl] + part[1][cl]) + part[2][cl]) + part[3][cl];
        const float den = fmaxf(((cnt[0] + cnt[1]) + cnt[2]) + cnt[3], 1.f);
        out[(long)b * ldo + c] = Cvt<T>::from_f(tot / den);
    }
}
extern "C" int mmx_pool_rows(const float* x, int64_t x_bs, int rows, int C, int batch, const float* mask, int64_t m_bs, void* out,
                             int64_t ldo, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(x && out && rows > 0 && C > 0 && batch > 0 && batch <= 65535 && ldo >= C && x_bs >= (int64_t)rows * C);
    MMX_CHECK_ARG(!mask || m_bs >= rows);
    const dim3 grid((C + 63) / 64, batch);
    if (dtype == MMX_BF16) hipLaunchKernelGGL(pool_rows_kernel<bf16_t>, grid, dim3(256), 0, stream, x, (long)x_bs, rows, C, mask, (long)m_bs, (bf16_t*)out, (long)ldo);
    else hipLaunchKernelGGL(pool_rows_kernel<float>, grid, dim3(256), 0, stream, x, (long)x_bs, rows, C, mask, (long)m_bs, (float*)out, (long)ldo);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

// ---------------------------------------------------------------------------- weight prefetch into L2 / Infinity Cache
// Reads up to four byte ranges with default-policy 16-byte loads and keeps nothing: the lines stay in the issuing XCD's L2 and in
// the memory-side Infinity Cache.  Launched on a SIDE stream of the captured LM decode step with the NEXT layer's packed weights
// while the current layer computes (mmx/llm.py: LlmEngine.prefetch), so that the next layer's projections - one dependent round of
// weight loads each - find their 30 MB in the Infinity Cache (545 cycles, ~10 TB/s) instead of HBM (900 cycles).  The loaded
// words are folded into one value that is stored only if it equals a sentinel no data produces (the loads stay, nothing is written).
struct PrefetchArgs { const uint4* p[4]; long n[4]; unsigned* sink; };
__global__ __launch_bounds__(256) void prefetch_kernel(PrefetchArgs a) {
    unsigned acc = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long n16 = a.n[r] >> 4;
        for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long)gridDim.x * 256 * 4) {
            uint4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long j = i + (long)u * gridDim.x * 256;
                v[u] = j < n16 ? a.p[r][j] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc ^= v[u].x ^ v[u].y ^ v[u].z ^ v[u].w;
        }
    }
    if (acc == 0x9E3779B9u && a.sink) *a.sink = acc;   // never true for packed weights in practice; harmless if it is
}
extern "C" int mmx_prefetch4(const void* p0, int64_t n0, const void* p1, int64_t n1, const void* p2, int64_t n2, const void* p3,
                             int64_t n3, void* sink, int workgroups, hipStream_t stream) {
    MMX_CHECK_ARG(workgroups > 0 && workgroups <= 4096 && n0 >= 0 && n1 >= 0 && n2 >= 0 && n3 >= 0);
    MMX_CHECK_ARG(((uintptr_t)p0 % 16) == 0 && ((uintptr_t)p1 % 16) == 0 && ((uintptr_t)p2 % 16) == 0 && ((uintptr_t)p3 % 16) == 0);
    PrefetchArgs a{{(const uint4*)p0, (const uint4*)p1, (const uint4*)p2, (const uint4*)p3}, {p0 ? n0 : 0, p1 ? n1 : 0, p2 ? n2 : 0, p3 ? n3 : 0},
                   (unsigned*)sink};
    hipLaunchKernelGGL(prefetch_kernel, dim3(workgroups), dim3(256), 0, stream, a);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

// ---------------------------------------------------------------------------- linear resampling in time (speed change)
// F.interpolate(x [rows][T], size=T2, mode="linear", align_corners=False) as torch's CPU kernel computes it: scale = T / T2 in
// fp32, src = scale * (t + 0.5) - 0.5 clamped at 0, out = (1 - w) * x[i0] + w * x[min(i0 + 1, T - 1)], w = src - i0
// (speech/cosyvoice/cli/model.py:312-314: tts_mel resampled by 1 / speed before the vocoder).
__global__ void resample_linear_kernel(const float* __restrict__ x, int T, int T2, long rows, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * T2) return;
    const long r = i / T2;
    const int t = (int)(i - r * T2);
    const float scale = (float)T / (float)T2;
    float src = scale * ((float)t + 0.5f) - 0.5f;
    src = src < 0.f ? 0.f : src;
    const int i0 = (int)src;
    const int i1 = i0 + (i0 < T - 1 ? 1 : 0);
    const float w1 = src - (float)i0, w0 = 1.f - w1;
    out[i] = w0 * x[r * T + i0] + w1 * x[r * T + i1];
}
extern "C" int mmx_resample_linear(const float* x, int64_t rows, int T, int T2, float* out, hipStream_t stream) {
    MMX_CHECK_ARG(x && out && rows > 0 && T > 0 && T2 > 0);
    const long n = rows * T2;
    hipLaunchKernelGGL(resample_linear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, x, T, T2, (long)rows, out);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

// ---------------------------------------------------------------------------- SwiGLU (prefill)
template <typename T>
__global__ void swiglu_kernel(const float* __restrict__ gu, long ldgu, int I, T* __restrict__ out, long ldo) {
    const long r = blockIdx.y;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= I) return;
    float g = gu[r * ldgu + c], u = gu[r * ldgu + I + c];
    float s = g / (1.f + expf(-g));
    out[r * ldo + c] = Cvt<T>::from_f(s * u);
}
extern "C" int mmx_swiglu(const float* gu, int64_t ldgu, int rows, int I, void* out, int64_t ldo, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(gu && out && rows > 0 && I > 0);
    dim3 grid((I + 255) / 256, rows);
    return dispatch_dtype(dtype, [&](auto el) {
        hipLaunchKernelGGL(swiglu_kernel<decltype(el)>, grid, dim3(256), 0, stream, gu, ldgu, I, (decltype(el)*)out, ldo);
        return launch_status();
    });
}

// ---------------------------------------------------------------------------- GroupNorm over time-major [B][T][C]
// one workgroup per (group, batch): statistics over (C/groups channels) x T, two-pass in fp32 (mean, then variance),
// like torch.nn.GroupNorm on x.float() (arch_util.GroupNorm32).  T is a few hundred frames: a reference mel crop.
template <typename T>
__global__ __launch_bounds__(256) void groupnorm_kernel(const float* __restrict__ x, int Tn, int C, int cpg,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, int act, const float* __restrict__ rowmask,
                                                        T* __restrict__ out) {
    __shared__ float sh[8];
    const int g = blockIdx.x, b = blockIdx.y;
    const float* xb = x + (long)b * Tn * C + g * cpg;
    T* ob = out + (long)b * Tn * C + g * cpg;
    const int n = Tn * cpg;
    auto block_sum = [&](float v) {
        v = wave_sum(v);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
        __syncthreads();
        return sh[0] + sh[1] + sh[2] + sh[3];
    };
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += xb[(long)(i / cpg) * C + i % cpg];
    const float mean = block_sum(s) / (float)n;
    float q = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        float d = xb[(long)(i / cpg) * C + i % cpg] - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(block_sum(q) / (float)n + eps);
    for (int i = threadIdx.x; i < n; i += 256) {
        const int c = i % cpg;
        const long o = (long)(i / cpg) * C + c;
        float y = (xb[o] - mean) * rstd * gamma[g * cpg + c] + beta[g * cpg + c];
        if (act == ACT_MISH) y = act_c<ACT_MISH, sizeof(T) == 4>(y, 0.f);
        if (rowmask) y *= rowmask[(long)b * Tn + i / cpg];
        ob[o] = Cvt<T>::from_f(y);
    }
}
extern "C" int mmx_groupnorm(const float* x, int B, int T_, int C, int groups, const float* gamma, const float* beta,
                             float eps, int act, const float* rowmask, void* out, int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(x && gamma && beta && out && B > 0 && T_ > 0 && C > 0 && groups > 0 && C % groups == 0);
    MMX_CHECK_ARG(act == ACT_NONE || act == ACT_MISH);
    dim3 grid(groups, B);
    return dispatch_dtype(dtype, [&](auto el) {
        hipLaunchKernelGGL(groupnorm_kernel<decltype(el)>, grid, dim3(256), 0, stream, x, T_, C, C / groups, gamma, beta, eps, act, rowmask, (decltype(el)*)out);
        return launch_status();
    });
}

// ---------------------------------------------------------------------------- elementwise activation * row mask
template <typename T>
__global__ void act_rows_kernel(const float* __restrict__ x, long n, int C, int act, const float* __restrict__ rowmask,
                                float* __restrict__ outf, T* __restrict__ outa) {
    constexpr bool PRECISE = sizeof(T) == 4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float v = act_apply<PRECISE>(x[i], act, 0.1f);
        if (rowmask) v *= rowmask[i / C];
        if (outf) outf[i] = v;
        if (outa) outa[i] = Cvt<T>::from_f(v);
    }
}
extern "C" int mmx_act_rows(const float* x, int64_t rows, int C, int act, const float* rowmask, float* out_f32, void* out_act,
                            int dtype, hipStream_t stream) {
    dtype = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(x && rows > 0 && C > 0 && (out_f32 || out_act) && act >= ACT_NONE && act <= ACT_TANH);
    const long n = rows * C;
    const unsigned grid = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    return dispatch_dtype(dtype, [&](auto el) {
        hipLaunchKernelGGL(act_rows_kernel<decltype(el)>, dim3(grid), dim3(256), 0, stream, x, n, C, act, rowmask, out_f32, (decltype(el)*)out_act);
        return launch_status();
    });
}

extern "C" int mmx_abi_version(void) { return 10; }
