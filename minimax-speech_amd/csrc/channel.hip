// Channel degradations of mono fp32 clips (a ragged batch) for gfx950: what the reference's low_pass / high_pass
// (dac-vae/audiotools/core/dsp.py:153-215) and mel_filterbank / equalizer / clip_distortion / quantization / mulaw_quantization
// (core/effects.py:386-523) need beside the long FIR of degrade.hip.  mmx/channel.py states the definitions and designs the taps.
//
//   mmx_pad_edge_rows  pad_edge_kernel: row b of N + 2 half samples = the clip with its first and last sample repeated `half` times
//                      either side (replicate padding; half may exceed N), zeros from there to the row's width.  The padded rows go
//                      through mmx_ir_prepare / mmx_fir_rows as they are (wrap = 0): output n of the filter is sample n + 2 half.
//   mmx_row_select     row_select_kernel, exact order statistics of ragged rows for up to SEL_RANKS ranks per row: a radix select on
//                      the order-preserving integer image of the bits (sign flipped for positives, all bits for negatives; -0 counts
//                      as +0), 8 bits a pass, most significant first.  ALWAYS SEL_PASSES = 4 counting launches and one finishing
//                      launch: no loop bound is read from data.  A workgroup owns SEL_SPAN consecutive samples of one row (a longer
//                      row is split over blockIdx.x), counts the digit of the samples that carry a rank's prefix into an integer
//                      histogram in LDS (ds_add_u32) and adds its non-zero bins to the row's histogram in `work` (integer atomics:
//                      the sums do not depend on arrival order).  The launch of pass p first picks the digit of pass p - 1 from that
//                      pass's finished histogram - one wave per rank: four bins a lane, a shuffle scan over the lanes - and workgroup 0
//                      of the row leaves the prefix and the remaining rank in `work` for the next launch: nothing returns to the
//                      host.  Pass 0 also raises the row's NaN flag.
//   mmx_clip_rows      clip_rows_kernel: thresholds v[lo] + (v[hi] - v[lo]) w in fp64 from the order statistics and the host's
//                      weights, rounded once; out = min(max(x, lo), hi); a flagged row is NaN throughout.
//   mmx_quantize_rows  quantize_rows_kernel: the uniform and the mu-law quantizer, fp64 per sample, rounded once.
// A row's numbers depend on its own samples, length and parameters alone.  Whatever lens, ranks and q hold in device memory, no
// kernel here reads or writes outside the stated buffers: every index derived from them is clamped first.
#include "common.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int CH_THREADS = 256, CH_PER = 16;            // the elementwise kernels: 4096 samples a workgroup
constexpr int SEL_THREADS = 256, SEL_PER = 32;
constexpr int SEL_SPAN = 8192;                          // samples of one row a workgroup of the select counts
constexpr int SEL_RANKS = 4, SEL_PASSES = 4, SEL_BINS = 256;
constexpr int SEL_WORK = SEL_PASSES * SEL_BINS + 8;     // int32 per (row, rank): four histograms, three (prefix, rank) pairs, two spare
static_assert(SEL_SPAN == SEL_THREADS * SEL_PER && SEL_THREADS / 64 == SEL_RANKS && SEL_BINS == 4 * 64);

__global__ __launch_bounds__(CH_THREADS) void pad_edge_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                             int half, float* __restrict__ out, long o_bs) {
    const int b = blockIdx.y;
    const int N = row_len(lens, b, L);
    const long W = (long)L + 2L * half, end = (long)N + 2L * half;
    const long j0 = (long)blockIdx.x * (CH_THREADS * CH_PER) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < CH_PER; ++r) {
        const long j = j0 + r * CH_THREADS;
        if (j >= W) break;
        float v = 0.f;
        if (N > 0 && j < end) v = x[(long)b * x_bs + min(max(j - half, 0L), (long)N - 1)];
        out[(long)b * o_bs + j] = v;
    }
}

// ascending unsigned keys <-> ascending floats; -0 and +0 share a key
__device__ __forceinline__ unsigned sel_key(float v) {
    unsigned u = __float_as_uint(v);
    if ((u << 1) == 0u) u = 0u;                         // on the bits: a denormal is not a zero, whatever the float mode
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// pass 0 .. 3: count digit `pass`; pass 4: finish.  work int32 [B][R][SEL_WORK]
__global__ __launch_bounds__(SEL_THREADS) void row_select_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                                const int* __restrict__ ranks, int R, int pass, unsigned* __restrict__ work,
                                                                float* __restrict__ out, int* __restrict__ nanflag) {
    __shared__ unsigned hist[SEL_RANKS][SEL_BINS];
    __shared__ unsigned pre[SEL_RANKS], rem[SEL_RANKS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
    const int N = row_len(lens, b, L);
    if (N < 1) return;                                  // uniform; the entry point refuses such a row
    for (int i = tid; i < SEL_RANKS * SEL_BINS; i += SEL_THREADS) (&hist[0][0])[i] = 0u;

    // the state before this pass: wave r picks rank r's digit of pass - 1 from that pass's finished histogram
    if (wv < R) {
        unsigned* wr = work + ((long)b * R + wv) * SEL_WORK;
        unsigned prefix = 0u, k = (unsigned)max(0, min(ranks[b * R + wv], N - 1));
        if (pass > 1) {
            prefix = wr[SEL_PASSES * SEL_BINS + 2 * (pass - 2)];
            k = wr[SEL_PASSES * SEL_BINS + 2 * (pass - 2) + 1];
        }
        if (pass > 0) {
            const unsigned* h = wr + (pass - 1) * SEL_BINS + 4 * lane;
            const unsigned c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
            unsigned incl = c0 + c1 + c2 + c3;
            const unsigned own = incl;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            const unsigned excl = incl - own;
            // the one lane whose bins hold rank k; should the counts not reach k (they do: k < N), the last lane's last bin
            const bool mine = (excl <= k && k < incl) || (lane == 63 && k >= incl);
            if (mine) {
                unsigned d = 3u, below = excl + c0 + c1 + c2;
                if (k < excl + c0) { d = 0u; below = excl; }
                else if (k < excl + c0 + c1) { d = 1u; below = excl + c0; }
                else if (k < excl + c0 + c1 + c2) { d = 2u; below = excl + c0 + c1; }
                pre[wv] = (prefix << 8) | (4u * lane + d);
                rem[wv] = k >= below ? k - below : 0u;
            }
        } else if (lane == 0) {
            pre[wv] = 0u;
            rem[wv] = k;
        }
    }
    __syncthreads();
    if (pass > 0 && pass < SEL_PASSES && blockIdx.x == 0 && tid < R) {
        unsigned* wr = work + ((long)b * R + tid) * SEL_WORK + SEL_PASSES * SEL_BINS + 2 * (pass - 1);
        wr[0] = pre[tid];
        wr[1] = rem[tid];
    }
    if (pass == SEL_PASSES) {                           // the prefix is the whole key
        if (blockIdx.x == 0 && tid < R) out[b * R + tid] = nanflag[b] ? NAN : sel_value(pre[tid]);
        return;
    }

    const long j0 = (long)blockIdx.x * SEL_SPAN;
    if (j0 >= N) return;                                // uniform
    const int shift = 24 - 8 * pass;
    const float* xb = x + (long)b * x_bs;
    unsigned p[SEL_RANKS];
#pragma unroll
    for (int r = 0; r < SEL_RANKS; ++r) p[r] = r < R ? pre[r] : 0u;
    bool nan = false;
#pragma unroll 4
    for (int i = 0; i < SEL_PER; ++i) {
        const long j = j0 + i * SEL_THREADS + tid;
        if (j >= N) break;
        const float v = xb[j];
        nan |= v != v;
        const unsigned key = sel_key(v), d = (key >> shift) & 0xffu;
        if (pass == 0) {
            atomicAdd(&hist[0][d], 1u);                 // no prefix yet: one histogram serves every rank
        } else {
            const unsigned top = key >> (shift + 8);
#pragma unroll
            for (int r = 0; r < SEL_RANKS; ++r)
                if (r < R && top == p[r]) atomicAdd(&hist[r][d], 1u);
        }
    }
    if (pass == 0 && __any(nan) && lane == 0) atomicOr(nanflag + b, 1);
    __syncthreads();
    for (int r = 0; r < R; ++r) {
        const unsigned c = hist[pass == 0 ? 0 : r][tid];
        if (c) atomicAdd(work + ((long)b * R + r) * SEL_WORK + pass * SEL_BINS + tid, c);
    }
}

// stats fp32 [B][4]: v[lo], v[hi] of the lower quantile, v[lo], v[hi] of the upper; w f64 [B][2]
__global__ __launch_bounds__(CH_THREADS) void clip_rows_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                              const float* __restrict__ stats, const double* __restrict__ w,
                                                              const int* __restrict__ nanflag, float* __restrict__ thr,
                                                              float* __restrict__ out, long o_bs) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int N = row_len(lens, b, L);
    const bool bad = nanflag[b] != 0;
    const float* s = stats + 4 * b;
    const float lo = bad ? NAN : (float)((double)s[0] + ((double)s[1] - (double)s[0]) * w[2 * b]);
    const float hi = bad ? NAN : (float)((double)s[2] + ((double)s[3] - (double)s[2]) * w[2 * b + 1]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        thr[2 * b] = lo;
        thr[2 * b + 1] = hi;
    }
    const long j0 = (long)blockIdx.x * (CH_THREADS * CH_PER) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < CH_PER; ++r) {
        const long j = j0 + r * CH_THREADS;
        if (j >= L) break;
        float v = 0.f;
        if (j < N) {
            v = x[(long)b * x_bs + j];
            v = v < lo ? lo : v;                        // torch.clamp: min(max(x, lo), hi), a NaN sample stays
            v = hi < v ? hi : v;
            if (bad) v = NAN;
        }
        out[(long)b * o_bs + j] = v;
    }
}

template <int MODE>
__global__ __launch_bounds__(CH_THREADS) void quantize_rows_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                                  const int* __restrict__ q, float* __restrict__ out, long o_bs) {
#pragma clang fp contract(off)
    const int b = blockIdx.y;
    const int N = row_len(lens, b, L);
    const double Q = (double)max(q[b], 2), mu = Q - 1.0, lmu = log1p(mu);
    const long j0 = (long)blockIdx.x * (CH_THREADS * CH_PER) + threadIdx.x;
#pragma unroll 1
    for (int r = 0; r < CH_PER; ++r) {
        const long j = j0 + r * CH_THREADS;
        if (j >= L) break;
        float v = 0.f;
        if (j < N) {
            const double a = (double)x[(long)b * x_bs + j];
            if constexpr (MODE == 0) {                  // effects.py:481-486
                v = (float)(2.0 * (floor((a + 1.0) / 2.0 * Q) / Q) - 1.0);
            } else {                                    // effects.py:514-519
                const double sg = a > 0.0 ? 1.0 : a < 0.0 ? -1.0 : a;           // torch.sign: 0 at 0, NaN stays
                const double c = trunc((sg * log1p(mu * fabs(a)) / lmu + 1.0) / 2.0 * mu + 0.5);
                const double z = c / mu * 2.0 - 1.0;
                const double sz = z > 0.0 ? 1.0 : z < 0.0 ? -1.0 : z;
                v = (float)(sz * (exp(fabs(z) * lmu) - 1.0) / mu);
            }
        }
        out[(long)b * o_bs + j] = v;
    }
}

inline dim3 ch_grid(long width, int B) { return dim3((unsigned)((width + CH_THREADS * CH_PER - 1) / (CH_THREADS * CH_PER)), B); }

}  // namespace

extern "C" int mmx_pad_edge_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, int half,
                                 float* out, int64_t o_bs, hipStream_t stream) {
    MMX_CHECK_ARG(x && out && (const void*)x != (const void*)out && x_bs >= L && half >= 0 && half <= (1 << 24));
    if (int rc = rows_form(B, L, lens, h_lens, 1)) return rc;
    MMX_CHECK_ARG((long)L + 2L * half <= 0x7fffffffL && o_bs >= (long)L + 2L * half);
    hipLaunchKernelGGL(pad_edge_kernel, ch_grid((long)L + 2L * half, B), dim3(CH_THREADS), 0, stream, x, (long)x_bs, L, lens, half, out,
                       (long)o_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_row_select(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const int32_t* ranks,
                              const int32_t* h_ranks, int R, float* out, int32_t* nanflag, int32_t* work, hipStream_t stream) {
    MMX_CHECK_ARG(x && ranks && h_ranks && out && nanflag && work && x_bs >= L && R >= 1 && R <= SEL_RANKS);
    if (int rc = rows_form(B, L, lens, h_lens, 1)) return rc;
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < R; ++r) MMX_CHECK_ARG(h_ranks[b * R + r] >= 0 && h_ranks[b * R + r] < (h_lens ? h_lens[b] : L));
    if (hipMemsetAsync(work, 0, sizeof(int32_t) * (size_t)B * R * SEL_WORK, stream) != hipSuccess) return MMX_EARG;
    if (hipMemsetAsync(nanflag, 0, sizeof(int32_t) * B, stream) != hipSuccess) return MMX_EARG;
    for (int pass = 0; pass <= SEL_PASSES; ++pass) {
        const dim3 grid(pass < SEL_PASSES ? (L + SEL_SPAN - 1) / SEL_SPAN : 1, B);
        hipLaunchKernelGGL(row_select_kernel, grid, dim3(SEL_THREADS), 0, stream, x, (long)x_bs, L, lens, ranks, R, pass, (unsigned*)work,
                           out, nanflag);
        MMX_LAUNCH_CHECK();
    }
    return MMX_OK;
}

extern "C" int mmx_clip_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const float* stats,
                             const double* w, const int32_t* nanflag, float* thr, float* out, int64_t o_bs, hipStream_t stream) {
    MMX_CHECK_ARG(x && stats && w && nanflag && thr && out && x_bs >= L && o_bs >= L);
    if (int rc = rows_form(B, L, lens, h_lens, 1)) return rc;
    hipLaunchKernelGGL(clip_rows_kernel, ch_grid(L, B), dim3(CH_THREADS), 0, stream, x, (long)x_bs, L, lens, stats, w, nanflag, thr, out,
                       (long)o_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_quantize_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, int mode,
                                 const int32_t* q, const int32_t* h_q, float* out, int64_t o_bs, hipStream_t stream) {
    MMX_CHECK_ARG(x && q && h_q && out && x_bs >= L && o_bs >= L && (mode == 0 || mode == 1));
    if (int rc = rows_form(B, L, lens, h_lens, 1)) return rc;
    for (int b = 0; b < B; ++b) MMX_CHECK_ARG(h_q[b] >= 2);
    if (mode == 0)
        hipLaunchKernelGGL(quantize_rows_kernel<0>, ch_grid(L, B), dim3(CH_THREADS), 0, stream, x, (long)x_bs, L, lens, q, out, (long)o_bs);
    else
        hipLaunchKernelGGL(quantize_rows_kernel<1>, ch_grid(L, B), dim3(CH_THREADS), 0, stream, x, (long)x_bs, L, lens, q, out, (long)o_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
