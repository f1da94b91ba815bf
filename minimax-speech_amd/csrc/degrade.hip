// Room and noise simulation of mono fp32 clips (a ragged batch) for gfx950: the reference's EffectMixin.convolve / apply_ir /
// alter_drr / measure_drr / mix (dac-vae/audiotools/core/effects.py:27-179, 540-647).  mmx/degrade.py states the definitions and
// builds the one host table (the periodic Hann windows of alter_drr).
//
// The long FIR as a framed product on the spectral tile's arithmetic (spec_tile.h: split3, ld8, mfma6).  For a clip x of N samples
// and an impulse response h cut to L' = min(L, N) taps, peak position p, scale s (mmx_ir_prepare finds them):
//     y[n] = s * sum_t h[t] X(n + p - t),   X = x wrapped modulo N (wrap) or zero outside [0, N)
// With g[v] = h[L' - 1 - v] (zero outside [0, L')) and base = p - L' + 1:
//     y[16 m + j] = sum_u g[u - j] X(16 m + base + u),   0 <= u < L' + 15
// which is A[m][u] = X(16 m + base + u), the frames at HOP 16 of the sample span, times the ONE 16-column tile B[u][j] = g[u - j]
// (K = L' + 15 rounded up to 32 by zero rows).  Every MAC of a tile is a useful tap but the 15 x 15 corner triangles.
//   mmx_ir_prepare  ir_prepare_kernel, one workgroup per clip: alter_drr on the whole IR where a target is given (fp64 sums in a fixed
//                   tree order, the larger root, the floor max|late| / max|early|, ensure_max_of_audio(1)), the measured DRR of
//                   what it leaves, L', p, s;  ir_table_kernel: B as three bf16 planes [3][kcap / 32][64][8] (mmx_pack_skinny order).
//   mmx_fir_rows    fir_rows_kernel: a workgroup of 4 waves owns FIR_NOUT = 4096 consecutive outputs of one clip = 16 row tiles of
//                   16 frames x 16 columns; wave w holds the tiles w, w + 4, w + 8, w + 12 in registers, so a B fragment (loaded
//                   from L2 four steps ahead) feeds FIR_RT = 4 six-term products.  K is walked in chunks of FIR_CHUNK = 4096
//                   ascending, the MFMA chain restarted every 1024 taps and its sums added in order (fp32); a chunk's sample span (FIR_NOUT - 16 + chunk samples; the index rule applied once, here) is staged as
//                   three bf16 planes.  A frame's fragment read is ds_read_b128 at 32-byte row pitch: the four 16-lane groups of
//                   that instruction each fall on 16 different 16-byte slots (rows 0-3 / 12-15 with the next k group's rows 4-11),
//                   so the planes need no gap.  LDS: 3 * 2 * (4096 - 16 + min(4096, kp)) <= 49 056 bytes.
//                   y * s -> out (zeros from lens[b] to L), max |y * s| per row by an atomic max on the bit pattern.
//   mmx_row_absmax  max |x| per row, the same atomic.      mmx_mix_rows  x + exp((Lx - snr - Ln) ln 10 / 20) * noise.
// An output's bits are a function of its clip, its prepared IR and its position n: the workgroup and the tile are n / 4096 and
// (n % 4096) / 256, the K order is fixed; nothing depends on the batch, the row index or the companions.
// Whatever p, taps and lens hold in device memory, no kernel here reads or writes outside the stated buffers: every index that is
// derived from them is clamped or range-checked first.
#include "spec_tile.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int FIR_WAVES = 4, FIR_THREADS = FIR_WAVES * 64;
constexpr int FIR_RT = 4;                               // row tiles (256 outputs each) a wave holds
constexpr int FIR_NOUT = FIR_WAVES * FIR_RT * 256;      // outputs per workgroup
constexpr int FIR_CHUNK = 4096;                         // K columns staged at a time
constexpr int FIR_DEPTH = 4;                            // B fragments a wave keeps in flight (48 registers)
constexpr int FIR_FLUSH = 32;                           // K steps (1024 taps) summed by the MFMA chain before they join the total
constexpr int FIR_MAX_TAPS = 65536;
static_assert(FIR_FLUSH % FIR_DEPTH == 0 && (FIR_CHUNK / 32) % FIR_FLUSH == 0);
constexpr int PREP_THREADS = 512;

__host__ __device__ __forceinline__ int fir_kp(int taps) { return (taps + 15 + 31) / 32 * 32; }
__host__ __device__ __forceinline__ size_t fir_lds(int kp) { return (size_t)3 * (FIR_NOUT - 16 + min(FIR_CHUNK, kp)) * sizeof(bf16_t); }

// ------------------------------------------------------------------------------------------ block reductions (fixed tree order)
__device__ __forceinline__ double blk_sum(double v, double* sh, int tid) {
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = PREP_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    return sh[0];
}
__device__ __forceinline__ double blk_max(double v, double* sh, int tid) {
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int o = PREP_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) sh[tid] = fmax(sh[tid], sh[tid + o]);
        __syncthreads();
    }
    return sh[0];
}
// first index of the largest key over [0, n) (key = |v| or v); NaNs never win; n >= 1
template <bool ABS>
__device__ __forceinline__ int blk_argmax(const float* v, int n, float* kh, int* ih, int tid, float* best) {
    float k = -INFINITY;
    int at = 0x7fffffff;
    for (int i = tid; i < n; i += PREP_THREADS) {
        const float c = ABS ? fabsf(v[i]) : v[i];
        if (c > k) { k = c; at = i; }
    }
    __syncthreads();
    kh[tid] = k;
    ih[tid] = at;
    __syncthreads();
    for (int o = PREP_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const float k2 = kh[tid + o];
            const int i2 = ih[tid + o];
            if (k2 > kh[tid] || (k2 == kh[tid] && i2 < ih[tid])) { kh[tid] = k2; ih[tid] = i2; }
        }
        __syncthreads();
    }
    if (best) *best = kh[0];
    return ih[0] == 0x7fffffff ? 0 : ih[0];
}

// a wave's share of a row's max |x| (m its lanes' maxima, nan: a lane met a NaN) joins *peak by an atomic max on the bit pattern of
// a non-negative float; NaN is the largest pattern: it stays
__device__ __forceinline__ void peak_join(float m, bool nan, float* peak, int lane) {
    m = wave_max(m);
    if (__any(nan)) m = NAN;
    if (lane == 0) atomicMax(reinterpret_cast<unsigned*>(peak), __float_as_uint(fabsf(m)));
}

// hann: f64 [2 t0 + 1][2 t0 + 1], row c - 1 = the periodic Hann window of c points (scipy.signal.get_window("hann", c))
__global__ __launch_bounds__(PREP_THREADS) void ir_prepare_kernel(const float* __restrict__ ir, long ir_bs, int Lir, const int* __restrict__ ir_lens,
                                                                int Lsig, const int* __restrict__ sig_lens, const float* __restrict__ drr,
                                                                int t0, const double* __restrict__ hann, int start_at_max,
                                                                float* __restrict__ h_out, long h_bs, int* __restrict__ p_out,
                                                                float* __restrict__ s_out, int* __restrict__ taps_out,
                                                                float* __restrict__ drr_out) {
    __shared__ double sh[PREP_THREADS];
    __shared__ float kh[PREP_THREADS];
    __shared__ int ih[PREP_THREADS];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int L = max(1, row_len(ir_lens, b, Lir));
    const int N = max(1, row_len(sig_lens, b, Lsig));
    const float* src = ir + (long)b * ir_bs;
    float* dst = h_out + (long)b * h_bs;
    const int W = 2 * t0 + 1;
    const float target = drr ? drr[b] : NAN;

    if (target == target) {                             // alter_drr (effects.py:617-647) on the whole IR
        const int td = blk_argmax<false>(src, L, kh, ih, tid, nullptr);
        const int lo = max(td - t0, 0), hi = min(td + t0, L - 1);
        const double* w = hann + (long)(hi - lo) * W;   // count - 1 = hi - lo
        double a = 0.0, bq = 0.0, c1 = 0.0, l2 = 0.0, emax = 0.0, lmax = 0.0;
        for (int i = tid; i < L; i += PREP_THREADS) {
            const double v = (double)src[i], v2 = v * v;
            if (i >= lo && i <= hi) {
                const double wi = w[i - lo];
                a += wi * wi * v2;
                bq += 2.0 * (1.0 - wi) * wi * v2;
                c1 += (1.0 - wi) * (1.0 - wi) * v2;
                emax = fmax(emax, fabs(v));
            } else {
                l2 += v2;
                lmax = fmax(lmax, fabs(v));
            }
        }
        a = blk_sum(a, sh, tid);
        bq = blk_sum(bq, sh, tid);
        c1 = blk_sum(c1, sh, tid);
        l2 = blk_sum(l2, sh, tid);
        emax = blk_max(emax, sh, tid);
        lmax = blk_max(lmax, sh, tid);
        const double c = c1 - pow(10.0, (double)target / 10.0) * l2;
        const double disc = bq * bq - 4.0 * a * c;
        double alpha = NAN;                             // a negative discriminant: NaN, as the reference's sqrt gives
        if (disc >= 0.0) {
            const double e = sqrt(disc);
            alpha = fmax((-bq - e) / (2.0 * a), (-bq + e) / (2.0 * a));
            const double floor_ = lmax / emax;
            if (!(alpha == alpha) || !(floor_ == floor_)) alpha = NAN;
            else alpha = fmax(alpha, floor_);
        }
        auto altered = [&](int i) {
            const double v = (double)src[i];
            if (!(alpha == alpha)) return alpha;         // the reference's alpha * 0 * 0 outside the window: NaN everywhere
            if (i < lo || i > hi) return v;
            const double wi = w[i - lo];
            return alpha * wi * v + (1.0 - wi) * v;
        };
        double peak = 0.0;
        for (int i = tid; i < L; i += PREP_THREADS) peak = fmax(peak, fabs(altered(i)));
        peak = blk_max(peak, sh, tid);
        const double gain = peak > 1.0 ? 1.0 / peak : 1.0;          // ensure_max_of_audio(1.0)
        for (int i = tid; i < L; i += PREP_THREADS) dst[i] = (float)(altered(i) * gain);
    } else {
        for (int i = tid; i < L; i += PREP_THREADS) dst[i] = src[i];
    }
    for (int i = L + tid; i < Lir; i += PREP_THREADS) dst[i] = 0.f;
    __syncthreads();                                    // the block's own global writes are visible to it from here

    {                                                   // measure_drr (effects.py:576-589) of what is now in dst
        const int td = blk_argmax<false>(dst, L, kh, ih, tid, nullptr);
        const int lo = max(td - t0, 0), hi = min(td + t0, L - 1);
        double e2 = 0.0, l2 = 0.0;
        for (int i = tid; i < L; i += PREP_THREADS) {
            const double v = (double)dst[i];
            if (i >= lo && i <= hi) e2 += v * v;
            else l2 += v * v;
        }
        e2 = blk_sum(e2, sh, tid);
        l2 = blk_sum(l2, sh, tid);
        if (tid == 0) drr_out[b] = (float)(10.0 * log10(e2 / l2));
    }
    const int taps = min(L, N);                         // effects.py:85-90: an IR longer than the signal is truncated
    float peak = 0.f;
    const int p = blk_argmax<true>(dst, taps, kh, ih, tid, &peak);
    if (tid == 0) {
        p_out[b] = start_at_max ? p : 0;
        s_out[b] = 1.f / fmaxf(peak, 1e-5f);            // effects.py:113-119: the delta's response peaks at the IR's own peak
        taps_out[b] = taps;
    }
}

// table [B][3][kcap / 32][64][8]: element (kt, lane = (g, j), e) of plane s = term s of g[u - j], u = 32 kt + 8 g + e
__global__ __launch_bounds__(256) void ir_table_kernel(const float* __restrict__ h, long h_bs, int Lir, const int* __restrict__ taps_in,
                                                      bf16_t* __restrict__ table, int kcap) {
    const int b = blockIdx.y;
    const long PB = (long)kcap * 16;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= PB) return;
    const int taps = max(1, min(min(taps_in[b], Lir), FIR_MAX_TAPS));
    const int e = idx & 7, lane = (idx >> 3) & 63, kt = (int)(idx >> 9);
    const int u = kt * 32 + (lane >> 4) * 8 + e, v = u - (lane & 15);
    const float val = (v >= 0 && v < taps) ? h[(long)b * h_bs + (taps - 1 - v)] : 0.f;
    put3(table + (long)b * 3 * PB, PB, idx, val);
}

__global__ __launch_bounds__(FIR_THREADS) void fir_rows_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                              const bf16_t* __restrict__ table, int kcap, const int* __restrict__ p_in,
                                                              const float* __restrict__ s_in, const int* __restrict__ taps_in, int wrap,
                                                              float* __restrict__ out, long o_bs, float* __restrict__ peak) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y;
    const long out0 = (long)blockIdx.x * FIR_NOUT;
    const int N = row_len(lens, b, L);
    float* ob = out + (long)b * o_bs;
    const int width = (int)min((long)FIR_NOUT, L - out0);
    if (out0 >= N) {                                    // a workgroup of tail columns (uniform)
        for (int i = tid; i < width; i += FIR_THREADS) ob[out0 + i] = 0.f;
        return;
    }
    const int taps = max(1, min(min(taps_in[b], N), FIR_MAX_TAPS));
    const int kp = min(fir_kp(taps), kcap), nkt = kp / 32;
    const int p = max(0, min(p_in[b], taps - 1));
    const int CK = min(FIR_CHUNK, kp), SP = FIR_NOUT - 16 + CK;
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);       // [3][SP]
    const float* xb = x + (long)b * x_bs;
    const int valid = (int)min((long)FIR_NOUT, N - out0);           // outputs of this workgroup inside the clip
    const int ntiles = (valid + 255) / 256;
    const int mine = wv < ntiles ? (ntiles - wv + FIR_WAVES - 1) / FIR_WAVES : 0;      // tiles wv, wv + 4, ..
    const int span = (ntiles - 1) * 256 + 240;          // samples under the live tiles' frames, less the chunk's width
    const long PB = (long)kcap * 16;
    const bf16_t* tb = table + (long)b * 3 * PB + lane * 8;

    // part: the MFMA chain's sum over at most FIR_FLUSH steps; acc: the sum of those.  A chain of 24 000 taps in one fp32
    // accumulator measured 2.1e-6 of the output's peak against float64; in runs of 1024 it stays at the short chains' level.
    float4_t acc[FIR_RT], part[FIR_RT];
#pragma unroll
    for (int r = 0; r < FIR_RT; ++r) acc[r] = part[r] = float4_t{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int k0 = 0; k0 < kp; k0 += FIR_CHUNK) {
        const int steps = min(FIR_CHUNK, kp - k0) / 32;
        // stage: plane position q <-> sample X(out0 + p - taps + 1 + k0 + q); the index rule is applied here, once
        const int fill = span + steps * 32;
        const long first = out0 + p - taps + 1 + k0;
        if (wrap) {
            long i = (first + tid) % N;                 // N >= 1 here
            if (i < 0) i += N;
            const long step = FIR_THREADS % N;
            long ii = i;
            for (int q = tid; q < fill; q += FIR_THREADS) {
                put3(xs, SP, q, xb[ii]);
                ii += step;
                if (ii >= N) ii -= N;
            }
        } else {
            for (int q = tid; q < fill; q += FIR_THREADS) {
                const long i = first + q;
                put3(xs, SP, q, (i >= 0 && i < N) ? xb[i] : 0.f);
            }
        }
        __syncthreads();
        if (mine > 0) {                                 // uniform over the wave
            const bf16_t* ab = xs + (wv * 256 + l16 * 16) + g * 8;
            int pk = 0;                                 // the next step to fetch
            auto fetch = [&](short8_t (&f)[3]) {
                const bf16_t* q = tb + (long)(k0 / 32 + pk) * 512;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) f[pl] = ld8(q + pl * PB);
                if (pk + 1 < steps) ++pk;               // past the end: the last fragment again, which nothing uses
            };
            short8_t fb[FIR_DEPTH][3];
#pragma unroll
            for (int d = 0; d < FIR_DEPTH; ++d) fetch(fb[d]);
            for (int kt0 = 0; kt0 < steps; kt0 += FIR_DEPTH) {
#pragma unroll
                for (int d = 0; d < FIR_DEPTH; ++d) {
                    const int kt = kt0 + d;
                    if (kt >= steps) break;             // uniform
#pragma unroll
                    for (int r = 0; r < FIR_RT; ++r) {
                        if (r < mine) {
                            short8_t a[3];
#pragma unroll
                            for (int pl = 0; pl < 3; ++pl) a[pl] = ld8(ab + pl * SP + r * (FIR_WAVES * 256) + kt * 32);
                            part[r] = mfma6(a, fb[d], part[r]);
                        }
                    }
                    fetch(fb[d]);
                }
                if ((kt0 + FIR_DEPTH) % FIR_FLUSH == 0 || kt0 + FIR_DEPTH >= steps) {      // uniform; FIR_CHUNK / 32 is a multiple
#pragma unroll
                    for (int r = 0; r < FIR_RT; ++r) {
                        acc[r] += part[r];
                        part[r] = float4_t{0.f, 0.f, 0.f, 0.f};
                    }
                }
            }
        }
        __syncthreads();                                // every wave has read the planes before the next chunk overwrites them
    }

    // C layout: lane (g, l16) holds frames 4g .. 4g + 3 of column l16 of each of its tiles
    const float s = s_in[b];
    float pk = 0.f;
    bool nan = false;
#pragma unroll
    for (int r = 0; r < FIR_RT; ++r) {
        const int tile = wv + FIR_WAVES * r;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = tile * 256 + (4 * g + i) * 16 + l16;
            if (n >= width) continue;
            float v = 0.f;
            if (n < valid) {
                v = acc[r][i] * s;
                nan |= v != v;
                pk = fmaxf(pk, fabsf(v));
            }
            ob[out0 + n] = v;
        }
    }
    peak_join(pk, nan, peak + b, lane);
}

constexpr int RM_THREADS = 256, RM_PER = 16;
__global__ __launch_bounds__(RM_THREADS) void row_absmax_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                               float* __restrict__ peak) {
    const int b = blockIdx.y;
    const int len = row_len(lens, b, L);
    const long j0 = (long)blockIdx.x * (RM_THREADS * RM_PER) + threadIdx.x;
    if ((long)blockIdx.x * (RM_THREADS * RM_PER) >= len) return;
    float m = 0.f;
    bool nan = false;
#pragma unroll
    for (int r = 0; r < RM_PER; ++r) {
        const long j = j0 + r * RM_THREADS;
        if (j < len) {
            const float v = x[(long)b * x_bs + j];
            nan |= v != v;
            m = fmaxf(m, fabsf(v));
        }
    }
    peak_join(m, nan, peak + b, threadIdx.x & 63);
}

__global__ __launch_bounds__(RM_THREADS) void mix_rows_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                             const float* __restrict__ noise, long n_bs, int Ln, const int* __restrict__ nlens,
                                                             const float* __restrict__ lx, const float* __restrict__ ln,
                                                             const float* __restrict__ snr, float* __restrict__ out, long o_bs) {
    const int b = blockIdx.y;
    const int len = row_len(lens, b, L);
    const int nl = row_len(nlens, b, Ln);
    // effects.py:60-61, 214-217: tgt = Lx - snr, gain = exp((tgt - Ln) ln 10 / 20); the differences in fp32 as torch takes them
    const float gain = (float)exp((double)((lx[b] - snr[b]) - ln[b]) * 0.11512925464970229);
    const long j0 = (long)blockIdx.x * (RM_THREADS * RM_PER) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < RM_PER; ++r) {
        const long j = j0 + r * RM_THREADS;
        if (j >= L) break;
        float v = 0.f;
        if (j < len) {
            v = x[(long)b * x_bs + j];
            if (j < nl) v = __fadd_rn(v, __fmul_rn(gain, noise[(long)b * n_bs + j]));
        }
        out[(long)b * o_bs + j] = v;
    }
}

}  // namespace

extern "C" int mmx_ir_prepare(const float* ir, int64_t ir_bs, int Lir, int B, const int32_t* ir_lens, const int32_t* h_ir_lens, int Lsig,
                              const int32_t* sig_lens, const int32_t* h_sig_lens, const float* drr, int t0, const double* hann,
                              int start_at_max, float* h_out, int64_t h_bs, int32_t* p, float* s, int32_t* taps, float* drr_out,
                              void* table, int kcap, hipStream_t stream) {
    MMX_CHECK_ARG(ir && h_out && p && s && taps && drr_out && table && (const void*)ir != (const void*)h_out);
    MMX_CHECK_ARG((ir_bs == 0 || ir_bs >= Lir) && h_bs >= Lir && t0 >= 0 && t0 <= 4096 && hann);
    if (int rc = rows_form(B, Lir, ir_lens, h_ir_lens, 1)) return rc;
    if (int rc = rows_form(B, Lsig, sig_lens, h_sig_lens, 1)) return rc;
    int most = 0;
    for (int b = 0; b < B; ++b) most = max(most, min(h_ir_lens ? h_ir_lens[b] : Lir, h_sig_lens ? h_sig_lens[b] : Lsig));
    MMX_CHECK_ARG(most <= FIR_MAX_TAPS && kcap > 0 && kcap % 32 == 0 && kcap >= fir_kp(most));
    hipLaunchKernelGGL(ir_prepare_kernel, dim3(B), dim3(PREP_THREADS), 0, stream, ir, (long)ir_bs, Lir, ir_lens, Lsig, sig_lens, drr, t0,
                       hann, start_at_max, h_out, (long)h_bs, p, s, taps, drr_out);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(ir_table_kernel, dim3((unsigned)(((long)kcap * 16 + 255) / 256), B), dim3(256), 0, stream, (const float*)h_out,
                       (long)h_bs, Lir, (const int*)taps, (bf16_t*)table, kcap);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_fir_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const void* table,
                            int kcap, const int32_t* p, const float* s, const int32_t* taps, int wrap, float* out, int64_t o_bs,
                            float* peak, hipStream_t stream) {
    MMX_CHECK_ARG(x && table && p && s && taps && out && peak && x_bs >= L && o_bs >= L && (const void*)x != (const void*)out);
    MMX_CHECK_ARG(kcap >= 32 && kcap % 32 == 0 && kcap <= fir_kp(FIR_MAX_TAPS) && (wrap == 0 || wrap == 1));
    if (int rc = rows_form(B, L, lens, h_lens, 1)) return rc;
    if (hipMemsetAsync(peak, 0, sizeof(float) * B, stream) != hipSuccess) return MMX_EARG;
    const size_t lds = fir_lds(kcap);
    hipLaunchKernelGGL(fir_rows_kernel, dim3((L + FIR_NOUT - 1) / FIR_NOUT, B), dim3(FIR_THREADS), lds, stream, x, (long)x_bs, L, lens,
                       (const bf16_t*)table, kcap, p, s, taps, wrap, out, (long)o_bs, peak);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_row_absmax(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, float* peak, hipStream_t stream) {
    MMX_CHECK_ARG(x && peak && B > 0 && B <= 65535 && L > 0 && x_bs >= L);
    if (hipMemsetAsync(peak, 0, sizeof(float) * B, stream) != hipSuccess) return MMX_EARG;
    hipLaunchKernelGGL(row_absmax_kernel, dim3((L + RM_THREADS * RM_PER - 1) / (RM_THREADS * RM_PER), B), dim3(RM_THREADS), 0, stream, x,
                       (long)x_bs, L, lens, peak);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_mix_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const float* noise, int64_t n_bs, int Ln,
                            const int32_t* nlens, const float* lx, const float* ln, const float* snr, float* out, int64_t o_bs,
                            hipStream_t stream) {
    MMX_CHECK_ARG(x && noise && lx && ln && snr && out && B > 0 && B <= 65535 && L > 0 && Ln > 0 && x_bs >= L && n_bs >= Ln && o_bs >= L);
    hipLaunchKernelGGL(mix_rows_kernel, dim3((L + RM_THREADS * RM_PER - 1) / (RM_THREADS * RM_PER), B), dim3(RM_THREADS), 0, stream, x,
                       (long)x_bs, L, lens, noise, (long)n_bs, Ln, nlens, lx, ln, snr, out, (long)o_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
