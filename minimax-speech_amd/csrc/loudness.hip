// ITU-R BS.1770-4 integrated loudness of a ragged batch of mono fp32 rows for gfx950 (dac-vae/audiotools/core/loudness.py Meter /
// LoudnessMixin.loudness, core/effects.py:181-220 normalize / ensure_max_of_audio), without a host sync: K-weighted sub-block
// energies and sample peaks (mmx_kweight_blocks), two-stage gating and the gain (mmx_loudness_gate), the gain applied
// (mmx_scale_rows).  mmx/loudness.py states the definition and builds the tables.
//
// The K-weighting is two biquads in series, an exact 4th-order linear recursion (transposed direct form II, state s[4]):
//     y1 = b10 x + s0;  s0 = b11 x - a11 y1 + s1;  s1 = b12 x - a12 y1;    y2 = b20 y1 + s2;  s2 = b21 y1 - a21 y2 + s3;  s3 = b22 y1 - a22 y2
// With x = 0 the state moves by a constant 4 x 4 matrix A, so the state after a run of samples is A^n (state before) + (state the
// run reaches from zero).  That is what makes it parallel:
//   * a row is cut into sub-blocks of S = rate / 10 samples (a 400 ms block is four of them), a sub-block into nseg segments of
//     `seg` samples (S = nseg * seg, nseg <= 127; both depend on the rate only).  One workgroup owns one sub-block, one lane one
//     segment; the sub-block's samples go through LDS (coalesced loads; a lane walking its segment straight from HBM is not);
//   * ends launch: every lane walks its segment from zero state, a Hillis-Steele scan over the lanes with A^(seg 2^k) gives the state
//     the sub-block reaches from zero;  carry launch: one wave per row runs s <- A^S s + end over the row's sub-blocks, which leaves
//     every sub-block's true initial state;  energy launch: the same walk and scan, now seeded with that state, give every lane its
//     true initial state, and a second walk from it sums y2^2 over the segment; the lanes' sums are added in a fixed tree.
// State, filter output and energy sums are fp64: the high pass has a double pole of radius 0.985 .. 0.995, whose fp32 recursion
// is what the reference's CPU path loses up to 7e-4 dB to; fp64 FMAs leave the whole meter at float64's own rounding, and the kernel is
// bound by the dependent chain of the recursion (two FMAs per section and sample), not by the fp64 rate.
// Every value of a row is a function of that row's samples, length and rate only: not of the batch, the row index or the grid.
#include "common.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int KW_THREADS = 128;                         // lanes 0 .. nseg - 1 own a segment, lane l of the scan holds the state BEFORE segment l
constexpr int KW_SEG_MAX = 64;
constexpr int KW_NSEG_MAX = KW_THREADS - 1;
constexpr int KW_XS = KW_NSEG_MAX * (KW_SEG_MAX + 1);   // staged samples, segments an odd number of words apart (no bank conflicts)
constexpr int KW_STEPS = 7;                             // 2^7 = 128 scan entries; tab = 10 coefficients, A^(seg 2^k) for k < 7, A^S
constexpr double MIN_LOUDNESS = -70.0;

// LoudnessMixin.loudness: a clip shorter than 0.5 s is zero padded by int((0.5 - n / rate) * rate) samples (the same float64
// operations as mmx/loudness.py padded_len: one division, one subtraction, one product, nothing to contract)
__host__ __device__ __forceinline__ long kw_padded(long n, int rate) {
    const double dur = (double)n / (double)rate;
    return dur < 0.5 ? n + (long)((0.5 - dur) * (double)rate) : n;
}
// sub-blocks of a row: the blocks are [j S, j S + 4 S), j < nsub - 3.  pad (julius.core.unfold): ceil(n' / S); drop (BS.1770): n' / S
__host__ __device__ __forceinline__ long kw_nsub(long n, int rate, int S, int partial) {
    const long np = kw_padded(n, rate);
    return partial == MMX_LOUD_DROP ? np / S : (np + S - 1) / S;
}

struct Biquads {
    double b10, b11, b12, a11, a12, b20, b21, b22, a21, a22;
    __device__ __forceinline__ explicit Biquads(const double* t)
        : b10(t[0]), b11(t[1]), b12(t[2]), a11(t[3]), a12(t[4]), b20(t[5]), b21(t[6]), b22(t[7]), a21(t[8]), a22(t[9]) {}
    __device__ __forceinline__ double step(double x, double (&s)[4]) const {
        const double y1 = __builtin_fma(b10, x, s[0]);
        s[0] = __builtin_fma(b11, x, __builtin_fma(-a11, y1, s[1]));
        s[1] = __builtin_fma(b12, x, -a12 * y1);
        const double y2 = __builtin_fma(b20, y1, s[2]);
        s[2] = __builtin_fma(b21, y1, __builtin_fma(-a21, y2, s[3]));
        s[3] = __builtin_fma(b22, y1, -a22 * y2);
        return y2;
    }
};

// v += P u, P row-major 4 x 4 (a uniform address: scalar loads)
__device__ __forceinline__ void madd4(double (&v)[4], const double* __restrict__ P, const double (&u)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        double a = v[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) a = __builtin_fma(P[4 * r + c], u[c], a);
        v[r] = a;
    }
}

// ENERGY = false: work[b][i][0..3] <- the state sub-block i reaches from zero, work[b][i][4] <- max |x| over its samples below len.
// ENERGY = true:  work[b][i][0..3] holds the sub-block's true initial state; energy[b][i] <- sum of y2^2 over its samples below n' (0 beyond the
// row's sub-blocks).
template <bool ENERGY>
__global__ __launch_bounds__(KW_THREADS) void kweight_kernel(const float* __restrict__ wave, long w_bs, int L, const int* __restrict__ lens,
                                                            int rate, int S, int seg, int partial, const double* __restrict__ tab,
                                                            double* __restrict__ work, int cap, double* __restrict__ energy, long e_bs) {
    __shared__ float xs[KW_XS];
    __shared__ double sc[KW_THREADS][4];
    __shared__ double red[KW_THREADS];
    const int tid = threadIdx.x, b = blockIdx.y, i = blockIdx.x;            // i < cap
    const int len = row_len(lens, b, L);
    const bool live = i < kw_nsub(len, rate, S, partial);
    const long s0 = (long)i * S;
    double* wk = work + ((long)b * cap + i) * 5;
    if (ENERGY && !live) {                                                   // uniform over the workgroup
        if (tid == 0) energy[(long)b * e_bs + i] = 0.0;
        return;
    }
    const int nseg = S / seg, dp = seg | 1;
    const float* x = wave + (long)b * w_bs;
    float pk = 0.f;
    for (int q = tid; q < S; q += KW_THREADS) {
        const long smp = s0 + q;
        const float v = smp < len ? x[smp] : 0.f;                           // the padding comes from len, never from memory
        const int sg = q / seg;
        xs[sg * dp + (q - sg * seg)] = v;
        pk = fmaxf(pk, fabsf(v));
    }
    __syncthreads();

    const Biquads f(tab);
    const float* mine = xs + tid * dp;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (tid < nseg)
        for (int t = 0; t < seg; ++t) f.step((double)mine[t], z);
    // scan entry l: the state before segment l.  Entry 0 is the sub-block's initial state, entry l + 1 starts as lane l's zero-state end
    if (tid + 1 < KW_THREADS) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[tid + 1][r] = z[r];
    }
    if (tid == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[0][r] = ENERGY ? wk[r] : 0.0;
    }
    __syncthreads();
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = sc[tid][r];
    for (int k = 0; (1 << k) <= nseg; ++k) {                                // entries 0 .. nseg
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) sc[tid][r] = v[r];
        __syncthreads();
        if (tid >= (1 << k)) {
            double u[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) u[r] = sc[tid - (1 << k)][r];
            madd4(v, tab + 10 + 16 * k, u);
        }
    }

    if constexpr (!ENERGY) {
        red[tid] = (double)pk;
        __syncthreads();
        for (int h = KW_THREADS / 2; h > 0; h >>= 1) {
            if (tid < h) red[tid] = fmax(red[tid], red[tid + h]);
            __syncthreads();
        }
        if (tid == nseg) {                                                   // entry nseg: the state after the last segment
#pragma unroll
            for (int r = 0; r < 4; ++r) wk[r] = live ? v[r] : 0.0;
            wk[4] = red[0];
        }
    } else {
        // julius.core.unfold pads the FILTERED signal: the filter's ringing past the row's n' samples is not part of the tail block
        const long left = kw_padded(len, rate) - (s0 + (long)tid * seg);
        const int lim = (int)max(0L, min((long)seg, left));
        double acc = 0.0;
        if (tid < nseg)
            for (int t = 0; t < lim; ++t) {
                const double y = f.step((double)mine[t], v);
                acc = __builtin_fma(y, y, acc);
            }
        red[tid] = acc;
        __syncthreads();
        for (int h = KW_THREADS / 2; h > 0; h >>= 1) {                       // a fixed tree: the sum's bits depend on the row alone
            if (tid < h) red[tid] += red[tid + h];
            __syncthreads();
        }
        if (tid == 0) energy[(long)b * e_bs + i] = red[0];
    }
}

// One wave per row: the zero-state ends of the row's sub-blocks become their true initial states (s <- A^S s + end, in order), and
// the sub-blocks' peaks the row's peak.
__global__ __launch_bounds__(64) void kweight_carry_kernel(int L, const int* __restrict__ lens, int rate, int S, int partial,
                                                          const double* __restrict__ tab, double* __restrict__ work, int cap,
                                                          float* __restrict__ peak) {
    __shared__ double buf[64][4];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int len = row_len(lens, b, L);
    const int nsub = (int)min((long)cap, kw_nsub(len, rate, S, partial));
    double* wk = work + (long)b * cap * 5;
    const double* AS = tab + 10 + 16 * KW_STEPS;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    double pk = 0.0;
    for (int j = lane; j < cap; j += 64) pk = fmax(pk, wk[(long)j * 5 + 4]);   // sub-blocks at or beyond len hold 0
    for (int base = 0; base < nsub; base += 64) {
        const int j = base + lane;
        if (j < nsub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) buf[lane][r] = wk[(long)j * 5 + r];
        }
        __syncthreads();
        if (lane == 0) {
            const int m = min(64, nsub - base);
            for (int t = 0; t < m; ++t) {
                double e[4], n[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    e[r] = buf[t][r];
                    buf[t][r] = s[r];
                    n[r] = e[r];
                }
                madd4(n, AS, s);
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = n[r];
            }
        }
        __syncthreads();
        if (j < nsub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) wk[(long)j * 5 + r] = buf[lane][r];
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) pk = fmax(pk, __shfl_xor(pk, o, 64));
    if (lane == 0) peak[b] = (float)pk;                                      // exact: the maximum of fp32 values
}

struct GateArgs {
    double G[MMX_LOUD_MAX_CH];
};

// One wave per clip of nch adjacent rows: Meter.integrated_loudness's two-stage gating over the blocks j < nsub - 3, block j the
// sum of sub-blocks j .. j + 3.
__global__ __launch_bounds__(64) void loudness_gate_kernel(const double* __restrict__ energy, long e_bs, const float* __restrict__ peak,
                                                          const int* __restrict__ lens, int L, int nch, GateArgs ga, int rate, int S,
                                                          int partial, int cap, float* __restrict__ lufs, int want_gain, float target_db,
                                                          float max_peak, float* __restrict__ gain, unsigned char* __restrict__ mask,
                                                          long mask_bs) {
    const int lane = threadIdx.x, clip = blockIdx.x, row0 = clip * nch;
    const int len = row_len(lens, row0, L);
    const int F = (int)min((long)cap, kw_nsub(len, rate, S, partial)) - 3;
    const double den = 0.4 * (double)rate;
    const double* e = energy + (long)row0 * e_bs;

    auto block = [&](int j, double (&z)[MMX_LOUD_MAX_CH]) {                  // -> l[j]
        double w = 0.0;
#pragma unroll
        for (int c = 0; c < MMX_LOUD_MAX_CH; ++c) {
            z[c] = 0.0;
            if (c < nch) {
                const double* ec = e + (long)c * e_bs + j;
                z[c] = (((ec[0] + ec[1]) + ec[2]) + ec[3]) / den;
                w = __builtin_fma(ga.G[c], z[c], w);
            }
        }
        return -0.691 + 10.0 * log10(w);
    };
    auto gated = [&](double thr, bool write_mask, int& count) {              // -> loudness of the mean over the blocks above thr
        double sum[MMX_LOUD_MAX_CH] = {};
        double cnt = 0.0;
        for (int j = lane; j < F; j += 64) {
            double z[MMX_LOUD_MAX_CH];
            const double l = block(j, z);
            const bool keep = l > MIN_LOUDNESS && l > thr;
            if (keep) {
                cnt += 1.0;
#pragma unroll
                for (int c = 0; c < MMX_LOUD_MAX_CH; ++c) sum[c] += z[c];
            }
            if (write_mask) mask[(long)clip * mask_bs + j] = keep ? 1 : 0;
        }
        cnt = wave_sum_f64(cnt);
        double w = 0.0;
#pragma unroll
        for (int c = 0; c < MMX_LOUD_MAX_CH; ++c)
            if (c < nch) w = __builtin_fma(ga.G[c], wave_sum_f64(sum[c]) / cnt, w);
        count = (int)cnt;
        return -0.691 + 10.0 * log10(w);
    };

    int n1 = 0, n2 = 0;
    const double gamma_r = gated(MIN_LOUDNESS, false, n1) - 10.0;
    double lu = MIN_LOUDNESS;
    if (n1 > 0) {
        const double v = gated(gamma_r, mask != nullptr, n2);
        if (n2 > 0 && v > MIN_LOUDNESS) lu = v;                              // no block kept, or below the floor: MIN_LOUDNESS
    } else if (mask != nullptr) {
        for (int j = lane; j < F; j += 64) mask[(long)clip * mask_bs + j] = 0;
    }
    if (lane != 0) return;
    lufs[clip] = (float)lu;
    if (want_gain) {
#pragma clang fp contract(off)
        float pk = 0.f;
        for (int c = 0; c < nch; ++c) pk = fmaxf(pk, peak[row0 + c]);
        const double gd = exp(((double)target_db - lu) * (2.302585092994046 / 20.0));
        float g = (float)gd;
        if (gd * (double)pk > (double)max_peak) {                            // ensure_max_of_audio
            g = (float)((double)max_peak / (double)pk);
            // the scaled peak itself never passes max_peak: one ulp down (g is positive and finite here)
            if (g * pk > max_peak) g = __uint_as_float(__float_as_uint(g) - 1u);
        }
        gain[clip] = g;
    }
}

constexpr int SR_THREADS = 256, SR_PER = 4;

__global__ __launch_bounds__(SR_THREADS) void scale_rows_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                               const float* __restrict__ gain, int nch, float* __restrict__ out, long o_bs) {
    const int b = blockIdx.y;
    const int len = row_len(lens, b, L);
    const float g = gain[b / nch];
    const long j0 = (long)blockIdx.x * (SR_THREADS * SR_PER) + threadIdx.x;
#pragma unroll
    for (int r = 0; r < SR_PER; ++r) {
        const long j = j0 + r * SR_THREADS;
        if (j < len) out[(long)b * o_bs + j] = x[(long)b * x_bs + j] * g;
    }
}

// S of a supported rate (K = int(0.4 rate) = 4 int(0.4 rate 0.25), the arithmetic of the reference's Meter), 0 otherwise
int kw_sub_block(int rate) {
    const int K = (int)(0.4 * rate), S = (int)(0.4 * rate * 0.25);
    return (S > 0 && K == 4 * S) ? S : 0;
}
// sub-blocks the longest row of L columns can have (the 0.5 s rule pads to at most rate / 2 + 1 samples)
long kw_cap(int L, int rate, int S) { return (max((long)L, (long)rate / 2 + 1) + S - 1) / S; }

}  // namespace

extern "C" int mmx_kweight_blocks(const float* wave, int64_t w_bs, int L, int B, const int32_t* lens, int rate, int partial,
                                  const double* tab, int seg, double* work, int cap, double* energy, int64_t e_bs, float* peak,
                                  hipStream_t stream) {
    MMX_CHECK_ARG(wave && tab && work && energy && peak && B > 0 && B <= 65535 && L > 0 && w_bs >= L);
    MMX_CHECK_ARG(partial == MMX_LOUD_PAD || partial == MMX_LOUD_DROP);
    const int S = rate > 0 ? kw_sub_block(rate) : 0;
    MMX_CHECK_ARG(S > 0 && seg > 0 && seg <= KW_SEG_MAX && S % seg == 0 && S / seg <= KW_NSEG_MAX);
    MMX_CHECK_ARG(cap >= kw_cap(L, rate, S) && cap <= INT32_MAX / 8 && e_bs >= cap);
    const dim3 grid(cap, B);
    hipLaunchKernelGGL(kweight_kernel<false>, grid, dim3(KW_THREADS), 0, stream, wave, (long)w_bs, L, lens, rate, S, seg, partial, tab, work,
                       cap, energy, (long)e_bs);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(kweight_carry_kernel, dim3(B), dim3(64), 0, stream, L, lens, rate, S, partial, tab, work, cap, peak);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(kweight_kernel<true>, grid, dim3(KW_THREADS), 0, stream, wave, (long)w_bs, L, lens, rate, S, seg, partial, tab, work,
                       cap, energy, (long)e_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_loudness_gate(const double* energy, int64_t e_bs, int cap, const float* peak, const int32_t* lens, int L, int nclips,
                                 int nch, const double* G, int rate, int partial, float* lufs, int want_gain, float target_db,
                                 float max_peak, float* gain, uint8_t* mask, int64_t mask_bs, hipStream_t stream) {
    MMX_CHECK_ARG(energy && peak && lufs && nclips > 0 && nclips <= 65535 && nch >= 1 && nch <= MMX_LOUD_MAX_CH && L > 0);
    MMX_CHECK_ARG(partial == MMX_LOUD_PAD || partial == MMX_LOUD_DROP);
    const int S = rate > 0 ? kw_sub_block(rate) : 0;
    MMX_CHECK_ARG(S > 0 && cap >= kw_cap(L, rate, S) && e_bs >= cap && (!mask || mask_bs >= cap - 3));
    MMX_CHECK_ARG(!want_gain || (gain && max_peak > 0.f));
    static const double bs1770[MMX_LOUD_MAX_CH] = {1.0, 1.0, 1.0, 1.41, 1.41};
    GateArgs ga;
    for (int c = 0; c < MMX_LOUD_MAX_CH; ++c) ga.G[c] = G ? (c < nch ? G[c] : 0.0) : bs1770[c];
    hipLaunchKernelGGL(loudness_gate_kernel, dim3(nclips), dim3(64), 0, stream, energy, (long)e_bs, peak, lens, L, nch, ga, rate, S, partial,
                       cap, lufs, want_gain, target_db, max_peak, gain, mask, (long)mask_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_scale_rows(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const float* gain, int nch, float* out,
                              int64_t o_bs, hipStream_t stream) {
    MMX_CHECK_ARG(x && gain && out && B > 0 && B <= 65535 && L > 0 && x_bs >= L && o_bs >= L && nch >= 1);
    const dim3 grid((L + SR_THREADS * SR_PER - 1) / (SR_THREADS * SR_PER), B);
    hipLaunchKernelGGL(scale_rows_kernel, grid, dim3(SR_THREADS), 0, stream, x, (long)x_bs, L, lens, gain, nch, out, (long)o_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
