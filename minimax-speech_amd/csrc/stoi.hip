// Short-time objective intelligibility (STOI, Taal et al. 2011) and extended STOI (Jensen and Taal 2016) between a reference x and an
// estimate y at 10 kHz, for a ragged batch of mono fp32 rows of equal per-clip length, for gfx950: what the reference's
// audiotools.metrics.quality.stoi asks a host library for one clip at a time, without a host sync, without atomics and without a
// spectrogram in memory.  mmx/stoi.py builds the tables and states the definition (frames of 256 samples at hop 128 that start at
// i < len - 256, a 512-point DFT, 15 third-octave bands, segments of 30 frames).
//
//   mmx_stoi_select  stoi_energy_kernel, one wave per frame of the reference: e = 20 log10(|w x| + EPS), fp32 products, fp64 sum
//                    (4 per lane, then a fixed butterfly).  stoi_scan_kernel, one workgroup per clip: the clip's maximum, the keep
//                    mask max - 40 - e < 0, and its exclusive scan (ballot per wave, wave totals in wave order, 256 frames per
//                    round) as the map kept index -> source frame, and the kept count F.
//   mmx_stoi_bands   One workgroup takes 16 spectral frames of one clip through BOTH signals on the functions of spec_tile.h.  F and
//                    the map are read from device memory; the grid is sized by the capacity, workgroups past the clip's F - 1 frames
//                    exit.
//                    stage 0  the silence-removed signal is never stored: a sample p of it is the sum of at most two windowed source
//                             samples, of kept frames p / 128 - 1 and p / 128 in that order, found through the map (the overlap-add
//                             as a gather) -> LDS as three bf16 planes, hop-sized chunks 16 elements apart (the header's GAP).
//                    stage 1  the DFT as the six-term bf16 MFMA product, both signals on one load of the basis (spec_dft_tile<2, GAP>).
//                             The basis is that of a 512-point DFT with the window followed by 256 zeros; its zero half (which adds
//                             exact zeros) is left out of the table, so K = 256.  Only the 14 bin tiles below bin 224 are computed:
//                             the last band ends at bin 219.  |X|^2 (fp32) -> magnitude planes.
//                    stage 2  one spec_mel_tile per signal against the 0 / 1 band table (16 rows: 15 bands and a zero row), sqrt ->
//                             env fp32 [B][2][cap][16], the only intermediate in memory.
//   mmx_stoi_score   stoi_score_kernel, 16 segments of one clip per workgroup (their 45 frames of both envelopes in LDS, every term
//                    fp64): standard, one thread per (segment, band): scale, clip, remove the means, normalise, correlate;
//                    extended, rows (one thread per (segment, band): mean and norm) then columns (one thread per (segment, frame)).
//                    The workgroup's terms are added in a fixed order -> work[b][tile]; stoi_finish_kernel, one wave per clip, adds
//                    the clip's own tiles in a fixed order, divides, and writes 1e-5 where the clip has fewer than 30 frames.
// A clip's numbers are a function of its own samples and length: not of the batch, the row index, the capacity or the grid.
#include "spec_tile.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int ST_FRAME = 256, ST_HOP = 128, ST_SEG = 30, ST_BANDS = 15;
constexpr int ST_WAVES = 8, ST_THREADS = ST_WAVES * 64;
constexpr int ST_GAP = 16;                              // elements between hop-sized chunks of a sample plane
constexpr int ST_NBP = 288;                             // 257 bins rounded up to 32: the row count the tables are built with
constexpr int ST_BT = 14;                               // bin tiles computed: the last band ends at bin 219 <= 16 * 14
constexpr int ST_MS = 16 * ST_BT + 8;                   // magnitude row stride: 16-byte aligned rows, an odd number of 16-byte slots
constexpr int ST_SPAN = 15 * ST_HOP + ST_FRAME;         // samples under 16 frames
constexpr int ST_SP = ST_SPAN + ST_GAP * (ST_SPAN / ST_HOP);   // = spec_plane<ST_GAP>(ST_SPAN, ST_HOP)
constexpr size_t ST_LDS = (size_t)2 * 3 * ST_SP * sizeof(bf16_t) + (size_t)2 * 3 * 16 * ST_MS * sizeof(bf16_t);
constexpr int SC_SEGS = 16, SC_ROWS = SC_SEGS + ST_SEG - 1, SC_THREADS = 256, SC_LD = 17;
constexpr int SC_COLS = SC_SEGS * ST_SEG;               // (segment, frame) pairs of a workgroup
constexpr double ST_EPS = 2.220446049250313e-16;        // 2^-52
constexpr double ST_RANGE = 40.0;
constexpr double ST_CLIP = 6.623413251903491;           // 1 + 10^(15 / 20)
static_assert(ST_SPAN % ST_HOP == 0 && SC_THREADS == 16 * SC_SEGS);

// frames of a clip of len samples: starts 0, 128, .. strictly below len - 256
__host__ __device__ __forceinline__ int st_frames(int len) { return len > ST_FRAME ? (len - ST_FRAME + ST_HOP - 1) / ST_HOP : 0; }
__host__ __device__ __forceinline__ int st_seg_tiles(int cap) { return cap > ST_SEG ? (cap - ST_SEG + SC_SEGS - 1) / SC_SEGS : 1; }

__global__ __launch_bounds__(256) void stoi_energy_kernel(const float* __restrict__ ref, long r_bs, int L, const int* __restrict__ lens,
                                                         const float* __restrict__ window, double* __restrict__ energy, int cap) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int f = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int len = row_len(lens, b, L);
    if (f >= min(st_frames(len), cap)) return;          // uniform over the wave; 128 f + 255 < len - 1
    const float* r = ref + (long)b * r_bs + (long)f * ST_HOP;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < ST_FRAME / 64; ++i) {
        const float v = __fmul_rn(window[lane + 64 * i], r[lane + 64 * i]);
        s += (double)v * (double)v;
    }
    s = wave_sum_f64(s);
    if (lane == 0) energy[(long)b * cap + f] = 20.0 * log10(sqrt(s) + ST_EPS);
}

// mask [B][cap]: 1 kept, 0 silent or past the clip's frames;  map [B][cap]: source frame of kept frame i, -1 from F on;  kept [B]: F
__global__ __launch_bounds__(256) void stoi_scan_kernel(const double* __restrict__ energy, int L, const int* __restrict__ lens,
                                                       unsigned char* __restrict__ mask, int* __restrict__ map, int* __restrict__ kept,
                                                       int cap) {
    __shared__ double wmax[4];
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    const int len = row_len(lens, b, L);
    const int n = min(st_frames(len), cap);
    const double* e = energy + (long)b * cap;
    double m = -INFINITY;
    for (int i = tid; i < n; i += 256) m = fmax(m, e[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
    if (lane == 0) wmax[wv] = m;
    __syncthreads();
    const double thr = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3])) - ST_RANGE;
    int base = 0;
    for (int c0 = 0; c0 < cap; c0 += 256) {             // uniform over the workgroup
        const int i = c0 + tid;
        const bool k = i < n && thr - e[i] < 0.0;
        const unsigned long long bal = __ballot(k);
        if (lane == 0) wtot[wv] = __popcll(bal);
        __syncthreads();
        int off = base, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wv) off += wtot[w];
            tot += wtot[w];
        }
        if (i < cap) mask[(long)b * cap + i] = k ? 1 : 0;
        if (k) map[(long)b * cap + off + __popcll(bal & ((1ull << lane) - 1ull))] = i;      // off + .. <= i < cap
        base += tot;
        __syncthreads();
    }
    for (int i = base + tid; i < cap; i += 256) map[(long)b * cap + i] = -1;
    if (tid == 0) kept[b] = base;
}

// basis: [3 planes][2 * ST_NBP / 16 tiles][256 / 32][64][8], tile 2j = window * cos of bins 16j .. 16j + 15, tile 2j + 1 = window * sin
// filt : [3 planes][1 tile][ST_NBP / 32][64][8], the 0 / 1 band table
// env  : [B][2][cap][16], signal 0 the reference, 1 the estimate; rows at and past the clip's F - 1 frames are not written
__global__ __launch_bounds__(ST_THREADS) void stoi_bands_kernel(const float* __restrict__ est, long e_bs, const float* __restrict__ ref,
                                                               long r_bs, int L, const int* __restrict__ lens,
                                                               const float* __restrict__ window, const int* __restrict__ map,
                                                               const int* __restrict__ kept, const bf16_t* __restrict__ basis,
                                                               const bf16_t* __restrict__ filt, float* __restrict__ env, int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);       // [2][3][ST_SP]
    bf16_t* mg = xs + 2 * 3 * ST_SP;                    // [2][3][16][ST_MS]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * 16;
    const int len = row_len(lens, b, L);
    const int nf = min(st_frames(len), cap);            // source frames: a map entry is held below it, whatever the workspace holds
    const int F = min(max(kept[b], 0), nf);
    const int T = max(F - 1, 0);                        // frames of the (F + 1) * 128 samples that F kept frames rebuild
    if (t0 >= T) return;                                // uniform over the workgroup
    const int* mp = map + (long)b * cap;
    const float* xr = ref + (long)b * r_bs;
    const float* yr = est + (long)b * e_bs;

    for (int q = tid; q < ST_SPAN; q += ST_THREADS) {
        const int p = t0 * ST_HOP + q, k1 = p >> 7, o1 = p & (ST_HOP - 1);
        float vx = 0.f, vy = 0.f;
        if (k1 >= 1 && k1 - 1 < F) {                    // the second half of kept frame k1 - 1, added first: ascending frame order
            const long s = (long)min(max(mp[k1 - 1], 0), nf - 1) * ST_HOP + ST_HOP + o1;
            const float w = window[ST_HOP + o1];
            vx = __fmul_rn(w, xr[s]);
            vy = __fmul_rn(w, yr[s]);
        }
        if (k1 < F) {                                   // the first half of kept frame k1
            const long s = (long)min(max(mp[k1], 0), nf - 1) * ST_HOP + o1;
            const float w = window[o1];
            vx = __fadd_rn(vx, __fmul_rn(w, xr[s]));
            vy = __fadd_rn(vy, __fmul_rn(w, yr[s]));
        }
        const int pos = spec_pos<ST_GAP>(q, ST_HOP);
        put3(xs, ST_SP, pos, vx);
        put3(xs + 3 * ST_SP, ST_SP, pos, vy);
    }
    __syncthreads();

    const bf16_t* const sig[2] = {xs, xs + 3 * ST_SP};
    constexpr long PB = (long)2 * ST_NBP * ST_FRAME;    // elements per basis plane
    for (int j = wv; j < ST_BT; j += ST_WAVES) {
        float4_t re[2], im[2];
        spec_dft_tile<2, ST_GAP>(sig, ST_SP, ST_HOP, basis, PB, ST_FRAME / 32, j, lane, re, im);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                spec_store3(mg + s * 3 * 16 * ST_MS, ST_MS, 4 * g + r, j * 16 + l16, re[s][r] * re[s][r] + im[s][r] * im[s][r]);
    }
    __syncthreads();

    if (wv < 2) {                                       // wave 0 the reference, wave 1 the estimate
        const float4_t acc = spec_mel_tile(mg + wv * 3 * 16 * ST_MS, ST_MS, filt, (long)16 * ST_NBP, ST_BT / 2, 0, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = t0 + 4 * g + r;
            if (t < T) env[(((long)b * 2 + wv) * cap + t) * 16 + l16] = sqrtf(fmaxf(acc[r], 0.f));
        }
    }
}

// the workgroup's terms part[0 .. n) added by wave 0: lane l takes l, l + 64, .. in order, then the butterfly
__device__ __forceinline__ void score_reduce(const double* part, int n, int tid, double* dst) {
    if (tid < 64) {
        double s = 0.0;
        for (int i = tid; i < n; i += 64) s += part[i];
        s = wave_sum_f64(s);
        if (tid == 0) *dst = s;
    }
}

// work [B][wcap]: the sum over the tile's segments of the correlations (standard: over the 15 bands; extended: over the 30 columns)
template <bool EXT>
__global__ __launch_bounds__(SC_THREADS) void stoi_score_kernel(const float* __restrict__ env, int cap, const int* __restrict__ kept,
                                                               double* __restrict__ work, int wcap) {
    __shared__ float ev[2][SC_ROWS][SC_LD];
    __shared__ double part[EXT ? SC_COLS : SC_THREADS];
    __shared__ double rowstat[EXT ? 2 * SC_SEGS * 16 * 2 : 1];
    const int tid = threadIdx.x, b = blockIdx.y, m0 = blockIdx.x * SC_SEGS;
    const int T = min(max(kept[b] - 1, 0), cap - 1);
    const int J = T - (ST_SEG - 1);                     // segments: frames s .. s + 29 for s = 0 .. J - 1
    if (m0 >= J || (int)blockIdx.x >= wcap) return;     // uniform over the workgroup
    for (int i = tid; i < 2 * SC_ROWS * 16; i += SC_THREADS) {
        const int s = i / (SC_ROWS * 16), row = (i / 16) % SC_ROWS, col = i & 15, t = m0 + row;
        ev[s][row][col] = t < T ? env[(((long)b * 2 + s) * cap + t) * 16 + col] : 0.f;
    }
    __syncthreads();
    const int seg = tid >> 4, k = tid & 15;
    const bool live = k < ST_BANDS && m0 + seg < J;

    if constexpr (!EXT) {
        double val = 0.0;
        if (live) {
            double sxx = 0.0, syy = 0.0;
            for (int i = 0; i < ST_SEG; ++i) {
                const double x = (double)ev[0][seg + i][k], y = (double)ev[1][seg + i][k];
                sxx += x * x;
                syy += y * y;
            }
            const double c = sqrt(sxx) / (sqrt(syy) + ST_EPS);
            double mx = 0.0, my = 0.0;
            for (int i = 0; i < ST_SEG; ++i) {
                const double x = (double)ev[0][seg + i][k], y = (double)ev[1][seg + i][k];
                mx += x;
                my += fmin(c * y, x * ST_CLIP);
            }
            mx /= ST_SEG;
            my /= ST_SEG;
            double cxx = 0.0, cyy = 0.0, cxy = 0.0;
            for (int i = 0; i < ST_SEG; ++i) {
                const double x = (double)ev[0][seg + i][k], y = (double)ev[1][seg + i][k];
                const double dx = x - mx, dy = fmin(c * y, x * ST_CLIP) - my;
                cxx += dx * dx;
                cyy += dy * dy;
                cxy += dx * dy;
            }
            val = cxy / ((sqrt(cxx) + ST_EPS) * (sqrt(cyy) + ST_EPS));
        }
        part[tid] = val;
        __syncthreads();
        score_reduce(part, SC_THREADS, tid, work + (long)b * wcap + blockIdx.x);
    } else {
        if (live) {                                     // rows: mean and norm + EPS of the band over the segment's 30 frames
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                double m = 0.0, q = 0.0;
                for (int i = 0; i < ST_SEG; ++i) m += (double)ev[s][seg + i][k];
                m /= ST_SEG;
                for (int i = 0; i < ST_SEG; ++i) {
                    const double d = (double)ev[s][seg + i][k] - m;
                    q += d * d;
                }
                rowstat[((s * SC_SEGS + seg) * 16 + k) * 2] = m;
                rowstat[((s * SC_SEGS + seg) * 16 + k) * 2 + 1] = sqrt(q) + ST_EPS;
            }
        }
        __syncthreads();
        for (int it = tid; it < SC_COLS; it += SC_THREADS) {       // columns: one (segment, frame) per thread
            const int sg = it / ST_SEG, j = it - sg * ST_SEG;
            double val = 0.0;
            if (m0 + sg < J) {
                double a[2][ST_BANDS];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    double m = 0.0, q = 0.0;
#pragma unroll
                    for (int kk = 0; kk < ST_BANDS; ++kk) {
                        const double* rs = rowstat + ((s * SC_SEGS + sg) * 16 + kk) * 2;
                        a[s][kk] = ((double)ev[s][sg + j][kk] - rs[0]) / rs[1];
                        m += a[s][kk];
                    }
                    m /= ST_BANDS;
#pragma unroll
                    for (int kk = 0; kk < ST_BANDS; ++kk) {
                        a[s][kk] -= m;
                        q += a[s][kk] * a[s][kk];
                    }
                    q = sqrt(q) + ST_EPS;
#pragma unroll
                    for (int kk = 0; kk < ST_BANDS; ++kk) a[s][kk] /= q;
                }
#pragma unroll
                for (int kk = 0; kk < ST_BANDS; ++kk) val += a[0][kk] * a[1][kk];
            }
            part[it] = val;
        }
        __syncthreads();
        score_reduce(part, SC_COLS, tid, work + (long)b * wcap + blockIdx.x);
    }
}

// One wave per clip: the clip's own tiles of work added - lane l takes tiles l, l + 64, .. in order, then the butterfly
__global__ __launch_bounds__(64) void stoi_finish_kernel(const double* __restrict__ work, int wcap, int cap, const int* __restrict__ kept,
                                                        int extended, double* __restrict__ out, int* __restrict__ frames) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int T = min(max(kept[b] - 1, 0), cap - 1);
    const int J = T - (ST_SEG - 1);
    const int tiles = J > 0 ? min(wcap, (J + SC_SEGS - 1) / SC_SEGS) : 0;
    double s = 0.0;
    for (int i = lane; i < tiles; i += 64) s += work[(long)b * wcap + i];
    s = wave_sum_f64(s);
    if (lane == 0) {
        out[b] = J > 0 ? (extended ? s / ST_SEG / (double)J : s / ((double)J * ST_BANDS)) : 1e-5;
        frames[b] = T;
    }
}

// what mmx_stoi_select and mmx_stoi_bands refuse alike
inline int stoi_form(int L, int B, const int32_t* lens, const int32_t* h_lens, int cap) {
    if (int rc = rows_form(B, L, lens, h_lens, ST_FRAME + 1)) return rc;       // at least one frame
    MMX_CHECK_ARG(cap >= st_frames(L));
    return MMX_OK;
}

}  // namespace

extern "C" int mmx_stoi_select(const float* ref, int64_t r_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const float* window,
                               double* energy, uint8_t* mask, int32_t* map, int32_t* kept, int cap, hipStream_t stream) {
    MMX_CHECK_ARG(ref && window && energy && mask && map && kept && r_bs >= L);
    if (int rc = stoi_form(L, B, lens, h_lens, cap)) return rc;
    hipLaunchKernelGGL(stoi_energy_kernel, dim3((st_frames(L) + 3) / 4, B), dim3(256), 0, stream, ref, (long)r_bs, L, lens, window, energy, cap);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(stoi_scan_kernel, dim3(B), dim3(256), 0, stream, energy, L, lens, mask, map, kept, cap);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_stoi_bands(const float* est, int64_t e_bs, const float* ref, int64_t r_bs, int L, int B, const int32_t* lens,
                              const int32_t* h_lens, const float* window, const int32_t* map, const int32_t* kept, const void* basis,
                              const void* filt, float* env, int cap, hipStream_t stream) {
    MMX_CHECK_ARG(est && ref && window && map && kept && basis && filt && env && e_bs >= L && r_bs >= L);
    if (int rc = stoi_form(L, B, lens, h_lens, cap)) return rc;
    const int tiles = (max(st_frames(L) - 1, 1) + 15) / 16;
    MMX_LDS_OPT_IN(stoi_bands_kernel, ST_LDS);
    hipLaunchKernelGGL(stoi_bands_kernel, dim3(tiles, B), dim3(ST_THREADS), ST_LDS, stream, est, (long)e_bs, ref, (long)r_bs, L, lens, window,
                       map, kept, (const bf16_t*)basis, (const bf16_t*)filt, env, cap);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_stoi_score(const float* env, int cap, int B, const int32_t* kept, int extended, double* work, int wcap, double* out,
                              int32_t* frames, hipStream_t stream) {
    MMX_CHECK_ARG(env && kept && work && out && frames && B > 0 && B <= 65535 && cap >= 1 && (extended == 0 || extended == 1));
    const int tiles = st_seg_tiles(cap);
    MMX_CHECK_ARG(wcap >= tiles);
    if (extended)
        hipLaunchKernelGGL(stoi_score_kernel<true>, dim3(tiles, B), dim3(SC_THREADS), 0, stream, env, cap, kept, work, wcap);
    else
        hipLaunchKernelGGL(stoi_score_kernel<false>, dim3(tiles, B), dim3(SC_THREADS), 0, stream, env, cap, kept, work, wcap);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(stoi_finish_kernel, dim3(B), dim3(64), 0, stream, work, wcap, cap, kept, extended, out, frames);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
