// Distances between an estimate x and a reference y, two ragged batches of mono fp32 rows of equal per-clip length, for gfx950:
// what the reference's DAC-VAE validation reports (dac-vae/loss.py MultiScaleSTFTLoss / MelSpectrogramLoss / L1Loss / SISDRLoss,
// dac-vae/train.py:706-709) and its latent extractor writes (extract_dac_latents.py:89-95 mse / snr), without a host sync and without
// a spectrogram in HBM.  mmx/metrics.py builds the tables and states the definitions.
//
// mmx_spec_dist, one scale (n_fft, hop = n_fft / 4, torch.stft(center=True) with a periodic Hann window, 1 + len / hop frames):
//   One workgroup takes 16 frames of one clip through BOTH signals, on the functions of spec_tile.h.
//   stage 0  the sample span under the 16 frames (15 * hop + n_fft samples; the reflection by n_fft / 2 is index arithmetic on the
//            row) -> LDS as three bf16 planes hi + mid + lo = x, hop-sized chunks 16 elements apart (the header's GAP).
//   stage 1  DFT of all n_fft / 2 + 1 bins as the six-term bf16 MFMA product, fp32 accumulation.
//            STFT mode: both signals' planes are in LDS at once, a wave's lane holds re / im of the same (frame, bin) for x and y
//            (one load of the basis fragments serves both), and the distance terms come straight from the accumulators.
//            Mel mode: x alone goes samples -> magnitudes (LDS, three planes) -> mel = magnitudes x filter planes (stage 2, the
//            same six-term product), its mel accumulators stay in registers (a wave owns at most 3 of the <= 24 mel tiles) while y
//            takes the same LDS through the same code; then the terms.  Two signals' sample and magnitude planes of a 2048-point
//            scale are 2 x (59 + 100) KB, one signal's are 159 KB: staged one after the other they keep 16 frames per workgroup.
//   Every term from the subtraction on is fp64: |log10 max(a, eps) - log10 max(b, eps)| and |a - b| per (frame, bin or mel), summed
//   per lane in tile order, across the wave in a fixed butterfly, across the waves in wave order -> work[b][tile][2].  The finishing
//   launch, one wave per clip, adds the clip's own tiles in a fixed order and divides by frames * bins.
// mmx_wave_sums: sum x, y, x^2, y^2, xy, |x - y|, (x - y)^2 per clip in fp64 (products of fp32 values are exact in fp64), 4096 samples
//   per workgroup, the same fixed orders, the same finishing launch.
// A clip's numbers are a function of its own samples and length: not of the batch, the row index or the grid.
#include "spec_tile.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int SD_WAVES = 8, SD_THREADS = SD_WAVES * 64;
constexpr int SD_GAP = 16;                              // elements between hop-sized chunks of a sample plane
constexpr int SD_MT = 3;                                // mel tiles per wave: n_mels <= 16 * SD_MT * SD_WAVES = 384
constexpr int WS_THREADS = 256, WS_PER = 16, WS_CHUNK = WS_THREADS * WS_PER;

__host__ __device__ __forceinline__ int sd_frames(int len, int hop) { return 1 + len / hop; }
// elements of one sample plane: the span of 16 frames with its gaps
__host__ __device__ __forceinline__ int sd_plane(int n_fft, int hop) { return spec_plane<SD_GAP>(15 * hop + n_fft, hop); }
__host__ __device__ __forceinline__ size_t sd_lds(int n_fft, int nbp, bool mel) {
    const size_t planes = (size_t)3 * sd_plane(n_fft, n_fft / 4) * sizeof(bf16_t);
    return (mel ? planes + (size_t)3 * 16 * (nbp + 8) * sizeof(bf16_t) : 2 * planes) + SD_WAVES * 2 * sizeof(double);
}

struct Dist {
    double lg = 0.0, mg = 0.0;
    __device__ __forceinline__ void add(float a, float b, double eps) {
        const double da = (double)a, db = (double)b;
        lg += fabs(log10(fmax(da, eps)) - log10(fmax(db, eps)));
        mg += fabs(da - db);
    }
};

// basis: [3 planes][2 * nbp / 16 tiles][n_fft / 32][64][8], tile 2j = window * cos of bins 16j .. 16j + 15, tile 2j + 1 = window * sin
// filt : [3 planes][mp / 16 tiles][nbp / 32][64][8]
// work : [B][cap][2] (sum of the log terms, sum of the magnitude terms) of the clip's tile blockIdx.x
template <bool MEL>
__global__ __launch_bounds__(SD_THREADS) void spec_dist_kernel(const float* __restrict__ x, long x_bs, const float* __restrict__ y, long y_bs,
                                                              int L, const int* __restrict__ lens, const bf16_t* __restrict__ basis,
                                                              const bf16_t* __restrict__ filt, int n_fft, int nbp, int ncols, int mp,
                                                              double eps, double* __restrict__ work, int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int hop = n_fft / 4;
    const int S = 15 * hop + n_fft, SP = sd_plane(n_fft, hop);
    const int MS = nbp + 8;                             // magnitude row stride: 16-byte aligned rows, 4 banks apart
    double* red = reinterpret_cast<double*>(smem);      // [SD_WAVES][2]
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem + SD_WAVES * 2 * sizeof(double));   // [3][SP]
    bf16_t* ys = xs + 3 * SP;                           // STFT mode: [3][SP] of y;  mel mode: the magnitudes [3][16][MS]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * 16;
    const int len = row_len(lens, b, L);
    const int Tb = sd_frames(len, hop);
    if (len <= n_fft / 2 || t0 >= Tb) return;           // (the entry point refuses such a length) / a tile of padding frames
    const long first = (long)t0 * hop - n_fft / 2;      // of the tile's span on the unpadded row
    const int nkt = n_fft / 32;
    const long PB = (long)2 * nbp * n_fft;              // elements per basis plane
    const float* xr = x + (long)b * x_bs;
    const float* yr = y + (long)b * y_bs;
    Dist d;

    if constexpr (!MEL) {
        spec_stage<SD_GAP>(xr, len, first, S, S, 1.f, hop, xs, SP, tid, SD_THREADS);
        spec_stage<SD_GAP>(yr, len, first, S, S, 1.f, hop, ys, SP, tid, SD_THREADS);
        __syncthreads();
        const bf16_t* const sig[2] = {xs, ys};
        for (int j = wv; j < nbp / 16; j += SD_WAVES) {
            float4_t re[2], im[2];
            spec_dft_tile<2, SD_GAP>(sig, SP, hop, basis, PB, nkt, j, lane, re, im);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (j * 16 + l16 < ncols && t0 + 4 * g + r < Tb)
                    d.add(sqrtf(re[0][r] * re[0][r] + im[0][r] * im[0][r]), sqrtf(re[1][r] * re[1][r] + im[1][r] * im[1][r]), eps);
        }
    } else {
        bf16_t* mg = ys;
        const int mtiles = mp / 16;
        const bf16_t* const sig[1] = {xs};
        float4_t mx[SD_MT];
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {                   // the estimate, then the reference, through the same LDS and the same code
            spec_stage<SD_GAP>(s ? yr : xr, len, first, S, S, 1.f, hop, xs, SP, tid, SD_THREADS);
            __syncthreads();                            // also: every wave has read the first signal's magnitudes
            for (int j = wv; j < nbp / 16; j += SD_WAVES) {
                float4_t re[1], im[1];
                spec_dft_tile<1, SD_GAP>(sig, SP, hop, basis, PB, nkt, j, lane, re, im);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    spec_store3(mg, MS, 4 * g + r, j * 16 + l16, sqrtf(re[0][r] * re[0][r] + im[0][r] * im[0][r]));
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < SD_MT; ++i) {
                const int mt = wv + i * SD_WAVES;
                if (mt >= mtiles) continue;             // uniform over the wave
                const float4_t acc = spec_mel_tile(mg, MS, filt, (long)mp * nbp, nbp / 32, mt, lane);
                if (s == 0) {
                    mx[i] = acc;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (mt * 16 + l16 < ncols && t0 + 4 * g + r < Tb) d.add(mx[i][r], acc[r], eps);
                }
            }
        }
    }

    const double sl = wave_sum_f64(d.lg), sm = wave_sum_f64(d.mg);
    if (lane == 0) {
        red[2 * wv] = sl;
        red[2 * wv + 1] = sm;
    }
    __syncthreads();
    if (tid < 2) {
        double a = 0.0;
        for (int w = 0; w < SD_WAVES; ++w) a += red[2 * w + tid];
        work[((long)b * cap + blockIdx.x) * 2 + tid] = a;
    }
}

// One wave per clip: the clip's first `tiles` rows of work[b][cap][NV] added - lane l takes rows l, l + 64, .. in order, then the
// butterfly - so the order depends on the clip's own tile count alone.  Every lane returns the sums.
template <int NV>
__device__ __forceinline__ void clip_sums(const double* __restrict__ w, int tiles, int lane, double (&s)[NV]) {
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k] = 0.0;
    for (int i = lane; i < tiles; i += 64) {
#pragma unroll
        for (int k = 0; k < NV; ++k) s[k] += w[(long)i * NV + k];
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) s[k] = wave_sum_f64(s[k]);
}

__global__ __launch_bounds__(64) void spec_finish_kernel(const double* __restrict__ work, int cap, const int* __restrict__ lens, int L,
                                                        int n_fft, int ncols, double pw, double* __restrict__ out) {
    const int lane = threadIdx.x, b = blockIdx.x, hop = n_fft / 4;
    const int len = row_len(lens, b, L);
    const int T = sd_frames(max(len, 0), hop);
    double s[2];
    clip_sums<2>(work + (long)b * cap * 2, min(cap, (T + 15) / 16), lane, s);
    if (lane == 0) {
        const double den = (double)T * (double)ncols;
        out[2 * b] = pw * s[0] / den;                   // log10(v^pow) = pow log10(v): v >= eps > 0
        out[2 * b + 1] = s[1] / den;
    }
}

__global__ __launch_bounds__(WS_THREADS) void wave_sums_kernel(const float* __restrict__ x, long x_bs, const float* __restrict__ y, long y_bs,
                                                              int L, const int* __restrict__ lens, float clip, double* __restrict__ work,
                                                              int cap) {
    __shared__ double red[WS_THREADS / 64][7];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.y;
    const int len = row_len(lens, b, L);
    const long j0 = (long)blockIdx.x * WS_CHUNK;
    if (j0 >= len) return;                              // uniform over the workgroup
    const float* xr = x + (long)b * x_bs;
    const float* yr = y + (long)b * y_bs;
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int r = 0; r < WS_PER; ++r) {
        const long j = j0 + tid + r * WS_THREADS;
        if (j < len) {
            float xe = xr[j];
            if (clip > 0.f) xe = fminf(fmaxf(xe, -clip), clip);
            const double dx = (double)xe, dy = (double)yr[j], df = dx - dy;
            s[0] += dx;
            s[1] += dy;
            s[2] += dx * dx;
            s[3] += dy * dy;
            s[4] += dx * dy;
            s[5] += fabs(df);
            s[6] += df * df;
        }
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const double v = wave_sum_f64(s[k]);
        if (lane == 0) red[wv][k] = v;
    }
    __syncthreads();
    if (tid < 7) {
        double a = 0.0;
        for (int w = 0; w < WS_THREADS / 64; ++w) a += red[w][tid];
        work[((long)b * cap + blockIdx.x) * 7 + tid] = a;
    }
}

__global__ __launch_bounds__(64) void wave_finish_kernel(const double* __restrict__ work, int cap, const int* __restrict__ lens, int L,
                                                        double* __restrict__ out) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const int len = row_len(lens, b, L);
    double s[7];
    clip_sums<7>(work + (long)b * cap * 7, (int)min((long)cap, ((long)len + WS_CHUNK - 1) / WS_CHUNK), lane, s);
    if (lane < 7) {
        double v = s[0];
#pragma unroll
        for (int k = 1; k < 7; ++k) v = lane == k ? s[k] : v;
        out[7 * b + lane] = v;
    }
}

}  // namespace

extern "C" int mmx_spec_dist(const float* x, int64_t x_bs, const float* y, int64_t y_bs, int L, int B, const int32_t* lens,
                             const int32_t* h_lens, const void* basis, const void* filt, int n_fft, int n_mels, double eps, double pow,
                             double* work, int cap, double* out, hipStream_t stream) {
    MMX_CHECK_ARG(x && y && basis && work && out && x_bs >= L && y_bs >= L);
    MMX_CHECK_ARG(n_fft >= 32 && n_fft % 32 == 0 && n_fft <= (1 << 20) && eps > 0.0);
    MMX_CHECK_ARG(n_mels >= 0 && n_mels <= 16 * SD_MT * SD_WAVES && (!n_mels == !filt));
    const int hop = n_fft / 4;
    if (int rc = rows_form(B, L, lens, h_lens, n_fft / 2 + 1)) return rc;      // the reflection reads sample n_fft / 2
    MMX_CHECK_ARG(cap >= (sd_frames(L, hop) + 15) / 16);
    const int n_bins = n_fft / 2 + 1, nbp = (n_bins + 31) / 32 * 32, mp = (n_mels + 15) / 16 * 16;
    const size_t lds = sd_lds(n_fft, nbp, n_mels > 0);
    MMX_CHECK_ARG(lds <= 160 * 1024);
    const int tiles = (sd_frames(L, hop) + 15) / 16;
    const dim3 grid(tiles, B), block(SD_THREADS);
    if (n_mels > 0) {
        MMX_LDS_OPT_IN(spec_dist_kernel<true>, lds);
        hipLaunchKernelGGL(spec_dist_kernel<true>, grid, block, lds, stream, x, (long)x_bs, y, (long)y_bs, L, lens, (const bf16_t*)basis,
                           (const bf16_t*)filt, n_fft, nbp, n_mels, mp, eps, work, cap);
    } else {
        MMX_LDS_OPT_IN(spec_dist_kernel<false>, lds);
        hipLaunchKernelGGL(spec_dist_kernel<false>, grid, block, lds, stream, x, (long)x_bs, y, (long)y_bs, L, lens, (const bf16_t*)basis,
                           (const bf16_t*)nullptr, n_fft, nbp, n_bins, mp, eps, work, cap);
    }
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(spec_finish_kernel, dim3(B), dim3(64), 0, stream, work, cap, lens, L, n_fft, n_mels > 0 ? n_mels : n_bins, pow, out);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_wave_sums(const float* x, int64_t x_bs, const float* y, int64_t y_bs, int L, int B, const int32_t* lens, float clip,
                             double* work, int cap, double* out, hipStream_t stream) {
    MMX_CHECK_ARG(x && y && work && out && B > 0 && B <= 65535 && L > 0 && x_bs >= L && y_bs >= L && clip >= 0.f);
    const long chunks = ((long)L + WS_CHUNK - 1) / WS_CHUNK;
    MMX_CHECK_ARG(cap >= chunks);
    hipLaunchKernelGGL(wave_sums_kernel, dim3((unsigned)chunks, B), dim3(WS_THREADS), 0, stream, x, (long)x_bs, y, (long)y_bs, L, lens, clip,
                       work, cap);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(wave_finish_kernel, dim3(B), dim3(64), 0, stream, work, cap, lens, L, out);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
