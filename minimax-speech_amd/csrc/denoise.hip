// Spectral-gate noise reduction of mono fp32 clips (a ragged batch) for gfx950: the reference's SpectralGate
// (dac-vae/audiotools/ml/layers/spectral_gate.py, which transforms.NoiseReduce wraps), the Audacity-style gate, and with it the
// inverse STFT on the spectral tile of spec_tile.h.  mmx/denoise.py builds the tables and states the definitions.
//
// One scale: window length n, hop = n / 4, torch.stft(center=True) with the sqrt of the periodic Hann window folded into the basis
// (reflection by n / 2 as index arithmetic on the row), 1 + len / hop frames, n / 2 + 1 bins padded to nbp (a multiple of 32).
// A workgroup takes 32 frames of one clip: TWO 16-frame A tiles against ONE load of every table fragment (both products stream their
// whole table, 26 MB at n = 2048, per workgroup).
//   mmx_gate_threshold  noise clips -> per bin mean + n_std * std (unbiased) of dB = 20 log10 max(|N|, 1e-4).  gate_stft_kernel<true>:
//                       stage 0 / stage 1 of spec_tile.h (the second A tile is the same sample planes 16 hops further on: the
//                       two-signal form of spec_dft_tile), then per bin the fp64 sums of dB and dB^2 over the tile's valid frames
//                       (8 per lane, then the lanes 16 / 32 apart in a fixed butterfly) into work; gate_thresh_kernel, one thread
//                       per (clip, bin), adds the clip's tiles in tile order.  No atomics.
//   mmx_gate_analyze    clips + thresholds -> the spectrum (fp32 re | im per frame) and the mask bytes dB < thresh, in caller-owned
//                       workspaces.  gate_stft_kernel<false>; dB and the comparison are fp64 on the fp32 magnitude.  Frames past a
//                       member's last and bins past n / 2 get mask 0.
//   mmx_gate_synthesize gate_synth_kernel:
//                       (a) the mask summed over time with the integer triangle (n_time + 1 - |dt|) over the clip's OWN frames -> LDS
//                           as uint8 [32][nbp] (n_time <= 14: at most 225);
//                       (b) per K chunk of at most 17 steps of 32 columns of the 2 * nbp columns (re | im): the integer triangle
//                           over frequency (bins 0 .. n / 2 only) of (a), gain = 1 - amount * (sum / ((n_freq + 1)^2 (n_time + 1)^2))
//                           - the normalised outer product of the two triangles, exactly - times the spectrum value -> three bf16
//                           planes [3][32][chunk + 8] in LDS;
//                       (c) the inverse DFT of the chunk as the six-term bf16 MFMA product against the inverse table's columns
//                           (inv_chunk: a wave owns sample tiles wv, wv + 8, .. of both A tiles), added in chunk order to what the
//                           earlier chunks left in the frames workspace;
//                       (d) the last chunk multiplies by the synthesis window -> the windowed frames.
//                       gate_ola_kernel: overlap-add as a GATHER, one thread per output sample: its <= 4 frames in ascending order,
//                       the same for the window^2 envelope, one division; samples at or past a member's length are written as 0.
// LDS of gate_synth_kernel: 32 * nbp (a) + 3 * 32 * (32 * min(17, 2 nbp / 32) + 8) * 2 (b) bytes = 33 792 + 105 984 = 139 776 at
// n = 2048, whose 66 K steps go through in chunks of 17, 17, 17, 15.  All of K at once would be 33 792 + 407 040 (203 520 for 16 frames):
// over the 160 KB, hence the chunks in turn.
// gate_stft_kernel holds the sample planes of its 32 frames alone (110 880 bytes at n = 2048).
// A clip's output is a function of its own samples, length, thresholds and amount: not of the batch, the row index or the grid.
#include "spec_tile.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int GT_WAVES = 8, GT_THREADS = GT_WAVES * 64;
constexpr int GT_ROWS = 32;                             // frames per workgroup: two A tiles
constexpr int GT_GAP = 16;                              // elements between hop-sized chunks of a sample plane
constexpr int GT_MAX_N = 2048;                          // the LDS carve-ups below are stated and tested up to here
constexpr int GT_DEPTH = 6;                             // table fragments a wave of the inverse product keeps in flight (72 registers)
constexpr int GT_CHUNK = 17;                            // K steps (of 32 columns) of the gated spectrum in LDS at a time
constexpr int GT_MAX_SMOOTH = 14;                       // (n_time + 1)^2 fits a byte
constexpr double GT_FLOOR = 1e-4;                       // spectral_gate.py:99 magnitude.clamp(1e-4)

__host__ __device__ __forceinline__ int gt_frames(int len, int hop) { return 1 + len / hop; }
__host__ __device__ __forceinline__ int gt_plane(int n, int hop) { return spec_plane<GT_GAP>((GT_ROWS - 1) * hop + n, hop); }
__host__ __device__ __forceinline__ size_t gt_stft_lds(int n) { return (size_t)3 * gt_plane(n, n / 4) * sizeof(bf16_t); }
__host__ __device__ __forceinline__ int gt_chunk(int nbp) { return min(GT_CHUNK, 2 * nbp / 32); }
__host__ __device__ __forceinline__ size_t gt_synth_lds(int nbp) {
    return (size_t)GT_ROWS * nbp + (size_t)3 * GT_ROWS * (32 * gt_chunk(nbp) + 8) * sizeof(bf16_t);
}

__device__ __forceinline__ double gt_db(float re, float im) {
    return 20.0 * log10(fmax((double)sqrtf(re * re + im * im), GT_FLOOR));
}

// STATS: work [B][cap][nbp][2] (sum dB, sum dB^2 over the tile's valid frames);  else: spec [B][fcap][2 * nbp], mask [B][fcap][nbp]
template <bool STATS>
__global__ __launch_bounds__(GT_THREADS) void gate_stft_kernel(const float* __restrict__ x, long x_bs, int L, const int* __restrict__ lens,
                                                              const bf16_t* __restrict__ basis, int n, int nbp, int nbins,
                                                              double* __restrict__ work, int cap, const float* __restrict__ thresh,
                                                              long t_bs, float* __restrict__ spec, unsigned char* __restrict__ mask,
                                                              int fcap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int hop = n / 4;
    const int S = (GT_ROWS - 1) * hop + n, SP = gt_plane(n, hop);
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);       // [3][SP]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * GT_ROWS;
    const int len = row_len(lens, b, L);
    const int Tb = len > n / 2 ? gt_frames(len, hop) : 0;   // (the entry point refuses such a length)
    if (t0 >= Tb) {                                     // a tile of padding frames: no statistics; mask 0
        if constexpr (!STATS) {
            const int rows = min(GT_ROWS, fcap - t0);
            unsigned char* m = mask + ((long)b * fcap + t0) * nbp;
            for (int i = tid; i < rows * nbp; i += GT_THREADS) m[i] = 0;
        }
        return;
    }
    spec_stage<GT_GAP>(x + (long)b * x_bs, len, (long)t0 * hop - n / 2, S, S, 1.f, hop, xs, SP, tid, GT_THREADS);
    __syncthreads();
    const bool two = t0 + 16 < Tb;                      // the second A tile holds a frame of the clip (uniform over the workgroup)
    const bf16_t* const sig2[2] = {xs, xs + 16 * (hop + GT_GAP)};
    const bf16_t* const sig1[1] = {xs};
    const long PB = (long)2 * nbp * n;
    for (int j = wv; j < nbp / 16; j += GT_WAVES) {
        float4_t re[2], im[2];
        if (two) {
            spec_dft_tile<2, GT_GAP>(sig2, SP, hop, basis, PB, n / 32, j, lane, re, im);
        } else {                                        // the same MFMA sequence per frame as the two-tile form: the same bits
            float4_t r1[1], i1[1];
            spec_dft_tile<1, GT_GAP>(sig1, SP, hop, basis, PB, n / 32, j, lane, r1, i1);
            re[0] = r1[0];
            im[0] = i1[0];
            re[1] = im[1] = float4_t{0.f, 0.f, 0.f, 0.f};
        }
        const int k = j * 16 + l16;
        if constexpr (STATS) {
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (t0 + 16 * s + 4 * g + r < Tb) {
                        const double d = gt_db(re[s][r], im[s][r]);
                        s1 += d;
                        s2 += d * d;
                    }
            s1 += __shfl_xor(s1, 16, 64);
            s2 += __shfl_xor(s2, 16, 64);
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (g == 0) {
                double* w = work + (((long)b * cap + blockIdx.x) * nbp + k) * 2;
                w[0] = s1;
                w[1] = s2;
            }
        } else {
            const double th = k < nbins ? (double)thresh[(long)b * t_bs + k] : 0.0;
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int t = t0 + 16 * s + 4 * g + r;
                    if (t >= fcap) continue;
                    const long row = (long)b * fcap + t;
                    const bool live = t < Tb && k < nbins;
                    mask[row * nbp + k] = (live && gt_db(re[s][r], im[s][r]) < th) ? 1 : 0;
                    if (t < Tb) {                       // the basis holds +sin: the spectrum's imaginary part is its negative
                        spec[row * 2 * nbp + k] = live ? re[s][r] : 0.f;
                        spec[row * 2 * nbp + nbp + k] = live ? -im[s][r] : 0.f;
                    }
                }
        }
    }
}

// thresh[b][k] = mean + n_std * unbiased std over the clip's own frames, from its tiles in tile order
__global__ __launch_bounds__(64) void gate_thresh_kernel(const double* __restrict__ work, int cap, const int* __restrict__ lens, int L,
                                                        int n, int nbp, int nbins, double n_std, float* __restrict__ thresh, long t_bs) {
    const int k = blockIdx.x * 64 + threadIdx.x, b = blockIdx.y;
    if (k >= nbins) return;
    const int len = row_len(lens, b, L);
    const int T = gt_frames(max(len, 0), n / 4);
    const int tiles = min(cap, (T + GT_ROWS - 1) / GT_ROWS);
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < tiles; ++i) {
        const double* w = work + (((long)b * cap + i) * nbp + k) * 2;
        s1 += w[0];
        s2 += w[1];
    }
    const double mean = s1 / T;
    const double var = fmax(s2 - s1 * mean, 0.0) / (T - 1);     // T >= 3: a clip has more than n / 2 samples
    thresh[(long)b * t_bs + k] = (float)(mean + n_std * sqrt(var));
}

// One K chunk (`steps` steps from step k0 of the KT) of NA A tiles (mg [3][32][MS], rows 16 s .. 16 s + 15) against the wave's sample
// tiles wv, wv + 8, .. of the inverse table: spec_mel_tile for two row tiles, as ONE sequence of (tile, step) pairs whose table
// fragments are fetched GT_DEPTH pairs ahead.  A tile's sum over the chunk starts from zero and is added to what the earlier chunks left in fr (the workgroup's
// 32 rows of the frames workspace; this thread wrote those values itself), the last chunk multiplies by the window.
// C layout: lane (g, l16) holds frames 16 s + 4g .. + 3 of sample 16 mt + l16.
template <int NA>
__device__ __forceinline__ void inv_chunk(const bf16_t* mg, int MS, const bf16_t* __restrict__ inv, long PF, int KT, int k0, int steps,
                                          int wv, int ntiles, int lane, bool first, bool last, float* __restrict__ fr, int n, int rows,
                                          const float* __restrict__ window) {
    constexpr int D = GT_DEPTH;
    const int g = lane >> 4, l16 = lane & 15;
    const int mine = wv < ntiles ? (ntiles - wv + GT_WAVES - 1) / GT_WAVES : 0;
    if (mine == 0) return;                              // uniform over the wave
    const int total = mine * steps;
    const bf16_t* ma = mg + l16 * MS + g * 8;
    int pq = 0, pkt = 0, pmt = wv;                      // the next pair to fetch
    auto fetch = [&](short8_t (&f)[3]) {
        const bf16_t* p = inv + ((long)pmt * KT + k0 + pkt) * 512 + lane * 8;
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) f[pl] = ld8(p + pl * PF);
        if (pq + 1 < total) {                           // past the end: the last fragment again, which nothing uses
            ++pq;
            if (++pkt == steps) {
                pkt = 0;
                pmt += GT_WAVES;
            }
        }
    };
    short8_t fb[D][3];
#pragma unroll
    for (int d = 0; d < D; ++d) fetch(fb[d]);
    float4_t acc[NA];
#pragma unroll
    for (int s = 0; s < NA; ++s) acc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
    int kt = 0, mt = wv;
    for (int q0 = 0; q0 < total; q0 += D) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (q0 + d >= total) break;                 // uniform over the wave
            short8_t a[NA][3];
#pragma unroll
            for (int p = 0; p < 3; ++p)
#pragma unroll
                for (int s = 0; s < NA; ++s) a[s][p] = ld8(ma + (p * GT_ROWS + 16 * s) * MS + kt * 32);
#pragma unroll
            for (int s = 0; s < NA; ++s) acc[s] = mfma6(a[s], fb[d], acc[s]);
            fetch(fb[d]);
            if (++kt == steps) {                        // the tile's chunk is complete
                const int smp = mt * 16 + l16;
                const float w = window[smp];
#pragma unroll
                for (int s = 0; s < NA; ++s)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int row = 16 * s + 4 * g + r;
                        if (row < rows) {
                            float* o = fr + (long)row * n + smp;
                            float v = first ? acc[s][r] : *o + acc[s][r];
                            if (last) v *= w;
                            *o = v;
                        }
                    }
#pragma unroll
                for (int s = 0; s < NA; ++s) acc[s] = float4_t{0.f, 0.f, 0.f, 0.f};
                kt = 0;
                mt += GT_WAVES;
            }
        }
    }
}

// inv: [3 planes][n / 16 tiles][2 nbp / 32][64][8]: row s, column k = the real part's weight, column nbp + k the imaginary part's
__global__ __launch_bounds__(GT_THREADS) void gate_synth_kernel(const float* __restrict__ spec, const unsigned char* __restrict__ mask,
                                                               int fcap, int L, const int* __restrict__ lens,
                                                               const bf16_t* __restrict__ inv, const float* __restrict__ window, int n,
                                                               int nbp, int nbins, int n_freq, int n_time,
                                                               const float* __restrict__ amount, float* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int hop = n / 4, KT = 2 * nbp / 32, CH = gt_chunk(nbp), MS = 32 * CH + 8;
    unsigned char* tsm = reinterpret_cast<unsigned char*>(smem);                     // [32][nbp]
    bf16_t* mg = reinterpret_cast<bf16_t*>(smem + (size_t)GT_ROWS * nbp);             // [3][32][MS]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * GT_ROWS;
    const int len = row_len(lens, b, L);
    const int Tb = len > n / 2 ? gt_frames(len, hop) : 0;
    if (t0 >= Tb) return;                               // uniform over the workgroup
    const bool two = t0 + 16 < Tb;
    const unsigned char* mb = mask + (long)b * fcap * nbp;
    const float* sb = spec + (long)b * fcap * 2 * nbp;
    const float amt = amount[b];
    const float den = (float)((n_freq + 1) * (n_freq + 1) * (n_time + 1) * (n_time + 1));

    // (a) the triangle over time, over the clip's own frames: zero padding at both ends of [0, Tb)
    for (int i = tid; i < GT_ROWS * nbp; i += GT_THREADS) {
        const int f = i / nbp, k = i - f * nbp, t = t0 + f;
        int s = 0;
        if (t < Tb && k < nbins) {
            const int lo = max(t - n_time, 0), hi = min(t + n_time, Tb - 1);
            for (int tt = lo; tt <= hi; ++tt) s += (n_time + 1 - abs(tt - t)) * (int)mb[(long)tt * nbp + k];
        }
        tsm[i] = (unsigned char)s;
    }
    __syncthreads();

    const int ntiles = n / 16, rows = min(GT_ROWS, Tb - t0);
    const long PF = (long)n * 2 * nbp;                  // elements per plane of the inverse table
    float* fr = frames + ((long)b * fcap + t0) * n;
#pragma unroll 1
    for (int k0 = 0; k0 < KT; k0 += CH) {               // K chunks of the columns re | im
        const int steps = min(CH, KT - k0), cw = 32 * steps;
        // (b) the triangle over frequency, the gain, the gated value -> planes
        for (int i = tid; i < GT_ROWS * cw; i += GT_THREADS) {
            const int f = i / cw, c = i - f * cw, q = 32 * k0 + c, t = t0 + f;
            const int k = q >= nbp ? q - nbp : q;       // column q: the real part of bin q, or the imaginary part of bin q - nbp
            float v = 0.f;
            if (t < Tb && k < nbins) {
                const int lo = max(k - n_freq, 0), hi = min(k + n_freq, nbins - 1);
                int s = 0;
                for (int kk = lo; kk <= hi; ++kk) s += (n_freq + 1 - abs(kk - k)) * (int)tsm[f * nbp + kk];
                const float gain = 1.f - amt * ((float)s / den);
                v = sb[(long)t * 2 * nbp + q] * gain;
            }
            put3(mg + f * MS + c, GT_ROWS * MS, 0, v);
        }
        __syncthreads();
        // (c), (d) this chunk's inverse product into the frames workspace; the last chunk applies the synthesis window
        const bool first = k0 == 0, last = k0 + CH >= KT;
        if (two) inv_chunk<2>(mg, MS, inv, PF, KT, k0, steps, wv, ntiles, lane, first, last, fr, n, rows, window);
        else inv_chunk<1>(mg, MS, inv, PF, KT, k0, steps, wv, ntiles, lane, first, last, fr, n, rows, window);
        __syncthreads();                                // every wave has read the planes before the next chunk overwrites them
    }
}

// out[b][j] = (sum over the frames t that cover sample j + n / 2, ascending) / (the same sum of window^2); 0 at and past lens[b]
__global__ __launch_bounds__(256) void gate_ola_kernel(const float* __restrict__ frames, int fcap, int L, const int* __restrict__ lens,
                                                      const float* __restrict__ window, int n, float* __restrict__ out, long o_bs) {
    const int b = blockIdx.y;
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= L) return;
    const int hop = n / 4;
    const int len = row_len(lens, b, L);
    float v = 0.f;
    if (j < len && len > n / 2) {
        const int Tb = gt_frames(len, hop);
        const long p = j + n / 2;
        const int q = (int)(p / hop);
        const int lo = max(q - 3, 0), hi = min(q, Tb - 1);
        float s = 0.f, e = 0.f;
        for (int t = lo; t <= hi; ++t) {
            const int off = (int)(p - (long)t * hop);   // 0 <= off < n: t >= q - 3
            const float w = window[off];
            s += frames[((long)b * fcap + t) * n + off];
            e += w * w;
        }
        v = s / e;                                      // e >= 1/2: a frame of the clip is centred within hop of every sample j
    }
    out[(long)b * o_bs + j] = v;
}

// what the three entry points refuse alike; nbp out
inline int gate_form(int n, int B, int L, const int32_t* lens, const int32_t* h_lens, int* nbp) {
    MMX_CHECK_ARG(n >= 32 && n % 32 == 0 && n <= GT_MAX_N);
    if (int rc = rows_form(B, L, lens, h_lens, n / 2 + 1)) return rc;          // the reflection reads sample n / 2
    *nbp = (n / 2 + 1 + 31) / 32 * 32;
    MMX_CHECK_ARG(gt_stft_lds(n) <= 160 * 1024 && gt_synth_lds(*nbp) <= 160 * 1024);
    return MMX_OK;
}

}  // namespace

extern "C" int mmx_gate_threshold(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const void* basis,
                                  int n_fft, double n_std, double* work, int cap, float* thresh, int64_t t_bs, hipStream_t stream) {
    int nbp = 0;
    MMX_CHECK_ARG(x && basis && work && thresh && x_bs >= L);
    if (int rc = gate_form(n_fft, B, L, lens, h_lens, &nbp)) return rc;
    const int nbins = n_fft / 2 + 1, tiles = (gt_frames(L, n_fft / 4) + GT_ROWS - 1) / GT_ROWS;
    MMX_CHECK_ARG(cap >= tiles && t_bs >= nbins);
    const size_t lds = gt_stft_lds(n_fft);
    MMX_LDS_OPT_IN(gate_stft_kernel<true>, lds);
    hipLaunchKernelGGL(gate_stft_kernel<true>, dim3(tiles, B), dim3(GT_THREADS), lds, stream, x, (long)x_bs, L, lens, (const bf16_t*)basis,
                       n_fft, nbp, nbins, work, cap, (const float*)nullptr, 0L, (float*)nullptr, (unsigned char*)nullptr, 0);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(gate_thresh_kernel, dim3((nbins + 63) / 64, B), dim3(64), 0, stream, work, cap, lens, L, n_fft, nbp, nbins, n_std,
                       thresh, (long)t_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_gate_analyze(const float* x, int64_t x_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, const void* basis,
                                int n_fft, const float* thresh, int64_t t_bs, float* spec, uint8_t* mask, int frames_cap,
                                hipStream_t stream) {
    int nbp = 0;
    MMX_CHECK_ARG(x && basis && thresh && spec && mask && x_bs >= L && (t_bs == 0 || t_bs >= n_fft / 2 + 1));
    if (int rc = gate_form(n_fft, B, L, lens, h_lens, &nbp)) return rc;
    MMX_CHECK_ARG(frames_cap >= gt_frames(L, n_fft / 4));
    const size_t lds = gt_stft_lds(n_fft);
    MMX_LDS_OPT_IN(gate_stft_kernel<false>, lds);
    hipLaunchKernelGGL(gate_stft_kernel<false>, dim3((frames_cap + GT_ROWS - 1) / GT_ROWS, B), dim3(GT_THREADS), lds, stream, x, (long)x_bs,
                       L, lens, (const bf16_t*)basis, n_fft, nbp, n_fft / 2 + 1, (double*)nullptr, 0, thresh, (long)t_bs, spec, mask,
                       frames_cap);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_gate_synthesize(const float* spec, const uint8_t* mask, int frames_cap, int L, int B, const int32_t* lens,
                                   const int32_t* h_lens, const void* inv, const float* window, int n_fft, int n_freq, int n_time,
                                   const float* amount, float* frames, float* out, int64_t o_bs, hipStream_t stream) {
    int nbp = 0;
    MMX_CHECK_ARG(spec && mask && inv && window && amount && frames && out && o_bs >= L);
    MMX_CHECK_ARG(n_freq >= 0 && n_freq <= GT_MAX_SMOOTH && n_time >= 0 && n_time <= GT_MAX_SMOOTH);
    if (int rc = gate_form(n_fft, B, L, lens, h_lens, &nbp)) return rc;
    MMX_CHECK_ARG(frames_cap >= gt_frames(L, n_fft / 4));
    const size_t lds = gt_synth_lds(nbp);
    const dim3 grid((gt_frames(L, n_fft / 4) + GT_ROWS - 1) / GT_ROWS, B);
    MMX_LDS_OPT_IN(gate_synth_kernel, lds);
    hipLaunchKernelGGL(gate_synth_kernel, grid, dim3(GT_THREADS), lds, stream, spec, mask, frames_cap, L, lens, (const bf16_t*)inv, window,
                       n_fft, nbp, n_fft / 2 + 1, n_freq, n_time, amount, frames);
    MMX_LAUNCH_CHECK();
    hipLaunchKernelGGL(gate_ola_kernel, dim3((L + 255) / 256, B), dim3(256), 0, stream, frames, frames_cap, L, lens, window, n_fft, out,
                       (long)o_bs);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
