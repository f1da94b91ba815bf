// A clip -> log-mel frames in one launch for gfx950, under two conventions:
//   mmx_logmel    the reference audio of the speaker encoder (speech/matcha/utils/audio.py:45-82, center=False):
//                 y = reflect_pad(x * gain, (n_fft - hop) / 2);  S = |STFT(y, hann(n_fft))|;  mel = log(max(F . sqrt(S^2 + 1e-9), 1e-5))
//   mmx_logmel_w  the S3 tokenizer's Whisper-convention log-mel (speech/tools/S3Tokenizer/s3tokenizer/utils.py:220-267, center=True):
//                 reflection by n_fft / 2, len / hop frames, the power spectrum, log10(max(F . S^2, 1e-10)), and a finishing launch
//                 for the clip maximum: floor at max - 8, (v + 4) / 4
// One workgroup takes 16 frames of one batch member through both matrix products (spec_tile.h); the spectrum never leaves LDS.
//   stage 0  the padded sample span of the 16 frames (15 * hop + n_fft samples, then zeros up to 15 * hop + kp where the basis has
//            its K dimension zero padded to kp) -> LDS as three bf16 planes hi + mid + lo = fl(x * gain)
//   stage 1  DFT of the bins the filterbank reads -> the convention's spectrum value -> LDS, split once into three bf16 planes
//   stage 2  mel = spectrum x filter planes -> the convention's log -> both output layouts
// A wave owns whole 16-bin (stage 1) / 16-mel (stage 2) column tiles, so no reduction crosses waves and a member's result does
// not depend on the batch it is computed in.
#include "spec_tile.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int LM_WAVES = 8;

// A convention: the reflection pad, the frames of a member with `len` valid samples (0 where the reflection is undefined or no
// frame fits), the K dimension of its basis (n_fft rounded up to 32), the spectrum value of a bin, and the output of a mel value.
struct Matcha {
    static __host__ __device__ __forceinline__ int pad(int n_fft, int hop) { return (n_fft - hop) / 2; }
    static __host__ __device__ __forceinline__ int frames(int len, int n_fft, int hop) {
        const int pad = (n_fft - hop) / 2;
        return (len > pad && len + 2 * pad >= n_fft) ? (len + 2 * pad - n_fft) / hop + 1 : 0;
    }
    static __host__ __device__ __forceinline__ int kpad(int n_fft) { return n_fft; }     // mmx_logmel demands n_fft % 32 == 0
    static __device__ __forceinline__ float spectrum(float re, float im) { return sqrtf(re * re + im * im + 1e-9f); }
    // the clip value is fl(ln(fl(1e-5))): what log(clamp(v, 1e-5)) returns for every v <= 1e-5
    static __device__ __forceinline__ float out(float v) { return v > 1e-5f ? logf(v) : -11.512925148010254f; }
};
struct Whisper {
    static __host__ __device__ __forceinline__ int pad(int n_fft, int) { return n_fft / 2; }
    static __host__ __device__ __forceinline__ int frames(int len, int n_fft, int hop) { return len > n_fft / 2 ? len / hop : 0; }
    static __host__ __device__ __forceinline__ int kpad(int n_fft) { return (n_fft + 31) / 32 * 32; }
    static __device__ __forceinline__ float spectrum(float re, float im) { return re * re + im * im; }
    static __device__ __forceinline__ float out(float v) { return v > 1e-10f ? log10f(v) : -10.f; }
};

// Writes Conv::out(mel) for the member's own frames and 0 for the others.
template <typename TO, typename Conv>
__global__ __launch_bounds__(LM_WAVES * 64) void logmel_kernel(const float* __restrict__ wave, long w_bs, int L,
                                                               const float* __restrict__ gain, const int* __restrict__ lens,
                                                               const bf16_t* __restrict__ basis, const bf16_t* __restrict__ filt,
                                                               int n_fft, int hop, int nbp, int n_mels, int mp,
                                                               float* __restrict__ out_cm, long ldo, TO* __restrict__ out_tm, int T) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int kp = Conv::kpad(n_fft);
    const int S = 15 * hop + kp;                        // samples under 16 frames plus the K padding (a multiple of 8)
    const int MS = nbp + 8;
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);       // [3][S]
    bf16_t* mg = xs + 3 * S;                            // [3][16][MS]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * 16;
    const int len = row_len(lens, b, L);
    const int Tb = Conv::frames(len, n_fft, hop);

    if (t0 >= Tb) {                                     // a tile of padding frames (uniform over the workgroup): zeros
        for (int i = tid; i < 16 * n_mels; i += LM_WAVES * 64) {
            const int t = t0 + i / n_mels, mel = i % n_mels;
            if (t < T) {
                if (out_cm) out_cm[((long)b * n_mels + mel) * ldo + t] = 0.f;
                if (out_tm) out_tm[((long)b * T + t) * n_mels + mel] = Cvt<TO>::from_f(0.f);
            }
        }
        return;
    }

    spec_stage<0>(wave + (long)b * w_bs, len, (long)t0 * hop - Conv::pad(n_fft, hop), 15 * hop + n_fft, S, gain ? gain[b] : 1.f, hop, xs, S,
                  tid, LM_WAVES * 64);
    __syncthreads();

    const bf16_t* const sig[1] = {xs};
    for (int j = wv; j < nbp / 16; j += LM_WAVES) {
        float4_t re[1], im[1];
        spec_dft_tile<1, 0>(sig, S, hop, basis, (long)2 * nbp * kp, kp / 32, j, lane, re, im);
#pragma unroll
        for (int r = 0; r < 4; ++r) spec_store3(mg, MS, 4 * g + r, j * 16 + l16, Conv::spectrum(re[0][r], im[0][r]));
    }
    __syncthreads();

    for (int mt = wv; mt < mp / 16; mt += LM_WAVES) {
        const float4_t acc = spec_mel_tile(mg, MS, filt, (long)mp * nbp, nbp / 32, mt, lane);
        const int mel = mt * 16 + l16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int t = t0 + 4 * g + r;
            if (mel < n_mels && t < T) {
                const float o = t < Tb ? Conv::out(acc[r]) : 0.f;
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
    const int len = row_len(lens, b, L);
    const int Tb = min(Whisper::frames(len, n_fft, hop), T);
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

// What the two entry points share after their own argument checks: every member has a frame and fits the outputs, the padded
// sizes, the LDS, the grid, and the launch in the activation type of `act` (MMX_F32 or MMX_BF16).
template <typename Conv>
int launch_logmel(const float* wave, int64_t w_bs, int L, int B, const float* gain, const int32_t* lens, const int32_t* h_lens,
                  const void* basis, const void* filt, int n_fft, int hop, int n_bins, int n_mels, float* out_cm, int64_t ldo,
                  void* out_tm, int T, int act, hipStream_t stream) {
    const int pad = Conv::pad(n_fft, hop);
    if (int rc = rows_form(B, L, lens, h_lens, pad + 1)) return rc;            // the reflection reads sample `pad`
    int tmax = 0;
    for (int b = 0; b < B; ++b) {
        const int frames = Conv::frames(h_lens ? h_lens[b] : L, n_fft, hop);
        MMX_CHECK_ARG(frames > 0);
        tmax = max(tmax, frames);
    }
    MMX_CHECK_ARG(T >= tmax);                           // every frame a member has fits the outputs
    const int kp = Conv::kpad(n_fft), nbp = (n_bins + 31) / 32 * 32, mp = (n_mels + 15) / 16 * 16;
    const size_t lds = ((size_t)3 * (15 * hop + kp) + (size_t)3 * 16 * (nbp + 8)) * sizeof(bf16_t);
    MMX_CHECK_ARG(lds <= 160 * 1024);
    const dim3 grid((T + 15) / 16, B), block(LM_WAVES * 64);
    if (act == MMX_BF16) {
        MMX_LDS_OPT_IN((logmel_kernel<bf16_t, Conv>), lds);
        hipLaunchKernelGGL((logmel_kernel<bf16_t, Conv>), grid, block, lds, stream, wave, (long)w_bs, L, gain, lens, (const bf16_t*)basis,
                           (const bf16_t*)filt, n_fft, hop, nbp, n_mels, mp, out_cm, (long)ldo, (bf16_t*)out_tm, T);
    } else if (act == MMX_F32) {
        MMX_LDS_OPT_IN((logmel_kernel<float, Conv>), lds);
        hipLaunchKernelGGL((logmel_kernel<float, Conv>), grid, block, lds, stream, wave, (long)w_bs, L, gain, lens, (const bf16_t*)basis,
                           (const bf16_t*)filt, n_fft, hop, nbp, n_mels, mp, out_cm, (long)ldo, (float*)out_tm, T);
    } else return MMX_EARG;
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

}  // namespace

extern "C" int mmx_logmel(const float* wave, int64_t w_bs, int L, int B, const float* gain, const int32_t* lens,
                          const int32_t* h_lens, const void* basis, const void* filt, int n_fft, int hop, int bin0, int n_bins,
                          int n_mels, float* out_cm, int64_t ldo, void* out_tm, int T, int dtype, hipStream_t stream) {
    MMX_CHECK_ARG(wave && basis && filt && (out_cm || out_tm) && T > 0);
    MMX_CHECK_ARG(n_fft > 0 && n_fft % 32 == 0 && n_mels > 0 && n_mels <= 128);
    MMX_CHECK_ARG(hop > 0 && hop <= n_fft && hop % 8 == 0 && (n_fft - hop) % 2 == 0);
    MMX_CHECK_ARG(bin0 >= 0 && n_bins > 0 && bin0 + n_bins <= n_fft / 2 + 1);
    MMX_CHECK_ARG(w_bs >= L && (!out_cm || ldo >= T));
    return launch_logmel<Matcha>(wave, w_bs, L, B, gain, lens, h_lens, basis, filt, n_fft, hop, n_bins, n_mels, out_cm, ldo, out_tm, T,
                                 MMX_ACT_DTYPE(dtype), stream);
}

extern "C" int mmx_logmel_w(const float* wave, int64_t w_bs, int L, int B, const int32_t* lens, const int32_t* h_lens,
                            const void* basis, const void* filt, int n_fft, int hop, int bin0, int n_bins, int n_mels,
                            float* out_cm, int64_t ldo, void* out_tm, int T, int dtype, hipStream_t stream) {
    MMX_CHECK_ARG(wave && basis && filt && (out_cm || out_tm) && T > 0);
    MMX_CHECK_ARG(n_fft > 0 && n_fft % 16 == 0 && n_mels > 0 && n_mels <= 128);
    MMX_CHECK_ARG(hop > 0 && hop <= n_fft && hop % 8 == 0);
    MMX_CHECK_ARG(bin0 >= 0 && n_bins > 0 && bin0 + n_bins <= n_fft / 2 + 1);
    MMX_CHECK_ARG(w_bs >= L && (!out_cm || ldo >= T));
    const int act = MMX_ACT_DTYPE(dtype);
    MMX_CHECK_ARG(act == MMX_F32 || (act == MMX_BF16 && (out_cm || !out_tm)));   // the clip maximum is taken over fp32 values
    const int rc = launch_logmel<Whisper>(wave, w_bs, L, B, nullptr, lens, h_lens, basis, filt, n_fft, hop, n_bins, n_mels, out_cm, ldo,
                                          out_tm, T, act, stream);
    if (rc != MMX_OK) return rc;
    if (act == MMX_BF16)
        hipLaunchKernelGGL(logmel_w_finish<bf16_t>, dim3(B), dim3(LF_THREADS), 0, stream, lens, L, n_fft, hop, n_mels, out_cm, (long)ldo,
                           (bf16_t*)out_tm, T);
    else
        hipLaunchKernelGGL(logmel_w_finish<float>, dim3(B), dim3(LF_THREADS), 0, stream, lens, L, n_fft, hop, n_mels, out_cm, (long)ldo,
                           (float*)out_tm, T);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
