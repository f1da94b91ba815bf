// Reference audio -> log-mel frames in one launch (speech/matcha/utils/audio.py:45-82, center=False) for gfx950.
//   y = reflect_pad(x * gain, (n_fft - hop) / 2);  S = |STFT(y, hann(n_fft))|;  mel = log(max(F . sqrt(S^2 + 1e-9), 1e-5))
// One workgroup takes 16 frames of one batch member through both matrix products; the spectrum never leaves LDS.
//   stage 0  the padded sample span of the 16 frames (15 * hop + n_fft samples; the reflection is index arithmetic on the
//            unpadded row) -> LDS as three bf16 planes hi + mid + lo = fl(x * gain)
//   stage 1  DFT as a GEMM on v_mfma_f32_16x16x32_bf16: A = frames (LDS, frame l16 starts l16 * hop samples into the span),
//            B = window * cos | window * sin of the bins the filterbank reads, three bf16 planes of the float64 values in
//            mmx_pack_skinny order; every term pair s + p < 3 is kept (six MFMAs per fragment pair), fp32 accumulation
//            -> sqrt(re^2 + im^2 + 1e-9) -> LDS, split once into three bf16 planes
//   stage 2  mel = magnitudes x filter planes, the same six-term product -> log(max(v, 1e-5)) -> both output layouts
// A wave owns whole 16-bin (stage 1) / 16-mel (stage 2) column tiles, so no reduction crosses waves and a member's result does
// not depend on the batch it is computed in.
#include "common.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int LM_WAVES = 8;
constexpr float LM_LOG_CLIP = -11.512925148010254f;     // fl(ln(fl(1e-5))): what log(clamp(v, 1e-5)) returns for every v <= 1e-5

struct Bf3 { bf16_t h, m, l; };
__device__ __forceinline__ Bf3 split3(float v) {       // the remainders are exact in fp32
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

// frames of a member with `len` valid samples (0 where the reflection is undefined or no frame fits)
__host__ __device__ __forceinline__ int logmel_frames(int len, int n_fft, int hop) {
    const int pad = (n_fft - hop) / 2;
    return (len > pad && len + 2 * pad >= n_fft) ? (len + 2 * pad - n_fft) / hop + 1 : 0;
}

// basis: [3 planes][2 * nbp / 16 tiles][n_fft / 32][64][8], tile 2j = window * cos of bins 16j .. 16j + 15, tile 2j + 1 = window * sin
// filt : [3 planes][mp / 16 tiles][nbp / 32][64][8]
template <typename TO>
__global__ __launch_bounds__(LM_WAVES * 64) void logmel_kernel(const float* __restrict__ wave, long w_bs, int L,
                                                               const float* __restrict__ gain, const int* __restrict__ lens,
                                                               const bf16_t* __restrict__ basis, const bf16_t* __restrict__ filt,
                                                               int n_fft, int hop, int nbp, int n_mels, int mp,
                                                               float* __restrict__ out_cm, long ldo, TO* __restrict__ out_tm, int T) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int S = 15 * hop + n_fft;                     // samples under 16 frames (a multiple of 8)
    const int MS = nbp + 8;                             // magnitude row stride: 16-byte aligned rows, 4 banks apart
    bf16_t* xs = reinterpret_cast<bf16_t*>(smem);       // [3][S]
    bf16_t* mg = xs + 3 * S;                            // [3][16][MS]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int b = blockIdx.y, t0 = blockIdx.x * 16;
    const int pad = (n_fft - hop) / 2;
    const int len = lens ? min(lens[b], L) : L;
    const int Tb = logmel_frames(len, n_fft, hop);
    const int mtiles = mp / 16;

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

    // ---- stage 0: samples -> planes
    const float* x = wave + (long)b * w_bs;
    const float gn = gain ? gain[b] : 1.f;
    for (int q = tid; q < S; q += LM_WAVES * 64) {
        long i = (long)t0 * hop + q - pad;
        if (i < 0) i = -i;
        if (i >= len) i = 2L * (len - 1) - i;
        // beyond one reflection: only frames >= Tb reach there, and those are written as zeros
        const float v = (i >= 0 && i < len) ? __fmul_rn(x[i], gn) : 0.f;
        const Bf3 s = split3(v);
        xs[q] = s.h;
        xs[S + q] = s.m;
        xs[2 * S + q] = s.l;
    }
    __syncthreads();

    // ---- stage 1: DFT tiles -> magnitude planes
    const int nkt = n_fft / 32;
    const long PB = (long)2 * nbp * n_fft;              // elements per basis plane
    const bf16_t* xa = xs + l16 * hop + g * 8;
    for (int j = wv; j < nbp / 16; j += LM_WAVES) {
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
            const Bf3 m3 = split3(sqrtf(re[r] * re[r] + im[r] * im[r] + 1e-9f));
            bf16_t* d = mg + (4 * g + r) * MS + j * 16 + l16;
            d[0] = m3.h;
            d[16 * MS] = m3.m;
            d[32 * MS] = m3.l;
        }
    }
    __syncthreads();

    // ---- stage 2: mel projection, log, both layouts
    const int nk2 = nbp / 32;
    const long PF = (long)mp * nbp;
    const bf16_t* ma = mg + l16 * MS + g * 8;
    for (int mt = wv; mt < mtiles; mt += LM_WAVES) {
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
                const float o = t < Tb ? (v > 1e-5f ? logf(v) : LM_LOG_CLIP) : 0.f;
                if (out_cm) out_cm[((long)b * n_mels + mel) * ldo + t] = o;
                if (out_tm) out_tm[((long)b * T + t) * n_mels + mel] = Cvt<TO>::from_f(o);
            }
        }
    }
}

}  // namespace

extern "C" int mmx_logmel(const float* wave, int64_t w_bs, int L, int B, const float* gain, const int32_t* lens,
                          const int32_t* h_lens, const void* basis, const void* filt, int n_fft, int hop, int bin0, int n_bins,
                          int n_mels, float* out_cm, int64_t ldo, void* out_tm, int T, int dtype, hipStream_t stream) {
    MMX_CHECK_ARG(wave && basis && filt && (out_cm || out_tm) && B > 0 && B <= 65535 && T > 0 && L > 0);
    MMX_CHECK_ARG(n_fft > 0 && n_fft % 32 == 0 && n_mels > 0 && n_mels <= 128);
    MMX_CHECK_ARG(hop > 0 && hop <= n_fft && hop % 8 == 0 && (n_fft - hop) % 2 == 0);
    MMX_CHECK_ARG(bin0 >= 0 && n_bins > 0 && bin0 + n_bins <= n_fft / 2 + 1);
    MMX_CHECK_ARG(w_bs >= L && (!out_cm || ldo >= T) && (!lens == !h_lens));
    const int pad = (n_fft - hop) / 2;
    MMX_CHECK_ARG(L > pad);                             // the reflection reads sample `pad`
    int tmax = 0;
    for (int b = 0; b < B; ++b) {
        const int len = h_lens ? h_lens[b] : L;
        MMX_CHECK_ARG(len > pad && len <= L && logmel_frames(len, n_fft, hop) > 0);
        tmax = max(tmax, logmel_frames(len, n_fft, hop));
    }
    MMX_CHECK_ARG(T >= tmax);                           // every frame a member has fits the outputs
    const int nbp = (n_bins + 31) / 32 * 32, mp = (n_mels + 15) / 16 * 16;
    const size_t lds = ((size_t)3 * (15 * hop + n_fft) + (size_t)3 * 16 * (nbp + 8)) * sizeof(bf16_t);
    MMX_CHECK_ARG(lds <= 160 * 1024);
    const dim3 grid((T + 15) / 16, B), block(LM_WAVES * 64);
    if (MMX_ACT_DTYPE(dtype) == MMX_BF16) {
        MMX_LDS_OPT_IN(logmel_kernel<bf16_t>, lds);
        hipLaunchKernelGGL(logmel_kernel<bf16_t>, grid, block, lds, stream, wave, (long)w_bs, L, gain, lens, (const bf16_t*)basis,
                           (const bf16_t*)filt, n_fft, hop, nbp, n_mels, mp, out_cm, (long)ldo, (bf16_t*)out_tm, T);
    } else if (MMX_ACT_DTYPE(dtype) == MMX_F32) {
        MMX_LDS_OPT_IN(logmel_kernel<float>, lds);
        hipLaunchKernelGGL(logmel_kernel<float>, grid, block, lds, stream, wave, (long)w_bs, L, gain, lens, (const bf16_t*)basis,
                           (const bf16_t*)filt, n_fft, hop, nbp, n_mels, mp, out_cm, (long)ldo, (float*)out_tm, T);
    } else return MMX_EARG;
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
