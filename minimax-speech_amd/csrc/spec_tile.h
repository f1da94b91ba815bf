// What the spectral front ends share (mel.hip: logmel_kernel under both conventions; metrics.hip: spec_dist_kernel): 16 frames of
// one signal as three bf16 planes in LDS, the windowed DFT and the mel projection as six-term bf16 MFMA products on
// v_mfma_f32_16x16x32_bf16 against three-plane float64-derived tables in mmx_pack_skinny order (mmx/mel.py builds them).
//   spec_stage      stage 0: the sample span under the 16 frames (reflection as index arithmetic on the unpadded row) -> planes
//   spec_dft_tile   stage 1: re / im of one 16-bin tile for one or two signals that share the basis fragments
//   put3            a value -> its three bf16 terms in three planes
//   spec_store3     a spectrum value -> the three magnitude planes
//   spec_mel_tile   stage 2: one 16-mel tile of magnitudes x filter planes
// GAP (compile time, 0 or 16): elements between hop-sized chunks of a sample plane.  The 16 frames of an A fragment start hop
// samples apart, which at hop = 512 is 1024 B, one bank slot for all of them without the gap; with 16 the lanes of every
// ds_read_b128 group fall on 16 different slots for hop a multiple of 128.
// A wave owns whole column tiles, so no reduction crosses waves.  Every kernel keeps its own LDS carve-up, barriers, tile loops and
// what it does with the accumulators; everything here inlines into it.
// basis: [3 planes][2 * nbp / 16 tiles][kp / 32][64][8], kp = n_fft rounded up to 32 (zero columns beyond n_fft);
//        tile 2j = window * cos of bins 16j .. 16j + 15, tile 2j + 1 = window * sin
// filt : [3 planes][mp / 16 tiles][nbp / 32][64][8]
#pragma once
#include "common.h"

struct Bf3 { bf16_t h, m, l; };
__device__ __forceinline__ Bf3 split3(float v) {       // hi + mid + lo = v: the remainders are exact in fp32
    Bf3 o;
    o.h = f2bf(v);
    v -= bf2f(o.h);
    o.m = f2bf(v);
    v -= bf2f(o.m);
    o.l = f2bf(v);
    return o;
}

// v as its three terms at position pos of three planes `stride` elements apart
template <typename S, typename P>
__device__ __forceinline__ void put3(bf16_t* planes, S stride, P pos, float v) {
    const Bf3 s = split3(v);
    planes[pos] = s.h;
    planes[stride + pos] = s.m;
    planes[2 * stride + pos] = s.l;
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

// position of sample q of the span in a plane, and the elements of a plane that holds n samples
template <int GAP>
__host__ __device__ __forceinline__ int spec_pos(int q, int hop) {
    if constexpr (GAP > 0) return q + GAP * (q / hop);
    else return q;
}
template <int GAP>
__host__ __device__ __forceinline__ int spec_plane(int n, int hop) {
    if constexpr (GAP > 0) return n + GAP * ((n + hop - 1) / hop);
    else return n;
}

// stage 0: samples first .. first + real - 1 of the unpadded row x (len valid samples), times gain, -> xs[3][SP]; the elements
// real .. fill - 1 (the K padding: they multiply zero basis columns and only have to be finite) are zeros.
template <int GAP>
__device__ __forceinline__ void spec_stage(const float* __restrict__ x, int len, long first, int real, int fill, float gain, int hop,
                                           bf16_t* xs, int SP, int tid, int nthreads) {
    for (int q = tid; q < fill; q += nthreads) {
        long i = first + q;
        if (i < 0) i = -i;
        if (i >= len) i = 2L * (len - 1) - i;
        // beyond one reflection: only frames past the member's last reach there, and those enter no result
        const float v = (q < real && i >= 0 && i < len) ? __fmul_rn(x[i], gain) : 0.f;
        put3(xs, SP, spec_pos<GAP>(q, hop), v);
    }
}

// stage 1: bins 16j .. 16j + 15 of the 16 frames of NSIG signals (planes xs[s][3][SP]) against one load of the basis fragments.
// C layout: lane (g, l16) holds frames 4g .. 4g + 3 of bin 16j + l16.  PB: elements per basis plane, nkt = kp / 32.
template <int NSIG, int GAP>
__device__ __forceinline__ void spec_dft_tile(const bf16_t* const (&xs)[NSIG], int SP, int hop, const bf16_t* __restrict__ basis, long PB,
                                              int nkt, int j, int lane, float4_t (&re)[NSIG], float4_t (&im)[NSIG]) {
    static_assert(NSIG == 1 || NSIG == 2);
    const int g = lane >> 4, l16 = lane & 15;
    const bf16_t* wc = basis + (long)(2 * j) * nkt * 512 + lane * 8;
    const bf16_t* ws = wc + (long)nkt * 512;
#pragma unroll
    for (int n = 0; n < NSIG; ++n) re[n] = im[n] = float4_t{0.f, 0.f, 0.f, 0.f};
    auto step = [&](int kt) {
        const int off = l16 * (hop + GAP) + spec_pos<GAP>(kt * 32 + g * 8, hop);
        short8_t a[NSIG][3], c[3], s[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int n = 0; n < NSIG; ++n) a[n][p] = ld8(xs[n] + p * SP + off);
            c[p] = ld8(wc + p * PB + (long)kt * 512);
            s[p] = ld8(ws + p * PB + (long)kt * 512);
        }
#pragma unroll
        for (int n = 0; n < NSIG; ++n) {
            re[n] = mfma6(a[n], c, re[n]);
            im[n] = mfma6(a[n], s, im[n]);
        }
    };
    if constexpr (NSIG == 1) {
#pragma unroll 2
        for (int kt = 0; kt < nkt; ++kt) step(kt);
    } else {                                            // four accumulators and two A fragments: the loop stays rolled
        for (int kt = 0; kt < nkt; ++kt) step(kt);
    }
}

// the spectrum value v of (frame, column col) -> mg[3][16][MS]; MS = columns + 8: 16-byte aligned rows, 4 banks apart
__device__ __forceinline__ void spec_store3(bf16_t* mg, int MS, int frame, int col, float v) {
    put3(mg + frame * MS + col, 16 * MS, 0, v);         // the element's address first: the plane offsets stay wave-uniform
}

// stage 2: mels 16mt .. 16mt + 15 of the 16 frames in mg[3][16][MS]; the same C layout.  PF: elements per filter plane, nk2 = nbp / 32.
__device__ __forceinline__ float4_t spec_mel_tile(const bf16_t* mg, int MS, const bf16_t* __restrict__ filt, long PF, int nk2, int mt,
                                                  int lane) {
    const bf16_t* ma = mg + (lane & 15) * MS + (lane >> 4) * 8;
    const bf16_t* wf = filt + (long)mt * nk2 * 512 + lane * 8;
    float4_t acc = {0.f, 0.f, 0.f, 0.f};
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
    return acc;
}
