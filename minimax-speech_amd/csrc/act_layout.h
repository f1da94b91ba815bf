// The A-fragment order of an activation matrix (the ONE statement of it: csrc/llm.hip and csrc/decode.hip index through here).
// A [rows][K] activation whose consumer is an MFMA projection is kept, per 16-row tile m and k-block kb, in the order the
// A operand wants it, so that a fragment load is one contiguous 1 KiB per wave-instruction:
//     xp[m][kb][lane = g*16 + l16][j]  <->  x[m*16 + l16][kb*KB + g*E + j]        E = 8 (16-bit elements) / 4 (fp32), KB = 4E
// (include/mmx_hip.h: MMX_X_PACKED / MMX_OUT_PACKED, and each plane of the split-plane activations of mmx_skinny2).
#pragma once
#include "common.h"

// element index of (row, col) in an activation of nkb = K / KB k-blocks.  I: the index type.  csrc/decode.hip keeps `int` (all of
// its index arithmetic is 32-bit and free of divisions: a 64-bit division is ~150 scalar instructions on this ISA; its entry
// point bounds B <= 32 and the plane bytes < 2 GiB).  csrc/llm.hip keeps `long`, as it always indexed: its entry points bound
// neither N nor B * Hq.  Both give the same number wherever it fits 31 bits - every shape of the engines (B <= 64 rows and
// N < 2^21 columns: index < 64 * 2^21 = 2^27).
template <int E, typename I>
__device__ __forceinline__ I act_index(int row, int col, int nkb) {
    static_assert(E == 8 || E == 4, "16-bit or 32-bit elements");
    constexpr int LE = E == 8 ? 3 : 2, KB = 4 * E;     // shifts and masks (col >= 0): what csrc/decode.hip's epilogues always had
    return (((((I)(row >> 4) * nkb + (col >> (LE + 2))) << 6) + (((col & (KB - 1)) >> LE) << 4) + (row & 15)) << LE) + (col & (E - 1));
}

// v -> NS bf16 terms (NS = 3: hi + mid + lo = v; NS = 1, the bf16 build: bf16(v)) at `idx` of planes `ps` elements apart;
// F16: NS fp16 terms (round to nearest each; the remainder of a rounded fp32 value is exact in fp32)
template <int NS, bool F16 = false, typename I>
__device__ __forceinline__ void store_split(bf16_t* planes, I ps, I idx, float v) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if constexpr (F16) {
            const _Float16 h = (_Float16)v;
            planes[s * ps + idx] = __builtin_bit_cast(unsigned short, h);
            v -= (float)h;
        } else {
            const bf16_t h = f2bf(v);
            planes[s * ps + idx] = h;
            v -= bf2f(h);
        }
    }
}

// RoPE (HF rotate_half) of the channel pair (d, d + 32) of a 64-channel head at position p: cos / sin from rope_tab
// ([pos][cos 0..31 | sin 0..31], computed like HF on the host) or, without a table, cosf / sinf of p * inv_freq[d]
__device__ __forceinline__ void rope_pair(const float* __restrict__ rope_tab, const float* __restrict__ inv_freq, int p, int d,
                                          float x0, float x1, float& y0, float& y1) {
    float c, s;
    if (rope_tab) {
        c = rope_tab[(long)p * 64 + d];
        s = rope_tab[(long)p * 64 + 32 + d];
    } else {
        const float ang = (float)p * inv_freq[d];
        c = cosf(ang);
        s = sinf(ang);
    }
    y0 = x0 * c - x1 * s;
    y1 = x1 * c + x0 * s;
}
