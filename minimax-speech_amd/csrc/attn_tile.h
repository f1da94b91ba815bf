// What the MFMA flash kernels share (attention.hip: attn_flash_kernel, attn_relpos_kernel, attn_flash_splitk_kernel;
// attention_x.hip: attn_flash_x_kernel, attn_relpos_x_kernel): the workgroup mapping, the key window of a workgroup, the
// lazy-rescale step of the online softmax, the row sum, and the launchers' grid and tile rules.  Every kernel keeps its
// own loads, LDS layout, MFMA loop, barriers and prefetch; everything here inlines into it.
#pragma once
#include "common.h"

// ------------------------------------------------------------------------------------------ device
struct PairTile { int b, h, qt; bool valid; };
// XCD-aware mapping (1-D grid): the query tiles of one (batch, head) pair read the same K / V^T rows; they get linear ids
// with the same id % 8, i.e. the same XCD and L2, instead of being dealt round robin over all eight.  The grid is padded to
// a multiple of 8 pairs (pair_grid): a workgroup with !valid leaves at once (uniform, before any barrier).
__device__ __forceinline__ PairTile pair_tile(int nq, int nheads, int npairs) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int pair = (slot / nq) * 8 + xcd;
    if (pair >= npairs) return {0, 0, 0, false};
    return {pair / nheads, pair % nheads, slot % nq, true};
}

// The keys a workgroup of queries q0 .. q0 + nqueries - 1 walks, in tiles of 64.
//   Tk       valid keys of batch member b: klen[b] (a padded batch whose masks are prefixes), at most Tn; Tn without klen.
//            Unlike a key mask it is known before the loop: key tiles beyond it are never visited.
//   kend     keys beyond the last query's chunk are invisible to the whole workgroup; ntile = ceil(kend / 64)
//   vis_all  keys below it are visible to EVERY query of the workgroup (its first query's chunk end): those tiles run the
//            unmasked code, only the tiles that reach into the workgroup's own chunks compare
struct KeyWindow { int Tk, kend, ntile, vis_all; };
__device__ __forceinline__ KeyWindow key_window(int Tn, const int32_t* __restrict__ klen, int b, int chunk, int q0, int nqueries) {
    const int Tk = klen ? (klen[b] < Tn ? klen[b] : Tn) : Tn;
    int kend = Tk, vis_all = Tk;
    if (chunk > 0) {
        int qlast = q0 + nqueries - 1;
        if (qlast > Tn - 1) qlast = Tn - 1;
        const int e = (qlast / chunk + 1) * chunk;
        if (e < kend) kend = e;
        const int a = (q0 / chunk + 1) * chunk;
        if (a < vis_all) vis_all = a;
    }
    return {Tk, kend, (kend + 63) / 64, vis_all};
}

// keys j < lane_limit are visible to query i: its chunk's end, at most Tk
__device__ __forceinline__ int lane_limit(int i, int chunk, int Tk) {
    if (chunk <= 0) return Tk;
    const int c2 = (i / chunk + 1) * chunk;
    return c2 < Tk ? c2 : Tk;
}

// One tile's step of the online softmax.  mx: this LANE's maximum of the tile's scores (log2 units; keys 4g + r of the tile's
// four 16-key fragments).  Returns the maximum to subtract in the exponent; moves m_run and rescales l_run and o when it grew.
// Lazy rescale (cdna_hip_programming.md T13): keep the old running max while every score of the wave is at most 2^6 above
// it; p then reaches at most 64 (fine in bf16 / fp32 sums) and the O accumulators (AGPRs: a rescale costs a read + multiply
// + write per value) are left alone.  The test needs no cross-lane maximum (each lane checks its own keys against the query's
// running max, one wave vote), so a steady-state tile has no shuffle at all (ds_bpermute round trips sat on the critical
// path of a one-wave-per-SIMD loop); the four lanes of a query agree on the maximum only when it moves.  m_run stays
// uniform over those four lanes.
__device__ __forceinline__ float lazy_rescale(float mx, float& m_run, float& l_run, float4_t (&o)[4]) {
    float m_use = m_run;
    const bool grow = (mx - m_run) > 6.0f || m_run == -INFINITY;
    if (__any(grow)) {
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float m_safe = m_new == -INFINITY ? 0.f : m_new;
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);   // m_run = -inf -> 0
        l_run *= alpha;
#pragma unroll
        for (int df = 0; df < 4; ++df)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[df][r] *= alpha;
        m_run = m_new;
        m_use = m_safe;
    }
    return m_use;
}

// l_run is a per-lane partial sum (the lane's own keys): the four lanes of a query are added up once, after the last tile
// (all lanes call it: the shuffles come before the row guard)
__device__ __forceinline__ void row_sum(float& l_run) {
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
}

// ------------------------------------------------------------------------------------------ host
// 1-D grid of pair_tile: the (batch, head) pairs padded to a multiple of 8, nq query tiles each
static inline dim3 pair_grid(int npairs, int nq) { return dim3(8 * ((npairs + 7) / 8) * nq); }
// fewer 128-query tiles than ~3/4 of the CUs: such a launch takes 64-query workgroups
static inline bool few_tiles(int npairs, int Tq) { return (long)npairs * ((Tq + 127) / 128) < 192; }
