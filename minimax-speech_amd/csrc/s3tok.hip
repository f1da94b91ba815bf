// The S3 speech tokenizer's own kernels (speech/tools/S3Tokenizer/s3tokenizer/model_v2.py:51-70,83-112,177-189) for gfx950; its
// log-mel is mmx_logmel_w of mel.hip, everything else of the tokenizer runs on mmx_gemm_win / mmx_rownorm / the attention entry points.
//   mmx_s3_rope_fsmn  rotate-half RoPE on q and k in place and r = x + (depthwise31(v m) + v m) m in one launch, one wave per head
//   mmx_fsq_encode    project_down -> tanh -> * 0.999 -> round half to even -> base-3 index, one wave per row
// One fp32 arithmetic for every build; every sum runs in a fixed order that depends on neither the tiling nor the batch.
#include "common.h"
#include "../../include/mmx_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------ RoPE + FSMN memory
constexpr int RF_TT = 32;                               // output rows per wave
constexpr int RF_TAPS = 31, RF_HALF = 15;

// grid (time tiles, heads, batch), one wave: lane = channel of the head.  q / k are rotated in place (lane d and lane d ^ 32
// of the same wave hold the pair, both read before either writes).
__global__ __launch_bounds__(64) void s3_rope_fsmn_kernel(float* __restrict__ qkv, long ldqkv, long qkv_bs, int C,
                                                          const float* __restrict__ x, long x_bs, float* __restrict__ r, long r_bs,
                                                          const float* __restrict__ wt, const float* __restrict__ cs,
                                                          const float* __restrict__ sn, const int* __restrict__ lens, int T) {
    __shared__ float vs[(RF_TT + RF_TAPS - 1) * 64];
    const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z, t0 = blockIdx.x * RF_TT;
    const int c = h * 64 + lane;
    const int len = lens ? min(lens[b], T) : T;
    float* row0 = qkv + (long)b * qkv_bs;
    // v m of rows t0 - 15 .. t0 + TT + 14: zero outside [0, len)
    for (int i = 0; i < RF_TT + RF_TAPS - 1; ++i) {
        const int t = t0 - RF_HALF + i;
        vs[i * 64 + lane] = (t >= 0 && t < len) ? row0[(long)t * ldqkv + 2 * C + c] : 0.f;
    }
    float w[RF_TAPS];
#pragma unroll
    for (int j = 0; j < RF_TAPS; ++j) w[j] = wt[(long)j * C + c];
    __syncthreads();
    const int d = lane & 31;
    const int tend = min(t0 + RF_TT, T);
    for (int t = t0; t < tend; ++t) {
        float* qr = row0 + (long)t * ldqkv + c;
        const float xr = x[(long)b * x_bs + (long)t * C + c];
        float* rr = r + (long)b * r_bs + (long)t * C + c;
        if (t >= len) {                                 // padding row (uniform over the wave)
            *rr = xr;
            qr[0] = 0.f;
            qr[C] = 0.f;
            continue;
        }
        const float* vw = vs + (t - t0) * 64 + lane;
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < RF_TAPS; ++j) acc = __builtin_fmaf(w[j], vw[j * 64], acc);
        *rr = xr + (acc + vw[RF_HALF * 64]);
        const float co = cs[t * 32 + d], si = sn[t * 32 + d];
        const float q = qr[0], k = qr[C];
        const float qp = __shfl_xor(q, 32, 64), kp = __shfl_xor(k, 32, 64);
        const float qrot = lane < 32 ? -qp : qp, krot = lane < 32 ? -kp : kp;
        qr[0] = __fadd_rn(__fmul_rn(q, co), __fmul_rn(qrot, si));     // xq * cos + xq_r * sin, unfused as torch evaluates it
        qr[C] = __fadd_rn(__fmul_rn(k, co), __fmul_rn(krot, si));
    }
}

// ------------------------------------------------------------------------------------------------ FSQ head
constexpr int FQ_ROWS = 4;                              // rows (waves) per workgroup
constexpr float FQ_SCALE = 0.9990000128746033f;

__global__ __launch_bounds__(FQ_ROWS * 64) void fsq_encode_kernel(const float* __restrict__ x, long ldx, long x_bs, int T, int C, int B,
                                                                  const float* __restrict__ W, const float* __restrict__ bias,
                                                                  const int* __restrict__ lens, int* __restrict__ ids, long ld_ids,
                                                                  float* __restrict__ pre) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * FQ_ROWS + (threadIdx.x >> 6);
    if (row >= (long)B * T) return;                     // uniform over the wave
    const int b = (int)(row / T), t = (int)(row % T);
    const int len = lens ? min(lens[b], T) : T;
    int* idp = ids + (long)b * ld_ids + t;
    float* pp = pre ? pre + row * 8 : nullptr;
    if (t >= len) {
        if (lane == 0) *idp = 0;
        if (pp && lane < 8) pp[lane] = 0.f;
        return;
    }
    const float* xr = x + (long)b * x_bs + (long)t * ldx;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < C; c += 64) {
        const float xv = xr[c];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_fmaf(xv, W[(long)i * C + c], acc[i]);
    }
    int id = 0, p3 = 1;
    float mine = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float v = tanhf(wave_sum(acc[i]) + bias[i]) * FQ_SCALE;
        id += ((int)rintf(v) + 1) * p3;
        p3 *= 3;
        if (lane == i) mine = v;
    }
    if (lane == 0) *idp = id;
    if (pp && lane < 8) pp[lane] = mine;
}

}  // namespace

extern "C" int mmx_s3_rope_fsmn(float* qkv, int64_t ldqkv, int64_t qkv_bs, int B, int T, int C, const float* x, int64_t x_bs,
                                float* r, int64_t r_bs, const float* wt, const float* rope_cos, const float* rope_sin,
                                int rope_rows, const int32_t* lens, hipStream_t stream) {
    MMX_CHECK_ARG(qkv && x && r && wt && rope_cos && rope_sin && B > 0 && B <= 65535 && T > 0 && C > 0 && C % 64 == 0 && C / 64 <= 65535);
    MMX_CHECK_ARG(T <= rope_rows);                      // the position is the row index
    MMX_CHECK_ARG(ldqkv >= 3 * (int64_t)C && qkv_bs >= (int64_t)T * ldqkv && x_bs >= (int64_t)T * C && r_bs >= (int64_t)T * C);
    const dim3 grid((T + RF_TT - 1) / RF_TT, C / 64, B);
    hipLaunchKernelGGL(s3_rope_fsmn_kernel, grid, dim3(64), 0, stream, qkv, (long)ldqkv, (long)qkv_bs, C, x, (long)x_bs, r, (long)r_bs,
                       wt, rope_cos, rope_sin, lens, T);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}

extern "C" int mmx_fsq_encode(const float* x, int64_t ldx, int64_t x_bs, int B, int T, int C, const float* W, const float* bias,
                              const int32_t* lens, int32_t* ids, int64_t ld_ids, float* pre, hipStream_t stream) {
    MMX_CHECK_ARG(x && W && bias && ids && B > 0 && T > 0 && C > 0 && ldx >= C && x_bs >= (int64_t)T * ldx && ld_ids >= T);
    const long rows = (long)B * T;
    MMX_CHECK_ARG((rows + FQ_ROWS - 1) / FQ_ROWS <= 0x7fffffffL);
    hipLaunchKernelGGL(fsq_encode_kernel, dim3((unsigned)((rows + FQ_ROWS - 1) / FQ_ROWS)), dim3(FQ_ROWS * 64), 0, stream, x, (long)ldx,
                       (long)x_bs, T, C, B, W, bias, lens, ids, (long)ld_ids, pre);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
