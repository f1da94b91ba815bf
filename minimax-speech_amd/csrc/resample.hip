// Sample-rate conversion of a ragged batch of mono fp32 clips in one launch for gfx950: the polyphase windowed-sinc FIR that
// torchaudio documents as `sinc_interp_hann` (cosyvoice/utils/file_utils.py:44-50, cli/frontend.py:157-162).
//   rates reduced by their gcd to o -> n;  output j = frame f * n + phase p;  y[j] = sum_k h[p][k] * x[f * o + k - width]
// The bank arrives packed (mmx/resample.py): per phase the first live tap of the dense row and the live count (a tap with
// |t| >= lowpass_filter_width is exactly 0 in fp32), the live taps themselves tap-major, taps[c][p], so the lanes of a wave -
// adjacent outputs, adjacent phases - read adjacent LDS banks.
// One workgroup owns RS_NOUT consecutive outputs of one clip.  It copies the packed bank and the input span under its outputs
// (zero outside [0, len)) into LDS with coalesced loads, then every thread sums RS_PER outputs, RS_THREADS apart: one thread per
// output, taps ascending, explicit fmaf.  An output's bits therefore depend on its own taps and samples only, not on the batch,
// the row or the workgroup.
#include "common.h"
#include "../../include/mmx_hip.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PER = MMX_RESAMPLE_NOUT / RS_THREADS;
constexpr size_t RS_LDS_MAX = 64 * 1024;                // no opt-in, and two or more workgroups per CU
static_assert(MMX_RESAMPLE_NOUT % RS_THREADS == 0);

__host__ __device__ __forceinline__ long rs_out_len(long len, int o, int n) { return ((long)n * len + o - 1) / o; }

// input samples under RS_NOUT consecutive outputs: their centres span (RS_NOUT - 1) * o / n samples, each reaches less than
// lowpass_filter_width * o / base <= width samples to either side
__host__ __device__ __forceinline__ int rs_span(int o, int n, int width) {
    return (int)(((long)(MMX_RESAMPLE_NOUT - 1) * o + n - 1) / n) + 2 * width + 2;
}

__global__ __launch_bounds__(RS_THREADS) void resample_sinc_kernel(const float* __restrict__ wave, long w_bs, int L,
                                                                   const int* __restrict__ lens, int o, int n, int width,
                                                                   const float* __restrict__ taps, const int* __restrict__ first,
                                                                   const int* __restrict__ count, int cmax,
                                                                   float* __restrict__ out, long o_bs, int out_cols) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* hs = reinterpret_cast<float*>(smem);         // [cmax][n]
    float* xs = hs + cmax * n;                          // [span]
    const int tid = threadIdx.x, b = blockIdx.y;
    const int j0 = blockIdx.x * MMX_RESAMPLE_NOUT;      // < out_cols
    const int len = row_len(lens, b, L);
    const long olen = rs_out_len(len, o, n);
    float* y = out + (long)b * o_bs;

    if (j0 >= olen) {                                   // a run of tail columns (uniform over the workgroup): zeros
#pragma unroll
        for (int r = 0; r < RS_PER; ++r) {
            const int j = j0 + r * RS_THREADS + tid;
            if (j < out_cols) y[j] = 0.f;
        }
        return;
    }

    const int span = rs_span(o, n, width);
    const int f0 = j0 / n, p0 = j0 - f0 * n;
    const long s0 = (long)f0 * o + first[p0] - width;   // first sample of the span (may be negative: zeros)
    const float* x = wave + (long)b * w_bs;
    for (int q = tid; q < cmax * n; q += RS_THREADS) hs[q] = taps[q];
    for (int q = tid; q < span; q += RS_THREADS) {
        const long i = s0 + q;
        xs[q] = (i >= 0 && i < len) ? x[i] : 0.f;
    }
    __syncthreads();

    int p[RS_PER], s[RS_PER], cnt[RS_PER];
    float acc[RS_PER];
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) {
        const int j = j0 + r * RS_THREADS + tid;
        const int jc = j < olen ? j : j0;               // beyond the clip's outputs: no taps
        const int f = jc / n;
        p[r] = jc - f * n;
        const long sr = (long)f * o + first[p[r]] - width - s0;
        cnt[r] = j < olen ? min(count[p[r]], cmax) : 0;
        // the span holds every sample a bank built by mmx/resample.py reaches; whatever the tables say, nothing outside it is read
        if (sr < 0 || sr + cnt[r] > span) cnt[r] = 0;
        s[r] = (int)sr;
        acc[r] = 0.f;
    }
    for (int c = 0; c < cmax; ++c) {
#pragma unroll
        for (int r = 0; r < RS_PER; ++r)
            if (c < cnt[r]) acc[r] = __builtin_fmaf(hs[c * n + p[r]], xs[s[r] + c], acc[r]);
    }
#pragma unroll
    for (int r = 0; r < RS_PER; ++r) {
        const int j = j0 + r * RS_THREADS + tid;
        if (j < out_cols) y[j] = acc[r];                // cnt = 0 beyond the clip's outputs: zero
    }
}

int rs_gcd(int a, int b) {
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    return a;
}

}  // namespace

extern "C" int mmx_resample_sinc(const float* wave, int64_t w_bs, int L, int B, const int32_t* lens, const int32_t* h_lens, int orig,
                                 int neu, int width, const float* taps, const int32_t* first, const int32_t* count, int cmax,
                                 float* out, int64_t o_bs, int out_cols, hipStream_t stream) {
    MMX_CHECK_ARG(wave && taps && first && count && out && out_cols > 0);
    MMX_CHECK_ARG(orig > 0 && neu > 0 && orig != neu && rs_gcd(orig, neu) == 1 && width > 0 && cmax > 0 && cmax <= 2 * width);
    MMX_CHECK_ARG(w_bs >= L && o_bs >= out_cols && out_cols <= INT32_MAX - MMX_RESAMPLE_NOUT);
    if (int rc = rows_form(B, L, lens, h_lens, 1)) return rc;
    // the layout's limit: the packed bank and one workgroup's input span share 64 KB of LDS
    const long bank = (long)cmax * neu, span = ((long)(MMX_RESAMPLE_NOUT - 1) * orig + neu - 1) / neu + 2L * width + 2;
    MMX_CHECK_ARG((bank + span) * (long)sizeof(float) <= (long)RS_LDS_MAX);
    long omax = 0;
    for (int b = 0; b < B; ++b) omax = max(omax, rs_out_len(h_lens ? h_lens[b] : L, orig, neu));
    MMX_CHECK_ARG(out_cols >= omax);                    // every output a clip has fits its row
    const size_t lds = (size_t)(bank + span) * sizeof(float);
    const dim3 grid((out_cols + MMX_RESAMPLE_NOUT - 1) / MMX_RESAMPLE_NOUT, B), block(RS_THREADS);
    hipLaunchKernelGGL(resample_sinc_kernel, grid, block, lds, stream, wave, (long)w_bs, L, lens, orig, neu, width, taps, first, count,
                       cmax, out, (long)o_bs, out_cols);
    MMX_LAUNCH_CHECK();
    return MMX_OK;
}
