// Per-sample criteria of a batch: what the validation pass of the training loop averages (nn_train.py:51-71 validate_generator:
// model.compute_loss on one image at a time, nn_common.py:226-241, then statistics.mean of the weighted losses).
//
//   g = clip(y, 0, 1);  with loss_cs > 0 both g and t are cut to the centre loss_cs x loss_cs window (pt_ops.pt_crop_batch)
//   out[i] = { mean|g - t|, mean (g - t)^2, 1 - SSIM_i, 1 - MS-SSIM_i, sum_k w_k * column_k }       (means over c, y, x of sample i)
//
// HBM-bound and small: one pass reads y and target once at the crop offsets (rows of the window are contiguous: coalesced),
// writes the clipped window of g and the window of t contiguously when a score is wanted, and leaves one (sum |d|, sum d^2) pair
// per workgroup in a fixed slot; a workgroup never straddles two samples.  A second launch, one wave per sample, adds the pairs
// in index order, picks up the two scores (the launches of nd_ssim / nd_ms_ssim on the contiguous windows) and writes the five
// columns.  No atomics: the same bits on every run.
// Rounding: a thread adds kChain terms in a row, then the sums meet in trees (6 shuffle levels, 3 additions through LDS, and in the
// second launch ceil(groups / 64) terms per lane and 6 shuffle levels), so the longest serial chain of a sample's sum is
// kChain + 15 + ceil(groups / 64) terms: 32 for a 184 x 184 window, 43 for 1000 x 1000.
#include "nd_common.h"

namespace {
constexpr int kThreads = 256;
constexpr int kChain = 16;                        // elements per thread
constexpr int kChunk = kThreads * kChain;         // elements per workgroup

// sums over the 64 lanes in a fixed tree; the total arrives in lane 0
__device__ inline float2 wave_sum(float2 v) {
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        v.x += __shfl_down(v.x, k, 64);
        v.y += __shfl_down(v.y, k, 64);
    }
    return v;
}

// grid (groups per sample, n).  y, t: [n][3][H][W];  partial: [n][groups];  gc, tc (nullable together): [n][3][Lh][Lw]
__global__ __launch_bounds__(kThreads) void k_criteria_partial(const float *__restrict__ y, const float *__restrict__ t, int H, int W,
                                                               int Lh, int Lw, int oy, int ox, float2 *__restrict__ partial,
                                                               float *__restrict__ gc, float *__restrict__ tc) {
    __shared__ float2 red[kThreads / 64];
    const int sample = blockIdx.y;
    const int plane = Lh * Lw, elems = 3 * plane;           // elems <= 3 * 16384^2 is refused on the host: fits int
    const size_t src0 = (size_t)sample * 3 * H * W, dst0 = (size_t)sample * elems;
    const int e0 = blockIdx.x * kChunk + threadIdx.x;
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int k = 0; k < kChain; ++k) {
        const int e = e0 + k * kThreads;
        if (e >= elems) break;
        const int c = e / plane, r = e - c * plane;
        const int row = r / Lw, col = r - row * Lw;
        const size_t src = src0 + ((size_t)c * H + oy + row) * W + ox + col;
        const float g = fminf(fmaxf(y[src], 0.f), 1.f), tv = t[src];
        const float d = g - tv;
        acc.x += fabsf(d);
        acc.y += d * d;
        if (gc) {
            gc[dst0 + e] = g;
            tc[dst0 + e] = tv;
        }
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float2 s = red[0];
#pragma unroll
        for (int k = 1; k < kThreads / 64; ++k) {
            s.x += red[k].x;
            s.y += red[k].y;
        }
        partial[(size_t)sample * gridDim.x + blockIdx.x] = s;
    }
}

// one wave per sample.  ssim, msssim (nullable): the scores [n];  do_l1 / do_mse: whether columns 0 / 1 are computed
__global__ __launch_bounds__(64) void k_criteria_final(const float2 *__restrict__ partial, int groups, float inv_elems,
                                                       const float *__restrict__ ssim, const float *__restrict__ msssim, int do_l1,
                                                       int do_mse, float w_l1, float w_mse, float w_ssim, float w_msssim,
                                                       float *__restrict__ out) {
    const int sample = blockIdx.x;
    const float2 *p = partial + (size_t)sample * groups;
    float2 acc = make_float2(0.f, 0.f);
    for (int i = threadIdx.x; i < groups; i += 64) {
        acc.x += p[i].x;
        acc.y += p[i].y;
    }
    acc = wave_sum(acc);
    if (threadIdx.x != 0) return;
    float col[4] = {0.f, 0.f, 0.f, 0.f};
    if (do_l1) col[0] = acc.x * inv_elems;
    if (do_mse) col[1] = acc.y * inv_elems;
    if (ssim) col[2] = 1.f - ssim[sample];
    if (msssim) col[3] = 1.f - msssim[sample];
    const float w[4] = {w_l1, w_mse, w_ssim, w_msssim};
    float weighted = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (w[k] != 0.f) weighted += w[k] * col[k];
    float *o = out + (size_t)sample * 5;
    o[0] = col[0];
    o[1] = col[1];
    o[2] = col[2];
    o[3] = col[3];
    o[4] = weighted;
}

struct CriteriaPlan {
    int Lh, Lw, groups;
    float2 *partial;
    float *scores, *gc, *tc;
    void *ssim_ws;
    size_t ssim_ws_bytes, bytes;
};
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
CriteriaPlan criteria_plan(int n, int h, int w, int loss_cs, char *base) {
    CriteriaPlan p;
    p.Lh = loss_cs > 0 ? loss_cs : h;
    p.Lw = loss_cs > 0 ? loss_cs : w;
    const size_t elems = (size_t)3 * p.Lh * p.Lw;
    p.groups = (int)((elems + kChunk - 1) / kChunk);
    size_t off = 0;
    p.partial = (float2 *)(base + off);
    off += align256((size_t)n * p.groups * sizeof(float2));
    p.scores = (float *)(base + off);
    off += align256((size_t)2 * n * sizeof(float));
    p.gc = (float *)(base + off);
    off += align256((size_t)n * elems * sizeof(float));
    p.tc = (float *)(base + off);
    off += align256((size_t)n * elems * sizeof(float));
    p.ssim_ws = base + off;
    p.ssim_ws_bytes = nd_ssim_workspace_bytes(n, 3, p.Lh, p.Lw);
    off += align256(p.ssim_ws_bytes);
    p.bytes = off;
    return p;
}
bool bad_shape(int n, int h, int w, int loss_cs) {
    return n < 1 || n > 65535 || h < 1 || w < 1 || h > 16384 || w > 16384 || loss_cs < 0;
}
}  // namespace

extern "C" size_t nd_criteria_workspace_bytes(int n, int h, int w, int loss_cs) {
    if (bad_shape(n, h, w, loss_cs) || loss_cs > h || loss_cs > w) return 0;
    return criteria_plan(n, h, w, loss_cs, nullptr).bytes;
}

extern "C" int nd_criteria(const float *y, const float *target, int n, int h, int w, int loss_cs, float w_l1, float w_mse,
                           float w_ssim, float w_msssim, int also, float *out, void *ws, size_t ws_bytes, void *stream) {
    if (bad_shape(n, h, w, loss_cs)) ND_FAIL(ND_EINVAL, "nd_criteria: bad shape [%d,3,%d,%d], loss_cs %d (n <= 65535, sides <= 16384)", n, h, w, loss_cs);
    if (also & ~15) ND_FAIL(ND_EINVAL, "nd_criteria: unknown column bits 0x%x", also);
    const int Lh = loss_cs > 0 ? loss_cs : h, Lw = loss_cs > 0 ? loss_cs : w, L = Lh < Lw ? Lh : Lw;
    if (Lh > h || Lw > w) ND_FAIL(ND_EINVAL, "nd_criteria: loss_cs=%d exceeds the image size %dx%d", loss_cs, h, w);
    const bool do_l1 = w_l1 != 0.f || (also & 1), do_mse = w_mse != 0.f || (also & 2);
    const bool do_ssim = w_ssim != 0.f || (also & 4), do_msssim = w_msssim != 0.f || (also & 8);
    if (do_msssim && L < 161)
        ND_FAIL(ND_EINVAL, "nd_criteria: MS-SSIM needs a window of at least 161 pixels (five scales of an 11-tap window), got %d", L);
    if (do_ssim && L < 11) ND_FAIL(ND_EINVAL, "nd_criteria: SSIM needs a window of at least 11 pixels, got %d", L);
    if (!y || !target || !out || !ws) ND_FAIL(ND_EINVAL, "nd_criteria: null pointer");
    const CriteriaPlan p = criteria_plan(n, h, w, loss_cs, (char *)ws);
    if (ws_bytes < p.bytes) ND_FAIL(ND_ENOMEM, "nd_criteria: workspace %zu B given, %zu B needed", ws_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    const bool scores = do_ssim || do_msssim;
    hipLaunchKernelGGL(k_criteria_partial, dim3(p.groups, n), dim3(kThreads), 0, s, y, target, h, w, Lh, Lw, (h - Lh) / 2, (w - Lw) / 2,
                       p.partial, scores ? p.gc : (float *)nullptr, scores ? p.tc : (float *)nullptr);
    ND_HIP(hipGetLastError());
    if (do_ssim) ND_TRY(nd_ssim(p.gc, p.tc, n, 3, Lh, Lw, p.scores, p.ssim_ws, p.ssim_ws_bytes, stream));
    if (do_msssim) ND_TRY(nd_ms_ssim(p.gc, p.tc, n, 3, Lh, Lw, p.scores + n, p.ssim_ws, p.ssim_ws_bytes, stream));
    hipLaunchKernelGGL(k_criteria_final, dim3(n), dim3(64), 0, s, (const float2 *)p.partial, p.groups, (float)(1.0 / (3.0 * Lh * Lw)),
                       do_ssim ? (const float *)p.scores : (const float *)nullptr,
                       do_msssim ? (const float *)(p.scores + n) : (const float *)nullptr, (int)do_l1, (int)do_mse, w_l1, w_mse,
                       w_ssim, w_msssim, out);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
