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
//
// nd_criteria_grad is the training form of the same criteria: their weighted batch mean and its gradient with respect to y
// (Generator.compute_loss and loss.backward(), nn_common.py:201-255).  The fused step (utnet_train.hip) calls it between its halves.
#include "nd_common.h"

// The centre window and the refusals that every criteria entry point and the training step share
int nd_loss_window(const char *who, int n, int h, int w, int loss_cs, bool ssim, bool msssim, LossWindow *win) {
    if (n < 1 || h < 1 || w < 1 || h > 16384 || w > 16384 || loss_cs < 0)
        ND_FAIL(ND_EINVAL, "%s: bad shape [%d,3,%d,%d], loss_cs %d (sides <= 16384)", who, n, h, w, loss_cs);
    if (loss_cs > h || loss_cs > w) ND_FAIL(ND_EINVAL, "%s: loss_cs=%d exceeds the image size %dx%d", who, loss_cs, h, w);
    win->Lh = loss_cs > 0 ? loss_cs : h;
    win->Lw = loss_cs > 0 ? loss_cs : w;
    win->oy = (h - win->Lh) / 2;
    win->ox = (w - win->Lw) / 2;
    const int L = win->Lh < win->Lw ? win->Lh : win->Lw;
    if (msssim && L < 161)
        ND_FAIL(ND_EINVAL, "%s: MS-SSIM needs a window of at least 161 pixels (five scales of an 11-tap window), got %d; the reference "
                           "fails below it too (pt_losses.py:20-28)", who, L);
    if (ssim && L < 11) ND_FAIL(ND_EINVAL, "%s: SSIM needs a window of at least 11 pixels, got %d", who, L);
    return ND_OK;
}

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

// where element r (row-major) of plane p of the window lies in a [planes][H][W] tensor
__device__ inline size_t win_addr(const LossWindow &wd, int H, int W, size_t p, int r) {
    const int row = r / wd.Lw, col = r - row * wd.Lw;
    return (p * H + wd.oy + row) * W + wd.ox + col;
}
// d = clip(y, 0, 1) - t;  *g = the clipped value (Generator.denoise_batch, nn_common.py:198-199)
__device__ inline float clip_diff(float y, float t, float *g) {
    *g = fminf(fmaxf(y, 0.f), 1.f);
    return *g - t;
}

// grid (groups per sample, n).  y, t: [n][3][H][W];  partial: [n][groups];  gc, tc (nullable together): [n][3][Lh][Lw]
__global__ __launch_bounds__(kThreads) void k_criteria_partial(const float *__restrict__ y, const float *__restrict__ t, int H, int W,
                                                               LossWindow wd, float2 *__restrict__ partial, float *__restrict__ gc,
                                                               float *__restrict__ tc) {
    __shared__ float2 red[kThreads / 64];
    const int sample = blockIdx.y;
    const int plane = wd.Lh * wd.Lw, elems = 3 * plane;     // elems > 3 * 16384^2 is refused on the host: fits int
    const size_t dst0 = (size_t)sample * elems;
    const int e0 = blockIdx.x * kChunk + threadIdx.x;
    float2 acc = make_float2(0.f, 0.f);
#pragma unroll 4
    for (int k = 0; k < kChain; ++k) {
        const int e = e0 + k * kThreads;
        if (e >= elems) break;
        const int c = e / plane;
        const size_t src = win_addr(wd, H, W, (size_t)sample * 3 + c, e - c * plane);
        const float tv = t[src];
        float g;
        const float d = clip_diff(y[src], tv, &g);
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
    int groups;
    float2 *partial;
    float *scores, *gc, *tc;
    void *ssim_ws;
    size_t ssim_ws_bytes, bytes;
};
size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
CriteriaPlan criteria_plan(int n, const LossWindow &wd, char *base) {
    CriteriaPlan p;
    const size_t elems = (size_t)3 * wd.Lh * wd.Lw;
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
    p.ssim_ws_bytes = nd_ssim_workspace_bytes(n, 3, wd.Lh, wd.Lw);
    off += align256(p.ssim_ws_bytes);
    p.bytes = off;
    return p;
}

// ------------------------------------------------------------------ the training form: the batch loss and its gradient
constexpr int kLossBlocks = 1024;
// where element i of the contiguous windows [planes][Lh][Lw] lies in [planes][H][W]
__device__ inline size_t win_addr(const LossWindow &wd, int H, int W, long i) {
    const int plane = wd.Lh * wd.Lw;
    const long p = i / plane;
    return win_addr(wd, H, W, (size_t)p, (int)(i - p * plane));
}
// loss = w_l1 * mean|d| + w_mse * mean d^2 over the n window elements of the batch, d = clip(y, 0, 1) - t, and gy = d loss / d y at
// the window's addresses of the full-size gradient (nn_common.py:198-199, 236-255).  grid kLossBlocks x 256 walks the windows in
// linear order; partial[block]: the block's sum.  gc, tc (each nullable): the clipped window of y and the window of t, contiguous
// -- the operands of the SSIM terms
__global__ __launch_bounds__(256) void k_loss_grad(const float *__restrict__ y, const float *__restrict__ t, int H, int W, LossWindow wd,
                                                   long n, float w_l1, float w_mse, float *__restrict__ gy, float *__restrict__ partial,
                                                   float *__restrict__ gc, float *__restrict__ tc) {
    __shared__ float red[256];
    float acc = 0.f;
    const float inv = 1.f / (float)n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const size_t a = win_addr(wd, H, W, i);
        const float v = y[a], tv = t[a];
        float c;
        const float d = clip_diff(v, tv, &c);
        acc += w_l1 * fabsf(d) + w_mse * d * d;
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float pass = (v >= 0.f && v <= 1.f) ? 1.f : 0.f;   // clamp passes the gradient on [min, max]
        gy[a] = pass * (w_l1 * sgn + w_mse * 2.f * d) * inv;
        if (gc) gc[i] = c;
        if (tc) tc[i] = tv;
    }
    acc = nd_block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
// SSIM / MS-SSIM act on clip(y, 0, 1): gy += [0 <= y <= 1] * g, g = their gradient with respect to the clipped window
__global__ void k_add_clip_grad(const float *__restrict__ y, int H, int W, LossWindow wd, const float *__restrict__ g, long n,
                                float *__restrict__ gy) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const size_t a = win_addr(wd, H, W, i);
        const float v = y[a];
        if (v >= 0.f && v <= 1.f) gy[a] += g[i];
    }
}

struct GradPlan {
    float *partial, *gc, *tc, *gssim;   // the three windows: [n][3][Lh][Lw]
    void *ssim_ws;
    size_t ssim_ws_bytes, bytes;
};
// tc is laid out whether or not the window is cut, so that the size for loss_cs = 0 serves every loss_cs of the same (n, h, w)
GradPlan grad_plan(int n, const LossWindow &wd, char *base) {
    GradPlan p;
    const size_t img = align256((size_t)n * 3 * wd.Lh * wd.Lw * sizeof(float));
    size_t off = 0;
    p.partial = (float *)(base + off);
    off += align256(kLossBlocks * sizeof(float));
    for (float **pp : {&p.gc, &p.tc, &p.gssim}) {
        *pp = (float *)(base + off);
        off += img;
    }
    p.ssim_ws = base + off;
    p.ssim_ws_bytes = nd_ssim_loss_workspace_bytes(n, 3, wd.Lh, wd.Lw);
    off += align256(p.ssim_ws_bytes);
    p.bytes = off;
    return p;
}
}  // namespace

extern "C" size_t nd_criteria_workspace_bytes(int n, int h, int w, int loss_cs) {
    LossWindow wd;
    if (n > 65535 || nd_loss_window("nd_criteria", n, h, w, loss_cs, false, false, &wd) != ND_OK) return 0;
    return criteria_plan(n, wd, nullptr).bytes;
}

extern "C" int nd_criteria(const float *y, const float *target, int n, int h, int w, int loss_cs, float w_l1, float w_mse,
                           float w_ssim, float w_msssim, int also, float *out, void *ws, size_t ws_bytes, void *stream) {
    if (n > 65535) ND_FAIL(ND_EINVAL, "nd_criteria: n=%d (n <= 65535)", n);
    if (also & ~15) ND_FAIL(ND_EINVAL, "nd_criteria: unknown column bits 0x%x", also);
    const bool do_l1 = w_l1 != 0.f || (also & 1), do_mse = w_mse != 0.f || (also & 2);
    const bool do_ssim = w_ssim != 0.f || (also & 4), do_msssim = w_msssim != 0.f || (also & 8);
    LossWindow wd;
    ND_TRY(nd_loss_window("nd_criteria", n, h, w, loss_cs, do_ssim, do_msssim, &wd));
    if (!y || !target || !out || !ws) ND_FAIL(ND_EINVAL, "nd_criteria: null pointer");
    const CriteriaPlan p = criteria_plan(n, wd, (char *)ws);
    if (ws_bytes < p.bytes) ND_FAIL(ND_ENOMEM, "nd_criteria: workspace %zu B given, %zu B needed", ws_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    const bool scores = do_ssim || do_msssim;
    hipLaunchKernelGGL(k_criteria_partial, dim3(p.groups, n), dim3(kThreads), 0, s, y, target, h, w, wd, p.partial,
                       scores ? p.gc : (float *)nullptr, scores ? p.tc : (float *)nullptr);
    ND_HIP(hipGetLastError());
    if (do_ssim) ND_TRY(nd_ssim(p.gc, p.tc, n, 3, wd.Lh, wd.Lw, p.scores, p.ssim_ws, p.ssim_ws_bytes, stream));
    if (do_msssim) ND_TRY(nd_ms_ssim(p.gc, p.tc, n, 3, wd.Lh, wd.Lw, p.scores + n, p.ssim_ws, p.ssim_ws_bytes, stream));
    hipLaunchKernelGGL(k_criteria_final, dim3(n), dim3(64), 0, s, (const float2 *)p.partial, p.groups,
                       (float)(1.0 / (3.0 * wd.Lh * wd.Lw)), do_ssim ? (const float *)p.scores : (const float *)nullptr,
                       do_msssim ? (const float *)(p.scores + n) : (const float *)nullptr, (int)do_l1, (int)do_mse, w_l1, w_mse,
                       w_ssim, w_msssim, out);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

extern "C" size_t nd_criteria_grad_workspace_bytes(int n, int h, int w, int loss_cs) {
    LossWindow wd;
    if (nd_loss_window("nd_criteria_grad", n, h, w, loss_cs, false, false, &wd) != ND_OK) return 0;
    return grad_plan(n, wd, nullptr).bytes;
}

extern "C" int nd_criteria_grad(const float *y, const float *target, int n, int h, int w, int loss_cs, float w_l1, float w_mse,
                                float w_ssim, float w_msssim, float *loss_out, float *gy, void *ws, size_t ws_bytes, void *stream) {
    LossWindow wd;
    ND_TRY(nd_loss_window("nd_criteria_grad", n, h, w, loss_cs, w_ssim != 0.f, w_msssim != 0.f, &wd));
    if (!y || !target || !loss_out || !gy || !ws) ND_FAIL(ND_EINVAL, "nd_criteria_grad: null pointer");
    const GradPlan p = grad_plan(n, wd, (char *)ws);
    if (ws_bytes < p.bytes) ND_FAIL(ND_ENOMEM, "nd_criteria_grad: workspace %zu B given, %zu B needed", ws_bytes, p.bytes);
    hipStream_t s = (hipStream_t)stream;
    const long nwin = (long)n * 3 * wd.Lh * wd.Lw;
    const bool cut = wd.Lh != h || wd.Lw != w, scores = w_ssim != 0.f || w_msssim != 0.f;
    if (cut) ND_HIP(hipMemsetAsync(gy, 0, (size_t)n * 3 * h * w * sizeof(float), s));   // the gradient is zero outside the window
    // the whole image as the window: the target itself is the SSIM operand
    hipLaunchKernelGGL(k_loss_grad, dim3(kLossBlocks), dim3(256), 0, s, y, target, h, w, wd, nwin, w_l1, w_mse, gy, p.partial,
                       scores ? p.gc : (float *)nullptr, scores && cut ? p.tc : (float *)nullptr);
    ND_HIP(hipGetLastError());
    ND_TRY(nd_launch_sum(p.partial, kLossBlocks, 1.f / (float)nwin, loss_out, s));
    if (!scores) return ND_OK;
    const float *tl = cut ? p.tc : target;
    int acc = 0;
    if (w_ssim != 0.f) {
        ND_TRY(nd_ssim_loss_grad(p.gc, tl, n, 3, wd.Lh, wd.Lw, 0, w_ssim, loss_out, p.gssim, acc, p.ssim_ws, p.ssim_ws_bytes, stream));
        acc = 1;
    }
    if (w_msssim != 0.f)
        ND_TRY(nd_ssim_loss_grad(p.gc, tl, n, 3, wd.Lh, wd.Lw, 1, w_msssim, loss_out, p.gssim, acc, p.ssim_ws, p.ssim_ws_bytes, stream));
    hipLaunchKernelGGL(k_add_clip_grad, dim3(1024), dim3(256), 0, s, y, h, w, wd, (const float *)p.gssim, nwin, gy);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
