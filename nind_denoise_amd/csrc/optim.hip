// The optimizer on flat fp32 buffers, for every trainer (UtNetTrainer, UNetTrainer): Adam(amsgrad) in one launch, and the guarded
// step -- the gradient's global norm and its non-finite count in one streaming pass, then Adam behind that verdict.
#include <math.h>

#include <algorithm>

#include "nd_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Adam with amsgrad, torch.optim.Adam semantics (nn_common.py:185): no weight decay
__global__ void k_adam(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                       float *__restrict__ vmax, long n, float lr, float b1, float b2, float eps, float bc1, float bc2,
                       int amsgrad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float vd = vi;
    if (amsgrad) {
        vd = fmaxf(vmax[i], vi);
        vmax[i] = vd;
    }
    const float denom = sqrtf(vd) / sqrtf(bc2) + eps;
    p[i] -= (lr / bc1) * mi / denom;
}

// ------------------------------------------------------------------ guarded optimizer step
// One streaming pass over the flat gradient buffer: partial[2 b] = sum of g^2 (fp32 inputs squared and added in double: the
// square of an fp32 value is exact in double), partial[2 b + 1] = the number of non-finite entries, of workgroup b's share.  A
// thread reads 16-byte elements i, i + stride, ... (four loads in flight per round); thread t < n % 4 of workgroup 0 takes tail
// element 4 (n / 4) + t.  Fixed order, no atomics: the same bits on every run.
constexpr int kGuardMaxBlocks = 1024;
__device__ inline bool guard_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__device__ inline void guard_take(f32x4 v, double &s, double &c) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        s += (double)v[e] * (double)v[e];
        c += guard_nonfinite(v[e]) ? 1.0 : 0.0;
    }
}
__global__ __launch_bounds__(256) void k_grad_guard_partial(const float *__restrict__ g, long n, double *__restrict__ partial) {
    __shared__ double red[256];
    const f32x4 *g4 = (const f32x4 *)g;
    const long n4 = n >> 2, stride = (long)gridDim.x * 256;
    double s = 0.0, c = 0.0;
    long i = (long)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        const f32x4 v0 = g4[i], v1 = g4[i + stride], v2 = g4[i + 2 * stride], v3 = g4[i + 3 * stride];
        guard_take(v0, s, c);
        guard_take(v1, s, c);
        guard_take(v2, s, c);
        guard_take(v3, s, c);
    }
    for (; i < n4; i += stride) guard_take(g4[i], s, c);
    if (blockIdx.x == 0 && (long)threadIdx.x < n - 4 * n4) {
        const float t = g[4 * n4 + threadIdx.x];
        s += (double)t * (double)t;
        c += guard_nonfinite(t) ? 1.0 : 0.0;
    }
    s = nd_block_sum(s, red);
    __syncthreads();
    c = nd_block_sum(c, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = s;
        partial[2 * blockIdx.x + 1] = c;
    }
}
// One workgroup: thread t adds partials [t * per, (t + 1) * per) in index order, then the fixed tree.  state = {sum g^2, non-finite
// count, scale, ok}; scale is the coefficient of torch.nn.utils.clip_grad_norm_ (a NaN norm gives a NaN scale, as torch.clamp
// does: the comparison below is false for NaN)
__global__ __launch_bounds__(256) void k_grad_guard_finish(const double *__restrict__ partial, int nblocks, float max_norm,
                                                           int skip_nonfinite, double *__restrict__ state) {
    __shared__ double red[256];
    const int per = (nblocks + 255) / 256;
    double s = 0.0, c = 0.0;
    for (int k = threadIdx.x * per; k < (int)(threadIdx.x + 1) * per && k < nblocks; ++k) {
        s += partial[2 * k];
        c += partial[2 * k + 1];
    }
    s = nd_block_sum(s, red);
    __syncthreads();
    c = nd_block_sum(c, red);
    if (threadIdx.x != 0) return;
    double scale = 1.0;
    if (max_norm > 0.f) {
        const double q = (double)max_norm / (sqrt(s) + 1e-6);
        scale = q > 1.0 ? 1.0 : q;
    }
    state[0] = s;
    state[1] = c;
    state[2] = scale;
    state[3] = (skip_nonfinite && c > 0.0) ? 0.0 : 1.0;
}
// k_adam behind the guard: ok == 0 -> nothing is touched; else g = grads[i] * (float)scale, one fp32 multiply, and k_adam's
// expressions on it (scale == 1: the same bits as k_adam).  grads is read only.
__global__ void k_adam_guarded(float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v,
                               float *__restrict__ vmax, long n, float lr, float b1, float b2, float eps, float bc1, float bc2,
                               int amsgrad, const double *__restrict__ state) {
    // k_adam's roundings, spelled out: the compiler fuses k_adam's first moment into fma(1 - b1, g, b1 * m) and nothing else
    // (the second moment is two products and a sum).  Left to itself it fuses the other product here, one rounding apart, so
    // contraction is off in this kernel and the one fma is written down.  This restates what ONE compiler does with k_adam: if
    // tests/test_train_guard.py (guarded step == plain step, bit for bit) fails after a toolchain change, look at k_adam's ISA
    // again and write down here whatever it fuses now
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (state[3] == 0.0) return;
    const float sc = (float)state[2];
    const float gi = g[i] * sc;
    const float mi = fmaf(1.f - b1, gi, b1 * m[i]);
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    float vd = vi;
    if (amsgrad) {
        vd = fmaxf(vmax[i], vi);
        vmax[i] = vd;
    }
    const float denom = sqrtf(vd) / sqrtf(bc2) + eps;
    p[i] -= (lr / bc1) * mi / denom;
}

// ------------------------------------------------------------------ C ABI
// Adam's bias correction 1 - b^step, in double on the host and rounded once for the kernel (as torch takes 1 - beta ** step).
// In fp32 the subtraction cancels at small steps: 1 - 0.999^2 = 0.002 carries the 6e-8 spacing of 0.998, 1e-5 of itself, and
// sqrt(bc2) scales every element's update (tests/test_adam_exact.py holds the step to float64 Adam)
static float bias_correction(float b, int step) { return (float)(1.0 - pow((double)b, (double)step)); }

// torch.optim.Adam(params, lr, betas=(b1,b2), eps, amsgrad) on flat buffers; step = 1, 2, ...
extern "C" int nd_adam_step(float *params, const float *grads, float *m, float *v, float *vmax, size_t n, float lr, float b1,
                            float b2, float eps, int step, int amsgrad, void *stream) {
    if (!params || !grads || !m || !v || (amsgrad && !vmax) || step < 1) ND_FAIL(ND_EINVAL, "nd_adam_step: bad arguments");
    const float bc1 = bias_correction(b1, step), bc2 = bias_correction(b2, step);
    hipLaunchKernelGGL(k_adam, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grads, m, v, vmax,
                       (long)n, lr, b1, b2, eps, bc1, bc2, amsgrad);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// workgroups of the guard's streaming pass: a function of n alone (one per 256 16-byte elements, at most kGuardMaxBlocks)
static int guard_blocks(size_t n) {
    const size_t b = (n / 4 + 255) / 256;
    return (int)std::min<size_t>(std::max<size_t>(b, 1), (size_t)kGuardMaxBlocks);
}
extern "C" size_t nd_grad_guard_workspace_bytes(size_t n) { return n ? (size_t)guard_blocks(n) * 2 * sizeof(double) : 0; }
extern "C" int nd_grad_guard(const float *grads, size_t n, float max_norm, int skip_nonfinite, double *state, void *ws, size_t ws_bytes,
                             void *stream) {
    if (!grads || !state || !ws || n == 0) ND_FAIL(ND_EINVAL, "nd_grad_guard: bad arguments");
    if (((uintptr_t)grads & 15) || ((uintptr_t)ws & 7) || ((uintptr_t)state & 7))
        ND_FAIL(ND_EINVAL, "nd_grad_guard: grads must be 16-byte aligned, state and workspace 8-byte aligned");
    if (ws_bytes < nd_grad_guard_workspace_bytes(n))
        ND_FAIL(ND_EINVAL, "nd_grad_guard: workspace of %zu bytes, %zu needed", ws_bytes, nd_grad_guard_workspace_bytes(n));
    const int blocks = guard_blocks(n);
    hipLaunchKernelGGL(k_grad_guard_partial, dim3(blocks), dim3(256), 0, (hipStream_t)stream, grads, (long)n, (double *)ws);
    hipLaunchKernelGGL(k_grad_guard_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double *)ws, blocks, max_norm,
                       skip_nonfinite ? 1 : 0, state);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
// nd_adam_step behind the state nd_grad_guard left (same stream): see include/nind_hip.h
extern "C" int nd_adam_step_guarded(float *params, const float *grads, float *m, float *v, float *vmax, size_t n, float lr, float b1,
                                    float b2, float eps, int step, int amsgrad, const double *state, void *stream) {
    if (!params || !grads || !m || !v || (amsgrad && !vmax) || step < 1 || !state)
        ND_FAIL(ND_EINVAL, "nd_adam_step_guarded: bad arguments");
    const float bc1 = bias_correction(b1, step), bc2 = bias_correction(b2, step);
    hipLaunchKernelGGL(k_adam_guarded, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, params, grads, m, v,
                       vmax, (long)n, lr, b1, b2, eps, bc1, bc2, amsgrad, state);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
