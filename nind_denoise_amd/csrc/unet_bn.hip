// BatchNorm on the statistics of the batch (nn.BatchNorm2d in train() mode) + ReLU, forward and backward: the kernels of the UNet
// training step behind two launchers.  The walk around them is unet_grad.hip's, one for both BatchNorm modes: in train mode the
// weights are packed RAW (no fold), a Conv3 layer runs without activation into a pre-norm buffer z that is kept, and the kernels
// below do the rest:
//   forward   k_bn_stats1 / k_bn_stats2   per channel over the N = B H W interior pixels: S = sum z, SS = sum z^2 in double ->
//                                         mu = S / N, var = SS / N - mu^2 (= E[(z - mu)^2]; in double the cancellation costs
//                                         ~1e-16 E[z^2] / var, nothing at fp32), inv = 1 / sqrt(var + 1e-5); running statistics
//             k_bn_apply                  a = ReLU(gamma xhat + beta), xhat = (z - mu) inv, into the layer's activation buffer
//   backward  k_bn_bwd_red1 / _red2       dbeta = sum g_a m, dgamma = sum g_a m xhat in double (m = [a > 0])
//             k_bn_bwd_apply              g_z = gamma inv (g_a m - dbeta / N - xhat dgamma / N), in place in the gradient buffer
// All sums: one partial per workgroup (plane, image, pixel chunk) into the reduction scratch, then one workgroup per plane (4
// channels) adds them in a fixed order.  No atomics: two calls give the same bits.  z has no border (its pixels are one contiguous
// run per image), activations and gradients are addressed through their borders: every access is an interior pixel.
// mu is kept as an fp32 pair (hi + lo): z - mu then carries no rounding of the mean (an fp32 mu alone shifts every xhat of a
// channel by up to 6e-8 |mu| inv).
#include <algorithm>

#include "nd_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr float kBnEps = 1e-5f;
constexpr int kBnChunkPixels = 4096;   // pixels of one (plane, image) a stage-1 workgroup sums, at least
constexpr int kBnMaxChunks = 64;

// a bordered quad-planar buffer from its first plane in use
struct QView {
    f32x4 *p;
    long np;
    int Hb, Wb, pad;
    __device__ long at(int q, int b, int y, int x) const { return (long)q * np + ((long)b * Hb + y + pad) * Wb + x + pad; }
};
QView view_of(const QpBuf &q, int plane0) { return QView{(f32x4 *)q.base + (long)plane0 * q.np(), q.np(), q.Hb, q.Wb, q.pad}; }

// per-layer statistics kept for the backward: [mu_hi | mu_lo | inv], cout floats each
struct BnStat {
    const float *mu_hi, *mu_lo, *inv;
};

// 4 per-channel values of plane q (workgroup-uniform: scalar loads; no alignment asked of the flat parameter buffer)
__device__ inline f32x4 load4(const float *p, int q) { return f32x4{p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]}; }

// xhat of one pixel's 4 channels
__device__ inline f32x4 bn_xhat(f32x4 z, f32x4 mh, f32x4 ml, f32x4 inv) {
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = ((z[e] - mh[e]) - ml[e]) * inv[e];
    return r;
}

// stage 1 of the statistics: partial[(q * nb + b * nchunk + c) * 2 + {0, 1}] = {sum z, sum z^2} (4 channels each) over pixels
// [c * per, (c + 1) * per) of image b, plane q.  grid (planes, B, nchunk)
__global__ __launch_bounds__(256) void k_bn_stats1(const f32x4 *__restrict__ z, long znp, int HW, int per, f64x4 *__restrict__ partial) {
    __shared__ f64x4 red[256];
    const int q = blockIdx.x, b = blockIdx.y, c = blockIdx.z;
    const f32x4 *zp = z + (long)q * znp + (long)b * HW;
    const int i1 = min(HW, (c + 1) * per);
    f64x4 s = {0., 0., 0., 0.}, ss = {0., 0., 0., 0.};
    for (int i = c * per + threadIdx.x; i < i1; i += 256) {
        const f32x4 v = zp[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = (double)v[e];
            s[e] += d;
            ss[e] += d * d;
        }
    }
    s = nd_block_sum(s, red);
    __syncthreads();
    ss = nd_block_sum(ss, red);
    if (threadIdx.x == 0) {
        f64x4 *o = partial + ((long)q * gridDim.y * gridDim.z + (long)b * gridDim.z + c) * 2;
        o[0] = s;
        o[1] = ss;
    }
}

// the two totals of plane q from its nb partials, in a fixed order; every thread gets them
__device__ inline void bn_totals(const f64x4 *__restrict__ partial, int nb, f64x4 *red, f64x4 &t0, f64x4 &t1) {
    const f64x4 *p = partial + (long)blockIdx.x * nb * 2;
    f64x4 a = {0., 0., 0., 0.}, b = {0., 0., 0., 0.};
    for (int j = threadIdx.x; j < nb; j += 256) {
        a += p[2 * j];
        b += p[2 * j + 1];
    }
    t0 = nd_block_sum(a, red);
    __syncthreads();
    t1 = nd_block_sum(b, red);
}

// stage 2: one workgroup per plane.  mu, inv -> stat; running statistics as torch updates them (unbiased variance)
__global__ __launch_bounds__(256) void k_bn_stats2(const f64x4 *__restrict__ partial, int nb, double N, int cout, float momentum,
                                                   float *__restrict__ stat, float *__restrict__ rm, float *__restrict__ rv) {
    __shared__ f64x4 red[256];
    f64x4 s, ss;
    bn_totals(partial, nb, red, s, ss);
    const int e = threadIdx.x, co = 4 * blockIdx.x + e;
    if (e >= 4 || co >= cout) return;
    const double mu = s[e] / N, var = fmax(ss[e] / N - mu * mu, 0.0);
    const float mh = (float)mu;
    stat[co] = mh;
    stat[cout + co] = (float)(mu - (double)mh);
    stat[2 * cout + co] = (float)(1.0 / sqrt(var + (double)kBnEps));
    const double m = (double)momentum;
    rm[co] = (float)((1.0 - m) * (double)rm[co] + m * mu);
    rv[co] = (float)((1.0 - m) * (double)rv[co] + m * (var * (N / (N - 1.0))));
}

// a = ReLU(gamma xhat + beta).  grid (ceil(H W / 256), B, planes)
__global__ __launch_bounds__(256) void k_bn_apply(const f32x4 *__restrict__ z, long znp, QView a, int H, int W, BnStat st,
                                                  const float *__restrict__ gamma, const float *__restrict__ beta) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, q = blockIdx.z;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const f32x4 xh = bn_xhat(z[(long)q * znp + (long)b * H * W + i], load4(st.mu_hi, q), load4(st.mu_lo, q), load4(st.inv, q));
    const f32x4 g = load4(gamma, q), be = load4(beta, q);
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v = fmaf(g[e], xh[e], be[e]);
        r[e] = v > 0.f ? v : 0.f;
    }
    a.p[a.at(q, b, y, x)] = r;
}

// stage 1 of the backward sums: {sum g m, sum g m xhat}, laid out as k_bn_stats1's partials.  grid (planes, B, nchunk)
__global__ __launch_bounds__(256) void k_bn_bwd_red1(QView g, QView a, const f32x4 *__restrict__ z, long znp, int H, int W, int per,
                                                     BnStat st, f64x4 *__restrict__ partial) {
    __shared__ f64x4 red[256];
    const int q = blockIdx.x, b = blockIdx.y, c = blockIdx.z, HW = H * W;
    const f32x4 mh = load4(st.mu_hi, q), ml = load4(st.mu_lo, q), inv = load4(st.inv, q);
    const int i1 = min(HW, (c + 1) * per);
    f64x4 sb = {0., 0., 0., 0.}, sg = {0., 0., 0., 0.};
    for (int i = c * per + threadIdx.x; i < i1; i += 256) {
        const int y = i / W, x = i - y * W;
        const f32x4 gv = g.p[g.at(q, b, y, x)], av = a.p[a.at(q, b, y, x)];
        const f32x4 xh = bn_xhat(z[(long)q * znp + (long)b * HW + i], mh, ml, inv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double gm = av[e] > 0.f ? (double)gv[e] : 0.0;
            sb[e] += gm;
            sg[e] += gm * (double)xh[e];
        }
    }
    sb = nd_block_sum(sb, red);
    __syncthreads();
    sg = nd_block_sum(sg, red);
    if (threadIdx.x == 0) {
        f64x4 *o = partial + ((long)q * gridDim.y * gridDim.z + (long)b * gridDim.z + c) * 2;
        o[0] = sb;
        o[1] = sg;
    }
}

// stage 2: dbeta, dgamma (to the flat gradient buffer if there is one) and the two coefficients of k_bn_bwd_apply
__global__ __launch_bounds__(256) void k_bn_bwd_red2(const f64x4 *__restrict__ partial, int nb, double N, int cout,
                                                     float *__restrict__ coef, float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ f64x4 red[256];
    f64x4 sb, sg;
    bn_totals(partial, nb, red, sb, sg);
    const int e = threadIdx.x, co = 4 * blockIdx.x + e;
    if (e >= 4 || co >= cout) return;
    coef[co] = (float)(sb[e] / N);
    coef[cout + co] = (float)(sg[e] / N);
    if (dgamma) {
        dgamma[co] = (float)sg[e];
        dbeta[co] = (float)sb[e];
    }
}

// g <- g_z = gamma inv (g m - dbeta / N - xhat dgamma / N), in place.  grid (ceil(H W / 256), B, planes)
__global__ __launch_bounds__(256) void k_bn_bwd_apply(QView g, QView a, const f32x4 *__restrict__ z, long znp, int H, int W, BnStat st,
                                                      const float *__restrict__ gamma, const float *__restrict__ coef, int cout) {
    const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, q = blockIdx.z;
    if (i >= H * W) return;
    const int y = i / W, x = i - y * W;
    const f32x4 inv = load4(st.inv, q);
    const f32x4 xh = bn_xhat(z[(long)q * znp + (long)b * H * W + i], load4(st.mu_hi, q), load4(st.mu_lo, q), inv);
    const f32x4 ga = load4(gamma, q), c1 = load4(coef, q), c2 = load4(coef + cout, q);
    const long gi = g.at(q, b, y, x);
    const f32x4 gv = g.p[gi], av = a.p[a.at(q, b, y, x)];
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float gm = av[e] > 0.f ? gv[e] : 0.f;
        r[e] = (ga[e] * inv[e]) * ((gm - c1[e]) - xh[e] * c2[e]);
    }
    g.p[gi] = r;
}


// pixel chunks of a stage-1 launch: enough workgroups for the wide levels, partials that fit the reduction scratch
int bn_chunks(int planes, int B, int HW, long red_floats, int *nchunk, int *per) {
    const long fit = red_floats / ((long)planes * B * 16);   // 2 x 4 doubles = 16 floats per partial
    if (fit < 1) ND_FAIL(ND_EINVAL, "UNet training: %d planes x %d images do not fit the reduction scratch", planes, B);
    int n = std::min((HW + kBnChunkPixels - 1) / kBnChunkPixels, kBnMaxChunks);
    n = (int)std::min((long)std::max(n, 1), fit);
    *per = (HW + n - 1) / n;
    *nchunk = (HW + *per - 1) / *per;
    return ND_OK;
}

BnStat stat_of(const float *stat, int cout) { return BnStat{stat, stat + cout, stat + 2 * cout}; }
inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// ------------------------------------------------------------------ the two launchers (declared in nd_common.h)
int nd_launch_bn_train_fwd(const QpBuf &z, const QpBuf &a, int plane0, int cout, float momentum, const float *gamma, const float *beta,
                           float *rm, float *rv, float *stat, float *red, long red_floats, hipStream_t s) {
    const int B = z.B, H = z.Hb, W = z.Wb, planes = cout / 4;
    int nchunk, per;
    ND_TRY(bn_chunks(planes, B, H * W, red_floats, &nchunk, &per));
    hipLaunchKernelGGL(k_bn_stats1, dim3(planes, B, nchunk), dim3(256), 0, s, (const f32x4 *)z.base, z.np(), H * W, per, (f64x4 *)red);
    hipLaunchKernelGGL(k_bn_stats2, dim3(planes), dim3(256), 0, s, (const f64x4 *)red, B * nchunk, (double)B * H * W, cout, momentum,
                       stat, rm, rv);
    hipLaunchKernelGGL(k_bn_apply, dim3(blocks_of((long)H * W), B, planes), dim3(256), 0, s, (const f32x4 *)z.base, z.np(),
                       view_of(a, plane0), H, W, stat_of(stat, cout), gamma, beta);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_launch_bn_train_bwd(const QpBuf &g, const QpBuf &a, int plane0, const QpBuf &z, int cout, const float *gamma, const float *stat,
                           float *coef, float *dgamma, float *dbeta, float *red, long red_floats, hipStream_t s) {
    const int B = z.B, H = z.Hb, W = z.Wb, planes = cout / 4;
    const BnStat bs = stat_of(stat, cout);
    const QView gv = view_of(g, plane0), av = view_of(a, plane0);
    int nchunk, per;
    ND_TRY(bn_chunks(planes, B, H * W, red_floats, &nchunk, &per));
    hipLaunchKernelGGL(k_bn_bwd_red1, dim3(planes, B, nchunk), dim3(256), 0, s, gv, av, (const f32x4 *)z.base, z.np(), H, W, per, bs,
                       (f64x4 *)red);
    hipLaunchKernelGGL(k_bn_bwd_red2, dim3(planes), dim3(256), 0, s, (const f64x4 *)red, B * nchunk, (double)B * H * W, cout, coef,
                       dgamma, dbeta);
    hipLaunchKernelGGL(k_bn_bwd_apply, dim3(blocks_of((long)H * W), B, planes), dim3(256), 0, s, gv, av, (const f32x4 *)z.base, z.np(),
                       H, W, bs, gamma, (const float *)coef, cout);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
