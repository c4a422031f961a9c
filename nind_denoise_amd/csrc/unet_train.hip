// UNet training step halves: BatchNorm on the statistics of the batch (nn.BatchNorm2d in train() mode), forward and backward.
// Everything around the BatchNorm layer is the eval-mode machinery of unet_grad.hip on the same plan (unet_grad_net.h): the conv
// kernels in both roles, k_wgrad, the pool adjoint, the 1x1 head.  The weights are packed RAW (no fold), a Conv3 layer runs without
// activation into a pre-norm buffer z that is kept, and the kernels below do the rest:
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
#include "unet_grad_net.h"

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

// ------------------------------------------------------------------ plan
constexpr int kCoefFloats = 2 * 512;
struct TrainPlan {
    GradPlan g;
    QpBuf z[kNumSteps];      // pre-norm output of step i (BatchNorm layers only): cout / 4 planes on the level's grid, no border
    float *stat[kNumSteps];  // [mu_hi | mu_lo | inv] of step i
    float *coef;             // dbeta / N, dgamma / N of the layer in flight
    size_t bytes;
};
TrainPlan make_train_plan(int h, int w, int B, char *base) {
    TrainPlan t;
    t.g = make_grad_plan(h, w, B, base);
    size_t off = t.g.bytes;
    const auto &L = layers();
    for (int i = 0; i < kNumSteps; ++i) {
        const UStep &st = kSteps[i];
        t.z[i] = QpBuf();
        t.stat[i] = nullptr;
        if (st.layer < 0 || L[st.layer].bn.empty()) continue;
        const QpBuf &o = t.g.fwd.buf[st.dst];
        QpBuf &q = t.z[i];
        q.planes = L[st.layer].cout / 4;
        q.B = B;
        q.Hb = o.Hb - 2 * o.pad;
        q.Wb = o.Wb - 2 * o.pad;
        q.pad = 0;
        q.dt = ND_F32;
        q.pstride = (long)B * q.Hb * q.Wb;
        q.base = (float *)(base ? base + off : nullptr);
        off += ((size_t)q.planes * q.pstride + nd_buf_slack(q.Wb)) * 16;
        off = (off + 255) & ~(size_t)255;
    }
    for (int i = 0; i < kNumSteps; ++i) {
        if (!t.z[i].planes) continue;
        t.stat[i] = (float *)(base ? base + off : nullptr);
        off += (size_t)3 * 4 * t.z[i].planes * 4;
        off = (off + 255) & ~(size_t)255;
    }
    t.coef = (float *)(base ? base + off : nullptr);
    off += (size_t)kCoefFloats * 4;
    off = (off + 255) & ~(size_t)255;
    t.bytes = off;
    return t;
}

int check_train(int h, int w, int batch) {
    ND_TRY(check_grad(h, w, batch));
    if ((long)batch * (h / 16) * (w / 16) < 2)
        ND_FAIL(ND_EINVAL, "UNet training: %dx%dx%d leaves one value per channel at the bottom level (BatchNorm in training needs more than 1)",
                batch, h, w);
    return ND_OK;
}

// pixel chunks of a stage-1 launch: enough workgroups for the wide levels, partials that fit the reduction scratch
int bn_chunks(int planes, int B, int HW, int *nchunk, int *per) {
    const long fit = (long)kRedFloats / ((long)planes * B * 16);   // 2 x 4 doubles = 16 floats per partial
    if (fit < 1) ND_FAIL(ND_EINVAL, "UNet training: %d planes x %d images do not fit the reduction scratch", planes, B);
    int n = std::min((HW + kBnChunkPixels - 1) / kBnChunkPixels, kBnMaxChunks);
    n = (int)std::min((long)std::max(n, 1), fit);
    *per = (HW + n - 1) / n;
    *nchunk = (HW + *per - 1) / *per;
    return ND_OK;
}

struct TrainCtx {
    TrainPlan t;
    UParams pl;
    Blob bl;
    GradBlob gb;
    float *blobs;
    hipStream_t s;
};
int train_ctx(TrainCtx &c, int flags, const float *params, void *blobs, int batch, int h, int w, void *ws, size_t ws_bytes, void *stream) {
    ND_TRY(nd_check_flags(flags, false, true));
    ND_TRY(check_train(h, w, batch));
    if (!params || !blobs || !ws) ND_FAIL(ND_EINVAL, "UNet training: null pointer");
    c.t = make_train_plan(h, w, batch, (char *)ws);
    if (ws_bytes < c.t.bytes) ND_FAIL(ND_ENOMEM, "UNet training workspace: %zu B given, %zu B needed", ws_bytes, c.t.bytes);
    c.pl = param_layout();
    c.bl = blob_layout();
    c.gb = grad_blob_layout();
    c.blobs = (float *)blobs;
    c.s = (hipStream_t)stream;
    return ND_OK;
}

BnStat stat_of(const float *stat, int cout) { return BnStat{stat, stat + cout, stat + 2 * cout}; }

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t nd_unet_train_blob_bytes(void) { return grad_blob_layout().total * sizeof(float); }
extern "C" size_t nd_unet_train_workspace_bytes(int h, int w, int batch) {
    if (check_train(h, w, batch) != ND_OK) return 0;
    return make_train_plan(h, w, batch, nullptr).bytes;
}
extern "C" int nd_unet_train_workspace_init(void *ws, size_t ws_bytes, int h, int w, int batch, void *stream) {
    ND_TRY(check_train(h, w, batch));
    const size_t need = make_train_plan(h, w, batch, nullptr).bytes;
    if (!ws || ws_bytes < need) ND_FAIL(ND_ENOMEM, "UNet training workspace: %zu B given, %zu B needed", ws_bytes, need);
    ND_HIP(hipMemsetAsync(ws, 0, need, (hipStream_t)stream));   // zero borders of activations AND gradients, fix-up lines, slack
    return ND_OK;
}

extern "C" int nd_unet_train_forward(int flags, float *params, void *blobs, const float *x, float *y, int batch, int h, int w,
                                     float momentum, void *ws, size_t ws_bytes, void *stream) {
    if (!x || !y) ND_FAIL(ND_EINVAL, "nd_unet_train_forward: null pointer");
    if (!(momentum >= 0.f && momentum <= 1.f)) ND_FAIL(ND_EINVAL, "nd_unet_train_forward: momentum %g outside [0, 1]", (double)momentum);
    TrainCtx c;
    ND_TRY(train_ctx(c, flags, params, blobs, batch, h, w, ws, ws_bytes, stream));
    hipStream_t s = c.s;
    const auto &L = layers();
    auto P = [&](const std::string &name) -> float * { return params + c.pl.off[name_index(name)]; };
    float *fblob = c.blobs;
    for (size_t i = 0; i < L.size(); ++i) {   // raw weights and biases, both roles
        const ULayer &l = L[i];
        const float *wt = P(l.key + ".weight"), *b = P(l.key + ".bias");
        float *dst = fblob + c.bl.off[i], *bdst = c.blobs + c.gb.boff[i];
        if (l.kind == ND_CONV1) {   // [3][cin] weights, 3 biases, zero up to a multiple of 4
            const size_t n = (size_t)3 * l.cin + 3, padded = (n + 3) / 4 * 4;
            ND_HIP(hipMemcpyAsync(dst, wt, sizeof(float) * 3 * l.cin, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemcpyAsync(dst + 3 * l.cin, b, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemsetAsync(dst + n, 0, sizeof(float) * (padded - n), s));
            continue;
        }
        ND_TRY(nd_pack_layer_device(l.kind, l.cin, l.cout, ND_F32, wt, b, dst, s));
        if (l.bn.empty())
            ND_TRY(nd_pack_layer_device(ND_CONV2S2, l.cout, l.cin, ND_F32, wt, nullptr, bdst, s));
        else if (i > 0)
            ND_TRY(nd_pack_layer_device(ND_CONVT3, l.cout, l.cin, ND_F32, wt, nullptr, bdst, s));
    }
    const UPlan &pl = c.t.g.fwd;
    const bool nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
    ND_TRY(nd_launch_nchw_to_qp(x, 3, pl.buf[XIN], 0, s));
    for (int si = 0; si < kNumSteps; ++si) {
        const UStep &st = kSteps[si];
        if (st.layer < 0 || L[st.layer].bn.empty()) {
            ND_TRY(run_step(st, pl, fblob, c.bl, nullptr, nosplit, s));
            continue;
        }
        const ULayer &l = L[st.layer];
        const QpBuf &zq = c.t.z[si], &aq = pl.buf[st.dst];
        const int H = zq.Hb, W = zq.Wb, planes = l.cout / 4;
        ConvDesc d = step_desc(st, pl, fblob, c.bl, nullptr, nosplit);
        d.act = ND_ACT_NONE;
        d.out = zq;
        d.out_plane0 = 0;
        ND_TRY(nd_launch_conv(d, s));
        int nchunk, per;
        ND_TRY(bn_chunks(planes, batch, H * W, &nchunk, &per));
        hipLaunchKernelGGL(k_bn_stats1, dim3(planes, batch, nchunk), dim3(256), 0, s, (const f32x4 *)zq.base, zq.np(), H * W, per,
                           (f64x4 *)c.t.g.red);
        hipLaunchKernelGGL(k_bn_stats2, dim3(planes), dim3(256), 0, s, (const f64x4 *)c.t.g.red, batch * nchunk,
                           (double)batch * H * W, l.cout, momentum, c.t.stat[si], P(l.bn + ".running_mean"), P(l.bn + ".running_var"));
        hipLaunchKernelGGL(k_bn_apply, dim3(blocks_of((long)H * W), batch, planes), dim3(256), 0, s, (const f32x4 *)zq.base, zq.np(),
                           view_of(aq, st.dst_plane0), H, W, stat_of(c.t.stat[si], l.cout), (const float *)P(l.bn + ".weight"),
                           (const float *)P(l.bn + ".bias"));
        ND_HIP(hipGetLastError());
    }
    const float *fw = fblob + c.bl.off[L.size() - 1];
    ND_TRY(nd_launch_final1x1(pl.buf[U4B], 64, fw, fw + 3 * 64, 0, c.t.g.sig, h, w, s, 1));
    const long n = (long)batch * 3 * h * w;
    hipLaunchKernelGGL(k_unet_head, dim3(blocks_of(n)), dim3(256), 0, s, (const float *)c.t.g.sig, x, n, (flags & ND_FLAG_FIND_NOISE) ? 1 : 0, y);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_unet_train_backward(int flags, const float *params, float *grads, void *blobs, const float *gy, float *dx, int batch,
                                      int h, int w, void *ws, size_t ws_bytes, void *stream) {
    if (!gy) ND_FAIL(ND_EINVAL, "nd_unet_train_backward: null pointer");
    if (!grads && !dx) ND_FAIL(ND_EINVAL, "nd_unet_train_backward: neither parameter gradients nor the input gradient requested");
    TrainCtx c;
    ND_TRY(train_ctx(c, flags, params, blobs, batch, h, w, ws, ws_bytes, stream));
    hipStream_t s = c.s;
    GradPlan &t = c.t.g;
    const int B = batch;
    const auto &L = layers();
    const bool noise = (flags & ND_FLAG_FIND_NOISE) != 0;
    auto P = [&](const std::string &name) -> const float * { return params + c.pl.off[name_index(name)]; };
    auto G = [&](const std::string &name) -> float * { return grads + c.pl.off[name_index(name)]; };
    const float *fw = c.blobs + c.bl.off[L.size() - 1];
    // Sigmoid + final 1x1
    const long n = (long)B * 3 * h * w;
    hipLaunchKernelGGL(k_unet_head_bwd, dim3(blocks_of(n)), dim3(256), 0, s, gy, (const float *)t.sig, n, noise ? 1 : 0, t.gt);
    ND_HIP(hipGetLastError());
    if (grads) ND_TRY(nd_launch_final_wgrad(t.gt, h, w, t.fwd.buf[U4B], 64, 0, t.red, G("outc.conv.weight"), G("outc.conv.bias"), s));
    ND_TRY(nd_launch_final_bwd_data(t.gt, h, w, fw, 64, 1, t.g[U4B], s));
    for (int si = kNumSteps - 1; si >= 0; --si) {
        const UStep &st = kSteps[si];
        if (st.layer < 0) {   // pool of the skip half: route g(pooled) back and ADD it (fixed order, as in the eval-mode backward)
            ND_TRY(nd_launch_maxpool_bwd_add(t.g[st.dst], t.fwd.buf[st.src], 0, t.g[st.src], 0, st.dst_plane0, s));
            continue;
        }
        const ULayer &l = L[st.layer];
        const QpBuf &in = t.fwd.buf[st.src];   // layer input (forward values)
        const QpBuf &go = t.g[st.dst];         // gradient of the layer's output buffer
        const int oplane0 = st.dst_plane0, oplanes = l.cout / 4;
        const int ih = in.Hb - 2 * in.pad, iw = in.Wb - 2 * in.pad;
        float *dw = grads ? G(l.key + ".weight") : nullptr, *db = grads ? G(l.key + ".bias") : nullptr;
        ConvDesc d;
        d.cin = l.cout;
        d.cout = l.cin;
        d.wpk = c.blobs + c.gb.boff[st.layer];
        d.out = t.g[st.src];
        d.part = t.fwd.split;
        d.part_bytes = kSplitScratchBytes;
        d.nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
        if (l.kind == ND_CONVT2S2) {
            // adjoint of the F.pad fix-up: only rows / columns [0, 2 h_in) x [0, 2 w_in) of the up half came from this layer
            const QpBuf &gu = t.gup[up_index(st.layer)];
            ND_TRY(nd_launch_repitch(go, oplane0, oplanes, 1, 0, 0, gu, 0, 0, 2 * ih, 2 * iw, s));
            if (grads) {
                ND_TRY(nd_launch_channel_sum(gu, 0, l.cout, db, t.red, s));
                for (int ab = 0; ab < 4; ++ab) {   // four 1-tap problems on the input grid
                    QpBuf bq = scratch_view(t, oplanes, B, ih, iw);
                    ND_TRY(nd_launch_repitch(gu, 0, oplanes, 2, ab >> 1, ab & 1, bq, 0, 0, ih, iw, s));
                    ND_TRY(nd_launch_wgrad(in, 0, l.cin, bq, 0, l.cout, 1, 4, ab, t.partial, t.partial_floats, dw, s));
                }
            }
            d.kind = ND_CONV2S2;
            d.bias = d.wpk + nd_bias_offset(ND_CONV2S2, l.cout, l.cin);
            d.in = gu;
            ND_TRY(nd_launch_conv(d, s));
            continue;
        }
        // BatchNorm + ReLU backward: g_a -> g_z in place
        {
            const QpBuf &a = t.fwd.buf[st.dst], &zq = c.t.z[si];
            const int oh = zq.Hb, ow = zq.Wb;
            const BnStat bs = stat_of(c.t.stat[si], l.cout);
            const QView gv = view_of(go, oplane0), av = view_of(a, oplane0);
            int nchunk, per;
            ND_TRY(bn_chunks(oplanes, B, oh * ow, &nchunk, &per));
            hipLaunchKernelGGL(k_bn_bwd_red1, dim3(oplanes, B, nchunk), dim3(256), 0, s, gv, av, (const f32x4 *)zq.base, zq.np(), oh, ow, per,
                               bs, (f64x4 *)t.red);
            hipLaunchKernelGGL(k_bn_bwd_red2, dim3(oplanes), dim3(256), 0, s, (const f64x4 *)t.red, B * nchunk, (double)B * oh * ow, l.cout,
                               c.t.coef, grads ? G(l.bn + ".weight") : (float *)nullptr, grads ? G(l.bn + ".bias") : (float *)nullptr);
            hipLaunchKernelGGL(k_bn_bwd_apply, dim3(blocks_of((long)oh * ow), B, oplanes), dim3(256), 0, s, gv, av, (const f32x4 *)zq.base,
                               zq.np(), oh, ow, bs, P(l.bn + ".weight"), (const float *)c.t.coef, l.cout);
            ND_HIP(hipGetLastError());
            if (grads) {
                // the conv's bias feeds a BatchNorm, which removes the channel mean: its gradient is 0 exactly (sum g_z = 0)
                ND_HIP(hipMemsetAsync(db, 0, sizeof(float) * l.cout, s));
                QpBuf a2 = scratch_view(t, oplanes, B, in.Hb, in.Wb);
                ND_TRY(nd_launch_repitch(go, oplane0, oplanes, 1, 0, 0, a2, 0, 0, oh, ow, s));
                ND_TRY(nd_launch_wgrad(a2, 0, l.cout, in, 0, l.cin, 9, 9, 0, t.partial, t.partial_floats, dw, s));
            }
        }
        if (st.layer > 0) {   // data gradient: the transposed role on the gradient buffer's 1-pixel zero border
            d.kind = ND_CONVT3;
            d.bias = d.wpk + nd_bias_offset(ND_CONVT3, l.cout, l.cin);
            d.in = go;
            d.in_plane0 = oplane0;
            ND_TRY(nd_launch_conv(d, s));
        } else if (dx) {
            dim3 grid((unsigned)((w + 15) / 16), (unsigned)((h + 3) / 4), B);
            hipLaunchKernelGGL(k_unet_input_grad, grid, dim3(64 * kUigGroups), 0, s, (const f32x4 *)go.base, go.np(), go.Hb, go.Wb, oplanes,
                               P(L[0].key + ".weight"), h, w, noise ? gy : (const float *)nullptr, dx);
            ND_HIP(hipGetLastError());
        }
    }
    return ND_OK;
}
