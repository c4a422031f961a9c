// UNet under autograd, for both BatchNorm modes: eval (running statistics, folded into the convolutions) and train (the statistics of
// the batch, unet_bn.hip).  This file owns the plan, the layouts, the pack loop, the forward and the ONE backward walk; the mode is a
// bool that decides how the weights are packed, what a Conv3 + BatchNorm + ReLU layer launches in the forward, and -- at one branch of
// the walk -- how g_a becomes g_z, db and dw.
//   forward   eval: fold BatchNorm and pack on the device, in the forward role and in the transposed role; train: pack the raw weights.
//             Then the inference launch sequence on whole tiles (every layer's output stays in its own buffer of the plan; train mode
//             runs a BatchNorm layer's convolution into a kept pre-norm buffer z, then statistics and apply), final 1x1 + Sigmoid
//   backward  data gradients = the SAME conv kernel on the transposed-role blob (a padding-1 Conv2d(3): the transposed role on a
//             gradient buffer with a 1-pixel zero border; ConvTranspose2d(2, s=2): Conv 2x2 s2), weight gradients = k_wgrad (wgrad.hip),
//             pool backward = k_maxpool_bwd_add, exactly as utnet_train.hip does
// Small HBM-bound kernels below: the folded weights, ReLU backward from the kept post-activation, the Sigmoid head and its adjoint,
// the first layer's data gradient to the 3 input channels, the adjoint of the BatchNorm fold.  No atomics, fixed summation order.
// Parameters and gradients: ONE flat fp32 buffer in nd_unet_tensor_name order, buffers (running statistics) included so that the
// fold reads one array; their gradient slots are never written.
#include <algorithm>

#include "unet_net.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------ kernels
// wf[co][k] = w[co][k] * scale[co]: the folded weights in the torch layout, one rounding per value (what the pack kernel's `scale`
// writes into the forward blob); both roles are packed from it, and the first layer's data gradient reads it as it is
__global__ void k_unet_fold_w(const float *__restrict__ w, const float *__restrict__ scale, int per_co, long n, float *__restrict__ wf) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) wf[i] = w[i] * scale[i / per_co];
}

// g (interior of a bordered gradient buffer, planes from the pointer) *= (a > 0), a = the layer's kept output (torch: ReLU'(0) = 0)
__global__ __launch_bounds__(256) void k_relu_bwd_post(f32x4 *__restrict__ g, long gnp, int gHb, int gWb, int gpad,
                                                       const f32x4 *__restrict__ a, long anp, int aHb, int aWb, int apad, int H, int W,
                                                       int B) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int b = blockIdx.z % B, q = blockIdx.z / B;
    if (x >= W) return;
    f32x4 *gp = g + (long)q * gnp + ((long)b * gHb + y + gpad) * gWb + x + gpad;
    const f32x4 av = a[(long)q * anp + ((long)b * aHb + y + apad) * aWb + x + apad];
    f32x4 gv = *gp;
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = av[e] > 0.f ? gv[e] : 0.f;
    *gp = gv;
}

// Adjoint of the BatchNorm fold  W' = W s,  b' = (b - mean) s + beta,  s = gamma / sqrt(var + 1e-5).  One workgroup per output
// channel; dw / db hold dW' / db' on entry and dW / db on return:
//     dW = dW' s     db = db' s     dbeta = db'     dgamma = (sum dW' W + db' (b - mean)) / sqrt(var + eps)
// (dgamma from dW', not from dW / s: right for gamma = 0 and gamma < 0).  The sum runs in double: it is a sum over pixels in disguise
// (sum g * conv output) and cancels as one.
__global__ __launch_bounds__(256) void k_bn_fold_bwd(int per_co, const float *__restrict__ w, const float *__restrict__ b,
                                                     const float *__restrict__ gamma, const float *__restrict__ mean,
                                                     const float *__restrict__ var, float *__restrict__ dw, float *__restrict__ db,
                                                     float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double red[256];
    const int co = blockIdx.x;
    const float inv = 1.f / sqrtf(var[co] + 1e-5f), sc = gamma[co] * inv;
    const float *wc = w + (long)co * per_co;
    float *dwc = dw + (long)co * per_co;
    double acc = 0.0;
    for (int k = threadIdx.x; k < per_co; k += 256) {
        const float d = dwc[k];
        acc += (double)d * (double)wc[k];
        dwc[k] = d * sc;
    }
    acc = nd_block_sum(acc, red);
    if (threadIdx.x != 0) return;
    const float dbp = db[co];
    dgamma[co] = (float)((acc + (double)dbp * ((double)b[co] - (double)mean[co])) * (double)inv);
    dbeta[co] = dbp;
    db[co] = dbp * sc;
}

namespace {

// y = s, or x - s with find_noise (ThirdPartyNets.py:168-169); s = the Sigmoid output, kept for the backward
__global__ void k_unet_head(const float *__restrict__ sig, const float *__restrict__ x, long n, int noise, float *__restrict__ y) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = noise ? x[i] - sig[i] : sig[i];
}
// gt = d loss / d (input of the Sigmoid) = +-gy * s * (1 - s)   (-: find_noise, whose dx also takes gy itself: k_unet_input_grad)
__global__ void k_unet_head_bwd(const float *__restrict__ gy, const float *__restrict__ sig, long n, int noise, float *__restrict__ gt) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float s = sig[i], v = gy[i] * (s * (1.f - s));
    gt[i] = noise ? -v : v;
}

// d loss / d input image: the data gradient of the first Conv2d(3, 64, 3, padding=1) to its 3 input channels.
// g1 = d loss / d (conv output): planes of an H x W grid inside a zero border of 1; wf = the weight the forward convolved with,
// [cout][3][3][3] (eval mode: folded; train mode: raw):
//     dx[c][y][x] = sum_co sum_ky,kx g1[co][y + 1 - ky][x + 1 - kx] * wf[co][c][ky][kx]        (g1 zero outside its grid: the border)
//                   (+ gy[c][y][x] with find_noise: the output is x - sigmoid)
// A workgroup = one 16 x 4 pixel patch of one image x 4 plane groups (wave w takes planes w, w + 4, ...); the groups' partial sums
// meet in LDS in a fixed order.  Weight indices are wave-uniform (scalar loads).  Every output written once.
constexpr int kUigGroups = 4;
__global__ __launch_bounds__(64 * kUigGroups) void k_unet_input_grad(const f32x4 *__restrict__ g1, long gnp, int gHb, int gWb, int planes,
                                                                     const float *__restrict__ wf, int H, int W,
                                                                     const float *__restrict__ gy_add, float *__restrict__ dx) {
    __shared__ float part[kUigGroups][3][64];
    const int lane = threadIdx.x & 63, grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.z;
    const bool live = (int)blockIdx.x * 16 + (lane & 15) < W && (int)blockIdx.y * 4 + (lane >> 4) < H;
    const int x = live ? blockIdx.x * 16 + (lane & 15) : 0, y = live ? blockIdx.y * 4 + (lane >> 4) : 0;
    // bordered position of g1[y + 1 - ky][x + 1 - kx]: (y + 2 - ky, x + 2 - kx), inside [0, H + 2) x [0, W + 2)
    const f32x4 *gb = g1 + ((long)b * gHb + y + 2) * gWb + x + 2;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int q = grp; q < planes; q += kUigGroups) {
        const f32x4 *gq = gb + (long)q * gnp;
        const float *wq = wf + (long)q * 4 * 27;   // co = 4q .. 4q+3: 108 contiguous floats [e][c][ky][kx]
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t - 3 * ky;
            const f32x4 s = gq[-(long)ky * gWb - kx];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                a0 = fmaf(s[e], wq[e * 27 + t], a0);
                a1 = fmaf(s[e], wq[e * 27 + 9 + t], a1);
                a2 = fmaf(s[e], wq[e * 27 + 18 + t], a2);
            }
        }
    }
    part[grp][0][lane] = a0;
    part[grp][1][lane] = a1;
    part[grp][2][lane] = a2;
    __syncthreads();
    if (grp >= 3 || !live) return;
    const int c = grp;   // waves 0, 1, 2 write channels 0, 1, 2
    float v = part[0][c][lane];
#pragma unroll
    for (int k = 1; k < kUigGroups; ++k) v += part[k][c][lane];
    const long o = (((long)b * 3 + c) * H + y) * W + x;
    dx[o] = gy_add ? v + gy_add[o] : v;
}

// ------------------------------------------------------------------ layouts and the plan
inline int taps_of(int kind) { return kind == ND_CONV3 ? 9 : (kind == ND_CONVT2S2 ? 4 : 1); }

// flat parameter layout = nd_unet_tensor_name order (parameters and buffers)
struct UParams {
    std::vector<size_t> off, cnt;
    size_t total;
};
UParams param_layout() {
    UParams pl;
    size_t o = 0;
    auto add = [&](size_t n) {
        pl.off.push_back(o);
        pl.cnt.push_back(n);
        o += n;
    };
    for (const ULayer &l : layers()) {
        add((size_t)l.cin * l.cout * taps_of(l.kind));
        add((size_t)l.cout);
        if (!l.bn.empty())
            for (int k = 0; k < 4; ++k) add((size_t)l.cout);
    }
    pl.total = o;
    return pl;
}

// blobs: forward-role blob (the inference layout, bit for bit) | transposed-role packings (none for layer 0 and the final 1x1) |
// folded weights of the layer being packed | folded weights of layer 0 (kept: the input gradient reads them) | scale + folded bias
// (train mode packs the raw weights into the first two sections and uses nothing behind them)
struct GradBlob {
    std::vector<size_t> boff;
    size_t fwd_total, bwd, wfold, w0fold, stage, total;
};
constexpr size_t kStageFloats = 2 * 512;
GradBlob grad_blob_layout() {
    GradBlob g;
    const auto &L = layers();
    g.fwd_total = blob_layout().total;
    size_t o = g.fwd_total, wmax = 0;
    g.bwd = o;
    for (size_t i = 0; i < L.size(); ++i) {
        g.boff.push_back(o);
        const ULayer &l = L[i];
        if (i == 0 || l.kind == ND_CONV1) continue;
        o += nd_packed_floats(l.kind == ND_CONV3 ? ND_CONVT3 : ND_CONV2S2, l.cout, l.cin);
        if (!l.bn.empty()) wmax = std::max(wmax, (size_t)l.cin * l.cout * 9);
    }
    g.wfold = o;
    o += wmax;
    g.w0fold = o;
    o += (size_t)L[0].cin * L[0].cout * 9;
    o = (o + 3) & ~(size_t)3;
    g.stage = o;
    o += kStageFloats;
    g.total = o;
    return g;
}

// which up<n> (0..3) a 2x2 stride-2 layer is
int up_index(int layer) {
    int n = 0;
    for (int i = 0; i < layer; ++i)
        if (layers()[i].kind == ND_CONVT2S2) ++n;
    return n;
}

// train mode only: what BatchNorm on the statistics of the batch keeps per step.  Eval mode leaves it empty
constexpr int kCoefFloats = 2 * 512;
struct BnBatch {
    QpBuf z[kNumSteps];      // pre-norm output of step i (BatchNorm layers only): cout / 4 planes on the level's grid, no border
    float *stat[kNumSteps];  // [mu_hi | mu_lo | inv] of step i
    float *coef;             // dbeta / N, dgamma / N of the layer in flight
};

struct GradPlan {
    UPlan fwd;
    QpBuf g[NUB];     // gradient of every activation buffer, border 1 (g[XIN]: none)
    QpBuf gup[4];     // gradient of up<n>.up's own result: 2 h_in x 2 w_in, no border (the F.pad fix-up lines dropped)
    QpBuf scratch;    // re-pitched wgrad operand (largest over the layers)
    float *partial;   // wgrad K-slice partial sums
    size_t partial_floats;
    float *red;       // reduction scratch
    float *sig, *gt;  // Sigmoid output and the gradient at its input, [B,3,H,W]
    BnBatch bn;       // behind everything else, so the eval-mode layout is a prefix of the train-mode one
    size_t bytes;
};
constexpr int kRedFloats = 1 << 19;   // >= 5 * 3 * 16 * B and 4 * 128 * B floats: B <= 256 (checked)

// a quad-planar fp32 buffer at base + off (base null: sizes only); off moves past it
void place(QpBuf &q, int planes, int B, int Hb, int Wb, int pad, char *base, size_t &off) {
    q.planes = planes;
    q.B = B;
    q.Hb = Hb;
    q.Wb = Wb;
    q.pad = pad;
    q.dt = ND_F32;
    q.pstride = (long)B * Hb * Wb;
    q.base = (float *)(base ? base + off : nullptr);
    off += ((size_t)planes * q.pstride + nd_buf_slack(Wb)) * 16;
    off = (off + 255) & ~(size_t)255;
}

GradPlan make_grad_plan(int h, int w, int B, char *base) {
    GradPlan t;
    t.bn = BnBatch();
    t.fwd = make_plan(h, w, B, base);
    size_t off = t.fwd.bytes;
    auto alloc = [&](QpBuf &q, int planes, int Hb, int Wb, int pad) { place(q, planes, B, Hb, Wb, pad, base, off); };
    t.g[XIN] = QpBuf();
    for (int id = 1; id < NUB; ++id) {
        const QpBuf &o = t.fwd.buf[id];
        alloc(t.g[id], o.planes, o.Hb - 2 * o.pad + 2, o.Wb - 2 * o.pad + 2, 1);
    }
    const auto &L = layers();
    size_t scratch_elems = 0, pf = 0;
    for (const UStep &st : kSteps) {
        if (st.layer < 0) continue;
        const ULayer &l = L[st.layer];
        const QpBuf &in = t.fwd.buf[st.src];
        size_t e, p;
        if (l.kind == ND_CONV3) {   // A = g(out) on the input's bordered grid
            e = (size_t)(l.cout / 4) * B * in.Hb * in.Wb;
            p = nd_wgrad_partial_floats(9, l.cout, l.cin, (long)B * in.Hb * in.Wb, nullptr, nullptr);
        } else {                    // up: B = one phase of g(out) on the input grid (border 0)
            alloc(t.gup[up_index(st.layer)], l.cout / 4, 2 * in.Hb, 2 * in.Wb, 0);
            e = (size_t)(l.cout / 4) * B * in.Hb * in.Wb;
            p = nd_wgrad_partial_floats(1, l.cin, l.cout, (long)B * in.Hb * in.Wb, nullptr, nullptr);
        }
        scratch_elems = std::max(scratch_elems, e);
        pf = std::max(pf, p);
    }
    t.scratch = QpBuf();
    t.scratch.base = (float *)(base ? base + off : nullptr);
    off += (scratch_elems + 4096) * 16;
    off = (off + 255) & ~(size_t)255;
    t.partial = (float *)(base ? base + off : nullptr);
    t.partial_floats = pf;
    off += pf * 4;
    off = (off + 255) & ~(size_t)255;
    t.red = (float *)(base ? base + off : nullptr);
    off += (size_t)kRedFloats * 4;
    const size_t img = ((size_t)B * 3 * h * w * 4 + 255) & ~(size_t)255;
    t.sig = (float *)(base ? base + off : nullptr);
    off += img;
    t.gt = (float *)(base ? base + off : nullptr);
    off += img;
    t.bytes = off;
    return t;
}

QpBuf scratch_view(const GradPlan &t, int planes, int B, int H, int W) {
    QpBuf q = t.scratch;
    q.planes = planes;
    q.B = B;
    q.Hb = H;
    q.Wb = W;
    q.pad = 0;
    q.dt = ND_F32;
    q.pstride = (long)B * H * W;
    return q;
}

int check_grad(int h, int w, int batch) {
    ND_TRY(check(h, w, batch, ND_F32));
    // (the elementwise kernels put batch x planes, up to 128 of them, into gridDim.z <= 65535)
    if (batch > 256) ND_FAIL(ND_EINVAL, "UNet under autograd: batch %d (at most 256 per call)", batch);
    return ND_OK;
}

inline unsigned blocks_of(long n) { return (unsigned)((n + 255) / 256); }

// train mode: the grad plan followed by the batch-statistics extension
GradPlan make_train_plan(int h, int w, int B, char *base) {
    GradPlan t = make_grad_plan(h, w, B, base);
    size_t off = t.bytes;
    const auto &L = layers();
    for (int i = 0; i < kNumSteps; ++i) {
        const UStep &st = kSteps[i];
        if (st.layer < 0 || L[st.layer].bn.empty()) continue;
        const QpBuf &o = t.fwd.buf[st.dst];
        place(t.bn.z[i], L[st.layer].cout / 4, B, o.Hb - 2 * o.pad, o.Wb - 2 * o.pad, 0, base, off);
    }
    for (int i = 0; i < kNumSteps; ++i) {
        if (!t.bn.z[i].planes) continue;
        t.bn.stat[i] = (float *)(base ? base + off : nullptr);
        off += (size_t)3 * 4 * t.bn.z[i].planes * 4;
        off = (off + 255) & ~(size_t)255;
    }
    t.bn.coef = (float *)(base ? base + off : nullptr);
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

// ------------------------------------------------------------------ the mode: what differs by name between the two ABI families
int check_mode(bool train, int h, int w, int batch) { return train ? check_train(h, w, batch) : check_grad(h, w, batch); }
GradPlan make_mode_plan(bool train, int h, int w, int B, char *base) {
    return train ? make_train_plan(h, w, B, base) : make_grad_plan(h, w, B, base);
}
const char *mode_name(bool train) { return train ? "UNet training" : "UNet under autograd"; }
const char *mode_ws_name(bool train) { return train ? "UNet training workspace" : "UNet gradient workspace"; }

size_t workspace_bytes(bool train, int h, int w, int batch) {
    if (check_mode(train, h, w, batch) != ND_OK) return 0;
    return make_mode_plan(train, h, w, batch, nullptr).bytes;
}
int workspace_init(bool train, void *ws, size_t ws_bytes, int h, int w, int batch, void *stream) {
    ND_TRY(check_mode(train, h, w, batch));
    const size_t need = make_mode_plan(train, h, w, batch, nullptr).bytes;
    if (!ws || ws_bytes < need) ND_FAIL(ND_ENOMEM, "%s: %zu B given, %zu B needed", mode_ws_name(train), ws_bytes, need);
    ND_HIP(hipMemsetAsync(ws, 0, need, (hipStream_t)stream));   // zero borders of activations AND gradients, fix-up lines, slack
    return ND_OK;
}

struct GradCtx {
    bool train;
    int B, H, W, flags;
    GradPlan t;
    UParams pl;
    Blob bl;
    GradBlob gb;
    const float *params;
    float *grads;   // null: no parameter gradient is wanted (or a forward)
    float *blobs;
    hipStream_t s;
    size_t off(const std::string &name) const { return pl.off[name_index(name)]; }
    const float *P(const std::string &name) const { return params + off(name); }
    float *G(const std::string &name) const { return grads + off(name); }
};
int grad_ctx(GradCtx &c, bool train, int flags, const float *params, float *grads, void *blobs, int batch, int h, int w, void *ws,
             size_t ws_bytes, void *stream) {
    ND_TRY(nd_check_flags(flags, false, true));
    ND_TRY(check_mode(train, h, w, batch));
    if (!params || !blobs || !ws) ND_FAIL(ND_EINVAL, "%s: null pointer", mode_name(train));
    c.train = train;
    c.B = batch;
    c.H = h;
    c.W = w;
    c.flags = flags;
    c.t = make_mode_plan(train, h, w, batch, (char *)ws);
    if (ws_bytes < c.t.bytes) ND_FAIL(ND_ENOMEM, "%s: %zu B given, %zu B needed", mode_ws_name(train), ws_bytes, c.t.bytes);
    c.pl = param_layout();
    c.bl = blob_layout();
    c.gb = grad_blob_layout();
    c.params = params;
    c.grads = grads;
    c.blobs = (float *)blobs;
    c.s = (hipStream_t)stream;
    return ND_OK;
}

// ------------------------------------------------------------------ forward
// every layer into the blobs: the forward role, and (but for layer 0 and the final 1x1) the transposed role the data gradient runs
// on.  Eval mode folds BatchNorm through the staging area first; train mode packs the raw weights
int pack_weights(const GradCtx &c, const char *who) {
    hipStream_t s = c.s;
    const auto &L = layers();
    float *wfold = c.blobs + c.gb.wfold, *scale = c.blobs + c.gb.stage, *fbias = scale + kStageFloats / 2;
    for (size_t i = 0; i < L.size(); ++i) {
        const ULayer &l = L[i];
        const float *wt = c.P(l.key + ".weight"), *b = c.P(l.key + ".bias");
        float *dst = c.blobs + c.bl.off[i], *bdst = c.blobs + c.gb.boff[i];
        if (l.kind == ND_CONV1) {   // [3][cin] weights, 3 biases, zero up to a multiple of 4
            const size_t n = (size_t)3 * l.cin + 3, padded = (n + 3) / 4 * 4;
            ND_HIP(hipMemcpyAsync(dst, wt, sizeof(float) * 3 * l.cin, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemcpyAsync(dst + 3 * l.cin, b, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemsetAsync(dst + n, 0, sizeof(float) * (padded - n), s));
            continue;
        }
        if (!c.train && !l.bn.empty()) {   // wt, b <- the folded weights and bias (layer 0's are kept: the input gradient reads them)
            if ((size_t)l.cout > kStageFloats / 2) ND_FAIL(ND_EINVAL, "%s: no staging room for %s", who, l.key.c_str());
            ND_TRY(nd_launch_bn_fold(l.cout, b, c.P(l.bn + ".weight"), c.P(l.bn + ".bias"), c.P(l.bn + ".running_mean"),
                                     c.P(l.bn + ".running_var"), scale, fbias, s));
            const long n = (long)l.cin * l.cout * 9;
            float *wf = i == 0 ? c.blobs + c.gb.w0fold : wfold;
            hipLaunchKernelGGL(k_unet_fold_w, dim3(blocks_of(n)), dim3(256), 0, s, wt, (const float *)scale, l.cin * 9, n, wf);
            ND_HIP(hipGetLastError());
            wt = wf;
            b = fbias;
        }
        ND_TRY(nd_pack_layer_device(l.kind, l.cin, l.cout, ND_F32, wt, b, dst, s));
        // transposed role: cin' = cout, cout' = cin, no bias
        if (l.bn.empty())
            ND_TRY(nd_pack_layer_device(ND_CONV2S2, l.cout, l.cin, ND_F32, wt, nullptr, bdst, s));
        else if (i > 0)
            ND_TRY(nd_pack_layer_device(ND_CONVT3, l.cout, l.cin, ND_F32, wt, nullptr, bdst, s));
    }
    return ND_OK;
}

// running: the flat buffer again, writable (train mode moves the running statistics in it; eval mode: null)
int unet_forward(const GradCtx &c, float *running, float momentum, const float *x, float *y, const char *who) {
    hipStream_t s = c.s;
    const auto &L = layers();
    ND_TRY(pack_weights(c, who));
    const UPlan &pl = c.t.fwd;
    const bool nosplit = (c.flags & ND_FLAG_NO_SPLITK) != 0;
    ND_TRY(nd_launch_nchw_to_qp(x, 3, pl.buf[XIN], 0, s));
    for (int si = 0; si < kNumSteps; ++si) {
        const UStep &st = kSteps[si];
        if (!c.train || st.layer < 0 || L[st.layer].bn.empty()) {
            ND_TRY(run_step(st, pl, c.blobs, c.bl, nullptr, nosplit ? ND_FLAG_NO_SPLITK : 0, s));   // (every layer direct: no Winograd form here)
            continue;
        }
        // train mode, Conv3 + BatchNorm + ReLU: the convolution without activation into z, then stats1, stats2, apply
        const ULayer &l = L[st.layer];
        ConvDesc d = step_desc(st, pl, c.blobs, c.bl, nullptr, nosplit);
        d.act = ND_ACT_NONE;
        d.out = c.t.bn.z[si];
        d.out_plane0 = 0;
        ND_TRY(nd_launch_conv(d, s));
        ND_TRY(nd_launch_bn_train_fwd(c.t.bn.z[si], pl.buf[st.dst], st.dst_plane0, l.cout, momentum, c.P(l.bn + ".weight"),
                                      c.P(l.bn + ".bias"), running + c.off(l.bn + ".running_mean"),
                                      running + c.off(l.bn + ".running_var"), c.t.bn.stat[si], c.t.red, kRedFloats, s));
    }
    const float *fw = c.blobs + c.bl.off[L.size() - 1];
    ND_TRY(nd_launch_final1x1(pl.buf[U4B], 64, fw, fw + 3 * 64, 0, c.t.sig, c.H, c.W, s, 1));
    const long n = (long)c.B * 3 * c.H * c.W;
    hipLaunchKernelGGL(k_unet_head, dim3(blocks_of(n)), dim3(256), 0, s, (const float *)c.t.sig, x, n, (c.flags & ND_FLAG_FIND_NOISE) ? 1 : 0, y);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ backward
// dW of a Conv3 layer from g_z (in the gradient buffer of the step's output) and the layer's input
int conv3_wgrad(const GradCtx &c, const UStep &st, float *dw) {
    const GradPlan &t = c.t;
    const ULayer &l = layers()[st.layer];
    const QpBuf &in = t.fwd.buf[st.src], &go = t.g[st.dst];
    QpBuf a2 = scratch_view(t, l.cout / 4, c.B, in.Hb, in.Wb);
    ND_TRY(nd_launch_repitch(go, st.dst_plane0, l.cout / 4, 1, 0, 0, a2, 0, 0, go.Hb - 2, go.Wb - 2, c.s));
    return nd_launch_wgrad(a2, 0, l.cout, in, 0, l.cin, 9, 9, 0, t.partial, t.partial_floats, dw, c.s);
}

// g_a -> g_z, db, dw of a Conv3 + BatchNorm + ReLU layer, one function per mode.
// Eval: ReLU backward in place from the kept output; then db', dW' of the folded layer and the adjoint of the fold in place
int bn_layer_bwd_eval(const GradCtx &c, const UStep &st) {
    const ULayer &l = layers()[st.layer];
    const QpBuf &go = c.t.g[st.dst], &a = c.t.fwd.buf[st.dst];
    const int oplane0 = st.dst_plane0, oplanes = l.cout / 4, oh = go.Hb - 2, ow = go.Wb - 2;
    hipLaunchKernelGGL(k_relu_bwd_post, dim3((ow + 255) / 256, oh, c.B * oplanes), dim3(256), 0, c.s,
                       (f32x4 *)go.base + (long)oplane0 * go.np(), go.np(), go.Hb, go.Wb, go.pad,
                       (const f32x4 *)a.base + (long)oplane0 * a.np(), a.np(), a.Hb, a.Wb, a.pad, oh, ow, c.B);
    ND_HIP(hipGetLastError());
    if (!c.grads) return ND_OK;
    float *dw = c.G(l.key + ".weight"), *db = c.G(l.key + ".bias");
    ND_TRY(nd_launch_channel_sum(go, oplane0, l.cout, db, c.t.red, c.s));
    ND_TRY(conv3_wgrad(c, st, dw));
    hipLaunchKernelGGL(k_bn_fold_bwd, dim3(l.cout), dim3(256), 0, c.s, l.cin * 9, c.P(l.key + ".weight"), c.P(l.key + ".bias"),
                       c.P(l.bn + ".weight"), c.P(l.bn + ".running_mean"), c.P(l.bn + ".running_var"), dw, db, c.G(l.bn + ".weight"),
                       c.G(l.bn + ".bias"));
    ND_HIP(hipGetLastError());
    return ND_OK;
}
// Train: BatchNorm + ReLU backward in place (red1, red2, bwd_apply; dgamma, dbeta on the way), then dW from g_z
int bn_layer_bwd_train(const GradCtx &c, int si) {
    const UStep &st = kSteps[si];
    const ULayer &l = layers()[st.layer];
    ND_TRY(nd_launch_bn_train_bwd(c.t.g[st.dst], c.t.fwd.buf[st.dst], st.dst_plane0, c.t.bn.z[si], l.cout, c.P(l.bn + ".weight"),
                                  c.t.bn.stat[si], c.t.bn.coef, c.grads ? c.G(l.bn + ".weight") : nullptr,
                                  c.grads ? c.G(l.bn + ".bias") : nullptr, c.t.red, kRedFloats, c.s));
    if (!c.grads) return ND_OK;
    // the conv's bias feeds a BatchNorm, which removes the channel mean: its gradient is 0 exactly (sum g_z = 0)
    ND_HIP(hipMemsetAsync(c.G(l.key + ".bias"), 0, sizeof(float) * l.cout, c.s));
    return conv3_wgrad(c, st, c.G(l.key + ".weight"));
}

int unet_backward(const GradCtx &c, const float *gy, float *dx) {
    hipStream_t s = c.s;
    const GradPlan &t = c.t;
    const int B = c.B, h = c.H, w = c.W;
    const auto &L = layers();
    const bool noise = (c.flags & ND_FLAG_FIND_NOISE) != 0;
    const float *fw = c.blobs + c.bl.off[L.size() - 1];
    // Sigmoid + final 1x1
    const long n = (long)B * 3 * h * w;
    hipLaunchKernelGGL(k_unet_head_bwd, dim3(blocks_of(n)), dim3(256), 0, s, gy, (const float *)t.sig, n, noise ? 1 : 0, t.gt);
    ND_HIP(hipGetLastError());
    if (c.grads)
        ND_TRY(nd_launch_final_wgrad(t.gt, h, w, t.fwd.buf[U4B], 64, 0, t.red, c.G("outc.conv.weight"), c.G("outc.conv.bias"), s));
    ND_TRY(nd_launch_final_bwd_data(t.gt, h, w, fw, 64, 1, t.g[U4B], s));
    for (int si = kNumSteps - 1; si >= 0; --si) {
        const UStep &st = kSteps[si];
        if (st.layer < 0) {
            // pool of the skip half (planes from 0) of a concat buffer: route g(pooled) back and ADD it to what the decoder's
            // first layer of this level wrote there (that launch came earlier in this loop: a fixed order)
            ND_TRY(nd_launch_maxpool_bwd_add(t.g[st.dst], t.fwd.buf[st.src], 0, t.g[st.src], 0, st.dst_plane0, s));
            continue;
        }
        const ULayer &l = L[st.layer];
        const QpBuf &in = t.fwd.buf[st.src];   // layer input (forward values)
        const QpBuf &go = t.g[st.dst];         // gradient of the layer's output buffer
        const int oplane0 = st.dst_plane0, oplanes = l.cout / 4;
        const int ih = in.Hb - 2 * in.pad, iw = in.Wb - 2 * in.pad;
        ConvDesc d;
        d.cin = l.cout;
        d.cout = l.cin;
        d.wpk = c.blobs + c.gb.boff[st.layer];
        d.out = t.g[st.src];
        d.part = t.fwd.split;
        d.part_bytes = kSplitScratchBytes;
        d.nosplit = (c.flags & ND_FLAG_NO_SPLITK) != 0;
        if (l.kind == ND_CONVT2S2) {
            // adjoint of the F.pad fix-up: only rows / columns [0, 2 h_in) x [0, 2 w_in) of the up half came from this layer
            const QpBuf &gu = t.gup[up_index(st.layer)];
            ND_TRY(nd_launch_repitch(go, oplane0, oplanes, 1, 0, 0, gu, 0, 0, 2 * ih, 2 * iw, s));
            if (c.grads) {
                ND_TRY(nd_launch_channel_sum(gu, 0, l.cout, c.G(l.key + ".bias"), t.red, s));
                for (int ab = 0; ab < 4; ++ab) {   // four 1-tap problems on the input grid
                    QpBuf bq = scratch_view(t, oplanes, B, ih, iw);
                    ND_TRY(nd_launch_repitch(gu, 0, oplanes, 2, ab >> 1, ab & 1, bq, 0, 0, ih, iw, s));
                    ND_TRY(nd_launch_wgrad(in, 0, l.cin, bq, 0, l.cout, 1, 4, ab, t.partial, t.partial_floats, c.G(l.key + ".weight"), s));
                }
            }
            d.kind = ND_CONV2S2;
            d.bias = d.wpk + nd_bias_offset(ND_CONV2S2, l.cout, l.cin);
            d.in = gu;
            ND_TRY(nd_launch_conv(d, s));
            continue;
        }
        // Conv3 + BatchNorm + ReLU: the one place the mode decides the launches
        if (c.train)
            ND_TRY(bn_layer_bwd_train(c, si));
        else
            ND_TRY(bn_layer_bwd_eval(c, st));
        if (st.layer > 0) {   // data gradient: the transposed role on the gradient buffer's 1-pixel zero border
            d.kind = ND_CONVT3;
            d.bias = d.wpk + nd_bias_offset(ND_CONVT3, l.cout, l.cin);
            d.in = go;
            d.in_plane0 = oplane0;
            ND_TRY(nd_launch_conv(d, s));
        } else if (dx) {   // the weights the forward convolved with: raw in train mode, folded in eval mode
            const float *w0 = c.train ? c.P(l.key + ".weight") : c.blobs + c.gb.w0fold;
            dim3 grid((unsigned)((w + 15) / 16), (unsigned)((h + 3) / 4), B);
            hipLaunchKernelGGL(k_unet_input_grad, grid, dim3(64 * kUigGroups), 0, s, (const f32x4 *)go.base, go.np(), go.Hb, go.Wb, oplanes,
                               w0, h, w, noise ? gy : (const float *)nullptr, dx);
            ND_HIP(hipGetLastError());
        }
    }
    return ND_OK;
}

// the two halves behind the four entry points; who: the entry point's name, for its own messages
int forward_entry(bool train, const char *who, int flags, const float *params, float *running, float momentum, void *blobs, const float *x,
                  float *y, int batch, int h, int w, void *ws, size_t ws_bytes, void *stream) {
    if (!x || !y) ND_FAIL(ND_EINVAL, "%s: null pointer", who);
    if (train && !(momentum >= 0.f && momentum <= 1.f)) ND_FAIL(ND_EINVAL, "%s: momentum %g outside [0, 1]", who, (double)momentum);
    GradCtx c;
    ND_TRY(grad_ctx(c, train, flags, params, nullptr, blobs, batch, h, w, ws, ws_bytes, stream));
    return unet_forward(c, running, momentum, x, y, who);
}
int backward_entry(bool train, const char *who, int flags, const float *params, float *grads, void *blobs, const float *gy, float *dx,
                   int batch, int h, int w, void *ws, size_t ws_bytes, void *stream) {
    if (!gy) ND_FAIL(ND_EINVAL, "%s: null pointer", who);
    if (!grads && !dx) ND_FAIL(ND_EINVAL, "%s: neither parameter gradients nor the input gradient requested", who);
    GradCtx c;
    ND_TRY(grad_ctx(c, train, flags, params, grads, blobs, batch, h, w, ws, ws_bytes, stream));
    return unet_backward(c, gy, dx);
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t nd_unet_param_count(void) { return param_layout().total; }
extern "C" int nd_unet_param_range(int tensor_idx, size_t *offset, size_t *count) {
    const UParams pl = param_layout();
    if (tensor_idx < 0 || tensor_idx >= (int)pl.off.size()) ND_FAIL(ND_EINVAL, "tensor index %d out of range", tensor_idx);
    if (offset) *offset = pl.off[tensor_idx];
    if (count) *count = pl.cnt[tensor_idx];
    return ND_OK;
}
// one blob layout for both modes (train mode uses its first two sections)
extern "C" size_t nd_unet_grad_blob_bytes(void) { return grad_blob_layout().total * sizeof(float); }
extern "C" size_t nd_unet_train_blob_bytes(void) { return grad_blob_layout().total * sizeof(float); }
extern "C" size_t nd_unet_grad_workspace_bytes(int h, int w, int batch) { return workspace_bytes(false, h, w, batch); }
extern "C" size_t nd_unet_train_workspace_bytes(int h, int w, int batch) { return workspace_bytes(true, h, w, batch); }
extern "C" int nd_unet_grad_workspace_init(void *ws, size_t ws_bytes, int h, int w, int batch, void *stream) {
    return workspace_init(false, ws, ws_bytes, h, w, batch, stream);
}
extern "C" int nd_unet_train_workspace_init(void *ws, size_t ws_bytes, int h, int w, int batch, void *stream) {
    return workspace_init(true, ws, ws_bytes, h, w, batch, stream);
}

extern "C" int nd_unet_grad_forward(int flags, const float *params, void *blobs, const float *x, float *y, int batch, int h, int w,
                                    void *ws, size_t ws_bytes, void *stream) {
    return forward_entry(false, "nd_unet_grad_forward", flags, params, nullptr, 0.f, blobs, x, y, batch, h, w, ws, ws_bytes, stream);
}
extern "C" int nd_unet_train_forward(int flags, float *params, void *blobs, const float *x, float *y, int batch, int h, int w,
                                     float momentum, void *ws, size_t ws_bytes, void *stream) {
    return forward_entry(true, "nd_unet_train_forward", flags, params, params, momentum, blobs, x, y, batch, h, w, ws, ws_bytes, stream);
}
extern "C" int nd_unet_grad_backward(int flags, const float *params, float *grads, void *blobs, const float *gy, float *dx, int batch,
                                     int h, int w, void *ws, size_t ws_bytes, void *stream) {
    return backward_entry(false, "nd_unet_grad_backward", flags, params, grads, blobs, gy, dx, batch, h, w, ws, ws_bytes, stream);
}
extern "C" int nd_unet_train_backward(int flags, const float *params, float *grads, void *blobs, const float *gy, float *dx, int batch,
                                      int h, int w, void *ws, size_t ws_bytes, void *stream) {
    return backward_entry(true, "nd_unet_train_backward", flags, params, grads, blobs, gy, dx, batch, h, w, ws, ws_bytes, stream);
}
