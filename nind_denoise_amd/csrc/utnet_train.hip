// UtNet training step (forward + loss + backward) -- BASELINE config 5 / SURVEY.md section 8(f) rank 3.
// Reference: nn_train.py:308-380 (loop), nn_common.py:198-255 (denoise_batch = model(x).clip(0,1); compute_loss;
// loss.backward(); Adam(amsgrad).step()).
//
// Everything heavy reuses the inference machinery:
//   forward        the inference launch sequence (run_stack) with the conv epilogue also storing acc + bias ("pre")
//   data gradient  the SAME conv kernel on the weight tensor read in its transposed role:
//                  dgrad(Conv2d) = ConvTranspose2d, dgrad(ConvTranspose2d) = Conv2d, dgrad(ConvT 2x2 s2) = Conv 2x2 s2
//   weight gradient k_wgrad (wgrad.hip): MFMA contraction over pixels on a common grid (k_repitch)
// Small HBM-bound kernels below: PReLU backward (+ slope gradient), max-pool backward, final 1x1 backward, bias
// sums, device-side weight packing.  The loss and its gradient: nd_criteria_grad (criteria.hip); Adam(amsgrad): optim.hip.
// Gradients come out in ONE flat fp32 buffer in state-dict order, so the data-parallel all-reduce (RCCL) and the
// optimizer are single flat operations.
#include <math.h>

#include <algorithm>

#include "utnet_net.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

int nd_launch_repitch(const QpBuf &src, int src_plane0, int planes, int ss, int sy, int sx, const QpBuf &dst, int oy,
                      int ox, int h, int w, hipStream_t s);
size_t nd_wgrad_partial_floats(int taps, int M, int N, long K, int *ksplit_out, int *cps_out);
int nd_launch_wgrad(const QpBuf &A, int a_plane0, int M, const QpBuf &Bq, int b_plane0, int N, int taps, int taps_total,
                    int tap0, float *partial, size_t partial_floats, float *dw, hipStream_t s);
int nd_launch_channel_sum(const QpBuf &src, int plane0, int C, float *out, float *scratch, hipStream_t s);

// ------------------------------------------------------------------ elementwise kernels
// g (interior of a bordered gradient buffer, planes [plane0, plane0+planes)) *= act'(pre), pre = conv output + bias;
// PReLU also: partial[block] = sum g*pre over pre <= 0 (the slope's gradient).  ELU: act' = 1 | exp(pre); Hardswish: 0 | (2 pre + 3) / 6 | 1
// (torch's derivative at the break points: PReLU'(0) = slope, ELU'(0) = 1 from the exp branch, Hardswish'(-3) = 0 and Hardswish'(+3) = 1:
// the middle branch (2x+3)/6, which would give -1/2 and 3/2 there, holds on the open interval only -- see below)
template <int ACT>
__global__ __launch_bounds__(256) void k_act_bwd(f32x4 *__restrict__ g, long gnp, int gHb, int gWb, int gpad,
                                                 const f32x4 *__restrict__ pre, long pnp, int H, int W,
                                                 const float *__restrict__ slope, float *__restrict__ partial) {
    __shared__ float red[256];
    const int b = blockIdx.x, q = blockIdx.y;
    const float a = ACT == ND_ACT_PRELU ? *slope : 0.f;
    float acc = 0.f;
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int y = i / W, x = i - y * W;
        f32x4 *gp = g + (long)q * gnp + ((long)b * gHb + y + gpad) * gWb + x + gpad;
        const f32x4 pv = pre[(long)q * pnp + (long)b * H * W + i];
        f32x4 gv = *gp;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (ACT == ND_ACT_PRELU) {
                if (!(pv[e] > 0.f)) {
                    acc += gv[e] * pv[e];
                    gv[e] *= a;
                }
            } else if (ACT == ND_ACT_ELU) {
                if (!(pv[e] > 0.f)) gv[e] *= expf(pv[e]);                     // torch: grad * (x <= 0 ? alpha * exp(x) : 1), alpha = 1
            } else {
                // torch hardswish_backward: x <= -3 -> 0;  x < 3 -> grad * (x / 3 + 0.5);  else grad
                gv[e] = pv[e] <= -3.f ? 0.f : (pv[e] < 3.f ? gv[e] * (pv[e] / 3.f + 0.5f) : gv[e]);
            }
        }
        *gp = gv;
    }
    if (ACT != ND_ACT_PRELU) return;
    acc = nd_block_sum(acc, red);
    if (threadIdx.x == 0) partial[(long)q * gridDim.x + b] = acc;
}

// gfine[argmax of each 2x2 window] += gpool   (fwd: the forward values that were pooled; first maximum in row-major order)
__global__ void k_maxpool_bwd_add(const f32x4 *__restrict__ gpool, long pnp, int pHb, int pWb, int ppad,
                                  const f32x4 *__restrict__ fwd, long fnp, int fHb, int fWb, int fpad,
                                  f32x4 *__restrict__ gfine, long gnp, int gHb, int gWb, int gpad, int Ho, int Wo, int B) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int b = blockIdx.z % B, q = blockIdx.z / B;
    if (x >= Wo) return;
    const f32x4 gv = gpool[(long)q * pnp + ((long)b * pHb + y + ppad) * pWb + x + ppad];
    const f32x4 *f = fwd + (long)q * fnp + ((long)b * fHb + 2 * y + fpad) * fWb + 2 * x + fpad;
    f32x4 *g = gfine + (long)q * gnp + ((long)b * gHb + 2 * y + gpad) * gWb + 2 * x + gpad;
    const f32x4 v[4] = {f[0], f[1], f[fWb], f[fWb + 1]};
    f32x4 o[4] = {g[0], g[1], g[gWb], g[gWb + 1]};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int best = 0;
        float m = v[0][e];
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (v[k][e] > m) {
                m = v[k][e];
                best = k;
            }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k == best) o[k][e] += gv[e];
    }
    g[0] = o[0];
    g[1] = o[1];
    g[gWb] = o[2];
    g[gWb + 1] = o[3];
}

// data gradient of the final Conv2d(f,3,1) + crop: g[c][b][Y][X] = sum_co gy[co][b][Y-crop][X-crop] * w[co][c] (0 outside)
__global__ void k_final_bwd_data(const float *__restrict__ gy, int H, int W, const float *__restrict__ w, int cin, int crop,
                                 f32x4 *__restrict__ g, long gnp, int Hb, int Wb, int B) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    const int Y = blockIdx.y;
    const int b = blockIdx.z % B, q = blockIdx.z / B;
    if (X >= Wb) return;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    const int yy = Y - crop, xx = X - crop;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const float *p = gy + ((long)b * 3 * H + yy) * W + xx;
        const float g0 = p[0], g1 = p[(long)H * W], g2 = p[2 * (long)H * W];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            if (c < cin) o[e] = g0 * w[c] + g1 * w[cin + c] + g2 * w[2 * cin + c];
        }
    }
    g[(long)q * gnp + ((long)b * Hb + Y) * Wb + X] = o;
}

// weight / bias gradient of the final 1x1, stage 1: one workgroup per (co, plane, image) -> partial[(co*planes+q)*B + b] (x,y,z,w = dw, then db)
__global__ __launch_bounds__(256) void k_final_wgrad1(const float *__restrict__ gy, int H, int W, const f32x4 *__restrict__ act, long anp,
                                                      int Hb, int Wb, int crop, f32x4 *__restrict__ pw, float *__restrict__ pb) {
    __shared__ f32x4 red[256];
    __shared__ float redb[256];
    const int co = blockIdx.x, q = blockIdx.y, b = blockIdx.z;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float accb = 0.f;
    for (int i = threadIdx.x; i < H * W; i += 256) {
        const int y = i / W, x = i - y * W;
        const float gv = gy[(((long)b * 3 + co) * H + y) * W + x];
        acc += act[(long)q * anp + ((long)b * Hb + y + crop) * Wb + x + crop] * gv;
        accb += gv;
    }
    acc = nd_block_sum(acc, red);
    accb = nd_block_sum(accb, redb);
    if (threadIdx.x == 0) {
        const long o = ((long)co * gridDim.y + q) * gridDim.z + b;
        pw[o] = acc;
        pb[o] = accb;
    }
}
__global__ __launch_bounds__(64) void k_final_wgrad2(const f32x4 *__restrict__ pw, const float *__restrict__ pb, int planes, int B,
                                                     int cin, float *__restrict__ dw, float *__restrict__ db) {
    const int co = blockIdx.x, q = blockIdx.y;
    const long o = ((long)co * planes + q) * B;
    if (threadIdx.x < 4 && 4 * q + (int)threadIdx.x < cin) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += pw[o + b][threadIdx.x];
        dw[(long)co * cin + 4 * q + threadIdx.x] = acc;
    }
    if (threadIdx.x == 4 && q == 0) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += pb[o + b];
        db[co] = acc;
    }
}

// d loss / d input image: the data gradient of the first Conv2d(3, f, 3) fused with the adjoint of ReflectionPad2d(2) (UtNet.py:27,98).
// g1 = d loss / d pre-activation of convs1.0: f/4 planes of an (H+2) x (W+2) grid inside a zero border of gpad >= 2;
// w0 = convs1.0.weight [f][3][3][3]; dx [B,3,H,W] NCHW.  On the (H+4) x (W+4) padded input grid
//     gP[c][v][u] = sum_co sum_ky,kx g1[co][v-ky][u-kx] * w0[co][c][ky][kx]        (g1 zero outside its grid: the border)
// and dx[c][y][x] = sum of gP[c][v][u] over the (v, u) that the reflection maps onto (y, x): v = y + 2, plus v = 2 - y for
// y = 1, 2 and v = 2H - y for y = H-3, H-2 (the mirror that does not repeat the edge, reflect_nr); the same along x.
// gP is linear in g1, so a lane sums the 1, 2 or 4 source windows of g1 first and contracts once with w0.  A workgroup = one
// 16 x 4 pixel patch of one image x kIgGroups plane groups (wave w takes planes w, w + kIgGroups, ...: short dependent chains,
// four times the waves in flight); the groups' partial sums meet in LDS in a fixed order.  The patch shape keeps a wave's 3 x 3
// windows within 6 rows of 18 pixels (L1 reuse), and only waves on the image's edge take the mirror branches.  w0 indices are
// uniform (scalar loads).  Every output written once, no atomics.
constexpr int kIgGroups = 4;
__global__ __launch_bounds__(64 * kIgGroups) void k_input_grad(const f32x4 *__restrict__ g1, long gnp, int gHb, int gWb, int gpad,
                                                               int planes, const float *__restrict__ w0, int H, int W,
                                                               float *__restrict__ dx) {
    __shared__ float part[kIgGroups][3][64];
    const int lane = threadIdx.x & 63, grp = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: scalar weight loads
    const int b = blockIdx.z;
    const bool live = (int)blockIdx.x * 16 + (lane & 15) < W && (int)blockIdx.y * 4 + (lane >> 4) < H;
    const int x = live ? blockIdx.x * 16 + (lane & 15) : 0, y = live ? blockIdx.y * 4 + (lane >> 4) : 0;
    // bordered row of g1 for padded row v and tap ky: v - ky + gpad; rows of the second source as an offset from the first
    const int vm = (y == 1 || y == 2) ? 2 - y : ((y == H - 2 || y == H - 3) ? 2 * H - y : -1);
    const int um = (x == 1 || x == 2) ? 2 - x : ((x == W - 2 || x == W - 3) ? 2 * W - x : -1);
    const long drow = vm >= 0 ? (long)(vm - (y + 2)) * gWb : 0;
    const int dcol = um >= 0 ? um - (x + 2) : 0;
    const f32x4 *gb = g1 + ((long)b * gHb + y + 2 + gpad) * gWb + x + 2 + gpad;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int q = grp; q < planes; q += kIgGroups) {
        const f32x4 *gq = gb + (long)q * gnp;
        const float *wq = w0 + (long)q * 4 * 27;   // co = 4q .. 4q+3: 108 contiguous floats [e][c][ky][kx]
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const int ky = t / 3, kx = t - 3 * ky;
            const f32x4 *p = gq - (long)ky * gWb - kx;
            f32x4 s = p[0];
            if (vm >= 0) s += p[drow];
            if (um >= 0) s += p[dcol];
            if (vm >= 0 && um >= 0) s += p[drow + dcol];
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
    for (int k = 1; k < kIgGroups; ++k) v += part[k][c][lane];
    dx[(((long)b * 3 + c) * H + y) * W + x] = v;
}

namespace {

inline int transposed_kind(int kind) {
    return kind == ND_CONV3 ? ND_CONVT3 : (kind == ND_CONVT3 ? ND_CONV3 : (kind == ND_CONVT2S2 ? ND_CONV2S2 : -1));
}

// flat parameter layout = state-dict order (nd_utnet_tensor_name)
struct ParamLayout {
    std::vector<size_t> off, cnt;
    size_t total;
};
ParamLayout param_layout(int f) {
    ParamLayout pl;
    size_t o = 0;
    for (const std::string &name : tensor_names()) {
        size_t n = 1;   // PReLU slope
        for (int i = 0; i < kNumLayers; ++i) {
            const LayerSpec &l = kLayers[i];
            const int k = l.kind == ND_CONV1 ? 1 : (l.kind == ND_CONVT2S2 ? 2 : 3);
            if (name == std::string(l.key) + ".weight") n = (size_t)lcin(l, f) * lcout(l, f) * k * k;
            if (name == std::string(l.key) + ".bias") n = (size_t)lcout(l, f);
        }
        pl.off.push_back(o);
        pl.cnt.push_back(n);
        o += n;
    }
    pl.total = o;
    return pl;
}
// Gradient buckets for a data-parallel reduction that overlaps the backward pass: one per decoder / encoder level, numbered in
// the order the backward pass COMPLETES them (0: up4 + tconvs4, 1: up3 + tconvs3, 2: up2 + tconvs2, 3: up1 + tconvs1, 4: bottom,
// 5: convs4, 6: convs3, 7: convs2, 8: convs1).  Each is one contiguous range of the flat state-dict-order buffer.
constexpr int kNumBuckets = 9;
int bucket_of_key(const std::string &key) {
    static const char *const prefix[kNumBuckets][2] = {{"tconvs4", "up4"}, {"tconvs3", "up3"}, {"tconvs2", "up2"}, {"tconvs1", "up1"},
                                                        {"bottom", "bottom"}, {"convs4", "convs4"}, {"convs3", "convs3"},
                                                        {"convs2", "convs2"}, {"convs1", "convs1"}};
    for (int k = 0; k < kNumBuckets; ++k)
        for (int j = 0; j < 2; ++j) {
            const std::string p = prefix[k][j];
            if (key.compare(0, p.size(), p) == 0 && (key.size() == p.size() || key[p.size()] == '.')) return k;
        }
    return -1;
}
// the layer whose gradients finish a bucket: the bucket's first layer in forward order
int bucket_tail_layer(int k) {
    for (int i = 0; i < kNumLayers; ++i)
        if (bucket_of_key(kLayers[i].key) == k) return i;
    return -1;
}
// name of the PReLU tensor that follows layer `key` in its Sequential
std::string prelu_name(const char *key) {
    std::string k(key);
    const size_t dot = k.rfind('.');
    return k.substr(0, dot + 1) + std::to_string(atoi(k.c_str() + dot + 1) + 1) + ".weight";
}

struct BwdBlob {   // dgrad weights: per layer the transposed-kind packing (none for layer 0 and the final 1x1)
    size_t off[kNumLayers];
    size_t total;
};
BwdBlob bwd_blob_layout(int f) {
    BwdBlob b;
    size_t o = 0;
    for (int i = 0; i < kNumLayers; ++i) {
        b.off[i] = o;
        const LayerSpec &l = kLayers[i];
        if (i == 0 || l.kind == ND_CONV1) continue;
        const int kt = transposed_kind(l.kind);
        size_t n = nd_packed_floats(kt, lcout(l, f), lcin(l, f), ND_F32);
        if (kt == ND_CONV3 || kt == ND_CONVT3) n = std::max(n, nd_w1d_packed_floats(kW1dTile, lcout(l, f), lcin(l, f)));   // either packing
        o += n;
    }
    b.total = o;
    return b;
}

struct TrainPlan {
    Plan fwd;
    QpBuf pre[kNumSlopes];
    QpBuf g[NBUF];
    QpBuf scratch;          // re-pitched wgrad operand (largest over the layers)
    float *partial;         // wgrad K-slice partial sums
    size_t partial_floats;
    float *red;             // reduction scratch
    float *gy;              // d loss / d output  [B,3,H,W]
    char *crit_ws;          // nd_criteria_grad_workspace_bytes(B, H, W, 0): serves every loss_cs
    size_t crit_ws_bytes;
    size_t bytes;
};
constexpr int kRedFloats = 1 << 19;   // reduction scratch: >= 4 floats x planes x batch

int step_of_layer(int layer) {
    for (int i = 0; i < kNumSteps; ++i)
        if (kSteps[i].layer == layer) return i;
    return -1;
}
// pad of a gradient buffer: 2 when the tensor is produced by a Conv2d(3) layer (its data gradient is a transpose conv,
// which reads a zero-bordered input), else 0
int grad_pad(Buf id) {
    switch (id) {
        case A1: case A2: case A3: case A4: case BT0: case CAT1: case CAT2: case CAT3: case CAT4: return 2;
        default: return 0;
    }
}

TrainPlan make_train_plan(int f, int h, int w, int B, char *base) {
    TrainPlan t;
    t.fwd = make_plan(f, h, w, B, B, base, ND_F32);
    size_t off = t.fwd.bytes;
    auto alloc = [&](QpBuf &q, int planes, int Hb, int Wb, int pad) {
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
    };
    // pre-activation copies: compact, the layer's output size
    for (int i = 0; i < kNumLayers; ++i) {
        const LayerSpec &l = kLayers[i];
        if (l.prelu < 0) continue;
        const QpBuf &o = t.fwd.buf[kSteps[step_of_layer(i)].dst];
        alloc(t.pre[l.prelu], lcout(l, f) / 4, o.Hb - 2 * o.pad, o.Wb - 2 * o.pad, 0);
    }
    // gradient buffers
    size_t scratch_elems = 0;
    for (int id = 1; id < NBUF; ++id) {
        const QpBuf &o = t.fwd.buf[id];
        const int pad = grad_pad((Buf)id);
        alloc(t.g[id], o.planes, o.Hb - 2 * o.pad + 2 * pad, o.Wb - 2 * o.pad + 2 * pad, pad);
    }
    t.g[X0] = QpBuf();
    // scratch + wgrad partials: maxima over the layers
    size_t pf = 0;
    for (int i = 0; i < kNumLayers - 1; ++i) {
        const LayerSpec &l = kLayers[i];
        const Step &st = kSteps[step_of_layer(i)];
        const QpBuf &in = t.fwd.buf[st.src], &out = t.fwd.buf[st.dst];
        const int ih = in.Hb - 2 * in.pad, iw = in.Wb - 2 * in.pad, oh = out.Hb - 2 * out.pad, ow = out.Wb - 2 * out.pad;
        const int ci = lcin(l, f), co = lcout(l, f);
        size_t e = 0, p = 0;
        if (l.kind == ND_CONV3) {          // A = g(out) on the input grid
            e = (size_t)(co / 4) * B * in.Hb * in.Wb;
            p = nd_wgrad_partial_floats(9, co, ci, (long)B * in.Hb * in.Wb, nullptr, nullptr);
        } else if (l.kind == ND_CONVT3) {  // A = input interior on the output grid
            e = (size_t)((ci + 3) / 4) * B * oh * ow;
            p = nd_wgrad_partial_floats(9, ci, co, (long)B * oh * ow, nullptr, nullptr);
        } else {                           // up: B = one phase of g(out) on the input grid
            e = (size_t)(co / 4) * B * ih * iw;
            p = nd_wgrad_partial_floats(1, ci, co, (long)B * ih * iw, nullptr, nullptr);
        }
        if (e > scratch_elems) scratch_elems = e;
        if (p > pf) pf = p;
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
    off += kRedFloats * 4;
    t.gy = (float *)(base ? base + off : nullptr);
    off += (size_t)B * 3 * h * w * 4;
    off = (off + 255) & ~(size_t)255;
    t.crit_ws = base ? base + off : nullptr;
    t.crit_ws_bytes = nd_criteria_grad_workspace_bytes(B, h, w, 0);
    off += (t.crit_ws_bytes + 255) & ~(size_t)255;
    t.bytes = off;
    return t;
}

QpBuf scratch_view(const TrainPlan &t, int planes, int B, int H, int W) {
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

int check_train(int funit, int h, int w, int batch) {
    if (funit < 8 || funit % 8) ND_FAIL(ND_EINVAL, "UtNet training: funit=%d must be a positive multiple of 8", funit);
    for (int cs : {h, w})
        if (!valid_cs(cs)) ND_FAIL(ND_EINVAL, "UtNet training: crop side %d is not of the form 16k+56 (e.g. 136, 184)", cs);
    if (batch <= 0) ND_FAIL(ND_EINVAL, "UtNet training: batch=%d", batch);
    return ND_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t nd_utnet_param_count(int funit) { return (funit < 8 || funit % 8) ? 0 : param_layout(funit).total; }
extern "C" int nd_utnet_param_range(int funit, int tensor_idx, size_t *offset, size_t *count) {
    if (funit < 8 || funit % 8) ND_FAIL(ND_EINVAL, "bad funit");
    const ParamLayout pl = param_layout(funit);
    if (tensor_idx < 0 || tensor_idx >= (int)pl.off.size()) ND_FAIL(ND_EINVAL, "tensor index %d out of range", tensor_idx);
    if (offset) *offset = pl.off[tensor_idx];
    if (count) *count = pl.cnt[tensor_idx];
    return ND_OK;
}
extern "C" size_t nd_utnet_train_blob_bytes(int funit) {
    if (funit < 8 || funit % 8) return 0;
    return (blob_layout(funit, ND_F32, true).total + bwd_blob_layout(funit).total) * sizeof(float);
}
extern "C" size_t nd_utnet_train_workspace_bytes_hw(int funit, int h, int w, int batch) {
    if (check_train(funit, h, w, batch) != ND_OK) return 0;
    return make_train_plan(funit, h, w, batch, nullptr).bytes;
}
extern "C" int nd_utnet_train_workspace_init_hw(void *ws, size_t ws_bytes, int funit, int h, int w, int batch, void *stream) {
    ND_TRY(check_train(funit, h, w, batch));
    const size_t need = make_train_plan(funit, h, w, batch, nullptr).bytes;
    if (!ws || ws_bytes < need) ND_FAIL(ND_ENOMEM, "UtNet training workspace: %zu B given, %zu B needed", ws_bytes, need);
    ND_HIP(hipMemsetAsync(ws, 0, need, (hipStream_t)stream));   // zero borders of activations AND gradients, slack
    return ND_OK;
}

// ---- the step in two halves: (1) weight packing + forward with the pre-activations kept, (2) backward from d loss / d output.
// nd_utnet_train_step_act_hw runs both with the loss (nd_criteria_grad) between them; nd_utnet_train_forward_hw / nd_utnet_train_backward_hw expose the halves
// to torch.autograd (networks/UtNet.py: model(x).clip(0, 1), loss.backward() of nn_common.py:198-218 then work unchanged).
struct TrainCtx {
    int f, B, H, W, flags, act;
    TrainPlan t;
    ParamLayout pl;
    BlobLayout bl;
    BwdBlob bb;
    float *fblob, *bblob;
    unsigned char fwd_w1[kNumLayers], bwd_w1[kNumLayers];
    const float *slopes[kNumSlopes];
    hipStream_t s;
};

static int train_ctx(TrainCtx &c, int funit, int flags, int act, const float *params, void *blobs, int batch, int h, int w, void *ws,
                     size_t ws_bytes, void *stream) {
    ND_TRY(nd_check_flags(flags));
    ND_TRY(check_train(funit, h, w, batch));
    if (act < ND_ACT_PRELU || act > ND_ACT_HARDSWISH) ND_FAIL(ND_EINVAL, "UtNet training: unknown activation %d", act);
    if (!params || !blobs || !ws) ND_FAIL(ND_EINVAL, "train step: null pointer");
    c.f = funit;
    c.B = batch;
    c.H = h;
    c.W = w;
    c.flags = flags;
    c.act = act;
    c.t = make_train_plan(funit, h, w, batch, (char *)ws);
    if (ws_bytes < c.t.bytes) ND_FAIL(ND_ENOMEM, "UtNet training workspace: %zu B given, %zu B needed", ws_bytes, c.t.bytes);
    c.s = (hipStream_t)stream;
    c.pl = param_layout(funit);
    c.bl = blob_layout(funit, ND_F32, true);
    // 3x3 layers whose rows fit its LDS images run the fused 1-D Winograd kernel, forward and data gradient (else the direct one)
    memset(c.fwd_w1, 0, sizeof(c.fwd_w1));
    memset(c.bwd_w1, 0, sizeof(c.bwd_w1));
    for (const Step &st : kSteps) {
        if (st.layer < 0) continue;
        const LayerSpec &l = kLayers[st.layer];
        if (l.kind != ND_CONV3 && l.kind != ND_CONVT3) continue;
        if (!(flags & ND_FLAG_DIRECT_CONV)) {
            c.fwd_w1[st.layer] = nd_w1d_fits(kW1dTile, c.t.fwd.buf[st.src]);
            c.bwd_w1[st.layer] = st.layer > 0 && nd_w1d_fits(kW1dTile, c.t.g[st.dst]);
        }
    }
    c.bb = bwd_blob_layout(funit);
    c.fblob = (float *)blobs;
    c.bblob = c.fblob + c.bl.total;
    for (int k = 0; k < kNumSlopes; ++k) c.slopes[k] = nullptr;
    for (int i = 0; i < kNumLayers; ++i)
        if (kLayers[i].prelu >= 0) c.slopes[kLayers[i].prelu] = params + c.pl.off[tensor_index(prelu_name(kLayers[i].key))];
    return ND_OK;
}

// (1) pack the weights on the device (forward roles, and transposed roles for the data gradients), forward with the
// pre-activations kept; y_out: [batch,3,H,W]
static int train_forward(TrainCtx &c, const float *params, const float *x, float *y_out) {
    const int f = c.f, B = c.B, H = c.H, W = c.W;
    hipStream_t s = c.s;
    const BlobLayout &bl = c.bl;
    const BwdBlob &bb = c.bb;
    float *fblob = c.fblob, *bblob = c.bblob;
    auto P = [&](const std::string &name) -> const float * { return params + c.pl.off[tensor_index(name)]; };
    for (int i = 0; i < kNumLayers; ++i) {
        const LayerSpec &l = kLayers[i];
        const int ci = lcin(l, f), co = lcout(l, f);
        const float *w = P(std::string(l.key) + ".weight"), *b = P(std::string(l.key) + ".bias");
        if (l.kind == ND_CONV1) {
            ND_HIP(hipMemcpyAsync(fblob + bl.off[i], w, sizeof(float) * 3 * ci, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemcpyAsync(fblob + bl.off[i] + 3 * ci, b, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
            continue;
        }
        if (c.fwd_w1[i])
            nd_pack_w1d_device(kW1dTile, l.kind, ci, co, w, b, fblob + bl.off[i], s);
        else
            nd_pack_layer_device(l.kind, ci, co, ND_F32, w, b, fblob + bl.off[i], s);
        if (i > 0) {   // transposed role: cin' = co, cout' = ci, no bias
            const int kt = transposed_kind(l.kind);
            if (c.bwd_w1[i])
                nd_pack_w1d_device(kW1dTile, kt, co, ci, w, nullptr, bblob + bb.off[i], s);
            else
                nd_pack_layer_device(kt, co, ci, ND_F32, w, nullptr, bblob + bb.off[i], s);
        }
    }
    ND_HIP(hipGetLastError());
    // slope table of the forward blob header (PReLU only: the other activations have no parameters)
    if (c.act == ND_ACT_PRELU)
        for (int k = 0; k < kNumSlopes; ++k)
            ND_HIP(hipMemcpyAsync(fblob + k, c.slopes[k], sizeof(float), hipMemcpyDeviceToDevice, s));
    ND_TRY(nd_launch_reflect_pack(x, B, H, W, c.t.fwd.buf[X0], s));
    StackOpts o;
    o.flags = c.flags;
    o.pre = c.t.pre;
    o.train_w1 = c.fwd_w1;
    ND_TRY(run_stack(f, c.act, ND_F32, fblob, c.t.fwd, s, o));
    const float *fw = fblob + bl.off[kNumLayers - 1];
    ND_TRY(nd_launch_final1x1(c.t.fwd.buf[T4B], f, fw, fw + 3 * f, 2, y_out, H, W, s));
    return ND_OK;
}

// max-pool backward: planes [g_plane0, +planes) of gfine += the gradient of the pooled tensor gpool (planes from 0) at the argmax of
// each 2x2 window of fwd (planes from fwd_plane0)
int nd_launch_maxpool_bwd_add(const QpBuf &gpool, const QpBuf &fwd, int fwd_plane0, const QpBuf &gfine, int g_plane0, int planes,
                              hipStream_t s) {
    const int Ho = gpool.Hb - 2 * gpool.pad, Wo = gpool.Wb - 2 * gpool.pad, B = gpool.B;
    if (fwd.Hb - 2 * fwd.pad < 2 * Ho || fwd.Wb - 2 * fwd.pad < 2 * Wo || gfine.Hb - 2 * gfine.pad < 2 * Ho || gfine.Wb - 2 * gfine.pad < 2 * Wo ||
        fwd.B != B || gfine.B != B || gpool.planes < planes || fwd.planes < fwd_plane0 + planes || gfine.planes < g_plane0 + planes)
        ND_FAIL(ND_EINVAL, "maxpool backward: buffers do not fit %d planes of %d x %d windows", planes, Ho, Wo);
    dim3 grid((Wo + 127) / 128, Ho, B * planes);
    hipLaunchKernelGGL(k_maxpool_bwd_add, grid, dim3(128), 0, s, (const f32x4 *)gpool.base, gpool.np(), gpool.Hb, gpool.Wb, gpool.pad,
                       (const f32x4 *)fwd.base + (long)fwd_plane0 * fwd.np(), fwd.np(), fwd.Hb, fwd.Wb, fwd.pad,
                       (f32x4 *)gfine.base + (long)g_plane0 * gfine.np(), gfine.np(), gfine.Hb, gfine.Wb, gfine.pad, Ho, Wo, B);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
// final Conv2d(cin, 3, 1) behind a crop of `crop` pixels: weight [3][cin] and bias [3] gradients from gy [B,3,H,W] and the layer's
// input `act` (H + 2 crop rows); red: 5 * 3 * ceil(cin/4) * B floats of scratch
int nd_launch_final_wgrad(const float *gy, int H, int W, const QpBuf &act, int cin, int crop, float *red, float *dw, float *db,
                          hipStream_t s) {
    const int planes = (cin + 3) / 4, B = act.B;
    if (act.Hb != H + 2 * crop || act.Wb != W + 2 * crop || act.planes < planes) ND_FAIL(ND_EINVAL, "final 1x1 weight gradient: bad input geometry");
    f32x4 *pw = (f32x4 *)red;
    float *pb = red + (size_t)4 * 3 * planes * B;
    hipLaunchKernelGGL(k_final_wgrad1, dim3(3, planes, B), dim3(256), 0, s, gy, H, W, (const f32x4 *)act.base, act.np(), act.Hb, act.Wb,
                       crop, pw, pb);
    hipLaunchKernelGGL(k_final_wgrad2, dim3(3, planes), dim3(64), 0, s, (const f32x4 *)pw, (const float *)pb, planes, B, cin, dw, db);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
// ... and its data gradient into every element of g (ceil(cin/4) planes of H + 2 crop rows: zero outside the H x W centre)
int nd_launch_final_bwd_data(const float *gy, int H, int W, const float *w, int cin, int crop, const QpBuf &g, hipStream_t s) {
    if (g.Hb != H + 2 * crop || g.Wb != W + 2 * crop || g.planes < (cin + 3) / 4) ND_FAIL(ND_EINVAL, "final 1x1 data gradient: bad destination geometry");
    dim3 grid((g.Wb + 127) / 128, g.Hb, g.B * ((cin + 3) / 4));
    hipLaunchKernelGGL(k_final_bwd_data, grid, dim3(128), 0, s, gy, H, W, w, cin, crop, (f32x4 *)g.base, g.np(), g.Hb, g.Wb, g.B);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_launch_input_grad(const QpBuf &g1, const float *w0, int H, int W, float *dx, hipStream_t s) {
    if (g1.dt != ND_F32 || g1.pad < 2 || g1.Hb != H + 2 + 2 * g1.pad || g1.Wb != W + 2 + 2 * g1.pad)
        ND_FAIL(ND_EINVAL, "input gradient: bad source geometry");
    dim3 grid((unsigned)((W + 15) / 16), (unsigned)((H + 3) / 4), g1.B);
    hipLaunchKernelGGL(k_input_grad, grid, dim3(64 * kIgGroups), 0, s, (const f32x4 *)g1.base, g1.np(), g1.Hb, g1.Wb, g1.pad,
                       g1.planes, w0, H, W, dx);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// (2) backward: gy = d loss / d output [batch,3,H,W].  grads (nullable): every parameter gradient into the flat buffer;
// dx (nullable): d loss / d input image [batch,3,H,W].  Parameter-gradient launches and bucket events run only with grads.
static int train_backward(TrainCtx &c, const float *params, float *grads, const float *gy, float *dx, void *const *bucket_ev = nullptr) {
    const int f = c.f, B = c.B, H = c.H, W = c.W, flags = c.flags;
    hipStream_t s = c.s;
    TrainPlan &t = c.t;
    const BlobLayout &bl = c.bl;
    const BwdBlob &bb = c.bb;
    float *fblob = c.fblob, *bblob = c.bblob;
    const float *const *slopes = c.slopes;
    auto G = [&](const std::string &name) -> float * { return grads + c.pl.off[tensor_index(name)]; };
    const float *fw = fblob + bl.off[kNumLayers - 1];
    // ---- 4. backward
    // final 1x1
    if (grads)
        ND_TRY(nd_launch_final_wgrad(gy, H, W, t.fwd.buf[T4B], f, 2, t.red, G("tconvs4.4.weight"), G("tconvs4.4.bias"), s));
    ND_TRY(nd_launch_final_bwd_data(gy, H, W, fw, f, 2, t.g[T4B], s));
    for (int si = kNumSteps - 1; si >= 0; --si) {
        const Step &st = kSteps[si];
        if (st.layer < 0) {
            // pool: the skip half of the concat buffer was pooled into P; route g(P) back and ADD it to g(skip)
            const int planes = st.dst_plane0_mul * f / 4, plane0 = planes;
            ND_TRY(nd_launch_maxpool_bwd_add(t.g[st.dst], t.fwd.buf[st.src], plane0, t.g[st.src], plane0, planes, s));
            continue;
        }
        const LayerSpec &l = kLayers[st.layer];
        const int ci = lcin(l, f), co = lcout(l, f);
        const QpBuf &in = t.fwd.buf[st.src];    // layer input (forward values)
        const QpBuf &go = t.g[st.dst];          // gradient of the layer's output buffer
        const int oplane0 = st.dst_plane0_mul * f / 4, oplanes = co / 4;
        const int oh = go.Hb - 2 * go.pad, ow = go.Wb - 2 * go.pad;
        const int ih = in.Hb - 2 * in.pad, iw = in.Wb - 2 * in.pad;
        // activation backward (in place) + slope gradient
        if (l.prelu >= 0) {
            const QpBuf &pr = t.pre[l.prelu];
            f32x4 *gq = (f32x4 *)go.base + (long)oplane0 * go.np();
            if (c.act == ND_ACT_PRELU) {
                hipLaunchKernelGGL(k_act_bwd<ND_ACT_PRELU>, dim3(B, oplanes), dim3(256), 0, s, gq, go.np(), go.Hb, go.Wb, go.pad,
                                   (const f32x4 *)pr.base, pr.np(), oh, ow, slopes[l.prelu], t.red);
                if (grads) ND_TRY(nd_launch_sum(t.red, B * oplanes, 1.f, G(prelu_name(l.key)), s));
            } else if (c.act == ND_ACT_ELU) {
                hipLaunchKernelGGL(k_act_bwd<ND_ACT_ELU>, dim3(B, oplanes), dim3(256), 0, s, gq, go.np(), go.Hb, go.Wb, go.pad,
                                   (const f32x4 *)pr.base, pr.np(), oh, ow, (const float *)nullptr, t.red);
            } else {
                hipLaunchKernelGGL(k_act_bwd<ND_ACT_HARDSWISH>, dim3(B, oplanes), dim3(256), 0, s, gq, go.np(), go.Hb, go.Wb, go.pad,
                                   (const f32x4 *)pr.base, pr.np(), oh, ow, (const float *)nullptr, t.red);
            }
            ND_HIP(hipGetLastError());
        }
        // bias gradient
        if (grads) ND_TRY(nd_launch_channel_sum(go, oplane0, co, G(std::string(l.key) + ".bias"), t.red, s));
        // weight gradient (none without `grads`: frozen parameters)
        float *dw = grads ? G(std::string(l.key) + ".weight") : nullptr;
        if (grads && l.kind == ND_CONV3) {
            QpBuf a = scratch_view(t, oplanes, B, in.Hb, in.Wb);
            ND_TRY(nd_launch_repitch(go, oplane0, oplanes, 1, 0, 0, a, 0, 0, oh, ow, s));
            ND_TRY(nd_launch_wgrad(a, 0, co, in, 0, ci, 9, 9, 0, t.partial, t.partial_floats, dw, s));
        } else if (grads && l.kind == ND_CONVT3) {
            QpBuf a = scratch_view(t, (ci + 3) / 4, B, oh, ow);
            ND_TRY(nd_launch_repitch(in, 0, (ci + 3) / 4, 1, 0, 0, a, 0, 0, ih, iw, s));
            QpBuf gb = go;   // pad 0 by construction: the whole buffer is the grid
            ND_TRY(nd_launch_wgrad(a, 0, ci, gb, oplane0, co, 9, 9, 0, t.partial, t.partial_floats, dw, s));
        } else if (grads) {   // ConvTranspose2d(2, s=2): four 1-tap problems on the input grid
            for (int ab = 0; ab < 4; ++ab) {
                QpBuf bq = scratch_view(t, oplanes, B, ih, iw);
                ND_TRY(nd_launch_repitch(go, oplane0, oplanes, 2, ab >> 1, ab & 1, bq, 0, 0, ih, iw, s));
                ND_TRY(nd_launch_wgrad(in, 0, ci, bq, 0, co, 1, 4, ab, t.partial, t.partial_floats, dw, s));
            }
        }
        // data gradient into g(input buffer): a forward launch of the transposed kind
        if (st.layer > 0) {
            ConvDesc d;
            d.kind = transposed_kind(l.kind);
            d.cin = co;
            d.cout = ci;
            d.wpk = bblob + bb.off[st.layer];
            d.bias = d.wpk + nd_bias_offset(d.kind, co, ci, ND_F32, c.bwd_w1[st.layer] ? kW1dTile : 0);
            d.in = go;
            d.in_plane0 = oplane0;
            d.out = t.g[st.src];
            d.part = t.fwd.split;
            d.part_bytes = kSplitScratchBytes;
            d.nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
            // (a data gradient keeps no pre-activation copy: the F(4,3) form takes the inference path)
            ND_TRY(c.bwd_w1[st.layer] ? nd_launch_conv_f43(d, flags, s) : nd_launch_conv(d, s));
        } else if (dx) {
            // the input image's gradient: first layer's data gradient + the adjoint of ReflectionPad2d(2), one kernel
            ND_TRY(nd_launch_input_grad(go, params + c.pl.off[tensor_index("convs1.0.weight")], H, W, dx, s));
        }
        // every parameter gradient of this layer's level is final once the level's first layer is done: tell the reducer
        if (grads && bucket_ev) {
            const int k = bucket_of_key(l.key);
            if (k >= 0 && bucket_tail_layer(k) == st.layer) ND_HIP(hipEventRecord((hipEvent_t)bucket_ev[k], s));
        }
    }
    return ND_OK;
}

// One training step without the optimizer: packs the weights on the device, runs forward (act: ND_ACT_PRELU | ND_ACT_ELU |
// ND_ACT_HARDSWISH, as in the two halves below), the loss (nd_criteria_grad, criteria.hip)
//   loss = w_l1 * mean|g - target| + w_mse * mean (g - target)^2 + w_ssim * mean_n(1 - SSIM_n(g, target))
//          + w_msssim * mean_n(1 - MS-SSIM_n(g, target)),      g = clip(y, 0, 1)          (nn_common.py:198-199, 226-241)
// and the backward pass.  params / grads: flat fp32 buffers in state-dict order (nd_utnet_param_range);
// x, target, y_out: [batch,3,h,w] NCHW fp32 (each side 16k+56); loss_out: one float in HBM; blobs: nd_utnet_train_blob_bytes
// scratch.  bucket_events (nullable, else nd_utnet_grad_buckets of them): bucket_events[k] (hipEvent_t) is recorded on `stream` as soon as
// every gradient of bucket k is final -- a data-parallel run overlaps the gradient reduction with the backward pass.
extern "C" int nd_utnet_train_step_act_hw(int funit, int act, int flags, const float *params, float *grads, void *blobs, const float *x,
                                          const float *target, float *y_out, float w_l1, float w_mse, float w_ssim, float w_msssim,
                                          float *loss_out, int batch, int h, int w, int loss_cs, void *ws, size_t ws_bytes, void *stream,
                                          void *const *bucket_events, int n_events) {
    if (bucket_events && n_events != kNumBuckets) ND_FAIL(ND_EINVAL, "train step: %d bucket events expected", kNumBuckets);
    LossWindow win;   // refused before anything is launched
    ND_TRY(nd_loss_window("UtNet training", batch, h, w, loss_cs, w_ssim != 0.f, w_msssim != 0.f, &win));
    if (!grads || !x || !target || !y_out || !loss_out) ND_FAIL(ND_EINVAL, "train step: null pointer");
    TrainCtx c;
    ND_TRY(train_ctx(c, funit, flags, act, params, blobs, batch, h, w, ws, ws_bytes, stream));
    ND_TRY(train_forward(c, params, x, y_out));
    TrainPlan &t = c.t;
    // ---- 3. loss and its gradient, on the centre window (the whole output when there is none)
    ND_TRY(nd_criteria_grad(y_out, target, batch, h, w, loss_cs, w_l1, w_mse, w_ssim, w_msssim, loss_out, t.gy, t.crit_ws,
                            t.crit_ws_bytes, stream));
    return train_backward(c, params, grads, t.gy, nullptr, bucket_events);
}
// Buckets of the flat gradient buffer in the order the backward pass completes them (one per decoder / encoder level):
// offsets / counts in floats.  Returns the number of buckets (9); fills at most `max` entries.
extern "C" int nd_utnet_grad_buckets(int funit, size_t *offsets, size_t *counts, int max) {
    if (funit < 8 || funit % 8) ND_FAIL(ND_EINVAL, "bad funit");
    const ParamLayout pl = param_layout(funit);
    const auto &names = tensor_names();
    for (int k = 0; k < kNumBuckets && k < max; ++k) {
        size_t lo = (size_t)-1, hi = 0;
        for (size_t i = 0; i < names.size(); ++i) {
            const std::string key = names[i].substr(0, names[i].find('.') == std::string::npos ? names[i].size() : names[i].find('.'));
            if (bucket_of_key(key) != k) continue;
            if (pl.off[i] < lo) lo = pl.off[i];
            if (pl.off[i] + pl.cnt[i] > hi) hi = pl.off[i] + pl.cnt[i];
        }
        if (offsets) offsets[k] = lo;
        if (counts) counts[k] = hi - lo;
    }
    return kNumBuckets;
}

// The two halves for torch.autograd (act: ND_ACT_PRELU | ND_ACT_ELU | ND_ACT_HARDSWISH, the reference constructor's choices,
// networks/UtNet.py:17-26).  `ws` and `blobs` carry the forward's activations, pre-activations and packed weights to the
// backward call: the caller keeps both untouched in between.  The backward produces the parameter gradients (grads, nullable)
// and the input image's gradient (dx, nullable: the first layer's data gradient through the reflection padding); at least one.
extern "C" int nd_utnet_train_forward_hw(int funit, int act, int flags, const float *params, void *blobs, const float *x, float *y_out,
                                         int batch, int h, int w, void *ws, size_t ws_bytes, void *stream) {
    if (!x || !y_out) ND_FAIL(ND_EINVAL, "train forward: null pointer");
    TrainCtx c;
    ND_TRY(train_ctx(c, funit, flags, act, params, blobs, batch, h, w, ws, ws_bytes, stream));
    return train_forward(c, params, x, y_out);
}
extern "C" int nd_utnet_train_backward_hw(int funit, int act, int flags, const float *params, float *grads, void *blobs,
                                          const float *gy, float *dx, int batch, int h, int w, void *ws, size_t ws_bytes, void *stream,
                                          void *const *bucket_events, int n_events) {
    if (!gy) ND_FAIL(ND_EINVAL, "train backward: null pointer");
    if (!grads && !dx) ND_FAIL(ND_EINVAL, "train backward: neither parameter gradients nor the input gradient requested");
    if (bucket_events && n_events != kNumBuckets) ND_FAIL(ND_EINVAL, "train backward: %d bucket events expected", kNumBuckets);
    TrainCtx c;
    ND_TRY(train_ctx(c, funit, flags, act, params, blobs, batch, h, w, ws, ws_bytes, stream));
    return train_backward(c, params, grads, gy, dx, bucket_events);
}
