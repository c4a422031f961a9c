// The plan, the layouts and the small kernels the UNet backward passes share: eval mode on running statistics (unet_grad.hip) and
// train mode on batch statistics (unet_train.hip).  Everything here has internal linkage: each translation unit gets its own copy.
#pragma once
#include <algorithm>

#include "unet_net.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

// ------------------------------------------------------------------ kernels
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

struct GradPlan {
    UPlan fwd;
    QpBuf g[NUB];     // gradient of every activation buffer, border 1 (g[XIN]: none)
    QpBuf gup[4];     // gradient of up<n>.up's own result: 2 h_in x 2 w_in, no border (the F.pad fix-up lines dropped)
    QpBuf scratch;    // re-pitched wgrad operand (largest over the layers)
    float *partial;   // wgrad K-slice partial sums
    size_t partial_floats;
    float *red;       // reduction scratch
    float *sig, *gt;  // Sigmoid output and the gradient at its input, [B,3,H,W]
    size_t bytes;
};
constexpr int kRedFloats = 1 << 19;   // >= 5 * 3 * 16 * B and 4 * 128 * B floats: B <= 256 (checked)

GradPlan make_grad_plan(int h, int w, int B, char *base) {
    GradPlan t;
    t.fwd = make_plan(h, w, B, base);
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

}  // namespace
