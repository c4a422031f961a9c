// UNet executor (reference: networks/ThirdPartyNets.py:62-169, eval mode) on the same quad-planar conv kernel:
//   Conv2d(3, padding=1)  -> valid 3x3 correlation on a buffer with a 1-pixel zero border
//   BatchNorm2d (eval)    -> folded into the conv weights / bias at pack time (running stats, eps 1e-5)
//   ReLU                  -> the PReLU epilogue with slope 0
//   cat([skip, up])       -> zero-copy: skip FIRST, up-sampled second (the opposite of UtNet; ThirdPartyNets.py:124)
//   F.pad fix-up (:110-118) for odd sizes -> the 2x2 stride-2 result is written at offset 0 of a destination that is one
//                                            row / column larger; the remainder stays zero (never written)
//   outc + Sigmoid        -> k_final1x1 with the sigmoid flag
// Frames (denoise_image.py:240-267) run through nd_unet_denoise_frame: gather straight into the first layer's input, the same step
// list with the decoder restricted to what the kept centre of a tile depends on (plan_rois), final 1x1 + Sigmoid fused into the stitch.
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "nd_common.h"

namespace {

struct ULayer {
    std::string key;   // conv / convT module path
    std::string bn;    // BatchNorm module path ("" = none)
    int kind, cin, cout;
};

std::vector<ULayer> build_layers() {
    std::vector<ULayer> L;
    auto dconv = [&](const std::string &p, int ci, int co) {
        L.push_back({p + ".0", p + ".1", ND_CONV3, ci, co});
        L.push_back({p + ".3", p + ".4", ND_CONV3, co, co});
    };
    dconv("inc.conv.conv", 3, 64);
    const int dc[4][2] = {{64, 128}, {128, 256}, {256, 512}, {512, 512}};
    for (int n = 0; n < 4; ++n) dconv("down" + std::to_string(n + 1) + ".mpconv.1.conv", dc[n][0], dc[n][1]);
    const int uc[4][2] = {{1024, 256}, {512, 128}, {256, 64}, {128, 64}};
    for (int n = 0; n < 4; ++n) {
        const std::string u = "up" + std::to_string(n + 1);
        L.push_back({u + ".up", "", ND_CONVT2S2, uc[n][0] / 2, uc[n][0] / 2});
        dconv(u + ".conv.conv", uc[n][0], uc[n][1]);
    }
    L.push_back({"outc.conv", "", ND_CONV1, 64, 3});
    return L;
}
const std::vector<ULayer> &layers() {
    static const std::vector<ULayer> L = build_layers();
    return L;
}
std::vector<std::string> build_names() {
    std::vector<std::string> n;
    for (const ULayer &l : layers()) {
        n.push_back(l.key + ".weight");
        n.push_back(l.key + ".bias");
        if (!l.bn.empty())
            for (const char *s : {".weight", ".bias", ".running_mean", ".running_var"}) n.push_back(l.bn + s);
    }
    return n;
}
const std::vector<std::string> &names() {
    static const std::vector<std::string> n = build_names();
    return n;
}
int name_index(const std::string &s) {
    const auto &n = names();
    for (size_t i = 0; i < n.size(); ++i)
        if (n[i] == s) return (int)i;
    return -1;
}

struct Blob {
    std::vector<size_t> off;
    size_t total;
};
Blob blob_layout() {
    Blob b;
    size_t o = 0;
    for (const ULayer &l : layers()) {
        b.off.push_back(o);
        o += l.kind == ND_CONV1 ? (size_t)(3 * l.cin + 3 + 3) / 4 * 4 : nd_packed_floats(l.kind, l.cin, l.cout);
    }
    b.total = o;
    return b;
}

enum UB { XIN, I1, CAT4, Q1, D1, CAT3, Q2, D2, CAT2, Q3, D3, CAT1, Q4, D4, X5, U1A, U1B, U2A, U2B, U3A, U3B, U4A, U4B, NUB };
struct UPlan {
    QpBuf buf[NUB];
    float *split;
    size_t bytes;
};
// B: images the buffers hold (their plane stride); count: images in use (a partial last launch of the frame loop)
UPlan make_plan(int h, int w, int B, char *base, int count = 0) {
    UPlan p;
    size_t off = 0;
    int hs[5] = {h}, ws[5] = {w};
    for (int i = 1; i < 5; ++i) {
        hs[i] = hs[i - 1] / 2;
        ws[i] = ws[i - 1] / 2;
    }
    auto add = [&](UB id, int ch, int lvl, int pad) {
        QpBuf &q = p.buf[id];
        q.planes = id == XIN ? 2 : ch / 4;
        q.B = count > 0 ? count : B;
        q.Hb = hs[lvl] + 2 * pad;
        q.Wb = ws[lvl] + 2 * pad;
        q.pad = pad;
        q.pstride = (long)B * q.Hb * q.Wb;
        q.base = (float *)(base + off);
        off += ((size_t)q.planes * q.pstride + nd_buf_slack(q.Wb)) * 16;
        off = (off + 255) & ~(size_t)255;
    };
    add(XIN, 8, 0, 1); add(I1, 64, 0, 1); add(CAT4, 128, 0, 1);
    add(Q1, 64, 1, 1); add(D1, 128, 1, 1); add(CAT3, 256, 1, 1);
    add(Q2, 128, 2, 1); add(D2, 256, 2, 1); add(CAT2, 512, 2, 1);
    add(Q3, 256, 3, 1); add(D3, 512, 3, 1); add(CAT1, 1024, 3, 1);
    add(Q4, 512, 4, 1); add(D4, 512, 4, 1); add(X5, 512, 4, 0);
    add(U1A, 256, 3, 1); add(U1B, 256, 3, 0);
    add(U2A, 128, 2, 1); add(U2B, 128, 2, 0);
    add(U3A, 64, 1, 1); add(U3B, 64, 1, 0);
    add(U4A, 64, 0, 1); add(U4B, 64, 0, 0);
    p.split = (float *)(base + off);
    off += kSplitScratchBytes;
    p.bytes = off;
    return p;
}

struct UStep {
    int layer;  // index into layers(), -1: pool
    UB src, dst;
    int dst_plane0;  // destination plane offset (channels / 4); for pools: number of planes pooled from plane 0
};
const UStep kSteps[] = {
    {0, XIN, I1, 0},    {1, I1, CAT4, 0},   {-1, CAT4, Q1, 16},  {2, Q1, D1, 0},     {3, D1, CAT3, 0},   {-1, CAT3, Q2, 32},
    {4, Q2, D2, 0},     {5, D2, CAT2, 0},   {-1, CAT2, Q3, 64},  {6, Q3, D3, 0},     {7, D3, CAT1, 0},   {-1, CAT1, Q4, 128},
    {8, Q4, D4, 0},     {9, D4, X5, 0},     {10, X5, CAT1, 128}, {11, CAT1, U1A, 0}, {12, U1A, U1B, 0},  {13, U1B, CAT2, 64},
    {14, CAT2, U2A, 0}, {15, U2A, U2B, 0},  {16, U2B, CAT3, 32}, {17, CAT3, U3A, 0}, {18, U3A, U3B, 0},  {19, U3B, CAT4, 16},
    {20, CAT4, U4A, 0}, {21, U4A, U4B, 0},
};

constexpr int kNumSteps = (int)(sizeof(kSteps) / sizeof(kSteps[0]));
constexpr int kFirstDecoderStep = 14;   // up1.up: everything before it feeds a skip and stays whole

// Regions of the decoder layers when only the centre [crop_h, H - crop_h) x [crop_w, W - crop_w) of the output is kept (the useful
// crop of a tile, denoise_image.py:249-258).  The decoder is a chain (the skip halves of the concat buffers are whole), so one interval
// per axis walks it backwards from the final 1x1: a padding-1 3x3 layer with outputs [lo, hi) reads inputs [lo - 1, hi + 1) clipped
// to the tensor, a 2x2 stride-2 transpose makes output rows [lo, hi) from input rows [lo >> 1, (hi + 1) >> 1) clipped to its input (for
// an odd skip size the last row of the concat half is the F.pad fix-up: zero, never written).  A region lives on the output grid of a
// 3x3 layer and on the input grid of a transpose (ConvDesc::roi_*); rows 0 = the whole layer.  Returns the number of restricted steps.
struct Roi { int r0, c0, rows, cols; };
int plan_rois(const UPlan &pl, int crop_h, int crop_w, Roi *roi) {
    int lo[2][kNumSteps], hi[2][kNumSteps], full[2][kNumSteps];
    const auto &L = layers();
    for (int dim = 0; dim < 2; ++dim) {
        const QpBuf &last = pl.buf[U4B];
        int a = dim ? crop_w : crop_h, b = (dim ? last.Wb : last.Hb) - a;
        for (int i = kNumSteps - 1; i >= kFirstDecoderStep; --i) {
            const UStep &st = kSteps[i];
            const QpBuf &src = pl.buf[st.src], &dst = pl.buf[st.dst];
            const int si = (dim ? src.Wb : src.Hb) - 2 * src.pad;
            if (L[st.layer].kind == ND_CONV3) {
                lo[dim][i] = a;
                hi[dim][i] = b;
                full[dim][i] = (dim ? dst.Wb : dst.Hb) - 2 * dst.pad;
                a = a - 1 < 0 ? 0 : a - 1;
                b = b + 1 > si ? si : b + 1;
            } else {
                a = a >> 1;
                b = (b + 1) >> 1 > si ? si : (b + 1) >> 1;
                lo[dim][i] = a;
                hi[dim][i] = b;
                full[dim][i] = si;
            }
        }
    }
    int n = 0;
    for (int i = 0; i < kNumSteps; ++i) {
        roi[i] = Roi{0, 0, 0, 0};
        if (i < kFirstDecoderStep) continue;
        const bool whole = lo[0][i] == 0 && hi[0][i] == full[0][i] && lo[1][i] == 0 && hi[1][i] == full[1][i];
        if (whole || hi[0][i] <= lo[0][i] || hi[1][i] <= lo[1][i]) continue;
        roi[i] = Roi{lo[0][i], lo[1][i], hi[0][i] - lo[0][i], hi[1][i] - lo[1][i]};
        ++n;
    }
    return n;
}

int check(int h, int w, int batch, int dtype) {
    if (dtype != ND_F32) ND_FAIL(ND_EINVAL, "UNet: unsupported dtype %d", dtype);
    if (h < 16 || w < 16 || batch <= 0) ND_FAIL(ND_EINVAL, "UNet: input %dx%dx%d too small (four 2x2 pools)", batch, h, w);
    return ND_OK;
}

// one step of the stack: the launch both nd_unet_forward and nd_unet_denoise_frame make.  roi: the step's region (null or rows 0: whole)
ConvDesc step_desc(const UStep &st, const UPlan &pl, const float *blob, const Blob &bl, const Roi *roi, bool nosplit) {
    const ULayer &l = layers()[st.layer];
    ConvDesc d;
    d.kind = l.kind;
    d.act = l.kind == ND_CONV3 ? ND_ACT_PRELU : ND_ACT_NONE;   // ReLU = PReLU with slope 0
    d.slope = 0.f;
    d.cin = l.cin;
    d.cout = l.cout;
    d.wpk = blob + bl.off[st.layer];
    d.bias = d.wpk + nd_bias_offset(l.kind, l.cin, l.cout);
    d.in = pl.buf[st.src];
    d.out = pl.buf[st.dst];
    d.out_plane0 = st.dst_plane0;
    d.part = pl.split;
    d.part_bytes = kSplitScratchBytes;
    d.nosplit = nosplit;
    if (roi && roi->rows > 0) {
        d.roi_r0 = roi->r0;
        d.roi_c0 = roi->c0;
        d.roi_rows = roi->rows;
        d.roi_cols = roi->cols;
    }
    return d;
}
int run_step(const UStep &st, const UPlan &pl, const float *blob, const Blob &bl, const Roi *roi, bool nosplit, hipStream_t s) {
    if (st.layer < 0) return nd_launch_maxpool2(pl.buf[st.src], 0, st.dst_plane0, pl.buf[st.dst], s);
    return nd_launch_conv(step_desc(st, pl, blob, bl, roi, nosplit), s);
}
// every restricted layer finds a workgroup shape for its region; else no layer is restricted (a whole-tile layer needs whole-tile
// producers: the rois_supported rule of utnet_net.h)
bool rois_fit(const UPlan &pl, const float *blob, const Blob &bl, const Roi *rois) {
    for (int i = kFirstDecoderStep; i < kNumSteps; ++i)
        if (rois[i].rows > 0 && !nd_conv_roi_fits(step_desc(kSteps[i], pl, blob, bl, &rois[i], false))) return false;
    return true;
}

}  // namespace

extern "C" int nd_unet_num_tensors(void) { return (int)names().size(); }
extern "C" const char *nd_unet_tensor_name(int i) {
    return (i >= 0 && i < (int)names().size()) ? names()[i].c_str() : nullptr;
}
extern "C" size_t nd_unet_packed_bytes(int dtype) { return dtype == ND_F32 ? blob_layout().total * sizeof(float) : 0; }

extern "C" int nd_unet_pack_weights(int dtype, const float *const *tensors, int n_tensors, void *packed_host,
                                    size_t packed_bytes) {
    if (dtype != ND_F32) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: unsupported dtype %d", dtype);
    if (n_tensors != nd_unet_num_tensors()) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: expected %d tensors", nd_unet_num_tensors());
    const Blob bl = blob_layout();
    if (packed_bytes < bl.total * sizeof(float)) ND_FAIL(ND_ENOMEM, "nd_unet_pack_weights: packed buffer too small");
    float *blob = (float *)packed_host;
    memset(blob, 0, bl.total * sizeof(float));
    const auto &L = layers();
    for (size_t i = 0; i < L.size(); ++i) {
        const ULayer &l = L[i];
        const float *w = tensors[name_index(l.key + ".weight")], *b = tensors[name_index(l.key + ".bias")];
        if (!w || !b) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: missing %s", l.key.c_str());
        if (l.kind == ND_CONV1) {
            memcpy(blob + bl.off[i], w, sizeof(float) * 3 * l.cin);
            memcpy(blob + bl.off[i] + 3 * l.cin, b, sizeof(float) * 3);
            continue;
        }
        if (l.bn.empty()) {
            nd_pack_layer(l.kind, l.cin, l.cout, ND_F32, w, b, blob + bl.off[i]);
            continue;
        }
        // fold eval-mode BatchNorm2d: y = (conv + b - mean) * gamma / sqrt(var + eps) + beta
        const float *g = tensors[name_index(l.bn + ".weight")], *be = tensors[name_index(l.bn + ".bias")];
        const float *rm = tensors[name_index(l.bn + ".running_mean")], *rv = tensors[name_index(l.bn + ".running_var")];
        if (!g || !be || !rm || !rv) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: missing BatchNorm tensors of %s", l.bn.c_str());
        std::vector<float> wf((size_t)l.cout * l.cin * 9), bf(l.cout);
        for (int co = 0; co < l.cout; ++co) {
            const float sc = g[co] / sqrtf(rv[co] + 1e-5f);
            for (int k = 0; k < l.cin * 9; ++k) wf[(size_t)co * l.cin * 9 + k] = w[(size_t)co * l.cin * 9 + k] * sc;
            bf[co] = (b[co] - rm[co]) * sc + be[co];
        }
        nd_pack_layer(l.kind, l.cin, l.cout, ND_F32, wf.data(), bf.data(), blob + bl.off[i]);
    }
    return ND_OK;
}

// The same blob from tensors in HBM.  A BatchNorm layer: k_bn_fold writes the per-channel scale and the folded bias, the pack kernel
// multiplies the scale in while it writes the fragments.  The 2 * cout staged floats live in the NEXT layer's region of the blob: layers
// are packed in ascending order on one stream and every pack writes every word of its region, so the staging is overwritten by the
// region's own values before the call's work ends (no allocation, no state shared between calls).
extern "C" int nd_unet_pack_weights_device(int dtype, const float *const *tensors, int n_tensors, void *packed_dev, size_t packed_bytes,
                                           void *stream) {
    if (dtype != ND_F32) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: unsupported dtype %d", dtype);
    if (!tensors || n_tensors != nd_unet_num_tensors())
        ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: expected %d tensors", nd_unet_num_tensors());
    const Blob bl = blob_layout();
    if (!packed_dev || packed_bytes < bl.total * sizeof(float)) ND_FAIL(ND_ENOMEM, "nd_unet_pack_weights_device: packed buffer too small");
    float *blob = (float *)packed_dev;
    hipStream_t s = (hipStream_t)stream;
    const auto &L = layers();
    for (size_t i = 0; i < L.size(); ++i) {
        const ULayer &l = L[i];
        const float *w = tensors[name_index(l.key + ".weight")], *b = tensors[name_index(l.key + ".bias")];
        if (!w || !b) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: missing %s", l.key.c_str());
        if (l.kind == ND_CONV1) {   // [3][cin] weights, 3 biases, zero up to a multiple of 4
            const size_t n = (size_t)3 * l.cin + 3, padded = (n + 3) / 4 * 4;
            ND_HIP(hipMemcpyAsync(blob + bl.off[i], w, sizeof(float) * 3 * l.cin, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemcpyAsync(blob + bl.off[i] + 3 * l.cin, b, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemsetAsync(blob + bl.off[i] + n, 0, sizeof(float) * (padded - n), s));
            continue;
        }
        if (l.bn.empty()) {
            ND_TRY(nd_pack_layer_device(l.kind, l.cin, l.cout, ND_F32, w, b, blob + bl.off[i], s));
            continue;
        }
        const float *g = tensors[name_index(l.bn + ".weight")], *be = tensors[name_index(l.bn + ".bias")];
        const float *rm = tensors[name_index(l.bn + ".running_mean")], *rv = tensors[name_index(l.bn + ".running_var")];
        if (!g || !be || !rm || !rv) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: missing BatchNorm tensors of %s", l.bn.c_str());
        const size_t next_end = i + 2 < L.size() ? bl.off[i + 2] : bl.total;
        if (i + 1 >= L.size() || next_end - bl.off[i + 1] < (size_t)2 * l.cout)
            ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: no staging room behind %s", l.key.c_str());
        float *scale = blob + bl.off[i + 1], *fbias = scale + l.cout;
        ND_TRY(nd_launch_bn_fold(l.cout, b, g, be, rm, rv, scale, fbias, s));
        ND_TRY(nd_pack_layer_device(l.kind, l.cin, l.cout, ND_F32, w, fbias, blob + bl.off[i], s, scale));
    }
    return ND_OK;
}

extern "C" size_t nd_unet_workspace_bytes(int h, int w, int batch, int dtype) {
    if (check(h, w, batch, dtype) != ND_OK) return 0;
    return make_plan(h, w, batch, nullptr).bytes;
}

extern "C" int nd_unet_workspace_init(void *ws, size_t ws_bytes, int h, int w, int batch, int dtype, void *stream) {
    ND_TRY(check(h, w, batch, dtype));
    const size_t need = make_plan(h, w, batch, nullptr).bytes;
    if (!ws || ws_bytes < need) ND_FAIL(ND_ENOMEM, "UNet workspace: %zu B given, %zu B needed", ws_bytes, need);
    ND_HIP(hipMemsetAsync(ws, 0, need, (hipStream_t)stream));
    return ND_OK;
}

// UNet.forward (ThirdPartyNets.py:153-169, find_noise handled by the caller): x [B,3,H,W] -> sigmoid(outc(...)) [B,3,H,W]
extern "C" int nd_unet_forward(int dtype, const void *packed, const float *x, float *y, int batch, int h, int w, void *ws,
                               size_t ws_bytes, void *stream) {
    ND_TRY(check(h, w, batch, dtype));
    if (!packed || !x || !y || !ws) ND_FAIL(ND_EINVAL, "UNet: null pointer");
    UPlan pl = make_plan(h, w, batch, (char *)ws);
    if (ws_bytes < pl.bytes) ND_FAIL(ND_ENOMEM, "UNet workspace: %zu B given, %zu B needed", ws_bytes, pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    const float *blob = (const float *)packed;
    const Blob bl = blob_layout();
    const auto &L = layers();
    ND_TRY(nd_launch_nchw_to_qp(x, 3, pl.buf[XIN], 0, s));
    for (const UStep &st : kSteps) ND_TRY(run_step(st, pl, blob, bl, nullptr, false, s));
    const float *fw = blob + bl.off[L.size() - 1];
    ND_TRY(nd_launch_final1x1(pl.buf[U4B], 64, fw, fw + 3 * 64, 0, y, h, w, s, 1));
    return ND_OK;
}

// ------------------------------------------------------------------ useful-region plan (host only)
extern "C" int nd_unet_num_steps(void) { return kNumSteps; }
extern "C" const char *nd_unet_step_name(int i) {
    if (i < 0 || i >= kNumSteps) return nullptr;
    return kSteps[i].layer < 0 ? "pool" : layers()[kSteps[i].layer].key.c_str();
}
extern "C" int nd_unet_useful_region(int cs, int crop, int step, int *rect) {
    if (cs < 16 || crop < 0 || 2 * crop >= cs || step < 0 || step >= kNumSteps || !rect)
        ND_FAIL(ND_EINVAL, "nd_unet_useful_region: cs %d, crop %d, step %d", cs, crop, step);
    Roi rois[kNumSteps];
    const int n = plan_rois(make_plan(cs, cs, 1, nullptr), crop, crop, rois);
    rect[0] = rois[step].r0;
    rect[1] = rois[step].c0;
    rect[2] = rois[step].rows;
    rect[3] = rois[step].cols;
    return n;
}

// ------------------------------------------------------------------ frame loop (denoise_image.py:240-267)
// gather -> stack -> final 1x1 + Sigmoid + stitch for tiles [tile_begin, tile_begin + tile_count) in ascending launches of at most
// `batch` tiles; no NCHW tile batch exists.  A launch is self-contained: a restricted layer reads only what the restricted layer
// before it wrote in the same launch (plan_rois), and everything the encoder and the skip halves hold is rewritten whole.
extern "C" int nd_unet_denoise_frame(int dtype, int flags, const void *packed, const float *img, float *canvas, int width, int height,
                                     int cs, int ucs, int ol, int tile_begin, int tile_count, int batch, void *ws, size_t ws_bytes,
                                     void *stream, nd_progress_fn progress, void *progress_ctx) {
    ND_TRY(nd_check_flags(flags, false, true));
    ND_TRY(check(cs, cs, batch, dtype));
    int cols = 0, rows = 0, crop = 0;
    ND_TRY(nd_tile_grid(width, height, cs, ucs, ol, &cols, &rows, &crop));
    if (tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > cols * rows)
        ND_FAIL(ND_EINVAL, "nd_unet_denoise_frame: tiles [%d,+%d) outside the grid of %d", tile_begin, tile_count, cols * rows);
    if (!packed || !img || !canvas || !ws) ND_FAIL(ND_EINVAL, "UNet: null pointer");
    const size_t need = make_plan(cs, cs, batch, nullptr).bytes;
    if (ws_bytes < need) ND_FAIL(ND_ENOMEM, "UNet workspace: %zu B given, %zu B needed", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const float *blob = (const float *)packed;
    const Blob bl = blob_layout();
    const float *fw = blob + bl.off[layers().size() - 1];
    const bool nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
    const int end = tile_begin + tile_count;
    int n = 0;
    for (int t0 = tile_begin; t0 < end; t0 += batch, ++n) {
        const int cnt = end - t0 < batch ? end - t0 : batch;
        if (progress) progress(progress_ctx, n, t0, cnt);
        const UPlan pl = make_plan(cs, cs, batch, (char *)ws, cnt);
        Roi rois[kNumSteps];
        const bool useful = !(flags & ND_FLAG_FULL_TILES) && plan_rois(pl, crop, crop, rois) > 0 && rois_fit(pl, blob, bl, rois);
        ND_TRY(nd_launch_gather_pack(img, width, height, cs, ucs, ol, t0, cnt, pl.buf[XIN], s, 1, false));
        for (int i = 0; i < kNumSteps; ++i) ND_TRY(run_step(kSteps[i], pl, blob, bl, useful ? &rois[i] : nullptr, nosplit, s));
        ND_TRY(nd_launch_final1x1_stitch(pl.buf[U4B], 64, fw, fw + 3 * 64, 0, canvas, width, height, cs, ucs, ol, t0, cnt, s, 1,
                                         (flags & ND_FLAG_FIND_NOISE) ? img : nullptr));
    }
    return ND_OK;
}
