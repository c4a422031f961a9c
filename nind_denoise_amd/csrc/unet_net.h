// The UNet stack as data: layers, tensor names, packed-blob layout, activation plan, step list and the useful-region plan.
// Shared by the inference executor (unet.hip) and the autograd halves of both BatchNorm modes (unet_grad.hip); host code only.
#pragma once
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

// Form of every layer of layers() under ND_FLAG_UNET_WINOGRAD (the `form` codes of nd_step_profile), by the rule of utnet_net.h
// (wino_layer / step_form): three-pass F(6x6,3x3) where Cin >= 128, Cout >= 128 and Cin * Cout >= 128 * 256, the fused F(4,3) below,
// direct for the 3-channel first layer and for everything that is no 3x3 layer.  A layer measured slower in its Winograd form at the
// reference tile (20 tiles of 440: DESIGN section 4) is entered as direct here, with the measurement beside it.  step_form() falls
// back to direct where the form does not take the call's geometry.
enum UForm { UFORM_POOL = -1, UFORM_DIRECT = 0, UFORM_F43 = 1, UFORM_WINO3P = 3 };
const signed char kWinoPlan[] = {
    0, 1,      // inc.conv.conv.0 (Cin 3), .3
    1, 1,      // down1: 64 -> 128, 128 -> 128
    3, 3,      // down2
    3, 3,      // down3
    3, 3,      // down4
    0, 3, 3,   // up1.up, up1.conv.conv.0 (1024 -> 256), .3
    0, 3, 1,   // up2.up, up2.conv.conv.0 (512 -> 128), .3 (128 -> 128)
    0, 1, 1,   // up3.up, up3.conv.conv.0 (256 -> 64), .3
    0, 1, 1,   // up4.up, up4.conv.conv.0 (128 -> 64), .3
    0,         // outc.conv
};

struct Blob {
    std::vector<size_t> off;
    std::vector<size_t> woff;   // with ND_FLAG_UNET_WINOGRAD: the layer's Winograd form (F(4,3) or three-pass, kWinoPlan); 0: none
    size_t total;
};
// flags without ND_FLAG_UNET_WINOGRAD: the blob of the default path.  With it, the Winograd forms follow behind: no offset moves
Blob blob_layout(int flags = 0) {
    Blob b;
    size_t o = 0;
    const auto &L = layers();
    for (const ULayer &l : L) {
        b.off.push_back(o);
        o += l.kind == ND_CONV1 ? (size_t)(3 * l.cin + 3 + 3) / 4 * 4 : nd_packed_floats(l.kind, l.cin, l.cout);
    }
    b.woff.assign(L.size(), 0);
    if (flags & ND_FLAG_UNET_WINOGRAD)
        for (size_t i = 0; i < L.size(); ++i) {
            if (kWinoPlan[i] == UFORM_DIRECT) continue;
            b.woff[i] = o;
            o += ((kWinoPlan[i] == UFORM_WINO3P ? nd_wino_packed_floats(kWinoTile, L[i].cin, L[i].cout) : nd_w1d_packed_floats(kW1dTile, L[i].cin, L[i].cout)) + 63) / 64 * 64;
        }
    b.total = o;
    return b;
}

enum UB { XIN, I1, CAT4, Q1, D1, CAT3, Q2, D2, CAT2, Q3, D3, CAT1, Q4, D4, X5, U1A, U1B, U2A, U2B, U3A, U3B, U4A, U4B, NUB };
struct UPlan {
    QpBuf buf[NUB];
    float *split;
    char *wino;          // three-pass V / M scratch (ND_FLAG_UNET_WINOGRAD; else none)
    size_t wino_bytes;
    size_t bytes;
};
size_t wino_scratch(const UPlan &p, int B);   // (behind kSteps)
// B: images the buffers hold (their plane stride); count: images in use (a partial last launch of the frame loop); flags: with
// ND_FLAG_UNET_WINOGRAD the Winograd scratch follows behind everything else
UPlan make_plan(int h, int w, int B, char *base, int count = 0, int flags = 0) {
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
    p.wino = base + off;
    p.wino_bytes = (flags & ND_FLAG_UNET_WINOGRAD) ? wino_scratch(p, B) : 0;
    off += (p.wino_bytes + 255) & ~(size_t)255;
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
// V / M scratch of the largest three-pass layer at min(B, kWinoChunk) images (a larger launch runs in chunks: run_step)
size_t wino_scratch(const UPlan &p, int B) {
    size_t bytes = 0;
    for (const UStep &st : kSteps) {
        if (st.layer < 0 || kWinoPlan[st.layer] != UFORM_WINO3P) continue;
        QpBuf v = p.buf[st.src];
        v.B = B < kWinoChunk ? B : kWinoChunk;
        const size_t need = nd_wino_scratch_bytes(kWinoTile, v, layers()[st.layer].cin, layers()[st.layer].cout);
        if (need > bytes) bytes = need;
    }
    return bytes;
}
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

// the kernel family that runs step `st` of a call with `flags` on plan pl (roi: the step's region, null or rows 0: the whole layer)
UForm step_form(const UStep &st, const UPlan &pl, int flags, const Roi *roi) {
    if (st.layer < 0) return UFORM_POOL;
    const ULayer &l = layers()[st.layer];
    if (l.kind != ND_CONV3 || !(flags & ND_FLAG_UNET_WINOGRAD) || (flags & ND_FLAG_DIRECT_CONV)) return UFORM_DIRECT;
    const QpBuf &in = pl.buf[st.src];
    switch (kWinoPlan[st.layer]) {
        case UFORM_WINO3P: return l.cin % 16 == 0 && l.cout % 4 == 0 ? UFORM_WINO3P : UFORM_DIRECT;   // (takes a region: unpooled F(6x6))
        case UFORM_F43:
            if (nd_f43_w2d(in, l.cout, false, flags)) return UFORM_F43;            // conv_w2d: any row width, takes a region
            if (roi && roi->rows > 0) return UFORM_DIRECT;                         // conv_w1d takes none
            return nd_w1d_fits(kW1dTile, in) ? UFORM_F43 : UFORM_DIRECT;
        default: return UFORM_DIRECT;
    }
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
// flags: nd_flags of the call (ND_FLAG_NO_SPLITK; ND_FLAG_UNET_WINOGRAD: the blob and the plan were made with it).  ev2, tiles
// (profiling, nullable): the events and the tile count of a three-pass layer, as in nd_launch_conv_wino / nd_wino_launch_tiles
int run_step(const UStep &st, const UPlan &pl, const float *blob, const Blob &bl, const Roi *roi, int flags, hipStream_t s,
             hipEvent_t *ev2 = nullptr, long *tiles = nullptr) {
    if (st.layer < 0) return nd_launch_maxpool2(pl.buf[st.src], 0, st.dst_plane0, pl.buf[st.dst], s);
    ConvDesc d = step_desc(st, pl, blob, bl, roi, (flags & ND_FLAG_NO_SPLITK) != 0);
    const UForm form = step_form(st, pl, flags, roi);
    if (form == UFORM_DIRECT) return nd_launch_conv(d, s);
    if (!bl.woff[st.layer]) ND_FAIL(ND_EINVAL, "UNet: no Winograd form of %s in the blob", layers()[st.layer].key.c_str());
    d.wpk = blob + bl.woff[st.layer];
    if (form == UFORM_F43) {
        d.bias = d.wpk + nd_bias_offset(d.kind, d.cin, d.cout, ND_F32, kW1dTile);
        return nd_launch_conv_f43(d, flags, s);
    }
    // three-pass form, kWinoChunk images per pass (views of the same buffers)
    d.bias = nullptr;
    d.tile_wino = (flags & ND_FLAG_TILE_WINO) != 0;
    const int nimg = d.in.B;
    for (int b0 = 0; b0 < nimg; b0 += kWinoChunk) {
        ConvDesc c = d;
        c.in.B = c.out.B = nimg - b0 < kWinoChunk ? nimg - b0 : kWinoChunk;
        c.in.base = d.in.base + (size_t)b0 * d.in.Hb * d.in.Wb * 4;
        c.out.base = d.out.base + (size_t)b0 * d.out.Hb * d.out.Wb * 4;
        ND_TRY(nd_launch_conv_wino(kWinoTile, c, pl.wino, pl.wino_bytes, s, nimg <= kWinoChunk ? ev2 : nullptr));
        if (tiles) *tiles += nd_wino_launch_tiles(kWinoTile, c);
    }
    return ND_OK;
}
// every restricted layer finds a workgroup shape for its region in the form that will run it (the Winograd forms that step_form
// returns for a restricted step take any region); else no layer is restricted (a whole-tile layer needs whole-tile producers: the
// rois_supported rule of utnet_net.h)
bool rois_fit(const UPlan &pl, const float *blob, const Blob &bl, const Roi *rois, int flags) {
    for (int i = kFirstDecoderStep; i < kNumSteps; ++i)
        if (rois[i].rows > 0 && step_form(kSteps[i], pl, flags, &rois[i]) == UFORM_DIRECT &&
            !nd_conv_roi_fits(step_desc(kSteps[i], pl, blob, bl, &rois[i], false)))
            return false;
    return true;
}

}  // namespace
