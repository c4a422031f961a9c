// UtNet description shared by the inference executor (utnet.hip) and the training step (utnet_train.hip):
// layer table, state-dict tensor order, packed-blob layout, activation-buffer plan and the forward launch sequence.
// Everything lives in an unnamed namespace: each translation unit gets its own copy.
#pragma once
#include <string.h>

#include <string>
#include <vector>

#include "nd_common.h"

namespace {

struct LayerSpec {
    const char *key;
    int kind;
    int cin_mul, cout_mul;  // channels = mul * funit (cin_mul 0 -> 3 input channels, cout_mul 0 -> 3 output channels)
    int prelu;              // index into the slope table, -1: no activation
};

// forward order; prelu indices follow the state-dict order of the activation modules
const LayerSpec kLayers[] = {
    {"convs1.0", ND_CONV3, 0, 1, 0},    {"convs1.2", ND_CONV3, 1, 1, 1},    {"convs2.0", ND_CONV3, 1, 2, 2},
    {"convs2.2", ND_CONV3, 2, 2, 3},    {"convs3.0", ND_CONV3, 2, 4, 4},    {"convs3.2", ND_CONV3, 4, 4, 5},
    {"convs4.0", ND_CONV3, 4, 8, 6},    {"convs4.2", ND_CONV3, 8, 8, 7},    {"bottom.0", ND_CONV3, 8, 16, 8},
    {"bottom.2", ND_CONVT3, 16, 16, 9}, {"up1", ND_CONVT2S2, 16, 8, -1},    {"tconvs1.0", ND_CONVT3, 16, 8, 10},
    {"tconvs1.2", ND_CONVT3, 8, 8, 11}, {"up2", ND_CONVT2S2, 8, 4, -1},     {"tconvs2.0", ND_CONVT3, 8, 4, 12},
    {"tconvs2.2", ND_CONVT3, 4, 4, 13}, {"up3", ND_CONVT2S2, 4, 2, -1},     {"tconvs3.0", ND_CONVT3, 4, 2, 14},
    {"tconvs3.2", ND_CONVT3, 2, 2, 15}, {"up4", ND_CONVT2S2, 2, 1, -1},     {"tconvs4.0", ND_CONVT3, 2, 1, 16},
    {"tconvs4.2", ND_CONVT3, 1, 1, 17}, {"tconvs4.4", ND_CONV1, 1, 0, -1},
};
constexpr int kNumLayers = (int)(sizeof(kLayers) / sizeof(kLayers[0]));
constexpr int kNumSlopes = 18;
constexpr int kHeaderFloats = 32;  // slope table (18 used)

// state-dict order of the reference module (UtNet.py:27-88): weight, bias of every layer, PReLU weights interleaved
std::vector<std::string> build_tensor_names() {
    std::vector<std::string> n;
    auto seq = [&](const std::string &p, int n_act_pairs, bool final1x1) {
        for (int k = 0; k < n_act_pairs; ++k) {
            n.push_back(p + "." + std::to_string(2 * k) + ".weight");
            n.push_back(p + "." + std::to_string(2 * k) + ".bias");
            n.push_back(p + "." + std::to_string(2 * k + 1) + ".weight");
        }
        if (final1x1) {
            n.push_back(p + ".4.weight");
            n.push_back(p + ".4.bias");
        }
    };
    for (int i = 1; i <= 4; ++i) seq("convs" + std::to_string(i), 2, false);
    seq("bottom", 2, false);
    for (int i = 1; i <= 4; ++i) {
        n.push_back("up" + std::to_string(i) + ".weight");
        n.push_back("up" + std::to_string(i) + ".bias");
        seq("tconvs" + std::to_string(i), 2, i == 4);
    }
    return n;
}
const std::vector<std::string> &tensor_names() {
    static const std::vector<std::string> n = build_tensor_names();
    return n;
}
int tensor_index(const std::string &name) {
    const auto &n = tensor_names();
    for (size_t i = 0; i < n.size(); ++i)
        if (n[i] == name) return (int)i;
    return -1;
}

inline int lcin(const LayerSpec &l, int f) { return l.cin_mul ? l.cin_mul * f : 3; }
inline int lcout(const LayerSpec &l, int f) { return l.cout_mul ? l.cout_mul * f : 3; }

// fp32 inference form of the 3x3 layers, chosen from measurements on the UtNet(64) shapes at 256 tiles per launch:
//   Cin * Cout >= 128 * 256 : three-pass Winograd F(6x6, 3x3) (winograd.hip; F(4x4) until late round 2): 1.65x (128 -> 256) ... 2.6x (1024 -> 512) the direct kernel
//   below                   : 1-D Winograd F(4, 3) along x inside the implicit-GEMM kernel (conv_w1d.hip): 1.43 - 1.5x the direct
//                             kernel; the three-pass form is HBM-bound on its transform passes there (64 -> 64: 0.87x, 128 -> 128: 1.4x)
constexpr int kWinoTile = 6;   // F(6x6,3x3): 64 MACs per 36 outputs and 1.78x |X| of transform traffic (F(4x4): 36 per 16, 2.25x); every
                             // three-pass layer of UtNet(64) measured 1 - 27 % faster than with F(4x4) at cs = 264 (bottom.2, a 13x13 output, the least)
constexpr int kW1dTile = 4;
constexpr int kWinoChunk = 256;  // images per three-pass Winograd pass: bounds the V / M scratch (60 MB per 264-pixel tile for the
                                 // largest layer); G24 at 256 tiles per launch: 46.1 MP/s with 64, 47.4 with 128, 47.8 with 256
inline bool wino_layer(const LayerSpec &l, int f, int dt) {
    return dt == ND_F32 && (l.kind == ND_CONV3 || l.kind == ND_CONVT3) && l.cin_mul * f >= 128 && l.cout_mul * f >= 128 &&
           ((long)l.cin_mul * f * l.cout_mul * f >= 128L * 256 || l.kind == ND_CONVT3) && (l.cin_mul * f) % 16 == 0;
    // (128 -> 128: the transposed layer tconvs3.2 is 0.47 ms faster in the three-pass form at 256 tiles of 264, the valid layer
    //  convs2.2 -- which also writes its pooled tensor -- 0.16 ms slower)
}

// float offsets of every layer inside the packed blob
struct BlobLayout {
    size_t off[kNumLayers];
    size_t woff[kNumLayers];   // three-pass Winograd F(6x6,3x3) form of the layer (0: none)
    size_t w1off[kNumLayers];  // 1-D F(4,3) form fused into the implicit-GEMM kernel (conv_w1d.hip): the other fp32 3x3 layers
    size_t w1off2[kNumLayers]; // ... and its F(2,3) form, for rows whose stage images do not fit the LDS with 18 weight planes
    size_t total;
};
// train: the layout of the training step's forward blob -- every 3x3 region can hold either the direct or the fused 1-D
// Winograd packing (the step picks per layer), no separate Winograd regions; else the inference blob with its Winograd regions
inline size_t layer_floats(const LayerSpec &l, int f, int dt, bool train) {
    const size_t direct = nd_packed_floats(l.kind, lcin(l, f), lcout(l, f), dt);
    if (!train || dt != ND_F32 || (l.kind != ND_CONV3 && l.kind != ND_CONVT3)) return direct;
    const size_t w1 = nd_w1d_packed_floats(kW1dTile, lcin(l, f), lcout(l, f));
    return w1 > direct ? w1 : direct;
}
BlobLayout blob_layout(int f, int dt, bool train = false) {
    BlobLayout b;
    size_t o = kHeaderFloats;
    for (int i = 0; i < kNumLayers; ++i) {
        b.off[i] = o;
        const LayerSpec &l = kLayers[i];
        if (i == kNumLayers - 1)
            o += ((size_t)3 * lcin(l, f) + 3 + 3) / 4 * 4;  // raw [3][cin] + bias[3] for the VALU 1x1 kernel
        else
            o += layer_floats(l, f, dt, train);
    }
    for (int i = 0; i < kNumLayers; ++i) {
        b.woff[i] = 0;
        if (!train && wino_layer(kLayers[i], f, dt)) {
            b.woff[i] = o;
            o += (nd_wino_packed_floats(kWinoTile, lcin(kLayers[i], f), lcout(kLayers[i], f)) + 63) / 64 * 64;
        }
        b.w1off[i] = b.w1off2[i] = 0;
        const LayerSpec &l = kLayers[i];
        if (!train && dt == ND_F32 && (l.kind == ND_CONV3 || l.kind == ND_CONVT3) && !b.woff[i]) {
            b.w1off[i] = o;
            o += (nd_w1d_packed_floats(kW1dTile, lcin(l, f), lcout(l, f)) + 63) / 64 * 64;
            b.w1off2[i] = o;
            o += (nd_w1d_packed_floats(2, lcin(l, f), lcout(l, f)) + 63) / 64 * 64;
        }
    }
    b.total = o;
    return b;
}

bool valid_cs(int cs) { return cs >= 104 && (cs - 56) % 16 == 0; }

int check_funit(int funit, int dtype) {
    if (dtype < ND_F32 || dtype > ND_F16) ND_FAIL(ND_EINVAL, "UtNet: unsupported dtype %d", dtype);
    const int q = 2 * nd_cpp(dtype);   // every conv input must be whole K blocks: 8 (fp32) / 16 (bf16, fp16) channels
    if (funit < q || funit % q) ND_FAIL(ND_EINVAL, "UtNet: funit=%d must be a positive multiple of %d for dtype %d", funit, q, dtype);
    return ND_OK;
}

int check_net(int funit, int h, int w, int batch, int dtype) {
    ND_TRY(check_funit(funit, dtype));
    for (int cs : {h, w})
        if (!valid_cs(cs))
            ND_FAIL(ND_EINVAL, "UtNet: tile size %d is not of the form 16k+56 (104, 120, ..., 248, 264, ..., 504, 520); "
                               "the reference network rejects it too (sizes of the skip concats do not match)", cs);
    if (batch <= 0) ND_FAIL(ND_EINVAL, "UtNet: batch=%d", batch);
    return ND_OK;
}

// ---------------------------------------------------------------- workspace plan
enum Buf { X0, A1, CAT4, P1, A2, CAT3, P2, A3, CAT2, P3, A4, CAT1, P4, BT0, BT1, T1A, T1B, T2A, T2B, T3A, T3B, T4A, T4B, NBUF };

struct Step {
    int layer;  // index into kLayers, or -1 for a pool
    Buf src, dst;
    int dst_plane0_mul;  // destination plane offset = mul * funit / 4
};
// the conv stack between the input pack and the final 1x1 (UtNet.py:99-107)
constexpr int kNumSteps = 26;
const Step kSteps[kNumSteps] = {
    {0, X0, A1, 0},     {1, A1, CAT4, 1},   {-1, CAT4, P1, 1},  {2, P1, A2, 0},    {3, A2, CAT3, 2},  {-1, CAT3, P2, 2},
    {4, P2, A3, 0},     {5, A3, CAT2, 4},   {-1, CAT2, P3, 4},  {6, P3, A4, 0},    {7, A4, CAT1, 8},  {-1, CAT1, P4, 8},
    {8, P4, BT0, 0},    {9, BT0, BT1, 0},   {10, BT1, CAT1, 0}, {11, CAT1, T1A, 0}, {12, T1A, T1B, 0}, {13, T1B, CAT2, 0},
    {14, CAT2, T2A, 0}, {15, T2A, T2B, 0},  {16, T2B, CAT3, 0}, {17, CAT3, T3A, 0}, {18, T3A, T3B, 0}, {19, T3B, CAT4, 0},
    {20, CAT4, T4A, 0}, {21, T4A, T4B, 0},
};

struct Plan {
    QpBuf buf[NBUF];
    float *split;   // split-K scratch shared by every conv launch of the stream (kSplitScratchBytes)
    char *wino;     // Winograd V / M scratch (largest layer at kWinoChunk images)
    size_t wino_bytes;
    size_t bytes;
};

// cap = batch the workspace was sized for; nimg = images in use (<= cap)
Plan make_plan(int f, int ch_, int cw_, int cap, int nimg, char *base, int dt) {
    Plan p;
    size_t off = 0;
    // `size` is the extent of the tensor for a SQUARE cs x cs input; the other dimension follows the same chain
    auto chain = [](int cs, int which) {
        const int l1 = cs, l2 = cs / 2 - 4, l3 = l2 / 2 - 4, l4 = l3 / 2 - 4, p4 = l4 / 2;
        const int v[] = {cs + 4, cs + 2, l1, l1 / 2, l1 / 2 - 2, l2, l2 / 2, l2 / 2 - 2, l3, l3 / 2, l3 / 2 - 2, l4, p4,
                         p4 - 2, p4, l4 + 2, l4 + 4, l3 + 2, l3 + 4, l2 + 2, l2 + 4, l1 + 2, l1 + 4};
        return v[which];
    };
    auto add = [&](Buf id, int ch, int /*size*/, int pad) {
        QpBuf &q = p.buf[id];
        q.planes = (ch + nd_cpp(dt) - 1) / nd_cpp(dt);
        if (id == X0) q.planes = 2;   // one K block: plane 0 = (r,g,b,0..), plane 1 = zeros
        q.dt = dt;
        q.B = nimg;
        q.Hb = chain(ch_, (int)id) + 2 * pad;
        q.Wb = chain(cw_, (int)id) + 2 * pad;
        q.pad = pad;
        q.pstride = (long)cap * q.Hb * q.Wb;
        q.base = (float *)(base + off);
        const size_t slack = nd_buf_slack(q.Wb);   // reads past the last plane (halo of the last tile / strip)
        off += ((size_t)q.planes * q.pstride + slack) * 16;
        off = (off + 255) & ~(size_t)255;
    };
    const int cs = ch_;
    const int l1 = cs, l2 = cs / 2 - 4, l3 = l2 / 2 - 4, l4 = l3 / 2 - 4, p4 = l4 / 2;
    add(X0, 8, cs + 4, 0);
    add(A1, f, cs + 2, 0);
    add(CAT4, 2 * f, l1, 2);
    add(P1, f, l1 / 2, 0);
    add(A2, 2 * f, l1 / 2 - 2, 0);
    add(CAT3, 4 * f, l2, 2);
    add(P2, 2 * f, l2 / 2, 0);
    add(A3, 4 * f, l2 / 2 - 2, 0);
    add(CAT2, 8 * f, l3, 2);
    add(P3, 4 * f, l3 / 2, 0);
    add(A4, 8 * f, l3 / 2 - 2, 0);
    add(CAT1, 16 * f, l4, 2);
    add(P4, 8 * f, p4, 0);
    add(BT0, 16 * f, p4 - 2, 2);
    add(BT1, 16 * f, p4, 0);
    add(T1A, 8 * f, l4 + 2, 2);
    add(T1B, 8 * f, l4 + 4, 0);
    add(T2A, 4 * f, l3 + 2, 2);
    add(T2B, 4 * f, l3 + 4, 0);
    add(T3A, 2 * f, l2 + 2, 2);
    add(T3B, 2 * f, l2 + 4, 0);
    add(T4A, f, l1 + 2, 2);
    add(T4B, f, l1 + 4, 0);
    p.split = (float *)(base + off);
    off += kSplitScratchBytes;
    p.wino = base + off;
    p.wino_bytes = 0;
    for (const Step &st : kSteps) {
        if (st.layer < 0 || !wino_layer(kLayers[st.layer], f, dt)) continue;
        QpBuf v = p.buf[st.src];
        v.B = cap < kWinoChunk ? cap : kWinoChunk;
        const size_t need = nd_wino_scratch_bytes(kWinoTile, v, lcin(kLayers[st.layer], f), lcout(kLayers[st.layer], f));
        if (need > p.wino_bytes) p.wino_bytes = need;
    }
    off += (p.wino_bytes + 255) & ~(size_t)255;
    p.bytes = off;
    return p;
}

// which kernel family runs step `st` of the stack (pl = the plan of the call: the fused 1-D form needs the row's LDS images to fit;
// train_w1: null for inference, else the training forward's per-layer choice, 1 = fused 1-D Winograd)
enum Form { FORM_POOL = -1, FORM_DIRECT = 0, FORM_W1D4 = 1, FORM_W1D2 = 2, FORM_WINO3P = 3 };
inline Form step_form(const Step &st, int f, int dt, int flags, const Plan &pl, const BlobLayout &bl,
                      const unsigned char *train_w1 = nullptr) {
    if (st.layer < 0) return FORM_POOL;
    const LayerSpec &l = kLayers[st.layer];
    if (l.kind != ND_CONV3 && l.kind != ND_CONVT3) return FORM_DIRECT;
    if (train_w1) return train_w1[st.layer] ? FORM_W1D4 : FORM_DIRECT;
    if (flags & ND_FLAG_DIRECT_CONV) return FORM_DIRECT;
    if (bl.w1off[st.layer]) {
        if (nd_f43_w2d(pl.buf[st.src], lcout(l, f), false, flags)) return FORM_W1D4;   // conv_w2d: any row width
        if (nd_w1d_fits(kW1dTile, pl.buf[st.src])) return FORM_W1D4;
        if (nd_w1d_fits(2, pl.buf[st.src])) return FORM_W1D2;
        return FORM_DIRECT;
    }
    return bl.woff[st.layer] ? FORM_WINO3P : FORM_DIRECT;
}

// Regions of interest of the decoder layers when only the centre [crop_h, H - crop_h) x [crop_w, W - crop_w) of the network
// output is used -- the fused denoise loop (denoise_image.py:249-258 crops every tile to its useful part before it is added to
// the canvas: pixels outside [pad, cs - pad) never reach it).  Walking the stack backwards from the final 1x1: a transposed 3x3
// layer needs input rows [lo - 2, hi) for output rows [lo, hi), a 2x2 stride-2 transpose input rows [lo / 2, (hi + 1) / 2).  With
// cs = 264 / ucs = 200 the last decoder level computes 204^2 of its 266^2 pixels, the level below 104^2 of 130^2; from the
// third level down everything is needed.  The encoder always runs whole (its pooled outputs feed every level).
struct Roi { int r0, c0, rows, cols; };
inline bool plan_rois(const Plan &pl, int crop_h, int crop_w, Roi *roi) {
    for (int i = 0; i < kNumSteps; ++i) roi[i] = Roi{0, 0, 0, 0};
    if (crop_h <= 0 && crop_w <= 0) return false;
    bool any = false;
    int lo[2][NBUF], hi[2][NBUF];
    for (int dim = 0; dim < 2; ++dim) {
        for (int b = 0; b < NBUF; ++b) {
            lo[dim][b] = 1 << 30;
            hi[dim][b] = -1;
        }
        const QpBuf &last = pl.buf[T4B];
        const int size = (dim ? last.Wb : last.Hb) - 2 * last.pad, crop = dim ? crop_w : crop_h;
        lo[dim][T4B] = crop + 2;          // final 1x1 + ZeroPad2d(-2): output pixel y is T4B pixel y + 2
        hi[dim][T4B] = size - 2 - crop;
        for (int i = kNumSteps - 1; i >= 0; --i) {
            const Step &st = kSteps[i];
            if (st.layer < 0) continue;
            const int kind = kLayers[st.layer].kind;
            if (kind != ND_CONVT3 && kind != ND_CONVT2S2) continue;
            if (hi[dim][st.dst] < 0) continue;   // nobody restricted this output
            const QpBuf &src = pl.buf[st.src];
            const int si = (dim ? src.Wb : src.Hb) - 2 * src.pad;
            int a = lo[dim][st.dst], b = hi[dim][st.dst];
            if (kind == ND_CONVT3) {
                a = a - 2 < 0 ? 0 : a - 2;
                b = b > si ? si : b;
            } else {
                a = a >> 1;
                b = (b + 1) >> 1;
                b = b > si ? si : b;
            }
            if (a < lo[dim][st.src]) lo[dim][st.src] = a;
            if (b > hi[dim][st.src]) hi[dim][st.src] = b;
        }
    }
    for (int i = 0; i < kNumSteps; ++i) {
        const Step &st = kSteps[i];
        if (st.layer < 0) continue;
        const int kind = kLayers[st.layer].kind;
        if (kind != ND_CONVT3 && kind != ND_CONVT2S2) continue;
        // the region lives on the layer's output grid (3x3) or input grid (2x2 stride-2)
        const Buf b = kind == ND_CONVT3 ? st.dst : st.src;
        const QpBuf &q = pl.buf[b];
        const int H = q.Hb - 2 * q.pad, W = q.Wb - 2 * q.pad;
        int r0 = 0, r1 = H, c0 = 0, c1 = W;
        if (kind == ND_CONVT3) {
            if (hi[0][b] >= 0) { r0 = lo[0][b]; r1 = hi[0][b]; }
            if (hi[1][b] >= 0) { c0 = lo[1][b]; c1 = hi[1][b]; }
        } else {
            if (hi[0][st.dst] >= 0) { r0 = lo[0][st.dst] >> 1; r1 = (hi[0][st.dst] + 1) >> 1; }
            if (hi[1][st.dst] >= 0) { c0 = lo[1][st.dst] >> 1; c1 = (hi[1][st.dst] + 1) >> 1; }
        }
        r0 = r0 < 0 ? 0 : r0; c0 = c0 < 0 ? 0 : c0;
        r1 = r1 > H ? H : r1; c1 = c1 > W ? W : c1;
        if (r0 == 0 && c0 == 0 && r1 == H && c1 == W) continue;
        if (r1 <= r0 || c1 <= c0) continue;
        roi[i] = Roi{r0, c0, r1 - r0, c1 - c0};
        any = true;
    }
    return any;
}

// every restricted layer must run in a kernel that takes a region (conv_qp, conv_w2d, three-pass F(6x6)): one that does not would
// compute its whole output from a producer that only wrote its region
inline bool rois_supported(int f, int dt, int flags, const Plan &pl, const BlobLayout &bl, const Roi *rois) {
    for (int i = 0; i < kNumSteps; ++i) {
        if (rois[i].rows <= 0) continue;
        const Form form = step_form(kSteps[i], f, dt, flags, pl, bl);
        if (form == FORM_DIRECT) {
            // conv_qp walks linear pixel ranges: a region much narrower than its buffer may not fit any stage image -- then no
            // layer is restricted (a whole-tile layer needs whole-tile producers)
            const LayerSpec &l = kLayers[kSteps[i].layer];
            ConvDesc d;
            d.kind = l.kind;
            d.cin = lcin(l, f);
            d.cout = lcout(l, f);
            d.in = pl.buf[kSteps[i].src];
            d.out = pl.buf[kSteps[i].dst];
            d.roi_r0 = rois[i].r0;
            d.roi_c0 = rois[i].c0;
            d.roi_rows = rois[i].rows;
            d.roi_cols = rois[i].cols;
            if (!nd_conv_roi_fits(d)) return false;
            continue;
        }
        if (form == FORM_WINO3P) continue;
        if (form == FORM_W1D4 && !(flags & ND_FLAG_W1D_REGS)) continue;
        return false;
    }
    return true;
}

// a step whose upper input planes come from a second source (ConvDesc::in2): the fused loop's skip halves, read from the band
struct StepSrc2 {
    int step = -1;         // index into kSteps (-1: unused)
    QpBuf buf = {};        // the band tensor
    int plane0 = 0, from = 0;   // first plane of buf; input plane of the step at which buf takes over
    const int *origin = nullptr;   // per image of the launch (HBM)
    long origin_max = 0;
    // the skip half is folded out of the step (launch_skip_fold): buf holds its product P, the step's addend source (ConvDesc::add),
    // and the step runs on the K blocks of its input planes below `from` alone
    bool addend = false;
};
// the kernel a step runs in takes a second input source -- and, all the same kernels, an addend source with a K-block sub-range
// of the weights: conv_w2d and the three-pass F(6x6) form
inline bool form_takes_src2(const Step &st, Form form, int f, int flags, const Plan &pl) {
    if (form == FORM_WINO3P) return kWinoTile == 6;
    return form == FORM_W1D4 && nd_f43_w2d(pl.buf[st.src], lcout(kLayers[st.layer], f), false, flags);
}

// what one run_stack call does besides the whole inference stack: a call site sets only the members that differ
struct StackOpts {
    int flags = 0;                     // nd_flags of the call (ND_FLAG_NO_SPLITK: every tile whole; ND_FLAG_DIRECT_CONV: no Winograd form)
    const Roi *rois = nullptr;         // per step: the region the layer computes (plan_rois; rows 0: the whole layer)
    int step_begin = 0, step_end = kNumSteps;   // the steps [step_begin, step_end) of kSteps
    const StepSrc2 *src2 = nullptr;    // nsrc2 steps with a second input source
    int nsrc2 = 0;
    hipEvent_t *ev = nullptr;          // profiling: kNumSteps+1 events, ev[i] recorded before step i, ev[kNumSteps] after the last one
    hipEvent_t *ev_x = nullptr;        // profiling, with ev: 2 events per step, recorded after the input transform and after the
                                       // GEMMs of a three-pass layer
    long *wino_tiles = nullptr;        // out (profiling), kNumSteps entries: the F(6x6) tiles the launches of a three-pass step ran
                                       // (nd_wino_launch_tiles of every chunk: per image, or a mosaic's); the caller zeroes them
    // training forward (both set): the blob of blob_layout(f, dt, true)
    const QpBuf *pre = nullptr;                // kNumSlopes compact buffers that receive acc + bias of every activated layer
    const unsigned char *train_w1 = nullptr;   // per layer, 1 = the layer's blob region holds the fused 1-D Winograd packing
};
int run_stack(int f, int act, int dt, const float *blob, const Plan &pl, hipStream_t s, const StackOpts &o) {
    const QpBuf *const pre = o.pre;
    const int flags = o.flags, step_begin = o.step_begin, step_end = o.step_end;
    const BlobLayout bl = blob_layout(f, dt, pre != nullptr);
    const int cpp = nd_cpp(dt);
    int si = step_begin;
    bool pool_done = false;   // the previous layer wrote the pooled tensor itself
    QpBuf pool_view;
    for (int k = step_begin; k < step_end; ++k) {
        const Step &st = kSteps[k];
        if (o.ev) ND_HIP(hipEventRecord(o.ev[si], s));
        const int this_step = si++;
        if (st.layer < 0) {
            if (pool_done) {
                pool_done = false;
                continue;
            }
            // pool reads the skip half of the concat buffer: planes [mul*f/4, 2*mul*f/4)
            ND_TRY(nd_launch_maxpool2(pl.buf[st.src], st.dst_plane0_mul * f / cpp, st.dst_plane0_mul * f / cpp, pl.buf[st.dst], s));
            continue;
        }
        const LayerSpec &l = kLayers[st.layer];
        ConvDesc d;
        d.kind = l.kind;
        d.act = l.prelu >= 0 ? act : ND_ACT_NONE;
        d.slope = 0.25f;
        d.slope_dev = (l.prelu >= 0 && act == ND_ACT_PRELU) ? blob + l.prelu : nullptr;
        if (pre && l.prelu >= 0) {
            d.pre = pre[l.prelu].base;
            d.pre_plane = pre[l.prelu].np();
        }
        const int cin = lcin(l, f);
        d.cin = cin;
        d.cout = lcout(l, f);
        d.wpk = blob + bl.off[st.layer];
        d.bias = d.wpk + nd_bias_offset(l.kind, d.cin, d.cout, dt);
        d.in = pl.buf[st.src];
        d.out = pl.buf[st.dst];
        d.out_plane0 = st.dst_plane0_mul * f / cpp;
        d.part = pl.split;
        d.part_bytes = kSplitScratchBytes;
        d.nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
        d.tile_wino = (flags & ND_FLAG_TILE_WINO) != 0;
        const Form form = step_form(st, f, dt, flags, pl, bl, o.train_w1);
        if (o.rois && o.rois[this_step].rows > 0) {
            d.roi_r0 = o.rois[this_step].r0;
            d.roi_c0 = o.rois[this_step].c0;
            d.roi_rows = o.rois[this_step].rows;
            d.roi_cols = o.rois[this_step].cols;
        }
        for (int i = 0; i < o.nsrc2; ++i)
            if (o.src2[i].step == k && o.src2[i].addend) {
                d.add = o.src2[i].buf;
                d.add_plane0 = o.src2[i].plane0;
                d.add_origin = o.src2[i].origin;
                d.add_origin_max = o.src2[i].origin_max;
                d.w_kb = nd_kblocks(cin, dt);
                d.cin = o.src2[i].from * cpp;
            } else if (o.src2[i].step == k) {
                d.in2 = o.src2[i].buf;
                d.in2_plane0 = o.src2[i].plane0;
                d.in2_from = o.src2[i].from;
                d.in2_origin = o.src2[i].origin;
                d.in2_origin_max = o.src2[i].origin_max;
            }
        // MaxPool2d(2) fused into the producing layer's epilogue where its kernel can (conv_w2d, three-pass output transform):
        // the pool kernel re-read the whole skip tensor from HBM (2.4 % of the fp32 conv stack)
        const bool next_is_pool = this_step + 1 < step_end && kSteps[this_step + 1].layer < 0;
        const bool w2d = form == FORM_W1D4 && nd_f43_w2d(d.in, d.cout, pre != nullptr, flags);
        if (next_is_pool && !pre && !(flags & ND_FLAG_UNFUSED_POOL)) {
            pool_view = pl.buf[kSteps[this_step + 1].dst];
            d.pool = &pool_view;
            // fp32: conv_w2d and the three-pass output transform pool; 16-bit storage: conv_qp over 2-row bands of pixels, where a
            // workgroup shape fits the longer stage image
            pool_done = w2d || form == FORM_WINO3P || (form == FORM_DIRECT && dt != ND_F32 && nd_conv_pool_fits(d));
            if (!pool_done) d.pool = nullptr;
        }
        if (form == FORM_W1D4 || form == FORM_W1D2) {
            // narrow layer: 1-D Winograd along x inside the implicit-GEMM kernel; F(4,3), or F(2,3) on rows too wide for it
            const int T = form == FORM_W1D4 ? kW1dTile : 2;
            if (!pre) d.wpk = blob + (T == kW1dTile ? bl.w1off[st.layer] : bl.w1off2[st.layer]);
            d.bias = d.wpk + nd_bias_offset(d.kind, cin, d.cout, ND_F32, T);
            ND_TRY(form == FORM_W1D4 ? nd_launch_conv_f43(d, flags, s) : nd_launch_conv_w1d(T, d, s));
            continue;
        }
        if (form == FORM_WINO3P) {
            // Winograd form, kWinoChunk images per pass (views of the same buffers)
            d.wpk = blob + bl.woff[st.layer];
            d.bias = nullptr;
            const int nimg = d.in.B;
            for (int b0 = 0; b0 < nimg; b0 += kWinoChunk) {
                ConvDesc c = d;
                c.in.B = c.out.B = nimg - b0 < kWinoChunk ? nimg - b0 : kWinoChunk;
                c.in.base = d.in.base + (size_t)b0 * d.in.Hb * d.in.Wb * 4;
                c.out.base = d.out.base + (size_t)b0 * d.out.Hb * d.out.Wb * 4;
                QpBuf pv;
                if (d.pool) {
                    pv = *d.pool;
                    pv.B = c.in.B;
                    pv.base = d.pool->base + (size_t)b0 * pv.Hb * pv.Wb * 4;
                    c.pool = &pv;
                }
                if (d.in2_origin) c.in2_origin = d.in2_origin + b0;   // (in2_origin_max bounds every chunk's entries)
                if (d.add_origin) c.add_origin = d.add_origin + b0;
                // (profiling: the split of a layer's time into its passes is recorded for a single-chunk layer only)
                ND_TRY(nd_launch_conv_wino(kWinoTile, c, pl.wino, pl.wino_bytes, s, (o.ev_x && nimg <= kWinoChunk) ? o.ev_x + 2 * this_step : nullptr));
                if (o.wino_tiles) o.wino_tiles[this_step] += nd_wino_launch_tiles(kWinoTile, c);
            }
            continue;
        }
        ND_TRY(nd_launch_conv(d, s));
    }
    if (o.ev) ND_HIP(hipEventRecord(o.ev[si], s));
    return ND_OK;
}

// ---------------------------------------------------------------- shared encoder of the fused denoise loop
// Tiles lie on a grid of stride S = ucs - ol, and every gathered tile is the window of one symmetric-padded frame at its origin.
// The encoder is a chain of valid 3x3 convolutions and 2x2 pools, so a tile's encoder tensors are windows of the same layers run
// on a band of tile rows -- where the tile's origin falls on a whole pixel of the level (and a pool's 2x2 phase agrees) -- except
// on the lines that its own ReflectionPad2d(2) reaches: rows / cols {0, 1, n-2, n-1} of the level-0 outputs, {0, n-1} below.
// fp32 useful-region mode shares levels 0 and 1 (convs1.0 ... the second pool: the conv_w2d layers, 64 % of the encoder's time at
// G24) when S % 4 == 0:
//   * the band runs steps [0, kSharedSteps) once on its window of the mirrored frame;
//   * the decoder reads neither the contaminated lines of CAT4 nor those of CAT3 (region plan) -- it reads the tile's skip halves
//     where the band wrote them (ConvDesc::in2; a step whose kernel has no second input source gets a copy of the window);
//   * P2 (the level-2 input, computed whole per tile) is copied from the band, and its contaminated rows / cols 0 and n-1 come
//     from kStrip-pixel edge images (16 input rows yield one P2 row through the 6 steps).  All tiles of a tile row reflect about
//     the same two frame lines, so their top / bottom rows are windows of two kStrip x wx images per tile row that follow the
//     tile along y (its reflection included) and the band along x: row_edge_plan, computed with the band.  Likewise two
//     hx x kStrip images per tile column of the band: col_edge_plan.  A windowed line is the tile's own except at its two end
//     pixels, where the tile's reflection along the other axis reaches: P2's four corner pixels come from kStrip x kStrip
//     patches reflected along both axes, four per tile of a launch (corner_plan).  Every image starts on the tile grid (S % 4 ==
//     0), so an F(4,3) pixel group of its first level covers the same pixels as in a strip of the tile's own input: with 8 | S a
//     windowed line has that strip's bits on pixels 2 ... n - 3; pixels 1 and n - 2 come from groups that also hold neighbours
//     of the reflected pixels and differ from it by fp32 rounding;
//   * launches take `batch` tiles across band seams: what they read of a band (CAT4, CAT3, P2 and the P2 lines of both edge
//     sets) lives in two slots, band b in slot b & 1, and a launch is cut at its second seam.
// The deeper levels stay per tile: their exact border lines would need strips of 36 / 76 input rows.
constexpr int kSharedSteps = 6;
constexpr int kStrip = 16;
constexpr double kBandBytes = 8.0 * (1 << 30);   // band tensors per launch of the shared steps (fixes the tile rows per band)

// extent of encoder buffer b (X0 ... P2) for a first-layer input of extent x (X0 = x, valid convs -2, pools /2)
inline int enc_extent(int x, int b) {
    const int p1 = (x - 4) / 2;
    switch (b) {
        case X0: return x;
        case A1: return x - 2;
        case CAT4: return x - 4;
        case P1: return p1;
        case A2: return p1 - 2;
        case CAT3: return p1 - 4;
        default: return (p1 - 4) / 2;   // P2
    }
}
// X0 ... P2 for B images of hx x wx first-layer input; planes sized for cap images of hcap x wcap (the plane stride does not move
// when a band or a batch is smaller: plane 1 of X0 and the slack stay zero from the one fill of the workspace).  slots > 1 (bands):
// the tensors the per-tile launches read -- CAT4, CAT3, P2 from `slotted` on (a band: all three, its edge images: P2) -- hold
// `slots` times the capacity, so that band b + 1 can be computed (into slot (b + 1) & 1: band_slot) while launches still read band b
Plan make_enc_plan(int f, int hx, int wx, int B, int hcap, int wcap, int cap, char *base, int dt, int slots = 1, Buf slotted = CAT4) {
    Plan p = {};
    size_t off = 0;
    auto add = [&](Buf id, int ch, int pad) {
        QpBuf &q = p.buf[id];
        q.planes = id == X0 ? 2 : (ch + nd_cpp(dt) - 1) / nd_cpp(dt);
        q.dt = dt;
        q.B = B;
        q.Hb = enc_extent(hx, id) + 2 * pad;
        q.Wb = enc_extent(wx, id) + 2 * pad;
        q.pad = pad;
        q.pstride = (long)cap * (enc_extent(hcap, id) + 2 * pad) * (enc_extent(wcap, id) + 2 * pad);
        if ((id == CAT4 || id == CAT3 || id == P2) && id >= slotted) q.pstride *= slots;
        q.base = (float *)(base + off);
        off += ((size_t)q.planes * q.pstride + nd_buf_slack(enc_extent(wcap, id) + 2 * pad)) * 16;
        off = (off + 255) & ~(size_t)255;
    };
    add(X0, 8, 0);
    add(A1, f, 0);
    add(CAT4, 2 * f, 2);
    add(P1, f, 0);
    add(A2, 2 * f, 0);
    add(CAT3, 4 * f, 2);
    add(P2, 2 * f, 0);
    p.split = nullptr;
    p.wino = nullptr;
    p.bytes = off;
    return p;
}

// 16-byte elements between the slots of a two-slot band tensor, and the view of a plan whose slotted tensors are slot `slot`
inline long slot_elems(const QpBuf &q, int slots) { return q.pstride / slots; }
inline Plan band_slot(Plan p, int slot, int slots, Buf slotted = CAT4) {
    for (Buf id : {CAT4, CAT3, P2})
        if (id >= slotted) p.buf[id].base += (size_t)slot * slot_elems(p.buf[id], slots) * 4;
    return p;
}

struct FramePlan {
    int D = 0;         // shared encoder levels (2, or 0: every tile runs its whole encoder)
    int aligned = 0;   // levels on which every tile origin is a whole pixel: 1 + the power of 2 in S, at most 4
    int S = 0, cols = 0, rows = 0, pad = 0;
    int R = 0, nbands = 0;   // tile rows per band, bands
    int slots = 1;           // slots of the band tensors the per-tile launches read (2 when there is more than one band)
    int hx = 0, wx = 0;      // first-layer input of a full band
    int win4[2] = {0, 0}, win3[2] = {0, 0};   // [lo, hi) of the CAT4 / CAT3 skip pixels the decoder reads (both axes)
    // frame workspace: band | row edges | column edges | corners | origins
    size_t band_bytes = 0, row_edge_bytes = 0, col_edge_bytes = 0, corner_bytes = 0, origin_bytes = 0, bytes = 0;
    // level 2 (levels == 3): behind the above, a third origin table | band | row images | column images | corner patches | Winograd scratch
    int levels = 0;          // encoder levels shared in all: D, or 3 with level 2
    int h2 = 0, w2 = 0;      // P2 of a full band
    int win2[2] = {0, 0};    // [lo, hi) of the CAT2 skip pixels the decoder reads
    size_t l2_band_bytes = 0, l2_row_bytes = 0, l2_col_bytes = 0, l2_corner_bytes = 0, l2_wino_bytes = 0;
    // bit k: the skip half of tconvs(4 - k).0 is folded out of the per-tile sums (frame_plan_folds); behind everything else in the
    // frame workspace, the Winograd scratch of the band launches of the folded three-pass steps (kFoldRows rows at a time)
    int folds = 0;
    size_t fold_wino_bytes = 0;
};
inline int band_hx(const FramePlan &fp, int nrows, int cs) { return (nrows - 1) * fp.S + cs + 4; }
// the edge images of a band of nrows tile rows (planes sized for a full band; P2 in the band's slots) and the corner patches of a
// launch of ntiles tiles (planes sized for cap): see the comment block above
inline Plan row_edge_plan(const FramePlan &fp, int f, int dt, int nrows, char *base) {
    return make_enc_plan(f, kStrip, fp.wx, 2 * nrows, kStrip, fp.wx, 2 * fp.R, base, dt, fp.slots, P2);
}
inline Plan col_edge_plan(const FramePlan &fp, int f, int dt, int nrows, int cs, char *base) {
    return make_enc_plan(f, band_hx(fp, nrows, cs), kStrip, 2 * fp.cols, fp.hx, kStrip, 2 * fp.cols, base, dt, fp.slots, P2);
}
inline Plan corner_plan(int f, int dt, int ntiles, int cap, char *base) {
    return make_enc_plan(f, kStrip, kStrip, 4 * ntiles, kStrip, kStrip, 4 * cap, base, dt);
}

// ---------------------------------------------------------------- level 2 of the shared encoder
// With 8 | S a tile origin is a whole P3 pixel too, and level 2 (convs3.0, convs3.2, the third pool: steps [kSharedSteps, kLevel2End))
// is shared the same way one level down:
//   * the band runs the three steps once on its P2.  A tile's reflection reaches only lines 0 and n - 1 of every level-2 tensor;
//   * tconvs2.0 leaves lines 0 and n - 1 of the CAT2 skip unread (region plan) and reads it where the band wrote it;
//   * a tile's P3 is its window of the band's P3, and its border lines come from kStrip2-line images at P2 resolution (6 P2 rows
//     yield one P3 row): the tile row's P2 edge line, which the level-0/1 row-edge images already produce, next to the five clean
//     band rows below (above) it -- two 6 x w2 images per tile row of a band, image side * nrows + row.  Likewise two h2 x 6 images
//     per tile column, image side * cols + column.  The four P3 corner pixels come from the 6 x 6 corner patches of the tile's own
//     assembled P2, image k * ntiles + t of a launch (k = 2 * bottom + right);
//   * the per-tile stack starts at convs4.0.
// Level 3 stays per tile: its border images would be one F(6x6) tile row of a 30-pixel tile side.
constexpr int kLevel2End = 9;
constexpr int kStrip2 = 6;

// extent of level-2 buffer b (P2 ... P3) for a P2 of extent x
inline int l2_extent(int x, int b) {
    switch (b) {
        case P2: return x;
        case A3: return x - 2;
        case CAT2: return x - 4;
        default: return (x - 4) / 2;   // P3
    }
}
// (P2) A3 CAT2 P3 for B images with a P2 of h2 x w2; planes sized for cap images of hcap x wcap.  The tensors the per-tile launches
// read -- CAT2 and P3 from `slotted` on (a band: both, its edge images: P3) -- hold `slots` times the capacity (make_enc_plan).
// own_p2 = false: P2 is the caller's (a band's, from its level-0/1 plan)
Plan make_l2_plan(int f, int h2, int w2, int B, int hcap, int wcap, int cap, char *base, int dt, int slots = 1, Buf slotted = CAT2,
                  bool own_p2 = true) {
    Plan p = {};
    size_t off = 0;
    auto add = [&](Buf id, int ch, int pad) {
        QpBuf &q = p.buf[id];
        q.planes = (ch + nd_cpp(dt) - 1) / nd_cpp(dt);
        q.dt = dt;
        q.B = B;
        q.Hb = l2_extent(h2, id) + 2 * pad;
        q.Wb = l2_extent(w2, id) + 2 * pad;
        q.pad = pad;
        q.pstride = (long)cap * (l2_extent(hcap, id) + 2 * pad) * (l2_extent(wcap, id) + 2 * pad);
        if ((id == CAT2 || id == P3) && id >= slotted) q.pstride *= slots;
        q.base = (float *)(base + off);
        off += ((size_t)q.planes * q.pstride + nd_buf_slack(l2_extent(wcap, id) + 2 * pad)) * 16;
        off = (off + 255) & ~(size_t)255;
    };
    if (own_p2) add(P2, 2 * f, 0);
    add(A3, 4 * f, 0);
    add(CAT2, 8 * f, 2);
    add(P3, 4 * f, 0);
    p.split = nullptr;
    p.wino = nullptr;
    p.bytes = off;
    return p;
}
inline Plan l2_slot(Plan p, int slot, int slots, Buf slotted = CAT2) {
    for (Buf id : {CAT2, P3})
        if (id >= slotted) p.buf[id].base += (size_t)slot * slot_elems(p.buf[id], slots) * 4;
    return p;
}

extern "C" int nd_tile_grid(int W, int H, int cs, int ucs, int ol, int *cols, int *rows, int *pad);

inline int band_h2(const FramePlan &fp, int nrows, int cs) { return enc_extent(band_hx(fp, nrows, cs), P2); }
inline Plan l2_band_plan(const FramePlan &fp, int f, int dt, int nrows, int cs, char *base) {
    return make_l2_plan(f, band_h2(fp, nrows, cs), fp.w2, 1, fp.h2, fp.w2, 1, base, dt, fp.slots, CAT2, false);
}
inline Plan l2_row_plan(const FramePlan &fp, int f, int dt, int nrows, char *base) {
    return make_l2_plan(f, kStrip2, fp.w2, 2 * nrows, kStrip2, fp.w2, 2 * fp.R, base, dt, fp.slots, P3);
}
inline Plan l2_col_plan(const FramePlan &fp, int f, int dt, int nrows, int cs, char *base) {
    return make_l2_plan(f, band_h2(fp, nrows, cs), kStrip2, 2 * fp.cols, fp.h2, kStrip2, 2 * fp.cols, base, dt, fp.slots, P3);
}
inline Plan l2_corner_plan(int f, int dt, int ntiles, int cap, char *base) {
    return make_l2_plan(f, kStrip2, kStrip2, 4 * ntiles, kStrip2, kStrip2, 4 * cap, base, dt);
}

// Level 2 on top of a level-0/1 plan (fp->D == 2): shared when 8 | S, the decoder leaves lines 0 and n - 1 of the CAT2 skip unread,
// and every level-2 step of the band, the two line image shapes and the corner patches runs in a kernel that takes any image
// shape and pools in its epilogue (conv_w2d, three-pass F(6x6)).  rois: the region plan of a tile
inline void frame_plan_level2(int f, int dt, int flags, int cs, int batch, const BlobLayout &bl, const Roi *rois, FramePlan *fp) {
    fp->levels = fp->D;
    if ((flags & ND_FLAG_TILE_LEVEL2) || fp->S % 8) return;
    const int n2 = enc_extent(cs + 4, P2), n = l2_extent(n2, CAT2);
    if (n2 < kStrip2 + 2 || l2_extent(n2, P3) < 3) return;
    bool reads_cat2 = false;
    for (int i = kLevel2End; i < kNumSteps; ++i) {
        const Step &st = kSteps[i];
        if (st.layer < 0 || st.src != CAT2 || kLayers[st.layer].kind != ND_CONVT3) continue;
        if (rois[i].rows <= 0 || rois[i].r0 != rois[i].c0 || rois[i].rows != rois[i].cols) return;
        fp->win2[0] = rois[i].r0 - 2 < 0 ? 0 : rois[i].r0 - 2;
        fp->win2[1] = rois[i].r0 + rois[i].rows > n ? n : rois[i].r0 + rois[i].rows;
        if (fp->win2[0] < 1 || fp->win2[1] > n - 1 || fp->win2[1] <= fp->win2[0]) return;
        reads_cat2 = true;
    }
    if (!reads_cat2) return;
    fp->h2 = enc_extent(fp->hx, P2);
    fp->w2 = enc_extent(fp->wx, P2);
    Plan plans[4] = {l2_band_plan(*fp, f, dt, fp->R, cs, nullptr), l2_row_plan(*fp, f, dt, fp->R, nullptr),
                     l2_col_plan(*fp, f, dt, fp->R, cs, nullptr), l2_corner_plan(f, dt, batch, batch, nullptr)};
    plans[0].buf[P2] = make_enc_plan(f, fp->hx, fp->wx, 1, fp->hx, fp->wx, 1, nullptr, dt).buf[P2];
    size_t wino = 0;
    for (const Plan &pp : plans)
        for (int i = kSharedSteps; i < kLevel2End; ++i) {
            const Step &st = kSteps[i];
            if (st.layer < 0) continue;
            const LayerSpec &l = kLayers[st.layer];
            const Form form = step_form(st, f, dt, flags, pp, bl);
            if (form == FORM_WINO3P) {
                // (the tile workspace's scratch is sized for the tiles of a launch: level 2 carries its own, for any batch)
                QpBuf v = pp.buf[st.src];
                v.B = v.B < kWinoChunk ? v.B : kWinoChunk;
                const size_t need = nd_wino_scratch_bytes(kWinoTile, v, lcin(l, f), lcout(l, f));
                wino = need > wino ? need : wino;
            } else if (form != FORM_W1D4 || !nd_f43_w2d(pp.buf[st.src], lcout(l, f), false, flags)) {
                return;
            }
        }
    fp->l2_band_bytes = plans[0].bytes;
    fp->l2_row_bytes = plans[1].bytes;
    fp->l2_col_bytes = plans[2].bytes;
    fp->l2_corner_bytes = plans[3].bytes;
    fp->l2_wino_bytes = (wino + 255) & ~(size_t)255;
    fp->bytes += fp->origin_bytes + fp->l2_band_bytes + fp->l2_row_bytes + fp->l2_col_bytes + fp->l2_corner_bytes + fp->l2_wino_bytes;
    fp->levels = 3;
}

// ---------------------------------------------------------------- skip halves of the decoder, once per band
// The first layer of a decoder level is a ConvTranspose2d(3) on cat([up, skip]), linear in its input channels:
//     act(b + W_up * up + W_skip * skip) = act(W_up * up + P),   P = W_skip * skip + b.
// Where the skip is a band tensor, P is a band tensor too: the same values for every tile that overlaps a pixel (2.0 / 2.1 / 2.6
// tiles on average at levels 0 / 1 / 2 of G24).  A folded step's P is computed with the band, right behind the concat tensor it
// derives from, into that tensor's up-sampled half -- which no band launch writes, has the skip half's plane geometry, and holds
// the n + 2 output of a ConvTranspose2d(3) inside its n + 4 bordered plane at border 1 -- restricted to the rows and columns some
// tile's region reads; the per-tile step then runs on the K blocks of its up-sampled half alone and takes its window of P as the
// addend of its epilogue (ConvDesc::add; the window starts where the in-place skip read starts: the same origin table).  The bias
// is part of P.  Both launches use the layer's one packed blob, each its K-block sub-range (ConvDesc::w_kb).
// Which steps fold: those that read a band skip and run in a kernel that takes an addend (conv_w2d, three-pass F(6x6)) -- the
// plan's decision, a function of geometry, dtype and flags; ND_FLAG_TILE_SKIPS folds none.  A three-pass step's band launch runs
// kFoldRows output rows at a time on Winograd scratch of its own in the frame workspace (a band is one image of any size; the tile
// workspace's scratch is sized for the tiles of a launch).
constexpr int kFoldRows = 48;
inline void frame_plan_folds(int f, int dt, int flags, const Plan &tp, const BlobLayout &bl, FramePlan *fp) {
    fp->folds = 0;
    fp->fold_wino_bytes = 0;
    if (!fp->D || (flags & ND_FLAG_TILE_SKIPS)) return;
    const Buf cats[3] = {CAT4, CAT3, CAT2};
    for (int k = 0; k < (fp->levels == 3 ? 3 : 2); ++k)
        for (int i = kSharedSteps; i < kNumSteps; ++i) {
            const Step &st = kSteps[i];
            if (st.layer < 0 || st.src != cats[k] || kLayers[st.layer].kind != ND_CONVT3) continue;
            const Form form = step_form(st, f, dt, flags, tp, bl);
            if (!form_takes_src2(st, form, f, flags, tp)) continue;
            fp->folds |= 1 << k;
            if (form != FORM_WINO3P) continue;
            QpBuf v = {};
            v.B = 1;
            v.Hb = kFoldRows + 2;
            v.Wb = (k == 2 ? l2_extent(fp->w2, CAT2) : enc_extent(fp->wx, cats[k])) + 4;
            const size_t need = nd_wino_scratch_bytes(kWinoTile, v, lcin(kLayers[st.layer], f) / 2, lcout(kLayers[st.layer], f));
            if (need > fp->fold_wino_bytes) fp->fold_wino_bytes = need;
        }
    fp->fold_wino_bytes = (fp->fold_wino_bytes + 255) & ~(size_t)255;
    fp->bytes += fp->fold_wino_bytes;
}
// P of decoder step `step` for a band of nrows tile rows whose concat tensor is `cat` (skip half: planes [planes, 2 * planes)):
// roi = the step's region on a tile, tstep = the tile stride at the level; form = the step's kernel family (conv_w2d, or the
// three-pass form on `wino`, kFoldRows rows of the band at a time)
inline int launch_skip_fold(int f, int flags, const float *blob, const BlobLayout &bl, int step, Form form, const QpBuf &cat, int planes,
                            const Roi &roi, int tstep, int nrows, int cols, float *split, char *wino, size_t wino_bytes, hipStream_t s) {
    const LayerSpec &l = kLayers[kSteps[step].layer];
    const int cin = lcin(l, f);
    ConvDesc d;
    d.kind = l.kind;
    d.act = ND_ACT_NONE;
    d.cin = planes * 4;
    d.cout = lcout(l, f);
    d.wpk = blob + bl.w1off[kSteps[step].layer];
    d.bias = d.wpk + nd_bias_offset(l.kind, cin, d.cout, ND_F32, kW1dTile);
    d.w_kb = nd_kblocks(cin);
    d.w_kb0 = planes / 2;
    d.in = cat;
    d.in_plane0 = planes;
    d.out = cat;
    d.out.pad = 1;
    d.out_plane0 = 0;
    d.part = split;
    d.part_bytes = split ? kSplitScratchBytes : 0;
    d.nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
    d.roi_r0 = roi.r0;
    d.roi_c0 = roi.c0;
    d.roi_rows = (nrows - 1) * tstep + roi.rows;
    d.roi_cols = (cols - 1) * tstep + roi.cols;
    if (form != FORM_WINO3P) return nd_launch_conv_w2d(d, s);
    d.wpk = blob + bl.woff[kSteps[step].layer];
    d.bias = nullptr;
    const int r_end = d.roi_r0 + d.roi_rows;
    for (int r0 = d.roi_r0; r0 < r_end; r0 += kFoldRows) {
        // rows [r0, r0 + rows) of the region as a view of rows + 2 bordered input rows (the scratch follows the view's extent)
        ConvDesc c = d;
        const int rows = r_end - r0 < kFoldRows ? r_end - r0 : kFoldRows;
        c.in.base = c.out.base = cat.base + (size_t)r0 * cat.Wb * 4;
        c.in.Hb = c.out.Hb = rows + 2;
        c.roi_r0 = 0;
        c.roi_rows = rows;
        ND_TRY(nd_launch_conv_wino(kWinoTile, c, wino, wino_bytes, s));
    }
    return ND_OK;
}

// the band plan: a function of the frame geometry, the dtype and the flags (batch only sizes the corner buffers and the tables)
int frame_plan(int f, int dt, int flags, int W, int H, int cs, int ucs, int ol, int batch, FramePlan *fp) {
    *fp = FramePlan();
    ND_TRY(check_funit(f, dt));
    if (!valid_cs(cs)) ND_FAIL(ND_EINVAL, "frame plan: tile size %d", cs);
    ND_TRY(nd_tile_grid(W, H, cs, ucs, ol, &fp->cols, &fp->rows, &fp->pad));
    fp->S = ucs - ol;
    fp->aligned = 1;
    while (fp->aligned < 4 && fp->S % (1 << fp->aligned) == 0) ++fp->aligned;
    // a tile origin must fall on a whole pixel of level 2 (the pooled input P2 is copied from the band), the arithmetic must be
    // the fp32 F(4,3) layers this plan was built for, and the decoder must leave the contaminated skip lines unread
    if (dt != ND_F32 || (flags & (ND_FLAG_FULL_TILES | ND_FLAG_TILE_ENCODER | ND_FLAG_DIRECT_CONV | ND_FLAG_W1D_REGS)) ||
        fp->S % 4 || W < cs || H < cs || batch <= 0)
        return ND_OK;
    const Plan tp = make_plan(f, cs, cs, 1, 1, nullptr, dt);
    const BlobLayout bl = blob_layout(f, dt);
    Roi rois[kNumSteps];
    const int crop = (cs - ucs) / 2;
    if (!plan_rois(tp, crop, crop, rois)) return ND_OK;   // (the executor also checks that the kernels take them: rois_supported)
    for (int i = 0; i < kNumSteps; ++i) {
        const Step &st = kSteps[i];
        if (st.layer < 0 || (st.src != CAT4 && st.src != CAT3) || kLayers[st.layer].kind != ND_CONVT3) continue;
        const int n = enc_extent(cs + 4, st.src), edge = st.src == CAT4 ? 2 : 1;
        if (rois[i].rows <= 0 || rois[i].r0 != rois[i].c0 || rois[i].rows != rois[i].cols) return ND_OK;
        int *w = st.src == CAT4 ? fp->win4 : fp->win3;
        w[0] = rois[i].r0 - 2 < 0 ? 0 : rois[i].r0 - 2;   // a transposed 3x3 layer reads input rows [lo - 2, hi) for output rows [lo, hi)
        w[1] = rois[i].r0 + rois[i].rows > n ? n : rois[i].r0 + rois[i].rows;
        if (w[0] < edge || w[1] > n - edge) return ND_OK;
    }
    if (fp->win4[1] <= fp->win4[0] || fp->win3[1] <= fp->win3[0]) return ND_OK;
    // tile rows per band: as many as kBandBytes holds
    fp->wx = (fp->cols - 1) * fp->S + cs + 4;
    for (int R = fp->rows; R >= 1; --R) {
        const int hx = band_hx(*fp, R, cs);
        const size_t b = make_enc_plan(f, hx, fp->wx, 1, hx, fp->wx, 1, nullptr, dt).bytes;
        if (b <= kBandBytes || R == 1) {
            fp->R = R;
            fp->hx = hx;
            fp->band_bytes = b;
            break;
        }
    }
    // as few bands as that allows, of near-equal height (a short last band would repeat the band border for few tiles)
    fp->nbands = (fp->rows + fp->R - 1) / fp->R;
    fp->R = (fp->rows + fp->nbands - 1) / fp->nbands;
    fp->hx = band_hx(*fp, fp->R, cs);
    // (the rows per band are fixed by one slot of every tensor: the second slot is memory on top of kBandBytes)
    fp->slots = fp->nbands > 1 ? 2 : 1;
    fp->band_bytes = make_enc_plan(f, fp->hx, fp->wx, 1, fp->hx, fp->wx, 1, nullptr, dt, fp->slots).bytes;
    if ((long)fp->hx * fp->wx >= (1L << 26)) return ND_OK;   // (32-bit offsets of the conv kernels on a band image)
    // every shared step of the band and of the three edge shapes must run in conv_w2d (its pool epilogue included)
    const Plan plans[4] = {make_enc_plan(f, fp->hx, fp->wx, 1, fp->hx, fp->wx, 1, nullptr, dt), row_edge_plan(*fp, f, dt, fp->R, nullptr),
                           col_edge_plan(*fp, f, dt, fp->R, cs, nullptr), corner_plan(f, dt, batch, batch, nullptr)};
    for (const Plan &pp : plans)
        for (int i = 0; i < kSharedSteps; ++i) {
            const Step &st = kSteps[i];
            if (st.layer < 0) continue;
            if (step_form(st, f, dt, flags, pp, bl) != FORM_W1D4 || !nd_f43_w2d(pp.buf[st.src], lcout(kLayers[st.layer], f), false, flags))
                return ND_OK;
        }
    fp->row_edge_bytes = plans[1].bytes;
    fp->col_edge_bytes = plans[2].bytes;
    fp->corner_bytes = plans[3].bytes;
    // where each tile of a launch lies in the band's CAT4 / CAT3 planes (the decoder reads the skip halves in place): two tables
    fp->origin_bytes = ((size_t)batch * sizeof(int) + 255) & ~(size_t)255;
    fp->bytes = fp->band_bytes + fp->row_edge_bytes + fp->col_edge_bytes + fp->corner_bytes + 2 * fp->origin_bytes;
    fp->D = 2;
    frame_plan_level2(f, dt, flags, cs, batch, bl, rois, fp);
    frame_plan_folds(f, dt, flags, tp, bl, fp);
    return ND_OK;
}

}  // namespace
