// Fused frame loop of UtNet with the shared encoder: what a shared level is (kLevels), the plan of a frame (bands, skip windows,
// folds, frame workspace) and the executor behind nd_utnet_denoise_frame.  The net itself -- layers, buffers, run_stack -- is
// utnet_net.h; the per-tile launch this loop falls back to is utnet.hip's nd_utnet_denoise_tiles.
#include <string.h>

#include "nd_common.h"

#include "utnet_net.h"

namespace {

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
//     tile along y (its reflection included) and the band along x: row_plan, computed with the band.  Likewise two
//     hx x kStrip images per tile column of the band: col_plan.  A windowed line is the tile's own except at its two end
//     pixels, where the tile's reflection along the other axis reaches: P2's four corner pixels come from kStrip x kStrip
//     patches reflected along both axes, four per tile of a launch (corner_plan).  Every image starts on the tile grid (S % 4 ==
//     0), so an F(4,3) pixel group of its first level covers the same pixels as in a strip of the tile's own input: with 8 | S a
//     windowed line has that strip's bits on pixels 2 ... n - 3; pixels 1 and n - 2 come from groups that also hold neighbours
//     of the reflected pixels and differ from it by fp32 rounding;
//   * launches take `batch` tiles across band seams: what they read of a band (CAT4, CAT3, P2 and the P2 lines of both edge
//     sets) lives in two slots, band b in slot b & 1, and a launch is cut at its second seam.
// The deeper levels stay per tile: their exact border lines would need strips of 36 / 76 input rows.
//
// With 8 | S a tile origin is a whole P3 pixel too, and level 2 (convs3.0, convs3.2, the third pool: steps [kSharedSteps, kLevel2End))
// is shared the same way one level down:
//   * the band runs the three steps once on its P2.  A tile's reflection reaches only lines 0 and n - 1 of every level-2 tensor;
//   * tconvs2.0 leaves lines 0 and n - 1 of the CAT2 skip unread (region plan) and reads it where the band wrote it;
//   * a tile's P3 is its window of the band's P3, and its border lines come from kStrip2-line images at P2 resolution (6 P2 rows
//     yield one P3 row): the tile row's P2 edge line, which the level-0/1 row-edge images already produce, next to the five clean
//     band rows below (above) it -- two 6 x w2 images per tile row of a band, image side * nrows + row.  Likewise two h2 x 6 images
//     per tile column, image side * cols + column.  The four P3 corner pixels come from the 6 x 6 corner patches of the tile's own
//     assembled P2, image k * ntiles + t of a launch (k = 2 * bottom + right) -- the only reader of a tile's own P2 then, so
//     only those corner windows of it are assembled (assemble_output);
//   * the per-tile stack starts at convs4.0.
// Level 3 stays per tile: its border images would be one F(6x6) tile row of a 30-pixel tile side.
constexpr int kSharedSteps = 6, kLevel2End = 9;
constexpr int kStrip = 16, kStrip2 = 6;
constexpr double kBandBytes = 8.0 * (1 << 30);   // band tensors per launch of the shared steps (fixes the tile rows per band)

// A shared level: everything the plan and the executor know about levels 0/1 and level 2 apart
struct Level {
    int begin, end;    // its steps of kSteps
    Buf in, out;       // its input (level 0/1: gathered from the frame; below: the band's own output of the level above) and its
                       // pooled output, which the per-tile launches assemble
    int strip;         // input lines that yield one output line: the short side of its line images and corner patches
    int out_shift;     // the tile stride at `out` is S >> out_shift; every tile origin must be a whole pixel there
    bool three_pass;   // its steps may run in the three-pass F(6x6) form, on Winograd scratch of the level's own in the frame workspace
                       // (the tile workspace's is sized for the tiles of a launch); else in conv_w2d alone
    bool by_side;      // its line images are numbered side * count + index and its corner patches k * ntiles + t: the splices that
                       // fill them write consecutive images; else 2 * index + side and 4 * t + k, as k_gather_edges writes them
};
const Level kLevels[2] = {{0, kSharedSteps, X0, P2, kStrip, 2, false, false}, {kSharedSteps, kLevel2End, P2, P3, kStrip2, 3, true, true}};
// The skip tensors the decoder reads in the band, by the level that writes them; `edge` lines on every side are contaminated and
// must stay unread.  Skip k has tile stride S >> k
struct SkipSpec { Buf cat; int level, edge; };
const SkipSpec kSkips[3] = {{CAT4, 0, 2}, {CAT3, 0, 1}, {CAT2, 1, 1}};
// the transposed 3x3 layer of the decoder that reads concat tensor `cat`
inline int skip_step(Buf cat) {
    for (int i = 0; i < kNumSteps; ++i)
        if (kSteps[i].layer >= 0 && kSteps[i].src == cat && kLayers[kSteps[i].layer].kind == ND_CONVT3) return i;
    return -1;
}

// the tensors of a level that the per-tile launches read: its concat tensors and its output
inline bool launch_reads(const Level &lv, int id) { return kBufs[id].pad == 2 || id == lv.out; }
// lv.in ... lv.out for B images with an input of h x w; planes sized for cap images of hcap x wcap (the plane stride does not move
// when a band or a batch is smaller: plane 1 of X0 and the slack stay zero from the one fill of the workspace).  own_in = false:
// lv.in is the caller's (a band's, from the plan of the level above).  slots > 1 (bands): the tensors the per-tile launches read,
// from `slotted` on (a band: all of them, its line images: lv.out), hold `slots` times the capacity, so that band b + 1 can be
// computed (into slot (b + 1) & 1: slot_view) while launches still read band b
Plan level_plan(const Level &lv, int f, int dt, int h, int w, int B, int hcap, int wcap, int cap, char *base, int slots = 1,
                Buf slotted = X0, bool own_in = true) {
    Plan p = {};
    size_t off = 0;
    const Extents eh = extents_from(lv.in, h), ew = extents_from(lv.in, w), ehc = extents_from(lv.in, hcap), ewc = extents_from(lv.in, wcap);
    for (int id = own_in ? lv.in : lv.in + 1; id <= lv.out; ++id)
        place_buf(p, (Buf)id, f, dt, B, eh[id], ew[id], cap, ehc[id], ewc[id], launch_reads(lv, id) && id >= slotted ? slots : 1, base, &off);
    p.bytes = off;
    return p;
}
// 16-byte elements between the slots of a two-slot band tensor, and the view of a plan whose slotted tensors are slot `slot`
inline long slot_elems(const QpBuf &q, int slots) { return q.pstride / slots; }
inline Plan slot_view(Plan p, const Level &lv, int slot, int slots, Buf slotted = X0) {
    for (int id = lv.in; id <= lv.out; ++id)
        if (launch_reads(lv, id) && id >= slotted) p.buf[id].base += (size_t)slot * slot_elems(p.buf[id], slots) * 4;
    return p;
}

struct LevelBytes { size_t band = 0, rows = 0, cols = 0, corners = 0, scratch = 0; };
struct FramePlan {
    int D = 0;         // shared encoder levels (2, or 0: every tile runs its whole encoder)
    int levels = 0;    // encoder levels shared in all: D, or 3 with level 2
    int aligned = 0;   // levels on which every tile origin is a whole pixel: 1 + the power of 2 in S, at most 4
    int S = 0, cols = 0, rows = 0, pad = 0;
    int R = 0, nbands = 0;   // tile rows per band, bands
    int slots = 1;           // slots of the band tensors the per-tile launches read (2 when there is more than one band)
    int in_h[2] = {0, 0}, in_w[2] = {0, 0};   // per level, its input of a full band (X0, P2)
    int win[3][2] = {};      // [lo, hi) of the pixels of skip k that the decoder reads (both axes)
    LevelBytes lb[2];        // per level, its parts of the frame workspace
    size_t origin_bytes = 0; // one table of where each tile of a launch lies in a band skip (the decoder reads it in place)
    // bit k: the skip half of tconvs(4 - k).0 is folded out of the per-tile sums (plan_folds); fold_bytes: the Winograd scratch of
    // the band launches of the folded three-pass steps (kFoldRows rows at a time)
    int folds = 0;
    size_t fold_bytes = 0;
    size_t bytes = 0;        // the frame workspace (frame_ws)
};
inline int shared_levels(const FramePlan &fp) { return fp.levels == 3 ? 2 : fp.D ? 1 : 0; }

// The frame workspace, in order: per level 0/1 its band | row lines | column lines | corner patches, two origin tables; with level
// 2 a third origin table and the level's four parts and scratch; the fold scratch.  A null base asks for the size alone
struct FrameWs {
    char *band[2], *rows[2], *cols[2], *corners[2], *scratch[2];
    int *origins[3];
    char *fold_scratch;
    size_t bytes;
};
inline FrameWs frame_ws(const FramePlan &fp, char *base) {
    FrameWs w = {};
    size_t off = 0;
    auto take = [&](size_t n) {
        char *const p = base ? base + off : nullptr;
        off += n;
        return p;
    };
    auto level = [&](int l) {
        w.band[l] = take(fp.lb[l].band);
        w.rows[l] = take(fp.lb[l].rows);
        w.cols[l] = take(fp.lb[l].cols);
        w.corners[l] = take(fp.lb[l].corners);
        w.scratch[l] = take(fp.lb[l].scratch);
    };
    level(0);
    for (int k = 0; k < 2; ++k) w.origins[k] = (int *)take(fp.origin_bytes);
    if (fp.levels == 3) {
        w.origins[2] = (int *)take(fp.origin_bytes);
        level(1);
    }
    w.fold_scratch = take(fp.fold_bytes);
    w.bytes = off;
    return w;
}

// The images of level l, one builder per shape (planes sized for a full band; the tensors the launches read in slot `slot` of the
// band's slots): a band of nrows tile rows, the two line images of each of its tile rows and of each tile column, and the four
// corner patches of each of the ntiles tiles of a launch (planes sized for cap tiles)
inline int band_hx(const FramePlan &fp, int nrows, int cs) { return (nrows - 1) * fp.S + cs + 4; }
inline int band_in_h(const FramePlan &fp, int l, int nrows, int cs) { return extents_from(X0, band_hx(fp, nrows, cs))[kLevels[l].in]; }
inline Plan band_plan(const FramePlan &fp, int l, int f, int dt, int nrows, int cs, char *base, int slot = 0) {
    const Level &lv = kLevels[l];
    return slot_view(level_plan(lv, f, dt, band_in_h(fp, l, nrows, cs), fp.in_w[l], 1, fp.in_h[l], fp.in_w[l], 1, base, fp.slots, X0, l == 0),
                     lv, slot, fp.slots);
}
inline Plan row_plan(const FramePlan &fp, int l, int f, int dt, int nrows, char *base, int slot = 0) {
    const Level &lv = kLevels[l];
    return slot_view(level_plan(lv, f, dt, lv.strip, fp.in_w[l], 2 * nrows, lv.strip, fp.in_w[l], 2 * fp.R, base, fp.slots, lv.out), lv, slot,
                     fp.slots, lv.out);
}
inline Plan col_plan(const FramePlan &fp, int l, int f, int dt, int nrows, int cs, char *base, int slot = 0) {
    const Level &lv = kLevels[l];
    return slot_view(level_plan(lv, f, dt, band_in_h(fp, l, nrows, cs), lv.strip, 2 * fp.cols, fp.in_h[l], lv.strip, 2 * fp.cols, base, fp.slots,
                                lv.out), lv, slot, fp.slots, lv.out);
}
inline Plan corner_plan(int l, int f, int dt, int ntiles, int cap, char *base) {
    const Level &lv = kLevels[l];
    return level_plan(lv, f, dt, lv.strip, lv.strip, 4 * ntiles, lv.strip, lv.strip, 4 * cap, base);
}

// Level l can be shared on this grid: every tile origin is a whole pixel of its output, a tile holds its line images with clean
// lines between them (any tile does at level 0/1), and the decoder's region plan (rois, of a tile) restricts the step that reads
// each of its skips to a square region that leaves the contaminated lines unread -- fp->win of those skips
inline bool level_shareable(int l, int cs, const Roi *rois, FramePlan *fp) {
    const Level &lv = kLevels[l];
    const Extents tile = extents_from(X0, cs + 4);
    if (fp->S % (1 << lv.out_shift) || tile[lv.in] < lv.strip + 2 || tile[lv.out] < 3) return false;
    for (int k = 0; k < 3; ++k) {
        if (kSkips[k].level != l) continue;
        const int n = tile[kSkips[k].cat], edge = kSkips[k].edge;
        const Roi &r = rois[skip_step(kSkips[k].cat)];
        if (r.rows <= 0 || r.r0 != r.c0 || r.rows != r.cols) return false;
        int *w = fp->win[k];
        w[0] = r.r0 - 2 < 0 ? 0 : r.r0 - 2;   // a transposed 3x3 layer reads input rows [lo - 2, hi) for output rows [lo, hi)
        w[1] = r.r0 + r.rows > n ? n : r.r0 + r.rows;
        if (w[0] < edge || w[1] > n - edge || w[1] <= w[0]) return false;
    }
    return true;
}

// The parts of level l in the frame workspace, for a launch capacity of `batch` tiles -- or false: every step of the band, of the
// two line image shapes and of the corner patches must run in a kernel that takes any image shape and pools in its epilogue:
// conv_w2d, or the three-pass form where the level carries scratch for it
inline bool plan_level(int l, int f, int dt, int flags, int cs, int batch, const BlobLayout &bl, FramePlan *fp) {
    const Level &lv = kLevels[l];
    Plan plans[4] = {band_plan(*fp, l, f, dt, fp->R, cs, nullptr), row_plan(*fp, l, f, dt, fp->R, nullptr),
                     col_plan(*fp, l, f, dt, fp->R, cs, nullptr), corner_plan(l, f, dt, batch, batch, nullptr)};
    if (l > 0) plans[0].buf[lv.in] = band_plan(*fp, l - 1, f, dt, fp->R, cs, nullptr).buf[lv.in];
    size_t scratch = 0;
    for (const Plan &pp : plans)
        for (int i = lv.begin; i < lv.end; ++i) {
            const Step &st = kSteps[i];
            if (st.layer < 0) continue;
            const LayerSpec &ly = kLayers[st.layer];
            const Form form = step_form(st, f, dt, flags, pp, bl);
            if (form == FORM_WINO3P && lv.three_pass) {
                QpBuf v = pp.buf[st.src];
                v.B = v.B < kWinoChunk ? v.B : kWinoChunk;
                const size_t need = nd_wino_scratch_bytes(kWinoTile, v, lcin(ly, f), lcout(ly, f));
                scratch = need > scratch ? need : scratch;
            } else if (form != FORM_W1D4 || !nd_f43_w2d(pp.buf[st.src], lcout(ly, f), false, flags)) {
                return false;
            }
        }
    fp->lb[l] = LevelBytes{plans[0].bytes, plans[1].bytes, plans[2].bytes, plans[3].bytes, (scratch + 255) & ~(size_t)255};
    return true;
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
// tp: the plan of a tile
inline void plan_folds(int f, int dt, int flags, const Plan &tp, const BlobLayout &bl, FramePlan *fp) {
    if (flags & ND_FLAG_TILE_SKIPS) return;
    const Extents band_w = extents_from(X0, fp->in_w[0]);
    for (int k = 0; k < 3; ++k) {
        if (kSkips[k].level >= shared_levels(*fp)) continue;
        const Step &st = kSteps[skip_step(kSkips[k].cat)];
        const Form form = step_form(st, f, dt, flags, tp, bl);
        if (!form_takes_src2(st, form, f, flags, tp)) continue;
        fp->folds |= 1 << k;
        if (form != FORM_WINO3P) continue;
        QpBuf v = {};
        v.B = 1;
        v.Hb = kFoldRows + 2;
        v.Wb = band_w[kSkips[k].cat] + 4;
        const size_t need = nd_wino_scratch_bytes(kWinoTile, v, lcin(kLayers[st.layer], f) / 2, lcout(kLayers[st.layer], f));
        if (need > fp->fold_bytes) fp->fold_bytes = need;
    }
    fp->fold_bytes = (fp->fold_bytes + 255) & ~(size_t)255;
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

// the plan of a frame: a function of the frame geometry, the dtype and the flags (batch only sizes the corner buffers and the tables)
int frame_plan(int f, int dt, int flags, int W, int H, int cs, int ucs, int ol, int batch, FramePlan *fp) {
    *fp = FramePlan();
    ND_TRY(check_funit(f, dt));
    if (!valid_cs(cs)) ND_FAIL(ND_EINVAL, "frame plan: tile size %d", cs);
    ND_TRY(nd_tile_grid(W, H, cs, ucs, ol, &fp->cols, &fp->rows, &fp->pad));
    fp->S = ucs - ol;
    fp->aligned = 1;
    while (fp->aligned < 4 && fp->S % (1 << fp->aligned) == 0) ++fp->aligned;
    // the arithmetic must be the fp32 F(4,3) layers this plan was built for, on the useful regions
    if (dt != ND_F32 || (flags & (ND_FLAG_FULL_TILES | ND_FLAG_TILE_ENCODER | ND_FLAG_DIRECT_CONV | ND_FLAG_W1D_REGS)) || W < cs || H < cs ||
        batch <= 0)
        return ND_OK;
    const Plan tp = make_plan(f, cs, cs, 1, 1, nullptr, dt);
    const BlobLayout bl = blob_layout(f, dt);
    Roi rois[kNumSteps];
    const int crop = (cs - ucs) / 2;
    if (!plan_rois(tp, crop, crop, rois)) return ND_OK;   // (the executor also checks that the kernels take them: rois_supported)
    if (!level_shareable(0, cs, rois, fp)) return ND_OK;
    // tile rows per band: as many as kBandBytes holds (one slot of every tensor: the second slot is memory on top of kBandBytes)
    const int wx = (fp->cols - 1) * fp->S + cs + 4;
    for (fp->R = fp->rows; fp->R > 1; --fp->R) {
        const int hx = band_hx(*fp, fp->R, cs);
        if (level_plan(kLevels[0], f, dt, hx, wx, 1, hx, wx, 1, nullptr).bytes <= kBandBytes) break;
    }
    // as few bands as that allows, of near-equal height (a short last band would repeat the band border for few tiles)
    fp->nbands = (fp->rows + fp->R - 1) / fp->R;
    fp->R = (fp->rows + fp->nbands - 1) / fp->nbands;
    fp->slots = fp->nbands > 1 ? 2 : 1;
    const Extents eh = extents_from(X0, band_hx(*fp, fp->R, cs)), ew = extents_from(X0, wx);
    for (int l = 0; l < 2; ++l) {
        fp->in_h[l] = eh[kLevels[l].in];
        fp->in_w[l] = ew[kLevels[l].in];
    }
    if ((long)fp->in_h[0] * fp->in_w[0] >= (1L << 26)) return ND_OK;   // (32-bit offsets of the conv kernels on a band image)
    if (!plan_level(0, f, dt, flags, cs, batch, bl, fp)) return ND_OK;
    fp->origin_bytes = ((size_t)batch * sizeof(int) + 255) & ~(size_t)255;
    fp->D = fp->levels = 2;
    if (!(flags & ND_FLAG_TILE_LEVEL2) && level_shareable(1, cs, rois, fp) && plan_level(1, f, dt, flags, cs, batch, bl, fp)) fp->levels = 3;
    plan_folds(f, dt, flags, tp, bl, fp);
    fp->bytes = frame_ws(*fp, nullptr).bytes;
    return ND_OK;
}

// ---------------------------------------------------------------- the executor
// what the routines of one nd_utnet_denoise_frame call share
struct Frame {
    int f, act, dt, flags;
    const float *blob;
    const float *img;
    float *canvas;
    int W, H, cs, ucs, ol, batch;
    hipStream_t s;
    BlobLayout bl;
    FramePlan fp;
    FrameWs ws;
    int nlev;              // shared_levels(fp)
    Plan pl;               // the tile workspace at capacity (its split-K scratch serves every launch of the stream)
    Roi rois[kNumSteps];   // the region plan of a tile
    Extents tile;          // the buffer extents of a tile
    // per level, the band plan at full height (slot 0) -- what a launch addresses, with each tile's band row and slot folded into
    // its origin / its splice
    Plan full[2];
    // how the decoder step that reads skip k gets it: in place from the band where its kernel has a second input source, else as
    // a copy of the window in the tile buffer, as the layer expects it (k_splice).  A step the plan folds (plan_folds) reads no
    // skip at all: its window of the band's P is its addend
    struct Skip { int step; bool in_place, fold; Form form; } skips[3];
    int skip_planes(int k) const { return pl.buf[kSkips[k].cat].planes / 2; }   // the skip is the upper half of the concat
    int tile_rows(int b) const { return fp.rows - b * fp.R < fp.R ? fp.rows - b * fp.R : fp.R; }
};

inline Plan level_scratch(const Frame &c, int l, Plan p) {
    p.split = c.pl.split;
    p.wino = c.ws.scratch[l];
    p.wino_bytes = c.fp.lb[l].scratch;
    return p;
}
inline int run_level(const Frame &c, int l, const Plan &p) {
    StackOpts o;
    o.flags = c.flags;
    o.step_begin = kLevels[l].begin;
    o.step_end = kLevels[l].end;
    return run_stack(c.f, c.act, c.dt, c.blob, p, c.s, o);
}
// image i * step + add is line image (index i, side) of a level with `count` lines per side
inline void line_image(const Level &lv, int side, int count, int *step, int *add) {
    *step = lv.by_side ? 1 : 2;
    *add = lv.by_side ? side * count : side;
}

// the splices that fill one tensor, gathered into one launch (a full list goes out and a new one starts)
struct SpliceList {
    hipStream_t s;
    SpliceJob job[kSpliceJobs];
    int n = 0;
    int flush() {
        const int k = n;
        n = 0;
        return k ? nd_launch_splices(job, k, s) : ND_OK;
    }
    int add(const SpliceJob &j) {
        if (n == kSpliceJobs) ND_TRY(flush());
        job[n++] = j;
        return ND_OK;
    }
};

// The line images of level l > 0 for a band of nrows tile rows, from the band (band), row (re) and column (ce) images of the level
// above: the edge line of a tile row (column), which the level above's line images produce, next to the strip - 1 clean band
// rows (columns) inside it
int splice_line_inputs(const Frame &c, int l, int nrows, const Plan &band, const Plan &re, const Plan &ce, const Plan &rows, const Plan &cols) {
    const Level &lv = kLevels[l], &up = kLevels[l - 1];
    const Buf in = lv.in;
    const int n = c.tile[in], planes = band.buf[in].planes, h = band.buf[in].Hb, w = band.buf[in].Wb;
    SpliceList jobs = {c.s};
    for (int side = 0; side < 2; ++side) {
        // (splice: "tile" t = tile row t of the band on a grid of one column / tile column t on a grid of one row)
        const int at = side * (lv.strip - 1), in0 = 1 - side, in1 = lv.strip - side;
        SpliceMap br, lr, bc, lc;
        br.step_y = bc.step_x = c.fp.S >> up.out_shift;
        br.oy = bc.ox = side * (n - lv.strip);
        line_image(up, side, nrows, &lr.img_y, &lr.img_add);
        line_image(up, side, c.fp.cols, &lc.img_x, &lc.img_add);
        lr.oy = lc.ox = -at;
        ND_TRY(jobs.add(nd_splice_job(band.buf[in], 0, rows.buf[in], 0, planes, 0, nrows, 1, 0, br, in0, in1, 0, w, 0, 0, side * nrows)));
        ND_TRY(jobs.add(nd_splice_job(re.buf[in], 0, rows.buf[in], 0, planes, 0, nrows, 1, 0, lr, at, at + 1, 0, w, 0, 0, side * nrows)));
        ND_TRY(jobs.add(nd_splice_job(band.buf[in], 0, cols.buf[in], 0, planes, 0, c.fp.cols, c.fp.cols, 0, bc, 0, h, in0, in1, 0, 0, side * c.fp.cols)));
        ND_TRY(jobs.add(nd_splice_job(ce.buf[in], 0, cols.buf[in], 0, planes, 0, c.fp.cols, c.fp.cols, 0, lc, 0, h, at, at + 1, 0, 0, side * c.fp.cols)));
    }
    return jobs.flush();
}

// Band b, level by level: its rows of tiles on the mirrored frame, the folds of the level's skips, then its line images -- top /
// bottom rows of every tile row, left / right columns of every tile column -- into slot b & 1
int build_band(const Frame &c, int b) {
    const FramePlan &fp = c.fp;
    const int row0 = b * fp.R, nrows = c.tile_rows(b), slot = b & 1;
    Plan band, re, ce;   // of the level above
    for (int l = 0; l < c.nlev; ++l) {
        const Level &lv = kLevels[l];
        Plan bp = level_scratch(c, l, band_plan(fp, l, c.f, c.dt, nrows, c.cs, c.ws.band[l], slot));
        if (l == 0)
            ND_TRY(nd_launch_gather_band(c.img, c.W, c.H, c.cs, c.ucs, c.ol, row0, bp.buf[lv.in], c.s));
        else
            bp.buf[lv.in] = band.buf[lv.in];
        ND_TRY(run_level(c, l, bp));
        for (int k = 0; k < 3; ++k)
            if (kSkips[k].level == l && c.skips[k].fold)
                ND_TRY(launch_skip_fold(c.f, c.flags, c.blob, c.bl, c.skips[k].step, c.skips[k].form, bp.buf[kSkips[k].cat], c.skip_planes(k),
                                        c.rois[c.skips[k].step], fp.S >> k, nrows, fp.cols, c.pl.split, c.ws.fold_scratch, fp.fold_bytes, c.s));
        const Plan rows = level_scratch(c, l, row_plan(fp, l, c.f, c.dt, nrows, c.ws.rows[l], slot));
        const Plan cols = level_scratch(c, l, col_plan(fp, l, c.f, c.dt, nrows, c.cs, c.ws.cols[l], slot));
        if (l == 0) {
            ND_TRY(nd_launch_gather_edges(c.img, c.W, c.H, c.cs, c.ucs, c.ol, ND_EDGE_ROWS, row0, nrows, rows.buf[lv.in], c.s));
            ND_TRY(nd_launch_gather_edges(c.img, c.W, c.H, c.cs, c.ucs, c.ol, ND_EDGE_COLS, row0, nrows, cols.buf[lv.in], c.s));
        } else {
            ND_TRY(splice_line_inputs(c, l, nrows, band, re, ce, rows, cols));
        }
        ND_TRY(run_level(c, l, rows));
        ND_TRY(run_level(c, l, cols));
        band = bp;
        re = rows;
        ce = cols;
    }
    return ND_OK;
}

// The corner patches of level l for tiles [t0, t0 + cnt), four per tile, run through the level: at level 0/1 the top-left,
// top-right, bottom-left, bottom-right kStrip x kStrip pixels of the tile's input; below, those of the tile's own assembled input tp.buf[lv.in]
int corner_patches(const Frame &c, int l, const Plan &tp, int t0, int cnt, Plan *cp) {
    const Level &lv = kLevels[l];
    *cp = level_scratch(c, l, corner_plan(l, c.f, c.dt, cnt, c.batch, c.ws.corners[l]));
    if (l == 0) ND_TRY(nd_launch_gather_edges(c.img, c.W, c.H, c.cs, c.ucs, c.ol, ND_EDGE_CORNERS, t0, cnt, cp->buf[lv.in], c.s));
    SpliceList jobs = {c.s};
    for (int k = 0; l > 0 && k < 4; ++k) {
        SpliceMap m;   // ("tile" t of a grid of one row: image t of the launch)
        m.img_t = 1;
        m.oy = (k >> 1) * (c.tile[lv.in] - lv.strip);
        m.ox = (k & 1) * (c.tile[lv.in] - lv.strip);
        ND_TRY(jobs.add(nd_splice_job(tp.buf[lv.in], 0, cp->buf[lv.in], 0, tp.buf[lv.in].planes, 0, cnt, cnt, 0, m, 0, lv.strip, 0, lv.strip, 0, 0, k * cnt)));
    }
    ND_TRY(jobs.flush());
    return run_level(c, l, *cp);
}

// The skips of a launch: per skip, the copy of its window into the tile buffer, or the second source / the addend of its decoder
// step and the table of where each tile of the launch lies in the band
int bind_skips(const Frame &c, const Plan &tp, int t0, int cnt, StepSrc2 *src2, int *nsrc2) {
    const FramePlan &fp = c.fp;
    *nsrc2 = 0;
    for (int k = 0; k < 3; ++k) {
        if (kSkips[k].level >= c.nlev) continue;
        const Buf cat = kSkips[k].cat;
        const QpBuf &src = c.full[kSkips[k].level].buf[cat];
        const int planes = c.skip_planes(k), tstep = fp.S >> k, *win = fp.win[k];
        if (!c.skips[k].in_place && !c.skips[k].fold) {
            SpliceMap m;
            m.step_y = m.step_x = tstep;
            ND_TRY(nd_launch_splice(src, planes, tp.buf[cat], planes, planes, t0, cnt, fp.cols, 0, m, win[0], win[1], win[0], win[1], c.s, fp.R,
                                    slot_elems(src, fp.slots)));
            continue;
        }
        StepSrc2 &q = src2[(*nsrc2)++];
        q.step = c.skips[k].step;
        q.buf = src;
        q.plane0 = q.from = planes;
        q.addend = c.skips[k].fold;
        if (q.addend) {   // P: the lower half, an n + 2 output inside the n + 4 bordered plane
            q.plane0 = 0;
            q.buf.pad = 1;
        }
        q.origin = c.ws.origins[k];
        ND_TRY(nd_launch_skip_origins(src, tp.buf[cat].pad, t0, cnt, fp.cols, fp.R, tstep, slot_elems(src, fp.slots), c.ws.origins[k],
                                      &q.origin_max, c.s));
    }
    return ND_OK;
}

// The output of level l in the buffers of tiles [t0, t0 + cnt): each tile's window of the band tensor, its border lines and
// corner pixels from the line images and the corner patches cp -- one splice launch
int assemble_output(const Frame &c, int l, const Plan &tp, const Plan &cp, int t0, int cnt) {
    const FramePlan &fp = c.fp;
    const Level &lv = kLevels[l];
    const QpBuf &dst = tp.buf[lv.out], &bt = c.full[l].buf[lv.out];
    const int n = c.tile[lv.out], step = fp.S >> lv.out_shift, per_band = fp.R * fp.cols;
    // The pieces are disjoint and go out as one launch: the window of the band covers [1, n - 1)^2, a row line columns [1, n - 1),
    // a column line rows [1, n - 1), and the corner pixels, which both reflections of the tile reach, stand alone.
    SpliceList jobs = {c.s};
    SpliceMap whole;
    whole.step_y = whole.step_x = step;
    // Where the level below is shared too, the tile's own copy of this output has one reader, corner_patches(l + 1): its four
    // strip x strip corner windows.  Only they are copied then (less the lines and corner pixels, which follow)
    const int strip = l + 1 < c.nlev ? kLevels[l + 1].strip : 0;
    if (strip > 0 && n >= 2 * strip) {
        for (int k = 0; k < 4; ++k) {
            const int r0 = (k >> 1) ? n - strip : 1, c0 = (k & 1) ? n - strip : 1;
            ND_TRY(jobs.add(nd_splice_job(bt, 0, dst, 0, dst.planes, t0, cnt, fp.cols, 0, whole, r0, r0 + strip - 1, c0, c0 + strip - 1, fp.R,
                                          slot_elems(bt, fp.slots))));
        }
    } else {
        ND_TRY(jobs.add(nd_splice_job(bt, 0, dst, 0, dst.planes, t0, cnt, fp.cols, 0, whole, 1, n - 1, 1, n - 1, fp.R, slot_elems(bt, fp.slots))));
    }
    // rows 0 / n - 1 and columns 0 / n - 1: the tile's window of its tile row's / tile column's lines (side 0 / 1), band by band
    // of the launch -- the column images of a short last band are shorter
    for (int b = t0 / per_band; b <= (t0 + cnt - 1) / per_band; ++b) {
        const int lo = t0 > b * per_band ? t0 : b * per_band, hi = t0 + cnt < (b + 1) * per_band ? t0 + cnt : (b + 1) * per_band;
        const int row0 = b * fp.R, nrows = c.tile_rows(b);
        const QpBuf rl = row_plan(fp, l, c.f, c.dt, nrows, c.ws.rows[l], b & 1).buf[lv.out];
        const QpBuf cl = col_plan(fp, l, c.f, c.dt, nrows, c.cs, c.ws.cols[l], b & 1).buf[lv.out];
        for (int side = 0; side < 2; ++side) {
            const int at = side * (n - 1);
            SpliceMap mr, mc;
            mr.step_x = mc.step_y = step;
            line_image(lv, side, nrows, &mr.img_y, &mr.img_add);
            line_image(lv, side, fp.cols, &mc.img_x, &mc.img_add);
            mr.oy = mc.ox = -at;
            ND_TRY(jobs.add(nd_splice_job(rl, 0, dst, 0, dst.planes, lo, hi - lo, fp.cols, row0, mr, at, at + 1, 1, n - 1, 0, 0, lo - t0)));
            ND_TRY(jobs.add(nd_splice_job(cl, 0, dst, 0, dst.planes, lo, hi - lo, fp.cols, row0, mc, 1, n - 1, at, at + 1, 0, 0, lo - t0)));
        }
    }
    for (int k = 0; k < 4; ++k) {
        const int r = (k >> 1) * (n - 1), col = (k & 1) * (n - 1);
        SpliceMap m;
        m.img_t = lv.by_side ? 1 : 4;
        m.img_add = lv.by_side ? k * cnt : k;
        m.oy = -r;
        m.ox = -col;
        ND_TRY(jobs.add(nd_splice_job(cp.buf[lv.out], 0, dst, 0, dst.planes, t0, cnt, fp.cols, 0, m, r, r + 1, col, col + 1)));
    }
    return jobs.flush();
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t nd_utnet_frame_workspace_bytes(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol,
                                                 int batch) {
    FramePlan fp;
    if (nd_check_flags(flags, true) != ND_OK || frame_plan(funit, dtype, flags, width, height, cs, ucs, ol, batch, &fp) != ND_OK) return 0;
    return fp.bytes;
}

extern "C" int nd_utnet_frame_plan(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol, int *out) {
    ND_TRY(nd_check_flags(flags, true));
    if (!out) ND_FAIL(ND_EINVAL, "nd_utnet_frame_plan: null output");
    FramePlan fp;
    ND_TRY(frame_plan(funit, dtype, flags, width, height, cs, ucs, ol, 1, &fp));
    const int v[8] = {fp.D, fp.aligned, fp.R, fp.nbands, fp.S, fp.cols, fp.rows, fp.in_h[0]};
    memcpy(out, v, sizeof(v));
    return ND_OK;
}

extern "C" int nd_utnet_frame_levels(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol, int *levels) {
    ND_TRY(nd_check_flags(flags, true));
    if (!levels) ND_FAIL(ND_EINVAL, "nd_utnet_frame_levels: null output");
    FramePlan fp;
    ND_TRY(frame_plan(funit, dtype, flags, width, height, cs, ucs, ol, 1, &fp));
    *levels = fp.levels;
    return ND_OK;
}

extern "C" int nd_utnet_frame_folds(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol, int *mask) {
    ND_TRY(nd_check_flags(flags, true));
    if (!mask) ND_FAIL(ND_EINVAL, "nd_utnet_frame_folds: null output");
    FramePlan fp;
    ND_TRY(frame_plan(funit, dtype, flags, width, height, cs, ucs, ol, 1, &fp));
    *mask = fp.folds;
    return ND_OK;
}

// the frame loop; tile_ok null: nd_utnet_denoise_frame, else nd_utnet_denoise_frame_checked -- every launch then ends in the verdict
// and the guarded stitch instead of the plain stitch, and nothing else differs
static int denoise_frame(int funit, int act, int dtype, int flags, const void *packed, const float *img, float *canvas, int width,
                         int height, int cs, int ucs, int ol, int tile_begin, int tile_count, int batch, void *ws, size_t ws_bytes, void *fws,
                         size_t fws_bytes, void *stream, nd_progress_fn progress, void *progress_ctx, unsigned char *tile_ok) {
    ND_TRY(nd_check_flags(flags, true));
    Frame c = {funit, act, dtype, flags, (const float *)packed, img, canvas, width, height, cs, ucs, ol, batch, (hipStream_t)stream};
    FramePlan &fp = c.fp;
    ND_TRY(frame_plan(funit, dtype, flags, width, height, cs, ucs, ol, batch, &fp));
    if (tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > fp.cols * fp.rows)
        ND_FAIL(ND_EINVAL, "nd_utnet_denoise_frame: tiles [%d,+%d) outside the grid of %d", tile_begin, tile_count, fp.cols * fp.rows);
    const int end = tile_begin + tile_count;
    ND_TRY(forward_common(funit, act, dtype, packed, batch, batch, cs, cs, ws, ws_bytes, &c.pl));
    c.bl = blob_layout(funit, dtype);
    const int crop = (cs - ucs) / 2;
    if (fp.D && !(plan_rois(c.pl, crop, crop, c.rois) && rois_supported(funit, dtype, flags, c.pl, c.bl, c.rois))) fp.D = 0;
    if (fp.D == 0) {   // every tile runs its whole encoder: launches of `batch` tiles from tile_begin
        int n = 0;
        for (int t0 = tile_begin; t0 < end; t0 += batch, ++n) {
            const int cnt = end - t0 < batch ? end - t0 : batch;
            if (progress) progress(progress_ctx, n, t0, cnt);
            ND_TRY(nd_utnet_denoise_tiles_ok(funit, act, dtype, flags & ~(ND_FLAG_TILE_LEVEL2 | ND_FLAG_TILE_SKIPS), packed, img, canvas, width, height, cs, ucs, ol, t0, cnt, batch, ws,
                                             ws_bytes, stream, tile_ok));
        }
        return ND_OK;
    }
    if (!img || !canvas) ND_FAIL(ND_EINVAL, "UtNet: null image");
    if (!fws || fws_bytes < fp.bytes || ((uintptr_t)fws & 255))
        ND_FAIL(ND_ENOMEM, "nd_utnet_denoise_frame: frame workspace %zu B given, %zu B needed (256-byte aligned)", fws_bytes, fp.bytes);
    c.ws = frame_ws(fp, (char *)fws);
    c.nlev = shared_levels(fp);
    c.tile = extents_from(X0, cs + 4);
    for (int l = 0; l < c.nlev; ++l) c.full[l] = band_plan(fp, l, funit, dtype, fp.R, cs, c.ws.band[l]);
    for (int k = 0; k < 3; ++k) {
        if (kSkips[k].level >= c.nlev) continue;
        Frame::Skip &sk = c.skips[k];
        sk.step = skip_step(kSkips[k].cat);
        sk.form = step_form(kSteps[sk.step], funit, dtype, flags, c.pl, c.bl);
        sk.in_place = form_takes_src2(kSteps[sk.step], sk.form, funit, flags, c.pl);
        sk.fold = ((fp.folds >> k) & 1) && sk.in_place;
    }
    const float *fw = c.blob + c.bl.off[kNumLayers - 1];
    // the rest of a tile's stack, on the useful regions
    StepSrc2 src2[3];
    StackOpts dec;
    dec.flags = flags;
    dec.step_begin = kLevels[c.nlev - 1].end;
    dec.rois = c.rois;
    dec.src2 = src2;
    // Bands are computed as the launches reach them, band b into slot b & 1 of the tensors the launches read (the output lines of
    // its row and column line images among them: a function of the frame geometry alone, as the band is); a launch takes `batch`
    // tiles across a band seam and is cut at its second seam, so it reads two slots at most.  One stream: band b + 2 overwrites
    // slot b & 1 only after the launches that read band b
    const int per_band = fp.R * fp.cols;
    int band_done = tile_begin / per_band - 1;
    for (int t0 = tile_begin, n = 0; t0 < end; ++n) {
        const int b0 = t0 / per_band;
        int cnt = end - t0 < batch ? end - t0 : batch;
        if (t0 + cnt > (b0 + 2) * per_band) cnt = (b0 + 2) * per_band - t0;
        for (; band_done < (t0 + cnt - 1) / per_band; ++band_done) ND_TRY(build_band(c, band_done + 1));
        if (progress) progress(progress_ctx, n, t0, cnt);
        const Plan tp = make_plan(funit, cs, cs, batch, cnt, (char *)ws, dtype);
        Plan cp;
        ND_TRY(corner_patches(c, 0, tp, t0, cnt, &cp));
        ND_TRY(bind_skips(c, tp, t0, cnt, src2, &dec.nsrc2));
        ND_TRY(assemble_output(c, 0, tp, cp, t0, cnt));
        for (int l = 1; l < c.nlev; ++l) {
            ND_TRY(corner_patches(c, l, tp, t0, cnt, &cp));
            ND_TRY(assemble_output(c, l, tp, cp, t0, cnt));
        }
        ND_TRY(run_stack(funit, act, dtype, c.blob, tp, c.s, dec));
        ND_TRY(nd_launch_utnet_stitch(tp.buf[T4B], funit, fw, fw + 3 * funit, canvas, width, height, cs, ucs, ol, t0, cnt, tile_ok, c.s));
        t0 += cnt;
    }
    return ND_OK;
}

extern "C" int nd_utnet_denoise_frame(int funit, int act, int dtype, int flags, const void *packed, const float *img, float *canvas,
                                      int width, int height, int cs, int ucs, int ol, int tile_begin, int tile_count, int batch,
                                      void *ws, size_t ws_bytes, void *fws, size_t fws_bytes, void *stream, nd_progress_fn progress,
                                      void *progress_ctx) {
    return denoise_frame(funit, act, dtype, flags, packed, img, canvas, width, height, cs, ucs, ol, tile_begin, tile_count, batch, ws, ws_bytes,
                         fws, fws_bytes, stream, progress, progress_ctx, nullptr);
}

extern "C" int nd_utnet_denoise_frame_checked(int funit, int act, int dtype, int flags, const void *packed, const float *img, float *canvas,
                                              int width, int height, int cs, int ucs, int ol, int tile_begin, int tile_count, int batch,
                                              void *ws, size_t ws_bytes, void *fws, size_t fws_bytes, void *stream,
                                              nd_progress_fn progress, void *progress_ctx, unsigned char *tile_ok) {
    if (!tile_ok) ND_FAIL(ND_EINVAL, "nd_utnet_denoise_frame_checked: null tile_ok");
    return denoise_frame(funit, act, dtype, flags, packed, img, canvas, width, height, cs, ucs, ol, tile_begin, tile_count, batch, ws, ws_bytes,
                         fws, fws_bytes, stream, progress, progress_ctx, tile_ok);
}
