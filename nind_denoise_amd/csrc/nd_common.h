// Internal declarations shared by the translation units of libnind_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "nind_hip.h"

// ------------------------------------------------------------------ errors
void nd_set_error(const char *fmt, ...);
#define ND_FAIL(code, ...)        \
    do {                          \
        nd_set_error(__VA_ARGS__); \
        return (code);            \
    } while (0)
#define ND_HIP(call)                                                                         \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) ND_FAIL(ND_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)
#define ND_TRY(call)        \
    do {                    \
        int r_ = (call);    \
        if (r_ != 0) return r_; \
    } while (0)

// ------------------------------------------------------------------ tile geometry and its two index maps (aux_kernels.hip)
// Grid constants of OneImageDS (denoise_image.py:100-104), filled and checked by make_geo: a geometry that passes folds a tile
// coordinate over a frame edge at most once.
struct TileGeo {
    int W, H, cs, ucs, ol, pad, stride, cols, rows;
};
__host__ __device__ static inline int ceil_div_py(int a, int b) {  // math.ceil(a / b) for b > 0, any sign of a
    return a >= 0 ? (a + b - 1) / b : -((-a) / b);
}
__host__ __device__ static inline int mirror_sym(int v, int n) {  // edge pixel repeated (np.flip of the adjacent band)
    return v < 0 ? -1 - v : (v >= n ? 2 * n - 1 - v : v);
}
// Gather map (OneImageDS.__getitem__, denoise_image.py:138-170): pixel (y, x) of tile i shows frame pixel (*Y, *X).  The gather
// kernel, its adjoint and nd_tile_source are this one function.
__host__ __device__ static inline void nd_tile_source_map(const TileGeo &g, int i, int y, int x, int *Y, int *X) {
    const int yi = i / g.cols, xi = i - yi * g.cols;
    *X = mirror_sym(xi * g.stride - g.pad + x, g.W);
    *Y = mirror_sym(yi * g.stride - g.pad + y, g.H);
}
// Stitch map (useful crop of nd_tile_geom + make_seamless_edges, denoise_image.py:204-213, 249-267): pixel (y, x) of tile i is added
// to canvas pixel (*Y, *X) with the returned weight -- 0 outside the useful crop (then *Y, *X name no pixel), else halved once per
// condition of make_seamless_edges that holds: 1, 1/2 or 1/4 wherever the two strips of an axis do not meet.  The adjoint of the
// stitch and nd_stitch_weight are this function; k_stitch_add walks the same map from the canvas pixel's side (for_each_cover).
__host__ __device__ static inline float nd_stitch_weight_map(const TileGeo &g, int i, int y, int x, int *Y, int *X) {
    const int yi = i / g.cols, xi = i - yi * g.cols;
    const int ax = xi * g.stride, ay = yi * g.stride;              // usefulstart
    const int x1pad = ax - g.pad + g.cs - g.W > 0 ? ax - g.pad + g.cs - g.W : 0;
    const int y1pad = ay - g.pad + g.cs - g.H > 0 ? ay - g.pad + g.cs - g.H : 0;
    const int uw = g.cs - (g.pad > x1pad ? g.pad : x1pad) - g.pad;
    const int uh = g.cs - (g.pad > y1pad ? g.pad : y1pad) - g.pad;
    const int dx = x - g.pad, dy = y - g.pad;
    *X = ax + dx;
    *Y = ay + dy;
    if (dx < 0 || dx >= uw || dy < 0 || dy >= uh) return 0.f;
    float f = 1.f;
    if (ax != 0 && dx < g.ol) f *= 0.5f;
    if (ay != 0 && dy < g.ol) f *= 0.5f;
    if (ax + g.ucs < g.W && g.ol && dx >= uw - g.ol) f *= 0.5f;
    if (ay + g.ucs < g.H && g.ol && dy >= uh - g.ol) f *= 0.5f;
    return f;
}

// ------------------------------------------------------------------ deterministic sums
// Sum of v over the 256 threads of a workgroup through `red` (256 elements of LDS): a fixed tree, the same bits on every run.
// T: float, double, or a vector of them (added component by component).  Every thread gets the total; `red` is free again
// after the next __syncthreads().
template <typename T>
__device__ inline T nd_block_sum(T v, T *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    return red[0];
}
// out[0] = scale * sum partial[0..n): one workgroup, fixed order (aux_kernels.hip)
int nd_launch_sum(const float *partial, int n, float scale, float *out, hipStream_t s);

// ------------------------------------------------------------------ the window the criteria see (criteria.hip)
// The centre Lh x Lw window of an h x w image at (oy, ox): loss_cs x loss_cs at ((h - loss_cs) / 2, (w - loss_cs) / 2), or the
// whole image for loss_cs = 0 (pt_ops.pt_crop_batch, nn_train.py:319-323).
struct LossWindow {
    int Lh, Lw, oy, ox;
};
// The one argument check of the criteria entry points and of the training step (`who`: the error prefix): n and the sides in
// range, loss_cs within the image, a window of at least 11 pixels for SSIM and 161 for MS-SSIM.  Fills *win on success.
int nd_loss_window(const char *who, int n, int h, int w, int loss_cs, bool ssim, bool msssim, LossWindow *win);

// ------------------------------------------------------------------ quad-planar activation buffers
// An activation tensor [B, C, H, W] lives in HBM as C/4 planes of float4 "channel quads":
//     plane q, image b, row y, col x  ->  float4 at  ((q * B + b) * Hb + y + pad) * Wb + x + pad
// where Hb = H + 2*pad, Wb = W + 2*pad and pad is the zero border the CONSUMER needs
// (2 when the consumer is a ConvTranspose2d(3): it then is a plain valid 3x3 correlation on the bordered buffer).
// Within a plane all images are contiguous, so a pixel has ONE linear index p = (b*Hb + y)*Wb + x and the 3x3
// neighbour (ky,kx) is p + ky*Wb + kx: an implicit-GEMM N tile is a contiguous pixel range and its LDS halo
// image is a contiguous copy.
// A plane element is ALWAYS 16 bytes per pixel: 4 fp32 channels (ND_F32) or 8 bf16 / fp16 channels (ND_BF16 / ND_F16),
// so the pixel indexing, the LDS-DMA images and the ds_read_b128 fragment reads are identical for every storage type.
static inline int nd_cpp(int dt) { return dt == ND_F32 ? 4 : 8; }   // channels per plane
struct QpBuf {
    float *base;    // first plane
    int planes;     // C / nd_cpp(dt) (channels padded to a whole plane)
    int B, Hb, Wb;  // images in use, bordered rows / cols
    int pad;        // zero border width
    long pstride;   // 16-byte elements per plane (capacity: batch * Hb * Wb); B may be smaller for a partial batch
    int dt = ND_F32;  // storage type (nd_dtype)
    long np() const { return pstride; }
    long used() const { return (long)B * Hb * Wb; }
};

// ------------------------------------------------------------------ one conv launch
struct ConvDesc {
    int kind = ND_CONV3;        // nd_layer_kind
    int act = ND_ACT_NONE;      // nd_act
    float slope = 1.f;          // PReLU slope (used when slope_dev is null)
    const float *slope_dev = nullptr;  // PReLU slope in HBM (the packed blob), or null
    const float *wpk = nullptr;   // packed weights [mtile][kb][tap][64 lanes][4]
    const float *bias = nullptr;  // [mtiles*32]
    int cin = 0, cout = 0;      // logical channels (cin is padded to 8 in the buffers)
    QpBuf in = {};              // bordered input (for CONVT3 its border supplies the implicit zero padding)
    QpBuf out = {};             // destination buffer (possibly a concat buffer)
    int out_plane0 = 0;         // first destination plane (channel offset / 4) inside `out`
    int variant = -1;           // -1: pick automatically
    int in_plane0 = 0;  // first input plane inside `in` (a channel slice of a concat / gradient buffer)
    float *pre = nullptr;   // training: also store the pre-activation (acc + bias), compact [C/4][B][Hv][Wv] float4 planes
    long pre_plane = 0;     // 16-byte elements per plane of `pre`
    float *part = nullptr;  // scratch for the split-K tail (raw accumulators of K slices); null: never split
    size_t part_bytes = 0;
    bool nosplit = false;   // ND_FLAG_NO_SPLITK of the call: keep every tile whole (bits independent of the launch composition)
    bool tile_wino = false;  // ND_FLAG_TILE_WINO of the call: a three-pass layer tiles every image on its own (no mosaic, winograd.hip)
    int nbatch = 1;         // independent problems of this shape in one launch (Winograd positions)
    long in_bs = 0, out_bs = 0;   // 16-byte elements between consecutive problems' input / output buffers
    size_t w_bs = 0;        // floats between consecutive problems' packed weights (the bias is shared)
    // fused MaxPool2d(2) (fp32 inference: conv_w2d.hip / winograd.hip; 16-bit storage: conv_qp): the layer also writes max over 2x2 blocks of its activated
    // output into planes [0, cout/4) of `pool` (UtNet.py:99-105: every pooled tensor is a conv output that is also a skip)
    const QpBuf *pool = nullptr;
    // region of interest (rows == 0: the whole layer).  3x3 layers (conv_w2d, three-pass F(6x6)): rectangle [r0, r0 + rows) x
    // [c0, c0 + cols) of the valid OUTPUT grid -- only these outputs are computed and stored, from input rows [r0, r0 + rows + 2);
    // 2x2 stride-2 transpose: rectangle of the INPUT grid (each input pixel makes its 2x2 outputs).  Used by the fused denoise
    // loop: the last decoder levels only compute what the useful crop of a tile can reach (utnet_net.h: plan_rois)
    int roi_r0 = 0, roi_c0 = 0, roi_rows = 0, roi_cols = 0;
    // second input source (in2.base null: none; conv_w2d and the three-pass F(6x6) form): input planes [in2_from, 2 KB) of `in`
    // are not read from `in` but from planes in2_plane0 + (k - in2_from) of `in2`, where bordered pixel (y, x) of image t is element
    // in2_origin[t] + y * in2.Wb + x of the plane.  The fused denoise loop reads the skip half of a concat straight from the
    // band tensor the shared encoder wrote (origins: nd_launch_skip_origins).  in2_origin lives in HBM, one entry per image of the
    // launch; in2_origin_max bounds its entries (the launcher checks the furthest read against in2 and its slack with it)
    QpBuf in2 = {};
    int in2_plane0 = 0, in2_from = 0;
    const int *in2_origin = nullptr;
    long in2_origin_max = 0;
    // K-block sub-range of the packed weights (w_kb 0: the blob is the launch's own; conv_w2d): the launch's cin channels are K blocks
    // [w_kb0, w_kb0 + cin / 8) of a blob packed for w_kb K blocks -- the M-tile stride of the blob is w_kb, not the launch's K extent.
    // The fused denoise loop runs the two halves of a decoder level's first layer apart: the up-sampled half per tile, the skip half
    // once per band
    int w_kb = 0, w_kb0 = 0;
    // addend source (add.base null: none; conv_w2d): the epilogue computes act(acc + addend) instead of act(acc + bias), where the
    // addend of output pixel (y, x) of image t, channel quad q, is element add_origin[t] + (y + add.pad) * add.Wb + x + add.pad of
    // plane add_plane0 + q of `add`.  Shaped like in2: add_origin lives in HBM, one entry per image of the launch, add_origin_max bounds
    // its entries.  The fused denoise loop adds the skip half's product P = W_skip * skip + b, computed once per band
    QpBuf add = {};
    int add_plane0 = 0;
    const int *add_origin = nullptr;
    long add_origin_max = 0;
};
// the furthest element (exclusive) of a plane of d.in2 a launch may touch stays inside the buffer and its slack: `reach` = elements
// past an image's origin (its window in the layer's bordered input, the kernel's over-read included)
int nd_check_in2(const char *who, const ConvDesc &d, int KB, long reach);
// the same for d.add: `reach` = elements past an image's origin of the furthest addend element the launch's valid output grid touches
int nd_check_add(const char *who, const ConvDesc &d, long reach);
// scratch that lets every layer split its partial round: 512 work items of 64 x 1024 accumulators
static const size_t kSplitScratchBytes = (size_t)512 * 64 * 1024 * 4;
int nd_launch_conv(const ConvDesc &d, hipStream_t stream);
bool nd_conv_pool_fits(const ConvDesc &d);  // a 16-bit 3x3 launch with d.pool set can pool in its epilogue (else: nd_launch_maxpool2 after it)
bool nd_conv_roi_fits(const ConvDesc &d);   // a launch restricted to d.roi_* finds a workgroup shape that fits the LDS
int nd_conv_variant_count();
int nd_conv_variant_gemm(int cin, int cout);   // 1-tap fp32 variant (256- / 128-row workgroup tiles) for a Winograd GEMM
// Winograd F(T x T, 3 x 3), T = 2 | 4 (winograd.hip): fp32 inference path of the wide 3x3 layers
size_t nd_wino_packed_floats(int T, int cin, int cout);
int nd_wino_pack(int T, int kind, int cin, int cout, const float *w, const float *bias, float *packed);
size_t nd_wino_scratch_bytes(int T, const QpBuf &in, int cin, int cout);
// ev2 (optional, profiling): two events, recorded after the input transform pass and after the GEMM launch
int nd_launch_conv_wino(int T, const ConvDesc &d, void *scratch, size_t scratch_bytes, hipStream_t s, hipEvent_t *ev2 = nullptr);
// F(T x T) tiles the launch of d runs: per image, or those of the mosaic where the launch takes one (nd_wino_mosaic)
long nd_wino_launch_tiles(int T, const ConvDesc &d);
// algorithmic HBM bytes of the two transform passes of a three-pass layer (X read + V written; M read + Y written); tiles: what its
// launches ran (nd_wino_launch_tiles; 0: per-image grids)
void nd_wino_xform_bytes(int T, const QpBuf &in, int cin, int cout, long tiles, double *bytes_in, double *bytes_out);
// the tiles both networks' executors run the Winograd forms at (measurements: utnet_net.h)
constexpr int kWinoTile = 6;     // three-pass F(6x6,3x3)
constexpr int kW1dTile = 4;      // fused F(4,3)
constexpr int kWinoChunk = 256;  // images per three-pass Winograd pass: bounds the V / M scratch
// 1-D Winograd F(2,3) along x inside the implicit-GEMM kernel (conv_w1d.hip): fp32 inference form of the narrow 3x3 layers
// (T = 2: F(2,3), 2/3 of the MFMAs;  T = 4: F(4,3), 1/2)
size_t nd_w1d_packed_floats(int T, int cin, int cout);
int nd_w1d_pack(int T, int kind, int cin, int cout, const float *w, const float *bias, float *packed);
bool nd_w1d_fits(int T, const QpBuf &in);
int nd_launch_conv_w1d(int T, const ConvDesc &d, hipStream_t stream);
// the same F(4,3) layer with the input transform shared by the workgroup through LDS (conv_w2d.hip; same packed weights as T = 4)
bool nd_w2d_ok(const QpBuf &in);
long nd_w2d_tiles(const QpBuf &in, int cout);   // workgroup tiles of the whole layer
int nd_launch_conv_w2d(const ConvDesc &d, hipStream_t stream);
// an F(4,3) layer (d.wpk: nd_w1d_pack blob with T = 4) in conv_w2d where it takes the layer, else in conv_w1d (flags: nd_flags)
bool nd_f43_w2d(const QpBuf &in, int cout, bool pre, int flags);
int nd_launch_conv_f43(const ConvDesc &d, int flags, hipStream_t stream);
// slack (16-byte elements) behind the last plane of an activation buffer: an N tile of the conv kernels may read a 3x3 halo past
// the last pixel, a strip of conv_w2d up to 9 rows + 5 pixels
static inline size_t nd_buf_slack(int Wb) { return (size_t)10 * Wb + 8 + 2048; }
// ------------------------------------------------------------------ per-device launch state (launch.hip)
// Entry points may be called from several host threads (include/nind_hip.h).  These calls are safe to race: the CU count is
// queried once per device, and a kernel's dynamic-LDS limit is checked and raised under one lock, so it only ever grows.
// current device (0 <= dev < 16) and, if ncus is given, its CU count
int nd_device(int *dev, int *ncus = nullptr);
// lets kernel fn use `bytes` of dynamic LDS on device dev; no HIP call once the limit is large enough
int nd_raise_lds(int dev, const void *fn, size_t bytes);
// runs init() once per device (the first caller on a device runs it; the others wait until it has succeeded)
int nd_once_per_device(int dev, int (*init)());
// checks of a conv layer; `who` is the launcher's error prefix.  Input planes [in_plane0, in_plane0 + 2 KB) exist; a launcher
// that does not take a second input source (takes_in2), or an addend / a K-block sub-range of the weights (takes_add), refuses a
// layer that has one
int nd_check_in_planes(const char *who, const ConvDesc &d, int KB, bool takes_in2 = false, bool takes_add = false);
// the destination holds B images of oh x ow plus its border (at_least: or more) and planes [out_plane0, out_plane0 + cout / cpp)
int nd_check_out(const char *who, const ConvDesc &d, int oh, int ow, bool at_least);
// the linear pixel index of `in` fits int32
int nd_check_int32(const char *who, const QpBuf &in);
// d's region of interest (if any) lies inside the Hv x Wv grid; refused: the launcher takes no region for this layer (`why`)
int nd_check_roi(const char *who, const ConvDesc &d, int Hv, int Wv, bool refused, const char *why);
// the arithmetic switches every flags-taking entry point accepts (include/nind_hip.h: nd_flags); unknown bits are an error.
// frame_loop: the frame-loop entry points (nd_utnet_frame_*, nd_utnet_denoise_frame) also take ND_FLAG_TILE_LEVEL2 and
// ND_FLAG_TILE_SKIPS, which mean nothing anywhere else; unet_frame: nd_unet_denoise_frame also takes ND_FLAG_FIND_NOISE; unet_wino:
// the UNet inference entry points also take ND_FLAG_UNET_WINOGRAD
static inline int nd_check_flags(int flags, bool frame_loop = false, bool unet_frame = false, bool unet_wino = false) {
    const int known = ND_FLAG_NO_SPLITK | ND_FLAG_DIRECT_CONV | ND_FLAG_W1D_REGS | ND_FLAG_FULL_TILES | ND_FLAG_UNFUSED_POOL |
                      ND_FLAG_TILE_ENCODER | ND_FLAG_TILE_WINO | (frame_loop ? ND_FLAG_TILE_LEVEL2 | ND_FLAG_TILE_SKIPS : 0) | (unet_frame ? ND_FLAG_FIND_NOISE : 0) |
                      (unet_wino ? ND_FLAG_UNET_WINOGRAD : 0);
    if (flags & ~known) ND_FAIL(ND_EINVAL, "unknown flag bits 0x%x", flags);
    return ND_OK;
}
const char *nd_conv_variant_label(int v);

// packed size helpers (host)
// 32-row MFMA tiles, padded so that every workgroup shape (M_blk <= 128, 256 for the 2x2 stride-2 layers) reads packed rows only
static inline int nd_mtiles(int kind, int cout) {
    return kind == ND_CONVT2S2 ? (4 * cout + 255) / 256 * 8 : (cout + 127) / 128 * 4;   // up layers use 256-row workgroup tiles
}
// Row order of the GEMM of a 2x2 stride-2 transpose (M = 4 * Cout rows; weights and bias are packed in it, the conv epilogue
// and k_split_finish decode it).  An MFMA accumulator hands lane (pixel j, half h) the rows 8g + 4h + e (e = 0..3) of a 32-row
// tile.  The order puts the SAME channels of the two horizontally adjacent output pixels (2x, 2x + 1) into the two lane
// halves, so that a wave's store instruction writes 64 consecutive 16-byte plane elements (1 KiB contiguous) instead of 16-byte
// pieces at a 32-byte stride:
//   fp32   (4 channels per plane element):  m = 8 * (a * Cout/4 + quad) + 4 * b + e          co = 4 * quad + e
//   16-bit (8 channels per plane element):  m = 16 * (a * Cout/8 + oct) + 8 * b + e8         co = 8 * oct + e8
//          (there the epilogue first exchanges the halves of two 8-row groups, v_permlane32_swap, so that a lane owns all 8
//           channels of one pixel)
// (a, b) = output sub-position (row, column) of ConvTranspose2d(2, stride 2): out[2y + a][2x + b].
struct NdUpRow { int a, b, co; };
__host__ __device__ static inline NdUpRow nd_up_row(int m, int cout, int dt) {
    NdUpRow r;
    const int cpp = dt == ND_F32 ? 4 : 8, q = cout / cpp;
    const int G = m / (2 * cpp), e = m % cpp;
    r.b = (m / cpp) & 1;
    r.a = G / q;
    r.co = cpp * (G % q) + e;
    return r;
}
static inline int nd_taps(int kind) { return (kind == ND_CONV3 || kind == ND_CONVT3) ? 9 : (kind == ND_CONV2S2 ? 4 : 1); }
// K block = two planes = the K extent of one ds_read_b128 per operand: 8 fp32 channels or 16 bf16/fp16 channels
static inline int nd_kblocks(int cin, int dt = ND_F32) { return (cin + 2 * nd_cpp(dt) - 1) / (2 * nd_cpp(dt)); }
// float offset of the fp32 bias inside a packed layer: behind the 1 KiB weight fragments [mtile][kb][plane] -- nd_taps(kind) planes
// per K block in the direct packing, 3 * (T + 2) in the 1-D Winograd F(T,3) packing (w1d_T = T; fp32, 3x3 kinds)
static inline size_t nd_bias_offset(int kind, int cin, int cout, int dt = ND_F32, int w1d_T = 0) {
    return (size_t)nd_mtiles(kind, cout) * nd_kblocks(cin, dt) * (w1d_T ? 3 * (w1d_T + 2) : nd_taps(kind)) * 256;
}
// packed layer size in 4-byte units: 1 KiB fragment pieces [mtile][kb][tap] (any dtype) + fp32 bias[mtiles*32]
static inline size_t nd_packed_floats(int kind, int cin, int cout, int dt = ND_F32) {
    return nd_bias_offset(kind, cin, cout, dt) + (size_t)nd_mtiles(kind, cout) * 32;
}
void nd_pack_layer(int kind, int cin, int cout, int dt, const float *w, const float *bias, float *packed);

// device-side packers (pack_dev.hip): the same layouts from weights in HBM (direct form: any storage type; Winograd forms: fp32)
// scale (nullable, HBM): one factor per output channel, multiplied into its weights as they are packed
int nd_pack_layer_device(int kind, int cin, int cout, int dt, const float *w, const float *bias, float *packed, hipStream_t s,
                         const float *scale = nullptr);
// eval-mode BatchNorm2d folded into the conv before it: scale[co] = g / sqrt(rv + 1e-5), fbias[co] = (b - rm) * scale + be, rounded
// operation by operation as the host packer of unet.hip does
int nd_launch_bn_fold(int cout, const float *b, const float *g, const float *be, const float *rm, const float *rv, float *scale,
                      float *fbias, hipStream_t s);
// Winograd forms.  scale: as above (each weight times its channel's factor, rounded once, before the transform).  host_bits: the
// transform in double, operation by operation as nd_w1d_pack / nd_wino_pack evaluate it -- the host packer's bytes (the default
// evaluates it in fp32: ~1e-7 relative off them)
int nd_pack_w1d_device(int T, int kind, int cin, int cout, const float *w, const float *bias, float *packed, hipStream_t s,
                       const float *scale = nullptr, bool host_bits = false);
int nd_pack_wino_device(int T, int kind, int cin, int cout, const float *w, const float *bias, float *packed, hipStream_t s,
                        const float *scale = nullptr, bool host_bits = false);

// ------------------------------------------------------------------ auxiliary kernels (aux_kernels.hip)
int nd_launch_nchw_to_qp(const float *x, int C, const QpBuf &dst, int plane0, hipStream_t s);
int nd_launch_qp_to_nchw(const QpBuf &src, int plane0, float *y, int C, hipStream_t s);
int nd_launch_reflect_pack(const float *x_nchw, int B, int H, int W, const QpBuf &dst, hipStream_t s);
int nd_launch_maxpool2(const QpBuf &src, int src_plane0, int planes, const QpBuf &dst, hipStream_t s);
int nd_launch_final1x1(const QpBuf &src, int cin, const float *w, const float *bias, int crop, float *y_nchw, int H,
                       int W, hipStream_t s, int sigmoid = 0);
// sigmoid: the UNet head; noise_img (nullable): the frame -- a tile then contributes frame pixel - result (UNet's find_noise: the
// useful part of a tile is never mirrored, so its input pixel there is the frame pixel)
int nd_launch_final1x1_stitch(const QpBuf &src, int cin, const float *w, const float *bias, int crop, float *canvas,
                              int width, int height, int cs, int ucs, int ol, int tile_begin, int tile_count,
                              hipStream_t s, int sigmoid = 0, const float *noise_img = nullptr);
// The checked frame loop (nd_utnet_denoise_frame_checked).  tile_ok: HBM, one byte per tile of the grid, indexed by the global tile
// index.  nd_launch_tile_verdict clears the flag of every tile of the launch for which the stitch would add a value that is not
// finite (k_tile_verdict evaluates the 1x1 on the tile's useful rectangle); nd_launch_final1x1_stitch_ok is the stitch above
// (UtNet head: no sigmoid, no noise image) that skips the tiles whose flag is 0 and leaves a pixel no good tile covers unwritten
int nd_launch_tile_verdict(const QpBuf &src, int cin, const float *w, const float *bias, int crop, int width, int height, int cs, int ucs,
                           int ol, int tile_begin, int tile_count, unsigned char *tile_ok, hipStream_t s);
int nd_launch_final1x1_stitch_ok(const QpBuf &src, int cin, const float *w, const float *bias, int crop, float *canvas, int width,
                                 int height, int cs, int ucs, int ol, int tile_begin, int tile_count, const unsigned char *tile_ok,
                                 hipStream_t s);
// the verdict + guarded stitch where tile_ok is given, the plain stitch where it is null: the one tail of the UtNet frame launches
static inline int nd_launch_utnet_stitch(const QpBuf &src, int cin, const float *w, const float *bias, float *canvas, int width, int height,
                                         int cs, int ucs, int ol, int tile_begin, int tile_count, unsigned char *tile_ok, hipStream_t s) {
    if (!tile_ok) return nd_launch_final1x1_stitch(src, cin, w, bias, 2, canvas, width, height, cs, ucs, ol, tile_begin, tile_count, s);
    ND_TRY(nd_launch_tile_verdict(src, cin, w, bias, 2, width, height, cs, ucs, ol, tile_begin, tile_count, tile_ok, s));
    return nd_launch_final1x1_stitch_ok(src, cin, w, bias, 2, canvas, width, height, cs, ucs, ol, tile_begin, tile_count, tile_ok, s);
}
// nd_utnet_denoise_tiles with the flags of the checked loop (utnet.hip; tile_ok null: the plain launch)
int nd_utnet_denoise_tiles_ok(int funit, int act, int dtype, int flags, const void *packed, const float *img, float *canvas, int width,
                              int height, int cs, int ucs, int ol, int tile_begin, int tile_count, int batch, void *ws, size_t ws_bytes,
                              void *stream, unsigned char *tile_ok);
// gather (+symmetric mirror) of tiles into plane 0 of a first-layer input of (cs + 2 * border)^2.  reflect: the border is
// ReflectionPad2d(border) of the tile (UtNet); else only the interior is written and the border stays as it is (UNet: zero)
int nd_launch_gather_pack(const float *img, int width, int height, int cs, int ucs, int ol, int tile_begin,
                          int tile_count, const QpBuf &dst, hipStream_t s, int border = 2, bool reflect = true);
// shared encoder of the fused loop (fp32): band of tile rows from band_row0 as one first-layer input image (B = 1, no reflect
// border); the images that yield P2's border lines (k_gather_edges: two row edges per tile row of a band, two column edges per
// tile column of a band, four corners per tile of a launch); per-tile copy of a window of a band or edge tensor into a tile buffer
// (see k_splice_jobs)
int nd_launch_gather_band(const float *img, int width, int height, int cs, int ucs, int ol, int band_row0, const QpBuf &dst,
                          hipStream_t s);
enum nd_edge_set { ND_EDGE_ROWS = 0, ND_EDGE_COLS = 1, ND_EDGE_CORNERS = 2 };
int nd_launch_gather_edges(const float *img, int width, int height, int cs, int ucs, int ol, int set, int first, int count,
                           const QpBuf &dst, hipStream_t s);
// table[t] = where bordered pixel (0, 0) of tile tile_begin + t's buffer (border dst_pad) lies inside a plane of band tensor `src`
// at a level with tile stride `step`: (band & 1) * slot_elems + ((yi - row0) * step + src.pad - dst_pad) * src.Wb + xi * step +
// src.pad - dst_pad, with (yi, xi) = the tile's grid position, band = yi / band_rows its band and row0 = band * band_rows that
// band's first tile row.  Written on the stream (no host-to-device copy); *origin_max = the largest entry
int nd_launch_skip_origins(const QpBuf &src, int dst_pad, int tile_begin, int tile_count, int cols, int band_rows, int step, long slot_elems,
                           int *table, long *origin_max, hipStream_t s);
// where tile t of a splice launch, at grid position (yi, xi) and yrel tile rows into its band, reads in the source: image
// img_t * t + img_y * yrel + img_x * xi + img_add, its region shifted by (yrel * step_y + oy, xi * step_x + ox).  A band tensor: one
// image, both steps = the tile stride at its level; the row / column edge lines: one step and img_y / img_x = 2; corners: img_t = 4
struct SpliceMap {
    int step_y = 0, step_x = 0, img_t = 0, img_y = 0, img_x = 0, img_add = 0, oy = 0, ox = 0;
};
int nd_launch_splice(const QpBuf &src, int src_p0, const QpBuf &dst, int dst_p0, int planes, int tile_begin, int tile_count, int cols,
                     int row0, const SpliceMap &m, int r0, int r1, int c0, int c1, hipStream_t s, int band_rows = 0,
                     long slot_elems = 0, int dst_img0 = 0);
// the same copy as one job of a launch of several (k_splice_jobs): every job is checked as nd_launch_splice checks its one, and jobs
// whose destination regions overlap are refused (ND_EINVAL) -- the order of the jobs of a launch means nothing
struct SpliceJob {
    QpBuf src, dst;
    int src_p0, dst_p0, planes, tile_begin, tile_count, cols, row0;
    SpliceMap m;
    int r0, r1, c0, c1, band_rows;
    long slot_elems;
    int dst_img0;
};
constexpr int kSpliceJobs = 16;
static inline SpliceJob nd_splice_job(const QpBuf &src, int src_p0, const QpBuf &dst, int dst_p0, int planes, int tile_begin, int tile_count,
                                      int cols, int row0, const SpliceMap &m, int r0, int r1, int c0, int c1, int band_rows = 0,
                                      long slot_elems = 0, int dst_img0 = 0) {
    return SpliceJob{src, dst, src_p0, dst_p0, planes, tile_begin, tile_count, cols, row0, m, r0, r1, c0, c1, band_rows, slot_elems, dst_img0};
}
int nd_launch_splices(const SpliceJob *jobs, int n, hipStream_t s);

// ------------------------------------------------------------------ gradient kernels shared by the two networks' backward passes
// (wgrad.hip, train.hip, utnet_train.hip, unet_grad.hip): no atomics, fixed summation order
// dst (its own grid) = zeros except dst[c][img][y + oy][x + ox] = src[c][img][y * ss + sy][x * ss + sx] for y < h, x < w (interior coordinates)
int nd_launch_repitch(const QpBuf &src, int src_plane0, int planes, int ss, int sy, int sx, const QpBuf &dst, int oy, int ox, int h, int w,
                      hipStream_t s);
size_t nd_wgrad_partial_floats(int taps, int M, int N, long K, int *ksplit_out, int *cps_out);
int nd_launch_wgrad(const QpBuf &A, int a_plane0, int M, const QpBuf &Bq, int b_plane0, int N, int taps, int taps_total, int tap0,
                    float *partial, size_t partial_floats, float *dw, hipStream_t s);
// out[c] = sum over the interior of planes [plane0, ...) of src; scratch: 4 * ceil(C/4) * B floats
int nd_launch_channel_sum(const QpBuf &src, int plane0, int C, float *out, float *scratch, hipStream_t s);
int nd_launch_maxpool_bwd_add(const QpBuf &gpool, const QpBuf &fwd, int fwd_plane0, const QpBuf &gfine, int g_plane0, int planes,
                              hipStream_t s);
int nd_launch_final_wgrad(const float *gy, int H, int W, const QpBuf &act, int cin, int crop, float *red, float *dw, float *db,
                          hipStream_t s);
int nd_launch_final_bwd_data(const float *gy, int H, int W, const float *w, int cin, int crop, const QpBuf &g, hipStream_t s);

// ------------------------------------------------------------------ BatchNorm on the statistics of the batch (unet_bn.hip)
// z: the pre-norm conv output (no border), a / g: the layer's activation / gradient buffer from plane0, stat: 3 * cout floats the
// forward leaves for the backward, red: reduction scratch of red_floats floats, coef: 2 * cout floats.
// forward: statistics of z -> stat, running statistics rm / rv moved by momentum, a = ReLU(gamma xhat + beta)
int nd_launch_bn_train_fwd(const QpBuf &z, const QpBuf &a, int plane0, int cout, float momentum, const float *gamma, const float *beta,
                           float *rm, float *rv, float *stat, float *red, long red_floats, hipStream_t s);
// backward: g_a -> g_z in place in g; dgamma / dbeta (nullable together) get the BatchNorm's parameter gradients
int nd_launch_bn_train_bwd(const QpBuf &g, const QpBuf &a, int plane0, const QpBuf &z, int cout, const float *gamma, const float *stat,
                           float *coef, float *dgamma, float *dbeta, float *red, long red_floats, hipStream_t s);
