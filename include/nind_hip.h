/* nind_hip.h -- C ABI of libnind_hip.so: the MI355X (gfx950) native tiled-denoise hot path.
 *
 * The reference (esq4/nind-denoise) is pure Python on torch and has NO native ABI; every entry point
 * below therefore cites the reference Python interface it stands in for (paths relative to
 * /root/reference/src/nind_denoise/).  The host side (the nind_denoise_amd Python package) binds these with ctypes;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success and a negative nd_status on failure; nd_last_error() returns a
 *     thread-local human-readable message for the last failure on the calling thread.
 *   - device pointers are plain `void*`/`float*` into HBM owned by the caller (torch's caching allocator);
 *     the library borrows them for the duration of the call, allocates nothing and frees nothing.
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it, no hidden synchronisation.
 *   - images are float32 CHW (RGB), tiles are float32 NCHW, exactly as in the reference.
 *
 * Workspaces (held to this by tests/test_workspace_contract.py, between guard bytes and after calls whose data was NaN)
 *   - alignment: pass every buffer as torch's allocator gives it, 512-byte aligned.  That is the only alignment the tests run, so it
 *     is the only one promised.  The entry points refuse less than 16 bytes for the UtNet workspace and packed weights and less than
 *     256 bytes for frame_ws; anything between what a check refuses and 512 bytes is untested.
 *   - a call writes nothing outside [ptr, ptr + the size its *_bytes query returns) of a workspace, or outside the elements of a
 *     tensor, and no byte outside them reaches a result.
 *   - workspaces with an init call -- nd_utnet_workspace_init_hw, nd_unet_workspace_init, nd_utnet_train_workspace_init_hw,
 *     nd_unet_grad_workspace_init, nd_unet_train_workspace_init -- may hold anything before it (callers pass torch.empty); the init
 *     call writes every byte the entry points later read without having written it (the zero borders, the padded channel planes, the
 *     slack).  It runs once per geometry, not once per call: whatever earlier calls with that geometry left behind -- whole-tile or
 *     useful-region runs, NaN and Inf included -- does not reach a later result.
 *   - plain scratch, no init call, contents on entry do not matter: the workspaces of nd_layer_forward, nd_layer_forward_winograd (the
 *     Winograd scratch behind the layer plan too), nd_maxpool2_forward, nd_layer_wgrad, nd_mse, nd_ssim, nd_ms_ssim, nd_ssim_loss_grad,
 *     nd_ssim_padded(_grad), nd_criteria, nd_criteria_grad; the training `blobs` (packed by every forward / step); the packed blob
 *     handed to a device packer.  One buffer may serve calls of any shapes one after the other.
 *   - outputs are written in full (y, canvas += on every pixel of the tile range, dx, dw, db, loss, gy, out); of `grads` every
 *     parameter's range is written, the ranges of UNet's running statistics and of PReLU slopes the activation does not have never.
 *   - frame_ws is zero-filled once by the caller, never byte-poisoned.  It may then serve any number of frames without another
 *     zero-fill, frames of another geometry that needs the same nd_utnet_frame_workspace_bytes included (the Python module caches
 *     the buffer by that size): every call writes what it reads, the tile-origin tables too, and a short last band does not read
 *     what a full band of an earlier frame left behind it.
 */
#ifndef NIND_HIP_H
#define NIND_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum nd_status {
    ND_OK = 0,
    ND_EINVAL = -1,   /* bad argument (e.g. cs not of the form 16k+56 for UtNet) */
    ND_ENOMEM = -2,   /* workspace / output buffer too small                     */
    ND_EHIP = -3      /* a HIP runtime call or kernel launch failed              */
} nd_status;

typedef enum nd_act {     /* UtNet.py:16-26 */
    ND_ACT_NONE = 0,
    ND_ACT_PRELU = 1,     /* one learned scalar slope per activation layer */
    ND_ACT_ELU = 2,
    ND_ACT_HARDSWISH = 3
} nd_act;

typedef enum nd_layer_kind {
    ND_CONV3 = 0,         /* nn.Conv2d(k=3, valid)            UtNet.py:29..54          */
    ND_CONVT3 = 1,        /* nn.ConvTranspose2d(k=3, s=1)     UtNet.py:56,61,63,...    */
    ND_CONVT2S2 = 2,      /* nn.ConvTranspose2d(k=2, s=2)     UtNet.py:59,66,73,80     */
    ND_CONV1 = 3,         /* nn.Conv2d(k=1)                   UtNet.py:86              */
    ND_CONV2S2 = 4        /* nn.Conv2d(k=2, stride=2): the data gradient of ConvTranspose2d(2, s=2) (training step) */
} nd_layer_kind;

typedef enum nd_dtype {
    ND_F32 = 0,           /* fp32 storage, fp32 MFMA (v_mfma_f32_32x32x2_f32), exact-fp32 products            */
    ND_BF16 = 1,          /* bf16 storage of activations + weights, fp32 accumulate (v_mfma_f32_32x32x16_bf16) */
    ND_F16 = 2            /* fp16 storage of activations + weights, fp32 accumulate (v_mfma_f32_32x32x16_f16)  */
} nd_dtype;

/* Per-call arithmetic flags (bit set; 0 = the default path).  There is no process-wide switch: two calls with different
 * flags may run concurrently on different streams, also from different host threads: the launchers' per-device state is
 * shared safely (the CU count is queried once per device; a kernel's dynamic-LDS limit and the SSIM window constants are
 * checked and set under one lock, and the LDS limit only ever grows), and nd_last_error is thread-local. */
typedef enum nd_flags {
    ND_FLAG_NO_SPLITK = 1,    /* keep every output tile whole: no split-K tail, so a tile's bits do not depend on which other
                                 tiles share its launch (the default splits the K loop of a launch's last, partial round of
                                 workgroups over the idle CUs: deterministic, but fp32 sums re-associate by <= 1e-5).  It also
                                 keeps the three-pass Winograd layers on per-image tile grids: a tile's place in a mosaic
                                 (ND_FLAG_TILE_WINO) depends on which images share its launch                                 */
    ND_FLAG_DIRECT_CONV = 2,  /* direct convolution on every 3x3 layer (default on the fp32 path: Winograd F(6x6,3x3) from
                                 128 channels up, 1-D F(4,3) inside the implicit-GEMM kernel below; ~1e-5 re-association)   */
    ND_FLAG_W1D_REGS = 4,     /* A/B switch: the 1-D F(4,3) layers through the kernel that transforms in registers (conv_w1d)
                                 instead of the one that shares the transform through LDS (conv_w2d, the default)            */
    ND_FLAG_UNFUSED_POOL = 16, /* A/B switch: every MaxPool2d(2) as its own kernel (default: written from the producing layer's
                                 epilogue wherever its kernel can -- identical values)                                        */
    ND_FLAG_TILE_ENCODER = 32, /* A/B switch: nd_utnet_denoise_frame runs every tile's whole encoder (default: the first two
                                 levels once per band of tile rows, see nd_utnet_frame_plan)                                   */
    ND_FLAG_TILE_LEVEL2 = 64,  /* A/B switch: nd_utnet_denoise_frame keeps the third encoder level per tile where it would share it
                                 too (nd_utnet_frame_levels: 3).  Taken by the frame-loop entry points only (nd_utnet_frame_*,
                                 nd_utnet_denoise_frame); an unknown bit everywhere else                                          */
    ND_FLAG_FIND_NOISE = 128,  /* nd_unet_denoise_frame only (an unknown bit everywhere else): UNet(find_noise=True), ThirdPartyNets.py:
                                 167-168 -- a tile contributes its input minus the network output                                   */
    ND_FLAG_TILE_SKIPS = 256,  /* A/B switch: nd_utnet_denoise_frame keeps the skip halves of tconvs4.0 / 3.0 / 2.0 in the per-tile sums
                                 where it would compute their products once per band (nd_utnet_frame_folds).  Taken by the
                                 frame-loop entry points only; an unknown bit everywhere else                                      */
    ND_FLAG_TILE_WINO = 512,   /* A/B switch: every three-pass F(6x6,3x3) layer tiles each image on its own (default: the small
                                 ConvTranspose2d(3) layers of a launch -- bottom.2, tconvs1.0 at cs 264 -- under one tile grid over a
                                 mosaic of the launch's images, nd_wino_mosaic; fp32 re-association in the tiles that straddle a seam).  Taken by every
                                 flags-taking entry point                                                                         */
    ND_FLAG_UNET_WINOGRAD = 1024, /* the UNet inference entry points only (nd_unet_*_flags, nd_unet_denoise_frame, nd_unet_step_form,
                                 nd_unet_profile_stack; an unknown bit everywhere else): the 3x3 layers in Winograd forms -- three-pass
                                 F(6x6,3x3) where Cin >= 128, Cout >= 128 and Cin * Cout >= 128 * 256, fused F(4,3) below, direct for
                                 the 3-channel first layer and where a form does not take the layer's geometry.  Opt-in: ~1e-6
                                 re-association against the default path.  Blob, workspace and call must agree on the bit          */
    ND_FLAG_FULL_TILES = 8    /* nd_utnet_denoise_tiles / nd_utnet_profile_stack: compute every layer on the whole tile, as
                                 UtNet.forward does.  Default there: the last decoder levels compute only the pixels that the
                                 useful crop [pad, cs - pad) of a tile can reach (denoise_image.py:249-258 discards the rest of
                                 the network output before the canvas +=) -- same canvas, 19 % less work at cs 264 / ucs 200.
                                 nd_unet_denoise_frame: the same switch for the UNet decoder (nd_unet_useful_region)             */
} nd_flags;

int nd_version(void);   /* 119 = this header */
const char *nd_last_error(void);

/* ---------------------------------------------------------------- tile geometry (host, pure integer)
 * OneImageDS.__init__   denoise_image.py:100-104  -> nd_tile_grid
 * OneImageDS.__getitem__ denoise_image.py:131-143,172-173 -> nd_tile_geom
 */
int nd_tile_grid(int width, int height, int cs, int ucs, int ol, int *cols, int *rows, int *pad);
int nd_tile_geom(int i, int width, int height, int cs, int ucs, int ol,
                 int *x0, int *y0, int usefuldim[4], int usefulstart[2]);

/* ---------------------------------------------------------------- device tiler
 * nd_tile_gather: OneImageDS.__getitem__ (denoise_image.py:138-170) for tiles [tile_begin, tile_begin+tile_count):
 *   crop + symmetric mirror padding, img_chw [3,H,W] -> tiles_nchw [tile_count,3,cs,cs].  Bit-exact copies.
 * nd_stitch_add: main-loop body (denoise_image.py:249-267) + make_seamless_edges (:204-213):
 *   canvas_chw [3,H,W] += halved-overlap useful crops of tiles_nchw, tiles taken in ascending index order
 *   (same fp32 summation order as the reference).
 */
int nd_tile_gather(const float *img_chw, int width, int height, int cs, int ucs, int ol,
                   int tile_begin, int tile_count, float *tiles_nchw, void *stream);
int nd_stitch_add(float *canvas_chw, int width, int height, int cs, int ucs, int ol,
                  const float *tiles_nchw, int tile_begin, int tile_count, void *stream);

/* The two index maps behind these kernels, as host functions (pure integer; the kernels run the same inline functions).
 * nd_tile_source: pixel (y, x) of tile i shows frame pixel (*Y, *X) -- the symmetric mirror of OneImageDS.__getitem__: with
 *   u = x0 + x,  X = u inside [0, W),  -1 - u left of it,  2W - 1 - u right of it; the same in y.
 * nd_stitch_weight: pixel (y, x) of tile i is added to canvas pixel (*Y, *X) with weight *w: 0 outside the useful crop of
 *   nd_tile_geom (*Y, *X then name no pixel), else 1, halved once for every condition of make_seamless_edges that holds.
 * ND_EINVAL: a geometry nd_tile_grid refuses, a tile or pixel outside its range, a null output pointer.
 *
 * The adjoints of the two linear operators, for gradients through a tiled frame (frame_grad.py).  Stream-ordered, no atomics,
 * deterministic; a result does not depend on how a tile range is cut into launches, except for the fp32 order of the += of
 * nd_tile_gather_grad across launches.  tile_count = 0 is a no-op.
 * nd_stitch_grad: gtiles_nchw[t, c, y, x] = w * gcanvas_chw[c, Y, X] over nd_stitch_weight, for tiles [tile_begin,
 *   tile_begin + tile_count); every element of [tile_count,3,cs,cs] is written, 0 where w = 0.
 * nd_tile_gather_grad: gimg_chw[c, Y, X] += the sum of gtiles_nchw over the tile pixels of the launch that nd_tile_source sends
 *   to (Y, X) -- summed from 0 in ascending tile index, within a tile in ascending y * cs + x over its at most 3 x 3 pre-images
 *   (direct and folded, per axis), then added to what gimg holds.  Its work is the launch's footprint -- the frame rows and
 *   columns its tiles and their folds reach -- not the frame.
 * ND_EINVAL: a null pointer, tiles outside the grid, cs above 16384, more than 65535 tiles in one launch. */
int nd_tile_source(int i, int width, int height, int cs, int ucs, int ol, int y, int x, int *Y, int *X);
int nd_stitch_weight(int i, int width, int height, int cs, int ucs, int ol, int y, int x, int *Y, int *X, float *w);
int nd_stitch_grad(const float *gcanvas_chw, int width, int height, int cs, int ucs, int ol, int tile_begin, int tile_count,
                   float *gtiles_nchw, void *stream);
int nd_tile_gather_grad(const float *gtiles_nchw, int width, int height, int cs, int ucs, int ol, int tile_begin, int tile_count,
                        float *gimg_chw, void *stream);

/* ---------------------------------------------------------------- UtNet (UtNet.py:13-109)
 * Weight contract: the reference state-dict.  nd_utnet_num_tensors / nd_utnet_tensor_name
 * enumerate the keys in the order nd_utnet_pack_weights expects host pointers (float32, contiguous, torch layout:
 * Conv2d [Cout,Cin,k,k], ConvTranspose2d [Cin,Cout,k,k], bias [Cout], PReLU weight [1]).  For ELU/Hardswish the
 * PReLU entries are absent from the state-dict; pass NULL for them.
 * nn_common.Model.instantiate_model (nn_common.py:116-138) -> pack once at load time, upload, keep resident.
 */
int nd_utnet_num_tensors(void);
const char *nd_utnet_tensor_name(int idx);
size_t nd_utnet_packed_bytes(int funit, int dtype);
int nd_utnet_pack_weights(int funit, int dtype, const float *const *tensors, int n_tensors,
                          void *packed_host, size_t packed_bytes);

/* The same blob built in HBM from tensors that already live there, for every storage type: device-side packers.  The bf16 / fp16
 * blob (direct-form layers only) is bit for bit the host function's; in the fp32 blob the Winograd weight transforms are
 * evaluated in fp32 instead of double (packed values agree to ~1e-7 relative).  Stream-ordered. */
int nd_utnet_pack_weights_device(int funit, int dtype, const float *const *dev_tensors, int n_tensors, void *packed_dev,
                                 size_t packed_bytes, void *stream);

/* UtNet.forward (UtNet.py:97-109): x_nchw [batch,3,h,w] -> y_nchw [batch,3,h,w], both float32 in HBM; h and w are each of the
 * form 16k+56 (h = w = cs for the tiles of the denoise loop; the --whole_image branch, denoise_image.py:110-128, passes a whole
 * image).  The workspace holds the activations of one (h, w, batch) geometry in the quad-planar layout, zero borders included;
 * nd_utnet_workspace_init_hw must run once on it before its first forward with that geometry. */
size_t nd_utnet_workspace_bytes_hw(int funit, int h, int w, int batch, int dtype);
int nd_utnet_workspace_init_hw(void *workspace, size_t workspace_bytes, int funit, int h, int w, int batch, int dtype,
                               void *stream);
int nd_utnet_forward_hw(int funit, int act, int dtype, int flags, const void *packed_dev,
                        const float *x_nchw, float *y_nchw, int batch, int h, int w,
                        void *workspace, size_t workspace_bytes, void *stream);

/* The whole hot loop of denoise_image.py:240-267 for tiles [tile_begin, tile_begin+tile_count) of one frame,
 * device resident: gather(+mirror) -> UtNet -> useful crop -> seamless edges -> canvas +=.
 * tile_count <= batch of the workspace.  Equivalent to nd_tile_gather + nd_utnet_forward_hw + nd_stitch_add
 * without materialising the NCHW tile batch. */
int nd_utnet_denoise_tiles(int funit, int act, int dtype, int flags, const void *packed_dev,
                           const float *img_chw, float *canvas_chw, int width, int height,
                           int cs, int ucs, int ol, int tile_begin, int tile_count, int batch,
                           void *workspace, size_t workspace_bytes, void *stream);

/* The same loop for tiles [tile_begin, tile_begin+tile_count) of any length, in ascending launches of at most `batch` tiles
 * (`workspace` as for nd_utnet_denoise_tiles with that batch).  fp32 storage in useful-region mode with a tile stride divisible
 * by 4 (nd_utnet_frame_plan: D = 2): the first two encoder levels (convs1.0 ... the second pool) run once per band of tile rows
 * on the band's window of the mirrored frame (valid 3x3 convolutions and 2x2 pools are translation-equivariant); the decoder
 * reads each tile's skip tensors where the band holds them, the pooled level-2 input is copied from the band, and the border lines
 * a tile's own ReflectionPad2d(2) reaches come from 16-pixel edge images computed with the band -- one pair per tile row and one
 * per tile column, which all tiles of that row / column share -- and four corner patches per tile.  Launches hold exactly `batch` tiles
 * (the last one fewer) and may cross one band seam; a launch that would reach a third band is cut at its second seam.  Same
 * canvas as the per-tile encoder up to fp32 re-association (<= 1e-5); bits do not depend on `batch` or the tile range with
 * ND_FLAG_NO_SPLITK.  Every other case runs nd_utnet_denoise_tiles.
 * frame_ws: nd_utnet_frame_workspace_bytes, zero-filled once (null / 0 when that is 0): the band tensors (those the launches
 * read in two slots when the frame has more than one band, so that the next band can be computed while launches still read the
 * last one), the row and column edge tensors of one band (their pooled lines in the same two slots), the corner tensors of
 * 4 x batch patches, and two tables of `batch` tile origins.  No state is carried from one call to
 * the next.  progress (optional) is called with (progress_ctx, launch index, first tile, tile count) before each launch is
 * enqueued. */
typedef void (*nd_progress_fn)(void *ctx, int n, int tile_begin, int tile_count);
size_t nd_utnet_frame_workspace_bytes(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol, int batch);
int nd_utnet_denoise_frame(int funit, int act, int dtype, int flags, const void *packed_dev,
                           const float *img_chw, float *canvas_chw, int width, int height,
                           int cs, int ucs, int ol, int tile_begin, int tile_count, int batch,
                           void *workspace, size_t workspace_bytes, void *frame_ws, size_t frame_ws_bytes, void *stream,
                           nd_progress_fn progress, void *progress_ctx);
/* The same loop with a verdict per tile, for callers that recompute overflowing 16-bit tiles in a type with more range
 * (pipeline.denoise_frame with UtNet(fallback_dtype=...)).  Same arguments plus tile_ok: device memory, one byte per tile of the
 * grid (cols * rows of nd_tile_grid), indexed by the tile's index in the frame; the caller presets the bytes of the range to 1.
 * Every dtype is accepted, and every launch of the loop -- those of the shared-encoder path and those of nd_utnet_denoise_tiles alike
 * -- ends as follows, on the same stream:
 *   verdict: tile t of the launch is bad when any value the stitch would add for it is not finite -- the 1x1 head evaluated (not a
 *     test of the stored activations' bits) on 3 channels x the tile's useful rectangle as truncated at the frame's edges, before
 *     the seam factor.  The kernel stores 0 into tile_ok[t] for a bad tile and writes nothing for a good one; it reads what the
 *     stitch reads of the launch's last activation buffer and nothing else;
 *   guarded stitch: the stitch of nd_utnet_denoise_frame, except that a covering tile whose tile_ok is 0 is skipped and a pixel
 *     that no good tile of the launch covers is not written.
 * Contract: when every tile of the range is good the canvas is bit-identical to nd_utnet_denoise_frame with the same arguments;
 * otherwise the good tiles contribute exactly what they would have, in the same (ascending) order, and the bad ones nothing.  A
 * tile_ok of 0 is final for the call: a tile whose byte is 0 on entry is computed but not stitched.  Entries outside
 * [tile_begin, tile_begin + tile_count) are neither read nor written.  No host read, no allocation, no atomics; stream-ordered
 * and deterministic.  ND_EINVAL: a null tile_ok, else as nd_utnet_denoise_frame. */
int nd_utnet_denoise_frame_checked(int funit, int act, int dtype, int flags, const void *packed_dev,
                                   const float *img_chw, float *canvas_chw, int width, int height,
                                   int cs, int ucs, int ol, int tile_begin, int tile_count, int batch,
                                   void *workspace, size_t workspace_bytes, void *frame_ws, size_t frame_ws_bytes, void *stream,
                                   nd_progress_fn progress, void *progress_ctx, unsigned char *tile_ok);
/* Host-only query (no GPU call): the band plan of nd_utnet_denoise_frame.  out[8] = {D (shared encoder levels: 2 or 0),
 * aligned levels (tile origins on whole pixels of level 0 .. aligned-1: 1 + the power of 2 in the stride, at most 4), tile rows
 * per band, bands, stride, grid columns, grid rows, band input rows of a full band}.  A function of the frame geometry, the dtype
 * and the flags only (batch enters only through the workspace size). */
int nd_utnet_frame_plan(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol, int *out);
/* Host-only query: the encoder levels nd_utnet_denoise_frame shares in all -- 0, 2 (D above), or 3 where the tile stride is also
 * divisible by 8 and the decoder's region plan leaves the border lines of the third skip unread (crop >= 32 at every valid cs):
 * then convs3.0, convs3.2 and the third pool also run once per band, on the band's pooled level-2 input; tconvs2.0 reads its skip
 * half where the band wrote it; a tile's pooled level-3 input is its window of the band's, with its border lines from 6-line
 * images at level-2 resolution (two per tile row and two per tile column of a band, built from the level-2 edge lines and the
 * band's clean neighbours) and its corner pixels from four 6 x 6 patches of the tile's own level-2 input; and the per-tile stack
 * starts at convs4.0.  Level-2 values are fp32 re-associations of the per-tile ones (the band's F(6x6) tile grid differs from a
 * tile's).  The frame workspace then also holds a third origin table, the level-2 band, line and corner tensors and their
 * Winograd scratch.  ND_FLAG_TILE_LEVEL2 keeps it at 2.  *levels is written; same arguments and errors as nd_utnet_frame_plan. */
int nd_utnet_frame_levels(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol, int *levels);
/* Host-only query: the decoder layers whose skip half nd_utnet_denoise_frame folds out of the per-tile sums.  The first layer of a
 * decoder level is a ConvTranspose2d(3) on cat([up, skip]) and linear in its input channels: act(b + W_up * up + W_skip * skip) =
 * act(W_up * up + P) with P = W_skip * skip + b.  Where the skip is a band tensor (the shared encoder levels) P is the same for
 * every tile that overlaps a pixel, so it is computed once per band -- into the never-written up-sampled half of the band's
 * concat tensor: the frame workspace does not grow -- and the per-tile layer runs on the up-sampled half of its K blocks with P as
 * its addend.  Bit k of *mask is set when tconvs(4-k).0 is folded: a step that takes its skip from the band (tconvs4.0, tconvs3.0;
 * tconvs2.0 where level 2 is shared) and runs in a kernel that takes an addend (conv_w2d; the three-pass F(6x6) form, whose band
 * launches carry Winograd scratch of their own in the frame workspace).  0 with ND_FLAG_TILE_SKIPS and wherever no encoder level
 * is shared.  Same canvas up to fp32 re-association (the two halves' sums are added in another order).  A function
 * of the frame geometry, the dtype and the flags only; same arguments and errors as nd_utnet_frame_plan. */
int nd_utnet_frame_folds(int funit, int dtype, int flags, int width, int height, int cs, int ucs, int ol, int *mask);

/* Profiling entry point for the roofline report: one pass of the conv stack (22 MFMA conv layers + 4 pools, the launches
 * between the input pack and the final 1x1) with a HIP event recorded on `stream` between launches.  Synchronises the stream.
 * nd_utnet_step_name(i): reference layer key of step i ("maxpool" for pools). */
typedef struct nd_step_profile {
    float ms;               /* duration of the step (all its launches)                                                      */
    float ms_xform_in;      /* three-pass Winograd layers: input transform pass, GEMM launch, output transform pass (0 for   */
    float ms_gemm;          /*   the other forms, and for batches above one Winograd chunk)                                  */
    float ms_xform_out;
    int form;               /* -1 pool; 0 direct implicit GEMM (conv_qp); 1 fused 1-D Winograd F(4,3) (conv_w1d); 2 F(2,3);  */
                            /*   3 three-pass Winograd F(6x6,3x3): k_wino_in2 -> 64 GEMMs in one conv_qp launch -> k_wino_out2      */
    int kind;               /* nd_layer_kind, -1 for pools                                                                  */
    double flops;           /* algorithmic FLOP for `batch` tiles (SURVEY.md 2a convention; 0 for pools)                    */
    double mfma_flops;      /* FLOP the matrix cores execute in that form (MFMA instructions x 4096)                        */
    double bytes;           /* algorithmic HBM bytes: input + output activations + weights                                   */
    double xform_bytes_in;  /* three-pass layers: algorithmic HBM bytes of the two transform passes                          */
    double xform_bytes_out;
} nd_step_profile;
/* crop: margin of the useful tile centre the caller will keep ((cs - ucs) / 2 of the denoise loop; 0: the whole output, as
 * nd_utnet_forward_hw computes it) -- the stack then runs exactly as inside nd_utnet_denoise_tiles with the same flags */
int nd_utnet_profile_stack(int funit, int act, int dtype, int flags, const void *packed_dev, int batch, int cs, int crop,
                           void *workspace, size_t workspace_bytes, void *stream, nd_step_profile *steps, int max_steps);
const char *nd_utnet_step_name(int i);
/* host-only: region {r0, c0, rows, cols} of stack step `step` that nd_utnet_denoise_tiles computes when the centre [crop, cs - crop)
 * of a tile is kept (output grid of a 3x3 layer, input grid of a 2x2 stride-2 transpose; zeros: the whole tensor); returns the number
 * of restricted steps (>= 0) or a negative nd_status */
int nd_utnet_useful_region(int funit, int cs, int crop, int step, int *rect);

/* ---------------------------------------------------------------- UNet (ThirdPartyNets.py:62-169, eval mode)
 * Same contract as the UtNet entry points; BatchNorm2d running statistics are folded into the convolutions when the
 * weights are packed (nd_unet_tensor_name enumerates conv weight/bias and BN weight/bias/running_mean/running_var keys).
 * Any h, w >= 16 (odd sizes go through the reference's F.pad fix-up).  y = sigmoid(outc(...)); `find_noise` is the
 * caller's x - y. */
int nd_unet_num_tensors(void);
const char *nd_unet_tensor_name(int idx);
size_t nd_unet_packed_bytes(int dtype);
int nd_unet_pack_weights(int dtype, const float *const *tensors, int n_tensors, void *packed_host, size_t packed_bytes);
size_t nd_unet_workspace_bytes(int h, int w, int batch, int dtype);
int nd_unet_workspace_init(void *workspace, size_t workspace_bytes, int h, int w, int batch, int dtype, void *stream);
int nd_unet_forward(int dtype, const void *packed_dev, const float *x_nchw, float *y_nchw, int batch, int h, int w,
                    void *workspace, size_t workspace_bytes, void *stream);

/* The same blob (bit for bit) built in HBM from tensors that already live there: eval-mode BatchNorm is folded by a small kernel
 * (per-channel scale and bias, each operation rounded once, in the host packer's order) and the scale is multiplied in while the
 * fragments are written.  No host copy of the weights; stream-ordered; allocates nothing. */
int nd_unet_pack_weights_device(int dtype, const float *const *dev_tensors, int n_tensors, void *packed_dev, size_t packed_bytes,
                                void *stream);

/* The same family with nd_flags; flags = 0 is the plain entry point above, byte for byte.  ND_FLAG_UNET_WINOGRAD: the packed blob
 * carries the Winograd forms behind the default blob (no offset of the default blob moves; host and device packers write the same
 * bytes), the workspace carries the three-pass V / M scratch behind the default workspace, and nd_unet_forward_flags /
 * nd_unet_denoise_frame run the forms of nd_unet_step_form.  A blob or workspace made without the bit is too small for a call with it
 * (ND_ENOMEM for the workspace; the caller keeps blob and call in step).  The zero borders of the activation buffers stay zero.
 * nd_unet_forward_flags takes the known bits of nd_flags and ND_FLAG_UNET_WINOGRAD (ND_FLAG_DIRECT_CONV: every layer direct on the
 * same blob; ND_FLAG_W1D_REGS: the F(4,3) layers through conv_w1d where the row fits it, else direct). */
size_t nd_unet_packed_bytes_flags(int dtype, int flags);
int nd_unet_pack_weights_flags(int dtype, int flags, const float *const *tensors, int n_tensors, void *packed_host, size_t packed_bytes);
int nd_unet_pack_weights_device_flags(int dtype, int flags, const float *const *dev_tensors, int n_tensors, void *packed_dev,
                                      size_t packed_bytes, void *stream);
size_t nd_unet_workspace_bytes_flags(int h, int w, int batch, int dtype, int flags);
int nd_unet_workspace_init_flags(void *workspace, size_t workspace_bytes, int h, int w, int batch, int dtype, int flags, void *stream);
int nd_unet_forward_flags(int dtype, int flags, const void *packed_dev, const float *x_nchw, float *y_nchw, int batch, int h, int w,
                          void *workspace, size_t workspace_bytes, void *stream);
/* Host-only: the `form` code of nd_step_profile (-1 pool, 0 direct, 1 fused F(4,3), 3 three-pass F(6x6,3x3)) of step `step` in a
 * whole forward of batch x 3 x h x w under `flags`; a bad argument gives ND_EINVAL - 100. */
int nd_unet_step_form(int flags, int batch, int h, int w, int step);
/* The UNet twin of nd_utnet_profile_stack: one pass of the 26 steps on `batch` tiles of cs x cs (whatever the workspace holds) with an
 * event between steps; crop > 0 restricts the decoder as nd_unet_denoise_frame does.  blob and workspace: those of `flags`. */
int nd_unet_profile_stack(int flags, const void *packed_dev, int batch, int cs, int crop, void *workspace, size_t workspace_bytes,
                          void *stream, nd_step_profile *steps, int max_steps);

/* Host-only: the step list of the UNet stack (26 steps: 22 conv launches and 4 pools, between the input pack and the final 1x1).
 * nd_unet_step_name: module path of the step's layer ("inc.conv.conv.0", "up1.up", ...), "pool" for pools.
 * nd_unet_useful_region: region {r0, c0, rows, cols} of step `step` that nd_unet_denoise_frame computes when the centre
 * [crop, cs - crop) of a tile is kept -- output grid of a 3x3 layer, input grid of a 2x2 stride-2 transpose; zeros: the whole tensor
 * (always for the encoder and the pools: their outputs are skips).  Walking the decoder backwards from the kept centre, per axis: a
 * 3x3 layer with outputs [lo, hi) reads inputs [max(lo - 1, 0), min(hi + 1, size)), a transpose makes them from input rows
 * [lo >> 1, min((hi + 1) >> 1, size_in)).  Returns the number of restricted steps (>= 0) or a negative nd_status. */
int nd_unet_num_steps(void);
const char *nd_unet_step_name(int i);
int nd_unet_useful_region(int cs, int crop, int step, int *rect);

/* The hot loop of denoise_image.py:240-267 with UNet for tiles [tile_begin, tile_begin + tile_count) of one frame, in ascending
 * launches of at most `batch` tiles: gather (+symmetric mirror) straight into the first layer's input, the conv stack, then final
 * 1x1 + Sigmoid + useful crop + seamless edges + canvas += in one kernel; no NCHW tile batch is written.  The decoder computes only
 * what the kept centre of a tile depends on (nd_unet_useful_region; all layers whole if a region fits no workgroup shape of the
 * direct kernel) unless ND_FLAG_FULL_TILES is set: same canvas bit for bit under ND_FLAG_NO_SPLITK, else up to fp32
 * re-association of the split-K tail.  workspace: nd_unet_workspace_bytes(cs, cs, batch, ND_F32), initialised by
 * nd_unet_workspace_init.  dtype: ND_F32 only.  flags: ND_FLAG_NO_SPLITK, ND_FLAG_FULL_TILES and ND_FLAG_FIND_NOISE switch something
 * here; the other known bits of nd_flags (fused pools, shared encoder: this stack has none of them) are accepted and ignored; unknown
 * bits are an error.  ND_FLAG_UNET_WINOGRAD: the Winograd forms, on the blob and the workspace of the *_flags entry points with the
 * same bit; a restricted decoder layer runs in its form where the form takes the region, else direct (with it, ND_FLAG_DIRECT_CONV
 * and ND_FLAG_W1D_REGS mean what they mean for UtNet; no UNet layer is a transposed 3x3, so none takes the mosaic that
 * ND_FLAG_TILE_WINO switches off).  progress: as in nd_utnet_denoise_frame. */
int nd_unet_denoise_frame(int dtype, int flags, const void *packed_dev, const float *img_chw, float *canvas_chw, int width,
                          int height, int cs, int ucs, int ol, int tile_begin, int tile_count, int batch, void *workspace,
                          size_t workspace_bytes, void *stream, nd_progress_fn progress, void *progress_ctx);

/* UNet under torch.autograd in EVAL mode (BatchNorm on its running statistics; train-mode batch statistics are not implemented), fp32,
 * any h, w >= 16, batch <= 256.  The two halves mirror nd_utnet_train_forward_hw / nd_utnet_train_backward_hw.
 *
 * Parameters and gradients are ONE flat float layout in nd_unet_tensor_name order, for parameters and buffers alike: conv / transpose
 * weights and biases, BatchNorm weight, bias, running_mean, running_var (nd_unet_param_range: offset and count of tensor
 * `tensor_idx`; nd_unet_param_count: the total).  Buffers have a slot so that the fold reads one array; their slots in `grads`
 * are never written.
 *
 * nd_unet_grad_forward: folds BatchNorm and packs on the device, into `blobs` (nd_unet_grad_blob_bytes), in the forward role (the
 * blob of nd_unet_pack_weights_device, bit for bit) and in the transposed role the data gradients read; runs every layer on the
 * whole tile with its output kept in `workspace`; final 1x1 + Sigmoid.  y = sigmoid(outc(...)), or x - sigmoid with
 * ND_FLAG_FIND_NOISE.  flags: ND_FLAG_NO_SPLITK and ND_FLAG_FIND_NOISE switch something; the other known bits are accepted and ignored.
 *
 * nd_unet_grad_backward: the whole backward from gy = d loss / d y.  grads (nullable): every parameter gradient into the flat
 * layout -- null launches no weight-gradient, bias-sum or fold-adjoint kernel (a frozen network costs forward + data gradients);
 * dx_nchw (nullable): d loss / d x; at least one of the two.  Same flags as the forward call.  Data gradients: the conv kernel
 * on the transposed-role blob (a padding-1 3x3 layer on a gradient buffer with a 1-pixel zero border; a 2x2 stride-2 transpose as a
 * 2x2 stride-2 conv over rows / columns [0, 2 h_in) only: the gradient on the F.pad fix-up lines is dropped); ReLU from the kept
 * output (ReLU'(0) = 0); max-pool to the first maximum, added to the skip half's gradient in a fixed order; weight gradients on
 * the matrix cores for the FOLDED weights W' = W s, b' = (b - mean) s + beta, s = gamma / sqrt(var + 1e-5), then the fold's adjoint:
 * dW = dW' s, db = db' s, dbeta = db', dgamma = (sum dW' W + db' (b - mean)) / sqrt(var + 1e-5).  No atomics: two calls give the
 * same bits.
 *
 * `workspace` (nd_unet_grad_workspace_bytes(h, w, batch), zero-filled once per geometry by nd_unet_grad_workspace_init) and `blobs`
 * carry the forward's state to the backward call: nothing else may use them in between.  A workspace of (h, w, batch) also serves
 * (h, w, fewer) after another nd_unet_grad_workspace_init for that count.  x, y, gy, dx: [batch,3,h,w] NCHW fp32 in HBM. */
size_t nd_unet_param_count(void);
int nd_unet_param_range(int tensor_idx, size_t *offset, size_t *count);
size_t nd_unet_grad_blob_bytes(void);
size_t nd_unet_grad_workspace_bytes(int h, int w, int batch);
int nd_unet_grad_workspace_init(void *workspace, size_t workspace_bytes, int h, int w, int batch, void *stream);
int nd_unet_grad_forward(int flags, const float *params, void *blobs, const float *x_nchw, float *y_nchw, int batch, int h, int w,
                         void *workspace, size_t workspace_bytes, void *stream);
int nd_unet_grad_backward(int flags, const float *params, float *grads, void *blobs, const float *gy_nchw, float *dx_nchw, int batch,
                          int h, int w, void *workspace, size_t workspace_bytes, void *stream);

/* UNet TRAINING step halves: BatchNorm on the statistics of the batch (nn.BatchNorm2d in train() mode), fp32, any h, w >= 16,
 * batch <= 256 and at least 2 values per channel in every BatchNorm layer: batch * (h / 16) * (w / 16) >= 2 (torch: "Expected more
 * than 1 value per channel when training"); else ND_EINVAL, and nd_unet_train_workspace_bytes returns 0.  params / grads: the flat
 * layout of nd_unet_param_range.  flags: those of nd_unet_grad_forward.
 *
 * nd_unet_train_forward: packs the RAW weights and biases (no fold) into `blobs` (nd_unet_train_blob_bytes) in both roles.  Each of
 * the 18 Conv3 + BatchNorm + ReLU layers: the convolution without activation into a pre-norm buffer z that is KEPT for the backward
 * (this about doubles the activation part of the workspace against nd_unet_grad_workspace_bytes); per channel over the N = batch *
 * H * W interior pixels of the level: mu = mean z, var = E[(z - mu)^2] (biased), inv = 1 / sqrt(var + 1e-5), both kept;
 * a = ReLU(gamma (z - mu) inv + beta) into the layer's activation buffer; and the running statistics IN `params` move as torch's:
 * rm <- (1 - momentum) rm + momentum mu, rv <- (1 - momentum) rv + momentum var N / (N - 1).  momentum in [0, 1].  Transposes,
 * pools, concat and F.pad fix-up lines, the 1x1 head and find_noise: as nd_unet_grad_forward.
 *
 * nd_unet_train_backward: from gy = d loss / d y.  For a BatchNorm layer with g_a = the gradient of its post-ReLU output, m = [a > 0]
 * and xhat = (z - mu) inv:  dbeta = sum g_a m,  dgamma = sum g_a m xhat,  g_z = gamma inv (g_a m - dbeta / N - xhat dgamma / N),
 * then the weight gradient and the data gradient of the convolution from g_z with the raw weights.  grads (nullable) receives every
 * parameter gradient; dx_nchw (nullable) d loss / d x; at least one of the two.  The bias gradient of the 18 convolutions that feed a
 * BatchNorm is written as EXACT ZEROS: BatchNorm removes the channel mean, so that is the exact value (torch writes the rounding
 * noise of sum g_z, about 1e-9, which Adam's g / (|g| + eps) would turn into full steps).  The slots of running statistics in
 * `grads` are never written.
 *
 * The statistics and the two backward sums are accumulated in double, in a fixed two-stage order (one partial per workgroup, then
 * one workgroup per 4 channels); no atomics anywhere: two calls give the same bits.  `workspace` (zero-filled once per geometry by
 * nd_unet_train_workspace_init) and `blobs` carry the forward's state to the backward call. */
size_t nd_unet_train_blob_bytes(void);
size_t nd_unet_train_workspace_bytes(int h, int w, int batch);
int nd_unet_train_workspace_init(void *workspace, size_t workspace_bytes, int h, int w, int batch, void *stream);
int nd_unet_train_forward(int flags, float *params, void *blobs, const float *x_nchw, float *y_nchw, int batch, int h, int w,
                          float momentum, void *workspace, size_t workspace_bytes, void *stream);
int nd_unet_train_backward(int flags, const float *params, float *grads, void *blobs, const float *gy_nchw, float *dx_nchw, int batch,
                           int h, int w, void *workspace, size_t workspace_bytes, void *stream);

/* FLOP per tile by the reference's own accounting, for roofline reports. */
double nd_utnet_flops(int funit, int cs);

/* ---------------------------------------------------------------- single-layer entry points (parity tests)
 * One weighted layer on NCHW float32 tensors: pack -> quad-planar conv kernel -> unpack.
 * y = act(layer(x) + bias); output shape: CONV3 (H-2,W-2); CONVT3 (H+2,W+2); CONVT2S2 (2H,2W); CONV1 (H,W). */
size_t nd_layer_packed_bytes(int kind, int cin, int cout, int dtype);
int nd_layer_pack(int kind, int cin, int cout, int dtype, const float *weight, const float *bias,
                  void *packed_host, size_t packed_bytes);
size_t nd_layer_workspace_bytes(int kind, int batch, int cin, int cout, int h, int w, int dtype);
int nd_layer_forward(int kind, int act, float slope, int dtype, const void *packed_dev,
                     const float *x_nchw, int batch, int cin, int h, int w, int cout, float *y_nchw,
                     void *workspace, size_t workspace_bytes, int variant, int flags, void *stream);
/* nn.MaxPool2d(2) (UtNet.py:34) on NCHW float32 through the quad-planar pool kernel. */
int nd_maxpool2_forward(const float *x_nchw, int batch, int c, int h, int w, float *y_nchw,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------- training-step building blocks (next row f3)
 * Weight and bias gradient of one layer (autograd's conv backward-weight; nn_common.py:201-218 loss.backward()):
 * x [B,cin,h,w] = the layer's input, dy = gradient w.r.t. the layer's (pre-activation) output, NCHW fp32 in HBM;
 * dw in the torch weight layout of the layer kind, db [cout].  The data gradient of a layer is a FORWARD launch of the
 * transposed kind (nd_layer_forward: CONV3 <-> CONVT3, CONVT2S2 -> CONV2S2) on the same weight tensor. */
size_t nd_layer_wgrad_workspace_bytes(int kind, int batch, int cin, int cout, int h, int w);
int nd_layer_wgrad(int kind, const float *x_nchw, const float *dy_nchw, int batch, int cin, int h, int w, int cout,
                   float *dw, float *db, void *workspace, size_t workspace_bytes, void *stream);

/* UtNet training step (BASELINE config 5; nn_train.py:308-380, nn_common.py:198-255), fp32, on crops of h x w pixels (each
 * side 16k+56, e.g. 136 / 184).  Parameters and gradients are flat float buffers in state-dict order (nd_utnet_tensor_name /
 * nd_utnet_param_range): one buffer for the data-parallel all-reduce and for the optimizer.  x, target, y_out, gy, dx:
 * [batch,3,h,w] NCHW fp32 in HBM.  The workspace holds one (h, w, batch) geometry; nd_utnet_train_workspace_init_hw zero-fills
 * it once before its first use.  blobs: nd_utnet_train_blob_bytes of packed weights.
 *
 * nd_utnet_train_step_act_hw = device-side weight packing + forward + loss + backward, for any activation the network takes
 * (act as in the two halves below):
 *     loss = w_l1 * mean|g - t| + w_mse * mean (g - t)^2 + w_ssim * mean_n(1 - SSIM_n(g, t))
 *            + w_msssim * mean_n(1 - MS-SSIM_n(g, t)),        g = clip(net(x), 0, 1), t = target   (nn_common.py:198-241;
 *     the SSIM terms as in nd_ssim_loss_grad; MS-SSIM needs a loss crop of at least 161 pixels)
 * loss_out: one float in HBM.  loss_cs > 0: the criteria see the centre loss_cs x loss_cs crop at y0 = (h - loss_cs) / 2,
 * x0 = (w - loss_cs) / 2 of output and target (pt_ops.pt_crop_batch, nn_train.py:319-323; --loss_cs), and the gradient is zero
 * outside it; 0: the whole output.  The loss and its gradient are nd_criteria_grad's, below.
 *
 * The two halves of the step for torch.autograd, so that the reference's own training statements
 * (nn_common.py:198-218: `self.model(noisy_batch).clip(0,1)`, `loss.backward()`) run unchanged on the module:
 * nd_utnet_train_forward_hw = device-side weight packing + forward with the pre-activations kept in `workspace`;
 * nd_utnet_train_backward_hw = the whole backward from gy = d loss / d output.  grads (nullable) = the flat parameter
 * gradients -- null skips every parameter-gradient launch and bucket event (a frozen network costs forward + data gradients
 * only); dx_nchw (nullable) = d loss / d x, the first layer's data gradient through the ReflectionPad2d(2) of the input; at
 * least one of the two.  act: ND_ACT_PRELU | ND_ACT_ELU | ND_ACT_HARDSWISH (networks/UtNet.py:17-26; tensors of the parameter
 * layout that the activation does not have -- PReLU slopes -- are ignored and their gradients left untouched).  `workspace`
 * and `blobs` carry the forward's state to the backward call: nothing else may use them in between.
 *
 * nd_adam_step = torch.optim.Adam(lr, betas, eps, amsgrad) on the flat buffers (nn_common.py:185). */
size_t nd_utnet_param_count(int funit);
int nd_utnet_param_range(int funit, int tensor_idx, size_t *offset, size_t *count);
size_t nd_utnet_train_blob_bytes(int funit);
size_t nd_utnet_train_workspace_bytes_hw(int funit, int h, int w, int batch);
int nd_utnet_train_workspace_init_hw(void *workspace, size_t workspace_bytes, int funit, int h, int w, int batch, void *stream);
int nd_utnet_train_step_act_hw(int funit, int act, int flags, const float *params, float *grads, void *blobs, const float *x_nchw,
                               const float *target_nchw, float *y_out_nchw, float w_l1, float w_mse, float w_ssim, float w_msssim,
                               float *loss_out, int batch, int h, int w, int loss_cs, void *workspace, size_t workspace_bytes,
                               void *stream, void *const *bucket_events, int n_events);
int nd_utnet_train_forward_hw(int funit, int act, int flags, const float *params, void *blobs, const float *x_nchw,
                              float *y_out_nchw, int batch, int h, int w, void *workspace, size_t workspace_bytes, void *stream);
int nd_utnet_train_backward_hw(int funit, int act, int flags, const float *params, float *grads, void *blobs, const float *gy_nchw,
                               float *dx_nchw, int batch, int h, int w, void *workspace, size_t workspace_bytes, void *stream,
                               void *const *bucket_events, int n_events);
/* Data-parallel training that overlaps the gradient reduction with the backward pass (BASELINE configs[4]): the flat gradient
 * buffer is cut into nd_utnet_grad_buckets = 9 contiguous ranges, one per decoder / encoder level, numbered in the order the
 * backward pass completes them.  bucket_events of nd_utnet_train_step_act_hw / nd_utnet_train_backward_hw: null, or n_events = 9
 * hipEvent_t; bucket_events[k] is recorded on `stream` when bucket k is final, so a reducer on another stream can all-reduce it
 * under the backward of the shallower levels. */
int nd_utnet_grad_buckets(int funit, size_t *offsets, size_t *counts, int max);
int nd_adam_step(float *params, const float *grads, float *m, float *v, float *vmax, size_t n, float lr, float beta1,
                 float beta2, float eps, int step, int amsgrad, void *stream);
/* Guarded optimizer step (119): gradient clipping by global norm and skipping of non-finite steps, decided on the device.  Both
 * calls are enqueued on `stream`: no host read, no allocation, no event.
 *
 * nd_grad_guard: one streaming pass over the n fp32 gradients (16-byte loads, grads 16-byte aligned, a scalar tail for n % 4;
 * the grid depends on n alone), per-workgroup partial sums in `workspace` (nd_grad_guard_workspace_bytes), then one workgroup
 * that adds them in a fixed order: no atomics, the same bits on every run.  It leaves four doubles in HBM at `state`:
 *   [0] sum of g^2, accumulated in double          [1] the number of non-finite entries (NaN, +inf, -inf)
 *   [2] scale = max_norm > 0 ? min(max_norm / (sqrt([0]) + 1e-6), 1) : 1  -- the coefficient of torch.nn.utils.clip_grad_norm_,
 *       in double; a NaN norm gives a NaN scale (torch.clamp keeps NaN), an infinite one gives 0
 *   [3] ok = skip_nonfinite && [1] > 0 ? 0 : 1
 *
 * nd_adam_step_guarded = nd_adam_step reading that state: with ok == 0 it touches nothing; otherwise every element takes
 * g = grads[i] * (float)scale, one fp32 multiply, into nd_adam_step's own arithmetic -- with scale == 1 the result equals
 * nd_adam_step bit for bit.  grads is NOT modified: it keeps the unclipped gradient.  `step` comes from the host as for
 * nd_adam_step (the host never waits to learn whether a step was applied), so a skipped step still advances it.  That differs
 * from torch.cuda.amp.GradScaler, which does not call optimizer.step() on a skipped step: here the bias-correction index counts
 * attempts, while m, v, vmax and the parameters do not move on a skipped step. */
size_t nd_grad_guard_workspace_bytes(size_t n);
int nd_grad_guard(const float *grads, size_t n, float max_norm, int skip_nonfinite, double *state, void *workspace,
                  size_t workspace_bytes, void *stream);
int nd_adam_step_guarded(float *params, const float *grads, float *m, float *v, float *vmax, size_t n, float lr, float beta1,
                         float beta2, float eps, int step, int amsgrad, const double *state, void *stream);

/* ---- image-quality scores of the eval harness ------------------------------------------
 * Replace pt_helpers.get_losses (common/libs/pt_helpers.py:40-48): F.mse_loss, piqa.SSIM and piqa.MS_SSIM with piqa's
 * defaults, reduction=None (common/libs/pt_losses.py:6-18 subtracts them from 1; so do the Python classes here).
 * x, y: float32 [n, c, h, w] in HBM, values in [0, 1].  out: float32 [n] in HBM (nd_mse: one float).
 * nd_ssim needs h, w >= 11; nd_ms_ssim needs h, w >= 161 (five scales of an 11-tap window) -- ND_EINVAL otherwise, where
 * piqa raises from the convolution.  The workspace of nd_ssim_workspace_bytes serves all three. */
size_t nd_ssim_workspace_bytes(int n, int c, int h, int w);
int nd_ssim(const float *x, const float *y, int n, int c, int h, int w, float *out, void *workspace, size_t workspace_bytes,
            void *stream);
int nd_ms_ssim(const float *x, const float *y, int n, int c, int h, int w, float *out, void *workspace,
               size_t workspace_bytes, void *stream);
int nd_mse(const float *x, const float *y, size_t count, float *out, void *workspace, size_t workspace_bytes, void *stream);

/* The same two scores as differentiable training losses (nn_common.py:170-177, 226-241: criterions['SSIM'|'MSSSIM'], weighted
 * sum, loss.backward()):   loss_acc[0] += weight * mean_n (1 - score_n(x, y));   gx = (accumulate ? gx : 0) + d(that)/dx.
 * x = generated batch, y = target, gx: float32 [n, c, h, w]; multiscale 0 = SSIM, 1 = MS-SSIM (h, w >= 161). */
size_t nd_ssim_loss_workspace_bytes(int n, int c, int h, int w);
int nd_ssim_loss_grad(const float *x, const float *y, int n, int c, int h, int w, int multiscale, float weight,
                      float *loss_acc, float *gx, int accumulate, void *workspace, size_t workspace_bytes, void *stream);

/* Per-sample criteria of a batch: what the validation pass of training averages (nn_train.py:51-71, nn_common.py:198-199, 226-241).
 * y = the raw network output, target = the clean batch, both [n,3,h,w] fp32 in HBM.  g = clip(y, 0, 1); with loss_cs > 0 both g and
 * target are cut to the centre loss_cs x loss_cs window at y0 = (h - loss_cs) / 2, x0 = (w - loss_cs) / 2 (pt_ops.pt_crop_batch);
 * 0: the whole image.  out: [n][5] fp32, per sample { mean|g - t|, mean (g - t)^2, 1 - SSIM (nd_ssim), 1 - MS-SSIM (nd_ms_ssim),
 * weighted = sum_k w_k * column_k over the computed columns with a non-zero weight }.  A column is computed iff its weight != 0 or its
 * bit is set in `also` (bit k = column k); the others are written as 0.  ND_EINVAL as nd_utnet_train_step_act_hw: an SSIM window below
 * 11, an MS-SSIM window below 161, loss_cs above h or w, a null pointer, n < 1 (also: n > 65535, a side above 16384);
 * ND_ENOMEM: a workspace below nd_criteria_workspace_bytes.  Stream-ordered, allocates nothing, deterministic (no atomics; partial
 * sums are added in a fixed order). */
size_t nd_criteria_workspace_bytes(int n, int h, int w, int loss_cs);
int nd_criteria(const float *y_nchw, const float *target_nchw, int n, int h, int w, int loss_cs, float w_l1, float w_mse,
                float w_ssim, float w_msssim, int also, float *out, void *workspace, size_t workspace_bytes, void *stream);
/* The same criteria as the training loss and its gradient (Generator.compute_loss, loss.backward(); nn_common.py:201-255) -- the
 * loss section of nd_utnet_train_step_act_hw:   loss_out[0] = w_l1 * mean|g - t| + w_mse * mean (g - t)^2
 *     + w_ssim * mean_n(1 - SSIM_n(g, t)) + w_msssim * mean_n(1 - MS-SSIM_n(g, t))     (written, not accumulated; means over the
 * window), g = clip(y, 0, 1) on the centre window as above.  gy_nchw: [n,3,h,w] = d loss_out / d y, written in full: clip passes the
 * gradient on the closed interval [0, 1], d|x|/dx = 0 at 0, and the gradient is exactly 0 outside the window.  Refusals as
 * nd_criteria (n is not limited to 65535).  The workspace size for loss_cs = 0 serves every loss_cs of the same (n, h, w).
 * Stream-ordered, allocates nothing, deterministic (no atomics). */
size_t nd_criteria_grad_workspace_bytes(int n, int h, int w, int loss_cs);
int nd_criteria_grad(const float *y_nchw, const float *target_nchw, int n, int h, int w, int loss_cs, float w_l1, float w_mse,
                     float w_ssim, float w_msssim, float *loss_out, float *gy_nchw, void *workspace, size_t workspace_bytes,
                     void *stream);

/* The SSIM the reference vendors itself (libs/pytorch_ssim/__init__.py:20-35; loss.py:29-45 gen_score writes res.txt with it).
 * Not the piqa score above: the Gaussian (sigma 1.5, `window` taps) is applied with zero padding of window / 2, so the map is
 * h x w and border pixels see zeros.   out[i] = mean over (c, h, w) of the map of sample i.
 * window: odd, 3 ... 11 (ND_EINVAL otherwise: an even window makes the reference's map one row and column larger).  Any
 * h, w >= 1: an image smaller than the window is defined by the padding.
 * nd_ssim_padded_grad: gx = sum_i gout[i] * d out[i] / dx with y constant; gout: float32 [n] in HBM, gx: float32 [n, c, h, w],
 * overwritten.  Both calls take the workspace of nd_ssim_padded_workspace_bytes (ND_ENOMEM if it is smaller) and are
 * deterministic: partial sums are added in a fixed order. */
size_t nd_ssim_padded_workspace_bytes(int n, int c, int h, int w, int window);
int nd_ssim_padded(const float *x, const float *y, int n, int c, int h, int w, int window, float *out, void *workspace,
                   size_t workspace_bytes, void *stream);
int nd_ssim_padded_grad(const float *x, const float *y, int n, int c, int h, int w, int window, const float *gout, float *gx,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- augmented training batches from a device-resident crop pool (dataset_torch_3.py:231-276, DenoisingDataset.__getitem__) ----
 * The pool is one byte buffer in HBM holding images as planar [3][H][W] samples in their file type, and `images`, a table in HBM of
 * four int64 per image: {byte offset into the pool (a multiple of the sample size), H, W, nd_sample_type}.  `draws`, in HBM, holds
 * eight int32 per sample: {clean image, noisy image, x0, y0, nrot, flip1, flip2, the bits of the float u in [0, 1)}.
 * nd_crop_batch writes clean_nchw and noisy_nchw, [batch,3,cs,cs] fp32, from the same draws, in one launch:
 *   samples are converted as np_imgops.img_path_to_np_flt does (u8 / 255, u16 / 65535 in fp32, f32 as it is);
 *   a side d < cs is zero-padded, centred, (cs - d) / 2 before (np_imgops.np_pad_img_pair); a side d > cs is cut at x0 / y0
 *   (np_crop_img_pair), so crop pixel (a, b) is source pixel (y0 + a - pad0_y, x0 + b - pad0_x) or 0 outside the image;
 *   output pixel (y, x) is the crop pixel nd_crop_source names: np.rot90(nrot, (1, 2)), np.flip(1) if flip1, np.flip(2) if flip2.
 * Exposure multiplier (dataset_torch_3.py:271-274): mult (nullable, HBM, [batch]) gives it per sample; without it and with
 * exp_mult_min != 1 a first launch writes xmax[n] = the maximum of the clean crop (a maximum of the integer samples for u8 / u16, converted once: order-free) and
 * mult_out[n] = exp_mult_min + (min(exp_mult_max, 1 / xmax[n]) - exp_mult_min) * u (xmax 0: exp_mult_max), both [batch] fp32 in HBM
 * and needed only then.  With a multiplier m: clean = clean * m, unclipped; noisy = clip(noisy * m, 0, 1).  Without: no clip.
 * Every read is guarded on the device: an image index outside the table, or a table row that does not lie inside the pool, gives a
 * zero sample, and no x0 / y0 reads outside an image.  Stream-ordered; allocates nothing.  ND_EINVAL: a null pointer, n_images < 1,
 * cs outside [1, 16384], batch outside [1, 65535].  Not built: the sigmamin / sigmamax artificial noise and the JPEG branch.
 * nd_crop_source (host only, the kernel's own inline map): *a, *b = the crop pixel that output pixel (y, x) shows;
 * flips: bit 0 = flip1, bit 1 = flip2. */
typedef enum nd_sample_type { ND_SAMPLE_U8 = 0, ND_SAMPLE_U16 = 1, ND_SAMPLE_F32 = 2 } nd_sample_type;
int nd_crop_source(int cs, int nrot, int flips, int y, int x, int *a, int *b);
int nd_crop_batch(const void *pool, size_t pool_bytes, const int64_t *images, int n_images, const int32_t *draws, int batch, int cs,
                  float exp_mult_min, float exp_mult_max, const float *mult, float *xmax, float *mult_out, float *clean_nchw,
                  float *noisy_nchw, void *stream);
/* Whole pool images as fp32, for work on the files as stored (the MS-SSIM of every clean-noisy pair, crop_pool.CropPool.score_pairs):
 * out_nchw[i] = image index[i] ([n] int32 in HBM) of the same pool and table, [n,3,h,w] fp32, samples converted as above and
 * nothing else: no crop, no padding, no orientation, no multiplier.  Guards as above, and a table row whose H x W is not h x w is
 * not the image asked for: out_nchw[i] is all zeros for it, for an index outside the table and for a row outside the pool; nothing
 * is read out of range.  Stream-ordered; allocates nothing.  ND_EINVAL: a null pointer, n_images < 1, n outside [1, 65535], h or w
 * outside [1, 16384]. */
int nd_pool_fetch(const void *pool, size_t pool_bytes, const int64_t *images, int n_images, const int32_t *index, int n, int h, int w,
                  float *out_nchw, void *stream);
/* The same two calls on a pool of whole frames, each stored once, whose images are windows into them (crop_pool.CropPool.from_full_size:
 * the crops of the reference's tools/crop_img.sh without the crop files).  `windows` is a table in HBM of eight int64 per image:
 *   {byte offset of the parent into the pool (a multiple of the sample size), H, W, nd_sample_type, y, x, PH, PW}
 * The parent is planar [3][PH][PW] at the offset; the image is its rows [y, y + H) x columns [x, x + W) in each plane, so sample
 * (c, i, j) of the image is sample c * PH * PW + (y + i) * PW + (x + j) of the parent: the row pitch is PW and the plane pitch PH * PW,
 * in samples.  The first four columns are those of the dense table, with the offset naming the parent.
 * Everything said above holds with "the image" meaning the window: conversion, centred zero padding of a side shorter than cs, the
 * cut at x0 / y0, orientation, xmax (the maximum over the window's part of the crop, not over the parent's) and the multiplier; and
 * a pixel outside the window reads as 0 even where the parent holds data there, so padding is zeros as it is for a crop file.
 * nd_crop_batch_windows on a window table gives, bit for bit, what nd_crop_batch gives on a dense pool of the cut-out windows.
 * Guards, on the device: an index outside the table, a bad type or alignment, a negative y or x, a window that does not lie inside
 * its parent (y + H > PH or x + W > PW), or a parent that does not lie inside the pool gives zero samples; for
 * nd_pool_fetch_windows a row of another size than h x w does too.  Nothing is read out of range, whatever the table or the draws
 * hold.  Stream-ordered; allocates nothing.  ND_EINVAL as for the dense forms. */
int nd_crop_batch_windows(const void *pool, size_t pool_bytes, const int64_t *windows, int n_windows, const int32_t *draws, int batch,
                          int cs, float exp_mult_min, float exp_mult_max, const float *mult, float *xmax, float *mult_out,
                          float *clean_nchw, float *noisy_nchw, void *stream);
int nd_pool_fetch_windows(const void *pool, size_t pool_bytes, const int64_t *windows, int n_windows, const int32_t *index, int n,
                          int h, int w, float *out_nchw, void *stream);

/* ---- Winograd forms of a 3x3 layer, fp32 inference (same math as nd_layer_forward on a CONV3 / CONVT3 layer, re-associated).
 * tile = 2 | 4 | 6: three-pass F(tile x tile, 3 x 3) (input transform, one launch of (tile+2)^2 GEMMs, output transform;
 *               Cin % 16 == 0; agrees with the direct kernel to ~1e-6 / ~1e-5 / ~2e-5 relative);
 * tile = 1 | 3: 1-D F(2,3) | F(4,3) along x inside the implicit-GEMM kernel, transform in registers (~1e-6 / ~5e-6);
 * tile = 5    : the same F(4,3) form with the input transform shared by the workgroup through LDS (conv_w2d). */
/* The mosaic a three-pass F(6x6,3x3) launch of B images of a ConvTranspose2d(3) layer with p x p outputs (p = input + 2) lays its
 * tile grid over: by rows of bx images at pitch p, whose shared zero border lines make the mosaic's transposed convolution the
 * per-image results side by side.  Every bx in [1, B] with by = ceil(B / bx) is tried and the fewest tiles win; a count within 1 %
 * of the fewest is a tie, and ties go to the squarer mosaic ((13, 256): 16 x 16 with 1225 tiles, not 43 x 6 with 1222).  Returns 1 and the mosaic where a launch takes one (p >= 8, B > 1, *tiles <= 0.9 *tiles_per_image;
 * the launch must also be whole-tensor, square, unpooled, single-source and without ND_FLAG_NO_SPLITK / ND_FLAG_TILE_WINO), else 0 with
 * *bx = *by = 0 and *tiles = *tiles_per_image = B * ceil(p / 6)^2.  Host only, pure integer; a function of (p, B) alone. */
int nd_wino_mosaic(int p, int B, int *bx, int *by, long *tiles, long *tiles_per_image);

size_t nd_winograd_packed_bytes(int tile, int cin, int cout);
int nd_winograd_pack(int tile, int kind, int cin, int cout, const float *w, const float *bias, void *packed,
                     size_t packed_bytes);
size_t nd_layer_winograd_workspace_bytes(int tile, int kind, int batch, int cin, int cout, int h, int w);
int nd_layer_forward_winograd(int tile, int kind, int act, float slope, const void *packed, const float *x, int batch,
                              int cin, int h, int w, int cout, float *y, void *workspace, size_t workspace_bytes, int flags,
                              void *stream);

/* Kernel micro-benchmark: `iters` launches of one conv layer (variant -1 = automatic choice) on pseudo-random
 * quad-planar data carved from `workspace` (nd_layer_workspace_bytes + nd_layer_packed_bytes + 256 B); mean launch
 * duration from HIP events on `stream`.  Synchronises the stream. */
int nd_conv_bench(int kind, int dtype, int batch, int cin, int cout, int h, int w, int variant, int iters,
                  void *workspace, size_t workspace_bytes, void *stream, float *mean_ms);

int nd_winograd_bench(int tile, int kind, int batch, int cin, int cout, int h, int w, int iters, void *workspace,
                      size_t workspace_bytes, void *stream, float *mean_ms);
/* the same with nd_flags (ND_FLAG_NO_SPLITK, ND_FLAG_TILE_WINO) */
int nd_winograd_bench_flags(int tile, int kind, int batch, int cin, int cout, int h, int w, int iters, int flags, void *workspace,
                            size_t workspace_bytes, void *stream, float *mean_ms);

/* Name and average duration bookkeeping for bench.py: number of conv-kernel variants compiled in. */
int nd_num_conv_variants(void);
const char *nd_conv_variant_name(int variant);

#ifdef __cplusplus
}
#endif
#endif /* NIND_HIP_H */
