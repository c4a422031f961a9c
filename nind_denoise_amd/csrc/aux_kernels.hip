// HBM-bound helpers around the conv stack: tile geometry, tile gather (+mirror), stitch, layout conversion,
// max-pool, the final 1x1 convolution.  All are pure copies / max / short dot products: the roofline that bounds them
// is HBM bandwidth, so they read and write 16 B (or one full pixel row segment) per lane, coalesced along x.
#include "nd_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// One 16-byte plane element = the channels of one pixel in one plane: 4 x fp32, 8 x bf16 or 8 x fp16.
template <int DT> struct Elem { typedef f32x4 vec; static constexpr int N = 4; typedef float scalar; };
template <> struct Elem<ND_BF16> { typedef bf16x8 vec; static constexpr int N = 8; typedef __bf16 scalar; };
template <> struct Elem<ND_F16> { typedef f16x8 vec; static constexpr int N = 8; typedef _Float16 scalar; };
#define ND_DISPATCH_DT(dt, CALL)                     \
    switch (dt) {                                    \
        case ND_F32: { constexpr int DT = ND_F32; CALL; break; }   \
        case ND_BF16: { constexpr int DT = ND_BF16; CALL; break; } \
        case ND_F16: { constexpr int DT = ND_F16; CALL; break; }   \
        default: ND_FAIL(ND_EINVAL, "unsupported storage type %d", dt); \
    }

// ------------------------------------------------------------------ tile geometry (OneImageDS, denoise_image.py:100-143)
// TileGeo and the two index maps over it (nd_tile_source_map, nd_stitch_weight_map): nd_common.h
static int make_geo(int W, int H, int cs, int ucs, int ol, TileGeo *g) {
    if (W <= 0 || H <= 0 || cs <= 0 || ucs <= 0 || ol < 0) ND_FAIL(ND_EINVAL, "tile grid: non-positive size");
    if (ucs - ol <= 0) ND_FAIL(ND_EINVAL, "tile grid: ucs (%d) must exceed the overlap (%d)", ucs, ol);
    if (cs < ucs) ND_FAIL(ND_EINVAL, "tile grid: cs (%d) < ucs (%d)", cs, ucs);
    g->W = W; g->H = H; g->cs = cs; g->ucs = ucs; g->ol = ol;
    g->stride = ucs - ol;
    g->pad = (cs - ucs) / 2;                                 // int((cs-ucs)/2), denoise_image.py:102
    g->cols = ceil_div_py(W - ucs, g->stride) + 1;           // iperhl + 1, :101
    g->rows = ceil_div_py(H - ucs, g->stride) + 1;           // ipervl + 1, :103
    if (g->cols <= 0 || g->rows <= 0) ND_FAIL(ND_EINVAL, "tile grid: image %dx%d smaller than ucs=%d (undefined in the reference)", W, H, ucs);
    // mirrored strips must come from inside the image (the reference's numpy slices fail otherwise)
    const int x1pad = (g->cols - 1) * g->stride - g->pad + cs - W;
    const int y1pad = (g->rows - 1) * g->stride - g->pad + cs - H;
    if (g->pad > W || g->pad > H || x1pad > W || y1pad > H)
        ND_FAIL(ND_EINVAL, "tile grid: mirror padding (%d,%d,%d) exceeds the image %dx%d", g->pad, x1pad, y1pad, W, H);
    return ND_OK;
}

extern "C" int nd_tile_grid(int W, int H, int cs, int ucs, int ol, int *cols, int *rows, int *pad) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (cols) *cols = g.cols;
    if (rows) *rows = g.rows;
    if (pad) *pad = g.pad;
    return ND_OK;
}

extern "C" int nd_tile_geom(int i, int W, int H, int cs, int ucs, int ol, int *x0, int *y0, int ud[4], int us[2]) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (i < 0 || i >= g.cols * g.rows) ND_FAIL(ND_EINVAL, "tile index %d outside [0,%d)", i, g.cols * g.rows);
    const int yi = i / g.cols, xi = i - yi * g.cols;  // == int(ceil((i+1)/(iperhl+1) - 1)), :131-132
    const int tx0 = xi * g.stride - g.pad, ty0 = yi * g.stride - g.pad;
    const int x1pad = tx0 + cs - W > 0 ? tx0 + cs - W : 0;
    const int y1pad = ty0 + cs - H > 0 ? ty0 + cs - H : 0;
    if (x0) *x0 = tx0;
    if (y0) *y0 = ty0;
    if (ud) {
        ud[0] = g.pad;
        ud[1] = g.pad;
        ud[2] = cs - (g.pad > x1pad ? g.pad : x1pad);
        ud[3] = cs - (g.pad > y1pad ? g.pad : y1pad);
    }
    if (us) {
        us[0] = tx0 + g.pad;
        us[1] = ty0 + g.pad;
    }
    return ND_OK;
}

__device__ __forceinline__ int reflect_nr(int v, int n) {  // nn.ReflectionPad2d: edge pixel NOT repeated
    return v < 0 ? -v : (v >= n ? 2 * (n - 1) - v : v);
}

// ------------------------------------------------------------------ gather: image CHW -> tiles NCHW
__global__ void k_tile_gather(const float *__restrict__ img, TileGeo g, int tile_begin, float *__restrict__ out) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    const int t = blockIdx.z;
    if (xx >= g.cs) return;
    int sy, sx;
    nd_tile_source_map(g, tile_begin + t, yy, xx, &sy, &sx);
    const size_t plane = (size_t)g.W * g.H;
    const size_t tplane = (size_t)g.cs * g.cs;
    const float *s = img + (size_t)sy * g.W + sx;
    float *d = out + ((size_t)t * 3) * tplane + (size_t)yy * g.cs + xx;
    d[0] = s[0];
    d[tplane] = s[plane];
    d[2 * tplane] = s[2 * plane];
}

extern "C" int nd_tile_gather(const float *img, int W, int H, int cs, int ucs, int ol, int tile_begin, int tile_count,
                              float *tiles, void *stream) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (tile_count == 0) return ND_OK;
    if (!img || !tiles || tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > g.cols * g.rows)
        ND_FAIL(ND_EINVAL, "nd_tile_gather: tiles [%d,%d) outside the grid of %d", tile_begin, tile_begin + tile_count, g.cols * g.rows);
    dim3 grid((cs + 255) / 256, cs, tile_count);
    hipLaunchKernelGGL(k_tile_gather, grid, dim3(256), 0, (hipStream_t)stream, img, g, tile_begin, tiles);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// fused: gather(+symmetric mirror) -> quad-planar first-layer input (plane 0 = r,g,b,0) of Sb = cs + 2 * border lines.  reflect: every
// line, the border = ReflectionPad2d(border) of the tile (UtNet.py:27,98); else the cs interior lines only (UNet: the border is the
// zero padding of Conv2d(3, padding=1) and stays untouched)
template <int DT>
__global__ void k_gather_pack(const float *__restrict__ img, TileGeo g, int tile_begin, typename Elem<DT>::vec *__restrict__ dst, int Sb,
                              int border, int reflect) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;  // column in the bordered tile (reflect) or in the tile
    const int v = blockIdx.y;
    const int t = blockIdx.z;
    if (u >= (reflect ? Sb : g.cs)) return;
    const int i = tile_begin + t;
    const int yi = i / g.cols, xi = i - yi * g.cols;
    const int qx = reflect ? reflect_nr(u - border, g.cs) : u, qy = reflect ? reflect_nr(v - border, g.cs) : v;
    const int du = reflect ? u : u + border, dv = reflect ? v : v + border;
    const int sx = mirror_sym(xi * g.stride - g.pad + qx, g.W);
    const int sy = mirror_sym(yi * g.stride - g.pad + qy, g.H);
    const size_t plane = (size_t)g.W * g.H;
    const float *s = img + (size_t)sy * g.W + sx;
    typename Elem<DT>::vec o = {};
    o[0] = (typename Elem<DT>::scalar)s[0];
    o[1] = (typename Elem<DT>::scalar)s[plane];
    o[2] = (typename Elem<DT>::scalar)s[2 * plane];
    dst[((size_t)t * Sb + dv) * Sb + du] = o;
}

int nd_launch_gather_pack(const float *img, int W, int H, int cs, int ucs, int ol, int tile_begin, int tile_count,
                          const QpBuf &dst, hipStream_t s, int border, bool reflect) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (tile_begin < 0 || tile_count <= 0 || tile_begin + tile_count > g.cols * g.rows || tile_count > dst.B)
        ND_FAIL(ND_EINVAL, "gather_pack: bad tile range [%d,+%d)", tile_begin, tile_count);
    const int Sb = cs + 2 * border;
    // (a reflected border is part of the buffer's pixels: pad 0; a zero border is the buffer's own)
    if (border < 0 || border >= cs || dst.Hb != Sb || dst.Wb != Sb || dst.pad != (reflect ? 0 : border) || dst.used() > dst.np())
        ND_FAIL(ND_EINVAL, "gather_pack: destination is not (cs+%d)^2", 2 * border);
    const int n = reflect ? Sb : cs;
    dim3 grid((n + 255) / 256, n, tile_count);
    ND_DISPATCH_DT(dst.dt, hipLaunchKernelGGL(k_gather_pack<DT>, grid, dim3(256), 0, s, img, g, tile_begin,
                                              (typename Elem<DT>::vec *)dst.base, Sb, border, reflect ? 1 : 0));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ shared encoder (fp32): band gather, edge gather, splice
// Every gathered tile is the window of the symmetric-padded frame at its origin, so a band of tile rows is gathered as one image:
// band pixel (v, u) = frame pixel (by0 + v, bx0 + u) under the same mirror.  The outer ring that no tile reaches unpadded (the
// 2-pixel reflect border of the first and last tiles) only feeds lines the edge images recompute: it is clamped into the frame.
__device__ __forceinline__ int band_axis(int b0, int line, int n) {
    const int v = mirror_sym(b0 + line, n);
    return v < 0 ? 0 : (v >= n ? n - 1 : v);
}
// line `line` of the `len` first (side 0) or last (side 1) lines of tile index ti's reflect-padded input along one axis: gather +
// ReflectionPad2d(2), as k_gather_pack
__device__ __forceinline__ int tile_axis(const TileGeo &g, int ti, int line, int side, int len, int n) {
    return mirror_sym(ti * g.stride - g.pad + reflect_nr(line + (side ? g.cs + 4 - len : 0) - 2, g.cs), n);
}

__global__ void k_gather_band(const float *__restrict__ img, TileGeo g, int by0, int bx0, f32x4 *__restrict__ dst, int Hb, int Wb) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y;
    if (u >= Wb) return;
    const int sx = band_axis(bx0, u, g.W), sy = band_axis(by0, v, g.H);
    const size_t plane = (size_t)g.W * g.H;
    const float *s = img + (size_t)sy * g.W + sx;
    f32x4 o = {s[0], s[plane], s[2 * plane], 0.f};
    dst[(size_t)v * Wb + u] = o;
}

int nd_launch_gather_band(const float *img, int W, int H, int cs, int ucs, int ol, int band_row0, const QpBuf &dst, hipStream_t s) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (dst.dt != ND_F32 || dst.pad != 0 || dst.B != 1 || (long)dst.Hb * dst.Wb > dst.pstride || band_row0 < 0 || band_row0 >= g.rows)
        ND_FAIL(ND_EINVAL, "gather_band: bad destination / band row %d", band_row0);
    dim3 grid((dst.Wb + 255) / 256, dst.Hb);
    hipLaunchKernelGGL(k_gather_band, grid, dim3(256), 0, s, img, g, band_row0 * g.stride - g.pad - 2, -g.pad - 2, (f32x4 *)dst.base,
                       dst.Hb, dst.Wb);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// The first-layer input of the images that yield P2's border lines (nd_edge_set).  Along an axis an image either follows a tile's
// own input (tile_axis: its reflections included) or the band image (band_axis), so that its interior is a window of both:
//   ND_EDGE_ROWS     image 2 * yrel + side: the top / bottom Hs rows of tile row `first` + yrel, over the band's width
//   ND_EDGE_COLS     image 2 * xi + side: the left / right Ws columns of tile column xi, over the height of the band whose
//                    first tile row is `first`
//   ND_EDGE_CORNERS  image 4 * t + 2 * bottom + right: that Hs x Ws corner of tile `first` + t, reflected along both axes
__global__ void k_gather_edges(const float *__restrict__ img, TileGeo g, int set, int first, f32x4 *__restrict__ dst, int Hs, int Ws) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y;
    const int b = blockIdx.z;
    if (u >= Ws) return;
    int sx, sy;
    if (set == ND_EDGE_ROWS) {
        sy = tile_axis(g, first + (b >> 1), v, b & 1, Hs, g.H);
        sx = band_axis(-g.pad - 2, u, g.W);
    } else if (set == ND_EDGE_COLS) {
        sy = band_axis(first * g.stride - g.pad - 2, v, g.H);
        sx = tile_axis(g, b >> 1, u, b & 1, Ws, g.W);
    } else {
        const int i = first + (b >> 2), yi = i / g.cols, xi = i - yi * g.cols;
        sy = tile_axis(g, yi, v, (b >> 1) & 1, Hs, g.H);
        sx = tile_axis(g, xi, u, b & 1, Ws, g.W);
    }
    const size_t plane = (size_t)g.W * g.H;
    const float *s = img + (size_t)sy * g.W + sx;
    f32x4 o = {s[0], s[plane], s[2 * plane], 0.f};
    dst[((size_t)b * Hs + v) * Ws + u] = o;
}

// count: tile rows of the band from tile row `first` (ND_EDGE_ROWS, ND_EDGE_COLS) or tiles from tile `first` (ND_EDGE_CORNERS)
int nd_launch_gather_edges(const float *img, int W, int H, int cs, int ucs, int ol, int set, int first, int count, const QpBuf &dst,
                           hipStream_t s) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    const bool corners = set == ND_EDGE_CORNERS;
    // a tile axis takes lines [0, cs + 4) of a tile inside the grid (their mirror stays inside the frame: make_geo); a band axis
    // is clamped into the frame at any length
    bool ok = img && dst.base && dst.dt == ND_F32 && dst.pad == 0 && dst.Hb >= 1 && dst.Wb >= 1 && dst.used() <= dst.pstride &&
              dst.B <= 65535 && dst.Hb <= 65535 && first >= 0 && count > 0 && cs >= 3;
    if (set == ND_EDGE_ROWS) ok = ok && first + count <= g.rows && dst.B == 2 * count && dst.Hb <= cs + 4;
    else if (set == ND_EDGE_COLS) ok = ok && first + count <= g.rows && dst.B == 2 * g.cols && dst.Wb <= cs + 4;
    else ok = ok && corners && first + count <= g.cols * g.rows && dst.B == 4 * count && dst.Hb <= cs + 4 && dst.Wb <= cs + 4;
    if (!ok) ND_FAIL(ND_EINVAL, "gather_edges: bad set %d, range [%d,+%d) or destination", set, first, count);
    dim3 grid((dst.Wb + 255) / 256, dst.Hb, dst.B);
    hipLaunchKernelGGL(k_gather_edges, grid, dim3(256), 0, s, img, g, set, first, (f32x4 *)dst.base, dst.Hb, dst.Wb);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// One job: dst image dst_img0 + t, plane dst_p0 + p, interior pixel (r, c) of [r0, r1) x [c0, c1)  <-  src plane src_p0 + p, image
// m.img_t * t + m.img_y * yrel + m.img_x * xi + m.img_add, interior pixel (yrel * m.step_y + r + m.oy, xi * m.step_x + c + m.ox),
// (yi, xi) = grid position of tile tile_begin + t, yrel = yi - row0 (SpliceMap: nd_common.h).  band_rows > 0: the source holds bands
// of band_rows tile rows in two slots, slot_elems apart -- a tile reads band yi / band_rows in slot (band & 1), row0 = the band's
// first tile row (a launch may cross a band seam).
struct SpliceArgs {
    const f32x4 *src;
    f32x4 *dst;
    long src_np, dst_np;
    int src_Hb, src_Wb, src_pad, dst_Hb, dst_Wb, dst_pad;
    int tile_begin, tiles, cols, row0, r0, c0, rows, ccols, planes, dst_img0;
    SpliceMap m;
    int band_rows;
    long slot_elems;
};
// Up to kSpliceJobs jobs in one launch, by value in the kernel arguments.  A job's elements -- pixel of the region (row-major; a
// region may be one column wide) under plane under tile -- are dealt to consecutive threads, and job j owns blocks [first[j],
// first[j + 1]): a one-pixel or one-line job takes the blocks its elements fill, not a block per pixel, and no block is empty.
struct SpliceJobArgs {
    SpliceArgs job[kSpliceJobs];
    int first[kSpliceJobs + 1];
    int n;
};
__global__ __launch_bounds__(256) void k_splice_jobs(SpliceJobArgs ja) {
    int j = 0;
    while (j + 1 < ja.n && (int)blockIdx.x >= ja.first[j + 1]) ++j;   // (wave-uniform)
    const SpliceArgs &a = ja.job[j];
    const int npix = a.rows * a.ccols;
    const int e = ((int)blockIdx.x - ja.first[j]) * 256 + (int)threadIdx.x;
    const int y = e / npix, k = e - y * npix;
    const int t = y / a.planes, p = y - t * a.planes;
    if (t >= a.tiles) return;
    const int r = a.r0 + k / a.ccols, c = a.c0 + k % a.ccols;
    const int i = a.tile_begin + t;
    const int yi = i / a.cols, xi = i - yi * a.cols;
    const int band = a.band_rows > 0 ? yi / a.band_rows : 0, yrel = yi - (a.band_rows > 0 ? band * a.band_rows : a.row0);
    const int simg = a.m.img_t * t + a.m.img_y * yrel + a.m.img_x * xi + a.m.img_add;
    const int sy = yrel * a.m.step_y + r + a.m.oy + a.src_pad, sx = xi * a.m.step_x + c + a.m.ox + a.src_pad;
    const long si = (long)p * a.src_np + (band & 1) * a.slot_elems + ((long)simg * a.src_Hb + sy) * a.src_Wb + sx;
    a.dst[(long)p * a.dst_np + ((long)(a.dst_img0 + t) * a.dst_Hb + r + a.dst_pad) * a.dst_Wb + c + a.dst_pad] = a.src[si];
}

// two jobs write a common element: regions of one destination tensor that meet in planes, images, rows and columns; jobs on
// different views are held apart by the byte extents of their planes
static bool splice_jobs_overlap(const SpliceJob &a, const SpliceJob &b) {
    auto meet = [](long a0, long a1, long b0, long b1) { return a0 < b1 && b0 < a1; };
    const QpBuf &p = a.dst, &q = b.dst;
    if (p.base == q.base && p.Hb == q.Hb && p.Wb == q.Wb && p.pad == q.pad && p.np() == q.np())
        return meet(a.dst_p0, a.dst_p0 + a.planes, b.dst_p0, b.dst_p0 + b.planes) &&
               meet(a.dst_img0, a.dst_img0 + a.tile_count, b.dst_img0, b.dst_img0 + b.tile_count) && meet(a.r0, a.r1, b.r0, b.r1) &&
               meet(a.c0, a.c1, b.c0, b.c1);
    const uintptr_t pa = (uintptr_t)p.base, pb = (uintptr_t)q.base;
    return meet(pa + (size_t)a.dst_p0 * p.np() * 16, pa + (size_t)(a.dst_p0 + a.planes) * p.np() * 16, pb + (size_t)b.dst_p0 * q.np() * 16,
                pb + (size_t)(b.dst_p0 + b.planes) * q.np() * 16);
}

int nd_launch_splices(const SpliceJob *jobs, int n, hipStream_t s) {
    if (!jobs || n < 1 || n > kSpliceJobs) ND_FAIL(ND_EINVAL, "splice: %d jobs in one launch (1 ... %d)", n, kSpliceJobs);
    SpliceJobArgs ja;
    long blocks = 0;
    for (int j = 0; j < n; ++j) {
        const SpliceJob &q = jobs[j];
        const QpBuf &src = q.src, &dst = q.dst;
        const int sH = src.Hb - 2 * src.pad, sW = src.Wb - 2 * src.pad, dH = dst.Hb - 2 * dst.pad, dW = dst.Wb - 2 * dst.pad;
        bool ok = src.base && dst.base && src.dt == ND_F32 && dst.dt == ND_F32 && q.tile_begin >= 0 && q.cols > 0 && q.tile_count > 0 &&
                  q.dst_img0 >= 0 && q.dst_img0 + q.tile_count <= dst.B && dst.used() <= dst.np() && src.used() <= src.np() && q.planes > 0 &&
                  q.src_p0 >= 0 && q.src_p0 + q.planes <= src.planes && q.dst_p0 >= 0 && q.dst_p0 + q.planes <= dst.planes &&
                  q.r0 >= 0 && q.c0 >= 0 && q.r1 > q.r0 && q.c1 > q.c0 && q.r1 <= dH && q.c1 <= dW && q.band_rows >= 0 &&
                  (q.band_rows == 0 || q.slot_elems >= 0);
        // the elements of a job are numbered in 32 bits
        const long elems = ok ? (long)q.tile_count * q.planes * (q.r1 - q.r0) * (q.c1 - q.c0) : 0;
        ok = ok && elems <= 0x7fffffffL - 256;
        // the source image and window of every tile of the job (a launch has at most a few hundred tiles)
        for (int t = 0; t < q.tile_count && ok; ++t) {
            const int yi = (q.tile_begin + t) / q.cols, xi = (q.tile_begin + t) % q.cols;
            const int yrel = yi - (q.band_rows > 0 ? yi / q.band_rows * q.band_rows : q.row0);
            const int simg = q.m.img_t * t + q.m.img_y * yrel + q.m.img_x * xi + q.m.img_add, y = yrel * q.m.step_y + q.m.oy,
                      x = xi * q.m.step_x + q.m.ox;
            if (q.band_rows > 0 && (yi / q.band_rows & 1)) ok = q.slot_elems >= src.used() && q.slot_elems + src.used() <= src.np();
            ok = ok && yrel >= 0 && simg >= 0 && simg < src.B && y + q.r0 >= 0 && y + q.r1 - 1 < sH && x + q.c0 >= 0 && x + q.c1 - 1 < sW;
        }
        if (!ok) ND_FAIL(ND_EINVAL, "splice: job %d, region [%d,%d) x [%d,%d) of %d tiles x %d planes outside its source / destination", j,
                         q.r0, q.r1, q.c0, q.c1, q.tile_count, q.planes);
        for (int i = 0; i < j; ++i)
            if (splice_jobs_overlap(jobs[i], q)) ND_FAIL(ND_EINVAL, "splice: jobs %d and %d write overlapping regions", i, j);
        SpliceArgs &a = ja.job[j];
        a.src = (const f32x4 *)src.base + (long)q.src_p0 * src.np();
        a.dst = (f32x4 *)dst.base + (long)q.dst_p0 * dst.np();
        a.src_np = src.np(); a.dst_np = dst.np();
        a.src_Hb = src.Hb; a.src_Wb = src.Wb; a.src_pad = src.pad;
        a.dst_Hb = dst.Hb; a.dst_Wb = dst.Wb; a.dst_pad = dst.pad;
        a.tile_begin = q.tile_begin; a.tiles = q.tile_count; a.cols = q.cols; a.row0 = q.row0; a.m = q.m; a.dst_img0 = q.dst_img0;
        a.r0 = q.r0; a.c0 = q.c0; a.rows = q.r1 - q.r0; a.ccols = q.c1 - q.c0; a.planes = q.planes;
        a.band_rows = q.band_rows; a.slot_elems = q.slot_elems;
        ja.first[j] = (int)blocks;
        blocks += (elems + 255) / 256;
        // (a grid holds fewer than 2^32 threads)
        if (blocks * 256 >= (1L << 32)) ND_FAIL(ND_EINVAL, "splice: %ld blocks of 256 threads in one launch", blocks);
    }
    for (int j = n; j < kSpliceJobs; ++j) ja.job[j] = ja.job[0];   // (never read)
    for (int j = n; j <= kSpliceJobs; ++j) ja.first[j] = (int)blocks;
    ja.n = n;
    hipLaunchKernelGGL(k_splice_jobs, dim3((unsigned)blocks), dim3(256), 0, s, ja);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_launch_splice(const QpBuf &src, int src_p0, const QpBuf &dst, int dst_p0, int planes, int tile_begin, int tile_count, int cols,
                     int row0, const SpliceMap &m, int r0, int r1, int c0, int c1, hipStream_t s, int band_rows, long slot_elems,
                     int dst_img0) {
    const SpliceJob q = nd_splice_job(src, src_p0, dst, dst_p0, planes, tile_begin, tile_count, cols, row0, m, r0, r1, c0, c1, band_rows,
                                      slot_elems, dst_img0);
    return nd_launch_splices(&q, 1, s);
}

// The conv kernels that read a skip half in place (ConvDesc::in2) take the tile's place in the band plane from a table in HBM: the
// division by `cols` and the band bookkeeping stay out of them.  One thread per tile of the launch.
__host__ __device__ static inline long skip_origin(int i, int cols, int band_rows, int step, int Wb, int dpad, long slot_elems) {
    const int yi = i / cols, xi = i - yi * cols, band = yi / band_rows;
    return (band & 1) * slot_elems + (long)((yi - band * band_rows) * step + dpad) * Wb + xi * step + dpad;
}
__global__ void k_skip_origins(int tile_begin, int tile_count, int cols, int band_rows, int step, int Wb, int dpad, long slot_elems,
                               int *__restrict__ table) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tile_count) return;
    table[t] = (int)skip_origin(tile_begin + t, cols, band_rows, step, Wb, dpad, slot_elems);
}

int nd_launch_skip_origins(const QpBuf &src, int dst_pad, int tile_begin, int tile_count, int cols, int band_rows, int step, long slot_elems,
                           int *table, long *origin_max, hipStream_t s) {
    const int dpad = src.pad - dst_pad;
    if (!table || tile_begin < 0 || tile_count <= 0 || cols <= 0 || band_rows <= 0 || step < 0 || dpad < 0 || slot_elems < 0 || src.B != 1)
        ND_FAIL(ND_EINVAL, "skip_origins: bad tile range [%d,+%d) / %d rows per band", tile_begin, tile_count, band_rows);
    long omax = 0;
    for (int t = 0; t < tile_count; ++t) {
        const long o = skip_origin(tile_begin + t, cols, band_rows, step, src.Wb, dpad, slot_elems);
        omax = o > omax ? o : omax;
    }
    if (omax >= (1L << 31)) ND_FAIL(ND_EINVAL, "skip_origins: origin %ld exceeds 32 bits", omax);
    if (origin_max) *origin_max = omax;
    hipLaunchKernelGGL(k_skip_origins, dim3((tile_count + 255) / 256), dim3(256), 0, s, tile_begin, tile_count, cols, band_rows, step, src.Wb,
                       dpad, slot_elems, table);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ stitch (denoise_image.py:204-213, 249-267)
// One thread per canvas pixel; contributions of the tiles [tile_begin, tile_begin+count) that cover it are added in
// ascending tile index order on top of the current canvas value: the fp32 sum order of the reference's loop.
struct Cover {
    int t;      // tile index relative to tile_begin
    int iy, ix; // position inside the tile
    float f;    // 1, .5 or .25 (seamless edges)
};

template <typename F>
__device__ __forceinline__ void for_each_cover(const TileGeo &g, int X, int Y, int tile_begin, int tile_count, F &&fn) {
    const int uwmax = g.cs - 2 * g.pad;
    int yi_lo = ceil_div_py(Y - uwmax + 1, g.stride);
    if (yi_lo < 0) yi_lo = 0;
    int yi_hi = Y / g.stride;
    if (yi_hi > g.rows - 1) yi_hi = g.rows - 1;
    int xi_lo = ceil_div_py(X - uwmax + 1, g.stride);
    if (xi_lo < 0) xi_lo = 0;
    int xi_hi = X / g.stride;
    if (xi_hi > g.cols - 1) xi_hi = g.cols - 1;
    for (int yi = yi_lo; yi <= yi_hi; ++yi) {
        const int ay = yi * g.stride;
        const int y1pad = max(0, ay - g.pad + g.cs - g.H);
        const int uh = g.cs - max(g.pad, y1pad) - g.pad;
        const int dy = Y - ay;
        if (dy >= uh) continue;
        float fy = 1.f;
        if (ay != 0 && dy < g.ol) fy *= 0.5f;
        if (ay + g.ucs < g.H && g.ol && dy >= uh - g.ol) fy *= 0.5f;
        for (int xi = xi_lo; xi <= xi_hi; ++xi) {
            const int i = yi * g.cols + xi;
            if (i < tile_begin || i >= tile_begin + tile_count) continue;
            const int ax = xi * g.stride;
            const int x1pad = max(0, ax - g.pad + g.cs - g.W);
            const int uw = g.cs - max(g.pad, x1pad) - g.pad;
            const int dx = X - ax;
            if (dx >= uw) continue;
            float f = fy;
            if (ax != 0 && dx < g.ol) f *= 0.5f;
            if (ax + g.ucs < g.W && g.ol && dx >= uw - g.ol) f *= 0.5f;
            fn(i - tile_begin, g.pad + dy, g.pad + dx, f);
        }
    }
}

__global__ void k_stitch_add(float *__restrict__ canvas, TileGeo g, const float *__restrict__ tiles, int tile_begin,
                             int tile_count, int y_first) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    const int Y = y_first + blockIdx.y;
    if (X >= g.W || Y >= g.H) return;
    const size_t plane = (size_t)g.W * g.H;
    const size_t tplane = (size_t)g.cs * g.cs;
    float *c = canvas + (size_t)Y * g.W + X;
    float v0 = c[0], v1 = c[plane], v2 = c[2 * plane];
    bool any = false;
    for_each_cover(g, X, Y, tile_begin, tile_count, [&](int t, int iy, int ix, float f) {
        const float *s = tiles + (size_t)t * 3 * tplane + (size_t)iy * g.cs + ix;
        v0 += s[0] * f;
        v1 += s[tplane] * f;
        v2 += s[2 * tplane] * f;
        any = true;
    });
    if (any) {
        c[0] = v0;
        c[plane] = v1;
        c[2 * plane] = v2;
    }
}

static void stitch_band(const TileGeo &g, int tile_begin, int tile_count, int *y_first, int *y_rows) {
    const int yi0 = tile_begin / g.cols, yi1 = (tile_begin + tile_count - 1) / g.cols;
    const int uwmax = g.cs - 2 * g.pad;
    int y0 = yi0 * g.stride, y1 = yi1 * g.stride + uwmax;
    if (y1 > g.H) y1 = g.H;
    *y_first = y0;
    *y_rows = y1 - y0;
}

extern "C" int nd_stitch_add(float *canvas, int W, int H, int cs, int ucs, int ol, const float *tiles, int tile_begin,
                             int tile_count, void *stream) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (tile_count == 0) return ND_OK;
    if (!canvas || !tiles || tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > g.cols * g.rows)
        ND_FAIL(ND_EINVAL, "nd_stitch_add: tiles [%d,%d) outside the grid of %d", tile_begin, tile_begin + tile_count, g.cols * g.rows);
    int yf, yr;
    stitch_band(g, tile_begin, tile_count, &yf, &yr);
    if (yr <= 0) return ND_OK;
    dim3 grid((W + 255) / 256, yr);
    hipLaunchKernelGGL(k_stitch_add, grid, dim3(256), 0, (hipStream_t)stream, canvas, g, tiles, tile_begin, tile_count, yf);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ adjoints of gather and stitch (gradients through a tiled frame)
// Both operators are linear, so their adjoints are the transposed index maps: the stitch's is a gather from the canvas gradient,
// the gather's a sum over the tile pixels that read a frame pixel.  Neither uses atomics: every output element has one thread,
// which adds its terms in a fixed order.
extern "C" int nd_tile_source(int i, int W, int H, int cs, int ucs, int ol, int y, int x, int *Y, int *X) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (!Y || !X) ND_FAIL(ND_EINVAL, "nd_tile_source: null output pointer");
    if (i < 0 || i >= g.cols * g.rows || y < 0 || y >= cs || x < 0 || x >= cs)
        ND_FAIL(ND_EINVAL, "nd_tile_source: tile %d of %d, pixel (%d, %d) of a %d-pixel tile", i, g.cols * g.rows, y, x, cs);
    nd_tile_source_map(g, i, y, x, Y, X);
    return ND_OK;
}

extern "C" int nd_stitch_weight(int i, int W, int H, int cs, int ucs, int ol, int y, int x, int *Y, int *X, float *w) {
    TileGeo g;
    ND_TRY(make_geo(W, H, cs, ucs, ol, &g));
    if (!Y || !X || !w) ND_FAIL(ND_EINVAL, "nd_stitch_weight: null output pointer");
    if (i < 0 || i >= g.cols * g.rows || y < 0 || y >= cs || x < 0 || x >= cs)
        ND_FAIL(ND_EINVAL, "nd_stitch_weight: tile %d of %d, pixel (%d, %d) of a %d-pixel tile", i, g.cols * g.rows, y, x, cs);
    *w = nd_stitch_weight_map(g, i, y, x, Y, X);
    return ND_OK;
}

// the checks the two adjoint entry points share; *run = false: nothing to launch (tile_count 0)
static int check_tile_range(const char *who, const void *a, const void *b, int W, int H, int cs, int ucs, int ol, int tile_begin,
                            int tile_count, TileGeo *g, bool *run) {
    ND_TRY(make_geo(W, H, cs, ucs, ol, g));
    *run = false;
    if (tile_begin < 0 || tile_count < 0 || tile_begin > g->cols * g->rows - tile_count)
        ND_FAIL(ND_EINVAL, "%s: tiles [%d,%d) outside the grid of %d", who, tile_begin, tile_begin + tile_count, g->cols * g->rows);
    if (tile_count == 0) return ND_OK;
    if (!a || !b) ND_FAIL(ND_EINVAL, "%s: null pointer", who);
    if (cs > 16384 || tile_count > 65535) ND_FAIL(ND_EINVAL, "%s: cs %d above 16384 or %d tiles above 65535 in one launch", who, cs, tile_count);
    *run = true;
    return ND_OK;
}

// gtiles[t, c, y, x] = w * gcanvas[c, Y, X] over nd_stitch_weight_map; every element of the launch's tiles is written (0 where w = 0)
__global__ void k_stitch_grad(const float *__restrict__ gcanvas, TileGeo g, int tile_begin, int tile_count, float *__restrict__ gtiles) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int t = blockIdx.z;
    if (x >= g.cs || y >= g.cs || t >= tile_count) return;
    const int i = tile_begin + t;
    const size_t plane = (size_t)g.W * g.H;
    const size_t tplane = (size_t)g.cs * g.cs;
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
    if (i >= 0 && i < g.cols * g.rows) {
        int Y, X;
        const float w = nd_stitch_weight_map(g, i, y, x, &Y, &X);
        if (w != 0.f && X >= 0 && X < g.W && Y >= 0 && Y < g.H) {
            const float *s = gcanvas + (size_t)Y * g.W + X;
            v0 = w * s[0];
            v1 = w * s[plane];
            v2 = w * s[2 * plane];
        }
    }
    float *d = gtiles + (size_t)t * 3 * tplane + (size_t)y * g.cs + x;
    d[0] = v0;
    d[tplane] = v1;
    d[2 * tplane] = v2;
}

extern "C" int nd_stitch_grad(const float *gcanvas, int W, int H, int cs, int ucs, int ol, int tile_begin, int tile_count,
                              float *gtiles, void *stream) {
    TileGeo g;
    bool run;
    ND_TRY(check_tile_range("nd_stitch_grad", gcanvas, gtiles, W, H, cs, ucs, ol, tile_begin, tile_count, &g, &run));
    if (!run) return ND_OK;
    dim3 grid((cs + 255) / 256, cs, tile_count);
    hipLaunchKernelGGL(k_stitch_grad, grid, dim3(256), 0, (hipStream_t)stream, gcanvas, g, tile_begin, tile_count, gtiles);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// The tile rows (columns) k in [0, count) whose window [k * stride - pad, k * stride - pad + cs) holds a pre-image of frame
// coordinate V under mirror_sym: the hull of the three ranges of u = -1 - V (fold over the first edge), V (direct) and
// 2n - 1 - V (fold over the last edge).  Tiles inside the hull that hold none are skipped by the caller's per-tile test.
__host__ __device__ static inline void preimage_tiles(const TileGeo &g, int V, int n, int count, int *lo, int *hi) {
    const int us[3] = {-1 - V, V, 2 * n - 1 - V};
    int l = count, h = -1;
    for (int k = 0; k < 3; ++k) {
        const int top = us[k] + g.pad;                              // k * stride <= top  and  k * stride > top - cs
        if (top < 0) continue;
        int a = ceil_div_py(top - g.cs + 1, g.stride), b = top / g.stride;
        if (a < 0) a = 0;
        if (b > count - 1) b = count - 1;
        if (a > b) continue;
        if (a < l) l = a;
        if (b > h) h = b;
    }
    *lo = l;
    *hi = h;
}

// gimg[c, Y, X] += sum of gtiles over the tile pixels of the launch that nd_tile_source_map sends to (Y, X): one thread per frame
// pixel of the launch's footprint box.  Order of the sum: ascending tile index; within a tile ascending y * cs + x over its at most
// 3 x 3 pre-images (fold over the first edge, direct, fold over the last edge, per axis -- ascending u is ascending tile coordinate).
__global__ void k_tile_gather_grad(const float *__restrict__ gtiles, TileGeo g, int tile_begin, int tile_count, int bx0, int by0,
                                   int bw, int bh, float *__restrict__ gimg) {
    const int X = bx0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (X >= bx0 + bw || X < 0 || X >= g.W) return;
    const size_t plane = (size_t)g.W * g.H;
    const size_t tplane = (size_t)g.cs * g.cs;
    const int yi_first = tile_begin / g.cols, yi_last = (tile_begin + tile_count - 1) / g.cols;
    int xi_lo, xi_hi;
    preimage_tiles(g, X, g.W, g.cols, &xi_lo, &xi_hi);
    const int ux[3] = {-1 - X, X, 2 * g.W - 1 - X};
    for (int Y = by0 + blockIdx.y; Y < by0 + bh; Y += gridDim.y) {
        if (Y < 0 || Y >= g.H) continue;
        int yi_lo, yi_hi;
        preimage_tiles(g, Y, g.H, g.rows, &yi_lo, &yi_hi);
        if (yi_lo < yi_first) yi_lo = yi_first;
        if (yi_hi > yi_last) yi_hi = yi_last;
        const int uy[3] = {-1 - Y, Y, 2 * g.H - 1 - Y};
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        bool any = false;
        for (int yi = yi_lo; yi <= yi_hi; ++yi) {
            for (int xi = xi_lo; xi <= xi_hi; ++xi) {
                const int t = yi * g.cols + xi - tile_begin;
                if (t < 0 || t >= tile_count) continue;
                const float *tile = gtiles + (size_t)t * 3 * tplane;
                for (int a = 0; a < 3; ++a) {
                    const int y = uy[a] - (yi * g.stride - g.pad);
                    if (y < 0 || y >= g.cs) continue;
                    for (int b = 0; b < 3; ++b) {
                        const int x = ux[b] - (xi * g.stride - g.pad);
                        if (x < 0 || x >= g.cs) continue;
                        const float *s = tile + (size_t)y * g.cs + x;
                        v0 += s[0];
                        v1 += s[tplane];
                        v2 += s[2 * tplane];
                        any = true;
                    }
                }
            }
        }
        if (any) {
            float *d = gimg + (size_t)Y * g.W + X;
            d[0] += v0;
            d[plane] += v1;
            d[2 * plane] += v2;
        }
    }
}

// the frame rows (columns) that tiles k0 .. k1 of an axis and their folds reach: [*lo, *hi)
static void footprint_axis(const TileGeo &g, int k0, int k1, int n, int *lo, int *hi) {
    int l = n, h = 0;
    for (int k = k0; k <= k1; ++k) {
        const int u0 = k * g.stride - g.pad, u1 = u0 + g.cs;
        int a = u0 < 0 ? 0 : u0, b = u1 > n ? n : u1;               // direct part; the fold over the first edge, [0, -u0), lies inside it
        if (u1 > n && 2 * n - u1 < a) a = 2 * n - u1;               // fold over the last edge: [2n - u1, n)
        if (a < 0) a = 0;
        if (a < l) l = a;
        if (b > h) h = b;
    }
    *lo = l;
    *hi = h;
}

extern "C" int nd_tile_gather_grad(const float *gtiles, int W, int H, int cs, int ucs, int ol, int tile_begin, int tile_count,
                                   float *gimg, void *stream) {
    TileGeo g;
    bool run;
    ND_TRY(check_tile_range("nd_tile_gather_grad", gtiles, gimg, W, H, cs, ucs, ol, tile_begin, tile_count, &g, &run));
    if (!run) return ND_OK;
    // footprint box: the rows of the launch's tile rows; the columns of its tiles where they lie in one tile row, else of every column
    const int yi0 = tile_begin / g.cols, yi1 = (tile_begin + tile_count - 1) / g.cols;
    const int xi0 = yi0 == yi1 ? tile_begin - yi0 * g.cols : 0, xi1 = yi0 == yi1 ? tile_begin + tile_count - 1 - yi0 * g.cols : g.cols - 1;
    int bx0, bx1, by0, by1;
    footprint_axis(g, xi0, xi1, W, &bx0, &bx1);
    footprint_axis(g, yi0, yi1, H, &by0, &by1);
    if (bx1 <= bx0 || by1 <= by0) return ND_OK;
    const int bh = by1 - by0;
    dim3 grid((bx1 - bx0 + 255) / 256, bh < 65535 ? bh : 65535);
    hipLaunchKernelGGL(k_tile_gather_grad, grid, dim3(256), 0, (hipStream_t)stream, gtiles, g, tile_begin, tile_count, bx0, by0, bx1 - bx0,
                       bh, gimg);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ layout conversion NCHW <-> quad-planar
template <int DT>
__global__ void k_nchw_to_qp(const float *__restrict__ x, int C, int H, int W, typename Elem<DT>::vec *__restrict__ dst,
                             long np, int Hb, int Wb, int pad, int plane0) {
    constexpr int N = Elem<DT>::N;
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    const int q = blockIdx.z % ((C + N - 1) / N), b = blockIdx.z / ((C + N - 1) / N);
    if (xx >= W) return;
    typename Elem<DT>::vec o;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int c = N * q + e;
        o[e] = (typename Elem<DT>::scalar)(c < C ? x[(((size_t)b * C + c) * H + yy) * W + xx] : 0.f);
    }
    dst[(size_t)(plane0 + q) * np + ((size_t)b * Hb + yy + pad) * Wb + xx + pad] = o;
}

int nd_launch_nchw_to_qp(const float *x, int C, const QpBuf &dst, int plane0, hipStream_t s) {
    const int H = dst.Hb - 2 * dst.pad, W = dst.Wb - 2 * dst.pad;
    const int n = nd_cpp(dst.dt);
    dim3 grid((W + 255) / 256, H, dst.B * ((C + n - 1) / n));
    ND_DISPATCH_DT(dst.dt, hipLaunchKernelGGL(k_nchw_to_qp<DT>, grid, dim3(256), 0, s, x, C, H, W,
                                              (typename Elem<DT>::vec *)dst.base, dst.np(), dst.Hb, dst.Wb, dst.pad, plane0));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

template <int DT>
__global__ void k_qp_to_nchw(const typename Elem<DT>::vec *__restrict__ src, long np, int Hb, int Wb, int pad, int plane0,
                             float *__restrict__ y, int C, int H, int W) {
    constexpr int N = Elem<DT>::N;
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    const int q = blockIdx.z % ((C + N - 1) / N), b = blockIdx.z / ((C + N - 1) / N);
    if (xx >= W) return;
    const typename Elem<DT>::vec v = src[(size_t)(plane0 + q) * np + ((size_t)b * Hb + yy + pad) * Wb + xx + pad];
#pragma unroll
    for (int e = 0; e < N; ++e) {
        const int c = N * q + e;
        if (c < C) y[(((size_t)b * C + c) * H + yy) * W + xx] = (float)v[e];
    }
}

int nd_launch_qp_to_nchw(const QpBuf &src, int plane0, float *y, int C, hipStream_t s) {
    const int H = src.Hb - 2 * src.pad, W = src.Wb - 2 * src.pad;
    const int n = nd_cpp(src.dt);
    dim3 grid((W + 255) / 256, H, src.B * ((C + n - 1) / n));
    ND_DISPATCH_DT(src.dt, hipLaunchKernelGGL(k_qp_to_nchw<DT>, grid, dim3(256), 0, s, (const typename Elem<DT>::vec *)src.base,
                                              src.np(), src.Hb, src.Wb, src.pad, plane0, y, C, H, W));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// x [B,3,H,W] -> ReflectionPad2d(2) (UtNet.py:27,98) -> plane 0 of the first-layer input [(H+4) x (W+4)]
template <int DT>
__global__ void k_reflect_pack(const float *__restrict__ x, int H, int W, typename Elem<DT>::vec *__restrict__ dst) {
    const int Hb = H + 4, Wb = W + 4;
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    const int v = blockIdx.y, b = blockIdx.z;
    if (u >= Wb) return;
    const int qx = reflect_nr(u - 2, W), qy = reflect_nr(v - 2, H);
    const size_t plane = (size_t)H * W;
    const float *s = x + ((size_t)b * 3 * H + qy) * W + qx;
    typename Elem<DT>::vec o = {};
    o[0] = (typename Elem<DT>::scalar)s[0];
    o[1] = (typename Elem<DT>::scalar)s[plane];
    o[2] = (typename Elem<DT>::scalar)s[2 * plane];
    dst[((size_t)b * Hb + v) * Wb + u] = o;
}

int nd_launch_reflect_pack(const float *x, int B, int H, int W, const QpBuf &dst, hipStream_t s) {
    if (dst.Hb != H + 4 || dst.Wb != W + 4 || dst.pad != 0 || B > dst.B) ND_FAIL(ND_EINVAL, "reflect_pack: bad destination");
    dim3 grid((W + 4 + 255) / 256, H + 4, B);
    ND_DISPATCH_DT(dst.dt, hipLaunchKernelGGL(k_reflect_pack<DT>, grid, dim3(256), 0, s, x, H, W, (typename Elem<DT>::vec *)dst.base));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ MaxPool2d(2) (UtNet.py:34), quad-planar
template <int DT>
__global__ void k_maxpool2(const typename Elem<DT>::vec *__restrict__ src, long snp, int sHb, int sWb, int spad, int splane0,
                           typename Elem<DT>::vec *__restrict__ dst, long dnp, int dHb, int dWb, int dpad, int Ho, int Wo, int B) {
    typedef typename Elem<DT>::vec V;
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y;
    const int b = blockIdx.z % B, q = blockIdx.z / B;
    if (xx >= Wo) return;
    const V *s = src + (size_t)(splane0 + q) * snp + ((size_t)b * sHb + 2 * yy + spad) * sWb + 2 * xx + spad;
    const V a = s[0], c = s[1], d = s[sWb], e = s[sWb + 1];
    V o;
#pragma unroll
    for (int k = 0; k < Elem<DT>::N; ++k)
        o[k] = (typename Elem<DT>::scalar)fmaxf(fmaxf((float)a[k], (float)c[k]), fmaxf((float)d[k], (float)e[k]));
    dst[(size_t)q * dnp + ((size_t)b * dHb + yy + dpad) * dWb + xx + dpad] = o;
}

int nd_launch_maxpool2(const QpBuf &src, int src_plane0, int planes, const QpBuf &dst, hipStream_t s) {
    const int Hi = src.Hb - 2 * src.pad, Wi = src.Wb - 2 * src.pad;
    const int Ho = Hi / 2, Wo = Wi / 2;
    if (dst.Hb - 2 * dst.pad != Ho || dst.Wb - 2 * dst.pad != Wo || dst.B != src.B || dst.planes < planes || dst.dt != src.dt)
        ND_FAIL(ND_EINVAL, "maxpool2: destination does not fit %dx%d", Ho, Wo);
    dim3 grid((Wo + 127) / 128, Ho, src.B * planes);
    ND_DISPATCH_DT(src.dt, hipLaunchKernelGGL(k_maxpool2<DT>, grid, dim3(128), 0, s, (const typename Elem<DT>::vec *)src.base,
                                              src.np(), src.Hb, src.Wb, src.pad, src_plane0, (typename Elem<DT>::vec *)dst.base,
                                              dst.np(), dst.Hb, dst.Wb, dst.pad, Ho, Wo, src.B));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ final Conv2d(funit,3,1) + ZeroPad2d(-2) (UtNet.py:86,88)
// w: [3][cin] (torch layout), bias [3].  One thread per output pixel; each plane read is a coalesced float4 stream.
template <int DT>
__device__ __forceinline__ void dot3(const typename Elem<DT>::vec *__restrict__ s, long np, int planes,
                                     const float *__restrict__ w, int cin, float &o0, float &o1, float &o2) {
    constexpr int N = Elem<DT>::N;
    for (int q = 0; q < planes; ++q) {
        const typename Elem<DT>::vec v = s[(size_t)q * np];
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const int c = N * q + e;
            if (c < cin) {
                const float f = (float)v[e];
                o0 = fmaf(f, w[c], o0);
                o1 = fmaf(f, w[cin + c], o1);
                o2 = fmaf(f, w[2 * cin + c], o2);
            }
        }
    }
}

template <int DT>
__global__ void k_final1x1(const typename Elem<DT>::vec *__restrict__ src, long np, int Hb, int Wb, int planes, int cin,
                           const float *__restrict__ w, const float *__restrict__ bias, int crop, float *__restrict__ y,
                           int H, int W, int sigmoid) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    const int yy = blockIdx.y, b = blockIdx.z;
    if (xx >= W) return;
    float o0 = bias[0], o1 = bias[1], o2 = bias[2];
    dot3<DT>(src + ((size_t)b * Hb + yy + crop) * Wb + xx + crop, np, planes, w, cin, o0, o1, o2);
    if (sigmoid) {   // UNet head (ThirdPartyNets.py:169)
        o0 = 1.f / (1.f + expf(-o0));
        o1 = 1.f / (1.f + expf(-o1));
        o2 = 1.f / (1.f + expf(-o2));
    }
    float *d = y + ((size_t)b * 3 * H + yy) * W + xx;
    d[0] = o0;
    d[(size_t)H * W] = o1;
    d[2 * (size_t)H * W] = o2;
}

int nd_launch_final1x1(const QpBuf &src, int cin, const float *w, const float *bias, int crop, float *y, int H, int W,
                       hipStream_t s, int sigmoid) {
    if (src.pad != 0 || src.Hb != H + 2 * crop || src.Wb != W + 2 * crop) ND_FAIL(ND_EINVAL, "final1x1: bad source geometry");
    dim3 grid((W + 255) / 256, H, src.B);
    const int n = nd_cpp(src.dt);
    ND_DISPATCH_DT(src.dt, hipLaunchKernelGGL(k_final1x1<DT>, grid, dim3(256), 0, s, (const typename Elem<DT>::vec *)src.base,
                                              src.np(), src.Hb, src.Wb, (cin + n - 1) / n, cin, w, bias, crop, y, H, W, sigmoid));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// fused: final 1x1 (+ Sigmoid) + crop + useful crop + seamless edges + canvas += (no NCHW tile batch in HBM).  noise_img: the
// contribution of a tile is frame pixel - result (UNet's find_noise; a useful pixel of a tile is the frame's pixel (Y, X) itself).
// GUARD (the checked frame loop): a covering tile whose tile_ok[global tile index] is 0 is skipped, and a pixel that no good
// tile of the launch covers is not written.  The unguarded form never reads tile_ok
template <int DT, bool GUARD>
__device__ __forceinline__ void final1x1_stitch_pixel(const typename Elem<DT>::vec *__restrict__ src, long np, int Hb, int Wb, int planes,
                                                      int cin, const float *__restrict__ w, const float *__restrict__ bias, int crop,
                                                      float *__restrict__ canvas, const TileGeo &g, int tile_begin, int tile_count,
                                                      int y_first, int sigmoid, const float *__restrict__ noise_img,
                                                      const unsigned char *__restrict__ tile_ok) {
    const int X = blockIdx.x * blockDim.x + threadIdx.x;
    const int Y = y_first + blockIdx.y;
    if (X >= g.W || Y >= g.H) return;
    const size_t plane = (size_t)g.W * g.H;
    float *c = canvas + (size_t)Y * g.W + X;
    float v0 = c[0], v1 = c[plane], v2 = c[2 * plane];
    float n0 = 0.f, n1 = 0.f, n2 = 0.f;
    if (noise_img) {
        const float *n = noise_img + (size_t)Y * g.W + X;
        n0 = n[0]; n1 = n[plane]; n2 = n[2 * plane];
    }
    bool any = false;
    for_each_cover(g, X, Y, tile_begin, tile_count, [&](int t, int iy, int ix, float f) {
        if (GUARD && !tile_ok[tile_begin + t]) return;
        float o0 = bias[0], o1 = bias[1], o2 = bias[2];
        dot3<DT>(src + ((size_t)t * Hb + iy + crop) * Wb + ix + crop, np, planes, w, cin, o0, o1, o2);
        if (sigmoid) {   // UNet head (ThirdPartyNets.py:169), as k_final1x1
            o0 = 1.f / (1.f + expf(-o0));
            o1 = 1.f / (1.f + expf(-o1));
            o2 = 1.f / (1.f + expf(-o2));
        }
        if (noise_img) {   // ThirdPartyNets.py:168
            o0 = n0 - o0;
            o1 = n1 - o1;
            o2 = n2 - o2;
        }
        v0 += o0 * f;
        v1 += o1 * f;
        v2 += o2 * f;
        any = true;
    });
    if (any) {
        c[0] = v0;
        c[plane] = v1;
        c[2 * plane] = v2;
    }
}

template <int DT>
__global__ void k_final1x1_stitch(const typename Elem<DT>::vec *__restrict__ src, long np, int Hb, int Wb, int planes, int cin,
                                  const float *__restrict__ w, const float *__restrict__ bias, int crop,
                                  float *__restrict__ canvas, TileGeo g, int tile_begin, int tile_count, int y_first, int sigmoid,
                                  const float *__restrict__ noise_img) {
    final1x1_stitch_pixel<DT, false>(src, np, Hb, Wb, planes, cin, w, bias, crop, canvas, g, tile_begin, tile_count, y_first, sigmoid,
                                     noise_img, nullptr);
}

template <int DT>
__global__ void k_final1x1_stitch_ok(const typename Elem<DT>::vec *__restrict__ src, long np, int Hb, int Wb, int planes, int cin,
                                     const float *__restrict__ w, const float *__restrict__ bias, int crop,
                                     float *__restrict__ canvas, TileGeo g, int tile_begin, int tile_count, int y_first,
                                     const unsigned char *__restrict__ tile_ok) {
    final1x1_stitch_pixel<DT, true>(src, np, Hb, Wb, planes, cin, w, bias, crop, canvas, g, tile_begin, tile_count, y_first, 0, nullptr,
                                    tile_ok);
}

// Verdict of the checked frame loop: tile_ok[tile_begin + t] = 0 when any value k_final1x1_stitch would add for tile t of the launch
// is not finite.  It EVALUATES the 1x1 (the same dot3 over the same activations, bias included) on the 3 channels x the tile's
// useful rectangle as for_each_cover truncates it at the frame's edges, before the seam factor -- it does not test the stored
// activations' exponent bits, so a head whose own fp32 weights are not finite is seen too.  One thread per pixel of the rectangle;
// it reads what the stitch reads of the tile and nothing else.  Flags are preset to 1 by the caller and only ever cleared: every
// writer stores the same byte, so neither an atomic nor an order among them is needed
template <int DT>
__global__ __launch_bounds__(256) void k_tile_verdict(const typename Elem<DT>::vec *__restrict__ src, long np, int Hb, int Wb,
                                                      int planes, int cin, const float *__restrict__ w,
                                                      const float *__restrict__ bias, int crop, TileGeo g, int tile_begin,
                                                      int tile_count, unsigned char *__restrict__ tile_ok) {
    const int t = blockIdx.y;
    if (t >= tile_count) return;
    const int i = tile_begin + t;
    const int yi = i / g.cols, xi = i - yi * g.cols;
    const int ax = xi * g.stride, ay = yi * g.stride;
    const int x1pad = max(0, ax - g.pad + g.cs - g.W), y1pad = max(0, ay - g.pad + g.cs - g.H);
    const int uw = min(g.cs - max(g.pad, x1pad) - g.pad, g.W - ax), uh = min(g.cs - max(g.pad, y1pad) - g.pad, g.H - ay);
    if (uw <= 0 || uh <= 0) return;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= uw * uh) return;
    const int dy = p / uw, dx = p - dy * uw;
    float o0 = bias[0], o1 = bias[1], o2 = bias[2];
    dot3<DT>(src + ((size_t)t * Hb + g.pad + dy + crop) * Wb + g.pad + dx + crop, np, planes, w, cin, o0, o1, o2);
    // exponent all ones: inf or NaN (a bit test, so no floating-point mode can fold it away)
    const unsigned e = 0x7f800000u;
    if ((__float_as_uint(o0) & e) == e || (__float_as_uint(o1) & e) == e || (__float_as_uint(o2) & e) == e) tile_ok[i] = 0;
}

// geometry and source checks of the stitch launchers; the canvas rows [*yf, *yf + *yr) the launch's tiles reach
static int stitch_launch_geo(const QpBuf &src, int crop, int W, int H, int cs, int ucs, int ol, int tile_begin, int tile_count, TileGeo *g,
                             int *yf, int *yr) {
    ND_TRY(make_geo(W, H, cs, ucs, ol, g));
    if (src.pad != 0 || src.Hb != cs + 2 * crop || src.Wb != cs + 2 * crop || tile_count > src.B)
        ND_FAIL(ND_EINVAL, "final1x1_stitch: bad source geometry");
    stitch_band(*g, tile_begin, tile_count, yf, yr);
    return ND_OK;
}

int nd_launch_final1x1_stitch(const QpBuf &src, int cin, const float *w, const float *bias, int crop, float *canvas,
                              int W, int H, int cs, int ucs, int ol, int tile_begin, int tile_count, hipStream_t s, int sigmoid,
                              const float *noise_img) {
    TileGeo g;
    int yf, yr;
    ND_TRY(stitch_launch_geo(src, crop, W, H, cs, ucs, ol, tile_begin, tile_count, &g, &yf, &yr));
    if (yr <= 0) return ND_OK;
    dim3 grid((W + 255) / 256, yr);
    const int n = nd_cpp(src.dt);
    ND_DISPATCH_DT(src.dt, hipLaunchKernelGGL(k_final1x1_stitch<DT>, grid, dim3(256), 0, s, (const typename Elem<DT>::vec *)src.base,
                                              src.np(), src.Hb, src.Wb, (cin + n - 1) / n, cin, w, bias, crop, canvas, g,
                                              tile_begin, tile_count, yf, sigmoid, noise_img));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_launch_tile_verdict(const QpBuf &src, int cin, const float *w, const float *bias, int crop, int W, int H, int cs, int ucs, int ol,
                           int tile_begin, int tile_count, unsigned char *tile_ok, hipStream_t s) {
    TileGeo g;
    int yf, yr;
    ND_TRY(stitch_launch_geo(src, crop, W, H, cs, ucs, ol, tile_begin, tile_count, &g, &yf, &yr));
    if (!tile_ok || tile_begin < 0 || tile_count <= 0 || tile_count > 65535 || tile_begin + tile_count > g.cols * g.rows)
        ND_FAIL(ND_EINVAL, "tile_verdict: tiles [%d,+%d) outside the grid of %d (at most 65535 per launch), or no flags", tile_begin,
                tile_count, g.cols * g.rows);
    const int uwmax = g.cs - 2 * g.pad;
    if (uwmax <= 0) return ND_OK;
    dim3 grid((uwmax * uwmax + 255) / 256, tile_count);
    const int n = nd_cpp(src.dt);
    ND_DISPATCH_DT(src.dt, hipLaunchKernelGGL(k_tile_verdict<DT>, grid, dim3(256), 0, s, (const typename Elem<DT>::vec *)src.base,
                                              src.np(), src.Hb, src.Wb, (cin + n - 1) / n, cin, w, bias, crop, g, tile_begin, tile_count,
                                              tile_ok));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_launch_final1x1_stitch_ok(const QpBuf &src, int cin, const float *w, const float *bias, int crop, float *canvas, int W, int H,
                                 int cs, int ucs, int ol, int tile_begin, int tile_count, const unsigned char *tile_ok, hipStream_t s) {
    TileGeo g;
    int yf, yr;
    ND_TRY(stitch_launch_geo(src, crop, W, H, cs, ucs, ol, tile_begin, tile_count, &g, &yf, &yr));
    if (!tile_ok) ND_FAIL(ND_EINVAL, "final1x1_stitch_ok: no flags");
    if (yr <= 0) return ND_OK;
    dim3 grid((W + 255) / 256, yr);
    const int n = nd_cpp(src.dt);
    ND_DISPATCH_DT(src.dt, hipLaunchKernelGGL(k_final1x1_stitch_ok<DT>, grid, dim3(256), 0, s, (const typename Elem<DT>::vec *)src.base,
                                              src.np(), src.Hb, src.Wb, (cin + n - 1) / n, cin, w, bias, crop, canvas, g,
                                              tile_begin, tile_count, yf, tile_ok));
    ND_HIP(hipGetLastError());
    return ND_OK;
}

// ------------------------------------------------------------------ final sum of per-workgroup partials
__global__ __launch_bounds__(256) void k_sum(const float *__restrict__ partial, int n, float scale, float *__restrict__ out) {
    __shared__ float red[256];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    acc = nd_block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = acc * scale;
}
int nd_launch_sum(const float *partial, int n, float scale, float *out, hipStream_t s) {
    hipLaunchKernelGGL(k_sum, dim3(1), dim3(256), 0, s, partial, n, scale, out);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
