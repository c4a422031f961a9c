// Augmented training batches from a device-resident pool of pre-cropped images: DenoisingDataset.__getitem__
// (dataset_torch_3.py:231-276) for a whole batch in one launch.
//
// Pool: one byte buffer in HBM holding images as planar [3][H][W] samples in their file type (u8, u16 or f32), and a table of
// int64 {byte offset, H, W, nd_sample_type} per image.  Draws: int32 {clean image, noisy image, x0, y0, nrot, flip1, flip2, bits of
// the float u} per sample.  Output: clean and noisy [B,3,cs,cs] fp32, both from the same draw.
//
//   sample -> float   np_imgops.img_path_to_np_flt: u8 / 255, u16 / 65535 (correctly rounded fp32 divisions), f32 as it is
//   pad, then crop    np_imgops.np_pad_img_pair + np_crop_img_pair: a side d < cs is centred between zeros (pad0 = (cs - d) / 2
//                     before), a side d > cs is cut at the drawn offset.  Crop pixel (a, b) is source pixel (y0 + a - pad0_y,
//                     x0 + b - pad0_x); outside the image it is 0
//   orientation       np.rot90(nrot, (1, 2)), then np.flip(1) if flip1, then np.flip(2) if flip2: nd_crop_source_map below
//   exposure          m = min + (min(max, 1 / xmax) - min) * u with xmax = the maximum of the clean crop (k_crop_max, an order-free
//                     reduction); clean * m unclipped, clip(noisy * m, 0, 1)  (dataset_torch_3.py:271-274)
//
// One thread per output pixel writes its six floats: stores are coalesced along x; loads are along x or along y of the source
// depending on nrot, at most 6 MB per batch of 30 x 184^2 from a pool that the cache lines of neighbouring threads share.
// Every read is guarded: an image index outside the table, a table row that does not lie inside the pool, or a pixel outside the
// image reads as 0, whatever the draw holds.
//
// Window table (nd_crop_batch_windows, nd_pool_fetch_windows): int64 {byte offset of a parent image, H, W, nd_sample_type, y, x, PH,
// PW} per image.  The image is the H x W rectangle at (y, x) of the parent, planar [3][PH][PW], which the pool stores once: its
// rows are PW samples apart and its planes PH * PW.  Everything above holds with "the image" meaning the window; what the parent
// holds around it is never shown: a pixel outside the window reads as 0.  A window that does not lie inside its parent, or a parent
// that does not lie inside the pool, reads as zeros.  The kernels are one body for both tables: TABLE_COLS picks the row format.
#include <limits.h>
#include <math.h>

#include "nd_common.h"

// output pixel (y, x) of the cs x cs crop <- crop pixel (a, b); flips: bit 0 = flip1 (rows), bit 1 = flip2 (columns)
__host__ __device__ static inline void nd_crop_source_map(int cs, int nrot, int flips, int y, int x, int *a, int *b) {
    int p = y, q = x;
    if (flips & 2) q = cs - 1 - q;
    if (flips & 1) p = cs - 1 - p;
    for (int k = 0; k < (nrot & 3); ++k) {
        const int t = p;
        p = q;
        q = cs - 1 - t;
    }
    *a = p;
    *b = q;
}

namespace {
constexpr int DENSE = 4, WINDOWS = 8;   // int64 per table row

struct CropImage {
    const unsigned char *base;   // sample (0, 0) of plane 0 of the image; null: reads as zeros
    long long h, w;
    size_t pitch, plane;         // samples from a row to the next, and from a plane to the next
    int type;
};

// TABLE_COLS DENSE: {off, H, W, type}, the image is the whole of [3][H][W] at off.  WINDOWS: {off, H, W, type, y, x, PH, PW}, the
// image is rows [y, y + H) x columns [x, x + W) of the parent [3][PH][PW] at off
template <int TABLE_COLS>
__device__ inline CropImage crop_image(const unsigned char *pool, size_t pool_bytes, const long long *images, int n_images, int idx) {
    CropImage im = {nullptr, 0, 0, 0, 0, 0};
    if (idx < 0 || idx >= n_images) return im;
    const long long *row = images + TABLE_COLS * (size_t)idx;
    const long long off = row[0], h = row[1], w = row[2], type = row[3];
    if (off < 0 || h < 1 || w < 1 || h > INT_MAX || w > INT_MAX || type < ND_SAMPLE_U8 || type > ND_SAMPLE_F32) return im;
    long long y = 0, x = 0, ph = h, pw = w;
    if (TABLE_COLS == WINDOWS) {
        y = row[4], x = row[5], ph = row[6], pw = row[7];
        // every term is below 2^31 once the first six comparisons hold, so the two differences cannot wrap
        if (y < 0 || x < 0 || ph < 1 || pw < 1 || ph > INT_MAX || pw > INT_MAX || h > ph || w > pw || y > ph - h || x > pw - w) return im;
    }
    const unsigned long long bps = type == ND_SAMPLE_U8 ? 1 : (type == ND_SAMPLE_U16 ? 2 : 4);
    const unsigned long long bytes = 3ull * (unsigned long long)ph * (unsigned long long)pw * bps;   // < 2^66 / 2^2: ph, pw < 2^31
    if ((unsigned long long)off % bps || (unsigned long long)off > pool_bytes || bytes > pool_bytes - (unsigned long long)off) return im;
    im.base = pool + off + ((size_t)y * (size_t)pw + (size_t)x) * bps;
    im.h = h;
    im.w = w;
    im.pitch = (size_t)pw;
    im.plane = (size_t)ph * (size_t)pw;
    im.type = (int)type;
    return im;
}

// centred zero padding of a side d < cs (np_pad_img_pair)
__device__ inline long long crop_pad0(long long d, int cs) { return d < cs ? (cs - d) / 2 : 0; }

__device__ inline float crop_sample(const CropImage &im, int c, long long sy, long long sx) {
    if (!im.base || sy < 0 || sy >= im.h || sx < 0 || sx >= im.w) return 0.f;
    const size_t i = (size_t)c * im.plane + (size_t)sy * im.pitch + (size_t)sx;
    if (im.type == ND_SAMPLE_U8) return (float)im.base[i] / 255.f;
    if (im.type == ND_SAMPLE_U16) return (float)((const unsigned short *)im.base)[i] / 65535.f;
    return ((const float *)im.base)[i];
}

// maximum of rows [ya, ya + rows) x columns [xa, xa + cols) of the three planes of an image, as a float (integer samples convert
// exactly): one wave per row, lanes along x, so that loads are coalesced and the index needs no division per sample.  Rows are
// `pitch` samples apart and planes `plane`: those of the parent when the image is a window
template <typename T>
__device__ inline float crop_window_max(const T *p, size_t plane, size_t pitch, long long ya, long long xa, int rows, int cols, float m) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    for (int rr = wave; rr < 3 * rows; rr += waves) {
        const int c = rr / rows;
        const T *row = p + (size_t)c * plane + (size_t)(ya + (rr - c * rows)) * pitch + xa;
        for (int x = lane; x < cols; x += 64) m = fmaxf(m, (float)row[x]);
    }
    return m;
}

// grid (B): xmax[n] = max of the clean crop of sample n (zeros of the padding included), mult[n] = the exposure multiplier
template <int TABLE_COLS>
__global__ __launch_bounds__(1024) void k_crop_max(const unsigned char *__restrict__ pool, size_t pool_bytes,
                                                   const long long *__restrict__ images, int n_images, const int *__restrict__ draws,
                                                   int cs, float mmin, float mmax, float *__restrict__ xmax, float *__restrict__ mult) {
    __shared__ float red[1024];
    const int n = blockIdx.x;
    const int *d = draws + 8 * (size_t)n;
    const CropImage im = crop_image<TABLE_COLS>(pool, pool_bytes, images, n_images, d[0]);
    // rows [ya, yb) x columns [xa, xb) of the source lie inside the crop window; orientation does not change the maximum
    const long long py = crop_pad0(im.h, cs), px = crop_pad0(im.w, cs);
    const long long wy = (long long)d[3] - py, wx = (long long)d[2] - px;
    const long long ya = wy > 0 ? wy : 0, yb = wy + cs < im.h ? wy + cs : im.h;
    const long long xa = wx > 0 ? wx : 0, xb = wx + cs < im.w ? wx + cs : im.w;
    const int rows = yb > ya ? (int)(yb - ya) : 0, cols = xb > xa ? (int)(xb - xa) : 0;   // <= cs
    const bool padded = !im.base || rows < cs || cols < cs;
    float fm = padded || im.type != ND_SAMPLE_F32 ? 0.f : -INFINITY;
    if (im.base && rows && cols) {
        if (im.type == ND_SAMPLE_U8) fm = crop_window_max(im.base, im.plane, im.pitch, ya, xa, rows, cols, fm);
        else if (im.type == ND_SAMPLE_U16) fm = crop_window_max((const unsigned short *)im.base, im.plane, im.pitch, ya, xa, rows, cols, fm);
        else fm = crop_window_max((const float *)im.base, im.plane, im.pitch, ya, xa, rows, cols, fm);
    }
    red[threadIdx.x] = fm;
    __syncthreads();
    for (int k = 512; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // the integer maximum converts to the maximum of the converted samples: the conversion is monotonic
        float m = red[0];
        if (im.base && im.type == ND_SAMPLE_U8) m = m / 255.f;
        if (im.base && im.type == ND_SAMPLE_U16) m = m / 65535.f;
        const float u = __int_as_float(d[7]);
        const float b = m == 0.f ? mmax : fminf(mmax, 1.f / m);
        xmax[n] = m;
        mult[n] = mmin + (b - mmin) * u;
    }
}

// grid (ceil(cs * cs / 256), B)
template <int TABLE_COLS>
__global__ __launch_bounds__(256) void k_crop_batch(const unsigned char *__restrict__ pool, size_t pool_bytes,
                                                    const long long *__restrict__ images, int n_images, const int *__restrict__ draws,
                                                    int cs, const float *__restrict__ mult, float *__restrict__ clean,
                                                    float *__restrict__ noisy) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= cs * cs) return;
    const int y = pix / cs, x = pix - y * cs;
    const int *d = draws + 8 * (size_t)n;
    const CropImage ic = crop_image<TABLE_COLS>(pool, pool_bytes, images, n_images, d[0]);
    const CropImage in = crop_image<TABLE_COLS>(pool, pool_bytes, images, n_images, d[1]);
    int a, b;
    nd_crop_source_map(cs, d[4], (d[5] ? 1 : 0) | (d[6] ? 2 : 0), y, x, &a, &b);
    const size_t plane = (size_t)cs * cs, out = (size_t)n * 3 * plane + pix;
    // the pair is padded and cut as one: both windows from the clean image's sides, as np_pad_img_pair / np_crop_img_pair take
    // them from img1 (a noisy image of another size is read inside its own bounds)
    const long long sy = (long long)d[3] + a - crop_pad0(ic.h, cs), sx = (long long)d[2] + b - crop_pad0(ic.w, cs);
    const long long ny = ic.base ? sy : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float vc = crop_sample(ic, c, sy, sx), vn = crop_sample(in, c, ny, sx);
        if (mult) {
            const float m = mult[n];
            vc = vc * m;
            vn = fminf(fmaxf(vn * m, 0.f), 1.f);
        }
        clean[out + c * plane] = vc;
        noisy[out + c * plane] = vn;
    }
}
// grid (ceil(h * w / 256), n): image index[n] as fp32, whole: no crop, no padding, no orientation.  A row of another size than
// h x w is not this image: it reads as zeros, like an index outside the table or a row outside the pool
template <int TABLE_COLS>
__global__ __launch_bounds__(256) void k_pool_fetch(const unsigned char *__restrict__ pool, size_t pool_bytes,
                                                    const long long *__restrict__ images, int n_images, const int *__restrict__ index,
                                                    int h, int w, float *__restrict__ out) {
    const int n = blockIdx.y;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= h * w) return;
    const int y = pix / w, x = pix - y * w;
    CropImage im = crop_image<TABLE_COLS>(pool, pool_bytes, images, n_images, index[n]);
    if (im.h != h || im.w != w) im.base = nullptr;
    const size_t plane = (size_t)h * w, o = (size_t)n * 3 * plane + pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[o + c * plane] = crop_sample(im, c, y, x);
}
}  // namespace

extern "C" int nd_crop_source(int cs, int nrot, int flips, int y, int x, int *a, int *b) {
    if (!a || !b) ND_FAIL(ND_EINVAL, "nd_crop_source: null output pointer");
    if (cs < 1 || nrot < 0 || nrot > 3 || (flips & ~3) || y < 0 || y >= cs || x < 0 || x >= cs)
        ND_FAIL(ND_EINVAL, "nd_crop_source: cs %d, nrot %d, flips %d, pixel (%d, %d) out of range", cs, nrot, flips, y, x);
    nd_crop_source_map(cs, nrot, flips, y, x, a, b);
    return ND_OK;
}

// the host side of both table formats: `name` is the entry point's, for its refusals
template <int TABLE_COLS>
static int crop_batch_launch(const char *name, const void *pool, size_t pool_bytes, const int64_t *images, int n_images,
                             const int32_t *draws, int batch, int cs, float exp_mult_min, float exp_mult_max, const float *mult,
                             float *xmax, float *mult_out, float *clean_nchw, float *noisy_nchw, void *stream) {
    if (!pool || !pool_bytes || !images || !draws || !clean_nchw || !noisy_nchw) ND_FAIL(ND_EINVAL, "%s: null pointer", name);
    if (n_images < 1) ND_FAIL(ND_EINVAL, "%s: n_images %d < 1", name, n_images);
    if (cs < 1 || cs > 16384) ND_FAIL(ND_EINVAL, "%s: cs %d outside [1, 16384]", name, cs);
    if (batch < 1 || batch > 65535) ND_FAIL(ND_EINVAL, "%s: batch %d outside [1, 65535]", name, batch);
    if ((long long)batch * 8 > INT_MAX) ND_FAIL(ND_EINVAL, "%s: the draw table of batch %d does not fit int32", name, batch);
    const bool draw_mult = !mult && exp_mult_min != 1.f;   // dataset_torch_3.py:271
    if (draw_mult && (!xmax || !mult_out)) ND_FAIL(ND_EINVAL, "%s: exp_mult_min != 1 needs xmax and mult_out", name);
    if (draw_mult && !(exp_mult_min <= exp_mult_max))
        ND_FAIL(ND_EINVAL, "%s: exp_mult_min %g > exp_mult_max %g", name, (double)exp_mult_min, (double)exp_mult_max);
    hipStream_t s = (hipStream_t)stream;
    const unsigned char *p = (const unsigned char *)pool;
    const long long *im = (const long long *)images;
    if (draw_mult) {
        hipLaunchKernelGGL(k_crop_max<TABLE_COLS>, dim3(batch), dim3(1024), 0, s, p, pool_bytes, im, n_images, draws, cs, exp_mult_min,
                           exp_mult_max, xmax, mult_out);
        mult = mult_out;
    }
    hipLaunchKernelGGL(k_crop_batch<TABLE_COLS>, dim3((cs * cs + 255) / 256, batch), dim3(256), 0, s, p, pool_bytes, im, n_images, draws,
                       cs, mult, clean_nchw, noisy_nchw);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

template <int TABLE_COLS>
static int pool_fetch_launch(const char *name, const void *pool, size_t pool_bytes, const int64_t *images, int n_images,
                             const int32_t *index, int n, int h, int w, float *out_nchw, void *stream) {
    if (!pool || !pool_bytes || !images || !index || !out_nchw) ND_FAIL(ND_EINVAL, "%s: null pointer", name);
    if (n_images < 1) ND_FAIL(ND_EINVAL, "%s: n_images %d < 1", name, n_images);
    if (h < 1 || h > 16384 || w < 1 || w > 16384) ND_FAIL(ND_EINVAL, "%s: %d x %d, a side outside [1, 16384]", name, h, w);
    if (n < 1 || n > 65535) ND_FAIL(ND_EINVAL, "%s: n %d outside [1, 65535]", name, n);
    hipLaunchKernelGGL(k_pool_fetch<TABLE_COLS>, dim3((h * w + 255) / 256, n), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char *)pool, pool_bytes, (const long long *)images, n_images, index, h, w, out_nchw);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_crop_batch(const void *pool, size_t pool_bytes, const int64_t *images, int n_images, const int32_t *draws, int batch,
                             int cs, float exp_mult_min, float exp_mult_max, const float *mult, float *xmax, float *mult_out,
                             float *clean_nchw, float *noisy_nchw, void *stream) {
    return crop_batch_launch<DENSE>("nd_crop_batch", pool, pool_bytes, images, n_images, draws, batch, cs, exp_mult_min, exp_mult_max,
                                    mult, xmax, mult_out, clean_nchw, noisy_nchw, stream);
}

extern "C" int nd_crop_batch_windows(const void *pool, size_t pool_bytes, const int64_t *windows, int n_windows, const int32_t *draws,
                                     int batch, int cs, float exp_mult_min, float exp_mult_max, const float *mult, float *xmax,
                                     float *mult_out, float *clean_nchw, float *noisy_nchw, void *stream) {
    return crop_batch_launch<WINDOWS>("nd_crop_batch_windows", pool, pool_bytes, windows, n_windows, draws, batch, cs, exp_mult_min,
                                      exp_mult_max, mult, xmax, mult_out, clean_nchw, noisy_nchw, stream);
}

extern "C" int nd_pool_fetch(const void *pool, size_t pool_bytes, const int64_t *images, int n_images, const int32_t *index, int n, int h,
                             int w, float *out_nchw, void *stream) {
    return pool_fetch_launch<DENSE>("nd_pool_fetch", pool, pool_bytes, images, n_images, index, n, h, w, out_nchw, stream);
}

extern "C" int nd_pool_fetch_windows(const void *pool, size_t pool_bytes, const int64_t *windows, int n_windows, const int32_t *index,
                                     int n, int h, int w, float *out_nchw, void *stream) {
    return pool_fetch_launch<WINDOWS>("nd_pool_fetch_windows", pool, pool_bytes, windows, n_windows, index, n, h, w, out_nchw, stream);
}
