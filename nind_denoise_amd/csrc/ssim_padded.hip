// The SSIM the reference vendors in its own tree (libs/pytorch_ssim/__init__.py:20-35, driven by loss.py:29-45 gen_score):
//   Gaussian window (sigma 1.5, `window` taps, normalised), per channel, ZERO-PADDED by window / 2: the maps are H x W and border
//   pixels see zeros;  C1 = 0.01^2, C2 = 0.03^2
//   mu = G * x,  s_xx = G * x^2 - mu_x^2 (s_yy, s_xy alike)
//   map = (2 mu_x mu_y + C1)(2 s_xy + C2) / ((mu_x^2 + mu_y^2 + C1)(s_xx + s_yy + C2)),   out[n] = mean_{c,h,w} map
// It is not the piqa score of ssim.hip (VALID window, (H-10) x (W-10) map).
//
// HBM-bound like k_ssim_tile, and shaped like it: one workgroup computes a 32 x 32 patch of the map from a (32 + window - 1)^2
// patch of x and y staged in LDS -- a load outside the image is the zero padding --, filters rows of the five moment maps
// into LDS, then columns per output pixel, and reduces the patch to one partial.  Partials are added per sample in a fixed
// order, in double (deterministic, no atomics).  The window is applied separably with the reference's float32 1-D taps, which the host
// computes and passes by value.
//
// Gradient (y constant): with A = d map / d mu_x, B = d map / d E[xx], C = d map / d E[xy] at every map position,
//   gx(u) = gout[n] / (c h w) * [ (G * A)(u) + 2 x(u) (G * B)(u) + y(u) (G * C)(u) ]
// (the same symmetric window, A = B = C = 0 outside the image).  One workgroup: 16 x 16 gradient pixels <- the derivative maps at
// (16 + window - 1)^2 positions <- a (16 + 2 (window - 1))^2 patch of x and y: the five moment maps are recomputed in LDS on
// a double halo and never travel through HBM (20 B per pixel: x, y read once for the score, once here, gx written).
#include <math.h>

#include "nd_common.h"

namespace {
constexpr int kMaxWin = 11;
constexpr int kTile = 32;   // forward: map pixels per workgroup side
constexpr int kBT = 16;     // gradient: pixels per workgroup side
struct Taps { float g[kMaxWin]; };

// grid (tiles_x, tiles_y, planes); x, y: [planes][H][W]; partial: [planes][tiles_y][tiles_x]
template <int WIN>
__global__ __launch_bounds__(256) void k_ssimp_tile(const float *__restrict__ x, const float *__restrict__ y, int H, int W, Taps taps,
                                                    float *__restrict__ partial) {
    constexpr int HALF = WIN / 2, IN = kTile + WIN - 1;
    __shared__ float sx[IN][IN + 1], sy[IN][IN + 1];
    __shared__ float hm[5][IN][kTile + 1];
    __shared__ float red[256];
    const int plane = blockIdx.z;
    const int ox0 = blockIdx.x * kTile, oy0 = blockIdx.y * kTile;
    const float *xp = x + (size_t)plane * H * W, *yp = y + (size_t)plane * H * W;
    for (int i = threadIdx.x; i < IN * IN; i += 256) {
        const int r = i / IN, c = i - r * IN;
        const int gy = oy0 - HALF + r, gx = ox0 - HALF + c;
        const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
        sx[r][c] = in ? xp[(size_t)gy * W + gx] : 0.f;
        sy[r][c] = in ? yp[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < IN * kTile; i += 256) {
        const int r = i / kTile, c = i - r * kTile;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = taps.g[k], u = sx[r][c + k], v = sy[r][c + k];
            a += g * u;
            b += g * v;
            aa += g * (u * u);
            bb += g * (v * v);
            ab += g * (u * v);
        }
        hm[0][r][c] = a;
        hm[1][r][c] = b;
        hm[2][r][c] = aa;
        hm[3][r][c] = bb;
        hm[4][r][c] = ab;
    }
    __syncthreads();
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    float sum = 0.f;
    for (int i = threadIdx.x; i < kTile * kTile; i += 256) {
        const int r = i / kTile, c = i - r * kTile;
        if (oy0 + r >= H || ox0 + c >= W) continue;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = taps.g[k];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] += g * hm[q][r + k][c];
        }
        const float mxx = m[0] * m[0], myy = m[1] * m[1], mxy = m[0] * m[1];
        const float sxx = m[2] - mxx, syy = m[3] - myy, sxy = m[4] - mxy;
        sum += ((2.f * mxy + c1) * (2.f * sxy + c2)) / ((mxx + myy + c1) * (sxx + syy + c2));
    }
    sum = nd_block_sum(sum, red);
    if (threadIdx.x == 0) partial[((size_t)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = sum;
}

// out[sample] = sum of the sample's `count` partials (its c planes are contiguous) * inv_pixels: one workgroup per sample
__global__ __launch_bounds__(256) void k_ssimp_reduce(const float *__restrict__ partial, size_t count, double inv_pixels,
                                                      float *__restrict__ out) {
    __shared__ double red[256];
    const float *p = partial + (size_t)blockIdx.x * count;
    double a = 0.;
    for (size_t i = threadIdx.x; i < count; i += 256) a += (double)p[i];
    a = nd_block_sum(a, red);
    if (threadIdx.x == 0) out[blockIdx.x] = (float)(a * inv_pixels);
}

// grid (tiles_x, tiles_y, planes) of 16 x 16 gradient pixels; gx[plane] = gout[plane / C] * inv_pixels * d(sum of the plane's map)/dx
template <int WIN>
__global__ __launch_bounds__(256) void k_ssimp_grad_tile(const float *__restrict__ x, const float *__restrict__ y, int C, int H, int W,
                                                         Taps taps, const float *__restrict__ gout, float inv_pixels,
                                                         float *__restrict__ gx) {
    constexpr int HALF = WIN / 2, BQ = kBT + WIN - 1, BI = BQ + WIN - 1;
    __shared__ float sx[BI][BI + 1], sy[BI][BI + 1];
    __shared__ float hm[5][BI][BQ + 1];
    __shared__ float dm[3][BQ][BQ + 1];
    float (*rm)[BQ][kBT + 1] = reinterpret_cast<float (*)[BQ][kBT + 1]>(&hm[0][0][0]);   // hm is dead once dm is written
    static_assert(3 * BQ * (kBT + 1) <= 5 * BI * (BQ + 1), "rm must fit in hm");
    const int plane = blockIdx.z;
    const int ux0 = blockIdx.x * kBT, uy0 = blockIdx.y * kBT;   // first gradient pixel of the tile
    const int qx0 = ux0 - HALF, qy0 = uy0 - HALF;               // first map position it depends on
    const int ix0 = qx0 - HALF, iy0 = qy0 - HALF;               // first input pixel those positions read
    const float *xp = x + (size_t)plane * H * W, *yp = y + (size_t)plane * H * W;
    for (int i = threadIdx.x; i < BI * BI; i += 256) {
        const int r = i / BI, c = i - r * BI;
        const int gy_ = iy0 + r, gx_ = ix0 + c;
        const bool in = gy_ >= 0 && gy_ < H && gx_ >= 0 && gx_ < W;
        sx[r][c] = in ? xp[(size_t)gy_ * W + gx_] : 0.f;
        sy[r][c] = in ? yp[(size_t)gy_ * W + gx_] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BI * BQ; i += 256) {
        const int r = i / BQ, c = i - r * BQ;
        float a = 0.f, b = 0.f, aa = 0.f, bb = 0.f, ab = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = taps.g[k], u = sx[r][c + k], v = sy[r][c + k];
            a += g * u;
            b += g * v;
            aa += g * (u * u);
            bb += g * (v * v);
            ab += g * (u * v);
        }
        hm[0][r][c] = a;
        hm[1][r][c] = b;
        hm[2][r][c] = aa;
        hm[3][r][c] = bb;
        hm[4][r][c] = ab;
    }
    __syncthreads();
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    for (int i = threadIdx.x; i < BQ * BQ; i += 256) {
        const int r = i / BQ, c = i - r * BQ;
        const int qy = qy0 + r, qx = qx0 + c;
        float A = 0.f, B = 0.f, Cd = 0.f;
        if (qy >= 0 && qy < H && qx >= 0 && qx < W) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float g = taps.g[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] += g * hm[q][r + k][c];
            }
            // map = l * cs,  l = (2 mx my + c1) / b1,  cs = (2 s_xy + c2) / b2
            const float mx = m[0], my = m[1];
            const float a2 = 2.f * (m[4] - mx * my) + c2, b2 = (m[2] - mx * mx) + (m[3] - my * my) + c2;
            const float cs = a2 / b2;
            const float dcs_mx = 2.f / b2 * (mx * cs - my), dcs_xx = -cs / b2, dcs_xy = 2.f / b2;
            const float b1 = mx * mx + my * my + c1, l = (2.f * mx * my + c1) / b1;
            A = 2.f / b1 * (my - mx * l) * cs + l * dcs_mx;
            B = l * dcs_xx;
            Cd = l * dcs_xy;
        }
        dm[0][r][c] = A;
        dm[1][r][c] = B;
        dm[2][r][c] = Cd;
    }
    __syncthreads();   // every read of hm is done: rm may overwrite it
    // rows: rm(q_row, u_col) = sum_k g[k] d(q_row, u_col - HALF + k);  local column of map position u - HALF + k is u_local + k
    for (int i = threadIdx.x; i < BQ * kBT; i += 256) {
        const int r = i / kBT, c = i - r * kBT;
        float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
            const float g = taps.g[k];
            a += g * dm[0][r][c + k];
            b += g * dm[1][r][c + k];
            d += g * dm[2][r][c + k];
        }
        rm[0][r][c] = a;
        rm[1][r][c] = b;
        rm[2][r][c] = d;
    }
    __syncthreads();
    {
        const int r = threadIdx.x / kBT, c = threadIdx.x - r * kBT;
        const int uy = uy0 + r, ux = ux0 + c;
        if (uy < H && ux < W) {
            float a = 0.f, b = 0.f, d = 0.f;
#pragma unroll
            for (int k = 0; k < WIN; ++k) {
                const float g = taps.g[k];
                a += g * rm[0][r + k][c];
                b += g * rm[1][r + k][c];
                d += g * rm[2][r + k][c];
            }
            const float xv = sx[r + 2 * HALF][c + 2 * HALF], yv = sy[r + 2 * HALF][c + 2 * HALF];
            gx[((size_t)plane * H + uy) * W + ux] = gout[plane / C] * inv_pixels * (a + 2.f * xv * b + yv * d);
        }
    }
}

// float32 values of the reference's gaussian(): exp of the float32-rounded exponents, their float32 sum (torch adds the few terms
// in an order that lands on the correctly rounded sum for every window here: a double sum, rounded once), one division each
Taps make_taps(int window) {
    Taps t = {};
    double sum = 0.;
    for (int k = 0; k < window; ++k) {
        const int d = k - window / 2;
        t.g[k] = expf((float)(-(double)(d * d) / (2.0 * 1.5 * 1.5)));
        sum += (double)t.g[k];
    }
    const float s = (float)sum;
    for (int k = 0; k < window; ++k) t.g[k] /= s;
    return t;
}

size_t partial_count(int n, int c, int h, int w) {
    return (size_t)n * c * ((h + kTile - 1) / kTile) * ((w + kTile - 1) / kTile);
}
size_t workspace_bytes(int n, int c, int h, int w) { return (partial_count(n, c, h, w) * 4 + 255) & ~(size_t)255; }

int check_args(const char *who, int n, int c, int h, int w, int window, const void *ws, size_t ws_bytes) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0) ND_FAIL(ND_EINVAL, "%s: bad shape [%d,%d,%d,%d]", who, n, c, h, w);
    if (window < 3 || window > kMaxWin || !(window & 1))
        ND_FAIL(ND_EINVAL, "%s: window %d is not odd and within 3...%d (an even window makes the reference's map one row and column larger)",
                who, window, kMaxWin);
    if ((long)n * c > 65535) ND_FAIL(ND_EINVAL, "%s: more than 65535 image planes", who);
    if (h > 65535 * kBT || w > 65535 * kBT) ND_FAIL(ND_EINVAL, "%s: %dx%d image is too large", who, h, w);
    const size_t need = workspace_bytes(n, c, h, w);
    if (!ws || ws_bytes < need) ND_FAIL(ND_ENOMEM, "%s: workspace %zu B given, %zu B needed", who, ws_bytes, need);
    return ND_OK;
}
}  // namespace

extern "C" size_t nd_ssim_padded_workspace_bytes(int n, int c, int h, int w, int window) {
    if (n <= 0 || c <= 0 || h <= 0 || w <= 0 || window < 3 || window > kMaxWin || !(window & 1)) return 0;
    return workspace_bytes(n, c, h, w);
}

extern "C" int nd_ssim_padded(const float *x, const float *y, int n, int c, int h, int w, int window, float *out, void *ws,
                              size_t ws_bytes, void *stream) {
    ND_TRY(check_args("nd_ssim_padded", n, c, h, w, window, ws, ws_bytes));
    hipStream_t s = (hipStream_t)stream;
    const Taps taps = make_taps(window);
    const dim3 g((w + kTile - 1) / kTile, (h + kTile - 1) / kTile, n * c);
    float *partial = (float *)ws;
    switch (window) {
#define ND_CASE(WIN) \
    case WIN: hipLaunchKernelGGL(k_ssimp_tile<WIN>, g, dim3(256), 0, s, x, y, h, w, taps, partial); break;
        ND_CASE(3) ND_CASE(5) ND_CASE(7) ND_CASE(9) ND_CASE(11)
#undef ND_CASE
    }
    hipLaunchKernelGGL(k_ssimp_reduce, dim3(n), dim3(256), 0, s, (const float *)partial, (size_t)c * g.x * g.y,
                       1.0 / ((double)c * h * w), out);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_ssim_padded_grad(const float *x, const float *y, int n, int c, int h, int w, int window, const float *gout,
                                   float *gx, void *ws, size_t ws_bytes, void *stream) {
    ND_TRY(check_args("nd_ssim_padded_grad", n, c, h, w, window, ws, ws_bytes));
    hipStream_t s = (hipStream_t)stream;
    const Taps taps = make_taps(window);
    const dim3 g((w + kBT - 1) / kBT, (h + kBT - 1) / kBT, n * c);
    const float inv_pixels = (float)(1.0 / ((double)c * h * w));
    switch (window) {
#define ND_CASE(WIN) \
    case WIN: hipLaunchKernelGGL(k_ssimp_grad_tile<WIN>, g, dim3(256), 0, s, x, y, c, h, w, taps, gout, inv_pixels, gx); break;
        ND_CASE(3) ND_CASE(5) ND_CASE(7) ND_CASE(9) ND_CASE(11)
#undef ND_CASE
    }
    ND_HIP(hipGetLastError());
    return ND_OK;
}
