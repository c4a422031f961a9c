// Device-side weight packing: the host packers of pack.hip / conv_w1d.hip / winograd.hip as kernels, for weights that
// live in HBM -- the training step re-packs every step (the weights change every step), and a model load packs here instead of
// on host threads (the Winograd transforms of UtNet(64) take ~1 s there).  Same layouts, same maps.  The direct form packs every
// storage type, bit for bit what the host packer writes; the Winograd forms are fp32 only and their transforms are
// evaluated in fp32 here by default (the host packers use double): the packed values agree to ~1e-7 relative.  With host_bits
// (the UNet blob) they are evaluated in double, operation by operation as on the host: the same bytes.
#include "nd_common.h"

namespace {

// the host's roundings (pack.hip: f32_to_bf16_rne / f32_to_f16_rne), bit for bit
__device__ __forceinline__ unsigned f32_to_bf16_rne(float f) {
    const unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return ((u >> 16) | 0x40) & 0xffffu;   // NaN stays NaN
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ unsigned f32_to_f16_rne(float f) {
    union {
        _Float16 h;
        unsigned short u;
    } c;
    c.h = (_Float16)f;   // v_cvt_f16_f32: nearest even, subnormals kept, overflow to +-inf
    return c.u;
}

// direct form (pack.hip: nd_pack_layer): nw 4-byte units of packed weights followed by nb biases.  fp32: one thread per value;
// 16-bit: one thread per 16-byte lane element (its 8 channels, one vector store).  scale (nullable): one factor per output channel,
// applied to every weight of that channel as it is written (the folded BatchNorm of UNet; `bias` is then the folded bias)
template <int DT>
__global__ void k_pack_dev(int kind, int cin, int cout, int M, int KB, int taps, const float *__restrict__ w,
                           const float *__restrict__ bias, float *__restrict__ packed, long nw, int nb, const float *__restrict__ scale) {
    constexpr int CPL = DT == ND_F32 ? 4 : 8;   // channels per lane of a piece
    constexpr int PER = DT == ND_F32 ? 1 : 8;   // ... and per thread
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nu = DT == ND_F32 ? nw : nw / 4;   // threads that pack weights
    if (idx < nu) {
        const int s0 = DT == ND_F32 ? (int)(idx & 3) : 0, lane = (int)((DT == ND_F32 ? idx >> 2 : idx) & 63);
        long rest = DT == ND_F32 ? idx >> 8 : idx >> 6;
        const int t = (int)(rest % taps);
        rest /= taps;
        const int kb = (int)(rest % KB), mt = (int)(rest / KB);
        const int m = 32 * mt + (lane & 31), ci0 = 2 * CPL * kb + CPL * (lane >> 5) + s0;
        float v[PER];
#pragma unroll
        for (int s = 0; s < PER; ++s) {
            const int ci = ci0 + s;
            v[s] = 0.f;
            if (m < M && ci < cin) {
                switch (kind) {
                    case ND_CONV3: v[s] = w[((long)m * cin + ci) * 9 + t]; break;
                    case ND_CONVT3: v[s] = w[((long)ci * cout + m) * 9 + (8 - t)]; break;
                    case ND_CONVT2S2: {
                        const NdUpRow r = nd_up_row(m, cout, DT);
                        v[s] = w[((long)ci * cout + r.co) * 4 + 2 * r.a + r.b];
                        break;
                    }
                    case ND_CONV2S2: v[s] = w[((long)m * cin + ci) * 4 + t]; break;
                    default: v[s] = w[(long)m * cin + ci]; break;
                }
                if (scale) v[s] = v[s] * scale[kind == ND_CONVT2S2 ? nd_up_row(m, cout, DT).co : m];   // one rounding, as the host's w * sc
            }
        }
        if constexpr (DT == ND_F32) {
            packed[idx] = v[0];
        } else {
            unsigned h[PER];
#pragma unroll
            for (int s = 0; s < PER; ++s) h[s] = DT == ND_BF16 ? f32_to_bf16_rne(v[s]) : f32_to_f16_rne(v[s]);
            reinterpret_cast<uint4 *>(packed)[idx] = make_uint4(h[0] | h[1] << 16, h[2] | h[3] << 16, h[4] | h[5] << 16, h[6] | h[7] << 16);
        }
    } else if (idx < nu + nb) {
        const int m = (int)(idx - nu);
        packed[nw + m] = (m < M && bias) ? bias[kind == ND_CONVT2S2 ? nd_up_row(m, cout, DT).co : m] : 0.f;
    }
}

// eval-mode BatchNorm2d folded into the conv before it (unet.hip: nd_unet_pack_weights): scale = g / sqrt(rv + eps),
// folded bias = (b - rm) * scale + be.  Every operation rounds once, in the host packer's order: no contraction into an FMA
__global__ void k_bn_fold(int cout, const float *__restrict__ b, const float *__restrict__ g, const float *__restrict__ be,
                          const float *__restrict__ rm, const float *__restrict__ rv, float *__restrict__ scale, float *__restrict__ fbias) {
#pragma clang fp contract(off)
    const int co = blockIdx.x * blockDim.x + threadIdx.x;
    if (co >= cout) return;
    const float sc = g[co] / sqrtf(rv[co] + 1e-5f);   // (correctly rounded division and square root: hipcc's default)
    scale[co] = sc;
    const float d = (b[co] - rm[co]) * sc;
    fbias[co] = d + be[co];
}

// one row of G g for F(T,3): u[0 .. T+2).  R = float: the fp32 evaluation; R = double: the host packers' (Wino<T>::g / W1<T>::g,
// the same operations in the same order -- no product feeds a sum, so nothing contracts into an FMA)
template <typename R>
__device__ __forceinline__ void wino_g(int T, const R *g, R *u) {
    if (T == 2) {
        u[0] = g[0];
        u[1] = R(0.5) * (g[0] + g[1] + g[2]);
        u[2] = R(0.5) * (g[0] - g[1] + g[2]);
        u[3] = g[2];
    } else if (T == 6) {
        u[0] = g[0];
        u[1] = R(-2) / R(9) * (g[0] + g[1] + g[2]);
        u[2] = R(-2) / R(9) * (g[0] - g[1] + g[2]);
        u[3] = g[0] / R(90) + g[1] / R(45) + g[2] * R(2) / R(45);
        u[4] = g[0] / R(90) - g[1] / R(45) + g[2] * R(2) / R(45);
        u[5] = g[0] * R(32) / R(45) + g[1] * R(16) / R(45) + g[2] * R(8) / R(45);
        u[6] = g[0] * R(32) / R(45) - g[1] * R(16) / R(45) + g[2] * R(8) / R(45);
        u[7] = g[2];
    } else {
        u[0] = g[0] / R(4);
        u[1] = -(g[0] + g[1] + g[2]) / R(6);
        u[2] = -(g[0] - g[1] + g[2]) / R(6);
        u[3] = g[0] / R(24) + g[1] / R(12) + g[2] / R(6);
        u[4] = g[0] / R(24) - g[1] / R(12) + g[2] / R(6);
        u[5] = g[2];
    }
}
// tap (ky, kx) of the layer as a valid correlation, times its output channel's factor where there is one (one rounding, in fp32)
__device__ __forceinline__ float tap3(int kind, const float *w, int cin, int cout, int co, int ci, int ky, int kx, const float *scale) {
    const float v = kind == ND_CONV3 ? w[((long)co * cin + ci) * 9 + ky * 3 + kx] : w[((long)ci * cout + co) * 9 + (8 - (ky * 3 + kx))];
    return scale ? v * scale[co] : v;
}

// fused 1-D Winograd form (conv_w1d.hip: nd_w1d_pack): [mt][kb][ky*(T+2) + xi][lane][4] + bias
template <typename R>
__global__ void k_pack_w1d_dev(int T, int kind, int cin, int cout, int KB, const float *__restrict__ w, const float *__restrict__ bias,
                               float *__restrict__ packed, long nw, int nb, const float *__restrict__ scale) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int NP = T + 2;
    if (idx < nw) {
        const int s = (int)(idx & 3), lane = (int)((idx >> 2) & 63);
        long rest = idx >> 8;
        const int plane = (int)(rest % (3 * NP));
        rest /= 3 * NP;
        const int kb = (int)(rest % KB), mt = (int)(rest / KB);
        const int ky = plane / NP, xi = plane - NP * ky;
        const int m = 32 * mt + (lane & 31), ci = 8 * kb + 4 * (lane >> 5) + s;
        float v = 0.f;
        // (the host packer transforms the zero taps of the padding rows and channels too: positions 1 and 2 of F(4,3) hold -0.0 there)
        const bool real = m < cout && ci < cin;
        if (real || sizeof(R) == sizeof(double)) {
            R g[3], u[6];
#pragma unroll
            for (int k = 0; k < 3; ++k) g[k] = real ? R(tap3(kind, w, cin, cout, m, ci, ky, k, scale)) : R(0);
            wino_g<R>(T, g, u);
            v = (float)u[xi];
        }
        packed[idx] = v;
    } else if (idx < nw + nb) {
        const int m = (int)(idx - nw);
        packed[idx] = (m < cout && bias) ? bias[m] : 0.f;
    }
}

// three-pass Winograd form (winograd.hip: nd_wino_pack): P = (T+2)^2 1-tap GEMM blobs [mt][kb][lane][4] + zero bias each,
// then bias[cout rounded up to 4].  gf = floats per position blob, nwp = packed weights per position
template <typename R>
__global__ void k_pack_wino_dev(int T, int kind, int cin, int cout, int KB, const float *__restrict__ w, const float *__restrict__ bias,
                                float *__restrict__ packed, long gf, long nwp, int P, const float *__restrict__ scale) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int A = T + 2;
    if (idx < (long)P * gf) {
        const int pos = (int)(idx / gf);
        const long r = idx - (long)pos * gf;
        float v = 0.f;
        if (r < nwp) {
            const int s = (int)(r & 3), lane = (int)((r >> 2) & 63);
            const long rest = r >> 8;
            const int kb = (int)(rest % KB), mt = (int)(rest / KB);
            const int m = 32 * mt + (lane & 31), ci = 8 * kb + 4 * (lane >> 5) + s;
            if (m < cout && ci < cin) {
                const int i = pos / A, j = pos - A * i;
                R col[3];   // (G g)[i][kx] for kx = 0..2
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    R g[3], u[8];
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) g[ky] = tap3(kind, w, cin, cout, m, ci, ky, kx, scale);
                    wino_g<R>(T, g, u);
                    col[kx] = u[i];
                }
                R u[8];
                wino_g<R>(T, col, u);
                v = (float)u[j];
            }
        }
        packed[idx] = v;   // (the tail of a position blob is its zero bias)
    } else {
        const long m = idx - (long)P * gf;
        if (m < (cout + 3) / 4 * 4) packed[idx] = (bias && m < cout) ? bias[m] : 0.f;
    }
}

}  // namespace

int nd_launch_bn_fold(int cout, const float *b, const float *g, const float *be, const float *rm, const float *rv, float *scale,
                      float *fbias, hipStream_t s) {
    if (cout <= 0 || !b || !g || !be || !rm || !rv || !scale || !fbias) ND_FAIL(ND_EINVAL, "bn_fold: null tensor");
    hipLaunchKernelGGL(k_bn_fold, dim3((cout + 255) / 256), dim3(256), 0, s, cout, b, g, be, rm, rv, scale, fbias);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_pack_layer_device(int kind, int cin, int cout, int dt, const float *w, const float *bias, float *packed, hipStream_t s,
                         const float *scale) {
    const int MT = nd_mtiles(kind, cout), KB = nd_kblocks(cin, dt), taps = nd_taps(kind);
    const int M = kind == ND_CONVT2S2 ? 4 * cout : cout;
    const long nw = (long)nd_bias_offset(kind, cin, cout, dt);
    const long threads = (dt == ND_F32 ? nw : nw / 4) + MT * 32;
    if (dt != ND_F32 && ((uintptr_t)packed & 15)) ND_FAIL(ND_EINVAL, "device packing: a 16-bit layer must be 16-byte aligned");
    if (kind == ND_CONVT2S2 && cout % nd_cpp(dt)) ND_FAIL(ND_EINVAL, "device packing: 2x2 stride-2 transpose with cout=%d (multiple of %d)", cout, nd_cpp(dt));
    const auto k = dt == ND_F32 ? k_pack_dev<ND_F32> : dt == ND_BF16 ? k_pack_dev<ND_BF16> : k_pack_dev<ND_F16>;
    hipLaunchKernelGGL(k, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, kind, cin, cout, M, KB, taps, w, bias, packed, nw,
                       MT * 32, scale);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_pack_w1d_device(int T, int kind, int cin, int cout, const float *w, const float *bias, float *packed, hipStream_t s,
                       const float *scale, bool host_bits) {
    if ((T != 2 && T != 4) || (kind != ND_CONV3 && kind != ND_CONVT3)) ND_FAIL(ND_EINVAL, "device w1d packing: T = 2 | 4, 3x3 layers");
    const int MT = nd_mtiles(ND_CONV3, cout), KB = nd_kblocks(cin);
    const long nw = (long)nd_bias_offset(kind, cin, cout, ND_F32, T);
    hipLaunchKernelGGL(host_bits ? k_pack_w1d_dev<double> : k_pack_w1d_dev<float>, dim3((unsigned)((nw + MT * 32 + 255) / 256)), dim3(256), 0, s, T,
                       kind, cin, cout, KB, w, bias, packed, nw, MT * 32, scale);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

int nd_pack_wino_device(int T, int kind, int cin, int cout, const float *w, const float *bias, float *packed, hipStream_t s,
                        const float *scale, bool host_bits) {
    if ((T != 2 && T != 4 && T != 6) || (kind != ND_CONV3 && kind != ND_CONVT3)) ND_FAIL(ND_EINVAL, "device Winograd packing: T = 2 | 4 | 6, 3x3 layers");
    const int P = (T + 2) * (T + 2), KB = nd_kblocks(cin);
    const long gf = (long)nd_packed_floats(ND_CONV1, cin, cout, ND_F32);
    const long nwp = (long)nd_bias_offset(ND_CONV1, cin, cout);
    const long total = (long)P * gf + (cout + 3) / 4 * 4;
    hipLaunchKernelGGL(host_bits ? k_pack_wino_dev<double> : k_pack_wino_dev<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, T, kind,
                       cin, cout, KB, w, bias, packed, gf, nwp, P, scale);
    ND_HIP(hipGetLastError());
    return ND_OK;
}
