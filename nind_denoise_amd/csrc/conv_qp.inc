// conv_qp.inc -- the implicit-GEMM convolution kernel; included by one translation unit per storage type
// (conv_f32.hip / conv_bf16.hip / conv_f16.hip) so that the three instantiation groups compile in parallel.
#pragma once
// Implicit-GEMM convolution on the fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32), quad-planar layout.
//
// One kernel serves every weighted 3x3 / 1x1-shaped layer of UtNet (reference: networks/UtNet.py:27-88):
//   Conv2d(3, valid)            -> 9 taps on the input buffer
//   ConvTranspose2d(3, s=1)     -> the same 9-tap valid correlation on a buffer that carries a 2-pixel ZERO border,
//                                  with weights flipped / channel-transposed at pack time (pack.hip)
//   ConvTranspose2d(2, s=2)     -> 1 tap, M = 4*Cout rows ordered (a,b,co); pixel-shuffle in the store
//   Conv2d(1)                   -> 1 tap
//
// GEMM view (per launch):  D[m][p] = sum_{tap,ci} Wp[m][tap,ci] * X[ci][p + off(tap)]
//   M = output channels (MFMA "A" operand = packed weights), N = linear pixels p of the bordered input buffer
//   (MFMA "B" operand), K = taps * Cin.  An N tile enumerates VALID output pixels only (compact index
//   r = y*Wv + x inside an image); the input pixels they read still form ONE contiguous range of the linear input index,
//   so the LDS halo image stays one contiguous copy per plane and only the per-lane fragment offset (computed once per
//   tile) knows about the row / image gaps.
//
// MFMA fragment use (f32 32x32x2: lane l supplies A[i=l&31][k=l>>5], B[k=l>>5][j=l&31]):
//   one ds_read_b128 per operand fetches 4 consecutive channels c..c+3 of channel-quad (2*kb + h), h = lane>>5;
//   MFMA step s (0..3) therefore contracts channels {8kb+s, 8kb+4+s}: the K order is permuted identically for A and B.
//   The accumulator holds, for lane (j,h), rows (r&3) + 8*(r>>2) + 4h: registers 4g..4g+3 are four CONSECUTIVE output
//   channels 8g+4h.. of pixel j  => one float4 store per (g) lands in the quad-planar output, 512 B contiguous per
//   half wave.
//
// Schedule: PERSISTENT workgroups (one per CU) walk a stream of (output tile, K chunk) steps.  LDS holds NSTAGE stage
// images (weights + activation halo image of one K chunk) filled by LDS-DMA (global_load_lds_dwordx4):
//   NSTAGE = 3: the DMA of step s+2 is issued at the top of step s; one barrier per step proves that step s+1 has landed
//               for every wave, so the first fragments of step s+1 are read BEFORE the next barrier and the matrix pipe
//               never drains at a step boundary -- nor at a tile boundary: the next tile's first chunks are already
//               in flight while the epilogue stores of the finished tile are issued.
//   NSTAGE = 2: (rows too wide for three stage images) DMA of step s+1 issued at the top of step s, fragments read after
//               the barrier.
// Workgroup ids are remapped so that the 32 workgroups sharing an XCD (and its L2) walk adjacent tiles.
#include <stdlib.h>

#include <initializer_list>
#include <type_traits>

#include "nd_common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// One 16-byte MFMA operand fragment per lane and K block:
//   ND_F32  : 4 fp32 channels  -> 4 x v_mfma_f32_32x32x2_f32   (K block = 8 channels over the two lane halves)
//   ND_BF16 : 8 bf16 channels  -> 1 x v_mfma_f32_32x32x16_bf16 (K block = 16 channels)
//   ND_F16  : 8 fp16 channels  -> 1 x v_mfma_f32_32x32x16_f16
template <int DT> struct FragOf { typedef f32x4 type; };
template <> struct FragOf<ND_BF16> { typedef bf16x8 type; };
template <> struct FragOf<ND_F16> { typedef f16x8 type; };

// n / d for n < 2^31 as one 64-bit multiply and shift (m = ceil(2^(31+s) / d), s = ceil(log2 d): exact below 2^31).  The tile
// geometry (image, row, column of a pixel; M / N tile of a work item) needs several divisions by launch constants per tile and
// lane; a hardware-less 32-bit division is ~35 VALU instructions, each of them matrix-pipe time next to the fp32 MFMA.
struct FastDiv {
    unsigned m;
    int sh;
};
static inline FastDiv nd_fastdiv(int d) {
    FastDiv f;
    int s = 0;
    while ((1L << s) < (long)d) ++s;
    f.m = (unsigned)((((unsigned long long)1 << (31 + s)) + (unsigned long long)d - 1) / (unsigned long long)d);
    f.sh = 31 + s;
    return f;
}
__device__ __forceinline__ unsigned fdiv(unsigned n, const FastDiv &f) { return (unsigned)(((unsigned long long)n * f.m) >> f.sh); }

struct ConvParams {
    const f32x4 *in;     // plane 0 of the input buffer
    const float *wpk;    // packed weights
    const float *bias;   // [mtiles*32]
    f32x4 *out;          // plane 0 of the destination buffer
    long in_plane;       // float4 per input plane
    long out_plane;      // float4 per output plane
    int nimg;            // images in the batch
    int P, Wb;           // Hb*Wb, Wb of the input buffer
    int Hv, Wv, PV;      // valid output rows / cols per image, PV = Hv*Wv
    int tpi;             // > 0: tiles never cross an image, tpi tiles per image (wide rows); 0: tiles run over the whole batch
    int G;               // 64-pixel DMA pieces per plane and stage (covers the largest input span of a tile + halo)
    int stride;          // input pixels per output pixel (2 for the 2x2 stride-2 convolution, else 1)
    int ioff;            // linear offset of the first valid input pixel (1- and 4-tap layers reading a bordered buffer)
    f32x4 *pre;          // training: pre-activation copy, compact planes (null: none)
    long pre_plane;
    int KB;              // Cin / 8
    int M;               // GEMM rows (Cout, or 4*Cout for the 2x2 stride-2 transpose)
    int cout;            // output channels
    int Po, Wo, opad;    // destination buffer: Hb*Wb, Wb, border
    int out_plane0;      // first destination plane
    int act;
    float slope;
    const float *slope_dev;
    int n_tiles_n;       // N tiles (pixels / NBLK, rounded up)
    int n_tiles_m;       // M tiles (rows / MBLK, rounded up)
    // split-K tail: tiles [split_first, ntiles) are cut into S slices of `cps` K chunks each (the last may be shorter);
    // a slice stores its raw accumulators tile-locally into `part` and k_split_finish adds them up.  nitems = work items.
    int split_first, S, cps, nitems;
    f32x4 *part;         // [slice item][MBLK/4 channel quads][NBLK pixels]
    // batch of independent problems of one shape in one launch (the 16 / 36 / 64 positions of a Winograd layer): tile ids run
    // over batch x (N tiles x M tiles); problem z reads in + z*in_bs, wpk + z*w_bs and writes out + z*out_bs
    int wpx;                 // > 0: valid pixels per row when the N enumeration has slots past the row end (conv_w1d.hip)
    int tiles_per_problem;   // n_tiles_n * n_tiles_m
    long in_bs, out_bs;      // 16-byte elements
    long w_bs;               // floats
    int dbg;                 // ablation bits for kernel timing experiments (0 in production)
    // 1: the valid grid has no gaps (1-tap layer on an unbordered buffer whose output has the same geometry -- the GEMMs of a
    // three-pass Winograd layer): pixel l of N tile nb IS linear index nb * NBLK + l on both sides, and the epilogue stores the raw
    // sums (no bias, no activation): no integer division and no arithmetic per tile
    int linear;
    FastDiv fd_PV, fd_Wv, fd_ntm, fd_tpp, fd_upq, fd_tpi;   // dividers by PV, Wv, n_tiles_m, tiles_per_problem, cout / (4 | 8), tpi (set by nd_conv_fastdivs)
    // conv_w2d.hip: fused 2x2 max pool of the activated output (null: none) -- plane stride, pixels per image, row width, border
    f32x4 *pool;
    long pool_plane;
    int pool_P, pool_W, pool_pad;
    // conv_qp with a fused pool (16-bit storage): the compact pixel index of an image runs over 2-ROW BANDS -- band, column, row
    // in band -- so that a 2x2 pooling block is four consecutive pixels of an N tile, i.e. four adjacent lanes of one accumulator
    int band2;
    FastDiv fd_2Wv;   // divider by 2 * Wv
    // conv_w2d.hip, second input source (ConvDesc::in2; null: none): K blocks [kb2, KB) read plane 2 * (kb - kb2) + half of in2, where
    // the bordered pixel (y, x) of image t is element origin2[t] + y * Wb2 + x
    const f32x4 *in2;
    long in2_plane;
    const int *origin2;
    int kb2, Wb2;
    // conv_qp, conv_w2d.hip: K blocks per M tile of the packed weights (ConvDesc::w_kb; = KB unless the launch runs a K-block
    // sub-range, whose first block wpk already points at)
    int KBw;
    // conv_w2d.hip, addend source (ConvDesc::add; null: none): the addend of valid output pixel (y, x) of image t, channel quad q, is
    // element origin_add[t] + y * W_add + x of plane q (the border and region shifts are folded into `add`)
    const f32x4 *add;
    long add_plane;
    const int *origin_add;
    int W_add;
};

static inline void nd_conv_fastdivs(ConvParams &p) {
    p.fd_PV = nd_fastdiv(p.PV > 0 ? p.PV : 1);
    p.fd_Wv = nd_fastdiv(p.Wv > 0 ? p.Wv : 1);
    p.fd_2Wv = nd_fastdiv(p.Wv > 0 ? 2 * p.Wv : 1);
    p.fd_ntm = nd_fastdiv(p.n_tiles_m > 0 ? p.n_tiles_m : 1);
    p.fd_tpp = nd_fastdiv(p.tiles_per_problem > 0 ? p.tiles_per_problem : 1);
    p.fd_upq = nd_fastdiv(p.cout / 4 > 0 ? p.cout / 4 : 1);   // fp32 (4 channels per plane element); nd_launch_conv overrides it for 16-bit storage
    p.fd_tpi = nd_fastdiv(p.tpi > 0 ? p.tpi : 1);
}

// ------------------------------------------------------------------ host side of the launchers (launch.hip)
// the fields every launcher sets the same way from the layer: input / destination pointers and geometry, pre-activation copy, K
// blocks, M rows, activation.  The launcher adds its valid grid (Hv, Wv, PV, wpx), G, stride, ioff, region shifts and schedule
ConvParams nd_conv_params(const ConvDesc &d, int KB, int M);
// fused MaxPool2d(2) of an Hv x Wv output into *d.pool (checked against it)
int nd_conv_pool(const char *who, const ConvDesc &d, int Hv, int Wv, ConvParams &p);
// tile counts: N tiles of nblk valid pixels (or groups) over the whole batch when tiles may cross images (tpi = 0), else tpi
// tiles per image; M tiles of mblk rows
void nd_conv_tiles(ConvParams &p, bool cross, int nblk, int mblk);
// persistent-grid schedule of ntiles tiles of nchunks K chunks on `slots` concurrent workgroups, with split-K scratch for `cap`
// work items (0: never split): sets split_first / S / cps / nitems and returns the grid
long nd_conv_schedule(ConvParams &p, long ntiles, int nchunks, long slots, long cap);
double nd_conv_schedule_time(long ntiles, int nchunks, long slots, long cap);   // its length in "one workgroup, one K chunk" units
// shared with conv_w1d.hip (defined in conv_f32.hip)
int nd_launch_split_finish(const ConvParams &p, int n_split_tiles, int mblk, int nblk, int up, int dt, hipStream_t s);
#ifdef ND_QP_STAMPS
// diagnostic build (make STAMPS=1): the launch without split-K, p.part carrying the stamp buffer ([workgroup][wave][phases, -,
// steps]), synchronous; if `print`, the header line and, per wave of `waves`, each phase's cycles per step
int nd_stamped_launch(void (*fn)(ConvParams), int threads, size_t lds, ConvParams p, long ntiles, int nchunks, long slots, hipStream_t s,
                      bool print, const char *header, const char *wave_prefix, const char *const *names, int nphases, std::initializer_list<int> waves);
#endif

__device__ __forceinline__ void glds16(const void *g, void *l) {
    // 64 lanes x 16 B: per-lane global source, LDS destination = wave-uniform base + lane*16
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                     (__attribute__((address_space(3))) void *)l, 16, 0, 0);
}

// 8 consecutive floats at a wave-uniform address through the scalar cache (lgkmcnt, not vmcnt)
__device__ __forceinline__ f32x8 sload8(const float *p) {
    // the address is wave-uniform by construction; say so explicitly so that it lives in SGPRs
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const float *sp = (const float *)(((unsigned long long)hi << 32) | lo);
    f32x8 v;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(sp) : "memory");
    return v;
}
// The bias of the 4 channels a lane owns in accumulator group g: channels m8 + 4h .. + 3 of the 8 at p (h = lane >> 5).  Two
// separate 4-float scalar loads and ONE select per value: written as `h ? b8[4 + e] : b8[e]` on an 8-float vector hipcc folds
// the select into a dynamic vector index and emits a 7-deep v_cmp / v_cndmask chain per value (~2,200 VALU instructions per
// epilogue of the 256 x 256 GEMM tile, each of them matrix-pipe time next to the fp32 MFMA).
__device__ __forceinline__ f32x4 sload_bias4(const float *p, int h) {
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)a);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32));
    const float *sp = (const float *)(((unsigned long long)hi << 32) | lo);
    f32x4 b0, b1;
    asm volatile("s_load_dwordx4 %0, %2, 0x0\n\ts_load_dwordx4 %1, %2, 0x10\n\ts_waitcnt lgkmcnt(0)" : "=&s"(b0), "=&s"(b1) : "s"(sp) : "memory");
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = h ? b1[e] : b0[e];
    return r;
}

#ifdef ND_QP_STAMPS
// diagnostic build (make STAMPS=1; ND_QP_DBG=128 at run time): s_memtime stamps around the phases of a step
__device__ __forceinline__ unsigned long long qp_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define QP_STAMP(k) do { if (stamps) { t1 = qp_stamp(); tph[k] += t1 - t0; t0 = t1; } } while (0)
#else
#define QP_STAMP(k) do { } while (0)
#endif

// maximum over the aligned quad of lanes 4k .. 4k + 3 (two DPP quad permutes: [1,0,3,2] then [2,3,0,1])
__device__ __forceinline__ float quad_max(float v) {
    int a = __builtin_bit_cast(int, v);
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(a, a, 0xB1, 0xF, 0xF, false)));
    a = __builtin_bit_cast(int, v);
    return fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(a, a, 0x4E, 0xF, 0xF, false)));
}

__device__ __forceinline__ float apply_act(float v, int act, float slope) {
    switch (act) {
        case ND_ACT_PRELU: return v > 0.f ? v : v * slope;
        case ND_ACT_ELU: return v > 0.f ? v : expm1f(v);
        case ND_ACT_HARDSWISH: return v * fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f;
        default: return v;
    }
}

// MR x NR : 32x32 MFMA tiles per wave;  WM x WN : waves per workgroup;  TAPS in {9,1};  KBC : 8-channel blocks per chunk
template <int DT, int MR, int NR, int WM, int WN, int TAPS, int KBC, bool UP, int NSTAGE>
__global__ __launch_bounds__(64 * WM * WN) void conv_qp(ConvParams p) {
    typedef typename FragOf<DT>::type Frag;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = WM * WN;
    constexpr int MTB = MR * WM;                    // 32-row tiles per workgroup
    constexpr int NBLK = 32 * NR * WN;              // pixels per workgroup tile
    constexpr int WBYTES = MTB * KBC * TAPS * 1024; // weight bytes per stage
    constexpr int STEPS = KBC * TAPS;               // fragment sub-steps per K chunk

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int j = lane & 31, h = lane >> 5;

    // XCD-aware id: hardware deals workgroups round-robin over the 8 XCDs; give each XCD a contiguous id range
    const int nwg = gridDim.x;
    const int bid = blockIdx.x;
    const int vb = (nwg % 8 == 0) ? (bid % 8) * (nwg / 8) + bid / 8 : bid;

    const int G = p.G;
    const int planeB = G * 1024;
    const int stageB = WBYTES + 2 * KBC * planeB;

    int toff[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; ++t)
        toff[t] = TAPS == 9 ? ((t / 3) * p.Wb + (t % 3)) * 16 : (TAPS == 4 ? ((t / 2) * p.Wb + (t % 2)) * 16 : 0);

    const int nchunks = p.KB / KBC;
    const int nitems = p.nitems;
    const int my_items = vb < nitems ? (nitems - vb + nwg - 1) / nwg : 0;
    // work item -> (tile, K chunk range, slice index or -1): whole tiles first, the K slices of the split tail after them
    struct Item { int tile, c0, c1, slice; };
    auto decode = [&](int w) -> Item {
        Item it;
        if (w < p.split_first) {
            it.tile = w; it.c0 = 0; it.c1 = nchunks; it.slice = -1;
        } else {
            const int u = w - p.split_first;
            const int t = u / p.S, ks = u - t * p.S;
            it.tile = p.split_first + t;
            it.c0 = ks * p.cps;
            it.c1 = it.c0 + p.cps < nchunks ? it.c0 + p.cps : nchunks;
            it.slice = u;
        }
        return it;
    };
    int nsteps = 0;
    if (p.split_first >= nitems)
        nsteps = my_items * nchunks;
    else
        for (int i = 0; i < my_items; ++i) {
            const Item it = decode(vb + i * nwg);
            nsteps += it.c1 - it.c0;
        }
    if (nsteps == 0) return;

    // ---- tile geometry: N tile nb covers NBLK consecutive valid pixels (of one image if p.tpi, else of the batch)
    // (image, compact index) of the l-th pixel of N tile nb; pixels past the end are clamped to the last valid one
    auto pixel_of = [&](int nb, int l, int &img, int &r) -> bool {
        bool ok;
        if (p.tpi) {
            img = (int)fdiv((unsigned)nb, p.fd_tpi);
            r = (nb - img * p.tpi) * NBLK + l;
            ok = r < p.PV;
            r = ok ? r : p.PV - 1;
        } else {
            // (the launcher refuses buffers of 2^31 linear pixels or more: 32-bit unsigned arithmetic, one cheap division)
            const unsigned g = (unsigned)nb * (unsigned)NBLK + (unsigned)l;
            const unsigned tot = (unsigned)p.nimg * (unsigned)p.PV;
            ok = g < tot;
            const unsigned gc = ok ? g : tot - 1;
            img = (int)fdiv(gc, p.fd_PV);
            r = (int)(gc - (unsigned)img * (unsigned)p.PV);
        }
        return ok;
    };
    // (row, column) of compact index r inside its image: row-major, or -- band2 -- 2-row bands [band][column][row in band]
    auto yx_of = [&](int r, int &y, int &x) {
        if (p.band2) {
            const int band = (int)fdiv((unsigned)r, p.fd_2Wv), rem = r - band * 2 * p.Wv;
            y = 2 * band + (rem & 1);
            x = rem >> 1;
        } else {
            y = (int)fdiv((unsigned)r, p.fd_Wv);
            x = r - y * p.Wv;
        }
    };
    // linear input index of (image, compact index)
    auto q_of = [&](int img, int r) -> long {
        int y, x;
        yx_of(r, y, x);
        return (long)img * p.P + (long)(y * p.stride) * p.Wb + x * p.stride + p.ioff;
    };
    auto tile_q0 = [&](int nb) -> long {   // wave-uniform: input index of the tile's first pixel
        if (TAPS == 1 && !UP && p.linear) return (long)nb * NBLK;
        int img, r;
        pixel_of(nb, 0, img, r);
        return q_of(img, r);
    };

    // ---- DMA cursor: walks the same (tile, chunk) stream as the compute loop, NSTAGE-1 steps ahead
    int f_id = vb, f_c = 0, f_end = 0, f_stage = 0, issued = 0;
    const float *f_w;
    const f32x4 *f_a;
    auto set_fill_tile = [&](int w) {
        const Item it = decode(w);
        f_c = it.c0;
        f_end = it.c1;
        const int z = (int)fdiv((unsigned)it.tile, p.fd_tpp), id = it.tile - z * p.tiles_per_problem;
        const int nb = (int)fdiv((unsigned)id, p.fd_ntm), mb = id - nb * p.n_tiles_m;   // M tiles of one N tile run back to back
        f_w = p.wpk + z * p.w_bs + (size_t)mb * MTB * p.KBw * TAPS * 256 + lane * 4;
        f_a = p.in + z * p.in_bs + tile_q0(nb) + lane;
    };
    set_fill_tile(f_id);
    // Who issues the DMA, and when.
    // fp32: waves 0..3 -- one per SIMD -- issue the whole step at its top; their SIMD partners (waves 4..7) go straight to their
    // MFMAs, so the matrix pipe is fed meanwhile (in-kernel stamps, profiles/r02_conv_qp_stamps.log: the two waves of a SIMD end up
    // taking turns, each running its 128 MFMAs alone at ~92 % of the pipe rate; interleaving the pieces with the issuing wave's
    // own MFMAs or cutting the instructions per piece moved nothing -- every instruction next to an fp32 MFMA is matrix-pipe time).
    // 16-bit storage (SPREAD): the MFMAs of a step are 4x shorter than its DMA issue phase, a wave running alone gets ~45 % of
    // the pipe (LDS fragment reads) and the step was [issue 3,200 | partner alone 5,300 | issuer alone 3,500 cycles]: there the
    // pieces are cut into NSLICE slices (the weights of one M tile; a share of one activation plane) that ALL waves issue, one
    // slice after each of their first MFMA groups, so that both waves of a SIMD run their MFMAs side by side.
    constexpr bool SPREAD = DT != ND_F32 && TAPS == 9;   // (the 1-tap layers have 1 - 4 groups per step: measured slower there)
    constexpr int NFILL = SPREAD ? NW : (NW > 4 ? 4 : NW);
    constexpr int RW = KBC * TAPS;                     // 1-KiB weight pieces per M tile and step
    constexpr int NGROUPS = STEPS * (DT == ND_F32 ? 4 : 1);   // MFMA groups (MR x NR MFMAs each) per step
    // the slices go out during the first NUSE groups (~60 % of the step: the last piece needs time to land), SPG per group;
    // planes are cut in PSUB shares where there are groups to spread them over
#ifndef ND_QP_NUSE_NUM
#define ND_QP_NUSE_NUM 5
#endif
    constexpr int NUSE = NGROUPS * ND_QP_NUSE_NUM / 8 > 1 ? NGROUPS * ND_QP_NUSE_NUM / 8 : 1;
    constexpr int PSUB_ = (NUSE - MTB) / (2 * KBC);
    constexpr int PSUB = PSUB_ < 1 ? 1 : (PSUB_ > 4 ? 4 : PSUB_);
    constexpr int NSLICE = MTB + 2 * KBC * PSUB;
    constexpr int SPG = (NSLICE + NUSE - 1) / NUSE;
    char *fill_sb = smem;
    bool fill_on = false;
    auto fill_begin = [&]() {
        fill_on = issued < nsteps;
        fill_sb = smem + f_stage * stageB;
    };
    auto fill_slice = [&](int i) {   // i: compile-time after unrolling
        if (!fill_on || wave >= NFILL) return;
#ifdef ND_QP_ABLATE
        if (p.dbg & (i < MTB ? 2 : 1)) return;   // timing experiment (make ABLATE=1): 1 = no activation DMA, 2 = no weight DMA
#endif
        if (i < MTB) {
            const float *src = f_w + ((size_t)i * p.KBw + (size_t)f_c * KBC) * TAPS * 256;
            char *dst = fill_sb + i * RW * 1024;
            for (int q = wave; q < RW; q += NFILL) glds16(src + q * 256, dst + q * 1024);
        } else {
            const int pl = (i - MTB) / PSUB, part = (i - MTB) % PSUB;
            const f32x4 *src = f_a + (size_t)(f_c * 2 * KBC + pl) * p.in_plane;
            char *dst = fill_sb + WBYTES + pl * planeB;
            for (int g = wave + part * NFILL; g < G; g += NFILL * PSUB) glds16(src + g * 64, dst + g * 1024);
        }
    };
    auto fill_end = [&]() {
        if (!fill_on) return;
        ++issued;
        f_stage = (f_stage + 1 == NSTAGE) ? 0 : f_stage + 1;
        if (++f_c == f_end) {
            f_id += nwg;
            if (f_id < nitems) set_fill_tile(f_id);
        }
    };
    auto fill_group = [&](int gi) {   // after MFMA group gi of the step (gi: compile-time after unrolling)
        if (!SPREAD || gi * SPG >= NSLICE) return;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < SPG; ++k)
            if (gi * SPG + k < NSLICE) {
                fill_slice(gi * SPG + k);
                if (gi * SPG + k == NSLICE - 1) fill_end();
            }
        __builtin_amdgcn_sched_barrier(0);
    };
    auto fill_next = [&]() {   // a whole step at once
        fill_begin();
#pragma unroll
        for (int i = 0; i < NSLICE; ++i) fill_slice(i);
        fill_end();
    };

    // ---- fragments
    const int aOff = (wm * MR) * KBC * TAPS * 1024 + lane * 16;
    // byte offset of this lane's pixel inside a stage's activation image, for each of the wave's NR pixel groups
    struct BOff { int v[NR]; };
    auto lane_offsets = [&](int w) -> BOff {
        BOff o;
        if (TAPS == 1 && !UP && p.linear) {   // the stage image starts at the tile's first pixel, pixel l sits at l
#pragma unroll
            for (int nr = 0; nr < NR; ++nr) o.v[nr] = WBYTES + h * planeB + ((wn * NR + nr) * 32 + j) * 16;
            return o;
        }
        const int tl_ = decode(w).tile;
        const int nb = (int)fdiv((unsigned)(tl_ - (int)fdiv((unsigned)tl_, p.fd_tpp) * p.tiles_per_problem), p.fd_ntm);
        const long q0 = tile_q0(nb);
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) {
            int img, r;
            pixel_of(nb, (wn * NR + nr) * 32 + j, img, r);
            o.v[nr] = WBYTES + h * planeB + (int)(q_of(img, r) - q0) * 16;
        }
        return o;
    };
    BOff bOff = lane_offsets(vb), bOffN = bOff;
    Frag a[2][MR] = {}, b[2][NR] = {};
    auto load_frags = [&](int buf, const char *sb, int step, const BOff &bo) {
        const int kbl = step / TAPS, t = step % TAPS;
#pragma unroll
        for (int mr = 0; mr < MR; ++mr)
            a[buf][mr] = *(const Frag *)(sb + aOff + ((mr * KBC + kbl) * TAPS + t) * 1024);
#pragma unroll
        for (int nr = 0; nr < NR; ++nr)
            b[buf][nr] = *(const Frag *)(sb + bo.v[nr] + kbl * 2 * planeB + toff[t]);
    };

    f32x16 acc[MR][NR];
#pragma unroll
    for (int x = 0; x < MR; ++x)
#pragma unroll
        for (int y = 0; y < NR; ++y)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[x][y][r] = 0.f;

    const float slope = p.act == ND_ACT_NONE ? 1.f : (p.slope_dev ? *p.slope_dev : p.slope);

    // ---- epilogue of one finished tile: bias + activation, float4 stores into the (bordered, concatenated) destination.
    // Every VALU instruction here is matrix-pipe time (on gfx950 the fp32 MFMA shares the SIMD's fp32 datapath: +4.5 cycles per
    // VALU instruction at two waves per SIMD, tools/ubench/mfma_f32_fillers.hip): the bias of a channel group is fetched once
    // (scalar cache) and reused for the wave's NR pixel groups, PReLU with 0 <= slope <= 1 is max(t, slope * t).
    const bool slope01 = p.act <= ND_ACT_PRELU && slope >= 0.f && slope <= 1.f;
    auto epilogue = [&](int gid, auto generic_act) {
        const int z = (int)fdiv((unsigned)gid, p.fd_tpp), id = gid - z * p.tiles_per_problem;
        const int nb = (int)fdiv((unsigned)id, p.fd_ntm), mb = id - nb * p.n_tiles_m;
        f32x4 *const outz = p.out + z * p.out_bs;
        if constexpr (TAPS == 1 && !UP && DT == ND_F32) {
            if (p.linear) {
                const unsigned tot = (unsigned)p.nimg * (unsigned)p.PV;
#pragma unroll
                for (int nr = 0; nr < NR; ++nr) {
                    const unsigned g = (unsigned)nb * (unsigned)NBLK + (unsigned)((wn * NR + nr) * 32 + j);
#pragma unroll
                    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                        for (int gq = 0; gq < 4; ++gq) {
                            const int m4 = ((mb * MTB + wm * MR + mr) * 32) + 8 * gq + 4 * h;
                            f32x4 v;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                v[e] = acc[mr][nr][4 * gq + e];
                                acc[mr][nr][4 * gq + e] = 0.f;
                            }
                            if (g < tot && m4 < p.M) outz[(long)(p.out_plane0 + (m4 >> 2)) * p.out_plane + g] = v;
                        }
                }
                return;
            }
        }
        bool valid[NR];
        long pbase[NR], prbase[NR], ppool[NR];   // (ppool: the pooled pixel of a lane's 2x2 block; used by lanes j % 4 == 0 of a band2 launch)
#pragma unroll
        for (int nr = 0; nr < NR; ++nr) {
            int bi, r;
            valid[nr] = pixel_of(nb, (wn * NR + nr) * 32 + j, bi, r);
            int y, x;
            yx_of(r, y, x);
            if constexpr (DT != ND_F32 && !UP) ppool[nr] = (long)bi * p.pool_P + (long)((y >> 1) + p.pool_pad) * p.pool_W + (x >> 1) + p.pool_pad;
            pbase[nr] = UP ? (long)bi * p.Po + (long)(2 * y + p.opad) * p.Wo + (2 * x + p.opad)
                           : (long)bi * p.Po + (long)(y + p.opad) * p.Wo + (x + p.opad);
            prbase[nr] = (long)bi * p.PV + r;
        }
        // bias + activation of the 4 rows (consecutive output channels) a lane owns in accumulator group g of (mr, nr)
        auto activated = [&](int mr, int nr, int g, const f32x4 &bv, long pre_off) -> f32x4 {
            f32x4 t, v;
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = acc[mr][nr][4 * g + e] + bv[e];
            if constexpr (DT == ND_F32 && !UP) {
                if (p.pre && pre_off >= 0) p.pre[pre_off] = t;   // training forward: acc + bias for the activation's backward pass
            }
            if constexpr (decltype(generic_act)::value == 2) {
                v = t;   // no activation (the 2x2 stride-2 transposes, data gradients): not even the max(t, 1 * t) of the PReLU form
            } else if constexpr (decltype(generic_act)::value == 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = apply_act(t[e], p.act, slope);
            } else {
                if (slope01) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(t[e], t[e] * slope);   // PReLU; "no activation" is slope 1
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = t[e] > 0.f ? t[e] : t[e] * slope;
                }
            }
            return v;
        };
        const int upq = p.cout / (DT == ND_F32 ? 4 : 8);   // plane elements per output pixel (2x2 stride-2 transpose: nd_up_row)
#pragma unroll
        for (int mr = 0; mr < MR; ++mr) {
            const int mbase = (mb * MTB + wm * MR + mr) * 32;   // wave-uniform
            if constexpr (DT == ND_F32) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    // bias through the scalar cache (a vector load here would make the compiler wait vmcnt(0), i.e. for the LDS-DMA of
                    // the next steps that is in flight during the epilogue)
                    const int m8 = mbase + 8 * g;   // wave-uniform
                    const f32x4 bv = sload_bias4(p.bias + m8, h);
                    // destination plane and pixel offset: rows m8 + 4h + e are 4 consecutive channels; for the 2x2 stride-2
                    // transpose the halves h are the output columns 2x, 2x + 1 of ONE channel quad (nd_up_row): scalar decode,
                    // and the 64 lanes of a store write 64 consecutive plane elements
                    int plane = p.out_plane0 + ((m8 + 4 * h) >> 2);
                    long pixo = 0;
                    bool rows_ok = m8 + 4 * h < p.M;
                    if (UP) {
                        const int G = m8 >> 3, a = (int)fdiv((unsigned)G, p.fd_upq);
                        plane = p.out_plane0 + (G - a * upq);
                        pixo = (long)a * p.Wo + h;
                        rows_ok = m8 < p.M;
                    }
#pragma unroll
                    for (int nr = 0; nr < NR; ++nr) {
                        if (valid[nr] && rows_ok) {
                            const f32x4 v = activated(mr, nr, g, bv, (DT == ND_F32 && !UP && p.pre) ? (long)((m8 + 4 * h) >> 2) * p.pre_plane + prbase[nr] : -1);
#ifdef ND_QP_ABLATE
                            if (!(p.dbg & 4))   // timing experiment: no epilogue stores
#endif
                            outz[(long)plane * p.out_plane + pbase[nr] + pixo] = v;
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[mr][nr][4 * g + e] = 0.f;
                    }
                }
            } else {
                // 16-bit storage: a plane element holds 8 channels (16 bytes) and a lane owns 4 (rows 8g + 4h + e).  Two groups at a
                // time: after bias + activation + rounding, v_permlane32_swap exchanges the upper lane half of group 2gp with the
                // lower half of group 2gp + 1, so that lane (j, 0) holds all 8 channels of group 2gp and lane (j, 1) all 8 of group
                // 2gp + 1: one 16-byte store per lane instead of two 8-byte ones (half the store instructions, whole elements).
                // 2x2 stride-2 transpose: the two groups are the output columns 2x, 2x + 1 of one channel octet (nd_up_row), the
                // 64 lanes write 64 consecutive plane elements.
#pragma unroll
                for (int gp = 0; gp < 2; ++gp) {
                    const int m16 = mbase + 16 * gp;   // wave-uniform
                    const f32x4 bv0 = sload_bias4(p.bias + m16, h), bv1 = sload_bias4(p.bias + m16 + 8, h);
                    int plane = p.out_plane0 + ((m16 + 8 * h) >> 3);
                    long pixo = 0;
                    bool rows_ok = m16 + 8 * h < p.M;
                    if (UP) {
                        const int G = m16 >> 4, a = (int)fdiv((unsigned)G, p.fd_upq);
                        plane = p.out_plane0 + (G - a * upq);
                        pixo = (long)a * p.Wo + h;
                        rows_ok = m16 < p.M;
                    }
#pragma unroll
                    for (int nr = 0; nr < NR; ++nr) {
                        const f32x4 v0 = activated(mr, nr, 2 * gp, bv0, -1), v1 = activated(mr, nr, 2 * gp + 1, bv1, -1);
                        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                        u32x2 q0, q1;
                        if constexpr (DT == ND_BF16) {
                            bf16x4 o0, o1;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                o0[e] = (__bf16)v0[e];
                                o1[e] = (__bf16)v1[e];
                            }
                            q0 = __builtin_bit_cast(u32x2, o0);
                            q1 = __builtin_bit_cast(u32x2, o1);
                        } else {
                            f16x4 o0, o1;
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                o0[e] = (_Float16)v0[e];
                                o1[e] = (_Float16)v1[e];
                            }
                            q0 = __builtin_bit_cast(u32x2, o0);
                            q1 = __builtin_bit_cast(u32x2, o1);
                        }
                        // swap(vdst, vsrc): vdst's lanes 32..63 <-> vsrc's lanes 0..31
                        const u32x2 s0 = __builtin_amdgcn_permlane32_swap(q0[0], q1[0], false, false);
                        const u32x2 s1 = __builtin_amdgcn_permlane32_swap(q0[1], q1[1], false, false);
                        const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};   // rows +0,1 | +2,3 | +4,5 | +6,7 of this lane's 8-row group
                        if (valid[nr] && rows_ok) {
#ifdef ND_QP_ABLATE
                            if (!(p.dbg & 4))
#endif
                            *(u32x4 *)((char *)outz + (((long)plane * p.out_plane + pbase[nr] + pixo) << 4)) = o;
                        }
                        if constexpr (!UP) {
                            if (p.pool) {   // wave-uniform
                                // fused MaxPool2d(2): in the band order the four pixels of a 2x2 block are the lanes 4k .. 4k + 3 of this
                                // accumulator: maximum over the lane quad (two DPP quad permutes), then the same rounding, pairing and
                                // 16-byte store as above from the quad's first lane (the maximum of rounded values = the rounded maximum)
                                f32x4 m0 = v0, m1 = v1;
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    m0[e] = quad_max(m0[e]);
                                    m1[e] = quad_max(m1[e]);
                                }
                                u32x2 r0, r1;
                                if constexpr (DT == ND_BF16) {
                                    bf16x4 o0, o1;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        o0[e] = (__bf16)m0[e];
                                        o1[e] = (__bf16)m1[e];
                                    }
                                    r0 = __builtin_bit_cast(u32x2, o0);
                                    r1 = __builtin_bit_cast(u32x2, o1);
                                } else {
                                    f16x4 o0, o1;
#pragma unroll
                                    for (int e = 0; e < 4; ++e) {
                                        o0[e] = (_Float16)m0[e];
                                        o1[e] = (_Float16)m1[e];
                                    }
                                    r0 = __builtin_bit_cast(u32x2, o0);
                                    r1 = __builtin_bit_cast(u32x2, o1);
                                }
                                const u32x2 t0 = __builtin_amdgcn_permlane32_swap(r0[0], r1[0], false, false);
                                const u32x2 t1 = __builtin_amdgcn_permlane32_swap(r0[1], r1[1], false, false);
                                const u32x4 po = {t0[0], t1[0], t0[1], t1[1]};
                                if (valid[nr] && rows_ok && !(j & 3))
                                    *(u32x4 *)((char *)p.pool + (((long)((m16 + 8 * h) >> 3) * p.pool_plane + ppool[nr]) << 4)) = po;
                            }
                        }
#pragma unroll
                        for (int e = 0; e < 8; ++e) acc[mr][nr][8 * gp + e] = 0.f;
                    }
                }
            }
        }
    };

    // ---- a K slice of a split tile: raw accumulators, tile-local layout [quad][pixel] (k_split_finish adds bias etc.)
    auto epilogue_partial = [&](int slice) {
        f32x4 *dst = p.part + (size_t)slice * (MTB * 8) * NBLK;
#pragma unroll
        for (int nr = 0; nr < NR; ++nr)
#pragma unroll
            for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        v[e] = acc[mr][nr][4 * g + e];
                        acc[mr][nr][4 * g + e] = 0.f;
                    }
                    dst[(size_t)((wm * MR + mr) * 8 + 2 * g + h) * NBLK + (wn * NR + nr) * 32 + j] = v;
                }
    };

    // ---- prologue
#pragma unroll
    for (int i = 0; i < NSTAGE - 1; ++i) fill_next();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (NSTAGE == 3) load_frags(0, smem, 0, bOff);

    int c_id = vb, c_stage = 0;
    Item c_it = decode(vb);
    int c_c = c_it.c0;
#ifdef ND_QP_STAMPS
    const bool stamps = p.dbg & 128;
    unsigned long long tph[5] = {0, 0, 0, 0, 0}, t0 = 0, t1 = 0;
#endif
    for (int s = 0; s < nsteps; ++s) {
#ifdef ND_QP_STAMPS
        if (stamps) t0 = qp_stamp();
#endif
        // my share of the youngest outstanding DMA was issued one whole step ago
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        QP_STAMP(3);
        __builtin_amdgcn_s_barrier();
        QP_STAMP(0);
        if (SPREAD) fill_begin(); else fill_next();
        QP_STAMP(1);
        const char *sb = smem + c_stage * stageB;
        const int n_stage = (c_stage + 1 == NSTAGE) ? 0 : c_stage + 1;
        const bool last_chunk = c_c + 1 == c_it.c1;
        // the fragments prefetched at the end of a tile's last chunk belong to the NEXT tile: its lane offsets
        if (last_chunk && c_id + nwg < nitems) bOffN = lane_offsets(c_id + nwg);
        if (NSTAGE == 2) load_frags(0, sb, 0, bOff);
#pragma unroll
        for (int st = 0; st < STEPS; ++st) {
            if (st + 1 < STEPS)
                load_frags((st + 1) & 1, sb, st + 1, bOff);
            else if (NSTAGE == 3 && s + 1 < nsteps)   // next step's first fragments, before its barrier
                load_frags((st + 1) & 1, smem + n_stage * stageB, 0, last_chunk ? bOffN : bOff);
            if constexpr (DT == ND_F32) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                        for (int nr = 0; nr < NR; ++nr)
                            acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st & 1][mr][q], b[st & 1][nr][q], acc[mr][nr], 0, 0, 0);
            } else {
#pragma unroll
                for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                    for (int nr = 0; nr < NR; ++nr) {
                        if constexpr (DT == ND_BF16)
                            acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[st & 1][mr], b[st & 1][nr], acc[mr][nr], 0, 0, 0);
                        else
                            acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[st & 1][mr], b[st & 1][nr], acc[mr][nr], 0, 0, 0);
                    }
                fill_group(st);
            }
        }
        if (NSTAGE == 3 && (STEPS & 1)) {
            // an odd number of sub-steps leaves the prefetched fragments in buffer 1: the next step starts from buffer 0
#pragma unroll
            for (int mr = 0; mr < MR; ++mr) a[0][mr] = a[1][mr];
#pragma unroll
            for (int nr = 0; nr < NR; ++nr) b[0][nr] = b[1][nr];
        }
        c_stage = n_stage;
        QP_STAMP(2);
        if (++c_c == c_it.c1) {
            if (c_it.slice >= 0)
                epilogue_partial(c_it.slice);
            else if (p.act == ND_ACT_NONE)
                epilogue(c_it.tile, std::integral_constant<int, 2>{});
            else if (p.act == ND_ACT_PRELU)
                epilogue(c_it.tile, std::integral_constant<int, 0>{});
            else
                epilogue(c_it.tile, std::integral_constant<int, 1>{});
            c_id += nwg;
            if (c_id < nitems) c_it = decode(c_id);
            c_c = c_it.c0;
            bOff = bOffN;
        }
        QP_STAMP(4);
    }
#ifdef ND_QP_STAMPS
    if (stamps && lane == 0) {   // the launcher passes the stamp buffer in p.part: [workgroup][wave][5 phases, -, steps]
        unsigned long long *o = (unsigned long long *)p.part + ((size_t)blockIdx.x * 8 + wave) * 8;
        for (int k = 0; k < 5; ++k) o[k] = tph[k];
        o[6] = (unsigned long long)nsteps;
    }
#endif
}


struct Variant {
    const char *name;
    int dt, mblk, nblk, threads, taps, kbc, nstage;
    bool up;
    void (*fn)(ConvParams);
};

#define ND_VARIANT(DT, DTN, MR, NR, WM, WN, TAPS, KBC, UP, NS)                                                         \
    {                                                                                                                  \
        DTN "_m" #MR "x" #WM "_n" #NR "x" #WN "_t" #TAPS "_k" #KBC "_up" #UP "_s" #NS, DT, 32 * MR * WM, 32 * NR * WN,  \
            64 * WM * WN, TAPS, KBC, NS, UP, conv_qp<DT, MR, NR, WM, WN, TAPS, KBC, UP, NS>                            \
    }
// the shapes every storage type gets (index inside a dtype group)
#define ND_VARIANT_GROUP(DT, DTN)                                                                                      \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 9, 1, false, 3),  /* 0: M64  x N512, 8 waves, 3 stages  (default 3x3)           */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 9, 1, false, 2),  /* 1: M64  x N512, 8 waves, 2 stages  (wide rows: cs >= ~400) */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 4, 9, 1, false, 2),  /* 2: M64  x N256, 4 waves, 2 stages  (widest rows)           */ \
    ND_VARIANT(DT, DTN, 1, 2, 1, 8, 9, 1, false, 3),  /* 3: M32  x N512, 8 waves (narrow nets / tests)              */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 1, 2, false, 3),  /* 4: 1x1, M64 x N512                                         */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 1, 1, false, 3),  /* 5: 1x1, single-K-block chunks                              */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 1, 2, true, 3),   /* 6: up (2x2 s2), M64 x N512                                 */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 1, 1, true, 3),   /* 7: up, single-K-block chunks                               */ \
    ND_VARIANT(DT, DTN, 2, 2, 2, 4, 1, 2, true, 3),   /* 8: up, M128 x N256, 8 waves                                */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 1, 4, true, 2),   /* 9: up, M64 x N512, 4 K blocks per step, 2 stages            */ \
    ND_VARIANT(DT, DTN, 2, 2, 2, 4, 1, 4, true, 2),   /* 10: up, M128 x N256, 4 K blocks per step, 2 stages          */ \
    ND_VARIANT(DT, DTN, 2, 4, 1, 8, 9, 1, false, 2),  /* 11: M64 x N1024, 8 waves x (64x128), 2 stages: 1/3 less DMA per FLOP */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 8, 4, 1, false, 2),  /* 12: 2x2 stride-2 conv (training: data gradient of upN), M64 x N512 */ \
    ND_VARIANT(DT, DTN, 2, 2, 1, 4, 4, 1, false, 2),  /* 13: same, M64 x N256 (its input span is 4x the tile: wide rows)    */ \
    ND_VARIANT(DT, DTN, 2, 4, 2, 4, 9, 1, false, 2)   /* 14: M128 x N512, 8 waves x (64x128), 2 stages: fewest LDS-DMA bytes per MFMA (Cout >= 128) */
// (tried: M128 x N512 on 4 waves x (128x128), one wave per SIMD, for half the LDS fragment reads per MFMA in 16-bit storage: the
//  256 accumulator registers fill the AGPR file and hipcc spills accumulators to scratch inside the K loop -- 15x slower;
//  round 3: M128 x N256 on 4 waves x (64x128), one wave per SIMD with the accumulators in AGPRs (227 + 128 registers, no spill):
//  785 - 845 TFLOP/s against 1,110 - 1,155 for shape 14 on the 128 ... 1024-channel layers in bf16 -- a lone wave does not cover its
//  LDS latency with the one-group prefetch the compiler schedules; the same on M64 x N512 with three stages: 815 - 850)
constexpr int kGroup = 15;

