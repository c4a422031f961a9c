// Host-side launch code shared by the kernel families: per-device launch state, the buffer checks of a conv layer, the ConvParams
// setup of the implicit-GEMM kernels (conv_qp, conv_w1d, conv_w2d), their persistent-grid / split-K schedule and the stamped
// diagnostic launch.  A kernel family supplies its geometry, its LDS size and its kernel pointer.  No device code.
#include <atomic>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "conv_qp.inc"

// ------------------------------------------------------------------ per-device launch state
namespace {
constexpr int kMaxDevices = 16;
std::atomic<int> g_cus[kMaxDevices];   // CU count per device (0: not queried yet); two threads that both miss store the same value
// per device, per key (a kernel, or a once-per-device initialiser): a value that only grows, read and raised under g_mu
std::mutex g_mu;
std::unordered_map<const void *, int> g_state[kMaxDevices];
}  // namespace

int nd_device(int *dev, int *ncus) {
    ND_HIP(hipGetDevice(dev));
    if (*dev < 0 || *dev >= kMaxDevices) ND_FAIL(ND_EINVAL, "device index %d outside [0, %d)", *dev, kMaxDevices);
    if (!ncus) return ND_OK;
    int n = g_cus[*dev].load(std::memory_order_relaxed);
    if (!n) {
        hipDeviceProp_t prop;
        ND_HIP(hipGetDeviceProperties(&prop, *dev));
        n = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
        g_cus[*dev].store(n, std::memory_order_relaxed);
    }
    *ncus = n;
    return ND_OK;
}

int nd_raise_lds(int dev, const void *fn, size_t bytes) {
    std::lock_guard<std::mutex> lock(g_mu);
    int &limit = g_state[dev][fn];
    if ((int)bytes <= limit) return ND_OK;
    ND_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    limit = (int)bytes;
    return ND_OK;
}

int nd_once_per_device(int dev, int (*init)()) {
    std::lock_guard<std::mutex> lock(g_mu);
    int &done = g_state[dev][(const void *)init];
    if (done) return ND_OK;
    ND_TRY(init());
    done = 1;
    return ND_OK;
}

// ------------------------------------------------------------------ checks of a conv layer
int nd_check_in_planes(const char *who, const ConvDesc &d, int KB, bool takes_in2, bool takes_add) {
    if (d.in.planes < d.in_plane0 + 2 * KB) ND_FAIL(ND_EINVAL, "%s: input buffer has %d planes, needs %d", who, d.in.planes, d.in_plane0 + 2 * KB);
    if (d.in2.base && !takes_in2) ND_FAIL(ND_EINVAL, "%s: this kernel form has no second input source", who);
    if ((d.add.base || d.w_kb) && !takes_add) ND_FAIL(ND_EINVAL, "%s: this kernel form takes no addend source and no K-block sub-range", who);
    if (d.w_kb && (d.w_kb0 < 0 || d.w_kb0 + KB > d.w_kb))
        ND_FAIL(ND_EINVAL, "%s: K blocks [%d,+%d) outside the %d of the packed weights", who, d.w_kb0, KB, d.w_kb);
    return ND_OK;
}

int nd_check_add(const char *who, const ConvDesc &d, long reach) {
    const QpBuf &q = d.add;
    const int n = d.cout / 4;   // planes read
    if (q.dt != ND_F32 || d.out.dt != ND_F32 || !d.add_origin || d.add_plane0 < 0 || d.add_plane0 + n > q.planes || d.add_origin_max < 0 ||
        reach <= 0)
        ND_FAIL(ND_EINVAL, "%s: addend source: planes [%d,+%d) of %d", who, d.add_plane0, n, q.planes);
    // the last plane read ends where the buffer's slack ends; every other plane is followed by a plane
    const long last = d.add_origin_max + reach, room = (long)(q.planes - d.add_plane0 - n + 1) * q.np() + (long)nd_buf_slack(q.Wb);
    if (last > room) ND_FAIL(ND_EINVAL, "%s: addend source: a launch reaches element %ld of a plane, the buffer ends at %ld", who, last, room);
    if (last * 16 >= (1L << 32)) ND_FAIL(ND_EINVAL, "%s: addend source too large for 32-bit byte offsets", who);
    return ND_OK;
}

int nd_check_in2(const char *who, const ConvDesc &d, int KB, long reach) {
    const QpBuf &q = d.in2;
    const int n2 = 2 * KB - d.in2_from;   // planes read from the second source
    if (q.dt != ND_F32 || d.in.dt != ND_F32 || !d.in2_origin || d.in2_from <= 0 || (d.in2_from & 1) || n2 <= 0 || d.in2_plane0 < 0 ||
        d.in2_plane0 + n2 > q.planes || d.in2_origin_max < 0 || reach <= 0)
        ND_FAIL(ND_EINVAL, "%s: second input source: planes [%d,+%d) of %d from input plane %d of %d", who, d.in2_plane0, n2, q.planes,
                d.in2_from, 2 * KB);
    // the last plane read ends where the buffer's slack ends; every other plane is followed by a plane
    const long last = d.in2_origin_max + reach, room = (long)(q.planes - d.in2_plane0 - n2 + 1) * q.np() + (long)nd_buf_slack(q.Wb);
    if (last > room) ND_FAIL(ND_EINVAL, "%s: second input source: a launch reaches element %ld of a plane, the buffer ends at %ld", who, last, room);
    if ((2 * q.np() + last) * 16 + 65536 >= (1L << 32)) ND_FAIL(ND_EINVAL, "%s: second input source too large for 32-bit byte offsets", who);
    return ND_OK;
}

int nd_check_out(const char *who, const ConvDesc &d, int oh, int ow, bool at_least) {
    const int Hb = oh + 2 * d.out.pad, Wb = ow + 2 * d.out.pad;
    const bool fits = at_least ? (d.out.Hb >= Hb && d.out.Wb >= Wb) : (d.out.Hb == Hb && d.out.Wb == Wb);
    if (!fits || d.out.B != d.in.B)
        ND_FAIL(ND_EINVAL, "%s: destination %dx%dx%d(pad %d) does not fit result %dx%dx%d", who, d.out.B, d.out.Hb, d.out.Wb, d.out.pad,
                d.in.B, oh, ow);
    if (d.out_plane0 + d.cout / nd_cpp(d.out.dt) > d.out.planes) ND_FAIL(ND_EINVAL, "%s: destination planes overflow", who);
    return ND_OK;
}

int nd_check_int32(const char *who, const QpBuf &in) {
    if (in.used() >= (1L << 31)) ND_FAIL(ND_EINVAL, "%s: %ld linear pixels exceed the int32 index range", who, in.used());
    return ND_OK;
}

int nd_check_roi(const char *who, const ConvDesc &d, int Hv, int Wv, bool refused, const char *why) {
    if (d.roi_rows <= 0) return ND_OK;
    if (refused || d.roi_r0 < 0 || d.roi_c0 < 0 || d.roi_cols < 1 || d.roi_r0 + d.roi_rows > Hv || d.roi_c0 + d.roi_cols > Wv)
        ND_FAIL(ND_EINVAL, "%s: region [%d,+%d) x [%d,+%d) outside the %d x %d grid (or %s)", who, d.roi_r0, d.roi_rows, d.roi_c0,
                d.roi_cols, Hv, Wv, why);
    return ND_OK;
}

// ------------------------------------------------------------------ ConvParams
ConvParams nd_conv_params(const ConvDesc &d, int KB, int M) {
    ConvParams p = {};
    p.in = (const f32x4 *)d.in.base + (long)d.in_plane0 * d.in.np();
    p.wpk = d.wpk;
    p.bias = d.bias;
    p.out = (f32x4 *)d.out.base;
    p.in_plane = d.in.np();
    p.out_plane = d.out.np();
    p.nimg = d.in.B;
    p.P = d.in.Hb * d.in.Wb;
    p.Wb = d.in.Wb;
    p.pre = (f32x4 *)d.pre;
    p.pre_plane = d.pre_plane;
    p.KB = KB;
    p.KBw = KB;
    p.M = M;
    p.cout = d.cout;
    p.Po = d.out.Hb * d.out.Wb;
    p.Wo = d.out.Wb;
    p.opad = d.out.pad;
    p.out_plane0 = d.out_plane0;
    p.act = d.act;
    p.slope = d.slope;
    p.slope_dev = d.slope_dev;
    return p;
}

int nd_conv_pool(const char *who, const ConvDesc &d, int Hv, int Wv, ConvParams &p) {
    const QpBuf &q = *d.pool;
    if (q.dt != d.in.dt || q.B != d.in.B || q.Hb - 2 * q.pad != Hv / 2 || q.Wb - 2 * q.pad != Wv / 2 || q.planes < d.cout / nd_cpp(d.in.dt))
        ND_FAIL(ND_EINVAL, "%s: pooled destination does not fit %d x %d x %d", who, d.cout, Hv / 2, Wv / 2);
    p.pool = (f32x4 *)q.base;
    p.pool_plane = q.np();
    p.pool_P = q.Hb * q.Wb;
    p.pool_W = q.Wb;
    p.pool_pad = q.pad;
    return ND_OK;
}

void nd_conv_tiles(ConvParams &p, bool cross, int nblk, int mblk) {
    if (cross) {
        p.tpi = 0;
        p.n_tiles_n = (int)(((long)p.nimg * p.PV + nblk - 1) / nblk);
    } else {
        p.tpi = (p.PV + nblk - 1) / nblk;
        p.n_tiles_n = p.tpi * p.nimg;
    }
    p.n_tiles_m = (p.M + mblk - 1) / mblk;
    p.tiles_per_problem = p.n_tiles_n * p.n_tiles_m;
}

// ------------------------------------------------------------------ split-K tail
// Persistent workgroups finish whole rounds of tiles at full rate, but the last, partial round leaves CUs idle (and a layer with
// fewer tiles than CUs -- the deep levels of a small batch -- is nothing but a partial round).  The tiles of that round are
// therefore cut along K into S slices that fill the idle CUs; slices store raw accumulators and the family's finish kernel adds
// them in slice order (deterministic), then applies bias / activation exactly like the conv epilogue.
// Time of a launch in units of "one workgroup runs one K chunk": `slots` workgroups run concurrently, `ntiles` tiles of `nchunks`
// chunks each.  Picks the split of the partial round (S slices of cps chunks) that minimises it; kSplitOver chunks of fixed cost
// per work item (pipeline prologue, epilogue / partial store + its share of the finish kernel).
namespace {
constexpr double kSplitOver = 3.0;
struct SplitPlan { int first, S, cps; double time; };
SplitPlan plan_split(long ntiles, int nchunks, long slots, long max_items) {
    SplitPlan b;
    const long full = ntiles / slots * slots, R = ntiles - full;
    b.first = (int)ntiles;
    b.S = 1;
    b.cps = nchunks;
    b.time = (double)((ntiles + slots - 1) / slots) * (nchunks + kSplitOver);
    if (R == 0 || max_items <= 0) return b;
    const double base = (double)(full / slots) * (nchunks + kSplitOver);
    for (int S = 2; S <= nchunks && S <= 64; ++S) {
        const int cps = (nchunks + S - 1) / S, Se = (nchunks + cps - 1) / cps;
        if (R * Se > max_items) break;
        const double t = base + (double)((R * Se + slots - 1) / slots) * (cps + 1.5 * kSplitOver);
        if (t < 0.93 * b.time) {
            b.first = (int)full;
            b.S = Se;
            b.cps = cps;
            b.time = t;
        }
    }
    return b;
}
}  // namespace

double nd_conv_schedule_time(long ntiles, int nchunks, long slots, long cap) { return plan_split(ntiles, nchunks, slots, cap).time; }

long nd_conv_schedule(ConvParams &p, long ntiles, int nchunks, long slots, long cap) {
    const SplitPlan sp = plan_split(ntiles, nchunks, slots, cap);
    p.split_first = sp.first;
    p.S = sp.S;
    p.cps = sp.cps;
    p.nitems = (int)(sp.first + (ntiles - sp.first) * sp.S);
    return p.nitems < slots ? p.nitems : slots;
}

#ifdef ND_QP_STAMPS
// ------------------------------------------------------------------ stamped diagnostic launch (make STAMPS=1)
int nd_stamped_launch(void (*fn)(ConvParams), int threads, size_t lds, ConvParams p, long ntiles, int nchunks, long slots, hipStream_t s,
                      bool print, const char *header, const char *wave_prefix, const char *const *names, int nphases, std::initializer_list<int> waves) {
    static unsigned long long *buf = nullptr;
    static size_t buf_n = 0;
    const size_t n = (size_t)slots * 8 * 8;   // [workgroup][wave][phases, -, steps]
    if (n > buf_n) {
        if (buf) ND_HIP(hipFree(buf));
        buf = nullptr;
        ND_HIP(hipMalloc(&buf, n * 8));
        buf_n = n;
    }
    ND_HIP(hipMemsetAsync(buf, 0, n * 8, s));
    p.split_first = (int)ntiles;
    p.S = 1;
    p.cps = nchunks;
    p.nitems = (int)ntiles;
    p.part = (f32x4 *)buf;
    const long g2 = ntiles < slots ? ntiles : slots;
    hipLaunchKernelGGL(fn, dim3((unsigned)g2), dim3(threads), lds, s, p);
    ND_HIP(hipStreamSynchronize(s));
    if (!print) return ND_OK;
    std::vector<unsigned long long> h(n);
    ND_HIP(hipMemcpy(h.data(), buf, n * 8, hipMemcpyDeviceToHost));
    if (header) fprintf(stderr, "%s\n", header);
    for (int w : waves) {
        double tot[8] = {0}, steps = 0;
        for (long b = 0; b < g2; ++b) {
            for (int k = 0; k < nphases; ++k) tot[k] += (double)h[((size_t)b * 8 + w) * 8 + k];
            steps += (double)h[((size_t)b * 8 + w) * 8 + 6];
        }
        double sum = 0;
        for (int k = 0; k < nphases; ++k) sum += tot[k];
        fprintf(stderr, "%s %d: %.0f cycles/step:", wave_prefix, w, sum / steps);
        for (int k = 0; k < nphases; ++k) fprintf(stderr, "  %s %.0f (%.1f%%)", names[k], tot[k] / steps, 100 * tot[k] / sum);
        fprintf(stderr, "\n");
    }
    return ND_OK;
}
#endif
