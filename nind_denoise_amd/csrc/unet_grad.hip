// UNet under autograd in eval mode (BatchNorm on its running statistics): the two halves torch.autograd calls.
//   forward   fold BatchNorm and pack on the device, in the forward role and in the transposed role, then the inference launch
//             sequence on whole tiles (every layer's output stays in its own buffer of the plan), final 1x1 + Sigmoid
//   backward  data gradients = the SAME conv kernel on the transposed-role blob (a padding-1 Conv2d(3): the transposed role on a
//             gradient buffer with a 1-pixel zero border; ConvTranspose2d(2, s=2): Conv 2x2 s2), weight gradients = k_wgrad (wgrad.hip),
//             pool backward = k_maxpool_bwd_add, exactly as utnet_train.hip does
// Small HBM-bound kernels below and in unet_grad_net.h: the folded weights, ReLU backward from the kept post-activation, the Sigmoid
// head and its adjoint, the first layer's data gradient to the 3 input channels, the adjoint of the BatchNorm fold.  No atomics, fixed
// summation order.
// Parameters and gradients: ONE flat fp32 buffer in nd_unet_tensor_name order, buffers (running statistics) included so that the
// fold reads one array; their gradient slots are never written.
#include "unet_grad_net.h"

// ------------------------------------------------------------------ kernels
// wf[co][k] = w[co][k] * scale[co]: the folded weights in the torch layout, one rounding per value (what the pack kernel's `scale`
// writes into the forward blob); both roles are packed from it, and the first layer's data gradient reads it as it is
__global__ void k_unet_fold_w(const float *__restrict__ w, const float *__restrict__ scale, int per_co, long n, float *__restrict__ wf) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) wf[i] = w[i] * scale[i / per_co];
}

// g (interior of a bordered gradient buffer, planes from the pointer) *= (a > 0), a = the layer's kept output (torch: ReLU'(0) = 0)
__global__ __launch_bounds__(256) void k_relu_bwd_post(f32x4 *__restrict__ g, long gnp, int gHb, int gWb, int gpad,
                                                       const f32x4 *__restrict__ a, long anp, int aHb, int aWb, int apad, int H, int W,
                                                       int B) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int y = blockIdx.y;
    const int b = blockIdx.z % B, q = blockIdx.z / B;
    if (x >= W) return;
    f32x4 *gp = g + (long)q * gnp + ((long)b * gHb + y + gpad) * gWb + x + gpad;
    const f32x4 av = a[(long)q * anp + ((long)b * aHb + y + apad) * aWb + x + apad];
    f32x4 gv = *gp;
#pragma unroll
    for (int e = 0; e < 4; ++e) gv[e] = av[e] > 0.f ? gv[e] : 0.f;
    *gp = gv;
}

// Adjoint of the BatchNorm fold  W' = W s,  b' = (b - mean) s + beta,  s = gamma / sqrt(var + 1e-5).  One workgroup per output
// channel; dw / db hold dW' / db' on entry and dW / db on return:
//     dW = dW' s     db = db' s     dbeta = db'     dgamma = (sum dW' W + db' (b - mean)) / sqrt(var + eps)
// (dgamma from dW', not from dW / s: right for gamma = 0 and gamma < 0).  The sum runs in double: it is a sum over pixels in disguise
// (sum g * conv output) and cancels as one.
__global__ __launch_bounds__(256) void k_bn_fold_bwd(int per_co, const float *__restrict__ w, const float *__restrict__ b,
                                                     const float *__restrict__ gamma, const float *__restrict__ mean,
                                                     const float *__restrict__ var, float *__restrict__ dw, float *__restrict__ db,
                                                     float *__restrict__ dgamma, float *__restrict__ dbeta) {
    __shared__ double red[256];
    const int co = blockIdx.x;
    const float inv = 1.f / sqrtf(var[co] + 1e-5f), sc = gamma[co] * inv;
    const float *wc = w + (long)co * per_co;
    float *dwc = dw + (long)co * per_co;
    double acc = 0.0;
    for (int k = threadIdx.x; k < per_co; k += 256) {
        const float d = dwc[k];
        acc += (double)d * (double)wc[k];
        dwc[k] = d * sc;
    }
    acc = nd_block_sum(acc, red);
    if (threadIdx.x != 0) return;
    const float dbp = db[co];
    dgamma[co] = (float)((acc + (double)dbp * ((double)b[co] - (double)mean[co])) * (double)inv);
    dbeta[co] = dbp;
    db[co] = dbp * sc;
}

namespace {

struct GradCtx {
    int B, H, W, flags;
    GradPlan t;
    UParams pl;
    Blob bl;
    GradBlob gb;
    float *blobs;
    hipStream_t s;
};
int grad_ctx(GradCtx &c, int flags, const float *params, void *blobs, int batch, int h, int w, void *ws, size_t ws_bytes, void *stream) {
    ND_TRY(nd_check_flags(flags, false, true));
    ND_TRY(check_grad(h, w, batch));
    if (!params || !blobs || !ws) ND_FAIL(ND_EINVAL, "UNet under autograd: null pointer");
    c.B = batch;
    c.H = h;
    c.W = w;
    c.flags = flags;
    c.t = make_grad_plan(h, w, batch, (char *)ws);
    if (ws_bytes < c.t.bytes) ND_FAIL(ND_ENOMEM, "UNet gradient workspace: %zu B given, %zu B needed", ws_bytes, c.t.bytes);
    c.pl = param_layout();
    c.bl = blob_layout();
    c.gb = grad_blob_layout();
    c.blobs = (float *)blobs;
    c.s = (hipStream_t)stream;
    return ND_OK;
}

}  // namespace

// ------------------------------------------------------------------ C ABI
extern "C" size_t nd_unet_param_count(void) { return param_layout().total; }
extern "C" int nd_unet_param_range(int tensor_idx, size_t *offset, size_t *count) {
    const UParams pl = param_layout();
    if (tensor_idx < 0 || tensor_idx >= (int)pl.off.size()) ND_FAIL(ND_EINVAL, "tensor index %d out of range", tensor_idx);
    if (offset) *offset = pl.off[tensor_idx];
    if (count) *count = pl.cnt[tensor_idx];
    return ND_OK;
}
extern "C" size_t nd_unet_grad_blob_bytes(void) { return grad_blob_layout().total * sizeof(float); }
extern "C" size_t nd_unet_grad_workspace_bytes(int h, int w, int batch) {
    if (check_grad(h, w, batch) != ND_OK) return 0;
    return make_grad_plan(h, w, batch, nullptr).bytes;
}
extern "C" int nd_unet_grad_workspace_init(void *ws, size_t ws_bytes, int h, int w, int batch, void *stream) {
    ND_TRY(check_grad(h, w, batch));
    const size_t need = make_grad_plan(h, w, batch, nullptr).bytes;
    if (!ws || ws_bytes < need) ND_FAIL(ND_ENOMEM, "UNet gradient workspace: %zu B given, %zu B needed", ws_bytes, need);
    ND_HIP(hipMemsetAsync(ws, 0, need, (hipStream_t)stream));   // zero borders of activations AND gradients, fix-up lines, slack
    return ND_OK;
}

extern "C" int nd_unet_grad_forward(int flags, const float *params, void *blobs, const float *x, float *y, int batch, int h, int w,
                                    void *ws, size_t ws_bytes, void *stream) {
    if (!x || !y) ND_FAIL(ND_EINVAL, "nd_unet_grad_forward: null pointer");
    GradCtx c;
    ND_TRY(grad_ctx(c, flags, params, blobs, batch, h, w, ws, ws_bytes, stream));
    hipStream_t s = c.s;
    const auto &L = layers();
    auto P = [&](const std::string &name) -> const float * { return params + c.pl.off[name_index(name)]; };
    float *fblob = c.blobs, *wfold = c.blobs + c.gb.wfold, *scale = c.blobs + c.gb.stage, *fbias = scale + kStageFloats / 2;
    for (size_t i = 0; i < L.size(); ++i) {
        const ULayer &l = L[i];
        const float *wt = P(l.key + ".weight"), *b = P(l.key + ".bias");
        float *dst = fblob + c.bl.off[i], *bdst = c.blobs + c.gb.boff[i];
        if (l.kind == ND_CONV1) {   // [3][cin] weights, 3 biases, zero up to a multiple of 4
            const size_t n = (size_t)3 * l.cin + 3, padded = (n + 3) / 4 * 4;
            ND_HIP(hipMemcpyAsync(dst, wt, sizeof(float) * 3 * l.cin, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemcpyAsync(dst + 3 * l.cin, b, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemsetAsync(dst + n, 0, sizeof(float) * (padded - n), s));
            continue;
        }
        if (l.bn.empty()) {   // up<n>.up; transposed role: cin' = cout, cout' = cin, no bias
            ND_TRY(nd_pack_layer_device(l.kind, l.cin, l.cout, ND_F32, wt, b, dst, s));
            ND_TRY(nd_pack_layer_device(ND_CONV2S2, l.cout, l.cin, ND_F32, wt, nullptr, bdst, s));
            continue;
        }
        if ((size_t)l.cout > kStageFloats / 2) ND_FAIL(ND_EINVAL, "nd_unet_grad_forward: no staging room for %s", l.key.c_str());
        ND_TRY(nd_launch_bn_fold(l.cout, b, P(l.bn + ".weight"), P(l.bn + ".bias"), P(l.bn + ".running_mean"), P(l.bn + ".running_var"),
                                 scale, fbias, s));
        const long n = (long)l.cin * l.cout * 9;
        float *wf = i == 0 ? c.blobs + c.gb.w0fold : wfold;
        hipLaunchKernelGGL(k_unet_fold_w, dim3(blocks_of(n)), dim3(256), 0, s, wt, (const float *)scale, l.cin * 9, n, wf);
        ND_HIP(hipGetLastError());
        ND_TRY(nd_pack_layer_device(ND_CONV3, l.cin, l.cout, ND_F32, wf, fbias, dst, s));
        if (i > 0) ND_TRY(nd_pack_layer_device(ND_CONVT3, l.cout, l.cin, ND_F32, wf, nullptr, bdst, s));
    }
    const UPlan &pl = c.t.fwd;
    const bool nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
    ND_TRY(nd_launch_nchw_to_qp(x, 3, pl.buf[XIN], 0, s));
    for (const UStep &st : kSteps) ND_TRY(run_step(st, pl, fblob, c.bl, nullptr, nosplit, s));
    const float *fw = fblob + c.bl.off[L.size() - 1];
    ND_TRY(nd_launch_final1x1(pl.buf[U4B], 64, fw, fw + 3 * 64, 0, c.t.sig, h, w, s, 1));
    const long n = (long)batch * 3 * h * w;
    hipLaunchKernelGGL(k_unet_head, dim3(blocks_of(n)), dim3(256), 0, s, (const float *)c.t.sig, x, n, (flags & ND_FLAG_FIND_NOISE) ? 1 : 0, y);
    ND_HIP(hipGetLastError());
    return ND_OK;
}

extern "C" int nd_unet_grad_backward(int flags, const float *params, float *grads, void *blobs, const float *gy, float *dx, int batch,
                                     int h, int w, void *ws, size_t ws_bytes, void *stream) {
    if (!gy) ND_FAIL(ND_EINVAL, "nd_unet_grad_backward: null pointer");
    if (!grads && !dx) ND_FAIL(ND_EINVAL, "nd_unet_grad_backward: neither parameter gradients nor the input gradient requested");
    GradCtx c;
    ND_TRY(grad_ctx(c, flags, params, blobs, batch, h, w, ws, ws_bytes, stream));
    hipStream_t s = c.s;
    GradPlan &t = c.t;
    const int B = batch;
    const auto &L = layers();
    const bool noise = (flags & ND_FLAG_FIND_NOISE) != 0;
    auto P = [&](const std::string &name) -> const float * { return params + c.pl.off[name_index(name)]; };
    auto G = [&](const std::string &name) -> float * { return grads + c.pl.off[name_index(name)]; };
    const float *fw = c.blobs + c.bl.off[L.size() - 1];
    // Sigmoid + final 1x1
    const long n = (long)B * 3 * h * w;
    hipLaunchKernelGGL(k_unet_head_bwd, dim3(blocks_of(n)), dim3(256), 0, s, gy, (const float *)t.sig, n, noise ? 1 : 0, t.gt);
    ND_HIP(hipGetLastError());
    if (grads) ND_TRY(nd_launch_final_wgrad(t.gt, h, w, t.fwd.buf[U4B], 64, 0, t.red, G("outc.conv.weight"), G("outc.conv.bias"), s));
    ND_TRY(nd_launch_final_bwd_data(t.gt, h, w, fw, 64, 1, t.g[U4B], s));
    for (int si = kNumSteps - 1; si >= 0; --si) {
        const UStep &st = kSteps[si];
        if (st.layer < 0) {
            // pool of the skip half (planes from 0) of a concat buffer: route g(pooled) back and ADD it to what the decoder's
            // first layer of this level wrote there (that launch came earlier in this loop: a fixed order)
            ND_TRY(nd_launch_maxpool_bwd_add(t.g[st.dst], t.fwd.buf[st.src], 0, t.g[st.src], 0, st.dst_plane0, s));
            continue;
        }
        const ULayer &l = L[st.layer];
        const QpBuf &in = t.fwd.buf[st.src];   // layer input (forward values)
        const QpBuf &go = t.g[st.dst];         // gradient of the layer's output buffer
        const int oplane0 = st.dst_plane0, oplanes = l.cout / 4;
        const int ih = in.Hb - 2 * in.pad, iw = in.Wb - 2 * in.pad;
        float *dw = grads ? G(l.key + ".weight") : nullptr, *db = grads ? G(l.key + ".bias") : nullptr;
        ConvDesc d;
        d.cin = l.cout;
        d.cout = l.cin;
        d.wpk = c.blobs + c.gb.boff[st.layer];
        d.out = t.g[st.src];
        d.part = t.fwd.split;
        d.part_bytes = kSplitScratchBytes;
        d.nosplit = (flags & ND_FLAG_NO_SPLITK) != 0;
        if (l.kind == ND_CONVT2S2) {
            // adjoint of the F.pad fix-up: only rows / columns [0, 2 h_in) x [0, 2 w_in) of the up half came from this layer
            const QpBuf &gu = t.gup[up_index(st.layer)];
            ND_TRY(nd_launch_repitch(go, oplane0, oplanes, 1, 0, 0, gu, 0, 0, 2 * ih, 2 * iw, s));
            if (grads) {
                ND_TRY(nd_launch_channel_sum(gu, 0, l.cout, db, t.red, s));
                for (int ab = 0; ab < 4; ++ab) {   // four 1-tap problems on the input grid
                    QpBuf bq = scratch_view(t, oplanes, B, ih, iw);
                    ND_TRY(nd_launch_repitch(gu, 0, oplanes, 2, ab >> 1, ab & 1, bq, 0, 0, ih, iw, s));
                    ND_TRY(nd_launch_wgrad(in, 0, l.cin, bq, 0, l.cout, 1, 4, ab, t.partial, t.partial_floats, dw, s));
                }
            }
            d.kind = ND_CONV2S2;
            d.bias = d.wpk + nd_bias_offset(ND_CONV2S2, l.cout, l.cin);
            d.in = gu;
            ND_TRY(nd_launch_conv(d, s));
            continue;
        }
        // ReLU backward in place, from the kept output
        {
            const QpBuf &a = t.fwd.buf[st.dst];
            const int oh = go.Hb - 2, ow = go.Wb - 2;
            hipLaunchKernelGGL(k_relu_bwd_post, dim3((ow + 255) / 256, oh, B * oplanes), dim3(256), 0, s,
                               (f32x4 *)go.base + (long)oplane0 * go.np(), go.np(), go.Hb, go.Wb, go.pad,
                               (const f32x4 *)a.base + (long)oplane0 * a.np(), a.np(), a.Hb, a.Wb, a.pad, oh, ow, B);
            ND_HIP(hipGetLastError());
            if (grads) {   // db', dW' of the folded layer, then the adjoint of the fold in place
                ND_TRY(nd_launch_channel_sum(go, oplane0, l.cout, db, t.red, s));
                QpBuf a2 = scratch_view(t, oplanes, B, in.Hb, in.Wb);
                ND_TRY(nd_launch_repitch(go, oplane0, oplanes, 1, 0, 0, a2, 0, 0, oh, ow, s));
                ND_TRY(nd_launch_wgrad(a2, 0, l.cout, in, 0, l.cin, 9, 9, 0, t.partial, t.partial_floats, dw, s));
                hipLaunchKernelGGL(k_bn_fold_bwd, dim3(l.cout), dim3(256), 0, s, l.cin * 9, P(l.key + ".weight"), P(l.key + ".bias"),
                                   P(l.bn + ".weight"), P(l.bn + ".running_mean"), P(l.bn + ".running_var"), dw, db,
                                   G(l.bn + ".weight"), G(l.bn + ".bias"));
                ND_HIP(hipGetLastError());
            }
        }
        if (st.layer > 0) {   // data gradient: the transposed role on the gradient buffer's 1-pixel zero border
            d.kind = ND_CONVT3;
            d.bias = d.wpk + nd_bias_offset(ND_CONVT3, l.cout, l.cin);
            d.in = go;
            d.in_plane0 = oplane0;
            ND_TRY(nd_launch_conv(d, s));
        } else if (dx) {
            dim3 grid((unsigned)((w + 15) / 16), (unsigned)((h + 3) / 4), B);
            hipLaunchKernelGGL(k_unet_input_grad, grid, dim3(64 * kUigGroups), 0, s, (const f32x4 *)go.base, go.np(), go.Hb, go.Wb, oplanes,
                               (const float *)(c.blobs + c.gb.w0fold), h, w, noise ? gy : (const float *)nullptr, dx);
            ND_HIP(hipGetLastError());
        }
    }
    return ND_OK;
}
