// UNet executor (reference: networks/ThirdPartyNets.py:62-169, eval mode) on the same quad-planar conv kernel:
//   Conv2d(3, padding=1)  -> valid 3x3 correlation on a buffer with a 1-pixel zero border
//   BatchNorm2d (eval)    -> folded into the conv weights / bias at pack time (running stats, eps 1e-5)
//   ReLU                  -> the PReLU epilogue with slope 0
//   cat([skip, up])       -> zero-copy: skip FIRST, up-sampled second (the opposite of UtNet; ThirdPartyNets.py:124)
//   F.pad fix-up (:110-118) for odd sizes -> the 2x2 stride-2 result is written at offset 0 of a destination that is one
//                                            row / column larger; the remainder stays zero (never written)
//   outc + Sigmoid        -> k_final1x1 with the sigmoid flag
// ND_FLAG_UNET_WINOGRAD (opt-in: UNet(winograd=True)) runs the 3x3 layers in the Winograd forms of kWinoPlan (unet_net.h): the fused
// F(4,3) and the three-pass F(6x6,3x3) kernels UtNet runs, on Winograd blobs behind the default ones and V / M scratch behind the
// default workspace.  Without the flag every launch, blob byte and workspace byte is the default path's: the *_flags entry points
// with flags = 0 are the plain ones.
// Frames (denoise_image.py:240-267) run through nd_unet_denoise_frame: gather straight into the first layer's input, the same step
// list with the decoder restricted to what the kept centre of a tile depends on (plan_rois), final 1x1 + Sigmoid fused into the stitch.
#include "unet_net.h"

extern "C" int nd_unet_num_tensors(void) { return (int)names().size(); }
extern "C" const char *nd_unet_tensor_name(int i) {
    return (i >= 0 && i < (int)names().size()) ? names()[i].c_str() : nullptr;
}
extern "C" size_t nd_unet_packed_bytes_flags(int dtype, int flags) {
    if (dtype != ND_F32 || nd_check_flags(flags, false, true, true) != ND_OK) return 0;
    return blob_layout(flags).total * sizeof(float);
}
extern "C" size_t nd_unet_packed_bytes(int dtype) { return nd_unet_packed_bytes_flags(dtype, 0); }

extern "C" int nd_unet_pack_weights_flags(int dtype, int flags, const float *const *tensors, int n_tensors, void *packed_host,
                                          size_t packed_bytes) {
    ND_TRY(nd_check_flags(flags, false, true, true));
    if (dtype != ND_F32) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: unsupported dtype %d", dtype);
    if (n_tensors != nd_unet_num_tensors()) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: expected %d tensors", nd_unet_num_tensors());
    const Blob bl = blob_layout(flags);
    if (packed_bytes < bl.total * sizeof(float)) ND_FAIL(ND_ENOMEM, "nd_unet_pack_weights: packed buffer too small");
    float *blob = (float *)packed_host;
    memset(blob, 0, bl.total * sizeof(float));
    const auto &L = layers();
    for (size_t i = 0; i < L.size(); ++i) {
        const ULayer &l = L[i];
        const float *w = tensors[name_index(l.key + ".weight")], *b = tensors[name_index(l.key + ".bias")];
        if (!w || !b) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: missing %s", l.key.c_str());
        if (l.kind == ND_CONV1) {
            memcpy(blob + bl.off[i], w, sizeof(float) * 3 * l.cin);
            memcpy(blob + bl.off[i] + 3 * l.cin, b, sizeof(float) * 3);
            continue;
        }
        if (l.bn.empty()) {
            nd_pack_layer(l.kind, l.cin, l.cout, ND_F32, w, b, blob + bl.off[i]);
            continue;
        }
        // fold eval-mode BatchNorm2d: y = (conv + b - mean) * gamma / sqrt(var + eps) + beta
        const float *g = tensors[name_index(l.bn + ".weight")], *be = tensors[name_index(l.bn + ".bias")];
        const float *rm = tensors[name_index(l.bn + ".running_mean")], *rv = tensors[name_index(l.bn + ".running_var")];
        if (!g || !be || !rm || !rv) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights: missing BatchNorm tensors of %s", l.bn.c_str());
        std::vector<float> wf((size_t)l.cout * l.cin * 9), bf(l.cout);
        for (int co = 0; co < l.cout; ++co) {
            const float sc = g[co] / sqrtf(rv[co] + 1e-5f);
            for (int k = 0; k < l.cin * 9; ++k) wf[(size_t)co * l.cin * 9 + k] = w[(size_t)co * l.cin * 9 + k] * sc;
            bf[co] = (b[co] - rm[co]) * sc + be[co];
        }
        nd_pack_layer(l.kind, l.cin, l.cout, ND_F32, wf.data(), bf.data(), blob + bl.off[i]);
        // the layer's Winograd form, from the folded weights (every planned layer has a BatchNorm)
        if (bl.woff[i] && kWinoPlan[i] == UFORM_WINO3P) ND_TRY(nd_wino_pack(kWinoTile, l.kind, l.cin, l.cout, wf.data(), bf.data(), blob + bl.woff[i]));
        if (bl.woff[i] && kWinoPlan[i] == UFORM_F43) ND_TRY(nd_w1d_pack(kW1dTile, l.kind, l.cin, l.cout, wf.data(), bf.data(), blob + bl.woff[i]));
    }
    return ND_OK;
}
extern "C" int nd_unet_pack_weights(int dtype, const float *const *tensors, int n_tensors, void *packed_host, size_t packed_bytes) {
    return nd_unet_pack_weights_flags(dtype, 0, tensors, n_tensors, packed_host, packed_bytes);
}

// The same blob from tensors in HBM.  A BatchNorm layer: k_bn_fold writes the per-channel scale and the folded bias, the pack kernel
// multiplies the scale in while it writes the fragments.  The 2 * cout staged floats live in the NEXT layer's region of the blob: layers
// are packed in ascending order on one stream and every pack writes every word of its region, so the staging is overwritten by the
// region's own values before the call's work ends (no allocation, no state shared between calls).  With ND_FLAG_UNET_WINOGRAD the
// layer's Winograd form is packed from the same scale and folded bias before the next layer overwrites them, with the transform in
// double as the host packers evaluate it: the host blob's bytes.
extern "C" int nd_unet_pack_weights_device_flags(int dtype, int flags, const float *const *tensors, int n_tensors, void *packed_dev,
                                                 size_t packed_bytes, void *stream) {
    ND_TRY(nd_check_flags(flags, false, true, true));
    if (dtype != ND_F32) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: unsupported dtype %d", dtype);
    if (!tensors || n_tensors != nd_unet_num_tensors())
        ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: expected %d tensors", nd_unet_num_tensors());
    const Blob bl = blob_layout(flags);
    if (!packed_dev || packed_bytes < bl.total * sizeof(float)) ND_FAIL(ND_ENOMEM, "nd_unet_pack_weights_device: packed buffer too small");
    float *blob = (float *)packed_dev;
    hipStream_t s = (hipStream_t)stream;
    const auto &L = layers();
    for (size_t i = 0; i < L.size(); ++i) {
        const ULayer &l = L[i];
        const float *w = tensors[name_index(l.key + ".weight")], *b = tensors[name_index(l.key + ".bias")];
        if (!w || !b) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: missing %s", l.key.c_str());
        if (l.kind == ND_CONV1) {   // [3][cin] weights, 3 biases, zero up to a multiple of 4
            const size_t n = (size_t)3 * l.cin + 3, padded = (n + 3) / 4 * 4;
            ND_HIP(hipMemcpyAsync(blob + bl.off[i], w, sizeof(float) * 3 * l.cin, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemcpyAsync(blob + bl.off[i] + 3 * l.cin, b, sizeof(float) * 3, hipMemcpyDeviceToDevice, s));
            ND_HIP(hipMemsetAsync(blob + bl.off[i] + n, 0, sizeof(float) * (padded - n), s));
            continue;
        }
        if (l.bn.empty()) {
            ND_TRY(nd_pack_layer_device(l.kind, l.cin, l.cout, ND_F32, w, b, blob + bl.off[i], s));
            continue;
        }
        const float *g = tensors[name_index(l.bn + ".weight")], *be = tensors[name_index(l.bn + ".bias")];
        const float *rm = tensors[name_index(l.bn + ".running_mean")], *rv = tensors[name_index(l.bn + ".running_var")];
        if (!g || !be || !rm || !rv) ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: missing BatchNorm tensors of %s", l.bn.c_str());
        const size_t next_end = i + 2 < L.size() ? bl.off[i + 2] : bl.total;
        if (i + 1 >= L.size() || next_end - bl.off[i + 1] < (size_t)2 * l.cout)
            ND_FAIL(ND_EINVAL, "nd_unet_pack_weights_device: no staging room behind %s", l.key.c_str());
        float *scale = blob + bl.off[i + 1], *fbias = scale + l.cout;
        ND_TRY(nd_launch_bn_fold(l.cout, b, g, be, rm, rv, scale, fbias, s));
        ND_TRY(nd_pack_layer_device(l.kind, l.cin, l.cout, ND_F32, w, fbias, blob + bl.off[i], s, scale));
        if (bl.woff[i] && kWinoPlan[i] == UFORM_WINO3P)
            ND_TRY(nd_pack_wino_device(kWinoTile, l.kind, l.cin, l.cout, w, fbias, blob + bl.woff[i], s, scale, true));
        if (bl.woff[i] && kWinoPlan[i] == UFORM_F43)
            ND_TRY(nd_pack_w1d_device(kW1dTile, l.kind, l.cin, l.cout, w, fbias, blob + bl.woff[i], s, scale, true));
    }
    // (the regions are rounded up to 64 floats: the packers leave the few floats behind a form unwritten, the host blob holds zeros)
    if (flags & ND_FLAG_UNET_WINOGRAD)
        for (size_t i = 0; i < L.size(); ++i) {
            if (!bl.woff[i]) continue;
            const size_t used = kWinoPlan[i] == UFORM_WINO3P ? nd_wino_packed_floats(kWinoTile, L[i].cin, L[i].cout)
                                                             : nd_w1d_packed_floats(kW1dTile, L[i].cin, L[i].cout);
            const size_t end = (used + 63) / 64 * 64;
            if (end > used) ND_HIP(hipMemsetAsync(blob + bl.woff[i] + used, 0, (end - used) * sizeof(float), s));
        }
    return ND_OK;
}
extern "C" int nd_unet_pack_weights_device(int dtype, const float *const *tensors, int n_tensors, void *packed_dev, size_t packed_bytes,
                                           void *stream) {
    return nd_unet_pack_weights_device_flags(dtype, 0, tensors, n_tensors, packed_dev, packed_bytes, stream);
}

extern "C" size_t nd_unet_workspace_bytes_flags(int h, int w, int batch, int dtype, int flags) {
    if (check(h, w, batch, dtype) != ND_OK || nd_check_flags(flags, false, true, true) != ND_OK) return 0;
    return make_plan(h, w, batch, nullptr, 0, flags).bytes;
}
extern "C" size_t nd_unet_workspace_bytes(int h, int w, int batch, int dtype) { return nd_unet_workspace_bytes_flags(h, w, batch, dtype, 0); }

extern "C" int nd_unet_workspace_init_flags(void *ws, size_t ws_bytes, int h, int w, int batch, int dtype, int flags, void *stream) {
    ND_TRY(check(h, w, batch, dtype));
    ND_TRY(nd_check_flags(flags, false, true, true));
    const size_t need = make_plan(h, w, batch, nullptr, 0, flags).bytes;
    if (!ws || ws_bytes < need) ND_FAIL(ND_ENOMEM, "UNet workspace: %zu B given, %zu B needed", ws_bytes, need);
    ND_HIP(hipMemsetAsync(ws, 0, need, (hipStream_t)stream));
    return ND_OK;
}
extern "C" int nd_unet_workspace_init(void *ws, size_t ws_bytes, int h, int w, int batch, int dtype, void *stream) {
    return nd_unet_workspace_init_flags(ws, ws_bytes, h, w, batch, dtype, 0, stream);
}

// UNet.forward (ThirdPartyNets.py:153-169, find_noise handled by the caller): x [B,3,H,W] -> sigmoid(outc(...)) [B,3,H,W]
extern "C" int nd_unet_forward_flags(int dtype, int flags, const void *packed, const float *x, float *y, int batch, int h, int w, void *ws,
                                     size_t ws_bytes, void *stream) {
    ND_TRY(nd_check_flags(flags, false, false, true));
    ND_TRY(check(h, w, batch, dtype));
    if (!packed || !x || !y || !ws) ND_FAIL(ND_EINVAL, "UNet: null pointer");
    UPlan pl = make_plan(h, w, batch, (char *)ws, 0, flags);
    if (ws_bytes < pl.bytes) ND_FAIL(ND_ENOMEM, "UNet workspace: %zu B given, %zu B needed", ws_bytes, pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    const float *blob = (const float *)packed;
    const Blob bl = blob_layout(flags);
    const auto &L = layers();
    ND_TRY(nd_launch_nchw_to_qp(x, 3, pl.buf[XIN], 0, s));
    for (const UStep &st : kSteps) ND_TRY(run_step(st, pl, blob, bl, nullptr, flags, s));
    const float *fw = blob + bl.off[L.size() - 1];
    ND_TRY(nd_launch_final1x1(pl.buf[U4B], 64, fw, fw + 3 * 64, 0, y, h, w, s, 1));
    return ND_OK;
}
extern "C" int nd_unet_forward(int dtype, const void *packed, const float *x, float *y, int batch, int h, int w, void *ws,
                               size_t ws_bytes, void *stream) {
    return nd_unet_forward_flags(dtype, 0, packed, x, y, batch, h, w, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------ useful-region plan (host only)
extern "C" int nd_unet_num_steps(void) { return kNumSteps; }
extern "C" const char *nd_unet_step_name(int i) {
    if (i < 0 || i >= kNumSteps) return nullptr;
    return kSteps[i].layer < 0 ? "pool" : layers()[kSteps[i].layer].key.c_str();
}
extern "C" int nd_unet_useful_region(int cs, int crop, int step, int *rect) {
    if (cs < 16 || crop < 0 || 2 * crop >= cs || step < 0 || step >= kNumSteps || !rect)
        ND_FAIL(ND_EINVAL, "nd_unet_useful_region: cs %d, crop %d, step %d", cs, crop, step);
    Roi rois[kNumSteps];
    const int n = plan_rois(make_plan(cs, cs, 1, nullptr), crop, crop, rois);
    rect[0] = rois[step].r0;
    rect[1] = rois[step].c0;
    rect[2] = rois[step].rows;
    rect[3] = rois[step].cols;
    return n;
}
// the `form` code of nd_step_profile that step `step` of a whole forward of batch x 3 x h x w runs in under `flags`; no GPU call.
// A bad argument: ND_EINVAL - 100 (-1 is the code of a pool)
extern "C" int nd_unet_step_form(int flags, int batch, int h, int w, int step) {
    if (nd_check_flags(flags, false, true, true) != ND_OK || check(h, w, batch, ND_F32) != ND_OK) return ND_EINVAL - 100;
    if (step < 0 || step >= kNumSteps) ND_FAIL(ND_EINVAL - 100, "nd_unet_step_form: step %d", step);
    return (int)step_form(kSteps[step], make_plan(h, w, batch, nullptr, 0, flags), flags, nullptr);
}

// ------------------------------------------------------------------ per-step profile (the UNet twin of nd_utnet_profile_stack)
// One pass of the conv stack on whatever the workspace holds, with an event between the steps (and around the GEMM launch of a
// three-pass layer); crop > 0: the decoder restricted as nd_unet_denoise_frame restricts it.  Synchronises the stream.
namespace {
struct StepEvents {
    hipEvent_t ev[3 * kNumSteps + 1];
    int n = 0;
    int create() {
        for (; n < 3 * kNumSteps + 1; ++n) ND_HIP(hipEventCreate(&ev[n]));
        return ND_OK;
    }
    ~StepEvents() {
        for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]);
    }
};
}  // namespace
extern "C" int nd_unet_profile_stack(int flags, const void *packed, int batch, int cs, int crop, void *ws, size_t ws_bytes, void *stream,
                                     nd_step_profile *steps, int max_steps) {
    ND_TRY(nd_check_flags(flags, false, true, true));
    ND_TRY(check(cs, cs, batch, ND_F32));
    if (!packed || !ws) ND_FAIL(ND_EINVAL, "UNet: null pointer");
    if (max_steps < kNumSteps || !steps) ND_FAIL(ND_EINVAL, "nd_unet_profile_stack: need room for %d steps", kNumSteps);
    if (crop < 0 || 2 * crop >= cs) ND_FAIL(ND_EINVAL, "nd_unet_profile_stack: crop %d", crop);
    const UPlan pl = make_plan(cs, cs, batch, (char *)ws, 0, flags);
    if (ws_bytes < pl.bytes) ND_FAIL(ND_ENOMEM, "UNet workspace: %zu B given, %zu B needed", ws_bytes, pl.bytes);
    hipStream_t s = (hipStream_t)stream;
    const float *blob = (const float *)packed;
    const Blob bl = blob_layout(flags);
    StepEvents evs;
    ND_TRY(evs.create());
    hipEvent_t *const ev = evs.ev, *const evx = evs.ev + kNumSteps + 1;
    Roi rois[kNumSteps];
    const bool useful = crop > 0 && !(flags & ND_FLAG_FULL_TILES) && plan_rois(pl, crop, crop, rois) > 0 && rois_fit(pl, blob, bl, rois, flags);
    long tiles_run[kNumSteps] = {};
    for (int i = 0; i < kNumSteps; ++i) {
        ND_HIP(hipEventRecord(ev[i], s));
        ND_TRY(run_step(kSteps[i], pl, blob, bl, useful ? &rois[i] : nullptr, flags, s, evx + 2 * i, &tiles_run[i]));
    }
    ND_HIP(hipEventRecord(ev[kNumSteps], s));
    ND_HIP(hipStreamSynchronize(s));
    const auto &L = layers();
    for (int i = 0; i < kNumSteps; ++i) {
        nd_step_profile &o = steps[i];
        memset(&o, 0, sizeof(o));
        ND_HIP(hipEventElapsedTime(&o.ms, ev[i], ev[i + 1]));
        const UStep &st = kSteps[i];
        const Roi *roi = useful && rois[i].rows > 0 ? &rois[i] : nullptr;
        const UForm form = step_form(st, pl, flags, roi);
        o.form = (int)form;
        o.kind = st.layer >= 0 ? L[st.layer].kind : -1;
        const QpBuf &in = pl.buf[st.src];
        const double B = batch;
        const double hin = in.Hb - 2 * in.pad, win = in.Wb - 2 * in.pad;
        if (st.layer < 0) {
            o.bytes = B * 4.0 * 4 * st.dst_plane0 * (hin * win + (double)((int)hin / 2) * ((int)win / 2));
            continue;
        }
        const ULayer &l = L[st.layer];
        const double ci = l.cin, co = l.cout, cip = nd_kblocks(l.cin) * 8.0;
        // output pixels computed and input pixels read: a region lives on the output grid of a 3x3 layer (padding 1: as large as the
        // input) and on the input grid of a transpose
        double hout = hin, wout = win, hrd = hin, wrd = win;
        if (roi) {
            hout = hrd = roi->rows;
            wout = wrd = roi->cols;
        }
        if (l.kind == ND_CONVT2S2) {
            hout = 2 * hrd;
            wout = 2 * wrd;
            o.flops = 2.0 * hrd * wrd * ci * co * 4 * B;
            o.mfma_flops = 2.0 * 4 * cip * co * hrd * wrd * B;
        } else {
            // (algorithmic FLOP without the padding-zero MACs of the border taps)
            const double taps_px = roi ? 9.0 * hout * wout : (3 * hout - 2) * (3 * wout - 2);
            o.flops = 2.0 * taps_px * ci * co * B;
            const double Wg = (double)(((long)wout + 3) / 4);
            o.mfma_flops = form == UFORM_F43      ? 2.0 * 3 * 6 * cip * co * hout * Wg * B
                           : form == UFORM_WINO3P ? 2.0 * (kWinoTile + 2) * (kWinoTile + 2) * cip * co * (double)tiles_run[i]
                                                  : 2.0 * 9 * cip * co * hout * wout * B;
        }
        o.bytes = B * 4.0 * (ci * hrd * wrd + co * hout * wout) + 4.0 * ci * co * nd_taps(l.kind);
        if (form == UFORM_WINO3P && batch <= kWinoChunk) {
            ND_HIP(hipEventElapsedTime(&o.ms_xform_in, ev[i], evx[2 * i]));
            ND_HIP(hipEventElapsedTime(&o.ms_gemm, evx[2 * i], evx[2 * i + 1]));
            ND_HIP(hipEventElapsedTime(&o.ms_xform_out, evx[2 * i + 1], ev[i + 1]));
            QpBuf v = in;
            if (roi) {   // the passes ran on a view of rows + 2 x cols + 2 bordered input pixels
                v.Hb = roi->rows + 2;
                v.Wb = roi->cols + 2;
            }
            nd_wino_xform_bytes(kWinoTile, v, l.cin, l.cout, tiles_run[i], &o.xform_bytes_in, &o.xform_bytes_out);
        }
    }
    return ND_OK;
}

// ------------------------------------------------------------------ frame loop (denoise_image.py:240-267)
// gather -> stack -> final 1x1 + Sigmoid + stitch for tiles [tile_begin, tile_begin + tile_count) in ascending launches of at most
// `batch` tiles; no NCHW tile batch exists.  A launch is self-contained: a restricted layer reads only what the restricted layer
// before it wrote in the same launch (plan_rois), and everything the encoder and the skip halves hold is rewritten whole.
extern "C" int nd_unet_denoise_frame(int dtype, int flags, const void *packed, const float *img, float *canvas, int width, int height,
                                     int cs, int ucs, int ol, int tile_begin, int tile_count, int batch, void *ws, size_t ws_bytes,
                                     void *stream, nd_progress_fn progress, void *progress_ctx) {
    ND_TRY(nd_check_flags(flags, false, true, true));
    ND_TRY(check(cs, cs, batch, dtype));
    int cols = 0, rows = 0, crop = 0;
    ND_TRY(nd_tile_grid(width, height, cs, ucs, ol, &cols, &rows, &crop));
    if (tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > cols * rows)
        ND_FAIL(ND_EINVAL, "nd_unet_denoise_frame: tiles [%d,+%d) outside the grid of %d", tile_begin, tile_count, cols * rows);
    if (!packed || !img || !canvas || !ws) ND_FAIL(ND_EINVAL, "UNet: null pointer");
    const size_t need = make_plan(cs, cs, batch, nullptr, 0, flags).bytes;
    if (ws_bytes < need) ND_FAIL(ND_ENOMEM, "UNet workspace: %zu B given, %zu B needed", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const float *blob = (const float *)packed;
    const Blob bl = blob_layout(flags);
    const float *fw = blob + bl.off[layers().size() - 1];
    const int end = tile_begin + tile_count;
    int n = 0;
    for (int t0 = tile_begin; t0 < end; t0 += batch, ++n) {
        const int cnt = end - t0 < batch ? end - t0 : batch;
        if (progress) progress(progress_ctx, n, t0, cnt);
        const UPlan pl = make_plan(cs, cs, batch, (char *)ws, cnt, flags);
        Roi rois[kNumSteps];
        const bool useful = !(flags & ND_FLAG_FULL_TILES) && plan_rois(pl, crop, crop, rois) > 0 && rois_fit(pl, blob, bl, rois, flags);
        ND_TRY(nd_launch_gather_pack(img, width, height, cs, ucs, ol, t0, cnt, pl.buf[XIN], s, 1, false));
        for (int i = 0; i < kNumSteps; ++i) ND_TRY(run_step(kSteps[i], pl, blob, bl, useful ? &rois[i] : nullptr, flags, s));
        ND_TRY(nd_launch_final1x1_stitch(pl.buf[U4B], 64, fw, fw + 3 * 64, 0, canvas, width, height, cs, ucs, ol, t0, cnt, s, 1,
                                         (flags & ND_FLAG_FIND_NOISE) ? img : nullptr));
    }
    return ND_OK;
}
