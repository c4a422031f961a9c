"""Gradients through the crop -> infer -> stitch loop over a frame (pipeline.denoise_frame, denoise_image.py:239-267).

The loop is gather (a linear operator: crop + symmetric mirror), the network on every tile, and stitch (linear: useful crop,
halved overlap strips, canvas +=).  The adjoints of the two linear operators are HIP kernels (``nd_stitch_grad``,
``nd_tile_gather_grad``: no atomics, fixed summation order), so a loss taken on the stitched canvas -- one that sees the
seams, the mirrored borders and the overlap blending -- reaches the frame and the network's parameters.

``gather_tiles`` / ``stitch_tiles`` are the two operators as differentiable torch functions: any torch-callable model
differentiates through a frame with them (``denoise_frame`` does exactly that for a model that is not a ``UtNet``).  torch
then keeps every launch's graph until the backward: the memory of a frame's worth of tile activations.

For ``UtNet``, ``denoise_frame`` keeps nothing but the frame: the forward is the fused inference loop of
``pipeline.denoise_frame`` (the same canvas, bit for bit), and the backward walks the launches in ascending order and, per
launch, gathers the tiles again, runs the training forward (``nd_utnet_train_forward_hw``: pre-activations kept), takes
the launch's tile gradients out of the canvas gradient (``nd_stitch_grad``), runs the training backward
(``nd_utnet_train_backward_hw``; parameter gradients and the input gradient each only if asked for) and adds the tiles'
input gradients into the frame gradient (``nd_tile_gather_grad``).  Memory: one training workspace of (cs, cs, batch).
The gradient is that of the recomputed forward (the training step's kernels, ``model.flags``: ``winograd`` and ``split_k``
are honoured), which agrees with the inference loop's canvas up to fp32 re-association.

The recompute uses the module's one training state.  Like every forward under autograd it bumps the state's generation
counter: a crop graph built by ``model(x)`` before a frame backward of the same module is stale afterwards, and its
backward raises.  A frame graph never goes stale (it holds no activations), so several may be in flight.

``UNet`` in eval mode gets the same treatment (``nd_unet_grad_forward`` / ``nd_unet_grad_backward``: BatchNorm on its running
statistics, every activation kept, ``find_noise`` honoured); a train-mode ``UNet`` raises ``RuntimeError`` as its forward does.

There is no CPU path: a CPU tensor raises.
"""
import torch

from . import _lib, pipeline
from .networks.ThirdPartyNets import UNet
from .networks.UtNet import UtNet


def _check_frame(t, what):
    if t.device.type != "cuda":
        raise RuntimeError(f"frame_grad: {what} must be resident on the GPU (no CPU fallback)")
    if t.dim() != 3 or t.size(0) != 3:
        raise ValueError(f"frame_grad: {what} must be [3,H,W], got {tuple(t.shape)}")


# ---------------------------------------------------------------------------- the two adjoint kernels

def stitch_grad(gcanvas, cs, ucs, ol, tile_begin, count, out=None):
    """nd_stitch_grad: gcanvas [3,H,W] float32 -> the gradient of tiles [tile_begin, tile_begin + count), [count,3,cs,cs]:
    weight of the stitch times the canvas gradient at the pixel a tile pixel is added to, 0 outside the useful crop."""
    _check_frame(gcanvas, "the canvas gradient")
    assert gcanvas.dtype == torch.float32 and gcanvas.is_contiguous()
    if out is None:
        out = torch.empty((count, 3, cs, cs), dtype=torch.float32, device=gcanvas.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and out.numel() >= count * 3 * cs * cs
    with torch.cuda.device(gcanvas.device):
        _lib.check(_lib.load().nd_stitch_grad(gcanvas.data_ptr(), gcanvas.size(2), gcanvas.size(1), cs, ucs, ol, tile_begin, count,
                                              out.data_ptr(), _lib.stream_ptr(gcanvas.device)), "nd_stitch_grad")
    return out


def tile_gather_grad(gtiles, gimg, cs, ucs, ol, tile_begin, count=None):
    """nd_tile_gather_grad: gimg [3,H,W] += the gradients of tiles [tile_begin, tile_begin + count) (gtiles [>=count,3,cs,cs]),
    every tile pixel added to the frame pixel it was gathered from (mirrored pixels included), in a fixed order."""
    _check_frame(gimg, "the frame gradient")
    count = gtiles.size(0) if count is None else count
    assert gimg.dtype == torch.float32 and gimg.is_contiguous()
    assert gtiles.is_cuda and gtiles.dtype == torch.float32 and gtiles.is_contiguous() and gtiles.numel() >= count * 3 * cs * cs
    with torch.cuda.device(gimg.device):
        _lib.check(_lib.load().nd_tile_gather_grad(gtiles.data_ptr(), gimg.size(2), gimg.size(1), cs, ucs, ol, tile_begin, count,
                                                   gimg.data_ptr(), _lib.stream_ptr(gimg.device)), "nd_tile_gather_grad")
    return gimg


# ---------------------------------------------------------------------------- gather and stitch under autograd

class _GatherTiles(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, cs, ucs, ol, tile_begin, count):
        ctx.geom = (tuple(img.shape), cs, ucs, ol, tile_begin, count)
        return pipeline.gather_tiles(img, cs, ucs, ol, tile_begin, count)

    @staticmethod
    def backward(ctx, g):
        shape, cs, ucs, ol, tile_begin, count = ctx.geom
        gimg = torch.zeros(shape, dtype=torch.float32, device=g.device)
        tile_gather_grad(g.to(torch.float32).contiguous(), gimg, cs, ucs, ol, tile_begin, count)
        return gimg, None, None, None, None, None


class _StitchTiles(torch.autograd.Function):
    @staticmethod
    def forward(ctx, canvas, tiles, cs, ucs, ol, tile_begin):
        ctx.geom = (cs, ucs, ol, tile_begin, tiles.size(0))
        return pipeline.stitch_tiles(canvas.clone(memory_format=torch.contiguous_format), tiles, cs, ucs, ol, tile_begin)

    @staticmethod
    def backward(ctx, g):
        cs, ucs, ol, tile_begin, count = ctx.geom
        gtiles = None
        if ctx.needs_input_grad[1]:
            gtiles = stitch_grad(g.to(torch.float32).contiguous(), cs, ucs, ol, tile_begin, count)
        return (g if ctx.needs_input_grad[0] else None), gtiles, None, None, None, None


def gather_tiles(img, cs, ucs, ol, tile_begin, count):
    """Differentiable pipeline.gather_tiles: img [3,H,W] float32 on the GPU -> tiles [count,3,cs,cs] (crop + symmetric mirror)."""
    _check_frame(img, "the frame")
    return _GatherTiles.apply(img.to(torch.float32), cs, ucs, ol, tile_begin, count)


def stitch_tiles(canvas, tiles, cs, ucs, ol, tile_begin):
    """Differentiable pipeline.stitch_tiles.  Returns a NEW canvas = canvas + the seamless useful crops of tiles [n,3,cs,cs]
    (tiles tile_begin ...); the canvas passed in is left as it is, as autograd requires."""
    _check_frame(canvas, "the canvas")
    if tiles.device != canvas.device:
        raise RuntimeError("frame_grad: tiles and canvas must be on the same GPU")
    return _StitchTiles.apply(canvas.to(torch.float32), tiles.to(torch.float32).contiguous(), cs, ucs, ol, tile_begin)


# ---------------------------------------------------------------------------- UtNet: recompute launch by launch

class _UtNetFrame(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, names, geom, img, *params):
        cs, ucs, ol, batch, begin, end = geom
        ctx.model, ctx.names, ctx.geom = model, names, geom
        ctx.save_for_backward(img, *params)
        return pipeline.denoise_frame(model, img, cs, ucs, ol, batch=batch, tile_range=(begin, end))

    @staticmethod
    def backward(ctx, gcanvas):
        model, names = ctx.model, ctx.names
        cs, ucs, ol, batch, begin, end = ctx.geom
        img, *params = ctx.saved_tensors
        want_img, want_p = ctx.needs_input_grad[3], ctx.needs_input_grad[4:]
        dev = img.device
        height, width = img.size(1), img.size(2)
        lib = _lib.load()
        st = model._train_state(dev)
        st.load(dict(zip(names, params)))
        gcanvas = gcanvas.to(torch.float32).contiguous()
        gimg = torch.zeros_like(img) if want_img else None
        acc = torch.zeros_like(st.grads) if any(want_p) else None
        batch = max(1, min(batch, end - begin))
        x = torch.empty((batch, 3, cs, cs), dtype=torch.float32, device=dev)
        y, gt = torch.empty_like(x), torch.empty_like(x)
        dx = torch.empty_like(x) if want_img else None
        act, flags = _lib.ACT[model.activation], model.flags
        with torch.cuda.device(dev):
            s = _lib.stream_ptr(dev)
            ws = st.workspace(cs, cs, batch)
            laid_out = batch                      # the launch size the workspace's zero borders are laid out for
            for t0 in range(begin, end, batch):
                cnt = min(batch, end - t0)
                if cnt != laid_out:               # the partial last launch: the same buffer, laid out for fewer tiles
                    assert lib.nd_utnet_train_workspace_bytes_hw(model.funit, cs, cs, cnt) <= ws.numel()
                    _lib.check(lib.nd_utnet_train_workspace_init_hw(ws.data_ptr(), ws.numel(), model.funit, cs, cs, cnt, s),
                               "nd_utnet_train_workspace_init_hw")
                    laid_out = cnt
                _lib.check(lib.nd_tile_gather(img.data_ptr(), width, height, cs, ucs, ol, t0, cnt, x.data_ptr(), s), "nd_tile_gather")
                _lib.check(lib.nd_utnet_train_forward_hw(model.funit, act, flags, st.flat.data_ptr(), st.blobs.data_ptr(), x.data_ptr(),
                                                         y.data_ptr(), cnt, cs, cs, ws.data_ptr(), ws.numel(), s),
                           "nd_utnet_train_forward_hw")
                st.generation += 1                # the workspace now holds this launch: an older crop graph is stale
                _lib.check(lib.nd_stitch_grad(gcanvas.data_ptr(), width, height, cs, ucs, ol, t0, cnt, gt.data_ptr(), s), "nd_stitch_grad")
                _lib.check(lib.nd_utnet_train_backward_hw(model.funit, act, flags, st.flat.data_ptr(),
                                                          st.grads.data_ptr() if acc is not None else None, st.blobs.data_ptr(),
                                                          gt.data_ptr(), dx.data_ptr() if want_img else None, cnt, cs, cs,
                                                          ws.data_ptr(), ws.numel(), s, None, 0), "nd_utnet_train_backward_hw")
                if acc is not None:
                    acc += st.grads
                if want_img:
                    _lib.check(lib.nd_tile_gather_grad(dx.data_ptr(), width, height, cs, ucs, ol, t0, cnt, gimg.data_ptr(), s),
                               "nd_tile_gather_grad")
            if laid_out != batch:                 # leave the state's workspace as its key says
                _lib.check(lib.nd_utnet_train_workspace_init_hw(ws.data_ptr(), ws.numel(), model.funit, cs, cs, batch, s),
                           "nd_utnet_train_workspace_init_hw")
        grads = []
        for n, p, want in zip(names, params, want_p):
            off, cnt = st.ranges[n]
            grads.append(acc[off:off + cnt].view(p.shape).clone() if want else None)
        return (None, None, None, gimg) + tuple(grads)


# ---------------------------------------------------------------------------- UNet (eval mode): the same recompute

class _UNetFrame(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, names, geom, img, *params):
        cs, ucs, ol, batch, begin, end = geom
        ctx.model, ctx.names, ctx.geom = model, names, geom
        ctx.save_for_backward(img, *params)
        return pipeline.denoise_frame(model, img, cs, ucs, ol, batch=batch, tile_range=(begin, end))

    @staticmethod
    def backward(ctx, gcanvas):
        model, names = ctx.model, ctx.names
        cs, ucs, ol, batch, begin, end = ctx.geom
        img, *params = ctx.saved_tensors
        want_img, want_p = ctx.needs_input_grad[3], ctx.needs_input_grad[4:]
        dev = img.device
        height, width = img.size(1), img.size(2)
        lib = _lib.load()
        st = model._grad_state(dev)
        st.load(dict(zip(names, params)))
        st.load(dict(model.named_buffers()))
        gcanvas = gcanvas.to(torch.float32).contiguous()
        gimg = torch.zeros_like(img) if want_img else None
        acc = torch.zeros_like(st.grads) if any(want_p) else None
        batch = max(1, min(batch, end - begin))
        x = torch.empty((batch, 3, cs, cs), dtype=torch.float32, device=dev)
        y, gt = torch.empty_like(x), torch.empty_like(x)
        dx = torch.empty_like(x) if want_img else None
        flags = model.grad_flags
        with torch.cuda.device(dev):
            s = _lib.stream_ptr(dev)
            ws = st.workspace(cs, cs, batch)
            laid_out = batch                      # the launch size the workspace's zero borders are laid out for
            for t0 in range(begin, end, batch):
                cnt = min(batch, end - t0)
                if cnt != laid_out:               # the partial last launch: the same buffer, laid out for fewer tiles
                    _lib.check(lib.nd_unet_grad_workspace_init(ws.data_ptr(), ws.numel(), cs, cs, cnt, s), "nd_unet_grad_workspace_init")
                    laid_out = cnt
                _lib.check(lib.nd_tile_gather(img.data_ptr(), width, height, cs, ucs, ol, t0, cnt, x.data_ptr(), s), "nd_tile_gather")
                _lib.check(lib.nd_unet_grad_forward(flags, st.flat.data_ptr(), st.blobs.data_ptr(), x.data_ptr(), y.data_ptr(), cnt, cs, cs,
                                                    ws.data_ptr(), ws.numel(), s), "nd_unet_grad_forward")
                st.generation += 1                # the workspace now holds this launch: an older crop graph is stale
                _lib.check(lib.nd_stitch_grad(gcanvas.data_ptr(), width, height, cs, ucs, ol, t0, cnt, gt.data_ptr(), s), "nd_stitch_grad")
                _lib.check(lib.nd_unet_grad_backward(flags, st.flat.data_ptr(), st.grads.data_ptr() if acc is not None else None,
                                                     st.blobs.data_ptr(), gt.data_ptr(), dx.data_ptr() if want_img else None, cnt, cs, cs,
                                                     ws.data_ptr(), ws.numel(), s), "nd_unet_grad_backward")
                if acc is not None:
                    acc += st.grads
                if want_img:
                    _lib.check(lib.nd_tile_gather_grad(dx.data_ptr(), width, height, cs, ucs, ol, t0, cnt, gimg.data_ptr(), s),
                               "nd_tile_gather_grad")
            if laid_out != batch:                 # leave the state's workspace as its key says
                _lib.check(lib.nd_unet_grad_workspace_init(ws.data_ptr(), ws.numel(), cs, cs, batch, s), "nd_unet_grad_workspace_init")
        grads = []
        for n, p, want in zip(names, params, want_p):
            off, cnt = st.ranges[n]
            grads.append(acc[off:off + cnt].view(p.shape).clone() if want else None)
        return (None, None, None, gimg) + tuple(grads)


def denoise_frame(model, img, cs, ucs, ol, batch=16, tile_range=None):
    """pipeline.denoise_frame with a graph behind its canvas.  img: [3,H,W] float32 on the GPU; returns the stitched [3,H,W]
    canvas.  When grad mode is on and img or a parameter of the model requires a gradient the canvas has a grad_fn (in
    train() and eval() alike); otherwise this is pipeline.denoise_frame.

    UtNet (fp32; another compute_dtype raises NotImplementedError, as UtNet.forward under autograd does): the fused inference
    loop forward, a launch-by-launch recompute backward -- memory is one training workspace of (cs, cs, batch), see the module
    docstring (also for the generation counter).  Any other torch-callable model: gather_tiles -> model -> stitch_tiles per
    launch, whose graphs torch keeps.  UNet (eval mode; train mode raises RuntimeError): as UtNet, on one gradient workspace.
    tile_range=(begin, end): only those tiles, as in pipeline.denoise_frame."""
    _check_frame(img, "the frame")
    params = [(n, p) for n, p in model.named_parameters()] if isinstance(model, torch.nn.Module) else []
    if not (torch.is_grad_enabled() and (img.requires_grad or any(p.requires_grad for _, p in params))):
        return pipeline.denoise_frame(model, img, cs, ucs, ol, batch=batch, tile_range=tile_range)
    if isinstance(model, UNet) and model.training:
        raise RuntimeError("nind_denoise_amd.UNet implements eval mode (BatchNorm running statistics) only; call .eval()")
    img = img.to(torch.float32).contiguous()
    total = pipeline.tile_count(img.size(2), img.size(1), cs, ucs, ol)
    begin, end = (0, total) if tile_range is None else tile_range
    if not 0 <= begin <= end <= total:
        raise ValueError(f"frame_grad.denoise_frame: tile range [{begin},{end}) outside the grid of {total}")
    batch = max(1, int(batch))
    if isinstance(model, UtNet):
        if model.compute_dtype != "f32":
            raise NotImplementedError("UtNet under autograd runs in fp32 (the training step's arithmetic)")
        return _UtNetFrame.apply(model, tuple(n for n, _ in params), (cs, ucs, ol, batch, begin, end), img, *[p for _, p in params])
    if isinstance(model, UNet):
        return _UNetFrame.apply(model, tuple(n for n, _ in params), (cs, ucs, ol, batch, begin, end), img, *[p for _, p in params])
    canvas = torch.zeros_like(img)
    for t0 in range(begin, end, batch):
        cnt = min(batch, end - t0)
        canvas = stitch_tiles(canvas, model(gather_tiles(img, cs, ucs, ol, t0, cnt)), cs, ucs, ol, t0)
    return canvas
