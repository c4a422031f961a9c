"""Device-resident crop -> infer -> stitch loop (the hot loop of the reference's denoise_image.py:239-267).

The frame stays in HBM as float32 CHW; tiles are gathered, denoised and stitched on the GPU in batches,
in ascending tile index order (the reference's fp32 summation order), with no host synchronisation
inside the loop.  For ``UtNet`` the three stages are fused by ``nd_utnet_denoise_frame`` (no NCHW tile
batch is ever materialised; in fp32 the first two encoder levels run once per band of tile rows), for
``UNet`` by ``nd_unet_denoise_frame`` (same fusion, the decoder restricted to what the kept centre of a
tile needs); any other callable model goes through ``nd_tile_gather`` -> model -> ``nd_stitch_add``.
"""
import torch

from . import _lib
from .networks.ThirdPartyNets import UNet
from .networks.UtNet import UtNet


def tile_count(width, height, cs, ucs, ol):
    cols, rows, _ = _lib.tile_grid(width, height, cs, ucs, ol)
    return cols * rows


def gather_tiles(img, cs, ucs, ol, tile_begin, count):
    """img: [3,H,W] float32 cuda -> [count,3,cs,cs] (OneImageDS.__getitem__, denoise_image.py:129-174)."""
    assert img.is_cuda and img.dtype == torch.float32 and img.dim() == 3 and img.size(0) == 3
    img = img.contiguous()
    out = torch.empty((count, 3, cs, cs), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().nd_tile_gather(img.data_ptr(), img.size(2), img.size(1), cs, ucs, ol, tile_begin, count,
                                              out.data_ptr(), _lib.stream_ptr(img.device)), "nd_tile_gather")
    return out


def stitch_tiles(canvas, tiles, cs, ucs, ol, tile_begin):
    """canvas [3,H,W] += seamless useful crops of tiles [n,3,cs,cs] (denoise_image.py:204-213,249-267)."""
    assert canvas.is_cuda and canvas.is_contiguous() and tiles.is_cuda
    tiles = tiles.to(torch.float32).contiguous()
    with torch.cuda.device(canvas.device):
        _lib.check(_lib.load().nd_stitch_add(canvas.data_ptr(), canvas.size(2), canvas.size(1), cs, ucs, ol,
                                             tiles.data_ptr(), tile_begin, tiles.size(0),
                                             _lib.stream_ptr(canvas.device)), "nd_stitch_add")
    return canvas


def denoise_frame(model, img, cs, ucs, ol, batch=16, tile_range=None, canvas=None, progress=None):
    """Denoise one frame.  img: [3,H,W] float32 on the GPU.  Returns the stitched [3,H,W] canvas (on the GPU).

    tile_range=(begin, end) restricts the loop to a contiguous range of tile indices (multi-GPU sharding);
    the canvas then only holds those tiles' contributions.
    """
    if img.device.type != "cuda":
        raise RuntimeError("denoise_frame: the frame must be resident on the GPU (no CPU fallback)")
    img = img.to(torch.float32).contiguous()
    height, width = img.size(1), img.size(2)
    total = tile_count(width, height, cs, ucs, ol)
    begin, end = (0, total) if tile_range is None else tile_range
    if canvas is None:
        canvas = torch.zeros_like(img)
    lib = _lib.load()
    with torch.cuda.device(img.device):
        if isinstance(model, UtNet):
            if end <= begin:
                return canvas
            # one call for the whole range: the library walks it band by band (nd_utnet_denoise_frame), in launches of <= batch
            batch = max(1, min(batch, end - begin))
            blob = model.packed_weights(img.device)
            ws = model.workspace(cs, batch, img.device)
            fws = model.frame_workspace(width, height, cs, ucs, ol, batch, img.device)
            cb = _lib.PROGRESS_FN(lambda _ctx, n, t0, cnt: progress(n, t0, cnt)) if progress is not None else _lib.PROGRESS_FN()
            _lib.check(lib.nd_utnet_denoise_frame(model.funit, _lib.ACT[model.activation], _lib.DTYPE[model.compute_dtype], model.frame_flags,
                                                  blob.data_ptr(), img.data_ptr(), canvas.data_ptr(), width, height, cs, ucs, ol,
                                                  begin, end - begin, batch, ws.data_ptr(), ws.numel(),
                                                  fws.data_ptr() if fws is not None else None, fws.numel() if fws is not None else 0,
                                                  _lib.stream_ptr(img.device), cb, None), "nd_utnet_denoise_frame")
            return canvas
        if isinstance(model, UNet):
            if end <= begin:
                return canvas
            if model.training:
                raise RuntimeError("nind_denoise_amd.UNet implements eval mode (BatchNorm running statistics) only; call .eval()")
            batch = max(1, min(batch, end - begin))
            blob = model.packed_weights(img.device)
            ws = model.workspace(cs, cs, batch, img.device)
            cb = _lib.PROGRESS_FN(lambda _ctx, n, t0, cnt: progress(n, t0, cnt)) if progress is not None else _lib.PROGRESS_FN()
            flags = model.flags | (_lib.FLAG_FIND_NOISE if model.find_noise else 0)
            _lib.check(lib.nd_unet_denoise_frame(_lib.ND_F32, flags, blob.data_ptr(), img.data_ptr(), canvas.data_ptr(), width, height,
                                                 cs, ucs, ol, begin, end - begin, batch, ws.data_ptr(), ws.numel(),
                                                 _lib.stream_ptr(img.device), cb, None), "nd_unet_denoise_frame")
            return canvas
        for n, t0 in enumerate(range(begin, end, batch)):
            cnt = min(batch, end - t0)
            if progress is not None:
                progress(n, t0, cnt)
            x = gather_tiles(img, cs, ucs, ol, t0, cnt)
            y = model(x)
            stitch_tiles(canvas, y, cs, ucs, ol, t0)
    return canvas
