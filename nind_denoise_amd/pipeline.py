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


FALLBACK_BATCH = 16   # tiles per launch of the recomputation, at most


def bad_tile_runs(tile_ok, begin=0):
    """Maximal runs of consecutive bad tiles: tile_ok is the sequence of flags of tiles begin, begin + 1, ... (0: bad); returns
    [(first tile, count), ...] in ascending order."""
    runs = []
    for k, ok in enumerate(tile_ok):
        if ok:
            continue
        if runs and runs[-1][0] + runs[-1][1] == begin + k:
            runs[-1][1] += 1
        else:
            runs.append([begin + k, 1])
    return [tuple(r) for r in runs]


def _utnet_frame_call(lib, model, dtype, flags, blob, ws, fws, img, canvas, geom, begin, count, batch, cb, tile_ok=None):
    width, height, cs, ucs, ol = geom
    args = (model.funit, _lib.ACT[model.activation], _lib.DTYPE[dtype], flags, blob.data_ptr(), img.data_ptr(), canvas.data_ptr(),
            width, height, cs, ucs, ol, begin, count, batch, ws.data_ptr(), ws.numel(),
            fws.data_ptr() if fws is not None else None, fws.numel() if fws is not None else 0, _lib.stream_ptr(img.device), cb, None)
    if tile_ok is None:
        _lib.check(lib.nd_utnet_denoise_frame(*args), "nd_utnet_denoise_frame")
    else:
        _lib.check(lib.nd_utnet_denoise_frame_checked(*args, tile_ok.data_ptr()), "nd_utnet_denoise_frame_checked")


def _fill_report(report, tiles, fallback_tiles, fallback_dtype):
    if report is not None:
        report.update(tiles=tiles, fallback_tiles=sorted(fallback_tiles), fallback_dtype=fallback_dtype)


def fallback_line(report):
    """The line the callers print when tiles were recomputed (None when none were)."""
    if not report or not report.get("fallback_tiles"):
        return None
    return f'fallback: {len(report["fallback_tiles"])} of {report["tiles"]} tiles recomputed in {report["fallback_dtype"]}'


def denoise_frame(model, img, cs, ucs, ol, batch=16, tile_range=None, canvas=None, progress=None, report=None):
    """Denoise one frame.  img: [3,H,W] float32 on the GPU.  Returns the stitched [3,H,W] canvas (on the GPU).

    tile_range=(begin, end) restricts the loop to a contiguous range of tile indices (multi-GPU sharding);
    the canvas then only holds those tiles' contributions.

    A ``UtNet`` with a ``fallback_dtype`` runs the checked loop (``nd_utnet_denoise_frame_checked``): a tile whose contribution is
    not finite in the compute dtype stays out of the canvas, and exactly those tiles are then recomputed in the fallback dtype with
    the per-tile encoder -- maximal runs of consecutive tiles, ascending, ``min(batch, 16, run length)`` tiles per launch -- and added
    to the same canvas.  A canvas pixel is therefore the sum of its good tiles in ascending order followed by its recomputed tiles
    in ascending order: the bits of the plain run wherever no bad tile covers it.  Between the two passes the flags of the range are
    read once: the one host synchronisation per call the option adds (also per shard call of a multi-GPU frame, where its cost has
    not been measured).  The fallback's blob and workspace are built on the first frame that needs them.  report (a dict, optional)
    receives ``tiles`` (of the range), ``fallback_tiles`` (sorted indices) and ``fallback_dtype`` (None for any other model).
    """
    if img.device.type != "cuda":
        raise RuntimeError("denoise_frame: the frame must be resident on the GPU (no CPU fallback)")
    img = img.to(torch.float32).contiguous()
    height, width = img.size(1), img.size(2)
    total = tile_count(width, height, cs, ucs, ol)
    begin, end = (0, total) if tile_range is None else tile_range
    if canvas is None:
        canvas = torch.zeros_like(img)
    _fill_report(report, max(0, end - begin), [], None)
    lib = _lib.load()
    with torch.cuda.device(img.device):
        if isinstance(model, UtNet):
            if end <= begin:
                return canvas
            # one call for the whole range: the library walks it band by band (nd_utnet_denoise_frame), in launches of <= batch
            batch = max(1, min(batch, end - begin))
            fallback = model.checked_fallback_dtype()      # (the pair is checked here: set_compute_dtype may have changed it)
            blob = model.packed_weights(img.device)
            ws = model.workspace(cs, batch, img.device)
            fws = model.frame_workspace(width, height, cs, ucs, ol, batch, img.device)
            cb = _lib.PROGRESS_FN(lambda _ctx, n, t0, cnt: progress(n, t0, cnt)) if progress is not None else _lib.PROGRESS_FN()
            geom = (width, height, cs, ucs, ol)
            if fallback is None:
                _utnet_frame_call(lib, model, model.compute_dtype, model.frame_flags, blob, ws, fws, img, canvas, geom, begin, end - begin,
                                  batch, cb)
                return canvas
            tile_ok = torch.ones(total, dtype=torch.uint8, device=img.device)
            _utnet_frame_call(lib, model, model.compute_dtype, model.frame_flags, blob, ws, fws, img, canvas, geom, begin, end - begin,
                              batch, cb, tile_ok)
            runs = bad_tile_runs(tile_ok[begin:end].tolist(), begin)     # the one host read (synchronises the stream)
            none = _lib.PROGRESS_FN()
            for t0, cnt in runs:
                fbatch = min(batch, FALLBACK_BATCH, cnt)
                _utnet_frame_call(lib, model, fallback, model.frame_flags | _lib.FLAG_TILE_ENCODER, model.packed_weights(img.device, fallback),
                                  model.workspace(cs, fbatch, img.device, dtype=fallback), None, img, canvas, geom, t0, cnt, fbatch, none)
            _fill_report(report, end - begin, [t for t0, cnt in runs for t in range(t0, t0 + cnt)], fallback)
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
