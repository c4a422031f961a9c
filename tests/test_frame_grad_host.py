"""CPU tests of the index maps behind gradients through a tiled frame (nind_denoise_amd/frame_grad.py, csrc/aux_kernels.hip):
nd_tile_source and nd_stitch_weight -- the inline functions the gather / stitch kernels and their adjoints run -- against
oracle.tiler, pixel by pixel and exactly, and the host checks of nd_stitch_grad / nd_tile_gather_grad.

The maps built here (``oracle_maps``) are shared with test_frame_grad.py, which runs the kernels against them."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from nind_denoise_amd import _lib
from oracle import tiler as otiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, H, cs, ucs, ol): all valid for nd_tile_grid
GEOMS = [
    (104, 104, 104, 72, 8),      # 2 x 2; the tile is as wide as the frame: both folds hit one tile, up to 9 reads of a frame pixel
    (150, 130, 104, 72, 8),      # 3 x 2; the right tile mirrors 66 columns
    (120, 230, 104, 88, 16),     # 2 x 3
    (131, 119, 104, 40, 6),      # 4 x 4; pad 32, up to 20 reads
    (300, 170, 136, 56, 24),     # 9 x 5; pad 40 > stride 32, up to 25 reads
]
GRIDS = [(2, 2), (3, 2), (2, 3), (4, 4), (9, 5)]


@functools.lru_cache(maxsize=None)
def oracle_maps(geom):
    """(src, dst, w) of a geometry from oracle.tiler, each [tiles, cs, cs]: src = flat frame index Y * W + X that tile pixel
    (y, x) is gathered from (gather_tile on an index image); w = float32 weight with which the stitch adds the tile pixel
    (make_seamless_edges on ones inside the useful crop, 0 outside); dst = flat canvas index it is added to (-1 where w = 0)."""
    W, H, cs, ucs, ol = geom
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    assert W * H < 2 ** 24                      # the index image is exact in float32
    index = np.broadcast_to(np.arange(H * W, dtype=np.float32).reshape(1, H, W), (3, H, W))
    src = np.empty((grid.size, cs, cs), dtype=np.int64)
    dst = np.full((grid.size, cs, cs), -1, dtype=np.int64)
    w = np.zeros((grid.size, cs, cs), dtype=np.float32)
    for i in range(grid.size):
        t = otiler.gather_tile(index, grid, i)
        assert np.array_equal(t[0], t[1]) and np.array_equal(t[0], t[2])
        src[i] = t[0].astype(np.int64)
        _, _, ud, us = grid.geom(i)
        crop = otiler.make_seamless_edges(np.ones((3, ud[3] - ud[1], ud[2] - ud[0]), dtype=np.float32), us[0], us[1], grid)
        w[i, ud[1]:ud[3], ud[0]:ud[2]] = crop[0]
        yy, xx = np.mgrid[ud[1]:ud[3], ud[0]:ud[2]]
        dst[i, ud[1]:ud[3], ud[0]:ud[2]] = (us[1] + yy - ud[1]) * W + us[0] + xx - ud[0]
    for a in (src, dst, w):
        a.setflags(write=False)
    return src, dst, w


@functools.lru_cache(maxsize=None)
def lib_maps(geom):
    """The same three arrays from nd_tile_source / nd_stitch_weight, one call per tile pixel."""
    W, H, cs, ucs, ol = geom
    lib = _lib.load()
    cols, rows, _ = _lib.tile_grid(W, H, cs, ucs, ol)
    n = cols * rows
    src = np.empty((n, cs, cs), dtype=np.int64)
    dst = np.full((n, cs, cs), -1, dtype=np.int64)
    w = np.zeros((n, cs, cs), dtype=np.float32)
    Y, X, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    pY, pX, pf = ctypes.byref(Y), ctypes.byref(X), ctypes.byref(f)
    source, weight = lib.nd_tile_source, lib.nd_stitch_weight
    for i in range(n):
        for y in range(cs):
            srow, drow, wrow = src[i, y], dst[i, y], w[i, y]
            for x in range(cs):
                assert source(i, W, H, cs, ucs, ol, y, x, pY, pX) == 0
                assert 0 <= Y.value < H and 0 <= X.value < W
                srow[x] = Y.value * W + X.value
                assert weight(i, W, H, cs, ucs, ol, y, x, pY, pX, pf) == 0
                if f.value != 0:
                    assert 0 <= Y.value < H and 0 <= X.value < W
                    drow[x] = Y.value * W + X.value
                    wrow[x] = f.value
    return src, dst, w


def test_geometries_are_the_grids_the_issue_names():
    for geom, (cols, rows) in zip(GEOMS, GRIDS):
        c, r, pad = _lib.tile_grid(*geom)
        assert (c, r) == (cols, rows) and pad == (geom[2] - geom[3]) // 2
        grid = otiler.TileGrid(*geom)
        assert (grid.cols, grid.rows) == (cols, rows)


@pytest.mark.parametrize("geom", GEOMS)
def test_tile_source_is_the_oracles_gather(geom):
    src, _, _ = oracle_maps(geom)
    got, _, _ = lib_maps(geom)
    assert np.array_equal(got, src)


@pytest.mark.parametrize("geom, reads", zip(GEOMS, [9, None, None, 20, 25]))
def test_reads_per_frame_pixel(geom, reads):
    W, H = geom[:2]
    counts = np.bincount(oracle_maps(geom)[0].reshape(-1), minlength=W * H)
    assert counts.min() >= 1
    if reads is not None:
        assert counts.max() == reads


@pytest.mark.parametrize("geom", GEOMS)
def test_stitch_weight_is_the_oracles_seamless_stitch(geom):
    W, H, cs, ucs, ol = geom
    _, dst, w = oracle_maps(geom)
    _, gdst, gw = lib_maps(geom)
    assert np.array_equal(gw.view(np.int32), w.view(np.int32))
    assert np.array_equal(gdst, dst)
    assert set(np.unique(gw).tolist()) <= {0.0, 0.25, 0.5, 1.0}
    # the canvas the oracle's loop stitches from tiles of ones is the scatter of the weights
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    canvas = np.zeros((3, H, W), dtype=np.float32)
    ones = np.ones((3, cs, cs), dtype=np.float32)
    for i in range(grid.size):
        otiler.stitch_add(canvas, ones, grid, i)
    scat = np.zeros(H * W, dtype=np.float32)
    np.add.at(scat, gdst[gw != 0], gw[gw != 0])
    assert np.array_equal(scat.reshape(H, W), canvas[0])
    assert np.array_equal(canvas[0], np.ones((H, W), dtype=np.float32))     # seamless: the weights over a pixel sum to 1


def test_maps_reject_bad_arguments():
    lib = _lib.load()
    Y, X, f = ctypes.c_int(), ctypes.c_int(), ctypes.c_float()
    W, H, cs, ucs, ol = GEOMS[1]
    for i, y, x in [(-1, 0, 0), (6, 0, 0), (0, -1, 0), (0, cs, 0), (0, 0, -1), (0, 0, cs)]:
        with pytest.raises(ValueError):
            _lib.check(lib.nd_tile_source(i, W, H, cs, ucs, ol, y, x, Y, X))
        with pytest.raises(ValueError):
            _lib.check(lib.nd_stitch_weight(i, W, H, cs, ucs, ol, y, x, Y, X, f))
    with pytest.raises(ValueError):
        _lib.check(lib.nd_tile_source(0, W, H, cs, ucs, ol, 0, 0, None, X))
    with pytest.raises(ValueError):
        _lib.check(lib.nd_stitch_weight(0, W, H, cs, ucs, ol, 0, 0, Y, X, None))
    with pytest.raises(ValueError):                                           # a geometry nd_tile_grid refuses
        _lib.check(lib.nd_tile_source(0, 40, 40, cs, ucs, ol, 0, 0, Y, X))


def test_adjoint_entry_points_check_their_arguments_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(64)            # never dereferenced: every call below ends in its host checks
    W, H, cs, ucs, ol = GEOMS[1]       # 6 tiles
    for fn in (lib.nd_stitch_grad, lib.nd_tile_gather_grad):
        for a, b, begin, count in [(None, p, 0, 6), (p, None, 0, 6), (p, p, 0, 7), (p, p, 5, 2), (p, p, -1, 2), (p, p, 0, -1),
                                   (p, p, 7, 0), (p, p, 2 ** 31 - 1, 2)]:
            with pytest.raises(ValueError):
                _lib.check(fn(a, W, H, cs, ucs, ol, begin, count, b, None))
        with pytest.raises(ValueError):                                       # ucs does not exceed the overlap
            _lib.check(fn(p, W, H, cs, 8, 8, 0, 1, p, None))
        with pytest.raises(ValueError):                                       # the frame is smaller than the mirror padding
            _lib.check(fn(p, 20, 20, cs, ucs, ol, 0, 1, p, None))
        for begin in (0, 3, 6):                                               # no tiles: a no-op
            assert fn(p, W, H, cs, ucs, ol, begin, 0, p, None) == 0


def test_header_and_bindings_declare_the_frame_gradient_entry_points():
    hdr = open(os.path.join(ROOT, "include", "nind_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", code))
    assert {"nd_tile_source", "nd_stitch_weight", "nd_stitch_grad", "nd_tile_gather_grad"} <= declared
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    assert _lib.load().nd_version() >= 116
