"""P2's border lines in the shared encoder: one pair of row-edge images per tile row and one pair of column-edge images per tile
column of a band, and four corner patches per tile (utnet_frame.hip: row_plan, col_plan, corner_plan).

CPU: the identity it rests on, in float64 with the oracle's tiler -- the P2 line of the long edge image, windowed at a tile, is the
tile's own border line except at its two end pixels, and the corner patch gives those.  GPU: the frame loop against the per-tile
encoder and float64 on geometries tests/test_shared_encoder.py does not run (a stride of 4 x odd, the narrowest and the lowest
frame the shared plan takes, a last band of a single tile row), and tile ranges inside one tile row / of a single tile."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import synth
from test_shared_encoder import (BAR_FRAME16, BAR_SHARED16, BAR_SHARED64, BAR_TILE64, VISIBLE_GAIN, _band_samples, _model64,
                                 _net_visible, _plan, _rel, _sd64)

K = 16          # kStrip: input lines that yield one P2 line through convs1.0 ... pool 2


def _p2_64(sd, x):
    """The six shared steps in float64: convs1, pool, convs2, pool.  Returns (convs2's output, P2 = its pool: the level-2 input)."""
    for lv in (1, 2):
        for k in (0, 2):
            p = f"convs{lv}.{k}"
            x = F.prelu(F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"]), sd[f"convs{lv}.{k + 1}.weight"])
        pre, x = x, F.max_pool2d(x, 2)
    return pre, x


def _mirror_sym(v, n):       # edge pixel repeated: the tiler's mirror of the frame
    return -1 - v if v < 0 else (2 * n - 1 - v if v >= n else v)


def _reflect_nr(v, n):       # nn.ReflectionPad2d: edge pixel not repeated
    return -v if v < 0 else (2 * (n - 1) - v if v >= n else v)


def _tile_axis(ti, S, pad, cs, n):
    """Frame lines of the cs + 4 lines of tile index ti's reflect-padded input along one axis."""
    return np.array([_mirror_sym(ti * S - pad + _reflect_nr(q - 2, cs), n) for q in range(cs + 4)])


def _band_axis(b0, length, n):
    """Frame lines of a band image along one axis: the mirrored frame from b0, clamped (the outer ring no tile reaches unpadded)."""
    return np.clip([_mirror_sym(b0 + u, n) for u in range(length)], 0, n - 1)


# the last: pad 40 > stride 32; the second: S = 68 = 4 * 17.  R: tile rows per band of this restatement (the last band is short)
@pytest.mark.parametrize("geom,R", [((333, 290, 120, 88, 16), 3), ((333, 290, 120, 88, 20), 2), ((300, 170, 136, 56, 24), 4)])
def test_edge_lines_are_windows_of_the_long_edge_images(geom, R):
    """Every tile of the frame: the windowed lines equal the tile's own P2 border lines to 1e-12 on pixels 1 ... n-2, and the corner
    patches equal its four corner pixels.  The end pixels of a windowed line are another function of the frame (the image lacks
    the tile's reflection along the line): convs2's output, which P2 pools, differs there for every tile and line.  P2 itself
    takes a 2 x 2 maximum that may fall on the clean half of the block in all 8 channels of one pixel, so a single end pixel can
    coincide: at least 3 in 4 of a frame's end pixels must differ."""
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.make_utnet_state_dict(funit=4, seed=5).items()}
    frame = synth.make_frame(W, H, seed=1).astype(np.float64)
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    S, pad = ucs - ol, grid.pad
    assert S % 4 == 0 and grid.rows > R > 1
    n2 = (cs // 2 - 4) // 2
    wx = (grid.cols - 1) * S + cs + 4
    xs_band = _band_axis(-pad - 2, wx, W)

    def p2(ys, xs):
        pre, out = _p2_64(sd, torch.from_numpy(frame[:, ys][:, :, xs])[None])
        return pre[0], out[0]

    def ends(k):
        return slice(0, K) if k == 0 else slice(cs + 4 - K, cs + 4)

    seen_edges, end_differs = set(), []
    for row0 in range(0, grid.rows, R):
        nrows = min(R, grid.rows - row0)
        ys_band = _band_axis(row0 * S - pad - 2, (nrows - 1) * S + cs + 4, H)
        # two column-edge images per tile column of the band, two row-edge images per tile row
        col_lines = [[p2(ys_band, _tile_axis(xi, S, pad, cs, W)[ends(k)]) for k in (0, 1)] for xi in range(grid.cols)]
        for yi in range(row0, row0 + nrows):
            ys = _tile_axis(yi, S, pad, cs, H)
            row_lines = [p2(ys[ends(k)], xs_band) for k in (0, 1)]
            assert row_lines[0][1].shape[1:] == (1, (grid.cols - 1) * S // 4 + n2)
            for xi in range(grid.cols):
                i = yi * grid.cols + xi
                xs = _tile_axis(xi, S, pad, cs, W)
                tile = otiler.gather_tile(frame.astype(np.float32), grid, i).astype(np.float64)
                xp = F.pad(torch.from_numpy(tile)[None], (2, 2, 2, 2), mode="reflect")
                assert np.array_equal(xp[0].numpy(), frame[:, ys][:, :, xs])      # the index maps above are the tiler's gather
                own3, own = (t[0] for t in _p2_64(sd, xp))
                assert own.shape[1:] == (n2, n2)
                ox, oy = xi * S // 4, (yi - row0) * S // 4
                seen_edges |= {("top", yi == 0), ("bottom", yi == grid.rows - 1), ("left", xi == 0), ("right", xi == grid.cols - 1)}
                for k, at in ((0, 0), (1, n2 - 1)):
                    (r3, r), (c3, c) = row_lines[k], col_lines[xi][k]
                    # (name, P2 line and the two convs2 lines it pools, of the edge image's window and of the tile: [C, n2] / [C, 2, 2 n2])
                    for name, line, line3, mine, mine3 in (
                            ("row", r[:, 0, ox:ox + n2], r3[:, :, 2 * ox:2 * (ox + n2)], own[:, at, :], own3[:, 2 * at:2 * at + 2, :]),
                            ("col", c[:, oy:oy + n2, 0], c3[:, 2 * oy:2 * (oy + n2), :].transpose(1, 2), own[:, :, at],
                             own3[:, :, 2 * at:2 * at + 2].transpose(1, 2))):
                        assert line.shape == mine.shape == (own.shape[0], n2) and line3.shape == mine3.shape == (own.shape[0], 2, 2 * n2)
                        assert torch.allclose(line[:, 1:-1], mine[:, 1:-1], rtol=0, atol=1e-12), (i, name, k)
                        # ... and the two end pixels do differ: the tile's reflection along the other axis reaches them
                        for e, blk in ((0, slice(0, 2)), (-1, slice(2 * n2 - 2, 2 * n2))):
                            assert not torch.allclose(line3[:, :, blk], mine3[:, :, blk], rtol=0, atol=1e-9), (i, name, k, e)
                            end_differs.append(not torch.allclose(line[:, e], mine[:, e], rtol=0, atol=1e-9))
                # the corner patches, reflected along both axes
                for ky, ry in ((0, 0), (1, n2 - 1)):
                    for kx, cx in ((0, 0), (1, n2 - 1)):
                        patch = p2(ys[ends(ky)], xs[ends(kx)])[1]
                        assert patch.shape[1:] == (1, 1)
                        assert torch.allclose(patch[:, 0, 0], own[:, ry, cx], rtol=0, atol=1e-12), (i, ky, kx)
    assert len(end_differs) == 8 * grid.size and 4 * sum(end_differs) >= 3 * len(end_differs), (sum(end_differs), len(end_differs))
    # mirrored edge tiles of the frame and interior tiles were both among them, on every side
    assert seen_edges == {(s, f) for s in ("top", "bottom", "left", "right") for f in (False, True)}


# ---------------------------------------------------------------------------- GPU

@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    from nind_denoise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# S = 68 = 4 * 17: the F(4,3) groups of a windowed level-1 line do not line up with the tile's own.  The shared plan needs a frame
# of at least one tile (W, H >= cs), where the grid still has two columns / rows: W = cs and H = cs are the narrowest and the lowest
# frame it takes -- every tile of them is a mirrored edge tile on both sides
SMALL = [(333, 290, 120, 88, 20), (120, 290, 120, 88, 16), (333, 120, 120, 88, 16), (120, 120, 120, 88, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("geom", SMALL, ids=lambda g: "{}x{}-{}-{}-{}".format(*g))
def test_small_frames_vs_per_tile_and_float64(dev, geom):
    from nind_denoise_amd import pipeline
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol, funit=16)
    assert (p["D"], p["bands"]) == (2, 1)
    if geom == SMALL[0]:
        assert p["S"] % 8 == 4
    net = _net_visible(dev, 16, 9)
    frame = synth.make_frame(W, H, seed=3)
    img = torch.from_numpy(frame).to(dev)
    ref = otiler.denoise_frame(frame, cs, ucs, ol, _model64(_sd64(16, 9)), batch=16)
    shared = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5)
    net.share_encoder = False
    tiled = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5)
    e_sh, e_ti, e_st = _rel(shared, ref), _rel(tiled, ref), _rel(shared, tiled)
    print(f"UtNet(16) gain {VISIBLE_GAIN} {geom}: shared {e_sh:.2e}, per-tile {e_ti:.2e} vs float64; shared vs per-tile {e_st:.2e}")
    assert e_sh <= BAR_FRAME16 and e_ti <= BAR_FRAME16 and e_st <= BAR_SHARED16, (e_sh, e_ti, e_st)


# two bands of 2 and 1 tile rows, 96 tiles per row: the column-edge images of the last band are one tile high
ONE_ROW_LAST_BAND = (13000, 400, 264, 200, 64)


@pytest.mark.gpu
def test_single_row_last_band_vs_per_tile_and_float64(dev):
    from nind_denoise_amd import pipeline
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = ONE_ROW_LAST_BAND
    p = _plan(W, H, cs, ucs, ol)
    assert (p["D"], p["bands"], p["R"], p["rows"]) == (2, 2, 2, 3)
    net = _net_visible(dev, 64, 123)
    frame = synth.make_frame(W, H, seed=24)
    img = torch.from_numpy(frame).to(dev)
    shared = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=256)
    net.share_encoder = False
    tiled = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=256)
    net.share_encoder = True
    e_st = _rel(shared, tiled)
    del tiled
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    picks = _band_samples(p)
    model_fn = _model64(_sd64(64, 123))
    errs = []
    for i in picks:
        y = model_fn(otiler.gather_tile(frame, grid, i)[None])[0]
        cv = torch.zeros_like(img)
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=1, tile_range=(i, i + 1), canvas=cv)
        _, _, ud, (ax, ay) = grid.geom(i)
        ref = otiler.make_seamless_edges(np.array(y[:, ud[1]:ud[3], ud[0]:ud[2]], dtype=np.float32), ax, ay, grid)
        h, w = ref.shape[1:]
        errs.append(_rel(cv[:, ay:ay + h, ax:ax + w], ref))
    net._workspaces.clear()
    worst = max(errs)
    print(f"UtNet(64) gain {VISIBLE_GAIN} {ONE_ROW_LAST_BAND}: sampled tiles {picks} vs float64 worst {worst:.2e} "
          f"(tile {picks[errs.index(worst)]}); canvas shared vs per-tile {e_st:.2e}")
    assert worst <= BAR_TILE64 and e_st <= BAR_SHARED64, (worst, e_st)


@pytest.mark.gpu
@pytest.mark.parametrize("funit,seed,geom,batch,ranges", [
    # 7 x 6 tiles, one band: (8, 12) lies inside tile row 1, (12, 13) and (20, 21) are single tiles
    (16, 4, (500, 430, 120, 88, 16), 6, ((0, 8), (8, 12), (12, 13), (13, 20), (20, 21), (21, 42))),
    # 96 x 3 tiles, seam at 192: (100, 140) inside row 1, (191, 192) / (192, 193) the single tiles on either side of the seam
    (64, 123, ONE_ROW_LAST_BAND, 256, ((0, 100), (100, 140), (140, 191), (191, 192), (192, 193), (193, 250), (250, 288))),
], ids=["500x430-120", "13000x400-264"])
def test_ranges_inside_a_tile_row_and_single_tiles_give_the_same_bits(dev, funit, seed, geom, batch, ranges):
    from nind_denoise_amd import pipeline
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol, funit=funit)
    total = pipeline.tile_count(W, H, cs, ucs, ol)
    assert p["D"] == 2 and ranges[0][0] == 0 and ranges[-1][1] == total and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert any(hi - lo == 1 for lo, hi in ranges) and any(hi - lo > 1 and lo // p["cols"] == (hi - 1) // p["cols"] for lo, hi in ranges)
    net = _net_visible(dev, funit, seed)
    net.split_k = False
    img = torch.from_numpy(synth.make_frame(W, H, seed=8)).to(dev)
    a = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch)
    cv = torch.zeros_like(img)
    for lo, hi in ranges:
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch, tile_range=(lo, hi), canvas=cv)
    assert torch.equal(a, cv)
    net._workspaces.clear()
