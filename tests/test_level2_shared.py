"""Level 2 of the shared encoder (convs3.0, convs3.2, the third pool) in the fused frame loop: once per band of tile rows on the band's
P2, with a tile's P3 border lines from 6-line images at P2 resolution and its P3 corner pixels from 6 x 6 patches of its own P2
(utnet_frame.hip: kLevels, plan_level; UtNet.share_level2 = False keeps level 2 per tile).

CPU: the identity it rests on, in float64 with the oracle's tiler, and a gate proving that the bars reused from
tests/test_shared_encoder.py see a skipped P3 border fix-up.  GPU: the loop against the per-tile path and float64 in conv_w2d
(UtNet(16), one band) and in the three-pass form (UtNet(64), two bands), the geometries on which the plan keeps level 2 per tile, and
the independence of its bits from the launch grouping."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth
from test_edge_strips import K, ONE_ROW_LAST_BAND, _band_axis, _p2_64, _tile_axis
from test_shared_encoder import (BAR_FRAME16, BAR_SHARED16, BAR_SHARED64, BAR_TILE64, VISIBLE_GAIN, _band_samples, _encoder64, _model64,
                                 _net_visible, _plan, _rel, _sd64)

K2 = 6          # kStrip2: P2 lines that yield one P3 line through convs3.0, convs3.2 and the pool


def _levels(W, H, cs, ucs, ol, funit=64, flags=0):
    out = ctypes.c_int(-1)
    _lib.check(_lib.load().nd_utnet_frame_levels(funit, 0, flags, W, H, cs, ucs, ol, ctypes.byref(out)), "nd_utnet_frame_levels")
    return out.value


def _level2_64(sd, p2):
    """Level 2 in float64 on [C, h, w]: (convs3.2's output = the CAT2 skip, P3 = its pool)."""
    x = p2[None]
    for k in (0, 2):
        x = F.prelu(F.conv2d(x, sd[f"convs3.{k}.weight"], sd[f"convs3.{k}.bias"]), sd[f"convs3.{k + 1}.weight"])
    return x[0], F.max_pool2d(x, 2)[0]


# ---------------------------------------------------------------------------- CPU: the identity

@pytest.mark.parametrize("geom,R", [((333, 290, 120, 88, 16), 3), ((300, 170, 136, 56, 24), 4)])   # the second: pad 40 > stride 32
def test_level2_of_a_tile_is_windows_of_the_band_and_its_line_images(geom, R):
    """Every tile of the frame, with bands of R < rows tile rows: the tile's convs3.2 output and P3 equal the band's windows on
    [1, n - 1) to 1e-12; the P3 line of a 6-line image (the tile row's / column's P2 edge line next to the five clean band lines
    inside it), windowed at the tile, equals the tile's P3 border line on pixels 1 ... n3 - 2; level 2 of the 6 x 6 corner patches
    of the tile's assembled P2 gives its four P3 corner pixels.  The end pixels of a windowed line lack the tile's reflection along
    the line: at least 3 in 4 of a frame's end pixels must differ (a 2 x 2 maximum may fall on the clean half of its block)."""
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.make_utnet_state_dict(funit=4, seed=5).items()}
    frame = synth.make_frame(W, H, seed=1).astype(np.float64)
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    S, pad = ucs - ol, grid.pad
    assert S % 8 == 0 and grid.rows > R > 1
    n2 = (cs // 2 - 4) // 2
    n3 = (n2 - 4) // 2
    wx = (grid.cols - 1) * S + cs + 4
    xs_band = _band_axis(-pad - 2, wx, W)

    def p2(ys, xs):
        return _p2_64(sd, torch.from_numpy(frame[:, ys][:, :, xs])[None])[1][0]

    def ends(k):
        return slice(0, K) if k == 0 else slice(cs + 4 - K, cs + 4)

    end_differs = []
    for row0 in range(0, grid.rows, R):
        nrows = min(R, grid.rows - row0)
        ys_band = _band_axis(row0 * S - pad - 2, (nrows - 1) * S + cs + 4, H)
        band2 = p2(ys_band, xs_band)
        band_skip, band3 = _level2_64(sd, band2)
        # two h2 x 6 images per tile column of the band: the column's P2 edge line and the five band columns inside it
        col3 = []
        for xi in range(grid.cols):
            o4 = xi * S // 4
            xs = _tile_axis(xi, S, pad, cs, W)
            left = torch.cat([p2(ys_band, xs[ends(0)]), band2[:, :, o4 + 1:o4 + K2]], 2)
            right = torch.cat([band2[:, :, o4 + n2 - K2:o4 + n2 - 1], p2(ys_band, xs[ends(1)])], 2)
            assert left.shape[1:] == right.shape[1:] == (band2.shape[1], K2)
            col3.append([_level2_64(sd, left)[1], _level2_64(sd, right)[1]])
        for yi in range(row0, row0 + nrows):
            ys = _tile_axis(yi, S, pad, cs, H)
            o4y, o8y = (yi - row0) * S // 4, (yi - row0) * S // 8
            lines2 = [p2(ys[ends(0)], xs_band), p2(ys[ends(1)], xs_band)]
            top = torch.cat([lines2[0], band2[:, o4y + 1:o4y + K2]], 1)
            bottom = torch.cat([band2[:, o4y + n2 - K2:o4y + n2 - 1], lines2[1]], 1)
            assert top.shape[1:] == bottom.shape[1:] == (K2, band2.shape[2])
            row3 = [_level2_64(sd, top)[1], _level2_64(sd, bottom)[1]]
            assert row3[0].shape[1:] == (1, band3.shape[2])
            for xi in range(grid.cols):
                i = yi * grid.cols + xi
                xs = _tile_axis(xi, S, pad, cs, W)
                o4x, o8x = xi * S // 4, xi * S // 8
                own2 = p2(ys, xs)
                own_skip, own3 = _level2_64(sd, own2)
                assert own2.shape[1:] == (n2, n2) and own3.shape[1:] == (n3, n3)
                n = own_skip.shape[-1]
                # interior: windows of the band
                assert torch.allclose(own3[:, 1:-1, 1:-1], band3[:, o8y + 1:o8y + n3 - 1, o8x + 1:o8x + n3 - 1], rtol=0, atol=1e-12), i
                assert torch.allclose(own_skip[:, 1:-1, 1:-1], band_skip[:, o4y + 1:o4y + n - 1, o4x + 1:o4x + n - 1], rtol=0, atol=1e-12), i
                # lines: windows of the line images, except at their end pixels
                for k, at in ((0, 0), (1, n3 - 1)):
                    for name, line, mine in (("row", row3[k][:, 0, o8x:o8x + n3], own3[:, at, :]),
                                             ("col", col3[xi][k][:, o8y:o8y + n3, 0], own3[:, :, at])):
                        assert line.shape == mine.shape == (own3.shape[0], n3)
                        assert torch.allclose(line[:, 1:-1], mine[:, 1:-1], rtol=0, atol=1e-12), (i, name, k)
                        end_differs += [not torch.allclose(line[:, e], mine[:, e], rtol=0, atol=1e-9) for e in (0, -1)]
                # corners: the tile's P2 as the loop assembles it (band window, edge lines, corner patches), then its 6 x 6 corners
                asm = band2[:, o4y:o4y + n2, o4x:o4x + n2].clone()
                for k, at in ((0, 0), (1, n2 - 1)):
                    asm[:, at, :] = lines2[k][:, 0, o4x:o4x + n2]
                    asm[:, :, at] = p2(ys_band, xs[ends(k)])[:, o4y:o4y + n2, 0]
                for ky, ry in ((0, 0), (1, n2 - 1)):
                    for kx, cx in ((0, 0), (1, n2 - 1)):
                        asm[:, ry, cx] = p2(ys[ends(ky)], xs[ends(kx)])[:, 0, 0]
                assert torch.allclose(asm, own2, rtol=0, atol=1e-12), i
                for ky, ry in ((0, 0), (1, n3 - 1)):
                    for kx, cx in ((0, 0), (1, n3 - 1)):
                        py, px = ky * (n2 - K2), kx * (n2 - K2)
                        patch = _level2_64(sd, asm[:, py:py + K2, px:px + K2])[1]
                        assert patch.shape[1:] == (1, 1)
                        assert torch.allclose(patch[:, 0, 0], own3[:, ry, cx], rtol=0, atol=1e-12), (i, ky, kx)
    assert len(end_differs) == 8 * grid.size and 4 * sum(end_differs) >= 3 * len(end_differs), (sum(end_differs), len(end_differs))


# ---------------------------------------------------------------------------- the frames of the GPU tests and what their bars see
# UtNet(16) seed 9 / make_frame seed 3, one band (level 2 in conv_w2d); all have crop 32, 8 | S and W, H >= cs.  The second and the
# third: the narrowest and the lowest frame the plan takes; the last: pad 40 > stride 32
ONE_BAND = [(333, 290, 120, 56, 16), (120, 290, 120, 56, 16), (333, 120, 120, 56, 16), (300, 170, 136, 56, 24)]
# level 2 stays per tile: S = 36 (a tile origin is no whole P3 pixel); crop 16 (tconvs2.0 reads line 0 of its skip)
FALLBACK = [(333, 290, 120, 52, 16), (333, 290, 120, 88, 16)]


def _utnet64_p3(sd, xp, p3_lines=None):
    """oracle.networks.utnet_forward on an already reflect-padded input, with P3's rows / cols 0 and n-1 optionally replaced."""
    from oracle import networks as onet

    def act(k, t):
        return onet._act(sd, k, t, "PReLU")

    def enc(n, t):
        t = act(f"{n}.1", F.conv2d(t, sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]))
        return act(f"{n}.3", F.conv2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    def dec(n, t):
        t = act(f"{n}.1", F.conv_transpose2d(t, sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]))
        return act(f"{n}.3", F.conv_transpose2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    def up(n, t):
        return F.conv_transpose2d(t, sd[f"{n}.weight"], sd[f"{n}.bias"], stride=2)

    l1 = enc("convs1", xp)
    l2 = enc("convs2", F.max_pool2d(l1, 2))
    l3 = enc("convs3", F.max_pool2d(l2, 2))
    p3 = F.max_pool2d(l3, 2)
    if p3_lines is not None:
        p3 = p3.clone()
        p3[:, :, [0, -1], :] = p3_lines[:, :, [0, -1], :]
        p3[:, :, :, [0, -1]] = p3_lines[:, :, :, [0, -1]]
    l4 = enc("convs4", p3)
    b = F.max_pool2d(l4, 2)
    b = act("bottom.1", F.conv2d(b, sd["bottom.0.weight"], sd["bottom.0.bias"]))
    b = act("bottom.3", F.conv_transpose2d(b, sd["bottom.2.weight"], sd["bottom.2.bias"]))
    l = torch.cat([up("up1", b), l4], 1)
    l = torch.cat([up("up2", dec("tconvs1", l)), l3], 1)
    l = torch.cat([up("up3", dec("tconvs2", l)), l2], 1)
    l = torch.cat([up("up4", dec("tconvs3", l)), l1], 1)
    l = dec("tconvs4", l)
    return F.conv2d(l, sd["tconvs4.4.weight"], sd["tconvs4.4.bias"])[:, :, 2:-2, 2:-2]


def _p3_fixup_sensitivity(funit, seed, geom, frame_seed):
    """Change of the kept output, relative to max(1, max |y|), of the middle tile of the frame when P3's border lines are taken from
    the frame window as the band holds them, i.e. the level-2 fix-up skipped."""
    from oracle import networks as onet
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    sd = _sd64(funit, seed)
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    S, pad = ucs - ol, grid.pad
    frame = synth.make_frame(W, H, seed=frame_seed).astype(np.float64)
    yi, xi = grid.rows // 2, grid.cols // 2
    ys_t, xs_t = _tile_axis(yi, S, pad, cs, H), _tile_axis(xi, S, pad, cs, W)
    ys_b, xs_b = _band_axis(yi * S - pad - 2, cs + 4, H), _band_axis(xi * S - pad - 2, cs + 4, W)
    xp = torch.from_numpy(frame[:, ys_t][:, :, xs_t])[None]
    win = torch.from_numpy(frame[:, ys_b][:, :, xs_b])[None]
    crop = (cs - ucs) // 2

    def kept(y):
        return y[:, :, crop:cs - crop, crop:cs - crop]
    y = _utnet64_p3(sd, xp)
    assert torch.equal(y, onet.utnet_forward(sd, xp[:, :, 2:-2, 2:-2]))       # the restatement above is the oracle's network
    p3_band = F.max_pool2d(_encoder64(sd, win)[2], 2)
    return (kept(_utnet64_p3(sd, xp, p3_band)) - kept(y)).abs().max().item() / max(1.0, kept(y).abs().max().item())


GATE_CASES = ([(16, 9, g, 3, (BAR_FRAME16, BAR_SHARED16)) for g in ONE_BAND] +
              [(64, 123, ONE_ROW_LAST_BAND, 24, (BAR_TILE64, BAR_SHARED64))])


@pytest.mark.parametrize("case", GATE_CASES, ids=lambda c: "f{}-{}x{}-{}-{}-{}".format(c[0], *c[2]))
def test_gpu_bars_see_a_skipped_p3_fixup(case):
    """The bars of the GPU tests below are those of tests/test_shared_encoder.py; by its rule each must lie 10x below what the fault
    does to the kept output: here P3's border lines left as the band holds them.  Measured in float64 at VISIBLE_GAIN:
    UtNet(16) seed 9: 9.15e-05 on (333, 290, 120, 56, 16), 1.39e-04 on (120, 290, 120, 56, 16), 7.40e-05 on (333, 120, 120, 56, 16),
    8.05e-05 on (300, 170, 136, 56, 24), against bars of 2e-6; UtNet(64) seed 123: 9.10e-05 on (13000, 400, 264, 200, 64), against
    bars of 8e-6."""
    funit, seed, geom, frame_seed, bars = case
    v = _p3_fixup_sensitivity(funit, seed, geom, frame_seed)
    print(f"UtNet({funit}) seed {seed} {geom}: skipped P3 fix-up {v:.2e}, bars {bars}")
    assert v >= 10 * max(bars), (v, bars)


# ---------------------------------------------------------------------------- GPU

@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref16():
    """float64 canvases of the UtNet(16) frames, computed once per geometry."""
    from oracle import tiler as otiler
    cache = {}

    def get(geom):
        if geom not in cache:
            W, H, cs, ucs, ol = geom
            cache[geom] = otiler.denoise_frame(synth.make_frame(W, H, seed=3), cs, ucs, ol, _model64(_sd64(16, 9)), batch=16)
        return cache[geom]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ONE_BAND, ids=lambda g: "{}x{}-{}-{}-{}".format(*g))
def test_one_band_frame_vs_per_tile_and_float64(dev, ref16, geom):
    from nind_denoise_amd import pipeline
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol, funit=16)
    assert (p["D"], p["bands"]) == (2, 1) and p["S"] % 8 == 0 and (cs - ucs) // 2 >= 32
    assert _levels(W, H, cs, ucs, ol, funit=16) == 3
    assert _levels(W, H, cs, ucs, ol, funit=16, flags=_lib.FLAG_TILE_LEVEL2) == 2
    net = _net_visible(dev, 16, 9)
    img = torch.from_numpy(synth.make_frame(W, H, seed=3)).to(dev)
    ref = ref16(geom)
    shared = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5)
    net.share_encoder = False
    tiled = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5)
    e_sh, e_ti, e_st = _rel(shared, ref), _rel(tiled, ref), _rel(shared, tiled)
    print(f"UtNet(16) gain {VISIBLE_GAIN} {geom}: shared {e_sh:.2e}, per-tile {e_ti:.2e} vs float64; shared vs per-tile {e_st:.2e}")
    assert e_sh <= BAR_FRAME16 and e_ti <= BAR_FRAME16 and e_st <= BAR_SHARED16, (e_sh, e_ti, e_st)


@pytest.mark.gpu
def test_two_bands_three_pass_vs_per_tile_and_float64(dev):
    """UtNet(64): level 2 runs in the three-pass F(6x6) form; a seam, and a last band of one tile row."""
    from nind_denoise_amd import pipeline
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = ONE_ROW_LAST_BAND
    p = _plan(W, H, cs, ucs, ol)
    assert (p["D"], p["bands"], p["R"], p["rows"]) == (2, 2, 2, 3) and _levels(W, H, cs, ucs, ol) == 3
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
@pytest.mark.parametrize("geom", FALLBACK, ids=lambda g: "{}x{}-{}-{}-{}".format(*g))
def test_plan_keeps_level2_per_tile(dev, geom):
    from nind_denoise_amd import pipeline
    W, H, cs, ucs, ol = geom
    assert _plan(W, H, cs, ucs, ol, funit=16)["D"] == 2 and _levels(W, H, cs, ucs, ol, funit=16) == 2
    net = _net_visible(dev, 16, 9)
    img = torch.from_numpy(synth.make_frame(W, H, seed=3)).to(dev)
    on = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5)
    net.share_level2 = False
    off = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5)
    assert torch.isfinite(on).all() and on.abs().max().item() > 0 and torch.equal(on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("funit,seed,geom,ranges", [
    # 8 x 7 tiles, one band: (9, 14) lies inside tile row 1, (14, 15) is a single tile
    (16, 9, ONE_BAND[0], ((0, 9), (9, 14), (14, 15), (15, 40), (40, 56))),
    # 96 x 3 tiles, seam at 192: (100, 140) inside row 1, (191, 192) / (192, 193) the single tiles on either side of the seam
    (64, 123, ONE_ROW_LAST_BAND, ((0, 100), (100, 140), (140, 191), (191, 192), (192, 193), (193, 250), (250, 288))),
], ids=["333x290-120", "13000x400-264"])
def test_bits_independent_of_batch_and_tile_range(dev, funit, seed, geom, ranges):
    from nind_denoise_amd import pipeline
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol, funit=funit)
    total = pipeline.tile_count(W, H, cs, ucs, ol)
    seams = [b * p["R"] * p["cols"] for b in range(1, p["bands"])]
    assert _levels(W, H, cs, ucs, ol, funit=funit) == 3 and ranges[0][0] == 0 and ranges[-1][1] == total
    assert all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    assert any(hi - lo == 1 for lo, hi in ranges) and any(hi - lo > 1 and lo // p["cols"] == (hi - 1) // p["cols"] for lo, hi in ranges)
    assert all((t - 1, t) in ranges and (t, t + 1) in ranges for t in seams)
    net = _net_visible(dev, funit, seed)
    net.split_k = False
    img = torch.from_numpy(synth.make_frame(W, H, seed=8)).to(dev)
    a = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=256)
    for batch in (1, 4, 11, 64):
        assert torch.equal(a, pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch)), batch
    cv = torch.zeros_like(img)
    for lo, hi in ranges:
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=64, tile_range=(lo, hi), canvas=cv)
    assert torch.equal(a, cv)
    net._workspaces.clear()
