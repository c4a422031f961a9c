"""Shared encoder of the fused frame loop (nd_utnet_denoise_frame): the first encoder levels run once per band of tile rows.

CPU: the translation-equivariance argument it rests on (float64, oracle layers), the host-only band plan, and a gate proving that
the GPU bars below can see an error in the deep levels or in the P2 border fix-up.  GPU: the shared loop against the per-tile
encoder (UtNet.share_encoder = False) and the oracle (fp32 and float64), single- and multi-band, its independence of launch grouping,
and the per-tile modes nd_utnet_denoise_frame falls back to."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth


def _encoder64(sd, x):
    """Encoder skips (convs1 ... convs4 outputs) of UtNet in float64: valid 3x3 convs, PReLU, 2x2 max-pools."""
    skips = []
    for lv in range(1, 5):
        for k in (0, 2):
            p = f"convs{lv}.{k}"
            x = F.prelu(F.conv2d(x, sd[p + ".weight"], sd[p + ".bias"]), sd[f"convs{lv}.{k + 1}.weight"])
        skips.append(x)
        x = F.max_pool2d(x, 2)
    return skips


@pytest.mark.parametrize("geom", [(333, 290, 120, 88, 16), (300, 170, 136, 56, 24)])   # the second: pad 40 > stride 32
def test_tile_encoder_is_a_window_of_the_frame_encoder(geom):
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    sd = {k: torch.from_numpy(np.asarray(v)).double() for k, v in synth.make_utnet_state_dict(funit=4, seed=5).items()}
    frame = synth.make_frame(W, H, seed=1).astype(np.float64)
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    S, pad = ucs - ol, grid.pad
    x1pad = (grid.cols - 1) * S - pad + cs - W
    y1pad = (grid.rows - 1) * S - pad + cs - H
    padded = np.pad(frame, ((0, 0), (pad + 2, y1pad + 2), (pad + 2, x1pad + 2)), mode="symmetric")
    big = _encoder64(sd, torch.from_numpy(padded)[None])
    for i in range(grid.size):
        tile = otiler.gather_tile(frame.astype(np.float32), grid, i).astype(np.float64)
        x0, y0, _, _ = grid.geom(i)
        # every gathered tile is its window of the symmetric-padded frame, mirrored edge tiles included
        assert np.array_equal(tile, padded[:, y0 + pad + 2:y0 + pad + 2 + cs, x0 + pad + 2:x0 + pad + 2 + cs])
        small = _encoder64(sd, F.pad(torch.from_numpy(tile)[None], (2, 2, 2, 2), mode="reflect"))
        for lv, (a, b) in enumerate(zip(small, big)):
            step = 2 ** lv
            assert S % step == 0
            oy, ox = (y0 + pad) // step, (x0 + pad) // step
            n = a.shape[-1]
            win = b[0, :, oy:oy + n, ox:ox + n]
            e = 2 if lv == 0 else 1       # lines the tile's own ReflectionPad2d(2) reaches
            assert torch.allclose(a[0, :, e:n - e, e:n - e], win[:, e:n - e, e:n - e], rtol=0, atol=1e-12), (i, lv)
            # ... and those lines do differ: they must be recomputed per tile
            assert not torch.allclose(a[0], win, rtol=0, atol=1e-9), (i, lv)


def _plan(W, H, cs, ucs, ol, funit=64, dtype=0, flags=0):
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.load().nd_utnet_frame_plan(funit, dtype, flags, W, H, cs, ucs, ol, out), "nd_utnet_frame_plan")
    return dict(zip(("D", "aligned", "R", "bands", "S", "cols", "rows", "hx"), list(out)))


@pytest.mark.parametrize("geom", [(6000, 4000, 264, 200, 64), (6000, 4000, 520, 496, 22), (333, 290, 120, 88, 16),
                                  (300, 170, 136, 56, 24), (500, 430, 120, 88, 18), (6000, 4000, 520, 456, 64)])
def test_frame_plan_matches_restatement(geom):
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol)
    S = ucs - ol
    grid_cols, grid_rows = math.ceil((W - ucs) / S) + 1, math.ceil((H - ucs) / S) + 1
    aligned = 1
    while aligned < 4 and S % (2 ** aligned) == 0:
        aligned += 1
    assert (p["S"], p["cols"], p["rows"], p["aligned"]) == (S, grid_cols, grid_rows, aligned)
    assert p["D"] == (2 if S % 4 == 0 else 0)
    if p["D"]:
        assert 1 <= p["R"] <= grid_rows and p["bands"] == math.ceil(grid_rows / p["R"])
        assert p["R"] == math.ceil(grid_rows / p["bands"])          # near-equal bands
        assert p["hx"] == (p["R"] - 1) * S + cs + 4
    # the plan is a function of the geometry: no batch argument; the per-tile modes keep the whole encoder per tile
    for flags in (_lib.FLAG_TILE_ENCODER, _lib.FLAG_FULL_TILES, _lib.FLAG_DIRECT_CONV, _lib.FLAG_W1D_REGS):
        assert _plan(W, H, cs, ucs, ol, flags=flags)["D"] == 0
    assert _plan(W, H, cs, ucs, ol, dtype=_lib.ND_BF16)["D"] == 0
    if geom[:5] == (6000, 4000, 264, 200, 64):
        assert (p["D"], p["aligned"]) == (2, 4)      # G24: levels 0-3 aligned (136 = 8 * 17), pool 4 per tile
    if geom[:5] == (6000, 4000, 520, 496, 22):
        assert p["D"] == 0                           # G24d: stride 474, the level-2 pool phase differs between tiles
    lib = _lib.load()
    nb = lib.nd_utnet_frame_workspace_bytes(64, 0, 0, W, H, cs, ucs, ol, 8)
    assert (nb > 0) == (p["D"] > 0)


# ---------------------------------------------------------------------------- visible weights and the bars they support
# With synth's default gain 1.0 the activations shrink with depth: a 1 % error on the input of level 2 (P2) or below moves the
# output by < 2e-8, far under any fp32 bar.  At VISIBLE_GAIN the output is O(1) and every level reaches it (figures below).
VISIBLE_GAIN = 2.2

# fp32 bars of the GPU tests at VISIBLE_GAIN, on max |error| / max(1, max |reference|).  test_gpu_bars_see_deep_levels_and_fixup
# requires each to be 10x below what a 1 % error on a level-1 ... level-4 input (and, with the shared encoder, a skipped P2 border
# fix-up) does to the kept output of that test's geometry and weights.  Worst values measured on MI355X in the comments; torch fp32 on
# the CPU against float64 gives 5e-7 (UtNet(16)) and 1e-6 (UtNet(64)) on the same tiles.
BAR_FRAME16 = 2e-6     # UtNet(16) frame canvas vs float64: shared, per-tile and the D = 0 fp32 modes (measured 7.0e-7)
BAR_SHARED16 = 2e-6    # UtNet(16) frame canvas, shared vs per-tile encoder (measured 6.5e-7)
BAR_TILE64 = 8e-6      # UtNet(64) multi-band frames, sampled tiles run alone vs float64 (measured 2.7e-6)
BAR_SHARED64 = 8e-6    # UtNet(64) multi-band frames, whole canvas shared vs per-tile encoder (measured 2.4e-6)
BAR_NET64 = 8e-6       # UtNet(64) forward of whole tiles vs float64 (test_hip_parity: Winograd remainders, wide tiles; measured 2.4e-6)

# frames the GPU tests run at VISIBLE_GAIN: (W, H, cs, ucs, ol), UtNet(16) seed 9 / UtNet(64) seed 123, make_frame seed 3 / 24
SINGLE_BAND = [(333, 290, 120, 88, 16), (500, 430, 120, 88, 16), (300, 170, 136, 56, 24)]   # the last: pad 40 > stride 32
# multi-band: (geometry, (bands, rows per band)) -- G24 (short last band), two bands, the CLI default tiling (1-row last band)
MULTI_BAND = [((6000, 4000, 264, 200, 64), (5, 6)), ((3000, 2000, 264, 200, 64), (2, 8)), ((6000, 4000, 504, 480, 24), (5, 2))]
PER_TILE_FP32 = (333, 290, 120, 88, 18)   # S = 70: a stride not divisible by 4 (G24d-type), D = 0


def _sd64(funit, seed, gain=VISIBLE_GAIN):
    return {k: torch.as_tensor(v).double() for k, v in synth.make_utnet_state_dict(funit=funit, seed=seed, gain=gain).items()}


def _utnet64(sd, xp, scale=(1.0, 1.0, 1.0, 1.0), p2_lines=None):
    """oracle.networks.utnet_forward on an already reflect-padded input, with the input of level 1 ... 4 (pooled convs1 ...
    convs4 outputs; level 2's is P2) scaled by scale[0 ... 3], and P2's rows / cols 0 and n-1 optionally replaced."""
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
    l2 = enc("convs2", F.max_pool2d(l1, 2) * scale[0])
    p2 = F.max_pool2d(l2, 2)
    if p2_lines is not None:
        p2 = p2.clone()
        p2[:, :, [0, -1], :] = p2_lines[:, :, [0, -1], :]
        p2[:, :, :, [0, -1]] = p2_lines[:, :, :, [0, -1]]
    l3 = enc("convs3", p2 * scale[1])
    l4 = enc("convs4", F.max_pool2d(l3, 2) * scale[2])
    b = F.max_pool2d(l4, 2) * scale[3]
    b = act("bottom.1", F.conv2d(b, sd["bottom.0.weight"], sd["bottom.0.bias"]))
    b = act("bottom.3", F.conv_transpose2d(b, sd["bottom.2.weight"], sd["bottom.2.bias"]))
    l = torch.cat([up("up1", b), l4], 1)
    l = torch.cat([up("up2", dec("tconvs1", l)), l3], 1)
    l = torch.cat([up("up3", dec("tconvs2", l)), l2], 1)
    l = torch.cat([up("up4", dec("tconvs3", l)), l1], 1)
    l = dec("tconvs4", l)
    return F.conv2d(l, sd["tconvs4.4.weight"], sd["tconvs4.4.bias"])[:, :, 2:-2, 2:-2]


def _sensitivity(funit, seed, geom, frame_seed, crop, fixup):
    """Change of the kept output (the tile less `crop` on each side), relative to max(1, max |y|), of one interior tile of the frame:
    a 1 % error on each of the level-1 ... level-4 inputs, and (fixup) P2's border lines taken from the frame window as the band
    holds them, i.e. the fix-up skipped."""
    from oracle import networks as onet
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    sd = _sd64(funit, seed)
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    x0, y0, _, _ = grid.geom((grid.rows // 2) * grid.cols + grid.cols // 2)
    assert x0 >= 2 and y0 >= 2 and x0 + cs + 2 <= W and y0 + cs + 2 <= H
    frame = synth.make_frame(W, H, seed=frame_seed)
    win = torch.from_numpy(frame[:, y0 - 2:y0 + cs + 2, x0 - 2:x0 + cs + 2].astype(np.float64))[None]
    tile = win[:, :, 2:-2, 2:-2]
    xp = F.pad(tile, (2, 2, 2, 2), mode="reflect")

    def kept(y):
        return y[:, :, crop:cs - crop, crop:cs - crop]
    y = _utnet64(sd, xp)
    assert torch.equal(y, onet.utnet_forward(sd, tile))       # the restatement above is the oracle's network
    scale = max(1.0, kept(y).abs().max().item())
    out = {}
    for lv in range(4):
        s = [1.0] * 4
        s[lv] = 1.01
        out[f"level{lv + 1}"] = (kept(_utnet64(sd, xp, s)) - kept(y)).abs().max().item() / scale
    if fixup:
        p2_band = F.max_pool2d(_encoder64(sd, win)[1], 2)
        out["fixup"] = (kept(_utnet64(sd, xp, p2_lines=p2_band)) - kept(y)).abs().max().item() / scale
    return out


# (funit, seed, frame geometry, make_frame seed, crop, shared encoder, bars of the GPU tests that run these weights there).  The
# whole-tile bar BAR_NET64 (crop 0) is gated at cs = 152 with the Winograd remainder test's weights (seed 7), and with the wide-tile
# test's weights (seed 123) on the cs = 504 frame geometry, whose kept region is a subset of the whole tile.
GATE_CASES = ([(16, 9, g, 3, (g[2] - g[3]) // 2, True, (BAR_FRAME16, BAR_SHARED16)) for g in SINGLE_BAND] +
              [(16, 9, PER_TILE_FP32, 3, (PER_TILE_FP32[2] - PER_TILE_FP32[3]) // 2, False, (BAR_FRAME16,))] +
              [(64, 123, g, 24, (g[2] - g[3]) // 2, True, (BAR_TILE64, BAR_SHARED64) + ((BAR_NET64,) if g[2] == 504 else ()))
               for g, _ in MULTI_BAND] +
              [(64, 7, (456, 456, 152, 120, 16), 7, 0, False, (BAR_NET64,))])


@pytest.mark.parametrize("case", GATE_CASES, ids=lambda c: "f{}-{}x{}-{}-{}-{}-crop{}".format(c[0], *c[2], c[4]))
def test_gpu_bars_see_deep_levels_and_fixup(case):
    funit, seed, geom, frame_seed, crop, shared, bars = case
    fig = _sensitivity(funit, seed, geom, frame_seed, crop, shared)
    print(f"UtNet({funit}) seed {seed} {geom}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    for k, v in fig.items():
        assert v >= 10 * max(bars), (k, v, bars)


# ---------------------------------------------------------------------------- GPU

@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _net(dev, funit=16, seed=9):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=funit)
    net.load_state_dict(synth.make_utnet_state_dict(funit=funit, seed=seed))
    return net.eval().to(dev)


@pytest.mark.gpu
def test_shared_encoder_matches_per_tile_and_oracle(dev):
    from nind_denoise_amd import pipeline
    from oracle import networks as onet
    from oracle import tiler as otiler
    sd = synth.make_utnet_state_dict(funit=16, seed=9)
    net = _net(dev)
    W, H, cs, ucs, ol = 333, 290, 120, 88, 16
    assert _plan(W, H, cs, ucs, ol, funit=16)["D"] == 2
    frame = synth.make_frame(W, H, seed=3)
    img = torch.from_numpy(frame).to(dev)

    def model_fn(x):
        with torch.no_grad():
            return onet.utnet_forward(sd, torch.from_numpy(x)).numpy()

    ref = torch.from_numpy(otiler.denoise_frame(frame, cs, ucs, ol, model_fn, batch=4))
    shared = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5).cpu()
    net.share_encoder = False
    tiled = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5).cpu()
    net.share_encoder = True
    scale = ref.abs().max().item()
    assert (shared - ref).abs().max().item() <= 2e-5 * max(1.0, scale)
    assert (shared - tiled).abs().max().item() <= 2e-6 * max(1.0, scale)
    # progress: one call per launch, ascending, covering the range
    seen = []
    pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5, progress=lambda n, t0, cnt: seen.append((n, t0, cnt)))
    assert [s[0] for s in seen] == list(range(len(seen)))
    assert seen[0][1] == 0 and all(a[1] + a[2] == b[1] for a, b in zip(seen, seen[1:]))
    assert seen[-1][1] + seen[-1][2] == pipeline.tile_count(W, H, cs, ucs, ol) and max(s[2] for s in seen) <= 5


@pytest.mark.gpu
def test_shared_encoder_bits_independent_of_grouping(dev):
    from nind_denoise_amd import pipeline
    net = _net(dev, seed=4)
    net.split_k = False
    W, H, cs, ucs, ol = 500, 430, 120, 88, 16        # 7 x 6 tiles: the plan's bands hold whole rows of 7
    img = torch.from_numpy(synth.make_frame(W, H, seed=8)).to(dev)
    total = pipeline.tile_count(W, H, cs, ucs, ol)
    a = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=6)
    for batch in (1, 4, 11, 64):
        assert torch.equal(a, pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch)), batch
    # ranges that start and end mid-row, launch by launch on one canvas (the canvas order of the stitch is kept)
    cv = torch.zeros_like(img)
    for lo, hi in ((0, 3), (3, 17), (17, 18), (18, 30), (30, total)):
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=5, tile_range=(lo, hi), canvas=cv)
    assert torch.equal(a, cv)


@pytest.mark.gpu
def test_shared_encoder_g24_frame(dev):
    from nind_denoise_amd import pipeline
    net = _net(dev, funit=64, seed=123)
    W, H, cs, ucs, ol = 6000, 4000, 264, 200, 64
    img = torch.from_numpy(synth.make_frame(W, H, seed=24)).to(dev)
    a = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=256)
    net.share_encoder = False
    b = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=256)
    err = (a - b).abs().max().item()
    assert torch.isfinite(a).all() and err <= 1e-5 * max(1.0, b.abs().max().item()), err
    net._workspaces.clear()


# ---------------------------------------------------------------------------- GPU, visible weights, against float64

def _net_visible(dev, funit, seed):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=funit)
    net.load_state_dict(synth.make_utnet_state_dict(funit=funit, seed=seed, gain=VISIBLE_GAIN))
    return net.eval().to(dev)


def _model64(sd):
    from oracle import networks as onet

    def model_fn(x):
        with torch.no_grad():
            return onet.utnet_forward(sd, torch.from_numpy(x).double()).numpy()
    return model_fn


def _rel(a, ref):
    """max |a - ref| / max(1, max |ref|) of two canvases (GPU or CPU tensors, numpy arrays)."""
    a, ref = torch.as_tensor(a).double().cpu(), torch.as_tensor(ref).double().cpu()
    assert torch.isfinite(a).all()
    return (a - ref).abs().max().item() / max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("geom", SINGLE_BAND, ids=lambda g: "{}x{}-{}-{}-{}".format(*g))
def test_single_band_frame_vs_float64(dev, geom):
    from nind_denoise_amd import pipeline
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol, funit=16)
    assert (p["D"], p["bands"]) == (2, 1)
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


def _band_samples(p):
    """Tiles of a multi-band frame worth a float64 check: the four corners, the first and last tile of both rows at every band seam
    (the last band's first row among them), and a bottom-edge tile between the corners."""
    cols, rows, R = p["cols"], p["rows"], p["R"]
    picks = {0, cols - 1, (rows - 1) * cols, rows * cols - 1, (rows - 1) * cols + cols // 2}
    for b in range(1, p["bands"]):
        for r in (b * R - 1, b * R):
            picks |= {r * cols, r * cols + cols - 1}
    return sorted(picks)


@pytest.mark.gpu
@pytest.mark.parametrize("geom,bands", MULTI_BAND, ids=["{}x{}-{}-{}-{}".format(*g) for g, _ in MULTI_BAND])
def test_multi_band_frame_vs_float64(dev, geom, bands):
    from nind_denoise_amd import pipeline
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol)
    assert (p["D"], p["bands"], p["R"]) == (2, *bands)
    last = p["rows"] - (p["bands"] - 1) * p["R"]
    assert 1 <= last < p["R"]                     # every case has a short last band
    net = _net_visible(dev, 64, 123)
    frame = synth.make_frame(W, H, seed=24)
    img = torch.from_numpy(frame).to(dev)
    batch = 256 if cs <= 264 else 64
    shared = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch)
    net.share_encoder = False
    tiled = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch)
    net.share_encoder = True
    e_st = _rel(shared, tiled)
    del tiled
    # sampled tiles, each run alone on a zero canvas, against the oracle's stitch of its float64 output
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
        got = cv[:, ay:ay + h, ax:ax + w].clone()
        cv[:, ay:ay + h, ax:ax + w] = 0
        assert not cv.any(), i                    # nothing outside the tile's useful region
        errs.append(_rel(got, ref))
    net._workspaces.clear()
    worst = max(errs)
    print(f"UtNet(64) gain {VISIBLE_GAIN} {geom}, {p['bands']} bands of {p['R']} rows (last {last}): sampled tiles {picks} "
          f"vs float64 worst {worst:.2e} (tile {picks[errs.index(worst)]}); canvas shared vs per-tile {e_st:.2e}")
    assert worst <= BAR_TILE64 and e_st <= BAR_SHARED64, (worst, e_st)


@pytest.mark.gpu
@pytest.mark.parametrize("geom,batches,ranges", [
    ((3000, 2000, 264, 200, 64), (256, 1, 11, 64), ((0, 3), (3, 170), (170, 190), (190, 309), (309, 330))),   # seam at 176
    ((6000, 4000, 504, 480, 24), (32, 1, 7), ((0, 5), (5, 33), (33, 100), (100, 112), (112, 126))),            # seams 28, 56, 84, 112
], ids=["3000x2000-264", "6000x4000-504"])
def test_multi_band_bits_independent_of_grouping(dev, geom, batches, ranges):
    from nind_denoise_amd import pipeline
    W, H, cs, ucs, ol = geom
    p = _plan(W, H, cs, ucs, ol)
    total = pipeline.tile_count(W, H, cs, ucs, ol)
    seams = [b * p["R"] * p["cols"] for b in range(1, p["bands"])]
    assert p["D"] == 2 and p["bands"] > 1 and ranges[-1][1] == total
    assert ranges[-1][0] >= seams[-1] and any(lo < t < hi for lo, hi in ranges for t in seams)   # the short last band alone; a seam crossed
    net = _net_visible(dev, 64, 123)
    net.split_k = False
    img = torch.from_numpy(synth.make_frame(W, H, seed=24)).to(dev)
    a = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batches[0])
    for batch in batches[1:]:
        assert torch.equal(a, pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch)), batch
    # ranges that start and end mid-row and cross band seams, launch by launch on one canvas
    cv = torch.zeros_like(img)
    for lo, hi in ranges:
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batches[0], tile_range=(lo, hi), canvas=cv)
    assert torch.equal(a, cv)
    net._workspaces.clear()


# 16-bit storage against float64 at VISIBLE_GAIN: PSNR over the canvas, peak = the reference's range (measured 64.3 / 82.8 dB)
PSNR_FRAME16 = {"bf16": 61.0, "f16": 79.0}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bf16", "f16", "stride", "tile_encoder"])
def test_per_tile_frame_modes_vs_float64(dev, mode):
    # the modes in which nd_utnet_denoise_frame runs every tile's whole encoder (plan D = 0)
    from nind_denoise_amd import pipeline
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = PER_TILE_FP32 if mode == "stride" else SINGLE_BAND[0]
    net = _net_visible(dev, 16, 9)
    dtype = mode if mode in ("bf16", "f16") else "f32"
    net.set_compute_dtype(dtype)
    net.share_encoder = mode != "tile_encoder"
    assert _plan(W, H, cs, ucs, ol, funit=16, dtype=_lib.DTYPE[dtype], flags=net.flags)["D"] == 0
    frame = synth.make_frame(W, H, seed=3)
    ref = otiler.denoise_frame(frame, cs, ucs, ol, _model64(_sd64(16, 9)), batch=16)
    y = pipeline.denoise_frame(net, torch.from_numpy(frame).to(dev), cs, ucs, ol, batch=5).cpu().numpy()
    e = _rel(y, ref)
    if dtype == "f32":
        print(f"UtNet(16) gain {VISIBLE_GAIN} {mode} {(W, H, cs, ucs, ol)}: vs float64 {e:.2e}")
        assert e <= BAR_FRAME16, e
    else:
        psnr = 10 * np.log10(float(ref.max() - ref.min()) ** 2 / max(float(np.mean((y.astype(np.float64) - ref) ** 2)), 1e-30))
        print(f"UtNet(16) gain {VISIBLE_GAIN} {mode} {(W, H, cs, ucs, ol)}: PSNR {psnr:.1f} dB vs float64, max abs err {e:.2e}")
        assert psnr >= PSNR_FRAME16[dtype], psnr
