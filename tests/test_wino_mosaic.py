"""Mosaic tile grids of the three-pass F(6x6,3x3) layers (csrc/winograd.hip: nd_wino_mosaic, k_wino_in2 / k_wino_out2 in mosaic mode).

A launch of B images of a ConvTranspose2d(3) layer with p x p outputs lays ONE tile grid over by rows of bx images at pitch p
instead of B grids of ceil(p / 6)^2 tiles; the two zero border lines behind an image are the two in front of its neighbour, so the
mosaic's transposed convolution is the per-image results side by side.  UtNet.mosaic_wino = False / ND_FLAG_TILE_WINO keeps the
per-image grids, and so does ND_FLAG_NO_SPLITK (a tile's place in a mosaic depends on which images share its launch).

Host: the planner.  GPU, layer level: the three-pass layer entry point (nd_layer_forward_winograd, tile code 6; the helper is the
body of test_layer_winograd in tests/test_hip_parity.py, restated here) on convT3 32 -> 16 PReLU layers with inputs of 6, 9, 11 and
26 pixels (p = 8, the smallest pitch the kernels take, 11, 13, 28) and batches of 2, 5, 7 (prime: empty slots or a strip) and 16.
The rule takes the mosaic at p = 8 and p = 13 for every one of these batches; at p = 11 and p = 28 it saves less than a tenth of
the tiles at these batch sizes and the launch stays per image -- those cases pin that the decision is taken without harm; p = 28,
the pitch of tconvs1.0 at cs 264, runs the mosaic kernels at B = 24 (6 x 4 images) in a case of its own.
Bars, from test_layer_winograd: against torch in float64 the three-pass form must be within ABS_TOL = 1e-3 and within
REL_TOL = 1e-3 of max |reference| (assert_close there); two forms of the same layer agree within 1e-4 * max(1, max |reference|).
The layer entry point writes a compact (border-free) output; a store outside an image's valid pixels there lands in a neighbour
image and fails the comparison.  The bordered destination is tconvs1.0's in the network tests: a touched border is read by tconvs1.2.

GPU, network level: UtNet(16) at cs 104, batch 5 (tconvs1.0 at p = 8 and tconvs1.2 at p = 10 take the mosaic) against the oracle in
float64 at BAR_NET64 (the bar of the whole-tile float64 forward tests, tests/test_shared_encoder.py) and against mosaic_wino =
False at 1e-5 of the output scale; the 16-tile UtNet(64) frame of tests/test_skip_fold.py (tconvs1.2 at p = 8), mosaic on against
off at 2e-6 of the canvas scale and, with split_k = False, bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth

ABS_TOL = REL_TOL = 1e-3      # test_layer_winograd's assert_close, three-pass form against torch
FORMS_TOL = 1e-4              # test_layer_winograd: two forms of one layer, relative to max(1, max |reference|)
NO_SPLITK, TILE_WINO = _lib.FLAG_NO_SPLITK, _lib.FLAG_TILE_WINO
CIN, COUT, SLOPE = 32, 16, 0.13


def _load(name):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py")
    spec = importlib.util.spec_from_file_location("_wino_mosaic_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_SE = _load("test_shared_encoder")


def mosaic(p, B):
    bx, by, tiles, per = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_long(-1), ctypes.c_long(-1)
    rc = _lib.load().nd_wino_mosaic(p, B, ctypes.byref(bx), ctypes.byref(by), ctypes.byref(tiles), ctypes.byref(per))
    assert rc in (0, 1), rc
    return rc, bx.value, by.value, tiles.value, per.value


# ---------------------------------------------------------------------------- host: the planner

def test_planner():
    cdiv = lambda a, b: -(-a // b)
    for p in list(range(1, 41)) + [58, 62, 134]:
        for B in list(range(1, 40)) + [64, 255, 256, 257]:
            rc, bx, by, tiles, per = mosaic(p, B)
            assert per == B * cdiv(p, 6) ** 2 and tiles <= per, (p, B)
            assert mosaic(p, B) == (rc, bx, by, tiles, per)            # same inputs, same answer
            if rc:
                assert p >= 8 and B > 1 and bx * by >= B and by == cdiv(B, bx) and 10 * tiles <= 9 * per, (p, B, bx, by)
                assert tiles == cdiv(bx * p, 6) * cdiv(by * p, 6), (p, B, bx, by)
            else:
                assert (bx, by, tiles) == (0, 0, per), (p, B)
    assert mosaic(13, 256)[3:] == (1225, 2304) and mosaic(13, 256)[0] == 1     # bottom.2 at cs 264
    assert mosaic(28, 256)[3:] == (5625, 6400) and mosaic(28, 256)[0] == 1     # tconvs1.0
    assert mosaic(30, 256)[0] == 0 and mosaic(6, 256)[0] == 0                  # tconvs1.2: an exact fit; below the smallest pitch
    assert all(mosaic(p, 1)[0] == 0 for p in (8, 13, 28))
    lib = _lib.load()
    assert lib.nd_wino_mosaic(0, 4, None, None, None, None) < 0 and b"nd_wino_mosaic" in lib.nd_last_error()


# ---------------------------------------------------------------------------- GPU: one layer

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def rnd(shape, seed, scale=1.0):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * 2 - 1) * scale


@pytest.fixture(scope="module")
def layer():
    """weights of the layer, its three-pass blob (host) and the float64 references, computed once per input."""
    lib = _lib.load()
    w, b = rnd((CIN, COUT, 3, 3), 2, 1.7 / np.sqrt(CIN * 9)), rnd((COUT,), 3, 0.2)
    nbytes = lib.nd_winograd_packed_bytes(6, CIN, COUT)
    packed = torch.empty(nbytes // 4, dtype=torch.float32)
    _lib.check(lib.nd_winograd_pack(6, _lib.KIND["convT3"], CIN, COUT, w.data_ptr(), b.data_ptr(), packed.data_ptr(), nbytes))
    refs, blobs = {}, {}

    def ref(key, x):
        if key not in refs:
            refs[key] = F.prelu(F.conv_transpose2d(x.double(), w.double(), b.double()), torch.tensor([SLOPE], dtype=torch.float64))
        return refs[key]

    def blob(dev):
        if dev not in blobs:
            blobs[dev] = packed.to(dev)
        return blobs[dev]
    return dict(w=w, b=b, ref=ref, blob=blob)


def images(n, B, hot=None, zero=None):
    """B images of n x n, every one from its own seed; image `hot` 100 x its neighbours, image `zero` all zeros."""
    x = torch.stack([rnd((CIN, n, n), 1000 * n + k, 1.0 if k == hot or hot is None else 0.01) for k in range(B)])
    if zero is not None:
        x[zero] = 0
    return x


def layer_forward(dev, layer, x, flags=0):
    """test_layer_winograd's call of the three-pass F(6x6) form; the output starts as NaN."""
    lib = _lib.load()
    B, cin, H, W = x.shape
    k = _lib.KIND["convT3"]
    y = torch.full((B, COUT, H + 2, W + 2), float("nan"), dtype=torch.float32, device=dev)
    wsb = lib.nd_layer_winograd_workspace_bytes(6, k, B, cin, COUT, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    xd = x.to(dev).contiguous()
    _lib.check(lib.nd_layer_forward_winograd(6, k, _lib.ACT["PReLU"], SLOPE, layer["blob"](dev).data_ptr(), xd.data_ptr(), B, cin, H, W,
                                             COUT, y.data_ptr(), ws.data_ptr(), wsb, flags, _lib.stream_ptr(dev)))
    torch.cuda.synchronize()
    return y.cpu()


def check_against(y, ref, what):
    assert y.shape == ref.shape and torch.isfinite(y).all(), what     # (no NaN of the pre-filled output is left)
    err, scale = (y.double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"{what}: max abs err {err:.2e}, max |ref| {scale:.2e}")
    assert err <= ABS_TOL and err <= REL_TOL * max(scale, 1e-6), (what, err, scale)
    return err


def run_case(dev, layer, n, B, hot=None):
    x = images(n, B, hot)
    ref = layer["ref"]((n, B, hot), x)
    p = n + 2
    y = layer_forward(dev, layer, x)
    y_tile = layer_forward(dev, layer, x, TILE_WINO)
    what = f"convT3 {CIN}->{COUT} n={n} B={B} hot={hot} mosaic={mosaic(p, B)[:3]}"
    check_against(y, ref, what)                                                        # 1
    check_against(y_tile, ref, what + " per-image grids")
    d = (y - y_tile).abs().max().item()                                                # 2
    print(f"{what}: mosaic vs per-image grids {d:.2e}")
    assert d <= ABS_TOL and d <= REL_TOL * ref.abs().max().item() and d <= FORMS_TOL * max(1.0, ref.abs().max().item()), (what, d)
    if not mosaic(p, B)[0]:
        assert torch.equal(y, y_tile), what                                            # no mosaic: the switch switches nothing
    y_whole = layer_forward(dev, layer, x, NO_SPLITK)                                   # 3
    assert torch.equal(y_whole, layer_forward(dev, layer, x, NO_SPLITK | TILE_WINO)), what
    assert torch.equal(y_whole[:1], layer_forward(dev, layer, x[:1], NO_SPLITK)), what
    if hot is not None:   # every neighbour on its own scale: a leak of the 100 x image across a seam is ~100 x its values
        for k in range(B):
            e = (y[k].double() - ref[k]).abs().max().item()
            assert e <= REL_TOL * ref[hot].abs().max().item() * (1.0 if k == hot else 0.1), (what, k, e)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [2, 5, 7, 16])
@pytest.mark.parametrize("n", [6, 9, 11, 26])
def test_layer_mosaic(dev, layer, n, B):
    run_case(dev, layer, n, B)


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", [(6, 16), (11, 7), (11, 5)])
def test_layer_mosaic_one_loud_image(dev, layer, n, B):
    """image 3 is 100 x its neighbours: a wrong image index puts O(1) values where O(0.01) belong."""
    assert mosaic(n + 2, B)[0] == 1
    run_case(dev, layer, n, B, hot=3)


@pytest.mark.gpu
@pytest.mark.parametrize("hot", [None, 3], ids=["even", "loud-image-3"])
def test_layer_mosaic_at_the_pitch_of_tconvs1_0(dev, layer, hot):
    """p = 28 (tconvs1.0 at cs 264; 28 % 6 = 4: other seam positions and row wraps than p = 8 and 13), at the smallest batch with
    seams in both directions at which the rule takes the mosaic: 24 images as 6 x 4, 532 tiles against 600."""
    assert mosaic(28, 24) == (1, 6, 4, 532, 600)
    run_case(dev, layer, 26, 24, hot=hot)


@pytest.mark.gpu
def test_layer_mosaic_zero_image(dev, layer):
    """B = 7 at p = 13 (4 x 2 images, one empty slot): image 6 is all zeros, so its outputs are act(bias) up to what the tiles it
    shares with its neighbours round their contribution to -- bar: REL_TOL of the largest neighbour output (slack on purpose)."""
    n, B = 11, 7
    assert mosaic(n + 2, B)[:3] == (1, 4, 2)
    x = images(n, B, zero=6)
    y = layer_forward(dev, layer, x)
    b = layer["b"]
    want = torch.where(b > 0, b, b * SLOPE)[None, :, None, None].expand(1, COUT, n + 2, n + 2)
    e, neighbours = (y[6:] - want).abs().max().item(), y[:6].abs().max().item()
    print(f"zero image among 6: max |out - act(bias)| {e:.2e}, max |neighbour output| {neighbours:.2e}")
    assert torch.isfinite(y).all() and e <= REL_TOL * neighbours, (e, neighbours)
    check_against(y, layer["ref"]((n, B, "zero6"), x), "zero image")


# ---------------------------------------------------------------------------- GPU: the network and the frame loop

@pytest.mark.gpu
def test_utnet16_forward_vs_float64(dev):
    from oracle import networks as onet
    cs, B = 104, 5
    assert mosaic(8, B)[0] == 1 and mosaic(10, B)[0] == 1          # tconvs1.0, tconvs1.2
    net = _SE._net_visible(dev, 16, 9)
    x = torch.rand(B, 3, cs, cs, generator=torch.Generator().manual_seed(104))
    with torch.no_grad():
        ref = onet.utnet_forward(_SE._sd64(16, 9), x.double())
    assert net.mosaic_wino and not (net.flags & TILE_WINO)
    with torch.no_grad():
        y = net(x.to(dev)).cpu()
        net.mosaic_wino = False
        assert net.flags & TILE_WINO
        y_tile = net(x.to(dev)).cpu()
    e, e_tile, d = _SE._rel(y, ref), _SE._rel(y_tile, ref), (y - y_tile).abs().max().item()
    scale = ref.abs().max().item()
    print(f"UtNet(16) gain {_SE.VISIBLE_GAIN} cs {cs} batch {B}: mosaic {e:.2e}, per-image grids {e_tile:.2e} vs float64; "
          f"mosaic vs per-image {d:.2e} at output scale {scale:.2e}")
    assert e <= _SE.BAR_NET64 and e_tile <= _SE.BAR_NET64, (e, e_tile)
    assert d <= 1e-5 * scale and not torch.equal(y, y_tile), d      # (the switch does switch something)


@pytest.mark.gpu
def test_frame_mosaic_on_off(dev):
    from nind_denoise_amd import pipeline
    geom = (176, 176, 120, 56, 16)                  # tests/test_skip_fold.py: GEOM_C, 16 tiles of UtNet(64)
    W, H, cs, ucs, ol = geom
    assert pipeline.tile_count(*geom) == 16 and mosaic(8, 16)[0] == 1          # tconvs1.2: 6 -> 8 pixels
    net = _SE._net_visible(dev, 64, 123)
    img = torch.from_numpy(synth.make_frame(W, H, seed=24)).to(dev)

    def run(on, split_k):
        net.mosaic_wino, net.split_k = on, split_k
        cv = torch.zeros_like(img)
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=16, canvas=cv)
        net.mosaic_wino, net.split_k = True, True
        return cv

    on, off = run(True, True), run(False, True)
    d, scale = (on - off).abs().max().item(), off.abs().max().item()
    print(f"UtNet(64) gain {_SE.VISIBLE_GAIN} {geom}: mosaic vs per-image grids {d:.2e} at canvas scale {scale:.2e}")
    assert torch.isfinite(on).all() and scale > 0 and d <= 2e-6 * scale and not torch.equal(on, off), (d, scale)
    assert torch.equal(run(True, False), run(False, False))
    net._workspaces.clear()
