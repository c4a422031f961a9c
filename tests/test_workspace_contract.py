"""Where the kernels read and write, and what they assume is already in the memory they are handed.

The rest of the suite pins values.  This file pins the workspace contract of include/nind_hip.h ("Workspaces"):

* Guarded calls.  Every device buffer an entry point receives -- inputs, outputs, packed weights, workspaces, training blobs, flat
  parameter / gradient / moment vectors -- is the interior of a guarded allocation (tests/workspace_guard.py).  Workspaces with an
  init call are filled with 0xFF bytes (NaN in every float type, -1 in every integer) BEFORE that init call, plain scratch is
  filled with 0xFF before the call, outputs are prefilled with NaN; the frame workspace is zero-filled, as its contract says.
  After the call every guard is intact, every output is finite, and the result is bit for bit the one of the same call made the
  existing way (plain tensors, the Python wrappers' own allocations).
* NaN floods.  A legitimate call whose float inputs are all NaN puts NaN exactly where the kernels write.  The next real call on the
  same object must give the bits of the same call on a freshly made object: no state is carried between calls.
* One case per family is also held to the float64 oracle, at the bar its own test module defines (loaded, not restated).

Exclusions: none.  No buffer is left out of the guards.
Shapes are the smallest at which each family still takes every path; constants come from the modules that own them."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, pipeline, synth

import workspace_guard as G

pytestmark = pytest.mark.gpu


def _load(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py")
    spec = importlib.util.spec_from_file_location("_workspace_contract_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_SE = _load("test_shared_encoder")
_SF = _load("test_skip_fold")
_HP = _load("test_hip_parity")
_U64 = _load("test_unet_float64")
_UFL = _load("test_unet_frame_loop")
_UT = _load("test_unet_train")
_UG = _load("test_unet_grad")
_CP = _load("test_crop_pool")

NAN = float("nan")
F32 = torch.float32


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


class Guards:
    """The guarded buffers of one call, by name."""

    def __init__(self, dev):
        self.dev, self.handles = dev, {}

    def _keep(self, name, pair):
        assert name not in self.handles, name
        self.handles[name] = pair[1]
        return pair[0]

    def copy(self, name, t):
        """An input: the values of t (any device) on a guarded interior."""
        return self._keep(name, G.typed_like(t.detach().contiguous().to(self.dev)))

    def out(self, name, shape, dtype=F32):
        """An output, prefilled with 0xFF bytes (NaN / -1)."""
        return self._keep(name, G.typed(shape, dtype, self.dev, fill=0xFF))

    def zeros(self, name, shape, dtype=F32):
        return self._keep(name, G.typed(shape, dtype, self.dev, fill=0))

    def scratch(self, name, nbytes, fill=0xFF):
        """A workspace of nbytes, 0xFF-filled (before its init call, or as plain scratch); fill=0: the frame workspace."""
        return self._keep(name, G.guarded(nbytes, self.dev, fill=fill))

    def check(self, what):
        torch.cuda.synchronize()
        G.assert_all_guards(self.handles, what)


# every NaN-flood case runs under default flags and with split_k = False (ND_FLAG_NO_SPLITK: the whole-tile kernels)
SPLIT_K = pytest.mark.parametrize("split_k", [True, False], ids=["split-k", "whole-tiles"])


def _sp(dev):
    return _lib.stream_ptr(dev)


def _nan_like(t):
    return torch.full_like(t, NAN)


def _rnd(shape, seed, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


# ============================================================================ UtNet: forward

UTNET16 = (16, 9)       # funit, seed of the visible weights (tests/test_shared_encoder.py)
UTNET64 = (64, 123)
# (funit, seed), shape, compute dtype, attributes: UtNet(16) default flags, ND_FLAG_DIRECT_CONV, ND_FLAG_NO_SPLITK, bf16, f16 with the
# fused pool on and off, at a square and a rectangular batch; UtNet(64): the only width with the three-pass F(6x6) form, its mosaic
# on the deep layers and the wide conv_w2d tiles
FORWARD_CASES = [(UTNET16, s, dt, at) for s in ((3, 104, 104), (2, 104, 120))
                 for dt, at in (("f32", {}), ("f32", {"winograd": False}), ("f32", {"split_k": False}), ("bf16", {}), ("f16", {}),
                                ("f16", {"fused_pool": False}))] + [(UTNET64, (2, 104, 104), "f32", {})]


def _fid(c):
    (funit, _), s, dt, at = c
    return f"utnet{funit}-{'x'.join(map(str, s))}-{dt}" + "".join(f"-{k}={v}" for k, v in at.items())


def _utnet(dev, model, dtype="f32", **attrs):
    net = _SE._net_visible(dev, *model)
    net.set_compute_dtype(dtype)
    for k, v in attrs.items():
        setattr(net, k, v)
    return net


def _pack_utnet_guarded(g, net):
    """nd_utnet_pack_weights_device from guarded tensors into a guarded, 0xFF-filled blob."""
    lib = _lib.load()
    sd, names = net.state_dict(), _lib.utnet_tensor_names()
    ptrs = (ctypes.c_void_p * len(names))()
    for i, n in enumerate(names):
        ptrs[i] = g.copy("tensor " + n, sd[n].to(F32)).data_ptr() if n in sd else None
    nbytes = lib.nd_utnet_packed_bytes(net.funit, net._dt)
    blob = g.scratch("packed weights", nbytes)
    _lib.check(lib.nd_utnet_pack_weights_device(net.funit, net._dt, ptrs, len(names), blob.data_ptr(), nbytes, _sp(g.dev)), "pack")
    return blob


def _utnet_workspace_guarded(g, net, h, w, batch):
    lib = _lib.load()
    nbytes = lib.nd_utnet_workspace_bytes_hw(net.funit, h, w, batch, net._dt)
    assert nbytes > 0
    ws = g.scratch("workspace", nbytes)
    _lib.check(lib.nd_utnet_workspace_init_hw(ws.data_ptr(), nbytes, net.funit, h, w, batch, net._dt, _sp(g.dev)), "init")
    return ws


def _utnet_forward_guarded(dev, net, x):
    lib = _lib.load()
    g = Guards(dev)
    b, _, h, w = x.shape
    blob = _pack_utnet_guarded(g, net)
    xg, y = g.copy("x", x), g.out("y", x.shape)
    ws = _utnet_workspace_guarded(g, net, h, w, b)
    _lib.check(lib.nd_utnet_forward_hw(net.funit, _lib.ACT[net.activation], net._dt, net.flags, blob.data_ptr(), xg.data_ptr(),
                                       y.data_ptr(), b, h, w, ws.data_ptr(), ws.numel(), _sp(dev)), "nd_utnet_forward_hw")
    g.check("nd_utnet_forward_hw")
    mine = net.packed_weights(dev).view(torch.uint8).reshape(-1)
    assert torch.equal(blob, mine), "nd_utnet_pack_weights_device guarded vs the module's blob: " + G.mismatch(blob, mine)
    return y


@pytest.mark.parametrize("case", FORWARD_CASES, ids=_fid)
def test_utnet_forward_guarded_and_after_a_nan_batch(dev, case):
    model, shape, dtype, attrs = case
    x = _rnd((shape[0], 3) + shape[1:], 5).to(dev)
    used = _utnet(dev, model, dtype, **attrs)
    plain = used(x)                                                   # the existing way
    G.assert_same(_utnet_forward_guarded(dev, used, x), plain, "nd_utnet_forward_hw guarded vs plain")
    fresh = _utnet(dev, model, dtype, **attrs)
    G.flood_then(lambda: used(_nan_like(x)), lambda: used(x), lambda: fresh(x), "UtNet.forward")
    G.assert_same(fresh(x), plain, "UtNet.forward fresh vs first")
    if model == UTNET64:                                              # the link to float64 (family: UtNet forward)
        from oracle import networks as onet
        with torch.no_grad():
            ref = onet.utnet_forward(_SE._sd64(*model), x.cpu().double())
        e = _SE._rel(plain, ref)
        print(f"UtNet(64) {shape} forward vs float64 {e:.2e}")
        assert e <= _SE.BAR_NET64, e


# ============================================================================ UtNet: tiles and frames

# (W, H, cs, ucs, ol), dtype: three shared levels with all folds; two levels; stride 70 -> per-tile encoder; bf16 -> per tile; the
# narrowest and the lowest frame
GEOM3, GEOM2, GEOM0 = _SF.GEOM_A, _SF.LEVEL2_PER_TILE, _SF.NO_BAND
LOWEST = (GEOM3[0], GEOM3[2]) + GEOM3[2:]                            # as _SF.NARROWEST, in the other direction: one tile row
FRAME_BATCH = 6
FRAME_CASES = [(GEOM3, "f32"), (GEOM2, "f32"), (GEOM0, "f32"), (GEOM3, "bf16"), (_SF.NARROWEST, "f32"), (LOWEST, "f32")]
PLANS = [GEOM3, GEOM2, GEOM0]


def _gid(c):
    geom, dtype = c
    return "{}x{}-{}-{}-{}-".format(*geom) + dtype


def _levels(net, geom):
    out = ctypes.c_int(-1)
    _lib.check(_lib.load().nd_utnet_frame_levels(net.funit, net._dt, net.frame_flags, *geom, ctypes.byref(out)))
    return out.value


def _frame_img(geom, seed, dev):
    return torch.from_numpy(synth.make_frame(geom[0], geom[1], seed=seed)).to(dev)


def _utnet_frame_guarded(dev, net, img, geom, batch, tile_range=None, tiles_api=False):
    """nd_utnet_denoise_frame (or nd_utnet_denoise_tiles) with every buffer guarded; the canvas starts at zero, as the wrappers' does."""
    lib = _lib.load()
    W, H, cs, ucs, ol = geom
    begin, end = tile_range if tile_range is not None else (0, pipeline.tile_count(*geom))
    g = Guards(dev)
    blob = _pack_utnet_guarded(g, net)
    ig, canvas = g.copy("frame", img), g.zeros("canvas", img.shape)
    ws = _utnet_workspace_guarded(g, net, cs, cs, batch)
    act, fl = _lib.ACT[net.activation], net.frame_flags
    if tiles_api:
        assert end - begin <= batch
        _lib.check(lib.nd_utnet_denoise_tiles(net.funit, act, net._dt, net.flags, blob.data_ptr(), ig.data_ptr(), canvas.data_ptr(), W, H,
                                              cs, ucs, ol, begin, end - begin, batch, ws.data_ptr(), ws.numel(), _sp(dev)),
                   "nd_utnet_denoise_tiles")
    else:
        fbytes = lib.nd_utnet_frame_workspace_bytes(net.funit, net._dt, fl, W, H, cs, ucs, ol, batch)
        fws = g.scratch("frame workspace", fbytes, fill=0) if fbytes else None      # zero-filled: it holds the tile-origin tables
        _lib.check(lib.nd_utnet_denoise_frame(net.funit, act, net._dt, fl, blob.data_ptr(), ig.data_ptr(), canvas.data_ptr(), W, H, cs,
                                              ucs, ol, begin, end - begin, batch, ws.data_ptr(), ws.numel(),
                                              fws.data_ptr() if fbytes else None, fbytes, _sp(dev), _lib.PROGRESS_FN(), None),
                   "nd_utnet_denoise_frame")
    g.check("nd_utnet_denoise_tiles" if tiles_api else "nd_utnet_denoise_frame")
    return canvas


@pytest.fixture(scope="module")
def ref16():
    """float64 canvas of the UtNet(16) frame GEOM3 (frame seed 3), computed once."""
    from oracle import tiler as otiler
    cache = {}

    def get():
        if not cache:
            W, H, cs, ucs, ol = GEOM3
            cache[0] = otiler.denoise_frame(synth.make_frame(W, H, seed=3), cs, ucs, ol, _SE._model64(_SE._sd64(*UTNET16)), batch=16)
        return cache[0]
    return get


@pytest.mark.parametrize("case", FRAME_CASES, ids=_gid)
def test_utnet_frame_guarded(dev, case, ref16):
    geom, dtype = case
    net = _utnet(dev, UTNET16, dtype)
    assert _levels(net, geom) == {(GEOM2, "f32"): 2, (GEOM0, "f32"): 0, (GEOM3, "bf16"): 0}.get(case, 3)
    img = _frame_img(geom, 3, dev)
    cs, ucs, ol = geom[2:]
    plain = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=FRAME_BATCH)
    G.assert_same(_utnet_frame_guarded(dev, net, img, geom, FRAME_BATCH), plain, "nd_utnet_denoise_frame guarded vs plain")
    if case == (GEOM3, "f32"):                                        # the link to float64 (family: UtNet frame)
        e = _SE._rel(plain, ref16())
        print(f"UtNet(16) {geom} frame vs float64 {e:.2e}")
        assert e <= _SE.BAR_FRAME16, e


def test_utnet_tile_range_that_ends_inside_a_tile_row_guarded(dev):
    geom = GEOM3
    cols, rows, _ = _lib.tile_grid(*geom)
    rng = (3, 2 * cols + 5)                                           # starts and ends inside a tile row; launches of 6, 6, 6
    assert rng[0] % cols and rng[1] % cols and rng[1] < cols * rows
    net = _utnet(dev, UTNET16)
    img = _frame_img(geom, 3, dev)
    plain = pipeline.denoise_frame(net, img, *geom[2:], batch=FRAME_BATCH, tile_range=rng)
    G.assert_same(_utnet_frame_guarded(dev, net, img, geom, FRAME_BATCH, rng), plain, "nd_utnet_denoise_frame, tile range")
    # nd_utnet_denoise_tiles: one launch of fewer tiles than the workspace's batch, in useful-region mode
    net.share_encoder = False
    one = (cols - 2, cols + 2)
    plain = pipeline.denoise_frame(net, img, *geom[2:], batch=FRAME_BATCH, tile_range=one)
    got = _utnet_frame_guarded(dev, net, img, geom, FRAME_BATCH, one, tiles_api=True)
    G.assert_same(got, plain, "nd_utnet_denoise_tiles")


@SPLIT_K
@pytest.mark.parametrize("geom", PLANS, ids=lambda g: "{}x{}-{}-{}-{}".format(*g))
def test_whole_tiles_then_useful_regions_and_frame_after_nan_frame(dev, geom, split_k):
    """One activation workspace, key (device, 120, 120, 6, dtype), serves net(x) on whole tiles and the frame loop in useful-region
    mode: after a whole-tile forward of NaN everything outside the regions holds NaN.  Then a NaN frame, then the real one."""
    cs, ucs, ol = geom[2:]
    img = _frame_img(geom, 3, dev)
    fresh = _utnet(dev, UTNET16, split_k=split_k)
    want = pipeline.denoise_frame(fresh, img, cs, ucs, ol, batch=FRAME_BATCH)
    used = _utnet(dev, UTNET16, split_k=split_k)
    used(torch.full((FRAME_BATCH, 3, cs, cs), NAN, device=dev))
    assert len(used._workspaces) == 1
    ws = next(iter(used._workspaces.values())).view(F32)
    flooded = int(torch.isnan(ws).sum())
    assert flooded >= FRAME_BATCH * used.funit * cs * cs, (flooded, ws.numel())  # (the flood is real: NaN wherever the kernels wrote)
    got = pipeline.denoise_frame(used, img, cs, ucs, ol, batch=FRAME_BATCH)
    assert len([k for k in used._workspaces if k[1] != "frame"]) == 1          # (the same activation workspace served both)
    print(f"{geom}: {flooded} NaN in the activation workspace after the whole-tile forward, {int(torch.isnan(ws).sum())} left after the "
          "useful-region frame")
    G.assert_same(got, want, "frame after a whole-tile NaN forward")
    G.flood_then(lambda: pipeline.denoise_frame(used, _nan_like(img), cs, ucs, ol, batch=FRAME_BATCH),
                 lambda: pipeline.denoise_frame(used, img, cs, ucs, ol, batch=FRAME_BATCH), lambda: want, "frame after a NaN frame")


@SPLIT_K
def test_frame_engine_after_a_nan_frame(dev, split_k):
    """The resident worker's path: FrameEngine.run([NaN frame, frame]) against a fresh net."""
    from nind_denoise_amd.serve import FrameEngine
    geom = GEOM3
    W, H, cs, ucs, ol = geom
    frame = synth.make_frame(W, H, seed=3)
    want = pipeline.denoise_frame(_utnet(dev, UTNET16, split_k=split_k), torch.from_numpy(frame).to(dev), cs, ucs, ol, batch=FRAME_BATCH)
    eng = FrameEngine(_utnet(dev, UTNET16, split_k=split_k), W, H, cs, ucs, ol, batch=FRAME_BATCH, slots=2, device=dev)
    outs = list(eng.run([np.full_like(frame, np.nan), frame]))
    assert len(outs) == 2 and np.isnan(outs[0]).all()
    G.assert_same(torch.from_numpy(np.ascontiguousarray(outs[1])), want.cpu(), "FrameEngine: frame after a NaN frame")


def _plan(net, geom):
    out = (ctypes.c_int * 8)()
    _lib.check(_lib.load().nd_utnet_frame_plan(net.funit, net._dt, net.frame_flags, *geom, out))
    return dict(zip(("D", "aligned", "R", "bands", "S", "cols", "rows", "hx"), out))


def _two_geometries_in_one_frame_workspace(dev, model, geom_a, geom_b, batch, seeds, split_k):
    """Frames of two geometries whose frame workspaces have the same size share one cached buffer: both orders, the first frame
    real and NaN.  One net lives at a time: the fresh canvases go to the host before the used net is made."""
    lib = _lib.load()
    imgs = {g: _frame_img(g, s, dev) for g, s in zip((geom_a, geom_b), seeds)}

    def run(net, geom, img=None):
        return pipeline.denoise_frame(net, imgs[geom] if img is None else img, *geom[2:], batch=batch)

    want = {}
    for g in (geom_a, geom_b):
        net = _utnet(dev, model, split_k=split_k)
        want[g] = run(net, g).cpu()
        assert torch.isfinite(want[g]).all()
        net._workspaces.clear()
        del net
    torch.cuda.empty_cache()
    used = _utnet(dev, model, split_k=split_k)
    sizes = [lib.nd_utnet_frame_workspace_bytes(used.funit, used._dt, used.frame_flags, *g, batch) for g in (geom_a, geom_b)]
    assert sizes[0] == sizes[1] > 0, sizes
    assert used.frame_workspace(*geom_a, batch, dev) is used.frame_workspace(*geom_b, batch, dev)
    for first, second in ((geom_a, geom_b), (geom_b, geom_a)):
        for flood in (False, True):
            run(used, first, _nan_like(imgs[first]) if flood else None)
            got = run(used, second).cpu()
            G.assert_same(got, want[second], f"{second} after {'a NaN frame of ' if flood else ''}{first} in one frame workspace")
    used._workspaces.clear()


@SPLIT_K
def test_frame_after_another_geometry_utnet16(dev, split_k):
    a, b = GEOM3, (310, 270) + GEOM3[2:]
    net = _utnet(dev, UTNET16)
    pa, pb = _plan(net, a), _plan(net, b)
    assert (pa["cols"], pa["rows"]) == (pb["cols"], pb["rows"]) == (8, 7) and a[:2] != b[:2]
    _two_geometries_in_one_frame_workspace(dev, UTNET16, a, b, FRAME_BATCH, (3, 4), split_k)


@SPLIT_K
def test_frame_after_another_geometry_utnet64_short_last_band(dev, split_k):
    """3000 x 2136 plans 16 tile rows in bands of 8 + 8, 3000 x 2000 plans 15 in bands of 8 + 7: the second frame's short last band
    lies where the first frame's full band was."""
    a, b = (3000, 2136, 264, 200, 64), (3000, 2000, 264, 200, 64)
    assert b == _SE.MULTI_BAND[1][0]
    net = _utnet(dev, UTNET64)
    pa, pb = _plan(net, a), _plan(net, b)
    assert (pa["rows"], pa["bands"], pa["R"]) == (16, 2, 8) and (pb["rows"], pb["bands"], pb["R"]) == (15, 2, 8)
    del net
    _two_geometries_in_one_frame_workspace(dev, UTNET64, a, b, 64, (24, 25), split_k)
    torch.cuda.empty_cache()


# ============================================================================ guarded vs plain: one body, two allocators

class Plain:
    """The existing way: plain tensors, zeroed scratch."""

    def __init__(self, dev):
        self.dev = dev

    def copy(self, name, t):
        return t.detach().contiguous().to(self.dev).clone()

    def out(self, name, shape, dtype=F32):
        return torch.zeros(tuple(shape) if not isinstance(shape, int) else (shape,), dtype=dtype, device=self.dev)

    zeros = out

    def scratch(self, name, nbytes, fill=0xFF):
        return torch.zeros(nbytes, dtype=torch.uint8, device=self.dev)

    def check(self, what):
        torch.cuda.synchronize()


def _both(dev, body, what):
    """body(allocator) -> results.  Guarded (0xFF scratch, NaN outputs, guards checked) against plain (zeroed scratch): finite, same bits."""
    g = Guards(dev)
    got = body(g)
    g.check(what)
    want = body(Plain(dev))
    torch.cuda.synchronize()
    G.assert_same(got, want, what + " guarded vs plain")
    return got


# ============================================================================ UNet

def _pack_unet(a, net):
    lib = _lib.load()
    sd, n = net.state_dict(), lib.nd_unet_num_tensors()
    ptrs = (ctypes.c_void_p * n)()
    keep = []
    for i in range(n):
        name = lib.nd_unet_tensor_name(i).decode()
        keep.append(a.copy("tensor " + name, sd[name].to(F32)))
        ptrs[i] = keep[-1].data_ptr()
    nbytes = lib.nd_unet_packed_bytes(_lib.ND_F32)
    blob = a.scratch("packed weights", nbytes)
    _lib.check(lib.nd_unet_pack_weights_device(_lib.ND_F32, ptrs, n, blob.data_ptr(), nbytes, _sp(a.dev)), "nd_unet_pack_weights_device")
    torch.cuda.synchronize()
    return blob


def _unet_workspace(a, h, w, batch):
    lib = _lib.load()
    nbytes = lib.nd_unet_workspace_bytes(h, w, batch, _lib.ND_F32)
    assert nbytes > 0
    ws = a.scratch("workspace", nbytes)
    _lib.check(lib.nd_unet_workspace_init(ws.data_ptr(), nbytes, h, w, batch, _lib.ND_F32, _sp(a.dev)), "nd_unet_workspace_init")
    return ws


UNET_SHAPES = [_U64.SMALL_SHAPES[0]] + _U64.ODD_SHAPES[:2]           # the smallest, and two with fix-up lines


@pytest.mark.parametrize("shape", UNET_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_unet_forward_guarded_and_after_a_nan_batch(dev, shape):
    lib = _lib.load()
    seed = 3
    x, ref = _U64._ref(seed, False, shape)
    used = _U64._net(dev, seed)
    xd = x.to(dev)
    plain = used(xd)

    def body(a):
        b, _, h, w = x.shape
        blob, xg, y = _pack_unet(a, used), a.copy("x", x), a.out("y", x.shape)
        ws = _unet_workspace(a, h, w, b)
        _lib.check(lib.nd_unet_forward(_lib.ND_F32, blob.data_ptr(), xg.data_ptr(), y.data_ptr(), b, h, w, ws.data_ptr(), ws.numel(),
                                       _sp(dev)), "nd_unet_forward")
        return y, blob

    y, blob = _both(dev, body, "nd_unet_forward")
    G.assert_same(y, plain, "nd_unet_forward guarded vs the module")
    assert torch.equal(blob, used.packed_weights(dev).view(torch.uint8).reshape(-1))
    G.flood_then(lambda: used(_nan_like(xd)), lambda: used(xd), lambda: _U64._net(dev, seed)(xd), "UNet.forward")
    if shape == UNET_SHAPES[-1]:                                     # the link to float64 (family: UNet)
        e = _U64._err(plain, ref)
        print(f"UNet {shape} forward vs float64 {e:.2e}")
        assert e <= _U64.BAR_UNET_FWD, e


UNET_FRAMES = [_UFL.GEOMS[2], _UFL.GEOMS[3]]                         # odd cs - ucs; the smallest tiles


@SPLIT_K
@pytest.mark.parametrize("geom", UNET_FRAMES, ids=lambda g: "{}x{}-{}-{}-{}-b{}".format(*g))
def test_unet_frame_guarded_and_after_a_nan_frame(dev, geom, split_k):
    lib = _lib.load()
    W, H, cs, ucs, ol, batch = geom
    img = torch.from_numpy(synth.make_frame(W, H, seed=W + H)).to(dev)
    used = _UFL.make_net(dev, split_k=split_k)
    plain = pipeline.denoise_frame(used, img, cs, ucs, ol, batch=batch)

    def body(a):
        blob, ig, canvas = _pack_unet(a, used), a.copy("frame", img), a.zeros("canvas", img.shape)
        ws = _unet_workspace(a, cs, cs, batch)
        _lib.check(lib.nd_unet_denoise_frame(_lib.ND_F32, used.flags, blob.data_ptr(), ig.data_ptr(), canvas.data_ptr(), W, H, cs, ucs, ol, 0,
                                             pipeline.tile_count(W, H, cs, ucs, ol), batch, ws.data_ptr(), ws.numel(), _sp(dev),
                                             _lib.PROGRESS_FN(), None), "nd_unet_denoise_frame")
        return canvas

    G.assert_same(_both(dev, body, "nd_unet_denoise_frame"), plain, "nd_unet_denoise_frame guarded vs the module")
    # whole tiles (UNet.forward on the same workspace key), then the useful-region loop; then a NaN frame
    used(torch.full((batch, 3, cs, cs), NAN, device=dev))
    G.assert_same(pipeline.denoise_frame(used, img, cs, ucs, ol, batch=batch), plain, "UNet frame after a whole-tile NaN forward")
    G.flood_then(lambda: pipeline.denoise_frame(used, _nan_like(img), cs, ucs, ol, batch=batch),
                 lambda: pipeline.denoise_frame(used, img, cs, ucs, ol, batch=batch),
                 lambda: pipeline.denoise_frame(_UFL.make_net(dev, split_k=split_k), img, cs, ucs, ol, batch=batch), "UNet frame loop")


def _param_mask(ranges, n, dev, keep):
    m = torch.zeros(n, dtype=torch.bool, device=dev)
    for k, (off, cnt) in ranges.items():
        if keep(k):
            m[off:off + cnt] = True
    return m


def _unet_halves(dev, tr, x, target, train, flags):
    """nd_unet_train_* (train) or nd_unet_grad_* on the (3, 33, 47) case: y, dx, the parameter gradients, the flat buffer after."""
    lib = _lib.load()
    b, _, h, w = x.shape
    is_par = _param_mask(tr.ranges, tr.flat.numel(), dev, _UG.is_parameter)
    size, init, fwd, bwd, blob_bytes = ((lib.nd_unet_train_workspace_bytes, lib.nd_unet_train_workspace_init, lib.nd_unet_train_forward,
                                         lib.nd_unet_train_backward, lib.nd_unet_train_blob_bytes()) if train else
                                        (lib.nd_unet_grad_workspace_bytes, lib.nd_unet_grad_workspace_init, lib.nd_unet_grad_forward,
                                         lib.nd_unet_grad_backward, lib.nd_unet_grad_blob_bytes()))
    flat0 = tr.flat.clone()

    def body(a):
        flat, grads, blobs = a.copy("flat parameters", flat0), a.out("flat gradients", flat0.shape), a.scratch("blobs", blob_bytes)
        xg, tg, y, dx = a.copy("x", x), a.copy("target", target), a.out("y", x.shape), a.out("dx", x.shape)
        nbytes = size(h, w, b)
        ws = a.scratch("workspace", nbytes)
        _lib.check(init(ws.data_ptr(), nbytes, h, w, b, _sp(dev)), "workspace init")
        mom = (_UT.MOMENTUM,) if train else ()
        _lib.check(fwd(flags, flat.data_ptr(), blobs.data_ptr(), xg.data_ptr(), y.data_ptr(), b, h, w, *mom, ws.data_ptr(), nbytes,
                       _sp(dev)), "forward")
        gy = a.copy("gy", (2.0 / y.numel()) * (y - tg))
        _lib.check(bwd(flags, flat.data_ptr(), grads.data_ptr(), blobs.data_ptr(), gy.data_ptr(), dx.data_ptr(), b, h, w, ws.data_ptr(),
                       nbytes, _sp(dev)), "backward")
        torch.cuda.synchronize()
        # the slots of running statistics in `grads` are never written (include/nind_hip.h): they keep what the caller put there
        return y, dx, grads[is_par], flat.clone()

    return _both(dev, body, "nd_unet_train_*" if train else "nd_unet_grad_*")


@SPLIT_K
def test_unet_train_halves_guarded_and_after_a_nan_batch(dev, split_k):
    sd, x, target, *ref = _UT.train_case(_UT.MAIN)
    assert _UT.MAIN[1] == (3, 33, 47)
    tr = _UT._trainer(dev, sd, split_k=split_k)
    assert bool(tr.flags & _lib.FLAG_NO_SPLITK) == (not split_k)
    y, dx, grads, flat = _unet_halves(dev, tr, x.to(dev), target.to(dev), True, tr.flags)
    flat0 = tr.flat.clone()
    out = _UT._run(tr, x, target)                                    # the existing way, and the link to float64 (family: UNet training)
    _UT._check_case("workspace contract", out, ref, _UT.BARS if split_k else _UT.BARS_NO_SPLITK)
    G.assert_same(y, out[0], "nd_unet_train_forward guarded vs the trainer")
    G.assert_same(dx, out[1], "nd_unet_train_backward dx guarded vs the trainer")
    is_par = _param_mask(tr.ranges, tr.flat.numel(), dev, _UG.is_parameter)
    G.assert_same(grads, tr.grads[is_par], "nd_unet_train_backward gradients guarded vs the trainer")
    G.assert_same(flat, tr.flat, "running statistics guarded vs the trainer")
    # NaN batch, then the real one: the forward rewrites the running statistics, so they are put back; workspace and blobs stay
    fresh = [t.clone() for t in out[:2]] + [tr.grads[is_par].clone()]
    tr.flat.copy_(flat0)
    snap = tr.flat.clone()
    _UT._run(tr, torch.full_like(x, NAN), target)
    tr.flat.copy_(snap)
    again = _UT._run(tr, x, target)
    G.assert_same([again[0], again[1], tr.grads[is_par]], fresh, "UNetTrainer after a NaN batch")


@SPLIT_K
def test_unet_autograd_guarded_and_after_a_nan_batch(dev, split_k):
    shape = (3, 33, 47)
    sd, x, target, y64, dx64, g64 = _UG.crop_case(shape)
    net = _UG._net(dev, sd)
    net.split_k = split_k
    assert bool(net.grad_flags & _lib.FLAG_NO_SPLITK) == (not split_k)
    y0, dx0, grads0 = _UG._run(net, x, target, dev)
    grads0 = {k: v.clone() for k, v in grads0.items()}               # (a later backward accumulates into p.grad in place)
    e = _U64._err(y0, y64)
    assert e <= _UG.BAR_UNET_FWD, e
    if split_k:                                                      # (the float64 bars of test_unet_grad are those of the default flags)
        _UG._assert_bars("workspace contract", _UG.class_figures(dx0, grads0, dx64, g64))
    st = net._gstate
    y, dx, grads, _ = _unet_halves(dev, st, x.to(dev), target.to(dev), False, net.grad_flags)
    G.assert_same(y, y0, "nd_unet_grad_forward guarded vs the module")
    xn = torch.full_like(x, NAN).to(dev).requires_grad_()
    net(xn).sum().backward()
    y1, dx1, grads1 = _UG._run(net, x, target, dev)
    G.assert_same([y1, dx1] + [grads1[k] for k in sorted(grads1)], [y0, dx0] + [grads0[k] for k in sorted(grads0)],
                  "UNet under autograd after a NaN batch")


# ============================================================================ UtNet training

def _utnet_trainer(dev, funit, weights, loss_cs=None, seed=31, **attrs):
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    net = UtNet(funit=funit)
    net.load_state_dict(synth.make_utnet_state_dict(funit=funit, seed=seed, gain=1.8))      # (the weights of test_hip_parity's step tests)
    for k, v in attrs.items():
        setattr(net, k, v)
    return UtNetTrainer(net, device=dev, weights=weights, loss_cs=loss_cs)


def _train_pair(shape, seed=3):
    b, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(b, 3, h, w, generator=g)
    return x, (x * 0.9 + 0.05 * torch.rand(b, 3, h, w, generator=g)).clip(0, 1)


# funit, (B, h, w), weights, loss_cs: L1 + MSE; SSIM on a centre window of a rectangular crop; UtNet(64): the weight gradients at
# 512 / 1024 channels and few pixels
STEP_CASES = [(8, (2, 104, 104), {"L1": 0.3, "MSE": 0.7}, None), (8, (2, 120, 104), {"SSIM": 1.0}, 88),
              (64, (2, 104, 104), {"MSE": 1.0}, None)]


@SPLIT_K
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: f"utnet{c[0]}-{'x'.join(map(str, c[1]))}-{'+'.join(c[2])}")
def test_utnet_train_step_guarded_and_after_a_nan_batch(dev, case, split_k):
    lib = _lib.load()
    funit, shape, weights, loss_cs = case
    b, h, w = shape
    x, t = _train_pair(shape)
    tr = _utnet_trainer(dev, funit, weights, loss_cs, split_k=split_k)
    assert bool(tr.model.flags & _lib.FLAG_NO_SPLITK) == (not split_k)
    y0, loss0 = tr.forward_backward(x, t)                             # the existing way
    y0, loss0, g0 = y0.clone(), loss0.clone(), tr.grads.clone()

    def body(a):
        flat, grads = a.copy("flat parameters", tr.flat), a.out("flat gradients", tr.grads.shape)
        blobs = a.scratch("training blobs", lib.nd_utnet_train_blob_bytes(funit))
        xg, tg, y, loss = a.copy("x", x), a.copy("target", t), a.out("y", x.shape), a.out("loss", (1,))
        nbytes = lib.nd_utnet_train_workspace_bytes_hw(funit, h, w, b)
        ws = a.scratch("training workspace", nbytes)
        _lib.check(lib.nd_utnet_train_workspace_init_hw(ws.data_ptr(), nbytes, funit, h, w, b, _sp(dev)), "init")
        _lib.check(lib.nd_utnet_train_step_act_hw(funit, _lib.ACT[tr.model.activation], tr.model.flags, flat.data_ptr(), grads.data_ptr(),
                                                  blobs.data_ptr(), xg.data_ptr(), tg.data_ptr(), y.data_ptr(),
                                                  *[float(weights.get(k, 0.0)) for k in ("L1", "MSE", "SSIM", "MSSSIM")],
                                                  loss.data_ptr(), b, h, w, int(loss_cs or 0), ws.data_ptr(), nbytes, _sp(dev), None, 0),
                   "nd_utnet_train_step_act_hw")
        return y, loss, grads

    G.assert_same(_both(dev, body, "nd_utnet_train_step_act_hw"), (y0, loss0, g0), "nd_utnet_train_step_act_hw guarded vs the trainer")
    # NaN batch (no optimizer step after it), then the real one, against a fresh trainer
    tr.forward_backward(_nan_like(x), _nan_like(t))
    y1, loss1 = tr.forward_backward(x, t)
    fresh = _utnet_trainer(dev, funit, weights, loss_cs, split_k=split_k)
    y2, loss2 = fresh.forward_backward(x, t)
    G.assert_same((y1, loss1, tr.grads), (y2, loss2, fresh.grads), "UtNetTrainer after a NaN batch vs a fresh trainer")
    G.assert_same((y2, loss2, fresh.grads), (y0, loss0, g0), "fresh trainer vs first")
    if funit == 64 and split_k:                                       # the link to float64 (family: UtNet training step)
        sd = synth.make_utnet_state_dict(funit=funit, seed=31, gain=1.8)
        y_ref, loss_ref, params = _HP._autograd_reference(sd, x, t, 0.0, 1.0, torch.float64)
        _HP.assert_close(y0, y_ref.float(), "training forward")
        assert abs(loss0.item() - loss_ref.item()) <= _HP.TRAIN_LOSS_REL_TOL * max(1.0, abs(loss_ref.item()))
        for name, p in params.items():
            got, ref = tr.grad_of(name).cpu(), p.grad.float()
            err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-8)
            assert err <= _HP.TRAIN_GRAD_BAR_WIDE_F64, (name, err)


@SPLIT_K
def test_utnet_train_halves_with_dx_guarded_and_autograd_after_a_nan_batch(dev, split_k):
    lib = _lib.load()
    funit, shape = 8, (2, 104, 120)
    b, h, w = shape
    x, _ = _train_pair(shape)
    gy = _rnd((b, 3, h, w), 11, -1.0, 1.0).to(dev)

    def module():
        return _utnet_trainer(dev, funit, {"MSE": 1.0}, split_k=split_k).model.train()

    def autograd(net, xin):
        net.zero_grad(set_to_none=True)
        xd = xin.to(dev).requires_grad_()
        y = net(xd)
        y.backward(gy)
        return [y.detach(), xd.grad] + [p.grad.clone() for _, p in sorted(net.named_parameters())]

    used = module()
    want = autograd(used, x)                                          # the existing way
    st = used._tstate

    def body(a):
        flat, grads = a.copy("flat parameters", st.flat), a.out("flat gradients", st.grads.shape)
        blobs = a.scratch("training blobs", lib.nd_utnet_train_blob_bytes(funit))
        xg, y, gyg, dx = a.copy("x", x), a.out("y", x.shape), a.copy("gy", gy), a.out("dx", x.shape)
        nbytes = lib.nd_utnet_train_workspace_bytes_hw(funit, h, w, b)
        ws = a.scratch("training workspace", nbytes)
        act, fl = _lib.ACT[used.activation], used.flags
        _lib.check(lib.nd_utnet_train_workspace_init_hw(ws.data_ptr(), nbytes, funit, h, w, b, _sp(dev)), "init")
        _lib.check(lib.nd_utnet_train_forward_hw(funit, act, fl, flat.data_ptr(), blobs.data_ptr(), xg.data_ptr(), y.data_ptr(), b, h, w,
                                                 ws.data_ptr(), nbytes, _sp(dev)), "nd_utnet_train_forward_hw")
        _lib.check(lib.nd_utnet_train_backward_hw(funit, act, fl, flat.data_ptr(), grads.data_ptr(), blobs.data_ptr(), gyg.data_ptr(),
                                                  dx.data_ptr(), b, h, w, ws.data_ptr(), nbytes, _sp(dev), None, 0),
                   "nd_utnet_train_backward_hw")
        return y, dx, grads

    y, dx, grads = _both(dev, body, "nd_utnet_train_forward_hw / _backward_hw")
    G.assert_same([y, dx], want[:2], "training halves guarded vs autograd on the module")
    for (name, p), gp in zip(sorted(used.named_parameters()), want[2:]):
        off, cnt = st.ranges[name]
        G.assert_same(grads[off:off + cnt].view(gp.shape), gp, "gradient of " + name)
    # the autograd path after a NaN batch: net.train()(x).sum().backward()
    xn = torch.full_like(x, NAN).to(dev).requires_grad_()
    used(xn).sum().backward()
    G.assert_same(autograd(used, x), autograd(module(), x), "UtNet under autograd after a NaN batch")


# ============================================================================ single layers

def _layer_data(kind, B, cin, cout, H, W, seed=1):
    k = {"conv3": 3, "convT3": 3, "convT2s2": 2, "conv1": 1}[kind]
    x = _HP.rnd((B, cin, H, W), seed)
    wshape = (cout, cin, k, k) if kind in ("conv3", "conv1") else (cin, cout, k, k)
    return x, _HP.rnd(wshape, seed + 1, 1.7 / np.sqrt(cin * k * k)), _HP.rnd((cout,), seed + 2, 0.2)


def _ref_layer64(kind, x, w, b, act, slope):
    """test_hip_parity.ref_layer in float64."""
    x, w, b = x.double(), w.double(), b.double()
    y = F.conv2d(x, w, b) if kind in ("conv3", "conv1") else F.conv_transpose2d(x, w, b, stride=2 if kind == "convT2s2" else 1)
    if act == "PReLU":
        y = torch.where(y >= 0, y, slope * y)
    else:
        assert act == "none", act
    return y


def _out_hw(kind, H, W):
    return {"conv3": (H - 2, W - 2), "convT3": (H + 2, W + 2), "convT2s2": (2 * H, 2 * W), "conv1": (H, W)}[kind]


# one odd-sized case per kind of test_hip_parity.LAYER_CASES, and its first-layer case (cin 3)
def _first(cases, pred):
    return next(c for c in cases if pred(c))


def _odd(c):
    return c[4] % 2 == 1 and c[5] % 2 == 1


LAYERS = [_first(_HP.LAYER_CASES, lambda c, k=k: c[0] == k and _odd(c)) for k in ("conv3", "convT3", "convT2s2", "conv1")] + \
    [_first(_HP.LAYER_CASES, lambda c: c[2] == 3)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("case", LAYERS, ids=lambda c: "-".join(str(v) for v in c))
def test_layer_forward_guarded(dev, case, dtype):
    lib = _lib.load()
    kind, B, cin, cout, H, W, act = case
    x, w, b = _layer_data(kind, B, cin, cout, H, W)
    k, dt = _lib.KIND[kind], _lib.DTYPE[dtype]
    nbytes = lib.nd_layer_packed_bytes(k, cin, cout, dt)
    packed = torch.empty(nbytes // 4, dtype=F32)
    _lib.check(lib.nd_layer_pack(k, cin, cout, dt, w.contiguous().data_ptr(), b.data_ptr(), packed.data_ptr(), nbytes))

    def body(a):
        pk, xg, y = a.copy("packed weights", packed), a.copy("x", x), a.out("y", (B, cout) + _out_hw(kind, H, W))
        wsb = lib.nd_layer_workspace_bytes(k, B, cin, cout, H, W, dt)
        ws = a.scratch("workspace", wsb)
        _lib.check(lib.nd_layer_forward(k, _lib.ACT[act], 0.13, dt, pk.data_ptr(), xg.data_ptr(), B, cin, H, W, cout, y.data_ptr(),
                                        ws.data_ptr(), wsb, -1, 0, _sp(dev)), "nd_layer_forward")
        return y

    y = _both(dev, body, "nd_layer_forward")
    G.assert_same(y, _HP.layer_forward(dev, kind, x, w, b, act, 0.13, dtype=dtype), "nd_layer_forward guarded vs test_hip_parity's call")
    if dtype == "f32":                                                # the link to float64 (family: single layers)
        _HP.assert_close(y, _ref_layer64(kind, x, w, b, act, 0.13), str(case))


# the two cases of test_hip_parity.WINO_CASES that the issue names: partial tiles masked; a transposed layer with a zero border
WINO_LAYERS = [c for c in _HP.WINO_CASES if c[:6] in (("conv3", 3, 64, 128, 21, 19), ("convT3", 2, 32, 256, 11, 11))]
assert len(WINO_LAYERS) == 2


@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("case", WINO_LAYERS, ids=lambda c: "-".join(str(v) for v in c))
def test_layer_forward_winograd_guarded(dev, case, tile):
    """nd_layer_forward_winograd zeroes the layer plan but not the Winograd scratch behind it: that scratch is 0xFF here."""
    lib = _lib.load()
    kind, B, cin, cout, H, W, act = case
    x, w, b = _layer_data(kind, B, cin, cout, H, W)
    k = _lib.KIND[kind]
    nbytes = lib.nd_winograd_packed_bytes(tile, cin, cout)
    packed = torch.empty(nbytes // 4, dtype=F32)
    _lib.check(lib.nd_winograd_pack(tile, k, cin, cout, w.contiguous().data_ptr(), b.data_ptr(), packed.data_ptr(), nbytes))

    def body(a):
        pk, xg, y = a.copy("packed weights", packed), a.copy("x", x), a.out("y", (B, cout) + _out_hw(kind, H, W))
        wsb = lib.nd_layer_winograd_workspace_bytes(tile, k, B, cin, cout, H, W)
        ws = a.scratch("workspace", wsb)
        _lib.check(lib.nd_layer_forward_winograd(tile, k, _lib.ACT[act], 0.13, pk.data_ptr(), xg.data_ptr(), B, cin, H, W, cout,
                                                 y.data_ptr(), ws.data_ptr(), wsb, 0, _sp(dev)), "nd_layer_forward_winograd")
        return y

    y = _both(dev, body, f"nd_layer_forward_winograd tile {tile}")
    _HP.assert_close(y, _ref_layer64(kind, x, w, b, act, 0.13), f"tile {tile} {case}")


# the first-layer, the convT2s2 and the 128 x 72 cases of test_hip_parity.WGRAD_CASES, and a single image with a 3 x 3 gradient: K (9
# pixels) shorter than one 62-pixel chunk
WGRADS = [_first(_HP.WGRAD_CASES, lambda c: c[2] == 3), _first(_HP.WGRAD_CASES, lambda c: c[0] == "convT2s2"),
          _first(_HP.WGRAD_CASES, lambda c: (c[2], c[3]) == (128, 72)), ("conv3", 1, 16, 32, 5, 5)]


@pytest.mark.parametrize("case", WGRADS, ids=lambda c: "-".join(str(v) for v in c))
def test_layer_wgrad_guarded(dev, case):
    lib = _lib.load()
    kind, B, cin, cout, H, W = case
    x, w, _ = _layer_data(kind, B, cin, cout, H, W)
    dy = _HP.rnd((B, cout) + _out_hw(kind, H, W), 4)

    def body(a):
        xg, dyg, dw, db = a.copy("x", x), a.copy("dy", dy), a.out("dw", w.shape), a.out("db", (cout,))
        wsb = lib.nd_layer_wgrad_workspace_bytes(_lib.KIND[kind], B, cin, cout, H, W)
        ws = a.scratch("workspace", wsb)
        _lib.check(lib.nd_layer_wgrad(_lib.KIND[kind], xg.data_ptr(), dyg.data_ptr(), B, cin, H, W, cout, dw.data_ptr(), db.data_ptr(),
                                      ws.data_ptr(), wsb, _sp(dev)), "nd_layer_wgrad")
        return dw, db

    dw, db = _both(dev, body, "nd_layer_wgrad")
    w64 = w.double().requires_grad_()
    b64 = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x.double(), w64, b64) if kind == "conv3" else F.conv_transpose2d(x.double(), w64, b64, stride=2)
    y.backward(dy.double())
    for got, ref, what in ((dw, w64.grad, "dW"), (db, b64.grad, "db")):      # the bar of test_weight_gradient_vs_autograd
        err = (got.cpu().double() - ref).abs().max().item()
        assert err <= _HP.WGRAD_REL_TOL * max(ref.abs().max().item(), 1.0) + _HP.WGRAD_ABS_TOL, (case, what, err)


def test_maxpool_guarded(dev):
    lib = _lib.load()
    b, c, h, w = _first(_HP.MAXPOOL_SHAPES, lambda q: q[2] % 2 == 1 and q[3] % 2 == 1)      # test_hip_parity.test_maxpool's odd case
    x = _HP.rnd((b, c, h, w), 5)

    def body(a):
        xg, y = a.copy("x", x), a.out("y", (b, c, h // 2, w // 2))
        planes = (c + 3) // 4
        need = ((planes * b * h * w * 16 + 255) & ~255) + planes * b * (h // 2) * (w // 2) * 16
        ws = a.scratch("workspace", need)
        _lib.check(lib.nd_maxpool2_forward(xg.data_ptr(), b, c, h, w, y.data_ptr(), ws.data_ptr(), need, _sp(dev)), "nd_maxpool2_forward")
        with pytest.raises(MemoryError):                               # (the size above is the least the entry point takes)
            _lib.check(lib.nd_maxpool2_forward(xg.data_ptr(), b, c, h, w, y.data_ptr(), ws.data_ptr(), need - 1, _sp(dev)))
        return y

    assert torch.equal(_both(dev, body, "nd_maxpool2_forward").cpu(), F.max_pool2d(x, 2))


# ============================================================================ criteria and scores

SCORE_SHAPES = [(2, 3, 40, 57), (1, 3, 163, 201)]                    # odd sides; five scales


def _score_pair(shape, seed=7):
    x = _rnd(shape, seed)
    return x, (x + 0.1 * (_rnd(shape, seed + 1) - 0.5)).clip(0, 1)


@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_scores_guarded(dev, shape):
    """nd_mse, nd_ssim, nd_ms_ssim, nd_ssim_loss_grad (both modes), nd_ssim_padded and its gradient."""
    from oracle import losses as olosses
    lib = _lib.load()
    n, c, h, w = shape
    x, y = _score_pair(shape)
    multi = h >= 161 and w >= 161
    gout = _rnd((n,), 3, 0.5, 1.5)

    def body(a):
        xg, yg = a.copy("x", x), a.copy("y", y)
        res = {}
        ws = a.scratch("mse workspace", 4096)
        res["mse"] = a.out("mse", (1,))
        _lib.check(lib.nd_mse(xg.data_ptr(), yg.data_ptr(), x.numel(), res["mse"].data_ptr(), ws.data_ptr(), 4096, _sp(dev)), "nd_mse")
        wsb = lib.nd_ssim_workspace_bytes(n, c, h, w)
        ws1 = a.scratch("ssim workspace", wsb)
        res["ssim"] = a.out("ssim", (n,))
        _lib.check(lib.nd_ssim(xg.data_ptr(), yg.data_ptr(), n, c, h, w, res["ssim"].data_ptr(), ws1.data_ptr(), wsb, _sp(dev)), "nd_ssim")
        if multi:
            ws2 = a.scratch("ms-ssim workspace", wsb)
            res["msssim"] = a.out("msssim", (n,))
            _lib.check(lib.nd_ms_ssim(xg.data_ptr(), yg.data_ptr(), n, c, h, w, res["msssim"].data_ptr(), ws2.data_ptr(), wsb, _sp(dev)),
                       "nd_ms_ssim")
        for mode in ((0, 1) if multi else (0,)):
            lb = lib.nd_ssim_loss_workspace_bytes(n, c, h, w)
            ws3 = a.scratch(f"loss workspace {mode}", lb)
            res[f"loss{mode}"], res[f"gx{mode}"] = a.zeros(f"loss {mode}", (1,)), a.out(f"gx {mode}", shape)      # (the loss is accumulated)
            _lib.check(lib.nd_ssim_loss_grad(xg.data_ptr(), yg.data_ptr(), n, c, h, w, mode, 0.7, res[f"loss{mode}"].data_ptr(),
                                             res[f"gx{mode}"].data_ptr(), 0, ws3.data_ptr(), lb, _sp(dev)), "nd_ssim_loss_grad")
        pb = lib.nd_ssim_padded_workspace_bytes(n, c, h, w, 11)
        ws4, ws5 = a.scratch("padded workspace", pb), a.scratch("padded grad workspace", pb)
        res["padded"], res["padded_gx"], go = a.out("padded", (n,)), a.out("padded gx", shape), a.copy("gout", gout)
        _lib.check(lib.nd_ssim_padded(xg.data_ptr(), yg.data_ptr(), n, c, h, w, 11, res["padded"].data_ptr(), ws4.data_ptr(), pb, _sp(dev)),
                   "nd_ssim_padded")
        _lib.check(lib.nd_ssim_padded_grad(xg.data_ptr(), yg.data_ptr(), n, c, h, w, 11, go.data_ptr(), res["padded_gx"].data_ptr(),
                                           ws5.data_ptr(), pb, _sp(dev)), "nd_ssim_padded_grad")
        return res

    res = _both(dev, body, "scores")
    # the link to float64 (family: scores), at test_eval_harness.SCORE_TOL
    tol = _load("test_eval_harness").SCORE_TOL
    assert (res["ssim"].cpu().double() - olosses.ssim(x.double(), y.double())).abs().max().item() <= tol
    if multi:
        assert (res["msssim"].cpu().double() - olosses.ms_ssim(x.double(), y.double())).abs().max().item() <= tol


@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_criteria_guarded(dev, shape):
    lib = _lib.load()
    n, _, h, w = shape
    y, t = _score_pair(shape)
    y = y * 1.2 - 0.1                                                  # (the clip to [0, 1] has something to do)
    multi = h >= 161 and w >= 161
    wts = (0.2, 0.2, 0.2, 0.4 if multi else 0.0)
    loss_cs = 161 if multi else 33

    def body(a):
        yg, tg = a.copy("y", y), a.copy("target", t)
        cb = lib.nd_criteria_workspace_bytes(n, h, w, loss_cs)
        ws, out = a.scratch("criteria workspace", cb), a.out("out", (n, 5))
        _lib.check(lib.nd_criteria(yg.data_ptr(), tg.data_ptr(), n, h, w, loss_cs, *wts, 0, out.data_ptr(), ws.data_ptr(), cb, _sp(dev)),
                   "nd_criteria")
        gb = lib.nd_criteria_grad_workspace_bytes(n, h, w, loss_cs)
        ws2, loss, gy = a.scratch("criteria_grad workspace", gb), a.out("loss", (1,)), a.out("gy", shape)
        _lib.check(lib.nd_criteria_grad(yg.data_ptr(), tg.data_ptr(), n, h, w, loss_cs, *wts, loss.data_ptr(), gy.data_ptr(), ws2.data_ptr(),
                                        gb, _sp(dev)), "nd_criteria_grad")
        return out, loss, gy

    _both(dev, body, "nd_criteria / nd_criteria_grad")


def test_validation_scratch_after_a_nan_batch_of_another_shape(dev):
    """validation._workspace is one grown-on-demand torch.empty buffer shared by nd_criteria / nd_criteria_grad calls of every shape."""
    from nind_denoise_amd import validation
    wts = {"L1": 0.2, "MSE": 0.2, "SSIM": 0.2, "MSSSIM": 0.4}
    big = torch.full((2, 3, 184, 184), NAN, device=dev)
    y, t = (v.to(dev) for v in _score_pair((2, 3, 168, 168)))

    def real():
        c = validation.criteria(y, t, wts, 161)
        loss, gy = validation.criteria_grad(y, t, wts, 161)
        return {k: v.clone() for k, v in c.items()}, loss.clone(), gy.clone()

    def flood():
        validation.criteria(big, big, wts, None)
        validation.criteria_grad(big, big, wts, None)

    def fresh():
        # a zeroed buffer of this shape's size put where the module caches its scratch: after clear() alone, torch.empty would most
        # likely hand back the same, still NaN-dirty block, and only the finite check would carry the case
        lib = _lib.load()
        nbytes = max(lib.nd_criteria_workspace_bytes(2, 168, 168, 161), lib.nd_criteria_grad_workspace_bytes(2, 168, 168, 161))
        validation._workspaces.clear()
        validation._workspaces[str(y.device)] = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        return real()

    validation._workspaces.clear()
    G.flood_then(flood, real, fresh, "validation.criteria / criteria_grad")


# ============================================================================ tiler and batches

def test_tiler_and_its_adjoints_guarded(dev):
    """nd_tile_gather, nd_stitch_add, nd_stitch_grad, nd_tile_gather_grad on the smallest geometry of tests/golden/tiler_geoms.json."""
    from oracle import tiler as otiler
    lib = _lib.load()
    g = min(_HP._geoms(), key=lambda q: q["W"] * q["H"])
    W, H, cs, ucs, ol = (g[k] for k in ("W", "H", "cs", "ucs", "ol"))
    frame = synth.make_frame(W, H, seed=g["seed"])
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    begin, count = 1, grid.size - 1                                    # (a range that starts inside the first tile row)
    tiles_in = _HP.rnd((count, 3, cs, cs), 2)

    def body(a):
        img, tiles = a.copy("frame", torch.from_numpy(frame)), a.out("tiles", (count, 3, cs, cs))
        _lib.check(lib.nd_tile_gather(img.data_ptr(), W, H, cs, ucs, ol, begin, count, tiles.data_ptr(), _sp(dev)), "nd_tile_gather")
        canvas, tin = a.zeros("canvas", (3, H, W)), a.copy("tile outputs", tiles_in)
        _lib.check(lib.nd_stitch_add(canvas.data_ptr(), W, H, cs, ucs, ol, tin.data_ptr(), begin, count, _sp(dev)), "nd_stitch_add")
        gt = a.out("gtiles", (count, 3, cs, cs))
        _lib.check(lib.nd_stitch_grad(img.data_ptr(), W, H, cs, ucs, ol, begin, count, gt.data_ptr(), _sp(dev)), "nd_stitch_grad")
        gimg = a.zeros("gimg", (3, H, W))
        _lib.check(lib.nd_tile_gather_grad(tin.data_ptr(), W, H, cs, ucs, ol, begin, count, gimg.data_ptr(), _sp(dev)), "nd_tile_gather_grad")
        return tiles, canvas, gt, gimg

    tiles, canvas, _, _ = _both(dev, body, "tiler")
    ref = np.zeros((3, H, W), dtype=np.float32)
    for i in range(count):
        assert np.array_equal(tiles[i].cpu().numpy(), otiler.gather_tile(frame, grid, begin + i))
        otiler.stitch_add(ref, tiles_in[i].numpy(), grid, begin + i)
    assert np.array_equal(canvas.cpu().numpy(), ref)


def test_crop_batch_with_the_device_drawn_multiplier_guarded(dev):
    from nind_denoise_amd.crop_pool import CropPool, pack_draws
    lib = _lib.load()
    cs = _CP.CS
    rng = np.random.default_rng(5)
    srcs = [[rng.integers(0, 256, (3, 40, 36)).astype(np.uint8) for _ in range(2)],
            [rng.integers(0, 30000, (3, 33, 40)).astype(np.uint16) for _ in range(2)],
            [rng.uniform(0.0, 0.7, (3, 20, 40)).astype(np.float32) for _ in range(2)]]       # the last: padded in y
    pool = CropPool(dev, cs=cs)
    for c, n in srcs:
        pool.add_group([c], [n])
    rows = []
    for gi in range(len(srcs)):
        cl, no, h, w = pool.group(gi)
        rows += [(cl[0], no[0], max(w - cs, 0), max(h - cs, 0), gi + 1, gi & 1, 1), (cl[0], no[0], 0, 0, 0, 0, 0)]
    table = pack_draws(*zip(*rows), [0.37] * len(rows))
    n = len(rows)
    want = pool.batch(table, cs, exp_mult_min=0.8, exp_mult_max=1.3)     # the existing way
    bytes_, images = pool._upload()

    def body(a):
        pb, im, dr = a.copy("pool", bytes_), a.copy("image table", images), a.copy("draws", torch.as_tensor(table))
        xmax, mult, clean, noisy = a.out("xmax", (n,)), a.out("mult", (n,)), a.out("clean", (n, 3, cs, cs)), a.out("noisy", (n, 3, cs, cs))
        _lib.check(lib.nd_crop_batch(pb.data_ptr(), pb.numel(), im.data_ptr(), im.shape[0], dr.data_ptr(), n, cs, 0.8, 1.3, None,
                                     xmax.data_ptr(), mult.data_ptr(), clean.data_ptr(), noisy.data_ptr(), _sp(dev)), "nd_crop_batch")
        return clean, noisy, xmax, mult

    got = _both(dev, body, "nd_crop_batch")
    G.assert_same(got, (want[0], want[1], pool.last_xmax, pool.last_mult), "nd_crop_batch guarded vs CropPool.batch")


def test_adam_step_guarded(dev):
    lib = _lib.load()
    n = 257
    p0, g0 = _rnd((n,), 1, -1, 1), _rnd((n,), 2, -1, 1)

    def body(a):
        p, g, m, v, vmax = a.copy("params", p0), a.copy("grads", g0), a.zeros("m", (n,)), a.zeros("v", (n,)), a.zeros("vmax", (n,))
        for step in (1, 2):
            _lib.check(lib.nd_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), vmax.data_ptr(), n, 1e-3, 0.75, 0.999, 1e-8,
                                        step, 1, _sp(dev)), "nd_adam_step")
        return p, m, v, vmax

    p, *_ = _both(dev, body, "nd_adam_step")
    ref = p0.clone().requires_grad_()
    opt = torch.optim.Adam([ref], lr=1e-3, betas=(0.75, 0.999), amsgrad=True)
    for _ in range(2):
        ref.grad = g0.clone()
        opt.step()
    # both sides work in fp32 on |p| <= 1: each of the two steps rounds p once on either side (half an ulp of 1 = 2^-24 each); the
    # update itself, lr * m / (sqrt(v) + eps) ~ 1e-3, carries a few ulps of 1e-3 (< 1e-9).  4 x 2^-24 in the worst case; bar 4x that
    assert (p.cpu() - ref.detach()).abs().max().item() <= 16 * 2.0 ** -24
