"""UNet(winograd=True) -- ND_FLAG_UNET_WINOGRAD: the fused F(4,3) and three-pass F(6x6,3x3) forms of the 3x3 layers -- against float64.

The cases, the visible weights, the float64 references and the CPU gate are those of tests/test_unet_float64.py (imported, not
restated).  CPU: the shapes show every tile remainder to every Winograd layer, and the bar sees a 1 % error at every level of every
case.  GPU: UNet.forward and the frame loop against float64; two inputs through one workspace; the workspace contract (guards, NaN
flood); host-packed against device-packed blob; the command line; and that the parameter leaves the gradients' bits alone."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib, pipeline

import test_unet_float64 as U64
import workspace_guard as G

WINO = _lib.FLAG_UNET_WINOGRAD

# The bar of every comparison with float64 below: the one the project grants an fp32 UNet path (BAR_UNET_FRAME = 1e-5), which the
# gate of tests/test_unet_float64.py shows to lie 10x under what a 1 % error at any level moves (run here for the added shapes too).
# Measured worst on MI355X: 7.86e-6 (the forward at 1x256x256); per case in MEASURED below.
BAR = U64.BAR_UNET_FRAME
assert BAR == 1e-5

# Three more small shapes (B, h, w).  The issue asks for two; two cannot do it: a three-pass layer's height is h // 4 (down2,
# up2.conv.0), h // 8 (down3, up1) or h // 16 (down4), and after the given cases the heights still lack residue 5 at h // 4 and 1
# and 3 at h // 8 (and 3 at h // 16).  h // 4 = 5 (mod 6) forces h // 8 = 2 or 5 (mod 6), and h // 8 = 3 (mod 6) forces
# h // 4 = 0 or 1: one shape for each, and a third for h // 8 = 1 with h // 16 = 3.
#   61 x 57: h // 4, 8, 16 = 15, 7, 3 (3, 1, 3 mod 6); w = 14, 7, 3 (2, 1, 3); all four fix-ups in h
#   27 x 37: h // 8 = 3; w // 8 = 4
#   23 x 18: h // 4 = 5
EXTRA_SHAPES = [(1, 61, 57), (2, 27, 37), (1, 23, 18)]
FWD_CASES = U64.FWD_CASES + [(3, False, s) for s in EXTRA_SHAPES]
FRAME_MODES = {"fused": {}, "no_splitk": {"split_k": False}, "full_tiles": {"useful_only": False}}

# max |y - float64| measured on MI355X per case (each test prints its own figure before it asserts)
MEASURED = {
    "forward": {"seed0-1x16x16": 8.21e-07, "seed3-1x16x16": 7.46e-07, "seed0-2x17x31": 1.06e-06, "seed3-2x17x31": 1.12e-06,
                "seed0-3x33x47": 2.96e-06, "seed3-3x33x47": 2.76e-06, "seed0-2x100x92": 4.80e-06, "seed3-2x100x92": 5.30e-06,
                "seed0-1x64x16": 1.10e-06, "seed3-1x64x16": 1.29e-06, "seed0-1x256x256": 7.86e-06, "seed3-1x61x57": 2.95e-06,
                "seed3-2x27x37": 1.33e-06, "seed3-1x23x18": 9.82e-07},
    "frame": {"seed3-cs90": {"fused": 4.08e-06, "no_splitk": 5.75e-06, "full_tiles": 4.53e-06},
              "seed0-cs96": {"fused": 4.41e-06, "no_splitk": 7.48e-06, "full_tiles": 5.42e-06}},
    "second input through one workspace": {"2x100x92": 5.87e-06, "1x61x57": 4.37e-06},
}

THREE_PASS_LEVELS = (2, 3, 4)     # down2 / up2.conv.0, down3 / up1.conv.*, down4
F43_LEVELS = (0, 1, 2)            # inc.3 / up4.conv.*, down1 / up3.conv.*, up2.conv.3


def _seen_extents():
    """{level: (heights, widths)} of the whole layers over the forward cases and the frame tiles, plus the regions the restricted
    decoder layers of the frame cases run on (nd_unet_useful_region: square)."""
    lib = _lib.load()
    seen = {lvl: (set(), set()) for lvl in range(5)}
    for _, _, (_, h, w) in FWD_CASES:
        for lvl in range(5):
            seen[lvl][0].add(h >> lvl)
            seen[lvl][1].add(w >> lvl)
    names = [lib.nd_unet_step_name(i).decode() for i in range(lib.nd_unet_num_steps())]
    level_of = {"up1": 3, "up2": 2, "up3": 1, "up4": 0}
    for _, (W, H, cs, ucs, ol, batch) in U64.FRAME_CASES:
        for lvl in range(5):
            seen[lvl][0].add(cs >> lvl)
            seen[lvl][1].add(cs >> lvl)
        rect = (ctypes.c_int * 4)()
        for i, n in enumerate(names):
            if n == "pool" or n.endswith(".up") or n.split(".")[0] not in level_of:
                continue
            assert lib.nd_unet_useful_region(cs, (cs - ucs) // 2, i, rect) >= 0
            if rect[2] > 0:
                seen[level_of[n.split(".")[0]]][0].add(rect[2])
                seen[level_of[n.split(".")[0]]][1].add(rect[3])
    return seen


def test_cases_show_every_tile_remainder_to_every_winograd_layer():
    seen = _seen_extents()
    for lvl in THREE_PASS_LEVELS:
        for axis, name in ((0, "height"), (1, "width")):
            assert {v % 6 for v in seen[lvl][axis]} == set(range(6)), (lvl, name, sorted(seen[lvl][axis]))
    for lvl in F43_LEVELS:
        assert {v % 4 for v in seen[lvl][1]} == set(range(4)), (lvl, sorted(seen[lvl][1]))
    # more than one image, more than one F(6x6) tile per side and one-tile images are all there
    assert any(b > 1 for _, _, (b, _, _) in FWD_CASES)
    assert min(seen[4][0]) == 1 and max(seen[2][0]) > 12


@pytest.mark.parametrize("case", [(seed, planted, "fwd", shape, 0, (BAR,)) for seed, planted, shape in FWD_CASES], ids=U64._gate_id)
def test_bar_sees_every_level_of_every_forward_case(case):
    # (the frame cases are gated at this bar by tests/test_unet_float64.py itself)
    U64.test_gpu_bars_see_every_level_and_fixup(case)


# ---------------------------------------------------------------------------- GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _net(dev, seed, winograd=True, **attrs):
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    net = UNet(winograd=winograd)
    net.load_state_dict(U64._sd(seed))
    for k, v in attrs.items():
        setattr(net, k, v)
    return net.eval().to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=U64._case_id)
def test_forward_vs_float64(dev, case):
    seed, planted, shape = case
    x, ref = U64._ref(seed, planted, shape)
    net = _net(dev, seed)
    e = U64._err(net(x.to(dev)), ref)
    print(f"UNet winograd {U64._case_id(case)}: forward vs float64 {e:.2e}")
    assert e <= BAR, e


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FRAME_MODES))
@pytest.mark.parametrize("case", U64.FRAME_CASES, ids=lambda c: "seed{}-{}x{}-{}-{}-{}-b{}".format(c[0], *c[1]))
def test_frame_vs_float64(dev, case, mode):
    seed, geom = case
    W, H, cs, ucs, ol, batch = geom
    ref = U64._frame_ref(seed, geom)
    img = torch.from_numpy(U64._frame(geom)).to(dev)
    out = pipeline.denoise_frame(_net(dev, seed, **FRAME_MODES[mode]), img, cs, ucs, ol, batch=batch)
    e = U64._err(out, torch.from_numpy(ref).double())
    print(f"UNet winograd seed {seed} {geom} {mode}: canvas vs float64 tiler {e:.2e}")
    assert e <= BAR, e


@functools.lru_cache(maxsize=None)
def _second_ref(seed, shape):
    """Another input of `shape` for the weights of `seed`."""
    from oracle import networks as onet
    x = U64._input(seed + 11, shape)
    with torch.no_grad():
        return x, onet.unet_forward(U64._sd64(seed), x.double())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 100, 92), (1, 61, 57)], ids=lambda s: "x".join(map(str, s)))
def test_two_inputs_through_one_workspace(dev, shape):
    # a border that a Winograd launch dirtied, or scratch it did not rewrite, is the first input's: it shows in the second result
    seed = 3
    net = _net(dev, seed)
    x1, ref1 = U64._ref(seed, False, shape)
    x2, ref2 = _second_ref(seed, shape)
    y1 = net(x1.to(dev))
    y2 = net(x2.to(dev))
    assert len(net._workspaces) == 1
    e1, e2 = U64._err(y1, ref1), U64._err(y2, ref2)
    print(f"UNet winograd {shape}: first input {e1:.2e}, second input through the same workspace {e2:.2e} vs float64")
    assert e1 <= BAR and e2 <= BAR, (e1, e2)
    assert torch.equal(y2, _net(dev, seed)(x2.to(dev)))          # and bit for bit what a fresh module gives
    assert torch.equal(net(x1.to(dev)), y1)


def _pack_guarded(handles, dev, net, flags):
    lib = _lib.load()
    sd, n = net.state_dict(), lib.nd_unet_num_tensors()
    ptrs, keep = (ctypes.c_void_p * n)(), []
    for i in range(n):
        name = lib.nd_unet_tensor_name(i).decode()
        t, handles["tensor " + name] = G.typed_like(sd[name].detach().to(torch.float32).contiguous().to(dev))
        keep.append(t)
        ptrs[i] = t.data_ptr()
    nbytes = lib.nd_unet_packed_bytes_flags(_lib.ND_F32, flags)
    blob, handles["packed weights"] = G.guarded(nbytes, dev, fill=0xFF)
    _lib.check(lib.nd_unet_pack_weights_device_flags(_lib.ND_F32, flags, ptrs, n, blob.data_ptr(), nbytes, _lib.stream_ptr(dev)),
               "nd_unet_pack_weights_device_flags")
    torch.cuda.synchronize()
    return blob


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 33, 47), (1, 61, 57)], ids=lambda s: "x".join(map(str, s)))
def test_forward_guarded_and_after_a_nan_batch(dev, shape):
    lib = _lib.load()
    seed = 3
    b, h, w = shape
    x, ref = U64._ref(seed, False, shape)
    used = _net(dev, seed)
    xd = x.to(dev)
    plain = used(xd)
    handles = {}
    blob = _pack_guarded(handles, dev, used, WINO)
    xg, handles["x"] = G.typed_like(xd)
    y, handles["y"] = G.typed(xd.shape, torch.float32, dev, fill=0xFF)
    nbytes = lib.nd_unet_workspace_bytes_flags(h, w, b, _lib.ND_F32, WINO)
    assert nbytes > lib.nd_unet_workspace_bytes(h, w, b, _lib.ND_F32)
    ws, handles["workspace"] = G.guarded(nbytes, dev, fill=0xFF)          # NaN everywhere before the init call
    _lib.check(lib.nd_unet_workspace_init_flags(ws.data_ptr(), nbytes, h, w, b, _lib.ND_F32, WINO, _lib.stream_ptr(dev)), "init")
    _lib.check(lib.nd_unet_forward_flags(_lib.ND_F32, WINO, blob.data_ptr(), xg.data_ptr(), y.data_ptr(), b, h, w, ws.data_ptr(), nbytes,
                                         _lib.stream_ptr(dev)), "nd_unet_forward_flags")
    torch.cuda.synchronize()
    G.assert_all_guards(handles, "nd_unet_forward_flags")
    G.assert_same(y, plain, "nd_unet_forward_flags guarded vs the module")
    assert torch.equal(blob, used.packed_weights(dev).view(torch.uint8).reshape(-1))
    # a workspace sized without the flag is refused, not overrun
    small = lib.nd_unet_workspace_bytes(h, w, b, _lib.ND_F32)
    assert lib.nd_unet_forward_flags(_lib.ND_F32, WINO, blob.data_ptr(), xg.data_ptr(), y.data_ptr(), b, h, w, ws.data_ptr(), small,
                                     _lib.stream_ptr(dev)) == -2
    G.flood_then(lambda: used(torch.full_like(xd, float("nan"))), lambda: used(xd), lambda: _net(dev, seed)(xd), "UNet(winograd).forward")
    e = U64._err(plain, ref)
    print(f"UNet winograd {shape} guarded forward vs float64 {e:.2e}")
    assert e <= BAR, e


@pytest.mark.gpu
def test_frame_after_a_nan_frame(dev):
    seed, geom = U64.FRAME_CASES[0]
    W, H, cs, ucs, ol, batch = geom
    img = torch.from_numpy(U64._frame(geom)).to(dev)
    used = _net(dev, seed)
    G.flood_then(lambda: pipeline.denoise_frame(used, torch.full_like(img, float("nan")), cs, ucs, ol, batch=batch),
                 lambda: pipeline.denoise_frame(used, img, cs, ucs, ol, batch=batch),
                 lambda: pipeline.denoise_frame(_net(dev, seed), img, cs, ucs, ol, batch=batch), "UNet(winograd) frame loop")


@pytest.mark.gpu
def test_host_and_device_blobs_are_the_same_bytes(dev):
    seed, planted = U64.PLANTED_CASE[:2]                          # negative and zero BatchNorm weights in the fold
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    blobs = {}
    for on_device in (True, False):
        net = UNet(winograd=True)
        net.load_state_dict(U64._sd(seed, planted))
        net.pack_on_device = on_device
        blobs[on_device] = net.eval().to(dev).packed_weights(dev).view(torch.int32).cpu()
    lib = _lib.load()
    assert blobs[True].numel() * 4 == lib.nd_unet_packed_bytes_flags(_lib.ND_F32, WINO)
    ne = blobs[True] != blobs[False]
    assert not ne.any(), f"{int(ne.sum())} of {ne.numel()} words differ, the first at {int(ne.nonzero()[0])}"
    plain = _net(dev, seed, winograd=False)
    plain.load_state_dict(U64._sd(seed, planted))
    head = plain.packed_weights(dev).view(torch.int32).cpu()
    assert torch.equal(blobs[True][:head.numel()], head)          # the default blob's words, where they were


@pytest.mark.gpu
def test_cli_runs_the_winograd_forms(dev, tmp_path):
    from nind_denoise_amd import denoise_image as di, synth
    from nind_denoise_amd.common.libs import imgcodec, np_imgops
    seed, (W, H, cs, ucs, ol) = 0, (96, 80, 48, 32, 4)
    torch.save(U64._sd(seed), tmp_path / "generator_1.pt")
    frame = synth.make_frame(W, H, seed=5)
    imgcodec.write_png(str(tmp_path / "in.png"), np.ascontiguousarray((frame.transpose(1, 2, 0) * 255 + 0.5).astype(np.uint8)))
    common = ["--network", "UNet", "--model_path", str(tmp_path / "generator_1.pt"), "--input", str(tmp_path / "in.png"), "--cs", str(cs),
              "--ucs", str(ucs), "--overlap", str(ol), "--exif_method", "noexif"]
    assert di.main(common + ["--model_parameters", "winograd=1", "--output", str(tmp_path / "wino.tif")]) == 0
    assert di.main(common + ["--output", str(tmp_path / "plain.tif")]) == 0
    img = np_imgops.img_path_to_device_flt(str(tmp_path / "in.png"), dev)
    want = {w: di.denoise_file(_net(dev, seed, winograd=w), str(tmp_path / "in.png"), str(tmp_path / f"module_{w}.tif"), cs, ucs, ol,
                               batch=64, device=dev, verbose=False) for w in (True, False)}
    assert img.shape == (3, H, W) and torch.isfinite(want[True]).all()
    assert not torch.equal(want[True], want[False]), "winograd=True changed nothing"
    for cli, w in (("wino.tif", True), ("plain.tif", False)):
        got, mod = (np_imgops.img_path_to_np_flt(str(tmp_path / f)) for f in (cli, f"module_{w}.tif"))
        assert got.shape == (3, H, W) and np.array_equal(got, mod), cli
    assert torch.equal(want[True], pipeline.denoise_frame(_net(dev, seed), img, cs, ucs, ol, batch=64))


@pytest.mark.gpu
def test_winograd_is_inference_only(dev):
    shape = (2, 17, 31)
    x, _ = U64._ref(3, False, shape)
    out = {}
    for w in (True, False):
        net = _net(dev, 3, winograd=w)
        xd = x.to(dev).requires_grad_()
        y = net(xd)
        (y * torch.linspace(0.5, 1.5, y.numel(), device=dev).view_as(y)).sum().backward()
        out[w] = (y.detach().clone(), xd.grad.clone())
        assert torch.isfinite(xd.grad).all() and xd.grad.abs().max() > 0
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])
    # ... while the inference path of the same module does run the Winograd forms
    with torch.no_grad():
        assert not torch.equal(_net(dev, 3)(x.to(dev)), _net(dev, 3, winograd=False)(x.to(dev)))
