"""GPU tests of UNet on the fused frame loop (nd_unet_denoise_frame) and of the device-side weight packer.

Bars: 0.0 between two launches of the same tiles with the split-K tail off (a pixel's K loop in the direct kernel does not depend on
the launch: the rule tests/test_roi.py holds the direct kernels to); 3e-6 where fp32 sums may re-associate (split-K on, or the fused
stitch against the separate final 1x1 + stitch) -- outputs are sigmoids, so the scale is 1; the project's fp32 parity bar against the
oracle (max abs <= 1e-3 and <= 1e-3 * max|ref|).

Geometry note: the 440/320/6 frame is 500x347, not 500x330: nd_tile_grid refuses 500x330 (the second tile row would mirror 364
rows of a 330-row frame, which the reference's numpy slices cannot do either); 347 is the smallest height with the same four tiles."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib, pipeline, synth
from nind_denoise_amd.networks.ThirdPartyNets import UNet

pytestmark = pytest.mark.gpu

REASSOC_BAR = 3e-6
ABS_TOL = REL_TOL = 1e-3

# (W, H, cs, ucs, ol, batch)
GEOMS = [(200, 170, 96, 64, 8, 5), (230, 190, 100, 68, 10, 3), (210, 160, 90, 61, 7, 4), (200, 180, 80, 76, 4, 6),
         (220, 200, 96, 8, 2, 7), (500, 347, 440, 320, 6, 4)]
IDS = [f"{g[0]}x{g[1]}-{g[2]}/{g[3]}/{g[4]}-b{g[5]}" for g in GEOMS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def make_net(dev, sd=None, **attrs):
    net = UNet(find_noise=attrs.pop("find_noise", False))
    net.load_state_dict(sd if sd is not None else synth.make_unet_state_dict(seed=0))
    for k, v in attrs.items():
        setattr(net, k, v)
    return net.eval().to(dev)


@functools.lru_cache(maxsize=None)
def frame(W, H):
    return torch.from_numpy(synth.make_frame(W, H, seed=W + H)).cuda()


@functools.lru_cache(maxsize=None)
def fused(geom, split_k=True, useful_only=True, find_noise=False):
    """Canvas of the fused loop, computed once per (geometry, switches) and shared by the tests (never modified)."""
    W, H, cs, ucs, ol, batch = geom
    net = make_net(torch.device("cuda:0"), split_k=split_k, useful_only=useful_only, find_noise=find_noise)
    out = pipeline.denoise_frame(net, frame(W, H), cs, ucs, ol, batch=batch)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


@functools.lru_cache(maxsize=None)
def generic(geom, find_noise=False):
    """The explicit generic path: nd_tile_gather -> UNet.forward -> nd_stitch_add, same launches."""
    W, H, cs, ucs, ol, batch = geom
    net = make_net(torch.device("cuda:0"), find_noise=find_noise)
    img = frame(W, H)
    canvas = torch.zeros_like(img)
    for t0 in range(0, pipeline.tile_count(W, H, cs, ucs, ol), batch):
        cnt = min(batch, pipeline.tile_count(W, H, cs, ucs, ol) - t0)
        pipeline.stitch_tiles(canvas, net(pipeline.gather_tiles(img, cs, ucs, ol, t0, cnt)), cs, ucs, ol, t0)
    torch.cuda.synchronize()
    return canvas


def maxdiff(a, b):
    return (a - b).abs().max().item()


# ------------------------------------------------------------------------------------------------ 1. device packer
def planted_state_dict():
    """BatchNorm statistics planted per channel: negative and zero weight, running_var 0 and 1e-12, large running_mean."""
    sd = synth.make_unet_state_dict(seed=3)
    for k in list(sd):
        if k.endswith(".running_var"):
            p = k[:-len("running_var")]
            n = sd[k].numel()
            sd[p + "weight"][0::7] *= -1.0
            sd[p + "weight"][3::11] = 0.0
            sd[k][1::5] = 0.0
            sd[k][2::9] = 1e-12
            sd[p + "running_mean"][4::6] = 1.0e4
            sd[p + "running_mean"][5::13] = -3.0e5
            assert n >= 64
    return sd


@pytest.mark.parametrize("planted", [False, True], ids=["synth", "planted_bn"])
def test_device_packed_blob_equals_host_packed_blob(dev, planted):
    sd = planted_state_dict() if planted else synth.make_unet_state_dict(seed=0)
    on_dev, on_host = make_net(dev, sd, pack_on_device=True), make_net(dev, sd, pack_on_device=False)
    a, b = on_dev.packed_weights(dev), on_host.packed_weights(dev)
    torch.cuda.synchronize()
    ai, bi = a.view(torch.int32), b.view(torch.int32)
    assert ai.shape == bi.shape
    bad = (ai != bi).nonzero().flatten()
    assert bad.numel() == 0, f"{bad.numel()} words differ, first at {bad[:4].tolist()}"
    g = torch.Generator().manual_seed(9)
    for shape in ((1, 3, 256, 256), (2, 3, 100, 92)):
        x = torch.rand(shape, generator=g).to(dev)
        # as words: torch.equal that also holds where the planted statistics saturate the sigmoid or overflow a layer
        assert torch.equal(on_dev(x).view(torch.int32), on_host(x).view(torch.int32)), shape


def test_device_packer_arguments(dev):
    lib = _lib.load()
    n = lib.nd_unet_num_tensors()
    ptrs = (ctypes.c_void_p * n)()
    blob = torch.empty(lib.nd_unet_packed_bytes(_lib.ND_F32) // 4, device=dev)
    s = _lib.stream_ptr(dev)
    assert lib.nd_unet_pack_weights_device(_lib.ND_BF16, ptrs, n, blob.data_ptr(), blob.numel() * 4, s) == -1   # fp32 only
    assert lib.nd_unet_pack_weights_device(_lib.ND_F32, ptrs, n - 1, blob.data_ptr(), blob.numel() * 4, s) == -1
    assert lib.nd_unet_pack_weights_device(_lib.ND_F32, ptrs, n, blob.data_ptr(), 16, s) == -2
    assert lib.nd_unet_pack_weights_device(_lib.ND_F32, ptrs, n, blob.data_ptr(), blob.numel() * 4, s) == -1   # null tensors
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. useful regions against whole tiles
@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_useful_region_canvas_equals_full_tile_canvas(dev, geom):
    d0 = maxdiff(fused(geom, split_k=False, useful_only=True), fused(geom, split_k=False, useful_only=False))
    d1 = maxdiff(fused(geom, split_k=True, useful_only=True), fused(geom, split_k=True, useful_only=False))
    print(f"{geom}: useful vs full: split-K off {d0:.3e}, on {d1:.3e}")
    assert d0 == 0.0
    assert d1 <= REASSOC_BAR


# ------------------------------------------------------------------------------------------------ 3. fused against generic
@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_fused_canvas_against_generic_path(dev, geom):
    d = maxdiff(fused(geom), generic(geom))
    print(f"{geom}: fused vs generic {d:.3e}")
    assert d <= REASSOC_BAR


# ------------------------------------------------------------------------------------------------ 4. fused against the oracle
@pytest.mark.parametrize("geom", GEOMS[:3], ids=IDS[:3])
def test_fused_canvas_against_oracle(dev, geom):
    from oracle import networks as onet
    from oracle import tiler as otiler
    W, H, cs, ucs, ol, batch = geom
    sd = synth.make_unet_state_dict(seed=0)

    def model_fn(x):
        with torch.no_grad():
            return onet.unet_forward(sd, torch.from_numpy(x)).numpy()

    ref = otiler.denoise_frame(frame(W, H).cpu().numpy(), cs, ucs, ol, model_fn, batch=batch)
    err = float(np.abs(fused(geom).cpu().numpy() - ref).max())
    scale = float(np.abs(ref).max())
    print(f"{geom}: fused vs oracle {err:.3e} (max|ref| {scale:.3e})")
    assert err <= ABS_TOL and err <= REL_TOL * scale


# ------------------------------------------------------------------------------------------------ 5. find_noise
@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2], GEOMS[5]], ids=[IDS[0], IDS[2], IDS[5]])
def test_find_noise(dev, geom):
    a, b = fused(geom, find_noise=True), generic(geom, find_noise=True)
    d = maxdiff(a, b)
    print(f"{geom}: find_noise fused vs generic {d:.3e}")
    assert d <= REASSOC_BAR
    assert maxdiff(a, fused(geom)) > 1e-2       # x - sigmoid(...) is not sigmoid(...)


# ------------------------------------------------------------------------------------------------ 6. tile_range and canvas
@pytest.mark.parametrize("geom", [GEOMS[0], GEOMS[2]], ids=[IDS[0], IDS[2]])
def test_tile_ranges_into_prefilled_canvas(dev, geom):
    W, H, cs, ucs, ol, batch = geom
    net = make_net(dev, split_k=False)
    img = frame(W, H)
    total = pipeline.tile_count(W, H, cs, ucs, ol)
    fill = torch.from_numpy(synth.make_frame(W, H, seed=77)).to(dev) + 0.5
    one = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch, canvas=fill.clone())
    two = fill.clone()
    cut = total // 2 + 1                        # not a multiple of the batch: the launches differ from the full call's
    seen = []
    pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch, tile_range=(0, cut), canvas=two, progress=lambda n, t0, c: seen.append((n, t0, c)))
    pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch, tile_range=(cut, total), canvas=two)
    pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch, tile_range=(total, total), canvas=two)   # empty range: no-op
    torch.cuda.synchronize()
    assert seen == [(n, t0, min(batch, cut - t0)) for n, t0 in enumerate(range(0, cut, batch))]
    assert maxdiff(one, two) == 0.0
    assert maxdiff(one, fill + fused(geom, split_k=False)) <= REASSOC_BAR      # += on top of what was there


# ------------------------------------------------------------------------------------------------ 7. stale workspace
@pytest.mark.parametrize("geom", [GEOMS[4], GEOMS[5]], ids=[IDS[4], IDS[5]])
def test_second_frame_through_a_used_workspace(dev, geom):
    W, H, cs, ucs, ol, batch = geom
    a = torch.from_numpy(synth.make_frame(W, H, seed=101)).to(dev)
    used = make_net(dev)
    pipeline.denoise_frame(used, a, cs, ucs, ol, batch=batch)               # frame A leaves its activations behind
    b = pipeline.denoise_frame(used, frame(W, H), cs, ucs, ol, batch=batch)
    torch.cuda.synchronize()
    assert torch.equal(b, fused(geom))                                     # frame B through a fresh model instance


# ------------------------------------------------------------------------------------------------ 8. FrameEngine
def test_frame_engine_takes_a_unet(dev):
    from nind_denoise_amd.serve import FrameEngine
    W, H, cs, ucs, ol, batch = GEOMS[0]
    net = make_net(dev)
    frames = [synth.make_frame(W, H, seed=200 + i) for i in range(3)]
    eng = FrameEngine(net, W, H, cs, ucs, ol, batch=batch, slots=2, device=dev)
    outs = list(eng.run(frames))
    assert len(outs) == 3
    for f, o in zip(frames, outs):
        want = pipeline.denoise_frame(net, torch.from_numpy(f).to(dev), cs, ucs, ol, batch=batch)
        assert np.array_equal(o, want.cpu().numpy())


# ------------------------------------------------------------------------------------------------ entry-point arguments
def test_denoise_frame_arguments(dev):
    lib = _lib.load()
    W, H, cs, ucs, ol, batch = GEOMS[0]
    net = make_net(dev)
    blob, ws = net.packed_weights(dev), net.workspace(cs, cs, batch, dev)
    img = frame(W, H)
    canvas = torch.zeros_like(img)

    def call(dtype=_lib.ND_F32, flags=0, begin=0, count=1, ws_bytes=ws.numel()):
        return lib.nd_unet_denoise_frame(dtype, flags, blob.data_ptr(), img.data_ptr(), canvas.data_ptr(), W, H, cs, ucs, ol, begin, count,
                                         batch, ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev), _lib.PROGRESS_FN(), None)

    assert call(dtype=_lib.ND_BF16) == -1
    assert call(flags=256) == -1 and b"flag" in lib.nd_last_error()
    assert call(begin=11, count=2) == -1                                    # 12 tiles
    assert call(ws_bytes=ws.numel() - 1) == -2
    known_but_idle = _lib.FLAG_DIRECT_CONV | _lib.FLAG_W1D_REGS | _lib.FLAG_UNFUSED_POOL | _lib.FLAG_TILE_ENCODER
    assert call(flags=known_but_idle, count=12) == 0
    torch.cuda.synchronize()
    assert torch.equal(canvas, fused(GEOMS[0]))                             # ... and they switch nothing
    assert canvas.abs().max().item() > 0
