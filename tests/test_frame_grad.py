"""GPU tests of gradients through a tiled frame (nind_denoise_amd/frame_grad.py): the two adjoint kernels against the index
maps of test_frame_grad_host.py on integer data (every sum exact in fp32, so a wrong index is a wrong integer), determinism,
the forward's identity with pipeline.denoise_frame, whole-frame gradients against float64, the generic path, the refusals.

float64 reference: oracle.networks.utnet_forward on the CPU, with gather and stitch written in torch from the maps (an index
select and an index_add with the stitch weights); loss = MSE of the canvas against a random target.  Bar: the project's
gradient bar (test_utnet_input_grad.py), max|got - ref| / max|ref| <= 1e-3, on img.grad, on its 40-pixel border band (where
the folds act) and on every parameter gradient.  Weights: synth.make_utnet_state_dict(gain=1.8); frames: synth.make_frame
(textured: no pool ties)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth
from test_frame_grad_host import GEOMS, oracle_maps

REL = 1e-3
BAND = 40


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _maps(geom):
    src, dst, w = oracle_maps(geom)
    return torch.from_numpy(src.copy()), torch.from_numpy(dst.copy()), torch.from_numpy(w.copy())


def _ints(shape, seed):
    """Integer-valued float32 data in [-8, 8]."""
    return torch.randint(-8, 9, shape, generator=torch.Generator().manual_seed(seed)).float()


def _gather_adjoint_ref(geom, gtiles, begin, count, gimg):
    """np.add.at over the gather map: gimg [3,H,W] + the tile gradients of tiles [begin, begin + count)."""
    W, H = geom[:2]
    src = oracle_maps(geom)[0][begin:begin + count].reshape(-1)
    out = gimg.clone().numpy().reshape(3, H * W)
    g = gtiles.numpy()
    for c in range(3):
        np.add.at(out[c], src, g[:, c].reshape(-1))
    return torch.from_numpy(out.reshape(3, H, W))


def _stitch_adjoint_ref(geom, gcanvas, begin, count):
    """weight map times the canvas gradient: [count,3,cs,cs]."""
    W, H, cs = geom[:3]
    _, dst, w = _maps(geom)
    dst, w = dst[begin:begin + count], w[begin:begin + count]
    g = gcanvas.reshape(3, H * W)[:, dst.clamp(min=0).reshape(-1)].reshape(3, count, cs, cs)
    return (g * w).permute(1, 0, 2, 3).contiguous()


def _launches(n, step):
    return [(t0, min(step, n - t0)) for t0 in range(0, n, step)]


# ---------------------------------------------------------------------------- 4. the adjoint kernels, exact

@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMS)
def test_tile_gather_grad_is_the_transposed_gather_map(dev, geom):
    from nind_denoise_amd import frame_grad, pipeline
    W, H, cs, ucs, ol = geom
    n = oracle_maps(geom)[0].shape[0]
    gt = _ints((n, 3, cs, cs), 1)
    gtd = gt.to(dev)
    ref = _gather_adjoint_ref(geom, gt, 0, n, torch.zeros(3, H, W))
    assert ref.abs().max().item() < 2 ** 24
    for step in (n, 4):                                        # one launch; launches of 4 (a partial last one on the 6-tile grids)
        gimg = torch.zeros(3, H, W, device=dev)
        for t0, cnt in _launches(n, step):
            frame_grad.tile_gather_grad(gtd[t0:t0 + cnt], gimg, cs, ucs, ol, t0)
        assert torch.equal(gimg.cpu(), ref), (geom, step)
    begin, cnt = 1, n - 2                                      # a middle range into a pre-filled gradient: += keeps what was there
    pre = _ints((3, H, W), 2)
    gimg = pre.to(dev)
    frame_grad.tile_gather_grad(gtd[begin:begin + cnt], gimg, cs, ucs, ol, begin)
    assert torch.equal(gimg.cpu(), _gather_adjoint_ref(geom, gt[begin:begin + cnt], begin, cnt, pre)), geom
    # the adjoint identity <gather x, g> = <x, gather^T g>, exact on integers
    x = _ints((3, H, W), 3)
    tiles = pipeline.gather_tiles(x.to(dev), cs, ucs, ol, 0, n).cpu()
    assert torch.equal(tiles, x.reshape(3, -1)[:, _maps(geom)[0].reshape(-1)].reshape(3, n, cs, cs).permute(1, 0, 2, 3))
    assert (tiles.double() * gt.double()).sum().item() == (x.double() * ref.double()).sum().item()


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMS)
def test_stitch_grad_is_the_transposed_stitch_map(dev, geom):
    from nind_denoise_amd import frame_grad, pipeline
    W, H, cs, ucs, ol = geom
    n = oracle_maps(geom)[0].shape[0]
    gc = _ints((3, H, W), 4)
    gcd = gc.to(dev)
    ref = _stitch_adjoint_ref(geom, gc, 0, n)
    for step in (n, 4):
        out = torch.full((n, 3, cs, cs), float("nan"), device=dev)       # every element must be written
        for t0, cnt in _launches(n, step):
            frame_grad.stitch_grad(gcd, cs, ucs, ol, t0, cnt, out=out[t0:t0 + cnt])
        assert torch.equal(out.cpu(), ref), (geom, step)
    begin, cnt = 1, n - 2
    assert torch.equal(frame_grad.stitch_grad(gcd, cs, ucs, ol, begin, cnt).cpu(), ref[begin:begin + cnt]), geom
    # <stitch t, g> = <t, stitch^T g>: the weights are powers of two, so both sides are exact
    t = _ints((n, 3, cs, cs), 5)
    canvas = pipeline.stitch_tiles(torch.zeros(3, H, W, device=dev), t.to(dev), cs, ucs, ol, 0).cpu()
    assert (canvas.double() * gc.double()).sum().item() == (t.double() * ref.double()).sum().item()


# ---------------------------------------------------------------------------- 5. determinism

@pytest.mark.gpu
def test_adjoint_kernels_are_deterministic(dev):
    from nind_denoise_amd import frame_grad
    geom = GEOMS[4]
    W, H, cs, ucs, ol = geom
    n = oracle_maps(geom)[0].shape[0]
    g = torch.Generator().manual_seed(6)
    gt = (torch.rand(n, 3, cs, cs, generator=g) - 0.5).to(dev)
    gc = (torch.rand(3, H, W, generator=g) - 0.5).to(dev)
    pre = (torch.rand(3, H, W, generator=g) - 0.5).to(dev)
    runs = []
    for _ in range(2):
        gimg = pre.clone()
        for t0, cnt in _launches(n, 7):
            frame_grad.tile_gather_grad(gt[t0:t0 + cnt], gimg, cs, ucs, ol, t0)
        runs.append((gimg, frame_grad.stitch_grad(gc, cs, ucs, ol, 0, n)))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert not torch.equal(runs[0][0], pre)


# ---------------------------------------------------------------------------- 6. forward identity

def _net(sd, funit, activation="PReLU", **kw):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=funit, activation=activation, **kw)
    net.load_state_dict(sd)
    return net


@pytest.mark.gpu
def test_forward_is_the_fused_inference_loop(dev):
    from nind_denoise_amd import frame_grad, pipeline
    W, H, cs, ucs, ol = GEOMS[1]
    sd = synth.make_utnet_state_dict(funit=8, seed=31, gain=1.8)
    net = _net(sd, 8).to(dev).eval()
    img = torch.from_numpy(synth.make_frame(W, H, seed=2)).to(dev)
    want = pipeline.denoise_frame(net, img, cs, ucs, ol, batch=4)
    got = frame_grad.denoise_frame(net, img.clone().requires_grad_(), cs, ucs, ol, batch=4)
    assert got.grad_fn is not None and torch.equal(got.detach(), want)
    net.requires_grad_(False)
    assert frame_grad.denoise_frame(net, img, cs, ucs, ol, batch=4).grad_fn is None       # nothing requires a gradient
    with torch.no_grad():
        assert frame_grad.denoise_frame(net, img.clone().requires_grad_(), cs, ucs, ol, batch=4).grad_fn is None
    part = frame_grad.denoise_frame(net, img.clone().requires_grad_(), cs, ucs, ol, batch=4, tile_range=(1, 5))
    assert torch.equal(part.detach(), pipeline.denoise_frame(net, img, cs, ucs, ol, batch=4, tile_range=(1, 5)))


# ---------------------------------------------------------------------------- 7. whole-frame gradients against float64

@functools.lru_cache(maxsize=None)
def _case(gi, funit, activation):
    """(sd, frame, target, loss, d loss / d frame, {name: d loss / d parameter}) in float64 on the CPU, computed once."""
    from oracle import networks as onet
    geom = GEOMS[gi]
    W, H, cs, ucs, ol = geom
    src, dst, w = _maps(geom)
    n = src.shape[0]
    sd = synth.make_utnet_state_dict(funit=funit, seed=31, activation=activation, gain=1.8)
    frame = torch.from_numpy(synth.make_frame(W, H, seed=2))
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(7))
    params = {k: v.clone().double().requires_grad_() for k, v in sd.items()}
    x = frame.double().requires_grad_()
    tiles = x.reshape(3, H * W)[:, src.reshape(-1)].reshape(3, n, cs, cs).permute(1, 0, 2, 3)
    y = torch.cat([onet.utnet_forward(params, tiles[t0:t0 + 8], activation=activation) for t0 in range(0, n, 8)])
    keep = (w != 0).reshape(-1)
    contrib = (y * w.double().unsqueeze(1)).permute(1, 0, 2, 3).reshape(3, -1)[:, keep]
    canvas = torch.zeros(3, H * W, dtype=torch.float64).index_add(1, dst.reshape(-1)[keep], contrib).reshape(3, H, W)
    loss = F.mse_loss(canvas, target.double())
    loss.backward()
    return sd, frame, target, loss.item(), x.grad, {k: p.grad for k, p in params.items()}


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def _band(t):
    """The 40-pixel border band of [3, H, W] as one flat tensor."""
    return torch.cat([t[..., :BAND, :].reshape(-1), t[..., -BAND:, :].reshape(-1),
                      t[..., BAND:-BAND, :BAND].reshape(-1), t[..., BAND:-BAND, -BAND:].reshape(-1)])


def _run(dev, gi, funit, activation, batch, want_img=True, want_params=True, train=True):
    from nind_denoise_amd import frame_grad
    W, H, cs, ucs, ol = GEOMS[gi]
    sd, frame, target, loss_ref, gx_ref, gp_ref = _case(gi, funit, activation)
    net = _net(sd, funit, activation).to(dev)
    net = net.train() if train else net.eval()
    net.requires_grad_(want_params)
    img = frame.to(dev).requires_grad_(want_img)
    canvas = frame_grad.denoise_frame(net, img, cs, ucs, ol, batch=batch)
    assert canvas.grad_fn is not None
    loss = F.mse_loss(canvas, target.to(dev))
    loss.backward()
    what = (GEOMS[gi], funit, activation, batch, want_img, want_params, train)
    assert abs(loss.item() - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref)), (what, loss.item(), loss_ref)
    figures = {}
    if want_img:
        figures["img"] = _rel(img.grad, gx_ref)
        figures["band"] = _rel(_band(img.grad.cpu()), _band(gx_ref))
    else:
        assert img.grad is None
    worst = ("", 0.0)
    for name, p in net.named_parameters():
        if want_params:
            e = _rel(p.grad, gp_ref[name])
            worst = max(worst, (name, e), key=lambda t: t[1])
        else:
            assert p.grad is None, name
    if want_params:
        figures["params"] = worst
    print(f"frame grad {what}: {figures}")
    if want_img:
        assert gx_ref.abs().max().item() > 0 and _band(gx_ref).abs().max().item() > 0
        assert figures["img"] <= REL, (what, "img.grad", figures["img"])
        assert figures["band"] <= REL, (what, "img.grad border band", figures["band"])
    if want_params:
        assert worst[1] <= REL, (what, worst)


@pytest.mark.gpu
@pytest.mark.parametrize("gi, funit, batch", [(0, 8, 16), (1, 8, 4), (4, 16, 7)])
def test_frame_gradients_match_float64(dev, gi, funit, batch):
    _run(dev, gi, funit, "PReLU", batch)


@pytest.mark.gpu
@pytest.mark.parametrize("activation", ["ELU", "Hardswish"])
def test_frame_gradients_other_activations(dev, activation):
    _run(dev, 0, 8, activation, 3)


@pytest.mark.gpu
def test_frozen_parameters_give_the_frame_gradient_only(dev):
    _run(dev, 1, 8, "PReLU", 4, want_params=False)


@pytest.mark.gpu
def test_frame_without_gradient_gives_parameter_gradients_only(dev):
    _run(dev, 1, 8, "PReLU", 4, want_img=False)


@pytest.mark.gpu
def test_eval_mode_gives_the_same_gradients(dev):
    _run(dev, 1, 8, "PReLU", 4, train=False)


@pytest.mark.gpu
def test_flags_are_honoured_in_the_recompute(dev):
    """winograd = False / split_k = False reach the recompute: the gradients stay within the bar and the flags word differs."""
    from nind_denoise_amd import frame_grad
    W, H, cs, ucs, ol = GEOMS[0]
    sd, frame, target, _, gx_ref, gp_ref = _case(0, 8, "PReLU")
    net = _net(sd, 8).to(dev).train()
    net.winograd, net.split_k = False, False
    assert net.flags & _lib.FLAG_DIRECT_CONV and net.flags & _lib.FLAG_NO_SPLITK
    img = frame.to(dev).requires_grad_()
    F.mse_loss(frame_grad.denoise_frame(net, img, cs, ucs, ol, batch=4), target.to(dev)).backward()
    assert _rel(img.grad, gx_ref) <= REL
    for name, p in net.named_parameters():
        assert _rel(p.grad, gp_ref[name]) <= REL, name


# ---------------------------------------------------------------------------- 8. the generic path

@pytest.mark.gpu
def test_generic_model_through_gather_and_stitch(dev):
    """t -> 0.5 t^2 + t per tile pixel; loss = <canvas, r>.  Closed form: d loss / d frame = G^T((G x + 1) * S^T r) with G the
    gather map and S the weighted stitch map, in float64."""
    from nind_denoise_amd import frame_grad
    geom = GEOMS[3]
    W, H, cs, ucs, ol = geom
    src, dst, w = _maps(geom)
    n = src.shape[0]
    frame = torch.from_numpy(synth.make_frame(W, H, seed=4))
    r = torch.rand(3, H, W, generator=torch.Generator().manual_seed(8)) - 0.5
    tiles = frame.double().reshape(3, -1)[:, src.reshape(-1)]                                      # G x: [3, n cs cs]
    str_r = r.double().reshape(3, -1)[:, dst.clamp(min=0).reshape(-1)] * w.double().reshape(-1)     # S^T r
    ref = torch.zeros(3, H * W, dtype=torch.float64).index_add(1, src.reshape(-1), (tiles + 1) * str_r).reshape(3, H, W)
    canvas_ref = torch.zeros(3, H * W, dtype=torch.float64).index_add(
        1, dst.clamp(min=0).reshape(-1), (0.5 * tiles * tiles + tiles) * w.double().reshape(-1)).reshape(3, H, W)

    def model(t):
        return 0.5 * t * t + t

    img = frame.to(dev).requires_grad_()
    canvas = frame_grad.denoise_frame(model, img, cs, ucs, ol, batch=5)
    assert _rel(canvas, canvas_ref) <= 1e-6
    (canvas * r.to(dev)).sum().backward()
    err = _rel(img.grad, ref)
    print(f"generic path: img.grad {err:.2e}")
    assert err <= 1e-6, err
    # the same by hand, launch by launch, and stitch_tiles leaves the canvas it is given alone
    img2 = frame.to(dev).requires_grad_()
    c0 = torch.zeros(3, H, W, device=dev)
    c1 = frame_grad.stitch_tiles(c0, model(frame_grad.gather_tiles(img2, cs, ucs, ol, 0, 9)), cs, ucs, ol, 0)
    c2 = frame_grad.stitch_tiles(c1, model(frame_grad.gather_tiles(img2, cs, ucs, ol, 9, n - 9)), cs, ucs, ol, 9)
    assert not c0.any() and c2.grad_fn is not None
    (c2 * r.to(dev)).sum().backward()
    assert _rel(img2.grad, ref) <= 1e-6


# ---------------------------------------------------------------------------- 9. refusals

@pytest.mark.gpu
def test_refusals(dev):
    from nind_denoise_amd import frame_grad
    W, H, cs, ucs, ol = GEOMS[0]
    sd = synth.make_utnet_state_dict(funit=16, seed=31, gain=1.8)
    frame = torch.from_numpy(synth.make_frame(W, H, seed=2))
    with pytest.raises(NotImplementedError):
        frame_grad.denoise_frame(_net(sd, 16, compute_dtype="bf16").to(dev), frame.to(dev).requires_grad_(), cs, ucs, ol)
    net = _net(sd, 16).to(dev).train()
    with pytest.raises(RuntimeError):
        frame_grad.denoise_frame(net, frame.clone().requires_grad_(), cs, ucs, ol)
    with pytest.raises(RuntimeError):
        frame_grad.gather_tiles(frame, cs, ucs, ol, 0, 1)
    with pytest.raises(ValueError):
        frame_grad.denoise_frame(net, frame.to(dev).requires_grad_(), cs, ucs, ol, tile_range=(0, 5))
    # a crop graph that predates a frame backward of the same module is stale: the recompute used the module's workspace
    x = torch.rand(2, 3, cs, cs, generator=torch.Generator().manual_seed(9)).to(dev).requires_grad_()
    y = net(x)
    img = frame.to(dev).requires_grad_()
    canvas = frame_grad.denoise_frame(net, img, cs, ucs, ol, batch=2)
    canvas.sum().backward()
    assert img.grad is not None and img.grad.abs().max().item() > 0
    with pytest.raises(RuntimeError, match="another forward of this module"):
        y.sum().backward()
