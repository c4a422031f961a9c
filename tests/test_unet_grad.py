"""UNet under autograd in eval mode (nd_unet_grad_forward / nd_unet_grad_backward, frame_grad.denoise_frame) against float64 autograd
of the same eval-mode graph: d loss / d x and every parameter gradient on crops and on tiled frames.

Shapes, frames and weights are those of test_unet_float64.py (loaded with importlib): SMALL_SHAPES cover the 1x1 bottom, every F.pad
fix-up and the batch stride through odd buffers; FRAME_CASES have an odd and an even tile side, both with a partial last launch; the
weights are visible_unet_sd (gain 3), so that every level carries gradients of the order of the top ones.  Loss: MSE against a random
target.

Conditioning, so that fp32 can be held near its own rounding (`conditioned`): in forward order, the bias of every BatchNorm channel is
shifted by the least amount that leaves no float64 BatchNorm output of the batch within KINK_MARGIN of 0, then rounded to fp32 (both
sides start from the same weights); the margin is asserted with the rounded weights, and so is POOL_MARGIN: no 2x2 pool window whose two
largest positive float64 values are closer than that.  Without the shift a single ReLU that flips between the two forward passes moves a
weight gradient by 1e-3 ... 1e-1; with it torch's own fp32 autograd on the CPU is within a few 1e-6 of float64 on every gradient
(test_unet_grad_host.py prints and asserts those figures, and gates the bars below against the errors a backward pass can make)."""
import functools
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib


def _load(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    spec = importlib.util.spec_from_file_location("_unet_grad_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


f64 = _load("test_unet_float64.py")
SMALL_SHAPES, FRAME_CASES, BAR_UNET_FWD = f64.SMALL_SHAPES, f64.FRAME_CASES, f64.BAR_UNET_FWD

SEED = 3                 # weights and input seed of the crop cases: four of the five shapes meet both margins with it
# (1, 16, 16) with seed 3 has one pool window of down1 whose two largest values are 2.1e-7 apart and no BatchNorm output near 0, so
# nothing to shift: that shape runs with the other seed of test_unet_float64.py's forward cases, which meets both margins
SHAPE_SEED = {(1, 16, 16): 0}
KINK_MARGIN = 3e-5       # no float64 BatchNorm output of the batch closer than this to 0
POOL_MARGIN = 3e-6       # no pool window whose two largest positive float64 values are closer than this
SLACK = 1.001           # a shifted channel's nearest output lands at SLACK x KINK_MARGIN: the margin survives the bias' rounding to fp32

# Bars: max |err| / max |ref| per tensor against float64, per class of tensor.  About 3x the worst value measured on the MI355X over
# every case below (re-association between launch shapes and split-K plans); in brackets torch fp32 autograd on the CPU against the same
# float64 reference, worst over the crop cases (test_unet_grad_host.py::test_cpu_fp32_autograd_is_near_float64 prints them).  y is held
# to BAR_UNET_FWD (max |err|, a sigmoid).  test_unet_grad_host.py::test_bars_see_backward_errors requires every bar to be 10x below
# what a 1 % error in a pool's or a transpose's gradient, or a fix-up line's gradient that is not dropped, does to the class.
BARS = {
    "dx": 2.5e-6,      # measured 7.1e-7 (3x33x47 planted)                      [cpu fp32 7.5e-7]
    "conv_w": 3e-6,    # measured 1.01e-6 (down4.mpconv.1.conv.0, find_noise)   [cpu fp32 2.6e-6]
    "conv_b": 2.5e-6,  # measured 8.4e-7 (down3.mpconv.1.conv.0, 1x16x16)       [cpu fp32 1.7e-6]
    "bn_w": 3.5e-6,    # measured 1.18e-6 (up1.conv.conv.4, planted)            [cpu fp32 1.0e-6]
    "bn_b": 2.5e-6,    # measured 7.2e-7 (down4.mpconv.1.conv.4, 1x16x16)       [cpu fp32 1.0e-6]
    "up_w": 2.5e-6,    # measured 7.3e-7 (up1.up, 1x64x16)                      [cpu fp32 1.0e-6]
    "up_b": 2e-6,      # measured 6.7e-7 (up2.up, planted)                      [cpu fp32 2.0e-6]
}
# (with split_k = False the deep layers' 4608 ... 9216-term sums run as one fp32 chain: up to 2.9e-6 on the same cases, not asserted)
#
# Frames.  A frame's tiles hold 3.5 million pool windows, so some pair of maxima is closer than POOL_MARGIN whatever the BatchNorm
# shifts do, and fp32 may order such a pair the other way.  That moves one pooled pixel's gradient to its neighbour: in float64,
# flipping the closest window of down2 alone moves frame.grad by 1e-3 ... 2e-3 of its maximum within the window's receptive field, the
# encoder tensors above it by 2e-6 ... 1.6e-5, and the transposes by 1e-12.
#   cs 90 (FRAME_CASES[0]): the MI355X orders every window as float64 does -- every class <= 5.9e-7, frame.grad 5.7e-7 over the whole
#     frame.  The crop BARS hold, frame.grad unmasked.
#   cs 96 (FRAME_CASES[1]): 13 + 7 windows of down1 / down2 lie under POOL_MARGIN, two of them 1.4e-7 apart, and the MI355X shows the
#     signature above (conv_w 2.3e-5 inc.conv.conv.0, conv_b 1.5e-5 inc.conv.conv.3, bn_w 1.0e-5 inc.conv.conv.4, bn_b 1.4e-5
#     down1.mpconv.1.conv.1, up_w 4.7e-7; frame.grad 7.6e-3 at single pixels).  For this case alone: frame.grad is held to BARS["dx"]
#     outside the exact reach of the windows closer than POOL_MARGIN in the float64 forward (frame_case: near_tie_mask, at most
#     NEAR_TIE_SHARE of the frame) and to FRAME_DX_WHOLE over the whole frame, the four encoder-side classes to 3x what was measured,
#     the transposes to their crop bars.  (bn_b is then 41x its CPU fp32 figure: the cause is the flipped maximum, not rounding.)
FRAME_BARS = {0: BARS, 1: dict(BARS, conv_w=7e-5, conv_b=4.5e-5, bn_w=3e-5, bn_b=4.5e-5)}
FRAME_MASKED = {0: False, 1: True}
FRAME_DX_WHOLE = 2.5e-2     # cs 96, whole frame: measured 7.6e-3
NEAR_TIE_SHARE = 0.04       # cs 96: 3.0 % of the frame lies within reach of a window closer than POOL_MARGIN


def klass(name):
    """Class of a parameter by its state-dict name."""
    kind = "w" if name.endswith(".weight") else "b"
    if ".up." in name:
        return "up_" + kind
    if name.startswith("outc.") or name.rsplit(".", 2)[1] in ("0", "3"):
        return "conv_" + kind
    return "bn_" + kind


def is_parameter(name):
    return name.endswith((".weight", ".bias"))


# ---------------------------------------------------------------------------- the eval-mode graph in float64, with taps
class _GScale(torch.autograd.Function):
    """Identity whose gradient is multiplied by knobs.get(key, 1): the modelled 1 % errors of the gate."""

    @staticmethod
    def forward(ctx, t, knobs, key):
        ctx.knobs, ctx.key = knobs, key
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.knobs.get(ctx.key, 1.0), None, None


class _FixPad(torch.autograd.Function):
    """F.pad(up, (0, dx, 0, dy)): the gradient on the padded line(s) is dropped -- or, with knobs[key] set, added to the neighbouring
    line of `up` (the modelled error: a fix-up line that the 2x2 stride-2 data gradient reads)."""

    @staticmethod
    def forward(ctx, up, dy, dx, knobs, key):
        ctx.args = (up.size(2), up.size(3), dy, dx, knobs, key)
        return F.pad(up, (0, dx, 0, dy))

    @staticmethod
    def backward(ctx, g):
        h, w, dy, dx, knobs, key = ctx.args
        gu = g[:, :, :h, :w].clone()
        if knobs.get(key):
            if dy:
                gu[:, :, h - 1, :] += g[:, :, h, :w]
            if dx:
                gu[:, :, :, w - 1] += g[:, :, :h, w]
        return gu, None, None, None, None


def _double_conv(sd, p, x, bn_hook):
    for k in (0, 3):
        x = F.conv2d(x, sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"], padding=1)
        x = F.batch_norm(x, sd[f"{p}.{k + 1}.running_mean"], sd[f"{p}.{k + 1}.running_var"], sd[f"{p}.{k + 1}.weight"],
                         sd[f"{p}.{k + 1}.bias"], training=False, eps=1e-5)
        if bn_hook is not None:
            x = bn_hook(f"{p}.{k + 1}", x)
        x = F.relu(x)
    return x


def forward_graph(sd, x, find_noise=False, knobs=None, bn_hook=None, pool_hook=None):
    """UNet.forward in eval mode (test_unet_float64._encode64 / _decode64 restated with taps).  knobs: a dict read at BACKWARD time --
    d<n>: factor on the gradient entering the pool of down<n>; u<n>: factor on the gradient leaving up<n>'s transpose; fix<n>: the
    fix-up line's gradient of up<n> is added to its neighbour.  bn_hook(name, t) -> t sees every BatchNorm output, pool_hook(n, t)
    every pooled tensor's source."""
    knobs = {} if knobs is None else knobs
    skips = [_double_conv(sd, "inc.conv.conv", x, bn_hook)]
    for n in (1, 2, 3, 4):
        if pool_hook is not None:
            pool_hook(n, skips[-1])
        p = _GScale.apply(F.max_pool2d(skips[-1], 2), knobs, f"d{n}")
        skips.append(_double_conv(sd, f"down{n}.mpconv.1.conv", p, bn_hook))
    t = skips[4]
    for n, skip in zip((1, 2, 3, 4), (skips[3], skips[2], skips[1], skips[0])):
        up = F.conv_transpose2d(_GScale.apply(t, knobs, f"u{n}"), sd[f"up{n}.up.weight"], sd[f"up{n}.up.bias"], stride=2)
        dy, dx = skip.size(2) - up.size(2), skip.size(3) - up.size(3)
        assert dy in (0, 1) and dx in (0, 1)
        up = _FixPad.apply(up, dy, dx, knobs, f"fix{n}")
        t = _double_conv(sd, f"up{n}.conv.conv", torch.cat([skip, up], dim=1), bn_hook)
    s = torch.sigmoid(F.conv2d(t, sd["outc.conv.weight"], sd["outc.conv.bias"]))
    return x - s if find_noise else s


def fixups(h, w):
    """The up<n> (1 ... 4) whose result is one line short of its skip at input size h x w."""
    hs, ws = f64._level_sizes(h), f64._level_sizes(w)
    return [n for n in (1, 2, 3, 4) if hs[4 - n] != 2 * hs[5 - n] or ws[4 - n] != 2 * ws[5 - n]]


# ---------------------------------------------------------------------------- conditioning
def _least_shift(v, delta):
    """The s of least |s| with |v + s| >= SLACK delta for every value of v (1-D, float64), 0 if |v| >= delta already: the new origin -s
    is the point nearest 0 that lies SLACK delta inside a gap between neighbouring sorted values (or beyond an end)."""
    if v.abs().min().item() >= delta:
        return 0.0
    w = torch.sort(v).values
    lo = torch.cat([w.new_tensor([-float("inf")]), w]) + SLACK * delta          # allowed origins of the gap below / between / above
    hi = torch.cat([w, w.new_tensor([float("inf")])]) - SLACK * delta
    ok = hi >= lo
    cands = torch.minimum(torch.maximum(torch.zeros_like(lo), lo), hi)[ok]
    return -cands[cands.abs().argmin()].item()


def conditioned(sd, x, pool_margin=POOL_MARGIN):
    """sd (fp32, test_unet_float64._sd) with the BatchNorm biases shifted as the module docstring says, for the batch x (fp32).  Returns
    (sd, report): report = {"shifted": channels shifted, "max_shift": largest |shift|, "kink": least |BatchNorm output|, "pool": least gap
    between the two largest positive values of a pool window} with the returned fp32 weights, both margins asserted (pool_margin None:
    the kink margin only)."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd64 = {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}
    report = {"shifted": 0, "max_shift": 0.0}

    def shift(name, t):
        near = (t.abs().amin(dim=(0, 2, 3)) < KINK_MARGIN).nonzero().flatten().tolist()
        for c in near:
            s = _least_shift(t[:, c].reshape(-1), KINK_MARGIN)
            b = sd64[name + ".bias"][c].item()
            nb = torch.tensor(b + s, dtype=torch.float64).float()
            sd[name + ".bias"][c] = nb
            sd64[name + ".bias"][c] = nb.double()
            t[:, c] += nb.double().item() - b
            report["shifted"] += 1
            report["max_shift"] = max(report["max_shift"], abs(s))
        return t

    with torch.no_grad():
        forward_graph(sd64, x.double(), bn_hook=shift)
        report.update(margins({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double()))
    assert report["kink"] >= KINK_MARGIN, report
    assert pool_margin is None or report["pool"] >= pool_margin, report
    return sd, report


def margins(sd64, x64):
    """{"kink": least |BatchNorm output|, "pool": least gap between the two largest positive values of a 2x2 pool window} of a forward."""
    out = {"kink": float("inf"), "pool": float("inf")}

    def bn(name, t):
        out["kink"] = min(out["kink"], t.abs().min().item())
        return t

    def pool(n, t):
        h, w = t.size(2) // 2 * 2, t.size(3) // 2 * 2
        win = F.unfold(t[:, :, :h, :w].reshape(-1, 1, h, w), 2, stride=2)          # [B*C, 4, windows]
        top = win.topk(2, dim=1).values
        # (two values that are exactly equal come from a constant channel -- a zero BatchNorm weight -- in fp32 as in float64, and
        # both sides then take the first in row-major order)
        both = (top[:, 1] > 0) & (top[:, 0] != top[:, 1])
        if both.any():
            out["pool"] = min(out["pool"], (top[:, 0] - top[:, 1])[both].min().item())

    with torch.no_grad():
        forward_graph(sd64, x64, bn_hook=bn, pool_hook=pool)
    return out


def target_for(shape, seed):
    b, h, w = shape
    return torch.rand((b, 3, h, w), generator=torch.Generator().manual_seed(77 + 13 * seed + h + w))


def reference(sd, x, target, find_noise=False, knobs=None, dtype=torch.float64):
    """(y, loss, dx, {name: gradient}) of MSE(forward(x), target) by torch autograd on the CPU in `dtype`; knobs: forward_graph's."""
    p = {k: (v.to(dtype).requires_grad_(is_parameter(k)) if v.is_floating_point() else v) for k, v in sd.items()}
    xr = x.to(dtype).requires_grad_()
    y = forward_graph(p, xr, find_noise=find_noise, knobs=knobs)
    loss = F.mse_loss(y, target.to(dtype))
    names = [k for k in p if is_parameter(k)]
    g = torch.autograd.grad(loss, [xr] + [p[k] for k in names])
    return y.detach(), loss.item(), g[0], dict(zip(names, g[1:]))


@functools.lru_cache(maxsize=None)
def crop_case(shape, planted=False, find_noise=False):
    """(conditioned fp32 weights, input, target, float64 y, float64 dx, {name: float64 gradient}), computed once and shared (never modified)."""
    seed = SHAPE_SEED.get(shape, SEED)
    x = f64._input(seed, shape)
    sd, _ = conditioned(f64._sd(seed, planted), x)
    target = target_for(shape, seed)
    y, _, dx, grads = reference(sd, x, target, find_noise)
    return sd, x, target, y, dx, grads


def rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-300)


def class_figures(dx, grads, ref_dx, ref_grads, want=None):
    """{class: (worst max|err| / max|ref| over its tensors, the tensor)} of dx and the parameter gradients (want: the names to compare)."""
    fig = {"dx": (rel(dx, ref_dx), "dx")} if dx is not None else {}
    for k, r in ref_grads.items():
        if want is not None and k not in want:
            continue
        e = rel(grads[k], r)
        if e >= fig.get(klass(k), (-1.0, ""))[0]:
            fig[klass(k)] = (e, k)
    return fig


def _show(what, fig):
    print(f"UNet grad {what}: " + ", ".join(f"{c} {v:.2e} ({k})" for c, (v, k) in sorted(fig.items())))


def _assert_bars(what, fig, bars=BARS):
    _show(what, fig)
    for c, (v, k) in fig.items():
        assert v <= bars[c], (what, c, k, v, bars[c])


# ---------------------------------------------------------------------------- GPU: crops
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _net(dev, sd, find_noise=False):
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    net = UNet(find_noise=find_noise)
    net.load_state_dict(sd)
    return net.eval().to(dev)


def _run(net, x, target, dev, want_dx=True):
    """One forward / backward through the module: (y, dx, {name: grad or None})."""
    net.zero_grad(set_to_none=True)
    xd = x.to(dev).requires_grad_(want_dx)
    y = net(xd)
    F.mse_loss(y, target.to(dev)).backward()
    return y.detach(), xd.grad, {k: p.grad for k, p in net.named_parameters()}


def _sid(s):
    return "x".join(str(v) for v in s)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=_sid)
def test_dx_and_every_parameter_gradient(dev, shape):
    sd, x, target, y64, dx64, g64 = crop_case(shape)
    y, dx, grads = _run(_net(dev, sd), x, target, dev)
    ey = (y.double().cpu() - y64).abs().max().item()
    print(f"UNet grad {shape}: y vs float64 {ey:.2e}")
    assert ey <= BAR_UNET_FWD, ey
    assert set(grads) == set(g64) and all(g is not None for g in grads.values())
    _assert_bars(shape, class_figures(dx, grads, dx64, g64))


@pytest.mark.gpu
def test_frozen_parameters_dx_only(dev):
    shape = (2, 17, 31)
    sd, x, target, y64, dx64, g64 = crop_case(shape)
    net = _net(dev, sd).requires_grad_(False)
    st = net._grad_state(dev)
    st.grads.fill_(float("nan"))
    y, dx, grads = _run(net, x, target, dev)
    assert all(g is None for g in grads.values())
    assert torch.isnan(st.grads).all()                     # null `grads`: no parameter-gradient kernel wrote anything
    _assert_bars(f"{shape} frozen", class_figures(dx, {}, dx64, {}))
    full = _run(_net(dev, sd), x, target, dev)
    assert torch.equal(dx, full[1]) and torch.equal(y, full[0])


@pytest.mark.gpu
def test_half_the_parameters_frozen(dev):
    shape = (3, 33, 47)
    sd, x, target, y64, dx64, g64 = crop_case(shape)
    net = _net(dev, sd)
    frozen = {k for i, (k, p) in enumerate(net.named_parameters()) if i % 2}
    for k, p in net.named_parameters():
        p.requires_grad_(k not in frozen)
    y, dx, grads = _run(net, x, target, dev)
    assert all((grads[k] is None) == (k in frozen) for k in grads) and 0 < len(frozen) < len(grads)
    _assert_bars(f"{shape} half frozen", class_figures(dx, grads, dx64, g64, want=set(grads) - frozen))
    assert net(x.to(dev)).grad_fn is None                            # an input without a gradient: the inference path, no graph


@pytest.mark.gpu
def test_find_noise(dev):
    shape = (2, 17, 31)
    sd, x, target, y64, dx64, g64 = crop_case(shape, find_noise=True)
    assert not torch.equal(dx64, crop_case(shape)[4])
    y, dx, grads = _run(_net(dev, sd, find_noise=True), x, target, dev)
    assert (y.double().cpu() - y64).abs().max().item() <= BAR_UNET_FWD
    _assert_bars(f"{shape} find_noise", class_figures(dx, grads, dx64, g64))


@pytest.mark.gpu
def test_planted_batchnorm(dev):
    shape = (3, 33, 47)
    sd, x, target, y64, dx64, g64 = crop_case(shape, planted=True)
    gamma = sd["down2.mpconv.1.conv.1.weight"]
    assert (gamma == 0).any() and (gamma < 0).any()
    y, dx, grads = _run(_net(dev, sd), x, target, dev)
    assert (y.double().cpu() - y64).abs().max().item() <= BAR_UNET_FWD
    _assert_bars(f"{shape} planted", class_figures(dx, grads, dx64, g64))
    # a zero weight: its conv's gradients vanish; its own does not (where its constant output, the BatchNorm bias, passes the ReLU)
    dead = (gamma == 0).nonzero().flatten().tolist()
    live = g64["down2.mpconv.1.conv.1.weight"][dead] != 0
    assert not grads["down2.mpconv.1.conv.0.weight"][dead].any() and not grads["down2.mpconv.1.conv.0.bias"][dead].any()
    assert live.any() and torch.equal(grads["down2.mpconv.1.conv.1.weight"][dead].cpu() != 0, live)


@pytest.mark.gpu
def test_two_backward_passes_are_equal(dev):
    shape = (2, 100, 92)
    sd, x, target = crop_case(shape)[:3]
    net = _net(dev, sd)
    a = _run(net, x, target, dev)
    b = _run(net, x, target, dev)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.equal(a[2][k], b[2][k]) for k in a[2])


@pytest.mark.gpu
def test_generation_guard_and_train_mode(dev):
    shape = (1, 16, 16)
    sd, x, target = crop_case(shape)[:3]
    net = _net(dev, sd)
    y1 = net(x.to(dev).requires_grad_())
    y2 = net(x.to(dev).requires_grad_())
    with pytest.raises(RuntimeError, match="another forward of this module"):
        y1.sum().backward()
    y2.sum().backward()
    with pytest.raises(RuntimeError, match="eval mode"):
        net.train()(x.to(dev).requires_grad_())
    with pytest.raises(RuntimeError, match="eval mode"):
        net.train()(x.to(dev))


@pytest.mark.gpu
def test_input_without_gradient_takes_the_inference_path(dev):
    lib = _lib.load()
    shape = (2, 17, 31)
    b, h, w = shape
    sd, x, _ = crop_case(shape)[:3]
    net = _net(dev, sd)
    xd = x.to(dev)
    want = torch.empty_like(xd)                                        # nd_unet_forward itself, as the module called it before
    blob, ws = net.packed_weights(dev), net.workspace(h, w, b, dev)
    _lib.check(lib.nd_unet_forward(_lib.ND_F32, blob.data_ptr(), xd.data_ptr(), want.data_ptr(), b, h, w, ws.data_ptr(), ws.numel(),
                                   _lib.stream_ptr(dev)), "nd_unet_forward")
    y = net(xd)                                                        # parameters require gradients, the input does not
    assert y.grad_fn is None and torch.equal(y, want)
    with torch.no_grad():
        y = net(xd.clone().requires_grad_())
    assert y.grad_fn is None and torch.equal(y, want)
    assert getattr(net, "_gstate", None) is None                       # neither call touched the autograd state
    yg = net(xd.clone().requires_grad_())
    assert yg.grad_fn is not None and torch.equal(yg.detach(), want)   # the same launches on the same blob


@pytest.mark.gpu
def test_workspace_recreated_for_another_odd_shape(dev):
    a, b = (2, 17, 31), (3, 33, 47)
    sd = crop_case(a)[0]                                               # one set of weights through both shapes
    net = _net(dev, sd)
    first = _run(net, crop_case(a)[1], crop_case(a)[2], dev)
    key = net._gstate.ws_key
    other = _run(net, crop_case(b)[1], crop_case(b)[2], dev)
    assert net._gstate.ws_key != key and torch.isfinite(other[1]).all()
    again = _run(net, crop_case(a)[1], crop_case(a)[2], dev)
    assert net._gstate.ws_key == key
    assert torch.equal(first[1], again[1]) and all(torch.equal(first[2][k], again[2][k]) for k in first[2])
    _assert_bars(f"{a} after {b}", class_figures(again[1], again[2], crop_case(a)[4], crop_case(a)[5]))


@pytest.mark.gpu
def test_outputs_prefilled_with_nan_come_back_finite(dev):
    lib = _lib.load()
    shape = (2, 17, 31)
    b, h, w = shape
    sd, x, target, y64, dx64, g64 = crop_case(shape)
    net = _net(dev, sd)
    y, dx, grads = _run(net, x, target, dev)
    st = net._gstate
    xd = x.to(dev)
    nan = float("nan")
    y2, dx2, flat = torch.full_like(xd, nan), torch.full_like(xd, nan), torch.full_like(st.grads, nan)
    gy = (2.0 / y.numel()) * (y - target.to(dev))
    args = (b, h, w, st.ws.data_ptr(), st.ws.numel(), _lib.stream_ptr(dev))
    _lib.check(lib.nd_unet_grad_forward(net.grad_flags, st.flat.data_ptr(), st.blobs.data_ptr(), xd.data_ptr(), y2.data_ptr(), *args))
    _lib.check(lib.nd_unet_grad_backward(net.grad_flags, st.flat.data_ptr(), flat.data_ptr(), st.blobs.data_ptr(), gy.data_ptr(),
                                         dx2.data_ptr(), *args))
    torch.cuda.synchronize()
    assert torch.equal(y2, y) and torch.isfinite(dx2).all()
    assert rel(dx2, dx) <= 1e-6                                         # (gy here is torch's product, not autograd's: last-bit differences)
    for k, (off, cnt) in st.ranges.items():
        if is_parameter(k):
            assert torch.isfinite(flat[off:off + cnt]).all(), k
            assert rel(flat[off:off + cnt].view(grads[k].shape), grads[k]) <= 1e-6, k
        else:
            assert torch.isnan(flat[off:off + cnt]).all(), k            # a buffer's slot is never written
    with pytest.raises(ValueError):
        _lib.check(lib.nd_unet_grad_backward(net.grad_flags, st.flat.data_ptr(), None, st.blobs.data_ptr(), gy.data_ptr(), None, *args))


# ---------------------------------------------------------------------------- GPU: frames
def _fid(c):
    return "seed{}-{}x{}-{}-{}-{}-b{}".format(c[0], *c[1])


@functools.lru_cache(maxsize=None)
def frame_case(ci):
    """FRAME_CASES[ci]: (conditioned weights, frame, target, float64 canvas, d loss / d frame, {name: gradient}, near_tie_mask [H,W]) with gather and stitch
    written from the oracle's index maps (test_frame_grad_host.oracle_maps), loss = MSE of the canvas against a random target.  The
    weights are conditioned on the batch of all the frame's tiles for the kink margin alone: a frame's tiles hold millions of pool
    windows, and some pair of maxima closer than POOL_MARGIN cannot be avoided (gaps down to 7e-8 here)."""
    seed, geom = FRAME_CASES[ci]
    W, H, cs, ucs, ol, batch = geom
    src, dst, w = (torch.from_numpy(a.copy()) for a in _load("test_frame_grad_host.py").oracle_maps((W, H, cs, ucs, ol)))
    n = src.shape[0]
    frame = torch.from_numpy(f64._frame(geom))
    tiles32 = frame.reshape(3, H * W)[:, src.reshape(-1)].reshape(3, n, cs, cs).permute(1, 0, 2, 3).contiguous()
    sd, _ = conditioned(f64._sd(seed), tiles32, pool_margin=None)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(7 + seed))
    p = {k: (v.double().requires_grad_(is_parameter(k)) if v.is_floating_point() else v) for k, v in sd.items()}
    xr = frame.double().requires_grad_()
    tiles = xr.reshape(3, H * W)[:, src.reshape(-1)].reshape(3, n, cs, cs).permute(1, 0, 2, 3)
    mask = torch.zeros(H * W, dtype=torch.bool)          # near_tie_mask: frame pixels within reach of a pool window closer than POOL_MARGIN

    def near_ties(lvl, t):
        h, w_ = t.size(2) // 2 * 2, t.size(3) // 2 * 2
        top = F.unfold(t.detach()[:, :, :h, :w_].reshape(-1, 1, h, w_), 2, stride=2).topk(2, dim=1).values
        close = ((top[:, 1] > 0) & (top[:, 0] - top[:, 1] < POOL_MARGIN)).reshape(n, -1, h // 2, w_ // 2).any(dim=1)
        # a window of level lvl covers 2^lvl tile pixels a side.  Which of its pixels takes the gradient decides nothing outside the way
        # back to the input: the double conv of every level above spreads it by 2 pixels of that level, a pool stays inside its
        # cell: 2 * (2^(lvl-1) + ... + 1) = 2^(lvl+1) - 2 tile pixels further on each side
        s_, r = 2 ** lvl, 2 ** (lvl + 1) - 2
        for i, wy, wx in close.nonzero().tolist():
            ys, xs = slice(max(0, wy * s_ - r), (wy + 1) * s_ + r), slice(max(0, wx * s_ - r), (wx + 1) * s_ + r)
            mask[src[i, ys, xs].reshape(-1)] = True

    y = forward_graph(p, tiles, pool_hook=near_ties)
    keep = (w != 0).reshape(-1)
    contrib = (y * w.double().unsqueeze(1)).permute(1, 0, 2, 3).reshape(3, -1)[:, keep]
    canvas = torch.zeros(3, H * W, dtype=torch.float64).index_add(1, dst.reshape(-1)[keep], contrib).reshape(3, H, W)
    names = [k for k in p if is_parameter(k)]
    g = torch.autograd.grad(F.mse_loss(canvas, target.double()), [xr] + [p[k] for k in names])
    return sd, frame, target, canvas.detach(), g[0], dict(zip(names, g[1:])), mask.reshape(H, W)


def _frame_run(net, frame, cot, dev, geom, want_img=True, tile_range=None):
    """canvas.backward(cot) through frame_grad.denoise_frame: (canvas, frame gradient, {name: grad})."""
    from nind_denoise_amd import frame_grad
    W, H, cs, ucs, ol, batch = geom
    net.zero_grad(set_to_none=True)
    img = frame.to(dev).requires_grad_(want_img)
    canvas = frame_grad.denoise_frame(net, img, cs, ucs, ol, batch=batch, tile_range=tile_range)
    canvas.backward(cot)
    return canvas.detach(), img.grad, {k: p.grad for k, p in net.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(FRAME_CASES)), ids=lambda i: _fid(FRAME_CASES[i]))
def test_frame_gradients(dev, ci):
    from nind_denoise_amd import pipeline
    geom = FRAME_CASES[ci][1]
    W, H, cs, ucs, ol, batch = geom
    sd, frame, target, canvas64, gimg64, g64, near = frame_case(ci)
    net = _net(dev, sd)
    want = pipeline.denoise_frame(net, frame.to(dev), cs, ucs, ol, batch=batch)
    cot = (2.0 / want.numel()) * (want - target.to(dev))                       # d MSE / d canvas at the canvas the forward gives
    canvas, gimg, grads = _frame_run(net, frame, cot, dev, geom)
    assert torch.equal(canvas, want)
    e = (canvas.double().cpu() - canvas64).abs().max().item()
    print(f"UNet grad frame {geom}: canvas vs float64 {e:.2e}")
    assert e <= f64.BAR_UNET_FRAME, e
    whole = rel(gimg, gimg64)
    print(f"UNet grad frame {geom}: frame.grad over the whole frame {whole:.2e}, {int(near.sum())} of {H * W} pixels within reach of a near tie")
    if FRAME_MASKED[ci]:
        assert near.float().mean().item() <= NEAR_TIE_SHARE and whole <= FRAME_DX_WHOLE, (near.float().mean().item(), whole)
        fig = class_figures(None, grads, None, g64)
        far = (~near).expand(3, H, W)
        fig["dx"] = ((gimg.double().cpu() - gimg64)[far].abs().max().item() / gimg64.abs().max().item(), "frame.grad off the near ties")
    else:
        fig = class_figures(gimg, grads, gimg64, g64)
    _assert_bars(f"frame {geom}", fig, FRAME_BARS[ci])
    # the frame's gradient alone: the same bits, no parameter gradient
    net.requires_grad_(False)
    c2, gimg2, grads2 = _frame_run(net, frame, cot, dev, geom)
    assert torch.equal(c2, want) and torch.equal(gimg2, gimg) and all(g is None for g in grads2.values())
    # parameters alone
    net.requires_grad_(True)
    c3, gimg3, grads3 = _frame_run(net, frame, cot, dev, geom, want_img=False)
    assert gimg3 is None and all(torch.equal(grads3[k], grads[k]) for k in grads)


@pytest.mark.gpu
def test_frame_tile_ranges_add_up(dev):
    from nind_denoise_amd import frame_grad, pipeline
    geom = FRAME_CASES[0][1]
    W, H, cs, ucs, ol, batch = geom
    sd, frame = frame_case(0)[:2]
    net = _net(dev, sd)
    n = pipeline.tile_count(W, H, cs, ucs, ol)
    cut = batch + 1                                                             # both ranges end in a partial launch
    assert 0 < cut < n and cut % batch and (n - cut) % batch
    cot = torch.rand(3, H, W, generator=torch.Generator().manual_seed(11)).to(dev) - 0.5
    whole = _frame_run(net, frame, cot, dev, geom)
    a = _frame_run(net, frame, cot, dev, geom, tile_range=(0, cut))
    b = _frame_run(net, frame, cot, dev, geom, tile_range=(cut, n))
    assert torch.equal(a[0], pipeline.denoise_frame(net, frame.to(dev), cs, ucs, ol, batch=batch, tile_range=(0, cut)))
    assert not torch.equal(a[1], whole[1]) and a[1].abs().max().item() > 0
    # the backward is linear in the tiles, but the launches group differently, so the fp32 sums re-associate: both sides are fp32
    # evaluations of one exact quantity, each held to its class bar, so they differ by at most twice that
    fig = class_figures(a[1] + b[1], {k: a[2][k] + b[2][k] for k in a[2]}, whole[1], whole[2])
    _show(f"frame {geom} ranges [0,{cut}) + [{cut},{n}) vs whole", fig)
    assert all(v <= 2 * BARS[c] for c, (v, _) in fig.items()), fig
    with pytest.raises(RuntimeError, match="eval mode"):
        frame_grad.denoise_frame(net.train(), frame.to(dev).requires_grad_(), cs, ucs, ol, batch=batch)
