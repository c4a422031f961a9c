"""UNet training on batch statistics (nd_unet_train_forward / nd_unet_train_backward, train.UNetTrainer) against float64 autograd of
the train-mode graph: test_unet_grad.forward_graph restated with F.batch_norm(z, None, None, gamma, beta, training=True, eps=1e-5).

Weights, inputs and the conditioning are those of test_unet_grad.py (loaded with importlib): `conditioned` runs on the TRAIN-mode
float64 forward -- a BatchNorm bias shift changes only that channel's output, exactly as in eval mode, because the statistics are
taken before it -- with the same KINK_MARGIN, SLACK and POOL_MARGIN, both margins asserted with the rounded weights.  Loss: MSE against
torch.rand(shape, manual_seed(5)).

CASES are the shapes at which the float64 reference itself is well conditioned: every BatchNorm layer sees at least 8 values per channel
and no batch variance below 1e-3 (test_unet_train_host.py prints and asserts the conditioning report and torch's own fp32 on the CPU
against float64).  (2,16,16) and (4,17,31) are not cases: 2 and 4 values per channel at the bottom, batch variances of 7e-10 and 1e-4.

One divergence from torch, asserted here: the bias gradient of the 18 convolutions that feed a BatchNorm is EXACTLY 0 (its exact value;
float64 autograd gives <= 5e-17, torch fp32 about 3e-9 of rounding noise), so those tensors are compared with `== 0`, not with a
relative error, and after an optimiser step those biases are bit-unchanged."""
import functools
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib


def _load(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    spec = importlib.util.spec_from_file_location("_unet_train_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("test_unet_grad.py")
f64 = G.f64
BAR_UNET_FWD = f64.BAR_UNET_FWD
KINK_MARGIN, POOL_MARGIN = G.KINK_MARGIN, G.POOL_MARGIN
MOMENTUM = 0.1

# (seed, shape, planted)
CASES = [(3, (3, 33, 47), False),      # fix-up lines at odd sizes, 12 values per channel at the bottom
         (3, (2, 100, 92), False),     # a fix-up, larger planes
         (3, (8, 16, 16), False),      # 1x1 bottom: statistics purely across the batch
         (0, (2, 32, 32), False),
         (0, (2, 64, 16), False),
         (3, (3, 33, 47), True)]       # gamma = 0 and gamma < 0 channels
MAIN = CASES[0]

# Bars: max |err| / max |ref| per tensor against float64, per class of tensor; about 3x the worst value measured on the MI355X over
# CASES, in brackets torch fp32 autograd on the CPU against the same reference (test_unet_train_host.py prints and asserts those).
# y is held to BAR_UNET_FWD (max |err|, a sigmoid).  run_mean / run_var: the running statistics after one forward.
# test_unet_train_host.py::test_bars_see_batchnorm_errors requires every bar to be 10x below what a dropped dbeta / N or
# xhat dgamma / N term, N - 1 for N in the variance, or a fix-up line counted in a statistic does to the class.
BARS = {
    "dx": 1.15e-5,       # measured 3.79e-6 (2x64x16)                                  [cpu fp32 4.5e-6]
    "conv_w": 2e-5,      # measured 6.54e-6 (down4.mpconv.1.conv.3, 2x64x16)           [cpu fp32 1.4e-5]
    "conv_b": 3e-7,      # measured 1.01e-7 (outc.conv.bias alone, 3x33x47: the 18 pre-BatchNorm biases are == 0)   [cpu fp32 3.6e-7]
    "bn_w": 2.1e-5,      # measured 7.08e-6 (inc.conv.conv.4, 2x64x16)                 [cpu fp32 8.3e-6]
    "bn_b": 1.35e-5,     # measured 4.48e-6 (down3.mpconv.1.conv.1, 8x16x16)           [cpu fp32 5.0e-6]
    "up_w": 3.2e-5,      # measured 1.05e-5 (up1.up, 8x16x16)                          [cpu fp32 1.0e-5]
    "up_b": 2e-5,        # measured 6.51e-6 (up4.up, 2x100x92)                         [cpu fp32 1.8e-5]
    "run_mean": 1.6e-6,  # measured 5.18e-7 (down4.mpconv.1.conv.1, 2x32x32)           [cpu fp32 6.0e-7]
    "run_var": 1e-6,     # measured 3.20e-7 (down4.mpconv.1.conv.1, 3x33x47)           [cpu fp32 5.8e-7]
}
# split_k = False (ND_FLAG_NO_SPLITK): the deep layers' 4608 ... 9216-term sums run as one fp32 chain, in the forward and in both
# gradients.  3x what was measured on 3x33x47, its one case; y there 2.67e-6, held to BAR_UNET_FWD like every other.
BARS_NO_SPLITK = {"dx": 1.7e-5, "conv_w": 3.4e-5, "conv_b": 6.2e-7, "bn_w": 3.2e-5, "bn_b": 2.8e-5, "up_w": 4.7e-5, "up_b": 1.2e-5,
                  "run_mean": 3.2e-6, "run_var": 1.7e-6}
# (measured:      dx 5.65e-6, conv_w 1.14e-5, conv_b 2.06e-7, bn_w 1.08e-5, bn_b 9.26e-6, up_w 1.55e-5, up_b 4.00e-6, run_mean 1.05e-6, 5.74e-7)


def pre_bn_bias(name):
    """One of the 18 convolution biases that feed a BatchNorm (outc.conv.bias does not)."""
    return G.klass(name) == "conv_b" and not name.startswith("outc.")


def _cid(c):
    return f"seed{c[0]}-" + "x".join(str(v) for v in c[1]) + ("-planted" if c[2] else "")


# ---------------------------------------------------------------------------- the train-mode graph in float64
class _BnReluFormulas(torch.autograd.Function):
    """a = ReLU(gamma xhat + beta) on batch statistics and its backward, written from the formulas the kernels implement; knobs model
    the errors of the gate: "nm1" (N - 1 for N in the forward variance), "line" (one zero line per image counted in the statistics),
    "no_dbeta" / "no_dgamma" (that term of g_z dropped; read at backward time)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, knobs):
        n = z.numel() // z.size(1)
        zs = F.pad(z, (0, 0, 0, 1)) if knobs.get("line") else z
        ns = zs.numel() // zs.size(1)
        mu = zs.sum(dim=(0, 2, 3)) / ns
        var = ((zs - mu[None, :, None, None]) ** 2).sum(dim=(0, 2, 3)) / (ns - 1 if knobs.get("nm1") else ns)
        inv = 1.0 / torch.sqrt(var + 1e-5)
        xhat = (z - mu[None, :, None, None]) * inv[None, :, None, None]
        a = F.relu(gamma[None, :, None, None] * xhat + beta[None, :, None, None])
        ctx.save_for_backward(xhat, a, gamma, inv)
        ctx.n, ctx.knobs = n, knobs
        return a

    @staticmethod
    def backward(ctx, ga):
        xhat, a, gamma, inv = ctx.saved_tensors
        gm = ga * (a > 0)
        dbeta = gm.sum(dim=(0, 2, 3))
        dgamma = (gm * xhat).sum(dim=(0, 2, 3))
        t = gm
        if not ctx.knobs.get("no_dbeta"):
            t = t - (dbeta / ctx.n)[None, :, None, None]
        if not ctx.knobs.get("no_dgamma"):
            t = t - xhat * (dgamma / ctx.n)[None, :, None, None]
        return (gamma * inv)[None, :, None, None] * t, dgamma, dbeta, None


def _double_conv(sd, p, x, bn_hook, knobs, momentum, line):
    for k in (0, 3):
        z = F.conv2d(x, sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"], padding=1)
        g, b = sd[f"{p}.{k + 1}.weight"], sd[f"{p}.{k + 1}.bias"]
        if knobs:      # the formulas, with the gate's errors ("line": only in the layer that reads a fix-up line)
            x = _BnReluFormulas.apply(z, g, b, dict(knobs, line=knobs.get("line") and line and k == 0))
            continue
        rm, rv = (sd[f"{p}.{k + 1}.running_mean"], sd[f"{p}.{k + 1}.running_var"]) if momentum is not None else (None, None)
        t = F.batch_norm(z, rm, rv, g, b, training=True, momentum=momentum or 0.0, eps=1e-5)      # (rm, rv move in place)
        if bn_hook is not None:
            t = bn_hook(f"{p}.{k + 1}", t)
        x = F.relu(t)
    return x


def train_graph(sd, x, find_noise=False, knobs=None, bn_hook=None, pool_hook=None, momentum=None):
    """UNet.forward in train() mode (test_unet_grad.forward_graph with batch statistics).  momentum: the running statistics in sd are
    updated in place as nn.BatchNorm2d does (None: left alone).  knobs: non-empty = the formula restatement with the gate's errors."""
    knobs = knobs or {}
    skips = [_double_conv(sd, "inc.conv.conv", x, bn_hook, knobs, momentum, False)]
    for n in (1, 2, 3, 4):
        if pool_hook is not None:
            pool_hook(n, skips[-1])
        skips.append(_double_conv(sd, f"down{n}.mpconv.1.conv", F.max_pool2d(skips[-1], 2), bn_hook, knobs, momentum, False))
    t = skips[4]
    for n, skip in zip((1, 2, 3, 4), (skips[3], skips[2], skips[1], skips[0])):
        up = F.conv_transpose2d(t, sd[f"up{n}.up.weight"], sd[f"up{n}.up.bias"], stride=2)
        dy, dx = skip.size(2) - up.size(2), skip.size(3) - up.size(3)
        assert dy in (0, 1) and dx in (0, 1)
        up = F.pad(up, (0, dx, 0, dy))
        t = _double_conv(sd, f"up{n}.conv.conv", torch.cat([skip, up], dim=1), bn_hook, knobs, momentum, bool(dy or dx))
    s = torch.sigmoid(F.conv2d(t, sd["outc.conv.weight"], sd["outc.conv.bias"]))
    return x - s if find_noise else s


def _to64(sd):
    return {k: v.double() if v.is_floating_point() else v for k, v in sd.items()}


def margins(sd64, x64):
    """test_unet_grad.margins on the train-mode forward, plus the least values per channel and the least batch variance of a layer."""
    out = {"kink": float("inf"), "pool": float("inf"), "values": 10 ** 9, "variance": float("inf")}

    def bn(name, t):
        out["kink"] = min(out["kink"], t.abs().min().item())
        out["values"] = min(out["values"], t.numel() // t.size(1))
        g, b = sd64[name + ".weight"], sd64[name + ".bias"]
        live = g != 0
        if live.any():      # var of z = var of (t - beta) / gamma ... of xhat-scaled output: recover the batch variance of z
            xh = (t - b[None, :, None, None])[:, live] / g[live][None, :, None, None]
            v = xh.var(dim=(0, 2, 3), unbiased=False)              # = var_z / (var_z + eps)
            out["variance"] = min(out["variance"], (1e-5 * v / (1 - v).clamp_min(1e-300)).min().item())
        return t

    def pool(n, t):
        h, w = t.size(2) // 2 * 2, t.size(3) // 2 * 2
        top = F.unfold(t[:, :, :h, :w].reshape(-1, 1, h, w), 2, stride=2).topk(2, dim=1).values
        both = (top[:, 1] > 0) & (top[:, 0] != top[:, 1])
        if both.any():
            out["pool"] = min(out["pool"], (top[:, 0] - top[:, 1])[both].min().item())

    with torch.no_grad():
        train_graph(sd64, x64, bn_hook=bn, pool_hook=pool)
    return out


def conditioned(sd, x):
    """test_unet_grad.conditioned on the train-mode float64 forward: (fp32 weights with shifted BatchNorm biases, report), both
    margins asserted with the rounded weights."""
    sd = {k: v.clone() for k, v in sd.items()}
    sd64 = _to64(sd)
    report = {"shifted": 0, "max_shift": 0.0}

    def shift(name, t):
        near = (t.abs().amin(dim=(0, 2, 3)) < KINK_MARGIN).nonzero().flatten().tolist()
        for c in near:
            s = G._least_shift(t[:, c].reshape(-1), KINK_MARGIN)
            b = sd64[name + ".bias"][c].item()
            nb = torch.tensor(b + s, dtype=torch.float64).float()
            sd[name + ".bias"][c] = nb
            sd64[name + ".bias"][c] = nb.double()
            t[:, c] += nb.double().item() - b
            report["shifted"] += 1
            report["max_shift"] = max(report["max_shift"], abs(s))
        return t

    with torch.no_grad():
        train_graph(sd64, x.double(), bn_hook=shift)
    report.update(margins(_to64(sd), x.double()))
    assert report["kink"] >= KINK_MARGIN and report["pool"] >= POOL_MARGIN, report
    return sd, report


def target_for(shape):
    b, h, w = shape
    return torch.rand((b, 3, h, w), generator=torch.Generator().manual_seed(5))


def reference(sd, x, target, find_noise=False, knobs=None, dtype=torch.float64):
    """(y, dx, {name: gradient}, {name: running statistic after one forward}) of MSE(train_graph(x), target) by torch autograd on the
    CPU in `dtype`."""
    p = {k: (v.to(dtype).clone().requires_grad_(G.is_parameter(k)) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    xr = x.to(dtype).requires_grad_()
    y = train_graph(p, xr, find_noise=find_noise, knobs=knobs, momentum=None if knobs else MOMENTUM)
    loss = F.mse_loss(y, target.to(dtype))
    names = [k for k in p if G.is_parameter(k)]
    g = torch.autograd.grad(loss, [xr] + [p[k] for k in names])
    stats = {k: v.detach() for k, v in p.items() if k.endswith(("running_mean", "running_var"))}
    return y.detach(), g[0], dict(zip(names, g[1:])), stats


@functools.lru_cache(maxsize=None)
def train_case(case, find_noise=False):
    """(conditioned fp32 weights, input, target, float64 y, dx, {name: gradient}, {name: running statistic}); computed once, never
    modified."""
    seed, shape, planted = case
    x = f64._input(seed, shape)
    sd, _ = conditioned(f64._sd(seed, planted), x)
    target = target_for(shape)
    return (sd, x, target) + reference(sd, x, target, find_noise)


def class_figures(dx, grads, ref_dx, ref_grads):
    """test_unet_grad.class_figures without the 18 pre-BatchNorm biases."""
    return G.class_figures(dx, grads, ref_dx, ref_grads, want={k for k in ref_grads if not pre_bn_bias(k)})


def stat_figures(got, ref):
    fig = {}
    for k, r in ref.items():
        c = "run_mean" if k.endswith("running_mean") else "run_var"
        e = G.rel(got[k], r)
        if e >= fig.get(c, (-1.0, ""))[0]:
            fig[c] = (e, k)
    return fig


def _assert_bars(what, fig, bars):
    print(f"UNet train {what}: " + ", ".join(f"{c} {v:.2e} ({k})" for c, (v, k) in sorted(fig.items())))
    for c, (v, k) in fig.items():
        assert v <= bars[c], (what, c, k, v, bars[c])


# ---------------------------------------------------------------------------- GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _trainer(dev, sd, find_noise=False, split_k=True, **kw):
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    from nind_denoise_amd.train import UNetTrainer
    net = UNet(find_noise=find_noise)
    net.load_state_dict(sd)
    net.split_k = split_k
    return UNetTrainer(net, device=dev, **kw)


def _run(tr, x, target, want_dx=True):
    """One forward / backward through the trainer's two halves with torch's MSE gradient in between: (y, dx, {name: grad},
    {name: running statistic})."""
    dev = tr.device
    y = tr.forward(x.to(dev))
    gy = (2.0 / y.numel()) * (y - target.to(dev))
    dx = tr.backward(gy, want_dx=want_dx)
    sd = tr.model.state_dict()
    grads = {k: tr.grad_of(k).clone() for k in sd if G.is_parameter(k)}
    stats = {k: v.clone() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))}
    return y, dx, grads, stats


def _check_case(what, out, ref, bars=BARS):
    y, dx, grads, stats = out
    y64, dx64, g64, s64 = ref
    ey = (y.double().cpu() - y64).abs().max().item()
    print(f"UNet train {what}: y vs float64 {ey:.2e}")
    fig = class_figures(dx, grads, dx64, g64)
    fig.update(stat_figures(stats, s64))
    _assert_bars(what, fig, bars)
    assert ey <= BAR_UNET_FWD, ey
    zero = [k for k in g64 if pre_bn_bias(k)]
    assert len(zero) == 18 and all(not grads[k].any() for k in zero)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_cid)
def test_y_dx_every_gradient_and_the_running_statistics(dev, case):
    sd, x, target, *ref = train_case(case)
    if case[2]:
        gamma = sd["down2.mpconv.1.conv.1.weight"]
        assert (gamma == 0).any() and (gamma < 0).any()
    tr = _trainer(dev, sd)
    before = [t.item() for t in tr._tracked]
    out = _run(tr, x, target)
    _check_case(_cid(case), out, ref)
    assert len(before) == 18 and [t.item() for t in tr._tracked] == [b + 1 for b in before]
    tracked = {k: v.item() for k, v in tr.model.state_dict().items() if k.endswith("num_batches_tracked")}
    assert len(tracked) == 18 and all(v == sd[k].item() + 1 for k, v in tracked.items())


@pytest.mark.gpu
def test_find_noise(dev):
    sd, x, target, *ref = train_case(MAIN, find_noise=True)
    assert not torch.equal(ref[1], train_case(MAIN)[4])
    _check_case("find_noise", _run(_trainer(dev, sd, find_noise=True), x, target), ref)


@pytest.mark.gpu
def test_no_splitk(dev):
    sd, x, target, *ref = train_case(MAIN)
    _check_case("split_k=False", _run(_trainer(dev, sd, split_k=False), x, target), ref, BARS_NO_SPLITK)


@pytest.mark.gpu
def test_without_dx_and_twice_the_same_bits(dev):
    sd, x, target = train_case(MAIN)[:3]
    a = _run(_trainer(dev, sd), x, target)
    b = _run(_trainer(dev, sd), x, target)
    c = _run(_trainer(dev, sd), x, target, want_dx=False)
    assert c[1] is None
    for other in (b, c):
        assert torch.equal(a[0], other[0]) and (other[1] is None or torch.equal(a[1], other[1]))
        assert all(torch.equal(a[2][k], other[2][k]) for k in a[2]) and all(torch.equal(a[3][k], other[3][k]) for k in a[3])
    # and on ONE trainer, from the same weights and statistics: the same bits again
    tr = _trainer(dev, sd)
    flat0 = tr.flat.clone()
    first = _run(tr, x, target)
    tr.flat.copy_(flat0)
    again = _run(tr, x, target)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert all(torch.equal(first[2][k], again[2][k]) for k in first[2]) and all(torch.equal(first[3][k], again[3][k]) for k in first[3])


@pytest.mark.gpu
def test_workspace_rebuilt_for_another_shape(dev):
    sd, x, target, *ref = train_case(MAIN)
    tr = _trainer(dev, sd)
    flat0 = tr.flat.clone()
    first = _run(tr, x, target)
    other = CASES[3]
    mid = _run(tr, train_case(other)[1], train_case(other)[2])
    assert torch.isfinite(mid[1]).all() and list(tr._ws) == [(32, 32, 2)]
    tr.flat.copy_(flat0)
    again = _run(tr, x, target)
    assert list(tr._ws) == [(33, 47, 3)]
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert all(torch.equal(first[2][k], again[2][k]) for k in first[2])
    _check_case("after another shape", again, ref)


@pytest.mark.gpu
def test_outputs_prefilled_with_nan_are_overwritten(dev):
    lib = _lib.load()
    sd, x, target = train_case(MAIN)[:3]
    b, h, w = MAIN[1]
    tr = _trainer(dev, sd)
    flat0 = tr.flat.clone()
    y, dx, grads, _ = _run(tr, x, target)
    tr.flat.copy_(flat0)
    xd, nan = x.to(dev), float("nan")
    y2, dx2, flat = torch.full_like(xd, nan), torch.full_like(xd, nan), torch.full_like(tr.grads, nan)
    ws = tr.workspace(h, w, b)
    args = (b, h, w)
    tail = (ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(lib.nd_unet_train_forward(tr.flags, tr.flat.data_ptr(), tr.blobs.data_ptr(), xd.data_ptr(), y2.data_ptr(), *args, MOMENTUM, *tail))
    gy = (2.0 / y2.numel()) * (y2 - target.to(dev))
    _lib.check(lib.nd_unet_train_backward(tr.flags, tr.flat.data_ptr(), flat.data_ptr(), tr.blobs.data_ptr(), gy.data_ptr(), dx2.data_ptr(),
                                          *args, *tail))
    torch.cuda.synchronize()
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    for k, (off, cnt) in tr.ranges.items():
        if G.is_parameter(k):
            assert torch.equal(flat[off:off + cnt].view(grads[k].shape), grads[k]), k
        else:
            assert torch.isnan(flat[off:off + cnt]).all(), k            # a running statistic's slot is never written
    with pytest.raises(ValueError):                                     # neither gradients nor dx
        _lib.check(lib.nd_unet_train_backward(tr.flags, tr.flat.data_ptr(), None, tr.blobs.data_ptr(), gy.data_ptr(), None, *args, *tail))
    for bad in (-0.1, 1.5, nan):
        with pytest.raises(ValueError, match="momentum"):
            _lib.check(lib.nd_unet_train_forward(tr.flags, tr.flat.data_ptr(), tr.blobs.data_ptr(), xd.data_ptr(), y2.data_ptr(), *args, bad,
                                                 *tail))
    with pytest.raises(ValueError, match="unknown flag"):
        _lib.check(lib.nd_unet_train_forward(1 << 20, tr.flat.data_ptr(), tr.blobs.data_ptr(), xd.data_ptr(), y2.data_ptr(), *args, MOMENTUM,
                                             *tail))


@pytest.mark.gpu
def test_one_value_per_channel_raises(dev):
    tr = _trainer(dev, train_case(MAIN)[0])
    with pytest.raises(ValueError, match="more than 1"):
        tr.forward(torch.rand(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="eval mode"):
        tr.model.train()(torch.rand(2, 3, 16, 16, device=dev))


# ---------------------------------------------------------------------------- the trainer
STEPS, LR = 3, 1e-4
# Three Adam(amsgrad) steps at lr 1e-4, MSE weight 1, on MAIN, against the float64 graph under torch.optim.Adam(amsgrad=True) on the
# CPU.  Figure per tensor, worst per class: ||p - p64|| / ||p64 - p0|| (2-norms; p0 = the starting value: the error of the UPDATE), running
# statistics ||err|| / ||ref||.
# Adam's steps are sign-like (m / sqrt(v) = +-1 whatever |g|): an element whose gradient is within rounding of 0 moves by another
# fraction of lr on the two sides, so even the first step is far looser than the gradient bars (STEP1_BARS).  After it every element
# has moved by ~lr = 3x KINK_MARGIN, the conditioning of the case is gone, and the float64 loop sits next to a ReLU / pool-maximum
# decision that fp32 evaluations take either way: torch's own fp32 loop on the CPU lands at ~1e-3 with its default convolutions, at
# ~7e-3 with the oneDNN ones switched off, and at 2 ... 3e-2 from weights one fp32 rounding away (one_rounding_away seeds 1 and 3) --
# three branches, and nothing in between.  An element-wise maximum is no measure at all there (0.09 ... 0.48 x STEPS x LR on single
# elements of conv_w over the same four loops; printed, not asserted), while a wrong lr, bias correction or amsgrad moves EVERY
# element and shows in the 2-norm at 0.1 ... 1, and in the first step alone against bars 30x tighter.
# Bars: 3x the worst of those four fp32 CPU loops against float64, worst figure in brackets
# (test_unet_train_host.py::test_cpu_fp32_adam_loop runs the four loops, prints and asserts them).
STEP1_BARS = {
    "conv_w": 1.53e-3,    # [cpu fp32 5.07e-4, inc.conv.conv.3.weight, oneDNN off]
    "conv_b": 2.46e-4,    # [cpu fp32 8.18e-5, outc.conv.bias, neighbour 1]
    "bn_w": 2.76e-3,      # [cpu fp32 9.18e-4, up3.conv.conv.1.weight, neighbour 1]
    "bn_b": 6.21e-4,      # [cpu fp32 2.06e-4, down4.mpconv.1.conv.1.bias, neighbour 1]
    "up_w": 3.24e-4,      # [cpu fp32 1.07e-4, up3.up.weight, oneDNN off]
    "up_b": 9.69e-5,      # [cpu fp32 3.22e-5, up4.up.bias, neighbour 3]
    "run_mean": 1.83e-6,  # [cpu fp32 6.07e-7, down4.mpconv.1.conv.1.running_mean, oneDNN off]
    "run_var": 4.92e-7,   # [cpu fp32 1.63e-7, down4.mpconv.1.conv.1.running_var, oneDNN off]
}
STEP_BARS = {
    "conv_w": 7.98e-2,    # [cpu fp32 2.65e-2, down4.mpconv.1.conv.3.weight, neighbour 1]
    "conv_b": 6.81e-5,    # [cpu fp32 2.26e-5, outc.conv.bias, default]
    "bn_w": 8.4e-2,       # [cpu fp32 2.79e-2, inc.conv.conv.4.weight, neighbour 1]
    "bn_b": 9.75e-2,      # [cpu fp32 3.24e-2, up2.conv.conv.4.bias, neighbour 3]
    "up_w": 6.03e-2,      # [cpu fp32 2.00e-2, up2.up.weight, neighbour 1]
    "up_b": 5.31e-2,      # [cpu fp32 1.76e-2, up2.up.bias, neighbour 3]
    "run_mean": 5.04e-4,  # [cpu fp32 1.67e-4, down4.mpconv.1.conv.4.running_mean, neighbour 1]
    "run_var": 1.65e-4,   # [cpu fp32 5.49e-5, down4.mpconv.1.conv.1.running_var, neighbour 1]
}
# measured on the MI355X after the first step: conv_w 2.04e-4, conv_b 1.57e-5, bn_w 3.27e-4, bn_b 5.41e-5, up_w 6.24e-5, up_b 1.35e-5,
# run_mean 3.81e-7, run_var 1.01e-7; after three (the branch of neighbour 1): conv_w 2.67e-2, conv_b 2.27e-5, bn_w 2.70e-2, bn_b 2.92e-2, up_w 2.01e-2,
# up_b 1.75e-2, run_mean 1.67e-4, run_var 5.49e-5


def adam_loop(sd, x, target, dtype):
    """[{name: tensor} after step 1, ..., after step STEPS] of the train-mode graph under torch.optim.Adam(amsgrad=True) on the CPU in
    `dtype`."""
    p = {k: (v.to(dtype).clone().requires_grad_(G.is_parameter(k)) if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    names = [k for k in p if G.is_parameter(k)]
    opt = torch.optim.Adam([p[k] for k in names], lr=LR, betas=(0.75, 0.999), eps=1e-8, amsgrad=True)
    states = []
    for _ in range(STEPS):
        opt.zero_grad()
        F.mse_loss(train_graph(p, x.to(dtype), momentum=MOMENTUM), target.to(dtype)).backward()
        opt.step()
        states.append({k: v.detach().clone() for k, v in p.items()})
    return states


@functools.lru_cache(maxsize=None)
def adam_reference():
    sd, x, target = train_case(MAIN)[:3]
    return adam_loop(sd, x, target, torch.float64)


def one_rounding_away(sd, seed):
    """sd with every parameter element moved to a neighbouring fp32 number, or left, at random: weights that round to the same float64
    reference within 6e-8, for another fp32 evaluation of the same loop."""
    g = torch.Generator().manual_seed(seed)
    return {k: (torch.nextafter(v, v + (torch.randint(0, 3, v.shape, generator=g) - 1).float()) if G.is_parameter(k) else v)
            for k, v in sd.items()}


def step_figures(got, ref, start, elementwise=False, steps=STEPS):
    """{class: (worst figure, tensor)} of a state-dict after the loop against the float64 one, without the 18 pre-BatchNorm biases:
    the figure STEP_BARS describes (start: the state-dict before the loop), or with elementwise max |p - ref| / (STEPS LR) for the
    parameters and max |err| / max |ref| for the statistics (printed for the record, not asserted)."""
    fig = {}
    for k, r in ref.items():
        if k.endswith("num_batches_tracked") or pre_bn_bias(k):
            continue
        g, r = got[k].detach().double().cpu(), r.double()
        if G.is_parameter(k):
            c = G.klass(k)
            e = (g - r).abs().max().item() / (steps * LR) if elementwise else ((g - r).norm() / (r - start[k].double()).norm()).item()
        else:
            c = "run_mean" if k.endswith("running_mean") else "run_var"
            e = G.rel(g, r) if elementwise else ((g - r).norm() / r.norm()).item()
        if e >= fig.get(c, (-1.0, ""))[0]:
            fig[c] = (e, k)
    return fig


def show_steps(what, got, ref, start, steps=STEPS):
    fig = step_figures(got, ref, start)
    print(f"UNet train {steps} steps, {what}: " + ", ".join(f"{c} {v:.2e} ({k})" for c, (v, k) in sorted(fig.items())))
    print(f"UNet train {steps} steps, {what}, element-wise: " + ", ".join(
        f"{c} {v:.2e} ({k})" for c, (v, k) in sorted(step_figures(got, ref, start, elementwise=True, steps=steps).items())))
    return fig


@pytest.mark.gpu
def test_three_learn_steps(dev):
    sd, x, target = train_case(MAIN)[:3]
    tr = _trainer(dev, sd, lr=LR, weights={"MSE": 1.0})
    ref = adam_reference()
    losses = [tr.learn(x, target).item()]
    first = {k: v.clone() for k, v in tr.model.state_dict().items()}
    losses += [tr.learn(x, target).item() for _ in range(STEPS - 1)]
    assert tr.steps == STEPS and all(l > 0 for l in losses)
    got = tr.model.state_dict()
    fig1 = show_steps("MI355X", first, ref[0], sd, steps=1)
    fig = show_steps("MI355X", got, ref[-1], sd)
    for c in STEP_BARS:
        assert fig1[c][0] <= STEP1_BARS[c], (1, c, fig1[c])
        assert fig[c][0] <= STEP_BARS[c], (STEPS, c, fig[c])
    frozen = [k for k in sd if pre_bn_bias(k)]
    assert len(frozen) == 18 and all(torch.equal(got[k].cpu(), sd[k]) for k in frozen)
    assert all(got[k].item() == sd[k].item() + STEPS for k in sd if k.endswith("num_batches_tracked"))
    moved = [k for k in sd if G.is_parameter(k) and not pre_bn_bias(k)]
    assert all(not torch.equal(got[k].cpu(), sd[k]) for k in moved)


@pytest.mark.gpu
def test_eval_forward_after_learn_reads_the_new_weights(dev):
    sd, x, target = train_case(MAIN)[:3]
    tr = _trainer(dev, sd, lr=1e-2, weights={"MSE": 1.0})      # a step large enough to show in the output
    net = tr.model
    with torch.no_grad():
        y0 = net.eval()(x.to(dev))                              # packs and caches the inference blob
        tr.forward(x)                                           # moves the running statistics only
        y1 = net.eval()(x.to(dev))
        tr.learn(x, target)
        y2 = net.eval()(x.to(dev))
        now = _to64({k: v.cpu() for k, v in net.state_dict().items()})
        want = G.forward_graph(now, x.double())
    assert (y2.double().cpu() - want).abs().max().item() <= BAR_UNET_FWD
    assert (y1 - y0).abs().max().item() > 10 * BAR_UNET_FWD and (y2 - y1).abs().max().item() > 10 * BAR_UNET_FWD
    with pytest.raises(RuntimeError, match="eval mode"):
        net.train()(x.to(dev))


@pytest.mark.gpu
def test_reference_configuration_shape_at_batch_2(dev):
    from nind_denoise_amd import validation
    shape = (2, 220, 220)
    x, clean = f64._input(1, shape), target_for(shape)
    weights = {"MSSSIM": 1.0}
    tr = _trainer(dev, f64._sd(3), lr=3e-4, beta1=0.5, weights=weights, loss_cs=161)
    y, loss = tr.forward_backward(x, clean)
    want = validation.criteria(y, clean.to(dev), weights, 161)["weighted"].mean().item()
    # both are fp32 sums of the same two per-sample terms, divided by 2: a few ulp of the loss
    assert abs(loss.item() - want) <= 1e-6 * abs(want), (loss.item(), want)
    assert torch.isfinite(tr.grads).all() and tr.grads.abs().max().item() > 0
    tr.optimizer_step()
    assert tr.steps == 1 and torch.isfinite(tr.flat).all()
