"""UtNet(64) training against float64 autograd at the shapes the reference trains with: batch 30 of 184-pixel crops under
MS-SSIM (configs/train_conf_utnet_std.yaml), batch 30 of 136-pixel crops (tools/bench_train.py), Hardswish on rectangular
crops with the input image's gradient, and the split-K tail on and off.  Batch 30 sets the split-K tail of the forward and
data-gradient launches, the switch to conv_w2d from 512 workgroup tiles and the K-slice count of k_wgrad; none of the
other training tests reaches it.

A well-conditioned setup, so that the bars can sit near fp32's own error:
  * weights at VISIBLE_GAIN (test_shared_encoder.py), whose deep levels reach the output and carry gradients of the same
    order as the top ones;
  * the last 1x1 (tconvs4.4) rescaled affinely in float64 so that the float64 output of the first CAL crops has mean 0.5
    and std 0.05, then stored as fp32: both sides start from the same fp32 weights;
  * every float64 output pixel of the batch at least MARGIN from 0 and 1, so that clip(0, 1) is the identity on both
    sides and no pixel's gradient switches on or off between the two forward passes;
  * in the layers with fewer than NUDGE_PIXELS pixels per channel, no float64 pre-activation of the batch within KINK_MARGIN
    of an activation's kink (biases shifted where needed), so that no branch there differs between the two forward passes;
  * image-like crops (bilinear-upsampled noise) and targets clip(y64 + 0.02 + 0.03 randn): MS-SSIM's contrast terms stay
    positive, and the last bias' gradient does not hinge on the sample mean of the noise;
  * smooth criteria only (MSE, MS-SSIM).  L1 is left out: the sign of g - t flips on pixels where the two forward passes
    differ in the last bits, which moves a gradient by far more than rounding does.

The CPU gate test_train_bars_see_deep_gradients shows which bars can see a 1 % error in the gradient that flows back through a
pool or the bottom block (see BARS for the ones that cannot)."""
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth


def _shared_encoder_tests():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_shared_encoder.py")
    spec = importlib.util.spec_from_file_location("_shared_encoder_bars", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


VISIBLE_GAIN = _shared_encoder_tests().VISIBLE_GAIN

CAL = 4          # crops whose float64 output calibrates the last layer: the first CAL crops of every batch (the gate's batch)
MARGIN = 0.05    # no float64 output pixel closer than this to 0 or 1
BAND = 3         # border band of the input gradient (test_utnet_input_grad.py): every pixel the reflection fold touches

# Bars, per quantity class: y = max |err| / max(1, max |ref|); loss = |err| / |ref|; conv weights and biases = max |err| / max |ref|
# of each tensor, in three classes (the TOP levels, the bottom block, the other levels); PReLU slopes = |err| / max(|ref|,
# SLOPE_FLOOR x the largest slope gradient of the network); dx = ||err|| / ||ref|| (L2, whole and border band).  Worst values
# measured on MI355X in the comments.
#
# What sets how close fp32 comes to float64 here (torch fp32 autograd on the CPU shows the same figures on the same tensors):
#   * kink flips in the dense layers, which the kink margin above cannot clear: each moves one pixel's gradient by (1 - slope),
#     i.e. a deep weight gradient by ~1e-5, the input gradient locally by a few % -- so dx is compared in L2 (max |err| / max |ref|:
#     9e-3 in C, 4e-2 in D), and even there those pixels dominate.  Hardswish has no kink at 0: case C is 1.4e-6 off everywhere;
#   * the bottom block's few terms per weight-gradient entry (a 30 x 136^2 batch gives each bottom.0 entry 270 products);
#   * a slope gradient is one sum over the whole batch of terms of both signs.  Where it cancels to 1e-4 of the network's
#     largest slope gradient (tconvs3.1 in B / D) fp32 keeps few of its digits: SLOPE_FLOOR caps the relative error asked of such
#     a slope at bar / SLOPE_FLOOR (1.5e-2 for "prelu") of its own value;
#   * MS-SSIM: its gradient changes sign from pixel to pixel, so every whole-batch sum keeps fewer digits (torch fp32 autograd
#     is 2e-3 off on bottom.0.weight and tconvs1.0.weight).
# Gated (test_train_bars_see_deep_gradients): every "smooth" conv class, and the "prelu" top and bottom classes.  Not gated, and
# therefore blind to a 1 % error in the gradient through pool 3 or pool 4 (which moves convs3 / convs4 by 7e-4 / 1.3e-3): the
# "prelu" deep class, and all of case A, whose bars would also pass a 0.2 % error on a single tensor.
SLOPE_FLOOR = 1e-2
TOP = ("convs1", "convs2", "up3", "tconvs3", "up4", "tconvs4")   # the full- and half-resolution levels: k_wgrad's most K slices
BARS = {
    # Hardswish, MSE (case C)
    "smooth": {"y": 2e-6,        # (measured 5.6e-7)
               "loss": 5e-7,     # (1.1e-7: one fp32 ulp of the loss)
               "top": 5e-6,      # (1.3e-6, tconvs3.0.weight)
               "deep": 5e-6,     # (1.4e-6, up2.weight)
               "bottom": 5e-6,   # (below 1.4e-6)
               "dx": 6e-4},      # (2.1e-4; band 2.9e-5)
    # PReLU, MSE (cases B, D; split-K on and off)
    "prelu": {"y": 2e-6,         # (7.0e-7)
              "loss": 5e-7,      # (3.0e-9: only the distance of fl32(loss) from the float64 loss; one fp32 ulp there is 9e-8)
              "top": 5e-5,       # (2.0e-5, tconvs3.2.weight; the gate allows at most 5.3e-5)
              "deep": 3e-4,      # (9.2e-5, up1.weight without split-K)
              "bottom": 4e-4,    # (1.3e-4, bottom.2.weight)
              "slope": 1.5e-4,   # (5.3e-5, tconvs3.1.weight)
              "dx": 3e-3},       # (1.0e-3; band 2.3e-4)
    # PReLU, MS-SSIM (case A)
    "msssim": {"y": 2e-6,        # (6.7e-7)
               "loss": 1.2e-4,   # (4.1e-5 of a loss of 0.093)
               "top": 3e-3,      # (9.9e-4, tconvs4.4.bias)
               "deep": 2e-3,     # (5.5e-4, up1.weight)
               "bottom": 2e-3,   # (7.1e-4, bottom.2.bias)
               "slope": 4e-3},   # (1.2e-3, convs2.3.weight)
}

# (activation, weights seed, crop seed) of each setup; cases A, B and D share theirs
SETUP_STD = ("PReLU", 31, 5)
SETUP_HSW = ("Hardswish", 43, 7)


# ---------------------------------------------------------------------------- the setup

def _f64(sd):
    return {k: v.double() for k, v in sd.items()}


def _crops(n, h, w, seed):
    """Image-like crops: bilinear-upsampled noise plus fine noise, one generator per crop (a batch's first crops do not depend
    on its size)."""
    out = []
    for i in range(n):
        g = torch.Generator().manual_seed(seed * 1000 + i)
        c = F.interpolate(torch.rand(1, 3, h // 8, w // 8, generator=g), size=(h, w), mode="bilinear", align_corners=False)
        out.append((0.8 * c + 0.1 + 0.05 * torch.randn(1, 3, h, w, generator=g)).clip(0, 1))
    return torch.cat(out)


# Kinks of the activations' derivatives: a pre-activation within rounding of one takes the other branch on one side.  Where a
# channel holds fewer than NUDGE_PIXELS pixels over the batch, one such pixel moves the channel's weight gradient by up to
# (1 - slope) / pixels; there the bias of every channel whose float64 pre-activations come within KINK_MARGIN x the layer's std of
# a kink is shifted (by the least amount that clears a gap around it).  The denser layers cannot be cleared (a 30 x 136^2 batch
# puts 5.7e5 pixels in a convs1 channel, 2e-6 std apart near 0) and do not need it: one flip there moves a channel by < 2e-5.
KINKS = {"PReLU": (0.0,), "Hardswish": (-3.0, 3.0)}
KINK_MARGIN = 3e-5
NUDGE_PIXELS = 65536


def _kink_shift(v, kinks, delta, reach):
    """The shift s of least |s| with |v + s - k| >= delta for every value v (1-D) and kink k: k - s at the middle of a gap of
    at least 2 delta between sorted values within `reach` of a kink."""
    def clear(s):
        return all((v + s - k).abs().min().item() >= delta for k in kinks)
    if clear(0.0):
        return 0.0
    w = torch.sort(v).values
    cands = []
    for k in kinks:
        lo, hi = torch.searchsorted(w, torch.tensor([k - reach, k + reach], dtype=w.dtype)).tolist()
        seg = w[max(lo - 1, 0):hi + 1]
        wide = (seg[1:] - seg[:-1]) >= 2.5 * delta
        cands += (k - (seg[1:] + seg[:-1])[wide] / 2).tolist()
    for c in sorted(cands, key=abs):
        if clear(c):
            return c
    raise AssertionError("no gap around the kinks")


def _clear_kinks(sd, x, activation):
    """Shift (in float64, stored as fp32) the biases of the sparse layers' channels whose pre-activations on batch x lie within
    KINK_MARGIN std of a kink; asserts the margin with the fp32 biases."""
    sd64 = _f64(sd)
    worst = {}

    def pre(k, t):
        px = t.shape[0] * t.shape[2] * t.shape[3]
        if px >= NUDGE_PIXELS:
            return t
        bias = k.rsplit(".", 1)[0] + "." + str(int(k.rsplit(".", 1)[1]) - 1) + ".bias"
        std = t.std().item()
        near = torch.stack([(t - kk).abs().amin(dim=(0, 2, 3)) for kk in KINKS[activation]]).amin(0) < KINK_MARGIN * std
        for c in near.nonzero().flatten().tolist():
            s = _kink_shift(t[:, c].reshape(-1), KINKS[activation], KINK_MARGIN * std, 0.25 * std)
            b = sd[bias][c].double()
            nb = torch.tensor((b + s).item(), dtype=torch.float32)
            sd[bias][c] = nb
            t[:, c] += nb.double() - b
        worst[k] = (min((t - kk).abs().min().item() for kk in KINKS[activation]) / std, int(near.sum()))
        assert worst[k][0] >= 0.5 * KINK_MARGIN, (k, worst[k])
        return t

    with torch.no_grad():
        _forward64(sd64, x.double(), activation, pre=pre)
    return worst


def _weights(activation, seed, x):
    """UtNet(64) at VISIBLE_GAIN with the sparse layers' kinks cleared on batch x, and the last 1x1 rescaled (in float64) so
    that the float64 output of its first CAL crops has mean 0.5 and std 0.05; returned as fp32, the values both sides use."""
    from oracle import networks as onet
    sd = synth.make_utnet_state_dict(funit=64, seed=seed, activation=activation, gain=VISIBLE_GAIN)
    _clear_kinks(sd, x, activation)
    with torch.no_grad():
        y = onet.utnet_forward(_f64(sd), x[:CAL].double(), activation=activation)
        k = 0.05 / y.std()
        sd["tconvs4.4.weight"] = (sd["tconvs4.4.weight"].double() * k).float()
        sd["tconvs4.4.bias"] = ((sd["tconvs4.4.bias"].double() - y.mean()) * k + 0.5).float()
    return sd


def _setup(setup, B, h, w):
    """(weights, crops) of a case: the weights depend on the whole batch of B crops (the kink margin)."""
    activation, seed, data_seed = setup
    x = _crops(B, h, w, data_seed)
    return _weights(activation, seed, x), x


def _targets(y64, seed):
    """clip(y64 + 0.02 + 0.03 randn), one generator per crop; asserts that clip(0, 1) is the identity on y64."""
    lo = torch.minimum(y64, 1 - y64).min().item()
    assert lo >= MARGIN, f"a float64 output pixel lies {lo:.3f} from 0 or 1"
    n = [torch.randn(1, *y64.shape[1:], generator=torch.Generator().manual_seed(seed * 1000 + 500 + i), dtype=torch.float64)
         for i in range(y64.shape[0])]
    return (y64 + 0.02 + 0.03 * torch.cat(n)).clip(0, 1).float()


def _criterion(weights, g, t):
    from oracle import losses as olosses
    loss = 0.0
    if weights.get("MSE"):
        loss = loss + weights["MSE"] * F.mse_loss(g, t)
    if weights.get("MSSSIM"):
        loss = loss + weights["MSSSIM"] * (1 - olosses.ms_ssim(g, t)).mean()
    assert set(weights) <= {"MSE", "MSSSIM"}    # smooth criteria only
    return loss


class _ScaleGrad(torch.autograd.Function):
    """Identity forward; the backward multiplies the gradient by a factor."""

    @staticmethod
    def forward(ctx, t, factor):
        ctx.factor = factor
        return t.view_as(t)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.factor, None


GATE_POINTS = ("pool1", "pool2", "pool3", "pool4", "bottom")
# the parameter tensors whose gradients depend on the gradient through each point: the levels above it
_ABOVE = {"pool1": ("convs1",), "pool2": ("convs1", "convs2"), "pool3": ("convs1", "convs2", "convs3"),
          "pool4": ("convs1", "convs2", "convs3", "convs4"), "bottom": ("convs1", "convs2", "convs3", "convs4", "bottom")}


def _forward64(sd, x, activation, gscale=None, pre=None):
    """oracle.networks.utnet_forward restated, with the gradient that flows back through the output of pool 1 ... 4 and of the
    bottom block (the data gradient arriving at each deeper level's input) scaled by gscale[point]; pre(key, t) sees (and may
    replace) every pre-activation before its activation `key`."""
    from oracle import networks as onet
    gscale = gscale or {}

    def pt(name, t):
        return _ScaleGrad.apply(t, gscale[name]) if name in gscale else t

    def act(k, t):
        return onet._act(sd, k, t if pre is None else pre(k, t), activation)

    def enc(n, t):
        t = act(f"{n}.1", F.conv2d(t, sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]))
        return act(f"{n}.3", F.conv2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    def dec(n, t):
        t = act(f"{n}.1", F.conv_transpose2d(t, sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]))
        return act(f"{n}.3", F.conv_transpose2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    def up(n, t):
        return F.conv_transpose2d(t, sd[f"{n}.weight"], sd[f"{n}.bias"], stride=2)

    l1 = enc("convs1", F.pad(x, (2, 2, 2, 2), mode="reflect"))
    l2 = enc("convs2", pt("pool1", F.max_pool2d(l1, 2)))
    l3 = enc("convs3", pt("pool2", F.max_pool2d(l2, 2)))
    l4 = enc("convs4", pt("pool3", F.max_pool2d(l3, 2)))
    b = pt("pool4", F.max_pool2d(l4, 2))
    b = act("bottom.1", F.conv2d(b, sd["bottom.0.weight"], sd["bottom.0.bias"]))
    b = pt("bottom", act("bottom.3", F.conv_transpose2d(b, sd["bottom.2.weight"], sd["bottom.2.bias"])))
    l = torch.cat([up("up1", b), l4], 1)
    l = torch.cat([up("up2", dec("tconvs1", l)), l3], 1)
    l = torch.cat([up("up3", dec("tconvs2", l)), l2], 1)
    l = torch.cat([up("up4", dec("tconvs3", l)), l1], 1)
    l = dec("tconvs4", l)
    return F.conv2d(l, sd["tconvs4.4.weight"], sd["tconvs4.4.bias"])[:, :, 2:-2, 2:-2]


def _reference(sd, x, activation, weights, target_seed, x_grad=False, gscale=None):
    """float64 CPU autograd of the network (oracle.networks.utnet_forward, or _forward64 with gscale) and the criteria on the
    same fp32 weights and crops: (y, targets, loss, {name: grad}, dx or None).  The graph is freed on return."""
    from oracle import networks as onet
    params = {k: v.double().requires_grad_() for k, v in sd.items()}
    x = x.double().requires_grad_(x_grad)
    y = onet.utnet_forward(params, x, activation=activation) if gscale is None else _forward64(params, x, activation, gscale)
    t = _targets(y.detach(), target_seed)
    loss = _criterion(weights, y.clip(0, 1), t.double())
    loss.backward()
    return (y.detach(), t, loss.item(), {k: p.grad for k, p in params.items()}, x.grad if x_grad else None)


def _is_slope(name):
    return name.rsplit(".", 1)[0] in synth.utnet_prelu_keys()


def _band(t):
    """The BAND-pixel border band of [..., H, W] as one flat tensor."""
    return torch.cat([t[..., :BAND, :].reshape(-1), t[..., -BAND:, :].reshape(-1),
                      t[..., BAND:-BAND, :BAND].reshape(-1), t[..., BAND:-BAND, -BAND:].reshape(-1)])


def _rel(got, ref):
    """max |got - ref| / max |ref| (both nonzero, got finite)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    assert got.abs().max().item() > 0 and ref.abs().max().item() > 0
    return (got - ref).abs().max().item() / ref.abs().max().item()


def _l2(got, ref):
    """||got - ref|| / ||ref||"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all() and ref.abs().max().item() > 0
    return ((got - ref).norm() / ref.norm()).item()


def _errors(grads, grads_ref):
    """{name: error} of every parameter gradient: conv weights and biases max |err| / max |ref|, PReLU slopes |err| /
    max(|ref|, SLOPE_FLOOR x the largest slope gradient)."""
    assert set(grads) == set(grads_ref)
    slopes = [n for n in grads_ref if _is_slope(n)]
    floor = SLOPE_FLOOR * max((grads_ref[n].abs().max().item() for n in slopes), default=0.0)
    out = {}
    for n, ref in grads_ref.items():
        e = _rel(grads[n], ref)
        out[n] = e * ref.abs().max().item() / max(ref.abs().max().item(), floor) if n in slopes else e
    return out


# ---------------------------------------------------------------------------- CPU gate

def _gate_change(setup, B, h, w, weights):
    """Change of every parameter gradient (the metrics of _errors) and of dx (L2, whole and border band) when the gradient
    through each GATE_POINTS point is multiplied by 1.01: the weights of the setup's B-crop case, its first CAL crops."""
    from oracle import networks as onet
    sd, x = _setup(setup, B, h, w)
    x = x[:CAL]
    activation = setup[0]
    y, _, _, g0, dx0 = _reference(sd, x, activation, weights, setup[2], x_grad=True, gscale={p: 1.0 for p in GATE_POINTS})
    with torch.no_grad():
        assert torch.equal(y, onet.utnet_forward(_f64(sd), x.double(), activation=activation))   # the restatement is the oracle's network
    out = {}
    for p in GATE_POINTS:
        _, _, _, g, dx = _reference(sd, x, activation, weights, setup[2], x_grad=True, gscale={p: 1.01})
        ch = _errors(g, g0)
        ch["dx"], ch["dx band"] = _l2(dx, dx0), _l2(_band(dx), _band(dx0))
        out[p] = ch
    return out


@pytest.mark.parametrize("setup,B,h,w,bars", [(SETUP_STD, 30, 136, 136, "prelu"), (SETUP_HSW, 8, 136, 184, "smooth")],
                         ids=["B-D-PReLU-136", "C-Hardswish-136x184"])
def test_train_bars_see_deep_gradients(setup, B, h, w, bars):
    """The weights of cases B / D and of case C: a 1 % error in the data gradient arriving at a deeper level's input -- the
    backward of a pool or of the bottom block -- moves every conv gradient of the level directly above it by at least 10x that
    class's bar.  The levels further up see it through the skip connections' sum, diluted ~10x per level.  Not asserted for the
    PReLU deep class (pool 3, pool 4): its bar, set by kink flips, lets such an error through (see BARS)."""
    bars = BARS[bars]
    fig = _gate_change(setup, B, h, w, {"MSE": 1.0})
    for p, ch in fig.items():
        level = _ABOVE[p][-1]
        conv = {n: v for n, v in ch.items() if n.split(".")[0] == level and not _is_slope(n)}
        wc = min(conv, key=conv.get)
        cls = "top" if level in TOP else ("bottom" if level == "bottom" else "deep")
        print(f"{setup[0]} {h}x{w} {p}: {level} {conv[wc]:.2e} ({wc}, bar {bars[cls]:.0e}), dx {ch['dx']:.2e}, "
              f"dx band {ch['dx band']:.2e}")
        if cls != "deep" or setup[0] != "PReLU":
            assert conv[wc] >= 10 * bars[cls], (p, wc, conv[wc])


# ---------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _classes(errs):
    """{class: {name: error}}: conv weights and biases of the TOP levels, of the bottom block and of the other levels; PReLU
    slopes."""
    out = {"top": {}, "deep": {}, "bottom": {}, "slope": {}}
    for n, e in errs.items():
        lv = n.split(".")[0]
        out["slope" if _is_slope(n) else ("top" if lv in TOP else ("bottom" if lv == "bottom" else "deep"))][n] = e
    return {c: d for c, d in out.items() if d}


def _check(what, bars, y, y_ref, loss, loss_ref, grads, grads_ref, dx=None, dx_ref=None):
    """Errors of one run against float64 per quantity class, printed with the worst tensor of each, then asserted."""
    y, y_ref = y.detach().double().cpu(), y_ref.double()
    assert torch.isfinite(y).all(), what
    e_y = (y - y_ref).abs().max().item() / max(1.0, y_ref.abs().max().item())
    e_loss = abs(loss - loss_ref) / abs(loss_ref)
    cls = _classes(_errors(grads, grads_ref))
    msg = f"{what}: y {e_y:.2e}, loss {e_loss:.2e}"
    for c, d in cls.items():
        w = max(d, key=d.get)
        msg += f", {c} {d[w]:.2e} ({w})"
    if dx_ref is not None:
        e_dx, e_band = _l2(dx, dx_ref), _l2(_band(dx.detach().cpu()), _band(dx_ref))
        msg += f", dx {e_dx:.2e} (band {e_band:.2e}; max |err| / max |ref| {_rel(dx, dx_ref):.2e})"
    print(msg)
    assert e_y <= bars["y"] and e_loss <= bars["loss"], (what, e_y, e_loss)
    for c, d in cls.items():
        assert all(e <= bars[c] for e in d.values()), (what, c, {n: e for n, e in d.items() if e > bars[c]})
    if dx_ref is not None:
        assert e_dx <= bars["dx"] and e_band <= bars["dx"], (what, e_dx, e_band)


@pytest.mark.gpu
@pytest.mark.parametrize("case,cs,weights", [("A", 184, {"MSSSIM": 1.0}), ("B", 136, {"MSE": 1.0})], ids=["A-184-MSSSIM", "B-136-MSE"])
def test_fused_step_batch30_vs_float64(dev, case, cs, weights):
    """UtNetTrainer.forward_backward (nd_utnet_train_step_act_hw) on 30 crops: A the reference's UtNet config (184, MS-SSIM),
    B the bench shape (136, MSE)."""
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    B = 30
    sd, x = _setup(SETUP_STD, B, cs, cs)
    y_ref, t, loss_ref, g_ref, _ = _reference(sd, x, "PReLU", weights, SETUP_STD[2])
    net = UtNet(funit=64)
    net.load_state_dict(sd)
    tr = UtNetTrainer(net, device=dev, weights=weights)
    y, loss = tr.forward_backward(x, t)
    torch.cuda.synchronize()
    grads = {n: tr.grad_of(n).cpu() for n in g_ref}
    assert len(grads) == 64
    _check(f"{case}: fused step {B}x{cs}x{cs} {weights}", BARS["msssim" if "MSSSIM" in weights else "prelu"], y, y_ref, loss.item(), loss_ref, grads, g_ref)
    del tr, net
    torch.cuda.empty_cache()


def _autograd_run(dev, sd, activation, x, t, split_k=True):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=64, activation=activation)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    net.split_k = split_k
    xd = x.to(dev).requires_grad_()
    out = net(xd)
    loss = F.mse_loss(out.clip(0, 1), t.to(dev))
    loss.backward()
    torch.cuda.synchronize()
    res = (out.detach().cpu(), loss.item(), {n: p.grad.cpu() for n, p in net.named_parameters()}, xd.grad.cpu())
    del net, out, xd
    torch.cuda.empty_cache()
    return res


@pytest.mark.gpu
def test_autograd_hardswish_rectangular_vs_float64(dev):
    """C: loss.backward() through UtNet(64, Hardswish) on 8 crops of 136 x 184: parameter gradients and the input gradient."""
    B, h, w = 8, 136, 184
    sd, x = _setup(SETUP_HSW, B, h, w)
    y_ref, t, loss_ref, g_ref, dx_ref = _reference(sd, x, "Hardswish", {"MSE": 1.0}, SETUP_HSW[2], x_grad=True)
    y, loss, grads, dx = _autograd_run(dev, sd, "Hardswish", x, t)
    _check(f"C: autograd Hardswish {B}x{h}x{w} MSE", BARS["smooth"], y, y_ref, loss, loss_ref, grads, g_ref, dx, dx_ref)


@pytest.mark.gpu
def test_autograd_batch30_split_k_on_and_off_vs_float64(dev):
    """D: loss.backward() through UtNet(64, PReLU) on 30 crops of 136, with the split-K tail (ND_FLAG_NO_SPLITK off) and
    without it, both against float64."""
    B, cs = 30, 136
    sd, x = _setup(SETUP_STD, B, cs, cs)
    y_ref, t, loss_ref, g_ref, dx_ref = _reference(sd, x, "PReLU", {"MSE": 1.0}, SETUP_STD[2], x_grad=True)
    for split_k in (True, False):
        y, loss, grads, dx = _autograd_run(dev, sd, "PReLU", x, t, split_k)
        _check(f"D: autograd PReLU {B}x{cs}x{cs} MSE split_k={split_k}", BARS["prelu"], y, y_ref, loss, loss_ref, grads, g_ref, dx, dx_ref)
