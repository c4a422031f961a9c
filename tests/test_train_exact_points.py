"""UtNet training gradients at the points where a convention, not rounding, decides the result.

test_train_float64.py keeps away from them on purpose (no output pixel near 0 or 1, no sparse pre-activation near a kink, no L1)
and random data never lands on them, so four choices of csrc/utnet_train.hip are seen by no other test:
  1. which element of a tied 2x2 window gets the pool gradient (k_maxpool_bwd_add: the first in row-major order, as torch);
  2. the derivative of each activation at its break points (k_act_bwd: PReLU'(0) = slope, ELU'(0) = 1, Hardswish'(-3) = 0,
     Hardswish'(+3) = 1);
  3. whether clip(0, 1) passes the gradient at exactly 0 and 1 (k_loss_grad, k_add_clip_grad: it does);
  4. sign(0) = 0 of the L1 term (k_loss_grad).
Training reaches them: blown highlights and blacks are exactly 1.0 and 0.0, a constant region stays bit-identical through
ReflectionPad2d and the encoder's convolutions, and every pool window inside it is an exact tie.

The setups make the arithmetic exact on both sides, so that the convention alone decides and a bar near fp32's own error sees
a wrong one:
  A  zero state: UtNet(8), two 104 x 104 crops, x = 0, every conv bias 0 but tconvs4.4.bias.  Every pre-activation is exactly
     0 in every kernel form (Winograd transforms of zeros are zeros), every pool window a tie, y exactly its bias per channel:
     0, 1 and 0.5.  Every conv-weight and PReLU-slope gradient is exactly 0 (each is a sum of products with a zero activation
     or pre-activation; a launch that read stale workspace would not give 0 -- every GPU run first takes a step on random
     crops through the same workspace); the 23 bias gradients and dx are not.
  B  Hardswish break points: A with y = 0.5 + the last layer's products, and the biases of tconvs4.2 planted on +3 / -3 / 0:
     the pre-activations of the last activation layer are exactly those.  Only this layer can be planted: everything
     upstream stays zero, so nothing nonzero reaches a pool or a Winograd transform.
  C  saturated frames: UtNet(16, PReLU), 120 x 120, one frame all 1.0 and one whose right half is 1.0, last 1x1 calibrated as
     test_train_float64._weights does (y stays MARGIN from 0 and 1).  Pool ties over whole regions at ordinary values.  The
     reference computes the encoder's convolutions tap by tap (_conv_by_taps): torch's float64 CPU convolution is not
     position-independent on every machine, and the ties have to survive the reference first.  The noise is chosen so that no
     window of it is a near-tie that rounding would decide (NOISE_SEED_C).  Parameter
     gradients do not depend on the tie rule there (4e-6); dx does (0.5 ... 0.7 in L2), and rounding-sized noise on the
     pre-activations moves it as much.  So dx is asserted under winograd=False, split_k=False only, where every output pixel's K
     loop is the same whatever its position (test_roi.py) and ties survive; under the default flags the fused 1-D Winograd
     forward's sums depend on the position in the tile, ties break by rounding, and dx is printed (DESIGN.md records it).

Metrics of test_train_float64: max |err| / max |ref| per parameter tensor, L2 for dx (per frame, the worst).  Each bar is 10x
the error of torch's own fp32 CPU autograd against float64 on that case (test_torch_fp32_within_a_tenth_of_the_bars asserts
it): 10 is the upper end of the 3 ... 10x that this suite records for MFMA's sequential fma chains over torch's fp32.  The CPU
gate test_wrong_convention_moves_an_asserted_quantity shows that each wrong convention moves an asserted quantity by at least
10x its bar."""
import functools
import importlib.util
import os

import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth


def _train_float64_tests():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_train_float64.py")
    spec = importlib.util.spec_from_file_location("_train_float64_bars", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_T = _train_float64_tests()
VISIBLE_GAIN, MARGIN, _rel, _l2 = _T.VISIBLE_GAIN, _T.MARGIN, _T._rel, _T._l2

Y_PLANTED = (0.0, 1.0, 0.5)    # setup A: tconvs4.4.bias, and therefore y, per channel
SEED_A, SEED_C = 9, 9          # synth weights; C: UtNet(16, gain 2.2, seed 9)
# The noise of setup C's second frame.  Its windows are no ties, and where the two largest values of one lie closer than fp32
# rounds the encoder, rounding and not the convention picks the pixel that gets the gradient: with seed 79 one pool-3 window of
# 9216 had a gap of 5e-8 of the layer's std, 0.4x torch fp32's own error on its two values; three of eight fp32 summation orders
# of the encoder on the CPU and the MI355X under the direct flags took the other pixel, which moved dx of that frame by 5.03e-5
# in L2 and convs3.1.weight by 2.2e-5.  NEAR_TIE_FACTOR (test_oracle_preconditions): every pool window of the float64 reference
# is an exact tie or has a gap of at least 10x torch fp32's error on its two largest values -- the factor of the bars.  110 is
# the first seed from 79 on that meets it (one in ~25 does; the encoder by taps gives the same bits on every machine).
NOISE_SEED_C = 110
NEAR_TIE_FACTOR = 10

# name: (setup, activation, criteria, loss_cs, path) -- path "fused": UtNetTrainer.forward_backward (the criteria and clip(0, 1)
# in k_loss_grad / k_add_clip_grad); "module": loss.backward() through the module (torch's criteria on its output), with dx
CASES = {
    "A-fused-L1+MSE": ("A", "PReLU", {"L1": 1.0, "MSE": 1.0}, None, "fused"),
    "A-fused-MSE+SSIM": ("A", "PReLU", {"MSE": 1.0, "SSIM": 1.0}, None, "fused"),
    "A-fused-L1+MSE-cs88": ("A", "PReLU", {"L1": 1.0, "MSE": 1.0}, 88, "fused"),
    "A-PReLU": ("A", "PReLU", {"MSE": 1.0}, None, "module"),
    "A-ELU": ("A", "ELU", {"MSE": 1.0}, None, "module"),
    "A-Hardswish": ("A", "Hardswish", {"MSE": 1.0}, None, "module"),
    "B-Hardswish": ("B", "Hardswish", {"MSE": 1.0}, None, "module"),
    "C-PReLU": ("C", "PReLU", {"MSE": 1.0}, None, "module"),
}
FLAGS = {"default": False, "direct": True}    # direct: winograd=False, split_k=False

# y: max |err| / max(1, max |ref|), and loss: |err| / |ref|, where they are not exact: the bars of test_train_float64 (a few
# fp32 ulps of an O(1) value; torch's fp32 meets them as they stand).  The SSIM term is a mean of quotients of filtered sums.
Y_BAR = 2e-6
LOSS_BAR = 5e-7
# Gradient bars: 10x torch fp32 CPU autograd's error against float64 (first figure in the comment; the worst tensor), then the
# worst MI355X figure over both flag settings.  Each bar is 10x the fp32 figure plus 10 %, rounded up to the next of 1, 1.5, 2, 2.5,
# 3, 4, 5, 6, 8 x 10^k (1.1 ... 1.3x above 10x the figure), so that the bar / 10 gate does not sit on the last digit of a sum
# whose order the CPU library picks.  "dx" of C holds under the direct flags only.
BARS = {
    "A-fused-L1+MSE": {"param": 4e-5},                  # torch fp32 3.5e-6 (up4.bias); MI355X 1.5e-6 (bottom.0.bias)
    "A-fused-MSE+SSIM": {"param": 3e-5},                # 2.3e-6 (tconvs4.0.bias); MI355X 2.6e-6 (convs3.0.bias)
    "A-fused-L1+MSE-cs88": {"param": 6e-5},             # 4.6e-6 (tconvs4.0.bias); MI355X 1.6e-6
    "A-PReLU": {"param": 5e-5, "dx": 6e-6},             # 4.2e-6 (tconvs4.0.bias), dx 4.6e-7; MI355X 1.2e-6, dx 6.5e-7
    "A-ELU": {"param": 4e-5, "dx": 8e-6},               # 3.1e-6 (up4.bias), dx 6.5e-7; MI355X 1.5e-6, dx 1.0e-6
    "A-Hardswish": {"param": 4e-5, "dx": 6e-6},         # 3.1e-6 (up4.bias), dx 4.6e-7; MI355X 1.5e-6, dx 6.4e-7
    "B-Hardswish": {"param": 3e-5, "dx": 4e-6},         # 2.3e-6 (tconvs4.2.bias), dx 3.2e-7; MI355X 1.3e-6, dx 6.4e-7 (the old rule: 1.3, dx 0.57)
    # 3.1e-6 (up4.bias), dx 1.9e-6; MI355X direct flags 2.5e-6 (convs3.1.weight), dx 2.0e-6 on either frame; default flags 3.7e-6
    # (bottom.1.weight), dx 0.174 / 0.121 (printed, not asserted)
    "C-PReLU": {"param": 4e-5, "dx": 2.5e-5},
}


# ---------------------------------------------------------------------------- wrong conventions (float64, the CPU gates)

class _Pool(torch.autograd.Function):
    """max_pool2d(t, 2) whose gradient goes to the first or to the last maximum of each window in row-major order."""

    @staticmethod
    def forward(ctx, t, last):
        B, C, H, W = t.shape
        w = t.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
        m = w.amax(-1)
        rank = torch.arange(1, 5) if last else torch.arange(4, 0, -1)    # distinct ranks: one largest among the maxima
        ctx.idx = ((w == m[..., None]) * rank).argmax(-1)
        return m

    @staticmethod
    def backward(ctx, g):
        B, C, h, w = g.shape
        gw = torch.zeros(B, C, h, w, 4, dtype=g.dtype).scatter_(-1, ctx.idx[..., None], g[..., None])
        return gw.reshape(B, C, h, w, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * h, 2 * w), None


class _PReLUOne(torch.autograd.Function):
    """PReLU with derivative 1 at 0."""

    @staticmethod
    def forward(ctx, t, a):
        ctx.save_for_backward(t, a)
        return torch.where(t > 0, t, a * t)

    @staticmethod
    def backward(ctx, g):
        t, a = ctx.saved_tensors
        return g * torch.where(t >= 0, torch.ones_like(t), a.expand_as(t)), (g * torch.where(t < 0, t, torch.zeros_like(t))).sum().reshape(1)


class _HardswishOld(torch.autograd.Function):
    """Hardswish with the middle branch x / 3 + 1 / 2 on the closed interval: -1/2 at -3 and 3/2 at +3."""

    @staticmethod
    def forward(ctx, t):
        ctx.save_for_backward(t)
        return F.hardswish(t)

    @staticmethod
    def backward(ctx, g):
        t, = ctx.saved_tensors
        return torch.where(t < -3, torch.zeros_like(g), torch.where(t <= 3, g * (t / 3 + 0.5), g))


class _StrictClip(torch.autograd.Function):
    """clip(0, 1) that passes the gradient on the open interval only."""

    @staticmethod
    def forward(ctx, t):
        ctx.save_for_backward(t)
        return t.clip(0, 1)

    @staticmethod
    def backward(ctx, g):
        t, = ctx.saved_tensors
        return g * ((t > 0) & (t < 1))


class _AbsPlus(torch.autograd.Function):
    """|d| with sign(0) = +1."""

    @staticmethod
    def forward(ctx, d):
        ctx.save_for_backward(d)
        return d.abs()

    @staticmethod
    def backward(ctx, g):
        d, = ctx.saved_tensors
        return g * torch.where(d >= 0, torch.ones_like(d), -torch.ones_like(d))


def _conv_by_taps(t, w, b):
    """F.conv2d(t, w, b) of a 3x3 kernel as bias + the sum over (input channel, tap) of elementwise products, in that order.
    Every step is one correctly rounded multiplication or addition per element, so every output pixel goes through the same
    sequence whatever its position, thread or vector lane: equal windows give equal bits.  torch's own CPU convolution does
    not promise that -- its float64 form runs through a threaded GEMM, and on one machine 6 % of the pool-4 windows of the
    constant frame of setup C were no ties in float64, which moved the reference's own dx by 1.8e-3."""
    H, W = t.shape[-2] - 2, t.shape[-1] - 2
    out = b.view(1, -1, 1, 1)
    for c in range(w.shape[1]):
        for ky in range(3):
            for kx in range(3):
                out = out + w[:, c, ky, kx].view(1, -1, 1, 1) * t[:, c:c + 1, ky:ky + H, kx:kx + W]
    return out


def _forward(sd, x, activation, conv=(), taps=None):
    """oracle.networks.utnet_forward restated, with the conventions named in `conv` replaced ("ties_last" / "ties_first",
    "prelu_one", "hardswish_old"); "by_taps": the encoder's convolutions -- the layers whose outputs are pooled -- through
    _conv_by_taps.  taps receives every pool's input and every pre-activation."""
    from oracle import networks as onet

    def act(k, t):
        if taps is not None:
            taps["pre " + k] = t
        if activation == "PReLU" and "prelu_one" in conv:
            return _PReLUOne.apply(t, sd[k + ".weight"])
        if activation == "Hardswish" and "hardswish_old" in conv:
            return _HardswishOld.apply(t)
        return onet._act(sd, k, t, activation)

    def pool(n, t):
        if taps is not None:
            taps[n] = t
        if "ties_last" in conv or "ties_first" in conv:
            return _Pool.apply(t, "ties_last" in conv)
        return F.max_pool2d(t, 2)

    conv2d = _conv_by_taps if "by_taps" in conv else F.conv2d

    def enc(n, t):
        t = act(f"{n}.1", conv2d(t, sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]))
        return act(f"{n}.3", conv2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    def dec(n, t):
        t = act(f"{n}.1", F.conv_transpose2d(t, sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]))
        return act(f"{n}.3", F.conv_transpose2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    def up(n, t):
        return F.conv_transpose2d(t, sd[f"{n}.weight"], sd[f"{n}.bias"], stride=2)

    l1 = enc("convs1", F.pad(x, (2, 2, 2, 2), mode="reflect"))
    l2 = enc("convs2", pool("pool1", l1))
    l3 = enc("convs3", pool("pool2", l2))
    l4 = enc("convs4", pool("pool3", l3))
    b = pool("pool4", l4)
    b = act("bottom.1", F.conv2d(b, sd["bottom.0.weight"], sd["bottom.0.bias"]))
    b = act("bottom.3", F.conv_transpose2d(b, sd["bottom.2.weight"], sd["bottom.2.bias"]))
    l = torch.cat([up("up1", b), l4], 1)
    l = torch.cat([up("up2", dec("tconvs1", l)), l3], 1)
    l = torch.cat([up("up3", dec("tconvs2", l)), l2], 1)
    l = torch.cat([up("up4", dec("tconvs3", l)), l1], 1)
    l = dec("tconvs4", l)
    return F.conv2d(l, sd["tconvs4.4.weight"], sd["tconvs4.4.bias"])[:, :, 2:-2, 2:-2]


def _center(t, cs):
    """pt_ops.pt_crop_batch: the centre cs x cs crop (the whole tensor without cs)."""
    if not cs:
        return t
    oy, ox = (t.shape[-2] - cs) // 2, (t.shape[-1] - cs) // 2
    return t[..., oy:oy + cs, ox:ox + cs]


def _criterion(weights, y, t, loss_cs=None, conv=()):
    """sum_k weight_k criterion_k(crop(clip(y, 0, 1)), crop(t)), as the reference's training loop states it; the conventions
    "strict_clip", "strict_clip_ssim" (the SSIM term's input only: k_add_clip_grad by itself) and "sign_plus" replaced on request."""
    from oracle import losses as olosses
    assert set(weights) <= {"L1", "MSE", "SSIM"}
    g = _center(_StrictClip.apply(y) if "strict_clip" in conv else y.clip(0, 1), loss_cs)
    t = _center(t, loss_cs)
    loss = 0.0
    if weights.get("L1"):
        loss = loss + weights["L1"] * (_AbsPlus.apply(g - t) if "sign_plus" in conv else (g - t).abs()).mean()
    if weights.get("MSE"):
        loss = loss + weights["MSE"] * F.mse_loss(g, t)
    if weights.get("SSIM"):
        gs = _center(_StrictClip.apply(y), loss_cs) if "strict_clip_ssim" in conv else g
        loss = loss + weights["SSIM"] * (1 - olosses.ssim(gs, t)).mean()
    return loss


# ---------------------------------------------------------------------------- the setups

def _zero_state(activation, final_bias):
    sd = synth.make_utnet_state_dict(funit=8, seed=SEED_A, activation=activation, gain=VISIBLE_GAIN)
    for k in sd:
        if k.endswith(".bias"):
            sd[k] = torch.zeros_like(sd[k])
    sd["tconvs4.4.bias"] = torch.tensor(final_bias, dtype=torch.float32)
    return sd, torch.zeros(2, 3, 104, 104)


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def _case(name):
    """The fp32 weights, crops and targets of a case (both sides start from them), the names of the gradients that are
    exactly zero, and float64 autograd on them.  Computed once, shared, never written to."""
    from oracle import networks as onet
    setup, activation, weights, loss_cs, path = CASES[name]
    if setup == "A":
        sd, x = _zero_state(activation, Y_PLANTED)
        t = _rand(x.shape, 77)
        if weights.get("L1"):
            t[:, 2] = 0.5                       # g - t is exactly 0 on channel 2: sign(0)
        zeros = {k for k in sd if not k.endswith(".bias")}
    elif setup == "B":
        sd, x = _zero_state(activation, (0.5, 0.5, 0.5))
        b = torch.zeros(8)
        b[0::3], b[1::3] = 3.0, -3.0
        sd["tconvs4.2.bias"] = b
        h = F.hardswish(b.double())                               # the last activation layer's output, per channel
        w = sd["tconvs4.4.weight"].double()
        k = 0.0999 / (w.reshape(3, 8) @ h).abs().max()            # |y - 0.5| <= 0.1 after the fp32 rounding of the weights
        sd["tconvs4.4.weight"] = (w * k).float()
        t = _rand(x.shape, 78)
        zeros = {k for k in sd if k.endswith(".weight") and k != "tconvs4.4.weight"}
    else:
        sd = synth.make_utnet_state_dict(funit=16, seed=SEED_C, activation=activation, gain=VISIBLE_GAIN)
        x = torch.ones(2, 3, 120, 120)
        x[1, :, :, :60] = _rand((3, 120, 60), NOISE_SEED_C)       # frame 0: all 1.0; frame 1: right half 1.0, left half noise
        with torch.no_grad():                                     # test_train_float64._weights: mean 0.5, std 0.05, in float64
            y = onet.utnet_forward(_T._f64(sd), x.double(), activation=activation)
            k = 0.05 / y.std()
            sd["tconvs4.4.weight"] = (sd["tconvs4.4.weight"].double() * k).float()
            sd["tconvs4.4.bias"] = ((sd["tconvs4.4.bias"].double() - y.mean()) * k + 0.5).float()
            y = onet.utnet_forward(_T._f64(sd), x.double(), activation=activation)
        t = _T._targets(y, 80)                                    # asserts MARGIN; clip(y64 + 0.02 + 0.03 randn)
        zeros = set()
    c = {"name": name, "setup": setup, "activation": activation, "weights": weights, "loss_cs": loss_cs, "path": path,
         "funit": 16 if setup == "C" else 8, "sd": sd, "x": x, "t": t, "zeros": zeros}
    c["ref"] = _autograd_cpu(c)
    return c


def _autograd_cpu(c, dtype=torch.float64, conv=(), taps=None):
    """torch CPU autograd of the network and the criteria in `dtype`: {"y", "loss", "grads", "dx"}."""
    params = {k: v.to(dtype, copy=True).requires_grad_() for k, v in c["sd"].items()}
    x = c["x"].to(dtype, copy=True).requires_grad_()
    if c["setup"] == "C":      # ties over regions at ordinary values: they have to survive the reference's own convolutions
        conv = tuple(conv) + ("by_taps",)
    y = _forward(params, x, c["activation"], conv, taps)
    loss = _criterion(c["weights"], y, c["t"].to(dtype), c["loss_cs"], conv)
    loss.backward()
    return {"y": y.detach(), "loss": loss.item(), "grads": {k: p.grad for k, p in params.items()}, "dx": x.grad}


def _tie_share(t):
    """Share of the 2x2 windows of [B, C, H, W] whose maximum is taken more than once, per frame."""
    B, C, H, W = t.shape
    w = t.detach().reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    return ((w == w.amax(-1, keepdim=True)).sum(-1) >= 2).double().mean(dim=(1, 2, 3)).tolist()


def _near_tie_ratio(t64, t32):
    """Over the 2x2 windows of a pool input that are no exact ties in float64: the smallest gap between the two largest
    values / the sum of the fp32 forward's errors on those two values."""
    def windows(t):
        B, C, H, W = t.shape
        return t.detach().reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    s, i = windows(t64).sort(-1, descending=True)
    gap = s[..., 0] - s[..., 1]
    err = windows((t32.double() - t64).abs()).gather(-1, i[..., :2]).sum(-1)
    return (gap / err.clamp_min(1e-300))[gap > 0].min().item() if (gap > 0).any() else float("inf")


def _dx_err(got, ref):
    """L2 distance of dx per frame, the worst."""
    return max(_l2(got[i], ref[i]) for i in range(ref.shape[0]))


def _errors(c, got, what, dx=True):
    """Errors of one run against the case's float64 autograd: {"y", "loss", "param", "dx"}.  Asserts what is exact: y of
    setup A and the zero gradients, on both sides."""
    ref = c["ref"]
    y = got["y"].detach().double().cpu()
    assert torch.isfinite(y).all(), what
    if c["setup"] == "A":
        planted = torch.tensor(Y_PLANTED, dtype=torch.float64).view(1, 3, 1, 1).expand_as(y)
        assert torch.equal(y, planted) and torch.equal(ref["y"], planted), what
    out = {"y": (y - ref["y"]).abs().max().item() / max(1.0, ref["y"].abs().max().item()),
           "loss": abs(got["loss"] - ref["loss"]) / abs(ref["loss"])}
    assert set(got["grads"]) == set(ref["grads"])
    per = {}
    for n, r in ref["grads"].items():
        g = got["grads"][n].detach().cpu()
        if n in c["zeros"]:
            assert torch.count_nonzero(r) == 0, (what, n)
            assert torch.isfinite(g).all() and torch.count_nonzero(g) == 0, (what, n, g.abs().max().item())
        else:
            per[n] = _rel(g, r)
    worst = max(per, key=per.get)
    out["param"], out["worst"] = per[worst], worst
    if dx and c["path"] == "module":
        out["dx"] = _dx_err(got["dx"], ref["dx"])
    return out


def _report(what, e):
    print(f"{what}: y {e['y']:.2e}, loss {e['loss']:.2e}, param {e['param']:.2e} ({e['worst']})"
          + (f", dx {e['dx']:.2e}" if "dx" in e else ""))


# ---------------------------------------------------------------------------- CPU gates

@pytest.mark.parametrize("name", list(CASES))
def test_oracle_preconditions(name):
    """The float64 and the fp32 reference are in the state the setup claims: the restated network is the oracle's, y has the
    planted values, the pre-activations sit exactly on the break points, the tie shares hold, the expected zeros are exact."""
    from oracle import networks as onet
    c = _case(name)
    seen = {}
    for dtype in (torch.float64, torch.float32):
        taps = seen[dtype] = {}
        r = _autograd_cpu(c, dtype, taps=taps)
        with torch.no_grad():
            sd = {k: v.to(dtype) for k, v in c["sd"].items()}
            y = onet.utnet_forward(sd, c["x"].to(dtype), activation=c["activation"])
            if c["setup"] == "C":      # the encoder by taps: the oracle's network up to the order of its sums
                assert (r["y"] - y).abs().max().item() <= (1e-12 if dtype == torch.float64 else 2e-6)
            else:
                assert torch.equal(r["y"], y)
        _errors(c, r, f"{name} {dtype}")      # asserts y of setup A and the exact zeros
        assert len([n for n in r["grads"] if n.endswith(".bias")]) == 23
        assert all(r["grads"][n].abs().max().item() > 0 for n in r["grads"] if n not in c["zeros"])
        assert r["dx"].abs().max().item() > 0
        pools = {p: _tie_share(taps[p]) for p in ("pool1", "pool2", "pool3", "pool4")}
        pre = {k[4:]: v.detach() for k, v in taps.items() if k.startswith("pre ")}
        if c["setup"] in "AB":
            assert all(s == 1.0 for p in pools.values() for s in p), pools
            planted = c["sd"]["tconvs4.2.bias"].to(dtype)
            for k, v in pre.items():
                if c["setup"] == "B" and k == "tconvs4.3":
                    assert torch.equal(v, planted.view(1, -1, 1, 1).expand_as(v))
                    assert sorted(set(planted.tolist())) == [-3.0, 0.0, 3.0]
                else:
                    assert torch.count_nonzero(v) == 0, k
        if c["setup"] == "B":
            assert (r["y"] - 0.5).abs().max().item() <= 0.1 and (r["y"] - 0.5).abs().max().item() >= 0.09
        if c["setup"] == "C":
            print(f"{name} {dtype}: tie shares per frame " + ", ".join(f"{p} {s[0]:.2f} / {s[1]:.2f}" for p, s in pools.items()))
            assert all(s[0] == 1.0 for s in pools.values()), pools                          # the constant frame
            assert all(pools[p][1] >= 0.30 for p in ("pool1", "pool2", "pool3")), pools     # right half 1.0
            assert torch.minimum(r["y"], 1 - r["y"]).min().item() >= MARGIN
            if dtype == torch.float32:
                near = {p: _near_tie_ratio(seen[torch.float64][p], taps[p]) for p in pools}
                print(f"{name}: smallest pool gap / torch fp32's error on its two values: " + ", ".join(f"{p} {v:.1f}" for p, v in near.items()))
                assert all(v >= NEAR_TIE_FACTOR for v in near.values()), near
        if c["loss_cs"]:
            yy = r["y"].clone().requires_grad_()
            gy = torch.autograd.grad(_criterion(c["weights"], yy, c["t"].to(dtype), c["loss_cs"]), yy)[0]
            inside = torch.zeros_like(gy, dtype=torch.bool)
            _center(inside, c["loss_cs"])[...] = True
            assert torch.count_nonzero(gy[~inside]) == 0 and torch.count_nonzero(gy[inside]) > 0


def test_torch_breakpoint_conventions():
    """What torch itself returns at the points: the conventions the kernels restate."""
    x = torch.tensor([-3.0, 3.0, 0.0], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.grad(F.hardswish(x).sum(), x)[0].tolist() == [0.0, 1.0, 0.5]
    assert torch.autograd.grad(F.elu(x).sum(), x)[0][2].item() == 1.0
    assert torch.autograd.grad(F.prelu(x, torch.tensor([0.25], dtype=torch.float64)).sum(), x)[0][2].item() == 0.25
    c = torch.tensor([0.0, 1.0], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.grad(c.clip(0, 1).sum(), c)[0].tolist() == [1.0, 1.0]
    assert torch.autograd.grad(c.abs().sum(), c)[0][0].item() == 0.0
    w = torch.zeros(1, 1, 2, 2, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.grad(F.max_pool2d(w, 2).sum(), w)[0].flatten().tolist() == [1.0, 0.0, 0.0, 0.0]


# (wrong convention, case, the asserted quantities it must move)
GATES = [("ties_last", "A-PReLU", ("dx",)), ("ties_last", "A-ELU", ("dx",)), ("ties_last", "A-Hardswish", ("dx",)),
         ("ties_last", "C-PReLU", ("dx",)),
         ("prelu_one", "A-PReLU", ("param", "dx")), ("prelu_one", "A-fused-L1+MSE", ("param",)),
         ("strict_clip", "A-fused-L1+MSE", ("param",)), ("strict_clip", "A-fused-MSE+SSIM", ("param",)),
         ("strict_clip", "A-fused-L1+MSE-cs88", ("param",)), ("strict_clip_ssim", "A-fused-MSE+SSIM", ("param",)),
         ("sign_plus", "A-fused-L1+MSE", ("param",)), ("sign_plus", "A-fused-L1+MSE-cs88", ("param",)),
         ("hardswish_old", "B-Hardswish", ("param", "dx"))]


@pytest.mark.parametrize("conv,name,moved", GATES, ids=[f"{g[0]}-{g[1]}" for g in GATES])
def test_wrong_convention_moves_an_asserted_quantity(conv, name, moved):
    """Each wrong convention, applied in float64, moves an asserted quantity of the case by at least 10x its bar (the worst
    parameter tensor, dx of the worst frame).  The pool restatement with ties to the first element is torch's, bit for bit."""
    c = _case(name)
    ref = c["ref"]
    if conv == "ties_last":
        first = _autograd_cpu(c, conv=("ties_first",))
        assert torch.equal(first["dx"], ref["dx"]) and all(torch.equal(first["grads"][n], ref["grads"][n]) for n in ref["grads"])
    wrong = _autograd_cpu(c, conv=(conv,))
    ch = {"param": max((wrong["grads"][n] - r).abs().max().item() / r.abs().max().item()
                       for n, r in ref["grads"].items() if n not in c["zeros"]),
          "dx": _dx_err(wrong["dx"], ref["dx"])}
    print(f"{conv} on {name}: " + ", ".join(f"{q} moved {ch[q]:.2e} (bar {BARS[name][q]:.1e})" for q in moved))
    for q in moved:
        assert ch[q] >= 10 * BARS[name][q], (conv, name, q, ch[q])


@pytest.mark.parametrize("name", list(CASES))
def test_torch_fp32_within_a_tenth_of_the_bars(name):
    """torch's fp32 CPU autograd stays within bar / 10 of float64 on every case: the reference alone meets the condition, and
    this is where the bars come from."""
    c = _case(name)
    e = _errors(c, _autograd_cpu(c, torch.float32), f"{name} torch fp32")
    _report(f"{name} torch fp32 (CPU)", e)
    assert e["y"] <= Y_BAR and e["loss"] <= LOSS_BAR, (name, e["y"], e["loss"])
    for q, bar in BARS[name].items():
        assert e[q] <= bar / 10, (name, q, e[q], bar)


# ---------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _net(c, direct):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=c["funit"], activation=c["activation"])
    net.load_state_dict(c["sd"])
    net.winograd = net.split_k = not direct
    return net


def _fused_run(dev, c, direct, t=None):
    """UtNetTrainer.forward_backward on the case, after one step on random crops through the same workspace."""
    from nind_denoise_amd.train import UtNetTrainer
    tr = UtNetTrainer(_net(c, direct), device=dev, weights=c["weights"])
    tr.forward_backward(_rand(c["x"].shape, 1), _rand(c["x"].shape, 2))
    tr.loss_cs = c["loss_cs"]
    runs = []
    for tt in (c["t"],) if t is None else (c["t"], t):
        y, loss = tr.forward_backward(c["x"], tt)
        torch.cuda.synchronize()
        runs.append({"y": y.cpu(), "loss": loss.item(), "grads": {n: tr.grad_of(n).cpu().clone() for n in c["ref"]["grads"]}})
    del tr
    torch.cuda.empty_cache()
    return runs


def _module_run(dev, c, direct):
    """loss.backward() through the module on the case, after one forward / backward on random crops through the same
    workspace."""
    net = _net(c, direct).to(dev).train()
    xp = _rand(c["x"].shape, 1).to(dev).requires_grad_()
    _criterion(c["weights"], net(xp), _rand(c["x"].shape, 2).to(dev)).backward()
    net.zero_grad()
    xd = c["x"].to(dev).requires_grad_()
    y = net(xd)
    loss = _criterion(c["weights"], y, c["t"].to(dev), c["loss_cs"])
    loss.backward()
    torch.cuda.synchronize()
    res = {"y": y.detach().cpu(), "loss": loss.item(), "grads": {n: p.grad.cpu() for n, p in net.named_parameters()}, "dx": xd.grad.cpu()}
    del net, y, xd, xp
    torch.cuda.empty_cache()
    return res


def _assert_bars(name, what, e, skip=()):
    assert e["y"] <= Y_BAR and e["loss"] <= LOSS_BAR, (what, e["y"], e["loss"])
    for q, bar in BARS[name].items():
        if q not in skip:
            assert e[q] <= bar, (what, q, e[q], bar)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][4] == "fused"])
def test_fused_step_zero_state_vs_float64(dev, name, flags):
    """Setup A through UtNetTrainer.forward_backward: y exact, every weight and slope gradient exactly 0, the bias gradients
    against float64 -- clip(0, 1) at y = 0 and 1 (k_loss_grad; k_add_clip_grad under SSIM) and sign(0) of L1 on channel 2.
    With loss_cs the gradient is exactly 0 outside the centre crop: targets that differ only there change no bit."""
    c = _case(name)
    t2 = None
    if c["loss_cs"]:
        t2 = 1 - c["t"]
        _center(t2, c["loss_cs"])[...] = _center(c["t"], c["loss_cs"])
    runs = _fused_run(dev, c, FLAGS[flags], t2)
    e = _errors(c, runs[0], f"{name} {flags}")
    _report(f"{name} {flags}", e)
    _assert_bars(name, f"{name} {flags}", e)
    if t2 is not None:
        assert runs[1]["loss"] == runs[0]["loss"]
        assert all(torch.equal(runs[1]["grads"][n], g) for n, g in runs[0]["grads"].items())


@pytest.mark.gpu
@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][4] == "module" and CASES[n][0] == "A"])
def test_autograd_zero_state_vs_float64(dev, name, flags):
    """Setup A through loss.backward() on the module, PReLU / ELU / Hardswish: every pool window a tie, every pre-activation
    on 0; the exact zeros, the bias gradients and dx against float64."""
    c = _case(name)
    e = _errors(c, _module_run(dev, c, FLAGS[flags]), f"{name} {flags}")
    _report(f"{name} {flags}", e)
    _assert_bars(name, f"{name} {flags}", e)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", list(FLAGS))
def test_autograd_hardswish_break_points_vs_float64(dev, flags):
    """Setup B: the pre-activations of the last activation layer exactly on +3, -3 and 0.  k_act_bwd<HARDSWISH> took the middle
    branch on the closed interval (-g / 2 at -3, 3 g / 2 at +3): 1.3 off on tconvs2.2.bias and 0.57 on dx
    (measured on MI355X with that rule, and by the CPU gate)."""
    c = _case("B-Hardswish")
    e = _errors(c, _module_run(dev, c, FLAGS[flags]), f"B-Hardswish {flags}")
    _report(f"B-Hardswish {flags}", e)
    _assert_bars("B-Hardswish", f"B-Hardswish {flags}", e)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", list(FLAGS))
def test_autograd_saturated_frames_vs_float64(dev, flags):
    """Setup C: parameter gradients under both flag settings; dx under the direct flags, where ties survive.  Under the default
    flags dx is printed only: the fused Winograd forward breaks the ties of exactly constant regions by rounding."""
    c = _case("C-PReLU")
    got = _module_run(dev, c, FLAGS[flags])
    e = _errors(c, got, f"C-PReLU {flags}")
    _report(f"C-PReLU {flags}", e)
    print(f"C-PReLU {flags}: dx per frame " + ", ".join(f"{_l2(got['dx'][i], c['ref']['dx'][i]):.2e}" for i in range(2)))
    _assert_bars("C-PReLU", f"C-PReLU {flags}", e, skip=() if FLAGS[flags] else ("dx",))
