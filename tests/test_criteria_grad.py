"""GPU tests of the training loss and its gradient on their own (csrc/criteria.hip, nd_criteria_grad; validation.criteria_grad):
the loss section of the fused training step, reached without a network.  Against float64 autograd on the CPU through clip(0, 1),
the centre slice and oracle/losses.py; at planted pixels where the conventions decide (clamp passes the gradient on the closed
interval, sign(0) = 0, zero outside the window) with exact expected values; and against the per-sample criteria of validation."""
import functools

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib
from nind_denoise_amd.validation import COLUMNS, _workspace, criteria, criteria_grad
from test_nn_train import MEAN_TOL, SCORE_TOL, dev, image_like  # noqa: F401  (dev: the module's GPU fixture)

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-4       # max|err| / max|ref| of a gradient with SSIM terms: the bar of test_ssim_losses_backward_vs_oracle_autograd
# Without SSIM terms an element is one fp32 expression, pass * (w_l1 * sgn + w_mse * 2 * d) * (1 / N): d = clip(y) - t rounds once
# (clip, sgn, pass and the factor 2 are exact), the two products with the weights, their sum, the rounding of 1 / N and the product
# with it once each: six roundings of at most 2^-24 relative each, whatever the compiler fuses.  The sum's operands may cancel, so a
# rounding is relative to the larger operand, hence to max|ref| rather than to the element: 8 * 2^-24 of max|ref| leaves two spare.
PLAIN_GRAD_TOL = 8 * 2.0 ** -24

CASES = [
    # n, h, w, loss_cs, weights
    (3, 72, 88, 61, {"L1": 0.3, "MSE": 0.2, "SSIM": 0.5}),     # odd margins, rectangular, 3 * 61^2 is no multiple of 256
    (1, 56, 56, 0, {"MSE": 1.0}),
    (2, 184, 168, 161, {"MSSSIM": 0.6, "L1": 0.4}),
]
IDS = ["72x88-cs61", "56x56", "184x168-cs161"]


def window(h, w, loss_cs):
    """rows and columns of the centre window as slices (pt_ops.pt_crop_batch)"""
    if not loss_cs:
        return slice(0, h), slice(0, w)
    y0, x0 = (h - loss_cs) // 2, (w - loss_cs) // 2
    return slice(y0, y0 + loss_cs), slice(x0, x0 + loss_cs)


@functools.lru_cache(maxsize=None)
def case_data(i):
    """Inputs of case i as in test_criteria_vs_float64 (y spans [-0.2, 1.2]: the clip bites), and the float64 reference, made once:
    (y, t, loss, the L1 / MSE part of the loss, gy)"""
    from oracle import losses as olosses
    n, h, w, loss_cs, weights = CASES[i]
    t = image_like(n, h, w, seed=11)
    g = torch.Generator().manual_seed(12)
    y = -0.2 + 1.4 * (t + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)
    assert y.min() < -0.05 and y.max() > 1.05 and 0 <= t.min() and t.max() <= 1
    rows, cols = window(h, w, loss_cs)
    yd = y.double().requires_grad_()
    gw, tw = yd.clip(0, 1)[:, :, rows, cols], t.double()[:, :, rows, cols]
    plain = weights.get("L1", 0.0) * (gw - tw).abs().mean() + weights.get("MSE", 0.0) * ((gw - tw) ** 2).mean()
    loss = plain
    if weights.get("SSIM"):
        loss = loss + weights["SSIM"] * (1 - olosses.ssim(gw, tw)).mean()
    if weights.get("MSSSIM"):
        loss = loss + weights["MSSSIM"] * (1 - olosses.ms_ssim(gw, tw)).mean()
    loss.backward()
    return y, t, loss.item(), plain.item(), yd.grad


def run(y, t, weights, loss_cs):
    """nd_criteria_grad on device tensors with gy pre-filled with NaN: whatever the call does not write stays visible"""
    lib = _lib.load()
    n, _, h, w = y.shape
    loss = torch.full((), float("nan"), dtype=torch.float32, device=y.device)
    gy = torch.full_like(y, float("nan"))
    ws = _workspace(y.device, lib.nd_criteria_grad_workspace_bytes(n, h, w, 0))    # the size for the whole image serves every loss_cs
    _lib.check(lib.nd_criteria_grad(y.data_ptr(), t.data_ptr(), n, h, w, loss_cs, *[float(weights.get(k) or 0.0) for k in COLUMNS],
                                    loss.data_ptr(), gy.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(y.device)),
               "nd_criteria_grad")
    return loss, gy


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_criteria_grad_vs_float64(dev, i):
    n, h, w, loss_cs, weights = CASES[i]
    y, t, loss_ref, plain_ref, gy_ref = case_data(i)
    yd, td = y.to(dev), t.to(dev)
    loss, gy = run(yd, td, weights, loss_cs)
    torch.cuda.synchronize()
    what = f"criteria_grad {n}x{h}x{w} cs{loss_cs}"
    rows, cols = window(h, w, loss_cs)
    assert torch.isfinite(gy).all() and torch.isfinite(loss), what                 # written in full over the NaN fill
    outside = torch.ones(h, w, dtype=torch.bool, device=dev)
    outside[rows, cols] = False
    assert int(outside.sum()) == h * w - (rows.stop - rows.start) * (cols.stop - cols.start)
    assert torch.equal(gy[:, :, outside], torch.zeros_like(gy[:, :, outside])), what
    # the loss: MEAN_TOL relative for the L1 / MSE part (a thread adds at most ceil(N / 2^18) terms in a row, then two trees of 8 levels
    # with 4 terms per thread between them: a shorter chain than the one MEAN_TOL is worked out for), SCORE_TOL per unit of score weight
    bar = MEAN_TOL * abs(plain_ref) + SCORE_TOL * (abs(weights.get("SSIM", 0.0)) + abs(weights.get("MSSSIM", 0.0)))
    err = abs(loss.item() - loss_ref)
    print(f"{what} loss: {loss.item():.9g}, float64 {loss_ref:.9g}, |err| {err:.3e}, bar {bar:.3e}")
    assert err <= bar, (what, loss.item(), loss_ref)
    scale = gy_ref.abs().max().item()
    gerr = (gy.double().cpu() - gy_ref).abs().max().item() / scale
    gbar = GRAD_TOL if weights.get("SSIM") or weights.get("MSSSIM") else PLAIN_GRAD_TOL
    print(f"{what} gy: worst |err| / max|ref| {gerr:.3e}, bar {gbar:.3e}, max|ref| {scale:.3e}")
    assert scale > 0 and gerr <= gbar, (what, gerr, gbar)
    # deterministic: the same bits from a second call, and through the Python wrapper
    loss2, gy2 = run(yd, td, weights, loss_cs)
    loss3, gy3 = criteria_grad(yd, td, weights, loss_cs)
    assert torch.equal(loss, loss2) and torch.equal(gy, gy2) and torch.equal(loss, loss3) and torch.equal(gy, gy3), what
    # The last sample alone: n enters a gradient only as the divisor of the mean (1 / (n * 3 * Lh * Lw); weight / (n * 3) in the
    # SSIM coefficients).  For n = 2 that divisor is the lone sample's times a power of two, so every intermediate is the lone
    # sample's halved, exactly (nothing here is near the subnormal range); asserted to within one rounding.  n = 3 scales by no
    # power of two: fp32(1 / 3N) is not fp32(1 / N) / 3, so that case is left out.
    if n == 2:
        _, one = run(yd[n - 1:].contiguous(), td[n - 1:].contiguous(), weights, loss_cs)
        assert (one - n * gy[n - 1:]).abs().le(2.0 ** -23 * one.abs()).all(), what
    # tie to validation: the batch loss is the mean of the per-sample weighted criteria (the bar of
    # test_criteria_mean_equals_the_training_steps_loss)
    mean = criteria(yd, td, weights, loss_cs)["weighted"].double().mean().item()
    print(f"{what}: loss {loss.item():.9g}, mean of the per-sample weighted criteria {mean:.9g}")
    assert abs(mean - loss.item()) <= 1e-5 * abs(loss.item()), (what, mean, loss.item())


def test_conventions_at_planted_pixels(dev):
    """56 x 56, loss_cs 40, L1 + MSE, n = 2.  y == t everywhere in the window except at planted pixels, weights and planted values
    dyadic: every product and sum below is exact in fp32 in any order and however fused, so the expected values are exact --
    S * fp32(1 / N) rounded once, N = 2 * 3 * 40 * 40."""
    n, h, w, cs, weights = 2, 56, 56, 40, {"L1": 0.5, "MSE": 0.5}
    t = image_like(n, h, w, seed=21)
    g = torch.Generator().manual_seed(22)
    y = -0.2 + 1.4 * torch.rand(n, 3, h, w, generator=g)      # outside the window: anything, also beyond [0, 1]
    rows, cols = window(h, w, cs)
    assert (rows.start, rows.stop) == (8, 48)
    y[:, :, rows, cols] = t[:, :, rows, cols]
    tiny, above = -float(np.finfo(np.float32).tiny), float(np.nextafter(np.float32(1), np.float32(2)))   # the nearest normal numbers outside [0, 1]
    # (sample, channel, row, column): y, t -> d = clip(y) - t, whether the clamp passes the gradient
    planted = {(0, 0, 8, 8): (0.0, 0.25, -0.25, True),          # first pixel of the window: the gradient passes at 0.0
               (0, 0, 8, 9): (tiny, 0.25, -0.25, False),        # beside it, just below 0: exactly 0
               (0, 2, 47, 47): (1.0, 0.25, 0.75, True),         # last pixel of the window: the gradient passes at 1.0
               (0, 2, 47, 46): (above, 0.25, 0.75, False),      # just above 1: exactly 0
               (1, 1, 30, 17): (0.5, 0.5, 0.0, True),           # y == target: sign(0) = 0, the L1 part is exactly 0
               (1, 1, 30, 18): (1.0, 1.0, 0.0, True),
               (1, 0, 47, 8): (0.0, 0.75, -0.75, True)}
    for (b, c, r, x), (yv, tv, _, _) in planted.items():
        y[b, c, r, x], t[b, c, r, x] = yv, tv
    yd, td = y.to(dev), t.to(dev)
    loss, gy = run(yd, td, weights, cs)
    torch.cuda.synchronize()
    inv = np.float32(1) / np.float32(n * 3 * cs * cs)
    total = np.float32(sum(0.5 * abs(d) + 0.5 * d * d for _, _, d, _ in planted.values()))       # dyadic: exact
    assert loss.item() == float(total * inv), (loss.item(), float(total * inv))
    expect = torch.zeros_like(y)
    for (b, c, r, x), (_, _, d, passes) in planted.items():
        sgn = (d > 0) - (d < 0)
        expect[b, c, r, x] = float(np.float32(0.5 * sgn + 0.5 * 2 * d) * inv) if passes else 0.0
    assert expect[0, 0, 8, 8] == float(np.float32(-0.75) * inv) and expect[0, 2, 47, 47] == float(np.float32(1.25) * inv)
    assert expect[1, 1, 30, 17] == 0 and expect[0, 0, 8, 9] == 0 and int((expect != 0).sum()) == 3
    assert torch.equal(gy.cpu(), expect)              # the planted values, 0 at every d == 0 and outside the window
    # a flipped target outside the window changes no bit
    t2 = 1 - t
    t2[:, :, rows, cols] = t[:, :, rows, cols]
    loss2, gy2 = run(yd, t2.to(dev), weights, cs)
    assert torch.equal(loss, loss2) and torch.equal(gy, gy2)
