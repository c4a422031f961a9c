"""GPU tests of the piqa-style SSIM / MS-SSIM (csrc/ssim.hip) against float64 on image-like pairs, through ctypes on the three entry
points nd_ssim, nd_ms_ssim and nd_ssim_loss_grad.  Cases, references, bars and edge classes: tests/ssim_cases.py; that the bars see
planted errors and stay under their cap: tests/test_ssim_float64_host.py.

Bars.  Score: |gpu - R64| <= max(10 |R32 - R64|, 4 * 2^-24) per sample.  Gradient (weight 0.7, accumulate = 0 into a NaN-filled gx),
per sample and edge class: max_class |g - g64| / max_class |g64| <= 10 x the same figure of R32's autograd gradient; where g64 is 0
(x == y) max_class |g| <= 10 max_class |g32|; on a plane with y = 1 - x the gradient is 0.

Measured on an MI355X (test_worst_ratios_by_regime prints this table): the worst GPU / R32 error ratio per mode and regime, 10 being
the bar.  Score: |gpu - R64| / max(|R32 - R64|, 0.4 * 2^-24).  Gradient: max_class |g - g64| over R32's own, with the class
(d_y, d_x) that held it ('abs' regimes: max_class |g| over max_class |g32|).

  mode    regime          score   gradient class          before: score   gradient class
  ssim    dark_exposure    5.10    2.94 (8,7)                      3.38    14.33 (7,3)
  ssim    bright_flat      0.16    0.02 (4,8)                      2.07    18.72 (6,3)
  ssim    texture          2.87    1.61 (5,2)                    152.13    54.41 (5,2)
  ssim    near             1.00    1.08 (2,2)                     17.38    18.99 (3,2)
  ssim    identical        2.50    0    (g == 0)                   2.50    inf   (0,0)
  msssim  dark_exposure    2.47    3.28 (1,5)                      3.26     6.48 (1,5)
  msssim  bright_flat      0.01    2.72 (9,7)                      0.95    17.90 (9,7)
  msssim  texture          0.47    0.59 (0,8)                      4.55    12.22 (7,4)
  msssim  near             0.25    1.27 (0,0)                      3.94     5.70 (8,2)
  msssim  identical        0       0    (g == 0)                   0       inf   (0,0)
  msssim  dead_plane       0.36    0.68 (0,4)                      4.44    28.29 (5,8)

'before' is csrc/ssim.hip as these tests found it, 38 of them failing, for three reasons.  write_window() added the 11 taps one
after the other in fp32, one ulp below torch's sum, so its window was not piqa's: every textured SSIM score sat 3e-6 low.
k_ssim_bwd_tile left its moments to the compiler's contraction, so the gradient of (image, image) was not 0 where torch's is (inf
above), and E[xx] - mu^2 lost its digits on bright flat and nearly equal pairs.  Now both kernels take the moments of x and y less one
level per workgroup with the forward kernel's explicit fmaf operations, and the shifted moments account for the window's sum."""
import pytest
import torch

import ssim_cases as S
from nind_denoise_amd import _lib

pytestmark = pytest.mark.gpu

CASES = S.all_cases()
IDS = [S.case_id(*k) for k in CASES]
LOSS_PREFILL = 0.75               # loss_acc before a call: its fp32 spacing, 2^-24, is half the spacing of any sum in [1, 2)
ULP_PREFILL = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def run_score(mode, xd, yd):
    lib = _lib.load()
    n, c, h, w = xd.shape
    wsb = lib.nd_ssim_workspace_bytes(n, c, h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=xd.device)
    out = torch.full((n,), float("nan"), dtype=torch.float32, device=xd.device)
    name = "nd_ms_ssim" if mode == "msssim" else "nd_ssim"
    _lib.check(getattr(lib, name)(xd.data_ptr(), yd.data_ptr(), n, c, h, w, out.data_ptr(), ws.data_ptr(), wsb, _lib.stream_ptr(xd.device)),
               name)
    return out


def run_grad(mode, xd, yd, gx, loss, accumulate):
    """nd_ssim_loss_grad on prefilled gx and loss_acc (both are written in place)"""
    lib = _lib.load()
    n, c, h, w = xd.shape
    wsb = lib.nd_ssim_loss_workspace_bytes(n, c, h, w)
    ws = torch.empty(wsb, dtype=torch.uint8, device=xd.device)
    assert gx.shape == xd.shape and gx.is_contiguous() and xd.is_contiguous() and yd.is_contiguous() and loss.numel() == 1
    _lib.check(lib.nd_ssim_loss_grad(xd.data_ptr(), yd.data_ptr(), n, c, h, w, 1 if mode == "msssim" else 0, S.WEIGHT, loss.data_ptr(),
                                     gx.data_ptr(), accumulate, ws.data_ptr(), wsb, _lib.stream_ptr(xd.device)), "nd_ssim_loss_grad")
    return loss, gx


_results = {}


def gpu(dev, key):
    """every call of one case, made once: scores, gradient and loss (accumulate = 0), both again, and the accumulating call"""
    if key not in _results:
        mode = key[0]
        cs = S.case(*key)
        xd, yd = cs["x"].to(dev), cs["y"].to(dev)
        prefill = torch.empty_like(cs["x"]).uniform_(-1, 1, generator=torch.Generator().manual_seed(1)).to(dev)
        res = {}
        for tag in ("", "2"):
            res["score" + tag] = run_score(mode, xd, yd)
            res["loss" + tag], res["gx" + tag] = run_grad(mode, xd, yd, torch.full_like(xd, float("nan")),
                                                          torch.full((1,), LOSS_PREFILL, dtype=torch.float32, device=dev), 0)
        res["loss_acc"], res["gx_acc"] = run_grad(mode, xd, yd, prefill.clone(), torch.full((1,), LOSS_PREFILL, dtype=torch.float32, device=dev), 1)
        res["sum"] = prefill + res["gx"]                                               # one fp32 add
        torch.cuda.synchronize()
        _results[key] = {k: v.cpu() for k, v in res.items()}
    return _results[key]


def score_figures(cs, got):
    """per sample: |gpu - R64|, the bar, and the error against R32's own (GPU / max(|R32 - R64|, 0.4 * 2^-24): 10 is the bar)"""
    err = (got.double() - cs["s64"]).abs()
    return err, cs["score_bar"], S.FACTOR * err / cs["score_bar"]


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_scores_vs_float64(dev, key):
    cs, res = S.case(*key), gpu(dev, key)
    err, bar, ratio = score_figures(cs, res["score"])
    for i, regime in enumerate(cs["regimes"]):
        print(f"{S.case_id(*key)} sample {i} {regime}: score {res['score'][i].item():.9g}, float64 {cs['s64'][i].item():.12g}, "
              f"|err| {err[i].item():.2e}, bar {bar[i].item():.2e}, GPU / R32 {ratio[i].item():.2f}")
    assert torch.isfinite(res["score"]).all()
    assert (err <= bar).all(), (err, bar)
    for i, regime in enumerate(cs["regimes"]):
        if regime == "identical":
            assert abs(res["score"][i].item() - 1) <= 1e-6


def worst_class(r):
    p = r["present"]
    k = int(torch.where(p, r["ratio"], torch.full_like(r["ratio"], -1.0)).argmax())
    return r["ratio"][k].item(), k


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_gradient_vs_float64_per_edge_class(dev, key):
    cs, res = S.case(*key), gpu(dev, key)
    g = res["gx"]
    assert torch.isfinite(g).all()                                                     # written in full over the NaN fill
    failures = []
    for r in S.grad_report(cs, g):
        p = r["present"]
        ratio, k = worst_class(r)
        print(f"{S.case_id(*key)} sample {r['sample']} {r['regime']} ({r['kind']}): worst GPU / R32 {ratio:.2f} in class {S.class_name(k)} "
              f"(figure {r['fig'][k].item():.2e}, bar {r['bar'][k].item():.2e}); largest figure {r['fig'][p].max().item():.2e}")
        bad = p & ~(r["fig"] <= r["bar"])
        failures += [(r["sample"], r["regime"], S.class_name(int(k)), r["fig"][k].item(), r["bar"][k].item()) for k in bad.nonzero().flatten()]
    assert not failures, failures[:8]
    for i, ch in S.dead_planes(cs):
        assert not g[i, ch].any()                                                      # == 0 everywhere


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_accumulation_and_loss(dev, key):
    cs, res = S.case(*key), gpu(dev, key)
    assert torch.equal(res["gx_acc"], res["sum"])                                      # prefill + g, one fp32 add
    bar = S.WEIGHT * cs["score_bar"].mean().item() + ULP_PREFILL
    for tag in ("loss", "loss_acc"):
        moved = res[tag].double().item() - LOSS_PREFILL
        print(f"{S.case_id(*key)} {tag}: moved by {moved:.9g}, float64 {cs['loss64']:.12g}, |err| {abs(moved - cs['loss64']):.2e}, bar {bar:.2e}")
        assert abs(moved - cs["loss64"]) <= bar, (tag, moved, cs["loss64"], bar)
    assert torch.equal(res["loss"], res["loss_acc"])


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_two_calls_are_bit_equal(dev, key):
    res = gpu(dev, key)
    assert torch.equal(res["score"], res["score2"]) and torch.equal(res["loss"], res["loss2"])
    assert torch.equal(res["gx"].view(torch.int32), res["gx2"].view(torch.int32))


@pytest.mark.parametrize("key", [("ssim", (1, 3, 17, 75), "dark_exposure"), ("msssim", (1, 3, 161, 161), "near")],
                         ids=lambda k: S.case_id(*k))
def test_wrappers_are_the_ctypes_path(dev, key):
    """pt_losses.SSIM_loss / MS_SSIM_loss: 1 - the same scores, and through .backward() the same gradient (one sample: the wrapper
    hands nd_ssim_loss_grad each sample with its incoming gradient as the weight, here fp32(0.7) as in the direct call)"""
    from nind_denoise_amd.common.libs import pt_losses
    cs, res = S.case(*key), gpu(dev, key)
    assert cs["shape"][0] == 1
    xd = cs["x"].to(dev).requires_grad_()
    crit = pt_losses.MS_SSIM_loss() if key[0] == "msssim" else pt_losses.SSIM_loss()
    loss = crit(xd, cs["y"].to(dev))
    (S.WEIGHT * loss).sum().backward()
    assert torch.equal(loss.detach().cpu(), 1 - res["score"])
    assert torch.equal(xd.grad.cpu(), res["gx"])


def test_worst_ratios_by_regime(dev):
    """The table of this module's docstring: per mode and regime, the worst GPU / R32 error ratio of a score and of a gradient class,
    and the class that held it.  The bars are asserted case by case above; this asserts only that every regime was measured."""
    table = {}
    for key in CASES:
        cs, res = S.case(*key), gpu(dev, key)
        _, _, sratio = score_figures(cs, res["score"])
        for r in S.grad_report(cs, res["gx"]):
            ratio, k = worst_class(r)
            row = table.setdefault((key[0], r["regime"]), dict(score=(-1.0, ""), grad=(-1.0, "", "")))
            cid = f"{S.shape_id(key[1])} sample {r['sample']}"
            row["score"] = max(row["score"], (sratio[r["sample"]].item(), cid))
            row["grad"] = max(row["grad"], (ratio, S.class_name(k), cid))
    print("mode     regime          score GPU/R32 (where)                         gradient class GPU/R32 (class, where)")
    for (mode, regime), row in sorted(table.items()):
        print(f"{mode:8s} {regime:14s} {row['score'][0]:8.2f} ({row['score'][1]:28s})   {row['grad'][0]:8.2f} ({row['grad'][1]}, {row['grad'][2]})")
    assert set(table) == {(m, r) for m in S.REGIMES for r in S.REGIMES[m]}
