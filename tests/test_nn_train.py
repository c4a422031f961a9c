"""GPU tests of the training loop: per-sample criteria (csrc/criteria.hip) against float64, their agreement with the fused
training step's own loss, the batched validation pass, the fused step for ELU and Hardswish against the autograd path, and
nn_train end to end on a synthetic tree (files of a run, pruning, resuming, reproducibility, and that it learns).

Everything runs at funit 8.  The smallest crop the network takes is 104 (16k + 56 with a bottom level of at least 3 pixels), so
the network cases run at 104 x 104 (MS-SSIM: 168 x 168); the criteria alone also run on smaller and rectangular images."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from nind_denoise_amd import _lib, synth
from nind_denoise_amd.common.libs import imgcodec

pytestmark = pytest.mark.gpu

FUNIT = 8
SCORE_TOL = 2e-5      # the project's bar for fp32 SSIM / MS-SSIM scores (test_eval_harness.py), absolute
MEAN_TOL = 2e-5       # L1 / MSE, relative: a sum of N fp32 terms whose longest serial chain is c terms is within about
#                       (c + log2 N) * 2^-24 of the exact one; nd_criteria keeps c below 40 at these sizes (16 per thread, then
#                       trees), N = 3 * 184 * 168 < 2^17: 57 * 6e-8 = 3.4e-6, under the bar with room for the clip and the square
Y_BAR = 2e-6          # fp32 forward against float64, relative to max(1, max|ref|): the "y" bar of test_train_float64.py


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def image_like(n, h, w, seed):
    """bilinear-upsampled noise plus fine noise, in [0, 1] (the crops of test_train_float64.py)"""
    g = torch.Generator().manual_seed(seed)
    c = F.interpolate(torch.rand(n, 3, max(h // 8, 2), max(w // 8, 2), generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * c + 0.1 + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)


def oracle_criteria(y, t, weights, loss_cs, also=()):
    """The five columns in float64 on the CPU: plain torch and oracle/losses.py.  Columns that are not computed are 0."""
    from oracle import losses as olosses
    g, t = y.double().clip(0, 1), t.double()
    if loss_cs:
        y0, x0 = (g.shape[2] - loss_cs) // 2, (g.shape[3] - loss_cs) // 2
        g, t = g[:, :, y0:y0 + loss_cs, x0:x0 + loss_cs], t[:, :, y0:y0 + loss_cs, x0:x0 + loss_cs]
    fns = {"L1": lambda: (g - t).abs().mean((1, 2, 3)), "MSE": lambda: ((g - t) ** 2).mean((1, 2, 3)),
           "SSIM": lambda: 1 - olosses.ssim(g, t), "MSSSIM": lambda: 1 - olosses.ms_ssim(g, t)}
    out = {k: (fn() if weights.get(k) or k in also else torch.zeros(g.shape[0], dtype=torch.float64)) for k, fn in fns.items()}
    out["weighted"] = sum(weights[k] * out[k] for k in fns if weights.get(k))
    return out


def column_bars(ref, weights, y_err=0.0):
    """Bars per column for a float64 reference `ref`.  y_err: what the generated image itself may be off by (0 when both sides
    see the same image): it moves L1 by at most y_err and MSE by at most 2 max|g - t| y_err <= 2 y_err.  (Not worked out for the
    scores: a case with y_err weights L1 and MSE only.)"""
    assert not (y_err and (weights.get("SSIM") or weights.get("MSSSIM")))
    bars = {"L1": MEAN_TOL * ref["L1"] + y_err, "MSE": MEAN_TOL * ref["MSE"] + 2 * y_err,
            "SSIM": torch.full_like(ref["SSIM"], SCORE_TOL), "MSSSIM": torch.full_like(ref["MSSSIM"], SCORE_TOL)}
    bars["weighted"] = sum(abs(weights[k]) * bars[k] for k in ("L1", "MSE", "SSIM", "MSSSIM") if weights.get(k))
    return bars


def assert_columns(got, ref, bars, what):
    for k in ("L1", "MSE", "SSIM", "MSSSIM", "weighted"):
        g = got[k].detach().double().cpu()
        err = (g - ref[k]).abs()
        print(f"{what} {k}: worst |err| {err.max().item():.3e}, bar {torch.as_tensor(bars[k]).min().item():.3e}, ref {ref[k].tolist()}")
        assert g.shape == ref[k].shape and torch.isfinite(g).all(), (what, k)
        assert (err <= bars[k]).all(), (what, k, g.tolist(), ref[k].tolist())


# ------------------------------------------------------------------ 1. criteria vs float64
CRITERIA_CASES = [
    # n, h, w, loss_cs, weights, also
    (3, 72, 88, 61, {"L1": 0.3, "MSE": 0.2, "SSIM": 0.5}, ()),            # odd margins, rectangular, 3 * 61^2 is no multiple of 256
    (1, 56, 56, 0, {"MSE": 1.0}, ("L1", "SSIM")),                          # the `also` bits: computed, not weighted
    (2, 168, 168, 0, {"MSSSIM": 0.6, "L1": 0.4}, ()),
    (2, 184, 168, 161, {"MSSSIM": 1.0}, ("MSE",)),
]


@pytest.mark.parametrize("n,h,w,loss_cs,weights,also", CRITERIA_CASES, ids=["72x88-cs61", "56x56", "168x168-msssim", "184x168-cs161"])
def test_criteria_vs_float64(dev, n, h, w, loss_cs, weights, also):
    from nind_denoise_amd.validation import criteria
    t = image_like(n, h, w, seed=11)
    g = torch.Generator().manual_seed(12)
    # y in [-0.2, 1.2]: the clip bites below 1/7 and above 6/7 of the unclipped image; t in [0, 1]
    y = -0.2 + 1.4 * (t + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)
    assert y.min() < -0.05 and y.max() > 1.05 and 0 <= t.min() and t.max() <= 1
    got = criteria(y.to(dev), t.to(dev), weights, loss_cs, also)
    torch.cuda.synchronize()
    ref = oracle_criteria(y, t, weights, loss_cs, also)
    assert_columns(got, ref, column_bars(ref, weights), f"criteria {n}x{h}x{w} cs{loss_cs}")
    for k in ("L1", "MSE", "SSIM", "MSSSIM"):
        if weights.get(k) or k in also:
            assert (got[k] > 0).all(), k                 # computed (the images differ)
        else:
            assert (got[k] == 0).all(), k                # not computed: written as 0
    # deterministic: the same bits from a second call, and from a batch of one
    again = criteria(y.to(dev), t.to(dev), weights, loss_cs, also)
    one = criteria(y[n - 1:].to(dev), t[n - 1:].to(dev), weights, loss_cs, also)
    for k in got:
        assert torch.equal(got[k], again[k]) and torch.equal(got[k][n - 1:], one[k]), k


# ------------------------------------------------------------------ 2. consistency with the training step
@pytest.mark.parametrize("cs,B,weights", [(104, 3, {"MSE": 1.0}), (168, 2, {"MSSSIM": 0.6, "L1": 0.4})], ids=["mse-104", "msssim-l1-168"])
def test_criteria_mean_equals_the_training_steps_loss(dev, cs, B, weights):
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    from nind_denoise_amd.validation import criteria
    net = UtNet(funit=FUNIT)
    net.load_state_dict(synth.make_utnet_state_dict(funit=FUNIT, seed=31, gain=1.8))
    tr = UtNetTrainer(net, device=dev, weights=weights)
    x = image_like(B, cs, cs, seed=3)
    t = (x * 0.9 + 0.05 * image_like(B, cs, cs, seed=4)).clip(0, 1)
    y, loss = tr.forward_backward(x, t)
    got = criteria(y, t.to(dev), weights)
    mean, loss = got["weighted"].double().mean().item(), loss.item()
    print(f"step loss {loss:.9g}, mean of the per-sample weighted criteria {mean:.9g}")
    assert abs(mean - loss) <= 1e-5 * abs(loss), (mean, loss)


# ------------------------------------------------------------------ 3. validate
def dark_pairs(n, side, seed):
    """A dim scene under red light: the clean red channel is image-like in [0.2, 0.32], green and blue are black; noisy = clean +
    fixed noise.  Chosen for what a fresh network can learn in the 16 updates of the end-to-end run: with torch's default
    initialisation under seed 7 the last layer's biases are (0.12, -0.11, -0.34), the green and blue outputs start below 0
    everywhere, and clip(0, 1) passes no gradient there (nn_common.py:198-199), so only the red channel can move, by about 0.05 at
    lr 1e-3.  A target 0.13 above the initial red output, and at the clipped value of the other two, is within reach."""
    clean = torch.zeros(n, 3, side, side)
    clean[:, 0] = 0.2 + 0.12 * image_like(n, side, side, seed)[:, 0]
    g = torch.Generator().manual_seed(seed + 1)
    return clean, (clean + 0.02 * torch.randn(n, 3, side, side, generator=g)).clip(0, 1)


def write_pairs(root, n, side, seed):
    """n [clean, noisy] pairs of side x side 8-bit PNGs"""
    os.makedirs(root, exist_ok=True)
    clean, noisy = dark_pairs(n, side, seed)
    pairs = []
    for i in range(n):
        paths = [os.path.join(root, f"{kind}_{i}.png") for kind in ("clean", "noisy")]
        for path, img in zip(paths, (clean[i], noisy[i])):
            imgcodec.write_png(path, (img * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy())
        pairs.append(paths)
    return pairs


def test_validate_batched_equals_one_by_one_and_float64(dev, tmp_path, monkeypatch):
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.validation import ValidationSet, validate
    from oracle import networks as onet
    monkeypatch.setattr(UtNet, "split_k", False)       # every tile whole: a sample's bits do not depend on its batch
    cs, loss_cs, weights = 104, 92, {"L1": 0.4, "MSE": 0.6}
    vs = ValidationSet(write_pairs(str(tmp_path / "val"), 5, 110, seed=21), dev, cs)
    sd = synth.make_utnet_state_dict(funit=FUNIT, seed=31, gain=1.8)
    net = UtNet(funit=FUNIT)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    avg2, per2 = validate(net, vs, weights, loss_cs, batch_size=2)        # 2 + 2 + 1: the last batch is partial
    assert net.training and isinstance(avg2, float)
    assert per2.shape == (5,) and not per2.requires_grad and per2.grad_fn is None
    avg1, per1 = validate(net, vs, weights, loss_cs, batch_size=1)
    assert torch.equal(per1, per2) and avg1 == avg2
    assert avg2 == per2.double().mean().item()
    with torch.no_grad():
        y = net.eval()(vs.noisy[:2])
        assert not y.requires_grad
    net.train()
    # float64: the oracle network and the oracle criteria on the same pairs
    y64 = onet.utnet_forward({k: v.double() for k, v in sd.items()}, vs.noisy.cpu().double())
    ref = oracle_criteria(y64, vs.clean.cpu(), weights, loss_cs)
    y_err = Y_BAR * max(1.0, y64.abs().max().item())
    bars = column_bars(ref, weights, y_err)
    err = (per2.double().cpu() - ref["weighted"]).abs()
    print(f"validate: per-sample weighted {per2.tolist()}, float64 {ref['weighted'].tolist()}, worst |err| {err.max().item():.3e}, "
          f"bar {bars['weighted'].min().item():.3e}")
    assert (err <= bars["weighted"]).all()
    assert abs(avg2 - ref["weighted"].mean().item()) <= bars["weighted"].max().item()
    # output_val_images: one 8-bit tif per pair, the whole clipped output
    out_dir = str(tmp_path / "val_out" / "3")
    validate(net, vs, weights, loss_cs, batch_size=2, output_to_dir=out_dir)
    assert sorted(os.listdir(out_dir)) == [f"{i}.tif" for i in range(5)]
    img = imgcodec.read_tiff(os.path.join(out_dir, "4.tif"))
    assert img.shape == (cs, cs, 3) and img.dtype == np.uint8
    want = (y64[4].clip(0, 1) * 255 + 0.5).floor().permute(1, 2, 0).numpy()
    assert np.abs(img.astype(np.int64) - want.astype(np.int64)).max() <= 1


# ------------------------------------------------------------------ 4. fused step with ELU and Hardswish
@pytest.mark.parametrize("activation", ["ELU", "Hardswish"])
def test_fused_step_equals_autograd_for_every_activation(dev, activation):
    """One forward_backward of the fused step against the autograd path (model.train(); model(x).clip(0, 1); MSE; backward()) on
    the same weights.  Both run the same forward and backward kernels, so the output is the same bit for bit, as in
    test_autograd_training_matches_fused_step (test_hip_parity.py), whose bars these are: the loss to 1e-6 relative, and 1e-5 for
    what comes behind the loss -- there the next step's output, here every gradient tensor relative to its largest entry.  (The
    two sides differ only in how d loss / d y is rounded: (2 d) / N in the step's kernel, torch's mse_loss and clamp backward in
    the other, one or two ulps per pixel; the backward pass is linear in it.)"""
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    cs, B = 104, 3
    sd = synth.make_utnet_state_dict(funit=FUNIT, seed=31, activation=activation, gain=1.8)
    x = image_like(B, cs, cs, seed=3)
    if activation == "Hardswish":       # inputs scaled until pre-activations lie on both sides of -3 and of +3
        x = x * 12
        pre = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), sd["convs1.0.weight"], sd["convs1.0.bias"])
        assert pre.min() < -3.5 and pre.max() > 3.5 and (pre.abs() < 2.5).any()
    t = image_like(B, cs, cs, seed=4)
    fused = UtNet(funit=FUNIT, activation=activation)
    fused.load_state_dict(sd)
    tr = UtNetTrainer(fused, device=dev, weights={"MSE": 1.0})
    y, loss = tr.forward_backward(x, t)
    loss = loss.item()
    net = UtNet(funit=FUNIT, activation=activation)
    net.load_state_dict(sd)
    net = net.to(dev).train()
    out = net(x.to(dev))
    ref_loss = F.mse_loss(out.clip(0, 1), t.to(dev))
    ref_loss.backward()
    assert torch.equal(out.detach(), y)
    assert ((y > 0) & (y < 1)).float().mean().item() > 0.05, "the clip leaves too few pixels a gradient"
    assert abs(loss - ref_loss.item()) <= 1e-6 * max(1.0, abs(ref_loss.item())), (loss, ref_loss.item())
    worst = 0.0
    names = [n for n, _ in net.named_parameters()]
    assert names and not any(n.rsplit(".", 1)[0] in synth.utnet_prelu_keys() for n in names)   # no slopes: every tensor is a conv's
    for name, p in net.named_parameters():
        got, ref = tr.grad_of(name), p.grad
        scale = ref.abs().max().item()
        assert scale > 0 and torch.isfinite(got).all(), name
        err = (got - ref).abs().max().item() / scale
        worst = max(worst, err)
        assert err <= 1e-5, (activation, name, err, scale)
    print(f"fused step {activation}: worst relative gradient difference to autograd {worst:.2e}")


# ------------------------------------------------------------------ 5. end to end
SIDE, CS, LOSS_CS, BATCH, GROUPS = 128, 104, 60, 4, 16


def make_tree(root):
    """16 groups of 128 x 128 8-bit crops in the directory shape the crop pool scans (<root>/<set>/<ISO>/<crop file>): four sets of
    four crops, a clean ISO and a noisy one, noisy = clean + fixed noise; and an 8-pair validation yaml."""
    data = os.path.join(root, f"SYN_{SIDE}_96")
    clean, noisy = dark_pairs(GROUPS, SIDE, seed=41)
    for k in range(GROUPS):
        aset, crop = f"set{k // 4}", f"{k % 4}_0"
        for iso, img in (("ISO100", clean[k]), ("ISO6400", noisy[k])):
            os.makedirs(os.path.join(data, aset, iso), exist_ok=True)
            imgcodec.write_png(os.path.join(data, aset, iso, f"SYN_{aset}_{iso}_{crop}_96.png"),
                               (img * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy())
    val_yaml = os.path.join(root, "val.yaml")
    with open(val_yaml, "w") as f:
        yaml.dump(write_pairs(os.path.join(root, "val"), 8, SIDE, seed=51), f)
    return data, val_yaml


def train_argv(data, val_yaml, models, expname, extra=()):
    return ["--g_funit", str(FUNIT), "--cs", str(CS), "--loss_cs", str(LOSS_CS), "--batch_size", str(BATCH), "--weight_MSE", "1",
            "--g_lr", "1e-3", "--epochs", "5", "--patience", "2", "--seed", "7", "--expname", expname, "--beta1", "0.75",
            "--reduce_lr_factor", "0.5", "--train_data", data, "--test_reserve", "0", "--validation_set_yaml", val_yaml,
            "--models_dpath", models, "--g_network", "UtNet"] + list(extra)


def test_nn_train_end_to_end(dev, tmp_path):
    from nind_denoise_amd import nn_common, nn_train
    from nind_denoise_amd.validation import ValidationSet, validate
    data, val_yaml = make_tree(str(tmp_path))
    models = str(tmp_path / "models")
    assert nn_train.main(train_argv(data, val_yaml, models, "run")) == 0
    run = os.path.join(models, "run")
    for name in ("train.log", "config.yaml", "trainres.json"):
        assert os.path.isfile(os.path.join(run, name)), name
    with open(os.path.join(run, "config.yaml")) as f:
        conf = yaml.safe_load(f)
    assert conf["cs"] == CS and conf["loss_cs"] == LOSS_CS and conf["seed"] == 7 and conf["test_reserve"] == []
    with open(os.path.join(run, "trainres.json")) as f:
        res = json.load(f)
    assert {"0", "1", "2", "3", "4", "best_epoch", "best_val"} <= set(res)
    assert set(res["0"]) == {"validation_loss"}
    for e in "1234":
        assert {"validation_loss", "train_weighted_loss", "gen_lr"} <= set(res[e]), e
        assert res[e]["gen_lr"] in (1e-3, 5e-4, 2.5e-4, 1.25e-4)          # the rate in use: g_lr times a power of the factor
    assert set(res["best_epoch"]) == set(res["best_val"]) == {"validation_loss", "train_weighted_loss", "gen_lr"}
    best = res["best_epoch"]["validation_loss"]
    assert res["best_val"]["validation_loss"] == res[str(best)]["validation_loss"] == min(res[str(e)]["validation_loss"] for e in range(5))

    # the checkpoints left: the keepers of the last pruning (the best epochs as recorded after epoch 3) plus epoch 4
    def best_after(last):
        keep = set()
        for key in ("validation_loss", "train_weighted_loss", "gen_lr"):
            vals = [(res[str(e)][key], e) for e in range(last + 1) if key in res[str(e)]]
            keep.add(min(vals)[1])              # (the first epoch at a tie: a later value has to be lower to take over)
        return keep
    on_disk = {int(f.split("_")[1].split(".")[0]) for f in os.listdir(run) if f.startswith("generator_")}
    assert on_disk == (best_after(3) - {0}) | {4}, (on_disk, best_after(3))
    with open(os.path.join(run, "train.log")) as f:
        log = f.read()
    assert "Validation loss:" in log and "Epoch 4 summary:" in log and "delete_outperformed_models removed" in log

    # the run directory resolves to its best epoch, which loads into a fresh module with weights_only=True
    assert best in on_disk
    model = nn_common.Model.instantiate_model(model_path=run, network="UtNet", strparameters=f"funit={FUNIT}", keyword="generator")
    sd = torch.load(os.path.join(run, f"generator_{best}.pt"), map_location="cpu", weights_only=True)
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in model.state_dict().items())
    vs = ValidationSet(val_yaml, dev, CS)
    avg, _ = validate(model, vs, {"MSE": 1.0}, LOSS_CS, batch_size=32)
    assert avg == res[str(best)]["validation_loss"]

    # it learns.  The same 16 updates (4 epochs of 16 groups at batch 4) with the float64 oracle and torch autograd on the CPU,
    # from this seed's initial weights and on this tree (tools/oracle_nn_train.py; its crops are numpy's draws, not the pool's):
    # validation loss 0.005390 before, 0.000137 after, a factor 39.  On the GPU: GPU_FIGURES
    first, last = res["0"]["validation_loss"], res["4"]["validation_loss"]
    print(f"validation loss: epoch 0 {first:.6f}, epoch 4 {last:.6f}; all {[res[str(e)]['validation_loss'] for e in range(5)]}")
    assert last < first

    # the same seed: the same results file and the same last checkpoint, bit for bit
    assert nn_train.main(train_argv(data, val_yaml, models, "again")) == 0
    again = os.path.join(models, "again")
    with open(os.path.join(again, "trainres.json"), "rb") as f1, open(os.path.join(run, "trainres.json"), "rb") as f2:
        assert f1.read() == f2.read()
    with open(os.path.join(again, "generator_4.pt"), "rb") as f1, open(os.path.join(run, "generator_4.pt"), "rb") as f2:
        assert f1.read() == f2.read()

    # resuming from the run directory starts from its best epoch: the first validation is that epoch's recorded loss
    assert nn_train.main(train_argv(data, val_yaml, models, "resumed", ["--g_model_path", run, "--start_epoch", "5", "--epochs", "7"])) == 0
    with open(os.path.join(models, "resumed", "trainres.json")) as f:
        res2 = json.load(f)
    assert res2["0"]["validation_loss"] == res[str(best)]["validation_loss"]
    assert {"5", "6"} <= set(res2) and not {"1", "2", "3", "4"} & set(res2)
    assert os.path.isfile(os.path.join(models, "resumed", "generator_6.pt"))
