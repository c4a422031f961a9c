#!/usr/bin/env python3
"""SHA-256 digests of what the training step, the criteria and the scores compute, to compare two revisions bit for bit.

    python tools/step_digest.py [--out digests.json]

Every case runs twice on fixed seeds: two equal lines per case mean the revision is deterministic there, and equal files from two
revisions mean they compute the same bits.  Step cases (funit 8): the output, the loss bits and the flat gradient buffer of
UtNetTrainer.forward_backward; then validation.criteria, and nd_ssim / nd_ms_ssim / nd_ssim_padded on one pair.  UNet cases, on
weights with planted BatchNorm (gamma = 0 and gamma < 0 channels), each with the library's four byte counts for its shape: eval mode
under autograd (y, dx, every parameter gradient), UNetTrainer (y, loss, grads, flat with its running statistics; dx of backward(gy,
want_dx=True)), and three learn steps of both trainers, plain and guarded (flat, m, v, vmax, guard_state)."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nind_denoise_amd import _lib, synth  # noqa: E402
from nind_denoise_amd.common.libs import pt_losses  # noqa: E402
from nind_denoise_amd.libs import pytorch_ssim  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.networks.ThirdPartyNets import UNet  # noqa: E402
from nind_denoise_amd.train import UNetTrainer, UtNetTrainer  # noqa: E402
from nind_denoise_amd.validation import criteria  # noqa: E402

STEP_CASES = [  # name, h, w, batch, loss_cs, weights, activation
    ("mse-104", 104, 104, 3, None, {"MSE": 1.0}, "PReLU"),
    ("l1-mse-120-cs88", 120, 120, 2, 88, {"L1": 0.4, "MSE": 0.6}, "PReLU"),
    ("ssim-136-cs101", 136, 136, 2, 101, {"SSIM": 1.0}, "PReLU"),
    ("msssim-l1-184x168-cs161", 184, 168, 2, 161, {"MSSSIM": 0.6, "L1": 0.4}, "PReLU"),
    ("hardswish-l1-ssim-104-cs77", 104, 104, 2, 77, {"L1": 0.5, "SSIM": 0.5}, "Hardswish"),
]
UNET_EVAL_SHAPES = [(3, 33, 47), (2, 32, 32)]
UNET_EVAL_MODES = [  # name, find_noise, split_k, parameters frozen
    ("plain", False, True, False), ("find-noise", True, True, False), ("no-split-k", False, False, False), ("frozen", False, True, True)]
UNET_TRAIN_SHAPES = [(3, 33, 47), (8, 16, 16), (2, 64, 16)]      # (8, 16, 16): a 1x1 bottom level
GUARDS = [("plain", {}), ("guarded", {"max_grad_norm": 1e-6, "skip_nonfinite": True})]      # 1e-6: every step clips


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def pair(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, 3, h, w, generator=g)
    return (-0.2 + 1.4 * (t + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)), t      # y beyond [0, 1], t inside


def unet_sd():
    """synth's UNet weights with every BatchNorm planted as tests/test_unet_grad.py plants them: negative and zero weights."""
    sd = synth.make_unet_state_dict(3)
    for k in list(sd):
        if k.endswith(".running_var"):
            w = k[:-len("running_var")] + "weight"
            sd[w][0::7] *= -1.0
            sd[w][3::11] = 0.0
    return sd


def unet_bytes(b, h, w):
    lib = _lib.load()
    return [int(lib.nd_unet_grad_workspace_bytes(h, w, b)), int(lib.nd_unet_train_workspace_bytes(h, w, b)),
            int(lib.nd_unet_grad_blob_bytes()), int(lib.nd_unet_train_blob_bytes())]


def unet_cases(dev, res):
    for b, h, w in UNET_EVAL_SHAPES:
        x, gy = pair(b, h, w, seed=h + w)
        for name, find_noise, split_k, frozen in UNET_EVAL_MODES:
            net = UNet(find_noise=find_noise)
            net.load_state_dict(unet_sd())
            net = net.eval().to(dev).requires_grad_(not frozen)
            net.split_k = split_k
            for rep in range(2):
                net.zero_grad(set_to_none=True)
                xin = x.to(dev).requires_grad_()
                y = net(xin)
                y.backward(gy.to(dev))
                grads = [p.grad for p in net.parameters() if p.grad is not None]
                res[f"unet eval {name} {b}x{h}x{w} run {rep}"] = {"y": sha(y), "dx": sha(xin.grad), "grads": sha(*grads) if grads else None,
                                                                 "bytes": unet_bytes(b, h, w)}
    for i, (b, h, w) in enumerate(UNET_TRAIN_SHAPES):
        x, t = pair(b, h, w, seed=h + w)
        for rep in range(2):
            net = UNet()      # a trainer of its own per run: the forward moves the running statistics in flat
            net.load_state_dict(unet_sd())
            tr = UNetTrainer(net, device=dev)
            y, loss = tr.forward_backward(x.clip(0, 1), t)
            r = {"y": sha(y), "loss": sha(loss), "grads": sha(tr.grads), "flat": sha(tr.flat), "bytes": unet_bytes(b, h, w)}
            if i == 0:
                r["backward dx"] = sha(tr.backward(x - t, want_dx=True), tr.grads)
            res[f"unet train {b}x{h}x{w} run {rep}"] = r
    for gname, guard in GUARDS:
        for rep in range(2):
            unet, utnet = UNet(), UtNet(funit=8)
            unet.load_state_dict(unet_sd())
            utnet.load_state_dict(synth.make_utnet_state_dict(funit=8, seed=31, gain=1.8), strict=True)
            for kind, tr, shape in (("unet", UNetTrainer(unet, device=dev, **guard), (2, 32, 32)),
                                    ("utnet", UtNetTrainer(utnet, device=dev, **guard), (2, 104, 104))):
                x, t = pair(*shape, seed=9)
                for _ in range(3):
                    tr.learn(x.clip(0, 1), t)
                state = [tr.flat, tr.m, tr.v, tr.vmax] + ([tr.guard_state] if tr.guarded else [])
                if tr.guarded:
                    assert tr.guard_state[2].item() < 1.0 and tr.guard_state[3].item() == 1.0, tr.guard_state
                res[f"optimizer {kind} {gname} run {rep}"] = sha(*state)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {}
    for name, h, w, batch, loss_cs, weights, act in STEP_CASES:
        net = UtNet(funit=8, activation=act)
        net.load_state_dict(synth.make_utnet_state_dict(funit=8, seed=31, gain=1.8, activation=act), strict=True)
        tr = UtNetTrainer(net, device=dev, weights=weights, loss_cs=loss_cs)
        x, t = pair(batch, h, w, seed=len(name))
        for rep in range(2):
            y, loss = tr.forward_backward(x.clip(0, 1), t)
            res[f"step {name} run {rep}"] = {"y": sha(y), "loss": sha(loss), "grads": sha(tr.grads)}
    y, t = (v.to(dev) for v in pair(2, 184, 168, seed=5))
    for rep in range(2):
        for cs, weights, also in ((0, {"L1": 0.3, "MSE": 0.2, "SSIM": 0.5}, ()), (161, {"MSSSIM": 1.0}, ("MSE",))):
            res[f"criteria cs{cs} run {rep}"] = sha(*criteria(y, t, weights, cs, also).values())
        g = y.clip(0, 1)
        res[f"scores run {rep}"] = {"ssim": sha(pt_losses.SSIM_loss()(g, t)), "ms_ssim": sha(pt_losses.MS_SSIM_loss()(g, t)),
                                    "ssim_padded": sha(pytorch_ssim.ssim(g, t, 11, size_average=False)), "mse": sha(pt_losses.mse(g, t))}
    unet_cases(dev, res)
    torch.cuda.synchronize()
    for k, v in res.items():
        print(k, json.dumps(v))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
