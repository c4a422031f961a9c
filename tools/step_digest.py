#!/usr/bin/env python3
"""SHA-256 digests of what the training step, the criteria and the scores compute, to compare two revisions bit for bit.

    python tools/step_digest.py [--out digests.json]

Every case runs twice on fixed seeds: two equal lines per case mean the revision is deterministic there, and equal files from two
revisions mean they compute the same bits.  Step cases (funit 8): the output, the loss bits and the flat gradient buffer of
UtNetTrainer.forward_backward; then validation.criteria, and nd_ssim / nd_ms_ssim / nd_ssim_padded on one pair."""
import argparse
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nind_denoise_amd import synth  # noqa: E402
from nind_denoise_amd.common.libs import pt_losses  # noqa: E402
from nind_denoise_amd.libs import pytorch_ssim  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.train import UtNetTrainer  # noqa: E402
from nind_denoise_amd.validation import criteria  # noqa: E402

STEP_CASES = [  # name, h, w, batch, loss_cs, weights, activation
    ("mse-104", 104, 104, 3, None, {"MSE": 1.0}, "PReLU"),
    ("l1-mse-120-cs88", 120, 120, 2, 88, {"L1": 0.4, "MSE": 0.6}, "PReLU"),
    ("ssim-136-cs101", 136, 136, 2, 101, {"SSIM": 1.0}, "PReLU"),
    ("msssim-l1-184x168-cs161", 184, 168, 2, 161, {"MSSSIM": 0.6, "L1": 0.4}, "PReLU"),
    ("hardswish-l1-ssim-104-cs77", 104, 104, 2, 77, {"L1": 0.5, "SSIM": 0.5}, "Hardswish"),
]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def pair(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, 3, h, w, generator=g)
    return (-0.2 + 1.4 * (t + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)), t      # y beyond [0, 1], t inside


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
    torch.cuda.synchronize()
    for k, v in res.items():
        print(k, json.dumps(v))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
