"""What should a short nn_train run learn?  The same kind of run on the CPU, in float64, with the oracle network
(oracle/networks.py), torch autograd and torch.optim.Adam(amsgrad): the validation loss before and after `--updates` updates.
It shares nothing with the HIP path but the module's initial weights (torch's default initialisation under --seed) and the file
readers; its crops are drawn by numpy, so it follows the same distribution of batches, not the same batches.  Used to choose the
synthetic data of tests/test_nn_train.py::test_nn_train_end_to_end (MSE only).

    python tools/oracle_nn_train.py --train_data <dir> --validation_set_yaml <yaml> --cs 104 --loss_cs 60 --updates 16
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nind_denoise_amd.crop_pool import CropPool  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.validation import ValidationSet  # noqa: E402
from oracle import networks as onet  # noqa: E402


def crop(t, loss_cs):
    y0, x0 = (t.shape[2] - loss_cs) // 2, (t.shape[3] - loss_cs) // 2
    return t[:, :, y0:y0 + loss_cs, x0:x0 + loss_cs]


def validation_loss(params, vs, loss_cs):
    with torch.no_grad():
        g = onet.utnet_forward(params, vs.noisy.double()).clip(0, 1)
        return ((crop(g, loss_cs) - crop(vs.clean.double(), loss_cs)) ** 2).mean((1, 2, 3)).mean().item()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--train_data", required=True)
    ap.add_argument("--validation_set_yaml", required=True)
    ap.add_argument("--cs", type=int, default=104)
    ap.add_argument("--loss_cs", type=int, default=60)
    ap.add_argument("--g_funit", type=int, default=8)
    ap.add_argument("--batch_size", type=int, default=4)
    ap.add_argument("--g_lr", type=float, default=1e-3)
    ap.add_argument("--beta1", type=float, default=0.75)
    ap.add_argument("--updates", type=int, default=16)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    torch.manual_seed(args.seed)
    params = {k: v.detach().double().requires_grad_() for k, v in UtNet(funit=args.g_funit).state_dict().items()}
    pool = CropPool.from_directories([args.train_data], device="cpu", cs=args.cs)
    vs = ValidationSet(args.validation_set_yaml, "cpu", args.cs)
    opt = torch.optim.Adam(list(params.values()), lr=args.g_lr, betas=(args.beta1, 0.999), amsgrad=True)
    rng = np.random.default_rng(args.seed)
    before = validation_loss(params, vs, args.loss_cs)
    print(f"validation loss before: {before:.6f}")
    order = []
    for step in range(args.updates):
        if len(order) < args.batch_size:
            order = list(rng.permutation(pool.n_groups))
        groups, order = order[:args.batch_size], order[args.batch_size:]
        clean, noisy = [], []
        for g in groups:
            cl, no, h, w = pool.group(int(g))
            y0, x0 = rng.integers(0, h - args.cs + 1), rng.integers(0, w - args.cs + 1)
            nrot, f1, f2 = rng.integers(0, 4), rng.integers(0, 2), rng.integers(0, 2)
            for ids, dst in ((cl, clean), (no, noisy)):
                img = pool.image(ids[rng.integers(0, len(ids))]).astype(np.float64) / 255
                img = np.rot90(img[:, y0:y0 + args.cs, x0:x0 + args.cs], nrot, (1, 2))
                img = np.flip(img, 1) if f1 else img
                img = np.flip(img, 2) if f2 else img
                dst.append(torch.from_numpy(np.ascontiguousarray(img)))
        clean, noisy = torch.stack(clean), torch.stack(noisy)
        opt.zero_grad()
        g = onet.utnet_forward(params, noisy).clip(0, 1)
        loss = F.mse_loss(crop(g, args.loss_cs), crop(clean, args.loss_cs))
        loss.backward()
        opt.step()
        print(f"update {step + 1}: train loss {loss.item():.6f}")
    after = validation_loss(params, vs, args.loss_cs)
    print(f"validation loss after {args.updates} updates: {after:.6f}  (before / after = {before / after:.2f})")


if __name__ == "__main__":
    main()
