#!/usr/bin/env python3
"""Crop-pool benchmark: what a training batch from the device-resident pool costs, and what it costs the training step.

    python tools/bench_crop_pool.py [--groups 1024] [--cs 184] [--batch 30] [--steps 20] [--out profiles/crop_pool.json]

One process measures, on one GPU:
  (a) ms per batch of `batch` x cs^2 pairs from a pool of 256 x 256 u8 pairs, exposure multiplier off and on: the launches alone
      (device events around `iters` calls of batch() on prepared draws) and draw() + batch() together (host clock around a loop that
      ends in a synchronise: the torch ops that fill the draw table are most of it);
  (b) UtNetTrainer.learn crops/s for UtNet(64) fed by a fresh pool batch every step against the same step fed by one resident
      batch (what tools/bench_train.py times), in alternating windows of `steps` steps;
  (c) the pool's resident bytes.
Images are seeded noise: the kernel's traffic does not depend on the picture."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nind_denoise_amd import synth  # noqa: E402
from nind_denoise_amd.crop_pool import CropPool  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.train import UtNetTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--cs", type=int, default=184)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--funit", type=int, default=64)
    ap.add_argument("--out", default=os.path.join("profiles", "crop_pool.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_crop_pool needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    pool = CropPool(dev, seed=1, cs=args.cs)
    t0 = time.perf_counter()
    for _ in range(args.groups):
        clean = rng.integers(0, 256, (3, args.side, args.side), dtype=np.uint8)
        pool.add_group([clean], [clean ^ rng.integers(0, 16, clean.shape, dtype=np.uint8)])
    pool.device_buffers()
    torch.cuda.synchronize()
    fill_s = time.perf_counter() - t0

    exposure = {"off": dict(), "on": dict(exp_mult_min=0.8, exp_mult_max=1.2)}
    res_a = {}
    for name, kw in exposure.items():
        prepared = [pool.draw(args.batch) for _ in range(16)]
        out = pool.batch(prepared[0], **kw)
        for d in prepared:                                       # warm-up: code objects, allocator
            pool.batch(d, out=out, **kw)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for i in range(args.iters):
            pool.batch(prepared[i % 16], out=out, **kw)
        ev[1].record()
        torch.cuda.synchronize()
        ms_launch = ev[0].elapsed_time(ev[1]) / args.iters
        t0 = time.perf_counter()
        for i in range(args.iters):
            pool.batch(pool.draw(args.batch), **kw)
        torch.cuda.synchronize()
        ms_all = 1e3 * (time.perf_counter() - t0) / args.iters
        res_a[name] = {"ms_per_batch_launches": round(ms_launch, 5), "ms_per_batch_draw_and_launches": round(ms_all, 5)}
    out_bytes = 2 * args.batch * 3 * args.cs * args.cs * 4
    in_bytes = 2 * args.batch * 3 * args.cs * args.cs

    net = UtNet(funit=args.funit)
    net.load_state_dict(synth.make_utnet_state_dict(args.funit, seed=123))
    tr = UtNetTrainer(net, lr=1e-4, beta1=0.75, device=dev, weights={"L1": 0.5, "MSE": 0.5})
    clean0, noisy0 = pool.batch(pool.draw(args.batch))

    def window(fresh):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if fresh:
                clean, noisy = pool.batch(pool.draw(args.batch))
                loss = tr.learn(noisy, clean)
            else:
                loss = tr.learn(noisy0, clean0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, float(loss.item())

    for _ in range(args.warmup):
        tr.learn(noisy0, clean0)
        tr.learn(*reversed(pool.batch(pool.draw(args.batch))))
    rates = {"resident": [], "pool": []}
    for _ in range(args.rounds):                                 # alternating windows: both see the same machine
        for name, fresh in (("resident", False), ("pool", True)):
            dt, loss = window(fresh)
            rates[name].append(round(args.batch * args.steps / dt, 2))
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    step_ms = 1e3 * args.batch / mean["resident"]
    result = {
        "device": torch.cuda.get_device_name(0),
        "config": {"groups": args.groups, "source": f"{args.side}x{args.side} u8 pairs", "cs": args.cs, "batch": args.batch,
                   "iters": args.iters, "steps": args.steps, "rounds": args.rounds, "funit": args.funit},
        "a_batch": dict(res_a, algorithmic_bytes_out=out_bytes, algorithmic_bytes_in=in_bytes),
        "b_train": {"crops_per_s_windows": rates, "crops_per_s_mean": {k: round(v, 2) for k, v in mean.items()},
                    "pool_over_resident": round(mean["pool"] / mean["resident"], 4), "ms_per_step_resident": round(step_ms, 3),
                    "batch_launches_share_of_step": round(res_a["on"]["ms_per_batch_launches"] / step_ms, 5),
                    "draw_and_launches_share_of_step": round(res_a["on"]["ms_per_batch_draw_and_launches"] / step_ms, 5),
                    "last_loss": loss},
        "c_pool": {"resident_bytes": pool.nbytes, "images": pool.n_images, "groups": pool.n_groups, "fill_and_upload_s": round(fill_s, 2)},
    }
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
