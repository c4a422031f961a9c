#!/usr/bin/env python3
"""Quality-score benchmark: what scoring every pair of the resident crop pool costs, and what a quality bar costs the epoch loop.

    python tools/bench_pool_quality.py [--groups 1024] [--side 256] [--score_batch 64] [--out profiles/pool_quality.json]

One process measures, on one GPU and on the 1024-group u8 pool of tools/bench_crop_pool.py (one pair per group):
  (a) CropPool.score_pairs: pairs/s of the whole pass (host clock around the call and a synchronise), the split between the
      nd_pool_fetch launches and the nd_ms_ssim launches of one pass (device events around each kind, run back to back), and the
      same pairs scored one at a time with a host read per pair (a fetch of one pair, pt_losses.MS_SSIM_loss, .item());
  (b) crops/s of nn_train.train_epoch for UtNet(64), as tools/bench_nn_train.py (a) times it, without a bar and with a bar that
      every pair passes, in alternating windows: the cost of the filtered pick.
Images are seeded noise: none of the kernels' traffic depends on the picture."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nind_denoise_amd import _lib, nn_train, synth  # noqa: E402
from nind_denoise_amd.common.libs import pt_losses  # noqa: E402
from nind_denoise_amd.crop_pool import CropPool  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.train import UtNetTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--score_batch", type=int, default=64)
    ap.add_argument("--cs", type=int, default=184)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--funit", type=int, default=64)
    ap.add_argument("--out", default=os.path.join("profiles", "pool_quality.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_pool_quality needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    pool = CropPool(dev, seed=1, cs=args.cs)
    for _ in range(args.groups):
        clean = rng.integers(0, 256, (3, args.side, args.side), dtype=np.uint8)
        pool.add_group([clean], [clean ^ rng.integers(0, 16, clean.shape, dtype=np.uint8)])
    buf, table = pool.device_buffers()
    pairs = pool.pair_table()
    n_pairs, h, w, sb = len(pairs), args.side, args.side, args.score_batch

    # ---- (a) the scoring pass
    scores = pool.score_pairs(sb)                               # warm-up: code objects, allocator
    torch.cuda.synchronize()
    pass_s = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        again = pool.score_pairs(sb)
        torch.cuda.synchronize()
        pass_s.append(time.perf_counter() - t0)
    assert torch.equal(again, scores) and bool(torch.isfinite(scores).all())

    lib, sp = _lib.load(), _lib.stream_ptr(dev)
    idx = torch.from_numpy(np.ascontiguousarray(pairs[:, 1:].T.astype(np.int32))).to(dev)
    x = torch.empty(2, sb, 3, h, w, device=dev)
    ws = torch.empty(lib.nd_ssim_workspace_bytes(sb, 3, h, w), dtype=torch.uint8, device=dev)
    out = torch.empty(n_pairs, device=dev)
    chunks = [(k, min(sb, n_pairs - k)) for k in range(0, n_pairs, sb)]

    def fetches():
        for k, m in chunks:
            for side in (0, 1):
                _lib.check(lib.nd_pool_fetch(buf.data_ptr(), buf.numel(), table.data_ptr(), table.shape[0], idx[side, k:k + m].data_ptr(),
                                             m, h, w, x[side].data_ptr(), sp), "nd_pool_fetch")

    def scorings():
        for k, m in chunks:
            _lib.check(lib.nd_ms_ssim(x[0].data_ptr(), x[1].data_ptr(), m, 3, h, w, out[k:k + m].data_ptr(), ws.data_ptr(), ws.numel(), sp),
                       "nd_ms_ssim")

    split = {"nd_pool_fetch_ms": [], "nd_ms_ssim_ms": []}
    for r in range(args.rounds + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        fetches()
        ev[1].record()
        scorings()
        ev[2].record()
        torch.cuda.synchronize()
        if r:                                                    # round 0 warms up
            split["nd_pool_fetch_ms"].append(round(ev[0].elapsed_time(ev[1]), 4))
            split["nd_ms_ssim_ms"].append(round(ev[1].elapsed_time(ev[2]), 4))
    fetch_ms, score_ms = (sum(v) / len(v) for v in (split["nd_pool_fetch_ms"], split["nd_ms_ssim_ms"]))

    msssim = pt_losses.MS_SSIM_loss()
    one = torch.empty(2, 1, 3, h, w, device=dev)

    def one_by_one():
        vals = []
        for k in range(n_pairs):
            for side in (0, 1):
                _lib.check(lib.nd_pool_fetch(buf.data_ptr(), buf.numel(), table.data_ptr(), table.shape[0], idx[side, k:k + 1].data_ptr(),
                                             1, h, w, one[side].data_ptr(), sp), "nd_pool_fetch")
            vals.append(1 - msssim(one[0], one[1]).item())
        return vals
    one_s = []
    for r in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vals = one_by_one()
        if r:
            one_s.append(time.perf_counter() - t0)
    worst = max(abs(a - b) for a, b in zip(vals, scores.tolist()))
    mean_pass = sum(pass_s) / len(pass_s)

    # ---- (b) the epoch loop without a bar and under a bar that every pair passes
    net = UtNet(funit=args.funit)
    net.load_state_dict(synth.make_utnet_state_dict(args.funit, seed=123))
    tr = UtNetTrainer(net, lr=1e-4, beta1=0.75, device=dev, weights={"MSSSIM": 1.0}, loss_cs=args.cs)
    steps = args.groups // args.batch
    losses = torch.zeros(steps, device=dev)

    def window(bar):
        pool.set_min_quality(-1.0 if bar else None)
        assert pool.n_active_groups == args.groups
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = nn_train.train_epoch(pool, tr, args.batch, losses, None, 0.85, 1.15, log_interval=50, log=lambda it, loss: None)
        losses[:n].double().mean().item()
        return args.batch * n / (time.perf_counter() - t0)

    for _ in range(args.warmup):
        tr.learn(*reversed(pool.batch(pool.draw(args.batch), exp_mult_min=0.85, exp_mult_max=1.15)))
    rates = {"no_bar": [], "bar_passing_every_pair": []}
    for _ in range(args.rounds):
        for name, bar in (("no_bar", False), ("bar_passing_every_pair", True)):
            rates[name].append(round(window(bar), 2))
    pool.set_min_quality(None)
    mean_rate = {k: sum(v) / len(v) for k, v in rates.items()}

    result = {
        "device": torch.cuda.get_device_name(0),
        "config": {"groups": args.groups, "pairs": n_pairs, "source": f"{h}x{w} u8 pairs", "score_batch": sb, "rounds": args.rounds,
                   "cs": args.cs, "batch": args.batch, "funit": args.funit, "weights": {"MSSSIM": 1.0}, "exp_mult": [0.85, 1.15]},
        "a_scoring": {"pass_s": [round(v, 5) for v in pass_s], "pairs_per_s": round(n_pairs / mean_pass, 1),
                      "device_ms_per_pass": dict(split, nd_pool_fetch_mean=round(fetch_ms, 4), nd_ms_ssim_mean=round(score_ms, 4),
                                                 fetch_share=round(fetch_ms / (fetch_ms + score_ms), 4)),
                      "fetch_bytes_read": 2 * n_pairs * 3 * h * w, "fetch_bytes_written": 2 * n_pairs * 3 * h * w * 4,
                      "one_pair_at_a_time_s": [round(v, 4) for v in one_s], "one_pair_at_a_time_pairs_per_s": round(n_pairs / one_s[0], 1),
                      "batched_over_one_at_a_time": round(one_s[0] / mean_pass, 2), "worst_score_difference_between_the_two": worst,
                      "score_min_max": [float(scores.min()), float(scores.max())]},
        "b_epoch_loop": {"crops_per_s_windows": rates, "crops_per_s_mean": {k: round(v, 2) for k, v in mean_rate.items()},
                         "bar_over_no_bar": round(mean_rate["bar_passing_every_pair"] / mean_rate["no_bar"], 4)},
    }
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
