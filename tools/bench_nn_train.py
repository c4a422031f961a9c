#!/usr/bin/env python3
"""nn_train benchmark: what the epoch loop, the validation pass and the per-sample criteria cost on one GPU.

    python tools/bench_nn_train.py [--groups 1024] [--cs 184] [--batch 30] [--pairs 300] [--out profiles/nn_train.json]

One process measures:
  (a) crops/s of nn_train.train_epoch (pool epoch + batch + learn + the loss kept on the device) for UtNet(64) on a synthetic
      pool, against UtNetTrainer.learn on one resident batch, in alternating windows;
  (b) validation.validate over `pairs` pairs at cs^2 in batches, against the pass the parent revision could run: one image at a
      time through the module, torch / pt_losses criteria on the clipped output, one .item() per image;
  (c) ms per nd_criteria call at batch x 3 x cs^2, with and without MS-SSIM (device events around `iters` calls).
Images are seeded noise: none of the kernels' traffic depends on the picture.

    python tools/bench_nn_train.py --gpus N [--dist_backend nccl|gloo] --out profiles/<name>.json

runs the data-parallel leg instead: this process stays off the GPU and starts N ranks of this file (nn_train.launch); every rank
times (a)'s epoch loop at `batch` crops per rank with the bucketed gradient mean, and validation.validate sharded over the ranks.
With more ranks than GPUs the ranks share cards over gloo: a rehearsal, not a scaling figure (profiles/nn_train_dp.json).

    python tools/bench_nn_train.py --g_clip_norm X [--skip_nonfinite_steps] --out profiles/train_guard.json

runs the guard leg instead: (a)'s epoch loop with a plain trainer and with a guarded one in alternating windows, nd_grad_guard and
the two optimizer launches alone (device events; the guard's share of the HBM rate from the bytes it reads), and the seconds one
train_state.pt takes to write."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nind_denoise_amd import nn_train, synth  # noqa: E402
from nind_denoise_amd.common.libs import pt_losses  # noqa: E402
from nind_denoise_amd.crop_pool import CropPool  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.train import UtNetTrainer  # noqa: E402
from nind_denoise_amd.validation import ValidationSet, criteria, validate  # noqa: E402


def data_parallel_leg(args, ranked):
    """One rank of --gpus N (started by nn_train.launch, below): the epoch loop with the bucketed gradient mean and the sharded
    validation pass, on the pool, network and shapes of the one-process legs.  Every rank times its own windows; rank 0 gathers
    them and writes the result.  With more ranks than GPUs (gloo) the ranks share cards and gradients are staged through the
    host: a rehearsal of the code path, which prices that staging and the sharing, not a scaling figure."""
    import torch.distributed as tdist
    rank, local_rank, world = ranked
    group = nn_train.init_rank(rank, local_rank, world, args.dist_backend)
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        rng = np.random.default_rng(0)
        pool = CropPool(dev, seed=1, cs=args.cs)                 # every rank: the same groups and generator state
        for _ in range(args.groups):
            clean = rng.integers(0, 256, (3, args.side, args.side), dtype=np.uint8)
            pool.add_group([clean], [clean ^ rng.integers(0, 16, clean.shape, dtype=np.uint8)])
        pool.device_buffers()
        steps = args.groups // args.batch // world
        net = UtNet(funit=args.funit)
        net.load_state_dict(synth.make_utnet_state_dict(args.funit, seed=123))
        weights = {"MSSSIM": 1.0}
        tr = UtNetTrainer(net, lr=1e-4, beta1=0.75, device=dev, weights=weights, loss_cs=args.cs, process_group=group)
        losses = torch.zeros(steps, device=dev)
        for _ in range(args.warmup):
            tr.learn(*reversed(pool.batch(pool.draw(args.batch), exp_mult_min=0.85, exp_mult_max=1.15)))
        rates = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            tdist.barrier(group)
            t0 = time.perf_counter()
            n = nn_train.train_epoch(pool, tr, args.batch, losses, None, 0.85, 1.15, rank, world, log_interval=50, log=lambda it, loss: None)
            means, count = nn_train.combine_epoch_sums([losses[:n].double().sum().item()], n, group)
            rates.append(round(args.batch * n / (time.perf_counter() - t0), 2))
        nn_train.check_agreement(tr.flat, group, 0)
        vclean = torch.rand(args.pairs, 3, args.cs, args.cs, generator=torch.Generator().manual_seed(2))
        vs = ValidationSet.from_tensors(vclean, (vclean + 0.05 * torch.randn(vclean.shape, generator=torch.Generator().manual_seed(3))).clip(0, 1), dev)
        val_s = []
        for r in range(args.rounds + 1):
            torch.cuda.synchronize()
            tdist.barrier(group)
            t0 = time.perf_counter()
            val_loss = validate(net, vs, weights, args.cs, batch_size=args.val_batch, group=group)[0]
            torch.cuda.synchronize()
            if r:                                                # round 0 warms up
                val_s.append(round(time.perf_counter() - t0, 4))
        gathered = [None] * world
        tdist.all_gather_object(gathered, {"crops_per_s_windows": rates, "validation_s": val_s}, group=group)
        if rank == 0:
            per_rank = [sum(g["crops_per_s_windows"]) / len(g["crops_per_s_windows"]) for g in gathered]
            result = {
                "device": torch.cuda.get_device_name(dev), "world": world, "backend": tdist.get_backend(group),
                "gpus_visible": torch.cuda.device_count(), "rehearsal_on_shared_gpus": world > torch.cuda.device_count(),
                "config": {"groups": args.groups, "source": f"{args.side}x{args.side} u8 pairs", "cs": args.cs, "batch_per_rank": args.batch,
                           "steps_per_rank_and_epoch": steps, "rounds": args.rounds, "funit": args.funit, "weights": weights,
                           "exp_mult": [0.85, 1.15], "pairs": args.pairs, "val_batch": args.val_batch},
                "epoch_loop": {"per_rank": gathered, "crops_per_s_per_rank_mean": [round(v, 2) for v in per_rank],
                               "crops_per_s_total": round(sum(per_rank), 2), "last_epoch_mean_loss": means[0], "steps_counted": count},
                "validation": {"sharded_s_rank0": val_s, "mean_s": round(sum(val_s) / len(val_s), 4), "loss": val_loss},
            }
            print(json.dumps(result))
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    finally:
        tdist.destroy_process_group()


def guard_leg(args, dev, pool, steps):
    """--g_clip_norm: what the guarded step costs in the epoch loop and on its own, and what the state file costs per epoch"""
    import tempfile
    from nind_denoise_amd import _lib
    weights = {"MSSSIM": 1.0}
    trainers = {}
    for name, kw in (("plain", {}), ("guarded", {"max_grad_norm": args.g_clip_norm, "skip_nonfinite": args.skip_nonfinite_steps})):
        net = UtNet(funit=args.funit)
        net.load_state_dict(synth.make_utnet_state_dict(args.funit, seed=123))
        trainers[name] = UtNetTrainer(net, lr=1e-4, beta1=0.75, device=dev, weights=weights, loss_cs=args.cs, **kw)
    losses = torch.zeros(steps, device=dev)
    guard_log = torch.zeros(steps, 4, dtype=torch.float64, device=dev)

    def window(name):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        extra = {"guard_log": guard_log} if name == "guarded" else {}
        n = nn_train.train_epoch(pool, trainers[name], args.batch, losses, None, 0.85, 1.15, log_interval=50, log=lambda it, loss: None, **extra)
        mean = losses[:n].double().mean().item()                # the epoch's one synchronisation
        summary = nn_train.guard_summary(guard_log[:n].cpu()) if extra else None
        return time.perf_counter() - t0, n, mean, summary
    for tr in trainers.values():
        for _ in range(args.warmup):
            tr.learn(*reversed(pool.batch(pool.draw(args.batch), exp_mult_min=0.85, exp_mult_max=1.15)))
    rates, summary = {"plain": [], "guarded": []}, None
    for _ in range(args.rounds):                                 # alternating windows: both see the same machine
        for name in rates:
            dt, n, mean, got = window(name)
            rates[name].append(round(args.batch * n / dt, 2))
            summary = got or summary
    median = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}

    # the launches alone
    tr, lib, sp = trainers["guarded"], _lib.load(), _lib.stream_ptr(dev)
    adam = (tr.flat.data_ptr(), tr.grads.data_ptr(), tr.m.data_ptr(), tr.v.data_ptr(), tr.vmax.data_ptr(), tr.flat.numel(), 0.0, 0.75,
            0.999, 1e-8, 10, 1)                                  # lr 0: the parameters stay where they are
    calls = {
        "nd_grad_guard": lambda: lib.nd_grad_guard(tr.grads.data_ptr(), tr.grads.numel(), args.g_clip_norm, int(args.skip_nonfinite_steps),
                                                   tr.guard_state.data_ptr(), tr._guard_ws.data_ptr(), tr._guard_ws.numel(), sp),
        "nd_adam_step": lambda: lib.nd_adam_step(*adam, sp),
        "nd_adam_step_guarded": lambda: lib.nd_adam_step_guarded(*adam, tr.guard_state.data_ptr(), sp),
    }
    ms = {}
    for name, call in calls.items():
        for _ in range(10):
            _lib.check(call(), name)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(args.iters):
            call()
        ev[1].record()
        torch.cuda.synchronize()
        ms[name] = round(ev[0].elapsed_time(ev[1]) / args.iters, 5)
    grad_bytes = tr.grads.numel() * 4
    # the guard's pass from HBM: copies of the gradient buffer taken in turn, together over four times the 256 MiB Infinity Cache, so
    # no call finds its buffer cached (measuring: a rate from a cache-resident buffer is no HBM rate)
    copies = [tr.grads.clone() for _ in range(max(2, -(-4 * 256 * 2 ** 20 // grad_bytes)))]

    def rotated(k):
        g = copies[k % len(copies)]
        return lib.nd_grad_guard(g.data_ptr(), g.numel(), args.g_clip_norm, int(args.skip_nonfinite_steps), tr.guard_state.data_ptr(),
                                 tr._guard_ws.data_ptr(), tr._guard_ws.numel(), sp)
    for k in range(len(copies)):
        _lib.check(rotated(k), "nd_grad_guard")
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for k in range(args.iters):
        rotated(k)
    ev[1].record()
    torch.cuda.synchronize()
    hbm_ms = ev[0].elapsed_time(ev[1]) / args.iters
    del copies

    # the state file
    write_s = []
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            path = nn_train.save_train_state(tmp, {"format": nn_train.STATE_FORMAT, "epoch": 1, "trainer": tr.state_dict(),
                                                   "pool_rng_state": pool.rng_state()})
            write_s.append(round(time.perf_counter() - t0, 4))
        state_bytes = os.path.getsize(path)
    result = {
        "device": torch.cuda.get_device_name(0),
        "config": {"groups": args.groups, "source": f"{args.side}x{args.side} u8 pairs", "cs": args.cs, "batch": args.batch,
                   "steps_per_epoch": steps, "rounds": args.rounds, "funit": args.funit, "weights": weights, "exp_mult": [0.85, 1.15],
                   "g_clip_norm": args.g_clip_norm, "skip_nonfinite_steps": args.skip_nonfinite_steps, "iters": args.iters},
        "epoch_loop": {"crops_per_s_windows": rates, "crops_per_s_median": median,
                       "guarded_over_plain": round(median["guarded"] / median["plain"], 4),
                       "last_guarded_epoch": dict(zip(("applied", "skipped", "clipped", "grad_norm_mean", "grad_norm_max"), summary))},
        "launches_ms_per_call": dict(ms, gradient_bytes=grad_bytes,
                                     nd_grad_guard_GB_per_s=round(grad_bytes / ms["nd_grad_guard"] / 1e6, 1),
                                     note="back-to-back calls on one buffer of %.0f MB: smaller than the 256 MB last-level cache, so the "
                                          "rate is an upper bound on what a step sees" % (grad_bytes / 1e6),
                                     nd_grad_guard_from_hbm={
                                         "ms_per_call": round(hbm_ms, 5), "GB_per_s": round(grad_bytes / hbm_ms / 1e6, 1),
                                         "share_of_8000_GB_per_s_spec": round(grad_bytes / hbm_ms / 1e6 / 8000, 3),
                                         "share_of_6290_GB_per_s_float4_copy": round(grad_bytes / hbm_ms / 1e6 / 6290, 3),
                                         "how": "buffers of %.0f MB taken in turn, over 1 GiB together (4 x the 256 MiB cache); both "
                                                "launches of the call timed" % (grad_bytes / 1e6)}),
        "state_file": {"write_s": write_s, "bytes": state_bytes},
    }
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1, help="> 1: the data-parallel leg alone, one fresh process per rank")
    ap.add_argument("--dist_backend", choices=("nccl", "gloo"))
    ap.add_argument("--groups", type=int, default=1024)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--cs", type=int, default=184)
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--val_batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--funit", type=int, default=64)
    ap.add_argument("--out", default=os.path.join("profiles", "nn_train.json"))
    ap.add_argument("--windows", action="store_true", help="a third leg: the epoch loop fed from a pool of frames and windows holding the same crops (tools/bench_crop_pool.py --windows)")
    ap.add_argument("--frame", default="3000x2000", help="--windows: WxH of a frame")
    ap.add_argument("--ds_stride", type=int, default=192, help="--windows: the cropper's stride (its crop size is --side)")
    ap.add_argument("--g_clip_norm", type=float, help="the guard leg alone: the epoch loop with and without nn_train's --g_clip_norm")
    ap.add_argument("--skip_nonfinite_steps", action="store_true", help="with --g_clip_norm: the guarded trainer also skips non-finite steps")
    args = ap.parse_args()
    ranked = nn_train.world_from_environment()
    if ranked is not None:
        return data_parallel_leg(args, ranked)
    if args.gpus > 1:        # this process stays off the GPU: the ranks are fresh children running this file
        return sys.exit(nn_train.launch(sys.argv[1:], args.gpus, command=[sys.executable, os.path.abspath(__file__)]))
    if not torch.cuda.is_available():
        sys.exit("bench_nn_train needs a GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    wpool = None
    if args.windows:            # the same crops twice: cut out (pool), and as windows into their frames (wpool)
        from bench_crop_pool import window_pools
        pools = window_pools(args, dev)
        pool, wpool = pools["dense"], pools["windows"]
    else:
        pool = CropPool(dev, seed=1, cs=args.cs)
        for _ in range(args.groups):
            clean = rng.integers(0, 256, (3, args.side, args.side), dtype=np.uint8)
            pool.add_group([clean], [clean ^ rng.integers(0, 16, clean.shape, dtype=np.uint8)])
        pool.device_buffers()
    steps = args.groups // args.batch
    if args.g_clip_norm is not None:
        return guard_leg(args, dev, pool, steps)

    # ---- (a) the epoch loop against the resident step
    net = UtNet(funit=args.funit)
    net.load_state_dict(synth.make_utnet_state_dict(args.funit, seed=123))
    weights = {"MSSSIM": 1.0}
    tr = UtNetTrainer(net, lr=1e-4, beta1=0.75, device=dev, weights=weights, loss_cs=args.cs)
    clean0, noisy0 = pool.batch(pool.draw(args.batch))
    losses = torch.zeros(steps, device=dev)

    def window(loop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if loop:
            n = nn_train.train_epoch(loop, tr, args.batch, losses, None, 0.85, 1.15, log_interval=50, log=lambda it, loss: None)
            mean = losses[:n].double().mean().item()            # the epoch's one synchronisation
        else:
            for k in range(steps):
                losses[k] = tr.learn(noisy0, clean0)[0]
            n, mean = steps, losses.double().mean().item()
        return time.perf_counter() - t0, n, mean

    for _ in range(args.warmup):
        tr.learn(noisy0, clean0)
        tr.learn(*reversed(pool.batch(pool.draw(args.batch), exp_mult_min=0.85, exp_mult_max=1.15)))
    legs = [("resident", None), ("epoch_loop", pool)] + ([("epoch_loop_windows", wpool)] if wpool is not None else [])
    rates = {name: [] for name, _ in legs}
    for _ in range(args.rounds):                                 # alternating windows: all see the same machine
        for name, loop in legs:
            dt, n, mean = window(loop)
            rates[name].append(round(args.batch * n / dt, 2))
    mean_rate = {k: sum(v) / len(v) for k, v in rates.items()}

    # ---- (b) validation: batched against one image at a time
    vclean = torch.rand(args.pairs, 3, args.cs, args.cs, generator=torch.Generator().manual_seed(2))
    vs = ValidationSet.from_tensors(vclean, (vclean + 0.05 * torch.randn(vclean.shape, generator=torch.Generator().manual_seed(3))).clip(0, 1), dev)
    msssim = pt_losses.MS_SSIM_loss()

    def one_by_one():
        net.eval()
        vals = []
        with torch.no_grad():
            for i in range(len(vs)):
                clean, noisy = vs[i]
                denoised = net(noisy.unsqueeze(0)).clip(0, 1)
                vals.append(msssim(denoised, clean.unsqueeze(0)).mean().item())
        net.train()
        return sum(vals) / len(vals)

    val = {"batched_s": [], "one_by_one_s": []}
    for r in range(args.rounds + 1):
        for name, fn in (("batched_s", lambda: validate(net, vs, weights, args.cs, batch_size=args.val_batch)[0]), ("one_by_one_s", one_by_one)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = fn()
            torch.cuda.synchronize()
            if r:                                                # round 0 warms both up
                val[name].append(round(time.perf_counter() - t0, 4))
            val[name.replace("_s", "_loss")] = loss
    vmean = {k: sum(v) / len(v) for k, v in val.items() if k.endswith("_s")}

    # ---- (c) the criteria launches alone
    y = torch.rand(args.batch, 3, args.cs, args.cs, device=dev) * 1.4 - 0.2
    t = torch.rand(args.batch, 3, args.cs, args.cs, device=dev)
    crit = {}
    for name, w in (("l1_mse", {"L1": 0.5, "MSE": 0.5}), ("ssim", {"SSIM": 1.0}), ("msssim", {"MSSSIM": 1.0}),
                    ("all_four", {"L1": 0.25, "MSE": 0.25, "SSIM": 0.25, "MSSSIM": 0.25})):
        for _ in range(10):
            criteria(y, t, w)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        for _ in range(args.iters):
            criteria(y, t, w)
        ev[1].record()
        torch.cuda.synchronize()
        crit[name] = round(ev[0].elapsed_time(ev[1]) / args.iters, 5)

    result = {
        "device": torch.cuda.get_device_name(0),
        "config": {"groups": args.groups, "source": f"{args.side}x{args.side} u8 pairs", "cs": args.cs, "batch": args.batch,
                   "steps_per_epoch": steps, "rounds": args.rounds, "funit": args.funit, "weights": weights, "exp_mult": [0.85, 1.15],
                   "pairs": args.pairs, "val_batch": args.val_batch, "iters": args.iters},
        "a_epoch": {"crops_per_s_windows": rates, "crops_per_s_mean": {k: round(v, 2) for k, v in mean_rate.items()},
                    "epoch_loop_over_resident": round(mean_rate["epoch_loop"] / mean_rate["resident"], 4),
                    "crop_pool_record": 0.9948, "last_epoch_mean_loss": mean},
        "b_validation": dict(val, mean_s={k: round(v, 4) for k, v in vmean.items()},
                             one_by_one_over_batched=round(vmean["one_by_one_s"] / vmean["batched_s"], 2)),
        "c_criteria_ms_per_call": dict(crit, bytes_read=2 * args.batch * 3 * args.cs * args.cs * 4),
    }
    if wpool is not None:
        result["config"]["source"] = f"{args.side}x{args.side} u8 crops of {args.frame} frames at stride {args.ds_stride}, cut out and as windows"
        result["a_epoch"]["epoch_loop_windows_over_resident"] = round(mean_rate["epoch_loop_windows"] / mean_rate["resident"], 4)
        result["a_epoch"]["epoch_loop_windows_over_epoch_loop"] = round(mean_rate["epoch_loop_windows"] / mean_rate["epoch_loop"], 4)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
