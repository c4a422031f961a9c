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
Images are seeded noise: the kernel's traffic does not depend on the picture.

    python tools/bench_crop_pool.py --windows [--frame 3000x2000] [--ds_stride 192] [--build_frames 24] [--out profiles/crop_pool_windows.json]

--windows: the same data as frames.  Seeded-noise frame pairs are cut on the cropper's grid (crop_pool.crop_grid, --side / --ds_stride)
until there are `groups` crops; one pool holds the frames and takes the crops as windows (nd_crop_batch_windows), the other holds
the cut-out crops (nd_crop_batch).  (a) and (b) are then measured for both, in alternating rounds, and (d) writes `build_frames`
frames as a PNG dataset of sets of one clean and one noisy image, crops it into a second tree, and times CropPool.from_full_size
on the first against CropPool.from_directories on the second (host-bound: decode and upload), with the bytes each holds.

    python tools/bench_crop_pool.py --validation [--val_pairs 300] [--frame 3000x2000] [--build_frames 24] [--out profiles/val_full_size.json]

--validation, alone: the dataset of (d), `val_pairs` pairs picked from it as tools.pick_validation_set picks them, and the seconds
to build the validation set from the full-size images (ValidationSet.from_full_size) against building it from the crop files."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nind_denoise_amd import synth  # noqa: E402
from nind_denoise_amd.common.libs import imgcodec  # noqa: E402
from nind_denoise_amd.crop_pool import CropPool, crop_grid  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.train import UtNetTrainer  # noqa: E402


def time_batches(pool, args, kw):
    """(ms per batch: the launches alone, ms per batch: draw() + batch())"""
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
    return ms_launch, 1e3 * (time.perf_counter() - t0) / args.iters


def write_png_dataset(tmp, args):
    """(dsdir, cropped tree, grid): args.build_frames frames as a PNG dataset of sets of one clean and one noisy image under tmp, and the
    tree a cropper writes for it at args.side / args.ds_stride"""
    fw, fh = (int(v) for v in args.frame.split("x"))
    rng = np.random.default_rng(2)
    dsdir = os.path.join(tmp, "SYN")
    cropped = os.path.join(tmp, "cropped", f"SYN_{args.side}_{args.ds_stride}")
    grid = crop_grid(fw, fh, args.side, args.ds_stride)
    for k in range(args.build_frames // 2):
        clean = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
        for iso, img in (("ISO100", clean), ("ISO6400", clean ^ rng.integers(0, 16, clean.shape, dtype=np.uint8))):
            os.makedirs(os.path.join(dsdir, f"set{k}"), exist_ok=True)
            os.makedirs(os.path.join(cropped, f"set{k}", iso), exist_ok=True)
            imgcodec.write_png(os.path.join(dsdir, f"set{k}", f"SYN_set{k}_{iso}.png"), img)
            for xc, yc, xb, yb in grid:
                imgcodec.write_png(os.path.join(cropped, f"set{k}", iso, f"SYN_set{k}_{iso}_{xc}_{yc}_{args.ds_stride}.png"),
                                   np.ascontiguousarray(img[yb:yb + args.side, xb:xb + args.side]))
    return dsdir, cropped, grid


def time_validation(args, dev):
    """--validation: ValidationSet.from_full_size on the PNG dataset of (d) against ValidationSet on its cropped tree, for
    args.val_pairs pairs that tools.pick_validation_set's candidates give under one seed.  Host-bound (decode, slicing, one upload);
    the files were just written, so both read from the page cache; alternating runs, the median of args.rounds."""
    import random
    from nind_denoise_amd.tools.pick_validation_set import candidates_of_full_size
    from nind_denoise_amd.validation import ValidationSet
    fw, fh = (int(v) for v in args.frame.split("x"))
    with tempfile.TemporaryDirectory() as tmp:
        dsdir, cropped, grid = write_png_dataset(tmp, args)
        candidates, _ = candidates_of_full_size([dsdir], [cropped], args.side, args.ds_stride, sorted(os.listdir(dsdir)))
        pairs = random.Random(3).sample(candidates, args.val_pairs)
        legs = {"from_crop_files": lambda: ValidationSet(pairs, dev, args.cs),
                "from_full_size": lambda: ValidationSet.from_full_size(pairs, dsdir, args.side, args.ds_stride, dev, args.cs)}
        secs, sets = {name: [] for name in legs}, {}
        for _ in range(args.rounds):
            for name, make in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sets[name] = make()
                torch.cuda.synchronize()
                secs[name].append(round(time.perf_counter() - t0, 3))
        same = bool(torch.equal(sets["from_crop_files"].clean, sets["from_full_size"].clean)
                    and torch.equal(sets["from_crop_files"].noisy, sets["from_full_size"].noisy))
        res = {"device": torch.cuda.get_device_name(0),
               "dataset": f"{args.build_frames} frames of {fw}x{fh} u8 PNG at {args.side}/{args.ds_stride}: {len(grid)} crops per frame, "
                          f"{len(candidates)} candidate pairs",
               "pairs": len(pairs), "cs": args.cs, "rounds": args.rounds, "tensors_equal": same,
               "from_crop_files": {"build_s": secs["from_crop_files"], "build_s_median": statistics.median(secs["from_crop_files"]),
                                   "files_decoded": 2 * len(pairs)},
               "from_full_size": {"build_s": secs["from_full_size"], "build_s_median": statistics.median(secs["from_full_size"]),
                                  "files_decoded": sets["from_full_size"].n_full_size_images}}
        res["full_size_over_crop_files"] = round(res["from_full_size"]["build_s_median"] / res["from_crop_files"]["build_s_median"], 3)
    return res


def time_builds(args, dev):
    """(d): from_full_size on a PNG dataset of args.build_frames frames against from_directories on the same dataset, cropped"""
    fw, fh = (int(v) for v in args.frame.split("x"))
    with tempfile.TemporaryDirectory() as tmp:
        dsdir, cropped, grid = write_png_dataset(tmp, args)
        res = {}
        for name, make in (("from_directories", lambda: CropPool.from_directories(cropped, device=dev)),
                           ("from_full_size", lambda: CropPool.from_full_size(dsdir, ds_cs=args.side, ds_stride=args.ds_stride, device=dev))):
            secs = []
            for _ in range(2):                                   # the second pass reads from the page cache, like the first of the other
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pool = make()
                pool.device_buffers()
                torch.cuda.synchronize()
                secs.append(round(time.perf_counter() - t0, 3))
            res[name] = {"build_and_upload_s": secs, "resident_bytes": pool.nbytes, "groups": pool.n_groups, "images": pool.n_images,
                         "files_read": pool.n_frames if pool.windowed else pool.n_images}
        res["bytes_dense_over_windows"] = round(res["from_directories"]["resident_bytes"] / res["from_full_size"]["resident_bytes"], 4)
        res["dataset"] = f"{args.build_frames} frames of {fw}x{fh} u8 at {args.side}/{args.ds_stride}: {len(grid)} crops per frame"
    return res


def window_pools(args, dev):
    """{"dense": a pool of the cut-out crops, "windows": a pool of the frames with the same crops as windows}: args.groups groups of
    args.side x args.side u8 pairs on the cropper's grid (args.ds_stride) over seeded-noise frame pairs (args.frame, WxH)"""
    fw, fh = (int(v) for v in args.frame.split("x"))
    grid = crop_grid(fw, fh, args.side, args.ds_stride)
    if not grid:
        sys.exit(f"a {fw}x{fh} frame yields no {args.side}/{args.ds_stride} crop")
    rng = np.random.default_rng(0)
    pools = {"dense": CropPool(dev, seed=1, cs=args.cs), "windows": CropPool(dev, seed=1, cs=args.cs)}
    while pools["dense"].n_groups < args.groups:
        clean = rng.integers(0, 256, (3, fh, fw), dtype=np.uint8)
        noisy = clean ^ rng.integers(0, 16, clean.shape, dtype=np.uint8)
        fc, fn = pools["windows"].add_frame(clean), pools["windows"].add_frame(noisy)
        for _, _, xb, yb in grid:
            pools["windows"].add_window_group([fc], [fn], yb, xb, args.side, args.side)
            pools["dense"].add_group([clean[:, yb:yb + args.side, xb:xb + args.side]], [noisy[:, yb:yb + args.side, xb:xb + args.side]])
    for pool in pools.values():
        pool.keep_groups(args.groups)
        pool.device_buffers()
    return pools


def main_windows(args, dev):
    fw, fh = (int(v) for v in args.frame.split("x"))
    pools = window_pools(args, dev)
    # a third pool, for (a) alone, that tells the window form from the layout: windows that are whole side x side frames, so the
    # window kernel and table on the dense pool's layout (rows `side` samples apart, not a frame's width)
    rng = np.random.default_rng(3)
    whole = CropPool(dev, seed=1, cs=args.cs)
    for _ in range(args.groups):
        clean = rng.integers(0, 256, (3, args.side, args.side), dtype=np.uint8)
        frames = [whole.add_frame(clean), whole.add_frame(clean ^ rng.integers(0, 16, clean.shape, dtype=np.uint8))]
        whole.add_window_group(frames[:1], frames[1:], 0, 0, args.side, args.side)
    whole.device_buffers()
    pools["windows_whole_frames"] = whole
    exposure = {"off": dict(), "on": dict(exp_mult_min=0.8, exp_mult_max=1.2)}
    runs ={name: {e: {"launches": [], "draw_and_launches": []} for e in exposure} for name in pools}
    for _ in range(args.rounds):                                 # alternating: both see the same machine
        for name, pool in pools.items():
            for e, kw in exposure.items():
                ms_launch, ms_all = time_batches(pool, args, kw)
                runs[name][e]["launches"].append(round(ms_launch, 5))
                runs[name][e]["draw_and_launches"].append(round(ms_all, 5))
    res_a = {name: {e: {"ms_per_batch_launches": r["launches"], "ms_per_batch_launches_median": statistics.median(r["launches"]),
                        "ms_per_batch_draw_and_launches_median": statistics.median(r["draw_and_launches"])}
                    for e, r in by_e.items()} for name, by_e in runs.items()}
    for e in exposure:
        res_a[f"windows_over_dense_{e}"] = round(res_a["windows"][e]["ms_per_batch_launches_median"]
                                                 / res_a["dense"][e]["ms_per_batch_launches_median"], 4)

    net = UtNet(funit=args.funit)
    net.load_state_dict(synth.make_utnet_state_dict(args.funit, seed=123))
    tr = UtNetTrainer(net, lr=1e-4, beta1=0.75, device=dev, weights={"L1": 0.5, "MSE": 0.5})
    clean0, noisy0 = pools["dense"].batch(pools["dense"].draw(args.batch))

    def window(pool):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            if pool is not None:
                clean, noisy = pool.batch(pool.draw(args.batch))
                tr.learn(noisy, clean)
            else:
                tr.learn(noisy0, clean0)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for _ in range(args.warmup):
        tr.learn(noisy0, clean0)
        for pool in pools.values():
            tr.learn(*reversed(pool.batch(pool.draw(args.batch))))
    rates = {"resident": [], "dense": [], "windows": []}
    for _ in range(args.rounds):
        for name in rates:
            rates[name].append(round(args.batch * args.steps / window(pools.get(name)), 2))
    mean = {k: sum(v) / len(v) for k, v in rates.items()}
    result = {
        "device": torch.cuda.get_device_name(0),
        "config": {"groups": args.groups, "source": f"{args.side}x{args.side} u8 windows of {fw}x{fh} frames at stride {args.ds_stride}",
                   "cs": args.cs, "batch": args.batch, "iters": args.iters, "steps": args.steps, "rounds": args.rounds, "funit": args.funit},
        "a_batch": res_a,
        "b_train": {"crops_per_s_windows": rates, "crops_per_s_mean": {k: round(v, 2) for k, v in mean.items()},
                    "dense_over_resident": round(mean["dense"] / mean["resident"], 4),
                    "windows_over_resident": round(mean["windows"] / mean["resident"], 4)},
        "c_pool": {name: {"resident_bytes": pool.nbytes, "images": pool.n_images, "groups": pool.n_groups, "frames": pool.n_frames}
                   for name, pool in pools.items()},
    }
    result["c_pool"]["bytes_dense_over_windows"] = round(pools["dense"].nbytes / pools["windows"].nbytes, 4)
    if args.build_frames:
        result["d_build"] = time_builds(args, dev)
    return result


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
    ap.add_argument("--out", default=None, help="default: profiles/crop_pool.json, with --windows profiles/crop_pool_windows.json, with --validation profiles/val_full_size.json")
    ap.add_argument("--windows", action="store_true", help="the same data as frames: windows against the cut-out crops")
    ap.add_argument("--frame", default="3000x2000", help="--windows: WxH of a frame")
    ap.add_argument("--ds_stride", type=int, default=192, help="--windows: the cropper's stride (its crop size is --side)")
    ap.add_argument("--build_frames", type=int, default=24, help="--windows: frames of the PNG dataset whose pool builds are timed (0: skip)")
    ap.add_argument("--validation", action="store_true", help="time the validation set from the full-size images against the one from crop files, alone")
    ap.add_argument("--val_pairs", type=int, default=300, help="--validation: picked pairs")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join("profiles", "val_full_size.json" if args.validation else
                                "crop_pool_windows.json" if args.windows else "crop_pool.json")
    if not torch.cuda.is_available():
        sys.exit("bench_crop_pool needs a GPU")
    dev = torch.device("cuda", 0)
    if args.validation or args.windows:
        result = time_validation(args, dev) if args.validation else main_windows(args, dev)
        print(json.dumps(result))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
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
        ms_launch, ms_all = time_batches(pool, args, kw)
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
