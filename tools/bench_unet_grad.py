#!/usr/bin/env python3
"""UNet under autograd in eval mode, measured on one MI355X at the reference's UNet tile (440 x 440, batch 8):

    inference forward                        nd_unet_forward (the module with an input that needs no gradient)
    autograd forward + backward, dx only     nd_unet_grad_forward + nd_unet_grad_backward with every parameter frozen
    autograd forward + backward, dx + params the same with every parameter's gradient
    the same three in plain torch ops        the eval-mode graph restated with F.conv2d / F.batch_norm / ... on ROCm, same process

and forward + backward through frame_grad.denoise_frame on one 6000 x 4000 frame at cs 440 / ucs 320 / ol 6.  Device events, median
of interleaved rounds after a warm-up of every leg.  Expectation from FLOP parity (data gradient ~ forward, weight gradient ~
forward): ~2x the whole-tile forward for dx only, ~3x with parameter gradients; the JSON holds both ratios beside it.

    python tools/bench_unet_grad.py [--out profiles/unet_grad.json] [--rounds 3] [--no-frame]
    python tools/bench_unet_grad.py --leg dx_params --iters 3        # one leg alone, for `rocprofv3 --kernel-trace --stats -- ...`
    python tools/bench_unet_grad.py --kernel-stats DIR_OR_CSV ...    # fold that trace's share of the small kernels into the JSON
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from nind_denoise_amd import frame_grad, pipeline, synth  # noqa: E402
from nind_denoise_amd.networks.ThirdPartyNets import UNet  # noqa: E402

# kernels this path adds to the conv / wgrad / pool machinery it shares with UtNet
SMALL_KERNELS = ("k_unet_fold_w", "k_relu_bwd_post", "k_unet_head", "k_unet_head_bwd", "k_unet_input_grad", "k_bn_fold_bwd")


def torch_graph(sd, x):
    """UNet.forward in eval mode with plain torch ops (networks/ThirdPartyNets.py of the reference)."""
    def dconv(p, t):
        for k in (0, 3):
            t = F.conv2d(t, sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"], padding=1)
            t = F.relu(F.batch_norm(t, sd[f"{p}.{k + 1}.running_mean"], sd[f"{p}.{k + 1}.running_var"], sd[f"{p}.{k + 1}.weight"],
                                    sd[f"{p}.{k + 1}.bias"], training=False, eps=1e-5))
        return t
    skips = [dconv("inc.conv.conv", x)]
    for n in (1, 2, 3, 4):
        skips.append(dconv(f"down{n}.mpconv.1.conv", F.max_pool2d(skips[-1], 2)))
    t = skips[4]
    for n, skip in zip((1, 2, 3, 4), skips[3::-1]):
        up = F.conv_transpose2d(t, sd[f"up{n}.up.weight"], sd[f"up{n}.up.bias"], stride=2)
        up = F.pad(up, (0, skip.size(3) - up.size(3), 0, skip.size(2) - up.size(2)))
        t = dconv(f"up{n}.conv.conv", torch.cat([skip, up], dim=1))
    return torch.sigmoid(F.conv2d(t, sd["outc.conv.weight"], sd["outc.conv.bias"]))


def small_kernel_share(path):
    """Share of kernel time in SMALL_KERNELS from a rocprofv3 --kernel-trace --stats run: its *kernel_stats.csv, or the `kernels` view
    of its *_results.db (the default output format of newer releases)."""
    csvs = [path] if path.endswith(".csv") else sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    dbs = [path] if path.endswith(".db") else sorted(glob.glob(os.path.join(path, "**", "*_results.db"), recursive=True))
    if csvs:
        with open(csvs[-1], newline="") as f:
            rows = [(r["Name"], float(r["TotalDurationNs"])) for r in csv.DictReader(f)]
        src = csvs[-1]
    elif dbs:
        import sqlite3
        rows = sqlite3.connect(dbs[-1]).execute("select name, sum(duration) from kernels group by name").fetchall()
        src = dbs[-1]
    else:
        raise SystemExit(f"no kernel_stats.csv and no _results.db under {path}")
    total = sum(ns for _, ns in rows)
    per = {}
    for name, ns in rows:
        for k in SMALL_KERNELS:
            if name == k or name.startswith(k + "("):
                per[k] = per.get(k, 0.0) + ns
    top = sorted(rows, key=lambda r: -r[1])[:8]
    return {"share": round(sum(per.values()) / total, 5),
            "share_by_kernel": {k: round(v / total, 5) for k, v in per.items()},
            "top": [[round(ns / total, 4), n[:60]] for n, ns in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cs", type=int, default=440)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3, help="calls per timed sample")
    ap.add_argument("--leg", default=None, help="run this leg alone, untimed (for a profiler)")
    ap.add_argument("--no-frame", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    trace = small_kernel_share(args.kernel_stats) if args.kernel_stats else None
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet_grad: no GPU (this measures the MI355X path; there is no fallback)")
    dev = torch.device("cuda:0")
    sd = synth.make_unet_state_dict(3)
    net = UNet()
    net.load_state_dict(sd)
    net = net.eval().to(dev)
    tsd = {k: v.to(dev).requires_grad_(k.endswith((".weight", ".bias"))) for k, v in sd.items() if v.is_floating_point()}
    tparams = [v for v in tsd.values() if v.requires_grad]
    g = torch.Generator().manual_seed(1)
    x = torch.rand(args.batch, 3, args.cs, args.cs, generator=g).to(dev)
    gy = (torch.rand(args.batch, 3, args.cs, args.cs, generator=g) - 0.5).to(dev)

    def hip(params):
        def run():
            net.requires_grad_(params)
            net.zero_grad(set_to_none=True)
            xin = x.clone().requires_grad_()
            net(xin).backward(gy)
        return run

    def plain(params):
        def run():
            for p in tparams:
                p.requires_grad_(params)
                p.grad = None
            xin = x.clone().requires_grad_()
            torch_graph(tsd, xin).backward(gy)
        return run

    def hip_fwd():
        with torch.no_grad():
            net(x)

    def plain_fwd():
        with torch.no_grad():
            torch_graph(tsd, x)

    legs = {"forward": hip_fwd, "dx": hip(False), "dx_params": hip(True),
            "torch_forward": plain_fwd, "torch_dx": plain(False), "torch_dx_params": plain(True)}
    if args.leg:
        for _ in range(1 + args.iters):
            legs[args.leg]()
        torch.cuda.synchronize()
        return

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / n

    for fn in legs.values():          # warm-up: code objects, workspaces, MIOpen's algorithm search
        fn()
        fn()
    samples = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            samples[k].append(timed(fn, args.iters))
    ms = {k: statistics.median(v) for k, v in samples.items()}
    # same numbers?  (the HIP path against the plain-torch graph, fp32 both; random weights and input, nothing cleared: ReLUs and pool
    # maxima that fall the other way in the two fp32 forward passes move dx locally by a few percent, a weight gradient by far less)
    net.requires_grad_(True)
    net.zero_grad(set_to_none=True)
    xin = x.clone().requires_grad_()
    net(xin).backward(gy)
    xt = x.clone().requires_grad_()
    for p in tparams:
        p.requires_grad_(True)
        p.grad = None
    torch_graph(tsd, xt).backward(gy)
    # dx element by element, relative to max |dx|: a flipped ReLU or pool maximum is a local event, so the largest deviation says little;
    # the median and the share of elements past 1e-4 say whether the two gradients are the same function
    e = ((xin.grad - xt.grad).abs() / xt.grad.abs().max()).flatten()
    wg, wt = net.inc.conv.conv[0].weight.grad, tsd["inc.conv.conv.0.weight"].grad
    agree = {"dx_max": e.max().item(), "dx_median": e.median().item(), "dx_share_over_1e-4": (e > 1e-4).float().mean().item(),
             "inc.conv.conv.0.weight_max": ((wg - wt).abs().max() / wt.abs().max()).item()}
    out = {
        "what": "tools/bench_unet_grad.py on one MI355X: UNet in eval mode under autograd at the reference's tile, against its inference "
                "forward and against the same graph in plain torch ops on ROCm, one process, device events, median of interleaved rounds",
        "device": torch.cuda.get_device_name(0), "cs": args.cs, "batch": args.batch, "rounds": args.rounds, "iters_per_sample": args.iters,
        "grad_workspace_bytes": int(net._grad_state(dev).ws.numel()),
        "ms": {k: round(v, 3) for k, v in ms.items()},
        "samples_ms": {k: [round(s, 3) for s in v] for k, v in samples.items()},
        "expected_ratio_dx": 2.0, "ratio_dx": round(ms["dx"] / ms["forward"], 3),
        "expected_ratio_dx_params": 3.0, "ratio_dx_params": round(ms["dx_params"] / ms["forward"], 3),
        "torch_over_hip": {k: round(ms["torch_" + k] / ms[k], 3) for k in ("forward", "dx", "dx_params")},
        "hip_vs_torch_max_rel": agree,
    }
    if not args.no_frame:
        W, H, cs, ucs, ol = 6000, 4000, 440, 320, 6
        img = torch.from_numpy(synth.make_frame(W, H, seed=5)).to(dev)
        gc = (torch.rand(3, H, W, generator=g) - 0.5).to(dev)

        def frame(params):
            def run():
                net.requires_grad_(params)
                net.zero_grad(set_to_none=True)
                im = img.clone().requires_grad_()
                frame_grad.denoise_frame(net, im, cs, ucs, ol, batch=args.batch).backward(gc)
            return run

        def frame_fwd():
            pipeline.denoise_frame(net, img, cs, ucs, ol, batch=args.batch)

        flegs = {"frame_forward": frame_fwd, "frame_dx": frame(False), "frame_dx_params": frame(True)}
        for fn in flegs.values():
            fn()
        fs = {k: [] for k in flegs}
        for _ in range(2):
            for k, fn in flegs.items():
                fs[k].append(timed(fn, 1) / 1e3)
        out["frame"] = {"size": [W, H], "cs": cs, "ucs": ucs, "ol": ol, "tiles": pipeline.tile_count(W, H, cs, ucs, ol),
                        "seconds": {k: round(statistics.median(v), 4) for k, v in fs.items()},
                        "samples_s": {k: [round(s, 4) for s in v] for k, v in fs.items()}}
    if trace:
        out["small_kernels_dx_params_trace"] = trace
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
