#!/usr/bin/env python3
"""UNet training step on one MI355X at the reference's training shape (configs/train_conf_unet.yaml: cs 220, batch 20, loss_cs 161,
MS-SSIM, lr 3e-4, beta1 0.5), one process, device events, median of interleaved rounds after a warm-up of every leg:

    learn             train.UNetTrainer.learn: nd_unet_train_forward + nd_criteria_grad + nd_unet_train_backward + nd_adam_step
    eval_fwd_bwd      the eval-mode module under autograd (running statistics), forward + backward with dx and every parameter gradient:
                      what the library could do before it had batch statistics -- no loss, no optimiser
    train_fwd_bwd     the trainer's two halves alone on the same output gradient: the like-for-like partner of eval_fwd_bwd
    torch_learn       the same train-mode step in plain torch ops on ROCm: F.conv2d / F.batch_norm(training=True) / ... under autograd
                      and torch.optim.Adam(amsgrad=True); the loss gradient comes from nd_criteria_grad in both (torch has no MS-SSIM)

    python tools/bench_unet_train.py [--out profiles/unet_train.json] [--rounds 3]
    python tools/bench_unet_train.py --leg learn --iters 5          # one leg alone, for `rocprofv3 --kernel-trace --stats -- ...`
    python tools/bench_unet_train.py --kernel-stats DIR_OR_CSV ...  # fold that trace into the JSON: the BatchNorm kernels' share of
                                                                    # kernel time and their achieved GB/s against algorithmic bytes
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

from nind_denoise_amd import _lib, synth, validation  # noqa: E402
from nind_denoise_amd.networks.ThirdPartyNets import UNet  # noqa: E402
from nind_denoise_amd.train import UNetTrainer  # noqa: E402

# (level, channels) of the 18 Conv3 + BatchNorm + ReLU layers, in forward order
BN_LAYERS = [(0, 64)] * 2 + [(1, 128)] * 2 + [(2, 256)] * 2 + [(3, 512)] * 2 + [(4, 512)] * 2 + [(3, 256)] * 2 + [(2, 128)] * 2 + \
            [(1, 64)] * 2 + [(0, 64)] * 2
# 16-byte plane elements (4 channels of one pixel) each kernel reads + writes per element of a layer: z | z, a | g, a, z | g, a, z, g
TOUCHES = {"k_bn_stats1": 1, "k_bn_apply": 2, "k_bn_bwd_red1": 3, "k_bn_bwd_apply": 4}
TINY = ("k_bn_stats2", "k_bn_bwd_red2")      # one workgroup per 4 channels over the partials: no HBM traffic to speak of
HBM_STREAM_GBS = 6300.0                      # what a streaming kernel reaches on this part (float4 copy)


def algorithmic_bytes(h, w, batch):
    """{kernel: bytes one training step moves}, from the shapes alone."""
    elems = sum((c // 4) * batch * (h >> lvl) * (w >> lvl) for lvl, c in BN_LAYERS)
    return {k: 16 * n * elems for k, n in TOUCHES.items()}


def torch_graph(sd, x):
    """UNet.forward in train() mode with plain torch ops; the running statistics in sd move in place."""
    def dconv(p, t):
        for k in (0, 3):
            t = F.conv2d(t, sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"], padding=1)
            t = F.relu(F.batch_norm(t, sd[f"{p}.{k + 1}.running_mean"], sd[f"{p}.{k + 1}.running_var"], sd[f"{p}.{k + 1}.weight"],
                                    sd[f"{p}.{k + 1}.bias"], training=True, momentum=0.1, eps=1e-5))
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


def kernel_rows(path):
    """[(name, total ns, calls)] of a rocprofv3 --kernel-trace --stats run: its *kernel_stats.csv, or the `kernels` view of its
    *_results.db (the default output format of newer releases)."""
    csvs = [path] if path.endswith(".csv") else sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    dbs = [path] if path.endswith(".db") else sorted(glob.glob(os.path.join(path, "**", "*_results.db"), recursive=True))
    if csvs:
        with open(csvs[-1], newline="") as f:
            return [(r["Name"], float(r["TotalDurationNs"]), int(r["Calls"])) for r in csv.DictReader(f)]
    if dbs:
        import sqlite3
        return sqlite3.connect(dbs[-1]).execute("select name, sum(duration), count(*) from kernels group by name").fetchall()
    raise SystemExit(f"no kernel_stats.csv and no _results.db under {path}")


def batchnorm_kernels(path, h, w, batch):
    """Share of kernel time and achieved GB/s of the BatchNorm kernels in a trace of `--leg learn`."""
    rows = kernel_rows(path)
    total = sum(ns for _, ns, _ in rows)
    need = algorithmic_bytes(h, w, batch)
    per = {}
    for name, ns, calls in rows:
        base = name.replace("(anonymous namespace)::", "")      # the kernels have internal linkage
        for k in tuple(TOUCHES) + TINY:
            if base == k or base.startswith(k + "("):
                e = per.setdefault(k, {"ns": 0.0, "calls": 0})
                e["ns"] += ns
                e["calls"] += calls
    out = {}
    for k, e in per.items():
        steps = e["calls"] / len(BN_LAYERS)
        o = {"share_of_kernel_time": round(e["ns"] / total, 5), "calls": e["calls"], "ms_per_step": round(e["ns"] / steps / 1e6, 4)}
        if k in need:
            gbs = need[k] * steps / e["ns"]
            o.update(algorithmic_bytes_per_step=need[k], achieved_GBs=round(gbs, 1), share_of_hbm_stream_rate=round(gbs / HBM_STREAM_GBS, 3))
        out[k] = o
    top = sorted(rows, key=lambda r: -r[1])[:8]
    return {"share_of_kernel_time": round(sum(e["ns"] for e in per.values()) / total, 5), "kernels": out,
            "top": [[round(ns / total, 4), n[:60]] for n, ns, _ in top]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cs", type=int, default=220)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--loss-cs", type=int, default=161)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=3, help="calls per timed sample")
    ap.add_argument("--leg", default=None, help="run this leg alone, untimed (for a profiler)")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cs, batch = args.cs, args.batch
    trace = batchnorm_kernels(args.kernel_stats, cs, cs, batch) if args.kernel_stats else None
    if not torch.cuda.is_available():
        raise SystemExit("bench_unet_train: no GPU (this measures the MI355X path; there is no fallback)")
    dev = torch.device("cuda:0")
    weights = {"MSSSIM": 1.0}
    sd = synth.make_unet_state_dict(3)
    g = torch.Generator().manual_seed(1)
    x = torch.rand(batch, 3, cs, cs, generator=g).to(dev)
    clean = torch.rand(batch, 3, cs, cs, generator=g).to(dev)
    gy = (torch.rand(batch, 3, cs, cs, generator=g) - 0.5).to(dev)

    tnet = UNet()
    tnet.load_state_dict(sd)
    trainer = UNetTrainer(tnet, lr=3e-4, beta1=0.5, weights=weights, device=dev, loss_cs=args.loss_cs)
    enet = UNet()
    enet.load_state_dict(sd)
    enet = enet.eval().to(dev)
    tsd = {k: v.to(dev).requires_grad_(k.endswith((".weight", ".bias"))) for k, v in sd.items() if v.is_floating_point()}
    opt = torch.optim.Adam([v for v in tsd.values() if v.requires_grad], lr=3e-4, betas=(0.5, 0.999), amsgrad=True)

    def learn():
        trainer.learn(x, clean)

    def train_fwd_bwd():
        trainer.forward(x)
        trainer.backward(gy, want_dx=True)

    def eval_fwd_bwd():
        enet.zero_grad(set_to_none=True)
        xin = x.clone().requires_grad_()
        enet(xin).backward(gy)

    def torch_learn():
        opt.zero_grad(set_to_none=True)
        y = torch_graph(tsd, x)
        y.backward(validation.criteria_grad(y.detach(), clean, weights, args.loss_cs)[1])
        opt.step()

    legs = {"learn": learn, "train_fwd_bwd": train_fwd_bwd, "eval_fwd_bwd": eval_fwd_bwd, "torch_learn": torch_learn}
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
    lib = _lib.load()
    out = {
        "what": "tools/bench_unet_train.py on one MI355X: one UNet training step on batch statistics at the reference's training shape, "
                "against the eval-mode forward + backward with every gradient and against the same step in plain torch ops on ROCm; one "
                "process, device events, median of interleaved rounds",
        "device": torch.cuda.get_device_name(0), "cs": cs, "batch": batch, "loss_cs": args.loss_cs, "loss": weights,
        "rounds": args.rounds, "iters_per_sample": args.iters,
        "ms": {k: round(v, 3) for k, v in ms.items()},
        "samples_ms": {k: [round(s, 3) for s in v] for k, v in samples.items()},
        "crops_per_s": round(batch / ms["learn"] * 1e3, 1),
        "train_over_eval_fwd_bwd": round(ms["train_fwd_bwd"] / ms["eval_fwd_bwd"], 3),
        "torch_over_hip_learn": round(ms["torch_learn"] / ms["learn"], 3),
        "train_workspace_bytes": int(lib.nd_unet_train_workspace_bytes(cs, cs, batch)),
        "eval_grad_workspace_bytes": int(lib.nd_unet_grad_workspace_bytes(cs, cs, batch)),
        "batchnorm_algorithmic_bytes_per_step": algorithmic_bytes(cs, cs, batch),
    }
    if trace:
        out["batchnorm_kernels_learn_trace"] = trace
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
