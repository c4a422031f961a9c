"""A/B of the fused frame loop: per-tile encoder (UtNet.share_encoder = False) against the shared encoder, alternating.

    python3 tools/ab_shared_encoder.py [--rounds 3] [--steps 5] [--only tile|level2|shared]

--only level2 (or --level2: a third mode between the two) shares levels 0-1 and keeps level 2 per tile (UtNet.share_level2 = False).

bench.py's flagship workload (fp32 G24: 6000x4000, cs 264 / ucs 200 / ol 64, UtNet(64), 256 tiles per launch), timed with CUDA
events around `steps` whole frames after one warm-up frame per mode.  Prints one JSON line per round and a summary; --only runs
one mode (for a profiler run of that mode alone)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nind_denoise_amd import pipeline, synth  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--only", choices=("tile", "level2", "shared"))
    ap.add_argument("--level2", action="store_true")
    a = ap.parse_args()
    W, H, cs, ucs, ol = 6000, 4000, 264, 200, 64
    dev = torch.device("cuda:0")
    net = UtNet(funit=64)
    net.load_state_dict(synth.make_utnet_state_dict(funit=64, seed=123))
    net = net.eval().to(dev)
    img = torch.from_numpy(synth.make_frame(W, H, seed=24)).to(dev)
    canvas = torch.zeros_like(img)
    modes = [a.only] if a.only else (["tile", "level2", "shared"] if a.level2 else ["tile", "shared"])

    def run(mode, steps):
        net.share_encoder = mode != "tile"
        net.share_level2 = mode != "level2"
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            canvas.zero_()
            pipeline.denoise_frame(net, img, cs, ucs, ol, batch=a.batch, canvas=canvas)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for m in modes:
        run(m, 1)
    res = {m: [] for m in modes}
    for r in range(a.rounds):
        for m in modes:
            ms = run(m, a.steps)
            res[m].append(ms)
            print(json.dumps({"round": r, "mode": m, "ms_per_frame": round(ms, 2), "mp_per_s": round(W * H / ms / 1e3, 2)}), flush=True)
    summary = {m: {"ms_per_frame": [round(x, 2) for x in v], "best_mp_per_s": round(W * H / min(v) / 1e3, 2)} for m, v in res.items()}
    if "tile" in res and "shared" in res:
        summary["speedup_median"] = round(sorted(res["tile"])[len(res["tile"]) // 2] / sorted(res["shared"])[len(res["shared"]) // 2], 3)
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
