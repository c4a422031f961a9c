"""Canvas of the flagship frame through the fused frame loop, for comparing two builds of the library bit for bit.

    python3 tools/dump_canvas.py --out new.npy [--no-split-k] [--tile-level2] [--tile-skips] [--tile-wino] [--batch 256] [--compare old.npy]

bench.py's flagship workload (fp32 G24: 6000x4000, cs 264 / ucs 200 / ol 64, UtNet(64) seed 123, frame seed 24).  A frame of another
seed runs first through the same net object and workspaces, so that anything a build leaves behind in them is wrong data for the
frame that is dumped.  --no-split-k sets UtNet.split_k = False (ND_FLAG_NO_SPLITK: a tile's bits do not depend on the launch
composition), --tile-level2 UtNet.share_level2 = False (ND_FLAG_TILE_LEVEL2: the third encoder level per tile),
--tile-skips UtNet.fold_skips = False (ND_FLAG_TILE_SKIPS: the skip halves of the decoder per tile), --tile-wino UtNet.mosaic_wino =
False (ND_FLAG_TILE_WINO: per-image Winograd tile grids).  --compare prints
one JSON line: equal bit for bit or not, and max |difference|.  Run once per build (swap nind_denoise_amd/libnind_hip.so between
runs, as tools/ab_builds.py does, or run the other build's own tree)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nind_denoise_amd import pipeline, synth  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--no-split-k", action="store_true")
    ap.add_argument("--tile-level2", action="store_true")
    ap.add_argument("--tile-skips", action="store_true")
    ap.add_argument("--tile-wino", action="store_true")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--compare", help="an earlier dump to compare this one with")
    a = ap.parse_args()
    W, H, cs, ucs, ol = 6000, 4000, 264, 200, 64
    dev = torch.device("cuda:0")
    net = UtNet(funit=64)
    net.load_state_dict(synth.make_utnet_state_dict(funit=64, seed=123))
    net = net.eval().to(dev)
    net.split_k = not a.no_split_k
    net.share_level2 = not a.tile_level2
    net.fold_skips = not a.tile_skips
    net.mosaic_wino = not a.tile_wino
    canvas = None
    for seed in (7, 24):
        img = torch.from_numpy(synth.make_frame(W, H, seed=seed)).to(dev)
        canvas = torch.zeros_like(img)
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=a.batch, canvas=canvas)
    torch.cuda.synchronize()
    out = canvas.cpu().numpy()
    np.save(a.out, out)
    res = {"out": a.out, "split_k": net.split_k, "share_level2": net.share_level2, "fold_skips": net.fold_skips, "mosaic_wino": net.mosaic_wino, "batch": a.batch, "max_abs": float(np.abs(out).max())}
    if a.compare:
        old = np.load(a.compare)
        res["compare"] = a.compare
        res["bit_identical"] = bool(np.array_equal(old.view(np.uint32), out.view(np.uint32)))
        res["max_abs_diff"] = float(np.abs(old.astype(np.float64) - out.astype(np.float64)).max())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
