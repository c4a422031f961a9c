"""What fallback_dtype costs on the two 16-bit bench configurations (bf16 G24 at 320 tiles per launch, fp16 G61 at 80 tiles per
launch, as `bench.py --full` runs them), written to profiles/fallback.json:

  overhead      the plain frame (nd_utnet_denoise_frame) against the checked frame (nd_utnet_denoise_frame_checked + the one host
                read of the flags) on a frame with no bad tile, alternating in one process; medians of --rounds rounds
  per_tile      fp16 G61 frames with 1, 4 and 16 bad tiles (a 4 x 4 patch of 1e5 in the middle of each): milliseconds added over
                the checked frame with no bad tile, fallback f32
  vs_parent     with --parent-root DIR (a built tree of the parent commit): the plain frame of that tree against this tree's,
                alternating child processes of this script (--plain-only), medians of --rounds runs and both spreads

    python3 tools/bench_fallback.py [--parent-root DIR] [--rounds 3] [--frames 3] [--out profiles/fallback.json]

Every child process runs under a time limit, and the first one that fails ends the comparison."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CONFIGS = {
    # key: (W, H, cs, ucs, ol), compute dtype, tiles per launch, frame seed -- OTHER_CONFIGS of bench.py
    "bf16_g24": ((6000, 4000, 264, 200, 64), "bf16", 320, 24),
    "f16_g61": ((9504, 6336, 520, 456, 64), "f16", 80, 61),
}
FUNIT = 64


def _net(dtype, fallback, dev, root_has_fallback=True):
    from nind_denoise_amd import synth
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=FUNIT, compute_dtype=dtype, **({"fallback_dtype": fallback} if root_has_fallback else {}))
    net.load_state_dict(synth.make_utnet_state_dict(funit=FUNIT, seed=123))
    return net.eval().to(dev)


def _time(fn, frames):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / frames


def plain_only(key, frames, rounds):
    """ms per plain frame of the tree on sys.path, one figure per round (a child process of vs_parent)"""
    import torch
    from nind_denoise_amd import pipeline, synth
    dev = torch.device("cuda:0")
    (W, H, cs, ucs, ol), dtype, batch, seed = CONFIGS[key]
    net = _net(dtype, None, dev, root_has_fallback=False)
    img = torch.from_numpy(synth.make_frame(W, H, seed=seed)).to(dev)
    canvas = torch.zeros_like(img)

    def run():
        canvas.zero_()
        pipeline.denoise_frame(net, img, cs, ucs, ol, batch=batch, canvas=canvas)
    run()
    return [round(_time(run, frames), 3) for _ in range(rounds)]


def overhead_and_tiles(key, frames, rounds, with_tiles):
    import torch
    from nind_denoise_amd import pipeline, synth
    dev = torch.device("cuda:0")
    (W, H, cs, ucs, ol), dtype, batch, seed = CONFIGS[key]
    plain, checked = _net(dtype, None, dev), _net(dtype, "f32", dev)
    frame = synth.make_frame(W, H, seed=seed)
    img = torch.from_numpy(frame).to(dev)
    canvas = torch.zeros_like(img)
    report = {}

    def run(net, im=img):
        canvas.zero_()
        pipeline.denoise_frame(net, im, cs, ucs, ol, batch=batch, canvas=canvas, report=report)
    run(plain)
    run(checked)
    assert report["fallback_tiles"] == []
    ms = {"plain": [], "checked": []}
    for _ in range(rounds):
        ms["plain"].append(round(_time(lambda: run(plain), frames), 3))
        ms["checked"].append(round(_time(lambda: run(checked), frames), 3))
    mp, mc = statistics.median(ms["plain"]), statistics.median(ms["checked"])
    out = {"geometry": {"width": W, "height": H, "cs": cs, "ucs": ucs, "ol": ol, "tiles": report["tiles"], "tiles_per_launch": batch},
           "dtype": dtype, "frames_per_round": frames, "ms_per_frame": ms, "median_plain_ms": mp, "median_checked_ms": mc,
           "checked_over_plain": round(mc / mp, 4), "added_ms": round(mc - mp, 3),
           "plain_spread_ms": round(max(ms["plain"]) - min(ms["plain"]), 3)}
    if with_tiles:
        from nind_denoise_amd import _lib
        cols, stride = _lib.tile_grid(W, H, cs, ucs, ol)[0], ucs - ol
        out["per_tile"] = {}
        for n, side in ((1, 1), (4, 2), (16, 4)):
            f = frame.copy()
            for r in range(4, 4 + side):         # the middle of a tile's useful square lies in that tile's window alone
                for c in range(4, 4 + side):
                    y, x = r * stride + ucs // 2, c * stride + ucs // 2
                    f[:, y:y + 4, x:x + 4] = 1e5
            im = torch.from_numpy(f).to(dev)
            run(checked, im)                        # (the first one builds the fallback's blob and workspace)
            assert len(report["fallback_tiles"]) == n, report
            assert bool(torch.isfinite(canvas).all())
            t = [round(_time(lambda: run(checked, im), frames), 3) for _ in range(rounds)]
            out["per_tile"][str(n)] = {"fallback_tiles": list(report["fallback_tiles"]), "ms_per_frame": t,
                                       "added_ms": round(statistics.median(t) - mc, 3),
                                       "added_ms_per_tile": round((statistics.median(t) - mc) / n, 3)}
        out["per_tile"]["fallback_dtype"] = "f32"
        out["per_tile"]["tiles_per_row"] = cols
    return out


def vs_parent(parent_root, key, frames, rounds, limit):
    res = {"parent": [], "this": []}
    for _ in range(rounds):
        for which, root in (("parent", parent_root), ("this", ROOT)):
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--plain-only", key, "--root", root,
                   "--frames", str(frames), "--rounds", "1"]
            r = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-4000:])
                raise SystemExit(f"the {which} tree's run ended with status {r.returncode}: the comparison stops here")
            res[which].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("[")][-1])[0])
    mp, mt = statistics.median(res["parent"]), statistics.median(res["this"])
    return {"ms_per_frame": res, "median_parent_ms": mp, "median_this_ms": mt, "this_over_parent": round(mt / mp, 4),
            "parent_spread_ms": round(max(res["parent"]) - min(res["parent"]), 3),
            "this_spread_ms": round(max(res["this"]) - min(res["this"]), 3),
            "inside_spread": abs(mt - mp) <= max(max(res["parent"]) - min(res["parent"]), max(res["this"]) - min(res["this"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", help="built tree of the parent commit")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per child process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fallback.json"))
    ap.add_argument("--plain-only", metavar="CONFIG", help="(child process) time the plain frame of the tree at --root")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.plain_only:
        print(json.dumps(plain_only(a.plain_only, a.frames, a.rounds)), flush=True)
        return
    out = {"what": "fallback_dtype: checked frame against plain frame with no bad tile, cost per recomputed tile, plain frame against "
                   "the parent commit; UtNet(64), medians of alternating rounds (tools/bench_fallback.py)",
           "overhead": {}, "vs_parent": {}}
    for key in CONFIGS:
        out["overhead"][key] = overhead_and_tiles(key, a.frames, a.rounds, with_tiles=key == "f16_g61")
        print(json.dumps({key: out["overhead"][key]}), flush=True)
    import torch
    torch.cuda.empty_cache()
    if a.parent_root:
        for key in CONFIGS:
            out["vs_parent"][key] = vs_parent(os.path.abspath(a.parent_root), key, a.frames, a.rounds, a.limit)
            print(json.dumps({"vs_parent " + key: out["vs_parent"][key]}), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
