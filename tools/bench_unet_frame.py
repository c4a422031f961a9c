"""UNet frame time: the generic path (nd_tile_gather -> UNet.forward -> nd_stitch_add) against the fused loop
(nd_unet_denoise_frame) on whole tiles and on the useful regions.  One synthetic 6000 x 4000 frame at the reference's UNet tiling
(cs 440 / ucs 320 / overlap 6: 260 tiles), UNet() with synthetic weights, fp32.

A leg = warm-up frames, then timed frames, each between two events on the stream; median, min and max over the timed frames.

    python tools/bench_unet_frame.py --legs generic,fused_full,fused_useful,pack            # one process, this checkout
    python tools/bench_unet_frame.py --parent DIR --parent-commit HASH --commit HASH --out profiles/unet_frame_loop.json

    python tools/bench_unet_frame.py --winograd --commit HASH --out profiles/unet_winograd.json

With --winograd the yardstick is the default path of this checkout in the same session: the fused loop on the useful regions with
UNet() and with UNet(winograd=True), each in `--rounds` processes of `--frames` timed frames, the two alternating; then one more
process records the per-step table of nd_unet_profile_stack at `--batch` tiles of cs x cs (median of 5 passes; whole tiles and the
frame loop's useful regions): direct ms, Winograd ms and the form of every step.

With --parent the yardstick is the `generic` leg of another checkout (built, at the parent commit; that leg only uses exports the
parent has).  Every leg then runs in a process of its own, `--rounds` times, parent and this checkout alternating, so that the
run-to-run spread of each leg is part of the record; a difference between two legs counts where their ranges do not overlap.
Nothing is started after a leg that failed.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, CS, UCS, OL = 6000, 4000, 440, 320, 6
LEGS = ("generic", "fused_full", "fused_useful")


def run_leg(leg, batch, frames, warmup):
    """One leg in this process, on the package found first on sys.path."""
    import torch
    from nind_denoise_amd import pipeline, synth
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    if not torch.cuda.is_available():
        sys.exit("bench_unet_frame: no GPU visible; a time measured elsewhere says nothing")
    dev = torch.device("cuda:0")
    wino = leg.endswith("_wino")
    net = UNet(winograd=True) if wino else UNet()
    net.load_state_dict(synth.make_unet_state_dict(seed=0))
    net = net.eval().to(dev)
    if leg == "layers":
        return layer_table(net, dev, batch)
    if leg == "pack":
        import time
        times = {"host": [], "device": []}
        for r in range(frames + 1):                      # round 0 warms both paths up and is dropped
            for path in ("host", "device"):
                net.pack_on_device = path == "device"
                net._packed = None
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                net.packed_weights(dev)
                torch.cuda.current_stream(dev).synchronize()
                if r:
                    times[path].append(1e3 * (time.perf_counter() - t0))
        return {"leg": leg, **{p: {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
                               for p, t in times.items()}}
    img = torch.from_numpy(synth.make_frame(W, H, seed=24)).to(dev)
    total = pipeline.tile_count(W, H, CS, UCS, OL)
    if leg == "generic":
        def frame():
            canvas = torch.zeros_like(img)
            for t0 in range(0, total, batch):
                cnt = min(batch, total - t0)
                pipeline.stitch_tiles(canvas, net(pipeline.gather_tiles(img, CS, UCS, OL, t0, cnt)), CS, UCS, OL, t0)
            return canvas
    else:
        net.useful_only = leg.startswith("fused_useful")

        def frame():
            return pipeline.denoise_frame(net, img, CS, UCS, OL, batch=batch)
    ms = []
    for k in range(warmup + frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = frame()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    return {"leg": leg, "tiles": total, "batch": batch, "frames": frames, "median_ms": round(med, 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "mp_per_s": round(W * H / 1e3 / med, 3), "checksum": float(out.double().sum().item()),
            "device": torch.cuda.get_device_name(dev)}


def layer_table(net, dev, batch, passes=5):
    """Per step of the stack at `batch` tiles of CS x CS: median ms of `passes` passes on the default path and under
    ND_FLAG_UNET_WINOGRAD, the form and the FLOP counts of the latter; whole tiles (crop 0) and the frame loop's regions."""
    import ctypes
    import torch
    from nind_denoise_amd import _lib
    lib = _lib.load()
    n = lib.nd_unet_num_steps()
    names = [lib.nd_unet_step_name(i).decode() for i in range(n)]
    out = {"leg": "layers", "batch": batch, "cs": CS, "passes": passes, "device": torch.cuda.get_device_name(dev), "tables": {}}
    for what, crop in (("whole_tiles", 0), ("useful_regions", (CS - UCS) // 2)):
        cols = {}
        for key, winograd in (("direct", False), ("winograd", True)):
            net.winograd = winograd
            net._packed = None
            flags = net.flags
            with torch.cuda.device(dev):
                blob, ws = net.packed_weights(dev), net.workspace(CS, CS, batch, dev)
                steps = (_lib.StepProfile * n)()
                rows = []
                for _ in range(passes + 1):                     # the first pass warms up
                    _lib.check(lib.nd_unet_profile_stack(flags, blob.data_ptr(), batch, CS, crop, ws.data_ptr(), ws.numel(),
                                                         _lib.stream_ptr(dev), ctypes.cast(steps, ctypes.c_void_p), n), "nd_unet_profile_stack")
                    rows.append([(s.ms, s.form, s.flops, s.mfma_flops, s.ms_xform_in, s.ms_gemm, s.ms_xform_out) for s in steps])
            cols[key] = [[statistics.median(r[i][k] for r in rows[1:]) for k in (0, 4, 5, 6)] + [rows[-1][i][1], rows[-1][i][2], rows[-1][i][3]]
                         for i in range(n)]
        table = []
        for i, name in enumerate(names):
            d, w = cols["direct"][i], cols["winograd"][i]
            row = {"step": i, "layer": name, "form": _lib.FORM_NAMES[w[4]], "direct_ms": round(d[0], 4), "winograd_ms": round(w[0], 4),
                   "speedup": round(d[0] / w[0], 3) if w[0] > 0 else None, "gflop": round(w[5] / 1e9, 2),
                   "direct_tflops": round(d[5] / d[0] / 1e9, 1) if d[0] > 0 else None}
            if w[4] == 3:
                row.update(xform_in_ms=round(w[1], 4), gemm_ms=round(w[2], 4), xform_out_ms=round(w[3], 4))
            table.append(row)
        out["tables"][what] = {"steps": table, "direct_total_ms": round(sum(r["direct_ms"] for r in table), 3),
                               "winograd_total_ms": round(sum(r["winograd_ms"] for r in table), 3)}
    return out


def child(root, leg, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--legs", leg, "--batch", str(a.batch), "--frames", str(a.frames),
           "--warmup", str(a.warmup)]
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=a.leg_timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"bench_unet_frame: leg {leg} of {root} failed with status {r.returncode}; nothing more is started")
    sys.stderr.write(f"{os.path.basename(root) or root} {lines[-1]}\n")
    sys.stderr.flush()
    return json.loads(lines[-1])


def summarise(runs):
    mp = [r["mp_per_s"] for r in runs]
    return {"mp_per_s": round(statistics.median(mp), 3), "mp_per_s_range": [min(mp), max(mp)],
            "median_ms": round(statistics.median(r["median_ms"] for r in runs), 3), "runs": runs}


def winograd_ab(a):
    legs = ("fused_useful", "fused_useful_wino")
    runs = {leg: [] for leg in legs}
    for _ in range(a.rounds):
        for leg in legs:
            runs[leg].append(child(ROOT, leg, a))
    res = {"what": f"UNet fp32, one synthetic {W}x{H} frame, cs {CS} / ucs {UCS} / ol {OL} ({runs[legs[0]][0]['tiles']} tiles), {a.batch} tiles "
                   f"per launch, fused loop on the useful regions; per process {a.warmup} warm-up + {a.frames} timed frames between stream "
                   f"events, median; {a.rounds} processes per leg, UNet() and UNet(winograd=True) alternating in one session; mp_per_s = "
                   "median over the processes, mp_per_s_range = their min and max (the run-to-run spread)",
           "device": runs[legs[0]][0]["device"], "commit": a.commit, "legs": {k: summarise(v) for k, v in runs.items()}}
    base, s = res["legs"]["fused_useful"], res["legs"]["fused_useful_wino"]
    s["ratio_to_default"] = round(s["mp_per_s"] / base["mp_per_s"], 4)
    s["beyond_spread"] = s["mp_per_s_range"][0] > base["mp_per_s_range"][1]
    res["layers"] = child(ROOT, "layers", a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--batch", type=int, default=20, help="tiles per launch (260 tiles = 13 launches of 20)")
    ap.add_argument("--frames", type=int, default=10, help="timed frames per leg and process (pack: timed rounds)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3, help="with --parent: processes per leg")
    ap.add_argument("--winograd", action="store_true", help="A/B of UNet(winograd=True) against the default path of this checkout, and the per-step table")
    ap.add_argument("--parent", help="built checkout of the parent commit: its `generic` leg is the yardstick")
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    legs = [x for x in a.legs.split(",") if x]
    if a.winograd and not a.child:
        return winograd_ab(a)
    if a.child or not a.parent:
        if not a.child and ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        res = [run_leg(leg, a.batch, a.frames, a.warmup) for leg in legs]
        for r in res:
            print(json.dumps(r), flush=True)
        return 0
    runs = {"parent_generic": []}
    runs.update({leg: [] for leg in legs if leg != "pack"})
    for _ in range(a.rounds):
        runs["parent_generic"].append(child(os.path.abspath(a.parent), "generic", a))
        for leg in legs:
            if leg != "pack":
                runs[leg].append(child(ROOT, leg, a))
    res = {"what": f"UNet fp32, one synthetic {W}x{H} frame, cs {CS} / ucs {UCS} / ol {OL} ({runs['parent_generic'][0]['tiles']} tiles), "
                   f"{a.batch} tiles per launch; per process {a.warmup} warm-up + {a.frames} timed frames between stream events, "
                   f"median; {a.rounds} processes per leg, parent and this checkout alternating; mp_per_s = median over the "
                   "processes, mp_per_s_range = their min and max (the run-to-run spread)",
           "device": runs["parent_generic"][0]["device"], "parent_commit": a.parent_commit, "commit": a.commit,
           "legs": {k: summarise(v) for k, v in runs.items()}}
    base = res["legs"]["parent_generic"]
    for leg in legs:
        if leg != "pack":
            s = res["legs"][leg]
            s["ratio_to_parent_generic"] = round(s["mp_per_s"] / base["mp_per_s"], 4)
            s["beyond_spread"] = s["mp_per_s_range"][0] > base["mp_per_s_range"][1]
    if "pack" in legs:
        res["packed_weights"] = child(ROOT, "pack", a)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
