"""What packing the 16-bit weight blob on the device buys: UtNet(64), wall clock around UtNet.packed_weights (cache cleared,
ending in a stream synchronise) for bf16 and fp16, host packer (pack_on_device = False) and device packer alternating; then the
wall time of a fresh `python -m nind_denoise_amd.denoise_image` process on one 6000 x 4000 16-bit TIFF (cs 264 / ucs 200 / ol 64,
UtNet(64)) per compute_dtype.  Prints one JSON object.

    python tools/pack_time.py [--rounds 5] [--cli-runs 3] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pack_times(dev, rounds):
    import torch
    from nind_denoise_amd import synth
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=64)
    net.load_state_dict(synth.make_utnet_state_dict(funit=64, seed=1))
    net = net.eval().to(dev)
    out = {}
    for dtype in ("bf16", "f16"):
        net.set_compute_dtype(dtype)
        times = {"host": [], "device": []}
        for r in range(rounds + 1):                    # round 0 warms both paths up and is dropped
            for path in ("host", "device"):
                net.pack_on_device = path == "device"
                net._packed.clear()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                net.packed_weights(dev)
                torch.cuda.current_stream(dev).synchronize()
                if r:
                    times[path].append(time.perf_counter() - t0)
        out[dtype] = {p: {"median_ms": round(1e3 * statistics.median(t), 3), "min_ms": round(1e3 * min(t), 3),
                          "max_ms": round(1e3 * max(t), 3), "all_ms": [round(1e3 * x, 3) for x in t]} for p, t in times.items()}
        out[dtype]["blob_bytes"] = net.packed_weights(dev).numel() * 4
    return out


def cli_walls(runs, workdir):
    import numpy as np
    import torch
    from nind_denoise_amd import synth
    from nind_denoise_amd.common.libs import imgcodec
    torch.save(synth.make_utnet_state_dict(funit=64, seed=1), os.path.join(workdir, "generator_650.pt"))
    frame = synth.make_frame(6000, 4000, seed=24)
    imgcodec.write_tiff(os.path.join(workdir, "in.tif"), (frame * 65535).round().astype(np.uint16).transpose(1, 2, 0))
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.pop("NIND_DENOISE_SERVER", None)
    out = {}
    for dtype in ("f32", "bf16", "f16"):
        out[dtype] = []
        for k in range(runs):
            cmd = [sys.executable, "-m", "nind_denoise_amd.denoise_image", "--network", "UtNet", "--model_path", "generator_650.pt",
                   "--model_parameters", f"funit=64,compute_dtype={dtype}", "--cs", "264", "--ucs", "200", "-ol", "64",
                   "--exif_method", "noexif", "--input", "in.tif", "--output", f"out_{dtype}.tiff"]
            t0 = time.perf_counter()
            r = subprocess.run(cmd, env=env, cwd=workdir, capture_output=True, text=True, timeout=300)
            wall = time.perf_counter() - t0
            timer = [ln for ln in r.stdout.splitlines() if ln.startswith("Elapsed time")]
            out[dtype].append({"returncode": r.returncode, "wall_s": round(wall, 3), "reference_timer_line": timer[-1] if timer else "",
                               "stderr_tail": r.stderr[-300:] if r.returncode else ""})
            if r.returncode != 0:      # a failed run ends the measurement: nothing more is started on the device
                return out, False
    return out, True


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cli-runs", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON object to this file")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        sys.exit("pack_time: no GPU visible; a time measured elsewhere says nothing")
    dev = torch.device("cuda:0")
    res = {"what": "UtNet(64): wall time of UtNet.packed_weights (cache cleared, stream synchronised), host packer vs device packer, "
                   f"alternating, {a.rounds} rounds after one warm-up round; wall time of a fresh denoise_image process on one "
                   "6000x4000 16-bit TIFF, cs 264 / ucs 200 / ol 64, float TIFF out",
           "device": torch.cuda.get_device_name(dev), "packed_weights": pack_times(dev, a.rounds)}
    ok = True
    if a.cli_runs > 0:
        with tempfile.TemporaryDirectory() as d:
            res["process_per_image"], ok = cli_walls(a.cli_runs, d)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
