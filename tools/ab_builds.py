"""A/B of two builds of libnind_hip.so on the flagship benchmark, alternating, in one process tree on one GPU.

    python3 tools/ab_builds.py --other /path/to/other/libnind_hip.so [--rounds 3] [--steps 20] [--warmup 5] [--out ab.json]
    python3 tools/ab_builds.py --other-root /path/to/other/tree ...

Per round: `python bench.py --gpus 1 --steps S --warmup W` with the other build's library in place of nind_denoise_amd/libnind_hip.so,
then with this tree's.  --other-root instead runs the bench.py of another built tree (its own Python and library) for the other
build: for a parent whose library lacks an entry point this tree's Python binds.  Every bench run is a child process of its own
under a time limit; the first one that fails ends the A/B (nothing more is started on the GPU) and this tree's library is put back
in either case.  The summary holds every round's ms_per_step, the other build's spread (max - min: the noise), the median gain,
and whether every round of this build beat every round of the other one."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "nind_denoise_amd", "libnind_hip.so")


def bench(steps, warmup, limit, root=ROOT):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps),
           "--warmup", str(warmup)]
    r = subprocess.run(cmd, cwd=root, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(f"bench.py ended with status {r.returncode}: the A/B stops here")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", help="libnind_hip.so of the build to compare with (the parent commit's)")
    ap.add_argument("--other-root", help="built tree of the build to compare with: its own bench.py runs, nothing is swapped")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds per bench run")
    ap.add_argument("--out")
    a = ap.parse_args()
    if bool(a.other) == bool(a.other_root):
        ap.error("give one of --other and --other-root")
    keep = tempfile.mkdtemp(prefix="ab_builds_")
    mine = os.path.join(keep, "this.so")
    shutil.copy2(LIB, mine)
    res = {"other": [], "this": []}
    try:
        for r in range(a.rounds):
            for which, src in (("other", a.other), ("this", mine)):
                if src:
                    shutil.copy2(src, LIB)
                j = bench(a.steps, a.warmup, a.limit, os.path.abspath(a.other_root) if which == "other" and a.other_root else ROOT)
                res[which].append(j["ms_per_step"])
                print(json.dumps({"round": r, "build": which, "ms_per_step": j["ms_per_step"], "value": j.get("value"), "unit": j.get("unit")}),
                      flush=True)
    finally:
        shutil.copy2(mine, LIB)
        shutil.rmtree(keep, ignore_errors=True)
    spread = max(res["other"]) - min(res["other"])
    gain = statistics.median(res["other"]) - statistics.median(res["this"])
    summary = {"steps": a.steps, "warmup": a.warmup, "ms_per_step": res, "other_spread_ms": round(spread, 3),
               "this_spread_ms": round(max(res["this"]) - min(res["this"]), 3), "median_gain_ms": round(gain, 3),
               "every_round_faster": max(res["this"]) < min(res["other"]),
               "gain_over_spread": round(gain / spread, 1) if spread > 0 else None}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(summary, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
