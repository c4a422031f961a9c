"""Bandwidth of the reference's own SSIM on the GPU (nd_ssim_padded, nd_ssim_padded_grad) beside the piqa-style nd_ssim as the
yardstick, on one 1 x 3 x 4000 x 6000 pair.  The C entry points are called directly on preallocated buffers; each round times every
variant once between device events (the variants alternate, so drift hits all of them alike), after warm-up rounds.  GB/s are
ALGORITHMIC bytes over the measured time: 8 B per pixel for a score (x and y read once), 20 B per pixel for score + gradient
(x and y read by each of the two passes, gx written).  Prints one JSON object.

    python tools/bench_ssim.py [--rounds 20] [--warmup 3] [--height 4000] [--width 6000] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=4000)
    ap.add_argument("--width", type=int, default=6000)
    ap.add_argument("--window", type=int, default=11)
    ap.add_argument("--out", help="also write the JSON object to this file")
    a = ap.parse_args(argv)
    import torch
    from nind_denoise_amd import _lib
    if not torch.cuda.is_available():
        sys.exit("bench_ssim: no GPU visible; a time measured elsewhere says nothing")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    n, c, h, w = 1, 3, a.height, a.width
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(n, c, h, w, device=dev, generator=g)
    y = (x + 0.05 * torch.randn(n, c, h, w, device=dev, generator=g)).clip(0, 1)
    out = torch.empty(n, device=dev)
    gout = torch.full((n,), -1.0, device=dev)
    gx = torch.empty_like(x)
    ws = torch.empty(max(lib.nd_ssim_padded_workspace_bytes(n, c, h, w, a.window), lib.nd_ssim_workspace_bytes(n, c, h, w), 4096),
                     dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr(dev)

    def padded_fwd():
        _lib.check(lib.nd_ssim_padded(x.data_ptr(), y.data_ptr(), n, c, h, w, a.window, out.data_ptr(), ws.data_ptr(), ws.numel(), s))

    def padded_fwd_bwd():
        padded_fwd()
        _lib.check(lib.nd_ssim_padded_grad(x.data_ptr(), y.data_ptr(), n, c, h, w, a.window, gout.data_ptr(), gx.data_ptr(),
                                           ws.data_ptr(), ws.numel(), s))

    def piqa_fwd():
        _lib.check(lib.nd_ssim(x.data_ptr(), y.data_ptr(), n, c, h, w, out.data_ptr(), ws.data_ptr(), ws.numel(), s))

    pixels = n * c * h * w
    variants = {"nd_ssim_padded": (padded_fwd, 8 * pixels), "nd_ssim_padded + nd_ssim_padded_grad": (padded_fwd_bwd, 20 * pixels),
                "nd_ssim (yardstick)": (piqa_fwd, 8 * pixels)}
    times = {k: [] for k in variants}
    for r in range(a.warmup + a.rounds):
        for k, (fn, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1))
    padded_fwd()
    score = out.item()
    res = {"what": f"device-event time of one call on a {n}x{c}x{h}x{w} float32 pair, window {a.window}; {a.rounds} rounds after {a.warmup} "
                   "warm-up rounds, variants alternating; GB/s = algorithmic bytes (8 B per pixel forward, 20 B per pixel forward + "
                   "gradient) over the median time",
           "device": torch.cuda.get_device_name(dev), "score_padded": score, "variants": {}}
    for k, (_, nbytes) in variants.items():
        med = statistics.median(times[k])
        res["variants"][k] = {"median_ms": round(med, 4), "min_ms": round(min(times[k]), 4), "max_ms": round(max(times[k]), 4),
                              "algorithmic_bytes": nbytes, "GBps": round(nbytes / med / 1e6, 1)}
    yard, fwd = res["variants"]["nd_ssim (yardstick)"], res["variants"]["nd_ssim_padded"]
    res["forward_time_per_byte_vs_nd_ssim"] = round(fwd["median_ms"] / yard["median_ms"], 3)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
