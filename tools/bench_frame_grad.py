#!/usr/bin/env python3
"""Cost of a gradient through a whole tiled frame (nind_denoise_amd/frame_grad.py) against the part of it that existed before:
the training forward + backward of the network on the same launches.

    python tools/bench_frame_grad.py [--width 6000] [--height 4000] [--funit 64] [--cs 264] [--ucs 200] [--ol 64]
                                     [--batch 16] [--rounds 3] [--out FILE]

Timed with device events, in one process, in interleaved rounds (median per leg):

    frame dx          forward + backward through frame_grad.denoise_frame, frozen parameters: d loss / d frame only
    frame dx+params   the same with parameter gradients
    net dx            the same launches (every full one, and the partial last one with the two workspace re-initialisations the
    net dx+params     frame loop spends on it) of nd_utnet_train_forward_hw + nd_utnet_train_backward_hw on one resident tile batch

What the frame legs add to the net legs: the fused inference forward that makes the canvas (timed on its own inside the frame
legs), and per launch nd_tile_gather, nd_stitch_grad, nd_tile_gather_grad and, with parameter gradients, one add of the flat
gradient buffer (those four timed on their own as `extras`).  Prints one JSON line; --out also writes it to a file."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nind_denoise_amd import _lib, frame_grad, pipeline, synth  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=6000)
    ap.add_argument("--height", type=int, default=4000)
    ap.add_argument("--funit", type=int, default=64)
    ap.add_argument("--cs", type=int, default=264)
    ap.add_argument("--ucs", type=int, default=200)
    ap.add_argument("--ol", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    W, H, f, cs, ucs, ol, batch = args.width, args.height, args.funit, args.cs, args.ucs, args.ol, args.batch
    net = UtNet(funit=f)
    net.load_state_dict(synth.make_utnet_state_dict(f, seed=123))
    net = net.to(dev).eval()
    img = torch.from_numpy(synth.make_frame(W, H, seed=24)).to(dev)
    total = pipeline.tile_count(W, H, cs, ucs, ol)
    launches = [(t0, min(batch, total - t0)) for t0 in range(0, total, batch)]
    gc = ((torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)) - 0.5) / (3 * H * W)).to(dev)

    def events(n):
        return [torch.cuda.Event(enable_timing=True) for _ in range(n)]

    def frame_leg(want_params):
        net.requires_grad_(want_params)
        x = img.clone().requires_grad_()
        e = events(3)
        torch.cuda.synchronize()
        e[0].record()
        canvas = frame_grad.denoise_frame(net, x, cs, ucs, ol, batch=batch)
        e[1].record()
        canvas.backward(gc)
        e[2].record()
        torch.cuda.synchronize()
        assert x.grad is not None and all((p.grad is not None) == want_params for p in net.parameters())
        net.zero_grad(set_to_none=True)
        return e[0].elapsed_time(e[2]), e[0].elapsed_time(e[1])

    frame_leg(True)                       # warm-up: packs the weights, allocates the workspaces, fills the flat parameters
    st = net._train_state(dev)
    ws = st.workspace(cs, cs, batch)
    s = _lib.stream_ptr(dev)
    act, flags = _lib.ACT[net.activation], net.flags
    xb = pipeline.gather_tiles(img, cs, ucs, ol, total // 2, batch)
    yb, dxb = torch.empty_like(xb), torch.empty_like(xb)
    gtb = frame_grad.stitch_grad(gc, cs, ucs, ol, total // 2, batch)
    acc = torch.zeros_like(st.grads)
    gimg = torch.zeros_like(img)

    def init_ws(cnt):
        _lib.check(lib.nd_utnet_train_workspace_init_hw(ws.data_ptr(), ws.numel(), f, cs, cs, cnt, s), "workspace init")

    def net_leg(want_params):
        e = events(2)
        torch.cuda.synchronize()
        e[0].record()
        for _, cnt in launches:
            if cnt != batch:
                init_ws(cnt)
            _lib.check(lib.nd_utnet_train_forward_hw(f, act, flags, st.flat.data_ptr(), st.blobs.data_ptr(), xb.data_ptr(), yb.data_ptr(),
                                                     cnt, cs, cs, ws.data_ptr(), ws.numel(), s), "forward")
            _lib.check(lib.nd_utnet_train_backward_hw(f, act, flags, st.flat.data_ptr(), st.grads.data_ptr() if want_params else None,
                                                      st.blobs.data_ptr(), gtb.data_ptr(), dxb.data_ptr(), cnt, cs, cs, ws.data_ptr(),
                                                      ws.numel(), s, None, 0), "backward")
            if cnt != batch:
                init_ws(batch)
        e[1].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1])

    def extras_leg(want_params):
        e = events(2)
        torch.cuda.synchronize()
        e[0].record()
        for t0, cnt in launches:
            _lib.check(lib.nd_tile_gather(img.data_ptr(), W, H, cs, ucs, ol, t0, cnt, xb.data_ptr(), s))
            _lib.check(lib.nd_stitch_grad(gc.data_ptr(), W, H, cs, ucs, ol, t0, cnt, gtb.data_ptr(), s))
            if want_params:
                acc.add_(st.grads)
            _lib.check(lib.nd_tile_gather_grad(dxb.data_ptr(), W, H, cs, ucs, ol, t0, cnt, gimg.data_ptr(), s))
        e[1].record()
        torch.cuda.synchronize()
        return e[0].elapsed_time(e[1])

    net_leg(True)
    samples = {k: [] for k in ("frame_dx", "frame_dx_fwd", "net_dx", "frame_dx_params", "frame_dx_params_fwd", "net_dx_params",
                               "extras_dx", "extras_dx_params")}
    for _ in range(args.rounds):
        for want_params, tag in ((False, "dx"), (True, "dx_params")):
            t, tf = frame_leg(want_params)
            samples[f"frame_{tag}"].append(t)
            samples[f"frame_{tag}_fwd"].append(tf)
            samples[f"net_{tag}"].append(net_leg(want_params))
            samples[f"extras_{tag}"].append(extras_leg(want_params))
    ms = {k: sorted(v)[len(v) // 2] for k, v in samples.items()}
    result = {"metric": "forward + backward through one tiled frame, ms", "device": torch.cuda.get_device_name(dev),
              "frame": [W, H], "funit": f, "cs": cs, "ucs": ucs, "ol": ol, "batch": batch, "tiles": total, "launches": len(launches),
              "train_workspace_bytes": ws.numel(), "rounds": args.rounds,
              "ms_frame_dx": round(ms["frame_dx"], 2), "ms_net_dx": round(ms["net_dx"], 2),
              "ratio_dx": round(ms["frame_dx"] / ms["net_dx"], 4),
              "ms_frame_dx_params": round(ms["frame_dx_params"], 2), "ms_net_dx_params": round(ms["net_dx_params"], 2),
              "ratio_dx_params": round(ms["frame_dx_params"] / ms["net_dx_params"], 4),
              "ms_inference_forward_inside_frame_legs": [round(ms["frame_dx_fwd"], 2), round(ms["frame_dx_params_fwd"], 2)],
              "ms_extras_alone": {"dx": round(ms["extras_dx"], 2), "dx_params": round(ms["extras_dx_params"], 2)},
              "samples_ms": {k: [round(v, 2) for v in vs] for k, vs in samples.items()}}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
