#!/usr/bin/env python3
"""Cost of the input-image gradient (k_input_grad: the first layer's data gradient through ReflectionPad2d(2)) inside the UtNet
training backward.  One forward (nd_utnet_train_forward_hw), then nd_utnet_train_backward_hw timed in three modes on the
same saved state:

    params      parameter gradients only (the fused step's and the trainable module's default)
    params+dx   parameter gradients and d loss / d x
    dx          d loss / d x only, grads = NULL (a frozen network as a differentiable stage)

    python tools/bench_input_grad.py [--funit 64] [--cs 136] [--width W] [--batch 30] [--iters 20] [--warmup 3]

The backward is idempotent on a saved forward (every gradient buffer is rewritten before it is accumulated into), so it is
repeated as is.  Prints one JSON line; dx share = (params+dx - params) / params+dx."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nind_denoise_amd import _lib, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--funit", type=int, default=64)
    ap.add_argument("--cs", type=int, default=136)
    ap.add_argument("--width", type=int, default=None, help="crop width (default: --cs)")
    ap.add_argument("--batch", type=int, default=30)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    f, h, w, B = args.funit, args.cs, args.width or args.cs, args.batch
    sd = synth.make_utnet_state_dict(f, seed=123)
    flat = torch.zeros(lib.nd_utnet_param_count(f), dtype=torch.float32)
    for i, name in enumerate(_lib.utnet_tensor_names()):
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.nd_utnet_param_range(f, i, off, cnt))
        flat[off.value:off.value + cnt.value] = sd[name].reshape(-1)
    params = flat.to(dev)
    grads = torch.zeros_like(params)
    blobs = torch.empty(lib.nd_utnet_train_blob_bytes(f), dtype=torch.uint8, device=dev)
    nbytes = lib.nd_utnet_train_workspace_bytes_hw(f, h, w, B)
    if nbytes == 0:
        _lib.check(lib.nd_utnet_train_workspace_init_hw(None, 0, f, h, w, B, None), "workspace")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr(dev)
    _lib.check(lib.nd_utnet_train_workspace_init_hw(ws.data_ptr(), nbytes, f, h, w, B, s), "workspace init")
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, 3, h, w, generator=g).to(dev)
    gy = ((torch.rand(B, 3, h, w, generator=g) - 0.5) / (B * 3 * h * w)).to(dev)
    y = torch.empty_like(x)
    dx = torch.empty_like(x)
    act = _lib.ACT["PReLU"]
    _lib.check(lib.nd_utnet_train_forward_hw(f, act, 0, params.data_ptr(), blobs.data_ptr(), x.data_ptr(), y.data_ptr(), B, h, w,
                                             ws.data_ptr(), nbytes, s), "forward")

    def backward(with_grads, with_dx):
        _lib.check(lib.nd_utnet_train_backward_hw(f, act, 0, params.data_ptr(), grads.data_ptr() if with_grads else None,
                                                  blobs.data_ptr(), gy.data_ptr(), dx.data_ptr() if with_dx else None, B, h, w,
                                                  ws.data_ptr(), nbytes, s, None, 0), "backward")

    def timed(with_grads, with_dx):
        for _ in range(args.warmup):
            backward(with_grads, with_dx)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.iters):
            backward(with_grads, with_dx)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.iters

    # interleaved rounds, median per mode: the three modes see the same clocks
    modes = {"params": (True, False), "params+dx": (True, True), "dx": (False, True)}
    samples = {k: [] for k in modes}
    for _ in range(3):
        for k, m in modes.items():
            samples[k].append(timed(*m))
    ms = {k: sorted(v)[len(v) // 2] for k, v in samples.items()}
    print(json.dumps({"metric": "UtNet training backward, ms", "funit": f, "crop": [h, w], "batch": B,
                      "ms_params": round(ms["params"], 3), "ms_params_dx": round(ms["params+dx"], 3), "ms_dx_only": round(ms["dx"], 3),
                      "dx_kernel_ms_est": round(ms["params+dx"] - ms["params"], 4),
                      "dx_share": round((ms["params+dx"] - ms["params"]) / ms["params+dx"], 4),
                      "samples_ms": {k: [round(v, 3) for v in vs] for k, vs in samples.items()}}))


if __name__ == "__main__":
    main()
