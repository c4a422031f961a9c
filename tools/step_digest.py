#!/usr/bin/env python3
"""SHA-256 digests of what the training step, the criteria, the scores and the fused frame loop compute, to compare two revisions
bit for bit.

    python tools/step_digest.py [--out digests.json] [--host]

Every case runs twice on fixed seeds: two equal lines per case mean the revision is deterministic there, and equal files from two
revisions mean they compute the same bits.  Step cases (funit 8): the output, the loss bits and the flat gradient buffer of
UtNetTrainer.forward_backward; then validation.criteria, and nd_ssim / nd_ms_ssim / nd_ssim_padded on one pair.  UNet cases, on
weights with planted BatchNorm (gamma = 0 and gamma < 0 channels), each with the library's four byte counts for its shape: eval mode
under autograd (y, dx, every parameter gradient), UNetTrainer (y, loss, grads, flat with its running statistics; dx of backward(gy,
want_dx=True)), and three learn steps of both trainers, plain and guarded (flat, m, v, vmax, guard_state).

Frame cases: the canvas of pipeline.denoise_frame on the smallest frames at which each stanza of the shared-encoder loop runs (the
geometries of tests/test_shared_encoder.py ... test_skip_fold.py), under the default flags and with each of split_k, share_level2,
fold_skips, mosaic_wino, share_encoder off.  UtNet(16) seed 9 at gain 2.2 on frame seed 3 at batch 5 and 256; UtNet(64) seed 123 on
the two-band frame FRAME64 (a one-row last band, three-pass level 2) at batch 256 (a launch over the band seam), at batch 11 and on
the tile range (191, 193).  Each run follows a frame of another seed through the same net object and workspaces.

Plan rows (--host prints only these; they need no GPU): per geometry, funit 16 / 64, flag set and dtype, the eight values of
nd_utnet_frame_plan, the levels, the folds, nd_utnet_frame_workspace_bytes and nd_utnet_workspace_bytes_hw."""
import argparse
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from nind_denoise_amd import _lib, pipeline, synth  # noqa: E402
from nind_denoise_amd.common.libs import pt_losses  # noqa: E402
from nind_denoise_amd.libs import pytorch_ssim  # noqa: E402
from nind_denoise_amd.networks.UtNet import UtNet  # noqa: E402
from nind_denoise_amd.networks.ThirdPartyNets import UNet  # noqa: E402
from nind_denoise_amd.train import UNetTrainer, UtNetTrainer  # noqa: E402
from nind_denoise_amd.validation import criteria  # noqa: E402

STEP_CASES = [  # name, h, w, batch, loss_cs, weights, activation
    ("mse-104", 104, 104, 3, None, {"MSE": 1.0}, "PReLU"),
    ("l1-mse-120-cs88", 120, 120, 2, 88, {"L1": 0.4, "MSE": 0.6}, "PReLU"),
    ("ssim-136-cs101", 136, 136, 2, 101, {"SSIM": 1.0}, "PReLU"),
    ("msssim-l1-184x168-cs161", 184, 168, 2, 161, {"MSSSIM": 0.6, "L1": 0.4}, "PReLU"),
    ("hardswish-l1-ssim-104-cs77", 104, 104, 2, 77, {"L1": 0.5, "SSIM": 0.5}, "Hardswish"),
]
UNET_EVAL_SHAPES = [(3, 33, 47), (2, 32, 32)]
UNET_EVAL_MODES = [  # name, find_noise, split_k, parameters frozen
    ("plain", False, True, False), ("find-noise", True, True, False), ("no-split-k", False, False, False), ("frozen", False, True, True)]
UNET_TRAIN_SHAPES = [(3, 33, 47), (8, 16, 16), (2, 64, 16)]      # (8, 16, 16): a 1x1 bottom level
FRAMES16 = [(333, 290, 120, 56, 16),      # levels 3, folds 7, 8 x 7 tiles
            (120, 290, 120, 56, 16),      # one column
            (333, 120, 120, 56, 16),      # one row
            (300, 170, 136, 56, 24),      # pad > stride
            (333, 290, 120, 88, 16),      # level 2 per tile, folds 3
            (333, 290, 120, 88, 20),      # S = 4 * odd
            (120, 120, 120, 88, 20),      # one tile
            (333, 290, 120, 88, 18)]      # D = 0
FRAME64 = (13000, 400, 264, 200, 64)
FRAME_SWITCHES = [None, "split_k", "share_level2", "fold_skips", "mosaic_wino", "share_encoder"]      # None: the default flags
PLAN_GEOMS = ([((6000, 4000, 264, 200, 64), 256), (FRAME64, 256), ((6000, 4000, 504, 480, 24), 64), ((6000, 4000, 520, 496, 22), 10)]
              + [(g, b) for g in FRAMES16 for b in (5, 256)])
PLAN_FLAGS = [0, _lib.FLAG_TILE_LEVEL2, _lib.FLAG_TILE_SKIPS, _lib.FLAG_TILE_ENCODER, _lib.FLAG_NO_SPLITK, _lib.FLAG_TILE_WINO]
GUARDS = [("plain", {}), ("guarded", {"max_grad_norm": 1e-6, "skip_nonfinite": True})]      # 1e-6: every step clips


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def pair(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.rand(n, 3, h, w, generator=g)
    return (-0.2 + 1.4 * (t + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)), t      # y beyond [0, 1], t inside


def unet_sd():
    """synth's UNet weights with every BatchNorm planted as tests/test_unet_grad.py plants them: negative and zero weights."""
    sd = synth.make_unet_state_dict(3)
    for k in list(sd):
        if k.endswith(".running_var"):
            w = k[:-len("running_var")] + "weight"
            sd[w][0::7] *= -1.0
            sd[w][3::11] = 0.0
    return sd


def unet_bytes(b, h, w):
    lib = _lib.load()
    return [int(lib.nd_unet_grad_workspace_bytes(h, w, b)), int(lib.nd_unet_train_workspace_bytes(h, w, b)),
            int(lib.nd_unet_grad_blob_bytes()), int(lib.nd_unet_train_blob_bytes())]


def unet_cases(dev, res):
    for b, h, w in UNET_EVAL_SHAPES:
        x, gy = pair(b, h, w, seed=h + w)
        for name, find_noise, split_k, frozen in UNET_EVAL_MODES:
            net = UNet(find_noise=find_noise)
            net.load_state_dict(unet_sd())
            net = net.eval().to(dev).requires_grad_(not frozen)
            net.split_k = split_k
            for rep in range(2):
                net.zero_grad(set_to_none=True)
                xin = x.to(dev).requires_grad_()
                y = net(xin)
                y.backward(gy.to(dev))
                grads = [p.grad for p in net.parameters() if p.grad is not None]
                res[f"unet eval {name} {b}x{h}x{w} run {rep}"] = {"y": sha(y), "dx": sha(xin.grad), "grads": sha(*grads) if grads else None,
                                                                 "bytes": unet_bytes(b, h, w)}
    for i, (b, h, w) in enumerate(UNET_TRAIN_SHAPES):
        x, t = pair(b, h, w, seed=h + w)
        for rep in range(2):
            net = UNet()      # a trainer of its own per run: the forward moves the running statistics in flat
            net.load_state_dict(unet_sd())
            tr = UNetTrainer(net, device=dev)
            y, loss = tr.forward_backward(x.clip(0, 1), t)
            r = {"y": sha(y), "loss": sha(loss), "grads": sha(tr.grads), "flat": sha(tr.flat), "bytes": unet_bytes(b, h, w)}
            if i == 0:
                r["backward dx"] = sha(tr.backward(x - t, want_dx=True), tr.grads)
            res[f"unet train {b}x{h}x{w} run {rep}"] = r
    for gname, guard in GUARDS:
        for rep in range(2):
            unet, utnet = UNet(), UtNet(funit=8)
            unet.load_state_dict(unet_sd())
            utnet.load_state_dict(synth.make_utnet_state_dict(funit=8, seed=31, gain=1.8), strict=True)
            for kind, tr, shape in (("unet", UNetTrainer(unet, device=dev, **guard), (2, 32, 32)),
                                    ("utnet", UtNetTrainer(utnet, device=dev, **guard), (2, 104, 104))):
                x, t = pair(*shape, seed=9)
                for _ in range(3):
                    tr.learn(x.clip(0, 1), t)
                state = [tr.flat, tr.m, tr.v, tr.vmax] + ([tr.guard_state] if tr.guarded else [])
                if tr.guarded:
                    assert tr.guard_state[2].item() < 1.0 and tr.guard_state[3].item() == 1.0, tr.guard_state
                res[f"optimizer {kind} {gname} run {rep}"] = sha(*state)


def plan_rows(res):
    lib = _lib.load()
    for geom, batch in PLAN_GEOMS:
        for funit in (16, 64):
            for flags in PLAN_FLAGS:
                for dt in (_lib.ND_F32, _lib.ND_BF16):
                    plan, one = (ctypes.c_int * 8)(), ctypes.c_int()
                    row = {"rc": [lib.nd_utnet_frame_plan(funit, dt, flags, *geom, plan)], "plan": list(plan)}
                    for key, fn in (("levels", lib.nd_utnet_frame_levels), ("folds", lib.nd_utnet_frame_folds)):
                        row["rc"].append(fn(funit, dt, flags, *geom, ctypes.byref(one)))
                        row[key] = one.value
                    row["frame_bytes"] = int(lib.nd_utnet_frame_workspace_bytes(funit, dt, flags, *geom, batch))
                    row["tile_bytes"] = int(lib.nd_utnet_workspace_bytes_hw(funit, geom[2], geom[2], batch, dt))
                    res[f"plan {geom}@{batch} funit {funit} flags {flags} dtype {dt}"] = row


def frame_cases(dev, res):
    runs = [(16, 9, 3, [(g, b, None) for g in FRAMES16 for b in (5, 256)]),
            (64, 123, 24, [(FRAME64, 256, None), (FRAME64, 11, None), (FRAME64, 256, (191, 193))])]
    for funit, seed, frame_seed, cases in runs:
        for switch in FRAME_SWITCHES:
            net = UtNet(funit=funit)
            net.load_state_dict(synth.make_utnet_state_dict(funit=funit, seed=seed, gain=2.2))
            net = net.eval().to(dev)
            if switch:
                setattr(net, switch, False)
            for geom, batch, tiles in cases:
                imgs = [torch.from_numpy(synth.make_frame(geom[0], geom[1], seed=sd)).to(dev) for sd in (frame_seed + 4, frame_seed)]
                for rep in range(2):
                    for img in imgs:
                        canvas = torch.zeros_like(img)
                        pipeline.denoise_frame(net, img, *geom[2:], batch=batch, tile_range=tiles, canvas=canvas)
                    res[f"frame UtNet({funit}) {geom} batch {batch} tiles {tiles} {switch or 'default'} off run {rep}"] = sha(canvas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--host", action="store_true", help="only the plan rows: no GPU needed")
    args = ap.parse_args()
    res = {}
    plan_rows(res)
    if not args.host:
        gpu_cases(torch.device("cuda", 0), res)
        torch.cuda.synchronize()
    for k, v in res.items():
        print(k, json.dumps(v))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def gpu_cases(dev, res):
    for name, h, w, batch, loss_cs, weights, act in STEP_CASES:
        net = UtNet(funit=8, activation=act)
        net.load_state_dict(synth.make_utnet_state_dict(funit=8, seed=31, gain=1.8, activation=act), strict=True)
        tr = UtNetTrainer(net, device=dev, weights=weights, loss_cs=loss_cs)
        x, t = pair(batch, h, w, seed=len(name))
        for rep in range(2):
            y, loss = tr.forward_backward(x.clip(0, 1), t)
            res[f"step {name} run {rep}"] = {"y": sha(y), "loss": sha(loss), "grads": sha(tr.grads)}
    y, t = (v.to(dev) for v in pair(2, 184, 168, seed=5))
    for rep in range(2):
        for cs, weights, also in ((0, {"L1": 0.3, "MSE": 0.2, "SSIM": 0.5}, ()), (161, {"MSSSIM": 1.0}, ("MSE",))):
            res[f"criteria cs{cs} run {rep}"] = sha(*criteria(y, t, weights, cs, also).values())
        g = y.clip(0, 1)
        res[f"scores run {rep}"] = {"ssim": sha(pt_losses.SSIM_loss()(g, t)), "ms_ssim": sha(pt_losses.MS_SSIM_loss()(g, t)),
                                    "ssim_padded": sha(pytorch_ssim.ssim(g, t, 11, size_average=False)), "mse": sha(pt_losses.mse(g, t))}
    unet_cases(dev, res)
    frame_cases(dev, res)


if __name__ == "__main__":
    main()
