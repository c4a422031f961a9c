#!/usr/bin/env python3
"""Generate tests/golden/pytorch_ssim.npz by running the REFERENCE's own pytorch_ssim on the CPU (build container only).

Run:  python tests/golden/make_golden_ssim.py        (needs the reference checkout make_golden.py names; never runs on the GPU box)

What is imported from the reference (read-only, executed here, never copied): libs/pytorch_ssim/__init__.py, by file path
(pure torch).  Stored per case: its float32 result in both size_average modes, the same functions evaluated on float64 inputs
with its own window cast to float64, and the distance of the two -- the reference's own float32 error, from which the tests take
their bars.  Inputs are not stored: synth.make_ssim_pair rebuilds them from the seed and the fixture holds a SHA-256 of each
pair.

Layout (few arrays, JSON as uint8 bytes: a zip entry per case would cost more than its numbers):
  index        JSON list of cases {id, shape, window, kind, seed, sigma, group, off, sha}; group 'tight' | 'const'
  score32/64   per-sample scores of every case, concatenated (case i: [off, off + n))
  mean32/64    size_average=True result per case
  dist         per case: max |float32 - float64| over both modes
  grads        JSON list {id, off, count, rel}: gradient of ((1 - ssim(x, y, size_average=False)) * linspace(0.5, 1.5, n)).sum()
  grad32/64    with respect to x from float32 autograd and from float64, flattened and concatenated; rel = max|g32 - g64| / max|g64|.
               grad64 is stored rounded to float32 (6e-8 relative, three orders below the gradient bar) to keep the file small
  files        JSON: the gen_score directory of the end-to-end test -- per ground-truth set the pair parameters of its files
               and, per scored file, the reference's SSIM() and MSELoss() on the 8-bit samples / 255, in float32 and float64
"""
import hashlib
import importlib.util
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden import REF  # noqa: E402  (where the reference lives)
from nind_denoise_amd import synth  # noqa: E402

SHAPES = [
    (1, 3, 5, 7),       # smaller than the window
    (1, 3, 1, 40),      # one row
    (1, 3, 11, 11),     # exactly one window
    (2, 3, 32, 32),     # exactly one workgroup tile, two different samples
    (1, 1, 33, 65),     # one pixel past a tile edge in both axes, C = 1
    (1, 3, 97, 130),    # several tiles with ragged edges
    (3, 3, 64, 48),     # order of the per-sample vector
]
KINDS = ("noisy", "indep", "q8")
EXTRA_WINDOWS = (3, 7)              # on (2,3,32,32)
GRADS = [((1, 3, 5, 7), "noisy"), ((2, 3, 32, 32), "indep"), ((1, 1, 33, 65), "noisy")]
TIGHT_CAP = 5e-7                    # reference-own float32 vs float64 distance of every non-constant case
# gen_score end to end: set -> [(file ISO, sigma)]; the first is the ground truth (sigma None: the clean image of the pair)
FILE_SETS = {"bike": dict(seed=41, h=70, w=90, files=[("ISO200", None), ("ISO3200", 0.05), ("ISOH1", 0.1)]),
             "tree": dict(seed=57, h=66, w=93, files=[("ISO100", None), ("ISO6400", 0.08), ("ISO800", 0.03)])}


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_pytorch_ssim", os.path.join(REF, "libs", "pytorch_ssim", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def sha_pair(x, y):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(x).tobytes())
    h.update(np.ascontiguousarray(y).tobytes())
    return h.hexdigest()


def jbytes(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)      # (a numpy str array spends 4 bytes per character)


def case_id(shape, window, kind):
    return "n{}c{}h{}w{}_ws{}_{}".format(*shape, window, kind)


def seed_of(shape, window, kind):
    return 1000 * shape[2] + 10 * shape[3] + window + 100000 * (("noisy", "indep", "q8", "const", "const_near").index(kind) + 1)


def ssim64(ref, x, y, window, size_average):
    c = x.shape[1]
    return ref._ssim(x.double(), y.double(), ref.create_window(window, c).double(), window, c, size_average)


def scores(ref, x, y, window):
    xt, yt = torch.from_numpy(x), torch.from_numpy(y)
    with torch.no_grad():
        s32 = ref.ssim(xt, yt, window_size=window, size_average=False).numpy()
        m32 = ref.SSIM(window_size=window, size_average=True)(xt, yt).item()
        s64 = ssim64(ref, xt, yt, window, False).numpy()
        m64 = ssim64(ref, xt, yt, window, True).item()
    assert s32.dtype == np.float32 and s64.dtype == np.float64
    return s32, m32, s64, m64


def main():
    torch.set_num_threads(8)
    ref = load_reference()
    cases = [(s, 11, k, "tight") for s in SHAPES for k in KINDS]
    cases += [((2, 3, 32, 32), ws, k, "tight") for ws in EXTRA_WINDOWS for k in KINDS]
    cases += [((1, 3, 40, 56), 11, "const", "const"), ((2, 3, 32, 32), 11, "const_near", "const")]
    index, s32s, s64s, m32s, m64s, dists = [], [], [], [], [], []
    off = 0
    for shape, window, kind, group in cases:
        seed = seed_of(shape, window, kind)
        x, y = synth.make_ssim_pair(*shape, kind, seed)
        s32, m32, s64, m64 = scores(ref, x, y, window)
        dist = max(float(np.abs(s32.astype(np.float64) - s64).max()), abs(m32 - m64))
        if group == "tight":
            assert dist <= TIGHT_CAP, (shape, window, kind, dist)
        index.append(dict(id=case_id(shape, window, kind), shape=list(shape), window=window, kind=kind, seed=seed, sigma=0.05,
                          group=group, off=off, sha=sha_pair(x, y)))
        off += shape[0]
        s32s.append(s32)
        s64s.append(s64)
        m32s.append(m32)
        m64s.append(m64)
        dists.append(dist)
        print(f"{index[-1]['id']:28s} {group:5s} mean64 {m64:.6f}  own distance {dist:.2e}")
    tight = [d for d, c in zip(dists, cases) if c[3] == "tight"]
    print(f"worst tight distance {max(tight):.2e}; worst const distance {max(d for d, c in zip(dists, cases) if c[3] == 'const'):.2e}")

    grads, g32s, g64s = [], [], []
    goff = 0
    for shape, kind in GRADS:
        seed = seed_of(shape, 11, kind)
        x, y = synth.make_ssim_pair(*shape, kind, seed)
        wvec = torch.linspace(0.5, 1.5, shape[0])
        xt = torch.from_numpy(x).requires_grad_()
        ((1 - ref.ssim(xt, torch.from_numpy(y), window_size=11, size_average=False)) * wvec).sum().backward()
        xd = torch.from_numpy(x).double().requires_grad_()
        ((1 - ssim64(ref, xd, torch.from_numpy(y), 11, False)) * wvec.double()).sum().backward()
        g32, g64 = xt.grad.numpy().ravel(), xd.grad.numpy().ravel()
        rel = float(np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max())
        grads.append(dict(id=case_id(shape, 11, kind), off=goff, count=int(g32.size), rel=rel))
        goff += g32.size
        g32s.append(g32)
        g64s.append(g64.astype(np.float32))
        print(f"grad {grads[-1]['id']:24s} max|g64| {np.abs(g64).max():.3e}  own relative distance {rel:.2e}")
    assert {k for _, k in GRADS} == {"noisy", "indep"}

    files = {}
    for aset, d in FILE_SETS.items():
        gt = None
        entries = []
        for iso, sigma in d["files"]:
            x, y = synth.make_ssim_pair(1, 3, d["h"], d["w"], "q8", d["seed"], sigma=sigma or 0.05)
            if sigma is None:
                gt = x
                entries.append(dict(iso=iso, sigma=None))
                continue
            gtt, yt = torch.from_numpy(gt), torch.from_numpy(y)
            with torch.no_grad():
                entries.append(dict(iso=iso, sigma=sigma, sha=sha_pair(gt, y),
                                    ssim32=ref.SSIM()(gtt, yt).item(), ssim64=ssim64(ref, gtt, yt, 11, True).item(),
                                    mse32=torch.nn.MSELoss()(gtt, yt).item(), mse64=torch.nn.MSELoss()(gtt.double(), yt.double()).item()))
            assert abs(entries[-1]["ssim32"] - entries[-1]["ssim64"]) <= TIGHT_CAP
        files[aset] = dict(seed=d["seed"], h=d["h"], w=d["w"], files=entries)

    out = os.path.join(HERE, "pytorch_ssim.npz")
    np.savez_compressed(out, index=jbytes(index), score32=np.concatenate(s32s), score64=np.concatenate(s64s),
             mean32=np.array(m32s, dtype=np.float32), mean64=np.array(m64s, dtype=np.float64), dist=np.array(dists, dtype=np.float64),
             grads=jbytes(grads), grad32=np.concatenate(g32s), grad64=np.concatenate(g64s),
             files=jbytes(files), tight_cap=np.array(TIGHT_CAP), torch_version=np.array(torch.__version__))
    print(f"{out}: {os.path.getsize(out)} bytes")
    assert os.path.getsize(out) < 100_000


if __name__ == "__main__":
    main()
