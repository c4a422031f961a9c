#!/usr/bin/env python3
"""Generate tests/golden/augment.npz by running the REFERENCE's own DenoisingDataset.__getitem__ on the CPU (build container only).

Run:  python tests/golden/make_golden_augment.py      (needs the reference checkout make_golden.py names; never runs on the GPU box)

What is imported from the reference (read-only, executed here, never copied): dataset_torch_3.py and common/libs/np_imgops.py.
Their imports that are absent here (cv2, torchvision, imageio, piexif, yaml, piqa) are inert placeholders: none of them is reached
by the code that runs.  Two things are put in their place:
  np_imgops.img_path_to_np_flt   a reader of in-memory integer arrays with the reference's conversion (samples / 255 or / 65535
                                 in float32): there are no files and no cv2
  random (in both modules)       a proxy that draws from one seeded random.Random and records every call, so that the draws of
                                 a case can be stored next to its outputs
The dataset object is a subclass that only sets cs, exp_mult_* and get_x_y_paths; __getitem__ and crop_and_pad_from_paths are the
reference's.  Pad cases (a side shorter than cs) cannot go through the reference's crop_and_pad_from_paths -- its call of the pad
function raises AttributeError (`yimg. self.cs`) -- so for them that one method is replaced by one that calls the reference's
np_pad_img_pair and np_crop_img_pair with the arguments the functions take; the orientation and the multiplier are still __getitem__'s.

Layout (JSON as uint8 bytes, as in pytorch_ssim.npz):
  index     JSON list of cases {id, src, cs, kind, x0, y0, nrot, flip1, flip2, mult (float32 bits or null), u, exp_mult_min,
            exp_mult_max, cap_binds}
  sources   JSON list {name, dtype, shape}; arrays src<k>_clean / src<k>_noisy: the integer samples, HWC as a file decodes
  clean, noisy   float32 [cases, 3, cs, cs]: what __getitem__ returned
"""
import json
import os
import random as _random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF  # noqa: E402  (where the reference lives)

CS = 24
# name, dtype, (H, W), brightness (the clean image's largest sample as a fraction of full scale)
SOURCES = [
    ("sq_u8", np.uint8, (40, 40), 1.0),
    ("rect_u8", np.uint8, (40, 36), 1.0),
    ("rect_u16", np.uint16, (33, 40), 1.0),
    ("dim_u8", np.uint8, (36, 40), 0.45),
    ("dim_u16", np.uint16, (40, 36), 0.5),
    ("pad_rows_u8", np.uint8, (20, 40), 1.0),
    ("pad_cols_u16", np.uint16, (40, 19), 1.0),
    ("pad_both_u8", np.uint8, (21, 18), 0.6),
]
# source, kind, exp_mult_min, exp_mult_max, seeds
RUNS = [
    ("sq_u8", "crop", 1, 1, range(100, 106)),
    ("rect_u8", "crop", 1, 1, range(200, 204)),
    ("rect_u16", "crop", 1, 1, range(300, 304)),
    ("sq_u8", "crop", 0.8, 1.3, range(400, 402)),      # bright: 1 / xmax < exp_mult_max, the cap binds
    ("rect_u16", "crop", 0.7, 1.5, range(410, 412)),
    ("dim_u8", "crop", 0.8, 1.3, range(420, 422)),     # dim: 1 / xmax > exp_mult_max
    ("dim_u16", "crop", 1.1, 1.6, range(430, 432)),
    ("pad_rows_u8", "pad", 1, 1, range(500, 503)),
    ("pad_cols_u16", "pad", 1, 1, range(510, 513)),
    ("pad_both_u8", "pad", 0.9, 1.4, range(520, 523)),
]


class RecordingRandom:
    """The names dataset_torch_3 and np_imgops use of `random`, drawn from one random.Random and logged."""

    def __init__(self):
        self.rng = _random.Random(0)
        self.log = []

    def seed(self, s):
        self.rng = _random.Random(s)
        self.log = []

    def randint(self, a, b):
        v = self.rng.randint(a, b)
        self.log.append(("randint", (a, b), v))
        return v

    def getrandbits(self, k):
        v = self.rng.getrandbits(k)
        self.log.append(("getrandbits", (k,), v))
        return v

    def choice(self, seq):
        v = self.rng.choice(seq)
        self.log.append(("choice", (), v))
        return v

    def uniform(self, a, b):
        u = self.rng.random()
        v = a + (b - a) * u            # random.Random.uniform, with its u kept
        self.log.append(("uniform", (a, b, u), v))
        return v


def placeholders():
    for name in ("cv2", "torchvision", "imageio", "piexif", "yaml"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["cv2"].error = Exception
    tv = sys.modules["torchvision"]
    tv.transforms = types.SimpleNamespace(ToTensor=lambda: None)
    piqa = types.ModuleType("piqa")
    piqa.SSIM = type("SSIM", (torch.nn.Module,), {})
    piqa.MS_SSIM = type("MS_SSIM", (torch.nn.Module,), {})
    sys.modules.setdefault("piqa", piqa)


def load_reference(rand, images):
    placeholders()
    sys.path.insert(0, os.path.dirname(REF))
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        from nind_denoise import dataset_torch_3 as ds
        from nind_denoise.common.libs import np_imgops
    finally:
        os.chdir(cwd)

    def read_array(fpath):
        img = images[fpath]                                  # HWC integer samples
        rgb_img = img.transpose(2, 0, 1)
        return rgb_img.astype(np.single) / (255 if rgb_img.dtype == np.ubyte else 65535)

    np_imgops.img_path_to_np_flt = read_array
    np_imgops.random = rand
    ds.random = rand
    return ds, np_imgops


def make_source(name, dtype, shape, bright, seed):
    rng = np.random.default_rng(seed)
    full = np.iinfo(dtype).max
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w]
    base = (0.15 + 0.85 * ((yy * 3 + xx * 5) % 37) / 36.0)[:, :, None] * np.array([1.0, 0.8, 0.6])
    clean = base * rng.uniform(0.7, 1.0, size=(h, w, 3))
    clean = clean / clean.max() * bright
    noisy = clean + rng.normal(0.0, 0.08, size=clean.shape)
    to_int = lambda a: np.clip(np.rint(a * full), 0, full).astype(dtype)
    return to_int(clean), to_int(noisy)


def jbytes(obj):
    return np.frombuffer(json.dumps(obj).encode(), dtype=np.uint8)


def main():
    rand = RecordingRandom()
    images = {}
    ds, np_imgops = load_reference(rand, images)

    class Fixed(ds.DenoisingDataset):
        def __init__(self, key, cs, exp_mult_min, exp_mult_max):
            self.key, self.cs, self.exp_mult_min, self.exp_mult_max = key, cs, exp_mult_min, exp_mult_max

        def get_x_y_paths(self, index):
            return self.key + "/clean", self.key + "/noisy"

    class FixedPad(Fixed):
        def crop_and_pad_from_paths(self, xpath, ypath):
            ximg, yimg = np_imgops.img_path_to_np_flt(xpath), np_imgops.img_path_to_np_flt(ypath)
            ximg, yimg = np_imgops.np_pad_img_pair(ximg, yimg, self.cs)
            return np_imgops.np_crop_img_pair(ximg, yimg, self.cs, np_imgops.CropMethod.RAND)

    arrays, sources = {}, []
    for k, (name, dtype, shape, bright) in enumerate(SOURCES):
        clean, noisy = make_source(name, dtype, shape, bright, seed=7000 + k)
        images[name + "/clean"], images[name + "/noisy"] = clean, noisy
        arrays[f"src{k}_clean"], arrays[f"src{k}_noisy"] = clean, noisy
        sources.append(dict(name=name, dtype=np.dtype(dtype).name, shape=list(shape)))
    names = [s["name"] for s in sources]

    index, cleans, noisys = [], [], []
    for name, kind, emin, emax, seeds in RUNS:
        for seed in seeds:
            rand.seed(seed)
            dataset = (FixedPad if kind == "pad" else Fixed)(name, CS, emin, emax)
            if kind == "pad":    # the reference's own method raises on these sources; checked once per run below
                try:
                    ds.DenoisingDataset.crop_and_pad_from_paths(dataset, name + "/clean", name + "/noisy")
                    raise SystemExit(f"{name}: the reference's pad call did not raise; use Fixed for it")
                except AttributeError:
                    rand.seed(seed)
            ximg, yimg = dataset[0]
            log = list(rand.log)
            ints = [v for f, _, v in log if f == "randint"]
            bits = [v for f, _, v in log if f == "getrandbits"]
            unis = [(a, v) for f, a, v in log if f == "uniform"]
            assert len(ints) == 3 and len(bits) == 2 and len(unis) == (emin != 1), log
            x0, y0, nrot = ints
            h, w = sources[names.index(name)]["shape"]
            assert 0 <= x0 <= max(w - CS, 0) and 0 <= y0 <= max(h - CS, 0) and 0 <= nrot <= 3
            case = dict(id=f"{name}_{kind}_s{seed}", src=names.index(name), cs=CS, kind=kind, x0=x0, y0=y0, nrot=nrot,
                        flip1=bits[0], flip2=bits[1], mult=None, u=None, exp_mult_min=emin, exp_mult_max=emax, cap_binds=None)
            if unis:
                (a, b, u), m = unis[0]
                m32 = np.float32(float(m))     # a float tensor times a Python or 0-dim scalar multiplies by its float32 value
                case.update(mult=int(m32.view(np.int32)), u=u, cap_binds=bool(float(b) < emax))
            assert ximg.dtype == torch.float32 and tuple(ximg.shape) == (3, CS, CS) == tuple(yimg.shape)
            index.append(case)
            cleans.append(ximg.numpy())
            noisys.append(yimg.numpy())
            print(case)
    binds = {c["cap_binds"] for c in index}
    assert binds == {None, True, False}, binds
    assert len({(c["nrot"], c["flip1"], c["flip2"]) for c in index}) >= 12

    out = os.path.join(HERE, "augment.npz")
    np.savez_compressed(out, index=jbytes(index), sources=jbytes(sources), clean=np.stack(cleans), noisy=np.stack(noisys),
                        torch_version=np.array(torch.__version__), **arrays)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(index)} cases")
    assert os.path.getsize(out) < 400_000


if __name__ == "__main__":
    main()
