"""CPU-only tests of the res.txt scoring pass (loss.py, libs/pytorch_ssim): ground-truth lookup and file listing on temp
directories, argument checks that need no GPU, the three nd_ssim_padded* names in the header and in _lib.EXPORTS, and the
fixture the reference's own pytorch_ssim generated (tests/golden/make_golden_ssim.py)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib, loss
from nind_denoise_amd.libs import pytorch_ssim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("nd_ssim_padded_workspace_bytes", "nd_ssim_padded", "nd_ssim_padded_grad")


def test_find_gt_path_and_files(tmp_path):
    gt = tmp_path / "gt"
    for aset, isos, ext in (("banana", ("ISO6400", "ISO200", "ISOH1"), "png"), ("MuseeL-Bobo", ("ISO800", "ISO100", "ISO3200"), "jpg")):
        (gt / aset).mkdir(parents=True)
        for iso in isos:
            (gt / aset / f"NIND_{aset}_{iso}.{ext}").write_bytes(b"")
    assert loss.find_gt_path("NIND_banana_ISO6400.png", str(gt)) == str(gt / "banana" / "NIND_banana_ISO200.png")
    assert loss.find_gt_path("NIND_banana_ISOH1.png", str(gt)) == str(gt / "banana" / "NIND_banana_ISO200.png")   # ISOH* sort last
    # the extension comes from the ground-truth set, not from the denoised file
    assert loss.find_gt_path("NIND_MuseeL-Bobo_ISO3200.jpg.tif", str(gt)) == str(gt / "MuseeL-Bobo" / "NIND_MuseeL-Bobo_ISO100.jpg")
    with pytest.raises(FileNotFoundError):
        loss.find_gt_path("NIND_nosuchset_ISO200.png", str(gt))
    # a mixed set: the extension of the first file in sorted order (ISO200.tif sorts before ISO6400.png)
    (gt / "mix").mkdir()
    (gt / "mix" / "NIND_mix_ISO6400.png").write_bytes(b"")
    (gt / "mix" / "NIND_mix_ISO200.tif").write_bytes(b"")
    assert loss.find_gt_path("NIND_mix_ISO6400.png", str(gt)).endswith("NIND_mix_ISO200.tif")

    out = tmp_path / "out"
    (out / "subdir").mkdir(parents=True)
    for fn in ("NIND_b_ISO800.png", "res.txt", "NIND_a_ISO200.png"):
        (out / fn).write_bytes(b"")
    assert list(loss.files(str(out))) == ["NIND_a_ISO200.png", "NIND_b_ISO800.png"]      # sorted; res.txt and directories skipped


@pytest.mark.parametrize("window_size", [0, 1, 2, 4, 10, 12, 13, -3])
def test_window_size_is_checked_before_anything_runs(window_size):
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(ValueError, match="window_size"):
        pytorch_ssim.ssim(x, x, window_size=window_size)
    with pytest.raises(ValueError, match="window_size"):
        pytorch_ssim.SSIM(window_size=window_size)


def test_cpu_tensors_are_refused():
    x = torch.rand(1, 3, 16, 16)
    for ws in (3, 11):
        with pytest.raises(RuntimeError, match="GPU only"):
            pytorch_ssim.ssim(x, x, window_size=ws)
    with pytest.raises(RuntimeError, match="GPU only"):
        pytorch_ssim.SSIM()(x, x)
    with pytest.raises(ValueError):
        pytorch_ssim.ssim(x, x[..., :8])
    with pytest.raises(NotImplementedError):
        pytorch_ssim.ssim(x, x.clone().requires_grad_())
    with pytest.raises(RuntimeError, match="GPU"):
        loss.gen_score("/nonexistent", device="cpu")


def test_header_and_exports_hold_the_new_names():
    hdr = open(os.path.join(ROOT, "include", "nind_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    # sizes are host arithmetic: one float per 32 x 32 tile of every plane, and 0 for what the calls refuse
    assert lib.nd_ssim_padded_workspace_bytes(2, 3, 33, 65, 11) >= 2 * 3 * 2 * 3 * 4
    assert lib.nd_ssim_padded_workspace_bytes(1, 3, 1, 1, 3) > 0
    for bad in (4, 13, 1, 0):
        assert lib.nd_ssim_padded_workspace_bytes(1, 3, 32, 32, bad) == 0
    assert lib.nd_version() >= 111


def test_fixture_loads_and_its_own_distances_hold(golden_dir):
    from nind_denoise_amd import synth
    import hashlib
    d = np.load(os.path.join(golden_dir, "pytorch_ssim.npz"))
    index = json.loads(bytes(d["index"]))
    cap = float(d["tight_cap"])
    assert cap == 5e-7
    tight = [i for i, c in enumerate(index) if c["group"] == "tight"]
    const = [i for i, c in enumerate(index) if c["group"] == "const"]
    assert len(tight) == 27 and len(const) == 2
    assert {tuple(index[i]["shape"]) for i in tight} == {(1, 3, 5, 7), (1, 3, 1, 40), (1, 3, 11, 11), (2, 3, 32, 32), (1, 1, 33, 65),
                                                         (1, 3, 97, 130), (3, 3, 64, 48)}
    assert {index[i]["window"] for i in tight if tuple(index[i]["shape"]) == (2, 3, 32, 32)} == {3, 7, 11}
    assert {index[i]["kind"] for i in tight} == {"noisy", "indep", "q8"}
    assert 0 < d["dist"][tight].max() <= cap
    assert d["dist"][const].min() > cap                      # the cancellation cases really are outside the tight set
    assert d["score32"].dtype == np.float32 and d["score64"].dtype == np.float64
    assert d["score64"].size == sum(c["shape"][0] for c in index) == d["score32"].size
    for i, c in enumerate(index):                            # the stored distance is the one of the stored numbers
        n = c["shape"][0]
        s32, s64 = d["score32"][c["off"]:c["off"] + n].astype(np.float64), d["score64"][c["off"]:c["off"] + n]
        assert max(np.abs(s32 - s64).max(), abs(float(d["mean32"][i]) - d["mean64"][i])) == d["dist"][i]
        assert abs(s64.mean() - d["mean64"][i]) < 1e-12
        x, y = synth.make_ssim_pair(*c["shape"], c["kind"], c["seed"])       # a drifting input generator fails here
        h = hashlib.sha256()
        h.update(x.tobytes())
        h.update(y.tobytes())
        assert h.hexdigest() == c["sha"], c["id"]
    grads = json.loads(bytes(d["grads"]))
    assert [g["id"] for g in grads] == ["n1c3h5w7_ws11_noisy", "n2c3h32w32_ws11_indep", "n1c1h33w65_ws11_noisy"]
    assert sum(g["count"] for g in grads) == d["grad32"].size == d["grad64"].size
    for g in grads:
        g32, g64 = (d[k][g["off"]:g["off"] + g["count"]].astype(np.float64) for k in ("grad32", "grad64"))
        assert 0 < g["rel"] < 1e-5 and abs(np.abs(g32 - g64).max() / np.abs(g64).max() - g["rel"]) < 2e-7
    files = json.loads(bytes(d["files"]))
    assert sorted(files) == ["bike", "tree"] and all(len(s["files"]) == 3 for s in files.values())
    assert os.path.getsize(os.path.join(golden_dir, "pytorch_ssim.npz")) < 100_000
