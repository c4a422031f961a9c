"""CPU tests of validation without the crop files: crop_pool.crop_source (a crop path -> a window of a full-size image),
ValidationSet.from_full_size against the constructor on the cropped tree, bit for bit, and tools.pick_validation_set.
tests/test_val_full_size.py trains with it.

The tree (ds 128 / 96): set "bark", 404 x 500 8-bit PNG, whose grid has 3 columns x 4 rows, with ISO100, ISO6400 and two files of
ISO800 -- the one that sorts second is the cropper's ISO800-2 -- and set "alley", 308 x 330 16-bit TIFF, 2 columns x 2 rows, with
ISO100, ISO800 and ISO6400.  The cropped tree is written with the cropper's names (the file of ISO800-2 under that name), by
test_pool_windows_host.crop_tree for the PNG set and by the same steps with write_tiff for the TIFF set, which crop_tree cannot
write; then the full-size file gets back the name a download has, so that the -2 is this code's doing."""
import os
import shutil

import numpy as np
import pytest
import yaml

from nind_denoise_amd.common.libs import imgcodec, np_imgops
from nind_denoise_amd.crop_pool import crop_grid, crop_source
from nind_denoise_amd.tools import pick_validation_set
from nind_denoise_amd.validation import ValidationSet
from test_pool_windows_host import crop_tree, image_u, write_full_size

CS, STRIDE = 128, 96
LEAF = f"SYN_{CS}_{STRIDE}"


def build_tree(root):
    """{"dsdir", "cropped"} under root, as the module docstring says"""
    dsdir = write_full_size(root, "SYN", 404, 500, sets=("bark",))
    bark = os.path.join(dsdir, "bark")
    os.rename(os.path.join(bark, "SYN_bark_ISO800.png"), os.path.join(bark, "SYN_bark_ISO800-2.png"))
    imgcodec.write_png(os.path.join(bark, "SYN_bark_ISO800.PNG"), image_u(500, 404, 77))      # sorts before SYN_bark_ISO800.png
    cropped = crop_tree(dsdir, CS, STRIDE)
    os.rename(os.path.join(bark, "SYN_bark_ISO800-2.png"), os.path.join(bark, "SYN_bark_ISO800.png"))
    os.makedirs(os.path.join(dsdir, "alley"))
    for k, iso in enumerate(("ISO100", "ISO800", "ISO6400")):
        img = image_u(330, 308, 20 + k, np.uint16)
        fn = f"SYN_alley_{iso}.tif"
        imgcodec.write_tiff(os.path.join(dsdir, "alley", fn), img)
        os.makedirs(os.path.join(cropped, "alley", iso))
        for xc, yc, xb, yb in crop_grid(308, 330, CS, STRIDE):
            imgcodec.write_tiff(os.path.join(cropped, "alley", iso, f"{fn[:-4]}_{xc}_{yc}_{STRIDE}.tif"),
                                np.ascontiguousarray(img[yb:yb + CS, xb:xb + CS]))
    return {"root": root, "dsdir": dsdir, "cropped": cropped}


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return build_tree(str(tmp_path_factory.mktemp("valfull")))


def crop_files(cropped):
    """every crop file of a cropped tree, as (set, iso, name)"""
    return [(aset, iso, fn) for aset in sorted(os.listdir(cropped)) for iso in sorted(os.listdir(os.path.join(cropped, aset)))
            for fn in sorted(os.listdir(os.path.join(cropped, aset, iso)))]


FULL_SIZE_OF = {("bark", "ISO100"): "SYN_bark_ISO100.png", ("bark", "ISO800"): "SYN_bark_ISO800.PNG",
                ("bark", "ISO800-2"): "SYN_bark_ISO800.png", ("bark", "ISO6400"): "SYN_bark_ISO6400.png",
                ("alley", "ISO100"): "SYN_alley_ISO100.tif", ("alley", "ISO800"): "SYN_alley_ISO800.tif",
                ("alley", "ISO6400"): "SYN_alley_ISO6400.tif"}


def test_the_tree_is_what_the_docstring_says(tree):
    files = crop_files(tree["cropped"])
    assert len(files) == 4 * 12 + 3 * 4 and {(s, i) for s, i, _ in files} == set(FULL_SIZE_OF)
    assert len({xc for xc, _, _, _ in crop_grid(404, 500, CS, STRIDE)}) == 3 and len({xc for xc, _, _, _ in crop_grid(308, 330, CS, STRIDE)}) == 2
    assert ("bark", "ISO800-2", "SYN_bark_ISO800-2_1_1_96.png") in files and ("alley", "ISO6400", "SYN_alley_ISO6400_2_2_96.tif") in files
    assert sorted(os.listdir(os.path.join(tree["dsdir"], "bark"))) == ["SYN_bark_ISO100.png", "SYN_bark_ISO6400.png", "SYN_bark_ISO800.PNG",
                                                                       "SYN_bark_ISO800.png"]
    assert imgcodec.image_size(os.path.join(tree["dsdir"], "bark", "SYN_bark_ISO100.png")) == (404, 500)
    assert imgcodec.image_size(os.path.join(tree["dsdir"], "alley", "SYN_alley_ISO100.tif")) == (308, 330)


# ------------------------------------------------------------------ crop_source
def spellings(cropped, aset, iso, fn):
    """absolute; the reference's list form, which does not exist from the working directory; a doubled slash"""
    return [os.path.join(cropped, aset, iso, fn), f"../../datasets/cropped/{LEAF}/{aset}/{iso}/{fn}",
            os.path.join(cropped, aset) + "//" + iso + "//" + fn]


def test_every_crop_file_is_a_window_of_its_image(tree):
    full = {}
    for aset, iso, fn in crop_files(tree["cropped"]):
        want = os.path.join(tree["dsdir"], aset, FULL_SIZE_OF[(aset, iso)])
        crop = np_imgops.img_path_to_np_samples(os.path.join(tree["cropped"], aset, iso, fn))
        assert crop.shape == (3, CS, CS)
        for spelled in spellings(tree["cropped"], aset, iso, fn):
            got = crop_source(spelled, tree["dsdir"], CS, STRIDE)
            assert got is not None and got[0] == want, (spelled, got)
            fpath, yb, xb = got
            if fpath not in full:
                full[fpath] = np_imgops.img_path_to_np_samples(fpath)
            assert np.array_equal(full[fpath][:, yb:yb + CS, xb:xb + CS], crop), spelled
        xc, yc = (int(v) for v in fn[:-4].split("_")[-3:-1])
        assert (xb, yb) == (xc * STRIDE - 16, yc * STRIDE - 16)
    assert not os.path.exists(spellings(tree["cropped"], "bark", "ISO100", "x")[1])
    assert len(full) == 7


def test_the_first_dsdir_whose_leaf_matches_takes_the_path(tree, tmp_path):
    other = write_full_size(str(tmp_path), "OTHER", 404, 500, sets=("bark",), isos=("ISO100", "ISO800"))
    path = f"x/{LEAF}/bark/ISO100/SYN_bark_ISO100_1_1_96.png"
    assert crop_source(path, [other, tree["dsdir"]], CS, STRIDE)[0] == os.path.join(tree["dsdir"], "bark", "SYN_bark_ISO100.png")
    assert crop_source("x/OTHER_128_96/bark/ISO800/OTHER_bark_ISO800_3_4_96.png", [other, tree["dsdir"]], CS, STRIDE) == \
        (os.path.join(other, "bark", "OTHER_bark_ISO800.png"), 4 * 96 - 16, 3 * 96 - 16)
    # a crops_dir entry gives its leaf to its dsdir; another crop size or stride is another leaf: not a crop of this data
    assert crop_source("/e/X_1/bark/ISO100/SYN_bark_ISO100_1_1_96.png", tree["dsdir"], CS, STRIDE, crops_dir="/elsewhere/X_1")[1:] == (80, 80)
    assert crop_source(path, tree["dsdir"], CS, STRIDE, crops_dir="/elsewhere/X_1") is None
    assert crop_source(path, tree["dsdir"], 256, 192) is None and crop_source(path, other, CS, STRIDE) is None
    assert crop_source("SYN_bark_ISO100_1_1_96.png", tree["dsdir"], CS, STRIDE) is None


# ------------------------------------------------------------------ ValidationSet.from_full_size
def twelve_pairs(cropped):
    """12 [clean, noisy] pairs over both sets and every ISO, in no file order, spelled absolutely and with doubled slashes"""
    picks = [("bark", "ISO6400", 3, 4), ("alley", "ISO800", 1, 2), ("bark", "ISO800-2", 1, 1), ("bark", "ISO800", 2, 3),
             ("alley", "ISO6400", 2, 2), ("bark", "ISO6400", 1, 1), ("alley", "ISO800", 2, 1), ("bark", "ISO800", 3, 1),
             ("bark", "ISO800-2", 2, 4), ("alley", "ISO6400", 1, 1), ("bark", "ISO800-2", 3, 2), ("bark", "ISO6400", 2, 2)]
    pairs = []
    for k, (aset, iso, xc, yc) in enumerate(picks):
        ext = "png" if aset == "bark" else "tif"
        names = [f"SYN_{aset}_{v}_{xc}_{yc}_{STRIDE}.{ext}" for v in ("ISO100", iso)]
        pairs.append([spellings(cropped, aset, v, fn)[0 if k % 3 == 0 else 2] for v, fn in zip(("ISO100", iso), names)])
    return pairs


def words(t):
    return t.contiguous().numpy().view(np.int32)


@pytest.fixture(scope="module")
def from_files(tree):
    """the constructor's tensors on the cropped tree, per cs: computed once, before any test removes a copy of the tree"""
    pairs = twelve_pairs(tree["cropped"])
    return {cs: ValidationSet(pairs, "cpu", cs) for cs in (104, 128)}


@pytest.mark.parametrize("cs", [104, 128])
def test_from_full_size_is_the_constructor_on_the_cropped_tree(tree, from_files, cs, tmp_path):
    """On a copy of both trees whose cropped tree is deleted before the first call: the pairs' paths name files that do not exist."""
    alone = shutil.copytree(tree["dsdir"], str(tmp_path / "SYN"))
    pairs = twelve_pairs(shutil.copytree(tree["cropped"], os.path.join(str(tmp_path), "cropped", LEAF)))
    shutil.rmtree(os.path.join(str(tmp_path), "cropped"))
    assert not any(os.path.exists(p) for pair in pairs for p in pair)
    got, want = ValidationSet.from_full_size(pairs, alone, CS, STRIDE, "cpu", cs), from_files[cs]
    assert got.clean.shape == want.clean.shape == (12, 3, cs, cs) and got.cs == cs and len(got) == 12
    assert np.array_equal(words(got.clean), words(want.clean)) and np.array_equal(words(got.noisy), words(want.noisy))
    assert got.val_tuples == pairs and (got.n_windows, got.n_full_size_images) == (12, 7)
    assert not torch_equal_anywhere(got.clean, got.noisy)
    # and with the tree in place the result is the same: the names decide, not the disk
    there = ValidationSet.from_full_size(twelve_pairs(tree["cropped"]), tree["dsdir"], CS, STRIDE, "cpu", cs)
    assert np.array_equal(words(there.clean), words(want.clean)) and np.array_equal(words(there.noisy), words(want.noisy))


def torch_equal_anywhere(a, b):
    return any(np.array_equal(x, y) for x, y in zip(a.numpy(), b.numpy()))


def test_a_yaml_list_and_the_default_crop_size(tree, from_files, tmp_path):
    pairs = twelve_pairs(tree["cropped"])
    with open(tmp_path / "val.yaml", "w") as fp:
        yaml.dump(pairs, fp)
    got = ValidationSet.from_full_size(str(tmp_path / "val.yaml"), [tree["dsdir"]], CS, STRIDE, "cpu")
    assert got.cs == CS and np.array_equal(words(got.clean), words(from_files[128].clean)) and got.val_tuples == pairs
    with pytest.raises(ValueError, match="no validation pair"):
        ValidationSet.from_full_size([], tree["dsdir"], CS, STRIDE, "cpu")
    with pytest.raises(ValueError, match="smaller than the crop size"):
        ValidationSet.from_full_size(pairs, tree["dsdir"], CS, STRIDE, "cpu", 136)


def test_each_full_size_file_is_decoded_once(tree, monkeypatch):
    decoded = []
    real = np_imgops.img_path_to_np_flt
    monkeypatch.setattr(np_imgops, "img_path_to_np_flt", lambda fpath: decoded.append(fpath) or real(fpath))
    pairs = twelve_pairs(tree["cropped"])
    ValidationSet.from_full_size(pairs, tree["dsdir"], CS, STRIDE, "cpu", 104)
    assert sorted(decoded) == sorted(os.path.join(tree["dsdir"], s, fn) for (s, _), fn in FULL_SIZE_OF.items())
    del decoded[:]
    ValidationSet.from_full_size(pairs[2:3] + pairs[8:9] + pairs[10:11], tree["dsdir"], CS, STRIDE, "cpu", 104)
    assert sorted(decoded) == [os.path.join(tree["dsdir"], "bark", fn) for fn in ("SYN_bark_ISO100.png", "SYN_bark_ISO800.png")]


# ------------------------------------------------------------------ refusals
def test_paths_the_cropper_does_not_write_are_refused(tree, tmp_path):
    def refused(path, dsdir=tree["dsdir"]):
        with pytest.raises(FileNotFoundError) as e:
            crop_source(path, dsdir, CS, STRIDE)
        assert path in str(e.value)
        return str(e.value)

    base = f"../../datasets/cropped/{LEAF}/bark/ISO100/"
    refused(base + "SYN_bark_ISO100_0_0_96.png")                     # the first column and row are never written
    assert "SYN_bark_ISO100_1_1_96.png" in refused(base + "SYN_bark_ISO100_4_1_96.png")      # beyond the grid: the first crop is named
    refused(base + "SYN_bark_ISO100_1_5_96.png")
    assert "SYN_bark_ISO100_2_3_96.png" in refused(base + "SYN_bark_ISO100_2_3_128.png")     # another stride suffix
    assert "SYN_bark_ISO100_2_3_96.png" in refused(base + "SYN_bark_ISO100_2_3_96.jpg")      # the list of the JPEG download
    refused(base + "NIND_bark_ISO100_2_3_96.png")                    # another stem
    refused(f"x/{LEAF}/bark/ISO200/SYN_bark_ISO200_1_1_96.png")      # an ISO the set does not have
    refused(f"x/{LEAF}/birch/ISO100/SYN_birch_ISO100_1_1_96.png")    # a set the dataset does not have
    refused(f"x/{LEAF}/alley/ISO100/SYN_alley_ISO100_3_1_96.tif")    # the TIFF set's grid has two columns
    # a noisy ISO whose image is one column of crops narrower
    small = write_full_size(str(tmp_path), "SYN", 404, 500, sets=("a",), isos=("ISO100", "ISO800"))
    imgcodec.write_png(os.path.join(small, "a", "SYN_a_ISO800.png"), image_u(500, 308, 3))
    assert crop_source(f"x/{LEAF}/a/ISO100/SYN_a_ISO100_3_1_96.png", small, CS, STRIDE) == (os.path.join(small, "a", "SYN_a_ISO100.png"), 80, 272)
    said = refused(f"x/{LEAF}/a/ISO800/SYN_a_ISO800_3_1_96.png", small)
    assert "SYN_a_ISO800_1_1_96.png" in said and "308 x 500" in said
    with pytest.raises(FileNotFoundError, match="SYN_a_ISO800_3_1_96.png"):
        ValidationSet.from_full_size([[f"x/{LEAF}/a/ISO100/SYN_a_ISO100_3_1_96.png", f"x/{LEAF}/a/ISO800/SYN_a_ISO800_3_1_96.png"]],
                                     small, CS, STRIDE, "cpu", 104)


def test_mixed_pairs_and_pairs_of_another_tree(tree, tmp_path):
    inside = os.path.join(tree["cropped"], "bark", "ISO100", "SYN_bark_ISO100_1_1_96.png")
    outside = str(tmp_path / "elsewhere_128_96" / "bark" / "ISO800" / "SYN_bark_ISO800_1_1_96.png")
    with pytest.raises(ValueError) as e:
        ValidationSet.from_full_size([[inside, outside]], tree["dsdir"], CS, STRIDE, "cpu", 104)
    assert inside in str(e.value) and outside in str(e.value)
    # a pair under another leaf is read from disk, as the constructor reads it: absent, the codec's FileNotFoundError
    with pytest.raises(FileNotFoundError) as e:
        ValidationSet.from_full_size([[outside.replace("ISO800", "ISO100"), outside]], tree["dsdir"], CS, STRIDE, "cpu", 104)
    assert str(e.value) == outside.replace("ISO800", "ISO100")
    # present, its samples, beside a window
    os.makedirs(os.path.dirname(outside))
    shutil.copy(os.path.join(tree["cropped"], "bark", "ISO800", "SYN_bark_ISO800_1_1_96.png"), outside)
    noisy = os.path.join(tree["cropped"], "bark", "ISO800", "SYN_bark_ISO800_1_1_96.png")
    got = ValidationSet.from_full_size([[outside, outside], [inside, noisy]], tree["dsdir"], CS, STRIDE, "cpu", 104)
    want = ValidationSet([[noisy, noisy], [inside, noisy]], "cpu", 104)
    assert np.array_equal(words(got.clean), words(want.clean)) and np.array_equal(words(got.noisy), words(want.noisy))
    assert (got.n_windows, got.n_full_size_images) == (1, 2)


# ------------------------------------------------------------------ pick_validation_set
def test_pick_validation_set_writes_one_list_from_either_tree(tree, from_files, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with open("test_set_syn.yaml", "w") as fp:
        yaml.dump(["bark", "alley"], fp)
    full = ["--full_size_data", tree["dsdir"], "--ds_cs", str(CS), "--ds_stride", str(STRIDE)]
    common = ["--test_reserve", "test_set_syn.yaml", "--seed", "3", "--num_crops", "7"]
    assert pick_validation_set.main(common + full) == 0
    default = os.path.join("configs", f"validation_set_7_{LEAF}_test_set_syn.yaml")
    assert "0 candidate pair(s) left out" in capsys.readouterr().out
    assert pick_validation_set.main(common + ["--train_data", tree["cropped"], "--out", "from_crops.yaml"]) == 0
    with open(default, "rb") as f1, open("from_crops.yaml", "rb") as f2:
        written = f1.read()
        assert written == f2.read()
    pairs = yaml.safe_load(written)
    assert len(pairs) == 7 and all(len(p) == 2 and os.path.isfile(p[0]) and os.path.isfile(p[1]) for p in pairs)
    assert all(p[0].startswith(tree["cropped"] + os.sep) and "/ISO100/" in p[0] and "/ISO100/" not in p[1] for p in pairs)
    got, want = ValidationSet.from_full_size(default, tree["dsdir"], CS, STRIDE, "cpu", 104), ValidationSet(default, "cpu", 104)
    assert np.array_equal(words(got.clean), words(want.clean)) and np.array_equal(words(got.noisy), words(want.noisy)) and got.n_windows == 7
    # a second run: the reference's message, and the file as it was; --overwrite, and another seed, another list
    with pytest.raises(SystemExit) as e:
        pick_validation_set.main(common + full)
    assert str(e.value) == f"{default} exists and args.overwrite is not set"
    assert pick_validation_set.main(["--test_reserve", "test_set_syn.yaml", "--seed", "4", "--num_crops", "7", "--overwrite"] + full) == 0
    with open(default, "rb") as f1:
        assert f1.read() != written
    # 3 x 12 + 2 x 4 candidates
    assert pick_validation_set.main(common[:-1] + ["44", "--out", "all.yaml"] + full) == 0
    with open("all.yaml") as fp:
        assert {p[0].split(os.sep)[-3] for p in yaml.safe_load(fp)} == {"bark", "alley"}
    with pytest.raises(ValueError) as e:
        pick_validation_set.main(common[:-1] + ["45", "--out", "more.yaml"] + full)
    assert "45" in str(e.value) and "44" in str(e.value) and not os.path.exists("more.yaml")
    with pytest.raises(ValueError, match="44"):
        pick_validation_set.main(common[:-1] + ["45", "--out", "more.yaml", "--train_data", tree["cropped"]])


def test_pick_validation_set_takes_sets_by_exact_name(tree, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    with open("reserve.yaml", "w") as fp:
        yaml.dump(["bar", "alleyway", "lley"], fp)       # the dataset's substring rule would reserve bark and alley for "bar" and "lley"
    for data in (["--full_size_data", tree["dsdir"], "--ds_cs", str(CS), "--ds_stride", str(STRIDE)], ["--train_data", tree["cropped"]]):
        with pytest.raises(ValueError, match=" 0 candidate"):
            pick_validation_set.main(["--test_reserve", "reserve.yaml", "--num_crops", "1"] + data)
    # set names on the command line need --out: the default name is the yaml file's
    with pytest.raises(SystemExit):
        pick_validation_set.main(["--test_reserve", "alley", "--num_crops", "1", "--train_data", tree["cropped"]])
    assert "--out" in capsys.readouterr().err
    assert pick_validation_set.main(["--test_reserve", "alley", "--num_crops", "8", "--out", "a.yaml", "--train_data", tree["cropped"]]) == 0
    with open("a.yaml") as fp:
        assert {p[1].split(os.sep)[-3] for p in yaml.safe_load(fp)} == {"alley"}


def test_a_noisy_crop_its_own_grid_does_not_yield_is_skipped_and_counted(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    small = write_full_size(str(tmp_path), "SYN", 404, 500, sets=("a",), isos=("ISO100", "ISO800"))
    imgcodec.write_png(os.path.join(small, "a", "SYN_a_ISO800.png"), image_u(500, 308, 3))      # 2 columns of the base ISO's 3
    argv = ["--test_reserve", "a", "--out", "v.yaml", "--full_size_data", small, "--ds_cs", str(CS), "--ds_stride", str(STRIDE), "--num_crops"]
    assert pick_validation_set.main(argv + ["8"]) == 0
    assert "4 candidate pair(s) left out" in capsys.readouterr().out
    with open("v.yaml") as fp:
        pairs = yaml.safe_load(fp)
    assert len(pairs) == 8 and not any(p[1].split("_")[-3] == "3" for p in pairs)
    assert ValidationSet.from_full_size(pairs, small, CS, STRIDE, "cpu", 104).n_windows == 8
    with pytest.raises(ValueError, match="8 candidate"):
        pick_validation_set.main(argv + ["9", "--overwrite"])
