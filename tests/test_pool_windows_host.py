"""CPU tests of the crop pool over full-size images (crop_pool.crop_grid, CropPool.add_frame / add_window_group /
from_full_size, and the options of nn_train and tools.make_dataset_crops_list): the grid against what the reference's own
crop_img.sh issued (tests/golden/make_golden_crop_grid.py), the scan against from_directories on a tree that this file's own
cropper writes, the bytes held, and the parser.  tests/test_pool_windows.py runs the kernels."""
import json
import os

import numpy as np
import pytest

from nind_denoise_amd import nn_train
from nind_denoise_amd.common.libs import imgcodec, np_imgops
from nind_denoise_amd.crop_pool import CropPool, crop_grid, findisoval
from nind_denoise_amd.tools import make_dataset_crops_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ trees (shared with test_pool_windows.py)
def image_u(h, w, seed, dtype=np.uint8):
    """[h, w, 3] samples, smooth enough to score and different at every pixel's neighbourhood"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    top = np.iinfo(dtype).max
    img = np.stack([0.5 + 0.4 * np.sin(yy / (7 + c) + seed) * np.cos(xx / (11 - c)) for c in range(3)], axis=2)
    return np.clip((img + rng.normal(0, 0.03, img.shape)) * top, 0, top).astype(dtype)


def write_full_size(root, name, width, height, dtype=np.uint8, sets=("bark", "alley"), isos=("ISO100", "ISO800", "ISO6400")):
    """<root>/<name>/<set>/<name>_<set>_<ISO>.png: the first ISO is the base, the others add noise to it.  Returns the directory."""
    dsdir = os.path.join(root, name)
    top = np.iinfo(dtype).max
    for s, aset in enumerate(sets):
        os.makedirs(os.path.join(dsdir, aset))
        clean = image_u(height, width, 10 * s + 1, dtype)
        for k, iso in enumerate(isos):
            rng = np.random.default_rng(100 * s + k)
            img = clean if k == 0 else np.clip(clean.astype(np.float64) + rng.normal(0, 0.02 * k * top, clean.shape), 0, top).astype(dtype)
            imgcodec.write_png(os.path.join(dsdir, aset, f"{name}_{aset}_{iso}.png"), img)
    return dsdir


def crop_tree(dsdir, cs, stride):
    """This file's cropper: crop_grid, numpy slicing and imgcodec.write_png, into the directory the reference's cropper would have
    made, <root of dsdir>/cropped/<leaf>_<cs>_<stride>/<set>/<ISO>/<basename>_<xcrop>_<ycrop>_<stride>.png.  Returns it."""
    out = os.path.join(os.path.dirname(dsdir), "cropped", f"{os.path.basename(dsdir)}_{cs}_{stride}")
    for aset in os.listdir(dsdir):
        for fn in os.listdir(os.path.join(dsdir, aset)):
            iso = findisoval(fn)
            os.makedirs(os.path.join(out, aset, iso), exist_ok=True)
            img = np_imgops.img_path_to_np_samples(os.path.join(dsdir, aset, fn)).transpose(1, 2, 0)
            for xc, yc, xb, yb in crop_grid(img.shape[1], img.shape[0], cs, stride):
                imgcodec.write_png(os.path.join(out, aset, iso, f"{fn[:-4]}_{xc}_{yc}_{stride}.png"),
                                   np.ascontiguousarray(img[yb:yb + cs, xb:xb + cs]))
    return out


# ------------------------------------------------------------------ crop_grid
with open(os.path.join(ROOT, "tests", "golden", "crop_grid.json")) as _f:
    GRID_CASES = json.load(_f)


def test_the_fixture_covers_the_cases_that_matter():
    have = {(c["width"], c["height"], c["cs"], c["stride"]) for c in GRID_CASES}
    assert {(812, 620, 128, 96), (768, 620, 128, 96), (6000, 4000, 256, 192), (300, 200, 256, 192)} <= have
    assert any(c["width"] == c["cs"] + (c["cs"] - c["stride"]) // 2 for c in GRID_CASES)
    assert [c for c in GRID_CASES if (c["width"], c["height"]) == (300, 200)][0]["crops"] == []
    assert any(c["ext"] == "jpg" for c in GRID_CASES) and sum(len(c["crops"]) for c in GRID_CASES) > 700


@pytest.mark.parametrize("case", GRID_CASES, ids=[f"{c['width']}x{c['height']}-{c['cs']}-{c['stride']}-{c['ext']}" for c in GRID_CASES])
def test_crop_grid_is_what_the_script_issued(case):
    cs, stride = case["cs"], case["stride"]
    grid = crop_grid(case["width"], case["height"], cs, stride)
    mine = [{"geometry": f"{cs}x{cs}+{xb}+{yb}", "name": f"{case['basename']}_{xc}_{yc}_{stride}.{case['ext']}"}
            for xc, yc, xb, yb in grid]
    assert len(mine) == len(case["crops"])
    for k, (m, ref) in enumerate(zip(mine, case["crops"])):      # entry by entry, in the script's order
        assert m == ref, (k, m, ref)
    for xc, yc, xb, yb in grid:                                    # and every crop lies inside the image
        assert 0 <= xb and xb + cs <= case["width"] and 0 <= yb and yb + cs <= case["height"]


@pytest.mark.parametrize("cs,stride", [(100, 96), (128, 100), (129, 96), (128, 4), (-8, 8), (128, 0)])
def test_crop_grid_refuses_what_the_script_refuses(cs, stride):
    with pytest.raises(ValueError, match="crop_grid"):
        crop_grid(812, 620, cs, stride)


def test_findisoval():
    assert findisoval("NIND_bark_ISO6400.png") == "ISO6400"
    assert findisoval("NIND_two_words_ISOH1.tif") == "ISOH1"
    assert findisoval("0001_GT_SRGB_010.PNG") == "GT_SRGB_010"
    assert findisoval("0001_NOISY_SRGB_010.PNG") == "NOISY_SRGB_010"
    assert findisoval("plain.png") is None


# ------------------------------------------------------------------ from_full_size against the cropped tree
CS, STRIDE = 128, 96


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fullsize"))
    dsdir = write_full_size(root, "SYN", 812, 620)
    return {"root": root, "dsdir": dsdir, "cropped": crop_tree(dsdir, CS, STRIDE)}


@pytest.fixture(scope="module")
def pools(trees):
    return (CropPool.from_full_size(trees["dsdir"], ds_cs=CS, ds_stride=STRIDE, device="cpu"),
            CropPool.from_directories(trees["cropped"], device="cpu"))


def test_from_full_size_is_from_directories_on_the_cropped_tree(trees, pools):
    wp, dp = pools
    assert wp.n_groups == dp.n_groups == 2 * 35 and wp.n_images == dp.n_images == 2 * 35 * 3
    assert wp.sets == dp.sets and wp.datadirs == dp.datadirs == [trees["cropped"]] and wp.dsname == dp.dsname == "SYN_128_96"
    assert wp.pair_paths() == dp.pair_paths()
    assert all(os.path.isfile(p) for pair in wp.pair_paths() for p in pair)        # the names are the crop files'
    assert np.array_equal(wp.pair_table(), dp.pair_table())
    assert [wp.group(g) for g in range(wp.n_groups)] == [dp.group(g) for g in range(dp.n_groups)]
    assert wp.cs == dp.cs == CS
    assert wp.windowed and not dp.windowed and wp.n_frames == 6 and dp.n_frames == 0
    # sets in sorted order, one base ISO and two noisy ones, crop names in sorted file-name order (10_1 before 1_1 before 2_1)
    assert [s[1] for s in wp.sets[::35]] == ["alley", "bark"]
    assert wp.sets[0][3:] == (("ISO100",), ("ISO800", "ISO6400"))
    names = [s[2] for s in wp.sets[:35]]
    assert names == sorted(names) and names[0] == "SYN_alley_ISO800_1_1_96.png"


def test_every_image_is_the_crop_files_samples(pools):
    wp, dp = pools
    for i in range(wp.n_images):
        a, b = wp.image(i), dp.image(i)
        assert a.dtype == b.dtype == np.uint8 and a.shape == b.shape == (3, CS, CS) and np.array_equal(a, b), i


def test_frames_are_counted_once(pools):
    wp, dp = pools
    frame = (3 * 620 * 812 + 15) // 16 * 16
    assert wp.nbytes == 6 * frame                                  # the frames' bytes, each aligned to 16
    assert dp.nbytes == 2 * 35 * 3 * 3 * CS * CS                   # every crop file: 1.14 times as much here, 1.8 at 256/192 on NIND
    assert wp.nbytes < dp.nbytes


def test_keep_groups_drops_the_frames_no_group_names(trees):
    wp = CropPool.from_full_size(trees["dsdir"], ds_cs=CS, ds_stride=STRIDE, device="cpu")
    dp = CropPool.from_directories(trees["cropped"], device="cpu")
    wp.keep_groups(12)
    dp.keep_groups(12)
    assert wp.n_groups == 12 and wp.n_frames == 3 and wp.nbytes == 3 * ((3 * 620 * 812 + 15) // 16 * 16)
    assert wp.sets == dp.sets and np.array_equal(wp.pair_table(), dp.pair_table())
    assert all(np.array_equal(wp.image(i), dp.image(i)) for i in range(wp.n_images))


def test_reserved_sets_and_a_set_without_crops(trees, tmp_path):
    wp = CropPool.from_full_size([trees["dsdir"]], ds_cs=CS, ds_stride=STRIDE, test_reserve=["bark"], device="cpu")
    assert wp.n_groups == 35 and wp.n_frames == 3 and {s[1] for s in wp.sets} == {"alley"}
    small = write_full_size(str(tmp_path), "TINY", 200, 150, sets=("a",))
    assert CropPool.from_full_size(small, ds_cs=CS, ds_stride=STRIDE, device="cpu").n_groups == 0
    wp = CropPool.from_full_size(trees["dsdir"], ds_cs=CS, ds_stride=STRIDE, crops_dir="/elsewhere/X_128_96", device="cpu")
    assert wp.pair_paths()[0][0] == "/elsewhere/X_128_96/alley/ISO100/SYN_alley_ISO100_1_1_96.png" and wp.dsname == "X_128_96"
    with pytest.raises(ValueError, match="crop_grid"):
        CropPool.from_full_size(trees["dsdir"], ds_cs=100, ds_stride=96, device="cpu")


def test_an_iso_of_another_size_names_the_missing_crop_file(tmp_path):
    dsdir = write_full_size(str(tmp_path), "SYN", 404, 500, sets=("a",), isos=("ISO100", "ISO800"))
    imgcodec.write_png(os.path.join(dsdir, "a", "SYN_a_ISO100.png"), image_u(500, 308, 3))      # one column of crops fewer
    cropped = crop_tree(dsdir, CS, STRIDE)
    with pytest.raises(FileNotFoundError) as dense:
        CropPool.from_directories(cropped, device="cpu")
    with pytest.raises(FileNotFoundError) as windows:
        CropPool.from_full_size(dsdir, ds_cs=CS, ds_stride=STRIDE, device="cpu")
    assert str(windows.value) == str(dense.value) and str(dense.value).endswith("cropped/SYN_128_96/a/ISO100/SYN_a_ISO100_3_1_96.png")


def test_duplicate_isos_are_named_in_sorted_file_order(tmp_path):
    dsdir = os.path.join(str(tmp_path), "DUP")
    os.makedirs(os.path.join(dsdir, "s"))
    for fn, seed in (("DUP_s_ISO100.png", 1), ("DUP_s_ISO800.png", 2), ("DUP_s_ISO800_b.png", 3), ("DUP_s_ISO800_c.png", 4)):
        imgcodec.write_png(os.path.join(dsdir, "s", fn), image_u(300, 308, seed))
    # _b is ISO800-2 and _c ISO800-2-2; sortISOs puts the repeats first, so the groups are named after ISO800-2's crops.  Crop names
    # of a set must differ by their ISO alone (from_directories forms one from another), which these do not: the error names the
    # crop file of ISO800-2-2 that the cropped tree would lack, and with it the names the ISOs got
    with pytest.raises(FileNotFoundError) as e:
        CropPool.from_full_size(dsdir, ds_cs=CS, ds_stride=STRIDE, device="cpu")
    assert str(e.value).endswith("cropped/DUP_128_96/s/ISO800-2-2/DUP_s_ISO800-2-2_b_1_1_96.png"), str(e.value)
    assert sorted(os.listdir(os.path.join(dsdir, "s"))) == ["DUP_s_ISO100.png", "DUP_s_ISO800.png", "DUP_s_ISO800_b.png", "DUP_s_ISO800_c.png"]


# ------------------------------------------------------------------ windows by hand
def test_a_pool_holds_dense_images_or_windows_not_both():
    frame = np.arange(3 * 20 * 30, dtype=np.uint16).reshape(3, 20, 30)
    pool = CropPool(device="cpu")
    f = pool.add_frame(frame)
    g = pool.add_window_group([f], [f], 2, 3, 8, 9)
    assert pool.group(g) == ([0], [0], 8, 9) and pool.n_images == 1                # equal lists: the images are shared
    assert np.array_equal(pool.image(0), frame[:, 2:10, 3:12])
    with pytest.raises(ValueError, match="not both"):
        pool.add_group([frame], [frame + 1])
    dense = CropPool(device="cpu")
    dense.add_group([frame], [frame + 1])
    with pytest.raises(ValueError, match="not both"):
        dense.add_frame(frame)
    with pytest.raises(ValueError, match="no frame"):
        dense.add_window_group([0], [0], 0, 0, 4, 4)
    for y, x, h, w in ((13, 0, 8, 8), (0, 22, 8, 9), (-1, 0, 4, 4), (0, 0, 0, 4), (0, 0, 21, 30)):
        with pytest.raises(ValueError, match="does not lie inside"):
            pool.add_window_group([f], [f], y, x, h, w)
    with pytest.raises(ValueError, match="frame 1 outside"):
        pool.add_window_group([1], [f], 0, 0, 4, 4)


# ------------------------------------------------------------------ parser
BASE = ["--test_reserve", "0", "--batch_size", "4"]
EXISTING = [
    BASE + ["--train_data", "datasets/train/NIND_256_192"],
    BASE + ["--train_data", "a_128_96", "b_128_96", "--cs", "104", "--loss_cs", "60", "--min_crop_size", "104", "--gpus", "2"],
    BASE + ["--train_data", "x", "--min_quality", "0.6", "--quality_csv", "f.csv", "--save_state", "--g_clip_norm", "0.5"],
    BASE,
]


@pytest.mark.parametrize("argv", EXISTING, ids=range(len(EXISTING)))
def test_an_existing_command_line_parses_to_what_it_did(argv, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)                 # no default config files
    args = vars(nn_train.parse_args(argv))
    assert not {"full_size_data", "ds_cs", "ds_stride"} & set(args)
    assert nn_train.full_size_options(nn_train.parse_args(argv)) == (None, 256, 192)
    if "--loss_cs" not in argv:
        assert args["loss_cs"] is None          # still left to the directory's name, in run()


def test_the_new_options_parse(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = nn_train.parse_args(BASE + ["--full_size_data", "datasets/NIND", "datasets/SIDD"])
    assert args.full_size_data == ["datasets/NIND", "datasets/SIDD"] and args.train_data is None
    assert nn_train.full_size_options(args) == (["datasets/NIND", "datasets/SIDD"], 256, 192)
    assert args.loss_cs == 192                  # the <UCS> of the directory the cropper would have made
    args = nn_train.parse_args(BASE + ["--full_size_data", "d", "--ds_cs", "128", "--ds_stride", "96", "--min_crop_size", "104"])
    assert (args.ds_cs, args.ds_stride, args.loss_cs, args.min_crop_size) == (128, 96, 96, 104)
    assert nn_train.parse_args(BASE + ["--full_size_data", "d", "--ds_stride", "96", "--loss_cs", "60"]).loss_cs == 60
    with open("conf.yaml", "w") as f:
        f.write("full_size_data: [d1]\nds_cs: 176\nds_stride: 128\n")
    args = nn_train.parse_args(BASE + ["--config", "conf.yaml"])
    assert nn_train.full_size_options(args) == (["d1"], 176, 128) and args.loss_cs == 128


def test_train_data_beside_full_size_data_is_refused(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    for parse in (nn_train.parse_args, make_dataset_crops_list.parse_args):
        with pytest.raises(SystemExit):
            parse(BASE + ["--train_data", "a_128_96", "--full_size_data", "d"])
        err = capsys.readouterr().err
        assert "--train_data" in err and "--full_size_data" in err


def test_make_dataset_crops_list_takes_the_options(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    args = make_dataset_crops_list.parse_args(["--test_reserve", "0", "--full_size_data", "d", "--ds_cs", "176", "--ds_stride", "128"])
    assert nn_train.full_size_options(args) == (["d"], 176, 128) and not args.train_data
    args = make_dataset_crops_list.parse_args(["--test_reserve", "0", "--train_data", "a_128_96"])
    assert not {"full_size_data", "ds_cs", "ds_stride"} & set(vars(args))
    with pytest.raises(SystemExit):
        make_dataset_crops_list.parse_args(["--test_reserve", "0"])
    assert "--train_data or --full_size_data" in capsys.readouterr().err
