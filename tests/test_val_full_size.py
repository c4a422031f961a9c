"""nn_train --full_size_data with validation, on the GPU, on a machine that holds no crop file: the validation pairs that
--validation_set_yaml names are windows into the full-size images of the reserved set (ValidationSet.from_full_size), and the run is
the run on the cropped tree, byte for byte.  tests/test_val_full_size_host.py holds the parts to their contracts on the CPU.

Sizes are those of tests/test_pool_windows.py (whose train_argv is the model): UtNet(8), 404 x 500 frames cut at 128 / 96, one
training set and one reserved set of 12 crops x (ISO100, ISO6400) each, 3 steps of 4 crops per epoch, 4 epochs.  The list is 6
pairs written by tools.pick_validation_set from the full-size tree; --val_batch_size 4 makes the second batch a partial one.
--patience 1 --reduce_lr_factor 0.5 with --g_lr 0.01: the validation loss of this run falls in epoch 1, rises in epoch 2 (0.218 to
0.247, while it keeps falling at 0.001 and 0.003) and falls again, so the learning rate is halved once, on the validation figure,
and the checkpoints compared were steered by it."""
import json
import os

import pytest
import torch

from nind_denoise_amd import _lib
from test_pool_windows_host import crop_tree, write_full_size

pytestmark = pytest.mark.gpu
FUNIT = 8
G_LR = 0.01
DS = ["--ds_cs", "128", "--ds_stride", "96"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture
def tree(tmp_path):
    """The full-size tree alone, and a list of 6 pairs of the reserved set's crops, none of which exists"""
    from nind_denoise_amd.tools import pick_validation_set
    root = str(tmp_path)
    dsdir = write_full_size(root, "SYN", 404, 500, sets=("bark", "alley"), isos=("ISO100", "ISO6400"))
    val_yaml = os.path.join(root, "validation_set_6.yaml")
    assert pick_validation_set.main(["--full_size_data", dsdir] + DS + ["--test_reserve", "bark", "--num_crops", "6", "--seed", "3",
                                                                         "--out", val_yaml]) == 0
    assert not os.path.exists(os.path.join(root, "cropped"))
    return {"root": root, "dsdir": dsdir, "val_yaml": val_yaml, "full": ["--full_size_data", dsdir] + DS}


def train_argv(tree, data, models, expname, epochs):
    return ["--g_funit", str(FUNIT), "--cs", "104", "--loss_cs", "60", "--batch_size", "4", "--weight_MSE", "1", "--g_lr", str(G_LR),
            "--epochs", str(epochs), "--patience", "1", "--seed", "7", "--beta1", "0.75", "--reduce_lr_factor", "0.5",
            "--test_reserve", "bark", "--validation_interval", "1", "--validation_set_yaml", tree["val_yaml"], "--val_batch_size", "4",
            "--models_dpath", models, "--expname", expname, "--log_interval", "0", "--g_network", "UtNet", "--save_state"] + list(data)


def same_file(a, b):
    with open(a, "rb") as f1, open(b, "rb") as f2:
        return f1.read() == f2.read()


def test_validation_windows_give_the_run_on_the_cropped_tree(tree, dev):
    from nind_denoise_amd import nn_train
    models = os.path.join(tree["root"], "models")
    assert nn_train.main(train_argv(tree, tree["full"], models, "windows", 4)) == 0      # (the parent commit: FileNotFoundError)
    assert not os.path.exists(os.path.join(tree["root"], "cropped"))
    cropped = crop_tree(tree["dsdir"], 128, 96)
    assert nn_train.main(train_argv(tree, ["--train_data", cropped], models, "files", 4)) == 0
    w, f = os.path.join(models, "windows"), os.path.join(models, "files")
    assert same_file(os.path.join(w, "trainres.json"), os.path.join(f, "trainres.json"))
    assert same_file(os.path.join(w, "generator_3.pt"), os.path.join(f, "generator_3.pt"))
    with open(os.path.join(w, "trainres.json")) as fp:
        res = json.load(fp)
    val = [res[e]["validation_loss"] for e in "0123"]
    assert all(isinstance(v, float) and 0 < v < 1 for v in val)
    print("validation_loss", val, "train_weighted_loss", [res[e]["train_weighted_loss"] for e in "123"], "gen_lr", [res[e]["gen_lr"] for e in "123"])
    assert any(res[e]["validation_loss"] != res[e]["train_weighted_loss"] for e in "123")
    # the rate was halved exactly where the validation loss rose above the epoch's before, and at least once
    lrs = [G_LR] + [res[e]["gen_lr"] for e in "123"]
    assert lrs[1] == G_LR and lrs[3] < G_LR
    for e in (2, 3):
        assert lrs[e] == (lrs[e - 1] * 0.5 if val[e] > val[e - 1] else lrs[e - 1]), (e, val, lrs)
    with open(os.path.join(w, "train.log")) as fp:
        log = fp.read()
    assert "Crop pool: 12 groups, 24 images (windows into 2 frames)" in log
    assert "Validation set: 6 pairs, 6 of them windows into 2 full-size images" in log
    assert log.index("Crop pool:") < log.index("Validation set:") < log.index("Validation loss:")
    with open(os.path.join(f, "train.log")) as fp:
        assert "Validation set:" not in fp.read()


def test_a_resumed_run_rebuilds_the_validation_windows(tree, dev):
    from nind_denoise_amd import nn_train
    models = os.path.join(tree["root"], "models_resume")
    assert nn_train.main(train_argv(tree, tree["full"], models, "straight", 4)) == 0
    assert nn_train.main(train_argv(tree, tree["full"], models, "stopped", 3)) == 0
    stopped = os.path.join(models, "stopped")
    assert not os.path.exists(os.path.join(stopped, "generator_3.pt"))
    assert nn_train.main(["--resume", stopped, "--epochs", "4"]) == 0
    assert not os.path.exists(os.path.join(tree["root"], "cropped"))
    assert same_file(os.path.join(stopped, "generator_3.pt"), os.path.join(models, "straight", "generator_3.pt"))
    assert same_file(os.path.join(stopped, "trainres.json"), os.path.join(models, "straight", "trainres.json"))
    with open(os.path.join(stopped, "trainres.json")) as fp:
        assert all("validation_loss" in entry for epoch, entry in json.load(fp).items() if epoch in ("0", "1", "2", "3"))
    with open(os.path.join(stopped, "train.log")) as fp:
        assert fp.read().count("Validation set: 6 pairs, 6 of them windows into 2 full-size images") == 2
