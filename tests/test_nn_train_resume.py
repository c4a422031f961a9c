"""GPU tests of nn_train --save_state / --resume and of the guard options of the command: a run stopped after epoch k and resumed
to epoch N leaves the same bits as the uninterrupted run -- the last checkpoint, the tensors and fields of train_state.pt, the
entries of trainres.json and the pool's next draw -- plainly, with a quality bar that lifts inside the resumed part, with clipping
and skipping on, and over two gloo ranks on the one GPU; and the options' own figures in trainres.json and the log.

A synthetic tree of 24 groups of 128 x 128 8-bit pairs; UtNet funit 16 on 104 x 104 crops, batch 4 (6 steps per epoch), MSE + L1,
no validation.  Everything compared is compared as bits."""
import json
import os
import re
import socket
from datetime import timedelta

import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib
from nind_denoise_amd.common.libs import imgcodec

pytestmark = pytest.mark.gpu

FUNIT, SIDE, CS, LOSS_CS, BATCH, GROUPS = 16, 128, 104, 96, 4, 24
START_TIMEOUT_S = 300


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def image_like(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    c = F.interpolate(torch.rand(n, 3, h // 8, w // 8, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * c + 0.1 + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)


def make_tree(root):
    """<root>/synth_128_96/<set>/ISO*/: 24 groups (six sets of four crops, a clean ISO and a noisy one)"""
    data = os.path.join(root, f"synth_{SIDE}_{LOSS_CS}")
    clean = image_like(GROUPS, SIDE, SIDE, seed=41)
    g = torch.Generator().manual_seed(42)
    noisy = (clean + 0.04 * torch.randn(clean.shape, generator=g)).clip(0, 1)
    for k in range(GROUPS):
        aset, crop = f"set{k // 4}", f"{k % 4}_0"
        for iso, img in (("ISO100", clean[k]), ("ISO6400", noisy[k])):
            os.makedirs(os.path.join(data, aset, iso), exist_ok=True)
            imgcodec.write_png(os.path.join(data, aset, iso, f"synth_{aset}_{iso}_{crop}_{LOSS_CS}.png"),
                               (img * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous().numpy())
    return data


def fresh_pool(data, dev):
    from nind_denoise_amd.crop_pool import CropPool
    return CropPool.from_directories([data], test_reserve=[], cs=CS, device=dev, seed=7)


@pytest.fixture(scope="module")
def tree(tmp_path_factory, dev):
    root = str(tmp_path_factory.mktemp("resume"))
    data = make_tree(root)
    # scores for --quality_csv (the files are below MS-SSIM's 161 pixels): two groups of three pass a bar of 0.5
    pool = fresh_pool(data, dev)
    csv_path = os.path.join(root, "scores.csv")
    with open(csv_path, "w") as f:
        f.write("xpath,ypath,score\n")
        for k, (x, y) in enumerate(pool.pair_paths()):
            f.write(f"{x},{y},{0.25 if k % 3 == 0 else 0.75}\n")
    return {"root": root, "data": data, "csv": csv_path}


def train_argv(tree, models, expname, epochs, extra=()):
    return ["--g_funit", str(FUNIT), "--cs", str(CS), "--batch_size", str(BATCH), "--weight_MSE", "0.5", "--weight_L1", "0.5",
            "--g_lr", "1e-3", "--epochs", str(epochs), "--patience", "1", "--seed", "7", "--beta1", "0.75", "--reduce_lr_factor", "0.5",
            "--train_data", tree["data"], "--test_reserve", "0", "--validation_interval", "0", "--models_dpath", models,
            "--expname", expname, "--log_interval", "0", "--save_state"] + list(extra)


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def load_state(run):
    return torch.load(os.path.join(run, "train_state.pt"), map_location="cpu", weights_only=True)


def assert_same_run(straight, resumed, last, data, dev):
    """the claim: everything a run leaves that the next epoch, or a reader, would look at"""
    a = torch.load(os.path.join(straight, f"generator_{last}.pt"), map_location="cpu", weights_only=True)
    b = torch.load(os.path.join(resumed, f"generator_{last}.pt"), map_location="cpu", weights_only=True)
    assert list(a) == list(b) and all(bits_equal(a[k], b[k]) for k in a)
    sa, sb = load_state(straight), load_state(resumed)
    assert set(sa) == set(sb) and sa["epoch"] == sb["epoch"] == last
    for key in sa:
        if key == "trainer":
            assert set(sa[key]) == set(sb[key])
            for k, v in sa[key].items():
                assert bits_equal(v, sb[key][k]) if torch.is_tensor(v) else v == sb[key][k], k
        elif torch.is_tensor(sa[key]):
            assert bits_equal(sa[key], sb[key]), key
        else:
            assert sa[key] == sb[key], key
    assert sa["trainer"]["steps"] > 0 and sa["trainer"]["m"].abs().max() > 0
    with open(os.path.join(straight, "trainres.json"), "rb") as f1, open(os.path.join(resumed, "trainres.json"), "rb") as f2:
        ra, rb = f1.read(), f2.read()
    assert json.loads(ra) == json.loads(rb) and ra == rb
    assert {str(e) for e in range(1, last + 1)} <= set(json.loads(ra))
    # the pool's next draw, from each state
    pool = fresh_pool(data, dev)
    assert not bits_equal(pool.rng_state(), sa["pool_rng_state"])
    draws = []
    for state in (sa, sb):
        pool.set_rng_state(state["pool_rng_state"])
        draws.append(pool.draw(BATCH).table.clone())
    assert bits_equal(draws[0].cpu(), draws[1].cpu())
    return sa


def straight_and_resumed(tree, name, extra, dev, stop=3, end=5):
    from nind_denoise_amd import nn_train
    models = os.path.join(tree["root"], "models_" + name)
    assert nn_train.main(train_argv(tree, models, "straight", end, extra)) == 0
    assert nn_train.main(train_argv(tree, models, "stopped", stop, extra)) == 0
    stopped = os.path.join(models, "stopped")
    assert load_state(stopped)["epoch"] == stop - 1
    assert nn_train.main(["--resume", stopped, "--epochs", str(end)]) == 0
    state = assert_same_run(os.path.join(models, "straight"), stopped, end - 1, tree["data"], dev)
    with open(os.path.join(stopped, "train.log")) as f:
        log = f.read()
    for epoch in range(1, end):
        assert log.count(f"Epoch {epoch} summary:") == 1, epoch
    assert log.count("Resumed from") == 1
    assert sorted(f for f in os.listdir(stopped) if not f.startswith("generator_")) == ["config.yaml", "train.log", "train_state.pt",
                                                                                       "trainres.json"]
    return state, log, stopped


# the log of a run with --validation_interval 0 and --log_interval 0, numbers replaced by #, as the revision before the options wrote it
TODAYS_LINES = {
    "test_reserve: []", "Crop pool: # groups, # images, # MB in HBM; # steps per epoch", "delete_outperformed_models removed []",
    "Epoch # summary:", "Time elapsed (s): # (epoch), # (total)", "Generator:", "Average weighted loss: #",
}


def test_resumed_run_equals_the_straight_run(dev, tree):
    state, log, run = straight_and_resumed(tree, "plain", [], dev)
    assert state["world"] == 1 and state["pool_groups"] == GROUPS and state["trainer"]["steps"] == 4 * (GROUPS // BATCH)
    print(f"loss history {state['loss_hist']}, learning rate {state['gen_lr']}")
    # a run without the option leaves no state file, and cannot be resumed
    from nind_denoise_amd import nn_train
    models = os.path.join(tree["root"], "models_nostate")
    argv = [a for a in train_argv(tree, models, "plain", 2) if a != "--save_state"]
    assert nn_train.main(argv) == 0
    assert sorted(os.listdir(os.path.join(models, "plain"))) == ["config.yaml", "generator_1.pt", "train.log", "trainres.json"]
    with pytest.raises(ValueError, match="train_state.pt"):
        nn_train.main(["--resume", os.path.join(models, "plain"), "--epochs", "3"])
    # the first epoch of the plain run is the first epoch of the run with the option
    a = torch.load(os.path.join(models, "plain", "generator_1.pt"), map_location="cpu", weights_only=True)
    with open(os.path.join(models, "plain", "trainres.json")) as f:
        first = json.load(f)["1"]
    with open(os.path.join(run, "trainres.json")) as f:
        assert json.load(f)["1"] == first and set(first) == {"train_weighted_loss", "gen_lr"}
    assert all(torch.isfinite(v).all() for v in a.values())
    # and its log is made of the lines a run wrote before the options existed
    with open(os.path.join(models, "plain", "train.log")) as f:
        templates = {re.sub(r"\d+(\.\d+)?(e-?\d+)?", "#", line) for line in f.read().splitlines() if not line.startswith(("Namespace(", "cmd: "))}
    assert templates <= TODAYS_LINES, templates - TODAYS_LINES
    assert {"Epoch # summary:", "Average weighted loss: #", "Generator:"} <= templates


def test_resumed_run_lifts_the_quality_bar_where_the_straight_run_does(dev, tree):
    extra = ["--min_quality", "0.5", "--min_quality_epochs", "2", "--quality_csv", tree["csv"]]
    state, log, _ = straight_and_resumed(tree, "quality", extra, dev)
    assert state["quality_bar_active"] is False
    assert log.count("Quality bar lifted after 2 epoch(s)") == 1 and log.count("Quality bar: MS-SSIM > 0.5") == 2
    assert log.index("Resumed from") < log.index("Quality bar lifted")
    assert state["trainer"]["steps"] == 2 * 4 + 2 * 6         # 16 of 24 groups for two epochs, then all


def test_resumed_run_with_clipping_and_skipping(dev, tree):
    extra = ["--g_clip_norm", "0.05", "--skip_nonfinite_steps"]
    state, log, run = straight_and_resumed(tree, "guard", extra, dev)
    assert state["trainer"]["max_grad_norm"] == 0.05 and state["trainer"]["skip_nonfinite"] is True
    with open(os.path.join(run, "trainres.json")) as f:
        res = json.load(f)
    for e in "1234":
        assert {"grad_norm_mean", "clipped_steps", "skipped_steps"} <= set(res[e]) and res[e]["skipped_steps"] == 0
    assert log.count("Gradient norm: mean") == 4


# ------------------------------------------------------------------ the options' own figures
def plant_nans(monkeypatch, calls):
    """CropPool.batch hands out a noisy batch with one NaN pixel at its calls number `calls` (counted from 1)"""
    from nind_denoise_amd.crop_pool import CropPool
    batch, count = CropPool.batch, [0]

    def planted(self, *args, **kwargs):
        clean, noisy = batch(self, *args, **kwargs)
        count[0] += 1
        if count[0] in calls:
            noisy = noisy.clone()
            noisy[1, 0, 40, 41] = float("nan")
        return clean, noisy
    monkeypatch.setattr(CropPool, "batch", planted)
    return count


def test_guard_options_are_counted_in_the_results(dev, tree, monkeypatch):
    from nind_denoise_amd import nn_train
    models = os.path.join(tree["root"], "models_options")
    count = plant_nans(monkeypatch, {2, 9, 10})         # step 2 of epoch 1; steps 3 and 4 of epoch 2
    extra = ["--g_clip_norm", "1e-4", "--skip_nonfinite_steps", "--max_skipped_steps", "2"]
    assert nn_train.main(train_argv(tree, models, "counted", 3, extra)) == 0
    assert count[0] == 12
    run = os.path.join(models, "counted")
    with open(os.path.join(run, "trainres.json")) as f:
        res = json.load(f)
    print(res)
    assert set(res["best_epoch"]) == set(res["best_val"]) == {"train_weighted_loss", "gen_lr"}     # the figures are no scores
    for e, skipped in (("1", 1), ("2", 2)):
        assert set(res[e]) == {"train_weighted_loss", "gen_lr", "grad_norm_mean", "clipped_steps", "skipped_steps"}
        assert res[e]["skipped_steps"] == skipped and res[e]["clipped_steps"] == 6 - skipped      # 1e-4 binds at every applied step
        assert 1e-4 < res[e]["grad_norm_mean"] < float("inf") and 0 < res[e]["train_weighted_loss"] < 1
    with open(os.path.join(run, "train.log")) as f:
        log = f.read()
    assert "clipped steps: 5, skipped steps: 1 (of 6)" in log and "clipped steps: 4, skipped steps: 2 (of 6)" in log
    sd = torch.load(os.path.join(run, "generator_2.pt"), map_location="cpu", weights_only=True)
    assert all(torch.isfinite(v).all() for v in sd.values())
    # without the options the same NaN reaches the parameters and the results
    count[0] = 0
    assert nn_train.main(train_argv(tree, models, "unguarded", 2)) == 0
    # (the criteria clip the output to [0, 1], which turns a NaN into a number: the loss of the ruined network stays finite, and
    # only the guard says that something happened)
    sd = torch.load(os.path.join(models, "unguarded", "generator_1.pt"), map_location="cpu", weights_only=True)
    assert not all(torch.isfinite(v).all() for v in sd.values())


def test_max_skipped_steps_ends_the_run_before_the_checkpoint(dev, tree, monkeypatch):
    from nind_denoise_amd import nn_train
    models = os.path.join(tree["root"], "models_maxskip")
    plant_nans(monkeypatch, {8})                        # step 2 of epoch 2
    extra = ["--skip_nonfinite_steps", "--max_skipped_steps", "0"]
    with pytest.raises(RuntimeError, match="epoch 2 skipped 1 of 6 steps"):
        nn_train.main(train_argv(tree, models, "run", 4, extra))
    run = os.path.join(models, "run")
    assert os.path.isfile(os.path.join(run, "generator_1.pt")) and not os.path.exists(os.path.join(run, "generator_2.pt"))
    assert load_state(run)["epoch"] == 1
    with open(os.path.join(run, "trainres.json")) as f:
        assert "2" not in json.load(f)


# ------------------------------------------------------------------ two ranks
def _rank_main(rank, world, port, tree, models, outq):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as tdist
    from nind_denoise_amd import nn_train
    torch.cuda.set_device(torch.device("cuda", 0))
    tdist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        group = tdist.group.WORLD
        extra = ["--g_clip_norm", "0.05", "--skip_nonfinite_steps"]
        for name, epochs in (("straight", 4), ("stopped", 3)):
            nn_train.run(nn_train.parse_args(train_argv(tree, models, name, epochs, extra)), group, argv=["nn_train.py"])
        stopped = os.path.join(models, "stopped")
        args = nn_train.parse_args(["--resume", stopped, "--epochs", "4"])
        nn_train.run(args, group, argv=["nn_train.py"])
        digest = {}
        for name in ("straight", "stopped"):
            sd = torch.load(os.path.join(models, name, "generator_3.pt"), map_location="cpu", weights_only=True)
            digest[name] = nn_train.parameters_digest(sd)
        # a world of one cannot take this run over
        refused = ""
        try:
            nn_train.check_resumable(nn_train.load_train_state(stopped), stopped, 1, GROUPS)
        except ValueError as e:
            refused = str(e)
        outq.put((rank, {"digest": digest, "refused": refused}))
    finally:
        tdist.destroy_process_group()


def test_two_ranks_resume_as_they_would_have_gone_on(dev, tree):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    models = os.path.join(tree["root"], "models_dp")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, tree, models, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=START_TIMEOUT_S) for _ in range(2))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    state = assert_same_run(os.path.join(models, "straight"), os.path.join(models, "stopped"), 3, tree["data"], dev)
    assert state["world"] == 2 and state["trainer"]["steps"] == 3 * (GROUPS // BATCH // 2)
    assert got[0]["digest"] == got[1]["digest"] and got[0]["digest"]["straight"] == got[0]["digest"]["stopped"]
    assert all("2 rank(s)" in got[r]["refused"] and "this one has 1" in got[r]["refused"] for r in range(2))
