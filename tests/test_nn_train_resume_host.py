"""Host-side tests of nn_train --save_state / --resume (no GPU): the state file's round trip and its atomic replacement, every
refusal, the options of a resumed run, how the launcher learns a resumed run's ranks, the learning-rate rule across a save / restore
boundary, and the guard's figures in trainres.json."""
import collections
import os

import pytest
import torch
import yaml

from nind_denoise_amd import nn_train
from nind_denoise_amd.common.libs import json_saver


def make_state(epoch=2, **over):
    g = torch.Generator().manual_seed(epoch)
    trainer = {"kind": "UtNetTrainer", "funit": 8, "param_count": 10, "steps": 12, "lr": 5e-4, "betas": (0.75, 0.999), "eps": 1e-8,
               "amsgrad": True, "max_grad_norm": None, "skip_nonfinite": False}
    for key in ("flat", "m", "v", "vmax"):
        trainer[key] = torch.randn(10, generator=g)
    state = {"format": nn_train.STATE_FORMAT, "epoch": epoch, "trainer": trainer, "loss_hist": [0.5, 0.25], "gen_lr": 5e-4,
             "validation_loss": None, "pool_rng_state": torch.arange(16, dtype=torch.uint8), "quality_bar_active": False, "world": 1,
             "pool_groups": 24, "generator_sha256": "0" * 64}
    state.update(over)
    return state


def same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    if torch.is_tensor(a):
        return a.dtype == b.dtype and torch.equal(a, b)
    return a == b and type(a) is type(b)


# ------------------------------------------------------------------ the file
def test_state_file_round_trip(tmp_path):
    state = make_state()
    path = nn_train.save_train_state(str(tmp_path), state)
    assert path == str(tmp_path / nn_train.STATE_FNAME) and os.listdir(tmp_path) == [nn_train.STATE_FNAME]
    assert same(nn_train.load_train_state(str(tmp_path)), state)
    # only the latest is kept
    nn_train.save_train_state(str(tmp_path), make_state(3))
    assert os.listdir(tmp_path) == [nn_train.STATE_FNAME] and nn_train.load_train_state(str(tmp_path))["epoch"] == 3


def test_a_failed_write_leaves_the_old_file(tmp_path, monkeypatch):
    old = make_state(2)
    nn_train.save_train_state(str(tmp_path), old)
    synced = []
    fsync = os.fsync
    monkeypatch.setattr(os, "fsync", lambda fd: (synced.append(fd), fsync(fd))[1])

    def fail(src, dst):
        assert synced and os.path.isfile(src) and os.path.getsize(src) > 0        # written and flushed before the rename
        raise OSError("disk gone")
    monkeypatch.setattr(os, "replace", fail)
    with pytest.raises(OSError, match="disk gone"):
        nn_train.save_train_state(str(tmp_path), make_state(3))
    monkeypatch.undo()
    assert os.listdir(tmp_path) == [nn_train.STATE_FNAME]
    assert same(nn_train.load_train_state(str(tmp_path)), old)

    def fail_save(obj, f):
        f.write(b"half")
        raise RuntimeError("interrupted")
    monkeypatch.setattr(torch, "save", fail_save)
    with pytest.raises(RuntimeError, match="interrupted"):
        nn_train.save_train_state(str(tmp_path), make_state(3))
    monkeypatch.undo()
    assert os.listdir(tmp_path) == [nn_train.STATE_FNAME] and same(nn_train.load_train_state(str(tmp_path)), old)


# ------------------------------------------------------------------ refusals
def test_missing_and_newer_state_files_are_refused(tmp_path):
    with pytest.raises(ValueError, match="no train_state.pt"):
        nn_train.load_train_state(str(tmp_path))
    nn_train.save_train_state(str(tmp_path), make_state(format=nn_train.STATE_FORMAT + 1))
    with pytest.raises(ValueError, match=f"format {nn_train.STATE_FORMAT + 1}"):
        nn_train.load_train_state(str(tmp_path))
    torch.save({"something": 1}, str(tmp_path / nn_train.STATE_FNAME))
    with pytest.raises(ValueError, match="not a training state"):
        nn_train.load_train_state(str(tmp_path))


def test_another_world_pool_or_checkpoint_is_refused(tmp_path):
    run = str(tmp_path)
    state = make_state(world=2)
    nn_train.check_resumable(state, run, 2, 24)
    with pytest.raises(ValueError, match=r"2 rank\(s\), this one has 1"):
        nn_train.check_resumable(state, run, 1, 24)
    with pytest.raises(ValueError, match="holds 23 groups, the state was written with 24"):
        nn_train.check_resumable(state, run, 2, 23)
    # the checkpoint of the state's epoch: absent (pruned) is fine, another file is not
    ckpt = tmp_path / "generator_2.pt"
    ckpt.write_bytes(b"some checkpoint")
    with pytest.raises(ValueError, match="sha256 differs"):
        nn_train.check_resumable(state, run, 2, 24)
    nn_train.check_resumable(dict(state, generator_sha256=nn_train.file_sha256(str(ckpt))), run, 2, 24)


# ------------------------------------------------------------------ the options of a resumed run
def first_run_config(tmp_path, **over):
    args = nn_train.parse_args(["--test_reserve", "0", "--epochs", "3", "--min_quality", "0.5", "--min_quality_epochs", "2", "--start_epoch",
                                "4", "--g_clip_norm", "0.5", "--batch_size", "4", "--seed", "9", "--save_state"])
    conf = dict(vars(args), test_reserve=["setA", "setB"], loss_cs=96, cs=104)       # as run() leaves them: expanded, filled in
    conf.pop("resume")
    conf.update(over)
    run = tmp_path / "run"
    run.mkdir()
    with open(run / "config.yaml", "w") as f:
        yaml.dump(conf, f)
    return str(run), conf


def test_resume_takes_the_runs_options(tmp_path):
    run, conf = first_run_config(tmp_path)
    args = nn_train.parse_args(["--resume", run + os.sep, "--epochs", "7", "--time_limit", "60", "--min_lr", "1e-6", "--log_interval", "0"])
    assert args.resume == run and args.save_state is True
    assert (args.epochs, args.time_limit, args.min_lr, args.log_interval) == (7, 60, 1e-6, 0)
    for key in ("start_epoch", "min_quality", "min_quality_epochs", "g_clip_norm", "batch_size", "seed", "loss_cs", "cs", "test_reserve"):
        assert getattr(args, key) == conf[key], key
    assert args.start_epoch == 4                          # --min_quality_epochs counts from the first run's start
    nn_train.check_supported(args)
    # nothing given: the run's own values, epochs too
    args = nn_train.parse_args(["--resume", run])
    assert args.epochs == 3 and args.time_limit is None


def test_resume_does_not_expand_test_reserve_again(tmp_path):
    """a reserved set that happens to be named like a yaml file stays a name (get_test_reserve_list would open it)"""
    run, conf = first_run_config(tmp_path)
    conf["test_reserve"] = ["sets.yaml"]
    with open(os.path.join(run, "config.yaml"), "w") as f:
        yaml.dump(conf, f)
    assert nn_train.parse_args(["--resume", run]).test_reserve == ["sets.yaml"]
    # an option the config of an older run does not know keeps its default
    del conf["g_clip_norm"], conf["skip_nonfinite_steps"]
    with open(os.path.join(run, "config.yaml"), "w") as f:
        yaml.dump(conf, f)
    args = nn_train.parse_args(["--resume", run])
    assert args.g_clip_norm is None and args.skip_nonfinite_steps is False


@pytest.mark.parametrize("argv,name", [(["--batch_size", "8"], "batch_size"), (["--g_lr", "1e-3"], "g_lr"), (["--seed", "1"], "seed"),
                                       (["--gpus", "2"], "gpus"), (["--g_clip_norm", "1"], "g_clip_norm"),
                                       (["--skip_nonfinite_steps"], "skip_nonfinite_steps"), (["--expname", "x"], "expname"),
                                       (["--test_reserve", "0"], "test_reserve"), (["--start_epoch", "3"], "start_epoch"),
                                       (["--config", "c.yaml"], "config")])
def test_resume_refuses_any_other_option(tmp_path, argv, name):
    run, _ = first_run_config(tmp_path)
    with pytest.raises(ValueError, match=f"--{name} cannot be given with --resume"):
        nn_train.parse_args(["--resume", run, "--epochs", "9"] + argv)


def test_resume_needs_a_run_directory(tmp_path):
    with pytest.raises(ValueError, match="config.yaml not found"):
        nn_train.parse_args(["--resume", str(tmp_path)])


# ------------------------------------------------------------------ the learning-rate rule across the boundary
class Rate:
    def __init__(self, lr):
        self.lr = lr

    def update_learning_rate(self, factor):
        self.lr *= factor
        return self.lr


def rule_run(losses, history, trainer, gen_lr):
    out = []
    for loss in losses:
        if nn_train.update_lr_on_plateau(history, loss, trainer, 0.5) is not None:
            gen_lr = trainer.lr
        out.append(gen_lr)
    return out, gen_lr


def test_plateau_rule_across_save_and_restore(tmp_path):
    """patience 2.  Losses fall for three epochs, then 0.45 is above both 0.4 and 0.3: epoch 4 decays.  A run saved after epoch 3
    decays at its first resumed epoch, which it can only know from the saved history.  Epoch 7 decays again, against (0.3, 0.31)."""
    losses = [0.5, 0.4, 0.3, 0.45, 0.3, 0.31, 0.32]
    straight, _ = rule_run(losses, collections.deque(maxlen=2), Rate(1e-3), 1e-3)
    assert straight == [1e-3, 1e-3, 1e-3, 5e-4, 5e-4, 5e-4, 2.5e-4]
    hist, trainer = collections.deque(maxlen=2), Rate(1e-3)
    first, gen_lr = rule_run(losses[:3], hist, trainer, 1e-3)
    state = make_state(3, loss_hist=list(hist), gen_lr=gen_lr)
    state["trainer"]["lr"] = trainer.lr
    nn_train.save_train_state(str(tmp_path), state)
    back = nn_train.load_train_state(str(tmp_path))
    assert back["loss_hist"] == [0.4, 0.3]
    hist2, trainer2 = collections.deque(back["loss_hist"], maxlen=2), Rate(back["trainer"]["lr"])
    rest, _ = rule_run(losses[3:], hist2, trainer2, back["gen_lr"])
    assert first + rest == straight and rest[0] == 5e-4
    # a resumed run that forgot the history would not
    forgot, _ = rule_run(losses[3:], collections.deque(maxlen=2), Rate(1e-3), 1e-3)
    assert forgot[0] == 1e-3


# ------------------------------------------------------------------ a launched run is resumed by the launcher
def launched_run(tmp_path, world):
    """the directory `nn_train --gpus N` leaves: launch() takes --gpus off every rank's command line, so rank 0 records gpus: null"""
    argv = ["--test_reserve", "0", "--epochs", "3", "--batch_size", "4", "--gpus", str(world), "--save_state"]
    rank_argv = nn_train.strip_option(argv, "--gpus")
    assert "--gpus" not in rank_argv
    run, conf = first_run_config(tmp_path, **{k: v for k, v in vars(nn_train.parse_args(rank_argv)).items() if k != "resume"})
    assert conf["gpus"] is None
    nn_train.save_train_state(run, make_state(world=world))
    return run


@pytest.mark.parametrize("world", [2, 8])
def test_resume_of_a_launched_run_starts_its_ranks_again(tmp_path, monkeypatch, world):
    run = launched_run(tmp_path, world)
    assert nn_train.state_world(run) == world
    calls = []
    monkeypatch.setattr(nn_train, "launch", lambda argv, gpus, command=None: calls.append((list(argv), gpus)) or 0)
    monkeypatch.setattr(nn_train, "run", lambda *a, **k: pytest.fail("the launcher must not train"))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = ["--resume", run, "--epochs", "9"]
    assert nn_train.main(argv) == 0
    assert calls == [(argv, world)]
    # what a rank then parses: the run's options, no --gpus of its own, so any world the launcher made passes main()'s check
    args = nn_train.parse_args(nn_train.strip_option(argv, "--gpus"))
    assert args.gpus is None and args.resume == run and args.epochs == 9


def test_resume_of_a_single_process_run_trains_in_this_process(tmp_path, monkeypatch):
    run = launched_run(tmp_path, 1)
    ran = []
    monkeypatch.setattr(nn_train, "launch", lambda *a, **k: pytest.fail("one rank needs no launcher"))
    monkeypatch.setattr(nn_train, "run", lambda args, process_group=None, argv=None: ran.append((args.resume, args.gpus, process_group)))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert nn_train.main(["--resume", run]) == 0
    assert ran == [(run, 1, None)]
    # and a directory without a state file is refused before anything starts
    os.remove(os.path.join(run, nn_train.STATE_FNAME))
    with pytest.raises(ValueError, match="no train_state.pt"):
        nn_train.main(["--resume", run])
    assert len(ran) == 1


def test_a_rank_does_not_ask_the_state_file_for_its_world(tmp_path, monkeypatch):
    """inside a rank (torchrun, or launch()) the environment says the world; check_resumable compares it with the state's"""
    run = launched_run(tmp_path, 2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setattr(nn_train, "state_world", lambda d: pytest.fail("a rank reads its world from the environment"))
    seen = []
    monkeypatch.setattr(nn_train, "init_rank", lambda rank, local, world, backend=None: seen.append((rank, world)) or "group")
    monkeypatch.setattr(nn_train, "run", lambda args, process_group=None, argv=None: seen.append(process_group))
    import torch.distributed as tdist
    monkeypatch.setattr(tdist, "destroy_process_group", lambda: None)
    assert nn_train.main(["--resume", run]) == 0
    assert seen == [(1, 2), "group"]


# ------------------------------------------------------------------ figures that are no scores
def test_guard_figures_stay_out_of_the_best_epochs(tmp_path):
    saver = json_saver.JSONSaver(str(tmp_path / "res.json"), step_type="epoch")
    for e, (loss, norm) in enumerate([(0.5, 0.1), (0.4, 0.9), (0.3, 0.5)], 1):
        nn_train.record_figures(saver, e, {"grad_norm_mean": norm, "clipped_steps": e, "skipped_steps": 3 - e})
        saver.add_res(e, {"train_weighted_loss": loss}, write=False)
        saver.add_res(e, {"gen_lr": 1e-3}, write=True)
    assert saver.get_best_steps() == {3, 1}                  # the best loss, the first rate: no epoch kept for its gradient norm
    again = json_saver.JSONSaver(str(tmp_path / "res.json"), step_type="epoch")
    assert set(again.results["best_epoch"]) == set(again.results["best_val"]) == {"train_weighted_loss", "gen_lr"}
    assert again.results[2] == {"grad_norm_mean": 0.9, "clipped_steps": 2, "skipped_steps": 1, "train_weighted_loss": 0.4, "gen_lr": 1e-3}
    nn_train.record_figures(nn_train._NoResults(), 1, {"skipped_steps": 1})      # a rank other than 0 records nothing
