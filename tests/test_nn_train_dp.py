"""GPU tests of data-parallel nn_train: two ranks over gloo on the one GPU (the rehearsal: ranks share the card and gradients are
staged through the host; RCCL refuses two ranks on one device).

Ranks are started twice for the whole module: once through the command itself (`python -m nind_denoise_amd.nn_train --gpus 2`,
a parent that never touches the GPU and two fresh children, all defaults), and once as the test's own rank function, which sets
UtNet.split_k = False and then does, in one process group, everything that needs it: the sharded validation pass, a whole run, one
data-parallel step, and a run in which rank 1 is made to diverge.  Every test reads what those two left.  The single-process
sides run in this process.

Everything runs at funit 8 with --weight_MSE 1 on 104 x 104 crops, the smallest the network takes (networks/UtNet.py: valid_cs;
UtNetTrainer refuses 72), from 112 x 112 8-bit files: 8 groups at 2 crops per rank and step (2 steps per rank and epoch), 5
validation pairs at --val_batch_size 2 (slices of 2 and 3, batches of 2 + 1 within the second), --epochs 2 (one validation before
training, one training epoch: trainres.json holds epochs 0 and 1, the last checkpoint is generator_1.pt)."""
import hashlib
import json
import os
import re
import signal
import socket
import subprocess
import sys
from datetime import timedelta

import numpy as np
import pytest
import torch
import torch.nn.functional as F
import yaml

from nind_denoise_amd import _lib, synth
from nind_denoise_amd.common.libs import imgcodec

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNIT, SIDE, CS, LOSS_CS, BATCH, GROUPS, PAIRS = 8, 112, 104, 96, 2, 8, 5
START_TIMEOUT_S = 300      # each of the two starts of ranks: about 30 s of process start-up and HIP initialisation, no retry

# generator_1.pt of the single-process run below (train_argv: 4 steps of 2 crops), as the parent revision writes it: recorded
# with that revision's nn_train.py, validation.py, dist.py and train.py in place, on an MI355X, by
#   python -c "import sys; sys.path.insert(0, 'tests'); import test_nn_train_dp as t; print(t.parent_digest('/tmp/dp'))"
# That revision wrote 8a25e7c337928a0f44b303aadcf2800523b1c6da3687104d1634c8003f0aedec.  Recorded again, by the same command, when
# nd_adam_step took its bias corrections in double (csrc/optim.hip; tests/test_adam_exact.py): from step 2 on every update moves
# by a few 1e-6 of itself, so no file trained for more than one step keeps its bits across that change.  The claim of the test
# below is unchanged -- the options off, or --gpus 1, write the file a run without them writes, bit for bit
PARENT_DIGEST = "774c831ca6fa2b48d8c15f3d0fc4a5b50a1bbd7e12b414046590df7adaaff3d2"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ data
def image_like(n, h, w, seed):
    """bilinear-upsampled noise plus fine noise, in [0, 1]"""
    g = torch.Generator().manual_seed(seed)
    c = F.interpolate(torch.rand(n, 3, h // 8, w // 8, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * c + 0.1 + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)


def pairs_u8(n, seed):
    """n (clean, noisy) pairs of SIDE x SIDE 8-bit images, [n,3,SIDE,SIDE] uint8 each: noisy = clean + fixed noise"""
    clean = image_like(n, SIDE, SIDE, seed)
    g = torch.Generator().manual_seed(seed + 1)
    noisy = (clean + 0.04 * torch.randn(clean.shape, generator=g)).clip(0, 1)
    return (clean * 255).round().to(torch.uint8), (noisy * 255).round().to(torch.uint8)


def write_png(path, chw):
    imgcodec.write_png(path, chw.permute(1, 2, 0).contiguous().numpy())


def make_tree(root):
    """<root>/SYN_112_96/<set>/ISO*/: 8 groups (two sets of four crops, a clean ISO and a noisy one), and a yaml of 5 pairs"""
    data = os.path.join(root, f"SYN_{SIDE}_{LOSS_CS}")
    clean, noisy = pairs_u8(GROUPS, seed=41)
    for k in range(GROUPS):
        aset, crop = f"set{k // 4}", f"{k % 4}_0"
        for iso, img in (("ISO100", clean[k]), ("ISO6400", noisy[k])):
            os.makedirs(os.path.join(data, aset, iso), exist_ok=True)
            write_png(os.path.join(data, aset, iso, f"SYN_{aset}_{iso}_{crop}_{LOSS_CS}.png"), img)
    vclean, vnoisy = pairs_u8(PAIRS, seed=51)
    pairs = []
    os.makedirs(os.path.join(root, "val"), exist_ok=True)
    for i in range(PAIRS):
        paths = [os.path.join(root, "val", f"{kind}_{i}.png") for kind in ("clean", "noisy")]
        write_png(paths[0], vclean[i])
        write_png(paths[1], vnoisy[i])
        pairs.append(paths)
    val_yaml = os.path.join(root, "val.yaml")
    with open(val_yaml, "w") as f:
        yaml.dump(pairs, f)
    return data, val_yaml


def train_argv(data, val_yaml, models, extra=()):
    """(--loss_cs is left to the directory's name: 96)"""
    return ["--g_funit", str(FUNIT), "--cs", str(CS), "--batch_size", str(BATCH), "--weight_MSE", "1", "--g_lr", "1e-3",
            "--epochs", "2", "--patience", "2", "--seed", "7", "--beta1", "0.75", "--reduce_lr_factor", "0.5", "--train_data", data,
            "--test_reserve", "0", "--validation_set_yaml", val_yaml, "--val_batch_size", "2", "--models_dpath", models] + list(extra)


def file_digest(path):
    from nind_denoise_amd import nn_train
    return nn_train.parameters_digest(torch.load(path, map_location="cpu", weights_only=True))


def parent_digest(root):
    """what PARENT_DIGEST records (the state dict's tensors in order, as bytes: nn_train.parameters_digest, which the parent
    revision does not have)"""
    from nind_denoise_amd import nn_train
    os.makedirs(root, exist_ok=True)
    data, val_yaml = make_tree(root)
    models = os.path.join(root, "models")
    assert nn_train.main(train_argv(data, val_yaml, models, ["--expname", "parent"])) == 0
    h = hashlib.sha256()
    for v in torch.load(os.path.join(models, "parent", "generator_1.pt"), map_location="cpu", weights_only=True).values():
        h.update(v.contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("dp"))
    data, val_yaml = make_tree(root)
    return {"root": root, "data": data, "val_yaml": val_yaml}


def step_pool(device):
    """4 groups for the one-step test: batch 2, so one step per rank at world 2 and two batches in one process"""
    from nind_denoise_amd.crop_pool import CropPool
    pool = CropPool(device, seed=5, cs=CS)
    clean, noisy = pairs_u8(4, seed=61)
    for k in range(4):
        pool.add_group([clean[k].numpy()], [noisy[k].numpy()])
    return pool


def fresh_trainer(device, group=None):
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    net = UtNet(funit=FUNIT)
    net.load_state_dict(synth.make_utnet_state_dict(funit=FUNIT, seed=31, gain=1.8))
    return UtNetTrainer(net, lr=1e-3, beta1=0.75, weights={"MSE": 1.0}, device=device, process_group=group, loss_cs=LOSS_CS)


def validation_model(device):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=FUNIT)
    net.load_state_dict(synth.make_utnet_state_dict(funit=FUNIT, seed=33, gain=1.8))
    return net.to(device).train()


# ------------------------------------------------------------------ start 1: the command, --gpus 2, all defaults
@pytest.fixture(scope="module")
def launched(dev, tree):
    models = os.path.join(tree["root"], "models_launched")
    cmd = [sys.executable, "-m", "nind_denoise_amd.nn_train", "--gpus", "2"] + train_argv(tree["data"], tree["val_yaml"], models)
    # a session of its own, so that a run that does not end can be ended with its ranks
    proc = subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, start_new_session=True)
    try:
        out, _ = proc.communicate(timeout=START_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        out, _ = proc.communicate()
        pytest.fail(f"nn_train --gpus 2 did not end within {START_TIMEOUT_S} s:\n{out[-4000:]}")
    print(out[-6000:])
    assert proc.returncode == 0, out[-4000:]
    return {"models": models, "out": out}


# ------------------------------------------------------------------ start 2: the test's own ranks, split_k = False
def _rank_main(rank, world, port, tree, outq):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as tdist
    from nind_denoise_amd import nn_train
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.validation import ValidationSet, validate
    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    tdist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=120))
    try:
        group = tdist.group.WORLD
        UtNet.split_k = False          # every tile whole: a sample's bits do not depend on its batch
        out = {}
        # the sharded pass alone, on a model with weights that make every level count
        vs = ValidationSet(tree["val_yaml"], device, CS)
        avg, per = validate(validation_model(device), vs, {"MSE": 1.0}, LOSS_CS, batch_size=2, group=group,
                            output_to_dir=os.path.join(tree["root"], "val_images_sharded"))
        out["validate"] = (avg, per.cpu().numpy())
        # a whole run
        models = os.path.join(tree["root"], "models_ranks")
        args = nn_train.parse_args(train_argv(tree["data"], tree["val_yaml"], models, ["--expname", "nosplit"]))
        nn_train.run(args, group, argv=["nn_train.py"])
        # one data-parallel step, on the kernels a run takes by default (split_k is one of the flags the training step reads, and
        # the single-process side of the comparison runs with the default): batch k of the epoch goes to rank k
        UtNet.split_k = True
        pool, tr = step_pool(device), fresh_trainer(device, group)
        steps = 0
        for draws in pool.epoch(BATCH, rank=rank, world=world):
            clean, noisy = pool.batch(draws)
            tr.learn(noisy, clean)
            steps += 1
        out["step"] = (steps, tr.flat.cpu().numpy())
        # a run in which rank 1 changes one parameter after the epoch's steps
        train_epoch = nn_train.train_epoch

        def train_epoch_then_diverge(pool, trainer, *a, **k):
            n = train_epoch(pool, trainer, *a, **k)
            if rank == 1:
                trainer.flat[1234] += 0.5
            return n
        nn_train.train_epoch = train_epoch_then_diverge
        args = nn_train.parse_args(train_argv(tree["data"], tree["val_yaml"], models, ["--expname", "diverged"]))
        try:
            nn_train.run(args, group, argv=["nn_train.py"])
            out["diverged"] = "no error"
        except RuntimeError as e:
            out["diverged"] = str(e)
        finally:
            nn_train.train_epoch = train_epoch
        outq.put((rank, out))
    finally:
        tdist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks(dev, tree):
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, tree, q)) for r in range(2)]
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
    return got


# ------------------------------------------------------------------ the single-process sides, in this process
@pytest.fixture(scope="module")
def single(dev, tree):
    """the same arguments in one process: without the option, with --gpus 1, and once more with split_k = False"""
    from nind_denoise_amd import nn_train
    from nind_denoise_amd.networks.UtNet import UtNet
    models = os.path.join(tree["root"], "models_single")
    assert nn_train.main(train_argv(tree["data"], tree["val_yaml"], models, ["--expname", "plain"])) == 0
    assert nn_train.main(train_argv(tree["data"], tree["val_yaml"], models, ["--expname", "gpus1", "--gpus", "1"])) == 0
    split_k = UtNet.split_k
    UtNet.split_k = False
    try:
        args = nn_train.parse_args(train_argv(tree["data"], tree["val_yaml"], models, ["--expname", "nosplit"]))
        nn_train.run(args, argv=["nn_train.py"])
    finally:
        UtNet.split_k = split_k
    return models


def results(run_dir):
    with open(os.path.join(run_dir, "trainres.json")) as f:
        return json.load(f)


# ------------------------------------------------------------------ 6. one run, written once
def test_one_run_directory_written_by_rank_0_alone(launched):
    runs = os.listdir(launched["models"])
    assert len(runs) == 1, runs                                    # no --expname: rank 0's name, on both ranks
    run = os.path.join(launched["models"], runs[0])
    assert sorted(os.listdir(run)) == ["config.yaml", "generator_1.pt", "train.log", "trainres.json"]
    with open(os.path.join(run, "train.log")) as f:
        log = f.read()
    for line in ("Epoch 1 summary:", "Average weighted loss:", "delete_outperformed_models removed", "cmd: python3"):
        assert log.count(line) == 1, line
    assert log.count("Validation loss:") == 2 and "[rank" not in log
    assert "Data parallel: 2 ranks, 2 crops per rank and step" in log and "2 steps per epoch" in log
    res = results(run)
    assert set(res) == {"0", "1", "best_epoch", "best_val"}
    assert set(res["0"]) == {"validation_loss"}
    assert set(res["1"]) == {"validation_loss", "train_weighted_loss", "gen_lr"} and res["1"]["gen_lr"] == 1e-3
    sd = torch.load(os.path.join(run, "generator_1.pt"), map_location="cpu", weights_only=True)
    assert all(torch.isfinite(v).all() for v in sd.values())
    with open(os.path.join(run, "config.yaml")) as f:
        conf = yaml.safe_load(f)
    assert conf["loss_cs"] == LOSS_CS and conf["gpus"] is None and conf["batch_size"] == BATCH
    # rank 1 said what it did on stdout, under its rank, and every line of rank 0's log is on stdout too
    assert "[rank 1] Epoch 1 summary:" in launched["out"] and "[rank 0]" not in launched["out"]
    # it trained: the validation loss moved (the figures: printed)
    print(f"validation loss: epoch 0 {res['0']['validation_loss']:.6f}, epoch 1 {res['1']['validation_loss']:.6f}; "
          f"train {res['1']['train_weighted_loss']:.6f}")
    assert res["1"]["validation_loss"] != res["0"]["validation_loss"]


# ------------------------------------------------------------------ 7. the ranks end with the same parameters, the saved ones
def test_ranks_end_with_the_parameters_of_the_checkpoint(launched):
    digests = dict(re.findall(r"rank (\d) of 2: parameters sha256 ([0-9a-f]{64})", launched["out"]))
    assert set(digests) == {"0", "1"}, launched["out"][-2000:]
    run = os.path.join(launched["models"], os.listdir(launched["models"])[0])
    assert digests["0"] == digests["1"] == file_digest(os.path.join(run, "generator_1.pt"))


# ------------------------------------------------------------------ 8. sharded validation is the validation
def test_sharded_validation_equals_the_single_process_pass_bit_for_bit(dev, tree, ranks, single, monkeypatch):
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.validation import ValidationSet, validate
    monkeypatch.setattr(UtNet, "split_k", False)
    vs = ValidationSet(tree["val_yaml"], dev, CS)
    out_dir = os.path.join(tree["root"], "val_images_single")
    avg, per = validate(validation_model(dev), vs, {"MSE": 1.0}, LOSS_CS, batch_size=2, output_to_dir=out_dir)
    per = per.cpu().numpy()
    assert per.shape == (PAIRS,) and np.isfinite(per).all() and len(set(per.tolist())) == PAIRS
    for r in range(2):
        got_avg, got_per = ranks[r]["validate"]
        print(f"rank {r}: mean {got_avg!r} (one process: {avg!r}), per sample {got_per.tolist()}")
        assert np.array_equal(got_per.view(np.int32), per.view(np.int32)), r
        assert got_avg == avg, r
    # each rank wrote the images of its own samples, under the sample's index: together, the files of the one process
    sharded_dir = os.path.join(tree["root"], "val_images_sharded")
    assert sorted(os.listdir(sharded_dir)) == sorted(os.listdir(out_dir)) == [f"{i}.tif" for i in range(PAIRS)]
    for name in os.listdir(out_dir):
        assert np.array_equal(imgcodec.read_tiff(os.path.join(sharded_dir, name)), imgcodec.read_tiff(os.path.join(out_dir, name))), name
    # and inside a run: before any step both runs hold the same parameters, so the first validation loss is the same float
    two = results(os.path.join(tree["root"], "models_ranks", "nosplit"))
    one = results(os.path.join(single, "nosplit"))
    assert two["0"]["validation_loss"] == one["0"]["validation_loss"]
    assert set(two["1"]) == {"validation_loss", "train_weighted_loss", "gen_lr"}


# ------------------------------------------------------------------ 9. one data-parallel step is the averaged step
def test_one_data_parallel_step_is_the_step_on_the_averaged_gradient(dev, ranks):
    """World 2: rank k learns batch k of the epoch, the averager takes the mean of the two gradients.  One process: two trainers
    from the same parameters, one gradient each, (g0 + g1) / 2, one nd_adam_step.  A two-term sum has one order and the halving
    is exact, so if the step is deterministic the parameters are the same bits.  The bar is 4 x the largest difference between
    two identical single-process steps, measured here first (two gradients and the step).  On an MI355X that difference is 0,
    so the bar is bit equality, and the world-2 parameters meet it (largest difference 0 on both ranks)."""
    pool = step_pool(dev)
    batches = [pool.batch(draws) for draws in pool.epoch(BATCH)]
    assert len(batches) == 2
    (clean0, noisy0), (clean1, noisy1) = batches
    # determinism first: the same step twice
    twice = []
    for _ in range(2):
        tr = fresh_trainer(dev)
        tr.learn(noisy0, clean0)
        twice.append(tr.flat.clone())
    run_to_run = (twice[0] - twice[1]).abs().max().item()
    bar = 4 * run_to_run
    a, b = fresh_trainer(dev), fresh_trainer(dev)
    start = a.flat.clone()
    a.forward_backward(noisy0, clean0)
    b.forward_backward(noisy1, clean1)
    assert not torch.equal(a.grads, b.grads)
    a.grads.copy_((a.grads + b.grads) / 2)
    a.optimizer_step()
    want = a.flat.cpu().numpy()
    assert np.abs(want - start.cpu().numpy()).max() > 1e-4          # the step moved the parameters (lr 1e-3, Adam's first step)
    for r in range(2):
        steps, got = ranks[r]["step"]
        diff = np.abs(got - want).max()
        print(f"rank {r}: {steps} step, largest difference to the averaged step {diff:.3e}; run to run {run_to_run:.3e}, bar {bar:.3e}")
        assert steps == 1
        assert diff <= bar, r
        # not the step on this rank's own gradient alone
        assert np.abs(got - twice[0].cpu().numpy()).max() > 0
    assert np.array_equal(ranks[0]["step"][1], ranks[1]["step"][1])


# ------------------------------------------------------------------ 10. the agreement check bites
def test_a_rank_that_diverges_is_named_on_every_rank(tree, ranks):
    for r in range(2):
        msg = ranks[r]["diverged"]
        assert "rank(s) [1]" in msg and "epoch 1" in msg and "differ from rank 0" in msg, (r, msg)
    run = os.path.join(tree["root"], "models_ranks", "diverged")
    assert not os.path.exists(os.path.join(run, "generator_1.pt"))  # nothing saved from parameters the ranks do not share


# ------------------------------------------------------------------ 11. one process: as before
def test_gpus_1_and_no_option_train_as_the_parent_revision(single):
    plain, gpus1 = (file_digest(os.path.join(single, name, "generator_1.pt")) for name in ("plain", "gpus1"))
    print(f"generator_1.pt: {plain}")
    assert plain == gpus1
    with open(os.path.join(single, "plain", "trainres.json"), "rb") as f1, open(os.path.join(single, "gpus1", "trainres.json"), "rb") as f2:
        assert f1.read() == f2.read()
    assert sorted(os.listdir(os.path.join(single, "plain"))) == ["config.yaml", "generator_1.pt", "train.log", "trainres.json"]
    with open(os.path.join(single, "plain", "train.log")) as f:
        log = f.read()
    assert "Data parallel" not in log and "sha256" not in log
    assert plain == PARENT_DIGEST
