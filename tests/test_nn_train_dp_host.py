"""CPU tests of data-parallel nn_train (nind_denoise_amd/nn_train.py --gpus N, validation.py's sharded pass): the launcher with
stub children, the option, the validation slices, and, on three gloo ranks over CPU tensors, the gather in index order, the
epoch mean over all ranks' steps, rank 0's decisions, and an averager built before its group.  test_nn_train_dp.py runs the
ranks on the GPU."""
import json
import os
import re
import socket
import sys
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nind_denoise_amd import nn_train, validation


# ------------------------------------------------------------------ 1. the launcher, with stub children
STUB = ("import json, os, sys; "
        "print(json.dumps({'argv': sys.argv[1:], 'env': {k: os.environ.get(k) for k in "
        "('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'OMP_NUM_THREADS')}}), flush=True)")


def test_launcher_gives_every_child_its_rank_and_one_port(capfd, monkeypatch):
    monkeypatch.setenv("OMP_NUM_THREADS", "5")
    argv = ["--batch_size", "4", "--gpus", "3", "--test_reserve", "0", "--gpus=3", "--expname", "x"]
    assert nn_train.launch(argv, 3, command=[sys.executable, "-c", STUB]) == 0
    seen = sorted((json.loads(line) for line in capfd.readouterr().out.splitlines() if line.startswith("{")),
                  key=lambda d: int(d["env"]["RANK"]))
    assert [d["env"]["RANK"] for d in seen] == ["0", "1", "2"]
    ports = set()
    for r, d in enumerate(seen):
        assert d["env"]["LOCAL_RANK"] == str(r) and d["env"]["WORLD_SIZE"] == "3" and d["env"]["MASTER_ADDR"] == "127.0.0.1"
        assert d["env"]["OMP_NUM_THREADS"] == "5"                  # left as it was
        assert d["argv"] == ["--batch_size", "4", "--test_reserve", "0", "--expname", "x"]     # --gpus N is gone, in both spellings
        ports.add(d["env"]["MASTER_PORT"])
    assert len(ports) == 1 and 0 < int(ports.pop()) < 65536
    assert not torch.cuda.is_initialized()                         # the parent never touched a GPU


def test_launcher_returns_the_failed_childs_status_and_ends_its_peers(tmp_path):
    # rank 1 exits 3 at once; rank 0 writes its pid and sleeps 60 s
    code = ("import os, sys, time\n"
            "if os.environ['RANK'] == '1':\n"
            "    sys.exit(3)\n"
            f"open(os.path.join({str(tmp_path)!r}, 'pid'), 'w').write(str(os.getpid()))\n"
            "time.sleep(60)\n")
    t0 = time.monotonic()
    status = nn_train.launch([], 2, command=[sys.executable, "-c", code])
    elapsed = time.monotonic() - t0
    assert status == 3
    assert elapsed < nn_train.KILL_GRACE_S + 5, elapsed             # (SIGTERM ends a sleeping python at once: about 0.1 s)
    pid_file = tmp_path / "pid"
    if pid_file.exists():                                          # (rank 0 may have been ended before it wrote it)
        with pytest.raises(ProcessLookupError):                    # launch() waited for it: the pid is gone, not a zombie
            os.kill(int(pid_file.read_text()), 0)
    assert not torch.cuda.is_initialized()


def test_launcher_ends_a_child_that_ignores_sigterm(tmp_path, monkeypatch):
    monkeypatch.setattr(nn_train, "KILL_GRACE_S", 1)               # the same path as the 10 s of a real run
    code = ("import os, signal, sys, time\n"
            "signal.signal(signal.SIGTERM, signal.SIG_IGN)\n"
            f"open(os.path.join({str(tmp_path)!r}, 'ready' + os.environ['RANK']), 'w').close()\n"
            "if os.environ['RANK'] == '0':\n"
            f"    while not os.path.exists(os.path.join({str(tmp_path)!r}, 'ready1')):\n"
            "        time.sleep(0.01)\n"
            "    sys.exit(7)\n"
            "time.sleep(60)\n")
    t0 = time.monotonic()
    assert nn_train.launch([], 2, command=[sys.executable, "-c", code]) == 7
    assert 0.9 < time.monotonic() - t0 < 6


def test_a_launcher_that_is_terminated_ends_its_children(tmp_path):
    import signal
    import subprocess
    child = ("import os, time\n"
             f"open(os.path.join({str(tmp_path)!r}, 'pid' + os.environ['RANK']), 'w').write(str(os.getpid()))\n"
             "time.sleep(60)\n")
    parent = ("import sys\n"
              "from nind_denoise_amd import nn_train\n"
              f"sys.exit(nn_train.launch([], 2, command=[sys.executable, '-c', {child!r}]))\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proc = subprocess.Popen([sys.executable, "-c", parent], cwd=root)
    try:
        deadline = time.monotonic() + 60
        while not all((tmp_path / f"pid{r}").exists() and (tmp_path / f"pid{r}").read_text() for r in range(2)):
            assert time.monotonic() < deadline and proc.poll() is None
            time.sleep(0.05)
        proc.send_signal(signal.SIGTERM)
        assert proc.wait(timeout=nn_train.KILL_GRACE_S + 10) == 128 + signal.SIGTERM
    finally:
        if proc.poll() is None:          # the test has failed: leave nothing running
            proc.kill()
            for r in range(2):
                try:
                    os.kill(int((tmp_path / f"pid{r}").read_text()), signal.SIGKILL)
                except (OSError, ValueError):
                    pass
    for r in range(2):
        with pytest.raises(ProcessLookupError):
            os.kill(int((tmp_path / f"pid{r}").read_text()), 0)


# ------------------------------------------------------------------ 2. the option
@pytest.mark.parametrize("n", ["0", "-1", "17"])
def test_gpus_out_of_range_is_refused_by_name(tmp_path, monkeypatch, n):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match=re.escape("--gpus")):       # the launcher itself, before it starts anything
        nn_train.launch([], int(n), command=[sys.executable, "-c", "import sys; sys.exit(9)"])
    monkeypatch.setattr(nn_train, "launch", lambda *a, **k: pytest.fail("launched"))
    monkeypatch.setattr(nn_train, "run", lambda *a, **k: pytest.fail("ran"))
    with pytest.raises(ValueError, match=re.escape("--gpus")):
        nn_train.main(["--test_reserve", "0", "--gpus", n])


def test_gpus_1_and_no_option_run_in_this_process(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    calls = []
    monkeypatch.setattr(nn_train, "launch", lambda *a, **k: pytest.fail("--gpus 1 took the launcher branch"))
    monkeypatch.setattr(nn_train, "run", lambda args, process_group=None, argv=None: calls.append((args.gpus, process_group, argv)))
    assert nn_train.main(["--test_reserve", "0", "--gpus", "1"]) == 0
    assert nn_train.main(["--test_reserve", "0"]) == 0
    assert calls == [(1, None, ["nn_train.py", "--test_reserve", "0", "--gpus", "1"]), (None, None, ["nn_train.py", "--test_reserve", "0"])]
    # more than one: the launcher, with the command line as it came, and its status is main's
    launched = []
    monkeypatch.setattr(nn_train, "launch", lambda argv, gpus, command=None: launched.append((argv, gpus)) or 5)
    assert nn_train.main(["--test_reserve", "0", "--gpus", "2"]) == 5
    assert launched == [(["--test_reserve", "0", "--gpus", "2"], 2)] and len(calls) == 2
    # what every rank would refuse is refused before any rank starts
    with pytest.raises(NotImplementedError, match="g_network"):
        nn_train.main(["--test_reserve", "0", "--gpus", "2", "--g_network", "UNet"])
    assert len(launched) == 1


def test_a_rank_does_not_start_ranks(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setattr(nn_train, "launch", lambda *a, **k: pytest.fail("a rank launched ranks"))
    monkeypatch.setattr(nn_train, "init_rank", lambda *a, **k: pytest.fail("joined a group"))
    with pytest.raises(ValueError, match=re.escape("--gpus 3")):
        nn_train.main(["--test_reserve", "0", "--gpus", "3"])
    assert nn_train.world_from_environment() == (1, 1, 2)
    monkeypatch.setenv("LOCAL_RANK", "0")
    assert nn_train.world_from_environment() == (1, 0, 2)
    monkeypatch.setenv("WORLD_SIZE", "1")
    assert nn_train.world_from_environment() is None


def test_help_names_the_options(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    text = nn_train.build_parser().format_help()
    assert "--gpus" in text and "--dist_backend" in text
    args = nn_train.parse_args(["--test_reserve", "0"])
    assert args.gpus is None and args.dist_backend is None
    assert nn_train.parse_args(["--test_reserve", "0", "--dist_backend", "gloo"]).dist_backend == "gloo"
    with pytest.raises(SystemExit):
        nn_train.parse_args(["--test_reserve", "0", "--dist_backend", "mpi"])


def test_strip_option():
    assert nn_train.strip_option(["--gpus", "2", "a", "--gpus=3", "--gpus_like", "b", "--gpus"], "--gpus") == ["a", "--gpus_like", "b"]


# ------------------------------------------------------------------ 3. the validation slices
@pytest.mark.parametrize("n", [1, 2, 5, 300])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_indices_cover_the_set_once_in_rank_order(n, world):
    slices = [validation.shard_indices(n, r, world) for r in range(world)]
    assert all(isinstance(s, range) and s.step == 1 for s in slices)           # contiguous
    assert slices[0].start == 0 and slices[-1].stop == n
    assert all(a.stop == b.start for a, b in zip(slices, slices[1:]))          # disjoint, in rank order, no gap
    assert [i for s in slices for i in s] == list(range(n))
    assert max(map(len, slices)) - min(map(len, slices)) <= 1
    assert any(len(s) == 0 for s in slices) == (n < world)
    with pytest.raises(ValueError):
        validation.shard_indices(n, world, world)


# ------------------------------------------------------------------ 4 and 5. three gloo ranks on CPU tensors
WORLD = 3


def planted_vector():
    """5 float32 values with the bits a copy must keep: two NaNs with payloads, -0.0, a denormal"""
    bits = np.array([0x7FC12345, 0x80000000, 0x3F800001, 0xFFA00F0F, 0x00000001], dtype=np.uint32)
    return torch.from_numpy(bits.view(np.int32).copy()).view(torch.float32)


def step_losses(rank):
    """what rank `rank` kept of its steps: float32 losses of one magnitude, a different count per rank"""
    g = torch.Generator().manual_seed(100 + rank)
    return 0.01 + torch.rand(4 + rank, 2, generator=g, dtype=torch.float32)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, outq):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from nind_denoise_amd import _lib
    from nind_denoise_amd import dist as ndist
    # an averager built before its group exists (a trainer built too early): it must average once the group is there
    n_params = _lib.load().nd_utnet_param_count(8)
    early = torch.full((n_params,), float(rank + 1))
    averager = ndist.BucketedGradientAverager(8, early)
    assert not averager.active
    averager.reduce()
    assert torch.equal(early, torch.full((n_params,), float(rank + 1)))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        group = dist.group.WORLD
        out = {}
        assert averager.active
        averager.reduce()
        out["early_averager"] = early.unique().tolist()
        # 4. this rank's slice of the planted vector, gathered
        full = planted_vector()
        mine = validation.shard_indices(full.numel(), rank, world)
        out["slice"] = (mine.start, mine.stop)
        out["gathered"] = validation.gather_in_order(full[mine.start:mine.stop].clone(), full.numel(), group).view(torch.int32).tolist()
        try:
            validation.gather_in_order(full[:0] if len(mine) else full[:1], full.numel(), group)
            out["wrong_length"] = "accepted"
        except ValueError:
            out["wrong_length"] = "refused"
        # 5. the epoch means, and rank 0's decision
        kept = step_losses(rank)
        means, count = nn_train.combine_epoch_sums(kept.double().sum(0).tolist(), kept.shape[0], group)
        out["means"], out["count"] = np.array(means, dtype=np.float64).view(np.int64).tolist(), count
        out["time_is_up"] = nn_train.from_rank0(rank != 0, group)          # rank 0 says False, the others True
        out["expname"] = nn_train.from_rank0(f"name-of-rank-{rank}", group)
        # the agreement check: equal buffers pass; one that differs on rank 2 raises on every rank, naming it and the epoch
        nn_train.check_agreement(torch.arange(100, dtype=torch.float32), group, 1)
        flat = torch.arange(100, dtype=torch.float32)
        flat[-1] = -flat[-1] if rank == 2 else flat[-1]                    # (the sum of magnitudes alone would miss a sign)
        try:
            nn_train.check_agreement(flat, group, 4)
            out["agreement"] = "passed"
        except RuntimeError as e:
            out["agreement"] = str(e)
        outq.put((rank, out))
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, WORLD, port, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=120) for _ in range(WORLD))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return got


def test_gather_in_index_order_keeps_every_bit(ranks):
    want = planted_vector().view(torch.int32).tolist()
    assert [ranks[r]["slice"] for r in range(WORLD)] == [(0, 1), (1, 3), (3, 5)]          # ragged: 1, 2 and 2 of 5
    for r in range(WORLD):
        assert ranks[r]["gathered"] == want, r
        assert ranks[r]["wrong_length"] == "refused"


def test_epoch_mean_is_over_all_ranks_steps_and_the_same_bits_everywhere(ranks):
    # sum(all steps) / count in double, the steps in rank order.  (Doubles add these float32 values exactly -- 24-bit mantissas
    # within a few binades of each other -- so the grouping by rank cannot show.)
    total, count = np.zeros(2, dtype=np.float64), 0
    for r in range(WORLD):
        for step in step_losses(r).double().numpy():
            total += step
            count += 1
    want = (total / count).view(np.int64).tolist()
    assert count == 4 + 5 + 6
    for r in range(WORLD):
        assert ranks[r]["count"] == count and ranks[r]["means"] == want, r


def test_rank_0_decides_for_everyone(ranks):
    for r in range(WORLD):
        assert ranks[r]["time_is_up"] is False and ranks[r]["expname"] == "name-of-rank-0", r


def test_agreement_check_names_the_rank_and_the_epoch_on_every_rank(ranks):
    for r in range(WORLD):
        msg = ranks[r]["agreement"]
        assert "rank(s) [2]" in msg and "epoch 4" in msg, (r, msg)


def test_an_averager_built_before_the_group_averages_once_it_exists(ranks):
    for r in range(WORLD):
        assert ranks[r]["early_averager"] == [2.0], r              # the mean of 1, 2 and 3: not this rank's own value
