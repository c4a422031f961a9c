"""CPU tests of the crop pool's quality bar: the pair order and paths of list_content_quality against a restatement of the
reference's get_all_crop_pairs_of_paths, the csv and its way back through set_min_quality, and what draws name once a bar is set.
Draws are torch ops under the pool's generator, so a CPU pool with hand-given scores makes them; scoring itself needs the GPU
(tests/test_pool_quality.py)."""
import csv
import math
import os
import re

import numpy as np
import pytest
import torch

from nind_denoise_amd import nn_common, nn_train
from nind_denoise_amd.common.libs import imgcodec, utilities
from nind_denoise_amd.crop_pool import CropPool

SETS = {"bike": ("ISO200", "ISO200-1", "ISO800", "ISO6400", "ISOH1"), "tree": ("ISO100", "ISO3200"), "stairs": ("GT", "ISO400", "ISO1600")}
CROPS = ("0_0", "16_0")


def write_tree(root, shape=(12, 10)):
    rng = np.random.default_rng(0)
    for aset, isos in SETS.items():
        for iso in isos:
            os.makedirs(os.path.join(root, aset, iso))
            for crop in CROPS:
                imgcodec.write_png(os.path.join(root, aset, iso, f"NIND_{aset}_{iso}_{crop}_16.png"),
                                   rng.integers(0, 255, shape + (3,)).astype(np.uint8))
    return root


def reference_pairs(pool):
    """dataset_torch_3.py:191 and 203-213, restated on the scan the pool kept: el = [path with ISOBASE, base ISOs, other ISOs]."""
    dataset = [[os.path.join(datadir, aset, 'ISOBASE', animg).replace(isos[0] + '_', 'ISOBASE_'), bisos, isos]
               for datadir, aset, animg, bisos, isos in pool.sets]
    for el in dataset:
        for biso in el[1]:
            for noisy_iso in el[2]:
                gt_crop_path = os.path.join(el[0].replace('ISOBASE_', biso + '_').replace('/ISOBASE/', '/' + biso + '/'))
                noisy_crop_path = os.path.join(el[0].replace('ISOBASE_', noisy_iso + '_').replace('/ISOBASE/', '/' + noisy_iso + '/'))
                yield gt_crop_path, noisy_crop_path


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    return write_tree(str(tmp_path_factory.mktemp("quality") / "NIND_24_16"))


def fresh_pool(root, seed=3):
    return CropPool.from_directories([root], device="cpu", seed=seed)


def hand_scores(pool):
    """One score per pair, distinct, in pair order: 0.50, 0.51, ...; but 0.1 for the last group's pairs, and NaN for the last pair
    of the third group from the end (which keeps another pair)."""
    table = pool.pair_table()
    scores = torch.tensor([0.5 + 0.01 * k for k in range(len(table))], dtype=torch.float32)
    scores[torch.from_numpy(table[:, 0] == pool.n_groups - 1)] = 0.1
    scores[int(np.flatnonzero(table[:, 0] == pool.n_groups - 3)[-1])] = float("nan")
    return table, scores


def test_pair_order_and_paths_are_the_reference_s(root):
    pool = fresh_pool(root)
    assert pool.n_groups == 6
    paths = pool.pair_paths()
    assert paths == list(reference_pairs(pool)) and len(paths) == 2 * (2 * 3 + 1 * 1 + 1 * 2)
    assert all(os.path.isfile(p) for pair in paths for p in pair)        # the files the scan read
    table = pool.pair_table()
    assert table.shape == (len(paths), 3) and table.dtype == np.int64
    # groups in pool order, base ISOs outer, other ISOs inner; the images are the pool's own
    want = [(g, c, n) for g in range(pool.n_groups) for c in pool.group(g)[0] for n in pool.group(g)[1]]
    assert [tuple(r) for r in table.tolist()] == want
    first = pool.sets[0]
    isos = [(os.path.basename(os.path.dirname(x)), os.path.basename(os.path.dirname(y))) for x, y in paths[:6]]
    assert first[1] == "bike" and isos == [(b, n) for b in first[3] for n in first[4]] and len(set(isos)) == 6
    assert pool.dsname == "NIND_24_16"
    two = CropPool.from_directories([root, root + os.sep], device="cpu")
    assert two.dsname == "NIND_24_16+NIND_24_16" and len(two.pair_paths()) == 2 * len(paths)
    hand = CropPool("cpu", cs=8)
    hand.add_group([np.zeros((3, 9, 9), np.uint8)], [np.ones((3, 9, 9), np.uint8)])
    with pytest.raises(ValueError, match="from_directories"):
        hand.list_content_quality()
    with pytest.raises(ValueError, match="from_directories"):
        hand.set_min_quality(0.5, scores="nothing.csv")


def test_list_of_tuples_to_csv(tmp_path):
    path = str(tmp_path / "t.csv")
    utilities.list_of_tuples_to_csv([("a", "b,c", 1.5), ("d", "e", "")], ("xpath", "ypath", "score"), path)
    with open(path, newline="") as f:
        assert list(csv.reader(f)) == [["xpath", "ypath", "score"], ["a", "b,c", "1.5"], ["d", "e", ""]]


def test_csv_header_round_trip_and_mismatch(root, tmp_path, capsys):
    pool = fresh_pool(root)
    table, scores = hand_scores(pool)
    pool.scores = scores                                        # as score_pairs leaves them; nothing here can score
    rows = pool.list_content_quality(export=True, out_dir=str(tmp_path / "datasets"))
    path = str(tmp_path / "datasets" / "NIND_24_16-msssim.csv")
    assert f"Quality check exported to {path}" in capsys.readouterr().out
    assert [r[:2] for r in rows] == pool.pair_paths()
    assert all(math.isnan(r[2]) if math.isnan(s) else r[2] == s for r, s in zip(rows, scores.tolist()))
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "xpath,ypath,score" and len(lines) == 1 + len(rows)
    for line, (x, y, s) in zip(lines[1:], rows):
        assert line == f"{x},{y}," + ("" if math.isnan(s) else repr(s))        # repr(float); NaN: an empty field
    assert any(line.endswith(",") for line in lines[1:])

    q = 0.545
    a, b = fresh_pool(root), fresh_pool(root)
    assert a.set_min_quality(q, scores=path) == b.set_min_quality(q, scores=scores) == int((scores > q).sum())
    assert a.n_active_groups == b.n_active_groups < a.n_groups
    for _ in range(5):
        assert torch.equal(a.draw(16).table, b.draw(16).table)

    # one path changed: the file no longer lists this pool's pairs, and the error says which path
    changed = rows[4][1].replace("NIND_bike", "NIND_boat")
    assert changed != rows[4][1]
    bad = str(tmp_path / "bad.csv")
    utilities.list_of_tuples_to_csv([(x, changed if k == 4 else y, repr(s)) for k, (x, y, s) in enumerate(rows)],
                                    ("xpath", "ypath", "score"), bad)
    with pytest.raises(ValueError, match=re.escape(changed)) as e:
        fresh_pool(root).set_min_quality(q, scores=bad)
    assert rows[4][1] in str(e.value)                             # and the pool's own path that the file lacks
    short = str(tmp_path / "short.csv")
    utilities.list_of_tuples_to_csv([(x, y, repr(s)) for x, y, s in rows[:-1]], ("xpath", "ypath", "score"), short)
    with pytest.raises(ValueError, match=re.escape(rows[-1][1])):
        fresh_pool(root).set_min_quality(q, scores=short)
    with pytest.raises(ValueError, match="scores for"):
        fresh_pool(root).set_min_quality(q, scores=scores[:-1])


def test_draws_never_name_a_pair_at_or_below_the_bar(root):
    pool = fresh_pool(root, seed=11)
    table, scores = hand_scores(pool)
    q = float(scores[7])                                          # a score that a pair holds exactly: strict >, so it fails
    passing = {(int(c), int(n)) for (g, c, n), s in zip(table.tolist(), scores.tolist()) if s > q}
    failing = {(int(c), int(n)) for (g, c, n), s in zip(table.tolist(), scores.tolist()) if not s > q}
    assert (int(table[7, 1]), int(table[7, 2])) in failing and passing and len(failing) >= 9
    active = sorted({g for (g, c, n), s in zip(table.tolist(), scores.tolist()) if s > q})
    dead = sorted(set(range(pool.n_groups)) - set(active))
    assert pool.n_groups - 1 in dead and len(dead) >= 2             # the 0.1 group, and every group below the bar
    assert pool.n_active_groups == pool.n_groups
    assert pool.set_min_quality(q, scores=scores) == len(passing)
    assert pool.n_active_groups == len(active) and pool.n_groups == 6 and pool.min_quality == q
    seen, seen_groups = set(), set()
    for _ in range(30):
        d = pool.draw(10, cs=8)
        seen |= {(int(c), int(n)) for c, n in d.table[:, :2].tolist()}
        seen_groups |= set(d.groups.tolist())
        group_of = {(int(c), int(n)): g for g, c, n in table.tolist()}
        assert [group_of[(int(c), int(n))] for c, n in d.table[:, :2].tolist()] == d.groups.tolist()
    assert seen == passing, (seen - passing, passing - seen)      # 300 draws: none at or below the bar, every passing pair
    assert seen_groups == set(active)
    # epochs: every active group once, no other; steps follow n_active_groups; the split rule holds for the active groups
    batches = list(pool.epoch(2, cs=8))
    assert len(batches) == len(active) // 2
    groups = [g for d in batches for g in d.groups.tolist()]
    assert len(set(groups)) == len(groups) and set(groups) <= set(active)
    assert all((int(c), int(n)) in passing for d in batches for c, n in d.table[:, :2].tolist())
    one = fresh_pool(root, seed=5)
    one.set_min_quality(0.0, scores=scores)                       # NaN never passes, whatever the bar; 0.1 does here
    assert one.n_active_groups == pool.n_groups
    nan_pairs = {(int(c), int(n)) for (g, c, n), s in zip(table.tolist(), scores.tolist()) if math.isnan(s)}
    assert nan_pairs
    for _ in range(30):
        assert not nan_pairs & {(int(c), int(n)) for c, n in one.draw(10, cs=8).table[:, :2].tolist()}
    ranks = [fresh_pool(root, seed=5) for _ in range(2)]
    for p in ranks:
        p.set_min_quality(0.0, scores=scores)
    whole = [d.table for d in fresh_and_barred(root, scores).epoch(1, cs=8)]
    dealt = [[d.table for d in p.epoch(1, cs=8, rank=r, world=2)] for r, p in enumerate(ranks)]
    assert len(dealt[0]) == len(dealt[1]) == len(whole) // 2
    for k in range(len(whole) // 2 * 2):
        assert torch.equal(dealt[k % 2][k // 2], whole[k])
    # a bar above every score leaves nothing to draw from
    pool.set_min_quality(2.0, scores=scores)
    assert pool.n_active_groups == 0 and list(pool.epoch(1, cs=8)) == []


def fresh_and_barred(root, scores):
    pool = fresh_pool(root, seed=5)
    pool.set_min_quality(0.0, scores=scores)
    return pool


def test_a_bar_set_and_removed_leaves_the_parent_s_draws(root):
    plain, barred = fresh_pool(root, seed=21), fresh_pool(root, seed=21)
    _, scores = hand_scores(barred)
    barred.set_min_quality(0.6, scores=scores)
    assert barred.n_active_groups < barred.n_groups
    barred.set_min_quality(None)
    assert barred.n_active_groups == barred.n_groups and barred.min_quality is None
    for _ in range(3):
        assert torch.equal(plain.draw(7).table, barred.draw(7).table)
    for a, b in zip(plain.epoch(2), barred.epoch(2)):
        assert torch.equal(a.table, b.table) and torch.equal(a.groups, b.groups)
    assert torch.equal(plain.generator.get_state(), barred.generator.get_state())


def test_nn_train_options_and_a_bar_that_leaves_less_than_one_step(root, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = nn_train.parse_args(["--test_reserve", "0"])
    assert (args.min_quality, args.min_quality_epochs, args.quality_csv) == (None, 0, None)
    args = nn_train.parse_args(["--test_reserve", "0", "--min_quality", "0.8", "--min_quality_epochs", "2", "--quality_csv", "q.csv"])
    assert (args.min_quality, args.min_quality_epochs, args.quality_csv) == (0.8, 2, "q.csv")
    for argv in (["--quality_csv", "q.csv"], ["--min_quality_epochs", "1"]):
        with pytest.raises(ValueError, match="needs --min_quality"):
            nn_train.check_supported(nn_train.parse_args(["--test_reserve", "0"] + argv))

    pool = fresh_pool(root)
    _, scores = hand_scores(pool)
    pool.scores = scores
    pool.list_content_quality(export=True, out_dir=str(tmp_path / "datasets"))
    path = str(tmp_path / "datasets" / "NIND_24_16-msssim.csv")
    # the run itself, on a pool that no GPU holds: with scores from a file the bar is set by torch ops alone, and the refusal comes
    # before the model, the trainer or any batch -- each of which would raise for want of a GPU here
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(nn_common, "default_device", lambda: torch.device("cpu"))
    argv = ["--test_reserve", "0", "--train_data", root, "--cs", "8", "--batch_size", "3", "--g_lr", "1e-3", "--beta1", "0.75",
            "--patience", "2", "--reduce_lr_factor", "0.5", "--models_dpath", str(tmp_path / "models"), "--expname", "bar",
            "--weight_MSE", "1", "--validation_interval", "0", "--quality_csv", path]
    q = float(scores[7])                                          # 4 active groups: one step of 3
    lines = []
    steps = nn_train.set_quality_bar(fresh_pool(root), q, path, 3, 1, lines.append)
    assert steps == 1 and "pairs pass" in lines[0] and "4 of 6 groups active; 1 steps per epoch" in lines[0]
    with pytest.raises(ValueError, match="--min_quality 0.635 leaves 2 active groups"):
        nn_train.run(nn_train.parse_args(argv + ["--min_quality", "0.635"]), argv=["nn_train.py"])
    with open(tmp_path / "models" / "bar" / "train.log") as f:
        log = f.read()
    assert "Quality bar: MS-SSIM > 0.635" in log and "2 of 6 groups active; 0 steps per epoch" in log
    assert not any(f.startswith("generator_") for f in os.listdir(tmp_path / "models" / "bar"))
