"""GPU tests of the crop pool's quality scores: nd_pool_fetch bit for bit against numpy, CropPool.score_pairs against the oracle's
MS-SSIM in float64, draws under a quality bar, and nn_train with --min_quality end to end.

Bars.  The fetch is a copy and one correctly rounded division: no tolerance.  A score is nd_ms_ssim's, held to SCORE_TOL, the bar
tests/test_eval_harness.py holds that kernel to.  A pair of one image with itself is held to |score - 1| <= 2^-23, one step of
fp32 at 1 (test_a_pair_of_one_image_with_itself_scores_one)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import workspace_guard as G
from nind_denoise_amd import _lib
from nind_denoise_amd.common.libs import imgcodec
from nind_denoise_amd.crop_pool import CropPool
from oracle import losses as olosses
from test_eval_harness import SCORE_TOL

pytestmark = pytest.mark.gpu

SIGMAS = (0.02, 0.06, 0.15)     # the noise of the three noisy ISOs of a group, in units of the full range
ONE_STEP = 2.0 ** -23


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def words(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def to_float(img):
    """np_imgops.img_path_to_np_flt on [3, H, W] samples: correctly rounded fp32 divisions"""
    if img.dtype == np.uint8:
        return img.astype(np.float32) / np.float32(255)
    if img.dtype == np.uint16:
        return img.astype(np.float32) / np.float32(65535)
    return img


def scene(h, w, seed):
    """bilinear-upsampled noise in [0.1, 0.9] as float [3, h, w]"""
    g = torch.Generator().manual_seed(seed)
    c = F.interpolate(torch.rand(1, 3, max(h // 8, 2), max(w // 8, 2), generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * c[0] + 0.1).numpy()


def as_u8(img):
    return (np.clip(img, 0, 1) * 255).round().astype(np.uint8)


def graded_group(h, w, seed):
    """2 clean x 3 noisy u8 images of one scene: the second clean image differs from the first by half a grey level of noise, the
    noisy ones carry SIGMAS"""
    rng = np.random.default_rng(seed)
    base = scene(h, w, seed)
    clean = [as_u8(base), as_u8(base + 0.002 * rng.standard_normal(base.shape))]
    noisy = [as_u8(base + s * rng.standard_normal(base.shape)) for s in SIGMAS]
    return clean, noisy


# ------------------------------------------------------------------ nd_pool_fetch
FETCH_SIZES = [(161, 161), (176, 161), (9, 17)]


def fetch(dev, pool, index, h, w):
    buf, table = pool.device_buffers()
    idx = torch.tensor(index, dtype=torch.int32, device=dev)
    out, handle = G.typed((len(index), 3, h, w), torch.float32, dev, fill=0xFF)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nd_pool_fetch(buf.data_ptr(), buf.numel(), table.data_ptr(), table.shape[0], idx.data_ptr(), len(index),
                                             h, w, out.data_ptr(), _lib.stream_ptr(dev)), "nd_pool_fetch")
    torch.cuda.synchronize()
    return out, handle


@pytest.fixture(scope="module")
def typed_pool(dev):
    """Per size of FETCH_SIZES one u8, one u16 and one f32 pair; the float images leave [0, 1] and hold negative samples."""
    rng = np.random.default_rng(5)
    pool, images = CropPool(dev, cs=8), []
    for h, w in FETCH_SIZES:
        for make in (lambda s: rng.integers(0, 256, s).astype(np.uint8), lambda s: rng.integers(0, 65536, s).astype(np.uint16),
                     lambda s: rng.uniform(-0.3, 1.4, s).astype(np.float32)):
            pair = [make((3, h, w)), make((3, h, w))]
            pool.add_group(pair[:1], pair[1:])
            images += pair
    return pool, images


@pytest.mark.parametrize("h,w", FETCH_SIZES, ids=[f"{h}x{w}" for h, w in FETCH_SIZES])
def test_pool_fetch_is_the_numpy_conversion_bit_for_bit(dev, typed_pool, h, w):
    pool, images = typed_pool
    mine = [i for i, img in enumerate(images) if img.shape[1:] == (h, w)]
    other = [i for i, img in enumerate(images) if img.shape[1:] != (h, w)]
    assert len(mine) == 6 and {images[i].dtype for i in mine} == {np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32)}
    # every image of this size, some twice and out of order; rows of another size; indices outside the table
    index = mine[::-1] + [other[0], mine[2], -1, len(images), other[-1], 2 ** 31 - 1, -2 ** 31, mine[0]]
    out, handle = fetch(dev, pool, index, h, w)
    G.assert_guards(handle, f"nd_pool_fetch {h}x{w}: out")
    got = words(out)
    for k, i in enumerate(index):
        if i in mine:
            want = np.ascontiguousarray(to_float(images[i]))
            assert want.dtype == np.float32 and np.array_equal(got[k], want.view(np.int32)), (k, i, images[i].dtype)
        else:
            assert not got[k].any(), (k, i)                     # all zeros, not the 0xFF the buffer held


def test_pool_fetch_refusals(dev, typed_pool):
    pool, images = typed_pool
    buf, table = pool.device_buffers()
    idx = torch.zeros(4, dtype=torch.int32, device=dev)
    out = torch.empty(4, 3, 9, 17, device=dev)
    lib, sp = _lib.load(), _lib.stream_ptr(dev)
    good = [buf.data_ptr(), buf.numel(), table.data_ptr(), table.shape[0], idx.data_ptr(), 4, 9, 17, out.data_ptr()]
    assert lib.nd_pool_fetch(*good, sp) == 0
    for pos, value in ((0, None), (2, None), (4, None), (8, None), (5, 0), (5, 65536), (6, 0), (6, 16385), (7, 0), (7, 16385)):
        args = list(good)
        args[pos] = value
        with pytest.raises(ValueError, match="nd_pool_fetch"):
            _lib.check(lib.nd_pool_fetch(*args, sp), "nd_pool_fetch")
    torch.cuda.synchronize()


# ------------------------------------------------------------------ scores
@pytest.fixture(scope="module")
def graded(dev):
    """The pool of the score tests -- two 161 x 161 groups and one 176 x 161 group of 2 clean x 3 noisy u8 images, then a 160 x 161
    group and a group that pairs an image with itself -- with its scores (batch_size 4) and their float64 reference.  Shared, never
    modified."""
    pool, sources = CropPool(dev, seed=3, cs=48), []
    for k, (h, w) in enumerate(((161, 161), (161, 161), (176, 161))):
        clean, noisy = graded_group(h, w, seed=10 + k)
        pool.add_group(clean, noisy)
        sources.append((clean, noisy))
    small = graded_group(160, 161, seed=20)
    pool.add_group(small[0][:1], small[1][:1])
    sources.append((small[0][:1], small[1][:1]))
    same = [sources[0][0][0]]
    pool.add_group(same, same)
    sources.append((same, same))
    scores = pool.score_pairs(4)
    assert scores is pool.scores and scores.dtype == torch.float32 and scores.device == dev
    table = pool.pair_table()
    assert torch.equal(pool.pairs.cpu(), torch.from_numpy(table)) and scores.shape == (len(table),) == (20,)
    want = []
    for g, c, n in table:
        cl, no, h, w = pool.group(g)
        x, y = (torch.from_numpy(to_float(src[i - first[0]])).double()[None] for src, first, i in
                ((sources[g][0], cl, c), (sources[g][1], no, n)))
        want.append(olosses.ms_ssim(x, y).item() if min(h, w) >= 161 else float("nan"))
    return pool, sources, table, scores.cpu(), torch.tensor(want, dtype=torch.float64)


def test_scores_equal_the_oracle_s_ms_ssim(graded):
    pool, _, table, scores, want = graded
    scored = ~torch.isnan(want)
    assert int(scored.sum()) == 19
    err = (scores.double() - want)[scored].abs()
    print(f"score_pairs: scores {scores.tolist()}, worst |err| to float64 {err.max().item():.3e}, bar {SCORE_TOL:.1e}")
    assert torch.isfinite(scores[scored]).all() and err.max().item() < SCORE_TOL
    # a 160-pixel side: NaN, where piqa raises
    assert torch.isnan(scores[~scored]).all() and [int(table[k, 0]) for k in (~scored).nonzero().reshape(-1)] == [3]


def test_a_pair_of_one_image_with_itself_scores_one(graded):
    """|score - 1| <= 2^-23 = 1.192e-07 for the pair (image, image).  k_ssim_tile (csrc/ssim.hip) forms the x, y and xy moments with
    the same explicit operations, so the SSIM and contrast maps of two equal images are exactly 1 at every pixel; what is left is
    the mean (sum * fl(1 / N)), powf and the channel average, each within a step of 2^-24.  With the moments left to the compiler's
    contraction, which fused s_xx and s_yy and not s_xy, this pair scored 1 - 1.788e-07."""
    pool, _, table, scores, _ = graded
    assert table[-1, 1] == table[-1, 2]
    print(f"self pair: score {scores[-1].item()!r}, 1 - score = {1 - scores[-1].double().item():.3e}, bar {ONE_STEP:.3e}")
    assert abs(scores[-1].double().item() - 1) <= ONE_STEP


def test_scores_fall_with_the_noise_level(graded):
    pool, _, table, scores, _ = graded
    for g in range(3):
        cl, no, _, _ = pool.group(g)
        for c in cl:
            s = [scores[int(np.flatnonzero((table[:, 1] == c) & (table[:, 2] == n))[0])].item() for n in no]
            assert s[0] > s[1] > s[2], (g, c, s)


def test_scores_do_not_depend_on_the_batch_size(dev, graded):
    pool, _, _, scores, _ = graded
    kept = pool.scores
    try:
        one, seven, whole = pool.score_pairs(1).cpu(), pool.score_pairs(7).cpu(), pool.score_pairs().cpu()
    finally:
        pool.scores = kept
    assert np.array_equal(words(one), words(seven)) and np.array_equal(words(one), words(whole))
    assert np.array_equal(words(one), words(scores))


# ------------------------------------------------------------------ filtered training data
def test_epoch_batches_hold_only_pairs_above_the_bar(dev, graded):
    pool, sources, table, scores, _ = graded
    cs = 48
    high = [k for k, (g, c, n) in enumerate(table) if g < 3 and n == pool.group(g)[1][2]]
    rest = [k for k, (g, c, n) in enumerate(table) if g < 3 and n != pool.group(g)[1][2]]
    q = (scores[high].max().item() + scores[rest].min().item()) / 2
    assert scores[high].max().item() < q < scores[rest].min().item()          # the bar lies between two ISO levels
    passing = {(int(table[k, 1]), int(table[k, 2])) for k in rest} | {(int(table[-1, 1]), int(table[-1, 2]))}
    try:
        assert pool.set_min_quality(q) == len(passing) and pool.n_active_groups == 4      # not the 160-pixel group
        batches = [(d, pool.batch(d)) for _ in range(6) for d in pool.epoch(2, cs=cs)]
    finally:
        pool.set_min_quality(None)
    torch.cuda.synchronize()
    assert len(batches) == 6 * 2
    # output pixel -> crop pixel for each orientation, from the library's own map
    lib, a, b = _lib.load(), _lib.c_int(), _lib.c_int()
    maps = {}
    seen = set()
    for d, (clean, noisy) in batches:
        assert set(d.groups.tolist()) <= {0, 1, 2, 4}
        rows = d.table.cpu().tolist()
        ids = sorted({i for r in rows for i in r[:2]})
        for k, (c, n, x0, y0, nrot, f1, f2, _) in enumerate(rows):
            assert (c, n) in passing, (c, n)
            seen.add((c, n))
            key = (nrot, f1 | (f2 << 1))
            if key not in maps:
                ya, xb = np.empty((cs, cs), np.int64), np.empty((cs, cs), np.int64)
                for y in range(cs):
                    for x in range(cs):
                        _lib.check(lib.nd_crop_source(cs, key[0], key[1], y, x, a, b), "nd_crop_source")
                        ya[y, x], xb[y, x] = a.value, b.value
                maps[key] = (ya, xb)
            ya, xb = maps[key]
            _, _, h, w = pool.group(int(d.groups[k]))
            whole, _ = fetch(dev, pool, [c, n], h, w)                 # the images the draw names, as nd_pool_fetch gives them
            whole = whole.cpu().numpy()
            for got, img in ((clean[k], whole[0]), (noisy[k], whole[1])):
                want = np.ascontiguousarray(img[:, y0 + ya, x0 + xb])
                assert np.array_equal(words(got), want.view(np.int32)), (c, n, x0, y0, nrot, f1, f2)
    assert len(seen) > 4                                              # more than one pair of a group is drawn


# ------------------------------------------------------------------ nn_train end to end
SIDE, CS, BATCH = 168, 104, 2


def write_tree(root):
    """<root>/SYN_168_96: set `fine` with four crops at ISO100, ISO400 (little noise) and ISO6400 (much), and set `rough` with four
    crops at ISO100 and ISO6400 only: under a bar between the two noise levels half of the eight groups have no pair left."""
    data = os.path.join(root, f"SYN_{SIDE}_96")
    rng = np.random.default_rng(7)
    for aset, isos in (("fine", {"ISO100": 0.0, "ISO400": SIGMAS[0], "ISO6400": SIGMAS[2]}), ("rough", {"ISO100": 0.0, "ISO6400": SIGMAS[2]})):
        for k in range(4):
            base = 0.3 * scene(SIDE, SIDE, seed=100 + k + 10 * len(isos))
            for iso, sigma in isos.items():
                os.makedirs(os.path.join(data, aset, iso), exist_ok=True)
                img = as_u8(base + sigma * rng.standard_normal(base.shape))
                imgcodec.write_png(os.path.join(data, aset, iso, f"SYN_{aset}_{iso}_{k}_0_96.png"), np.ascontiguousarray(img.transpose(1, 2, 0)))
    return data


def test_nn_train_with_a_quality_bar_end_to_end(dev, tmp_path, monkeypatch, capsys):
    from nind_denoise_amd import nn_train
    from nind_denoise_amd.tools import make_dataset_crops_list
    monkeypatch.chdir(tmp_path)
    data = write_tree(str(tmp_path))
    probe = CropPool.from_directories([data], device=dev)
    table, scores = probe.pair_table(), probe.score_pairs().cpu()
    assert probe.n_groups == 8 and len(table) == 12 and torch.isfinite(scores).all()
    low = [k for k, (x, y) in enumerate(probe.pair_paths()) if "ISO400" in y]
    high = [k for k in range(12) if k not in low]
    assert len(low) == 4 and scores[high].max() < scores[low].min()
    q = (scores[high].max().item() + scores[low].min().item()) / 2
    passing = {(int(table[k, 1]), int(table[k, 2])) for k in low}

    # the new command: the csv of this tree, and what it says on the way
    assert make_dataset_crops_list.main(["--train_data", data, "--test_reserve", "0"]) == 0
    said = capsys.readouterr().out
    csv_path = os.path.join("datasets", f"SYN_{SIDE}_96-msssim.csv")
    assert said.rstrip().endswith(f"Quality check exported to {csv_path}")
    assert re.search(r"12 pairs of 8 groups scored in [0-9.]+ s \([0-9]+ pairs/s\); 0 left unscored", said), said
    with open(csv_path) as f:
        lines = f.read().splitlines()
    assert lines[0] == "xpath,ypath,score" and [float(line.rsplit(",", 1)[1]) for line in lines[1:]] == scores.double().tolist()

    drawn = []
    batch = CropPool.batch

    def hooked(self, draws, *args, **kwargs):
        drawn.append((self.min_quality, draws.table[:, :2].clone()))
        return batch(self, draws, *args, **kwargs)
    monkeypatch.setattr(CropPool, "batch", hooked)

    def train(expname, extra):
        argv = ["--g_funit", "8", "--cs", str(CS), "--loss_cs", "60", "--batch_size", str(BATCH), "--weight_MSE", "1", "--g_lr", "1e-3",
                "--epochs", "3", "--patience", "2", "--seed", "7", "--expname", expname, "--beta1", "0.75", "--reduce_lr_factor", "0.5",
                "--train_data", data, "--test_reserve", "0", "--validation_interval", "0", "--models_dpath", str(tmp_path / "models"),
                "--log_interval", "1", "--min_quality", repr(q), "--min_quality_epochs", "1"] + extra
        del drawn[:]
        assert nn_train.main(argv) == 0
        run = os.path.join(str(tmp_path / "models"), expname)
        with open(os.path.join(run, "train.log")) as f:
            log = f.read()
        # epoch 1 under the bar: 4 active groups, 2 steps; epoch 2 without: 8 groups, 4 steps
        assert "4 of 12 pairs pass, 4 of 8 groups active; 2 steps per epoch" in log
        assert "Quality bar lifted after 1 epoch(s): 8 groups active; 4 steps per epoch" in log
        assert log.index("Epoch 1 summary:") < log.index("Quality bar lifted") < log.index("Epoch 2 batch 1/4")
        assert "Epoch 1 batch 2/2" in log and "Epoch 1 batch 3/" not in log and "Epoch 2 batch 4/4" in log
        assert [m is not None for m, _ in drawn] == [True] * 2 + [False] * 4
        first = [tuple(r) for m, t in drawn if m is not None for r in t.cpu().tolist()]
        assert len(first) == 2 * BATCH and set(first) <= passing, (first, passing)
        later = {tuple(r) for m, t in drawn if m is None for r in t.cpu().tolist()}
        assert later - passing                                          # the lifted bar lets the noisy pairs back in
        with open(os.path.join(run, "generator_2.pt"), "rb") as f:
            return log, f.read()

    log1, ckpt1 = train("scored", [])
    log2, ckpt2 = train("listed", ["--quality_csv", csv_path])
    assert "scored on the pool in" in log1 and csv_path in log2
    sd = torch.load(os.path.join(str(tmp_path / "models"), "scored", "generator_2.pt"), map_location="cpu", weights_only=True)
    assert all(torch.isfinite(v).all() for v in sd.values())
    assert ckpt1 == ckpt2                                               # scored at start or read from the file: the same run
