"""The window forms of the crop-pool kernels on the GPU (csrc/crop_batch.hip: nd_crop_batch_windows, nd_pool_fetch_windows) and
the pool of full-size images behind them (CropPool.from_full_size), bit for bit against the dense forms: a window must give what
the same rectangle gives once it is cut out and stored on its own, as a crop file is.  Every comparison is on the float32 words;
there is no tolerance to choose.

What catches what, in test_windows_equal_the_cut_out_images and test_padding_is_zeros_not_the_frame:
  a wrong row pitch (the window's width for the frame's)      every window narrower than its frame: rows after the first differ
                                                               from the cut-out image's (the equality of clean / noisy words)
  a plane pitch taken from the window (H * W for PH * PW)     the same equality, in planes 1 and 2 of every window smaller than its
                                                               frame; the one-pixel window shows nothing else
  padding read from the frame                                  the count of non-zero samples at cs above a side (the frames hold no
                                                               zero), and the equality; xmax of a window whose frame holds a
                                                               larger sample next to it"""
import itertools
import json
import os

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib
from nind_denoise_amd.crop_pool import CropPool, pack_draws
from test_crop_pool_host import numpy_sample
from test_pool_windows_host import crop_tree, write_full_size
from workspace_guard import assert_guards, guarded

pytestmark = pytest.mark.gpu
PH, PW = 37, 53
U8, U16, F32 = _lib.SAMPLE_U8, _lib.SAMPLE_U16, _lib.SAMPLE_F32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def words(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


# ------------------------------------------------------------------ kernel edges
# (y, x, h, w): the four corners, one pixel, the whole frame
WINDOWS = [(0, 0, 9, 11), (0, PW - 11, 9, 11), (PH - 9, 0, 9, 11), (PH - 9, PW - 11, 9, 11), (17, 23, 1, 1), (0, 0, PH, PW)]
# crop sizes below, equal to and above each side
CS_OF = {(9, 11): (7, 9, 10, 11, 14), (1, 1): (1, 2, 3), (PH, PW): (24, PH, 40, PW, 60)}
PLANTED = [(9, 5), (17, 24), (8, 11), (PH - 10, PW - 5)]     # just outside the first corner, the one-pixel and the last corner window


def frames():
    """One 3 x 37 x 53 frame of each sample type.  No sample is zero; u16 and f32 samples are all different; each frame's largest
    samples sit at PLANTED, next to windows and inside none but the whole frame."""
    idx = np.arange(3 * PH * PW).reshape(3, PH, PW)
    u8 = (idx * 7 % 199 + 1).astype(np.uint8)                      # 1..199
    u16 = (idx * 5 + 1).astype(np.uint16)                          # 1..29416, all different
    f32 = (0.001 + idx / (3 * PH * PW) * 0.6).astype(np.float32)   # 0.001..0.601, all different
    for c in range(3):
        for j, (y, x) in enumerate(PLANTED):
            u8[c, y, x], u16[c, y, x], f32[c, y, x] = 250 + c, 60000 + 10 * j + c, 0.9 + 0.01 * c + 0.001 * j
    assert u8.min() > 0 and len(np.unique(u16)) == u16.size and len(np.unique(f32)) == f32.size
    return [u8, u16, f32]


def lay_out(arrays, dev):
    """(pool bytes on the device between guard bytes, its handle, the byte offset of each array): each aligned to 16, and the pool
    ends with the last array's last byte, so that a read past it is a read of guard bytes"""
    offs, size = [], 0
    for a in arrays:
        offs.append((size + 15) // 16 * 16)
        size = offs[-1] + a.nbytes
    host = np.zeros(size, dtype=np.uint8)
    for off, a in zip(offs, arrays):
        host[off:off + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    pool, handle = guarded(size, dev)
    pool.copy_(torch.from_numpy(host))
    return pool, handle, offs


TYPE_OF = {np.dtype(np.uint8): U8, np.dtype(np.uint16): U16, np.dtype(np.float32): F32}


@pytest.fixture(scope="module")
def edges(dev):
    """The frames as a pool of windows and the cut-out windows as a dense pool, with one table row per (frame, window) in the same
    order in both: image 6 * f + k is window k of frame f."""
    frs = frames()
    wpool, whandle, woffs = lay_out(frs, dev)
    wrows = [(woffs[f], h, w, TYPE_OF[frs[f].dtype], y, x, PH, PW) for f in range(3) for (y, x, h, w) in WINDOWS]
    cuts = [np.ascontiguousarray(frs[f][:, y:y + h, x:x + w]) for f in range(3) for (y, x, h, w) in WINDOWS]
    dpool, dhandle, doffs = lay_out(cuts, dev)
    drows = [(off, a.shape[1], a.shape[2], TYPE_OF[a.dtype]) for off, a in zip(doffs, cuts)]
    return {"frames": frs, "cuts": cuts, "wpool": wpool, "whandle": whandle, "dpool": dpool, "dhandle": dhandle,
            "wtable": torch.tensor(wrows, dtype=torch.int64, device=dev), "dtable": torch.tensor(drows, dtype=torch.int64, device=dev)}


def run_batch(name, pool, table, draws, cs, dev, mmin=1.0, mmax=1.0, mult=None):
    """(clean, noisy, xmax, mult_out) of one call of the C entry point `name`, outputs prefilled with NaN"""
    n = draws.shape[0]
    clean = torch.full((n, 3, cs, cs), float("nan"), dtype=torch.float32, device=dev)
    noisy = torch.full_like(clean, float("nan"))
    xmax, mout = torch.full((2, n), float("nan"), dtype=torch.float32, device=dev)
    drawn = mult is None and mmin != 1.0
    with torch.cuda.device(dev):
        _lib.check(getattr(_lib.load(), name)(pool.data_ptr(), pool.numel(), table.data_ptr(), table.shape[0], draws.data_ptr(), n, cs,
                                              mmin, mmax, None if mult is None else mult.data_ptr(), xmax.data_ptr() if drawn else None,
                                              mout.data_ptr() if drawn else None, clean.data_ptr(), noisy.data_ptr(),
                                              _lib.stream_ptr(dev)), name)
    return clean, noisy, xmax, mout


def edge_draws(cs, dev):
    """Every window whose sizes list names cs, as the clean image of each frame with the same window of the next frame as the noisy
    one, in all four rotations and both flips, at each corner offset: rows (clean image, noisy image, x0, y0, nrot, flip1, flip2)"""
    rows = []
    for f, (k, (y, x, h, w)) in itertools.product(range(3), enumerate(WINDOWS)):
        if cs not in CS_OF[(h, w)]:
            continue
        for nrot, f1, f2, x0, y0 in itertools.product(range(4), (0, 1), (0, 1), {0, max(w - cs, 0)}, {0, max(h - cs, 0)}):
            rows.append((6 * f + k, 6 * ((f + 1) % 3) + k, x0, y0, nrot, f1, f2))
    u = [(37 * i % 101) / 101 for i in range(len(rows))]
    return rows, pack_draws(*zip(*rows), u, device=dev)


ALL_CS = sorted({cs for sizes in CS_OF.values() for cs in sizes})


@pytest.mark.parametrize("cs", ALL_CS)
def test_windows_equal_the_cut_out_images(edges, dev, cs):
    rows, draws = edge_draws(cs, dev)
    assert len(rows) >= 3 * 16 and {r[4:7] for r in rows} == set(itertools.product(range(4), (0, 1), (0, 1)))
    given = torch.linspace(0.4, 2.6, len(rows), device=dev)
    for what, kw in (("plain", {}), ("given multiplier", {"mult": given}), ("drawn multiplier", {"mmin": 0.85, "mmax": 1.15})):
        got = run_batch("nd_crop_batch_windows", edges["wpool"], edges["wtable"], draws, cs, dev, **kw)
        want = run_batch("nd_crop_batch", edges["dpool"], edges["dtable"], draws, cs, dev, **kw)
        for name, g, w in zip(("clean", "noisy", "xmax", "mult"), got, want):
            if name in ("xmax", "mult") and what != "drawn multiplier":
                assert torch.isnan(g).all(), (what, name)                 # not asked for: not written
                continue
            assert not torch.isnan(g).any(), (what, name)
            differ = (words(g) != words(w)).reshape(len(rows), -1).any(1)
            assert not differ.any(), (what, name, cs, [rows[i] for i in np.flatnonzero(differ)[:4]])
    assert_guards(edges["whandle"], "the pool of frames")
    assert_guards(edges["dhandle"], "the pool of cut-out windows")
    # and against numpy on the cut-out windows, so that the two kernels cannot be wrong alike
    clean, noisy, _, _ = run_batch("nd_crop_batch_windows", edges["wpool"], edges["wtable"], draws, cs, dev)
    clean, noisy = words(clean), words(noisy)
    for i in range(0, len(rows), 7):
        want = numpy_sample(edges["cuts"][rows[i][0]], edges["cuts"][rows[i][1]], cs, *rows[i][2:])
        assert np.array_equal(clean[i], want[0].view(np.int32)) and np.array_equal(noisy[i], want[1].view(np.int32)), rows[i]


@pytest.mark.parametrize("cs", ALL_CS)
def test_padding_is_zeros_not_the_frame(edges, dev, cs):
    """The frames hold no zero sample, so a crop shows min(h, cs) * min(w, cs) non-zero samples per plane and nothing else; and the
    maximum of a padded or cut window is the window's, not the larger sample the frame holds beside it."""
    rows, draws = edge_draws(cs, dev)
    clean, noisy, xmax, mult = run_batch("nd_crop_batch_windows", edges["wpool"], edges["wtable"], draws, cs, dev, mmin=0.85, mmax=1.15)
    top = {0: 255.0, 1: 65535.0, 2: 1.0}
    for i, r in enumerate(rows):
        f, k = divmod(r[0], 6)
        y, x, h, w = WINDOWS[k]
        inside = 3 * min(h, cs) * min(w, cs)
        assert int((clean[i] != 0).sum()) == inside and int((noisy[i] != 0).sum()) == inside, (cs, r)
        part = edges["cuts"][r[0]][:, r[3]:r[3] + cs, r[2]:r[2] + cs]                 # what the crop shows of the window
        m = np.float32(part.max()) / np.float32(top[f])
        if h < cs or w < cs:
            m = max(m, np.float32(0))
        assert xmax[i].item() == m, (cs, r, xmax[i].item(), m)
        if (h, w) != (PH, PW):
            assert xmax[i].item() < 0.9                                                # the planted samples are 0.9 and above
    if cs in CS_OF[(PH, PW)]:
        assert float(xmax.max()) >= 0.9                                                # the whole frame does show them


def test_bad_rows_read_as_zeros_and_neighbours_stay_right(edges, dev):
    """Each row below is one the device guard is written to catch; nothing here reads outside the pool."""
    frs = edges["frames"]
    good = edges["wtable"].cpu().numpy()
    offs = [int(good[6 * f][0]) for f in range(3)]
    nbytes = edges["wpool"].numel()
    bad = [
        (offs[0], 9, 11, U8, 0, PW - 10, PH, PW),          # leaves its parent on the right
        (offs[0], 9, 11, U8, PH - 8, 0, PH, PW),           # and below
        (offs[1], PH, PW, U16, 1, 0, PH, PW),              # the whole frame, one row down
        (offs[0], 9, 11, U8, -1, 0, PH, PW),               # negative origin
        (offs[0], 9, 11, U8, 0, -1, PH, PW),
        (offs[2], 9, 11, F32, 0, 0, PH + 1, PW),           # the parent leaves the pool: the last frame, one row longer
        (nbytes - 16, 9, 11, U8, 0, 0, PH, PW),            # a parent that starts inside the pool and ends outside
        (nbytes + 16, 1, 1, U8, 0, 0, 1, 1),               # and one that starts outside
        (-16, 9, 11, U8, 0, 0, PH, PW),
        (offs[0], 9, 11, 3, 0, 0, PH, PW),                 # bad type
        (offs[0], 9, 11, -1, 0, 0, PH, PW),
        (offs[1] + 1, 9, 11, U16, 0, 0, PH - 1, PW),       # bad alignment
        (offs[2] + 2, 9, 11, F32, 0, 0, PH - 1, PW),
        (offs[0], 0, 11, U8, 0, 0, PH, PW),                # an empty window
        (offs[0], 9, 11, U8, 0, 0, PH, 0),                 # an empty parent
        (offs[0], 2 ** 31, 11, U8, 0, 0, 2 ** 31, PW),     # sides that do not fit int32
        (offs[0], 9, 11, U8, 2 ** 62, 0, PH, PW),          # an origin whose sum with the side would wrap
    ]
    ok = 6 * 0 + 3                                          # the u8 frame's last corner, 9 x 11; its noisy partner in the u16 frame
    table = torch.tensor([tuple(r) for r in good] + bad, dtype=torch.int64, device=dev)
    n_good, cs = len(good), 14
    picks = [n_good + i for i in range(len(bad))] + [len(table), len(table) + 7, -1, 2 ** 31 - 1]     # and indices outside the table
    rows = []
    for p in picks:             # good, bad clean, good, bad noisy, good: every bad sample between two good ones
        rows += [(ok, ok + 6, 0, 0, 1, 1, 0), (p, ok + 6, 0, 0, 0, 0, 0), (ok, ok + 6, 0, 0, 2, 0, 1), (ok, p, 0, 0, 0, 0, 0)]
    draws = pack_draws(*zip(*rows), [0.5] * len(rows), device=dev)
    two = pack_draws(*zip(rows[0], rows[2]), [0.5, 0.5], device=dev)        # the good neighbours' draws, on the dense pool
    for kw in ({}, {"mmin": 0.85, "mmax": 1.15}):
        clean, noisy, xmax, mult = run_batch("nd_crop_batch_windows", edges["wpool"], table, draws, cs, dev, **kw)
        want = run_batch("nd_crop_batch", edges["dpool"], edges["dtable"], two, cs, dev, **kw)
        assert not torch.isnan(clean).any() and not torch.isnan(noisy).any()
        for i, r in enumerate(rows):
            kind = i % 4
            if kind in (0, 2):      # the good neighbours: what the dense pool gives for the same draw
                assert np.array_equal(words(clean[i]), words(want[0][kind // 2])), (i, r)
                assert np.array_equal(words(noisy[i]), words(want[1][kind // 2])), (i, r)
                assert int((clean[i] != 0).sum()) == 3 * 9 * 11
            elif kind == 1:         # a bad clean image: the pair is zeros (the noisy image is cut as the clean one is)
                assert not clean[i].any() and not noisy[i].any(), (i, r)
                if kw:
                    assert xmax[i].item() == 0 and 0.85 <= mult[i].item() <= 1.15
            else:                   # a bad noisy image: zeros beside the right clean crop
                assert not noisy[i].any() and int((clean[i] != 0).sum()) == 3 * 9 * 11, (i, r)
    assert_guards(edges["whandle"], "the pool of frames")
    # the same rows through nd_pool_fetch_windows, and a row of another size than the one asked for
    index = torch.tensor([ok, ok + 6] + picks + [0, 5, ok + 12], dtype=torch.int32, device=dev)
    out = torch.full((len(index), 3, 9, 11), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().nd_pool_fetch_windows(edges["wpool"].data_ptr(), nbytes, table.data_ptr(), table.shape[0], index.data_ptr(),
                                                     len(index), 9, 11, out.data_ptr(), _lib.stream_ptr(dev)), "nd_pool_fetch_windows")
    y, x, h, w = WINDOWS[3]
    assert np.array_equal(out[0].cpu().numpy(), frs[0][:, y:y + h, x:x + w].astype(np.float32) / np.float32(255))
    assert np.array_equal(out[1].cpu().numpy(), frs[1][:, y:y + h, x:x + w].astype(np.float32) / np.float32(65535))
    assert np.array_equal(out[-1].cpu().numpy(), frs[2][:, y:y + h, x:x + w])
    assert not out[2:-3].any() and not out[-2].any(), "a bad row, an index outside the table or a 37 x 53 row asked for as 9 x 11"
    assert np.array_equal(out[-3].cpu().numpy(), frs[0][:, :9, :11].astype(np.float32) / np.float32(255))
    assert_guards(edges["whandle"], "the pool of frames")


def test_refusals_are_the_dense_forms(edges, dev):
    lib = _lib.load()
    p, t = edges["wpool"], edges["wtable"]
    d = pack_draws([0], [6], [0], [0], [0], [0], [0], [0.5], device=dev)
    o = torch.empty(2, 1, 3, 8, 8, device=dev)
    s = _lib.stream_ptr(dev)
    for name in ("nd_crop_batch", "nd_crop_batch_windows"):
        f = getattr(lib, name)

        def call(pool=p.data_ptr(), nbytes=p.numel(), table=t.data_ptr(), n=18, draws=d.data_ptr(), batch=1, cs=8, mmin=1.0, xm=None):
            return f(pool, nbytes, table, n, draws, batch, cs, mmin, 1.0, None, xm, xm, o[0].data_ptr(), o[1].data_ptr(), s)
        assert call() == 0
        for kw in ({"pool": None}, {"nbytes": 0}, {"table": None}, {"draws": None}, {"n": 0}, {"cs": 0}, {"cs": 16385}, {"batch": 0},
                   {"batch": 65536}, {"mmin": 0.5}, {"mmin": 1.5, "xm": o.data_ptr()}):
            assert call(**kw) == -1, (name, kw)                      # ND_EINVAL
            assert name + ":" in lib.nd_last_error().decode(), (name, kw, lib.nd_last_error().decode())
    for name in ("nd_pool_fetch", "nd_pool_fetch_windows"):
        f = getattr(lib, name)
        i = torch.zeros(1, dtype=torch.int32, device=dev)
        for n, h, w in ((0, 8, 8), (65536, 8, 8), (1, 0, 8), (1, 8, 16385)):
            assert f(p.data_ptr(), p.numel(), t.data_ptr(), 18, i.data_ptr(), n, h, w, o.data_ptr(), s) == -1, (name, n, h, w)
            assert name + ":" in lib.nd_last_error().decode()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ equivalence on a tree
TREES = {"u8-812x620": (812, 620, np.uint8), "u16-404x500": (404, 500, np.uint16)}


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """Full-size trees of two sets with a base ISO and two noisy ones, and this suite's cropper's trees at 128/96 and 176/128."""
    out = {}
    for name, (w, h, dtype) in TREES.items():
        root = str(tmp_path_factory.mktemp(name))
        dsdir = write_full_size(root, "SYN", w, h, dtype)
        out[name] = {"root": root, "dsdir": dsdir, (128, 96): crop_tree(dsdir, 128, 96), (176, 128): crop_tree(dsdir, 176, 128)}
    return out


def pool_pair(tree, cs, stride, dev, seed=5):
    return (CropPool.from_full_size(tree["dsdir"], ds_cs=cs, ds_stride=stride, device=dev, seed=seed),
            CropPool.from_directories(tree[(cs, stride)], device=dev, seed=seed))


def assert_same_epoch(wp, dp, batch, cs, **kw):
    steps = 0
    for dw, dd in zip(wp.epoch(batch, cs), dp.epoch(batch, cs)):
        assert torch.equal(dw.table, dd.table) and torch.equal(dw.groups, dd.groups)
        (wc, wn), (dc, dn) = wp.batch(dw, **kw), dp.batch(dd, **kw)
        assert np.array_equal(words(wc), words(dc)) and np.array_equal(words(wn), words(dn)), steps
        assert torch.isfinite(wc).all() and wc.any() and wn.any()
        if kw:
            assert torch.equal(wp.last_xmax, dp.last_xmax) and torch.equal(wp.last_mult, dp.last_mult)
        steps += 1
    return steps


@pytest.mark.parametrize("name", list(TREES))
@pytest.mark.parametrize("cs", [104, 136], ids=["cut-104", "padded-136"])
def test_an_epoch_of_the_window_pool_is_the_cropped_trees(trees, dev, name, cs):
    wp, dp = pool_pair(trees[name], 128, 96, dev)
    groups = {"u8-812x620": 70, "u16-404x500": 24}[name]
    assert wp.n_groups == dp.n_groups == groups and wp.n_frames == 6
    w, h, dtype = TREES[name]
    assert wp.nbytes == 6 * ((3 * h * w * np.dtype(dtype).itemsize + 15) // 16 * 16)        # each frame once
    assert dp.nbytes == groups * 3 * 3 * 128 * 128 * np.dtype(dtype).itemsize                 # each crop file
    assert wp.device_buffers()[1].shape == (groups * 3, 8) and dp.device_buffers()[1].shape == (groups * 3, 4)
    assert assert_same_epoch(wp, dp, 6, cs) == groups // 6
    assert assert_same_epoch(wp, dp, 6, cs, exp_mult_min=0.85, exp_mult_max=1.15) == groups // 6
    dw, dd = wp.draw(5, cs), dp.draw(5, cs)
    assert torch.equal(dw.table, dd.table) and torch.equal(wp.rng_state(), dp.rng_state())
    i = 3 * groups - 1
    assert np.array_equal(wp.image(i), dp.image(i)) and wp.image(i).dtype == TREES[name][2]       # read back from the device


@pytest.mark.parametrize("name", list(TREES))
def test_scores_and_the_quality_bar_are_the_cropped_trees(trees, dev, name, tmp_path):
    wp, dp = pool_pair(trees[name], 176, 128, dev)
    pairs = {"u8-812x620": 60, "u16-404x500": 8}[name]
    sw, sd = wp.score_pairs(), dp.score_pairs()
    assert sw.shape == (pairs,) and torch.isfinite(sw).all() and np.array_equal(words(sw), words(sd))
    assert sw.min() > 0 and sw.max() < 1 and sw.min() < sw.max()
    assert np.array_equal(words(wp.score_pairs(batch_size=7)), words(sw))
    # each pool's csv is the other's, and sets the same bar on it
    (tmp_path / "w").mkdir(), (tmp_path / "d").mkdir()
    wp.list_content_quality(export=True, out_dir=str(tmp_path / "w"))
    dp.list_content_quality(export=True, out_dir=str(tmp_path / "d"))
    csvs = [os.path.join(str(tmp_path), k, "SYN_176_128-msssim.csv") for k in "wd"]
    with open(csvs[0], "rb") as f1, open(csvs[1], "rb") as f2:
        assert f1.read() == f2.read()
    q = float(sw.median())
    w2, d2 = pool_pair(trees[name], 176, 128, dev, seed=9)
    assert w2.set_min_quality(q, csvs[1]) == d2.set_min_quality(q, csvs[0]) == int((sw > q).sum()) > 0
    assert w2.n_active_groups == d2.n_active_groups <= w2.n_groups
    assert assert_same_epoch(w2, d2, 2, 168) == w2.n_active_groups // 2
    assert torch.equal(w2.draw(9, 168).table, d2.draw(9, 168).table)


# ------------------------------------------------------------------ nn_train end to end
FUNIT = 8       # as tests/test_nn_train.py


@pytest.fixture(scope="module")
def train_tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("train"))
    dsdir = write_full_size(root, "SYN", 404, 500, isos=("ISO100", "ISO6400"))
    return {"root": root, "dsdir": dsdir, "cropped": crop_tree(dsdir, 128, 96)}


def train_argv(data, models, expname, epochs, extra=()):
    return ["--g_funit", str(FUNIT), "--cs", "104", "--loss_cs", "60", "--batch_size", "4", "--weight_MSE", "1", "--g_lr", "1e-3",
            "--epochs", str(epochs), "--patience", "2", "--seed", "7", "--beta1", "0.75", "--reduce_lr_factor", "0.5",
            "--test_reserve", "0", "--validation_interval", "0", "--models_dpath", models, "--expname", expname, "--log_interval", "0",
            "--g_network", "UtNet", "--save_state"] + list(data) + list(extra)


def same_file(a, b):
    with open(a, "rb") as f1, open(b, "rb") as f2:
        return f1.read() == f2.read()


def test_nn_train_on_full_size_data_is_the_run_on_the_cropped_tree(train_tree, dev):
    import yaml
    from nind_denoise_amd import nn_train
    models = os.path.join(train_tree["root"], "models")
    full = ["--full_size_data", train_tree["dsdir"], "--ds_cs", "128", "--ds_stride", "96"]
    assert nn_train.main(train_argv(full, models, "windows", 4)) == 0
    assert nn_train.main(train_argv(["--train_data", train_tree["cropped"]], models, "files", 4)) == 0
    w, f = os.path.join(models, "windows"), os.path.join(models, "files")
    assert same_file(os.path.join(w, "trainres.json"), os.path.join(f, "trainres.json"))
    assert same_file(os.path.join(w, "generator_3.pt"), os.path.join(f, "generator_3.pt"))
    with open(os.path.join(w, "trainres.json")) as fp:
        res = json.load(fp)
    assert {"1", "2", "3"} <= set(res) and all(np.isfinite(res[e]["train_weighted_loss"]) for e in "123")
    with open(os.path.join(w, "config.yaml")) as fp:
        conf = yaml.safe_load(fp)
    assert conf["full_size_data"] == [train_tree["dsdir"]] and (conf["ds_cs"], conf["ds_stride"], conf["train_data"]) == (128, 96, None)
    with open(os.path.join(f, "config.yaml")) as fp:
        assert not {"full_size_data", "ds_cs", "ds_stride"} & set(yaml.safe_load(fp))
    with open(os.path.join(w, "train.log")) as fp:
        assert "Crop pool: 24 groups, 48 images (windows into 4 frames)" in fp.read()
    with open(os.path.join(f, "train.log")) as fp:
        assert "Crop pool: 24 groups, 48 images, " in fp.read()


def test_a_resumed_run_on_full_size_data_rebuilds_the_pool(train_tree, dev):
    from nind_denoise_amd import nn_train
    models = os.path.join(train_tree["root"], "models_resume")
    full = ["--full_size_data", train_tree["dsdir"], "--ds_cs", "128", "--ds_stride", "96"]
    assert nn_train.main(train_argv(full, models, "straight", 4)) == 0
    assert nn_train.main(train_argv(full, models, "stopped", 3)) == 0
    stopped = os.path.join(models, "stopped")
    assert not os.path.exists(os.path.join(stopped, "generator_3.pt"))
    assert nn_train.main(["--resume", stopped, "--epochs", "4"]) == 0
    assert same_file(os.path.join(stopped, "generator_3.pt"), os.path.join(models, "straight", "generator_3.pt"))
    assert same_file(os.path.join(stopped, "trainres.json"), os.path.join(models, "straight", "trainres.json"))


def test_short_run_keeps_the_same_groups(train_tree, dev):
    from nind_denoise_amd import nn_train
    models = os.path.join(train_tree["root"], "models_short")
    full = ["--full_size_data", train_tree["dsdir"], "--ds_cs", "128", "--ds_stride", "96"]
    assert nn_train.main(train_argv(full, models, "windows", 3, ["--debug_options", "short_run"])) == 0
    assert nn_train.main(train_argv(["--train_data", train_tree["cropped"]], models, "files", 3, ["--debug_options", "short_run"])) == 0
    w, f = os.path.join(models, "windows"), os.path.join(models, "files")
    assert same_file(os.path.join(w, "trainres.json"), os.path.join(f, "trainres.json"))
    assert same_file(os.path.join(w, "generator_2.pt"), os.path.join(f, "generator_2.pt"))
    with open(os.path.join(w, "train.log")) as fp:
        assert "Crop pool: 12 groups, 24 images (windows into 2 frames)" in fp.read()      # the first set's: the other's are dropped


def test_make_dataset_crops_list_writes_the_cropped_trees_csv(trees, dev, tmp_path, monkeypatch):
    from nind_denoise_amd.tools import make_dataset_crops_list
    tree = trees["u16-404x500"]
    for kind, data in (("w", ["--full_size_data", tree["dsdir"], "--ds_cs", "176", "--ds_stride", "128"]),
                       ("d", ["--train_data", tree[(176, 128)]])):
        (tmp_path / kind).mkdir()
        monkeypatch.chdir(tmp_path / kind)
        assert make_dataset_crops_list.main(["--test_reserve", "0"] + data) == 0
    assert same_file(str(tmp_path / "w" / "datasets" / "SYN_176_128-msssim.csv"), str(tmp_path / "d" / "datasets" / "SYN_176_128-msssim.csv"))
    with open(tmp_path / "w" / "datasets" / "SYN_176_128-msssim.csv") as fp:
        lines = fp.read().splitlines()
    assert len(lines) == 1 + 8 and lines[1].startswith(os.path.join(tree[(176, 128)], "alley", "ISO100", "SYN_alley_ISO100_1_1_128.png") + ",")
