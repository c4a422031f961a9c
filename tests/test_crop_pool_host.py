"""CPU tests of the crop pool (nind_denoise_amd/crop_pool.py, csrc/crop_batch.hip): the orientation map the kernel shares with
nd_crop_source, a numpy restatement of the whole transform against the fixture the reference's own DenoisingDataset.__getitem__
produced (tests/golden/make_golden_augment.py), the draw / epoch logic on CPU tensors, the directory scan, and the host
validation of explicit draws.  test_crop_pool.py runs the kernel against the same restatement and fixture."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib
from nind_denoise_amd.common.libs import imgcodec
from nind_denoise_amd.crop_pool import CropPool, pack_draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = 24


# ------------------------------------------------------------------ numpy restatement (shared with test_crop_pool.py)
def to_float(chw):
    """np_imgops.img_path_to_np_flt's conversion of [3, H, W] samples."""
    if chw.dtype == np.float32:
        return chw
    return chw.astype(np.single) / (255 if chw.dtype == np.uint8 else 65535)


def numpy_sample(clean, noisy, cs, x0, y0, nrot, flip1, flip2, mult=None):
    """One sample of the batch with numpy's own pad / slice / rot90 / flip on [3, H, W] integer or float sources: pad, crop,
    orientation and multiplier in the order of dataset_torch_3.py:231-276.  Returns (clean, noisy) float32 [3, cs, cs]."""
    out = []
    for img in (clean, noisy):
        img = to_float(img)
        _, h, w = img.shape
        py, px = max(0, (cs - h) // 2), max(0, (cs - w) // 2)
        img = np.pad(img, ((0, 0), (py, max(0, cs - h - py)), (px, max(0, cs - w - px))))
        img = img[:, y0:y0 + cs, x0:x0 + cs]
        img = np.rot90(img, nrot, (1, 2))
        if flip1:
            img = np.flip(img, 1)
        if flip2:
            img = np.flip(img, 2)
        assert img.shape == (3, cs, cs)
        out.append(np.ascontiguousarray(img))
    if mult is not None:
        m = np.float32(mult)
        out = [out[0] * m, np.clip(out[1] * m, np.float32(0), np.float32(1))]
    assert out[0].dtype == np.float32 and out[1].dtype == np.float32
    return out


def host_mult(xmax, u, mmin, mmax):
    """The exposure multiplier in float32, operation by operation."""
    f = np.float32
    b = f(mmax) if xmax == 0 else min(f(mmax), f(1) / f(xmax))
    return f(f(mmin) + f(f(b - f(mmin)) * f(u)))


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "augment.npz"))
    index = json.loads(bytes(z["index"]).decode())
    sources = json.loads(bytes(z["sources"]).decode())
    srcs = [(z[f"src{k}_clean"], z[f"src{k}_noisy"]) for k in range(len(sources))]        # HWC integer samples
    return index, sources, srcs, z["clean"], z["noisy"]


def case_mult(case):
    return None if case["mult"] is None else np.array([case["mult"]], dtype=np.int32).view(np.float32)[0]


# ------------------------------------------------------------------ the map
@pytest.mark.parametrize("cs", [6, 7])
def test_crop_source_is_rot90_then_two_flips(cs):
    lib = _lib.load()
    idx = np.arange(cs * cs).reshape(1, cs, cs)
    for nrot in range(4):
        for flips in range(4):
            want = np.rot90(idx, nrot, (1, 2))
            if flips & 1:
                want = np.flip(want, 1)
            if flips & 2:
                want = np.flip(want, 2)
            a, b = ctypes.c_int(), ctypes.c_int()
            for y in range(cs):
                for x in range(cs):
                    _lib.check(lib.nd_crop_source(cs, nrot, flips, y, x, a, b))
                    assert a.value * cs + b.value == want[0, y, x], (cs, nrot, flips, y, x)


def test_crop_source_rejects_bad_arguments():
    lib = _lib.load()
    a, b = ctypes.c_int(), ctypes.c_int()
    for args in [(0, 0, 0, 0, 0), (8, 4, 0, 0, 0), (8, -1, 0, 0, 0), (8, 0, 4, 0, 0), (8, 0, 0, 8, 0), (8, 0, 0, 0, -1)]:
        with pytest.raises(ValueError):
            _lib.check(lib.nd_crop_source(*args, a, b))
    with pytest.raises(ValueError):
        _lib.check(lib.nd_crop_source(8, 0, 0, 0, 0, None, b))


def test_crop_batch_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(64)       # never dereferenced: every call below fails its host checks
    ok = dict(pool=p, pool_bytes=64, images=p, n_images=1, draws=p, batch=2, cs=24, mmin=1.0, mmax=1.0, mult=None, xmax=None,
              mult_out=None, clean=p, noisy=p, stream=None)
    for bad in [dict(pool=None), dict(pool_bytes=0), dict(images=None), dict(draws=None), dict(clean=None), dict(noisy=None),
                dict(n_images=0), dict(batch=0), dict(batch=65536), dict(cs=0), dict(cs=16385), dict(mmin=0.5),
                dict(mmin=0.5, xmax=p), dict(mmin=2.0, mmax=1.0, xmax=p, mult_out=p)]:
        args = dict(ok, **bad)
        with pytest.raises(ValueError):
            _lib.check(lib.nd_crop_batch(*args.values()))


def test_header_and_bindings_declare_the_crop_entry_points():
    hdr = open(os.path.join(ROOT, "include", "nind_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", code))
    assert {"nd_crop_batch", "nd_crop_source"} <= declared
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    enum = dict(re.findall(r"(ND_SAMPLE_[A-Z0-9]+) = (\d+)", code))
    assert enum == {"ND_SAMPLE_U8": str(_lib.SAMPLE_U8), "ND_SAMPLE_U16": str(_lib.SAMPLE_U16), "ND_SAMPLE_F32": str(_lib.SAMPLE_F32)}
    assert _lib.load().nd_version() >= 113


# ------------------------------------------------------------------ the restatement against the reference's own outputs
def test_numpy_restatement_reproduces_the_reference_fixture(golden_dir):
    index, sources, srcs, clean, noisy = load_fixture(golden_dir)
    assert len(index) >= 25
    kinds = {(sources[c["src"]]["dtype"], c["kind"], c["cap_binds"]) for c in index}
    assert {("uint8", "crop", None), ("uint16", "crop", None), ("uint8", "pad", None), ("uint16", "pad", None)} <= kinds
    assert {b for _, _, b in kinds} == {None, True, False}
    shapes = {tuple(sources[c["src"]]["shape"]) for c in index if c["kind"] == "crop"}
    assert any(h == w for h, w in shapes) and any(h != w for h, w in shapes)
    for i, c in enumerate(index):
        sc, sn = (s.transpose(2, 0, 1) for s in srcs[c["src"]])
        got = numpy_sample(sc, sn, c["cs"], c["x0"], c["y0"], c["nrot"], c["flip1"], c["flip2"], case_mult(c))
        assert np.array_equal(got[0].view(np.int32), clean[i].view(np.int32)), c["id"]
        assert np.array_equal(got[1].view(np.int32), noisy[i].view(np.int32)), c["id"]
        if c["mult"] is not None:      # the recorded multiplier is the float32 formula on the recorded u and the crop's maximum
            unmult = numpy_sample(sc, sn, c["cs"], c["x0"], c["y0"], c["nrot"], c["flip1"], c["flip2"])[0]
            m = host_mult(unmult.max(), c["u"], c["exp_mult_min"], c["exp_mult_max"])
            assert abs(int(m.view(np.int32)) - c["mult"]) <= 1, c["id"]
            assert (float(np.float32(1) / unmult.max()) < c["exp_mult_max"]) == c["cap_binds"]


# ------------------------------------------------------------------ draws
def make_pool(n_groups=11, seed=5, cs=CS):
    rng = np.random.default_rng(1)
    pool = CropPool("cpu", seed=seed, cs=cs)
    sizes = [(40, 36), (20, 40), (24, 24), (33, 25)]
    for g in range(n_groups):
        h, w = sizes[g % len(sizes)]
        dtype = (np.uint8, np.uint16)[g % 2]
        pool.add_group([rng.integers(0, 255, (h, w, 3)).astype(dtype) for _ in range(1 + g % 3)],
                       [rng.integers(0, 255, (3, h, w)).astype(dtype) for _ in range(1 + g % 4)])
    return pool


def unpack(draws):
    t = draws.table
    assert t.dtype == torch.int32 and t.shape == (len(draws), 8)
    return t[:, :7].numpy().astype(np.int64), t[:, 7].contiguous().view(torch.float32).numpy()


def check_in_range(pool, draws):
    d, u = unpack(draws)
    groups = draws.groups.numpy()
    for row, uu, g in zip(d, u, groups):
        cl, no, h, w = pool.group(int(g))
        assert row[0] in cl and row[1] in no
        assert 0 <= row[2] <= max(w - draws.cs, 0) and 0 <= row[3] <= max(h - draws.cs, 0)
        if w <= draws.cs:
            assert row[2] == 0
        if h <= draws.cs:
            assert row[3] == 0
        assert 0 <= row[4] <= 3 and row[5] in (0, 1) and row[6] in (0, 1)
        assert 0.0 <= uu < 1.0
    pool.validate(draws.table, draws.cs)


def test_pool_layout_and_bytes():
    pool = make_pool()
    assert pool.n_groups == 11 and pool.n_images == sum(2 + g % 3 + g % 4 for g in range(11))
    want = 0
    for i in range(pool.n_images):
        img = pool.image(i)
        assert img.ndim == 3 and img.shape[0] == 3 and img.dtype in (np.uint8, np.uint16)
        want += (img.nbytes + 15) // 16 * 16
    assert pool.nbytes == want
    hwc = np.arange(5 * 4 * 3, dtype=np.uint8).reshape(5, 4, 3)
    g = pool.add_group([hwc], [hwc.transpose(2, 0, 1)])       # the same picture, once HWC and once CHW
    cl, no, h, w = pool.group(g)
    assert (h, w) == (5, 4) and np.array_equal(pool.image(cl[0]), pool.image(no[0])) and cl != no
    before = pool.nbytes
    g = pool.add_group([hwc], [hwc][:])                        # clean-clean: the same arrays are held once
    cl, no, _, _ = pool.group(g)
    assert cl == no and pool.nbytes == before + 64
    with pytest.raises(ValueError):
        pool.add_group([hwc], [np.zeros((6, 4, 3), np.uint8)])
    with pytest.raises(TypeError):
        pool.add_group([hwc.astype(np.float64)], [hwc])
    with pytest.raises(ValueError):
        pool.add_group([], [hwc])


def test_draw_values_are_in_range_and_cover_their_ranges():
    pool = make_pool()
    draws = pool.draw(400)
    check_in_range(pool, draws)
    d, u = unpack(draws)
    assert set(d[:, 4]) == {0, 1, 2, 3} and set(d[:, 5]) == {0, 1} and set(d[:, 6]) == {0, 1}
    assert set(draws.groups.tolist()) == set(range(pool.n_groups))
    g0 = d[draws.groups.numpy() % 4 == 0]                      # 40 x 36 groups at cs 24: offsets 0..12 and 0..16
    assert g0[:, 2].min() == 0 and g0[:, 2].max() == 12 and g0[:, 3].min() == 0 and g0[:, 3].max() == 16
    assert len(set(u.tolist())) > 390
    with pytest.raises(ValueError):
        CropPool("cpu").draw(4, cs=24)                         # no group
    with pytest.raises(ValueError):
        make_pool(cs=None).draw(4)                             # no crop size


def test_a_seed_reproduces_its_draws():
    a, b = make_pool(seed=9), make_pool(seed=9)
    ta = [a.draw(7).table for _ in range(3)] + [d.table for d in a.epoch(3)]
    tb = [b.draw(7).table for _ in range(3)] + [d.table for d in b.epoch(3)]
    assert len(ta) == len(tb) == 6 and all(torch.equal(x, y) for x, y in zip(ta, tb))
    a.seed(9)
    assert torch.equal(a.draw(7).table, ta[0])
    assert not torch.equal(make_pool(seed=10).draw(7).table, ta[0])


@pytest.mark.parametrize("n_groups, batch", [(11, 3), (12, 4), (5, 8)])
def test_epoch_is_a_permutation_in_full_batches(n_groups, batch):
    pool = make_pool(n_groups)
    batches = list(pool.epoch(batch))
    assert len(batches) == n_groups // batch
    seen = [g for d in batches for g in d.groups.tolist()]
    assert all(len(d) == batch for d in batches)
    assert len(seen) == len(set(seen)) == n_groups // batch * batch and set(seen) <= set(range(n_groups))
    for d in batches:
        check_in_range(pool, d)
    again = [g for d in pool.epoch(batch) for g in d.groups.tolist()]
    assert n_groups < 2 * batch or again != seen               # the next epoch is shuffled anew


@pytest.mark.parametrize("n_groups, batch, world", [(12, 2, 3), (13, 2, 4), (11, 3, 2)])
def test_ranks_take_disjoint_slices_of_one_epoch(n_groups, batch, world):
    single = [d for d in make_pool(n_groups, seed=3).epoch(batch)]
    per_rank = [list(make_pool(n_groups, seed=3).epoch(batch, rank=r, world=world)) for r in range(world)]
    steps = n_groups // batch // world
    assert all(len(p) == steps for p in per_rank)
    groups = [set(g for d in p for g in d.groups.tolist()) for p in per_rank]
    assert sum(len(s) for s in groups) == len(set().union(*groups)) == steps * world * batch
    for r, p in enumerate(per_rank):                           # batch k of the single-rank epoch is step k // world of rank k % world
        for s, d in enumerate(p):
            assert torch.equal(d.table, single[s * world + r].table)
    if n_groups // batch % world == 0:
        assert set().union(*groups) == set(g for d in single for g in d.groups.tolist())
    # every rank's generator has advanced alike: the next draws agree
    pools = [make_pool(n_groups, seed=3) for _ in range(world)]
    for r, p in enumerate(pools):
        list(p.epoch(batch, rank=r, world=world))
    nxt = [p.draw(4).table for p in pools]
    assert all(torch.equal(nxt[0], t) for t in nxt[1:])
    with pytest.raises(ValueError):
        list(make_pool().epoch(2, rank=2, world=2))


# ------------------------------------------------------------------ explicit draws
def test_explicit_draws_are_validated_on_the_host():
    pool = make_pool()
    cl, no, h, w = pool.group(0)                               # 40 x 36
    cl1, _, _, _ = pool.group(1)                               # 20 x 40
    good = dict(clean=[cl[0]], noisy=[no[0]], x0=[12], y0=[16], nrot=[3], flip1=[1], flip2=[0], u=[0.5])
    pool.validate(pack_draws(**good), CS)
    for bad in [dict(clean=[-1]), dict(clean=[pool.n_images]), dict(noisy=[pool.n_images]), dict(noisy=[-7]), dict(x0=[13]),
                dict(x0=[-1]), dict(y0=[17]), dict(y0=[-1]), dict(nrot=[4]), dict(nrot=[-1]), dict(flip1=[2]), dict(flip2=[-1]),
                dict(u=[1.0]), dict(u=[-0.25]), dict(u=[float("nan")]), dict(clean=[cl1[0]])]:
        with pytest.raises(ValueError):
            pool.validate(pack_draws(**dict(good, **bad)), CS)
        with pytest.raises(ValueError):                        # batch() checks before it uploads or launches anything
            pool.batch(pack_draws(**dict(good, **bad)), CS)
    table = pack_draws(**good)
    for wrong in [table[:, :7], table[0], table.to(torch.int64), table[:0], table.numpy().astype(np.float32)]:
        with pytest.raises(ValueError):
            pool.validate(wrong, CS)
    with pytest.raises(ValueError):
        pool.validate(pack_draws(**dict(good, x0=[12], y0=[16])), 30)      # valid at cs 24, outside at cs 30
    with pytest.raises(ValueError):
        make_pool().batch(pool.draw(2))                        # draws of another pool
    with pytest.raises(ValueError):
        pool.batch(pool.draw(2), cs=CS + 1)
    with pytest.raises(RuntimeError):
        pool.batch(pool.draw(2))                               # a CPU pool makes no batch: no fallback


# ------------------------------------------------------------------ directory scan
def write_tree(root, sets, crops=("0_0", "16_0"), shape=(12, 10), seed=0):
    rng = np.random.default_rng(seed)
    files = {}
    for aset, isos in sets.items():
        for iso, dtype in isos.items():
            os.makedirs(os.path.join(root, aset, iso))
            for crop in crops:
                img = rng.integers(0, np.iinfo(dtype).max, shape + (3,)).astype(dtype)
                path = os.path.join(root, aset, iso, f"NIND_{aset}_{iso}_{crop}_16.png")
                imgcodec.write_png(path, img)
                files[path] = img
    return files


def test_from_directories_groups_base_and_noisy_isos(tmp_path):
    root = str(tmp_path / "NIND_24_16")
    sets = {"bike": {"ISO200": np.uint8, "ISO200-1": np.uint8, "ISO800": np.uint8, "ISO6400": np.uint8, "ISOH1": np.uint8},
            "tree": {"ISO100": np.uint16, "ISO3200": np.uint16},
            "tree-test": {"ISO100": np.uint8, "ISO400": np.uint8},
            "stairs": {"GT": np.uint8, "ISO400": np.uint8}}
    files = write_tree(root, sets)
    pool = CropPool.from_directories([root], device="cpu")
    assert pool.cs == 24 and pool.n_groups == 8
    by_set = {}
    for g, (datadir, aset, animg, bisos, isos) in enumerate(pool.sets):
        by_set.setdefault(aset, []).append(g)
        cl, no, h, w = pool.group(g)
        assert (h, w) == (12, 10) and len(cl) == len(bisos) and len(no) == len(isos)
        crop = animg.split(isos[0] + "_")[1]
        for ids, names in ((cl, bisos), (no, isos)):
            for i, iso in zip(ids, names):
                want = files[os.path.join(root, aset, iso, f"NIND_{aset}_{iso}_{crop}")]
                assert np.array_equal(pool.image(i), want.transpose(2, 0, 1)) and pool.image(i).dtype == want.dtype
    assert {k: len(v) for k, v in by_set.items()} == {"bike": 2, "tree": 2, "tree-test": 2, "stairs": 2}
    bike = pool.sets[by_set["bike"][0]]
    assert set(bike[3]) == {"ISO200", "ISO200-1"} and bike[4] == ("ISO800", "ISO6400", "ISOH1")
    assert pool.sets[by_set["stairs"][0]][3:] == (("GT",), ("ISO400",))
    assert pool.nbytes == sum((pool.image(i).nbytes + 15) // 16 * 16 for i in range(pool.n_images))

    sub = CropPool.from_directories([root], test_reserve=["tree"], device="cpu")             # substring: tree and tree-test
    assert {s[1] for s in sub.sets} == {"bike", "stairs"}
    exact = CropPool.from_directories([root], test_reserve=["tree"], exact_reserve=True, device="cpu")
    assert {s[1] for s in exact.sets} == {"bike", "stairs", "tree-test"}
    assert CropPool.from_directories([root], min_crop_size=11, device="cpu").n_groups == 0     # 12 x 10 crops
    assert CropPool.from_directories([root, root], min_crop_size=10, device="cpu", cs=8).n_groups == 16


def test_from_directories_names_the_file_it_cannot_read(tmp_path):
    root = str(tmp_path / "crops")
    write_tree(root, {"bike": {"ISO200": np.uint8, "ISO800": np.uint8}}, crops=("0_0",))
    bad = os.path.join(root, "bike", "ISO800", "NIND_bike_ISO800_0_0_16.png")
    with open(bad, "wb") as f:
        f.write(b"not a png")
    with pytest.raises(ValueError, match=re.escape(bad)):
        CropPool.from_directories(root, device="cpu")
    os.remove(bad)                                             # the crop list comes from the first noisy ISO: no file, no group
    assert CropPool.from_directories(root, device="cpu").n_groups == 0
    write_tree(root, {"tree": {"ISO100": np.uint8, "ISO400": np.uint8}}, crops=("0_0",))
    gone = os.path.join(root, "tree", "ISO100", "NIND_tree_ISO100_0_0_16.png")
    os.remove(gone)                                            # a crop that its base ISO lacks
    with pytest.raises(FileNotFoundError, match=re.escape(gone)):
        CropPool.from_directories(root, device="cpu")
