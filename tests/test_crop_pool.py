"""The crop-pool kernel (csrc/crop_batch.hip through crop_pool.CropPool.batch) on the GPU, bit for bit: against the fixture the
reference's own DenoisingDataset.__getitem__ produced (tests/golden/augment.npz) and against the numpy restatement that
test_crop_pool_host.py ties to that fixture.  Every comparison is on the float32 words: the transform is copies, one correctly
rounded division and one multiplication, so there is no tolerance to choose.  The one exception is the multiplier the device
draws itself, m = min + (b - min) * u: the compiler may contract the multiply-add, so m may differ from the operation-by-operation
float32 value by one unit in the last place; the batch is then compared using the device's m."""
import itertools

import numpy as np
import pytest
import torch

from nind_denoise_amd import synth
from nind_denoise_amd.crop_pool import CropPool, pack_draws
from test_crop_pool_host import case_mult, host_mult, load_fixture, numpy_sample

pytestmark = pytest.mark.gpu
CS = 24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    from nind_denoise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def words(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def same_words(got, want):
    return np.array_equal(words(got) if torch.is_tensor(got) else got.view(np.int32), np.ascontiguousarray(want).view(np.int32))


def sweep_sources():
    """One 40 x 36 u8 pair, one 33 x 40 u16 pair and one 20 x 40 float32 pair (a padded side at cs 24; its noisy image leaves [0, 1]
    and its clean image has negative samples), as [3, H, W]."""
    rng = np.random.default_rng(11)
    u8 = [rng.integers(0, 256, (3, 40, 36)).astype(np.uint8) for _ in range(2)]
    u16 = [rng.integers(0, 65536, (3, 33, 40)).astype(np.uint16) for _ in range(2)]
    f32 = [rng.uniform(-0.2, 0.9, (3, 20, 40)).astype(np.float32), rng.uniform(-0.3, 1.4, (3, 20, 40)).astype(np.float32)]
    return [u8, u16, f32]


@pytest.fixture(scope="module")
def sweep(dev):
    """The pool of the three sweep pairs, every (pair, orientation, corner offset) draw, and the numpy restatement of each -- computed
    once and shared, never modified."""
    srcs = sweep_sources()
    pool = CropPool(dev, seed=1, cs=CS)
    for clean, noisy in srcs:
        pool.add_group([clean], [noisy])
    rows = []
    for g, (clean, _) in enumerate(srcs):
        cl, no, h, w = pool.group(g)
        for nrot, f1, f2, x0, y0 in itertools.product(range(4), (0, 1), (0, 1), (0, max(w - CS, 0)), (0, max(h - CS, 0))):
            rows.append((g, cl[0], no[0], x0, y0, nrot, f1, f2))
    rows = sorted(set(rows))
    want = [numpy_sample(srcs[r[0]][0], srcs[r[0]][1], CS, *r[3:]) for r in rows]
    return pool, srcs, rows, want


def table_of(rows, u=0.5):
    cols = list(zip(*rows))
    return pack_draws(*cols[1:8], [u] * len(rows))


def test_fixture_parity_with_the_reference(dev, golden_dir):
    index, sources, srcs, clean, noisy = load_fixture(golden_dir)
    pool = CropPool(dev, cs=CS)
    ids = [pool.group(pool.add_group([c], [n]))[:2] for c, n in srcs]          # HWC arrays, as a file decodes
    for with_mult in (False, True):
        sel = [i for i, c in enumerate(index) if (c["mult"] is not None) == with_mult]
        assert len(sel) >= 8
        cases = [index[i] for i in sel]
        table = pack_draws([ids[c["src"]][0][0] for c in cases], [ids[c["src"]][1][0] for c in cases], [c["x0"] for c in cases],
                           [c["y0"] for c in cases], [c["nrot"] for c in cases], [c["flip1"] for c in cases],
                           [c["flip2"] for c in cases], [0.0] * len(cases))
        mult = torch.tensor([case_mult(c) for c in cases], dtype=torch.float32) if with_mult else None
        got_c, got_n = pool.batch(table, CS, mult=mult)
        assert got_c.shape == (len(sel), 3, CS, CS) and got_c.dtype == torch.float32 and got_c.device == dev
        gc, gn = words(got_c), words(got_n)
        for k, i in enumerate(sel):
            assert np.array_equal(gc[k], clean[i].view(np.int32)), index[i]["id"]
            assert np.array_equal(gn[k], noisy[i].view(np.int32)), index[i]["id"]


def test_every_orientation_and_corner_offset(sweep):
    pool, srcs, rows, want = sweep
    assert len(rows) == 16 * (4 + 4 + 2)                      # the padded pair has one free offset
    assert {r[5:8] for r in rows} == set(itertools.product(range(4), (0, 1), (0, 1)))
    for at in range(0, len(rows), 5):                          # batches of 5 (the last one shorter)
        part = rows[at:at + 5]
        got_c, got_n = pool.batch(table_of(part), CS)
        for k in range(len(part)):
            assert same_words(got_c[k], want[at + k][0]), part[k]
            assert same_words(got_n[k], want[at + k][1]), part[k]


def test_given_multiplier_is_applied_and_only_noisy_is_clipped(sweep):
    pool, srcs, rows, _ = sweep
    part = rows[3::7]
    mult = np.linspace(0.4, 2.6, len(part)).astype(np.float32)
    got_c, got_n = pool.batch(table_of(part), CS, mult=torch.from_numpy(mult))
    for k, r in enumerate(part):
        want = numpy_sample(srcs[r[0]][0], srcs[r[0]][1], CS, *r[3:], mult=mult[k])
        assert same_words(got_c[k], want[0]) and same_words(got_n[k], want[1]), r
    assert got_c.max().item() > 1.0 and got_c.min().item() < 0.0           # clean is left unclipped
    assert got_n.max().item() == 1.0 and got_n.min().item() == 0.0
    # exp_mult_min == 1 and no mult: nothing is multiplied and nothing is clipped
    plain_c, plain_n = pool.batch(table_of(part), CS, exp_mult_min=1, exp_mult_max=3)
    assert plain_n.max().item() > 1.0 and pool.last_mult is None


def test_device_drawn_multiplier(dev):
    rng = np.random.default_rng(5)
    bright = [rng.integers(0, 256, (3, 40, 36)).astype(np.uint8) for _ in range(2)]
    dim16 = [rng.integers(0, 30000, (3, 33, 40)).astype(np.uint16) for _ in range(2)]       # 1 / xmax > 2: the cap does not bind
    black = [np.zeros((3, 30, 30), np.uint8), rng.integers(0, 256, (3, 30, 30)).astype(np.uint8)]
    padded = [rng.uniform(0.0, 0.7, (3, 20, 40)).astype(np.float32) for _ in range(2)]
    negative = [-rng.uniform(0.1, 0.7, (3, 20, 24)).astype(np.float32) for _ in range(2)]   # padded: its maximum is the zero border
    srcs = [bright, dim16, black, padded, negative]
    pool = CropPool(dev, cs=CS)
    for c, n in srcs:
        pool.add_group([c], [n])
    mmin, mmax = 0.8, 1.3
    rows, us = [], []
    for g in range(len(srcs)):
        cl, no, h, w = pool.group(g)
        for k, (x0, y0) in enumerate([(0, 0), (max(w - CS, 0), max(h - CS, 0)), (max(w - CS, 0) // 2, 0)]):
            rows.append((g, cl[0], no[0], x0, y0, (g + k) % 4, k & 1, (g >> 1) & 1))
            us.append([0.0, 0.37, 0.99999994][k])
    cols = list(zip(*rows))
    got_c, got_n = pool.batch(pack_draws(*cols[1:8], us), CS, exp_mult_min=mmin, exp_mult_max=mmax)
    xmax, m = pool.last_xmax.cpu().numpy(), pool.last_mult.cpu().numpy()
    binds = set()
    for k, r in enumerate(rows):
        plain = numpy_sample(srcs[r[0]][0], srcs[r[0]][1], CS, *r[3:])
        want_max = plain[0].max()
        assert xmax[k].view(np.int32) == want_max.view(np.int32), (r, xmax[k], want_max)
        want_m = host_mult(want_max, us[k], mmin, mmax)
        assert abs(int(m[k].view(np.int32)) - int(want_m.view(np.int32))) <= 1, (r, m[k], want_m)
        binds.add(bool(want_max > 0 and np.float32(1) / want_max < np.float32(mmax)))
        want = numpy_sample(srcs[r[0]][0], srcs[r[0]][1], CS, *r[3:], mult=m[k])
        assert same_words(got_c[k], want[0]) and same_words(got_n[k], want[1]), r
    assert binds == {True, False}
    assert xmax[6] == 0 and abs(m[7] - (mmin + (mmax - mmin) * 0.37)) < 1e-6       # a black clean crop takes exp_mult_max as its cap
    assert got_n.max().item() <= 1.0 and got_n.min().item() >= 0.0
    assert (m >= np.float32(mmin)).all() and (m <= np.float32(mmax)).all()


def test_one_seed_gives_the_same_batches(dev, sweep):
    _, srcs, _, _ = sweep
    out = []
    for _ in range(2):
        pool = CropPool(dev, seed=77, cs=CS)
        for clean, noisy in srcs:
            pool.add_group([clean, clean[:, ::-1].copy()], [noisy, noisy[:, :, ::-1].copy(), noisy])
        batches = [pool.batch(pool.draw(5), exp_mult_min=0.7, exp_mult_max=1.4) for _ in range(2)]
        batches += [pool.batch(d) for d in pool.epoch(3)]
        out.append([words(t) for pair in batches for t in pair])
    assert len(out[0]) == 6 and all(np.array_equal(a, b) for a, b in zip(*out))
    assert not np.array_equal(out[0][0], out[0][2])            # and the second batch is not the first


def test_a_second_batch_leaves_nothing_of_the_first(dev, sweep):
    pool, srcs, rows, want = sweep
    first = [r for r in rows if r[0] == 0][:5]                 # five crops of the 40 x 36 pair: no pixel is padding
    second = [r for r in rows if r[0] == 2][3:8]               # five of the 20 x 40 pair: two zero rows above and below
    clean = torch.full((5, 3, CS, CS), 7.0, device=dev)
    noisy = torch.full((5, 3, CS, CS), -7.0, device=dev)
    got = pool.batch(table_of(first), CS, out=(clean, noisy))
    assert got[0] is clean and got[1] is noisy and clean.min().item() >= 0 and clean.max().item() <= 1
    pool.batch(table_of(second), CS, out=(clean, noisy))
    for k, r in enumerate(second):
        w = want[rows.index(r)]
        assert same_words(clean[k], w[0]) and same_words(noisy[k], w[1]), r
        zeros = (w[0] == 0).all(axis=0)
        assert zeros.sum() == 4 * CS and (words(clean[k])[:, zeros] == 0).all() and (words(noisy[k])[:, zeros] == 0).all()


def test_reads_outside_an_image_or_the_table_are_zero(dev, sweep):
    """The guards of the kernel, through the C entry point (CropPool.batch refuses such draws on the host): a window that hangs over the
    image's edge reads zeros there, and an image index outside the table gives a zero sample."""
    from nind_denoise_amd import _lib
    pool, srcs, _, _ = sweep
    buf, images = pool.device_buffers()
    cl, no, h, w = pool.group(1)                               # 33 x 40 u16, in the middle of the pool buffer
    table = pack_draws([cl[0], cl[0], pool.n_images, cl[0]], [no[0], no[0], no[0], -1], [w - CS + 5, 0, 0, 3], [0, -3, 0, 2],
                       [0, 0, 0, 0], [0] * 4, [0] * 4, [0.0] * 4).to(dev)
    clean = torch.full((4, 3, CS, CS), 7.0, device=dev)
    noisy = torch.full((4, 3, CS, CS), 7.0, device=dev)
    _lib.check(_lib.load().nd_crop_batch(buf.data_ptr(), buf.numel(), images.data_ptr(), images.shape[0],
                                         table.data_ptr(), 4, CS, 1.0, 1.0, None, None, None, clean.data_ptr(), noisy.data_ptr(),
                                         _lib.stream_ptr(dev)), "nd_crop_batch")
    c, n = clean.cpu().numpy(), noisy.cpu().numpy()
    src_c, src_n = (a.astype(np.float32) / 65535 for a in srcs[1])
    assert (c[0][:, :, CS - 5:] == 0).all() and np.array_equal(c[0][:, :, :CS - 5], src_c[:, :CS, w - CS + 5:])
    assert (n[1][:, :3] == 0).all() and np.array_equal(n[1][:, 3:], src_n[:, :CS - 3, :CS])
    assert (c[2] == 0).all() and (n[2] == 0).all()             # no clean image: nothing to pair the noisy one with
    assert (n[3] == 0).all() and np.array_equal(c[3], src_c[:, 2:2 + CS, 3:3 + CS])


def test_trainer_takes_pool_batches(dev):
    """One UtNetTrainer(funit=8).learn at cs 104 fed straight from a pool equals, as words, the step fed with clones of the same two
    tensors: the batches are ordinary contiguous float32 tensors on the trainer's stream."""
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    rng = np.random.default_rng(3)
    pool = CropPool(dev, seed=4, cs=104)
    for g in range(3):
        clean = rng.integers(0, 256, (120 + 8 * g, 130, 3)).astype(np.uint8)
        noisy = np.clip(clean.astype(np.int32) + rng.integers(-20, 21, clean.shape), 0, 255).astype(np.uint8)
        pool.add_group([clean], [noisy])
    res = []
    for cloned in (False, True):
        pool.seed(4)
        net = UtNet(funit=8)
        net.load_state_dict(synth.make_utnet_state_dict(funit=8, seed=31, gain=1.8))
        tr = UtNetTrainer(net, device=dev, weights={"L1": 0.2, "MSE": 0.8})
        clean, noisy = pool.batch(pool.draw(2), exp_mult_min=0.8, exp_mult_max=1.2)          # batch[0] is the clean one
        assert clean.shape == (2, 3, 104, 104) and not torch.equal(clean, noisy)
        loss = tr.learn(noisy.clone(), clean.clone()) if cloned else tr.learn(noisy, clean)
        torch.cuda.synchronize()
        res.append((words(loss), words(tr.flat), words(clean), words(noisy)))
    assert all(np.array_equal(a, b) for a, b in zip(*res))
    assert np.isfinite(res[0][0].view(np.float32)).all() and res[0][0].view(np.float32)[0] > 0
