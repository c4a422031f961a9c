"""Addend loads issued ahead of their use, and the splices of an assembled tensor as the jobs of one launch.

The three-pass F(6x6) output transform with an addend (k_wino_out2<T, NTL, true>: the folded tconvs3.0 / tconvs2.0 of UtNet(64))
requests a thread's addend values before its first pass: which pixels a thread stores is a function of its index, its workgroup's
first tile and the geometry alone.  The frame loop fills a tile tensor (the output of a shared encoder level, the line images and
corner patches of the level below) with one k_splice_jobs launch of disjoint jobs; where level 2 is shared it copies of the tile's
own P2 only the four corner windows that the level-2 corner patches read (utnet_frame.hip: assemble_output).

Neither changes an arithmetic operation.  What can go wrong is an addend address taken for the wrong pixel or tile, a job that
reads the wrong band slot across a seam, a tile's index in its launch taken for its index in the frame, or a region left uncopied
that something reads.  tests/test_skip_fold.py already runs UtNet(16) at these geometries against float64 (every frame-loop test
runs the splice launches); what this file adds: UtNet(64) -- the three-pass addend transform of tconvs3.0 / tconvs2.0 -- with every
tile of the frame in one launch, with split-K and with whole tiles; bit equality of a launch of 5 and a launch of all tiles for
both nets; and the shared encoder against every tile's own over a band seam, where the job lists are longest.  Bars and helpers
are loaded from the tests that own them, not restated.  Every checked run follows a run on another frame through the same net
object and workspaces (_Loop): stale data is wrong data, not an earlier right answer.

Not here: a launch with two overlapping jobs, which nd_launch_splices refuses with ND_EINVAL -- the launcher is internal to the
library and no entry point of the C ABI reaches it with a job list of the caller's."""
import os

import pytest
import torch

from nind_denoise_amd import _lib


def _load(name):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py")
    spec = importlib.util.spec_from_file_location("_addend_ahead_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_SF = _load("test_skip_fold")
_SE, _ES = _SF._SE, _SF._ES
GEOM_A, NARROWEST = _SF.GEOM_A, _SF.NARROWEST
# per net: (weights seed, frame seed, bar vs float64, bar folded vs skip halves per tile) -- as tests/test_skip_fold.py uses them
NETS = {16: (9, 3, _SE.BAR_FRAME16, _SE.BAR_SHARED16), 64: (123, 24, _SE.BAR_TILE64, _SE.BAR_SHARED64)}
CASES = [(f, g) for f in (16, 64) for g in (GEOM_A, NARROWEST)]


def _id(v):
    return "{}x{}-{}-{}-{}".format(*v) if isinstance(v, tuple) else f"utnet{v}"


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref64():
    """float64 canvases, computed once per (net, geometry) and left unchanged."""
    from oracle import tiler as otiler
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    cache = {}

    def get(funit, geom, frame):
        if (funit, geom) not in cache:
            cs, ucs, ol = geom[2:]
            cache[funit, geom] = otiler.denoise_frame(frame, cs, ucs, ol, _SE._model64(_SE._sd64(funit, NETS[funit][0])), batch=8)
        return cache[funit, geom]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("funit,geom", CASES, ids=_id)
def test_every_tile_in_one_launch_vs_float64(dev, ref64, funit, geom):
    """All tiles of the frame in one launch (GEOM_A: 56, NARROWEST: 21 in one column), folds on, with split-K and with whole tiles
    only.  UtNet(64): the three-pass addend transform (tconvs3.0 / tconvs2.0); UtNet(16): all three folds in conv_w2d, here also
    with split_k = False."""
    seed, frame_seed, bar64, bar_off = NETS[funit]
    assert _SF._folds(geom, funit=funit) == 0b111
    lp = _SF._Loop(dev, funit, seed, geom, frame_seed)
    assert geom != GEOM_A or lp.total == 56
    ref = ref64(funit, geom, lp.frame)
    off = lp.run(lp.total, fold=False)
    for split_k in (True, False):
        on = lp.run(lp.total, split_k=split_k)
        e64, eoff = _SE._rel(on, ref), _SE._rel(on, off)
        print(f"UtNet({funit}) gain {_SE.VISIBLE_GAIN} {geom} batch {lp.total} split_k {split_k}: folded vs float64 {e64:.2e}, "
              f"vs skip halves per tile {eoff:.2e}")
        assert e64 <= bar64 and eoff <= bar_off, (split_k, e64, eoff)
        assert not torch.equal(on, off)                       # (the folds are on)
    lp.net._workspaces.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("funit,geom", CASES, ids=_id)
def test_launch_composition_leaves_the_bits(dev, funit, geom):
    """split_k = False (ND_FLAG_NO_SPLITK): a tile's bits do not depend on the launch it runs in.  An addend address that depends on
    where a tile falls in the launch, or a splice job that takes a tile's index in the launch for its index in the frame, breaks
    this."""
    seed, frame_seed = NETS[funit][:2]
    lp = _SF._Loop(dev, funit, seed, geom, frame_seed)
    few, all_ = lp.run(5, split_k=False), lp.run(lp.total, split_k=False)
    assert all_.abs().max().item() > 0
    assert torch.equal(few, all_)
    lp.net._workspaces.clear()


@pytest.mark.gpu
def test_splice_jobs_over_a_band_seam(dev):
    """Two bands, the last of one tile row: a launch that crosses the seam carries the line jobs of both bands, and its window jobs
    read each tile's band in its own slot.  The assembled encoder against every tile's own (share_encoder = False), and two launch
    compositions that cross the seam at different tiles."""
    geom = _ES.ONE_ROW_LAST_BAND
    p = _SE._plan(*geom)
    assert (p["D"], p["bands"], p["R"], p["rows"]) == (2, 2, 2, 3) and _SF._folds(geom) == 0b111
    per_band = p["R"] * p["cols"]
    for batch in (256, 100):   # some launch starts in band 0 and ends in band 1
        assert any(k * batch < per_band < (k + 1) * batch for k in range(p["cols"] * p["rows"] // batch + 1)), batch
    lp = _SF._Loop(dev, 64, 123, geom, 24)
    on, own = lp.run(256), lp.run(256, share=False)
    e = _SE._rel(on, own)
    print(f"UtNet(64) gain {_SE.VISIBLE_GAIN} {geom} batch 256: shared encoder vs every tile's own {e:.2e}")
    assert e <= _SE.BAR_SHARED64 and not torch.equal(on, own), e
    del on, own
    assert torch.equal(lp.run(256, split_k=False), lp.run(100, split_k=False))
    lp.net._workspaces.clear()
