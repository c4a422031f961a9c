"""The fused frame loop reads the shared encoder's skip halves in place and launches `batch` tiles across band seams.

tconvs4.0 / tconvs3.0 take the skip half of CAT4 / CAT3 from the band tensor (a second input source of conv_w2d and of the F(6x6)
input transform) instead of from a per-tile copy, and the band tensors the launches read live in two slots so that a launch may hold
tiles of two bands.  Checked here at visible weights against the float64 oracle and the per-tile encoder, with the bars
test_shared_encoder.py already holds the loop to on the same frames and weights (loaded from it, not restated).  Every checked frame
follows a frame of another seed through the same net object and workspaces: a per-tile skip half nobody writes any more, or a band
slot left over from another band, is then wrong data and not an earlier right answer."""
import os

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib, synth


def _shared_encoder_tests():
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_shared_encoder.py")
    spec = importlib.util.spec_from_file_location("_shared_encoder_bars", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_SE = _shared_encoder_tests()
BAR_FRAME16, BAR_SHARED16, BAR_TILE64, BAR_SHARED64 = _SE.BAR_FRAME16, _SE.BAR_SHARED16, _SE.BAR_TILE64, _SE.BAR_SHARED64


@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


class _Loop:
    """denoise_frame of `frame` through one net object, every run preceded by the same run on another frame."""

    def __init__(self, dev, funit, seed, geom, frame_seed):
        from nind_denoise_amd import pipeline
        self.pipeline, self.geom = pipeline, geom
        W, H = geom[:2]
        self.net = _SE._net_visible(dev, funit, seed)
        self.frame = synth.make_frame(W, H, seed=frame_seed)
        self.img = torch.from_numpy(self.frame).to(dev)
        self.other = torch.from_numpy(synth.make_frame(W, H, seed=frame_seed + 100)).to(dev)
        self.total = pipeline.tile_count(*geom)

    def run(self, batch, ranges=None, split_k=True, share=True, fresh=False):
        W, H, cs, ucs, ol = self.geom
        self.net.split_k, self.net.share_encoder = split_k, share
        if fresh:
            self.net._workspaces.clear()   # (frame workspaces of several GB per batch size)
        ranges = ranges or ((0, self.total),)
        for lo, hi in ranges:
            self.pipeline.denoise_frame(self.net, self.other, cs, ucs, ol, batch=batch, tile_range=(lo, hi))
        cv = torch.zeros_like(self.img)
        for lo, hi in ranges:
            self.pipeline.denoise_frame(self.net, self.img, cs, ucs, ol, batch=batch, tile_range=(lo, hi), canvas=cv)
        self.net.split_k, self.net.share_encoder = True, True
        return cv


@pytest.mark.gpu
@pytest.mark.parametrize("geom", _SE.SINGLE_BAND, ids=lambda g: "{}x{}-{}-{}-{}".format(*g))
def test_single_band_in_place_vs_float64(dev, geom):
    # UtNet(16): both in-place steps run in conv_w2d; the last tile row and column put the window at the band's bottom and right edge
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    p = _SE._plan(W, H, cs, ucs, ol, funit=16)
    assert (p["D"], p["bands"]) == (2, 1)
    lp = _Loop(dev, 16, 9, geom, 3)
    cols, total = p["cols"], lp.total
    assert total == cols * p["rows"] and cols >= 2
    ref = otiler.denoise_frame(lp.frame, cs, ucs, ol, _SE._model64(_SE._sd64(16, 9)), batch=16)
    tiled = lp.run(5, share=False)
    e_ti = _SE._rel(tiled, ref)
    print(f"UtNet(16) gain {_SE.VISIBLE_GAIN} {geom}: per-tile encoder vs float64 {e_ti:.2e}")
    assert e_ti <= BAR_FRAME16, e_ti
    mid = cols + cols // 2                                   # ranges that start and end mid-row
    cases = [("batch 1", 1, None), ("batch < cols", cols - 1, None), ("batch = all tiles", total, None),
             ("ranges", cols - 1, ((0, 1), (1, mid), (mid, total - 1), (total - 1, total)))]
    for name, batch, ranges in cases:
        got = lp.run(batch, ranges)
        e64, est = _SE._rel(got, ref), _SE._rel(got, tiled)
        print(f"  {name}: vs float64 {e64:.2e}, vs per-tile encoder {est:.2e}")
        assert e64 <= BAR_FRAME16 and est <= BAR_SHARED16, (name, e64, est)


# batches per multi-band frame: one that puts a launch over a seam (256 at 28 x 16 ... tiles of 264) and, at the 504-pixel tiling
# (28 tiles per band), two that would span three bands and must be cut at the second seam
_BATCHES = {264: (256,), 504: (64, 126)}


@pytest.mark.gpu
@pytest.mark.parametrize("geom,bands", _SE.MULTI_BAND, ids=["{}x{}-{}-{}-{}".format(*g) for g, _ in _SE.MULTI_BAND])
def test_multi_band_in_place_across_seams(dev, geom, bands):
    # UtNet(64): tconvs3.0 reads its skip half through the F(6x6) input transform, tconvs4.0 through conv_w2d
    from oracle import tiler as otiler
    W, H, cs, ucs, ol = geom
    p = _SE._plan(W, H, cs, ucs, ol)
    assert (p["D"], p["bands"], p["R"]) == (2, *bands)
    cols, R = p["cols"], p["R"]
    per_band = R * cols
    lp = _Loop(dev, 64, 123, geom, 24)
    batches = _BATCHES[cs]
    assert all(b <= lp.total for b in batches)
    if cs == 504:
        assert per_band == 28 and all(b > 2 * per_band for b in batches)    # a launch of `batch` would reach a third band
    else:
        assert any((k * 256) // per_band != (k * 256 + 255) // per_band for k in range(lp.total // 256))   # a launch over a seam

    # whole canvas against the per-tile encoder; with split-K off, equal bit for bit across the batches and batch 1
    tiled = lp.run(batches[0], share=False, fresh=True)
    for batch in batches:
        got = lp.run(batch, fresh=True)
        est = _SE._rel(got, tiled)
        print(f"UtNet(64) gain {_SE.VISIBLE_GAIN} {geom} batch {batch}: canvas shared vs per-tile encoder {est:.2e}")
        assert est <= BAR_SHARED64, (batch, est)
        del got
    # a range that begins in the middle of a band's last row and runs over the seam into the next band
    lo = (R - 1) * cols + cols // 2
    rng = ((lo, min(lp.total, lo + batches[0] + 3)),)
    assert rng[0][0] < per_band < rng[0][1]
    est = _SE._rel(lp.run(batches[0], rng), lp.run(batches[0], rng, share=False))
    print(f"  tiles {rng[0]}: shared vs per-tile encoder {est:.2e}")
    assert est <= BAR_SHARED64, est
    del tiled
    whole = lp.run(1, split_k=False, fresh=True)
    part = lp.run(1, rng, split_k=False)
    for batch in batches:
        assert torch.equal(whole, lp.run(batch, split_k=False, fresh=True)), batch
        assert torch.equal(part, lp.run(batch, rng, split_k=False)), batch
    del whole, part

    # the tiles at the band seams, each alone on a zero canvas, against the oracle's stitch of its float64 output
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    picks = [i for i in _SE._band_samples(p) if any(i // cols in (b * R - 1, b * R) for b in range(1, p["bands"]))]
    assert len(picks) >= 4 * (p["bands"] - 1)     # (a one-row last band puts the bottom-edge samples on a seam row too)
    model_fn = _SE._model64(_SE._sd64(64, 123))
    errs = []
    for i in picks:
        y = model_fn(otiler.gather_tile(lp.frame, grid, i)[None])[0]
        cv = lp.run(batches[0], ((i, i + 1),))
        _, _, ud, (ax, ay) = grid.geom(i)
        ref = otiler.make_seamless_edges(np.array(y[:, ud[1]:ud[3], ud[0]:ud[2]], dtype=np.float32), ax, ay, grid)
        h, w = ref.shape[1:]
        got = cv[:, ay:ay + h, ax:ax + w].clone()
        cv[:, ay:ay + h, ax:ax + w] = 0
        assert not cv.any(), i                    # nothing outside the tile's useful region
        errs.append(_SE._rel(got, ref))
    lp.net._workspaces.clear()
    worst = max(errs)
    print(f"  seam tiles {picks} vs float64 worst {worst:.2e} (tile {picks[errs.index(worst)]})")
    assert worst <= BAR_TILE64, worst
