"""The skip halves of tconvs4.0 / tconvs3.0 / tconvs2.0 folded out of the per-tile sums of the fused frame loop.

The first layer of a decoder level is a ConvTranspose2d(3) on cat([up, skip]) and linear in its input channels:
act(b + W_up * up + W_skip * skip) = act(W_up * up + P) with P = W_skip * skip + b.  Where the skip is a band tensor of the shared
encoder, P is computed once per band and the per-tile layer takes its window of P as the addend of its epilogue (utnet_frame.hip:
plan_folds, launch_skip_fold; ConvDesc::add; UtNet.fold_skips = False / ND_FLAG_TILE_SKIPS keeps the skip halves per tile).

CPU: the identity in float64 against the oracle network, with a gate proving that the bars reused from tests/test_shared_encoder.py
see an addend window read one pixel off; the host query.  GPU: the conv_w2d addend path on every folded layer (UtNet(16)), the
three-pass F(6x6) addend path (UtNet(64): tconvs3.0 / tconvs2.0; tconvs4.0 in conv_w2d), a launch over a band seam, and the geometries and switches under which nothing or less folds.  Bars and helpers are
loaded from the tests that own them, not restated.  Every checked GPU run follows a run on another frame through the same net object
and workspaces: a stale P, or a stale per-tile skip, is then wrong data and not an earlier right answer."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth


def _load(name):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py")
    spec = importlib.util.spec_from_file_location("_skip_fold_" + name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_SE = _load("test_shared_encoder")
_ES = _load("test_edge_strips")
BAR_FRAME16, BAR_SHARED16, BAR_TILE64, BAR_SHARED64 = _SE.BAR_FRAME16, _SE.BAR_SHARED16, _SE.BAR_TILE64, _SE.BAR_SHARED64

# (W, H, cs, ucs, ol): crop 32, 8 | S, so that all three encoder levels are shared; the second has pad 40 > stride 32
GEOM_A, GEOM_B, GEOM_C = (333, 290, 120, 56, 16), (300, 170, 136, 56, 24), (176, 176, 120, 56, 16)
NARROWEST = (120, 290, 120, 56, 16)
LEVEL2_PER_TILE = (333, 290, 120, 88, 16)     # crop 16: tconvs2.0 reads line 0 of its skip, level 2 stays per tile
NO_BAND = (333, 290, 120, 88, 18)             # S = 70: D = 0


def _folds(geom, funit=64, dtype=0, flags=0):
    out = ctypes.c_int(-1)
    _lib.check(_lib.load().nd_utnet_frame_folds(funit, dtype, flags, *geom, ctypes.byref(out)), "nd_utnet_frame_folds")
    return out.value


# ---------------------------------------------------------------------------- CPU: the identity

def _folded_forward(sd, xp, band=None, org=None, shift=(0, 0), fold=(True, True, True)):
    """UtNet in float64 on the reflect-padded tile input xp.  band: the encoder skips of the band window (level 0, 1, 2); where
    fold[k] is set, tconvs(4 - k).0 runs on its up-sampled half alone and adds its window of P = W_skip * band skip + b, which starts
    at band pixel org >> k (+ shift: the window read off its place)."""
    from oracle import networks as onet

    def act(k, t):
        return onet._act(sd, k, t, "PReLU")

    def enc(n, t):
        t = act(f"{n}.1", F.conv2d(t, sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]))
        return act(f"{n}.3", F.conv2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    def up(n, t):
        return F.conv_transpose2d(t, sd[f"{n}.weight"], sd[f"{n}.bias"], stride=2)

    def dec(n, u, skip, part=None, o=None):
        w, b = sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]
        if part is None:
            t = F.conv_transpose2d(torch.cat([u, skip], 1), w, b)
        else:
            t = F.conv_transpose2d(u, w[:u.shape[1]])
            h, wd = t.shape[2:]
            t = t + part[:, :, o[0] + shift[0]:o[0] + shift[0] + h, o[1] + shift[1]:o[1] + shift[1] + wd]
        t = act(f"{n}.1", t)
        return act(f"{n}.3", F.conv_transpose2d(t, sd[f"{n}.2.weight"], sd[f"{n}.2.bias"]))

    l1 = enc("convs1", xp)
    l2 = enc("convs2", F.max_pool2d(l1, 2))
    l3 = enc("convs3", F.max_pool2d(l2, 2))
    l4 = enc("convs4", F.max_pool2d(l3, 2))
    b = F.max_pool2d(l4, 2)
    b = act("bottom.1", F.conv2d(b, sd["bottom.0.weight"], sd["bottom.0.bias"]))
    b = act("bottom.3", F.conv_transpose2d(b, sd["bottom.2.weight"], sd["bottom.2.bias"]))
    parts, orgs = [None] * 3, [None] * 3
    if band is not None:
        for k, n in enumerate(("tconvs4", "tconvs3", "tconvs2")):
            if not fold[k]:
                continue
            w, bb = sd[f"{n}.0.weight"], sd[f"{n}.0.bias"]
            cu = w.shape[0] - band[k].shape[1]
            # (one pixel of margin around P, so that a shifted window stays inside it)
            parts[k] = F.pad(F.conv_transpose2d(band[k], w[cu:], bb), (1, 1, 1, 1))
            orgs[k] = ((org[0] >> k) + 1, (org[1] >> k) + 1)
    t = dec("tconvs1", up("up1", b), l4)
    t = dec("tconvs2", up("up2", t), l3, parts[2], orgs[2])
    t = dec("tconvs3", up("up3", t), l2, parts[1], orgs[1])
    t = dec("tconvs4", up("up4", t), l1, parts[0], orgs[0])
    return F.conv2d(t, sd["tconvs4.4.weight"], sd["tconvs4.4.bias"])[:, :, 2:-2, 2:-2]


@pytest.mark.parametrize("funit,seed,geom,frame_seed,bars", [
    (16, 9, GEOM_A, 3, (BAR_FRAME16, BAR_SHARED16)), (16, 9, GEOM_B, 3, (BAR_FRAME16, BAR_SHARED16)),
    (64, 123, GEOM_C, 24, (BAR_TILE64, BAR_SHARED64))], ids=["16-333x290", "16-300x170", "64-176x176"])
def test_fold_is_the_network_and_the_bars_see_a_shifted_addend(funit, seed, geom, frame_seed, bars):
    """First, middle and last-row / last-column tile: the kept output of the network with all three layers folded over a one-band
    window of the symmetric-padded frame equals oracle.networks.utnet_forward to 1e-12 (measured <= 1.3e-15); and every bar of the
    GPU tests lies 10x below what reading one layer's addend window one pixel off, in any direction, does to the kept output
    (measured: at least 2.3e-1 / 7.8e-2 / 1.8e-2 for tconvs4.0 / 3.0 / 2.0)."""
    from oracle import networks as onet
    from oracle import tiler as otiler
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    W, H, cs, ucs, ol = geom
    sd = _SE._sd64(funit, seed)
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    S, pad, crop = ucs - ol, grid.pad, (cs - ucs) // 2
    assert S % 8 == 0
    frame = synth.make_frame(W, H, seed=frame_seed).astype(np.float64)
    hb, wb = (grid.rows - 1) * S + cs + 4, (grid.cols - 1) * S + cs + 4
    ys_b, xs_b = _ES._band_axis(-pad - 2, hb, H), _ES._band_axis(-pad - 2, wb, W)
    with torch.no_grad():
        band = _SE._encoder64(sd, torch.from_numpy(frame[:, ys_b][:, :, xs_b])[None])

        def kept(y):
            return y[:, :, crop:cs - crop, crop:cs - crop]

        for yi, xi in ((0, 0), (grid.rows // 2, grid.cols // 2), (grid.rows - 1, grid.cols - 1)):
            ys_t, xs_t = _ES._tile_axis(yi, S, pad, cs, H), _ES._tile_axis(xi, S, pad, cs, W)
            xp = torch.from_numpy(frame[:, ys_t][:, :, xs_t])[None]
            y = onet.utnet_forward(sd, xp[:, :, 2:-2, 2:-2])
            assert torch.equal(_folded_forward(sd, xp), y)          # the restatement itself
            sc = max(1.0, kept(y).abs().max().item())
            org = (yi * S, xi * S)
            e = (kept(_folded_forward(sd, xp, band, org)) - kept(y)).abs().max().item() / sc
            sens = []
            for k in range(3):
                only = tuple(j == k for j in range(3))
                sens.append(min((kept(_folded_forward(sd, xp, band, org, sh, only)) - kept(y)).abs().max().item() / sc
                                for sh in ((0, 1), (1, 0), (0, -1), (-1, 0))))
            print(f"UtNet({funit}) {geom} tile ({yi}, {xi}): fold vs oracle {e:.2e}; addend window one pixel off (tconvs4.0, 3.0, 2.0): "
                  + " ".join(f"{v:.2e}" for v in sens))
            assert e <= 1e-12, (yi, xi, e)
            assert min(sens) >= 10 * max(bars), (yi, xi, sens, bars)


# ---------------------------------------------------------------------------- CPU: the host query

def test_frame_folds_query():
    """Bit k: tconvs(4 - k).0 is folded.  A step folds where it takes its skip from the band and runs in a kernel that takes an
    addend: conv_w2d (all three at UtNet(16), tconvs4.0 at UtNet(64)) and the three-pass F(6x6) form (tconvs3.0 / 2.0 at UtNet(64))."""
    for funit in (16, 64):
        for geom in (GEOM_A, GEOM_B, GEOM_C):
            assert _folds(geom, funit=funit) == 0b111, (funit, geom)
        assert _folds(LEVEL2_PER_TILE, funit=funit) == 0b011       # level 2 stays per tile: tconvs2.0's skip is no band tensor
        assert _folds(GEOM_A, funit=funit, flags=_lib.FLAG_TILE_LEVEL2) == 0b011
    for funit in (16, 64):
        for flags in (_lib.FLAG_TILE_SKIPS, _lib.FLAG_TILE_ENCODER, _lib.FLAG_FULL_TILES):
            assert _folds(GEOM_A, funit=funit, flags=flags) == 0, (funit, flags)
        assert _folds(GEOM_A, funit=funit, dtype=_lib.ND_BF16) == 0
        assert _folds(NO_BAND, funit=funit) == 0
    out = ctypes.c_int(0)
    assert _lib.load().nd_utnet_frame_folds(16, 0, 1 << 12, *GEOM_A, ctypes.byref(out)) != 0     # an unknown bit is refused


# ---------------------------------------------------------------------------- GPU

@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ref16():
    """float64 canvases of the UtNet(16) frames, computed once per geometry."""
    from oracle import tiler as otiler
    cache = {}

    def get(geom):
        if geom not in cache:
            W, H, cs, ucs, ol = geom
            cache[geom] = otiler.denoise_frame(synth.make_frame(W, H, seed=3), cs, ucs, ol, _SE._model64(_SE._sd64(16, 9)), batch=16)
        return cache[geom]
    return get


class _Loop:
    """denoise_frame of one frame through one net object, every run preceded by the same run on another frame."""

    def __init__(self, dev, funit, seed, geom, frame_seed):
        from nind_denoise_amd import pipeline
        self.pipeline, self.geom = pipeline, geom
        W, H = geom[:2]
        self.net = _SE._net_visible(dev, funit, seed)
        self.frame = synth.make_frame(W, H, seed=frame_seed)
        self.img = torch.from_numpy(self.frame).to(dev)
        self.other = torch.from_numpy(synth.make_frame(W, H, seed=frame_seed + 100)).to(dev)
        self.total = pipeline.tile_count(*geom)

    def run(self, batch, fold=True, split_k=True, share=True):
        W, H, cs, ucs, ol = self.geom
        self.net.fold_skips, self.net.split_k, self.net.share_encoder = fold, split_k, share
        self.pipeline.denoise_frame(self.net, self.other, cs, ucs, ol, batch=batch)
        cv = torch.zeros_like(self.img)
        self.pipeline.denoise_frame(self.net, self.img, cs, ucs, ol, batch=batch, canvas=cv)
        self.net.fold_skips, self.net.split_k, self.net.share_encoder = True, True, True
        return cv


@pytest.mark.gpu
@pytest.mark.parametrize("geom", [GEOM_A, NARROWEST, GEOM_B], ids=lambda g: "{}x{}-{}-{}-{}".format(*g))
def test_w2d_addend_every_layer_vs_float64(dev, ref16, geom):
    # UtNet(16): all three folded layers run in conv_w2d
    assert _folds(geom, funit=16) == 0b111
    lp = _Loop(dev, 16, 9, geom, 3)
    ref = ref16(geom)
    for batch in (5, lp.total):
        on, off = lp.run(batch), lp.run(batch, fold=False)
        e64, eoff = _SE._rel(on, ref), _SE._rel(on, off)
        print(f"UtNet(16) gain {_SE.VISIBLE_GAIN} {geom} batch {batch}: folded vs float64 {e64:.2e}, vs skip halves per tile {eoff:.2e}")
        assert e64 <= BAR_FRAME16 and eoff <= BAR_SHARED16, (batch, e64, eoff)
        assert not torch.equal(on, off)                       # (the switch does switch something)


@pytest.mark.gpu
@pytest.mark.parametrize("split_k", [True, False], ids=["split-k", "whole-tiles"])
def test_utnet64_folded_vs_float64(dev, split_k):
    # 16 tiles whose region sizes are no multiple of 6: partial F(6x6) tiles of tconvs3.0 / tconvs2.0 meet the addend
    from oracle import tiler as otiler
    geom = GEOM_C
    W, H, cs, ucs, ol = geom
    assert _folds(geom) == 0b111
    lp = _Loop(dev, 64, 123, geom, 24)
    assert lp.total == 16
    ref = otiler.denoise_frame(lp.frame, cs, ucs, ol, _SE._model64(_SE._sd64(64, 123)), batch=16)
    on, off = lp.run(16, split_k=split_k), lp.run(16, fold=False, split_k=split_k)
    e64, eoff = _SE._rel(on, ref), _SE._rel(on, off)
    print(f"UtNet(64) gain {_SE.VISIBLE_GAIN} {geom} split_k {split_k}: folded vs float64 {e64:.2e}, vs skip halves per tile {eoff:.2e}")
    assert e64 <= BAR_TILE64 and eoff <= BAR_SHARED64, (e64, eoff)
    assert not torch.equal(on, off)
    lp.net._workspaces.clear()


@pytest.mark.gpu
def test_launch_over_a_band_seam(dev):
    # two bands, the last of one tile row: a launch of 256 holds tiles of both slots, each reading its own slot's P
    geom = _ES.ONE_ROW_LAST_BAND
    p = _SE._plan(*geom)
    assert (p["D"], p["bands"], p["R"], p["rows"]) == (2, 2, 2, 3) and _folds(geom) != 0
    per_band = p["R"] * p["cols"]
    assert any((k * 256) // per_band != (k * 256 + 255) // per_band for k in range(p["cols"] * p["rows"] // 256))
    lp = _Loop(dev, 64, 123, geom, 24)
    on, off = lp.run(256), lp.run(256, fold=False)
    e = _SE._rel(on, off)
    print(f"UtNet(64) gain {_SE.VISIBLE_GAIN} {geom} batch 256: folded vs skip halves per tile {e:.2e}")
    assert e <= BAR_SHARED64 and not torch.equal(on, off), e
    del on, off
    assert torch.equal(lp.run(256, split_k=False), lp.run(11, split_k=False))
    lp.net._workspaces.clear()


@pytest.mark.gpu
def test_fallbacks(dev, ref16):
    geom = LEVEL2_PER_TILE
    assert _folds(geom, funit=16) == 0b011
    lp = _Loop(dev, 16, 9, geom, 3)
    ref = ref16(geom)
    on, off = lp.run(5), lp.run(5, fold=False)
    e_on, e_off = _SE._rel(on, ref), _SE._rel(off, ref)
    print(f"UtNet(16) gain {_SE.VISIBLE_GAIN} {geom}: levels 0 / 1 folded {e_on:.2e}, none {e_off:.2e} vs float64")
    assert not torch.equal(on, off) and e_on <= BAR_FRAME16 and e_off <= BAR_FRAME16, (e_on, e_off)
    # no band, nothing to fold: the attribute switches nothing
    a, b = lp.run(5, share=False), lp.run(5, fold=False, share=False)
    assert torch.isfinite(a).all() and a.abs().max().item() > 0 and torch.equal(a, b)
