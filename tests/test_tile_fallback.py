"""fallback_dtype on the GPU: the checked frame loop (nd_utnet_denoise_frame_checked) finds exactly the tiles whose fp16 result is
not finite, keeps them out of the canvas, and pipeline.denoise_frame recomputes them in the fallback dtype -- the canvas is the
stated composition bit for bit: good tiles ascending, then recomputed tiles ascending.

Frames: synth.make_frame with a 4 x 4 patch of 1e5 in all three channels.  1e5 is an fp16 infinity once the gather packs the
tile and a plain number in bf16 and fp32; every useful output of a tile depends on its whole input through the bottom level, so
a tile is bad in fp16 exactly when its gathered window (mirror copies included) holds a patch pixel.  The tests work that
expectation out themselves from pipeline.gather_tiles and compare it with the sets worked out on the CPU (CASES).

Bits are compared across launch shapes with split_k = False only (ND_FLAG_NO_SPLITK: a tile's bits do not depend on its launch)."""
import os

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib, pipeline, synth
from nind_denoise_amd.networks.UtNet import UtNet

from test_compute_dtype import GEOM, _Worker, _cli, _same_file  # noqa: F401  (GEOM: case A's tile geometry on the command line)

pytestmark = pytest.mark.gpu

# name: (W, H, cs, ucs, ol, patch x, patch y, tiles, expected bad tiles)
CASES = {
    "A": (310, 275, 120, 88, 16, 150, 130, 20, [6, 7, 11, 12]),      # two runs of two
    "B": (200, 150, 104, 72, 10, 190, 140, 12, [6, 7, 10, 11]),      # truncated last row and column; the patch is mirrored too
    "C": (200, 150, 104, 72, 10, 30, 40, 12, [0]),                   # a single corner tile
}
F16_MAX = 65504.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.load()
    return torch.device("cuda:0")


_SD = {}
_NETS = {}


def _sd(kind="plain"):
    if kind not in _SD:
        sd = synth.make_utnet_state_dict(funit=16, seed=21)
        if kind == "overflow":      # (the checkpoint of test_compute_dtype.test_non_finite_16bit_result_is_refused)
            w0 = sd["convs1.0.weight"]
            sd["convs1.0.weight"] = w0 * (1e7 / w0.abs().max().item())
        _SD[kind] = sd
    return _SD[kind]


def _net(dev, dtype, fallback=None, split_k=False, share_encoder=True, sd="plain"):
    key = (dtype, fallback, split_k, share_encoder, sd)
    if key not in _NETS:
        net = UtNet(funit=16, compute_dtype=dtype, fallback_dtype=fallback)
        net.load_state_dict(_sd(sd))
        net = net.eval().to(dev)
        net.split_k, net.share_encoder = split_k, share_encoder
        _NETS[key] = net
    return _NETS[key]


def _frame(case, patch=True):
    W, H, cs, ucs, ol, px, py, tiles, bad = CASES[case]
    frame = synth.make_frame(W, H, seed=8)
    if patch:
        frame[:, py:py + 4, px:px + 4] = 1e5
    return frame


def _case(dev, case, patch=True):
    """(frame on the device, (cs, ucs, ol), tiles, the bad tiles worked out from the gathered windows)"""
    W, H, cs, ucs, ol, px, py, tiles, bad = CASES[case]
    img = torch.from_numpy(_frame(case, patch)).to(dev)
    assert pipeline.tile_count(W, H, cs, ucs, ol) == tiles
    win = pipeline.gather_tiles(img, cs, ucs, ol, 0, tiles)
    expect = [t for t in range(tiles) if float(win[t].abs().max()) > F16_MAX]
    if patch:
        assert expect == bad, (case, expect)
        assert 0 < len(expect) < tiles
    else:
        assert expect == []
    return img, (cs, ucs, ol), tiles, expect


def _checked(net, img, geom, batch, rng=None, preset_outside=5):
    """nd_utnet_denoise_frame_checked itself: (canvas, flags).  Flags of the range preset to 1, the others to preset_outside."""
    cs, ucs, ol = geom
    H, W = img.size(1), img.size(2)
    tiles = pipeline.tile_count(W, H, cs, ucs, ol)
    begin, end = rng or (0, tiles)
    batch = max(1, min(batch, end - begin))
    dev = img.device
    flags = torch.full((tiles,), preset_outside, dtype=torch.uint8, device=dev)
    flags[begin:end] = 1
    canvas = torch.zeros_like(img)
    with torch.cuda.device(dev):
        blob, ws = net.packed_weights(dev), net.workspace(cs, batch, dev)
        fws = net.frame_workspace(W, H, cs, ucs, ol, batch, dev)
        _lib.check(_lib.load().nd_utnet_denoise_frame_checked(
            net.funit, _lib.ACT[net.activation], net._dt, net.frame_flags, blob.data_ptr(), img.data_ptr(), canvas.data_ptr(), W, H, cs, ucs,
            ol, begin, end - begin, batch, ws.data_ptr(), ws.numel(), fws.data_ptr() if fws is not None else None,
            fws.numel() if fws is not None else 0, _lib.stream_ptr(dev), _lib.PROGRESS_FN(), None, flags.data_ptr()),
            "nd_utnet_denoise_frame_checked")
    return canvas, flags.cpu().tolist()


def _cover(img, geom, tiles_of):
    """bool [H, W]: the pixels some tile of tiles_of adds to (the useful rectangles of nd_tile_geom)"""
    cs, ucs, ol = geom
    H, W = img.size(1), img.size(2)
    m = torch.zeros((H, W), dtype=torch.bool)
    for t in tiles_of:
        _, _, ud, us = _lib.tile_geom(t, W, H, cs, ucs, ol)
        m[us[1]:us[1] + ud[3] - ud[1], us[0]:us[0] + ud[2] - ud[0]] = True
    return m.to(img.device)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))     # bits (NaN payloads included)


# ---------------------------------------------------------------------------- 1. verdicts

@pytest.mark.parametrize("batch", [64, 5])
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_verdicts_are_the_tiles_that_hold_the_patch(dev, case, batch):
    """batch 64: one launch; batch 5: launch boundaries inside a run of bad tiles and a partial last launch"""
    img, geom, tiles, expect = _case(dev, case)
    _, flags = _checked(_net(dev, "f16"), img, geom, batch)
    assert [t for t in range(tiles) if flags[t] == 0] == expect and set(flags) == {0, 1}, flags


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
@pytest.mark.parametrize("case", ["A", "B", "C"])
def test_no_tile_is_bad_where_the_patch_fits_the_type(dev, case, dtype):
    img, geom, tiles, _ = _case(dev, case)
    canvas, flags = _checked(_net(dev, dtype, split_k=True), img, geom, 5)       # (f32: the shared-encoder path where the plan takes it)
    assert flags == [1] * tiles and bool(torch.isfinite(canvas).all())


def test_flags_outside_the_range_are_not_touched(dev):
    img, geom, tiles, expect = _case(dev, "A")
    _, flags = _checked(_net(dev, "f16"), img, geom, 3, rng=(5, 12), preset_outside=5)
    assert flags[:5] == [5] * 5 and flags[12:] == [5] * (tiles - 12), flags        # tile 12 is bad, and outside
    assert [t for t in range(5, 12) if flags[t] == 0] == [t for t in expect if 5 <= t < 12] == [6, 7, 11]
    assert all(flags[t] == 1 for t in (5, 8, 9, 10))


# ---------------------------------------------------------------------------- 2. the canvas is the stated composition

@pytest.mark.parametrize("fallback", ["f32", "bf16"])
@pytest.mark.parametrize("case,batch", [("A", 64), ("B", 5)])
def test_canvas_is_good_tiles_then_recomputed_tiles(dev, case, batch, fallback):
    img, geom, tiles, bad = _case(dev, case)
    good = [t for t in range(tiles) if t not in bad]
    plain16 = _net(dev, "f16")
    plain_fb = _net(dev, fallback, share_encoder=False)
    # the reference canvas through the existing public path only: every good tile in fp16, ascending, then every bad tile in the
    # fallback dtype with the per-tile encoder, ascending -- one call per tile
    ref = torch.zeros_like(img)
    for t in good:
        pipeline.denoise_frame(plain16, img, *geom, tile_range=(t, t + 1), canvas=ref)
    for t in bad:
        pipeline.denoise_frame(plain_fb, img, *geom, tile_range=(t, t + 1), canvas=ref)
    report = {}
    got = pipeline.denoise_frame(_net(dev, "f16", fallback), img, *geom, batch=batch, report=report)
    assert report == {"tiles": tiles, "fallback_tiles": bad, "fallback_dtype": fallback}
    assert bool(torch.isfinite(got).all()) and _same(got, ref), int((got != ref).sum())
    # pixels no bad tile covers: the plain fp16 canvas (which is not finite elsewhere)
    c16 = pipeline.denoise_frame(plain16, img, *geom, batch=batch)
    assert not bool(torch.isfinite(c16).all())
    clean = ~_cover(img, geom, bad)
    assert bool(clean.any()) and _same(got[:, clean], c16[:, clean])
    # pixels only bad tiles cover: the plain canvas of the fallback dtype with the per-tile encoder
    only_bad = _cover(img, geom, bad) & ~_cover(img, geom, good)
    if case == "A":
        block = torch.zeros_like(only_bad)
        block[88:216, 88:216] = True
        assert torch.equal(only_bad, block)
    assert bool(only_bad.any())
    cfb = pipeline.denoise_frame(plain_fb, img, *geom, batch=batch)
    assert _same(got[:, only_bad], cfb[:, only_bad])
    assert not _same(got[:, only_bad], c16[:, only_bad])


# ---------------------------------------------------------------------------- 3. nothing to do costs no bits

@pytest.mark.parametrize("dtype,fallback", [("f16", "f32"), ("f16", "bf16"), ("bf16", "f32")])
def test_no_bad_tile_gives_the_plain_canvas(dev, dtype, fallback):
    img, geom, tiles, _ = _case(dev, "A", patch=False)
    report = {}
    got = pipeline.denoise_frame(_net(dev, dtype, fallback, split_k=True), img, *geom, batch=7, report=report)
    plain = pipeline.denoise_frame(_net(dev, dtype, split_k=True), img, *geom, batch=7)
    assert report == {"tiles": tiles, "fallback_tiles": [], "fallback_dtype": fallback}
    assert bool(torch.isfinite(got).all()) and _same(got, plain)


@pytest.mark.parametrize("case", ["A", "B"])
def test_checked_entry_in_fp32_is_the_plain_entry(dev, case):
    """fp32 has no fallback; the checked entry still takes it (case A: through the shared encoder's launches)"""
    img, geom, tiles, _ = _case(dev, case, patch=False)
    net = _net(dev, "f32", split_k=True)
    if case == "A":
        plan = (_lib.c_int * 8)()
        _lib.check(_lib.load().nd_utnet_frame_plan(net.funit, net._dt, net.frame_flags, img.size(2), img.size(1), *geom, plan))
        assert plan[0] == 2, list(plan)       # (the shared-encoder path)
    got, flags = _checked(net, img, geom, 7)
    plain = pipeline.denoise_frame(net, img, *geom, batch=7)
    assert flags == [1] * tiles and _same(got, plain)


# ---------------------------------------------------------------------------- 4. every tile bad

def test_every_tile_bad_is_the_plain_fallback_run(dev):
    img, geom, tiles, _ = _case(dev, "A", patch=False)
    report = {}
    got = pipeline.denoise_frame(_net(dev, "f16", "bf16", sd="overflow"), img, *geom, batch=64, report=report)
    assert report["fallback_tiles"] == list(range(tiles)) and report["fallback_dtype"] == "bf16"
    plain = pipeline.denoise_frame(_net(dev, "bf16", sd="overflow"), img, *geom, batch=64)
    assert bool(torch.isfinite(plain).all()) and _same(got, plain)


# ---------------------------------------------------------------------------- 5. shards

def test_shards_add_up_to_the_whole_range(dev):
    """Tile ranges (0, 10) and (10, 20) into one canvas.  Each call adds its good tiles, then its recomputed ones, so the shards add
    a pixel's tiles in the order [good of 0..9, bad of 0..9, good of 10..19, bad of 10..19] and the whole-range call in the order
    [good, bad].  The two orders are the same sequence wherever no bad tile of the first range (6, 7) shares a pixel with a tile of
    the second range: there the canvases agree bit for bit.  On the other pixels the same n <= 4 fp32 terms (products with the seam
    factors 1, 1/2, 1/4 are exact) are added in another order: either sum is within gamma_3 * S of the exact one, S = sum |term|,
    gamma_3 = 3u / (1 - 3u), u = 2^-24 (n - 1 <= 3 rounded additions), so the canvases differ by <= 2 gamma_3 S.  S is taken per
    pixel: the stitch of |UtNet(tile)| -- fp16 forward for the good tiles, fp32 forward for the recomputed ones -- with 0.1 % on top,
    since a forward's values may be fp32 re-associations (<= 1e-5) of the frame loop's.  Measured on an MI355X: 2560 such pixels,
    max |diff| 2.98e-8 (S up to 0.34), every other sample identical -- so bit equality of the whole canvas, which the stated
    summation order does not promise, does not hold either."""
    img, geom, tiles, bad = _case(dev, "A")
    net = _net(dev, "f16", "f32")
    whole = pipeline.denoise_frame(net, img, *geom, batch=64)
    parts = torch.zeros_like(img)
    reports = [{}, {}]
    pipeline.denoise_frame(net, img, *geom, batch=64, tile_range=(0, 10), canvas=parts, report=reports[0])
    pipeline.denoise_frame(net, img, *geom, batch=64, tile_range=(10, 20), canvas=parts, report=reports[1])
    assert [r["fallback_tiles"] for r in reports] == [[6, 7], [11, 12]] and [r["tiles"] for r in reports] == [10, 10]
    assert bool(torch.isfinite(parts).all())
    reordered = _cover(img, geom, [6, 7]) & _cover(img, geom, range(10, 20))
    assert bool(reordered.any()) and _same(parts[:, ~reordered], whole[:, ~reordered])
    win = pipeline.gather_tiles(img, *geom, 0, tiles)
    terms = _net(dev, "f16")(win).abs()
    terms[bad] = _net(dev, "f32")(win[bad]).abs()
    S = 1.001 * pipeline.stitch_tiles(torch.zeros_like(img), terms, *geom, 0)
    assert bool(torch.isfinite(S).all())
    u = 2.0 ** -24
    bound = 2 * (3 * u / (1 - 3 * u)) * S[:, reordered]
    diff = (parts[:, reordered] - whole[:, reordered]).abs()
    print(f"shards vs whole range on the {int(reordered.sum())} re-ordered pixels: max |diff| {float(diff.max()):.3e}, "
          f"smallest bound - |diff| {float((bound - diff).min()):.3e}, max S {float(S[:, reordered].max()):.3e}")
    assert bool((diff <= bound).all())


# ---------------------------------------------------------------------------- 6. still refused

def _write_tiff(path, frame):
    from nind_denoise_amd.common.libs import imgcodec
    imgcodec.write_tiff(str(path), np.ascontiguousarray(frame.transpose(1, 2, 0)))


def test_a_frame_the_fallback_cannot_mend_is_refused(dev, tmp_path, capsys):
    from nind_denoise_amd import denoise_image
    W, H, cs, ucs, ol = CASES["A"][:5]
    frame = _frame("A", patch=False)
    frame[1, 130, 150] = np.nan
    _write_tiff(tmp_path / "nan.tif", frame)
    with pytest.raises(FloatingPointError) as e:
        denoise_image.denoise_file(_net(dev, "f16", "f32"), str(tmp_path / "nan.tif"), str(tmp_path / "nan_out.tiff"), cs, ucs, ol, batch=64,
                                   device=dev, verbose=False)
    assert "compute_dtype=f16" in str(e.value) and "fallback_dtype=f32" in str(e.value) and "nothing written" in str(e.value)
    assert not os.path.exists(tmp_path / "nan_out.tiff")
    assert "fallback: 4 of 20 tiles recomputed in f32" in capsys.readouterr().out      # (it tried)
    # without the parameter the patch frame is refused with today's message
    _write_tiff(tmp_path / "patch.tif", _frame("A"))
    with pytest.raises(FloatingPointError, match="use bf16 or f32") as e:
        denoise_image.denoise_file(_net(dev, "f16"), str(tmp_path / "patch.tif"), str(tmp_path / "patch_out.tiff"), cs, ucs, ol, batch=64,
                                   device=dev, verbose=False)
    assert "fallback_dtype" not in str(e.value) and "with compute_dtype=f16 for" in str(e.value)
    assert not os.path.exists(tmp_path / "patch_out.tiff")
    assert "fallback:" not in capsys.readouterr().out


# ---------------------------------------------------------------------------- 7. through the surfaces

def test_cli_and_worker_take_the_model_parameter(dev, tmp_path, capsys):
    from nind_denoise_amd.common.libs import np_imgops
    torch.save(_sd(), tmp_path / "generator_650.pt")
    _write_tiff(tmp_path / "in.tif", _frame("A"))
    img, geom, tiles, bad = _case(dev, "A")
    with_fb, without = "funit=16,compute_dtype=f16,fallback_dtype=f32", "funit=16,compute_dtype=f16"
    capsys.readouterr()
    assert _cli(tmp_path, "cli.tiff", with_fb) == 0
    assert "fallback: 4 of 20 tiles recomputed in f32" in capsys.readouterr().out
    got = np_imgops.img_path_to_np_flt(str(tmp_path / "cli.tiff"))
    want = pipeline.denoise_frame(_net(dev, "f16", "f32", split_k=True), img, *geom, batch=64)
    assert np.isfinite(got).all() and np.array_equal(got, want.cpu().numpy())
    assert _cli(tmp_path, "cli_bad.tiff", without) != 0
    assert "use bf16 or f32" in capsys.readouterr().err and not os.path.exists(tmp_path / "cli_bad.tiff")
    with _Worker(tmp_path) as w:
        r = w.denoise("w.tiff", with_fb)
        assert r.returncode == 0 and "fallback: 4 of 20 tiles recomputed in f32" in r.stdout, r.stdout + r.stderr
        assert _same_file(tmp_path / "w.tiff", tmp_path / "cli.tiff")
        # the other setting gets its own model (the cache key holds the parameter string), then the first one again
        r = w.denoise("w_bad.tiff", without)
        assert r.returncode != 0 and "use bf16 or f32" in r.stderr and not os.path.exists(tmp_path / "w_bad.tiff"), r.stdout + r.stderr
        r = w.denoise("w2.tiff", with_fb)
        assert r.returncode == 0 and _same_file(tmp_path / "w2.tiff", tmp_path / "cli.tiff"), r.stdout + r.stderr
        r = w.client("--ping")
        assert r.returncode == 0 and "2 model(s) resident" in r.stdout, r.stdout + r.stderr
