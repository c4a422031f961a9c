"""Host-only checks of the UNet frame loop's useful-region plan (nd_unet_useful_region) against the interval rule restated
here from UNet.forward (reference ThirdPartyNets.py:153-169): outc <- up4 <- up3 <- up2 <- up1, each `up` block being
ConvTranspose2d(2, stride 2) -> F.pad to the skip's size -> cat -> two Conv2d(3, padding=1).  No GPU."""
import ctypes

import pytest

from nind_denoise_amd import _lib

CASES = [(440, 320), (264, 200), (96, 64), (100, 68), (90, 61), (80, 76), (96, 8)]


def expected_plan(cs, ucs):
    """{step name: (r0, rows)} per axis for the restricted steps, from the kept centre [crop, cs - crop) backwards."""
    crop = int((cs - ucs) / 2)
    size = [cs, cs // 2, cs // 4, cs // 8, cs // 16]      # x1 .. x5 (four MaxPool2d(2))
    lo, hi = crop, cs - crop                              # outc is 1x1: same interval on up4's output
    plan = {}
    for n in (4, 3, 2, 1):                                # up4 works at size[0] from size[1], ..., up1 at size[3] from size[4]
        s_out, s_in = size[4 - n], size[5 - n]
        for conv in ("conv.conv.3", "conv.conv.0"):       # second conv first (walking backwards)
            if not (lo == 0 and hi == s_out):
                plan[f"up{n}.{conv}"] = (lo, hi - lo)     # region on the conv's output grid
            lo, hi = max(lo - 1, 0), min(hi + 1, s_out)   # padding=1: inputs one pixel further, clipped
        lo, hi = lo >> 1, min((hi + 1) >> 1, s_in)        # stride-2 transpose: region on its input grid
        if not (lo == 0 and hi == s_in):
            plan[f"up{n}.up"] = (lo, hi - lo)
    return plan


def library_plan(cs, ucs):
    lib = _lib.load()
    crop = int((cs - ucs) / 2)
    steps = lib.nd_unet_num_steps()
    names, rects, counts = [], [], set()
    for i in range(steps):
        rect = (ctypes.c_int * 4)()
        n = lib.nd_unet_useful_region(cs, crop, i, rect)
        assert n >= 0, lib.nd_last_error()
        counts.add(n)
        names.append(lib.nd_unet_step_name(i).decode())
        rects.append(tuple(rect))
    assert len(counts) == 1
    return names, rects, counts.pop()


def test_step_names():
    lib = _lib.load()
    assert lib.nd_version() >= 109
    names = [lib.nd_unet_step_name(i).decode() for i in range(lib.nd_unet_num_steps())]
    assert names.count("pool") == 4 and len(names) == 26
    want = ["inc.conv.conv.0", "inc.conv.conv.3"]
    for n in range(1, 5):
        want += ["pool", f"down{n}.mpconv.1.conv.0", f"down{n}.mpconv.1.conv.3"]
    for n in range(1, 5):
        want += [f"up{n}.up", f"up{n}.conv.conv.0", f"up{n}.conv.conv.3"]
    assert names == want
    assert lib.nd_unet_step_name(-1) is None and lib.nd_unet_step_name(26) is None


@pytest.mark.parametrize("cs,ucs", CASES)
def test_useful_region_follows_the_interval_rule(cs, ucs):
    names, rects, n = library_plan(cs, ucs)
    want = expected_plan(cs, ucs)
    assert n == len(want)
    for name, rect in zip(names, rects):
        if name in want:
            r0, rows = want[name]
            assert rect == (r0, r0, rows, rows), (name, rect, want[name])       # square tiles: the same interval on both axes
        else:
            assert rect == (0, 0, 0, 0), (name, rect)
        if name == "pool" or name.startswith(("inc.", "down")):
            assert rect == (0, 0, 0, 0)                                         # the encoder feeds the skips: always whole


def test_useful_region_table_of_the_reference_tiling():
    # cs 440 / ucs 320 (the reference's CS_UNET, UCS_UNET), worked by hand from the rule
    names, rects, n = library_plan(440, 320)
    got = {name: (r[0], r[2]) for name, r in zip(names, rects) if r[2]}
    assert n == 12 and got == {
        "up4.conv.conv.3": (60, 320), "up4.conv.conv.0": (59, 322), "up4.up": (29, 162),
        "up3.conv.conv.3": (29, 162), "up3.conv.conv.0": (28, 164), "up3.up": (13, 84),
        "up2.conv.conv.3": (13, 84), "up2.conv.conv.0": (12, 86), "up2.up": (5, 45),
        "up1.conv.conv.3": (5, 45), "up1.conv.conv.0": (4, 47), "up1.up": (1, 25)}
    names, rects, _ = library_plan(96, 64)
    whole = [name for name, r in zip(names, rects) if r == (0, 0, 0, 0) and name.startswith("up")]
    assert whole == ["up1.up", "up1.conv.conv.0", "up1.conv.conv.3", "up2.up"]


def test_useful_region_arguments():
    lib = _lib.load()
    rect = (ctypes.c_int * 4)()
    assert lib.nd_unet_useful_region(96, 16, 26, rect) == -1       # step outside the list
    assert lib.nd_unet_useful_region(96, 48, 0, rect) == -1        # nothing kept
    assert lib.nd_unet_useful_region(8, 0, 0, rect) == -1          # too small for four pools
    assert lib.nd_unet_useful_region(96, 0, 25, rect) == 0 and tuple(rect) == (0, 0, 0, 0)   # whole output kept: no region


def test_unet_flags_property():
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    net = UNet()
    assert (UNet.split_k, UNet.useful_only, UNet.pack_on_device) == (True, True, True) and net.flags == 0
    net.split_k = False
    assert net.flags == _lib.FLAG_NO_SPLITK
    net.useful_only = False
    assert net.flags == _lib.FLAG_NO_SPLITK | _lib.FLAG_FULL_TILES
