"""UNet(winograd=True) without a GPU: the parameter's spellings, the form plan behind ND_FLAG_UNET_WINOGRAD (nd_unet_step_form), the
flag-taking size functions against the plain ones, and who takes the flag."""
import ctypes

import pytest

from nind_denoise_amd import _lib
from nind_denoise_amd.networks.ThirdPartyNets import UNet

WINO = _lib.FLAG_UNET_WINOGRAD
POOL, DIRECT, F43, WINO3P = -1, 0, 1, 3

# the plan of the reference's UNet: F(4,3) for inc.3, down1.*, up2.conv.3, up3.*, up4.*; three-pass for down2 ... down4, up1.*,
# up2.conv.0; direct for inc.0 (Cin 3); transposes direct, pools as they are
PLAN = {
    "inc.conv.conv.0": DIRECT, "inc.conv.conv.3": F43,
    "down1.mpconv.1.conv.0": F43, "down1.mpconv.1.conv.3": F43,
    "down2.mpconv.1.conv.0": WINO3P, "down2.mpconv.1.conv.3": WINO3P,
    "down3.mpconv.1.conv.0": WINO3P, "down3.mpconv.1.conv.3": WINO3P,
    "down4.mpconv.1.conv.0": WINO3P, "down4.mpconv.1.conv.3": WINO3P,
    "up1.up": DIRECT, "up1.conv.conv.0": WINO3P, "up1.conv.conv.3": WINO3P,
    "up2.up": DIRECT, "up2.conv.conv.0": WINO3P, "up2.conv.conv.3": F43,
    "up3.up": DIRECT, "up3.conv.conv.0": F43, "up3.conv.conv.3": F43,
    "up4.up": DIRECT, "up4.conv.conv.0": F43, "up4.conv.conv.3": F43,
}


def _steps():
    lib = _lib.load()
    return [lib.nd_unet_step_name(i).decode() for i in range(lib.nd_unet_num_steps())]


def _forms(flags, shape):
    lib = _lib.load()
    return [lib.nd_unet_step_form(flags, *shape, i) for i in range(lib.nd_unet_num_steps())]


def _conv3_steps():
    return [i for i, n in enumerate(_steps()) if n.endswith(".0") or n.endswith(".3")]


@pytest.mark.parametrize("value", [True, "True", "true", "1"])
def test_true_spellings(value):
    net = UNet(winograd=value)
    assert net.winograd is True
    assert net.flags & WINO and not net.grad_flags & WINO


@pytest.mark.parametrize("value", [False, "False", "false", "0"])
def test_false_spellings(value):
    net = UNet(winograd=value)
    assert net.winograd is False
    assert not net.flags & WINO


def test_default_is_off():
    assert UNet().winograd is False and not UNet().flags & WINO


@pytest.mark.parametrize("value", ["yes", "on", 2, "winograd", "TRUE"])
def test_other_spellings_raise(value):
    with pytest.raises(ValueError):
        UNet(winograd=value)


def test_train_mode_still_raises():
    import torch
    net = UNet(winograd=True).train()
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 3, 16, 16))


@pytest.mark.parametrize("shape", [(20, 440, 440), (1, 256, 256), (2, 17, 31)])
def test_without_the_flag_every_conv3_is_direct(shape):
    forms = _forms(0, shape)
    conv3 = _conv3_steps()
    assert len(conv3) == 18
    assert all(forms[i] == DIRECT for i in conv3)
    assert [f for f, n in zip(forms, _steps()) if n == "pool"] == [POOL] * 4
    # the other switches alone choose no Winograd form either
    assert _forms(_lib.FLAG_TILE_WINO | _lib.FLAG_W1D_REGS, shape) == forms


@pytest.mark.parametrize("shape", [(20, 440, 440), (1, 256, 256)])
def test_plan_with_the_flag(shape):
    names, forms = _steps(), _forms(WINO, shape)
    assert len(names) == 26 and set(names) - {"pool"} == set(PLAN)
    for n, f in zip(names, forms):
        assert f == (POOL if n == "pool" else PLAN[n]), (n, f)
    assert sum(f == F43 for f in forms) == 8 and sum(f == WINO3P for f in forms) == 9


def test_direct_conv_flag_wins():
    assert _forms(WINO | _lib.FLAG_DIRECT_CONV, (1, 256, 256)) == _forms(0, (1, 256, 256))


def test_a_refused_layer_alone_is_direct():
    # ND_FLAG_W1D_REGS sends the F(4,3) layers to conv_w1d, whose stage images do not fit the LDS for the 442-pixel rows of the
    # full-resolution buffers: inc.3, up4.conv.0 and up4.conv.3 alone run direct, every other layer keeps its form
    names = _steps()
    wide = _forms(WINO | _lib.FLAG_W1D_REGS, (1, 440, 440))
    refused = {n for n, f in zip(names, wide) if n != "pool" and f != PLAN[n]}
    assert refused == {"inc.conv.conv.3", "up4.conv.conv.0", "up4.conv.conv.3"}
    assert all(wide[names.index(n)] == DIRECT for n in refused)
    # at 256 pixels the rows fit and nothing is refused
    assert _forms(WINO | _lib.FLAG_W1D_REGS, (1, 256, 256)) == _forms(WINO, (1, 256, 256))


def test_step_form_bad_arguments():
    lib = _lib.load()
    for args in [(WINO, 1, 256, 256, 26), (WINO, 1, 256, 256, -1), (WINO, 1, 8, 256, 0), (WINO, 0, 256, 256, 0), (2048, 1, 256, 256, 0)]:
        assert lib.nd_unet_step_form(*args) < -1, args


@pytest.mark.parametrize("shape", [(16, 16, 1), (17, 31, 2), (440, 440, 20), (256, 256, 1)])
def test_sizes_with_flags_zero_are_the_plain_ones(shape):
    lib = _lib.load()
    h, w, b = shape
    assert lib.nd_unet_packed_bytes_flags(_lib.ND_F32, 0) == lib.nd_unet_packed_bytes(_lib.ND_F32) > 0
    plain = lib.nd_unet_workspace_bytes(h, w, b, _lib.ND_F32)
    assert lib.nd_unet_workspace_bytes_flags(h, w, b, _lib.ND_F32, 0) == plain > 0
    # the other switches size nothing; the Winograd forms go behind: both grow
    assert lib.nd_unet_workspace_bytes_flags(h, w, b, _lib.ND_F32, _lib.FLAG_NO_SPLITK | _lib.FLAG_FULL_TILES) == plain
    assert lib.nd_unet_workspace_bytes_flags(h, w, b, _lib.ND_F32, WINO) > plain
    assert lib.nd_unet_packed_bytes_flags(_lib.ND_F32, WINO) > lib.nd_unet_packed_bytes(_lib.ND_F32)
    assert lib.nd_unet_packed_bytes_flags(_lib.ND_BF16, WINO) == 0


def test_host_pack_with_flags_zero_is_the_plain_blob():
    import torch
    from nind_denoise_amd import synth
    lib = _lib.load()
    sd = synth.make_unet_state_dict(2)
    n = lib.nd_unet_num_tensors()
    keep = [sd[lib.nd_unet_tensor_name(i).decode()].float().contiguous() for i in range(n)]
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in keep])
    plain_bytes, wino_bytes = lib.nd_unet_packed_bytes(_lib.ND_F32), lib.nd_unet_packed_bytes_flags(_lib.ND_F32, WINO)
    plain = torch.full((plain_bytes // 4,), float("nan"))
    flagged = torch.full((plain_bytes // 4,), float("nan"))
    wino = torch.full((wino_bytes // 4,), float("nan"))
    _lib.check(lib.nd_unet_pack_weights(_lib.ND_F32, ptrs, n, plain.data_ptr(), plain_bytes))
    _lib.check(lib.nd_unet_pack_weights_flags(_lib.ND_F32, 0, ptrs, n, flagged.data_ptr(), plain_bytes))
    _lib.check(lib.nd_unet_pack_weights_flags(_lib.ND_F32, WINO, ptrs, n, wino.data_ptr(), wino_bytes))
    assert torch.equal(plain.view(torch.int32), flagged.view(torch.int32))
    # the Winograd forms lie behind the default blob: no offset of it moves
    assert torch.equal(wino[:plain_bytes // 4].view(torch.int32), plain.view(torch.int32))
    assert torch.isfinite(wino).all() and wino[plain_bytes // 4:].abs().max() > 0
    # a blob sized without the flag is refused with it
    with pytest.raises(MemoryError):
        _lib.check(lib.nd_unet_pack_weights_flags(_lib.ND_F32, WINO, ptrs, n, plain.data_ptr(), plain_bytes))


def test_flag_is_unknown_outside_the_unet_inference_entry_points():
    lib = _lib.load()
    levels = (ctypes.c_int * 8)()
    # a UtNet entry point (host-only query): an unknown bit
    assert lib.nd_utnet_frame_plan(64, _lib.ND_F32, 0, 6000, 4000, 264, 200, 32, levels) == 0
    with pytest.raises(ValueError, match="unknown flag"):
        _lib.check(lib.nd_utnet_frame_plan(64, _lib.ND_F32, WINO, 6000, 4000, 264, 200, 32, levels))
    assert lib.nd_utnet_frame_workspace_bytes(64, _lib.ND_F32, WINO, 6000, 4000, 264, 200, 32, 8) == 0
    with pytest.raises(ValueError, match="unknown flag"):
        _lib.check(lib.nd_utnet_frame_levels(64, _lib.ND_F32, WINO, 6000, 4000, 264, 200, 32, levels))
