"""compute_dtype as a model parameter, host side (no GPU): the constructor / instantiate_model surface, the 16-bit layout of the
host packer pinned against a numpy restatement (it is the yardstick the device packer is held to, tests/test_compute_dtype.py),
and the CLI's parser and thin client."""
import json
import os
import socket
import threading

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib

SPELLINGS = {"f32": "f32", "fp32": "f32", "float32": "f32", "bf16": "bf16", "bfloat16": "bf16", "f16": "f16", "fp16": "f16",
             "float16": "f16"}


def test_compute_dtype_is_a_model_parameter():
    from nind_denoise_amd import nn_common
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    from nind_denoise_amd.networks.UtNet import UtNet
    assert set(SPELLINGS) == set(_lib.DTYPE)
    assert UtNet(funit=16).compute_dtype == "f32"
    for s, short in SPELLINGS.items():
        assert UtNet(funit=16, compute_dtype=s).compute_dtype == short
        assert UtNet(funit=16).set_compute_dtype(s).compute_dtype == short
    for bad in ("half", "F16", "", "int8"):
        with pytest.raises(ValueError, match="bf16"):      # (the message lists the choices)
            UtNet(funit=16, compute_dtype=bad)
        with pytest.raises(ValueError, match="bf16"):
            UtNet(funit=16).set_compute_dtype(bad)
    m = nn_common.Model.instantiate_model(network="UtNet", strparameters="funit=16,compute_dtype=f16", device="cpu")
    assert m.compute_dtype == "f16" and m.funit == 16
    with pytest.raises(NotImplementedError, match="UtNet only"):
        UNet(compute_dtype="bf16")
    with pytest.raises(ValueError):
        UNet(compute_dtype="half")
    UNet(compute_dtype="fp32")


# ---------------------------------------------------------------------------- the host packer's 16-bit layout

def special_weights(shape, seed, overflow=True, scale=1.0):
    """scale * randn with, planted at fixed strides: bf16 round-to-even ties (low 16 bits 0x8000, kept and rounded-up cases
    alike), fp16
    ties (low 13 bits 0x1000), fp16 subnormals (x 1e-6), values that round to zero in fp16 (x 1e-9), values past the fp16 range
    (x 1e5; optional) and -0.0."""
    w = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).reshape(-1).contiguous()
    bits = w.view(torch.int32).clone()
    n = w.numel()
    idx = torch.arange(n)
    bits[idx % 11 == 0] = (bits[idx % 11 == 0] & ~0xffff) | 0x8000
    bits[idx % 11 == 1] = (bits[idx % 11 == 1] & ~0x1fff) | 0x1000
    w = bits.view(torch.float32).clone()
    w[idx % 11 == 2] *= 1e-6
    w[idx % 11 == 3] *= 1e-9
    if overflow:
        w[idx % 11 == 4] *= 1e5
    w[idx % 11 == 5] = -0.0
    return w.reshape(shape).contiguous()


def _up_row(m, cout, cpp):
    """nd_up_row of csrc/nd_common.h: GEMM row m of a 2x2 stride-2 transpose -> (a, b, co)."""
    e, b, g = m % cpp, (m // cpp) & 1, m // (2 * cpp)
    return g // (cout // cpp), b, cpp * (g % (cout // cpp)) + e


def _ref_pack16(kind, cin, cout, w16, MT):
    """The layout csrc/pack.hip states for the 16-bit types, applied to the already rounded weights w16 (uint16, torch shape):
    piece [mtile][kb][tap] of 1 KiB; lane 32 h + i holds row m = 32 mtile + i, channels ci = 16 kb + 8 h + s (s = 0..7)."""
    taps = 9 if kind in ("conv3", "convT3") else 1
    M = 4 * cout if kind == "convT2s2" else cout
    KB = (cin + 15) // 16
    out = np.zeros((MT, KB, taps, 64, 8), dtype=np.uint16)
    for mt in range(MT):
        for lane in range(64):
            i, h = lane & 31, lane >> 5
            m = 32 * mt + i
            if m >= M:
                continue
            for kb in range(KB):
                for s in range(8):
                    ci = 16 * kb + 8 * h + s
                    if ci >= cin:
                        continue
                    if kind == "conv3":
                        v = w16[m, ci].reshape(9)
                    elif kind == "convT3":
                        v = w16[ci, m].reshape(9)[::-1]
                    elif kind == "convT2s2":
                        a, b, co = _up_row(m, cout, 8)
                        v = w16[ci, co, a, b]
                    else:
                        v = w16[m, ci, 0, 0]
                    out[mt, kb, :, lane, s] = v
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("kind,cin,cout", [("conv3", 16, 40), ("conv3", 48, 32), ("conv1", 32, 16), ("convT3", 24, 16),
                                           ("convT2s2", 16, 8), ("convT2s2", 32, 16)])
def test_host_packer_16bit_layout(kind, cin, cout, dtype):
    lib = _lib.load()
    k = {"conv3": 3, "convT3": 3, "convT2s2": 2, "conv1": 1}[kind]
    taps = 9 if k == 3 else 1
    shape = (cout, cin, k, k) if kind in ("conv3", "conv1") else (cin, cout, k, k)
    w = special_weights(shape, seed=cin * 100 + cout)
    b = torch.randn(cout, generator=torch.Generator().manual_seed(2))
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    w16 = w.to(tdt).view(torch.int16).numpy().view(np.uint16)
    # the planted cases are really there
    low = w.view(torch.int32) & 0xffff
    assert (low == 0x8000).any() and ((w.view(torch.int32) & 0x1fff) == 0x1000).any()
    h = w.to(torch.float16)
    assert torch.isinf(h).any() and ((h != 0) & (h.abs() < 6.1e-5)).any() and ((h == 0) & (w != 0)).any()
    assert (w.view(torch.int32) == -2 ** 31).any()
    nbytes = lib.nd_layer_packed_bytes(_lib.KIND[kind], cin, cout, _lib.DTYPE[dtype])
    KB = (cin + 15) // 16
    MT, rem = divmod(nbytes // 4, KB * taps * 256 + 32)     # (the 2x2 stride-2 transposes pad their row tiles)
    assert rem == 0 and MT * 32 >= (4 * cout if kind == "convT2s2" else cout)
    packed = torch.full((nbytes // 4,), float("nan"))
    _lib.check(lib.nd_layer_pack(_lib.KIND[kind], cin, cout, _lib.DTYPE[dtype], w.data_ptr(), b.data_ptr(), packed.data_ptr(), nbytes))
    nw = MT * KB * taps * 256
    got = packed.numpy()[:nw].view(np.uint16).reshape(MT, KB, taps, 64, 8)
    ref = _ref_pack16(kind, cin, cout, w16, MT)
    assert np.array_equal(got, ref)
    # every 16-bit slot of a row m >= M or a channel ci >= cin is zero
    M = 4 * cout if kind == "convT2s2" else cout
    lane = np.arange(64)
    m = 32 * np.arange(MT)[:, None] + (lane & 31)[None, :]                                             # [MT, 64]
    ci = 16 * np.arange(KB)[:, None, None] + 8 * (lane >> 5)[None, :, None] + np.arange(8)[None, None, :]   # [KB, 64, 8]
    pad = (m >= M)[:, None, None, :, None] | (ci >= cin)[None, :, None, :, :]
    assert not got[np.broadcast_to(pad, got.shape)].any()
    assert pad.any()
    # fp32 bias block behind the pieces (nd_bias_offset): the row's channel's bias, zeros beyond M
    bias = packed.numpy()[nw:]
    assert bias.size == MT * 32
    want = np.zeros(MT * 32, dtype=np.float32)
    want[:M] = b.numpy()[[_up_row(r, cout, 8)[2] for r in range(M)]] if kind == "convT2s2" else b.numpy()
    assert np.array_equal(bias.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------- CLI surface

def test_cli_help_names_compute_dtype_and_client_forwards_it(tmp_path, capsys):
    from nind_denoise_amd import client, denoise_dir, denoise_image
    text = " ".join(denoise_image.build_parser().format_help().split())
    assert "compute_dtype=f32|bf16|f16" in text and "only when this option is absent" in text and "PSNR" in text
    assert "compute_dtype" in denoise_dir.build_parser().format_help()
    args = denoise_image.parse_args(["--model_parameters", "funit=16,compute_dtype=bf16", "--config", "/nonexistent.yaml"])
    assert args.model_parameters == "funit=16,compute_dtype=bf16"
    # the thin client sends the argument list as it is
    sock = str(tmp_path / "s.sock")
    srv = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
    srv.bind(sock)
    srv.listen(1)
    seen = []

    def serve():
        conn, _ = srv.accept()
        with conn, conn.makefile("rwb") as f:
            seen.append(json.loads(f.readline()))
            f.write((json.dumps({"exit": 0}) + "\n").encode())
            f.flush()
    t = threading.Thread(target=serve, daemon=True)
    t.start()
    argv = ["--network", "UtNet", "--model_parameters", "funit=16,compute_dtype=bf16", "-i", "a.tif"]
    assert client.main(argv + ["--server", sock]) == 0
    t.join(timeout=10)
    srv.close()
    assert seen == [{"argv": argv, "cwd": os.getcwd()}]
