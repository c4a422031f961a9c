"""bf16 / fp16 storage held to exact results on the GPU: no tolerance anywhere in this file.

Inputs for which every product and every partial sum is exact in fp32 leave the 16-bit store as the only rounding, so the HIP
result must equal a float64 restatement with ``.to(bfloat16 / float16)`` at every stored tensor bit for bit -- in any summation
order, split-K slices and every tile shape included.

* The whole UtNet(16) with routed +-1 weights (tests/exact_net.py; its CPU gates are tests/test_half_exact_host.py): forward at
  three shapes under every split-K / fused-pool / packer combination, and the fused frame loop against the oracle tiler.
* Every 16-bit conv_qp variant through nd_layer_forward at its tile edges on dense small integers: valid-pixel counts of
  nblk -+ 1 per image at a row width that is no multiple of 8, batch 3 (tiles cross image seams where the launcher lets them),
  cout one step below and above mblk, cin of one K block and of a K loop with a remainder, split-K on and off.
"""
import itertools

import pytest
import torch

from nind_denoise_amd import _lib, pipeline

import exact_net as E
from exact_layer import _expected_layer, _integer_layer, _layer_forward, _mismatch, _pixel_grids, variants

pytestmark = pytest.mark.gpu

TYPES = ("bf16", "f16")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.load()
    return torch.device("cuda:0")


def _net(dev, dtype):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=E.FUNIT)
    net.load_state_dict(E.routed_state_dict())
    return net.eval().to(dev).set_compute_dtype(dtype)


def _forward_abi(net, x):
    """nd_utnet_forward_hw as UtNet.forward calls it, into an output prefilled with NaN."""
    batch, h, w = x.size(0), x.size(2), x.size(3)
    y = torch.full_like(x, float("nan"))
    with torch.cuda.device(x.device):
        blob = net.packed_weights(x.device)
        ws = net.workspace(h, batch, x.device, width=w)
        _lib.check(_lib.load().nd_utnet_forward_hw(net.funit, _lib.ACT[net.activation], _lib.DTYPE[net.compute_dtype], net.flags,
                                                   blob.data_ptr(), x.data_ptr(), y.data_ptr(), batch, h, w, ws.data_ptr(), ws.numel(),
                                                   _lib.stream_ptr(x.device)), "nd_utnet_forward_hw")
        torch.cuda.synchronize()
    return y.cpu()


# ---------------------------------------------------------------------------- the whole network

@pytest.mark.parametrize("shape", E.FORWARD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", TYPES)
def test_forward_is_the_restatement(dev, dtype, shape):
    want = E.expected_forward(dtype, shape)
    x = E.grid_input(*shape).to(dev)
    net = _net(dev, dtype)
    for on_device, split_k, fused_pool in itertools.product((True, False), repeat=3):
        if net.pack_on_device != on_device:
            net.pack_on_device = on_device
            net._packed.clear()
        net.split_k, net.fused_pool = split_k, fused_pool
        got = _forward_abi(net, x)
        same = torch.equal(got, want)         # (a plain bool: pytest must not render the tensors)
        assert same, f"{dtype} {shape} device-packed={on_device} split_k={split_k} fused_pool={fused_pool}: {_mismatch(got, want)}"
    got = net(x).cpu()                        # the module's own call
    same = torch.equal(got, want)
    assert same, _mismatch(got, want)


def test_fp32_direct_forward_is_the_unrounded_restatement(dev):
    """Same weights, fp32 storage, direct convolution on every 3x3 layer (the Winograd forms transform with non-dyadic
    fractions and are not part of this: tests/test_f32_exact.py holds them exactly on weights that are multiples of the denominators)."""
    shape = E.FORWARD_SHAPES[0]
    want = E.expected_forward(None, shape)
    net = _net(dev, "f32")
    net.winograd = False
    for split_k in (True, False):
        net.split_k = split_k
        got = _forward_abi(net, E.grid_input(*shape).to(dev))
        same = torch.equal(got, want)
        assert same, f"split_k={split_k}: {_mismatch(got, want)}"


@pytest.mark.parametrize("dtype", TYPES)
def test_frame_loop_is_the_restatement(dev, dtype):
    f = E.FRAME
    canvas, _, grid = E.expected_canvas(dtype)
    assert grid.size == 20
    want = torch.from_numpy(canvas).float()
    assert torch.equal(want.double(), torch.from_numpy(canvas))          # the expected canvas is fp32-exact
    img = torch.from_numpy(E.grid_frame(f["width"], f["height"])).to(dev)
    net = _net(dev, dtype)
    # launches of 5 (four whole ones) and of 3 (the last one holds two tiles)
    for batch, (useful_only, split_k) in itertools.product((f["batch"], 3), itertools.product((True, False), repeat=2)):
        net.useful_only, net.split_k = useful_only, split_k
        got = pipeline.denoise_frame(net, img, f["cs"], f["ucs"], f["ol"], batch=batch).cpu()
        same = torch.equal(got, want)
        assert same, f"{dtype} batch={batch} useful_only={useful_only} split_k={split_k}: {_mismatch(got, want)}"


# ---------------------------------------------------------------------------- every 16-bit variant at its tile edges

KBLOCK = 16      # input channels per K block in 16-bit storage


def _variants(dtype):
    return variants(dtype)


def _variant_shapes(V):
    """(kind, cin, cout, H, W) of every case of one variant, by rule (module docstring)."""
    kinds = {9: ("conv3", "convT3"), 1: ("conv1",), 4: ("conv2s2",)}[V["taps"]] if not V["up"] else ("convT2s2",)
    # cout one 16-channel step below / above mblk; a 2x2 stride-2 transpose has M = 4 * cout rows (one 8-channel plane = 32 rows)
    couts = (V["mblk"] // 4 - 8, V["mblk"] // 4 + 8) if V["up"] else (V["mblk"] - 16, V["mblk"] + 16)
    # one K block and 4 * kbc + 1 blocks (a remainder against kbc; the launcher refuses it for kbc > 1), and for kbc > 1 the same
    # in whole chunks: one chunk and five
    kblocks = sorted({1, 4 * V["kbc"] + 1, V["kbc"], 5 * V["kbc"]})
    cases = []
    for kind in kinds:
        for hv, wv in _pixel_grids(V["nblk"], kind):
            h, w = {"conv3": (hv + 2, wv + 2), "convT3": (hv - 2, wv - 2), "conv1": (hv, wv), "conv2s2": (2 * hv, 2 * wv),
                    "convT2s2": (hv, wv)}[kind]
            cases += [(kind, kb * KBLOCK, cout, h, w) for kb in kblocks for cout in couts]
    return cases


_RAN = {}       # (dtype, variant index in its group) -> [shapes run, shapes refused]


def _run_variant(dev, dtype, i):
    if (dtype, i) in _RAN:
        return _RAN[(dtype, i)]
    V = _variants(dtype)[i]
    tdt = E.TDT[dtype]
    ran, refused = [], []
    for n, case in enumerate(_variant_shapes(V)):
        kind = case[0]
        act = "none" if kind == "convT2s2" else "PReLU"
        x, w, b = _integer_layer(*case, seed=1000 * i + n)
        want = None
        outs = []
        for flags in (0, _lib.FLAG_NO_SPLITK):
            got = _layer_forward(dev, kind, x, w, b, act, 0.5, V["v"], dtype, flags)
            if got is None:
                break
            want = _expected_layer(kind, x, w, b, act, 0.5, tdt) if want is None else want
            same = torch.equal(got, want)
            assert same, f"{V['name']} {case} flags {flags}: {_mismatch(got, want)}"
            outs.append(got)
        if len(outs) == 2:
            same = torch.equal(outs[0], outs[1])
            assert same, f"{V['name']} {case}: split and whole differ"
            ran.append(case)
        else:
            assert not outs, f"{V['name']} {case}: refused with one flag only"
            refused.append(case)
    _RAN[(dtype, i)] = (ran, refused)
    return ran, refused


@pytest.mark.parametrize("i", range(15))
@pytest.mark.parametrize("dtype", TYPES)
def test_variant_at_its_tile_edges(dev, dtype, i):
    assert len(_variants(dtype)) == 15
    ran, refused = _run_variant(dev, dtype, i)
    print(f"{_variants(dtype)[i]['name']}: {len(ran)} shapes exact, {len(refused)} refused")
    assert len(ran) >= 2, (ran, refused)


def test_every_16bit_variant_is_covered(dev, capsys):
    counts = {}
    for dtype in TYPES:
        for i, V in enumerate(_variants(dtype)):
            counts[V["name"]] = len(_run_variant(dev, dtype, i)[0])
    covered = sum(c >= 2 for c in counts.values())
    with capsys.disabled():
        print(f"\n16-bit conv variants at two or more shapes: {covered} of {len(counts)} "
              f"({min(counts.values())} .. {max(counts.values())} shapes each, {sum(counts.values())} in all)")
    assert len(counts) == 30 and covered == 30, {n: c for n, c in counts.items() if c < 2}


# the five deep, few-tile shapes of SPLIT_CASES (test_hip_parity.py) with cin <= 256 and cout in proportion: fewer tiles than
# CUs, so K is split -- in both types (the fp16 split-K tail and k_split_finish's 16-bit stores)
SPLIT_SHAPES = [
    ("conv3", 30, 256, 512, 5, 5, "PReLU"),
    ("convT3", 30, 256, 256, 3, 3, "PReLU"),
    ("convT3", 6, 256, 128, 10, 10, "PReLU"),
    ("convT2s2", 8, 256, 128, 5, 5, "none"),
    ("conv1", 3, 256, 32, 9, 9, "none"),
]


@pytest.mark.parametrize("case", SPLIT_SHAPES, ids=lambda c: "-".join(str(v) for v in c))
@pytest.mark.parametrize("dtype", TYPES)
def test_split_k_tail_is_exact(dev, dtype, case):
    kind, B, cin, cout, H, W, act = case
    x, w, b = _integer_layer(kind, cin, cout, H, W, seed=77, batch=B)
    want = _expected_layer(kind, x, w, b, act, 0.5, E.TDT[dtype])
    for flags in (0, _lib.FLAG_NO_SPLITK):
        got = _layer_forward(dev, kind, x, w, b, act, 0.5, -1, dtype, flags)
        assert got is not None
        same = torch.equal(got, want)
        assert same, f"{case} flags {flags}: {_mismatch(got, want)}"
