"""Host side of UNet under autograd (no GPU): the new exports and the flat parameter layout, the refusals that need no device, the
conditioned setup of test_unet_grad.py (its margins, and torch's own fp32 autograd against the float64 reference), and the gate that
shows what the GPU bars can see."""
import ctypes
import importlib.util
import os

import pytest
import torch

from nind_denoise_amd import _lib, synth


def _load(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    spec = importlib.util.spec_from_file_location("_unet_grad_host_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load("test_unet_grad.py")
f64 = G.f64

NEW_EXPORTS = ("nd_unet_param_count", "nd_unet_param_range", "nd_unet_grad_blob_bytes", "nd_unet_grad_workspace_bytes",
               "nd_unet_grad_workspace_init", "nd_unet_grad_forward", "nd_unet_grad_backward")

# (shape, planted, find_noise) of every crop case the GPU file asserts bars on, and the frame cases by index
CROP_CASES = [(s, False, False) for s in G.SMALL_SHAPES] + [((2, 17, 31), False, True), ((3, 33, 47), True, False)]


def _cid(c):
    return "x".join(str(v) for v in c[0]) + ("-planted" if c[1] else "") + ("-find_noise" if c[2] else "")


# ---------------------------------------------------------------------------- ABI
def test_version_and_exports():
    lib = _lib.load()
    assert lib.nd_version() >= 117
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and hasattr(lib, name), name


def test_param_ranges_tile_the_flat_buffer_in_state_dict_order():
    lib = _lib.load()
    sd = synth.make_unet_state_dict(0)
    keys = [k for k in sd if not k.endswith("num_batches_tracked")]
    n = lib.nd_unet_num_tensors()
    assert [lib.nd_unet_tensor_name(i).decode() for i in range(n)] == keys
    at = 0
    for i, k in enumerate(keys):
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        assert lib.nd_unet_param_range(i, off, cnt) == 0
        assert (off.value, cnt.value) == (at, sd[k].numel()), k
        at += cnt.value
    assert at == lib.nd_unet_param_count() == sum(sd[k].numel() for k in keys)
    for bad in (-1, n):
        assert lib.nd_unet_param_range(bad, None, None) != 0
    assert lib.nd_unet_grad_blob_bytes() > lib.nd_unet_packed_bytes(_lib.ND_F32)


def test_workspace_refusals():
    lib = _lib.load()
    for h, w, b in ((15, 16, 1), (16, 15, 1), (16, 16, 0), (8, 64, 2)):
        assert lib.nd_unet_grad_workspace_bytes(h, w, b) == 0
        with pytest.raises(ValueError, match="too small"):
            _lib.check(lib.nd_unet_grad_workspace_init(None, 0, h, w, b, None))
    assert lib.nd_unet_grad_workspace_bytes(16, 16, 256) > 0 and lib.nd_unet_grad_workspace_bytes(16, 16, 257) == 0
    small, large = lib.nd_unet_grad_workspace_bytes(16, 16, 1), lib.nd_unet_grad_workspace_bytes(16, 16, 2)
    assert lib.nd_unet_workspace_bytes(16, 16, 1, _lib.ND_F32) < small < large     # a partial launch fits the whole launch's buffer
    with pytest.raises(MemoryError):
        _lib.check(lib.nd_unet_grad_workspace_init(None, 0, 16, 16, 1, None))


def test_module_refusals_without_a_device():
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    net = UNet()
    with pytest.raises(RuntimeError, match="HIP path only"):
        net.eval()(torch.zeros(1, 3, 16, 16, requires_grad=True))
    assert net.grad_flags == 0 and UNet(find_noise=True).grad_flags == _lib.FLAG_FIND_NOISE
    net.split_k = False
    assert net.grad_flags == _lib.FLAG_NO_SPLITK


# ---------------------------------------------------------------------------- the setup
def test_graph_restatement_is_the_float64_network():
    sd = f64._sd64(G.SEED)
    x = f64._input(G.SEED, (2, 17, 31)).double()
    with torch.no_grad():
        want = f64._decode64(sd, f64._encode64(sd, x))
        assert torch.equal(G.forward_graph(sd, x), want)
        assert torch.equal(G.forward_graph(sd, x, find_noise=True), x - want)
    assert [G.fixups(*s[1:]) for s in G.SMALL_SHAPES] == [[], [1, 2, 3, 4], [1, 2, 3, 4], [1, 2], []]
    assert G.fixups(90, 90) == [1, 3] and G.fixups(96, 96) == []
    names = [k for k in synth.make_unet_state_dict(0) if G.is_parameter(k)]
    assert {G.klass(k) for k in names} == set(G.BARS) - {"dx"}
    assert sum(G.klass(k) == "up_w" for k in names) == 4 and sum(G.klass(k) == "bn_w" for k in names) == 18
    assert sum(G.klass(k) == "conv_w" for k in names) == 19


def test_least_shift():
    v = torch.tensor([-1e-3, -1e-5, 2e-5, 2e-4], dtype=torch.float64)
    s = G._least_shift(v, G.KINK_MARGIN)
    assert (v + s).abs().min().item() >= G.KINK_MARGIN and abs(s) <= 5.1e-5
    assert G._least_shift(torch.tensor([1.0, -1.0], dtype=torch.float64), G.KINK_MARGIN) == 0.0
    z = torch.zeros(5, dtype=torch.float64)                      # a zero BatchNorm weight and bias: every value the same
    assert (z + G._least_shift(z, G.KINK_MARGIN)).abs().min().item() >= G.KINK_MARGIN


@pytest.mark.parametrize("case", CROP_CASES, ids=_cid)
def test_conditioning_holds_both_margins(case):
    shape, planted, _ = case
    seed = G.SHAPE_SEED.get(shape, G.SEED)
    x = f64._input(seed, shape)
    raw = f64._sd(seed, planted)
    sd, rep = G.conditioned(raw, x)
    print(f"UNet grad setup {_cid(case)}: {rep}")
    assert rep["kink"] >= G.KINK_MARGIN and rep["pool"] >= G.POOL_MARGIN and rep["max_shift"] <= 2e-4
    changed = [k for k in sd if not torch.equal(sd[k], raw[k])]
    assert all(G.klass(k) == "bn_b" for k in changed) and all(v.dtype == raw[k].dtype for k, v in sd.items())
    before = G.margins(f64._sd64(seed, planted), x.double())
    assert before["kink"] < G.KINK_MARGIN                       # the shift was needed


# ---------------------------------------------------------------------------- torch's own fp32 against the reference
# worst figure per class over the crop cases, as this test prints it, rounded up.  A crop bar more than ~30x its class' figure would mean
# a bug or a missed kink (FRAME_BARS[1]: a pool maximum that fp32 orders the other way, see test_unet_grad.py)
CPU_FP32 = {"dx": 7.5e-7, "conv_w": 2.7e-6, "conv_b": 1.7e-6, "bn_w": 1.1e-6, "bn_b": 1.1e-6, "up_w": 1.1e-6, "up_b": 2.1e-6}


@pytest.mark.parametrize("case", CROP_CASES, ids=_cid)
def test_cpu_fp32_autograd_is_near_float64(case):
    shape, planted, find_noise = case
    sd, x, target, y64, dx64, g64 = G.crop_case(shape, planted, find_noise)
    y, _, dx, grads = G.reference(sd, x, target, find_noise, dtype=torch.float32)
    fig = G.class_figures(dx, grads, dx64, g64)
    G._show(f"{_cid(case)} torch fp32 on the CPU", fig)
    assert (y.double() - y64).abs().max().item() <= G.BAR_UNET_FWD
    for c, (v, k) in fig.items():
        assert v <= CPU_FP32[c], (c, k, v)
        assert G.BARS[c] <= 30 * CPU_FP32[c]


# ---------------------------------------------------------------------------- the gate
# Classes that cannot see an error by construction: the gradient entering a pool flows to the encoder above it only, and the gradient
# leaving up1's transpose to down4 and, through the pools, the encoder -- neither reaches a transpose.  Their figure is exactly 0.
BLIND = {(c, k) for c in ("up_w", "up_b") for k in ("d1", "d2", "d3", "d4", "u1")}
GATE_CASES = CROP_CASES + [("frame", i) for i in range(len(G.FRAME_CASES))]


def _gate_setup(case):
    if case[0] == "frame":
        seed, geom = G.FRAME_CASES[case[1]]
        W, H, cs, ucs, ol, batch = geom
        from oracle import tiler as otiler
        grid = otiler.TileGrid(W, H, cs, ucs, ol)
        frame = f64._frame(geom)
        mid = (grid.rows // 2) * grid.cols + grid.cols // 2
        x = torch.stack([torch.from_numpy(otiler.gather_tile(frame, grid, i).copy()) for i in (0, mid)])   # a corner and a middle tile
        sd, _ = G.conditioned(f64._sd(seed), x, pool_margin=None)
        return sd, x, torch.rand(x.shape, generator=torch.Generator().manual_seed(5)), False
    shape, planted, find_noise = case
    sd, x, target = G.crop_case(shape, planted, find_noise)[:3]
    return sd, x, target, find_noise


@pytest.mark.parametrize("case", GATE_CASES, ids=lambda c: f"frame{c[1]}" if c[0] == "frame" else _cid(c))
def test_bars_see_backward_errors(case):
    sd, x, target, find_noise = _gate_setup(case)
    bars = G.FRAME_BARS[case[1]] if case[0] == "frame" else G.BARS
    h, w = x.shape[2:]
    knobs = {}
    p = {k: (v.double().requires_grad_(G.is_parameter(k)) if v.is_floating_point() else v) for k, v in sd.items()}
    xr = x.double().requires_grad_()
    loss = torch.nn.functional.mse_loss(G.forward_graph(p, xr, find_noise=find_noise, knobs=knobs), target.double())
    names = [k for k in p if G.is_parameter(k)]

    def grads():
        g = torch.autograd.grad(loss, [xr] + [p[k] for k in names], retain_graph=True)
        return g[0], dict(zip(names, g[1:]))

    dx0, g0 = grads()
    errors = [(f"d{n}", 1.01) for n in (1, 2, 3, 4)] + [(f"u{n}", 1.01) for n in (1, 2, 3, 4)] + [(f"fix{n}", True) for n in G.fixups(h, w)]
    for key, val in errors:
        knobs.clear()
        knobs[key] = val
        dx1, g1 = grads()
        fig = G.class_figures(dx1, g1, dx0, g0)
        print(f"UNet grad gate {case} {key}: " + ", ".join(f"{c} {v:.2e}" for c, (v, _) in sorted(fig.items())))
        for c, (v, k) in fig.items():
            if (c, key) in BLIND:
                assert v == 0.0, (c, key, v)
            else:
                assert v >= 10 * bars[c], (key, c, k, v, bars[c])
    assert not any(c in ("dx", "conv_w") for c, _ in BLIND)
