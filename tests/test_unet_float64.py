"""UNet (nd_unet_forward, nd_unet_denoise_frame) against float64, with weights that keep every level visible in the output.

CPU: a gate proving that the GPU bars below can see a 1 % error on the input of every `down` block (d1 ... d4), on the output of every
`up` transpose (u1 ... u4), and a stale (non-zero) F.pad fix-up line, at every shape, seed and kept crop the GPU tests use.  GPU:
UNet.forward at the smallest, odd and batched sizes, through a re-created workspace, into a NaN-filled output, with find_noise and with
planted BatchNorm statistics packed on the device and on the host; the frame loop (split-K and useful regions on and off) and the
generic gather -> forward -> stitch path against the oracle's tiler run with the float64 network."""
import functools

import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth

# ---------------------------------------------------------------------------- visible weights and the bars they support
# With synth's weights the `up` transposes shrink what comes from below: a 1 % error on the input of down4 or the output of up1.up
# moves the output by 7e-5 at 96x96 and by 2e-6 at 16x16, far under the suite's 1e-3 bar.  At VISIBLE_UP_GAIN = 3 every level moves
# the output by >= 1.4e-4 at every shape below while the pre-sigmoid range stays within about [-4.7, 3.2] (no saturation); the gate
# test does not force another value.
VISIBLE_UP_GAIN = 3.0

# fp32 bars of the GPU tests on max |y - float64|; outputs are sigmoids (find_noise: x - sigmoid), so the scale is 1.
# test_gpu_bars_see_every_level_and_fixup requires each to be 10x below what the errors listed above do to the kept output of every
# case that asserts it.  Worst values measured on MI355X in the comments; torch fp32 on the CPU against float64 gives at most 1.4e-6
# on the same forward shapes.
# The bars are about 3x the worst measured value (re-association between launch shapes and split-K plans).  The gate caps
# BAR_UNET_FWD at 1.6e-5 (u1 at 16x16, 1.6e-4) and BAR_UNET_FRAME at 3.5e-4 (d1 at cs 90, 3.5e-3).
BAR_UNET_FWD = 4e-6        # UNet.forward vs float64, every forward test (measured 1.48e-6 at 256x256; <= 1.04e-6 at the small shapes)
BAR_UNET_FRAME = 1e-5      # frame canvas vs the float64 tiler (measured 4.11e-6 with the split-K tail off: the 4608 ... 9216-term sums
#                            of the deep layers run as one fp32 chain; 1.13e-6 with it on and on the generic path)

# (B, h, w) of the forward tests.  16x16: the smallest size accepted, the level-4 tensor is one pixel; 17x31: fix-ups at up1 ... up4 in
# w and at up4 in h, level 4 again 1x1; 33x47: all four fix-ups, the batch stride through odd buffers; 100x92: up1 in w, up2 in both;
# 64x16: one side at the minimum.
SMALL_SHAPES = [(1, 16, 16), (2, 17, 31), (3, 33, 47), (2, 100, 92), (1, 64, 16)]
ODD_SHAPES = [(2, 17, 31), (3, 33, 47), (2, 100, 92)]           # the shapes with a fix-up line
LARGE_SHAPE = (1, 256, 256)
FWD_CASES = [(seed, False, s) for s in SMALL_SHAPES for seed in (0, 3)] + [(0, False, LARGE_SHAPE)]
PLANTED_CASE = (3, True, (3, 33, 47))
# (weights seed, (W, H, cs, ucs, ol, batch)): odd cs = odd tensors at two levels inside the fused loop (fix-ups at up1 and up3); even
FRAME_CASES = [(3, (210, 160, 90, 61, 7, 4)), (0, (200, 170, 96, 64, 8, 5))]


def visible_unet_sd(seed, gain=VISIBLE_UP_GAIN):
    """synth.make_unet_state_dict(seed) with up1.up.weight ... up4.up.weight multiplied by gain; everything else as it is."""
    sd = synth.make_unet_state_dict(seed)
    for n in (1, 2, 3, 4):
        sd[f"up{n}.up.weight"] = sd[f"up{n}.up.weight"] * gain
    return sd


def _sd(seed, planted=False):
    """The visible weights; planted: every BatchNorm with negative and zero weights (no tiny variances: they blow the activations up)."""
    sd = visible_unet_sd(seed)
    if planted:
        for k in list(sd):
            if k.endswith(".running_var"):
                w = k[:-len("running_var")] + "weight"
                sd[w][0::7] *= -1.0
                sd[w][3::11] = 0.0
    return sd


def _sd64(seed, planted=False):
    return {k: v.double() if v.is_floating_point() else v for k, v in _sd(seed, planted).items()}


def _input(seed, shape):
    b, h, w = shape
    return torch.rand((b, 3, h, w), generator=torch.Generator().manual_seed(1000 * seed + 7 * h + w + b))


def _frame(geom):
    W, H = geom[:2]
    return synth.make_frame(W, H, seed=W + H)


# ---------------------------------------------------------------------------- the float64 network with hooks
def _double_conv64(sd, p, x):
    for k in (0, 3):
        x = F.conv2d(x, sd[f"{p}.{k}.weight"], sd[f"{p}.{k}.bias"], padding=1)
        x = F.batch_norm(x, sd[f"{p}.{k + 1}.running_mean"], sd[f"{p}.{k + 1}.running_var"], sd[f"{p}.{k + 1}.weight"],
                         sd[f"{p}.{k + 1}.bias"], training=False, eps=1e-5)
        x = F.relu(x)
    return x


def _encode64(sd, x, d=(1.0, 1.0, 1.0, 1.0)):
    """inc and down1 ... down4 outputs; the pooled input of down<n> scaled by d[n - 1]."""
    skips = [_double_conv64(sd, "inc.conv.conv", x)]
    for n in (1, 2, 3, 4):
        skips.append(_double_conv64(sd, f"down{n}.mpconv.1.conv", F.max_pool2d(skips[-1], 2) * d[n - 1]))
    return skips


def _decode64(sd, skips, u=(1.0, 1.0, 1.0, 1.0), stale=None):
    """up1 ... up4, outc, sigmoid; the output of up<n>.up scaled by u[n - 1].  stale: {n: (rows, cols)} -- the F.pad fix-up line of
    up<n> along that axis holds a copy of its neighbour (a stale, non-zero line) and not zeros."""
    t = skips[4]
    for n, skip in zip((1, 2, 3, 4), (skips[3], skips[2], skips[1], skips[0])):
        up = F.conv_transpose2d(t, sd[f"up{n}.up.weight"], sd[f"up{n}.up.bias"], stride=2) * u[n - 1]
        dy, dx = skip.size(2) - up.size(2), skip.size(3) - up.size(3)
        assert dy in (0, 1) and dx in (0, 1)
        sy, sx = (stale or {}).get(n, (False, False))
        ry, rx = (dy if sy else 0), (dx if sx else 0)
        if ry or rx:
            up = F.pad(up, (0, rx, 0, ry), mode="replicate")
        up = F.pad(up, (0, dx - rx, 0, dy - ry))
        t = _double_conv64(sd, f"up{n}.conv.conv", torch.cat([skip, up], dim=1))
    return torch.sigmoid(F.conv2d(t, sd["outc.conv.weight"], sd["outc.conv.bias"]))


def _level_sizes(n):
    s = [n]
    for _ in range(4):
        s.append(s[-1] // 2)
    return s


def _line_reaches_kept(size, n, crop):
    """Along one axis of length `size`: can the fix-up line of up<n> (the last line of its concat half) move an output line kept
    in [crop, size - crop)?  A padding-1 double conv spreads a set of lines by 2 on each side, clipped to the tensor; the next 2x2
    stride-2 transpose, written at offset 0, maps input lines [a, b) to output lines [2a, 2b)."""
    sizes = _level_sizes(size)
    lvl = 4 - n                                   # up1 writes level 3 (size / 8), up4 level 0
    a, b = sizes[lvl] - 1, sizes[lvl]
    while True:
        a, b = max(0, a - 2), min(sizes[lvl], b + 2)
        if lvl == 0:
            return a < size - crop and b > crop
        a, b, lvl = 2 * a, 2 * b, lvl - 1


def _sensitivity(sd, x, crop):
    """max |change| of the kept output (the tile less `crop` on each side) under each modelled error.  Returns (figures, notes):
    figures d1 ... d4, u1 ... u4 and fix<n> for every up<n> whose fix-up line the kept region can reach; notes name the other levels."""
    from oracle import networks as onet
    h, w = x.shape[2:]

    def kept(y):
        return y[:, :, crop:h - crop, crop:w - crop]

    def one(i):
        s = [1.0] * 4
        s[i] = 1.01
        return s

    skips = _encode64(sd, x)
    y = _decode64(sd, skips)
    assert torch.equal(y, onet.unet_forward(sd, x))           # the restatement above is the oracle's network
    fig, notes = {}, []
    for i in range(4):
        fig[f"d{i + 1}"] = (kept(_decode64(sd, _encode64(sd, x, d=one(i)))) - kept(y)).abs().max().item()
    for i in range(4):
        fig[f"u{i + 1}"] = (kept(_decode64(sd, skips, u=one(i))) - kept(y)).abs().max().item()
    hs, ws = _level_sizes(h), _level_sizes(w)
    for n in (1, 2, 3, 4):
        lvl = 4 - n
        dy, dx = hs[lvl] - 2 * hs[lvl + 1], ws[lvl] - 2 * ws[lvl + 1]
        if not (dy or dx):
            notes.append(f"up{n}: no fix-up")
            continue
        ry, rx = bool(dy) and _line_reaches_kept(h, n, crop), bool(dx) and _line_reaches_kept(w, n, crop)
        if ry or rx:
            fig[f"fix{n}"] = (kept(_decode64(sd, skips, stale={n: (ry, rx)})) - kept(y)).abs().max().item()
        if (dy and not ry) or (dx and not rx):
            # derived out of reach: a stale line there must leave the kept output exactly as it is
            out = (bool(dy) and not ry, bool(dx) and not rx)
            assert torch.equal(kept(_decode64(sd, skips, stale={n: out})), kept(y)), (n, out)
            notes.append(f"up{n}: fix-up line ({'rows' if out[0] else ''}{'+' if all(out) else ''}{'cols' if out[1] else ''}) "
                         f"out of reach of the kept region")
    return fig, notes


def _gate_input(case):
    seed, planted, kind, what, crop, bars = case
    if kind == "fwd":
        return _input(seed, what).double()
    from oracle import tiler as otiler
    W, H, cs, ucs, ol, _ = what
    grid = otiler.TileGrid(W, H, cs, ucs, ol)
    assert grid.pad == crop
    return torch.from_numpy(otiler.gather_tile(_frame(what), grid, (grid.rows // 2) * grid.cols + grid.cols // 2))[None].double()


# (weights seed, planted BatchNorm, "fwd" / "frame", shape / geometry, kept crop, bars of the GPU tests that run it)
GATE_CASES = ([(seed, planted, "fwd", shape, 0, (BAR_UNET_FWD,)) for seed, planted, shape in FWD_CASES + [PLANTED_CASE]] +
              [(seed, False, "frame", g, (g[2] - g[3]) // 2, (BAR_UNET_FRAME,)) for seed, g in FRAME_CASES])


def _gate_id(c):
    return "seed{}{}-{}-{}-crop{}".format(c[0], "-planted" if c[1] else "", c[2], "x".join(str(v) for v in c[3]), c[4])


@pytest.mark.parametrize("case", GATE_CASES, ids=_gate_id)
def test_gpu_bars_see_every_level_and_fixup(case):
    seed, planted, kind, what, crop, bars = case
    with torch.no_grad():
        fig, notes = _sensitivity(_sd64(seed, planted), _gate_input(case), crop)
    print(f"UNet gain {VISIBLE_UP_GAIN} {_gate_id(case)}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()) +
          f"; min {min(fig.values()):.2e}; " + "; ".join(notes))
    assert set(fig) >= {f"{a}{n}" for a in "du" for n in (1, 2, 3, 4)}
    for k, v in fig.items():
        assert v >= 10 * max(bars), (k, v, bars)


def test_fixup_reach_restatement():
    # cs 90 kept [14, 76): sizes 90, 45, 22, 11, 5 pad at up1 (10 -> 11) and up3 (44 -> 45); only up1's line reaches the kept region
    assert [_line_reaches_kept(90, n, 14) for n in (1, 3)] == [True, False]
    assert all(_line_reaches_kept(s, n, 0) for s in (17, 31, 33, 47, 92, 100) for n in (1, 2, 3, 4))
    sd = visible_unet_sd(1)
    ref = synth.make_unet_state_dict(1)
    for k in ref:
        up = k.endswith(".up.weight")
        assert torch.equal(sd[k], ref[k] * VISIBLE_UP_GAIN if up else ref[k]), k
    assert sum(k.endswith(".up.weight") for k in ref) == 4


# ---------------------------------------------------------------------------- GPU
@pytest.fixture
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _net(dev, seed, planted=False, **attrs):
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    net = UNet(find_noise=attrs.pop("find_noise", False))
    net.load_state_dict(_sd(seed, planted))
    for k, v in attrs.items():
        setattr(net, k, v)
    return net.eval().to(dev)


@functools.lru_cache(maxsize=None)
def _ref(seed, planted, shape, find_noise=False):
    """(input, float64 output of the oracle's network), computed once per case and shared by the tests (never modified)."""
    from oracle import networks as onet
    x = _input(seed, shape)
    with torch.no_grad():
        return x, onet.unet_forward(_sd64(seed, planted), x.double(), find_noise=find_noise)


def _err(y, ref):
    y = y.double().cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all()
    return (y - ref).abs().max().item()


def _case_id(c):
    return "seed{}{}-{}".format(c[0], "-planted" if c[1] else "", "x".join(str(v) for v in c[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=_case_id)
def test_forward_vs_float64(dev, case):
    seed, planted, shape = case
    x, ref = _ref(seed, planted, shape)
    e = _err(_net(dev, seed)(x.to(dev)), ref)
    print(f"UNet gain {VISIBLE_UP_GAIN} {_case_id(case)}: forward vs float64 {e:.2e}")
    assert e <= BAR_UNET_FWD, e


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ODD_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_forward_again_through_a_recreated_workspace(dev, shape):
    # another odd shape in between: the module drops its workspace and builds one for the new shape, twice; the fix-up lines of the
    # second workspace may lie where the first one's activations were
    other = ODD_SHAPES[(ODD_SHAPES.index(shape) + 1) % len(ODD_SHAPES)]
    net = _net(dev, 3)
    x, ref = _ref(3, False, shape)
    first = net(x.to(dev))
    assert len(net._workspaces) == 1
    e_other = _err(net(_ref(3, False, other)[0].to(dev)), _ref(3, False, other)[1])
    assert len(net._workspaces) == 1 and next(iter(net._workspaces))[1:3] == other[1:]
    second = net(x.to(dev))
    e = _err(second, ref)
    print(f"UNet gain {VISIBLE_UP_GAIN} {shape} after {other}: vs float64 {e:.2e} (in between {e_other:.2e})")
    assert torch.equal(first, second)
    assert e <= BAR_UNET_FWD and e_other <= BAR_UNET_FWD, (e, e_other)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SMALL_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_forward_writes_every_output_element(dev, shape):
    # UNet.forward hands nd_unet_forward a torch.empty_like output: here it is NaN beforehand
    lib = _lib.load()
    b, h, w = shape
    net = _net(dev, 0)
    x, ref = _ref(0, False, shape)
    xd = x.to(dev)
    y = torch.full_like(xd, float("nan"))
    blob, ws = net.packed_weights(dev), net.workspace(h, w, b, dev)
    _lib.check(lib.nd_unet_forward(_lib.ND_F32, blob.data_ptr(), xd.data_ptr(), y.data_ptr(), b, h, w, ws.data_ptr(), ws.numel(),
                                   _lib.stream_ptr(dev)), "nd_unet_forward")
    torch.cuda.synchronize()
    assert torch.isfinite(y).all()
    e = _err(y, ref)
    print(f"UNet gain {VISIBLE_UP_GAIN} {shape}: NaN-prefilled output vs float64 {e:.2e}")
    assert e <= BAR_UNET_FWD, e
    assert torch.equal(y, net(xd))


@pytest.mark.gpu
def test_find_noise_vs_float64(dev):
    shape = (2, 17, 31)
    x, ref = _ref(3, False, shape, find_noise=True)
    assert not torch.equal(ref, _ref(3, False, shape)[1])
    e = _err(_net(dev, 3, find_noise=True)(x.to(dev)), ref)
    print(f"UNet gain {VISIBLE_UP_GAIN} {shape} find_noise: vs float64 {e:.2e}")
    assert e <= BAR_UNET_FWD, e


@pytest.mark.gpu
def test_planted_batchnorm_vs_float64(dev):
    seed, planted, shape = PLANTED_CASE
    x, ref = _ref(seed, planted, shape)
    on_dev = _net(dev, seed, planted, pack_on_device=True)(x.to(dev))
    on_host = _net(dev, seed, planted, pack_on_device=False)(x.to(dev))
    e_dev, e_host = _err(on_dev, ref), _err(on_host, ref)
    print(f"UNet gain {VISIBLE_UP_GAIN} {_case_id(PLANTED_CASE)}: packed on the device {e_dev:.2e}, on the host {e_host:.2e} vs float64")
    assert e_dev <= BAR_UNET_FWD and e_host <= BAR_UNET_FWD, (e_dev, e_host)
    assert torch.equal(on_dev, on_host)


# ---------------------------------------------------------------------------- GPU: frames against the float64 tiler
@functools.lru_cache(maxsize=None)
def _frame_ref(seed, geom):
    from oracle import networks as onet
    from oracle import tiler as otiler
    W, H, cs, ucs, ol, batch = geom
    sd = _sd64(seed)

    def model_fn(x):
        with torch.no_grad():
            return onet.unet_forward(sd, torch.from_numpy(x).double()).numpy()
    return otiler.denoise_frame(_frame(geom), cs, ucs, ol, model_fn, batch=batch)


FRAME_MODES = {"fused": {}, "no_splitk": {"split_k": False}, "full_tiles": {"useful_only": False},
               "no_splitk_full_tiles": {"split_k": False, "useful_only": False}, "generic": None}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FRAME_MODES))
@pytest.mark.parametrize("case", FRAME_CASES, ids=lambda c: "seed{}-{}x{}-{}-{}-{}-b{}".format(c[0], *c[1]))
def test_frame_vs_float64(dev, case, mode):
    from nind_denoise_amd import pipeline
    seed, geom = case
    W, H, cs, ucs, ol, batch = geom
    ref = _frame_ref(seed, geom)
    img = torch.from_numpy(_frame(geom)).to(dev)
    if FRAME_MODES[mode] is None:                 # gather -> UNet.forward -> stitch, the same launches
        net = _net(dev, seed)
        total = pipeline.tile_count(W, H, cs, ucs, ol)
        out = torch.zeros_like(img)
        for t0 in range(0, total, batch):
            cnt = min(batch, total - t0)
            pipeline.stitch_tiles(out, net(pipeline.gather_tiles(img, cs, ucs, ol, t0, cnt)), cs, ucs, ol, t0)
    else:
        out = pipeline.denoise_frame(_net(dev, seed, **FRAME_MODES[mode]), img, cs, ucs, ol, batch=batch)
    e = _err(out, torch.from_numpy(ref).double())
    print(f"UNet gain {VISIBLE_UP_GAIN} seed {seed} {geom} {mode}: canvas vs float64 tiler {e:.2e}")
    assert e <= BAR_UNET_FRAME, e
