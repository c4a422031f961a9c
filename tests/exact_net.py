"""An exactly computable UtNet for the 16-bit storage modes (test infrastructure; used by test_half_exact_host.py on the CPU
and by test_half_exact.py on the GPU, so the two cannot drift).

The idea.  If every product and every partial sum of a layer is exactly representable in fp32, the fp32 accumulator holds the
exact value whatever the summation order (split-K slices, any tile shape, any MFMA grouping).  The only rounding left is the 16-bit
store, a deterministic function of that exact value, so the GPU result must equal a CPU restatement bit for bit: float64
arithmetic with ``.to(bfloat16 / float16)`` at every tensor the 16-bit executor stores.

``routed_state_dict`` builds weights for which that holds: every conv weight is 0 except "routed" entries of +-1 (one or two
terms per output sum, six in the 1x1 head), biases are dyadic and the PReLU slopes are powers of two of both signs (the kernels
compute ``acc > 0 ? acc : acc * slope`` in fp32: exact, and a negative slope is legal).  Input channels are dealt out by
permutations, so every channel of every tensor is consumed and no deep layer is a dead end.

``restate`` is the network (oracle.networks.utnet_forward, operation for operation) with the 16-bit stores made explicit.
The gates that make "bit for bit" a fair demand -- order-free exactness, no subnormal or overflowing store, roundings that
actually bite, sensitivity to a misplaced weight -- are measured by the functions at the end and asserted on the CPU.
"""
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nind_denoise_amd.synth import utnet_layer_table, utnet_prelu_keys  # noqa: E402
from oracle import tiler as otiler  # noqa: E402

FUNIT = 16                                    # the smallest funit the 16-bit path takes
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
SLOPES = (-1.0, 0.5, 2.0, -0.5)               # cycled over the 18 activation layers
INPUT_GRID = 128                              # inputs are k / INPUT_GRID, k = 0 .. INPUT_GRID
# biases are k / BIAS_GRID, |k| <= BIAS_MAX: multiples of 2^-8 up to +-2.  The grids are a compromise between three gates
# (test_half_exact_host.py): finer grids (inputs k/256, biases k/4096 up to 1/16) reach fp16 subnormals (smallest stored magnitude
# 2^-16) and push the UNROUNDED network, whose values never coarsen, past 2^24 units per sum (biases k/1024: 2^24.2); coarser
# ones (k/64) leave the fp16 store nothing to round.  Biases of the inputs' size or larger keep every level at magnitudes where
# the 11-bit fp16 significand rounds.
BIAS_GRID, BIAS_MAX = 256, 512
SEED = 20

# the cases of the GPU tests; the CPU gates run on exactly these inputs
FORWARD_SHAPES = ((2, 104, 104), (1, 104, 136), (3, 120, 120))
FRAME = dict(width=333, height=290, cs=120, ucs=88, ol=16, batch=5)


# ---------------------------------------------------------------------------- weights and inputs

def _gen(seed, key):
    g = torch.Generator()
    g.manual_seed(seed * 7919 + sum(ord(c) * (i + 1) for i, c in enumerate(key)))
    return g


def _dealt(n_slots, cin, g):
    """n_slots input channels from concatenated random permutations of range(cin): every channel is used before any repeats."""
    perms = [torch.randperm(cin, generator=g) for _ in range((n_slots + cin - 1) // cin)]
    return torch.cat(perms)[:n_slots]


def _signs(n, g):
    return torch.randint(0, 2, (n,), generator=g).double() * 2 - 1


def routed_state_dict(funit=FUNIT, seed=SEED):
    """float32 state dict with the reference's key names (loads into UtNet(funit) and drives ``restate``)."""
    sd = {}
    for key, kind, cin, cout, k in utnet_layer_table(funit):
        g = _gen(seed, key)
        w = torch.zeros((cout, cin, k, k) if kind == "conv" else (cin, cout, k, k), dtype=torch.float64)
        if key == "tconvs4.4":              # fp32 1x1 head: input channel i -> output i % 3
            s = _signs(cin, g)
            for i in range(cin):
                w[i % 3, i, 0, 0] = s[i]
        elif kind == "up":                  # every sub-position (a, b) of every output channel has its own source channel
            src = _dealt(4 * cout, cin, g)
            s = _signs(4 * cout, g)
            for slot in range(4 * cout):
                o, a, b = slot // 4, (slot // 2) % 2, slot % 2
                w[src[slot], o, a, b] = s[slot]
        elif key.startswith("tconvs") and key.endswith(".0"):    # input = cat[up, skip]: one channel of each half
            half = cin // 2
            for base in (0, half):
                src = _dealt(cout, half, g)
                taps = torch.randint(0, 9, (cout,), generator=g)
                s = _signs(cout, g)
                for o in range(cout):
                    w[base + src[o], o, taps[o] // 3, taps[o] % 3] = s[o]
        else:                               # cout >= cin: output channel o reads one input channel at one tap
            assert cout >= cin, key
            src = _dealt(cout, cin, g)
            taps = torch.randint(0, 9, (cout,), generator=g)
            s = _signs(cout, g)
            for o in range(cout):
                if kind == "conv":
                    w[o, src[o], taps[o] // 3, taps[o] % 3] = s[o]
                else:
                    w[src[o], o, taps[o] // 3, taps[o] % 3] = s[o]
        sd[key + ".weight"] = w.float()
        sd[key + ".bias"] = (torch.randint(-BIAS_MAX, BIAS_MAX + 1, (cout,), generator=g).double() / BIAS_GRID).float()
    for i, key in enumerate(utnet_prelu_keys()):
        sd[key + ".weight"] = torch.tensor([SLOPES[i % len(SLOPES)]], dtype=torch.float32)
    return sd


def grid_input(batch, h, w, seed=SEED):
    """[batch, 3, h, w] float32 on the dyadic grid k / INPUT_GRID in [0, 1]."""
    g = _gen(seed, f"x{batch}x{h}x{w}")
    return (torch.randint(0, INPUT_GRID + 1, (batch, 3, h, w), generator=g).double() / INPUT_GRID).float()


def grid_frame(width, height, seed=SEED):
    """[3, height, width] float32 numpy frame on the same grid."""
    return grid_input(1, height, width, seed + 1)[0].numpy()


# ---------------------------------------------------------------------------- the restatement

def restate(sd, x, store=None, dtype=torch.float64, trace=None):
    """UtNet.forward as the 16-bit executor computes it: oracle.networks.utnet_forward in ``dtype`` arithmetic, rounded to the
    storage type ``store`` (torch.bfloat16 / torch.float16; None: no rounding, the fp32 direct path; a callable: that store
    rule, for checking that a wrong rounding mode would be noticed) at the 23 tensors the
    executor stores: the reflection-padded input, every conv / transposed-conv output after its activation, every upN output.
    Pools and concats move stored values; the 1x1 head is fp32 and is not rounded.

    ``trace`` (list) receives one dict per stored tensor and per weighted layer: name, the layer's input / weight / bias
    (None for the padded input), the exact value before the store and the stored value.
    """
    sd = {k: v.to(dtype) for k, v in sd.items()}

    def q(name, t, src=None):
        s = t if store is None else (store(t) if callable(store) else t.to(store).to(dtype))
        if trace is not None:
            trace.append(dict(name=name, exact=t, stored=s, rounds=True, **(src or {})))
        return s

    def layer(key, t, kind, act):
        w, b = sd[key + ".weight"], sd[key + ".bias"]
        if kind == "conv":
            y = F.conv2d(t, w, b)
        elif kind == "convT":
            y = F.conv_transpose2d(t, w, b)
        else:
            y = F.conv_transpose2d(t, w, b, stride=2)
        if act is not None:
            y = torch.where(y > 0, y, y * sd[act + ".weight"])      # (F.prelu, written as the kernels compute it)
        return y, dict(x=t, w=w, b=b, kind=kind)

    def block(name, t, kind):
        y, src = layer(f"{name}.0", t, kind, f"{name}.1")
        t = q(f"{name}.0", y, src)
        y, src = layer(f"{name}.2", t, kind, f"{name}.3")
        return q(f"{name}.2", y, src)

    def up(name, t):
        y, src = layer(name, t, "up", None)
        return q(name, y, src)

    l = q("input", F.pad(x.to(dtype), (2, 2, 2, 2), mode="reflect"))
    l1 = block("convs1", l, "conv")
    l2 = block("convs2", F.max_pool2d(l1, 2), "conv")
    l3 = block("convs3", F.max_pool2d(l2, 2), "conv")
    l4 = block("convs4", F.max_pool2d(l3, 2), "conv")
    y, src = layer("bottom.0", F.max_pool2d(l4, 2), "conv", "bottom.1")
    b = q("bottom.0", y, src)
    y, src = layer("bottom.2", b, "convT", "bottom.3")
    b = q("bottom.2", y, src)
    l = torch.cat([up("up1", b), l4], dim=1)
    l = torch.cat([up("up2", block("tconvs1", l, "convT")), l3], dim=1)
    l = torch.cat([up("up3", block("tconvs2", l, "convT")), l2], dim=1)
    l = torch.cat([up("up4", block("tconvs3", l, "convT")), l1], dim=1)
    l = block("tconvs4", l, "convT")
    y, src = layer("tconvs4.4", l, "conv", None)
    if trace is not None:
        trace.append(dict(name="tconvs4.4", exact=y, stored=y, rounds=False, **src))
    return y[:, :, 2:-2, 2:-2]


_EXPECTED = {}


def expected_forward(store_name, shape):
    """Restatement of forward on grid_input(*shape) as float32 (cached: every GPU case of a shape shares it)."""
    key = (store_name, tuple(shape))
    if key not in _EXPECTED:
        y = restate(routed_state_dict(), grid_input(*shape), TDT.get(store_name))
        assert torch.equal(y.float().double(), y)
        _EXPECTED[key] = y.float()
    return _EXPECTED[key]


# ---------------------------------------------------------------------------- the frame loop

def stitch_float64(tile_outputs, grid):
    """canvas (float64) = sum over tiles of the seamless useful crops: oracle.tiler.stitch_add without its float32 casts."""
    canvas = np.zeros((3, grid.height, grid.width), dtype=np.float64)
    for i in range(grid.size):
        _, _, ud, (ax, ay) = grid.geom(i)
        t = np.array(tile_outputs[i][:, ud[1]:ud[3], ud[0]:ud[2]], dtype=np.float64, copy=True)
        t = otiler.make_seamless_edges(t, ax, ay, grid)
        canvas[:, ay:ay + t.shape[1], ax:ax + t.shape[2]] += t
    return canvas


def frame_tiles(frame, cs, ucs, ol):
    grid = otiler.TileGrid(frame.shape[2], frame.shape[1], cs, ucs, ol)
    return grid, torch.from_numpy(np.stack([otiler.gather_tile(frame, grid, i) for i in range(grid.size)]))


def expected_canvas(store_name, sd=None, dtype=torch.float64, chunk=5):
    """(canvas float64, tile outputs float64 numpy, grid) of the FRAME case through the oracle tiler and the restatement."""
    f = FRAME
    frame = grid_frame(f["width"], f["height"])
    grid, tiles = frame_tiles(frame, f["cs"], f["ucs"], f["ol"])
    sd = routed_state_dict() if sd is None else sd
    outs = torch.cat([restate(sd, tiles[i:i + chunk], TDT.get(store_name), dtype) for i in range(0, grid.size, chunk)])
    outs = outs.double().numpy()
    return stitch_float64(outs, grid), outs, grid


# ---------------------------------------------------------------------------- gate figures

def lowbit_exp(t):
    """Exponent e of the finest power of two 2^e dividing every non-zero element of a float64 tensor (None: all zero)."""
    t = t[t != 0]
    if t.numel() == 0:
        return None
    m, e = torch.frexp(t.double().abs())
    n = (m * 2.0 ** 53).to(torch.int64)                      # exact: 53-bit mantissa
    low = (n & -n).double()                                  # lowest set bit, a power of two
    return int((e.double() - 53 + torch.log2(low)).min().item())


def layer_l1(rec):
    """max over outputs of sum |x||w| + |b| of one traced layer (float64)."""
    x, w, b = rec["x"].double().abs(), rec["w"].double().abs(), rec["b"].double().abs()
    if rec["kind"] == "conv":
        y = F.conv2d(x, w, b)
    else:
        y = F.conv_transpose2d(x, w, b, stride=2 if rec["kind"] == "up" else 1)
    return y.max().item()


def exactness_log2(trace):
    """Worst log2(L1 / unit) over the weighted layers of a trace: with L1 / unit < 2^24 every partial sum, in any order, is an
    integer below 2^24 in units of ``unit`` and therefore exact in fp32.  unit = the finest power of two dividing every term:
    (finest bit of x) * (finest bit of w), or the finest bit of the bias."""
    worst, where = -math.inf, None
    for rec in trace:
        if rec.get("w") is None:
            continue
        ex, ew, eb = lowbit_exp(rec["x"]), lowbit_exp(rec["w"]), lowbit_exp(rec["b"])
        unit = min(e for e in ((ex + ew) if ex is not None and ew is not None else None, eb) if e is not None)
        v = math.log2(layer_l1(rec)) - unit
        if v > worst:
            worst, where = v, rec["name"]
    return worst, where


def stored_range(trace):
    """(smallest, largest) non-zero magnitude over the stored (rounded) tensors of a trace."""
    lo, hi = math.inf, 0.0
    for rec in trace:
        if rec["rounds"]:
            a = rec["stored"].abs()
            nz = a[a != 0]
            if nz.numel():
                lo, hi = min(lo, nz.min().item()), max(hi, nz.max().item())
    return lo, hi


def rounding_bites(trace, store_name):
    """(tensors where the store changes >= 1 % of the elements, stored tensors, exact round-to-even ties hit).  A tie is an
    fp32-exact value whose dropped bits are exactly half a unit of the stored type (valid in the type's normal range)."""
    drop = 16 if store_name == "bf16" else 13
    bites = n = ties = 0
    for rec in trace:
        if not rec["rounds"]:
            continue
        n += 1
        bites += int((rec["exact"] != rec["stored"]).double().mean().item() >= 0.01)
        bits = rec["exact"].float().contiguous().view(torch.int32)
        ties += int(((bits & ((1 << drop) - 1)) == (1 << (drop - 1))).sum())
    return bites, n, ties


def weighted_keys():
    return [key for key, *_ in utnet_layer_table(FUNIT)]


def moved_weight(sd, key, position, move):
    """A copy of ``sd`` with one routed weight of layer ``key`` moved: ``move`` = "tap" (to the neighbouring tap) or "channel"
    (to the neighbouring input channel), ``position`` = 0 | 1 | 2 for the first, middle and last routed entry.  These are the
    mistakes a fragment map makes.  None where the layer has no such neighbour (the 1x1 head has one tap)."""
    kind = {k: kd for k, kd, *_ in utnet_layer_table(FUNIT)}[key]
    w = sd[key + ".weight"].clone()
    nz = torch.nonzero(w)
    i0, i1, ky, kx = nz[(0, len(nz) // 2, len(nz) - 1)[position]].tolist()
    val = w[i0, i1, ky, kx].item()
    if move == "tap":
        if w.shape[2] * w.shape[3] == 1:
            return None
        t = (ky * w.shape[3] + kx + 1) % (w.shape[2] * w.shape[3])
        dst = (i0, i1, t // w.shape[3], t % w.shape[3])
    else:
        cin_dim = 1 if kind == "conv" else 0
        idx = [i0, i1]
        idx[cin_dim] = (idx[cin_dim] + 1) % w.shape[cin_dim]
        dst = (idx[0], idx[1], ky, kx)
    w[i0, i1, ky, kx] = 0
    w[dst] += val
    out = dict(sd)
    out[key + ".weight"] = w
    return out


def gate_figures(sd, x, store_name, chunk=5):
    """The gate figures of one input batch under one storage type (None: unrounded), accumulated over chunks of images:
    worst log2(L1 / unit) and its layer, smallest / largest stored magnitude, per stored tensor the number of elements the
    store changed and the number of elements, the tie count, whether the fp32 evaluation equals the float64 one bit for bit,
    and the float64 output."""
    fig = dict(log2=-math.inf, where=None, lo=math.inf, hi=0.0, changed={}, numel={}, ties=0, f32_equal=True, out=[])
    for i in range(0, x.shape[0], chunk):
        trace = []
        y = restate(sd, x[i:i + chunk], TDT.get(store_name), trace=trace)
        fig["f32_equal"] &= torch.equal(restate(sd, x[i:i + chunk], TDT.get(store_name), dtype=torch.float32).double(), y)
        fig["out"].append(y)
        v, where = exactness_log2(trace)
        if v > fig["log2"]:
            fig["log2"], fig["where"] = v, where
        lo, hi = stored_range(trace)
        fig["lo"], fig["hi"] = min(fig["lo"], lo), max(fig["hi"], hi)
        if store_name is not None:
            fig["ties"] += rounding_bites(trace, store_name)[2]
        for rec in trace:
            if rec["rounds"]:
                fig["changed"][rec["name"]] = fig["changed"].get(rec["name"], 0) + int((rec["exact"] != rec["stored"]).sum())
                fig["numel"][rec["name"]] = fig["numel"].get(rec["name"], 0) + rec["exact"].numel()
    fig["out"] = torch.cat(fig["out"])
    fig["bites"] = sum(fig["changed"][n] >= 0.01 * fig["numel"][n] for n in fig["numel"])
    return fig


def canvas_exactness_log2(tile_outputs, grid):
    """log2(L1 / unit) of the stitch: L1 = the canvas of |tile outputs|, unit = a quarter of the outputs' finest bit (the stitch
    weights are 1, 1/2 and 1/4)."""
    l1 = stitch_float64(np.abs(tile_outputs), grid).max()
    return math.log2(l1) - (lowbit_exp(torch.from_numpy(tile_outputs)) - 2)
