"""CPU gates of the exactly computable UtNet (tests/exact_net.py): what makes "the 16-bit GPU result equals the restatement bit for
bit" (tests/test_half_exact.py) a fair demand and a sharp one.  Every gate runs on the very inputs of the GPU cases -- the three
forward shapes and the 20 tiles of the frame case -- for the unrounded network and both storage types.

1. Order-free exactness: per layer max L1 / unit < 2^23 (2^24 with one bit to spare), the stitch sums included, and the fp32
   evaluation equals the float64 one bit for bit.
2. No stored non-zero value is subnormal in, or beyond the finite range of, its type.
3. Rounding bites: the store changes >= 1 % of the elements in >= 12 of the 23 stored tensors, exact ties occur, and the bf16,
   f16 and unrounded outputs differ pairwise.
4. Sensitivity: one routed weight moved to the neighbouring tap, or to the neighbouring input channel, changes the output.
"""
import math

import numpy as np
import pytest
import torch

import exact_net as E

TYPES = ("bf16", "f16")
# smallest normal and largest finite magnitude
LIMITS = {"bf16": (2.0 ** -126, float(torch.finfo(torch.bfloat16).max)), "f16": (2.0 ** -14, 65504.0)}
SPARE_BITS = 1


@pytest.fixture(scope="module")
def sd():
    return E.routed_state_dict()


@pytest.fixture(scope="module")
def inputs():
    f = E.FRAME
    grid, tiles = E.frame_tiles(E.grid_frame(f["width"], f["height"]), f["cs"], f["ucs"], f["ol"])
    cases = {"x".join(map(str, s)): E.grid_input(*s) for s in E.FORWARD_SHAPES}
    cases["frame tiles"] = tiles
    return cases, grid


@pytest.fixture(scope="module")
def figures(sd, inputs):
    cases, _ = inputs
    return {(name, t): E.gate_figures(sd, x, t) for name, x in cases.items() for t in (None,) + TYPES}


def test_routing_uses_every_channel_and_every_tap(sd):
    taps = set()
    for key, kind, cin, cout, k in E.utnet_layer_table(E.FUNIT):
        w = sd[key + ".weight"]
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}, key
        cin_dim, cout_dim = (1, 0) if kind == "conv" else (0, 1)
        used_in = (w != 0).sum(dim=[d for d in range(4) if d != cin_dim])
        used_out = (w != 0).sum(dim=[d for d in range(4) if d != cout_dim])
        assert (used_in > 0).all(), f"{key}: input channel without a reader"
        terms = {"up": 4, "conv": 1, "convT": 1}[kind] * (2 if key.startswith("tconvs") and key.endswith(".0") else 1)
        if key == "tconvs4.4":
            assert used_out.tolist() == [6, 5, 5]
        else:
            assert (used_out == terms).all(), (key, used_out.unique().tolist())
        if k == 3:
            taps |= {(int(a), int(b)) for a, b in torch.nonzero(w)[:, 2:].tolist()}
        if kind == "up":
            assert ((w != 0).sum(dim=0) == 1).all(), f"{key}: a sub-position without exactly one source"
    assert len(taps) == 9
    slopes = [sd[k + ".weight"].item() for k in E.utnet_prelu_keys()]
    assert len(slopes) == 18 and set(slopes) == set(E.SLOPES)


def test_restatement_is_the_oracle_network_without_rounding(sd):
    from oracle import networks as onet
    x = E.grid_input(1, 104, 136)
    sd64 = {k: v.double() for k, v in sd.items()}
    assert torch.equal(E.restate(sd, x), onet.utnet_forward(sd64, x.double()))


def test_gate1_order_free_exactness(sd, inputs, figures, capsys):
    for t in (None,) + TYPES:
        worst = max((figures[(name, t)]["log2"], figures[(name, t)]["where"], name) for name in inputs[0])
        with capsys.disabled():
            print(f"\n[gate 1] {t or 'unrounded'}: worst log2(L1/unit) {worst[0]:.2f} at {worst[1]} ({worst[2]})")
        assert worst[0] < 24 - SPARE_BITS, worst
        for name in inputs[0]:
            assert figures[(name, t)]["f32_equal"], (name, t)
        if t is None:
            continue        # (the frame case runs in 16-bit storage only)
        # the stitch: weights 1, 1/2, 1/4 over at most four tiles
        canvas, outs, grid = E.expected_canvas(t)
        assert np.array_equal(outs, figures[("frame tiles", t)]["out"].numpy())
        log2 = E.canvas_exactness_log2(outs, grid)
        with capsys.disabled():
            print(f"[gate 1] {t or 'unrounded'}: stitch log2(L1/unit) {log2:.2f}")
        assert log2 < 24 - SPARE_BITS
        assert np.array_equal(canvas.astype(np.float32).astype(np.float64), canvas)
        # and the oracle's own fp32 loop, in launches of 3, gives the float64 canvas
        f = E.FRAME
        c32 = E.otiler.denoise_frame(E.grid_frame(f["width"], f["height"]), f["cs"], f["ucs"], f["ol"],
                                     lambda x: E.restate(sd, torch.from_numpy(x), E.TDT.get(t), torch.float32).numpy(), batch=3)
        assert c32.dtype == np.float32 and np.array_equal(c32.astype(np.float64), canvas)


@pytest.mark.parametrize("t", TYPES)
def test_gate2_stored_values_are_normal_and_finite(inputs, figures, capsys, t):
    lo = min(figures[(name, t)]["lo"] for name in inputs[0])
    hi = max(figures[(name, t)]["hi"] for name in inputs[0])
    with capsys.disabled():
        print(f"\n[gate 2] {t}: smallest stored magnitude 2^{math.log2(lo):.1f}, largest {hi:.4g}")
    assert lo >= LIMITS[t][0] and hi <= LIMITS[t][1], (lo, hi)
    for name in inputs[0]:
        assert torch.isfinite(figures[(name, t)]["out"]).all()


@pytest.mark.parametrize("t", TYPES)
def test_gate3_rounding_bites(inputs, figures, capsys, t):
    for name in inputs[0]:
        fig = figures[(name, t)]
        assert len(fig["numel"]) == 23
        with capsys.disabled():
            print(f"\n[gate 3] {t} {name}: the store changes >= 1 % of the elements in {fig['bites']} of 23 tensors, {fig['ties']} ties; "
                  f"output in [{fig['out'].min().item():.4g}, {fig['out'].max().item():.4g}], {fig['out'].unique().numel()} distinct values",
                  end="")
        assert fig["bites"] >= 12 and fig["ties"] >= 1, (name, fig["bites"], fig["ties"])
        a, b, c = fig["out"], figures[(name, None)]["out"], figures[(name, "f16" if t == "bf16" else "bf16")]["out"]
        assert not torch.equal(a, b) and not torch.equal(a, c)


def _probe_output(sd, x, t):
    return E.restate(sd, x, E.TDT[t], torch.float32)     # (the fp32 evaluation: gate 1 shows it is the float64 one)


@pytest.mark.parametrize("t", TYPES)
def test_gate4_a_moved_weight_changes_the_output(sd, capsys, t):
    shape = E.FORWARD_SHAPES[2]      # (at 104 pixels bottom.0 has ONE output pixel per image and channel)
    x = E.grid_input(*shape)
    base = _probe_output(sd, x, t)
    made = changed = 0
    silent = []
    for key in E.weighted_keys():
        for move in ("tap", "channel"):
            for position in (0, 1, 2):
                moved = E.moved_weight(sd, key, position, move)
                if moved is None:
                    assert key == "tconvs4.4" and move == "tap"      # one tap: no neighbour
                    continue
                made += 1
                if torch.equal(_probe_output(moved, x, t), base):
                    silent.append((key, move, position))
                else:
                    changed += 1
    with capsys.disabled():
        print(f"\n[gate 4] {t} forward {shape}: {changed} of {made} probes changed the output")
    assert len(E.weighted_keys()) == 23 and made == 23 * 6 - 3 and not silent, silent


@pytest.mark.parametrize("t", TYPES)
def test_gate4_a_moved_weight_changes_the_canvas(sd, capsys, t):
    base, _, _ = E.expected_canvas(t, sd, torch.float32)
    made = changed = 0
    silent = []
    for key in E.weighted_keys():
        moved = E.moved_weight(sd, key, 1, "channel" if key == "tconvs4.4" else "tap")
        made += 1
        canvas, _, _ = E.expected_canvas(t, moved, torch.float32)
        if np.array_equal(canvas, base):
            silent.append(key)
        else:
            changed += 1
    with capsys.disabled():
        print(f"\n[gate 4] {t} frame: {changed} of {made} probes changed the canvas")
    assert made == 23 and not silent, silent
