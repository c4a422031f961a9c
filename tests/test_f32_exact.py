"""fp32 single layers held to exact results on the GPU at their tile edges: the direct conv variants, the Winograd forms and the
weight gradient.  No tolerance anywhere in this file except the bar of the float64 Winograd group, which is built at run time from a
CPU restatement and never from the kernel.

Inputs for which every product and every partial sum is exact in fp32 (tests/exact_layer.py; the CPU gates that prove it on the very
tensors used here are tests/test_f32_exact_host.py) leave nothing to round, so the HIP result must equal float64 bit for bit -- in
any summation order, split-K slices, K chunks and every tile shape included -- and one wrong pixel, tap, channel or slice is an exact
mismatch count.

1. All 22 fp32 conv_qp variants through nd_layer_forward, by index, split-K on and off: nblk -+ 1 valid pixels per image at a row
   width that is no multiple of 8, batch 3, cout one plane below and above mblk, K loops of one block, one chunk, five chunks and a
   remainder, and the three-channel first layer.
2. nd_layer_forward_winograd.  Exact group -- tile codes 1, 2, 3, 5 and F(4x4) up to 64 channels, on weights that are multiples of
   the transform's denominators (2, 4, 24, 576): equal to the float64 plain convolution.  Float64 group -- F(6x6), whose A^T holds
   1/32 next to 32, and F(4x4) above 64 channels: max |error| against float64 within 10 x that of a torch fp32 restatement of the same
   algorithm on the same case (10 x: the upper end of the 3 ... 10 x this suite records for MFMA fma chains over torch fp32,
   test_train_exact_points.py); where the restatement is itself exact the bar is 0 and the case counts as exact.  Shapes: partial
   tiles in both directions, tile counts one below and above the transform blocks and the GEMM's nblk, every branch of
   nd_conv_variant_gemm, conv3 and convT3, batch 3.
3. nd_layer_wgrad at its seams (exact_layer.WGRAD_CASES): dw and db, prefilled with NaN, equal float64 autograd.

Measured on an MI355X: 294 direct shapes, 83 Winograd shapes and 18 weight-gradient cases exact; float64 group: F(6x6) worst GPU error /
restatement error 1.47 over 22 shapes, F(4x4) at 128 and 512 channels exact (the restatement is, so the bar is 0); the file runs in 4.4 s.
"""
import pytest
import torch

from nind_denoise_amd import _lib

import exact_layer as X

pytestmark = pytest.mark.gpu

RESTATEMENT_FACTOR = 10.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.load()
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------- 1. every fp32 direct variant at its tile edges

_RAN = {}       # variant index in the fp32 list -> [shapes run, shapes refused]


def _run_variant(dev, i):
    if i in _RAN:
        return _RAN[i]
    V = X.variants("f32")[i]
    ran, refused = [], []
    for n, case in enumerate(X.f32_variant_shapes(V)):
        kind = case[0]
        act = "none" if kind == "convT2s2" else "PReLU"
        x, w, b = X._integer_layer(*case, seed=1000 * i + n)
        want = None
        outs = []
        for flags in (0, _lib.FLAG_NO_SPLITK):
            got = X._layer_forward(dev, kind, x, w, b, act, X.SLOPE, V["v"], "f32", flags)
            if got is None:
                break
            want = X._expected_layer(kind, x, w, b, act, X.SLOPE, torch.float32) if want is None else want
            same = torch.equal(got, want)         # (a plain bool: pytest must not render the tensors)
            assert same, f"{V['name']} {case} flags {flags}: {X._mismatch(got, want)}"
            outs.append(got)
        if len(outs) == 2:
            same = torch.equal(outs[0], outs[1])
            assert same, f"{V['name']} {case}: split and whole differ"
            ran.append(case)
        else:
            assert not outs, f"{V['name']} {case}: refused with one flag only"
            refused.append(case)
    _RAN[i] = (ran, refused)
    return ran, refused


@pytest.mark.parametrize("i", range(22))
def test_variant_at_its_tile_edges(dev, i):
    assert len(X.variants("f32")) == 22
    ran, refused = _run_variant(dev, i)
    print(f"{X.variants('f32')[i]['name']}: {len(ran)} shapes exact, {len(refused)} refused")
    assert len(ran) >= 2, (ran, refused)


def test_every_fp32_variant_is_covered(dev, capsys):
    counts = {V["name"]: len(_run_variant(dev, i)[0]) for i, V in enumerate(X.variants("f32"))}
    covered = sum(c >= 2 for c in counts.values())
    with capsys.disabled():
        print(f"\nfp32 conv variants at two or more shapes: {covered} of {len(counts)} "
              f"({min(counts.values())} .. {max(counts.values())} shapes each, {sum(counts.values())} in all)")
    assert len(counts) == 22 and covered == 22, {n: c for n, c in counts.items() if c < 2}


# ---------------------------------------------------------------------------- 2. the Winograd forms at their tile edges

_WINO = {}      # tile code -> dict(exact=[cases], f64=[cases], refused=[cases], ratio=worst GPU error / restatement error)


def _run_winograd(dev, code):
    if code in _WINO:
        return _WINO[code]
    res = dict(exact=[], f64=[], refused=[], ratio=0.0)
    for n, case in enumerate(X.wino_cases(code)[0]):
        kind, batch, cin, cout, h, w = case
        x, wt, b = X.wino_layer(code, kind, cin, cout, h, w, 100 * code + n, batch)
        outs = []
        for flags in (0, _lib.FLAG_NO_SPLITK):
            got = X.wino_forward(dev, code, kind, x, wt, b, "PReLU", X.SLOPE, flags)
            if got is None:
                break
            outs.append(got)
        if len(outs) != 2:
            assert not outs, f"tile code {code} {case}: refused with one flag only"
            res["refused"].append(case)
            continue
        want = X._expected_layer(kind, x, wt, b, "PReLU", X.SLOPE, torch.float64).double()
        bar = 0.0
        if X.wino_group(code, cin) == "f64":
            restated = X.wino_restate(code, kind, x, wt, b, X.SLOPE, torch.float32)
            assert restated.dtype == torch.float32
            base = (restated.double() - want).abs().max().item()
            bar = RESTATEMENT_FACTOR * base
        for flags, got in zip((0, _lib.FLAG_NO_SPLITK), outs):
            if bar == 0.0:
                same = torch.equal(got.double(), want)
                assert same, f"tile code {code} {case} flags {flags}: {X._mismatch(got.double(), want)}"
            else:
                finite = bool(torch.isfinite(got).all())
                err = (got.double() - want).abs().max().item()
                print(f"tile code {code} {case} flags {flags}: GPU error {err:.3e}, fp32 restatement {base:.3e}, ratio {err / base:.2f}")
                res["ratio"] = max(res["ratio"], err / base)
                assert finite and err <= bar, f"tile code {code} {case} flags {flags}: error {err:.3e} above {RESTATEMENT_FACTOR:g} x {base:.3e}"
        res["exact" if bar == 0.0 else "f64"].append(case)
    _WINO[code] = res
    return res


@pytest.mark.parametrize("code", sorted(X.WINO_FORMS))
def test_winograd_form_at_its_tile_edges(dev, code):
    res = _run_winograd(dev, code)
    print(f"tile code {code}: {len(res['exact'])} shapes exact, {len(res['f64'])} within the float64 bar (worst ratio {res['ratio']:.2f}), "
          f"{len(res['refused'])} refused")
    ran = res["exact"] + res["f64"]
    assert {"conv3", "convT3"} == {c[0] for c in ran}
    # only what the launch code refuses by its own rule: a three-pass form at Cin % 16 != 0
    assert all(X.WINO_FORMS[code][1] and c[2] % 16 for c in res["refused"]), res["refused"]
    assert len(res["refused"]) == (1 if X.WINO_FORMS[code][1] else 0)


def test_winograd_coverage(dev, capsys):
    with capsys.disabled():
        print()
        for code in sorted(X.WINO_FORMS):
            res = _run_winograd(dev, code)
            print(f"Winograd tile code {code}: {len(res['exact'])} shapes exact, {len(res['f64'])} in the float64 group"
                  + (f" (worst GPU error / fp32 restatement error {res['ratio']:.2f})" if res["f64"] else "") + f", {len(res['refused'])} refused")
    for code in (1, 2, 3, 5):
        assert not _WINO[code]["f64"]
    assert _WINO[6]["f64"] and _WINO[4]["exact"]


# ---------------------------------------------------------------------------- 3. nd_layer_wgrad at its seams

@pytest.mark.parametrize("n", range(len(X.WGRAD_CASES)), ids=lambda n: "-".join(str(v) for v in X.WGRAD_CASES[n]))
def test_weight_gradient_is_exact(dev, n):
    case = X.WGRAD_CASES[n]
    x, dy = X.wgrad_layer(*case, seed=n)
    dw64, db64 = X.wgrad_expected(case[0], x, dy)
    dw, db = X.wgrad_forward(dev, case[0], x, dy)
    for got, want, what in ((dw, dw64, "dw"), (db, db64, "db")):
        assert torch.equal(want.float().double(), want)          # the expectation is fp32-exact
        same = torch.equal(got, want.float())
        assert same, f"{case} {what}: {X._mismatch(got, want.float())}"


def test_weight_gradient_cases_reach_every_split(capsys):
    """The ksplit values the launcher computes for these cases (mirror of nd_wgrad_partial_floats, held to the launch code's tables in
    test_f32_exact_host.py): 1, 3 (reduce waves without a slice), 4, 5, 16, 17 and 29 (both loops of k_wgrad_reduce) and the caps."""
    reached = set()
    for case in X.WGRAD_CASES:
        g = X.wgrad_geometry(*case)
        reached.add(X.wgrad_split(g["taps"], g["M"], g["N"], g["K"])["ksplit"])
    with capsys.disabled():
        print(f"\nnd_layer_wgrad: ksplit values reached {sorted(reached)}")
    assert reached >= {1, 3, 4, 5, 16, 17, 29, 128, 256, 512}
