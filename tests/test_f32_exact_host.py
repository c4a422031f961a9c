"""CPU gates of the exact fp32 single-layer tests (tests/test_f32_exact.py; helpers and shape rules in tests/exact_layer.py): what
makes "the GPU equals float64 bit for bit" a fair demand on these inputs, and a sharp one.  Every gate runs on the very tensors of
the GPU cases.

1. L1 bound: for every case of the direct variants, of the exact Winograd group and of nd_layer_wgrad, log2 of the largest sum of
   magnitudes behind one result is at most 23 (2^24 with one bit to spare), so every partial sum of every order is an integer (or a
   half, after PReLU) that fp32 holds.
2. Integer weights: nd_winograd_pack, on the host, turns the weights of every exact Winograd case into integers.
3. The mirrors: the Python statement of nd_wgrad_partial_floats gives the table of part 3 of the plan, and each shape rule produces
   the nblk -+ 1 and T k +- 1 counts it claims.
4. The tests bite: on the float64 restatement, dropping the last valid pixel of an image, the last input channel, or (weight gradient)
   the last pixel of the K range changes at least one value in every case.
"""
import pytest
import torch

import exact_layer as X

BAR_LOG2 = 23.0


def _direct_cases():
    for i, V in enumerate(X.variants("f32")):
        for n, case in enumerate(X.f32_variant_shapes(V)):
            yield V, case, 1000 * i + n


def _wino_exact_cases():
    for code in X.WINO_FORMS:
        for n, case in enumerate(X.wino_cases(code)[0]):
            if X.wino_group(code, case[2]) == "exact" and not (X.WINO_FORMS[code][1] and case[2] % 16):
                yield code, case, 100 * code + n


# ---------------------------------------------------------------------------- 1. L1 bounds

def test_l1_bound_of_the_direct_variants(capsys):
    assert len(X.variants("f32")) == 22
    worst = (0.0, None)
    for V, case, seed in _direct_cases():
        kind = case[0]
        x, w, b = X._integer_layer(*case, seed=seed)
        worst = max(worst, (X.log2_of(X.direct_l1(kind, x, w, b)), (V["name"], case)))
    with capsys.disabled():
        print(f"\n[L1] fp32 direct variants: worst log2(L1) {worst[0]:.2f} at {worst[1]}")
    assert worst[0] <= BAR_LOG2, worst


def test_the_cast_to_fp32_rounds_nothing():
    """_expected_layer(..., torch.float32) is the float64 result itself (one variant's cases: the data rule is the same for all)."""
    V = X.variants("f32")[14]
    for n, case in enumerate(X.f32_variant_shapes(V)):
        kind = case[0]
        x, w, b = X._integer_layer(*case, seed=14000 + n)
        y = X._linear_layer(kind, x.double(), w.double(), b.double())
        y = torch.where(y > 0, y, y * X.SLOPE)
        assert torch.equal(X._expected_layer(kind, x, w, b, "PReLU", X.SLOPE, torch.float32).double(), y)


def test_l1_bound_of_the_exact_winograd_group(capsys):
    worst = {}
    for code, case, seed in _wino_exact_cases():
        kind, batch, cin, cout, h, w = case
        x, wt, b = X.wino_layer(code, kind, cin, cout, h, w, seed, batch)
        l1 = X.log2_of(X.wino_restate(code, kind, x, wt, b, X.SLOPE, bound=True))
        worst[code] = max(worst.get(code, (0.0, None)), (l1, case))
        # and the algorithm, restated in float64, is the plain convolution exactly
        same = torch.equal(X.wino_restate(code, kind, x, wt, b, X.SLOPE), X._expected_layer(kind, x, wt, b, "PReLU", X.SLOPE, torch.float64).double())
        assert same, (code, case)
    with capsys.disabled():
        for code, (l1, case) in sorted(worst.items()):
            print(f"\n[L1] Winograd tile code {code} (weights x {X.WINO_FORMS[code][2]}): worst log2(L1) {l1:.2f} at {case}", end="")
        print()
    assert sorted(worst) == [1, 2, 3, 4, 5]
    assert all(l1 <= BAR_LOG2 for l1, _ in worst.values()), worst


def test_l1_bound_of_wgrad(capsys):
    worst = (0.0, None)
    for n, case in enumerate(X.WGRAD_CASES):
        x, dy = X.wgrad_layer(*case, seed=n)
        assert 6 * X.wgrad_geometry(*case)["K"] < 2 ** 24
        dw, db = X.wgrad_expected(case[0], x.abs(), dy.abs())
        worst = max(worst, (X.log2_of(max(dw.max(), db.max())), case))
    with capsys.disabled():
        print(f"\n[L1] nd_layer_wgrad: worst log2(L1) {worst[0]:.2f} at {worst[1]}")
    assert worst[0] <= BAR_LOG2, worst


# ---------------------------------------------------------------------------- 2. integer transformed weights

def test_packed_winograd_weights_are_integers(capsys):
    seen = {}
    for code, case, seed in _wino_exact_cases():
        kind, batch, cin, cout, h, w = case
        _, wt, b = X.wino_layer(code, kind, cin, cout, h, w, seed, batch)
        packed = X.wino_packed(code, kind, cin, cout, wt, b)
        assert torch.isfinite(packed).all() and torch.equal(packed, packed.round()), (code, case)
        seen[code] = max(seen.get(code, 0.0), float(packed.abs().max()))
    with capsys.disabled():
        print("\n[integer weights] largest packed |U| per tile code: " + ", ".join(f"{c}: {int(v)}" for c, v in sorted(seen.items())))
    assert sorted(seen) == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("code", [3, 4])
def test_a_smaller_multiplier_leaves_fractions(code):
    """The gate above can fail: F(4,3) weights that are multiples of 12 (F(4x4): 288) only do not transform to integers."""
    kind, cin, cout = "conv3", 16, 20
    _, wt, b = X.wino_layer(code, kind, cin, cout, 8, 8, seed=1)
    packed = X.wino_packed(code, kind, cin, cout, wt / 2, b)
    assert not torch.equal(packed, packed.round())


# ---------------------------------------------------------------------------- 3. the mirrors and the shape rules

# K chunks, tiles of 64 x 64 -> (ksplit, cps) by nd_wgrad_partial_floats: 512 / tiles slices at the most, in whole chunks
SPLIT_TABLE = [
    # taps, M, N, K, chunks, ksplit, cps
    (1, 1, 3, 63, 1, 1, 1), (9, 4, 3, 35, 1, 1, 1), (9, 63, 64, 186, 3, 3, 1), (9, 65, 4, 185, 3, 3, 1), (9, 72, 4, 187, 4, 4, 1),
    (1, 65, 64, 257, 5, 5, 1), (9, 64, 3, 972, 16, 16, 1), (9, 4, 3, 1020, 17, 17, 1), (1, 63, 65, 1809, 29, 29, 1),
    (9, 4, 4, 31740, 512, 512, 1), (1, 65, 64, 16383, 256, 256, 1), (1, 65, 72, 8151, 128, 128, 1), (9, 3, 4, 32508, 525, 263, 2),
    (9, 65, 65, 7950, 129, 65, 2),
    (9, 64, 64, 4 * 138 * 138, 1229, 410, 3), (1, 128, 128, 64 * 1000, 1000, 125, 8),      # training-size layers
]
KSPLITS = {1, 3, 4, 5, 16, 17, 29, 128, 256, 512}


def test_wgrad_split_mirror():
    for taps, m, n, k, chunks, ksplit, cps in SPLIT_TABLE:
        s = X.wgrad_split(taps, m, n, k)
        assert (s["chunks"], s["ksplit"], s["cps"]) == (chunks, ksplit, cps), (taps, m, n, k, s)
        assert s["ksplit"] <= s["cap"] and (s["ksplit"] - 1) * s["cps"] < s["chunks"] <= s["ksplit"] * s["cps"]


def wgrad_seams():
    """What the cases of nd_layer_wgrad reach between them, from the mirrors."""
    seams = dict(ksplit=set(), M=set(), N=set(), k_mod=set(), caps=set(), kinds=set())
    flags = set()
    for case in X.WGRAD_CASES:
        kind, batch, cin, cout, h, w = case
        g = X.wgrad_geometry(*case)
        s = X.wgrad_split(g["taps"], g["M"], g["N"], g["K"])
        seams["ksplit"].add(s["ksplit"])
        seams["M"].add(g["M"])
        seams["N"].add(g["N"])
        seams["kinds"].add(kind)
        if s["ksplit"] == s["cap"]:
            seams["caps"].add(s["cap"])
        if g["K"] > s["PC"]:
            seams["k_mod"].add({0: "PC n", 1: "PC n + 1", s["PC"] - 1: "PC n - 1"}.get(g["K"] % s["PC"]))
        oh, ow = {"conv3": (h - 2, w - 2), "convT3": (h + 2, w + 2), "convT2s2": (2 * h, 2 * w), "conv1": (h, w)}[kind]
        flags |= {name for name, hit in (
            ("below PC", g["K"] < s["PC"]), ("odd last chunk", s["last_chunk"] % 2 == 1 and s["chunks"] > 1),
            ("reduce wave without a slice", s["ksplit"] == 3), ("short last slice", s["last_slice"] < s["cps"]),
            ("reduce tail", (g["taps"] * g["M"] * g["N"]) % 64 != 0), ("two repitch blocks", 128 < g["gw"] < 256 and g["gw"] % 128 != 0),
            ("odd convT2s2", kind == "convT2s2" and h % 2 == 1 and w % 2 == 1), ("db below 256", oh * ow < 256),
            ("db 257", oh * ow == 257), ("cout % 4", cout % 4 != 0), ("two tiles", s["tiles"] == 2), ("four tiles", s["tiles"] == 4)) if hit}
    return seams, flags


def test_wgrad_cases_reach_every_seam(capsys):
    seams, flags = wgrad_seams()
    with capsys.disabled():
        print(f"\n[wgrad] ksplit values reached: {sorted(seams['ksplit'])}; M {sorted(seams['M'])}; N {sorted(seams['N'])}")
    assert seams["ksplit"] >= KSPLITS, KSPLITS - seams["ksplit"]
    assert seams["caps"] == {512, 256, 128}
    assert seams["M"] >= {1, 3, 4, 63, 64, 65, 72} and seams["N"] >= {1, 3, 4, 63, 64, 65, 72}
    assert seams["k_mod"] >= {"PC n", "PC n + 1", "PC n - 1"}, seams["k_mod"]
    assert seams["kinds"] == {"conv3", "convT3", "convT2s2", "conv1"}
    assert flags == {"below PC", "odd last chunk", "reduce wave without a slice", "short last slice", "reduce tail", "two repitch blocks",
                     "odd convT2s2", "db below 256", "db 257", "cout % 4", "two tiles", "four tiles"}, flags


def test_direct_shape_rules_produce_the_counts_they_claim():
    for V in X.variants("f32"):
        cases = X.f32_variant_shapes(V)
        pixels = {X.valid_pixels(kind, h, w) for kind, _, _, h, w in cases}
        assert {V["nblk"] - 1, V["nblk"] + 1} <= pixels, (V["name"], pixels)
        widths = {w - 2 if kind == "conv3" else w + 2 if kind == "convT3" else w // 2 if kind == "conv2s2" else w for kind, _, _, _, w in cases}
        assert all(wv % 8 for wv in widths), (V["name"], widths)
        m = {(4 if V["up"] else 1) * cout for _, _, cout, _, _ in cases}
        assert m == {V["mblk"] - (16 if V["up"] else 4), V["mblk"] + (16 if V["up"] else 4)}
        kblocks = {(cin + 7) // 8 for _, cin, _, _, _ in cases}
        assert kblocks == {1, 4 * V["kbc"] + 1, V["kbc"], 5 * V["kbc"]}
        assert (3 in {cin for _, cin, _, _, _ in cases}) == (V["taps"] == 9)


@pytest.mark.parametrize("code", sorted(X.WINO_FORMS))
def test_winograd_shape_rules_produce_the_counts_they_claim(code):
    T, two_d, _ = X.WINO_FORMS[code]
    cases, claims = X.wino_cases(code)
    outs = {((h - 2, w - 2) if kind == "conv3" else (h + 2, w + 2)) for kind, _, _, _, h, w in cases}
    assert set(claims["sizes"]) <= outs
    # every residue of a tile in each direction: T k - 1, T k, T k + 1, and less than one tile
    for axis in (0, 1) if two_d else (1,):
        sizes = {s[axis] for s in claims["sizes"]}
        assert {s % T for s in sizes if s > T} >= {T - 1, 0, 1} and min(sizes) < T, (code, axis, sizes)
    if not two_d:
        assert {65, 66, 67} <= {wv + 2 for _, wv in outs}       # bordered rows (outputs + 2 for either kind) around 64 + 2
    assert {"conv3", "convT3"} == {c[0] for c in cases}
    assert any(c[1] == X.BATCH for c in cases)
    for rule, counts in claims.items():
        if rule == "sizes":
            continue
        want = None
        if rule.startswith("gemm"):
            want = tuple(int(v) for v in rule.split()[1].split("x"))
        reached = {X.wino_tiles(code, batch, kind, h, w) for kind, batch, cin, cout, h, w in cases if want is None or (cin, cout) == want}
        assert set(counts) <= reached, (code, rule, counts, sorted(reached))
    if two_d:
        f32 = X.variants("f32")
        # the four 1-tap GEMM variants of nd_conv_variant_gemm and the automatic choice are all reached, each at nblk -+ 1
        assert {X.gemm_variant(cin, cout) for cin, cout in X.GEMM_PAIRS} == {17, 18, 19, 20, 4}
        assert [f32[X.gemm_variant(*p)]["nblk"] for p in X.GEMM_PAIRS] == [256, 256, 256, 512, 512]
        assert all(f32[X.gemm_variant(*p)]["taps"] == 1 and not f32[X.gemm_variant(*p)]["up"] for p in X.GEMM_PAIRS)
        assert X.KB_ODD_PAIR[0] % 16 and any(c[2:4] == X.KB_ODD_PAIR for c in cases)
        assert any(c[3] % 4 == 0 and c[3] % 32 for c in cases)
    else:
        assert any(c[2] == 3 for c in cases) and any(((c[2] + 7) // 8) % 2 for c in cases)


# ---------------------------------------------------------------------------- 4. the tests bite

def test_dropping_a_pixel_or_a_channel_changes_every_direct_case():
    for V, case, seed in _direct_cases():
        x, w, _ = X._integer_layer(*case, seed=seed)
        for what in ("pixel", "channel"):
            assert X.dropped_part_changes(case[0], x, w, what), (V["name"], case, what)


def test_dropping_a_pixel_or_a_channel_changes_every_winograd_case():
    for code in X.WINO_FORMS:
        for n, (kind, batch, cin, cout, h, w) in enumerate(X.wino_cases(code)[0]):
            x, wt, _ = X.wino_layer(code, kind, cin, cout, h, w, 100 * code + n, batch)
            for what in ("pixel", "channel"):
                assert X.dropped_part_changes(kind, x, wt, what), (code, kind, batch, cin, cout, h, w, what)


def test_dropping_the_last_pixel_changes_every_weight_gradient():
    """The last pixel of the K range that carries data: the last pixel of the last image of operand A (dy for Conv2d, x for the
    transposed kinds; for the 1-tap kinds that is pixel K - 1 itself, the one the `2 s + h < npix` mask of the last chunk lets in)."""
    for n, case in enumerate(X.WGRAD_CASES):
        kind = case[0]
        x, dy = X.wgrad_layer(*case, seed=n)
        dw, db = X.wgrad_expected(kind, x, dy)
        x2, dy2 = x.clone(), dy.clone()
        (dy2 if kind in ("conv3", "conv1") else x2)[-1, :, -1, -1] = 0
        dw2, _ = X.wgrad_expected(kind, x2, dy2)
        assert not torch.equal(dw, dw2), case
        dy3 = dy.clone()
        dy3[-1, :, -1, -1] = 0
        assert not torch.equal(db, X.wgrad_expected(kind, x, dy3)[1]), case
