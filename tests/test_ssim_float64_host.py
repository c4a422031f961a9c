"""CPU gates of the float64 SSIM / MS-SSIM tests (tests/ssim_cases.py, tests/test_ssim_float64.py): the restatement is the oracle,
the bars are tight enough to see planted errors and nowhere wider than the cap, and the white-noise inputs of the older tests are
blind to two of those errors -- the reason the image-like regimes exist.  No GPU."""
import pytest
import torch

import ssim_cases as S
from oracle import losses as olosses

CASES = S.all_cases()
IDS = [S.case_id(*k) for k in CASES]
GATE = 10.0          # a planted error must move an asserted quantity by this many bars


def test_edge_classes():
    ids = S.class_ids(43, 59)
    assert ids.shape == (43, 59) and S.NCLASS == 121 and S.class_present(43, 59).all()
    count = torch.bincount(ids.flatten(), minlength=S.NCLASS)
    assert count[0] == 4 and count[-1] == (43 - 20) * (59 - 20) and int(count.sum()) == 43 * 59     # four corners; the interior
    assert ids[0, 0] == 0 and ids[42, 58] == 0 and ids[0, 29] == 10 and ids[21, 0] == 110 and ids[15, 16] == 120
    assert S.class_name(int(ids[3, 57])) == "(3,1)"
    assert int(S.class_present(11, 11).sum()) == 36 and int(torch.bincount(S.class_ids(11, 11).flatten())[5 * 11 + 5]) == 1
    t = torch.zeros(2, 3, 43, 59)
    t[1, 2, 42, 0], t[1, 0, 20, 30], t[0, 1, 0, 5] = -3.0, 2.0, float("nan")
    m = S.class_max(t)
    assert m[1, 0] == 3 and m[1, 120] == 2 and m[1].sum() == 5 and torch.isnan(m[0, 5]) and int(torch.isnan(m).sum()) == 1


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_restatement_is_the_oracle(key):
    """no knobs, fp32 input: the same bits as oracle/losses.py, scores and maps"""
    mode, shape, _ = key
    cs = S.case(*key)
    x, y = cs["x"], cs["y"]
    assert x.dtype == torch.float32 and 0 <= x.min() and x.max() <= 1 and 0 <= y.min() and y.max() <= 1
    x2, y2 = S.make_pair(*key)
    assert torch.equal(x, x2) and torch.equal(y, y2)                                  # deterministic
    assert torch.equal(S.taps(torch.float32), olosses.gaussian_window())
    assert torch.equal(S.taps(torch.float64), olosses.gaussian_window().double())     # the fp32-rounded taps in every dtype
    for a, b in zip(S.ssim_maps(x, y), olosses.ssim_maps(x, y)):
        assert torch.equal(a, b)
    want = (olosses.ms_ssim if mode == "msssim" else olosses.ssim)(x, y)
    assert torch.equal(S.score(mode, x, y), want) and torch.equal(cs["s32"], want)
    if mode == "msssim":
        assert torch.equal(S.ms_ssim_planes(x, y).mean(-1), want)
    print(f"{S.case_id(*key)}: float64 on float64 taps is {S.tap_distance(mode, x, y):.2e} from float64 on the fp32 taps; "
          f"R32 is {(cs['s32'].double() - cs['s64']).abs().max().item():.2e} from R64")


@pytest.mark.parametrize("key", CASES, ids=IDS)
def test_every_class_has_a_bar_under_the_cap(key):
    """from R32 alone: every class the image has gets a finite bar, none wider than CLASS_BAR_CAP; the samples whose float64
    gradient is 0 are the ones expected, and the dead plane's is 0 in both references"""
    cs = S.case(*key)
    assert torch.isfinite(cs["g64"]).all() and torch.isfinite(cs["g32"]).all()
    rep = S.grad_report(cs, cs["g32"])
    assert [r["regime"] for r in rep] == list(cs["regimes"]) and cs["regimes"][0] == key[2]
    if cs["shape"][0] > 1:
        assert len(set(cs["regimes"])) == cs["shape"][0]                               # a batch mixes regimes
    for r in rep:
        p = r["present"]
        lone_dead = r["regime"] == "dead_plane" and cs["shape"][1] == 1
        assert r["kind"] == ("abs" if r["regime"] == "identical" or lone_dead else "rel"), r["regime"]
        assert torch.isfinite(r["bar"][p]).all()
        if r["kind"] == "rel":
            worst = r["bar"][p].max().item()
            k = int(torch.where(p, r["bar"], torch.zeros_like(r["bar"])).argmax())
            print(f"{S.case_id(*key)} sample {r['sample']} {r['regime']}: widest class bar {worst:.2e} at {S.class_name(k)}, "
                  f"narrowest {r['bar'][p].min().item():.2e}")
            assert (r["bar"][p] > 0).all() and worst <= S.CLASS_BAR_CAP, (r["regime"], S.class_name(k), worst)
            assert (r["fig"][p] <= r["bar"][p]).all()                                    # R32 meets its own bar
    assert (cs["score_bar"] >= S.SCORE_FLOOR).all() and cs["score_bar"].max() <= 1e-3
    for i, regime in enumerate(cs["regimes"]):
        if regime == "identical":
            assert abs(cs["s64"][i].item() - 1) <= 1e-12 and abs(cs["s32"][i].item() - 1) <= 1e-6
    for i, ch in S.dead_planes(cs):
        planes = S.ms_ssim_planes(cs["x"].double(), cs["y"].double())
        assert planes[i, ch] == 0 and (planes[i, :ch] > 0.5).all()
        assert not cs["g64"][i, ch].any() and not cs["g32"][i, ch].any()               # torch's autograd: 0, not NaN
        assert bool(cs["g64"][i, :ch].any()) == (ch > 0)


def _moved(a, b, bar):
    """|a - b| in bars; a NaN counts as seen"""
    d = (a - b).abs() / bar
    return float("inf") if torch.isnan(d).any() else d.max().item()


def test_bars_see_planted_errors():
    """Every forward knob moves the score of at least one sample of at least one case by >= 10 bars, in each mode it applies to."""
    best = {}
    for key in CASES:
        mode = key[0]
        cs = S.case(*key)
        xd, yd = cs["x"].double(), cs["y"].double()
        for knob in S.FORWARD_KNOBS:
            if mode == "ssim" and knob in S.MS_ONLY_KNOBS:
                continue
            moved = _moved(S.score(mode, xd, yd, {knob: True}), cs["s64"], cs["score_bar"])
            if moved >= best.get((knob, mode), (-1.0, ""))[0]:
                best[(knob, mode)] = (moved, S.case_id(*key))
    print("planted error, mode: the score it moves most, in bars")
    for (knob, mode), (moved, cid) in sorted(best.items()):
        print(f"  {knob:16s} {mode:7s} {moved:10.3g}  {cid}")
    assert set(best) == {(k, m) for k in S.FORWARD_KNOBS for m in ("ssim", "msssim") if m == "msssim" or k not in S.MS_ONLY_KNOBS}
    for (knob, mode), (moved, cid) in best.items():
        assert moved >= GATE, (knob, mode, moved, cid)


def test_bars_see_a_wrong_pixel():
    """The pixel knob: g64 with one pixel replaced by 0 misses the bar of that pixel's class by >= 10x, at a corner, at an edge
    midpoint and at the seam of the 16 x 16 backward tiles.  A norm over the whole gradient sees none of the first two."""
    print("pixel replaced by 0: its class figure in bars, the same error as a share of max|g64| over the whole sample")
    for what in ("corner", "edge midpoint", "tile seam"):
        best = (-1.0, "", 0.0)
        for key in CASES:
            cs = S.case(*key)
            n, c, h, w = cs["shape"]
            py, px = {"corner": (0, 0), "edge midpoint": (0, w // 2), "tile seam": (15, 16)}[what]
            if py >= h or px >= w:
                continue
            k = int(S.class_ids(h, w)[py, px])
            for i in range(n):
                for ch in range(c):
                    g = cs["g64"].clone()
                    g[i, ch, py, px] = 0
                    r = S.grad_report(cs, g)[i]
                    if r["kind"] != "rel":
                        continue
                    bars = (r["fig"][k] / r["bar"][k]).item()
                    if bars > best[0]:
                        best = (bars, f"{S.case_id(*key)} sample {i} channel {ch} class {S.class_name(k)}",
                                (cs["g64"][i, ch, py, px].abs() / cs["g64"][i].abs().max()).item())
        print(f"  {what:14s} {best[0]:10.3g}  {best[1]}; {best[2]:.1e} of the sample's largest gradient")
        assert best[0] >= GATE, (what, best)


def test_white_noise_is_blind_to_the_luminance_term_and_the_last_scale():
    """The inputs of test_eval_harness.py (torch.rand and y = x + noise) against its bar SCORE_TOL: local variance ~0.17 dwarfs
    c2 and the local means agree, so a wrong c1, or cs in place of ss at the fifth scale, moves the score by less than the bar.
    A documented fact, and why tests/test_ssim_float64.py runs on image-like pairs."""
    from test_eval_harness import SCORE_TOL, _pair
    seen = {}
    for mode, shape, seed, noise in (("ssim", (2, 3, 64, 75), 64, 0.1), ("msssim", (1, 3, 163, 301), 301, 0.2)):
        x, y = (t.double() for t in _pair(*shape, seed=seed, noise=noise))
        ref = S.score(mode, x, y)
        for knob in S.FORWARD_KNOBS:
            if mode == "ssim" and knob in S.MS_ONLY_KNOBS:
                continue
            d = (S.score(mode, x, y, {knob: True}) - ref).abs().max().item()
            seen[(knob, mode)] = d
            print(f"white noise {mode} {S.shape_id(shape)} {knob}: the score moves by {d:.2e} (bar {SCORE_TOL:.0e})")
    assert seen[("c1_unsquared", "ssim")] < SCORE_TOL and seen[("c1_unsquared", "msssim")] < SCORE_TOL
    assert seen[("last_cs", "msssim")] < SCORE_TOL
    assert seen[("c2_unsquared", "ssim")] > SCORE_TOL                                  # what it does see
