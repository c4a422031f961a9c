"""test_adam_exact.py without a device: k_adam and k_adam_guarded (csrc/optim.hip) restated in numpy fp32, on the inputs, the float64
reference and the bars of that file (loaded with importlib).

  * the restatement, with the bias corrections taken in double as the launchers take them, meets BAR_M, BAR_V, BAR_U and the exact
    checks on every one-step case, plain and behind a binding scale: inputs and bars can be met by a correct fp32 implementation;
  * with the launchers' former fp32 `1 - powf(b, step)` it exceeds BAR_U at steps 2 and 3 (numpy's fp32 power stands in for powf);
  * the input classes have the sizes the bars need to bite;
  * a gate of mistakes, each applied to the restatement, exceeds its bar 10x on at least one case;
  * torch.optim.Adam in fp32 on the CPU against the float64 trajectory gives the figures TRAJ_BARS are 3x of."""
import importlib.util
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def _load(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    spec = importlib.util.spec_from_file_location("_adam_exact_" + name[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _load("test_adam_exact.py")
U = T.U
f32 = np.float32


# ---------------------------------------------------------------------------- the kernels in numpy fp32
def _fma(a, b, c):
    """fp32 fma: the product of two fp32 values is exact in double; the sum rounds to double and then to fp32 (a double rounding only
    where the double lands on an fp32 tie, one ulp and far inside the bars)"""
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(f32)


def restate(g, m, v, vmax, p, lr, beta1, beta2, eps, step, amsgrad, scale=None, bc="double", knob=None):
    """k_adam (scale None) or k_adam_guarded with ok = 1, rounding for rounding: the first moment is fma(1 - b1, g, b1 m), everything
    else one fp32 operation at a time in the order the kernels write.  bc: "double" = the launchers' 1.0 - pow((double)b, step)
    rounded to fp32, "fp32" = their former 1.f - powf(b, (float)step).  knob: one of MISTAKES."""
    lr, b1, b2, eps = f32(lr), f32(beta1), f32(beta2), f32(eps)
    s1 = step + {"bc1 at step + 1": 1, "bc1 at step - 1": -1}.get(knob, 0)
    s2 = step + {"bc2 at step + 1": 1, "bc2 at step - 1": -1}.get(knob, 0)
    with np.errstate(all="ignore"):
        if bc == "double":
            bc1, bc2 = f32(1.0 - float(b1) ** s1), f32(1.0 - float(b2) ** s2)
        else:
            bc1, bc2 = f32(1) - np.power(b1, f32(s1)), f32(1) - np.power(b2, f32(s2))
        assert bc1.dtype == bc2.dtype == f32
        g, m, v, p = (np.asarray(a, dtype=f32) for a in (g, m, v, p))
        gm = gv = g if scale is None else g * f32(scale)
        if knob == "guarded: scale on the first moment only":
            gv = g
        if knob == "guarded: scale on the finished update":
            gm = gv = g
        one_b1, one_b2 = f32(1) - b1, f32(1) - b2
        keep, take = (one_b1, b1) if knob == "b1 and 1 - b1 swapped" else (b1, one_b1)
        mi = _fma(take, gm, keep * m)
        vi = b2 * v + (one_b2 * gv if knob == "g for g^2" else one_b2 * gv * gv)
        vmax_out, vd = vmax, vi
        if amsgrad or knob == "vmax written with amsgrad off":
            top = np.fmax(np.asarray(vmax, dtype=f32), vi)                 # fmaxf: a NaN operand loses
            vmax_out = top
            if amsgrad:
                vd = top
        if knob == "denominator from v' under a larger vmax":
            vd = vi
        if knob == "vmax stored bias-corrected" and amsgrad:
            vmax_out = vd / bc2
        root = np.sqrt(vd)
        if knob == "bc2 without the square root":
            denom = root / bc2 + eps
        elif knob == "eps inside the square root":
            denom = np.sqrt(vd / bc2 + eps)
        elif knob == "(sqrt(v) + eps) / sqrt(bc2)":
            denom = (root + eps) / np.sqrt(bc2)
        else:
            denom = root / np.sqrt(bc2) + eps
        upd = (lr if knob == "bc1 dropped" else lr / bc1) * mi / denom
        if knob == "guarded: scale on the finished update":
            upd = upd * f32(scale)
        out = SimpleNamespace(m=mi, v=vi, vmax=np.asarray(vmax_out, dtype=f32), p=p - upd)
    assert all(a.dtype == f32 for a in (out.m, out.v, out.vmax, out.p))
    return out


MISTAKES = ["bc1 at step + 1", "bc1 at step - 1", "bc2 at step + 1", "bc2 at step - 1", "bc2 without the square root", "bc1 dropped",
            "eps inside the square root", "(sqrt(v) + eps) / sqrt(bc2)", "denominator from v' under a larger vmax",
            "vmax stored bias-corrected", "vmax written with amsgrad off", "b1 and 1 - b1 swapped", "g for g^2",
            "guarded: scale on the first moment only", "guarded: scale on the finished update"]


def binding_scale(g):
    """the fp32 scale of a guard with max_norm = 0.25 |g|, from the float64 restatement of its coefficient"""
    norm = math.sqrt(float((np.asarray(g, dtype=np.float64) ** 2).sum()))
    return f32(T.clip_scale64(g, 0.25 * norm))


def one_step(case, scale=None, **kw):
    """The restatement on a one-step case from p = 0: the figures of test_adam_exact (with "vmax": the relative distance of the stored
    vmax from max(vmax_in, v_out), infinite for a buffer that amsgrad off should have left alone) and its bars."""
    n, amsgrad, step, beta1 = case
    inp = T.inputs(n, step, beta1)
    vmax_in = inp.vmax if amsgrad else T.nan_pattern(n)
    out = restate(inp.g, inp.m, inp.v, vmax_in, np.zeros(n, dtype=f32), T.LR, beta1, T.BETA2, T.EPS, step, amsgrad, scale=scale, **kw)
    g_ref = inp.g if scale is None else T.scaled_gradient(inp.g, scale)
    ref = T.adam64(g_ref, inp.m, inp.v, inp.vmax, T.LR, beta1, T.BETA2, T.EPS, step, amsgrad)
    fig = T.figures(out.m, out.v, -out.p, ref)
    if amsgrad:
        want = np.maximum(inp.vmax, out.v).astype(np.float64)
        fig["vmax"] = T._worst(np.abs(out.vmax.astype(np.float64) - want), want)
    else:
        fig["vmax"] = 0.0 if np.array_equal(T.bits(out.vmax), T.bits(vmax_in)) else float("inf")
    bars = {"m": T.BAR_M, "v": T.BAR_V + (T.GUARD_EXTRA_V if scale is not None else 0), "u": T.BAR_U + (T.GUARD_EXTRA_U if scale is not None else 0)}
    return inp, out, fig, bars


# ---------------------------------------------------------------------------- the cases themselves
def test_cases_cover_what_the_bars_need():
    assert {c[0] for c in T.ONE_STEP} == set(T.NS) and {c[3] for c in T.ONE_STEP} == set(T.BETA1S)
    for step in T.STEPS:
        assert {c[1] for c in T.ONE_STEP if c[2] == step} == {True, False}
    for n in T.NS:
        assert len({c[2] for c in T.ONE_STEP if c[0] == n}) >= 2


@pytest.mark.parametrize("case", T.ONE_STEP, ids=T.case_id)
def test_class_sizes(case):
    n, amsgrad, step, beta1 = case
    inp = T.inputs(n, step, beta1)
    assert T.inputs(n, step, beta1) is inp                                  # computed once, shared, read-only
    assert not inp.g.flags.writeable
    if n == 1:
        assert inp.cls[0] == T.ORDINARY
        return
    b1 = T.widen(beta1)
    share = {}
    for mode in (True, False):
        ref = T.adam64(inp.g, inp.m, inp.v, inp.vmax, T.LR, beta1, T.BETA2, T.EPS, step, mode)
        root = np.sqrt(ref.vd / ref.bc2)
        at_eps = (root >= 0.1 * T.widen(T.EPS)) & (root <= 10 * T.widen(T.EPS))
        share[f"eps-scale, amsgrad {mode}"] = at_eps.mean()
        assert at_eps[inp.cls == T.EPS_SCALE].all()
    live = inp.cls != T.AT_REST
    share["amsgrad binds"] = (live & (inp.vmax.astype(np.float64) > ref.v)).mean()
    share["amsgrad does not bind"] = (live & (inp.vmax.astype(np.float64) < ref.v)).mean()
    for k in (T.ORDINARY, T.EPS_SCALE, T.CANCELLING, T.AT_REST):
        share[f"class {k}"] = (inp.cls == k).mean()
    print(f"adam exact classes {T.case_id(case)}: " + ", ".join(f"{k} {x:.3f}" for k, x in share.items()))
    assert share["amsgrad binds"] >= 0.2 and share["amsgrad does not bind"] >= 0.2
    assert share["eps-scale, amsgrad True"] >= 0.05 and share["eps-scale, amsgrad False"] >= 0.05
    assert share[f"class {T.CANCELLING}"] >= 0.1 and share[f"class {T.AT_REST}"] >= 0.1
    c = inp.cls == T.CANCELLING
    t1, t2 = b1 * inp.m[c].astype(np.float64), (1.0 - b1) * inp.g[c].astype(np.float64)
    assert (t1 * t2 < 0).all() and (np.abs(np.abs(t1 / t2) - 1.0) <= 0.01 + 1e-6).all()
    r = inp.cls == T.AT_REST
    assert not (inp.g[r].any() or inp.m[r].any() or inp.v[r].any() or inp.vmax[r].any()) and np.signbit(inp.p[r]).any()


# ---------------------------------------------------------------------------- the restatement against the bars
@pytest.mark.parametrize("case", T.ONE_STEP, ids=T.case_id)
def test_restatement_meets_the_bars(case):
    n, amsgrad, step, beta1 = case
    for scale in (None, binding_scale(T.inputs(n, step, beta1).g)):
        inp, out, fig, bars = one_step(case, scale=scale)
        print(T.show(f"numpy fp32 {T.case_id(case)}" + ("" if scale is None else f" scale {scale:.4f}"), fig))
        assert fig["m"] <= bars["m"] and fig["v"] <= bars["v"] and fig["u"] <= bars["u"] and fig["vmax"] == 0.0, {k: x / U for k, x in fig.items()}
        assert np.array_equal(T.bits(out.vmax), T.bits(np.maximum(inp.vmax, out.v) if amsgrad else T.nan_pattern(n)))
        # from a random p: one fp32 subtraction ends the kernel; the elements at rest keep their bits
        again = restate(inp.g, inp.m, inp.v, inp.vmax if amsgrad else T.nan_pattern(n), inp.p, T.LR, beta1, T.BETA2, T.EPS, step, amsgrad,
                        scale=scale)
        rest = inp.cls == T.AT_REST
        assert np.array_equal(T.bits(again.p)[~rest], T.bits(inp.p + out.p)[~rest])
        assert np.array_equal(T.bits(again.p)[rest], T.bits(inp.p)[rest])


def test_fp32_bias_correction_misses_the_update_bar():
    """1 - powf(b, step) in fp32 cancels at small steps: bc2 at step 2 carries the spacing of 0.998, 1e-5 of itself"""
    seen = set()
    for case in T.ONE_STEP:
        fig = one_step(case, bc="fp32")[2]
        print(T.show(f"numpy fp32, fp32 bias correction, {T.case_id(case)}", fig))
        assert fig["m"] <= T.BAR_M and fig["v"] <= T.BAR_V                  # (the moments do not see it)
        if case[2] in (2, 3):
            assert fig["u"] > T.BAR_U, (case, fig["u"] / U)
            seen.add(case)
        elif case[2] == 1 or case[2] >= 1000:                               # 1 - b is exact; b^1000 is small beside 1
            assert fig["u"] <= T.BAR_U
    assert len(seen) == 4


# ---------------------------------------------------------------------------- the gate
def test_bars_see_adam_mistakes():
    """Each mistake, over every case it applies to: the largest figure / bar.  vmax is an exact check (bar 0): a mistake it sees must
    move it by at least 10 u, ten roundings, so that no last-bit accident counts."""
    for knob in MISTAKES:
        best = (0.0, None, None)
        for case in T.ONE_STEP:
            if knob.endswith("step - 1") and case[2] == 1:                  # step 0 is not a step the ABI takes
                continue
            scale = binding_scale(T.inputs(case[0], case[2], case[3]).g) if knob.startswith("guarded") else None
            _, _, fig, bars = one_step(case, scale=scale, knob=knob)
            for k, x in fig.items():
                factor = x / (bars[k] if k in bars else U)
                if factor > best[0]:
                    best = (factor, k, case)
        factor, k, case = best
        print(f"adam exact gate, {knob}: {factor:.3g} x the bar of {k} ({T.case_id(case) if case else None})")
        assert factor >= 10.0, (knob, best)


# ---------------------------------------------------------------------------- torch's fp32 Adam over the trajectory
def torch_trajectory(amsgrad, scales):
    g_all, _ = T.trajectory_gradients()
    p = torch.zeros(T.TRAJ_N, dtype=torch.float32, requires_grad=True)
    opt = torch.optim.Adam([p], lr=T.widen(T.TRAJ_LR), betas=(T.widen(T.TRAJ_BETA1), T.widen(T.BETA2)), eps=T.widen(T.EPS), amsgrad=amsgrad)
    for t in range(T.TRAJ_STEPS):
        g = g_all[t] if scales is None else T.scaled_gradient(g_all[t], scales[t])
        p.grad = torch.from_numpy(np.array(g, dtype=f32))
        opt.step()
    st = opt.state[p]
    return SimpleNamespace(m=st["exp_avg"].numpy(), v=st["exp_avg_sq"].numpy(), p=p.detach().numpy(),
                           vmax=st["max_exp_avg_sq"].numpy() if amsgrad else None)


def test_trajectory_bars_are_three_times_torch_fp32():
    g_all, max_norm = T.trajectory_gradients()
    scales = [f32(T.clip_scale64(g_all[t], max_norm)) for t in range(T.TRAJ_STEPS)]
    clipped = sum(s < 1 for s in scales)
    assert 8 <= clipped <= T.TRAJ_STEPS - 8 and min(scales) > 0.5, (clipped, min(scales))
    mags = np.abs(g_all.astype(np.float64)).mean(axis=0)
    assert mags.min() < 1e-5 and mags.max() > 0.1
    worst = {}
    for amsgrad, guarded in T.TRAJ_RUNS:
        ref = T.trajectory64(amsgrad, scales if guarded else None)
        assert ref.path.max() > 0.5 * T.TRAJ_STEPS * T.TRAJ_LR              # sign-like steps: the path is most of steps x lr
        fig = T.trajectory_figures(torch_trajectory(amsgrad, scales if guarded else None), ref, amsgrad)
        print(f"adam exact trajectory, torch fp32 on the CPU, amsgrad {amsgrad} guarded {guarded}: " + ", ".join(f"{k} {x:.3e}" for k, x in fig.items()))
        for k, x in fig.items():
            worst[k] = max(worst.get(k, 0.0), x)
    print("adam exact trajectory, torch fp32 on the CPU, worst: " + ", ".join(f"{k} {x:.3e}" for k, x in worst.items()))
    assert set(worst) == set(T.TRAJ_CPU_FP32) == set(T.TRAJ_BARS)
    for k, x in worst.items():
        assert T.TRAJ_BARS[k] == 3 * T.TRAJ_CPU_FP32[k]
        assert math.isclose(x, T.TRAJ_CPU_FP32[k], rel_tol=0.02), (k, x, T.TRAJ_CPU_FP32[k])      # elementwise fp32: the same on every run
