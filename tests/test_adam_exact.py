"""nd_adam_step and nd_adam_step_guarded (csrc/optim.hip: k_adam, k_adam_guarded) against Adam in float64, element by element.

Reference (adam64): Adam on the fp32 inputs widened to double.  lr, beta1, beta2, eps are the fp32 values the ABI receives, widened --
that is the operation the entry point is asked to perform; bc = 1 - b ** step in float64;
    m' = b1 m + (1 - b1) g,  v' = b2 v + (1 - b2) g^2,  vd = max(vmax, v') with amsgrad else v',
    u = (lr / bc1) m' / (sqrt(vd) / sqrt(bc2) + eps),  p' = p - u.
The same figures against the Python-double betas are printed, not asserted: the cost of passing betas as `float`.

Inputs (`inputs`): every element belongs to one class, laid out with period 8 (LAYOUT) so that n = 255 already holds all of them:
  ordinary    |g|, |m| log-uniform in [1e-8, 10], random signs; v in [1e-16, 1e2]; vmax = v 10^U(-1, 1): amsgrad binds on about half
  eps-scale   sqrt(vd / bc2) within [0.1, 10] eps at the step of the case, amsgrad on or off: the placement of eps decides the update
  cancelling  b1 m and (1 - b1) g of opposite signs, magnitudes within 1 %
  at rest     g = m = v = vmax = 0: p keeps its bits (-0.0 among them) -- what UNetTrainer relies on for its running-statistics slots
No input has g^2 (1 - b2) or v below 1e-30: denormals are not under test.

Measures, with u = 2^-24 and p = 0 on entry, so that the device's update is -p_out exactly:
  m       |m_out - m_ref| <= BAR_M (|b1 m| + |(1 - b1) g|)                                      BAR_M = 4 u
  v       |v_out / v_ref - 1| <= BAR_V                                                          BAR_V = 6 u
  update  |u_out - u_ref| <= BAR_U (lr / bc1) (|b1 m| + |(1 - b1) g|) / denom_ref               BAR_U = 16 u = 9.5e-7
First-order counts of fp32 roundings, not measurements: m 3; v 5; the update m's 3, about 7 through the denominator (v's halved by the
square root, the two square roots, the quotient, the + eps, bc2 rounded to fp32) and 4 for lr / bc1, the product and the last
quotient -- with correctly rounded fp32 sqrt and division (the Makefile passes no fast-math flag).  Behind the guard with a binding
norm the reference gradient is fl32(g fl32(state[2])) with the scale the device returned; BAR_V and BAR_U gain 2 u and 1 u.

Worst figures measured on the MI355X over ONE_STEP, in units of u (this file prints them per case):
                                    m (bar 4)    v (bar 6; 8 binding)    update (bar 16; 17 binding)
  nd_adam_step                      1.78         2.36                    5.15    (n256-amsgrad-step1000-b0.75)
  guarded, scale 1                  1.78         2.36                    5.15    (the plain step's bits)
  guarded, max_norm = 0.25 |g|      1.80         2.49                    3.95
  against Python-double betas       4.98         218                     115     (printed only: 0.999f is 0.999 (1 + 1.3e-8), so 1 - b2 is
                                                                                  off by 1.3e-5 of itself; 0.75 and 0.5 are exact, 0.9 is not)
Every figure equals the numpy fp32 restatement's of test_adam_exact_host.py to the digits printed.  With the launchers' former fp32
`1 - powf(b, step)` the same device gave an update of 60.3 u and 57.6 u at step 2, 56.3 u and 55.0 u at step 3, 22.6 u and 22.7 u at
step 7 (those six cases failed, plain and guarded), 6.2 u and 8.5 u at step 30; m and v were the same.

Exact: vmax with amsgrad == max(vmax_in, v_out) on the device's own v_out, bit for bit; without amsgrad the buffer (NaNs with a
payload) keeps its bits and a null pointer is accepted; for a random p_in, p_out == fl32(p_in + p_out_from_zero) bit for bit (one
fp32 subtraction ends the kernel); g, and the guard's state, are not written.

tests/test_adam_exact_host.py restates both kernels in numpy fp32 without a device: the restatement meets these bars on the same
inputs, the launchers' former fp32 bias correction misses BAR_U at steps 2 and 3, and every mistake of a gate exceeds them 10x."""
import functools
import gc
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BAR_M, BAR_V, BAR_U = 4 * U, 6 * U, 16 * U
GUARD_EXTRA_V, GUARD_EXTRA_U = 2 * U, 1 * U
LR, BETA2, EPS = 1e-4, 0.999, 1e-8
DENORMAL_EDGE = 1e-30

NS = (1, 255, 256, 257, 4099)
STEPS = (1, 2, 3, 7, 30, 100, 1000, 1 << 20)
BETA1S = (0.75, 0.9, 0.5)
# (n, amsgrad, step, beta1): every step with both amsgrad modes, every n with at least three steps, every beta1 with both modes
ONE_STEP = [(NS[(2 * k + j) % 5], amsgrad, step, BETA1S[(k + j) % 3]) for k, step in enumerate(STEPS) for j, amsgrad in enumerate((True, False))]


def case_id(c):
    return f"n{c[0]}-{'amsgrad' if c[1] else 'plain'}-step{c[2]}-b{c[3]}"


def widen(x):
    """the fp32 value a `float` argument of the ABI receives, as a Python double"""
    return float(np.float32(x))


# ---------------------------------------------------------------------------- inputs
ORDINARY, EPS_SCALE, CANCELLING, AT_REST = range(4)
LAYOUT = (ORDINARY, EPS_SCALE, CANCELLING, AT_REST, ORDINARY, ORDINARY, ORDINARY, ORDINARY)


def _log_uniform(rng, lo, hi, n):
    return 10.0 ** rng.uniform(math.log10(lo), math.log10(hi), n)


def _signs(rng, n):
    return rng.integers(0, 2, n) * 2.0 - 1.0


@functools.lru_cache(maxsize=None)
def inputs(n, step, beta1):
    """g, m, v, vmax, p (a random p_in) as read-only fp32 arrays and cls, the class of every element; computed once per case."""
    rng = np.random.default_rng([n, step % 1000003, int(round(beta1 * 100))])
    b1, b2 = widen(beta1), widen(BETA2)
    bc2 = 1.0 - b2 ** step
    cls = np.array([LAYOUT[i % len(LAYOUT)] for i in range(n)])
    g = _signs(rng, n) * _log_uniform(rng, 1e-8, 10.0, n)
    m = _signs(rng, n) * _log_uniform(rng, 1e-8, 10.0, n)
    v = _log_uniform(rng, 1e-16, 1e2, n)
    vmax = v * 10.0 ** rng.uniform(-1.0, 1.0, n)
    p = rng.standard_normal(n)

    # eps-scale: `top` and `low` both lie inside bc2 [1e-18, 1e-14]; v' and vmax take one each, so sqrt(vd / bc2) is within
    # [0.1, 10] eps whichever of them the step divides by
    e = cls == EPS_SCALE
    k = int(e.sum())
    top = bc2 * 10.0 ** rng.uniform(-16.9, -14.1, k)
    low = top * 10.0 ** -rng.uniform(0.05, 0.9, k)
    binds = rng.integers(0, 2, k).astype(bool)
    v1 = np.where(binds, low, top)
    v[e] = 0.7 * v1 / b2
    g[e] = _signs(rng, k) * np.sqrt(0.3 * v1 / (1.0 - b2))
    vmax[e] = np.where(binds, top, low)
    m[e] = _signs(rng, k) * np.abs(g[e]) * 10.0 ** rng.uniform(-1.0, 1.0, k)

    c = cls == CANCELLING
    m[c] = -(1.0 - b1) * g[c] / b1 * (1.0 + rng.uniform(-0.01, 0.01, int(c.sum())))

    r = cls == AT_REST
    g[r] = m[r] = v[r] = vmax[r] = 0.0
    p[np.flatnonzero(r)[::2]] = -0.0

    out = SimpleNamespace(n=n, cls=cls, **{k: np.asarray(a, dtype=np.float32) for k, a in dict(g=g, m=m, v=v, vmax=vmax, p=p).items()})
    for a in (out.cls, out.g, out.m, out.v, out.vmax, out.p):
        a.setflags(write=False)
    live = ~r
    g64, v64 = out.g[live].astype(np.float64), out.v[live].astype(np.float64)
    assert (g64 * g64 * (1.0 - b2) >= DENORMAL_EDGE).all() and (v64 >= DENORMAL_EDGE).all()
    return out


def nan_pattern(n):
    """n quiet NaNs with distinct payloads: what the vmax buffer holds when amsgrad is off (a read of it would show in every output)"""
    return (np.uint32(0x7FC00001) + (np.arange(n, dtype=np.uint32) & np.uint32(0xFFFF))).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- float64 Adam and the measures
def adam64(g, m, v, vmax, lr, beta1, beta2, eps, step, amsgrad, fp32_betas=True):
    """One Adam step in float64 on fp32 buffers widened: m, v, vd (= the new vmax with amsgrad), the update u, and the two scales the
    bars are stated in.  fp32_betas=False: the betas as Python doubles (printed for the record)."""
    g, m, v = (np.asarray(a, dtype=np.float64) for a in (g, m, v))
    lr, eps = widen(lr), widen(eps)
    b1, b2 = (widen(beta1), widen(beta2)) if fp32_betas else (float(beta1), float(beta2))
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    t1, t2 = b1 * m, (1.0 - b1) * g
    m1 = t1 + t2
    v1 = b2 * v + (1.0 - b2) * g * g
    vd = np.maximum(np.asarray(vmax, dtype=np.float64), v1) if amsgrad else v1
    denom = np.sqrt(vd) / math.sqrt(bc2) + eps
    mscale = np.abs(t1) + np.abs(t2)
    return SimpleNamespace(m=m1, v=v1, vd=vd, u=(lr / bc1) * m1 / denom, denom=denom, mscale=mscale, uscale=(lr / bc1) * mscale / denom,
                           bc1=bc1, bc2=bc2)


def _worst(err, scale):
    """max err / scale; where the scale is 0 (an element at rest) any error at all is infinite"""
    with np.errstate(all="ignore"):
        r = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max()) if r.size else 0.0


def figures(m_out, v_out, u_out, ref, where=None):
    """{"m", "v", "u"}: the worst value of each measure in the module docstring, as a multiple of its scale (compare with BAR_*)."""
    w = slice(None) if where is None else where
    f64 = lambda a: np.asarray(a, dtype=np.float64)[w]
    with np.errstate(all="ignore"):
        return {"m": _worst(np.abs(f64(m_out) - ref.m[w]), ref.mscale[w]),
                "v": _worst(np.abs(f64(v_out) - ref.v[w]), ref.v[w]),
                "u": _worst(np.abs(f64(u_out) - ref.u[w]), ref.uscale[w])}


def show(what, fig):
    return f"adam exact {what}: " + ", ".join(f"{k} {x / U:.2f} u" for k, x in fig.items())


def scaled_gradient(g, scale):
    """what k_adam_guarded takes for g: one fp32 multiply by the scale rounded to fp32"""
    return np.asarray(g, dtype=np.float32) * np.float32(scale)


# ---------------------------------------------------------------------------- the device
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    yield torch.device("cuda:0")
    # This file runs first in the suite and the UNet trainer alone caches half a gigabyte: hand the cached device memory back, so
    # that the files after this one place their tensors as they did before it existed
    gc.collect()
    torch.cuda.empty_cache()


def device_step(dev, g, m, v, vmax, p, step, beta1, amsgrad, lr=LR, beta2=BETA2, eps=EPS, max_norm=None):
    """nd_adam_step, or with max_norm nd_grad_guard + nd_adam_step_guarded, on copies of the given host buffers (vmax None: a null
    pointer).  Everything comes back as numpy: p, m, v, vmax, g, and the guard's state before and after the step kernel."""
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    up = lambda a: torch.from_numpy(np.array(a, dtype=np.float32)).to(dev)
    tp, tg, tm, tv = up(p), up(g), up(m), up(v)
    tvmax = None if vmax is None else up(vmax)
    n = tg.numel()
    adam = (tp.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(), None if tvmax is None else tvmax.data_ptr(), n, lr, beta1, beta2,
            eps, step, int(amsgrad))
    state = after = None
    if max_norm is None:
        _lib.check(lib.nd_adam_step(*adam, sp), "nd_adam_step")
    else:
        ws = torch.full((lib.nd_grad_guard_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=dev)
        ts = torch.full((4,), float("nan"), dtype=torch.float64, device=dev)
        _lib.check(lib.nd_grad_guard(tg.data_ptr(), n, max_norm, 0, ts.data_ptr(), ws.data_ptr(), ws.numel(), sp), "nd_grad_guard")
        state = ts.cpu().numpy().copy()
        _lib.check(lib.nd_adam_step_guarded(*adam, ts.data_ptr(), sp), "nd_adam_step_guarded")
        after = ts.cpu().numpy()
    host = lambda t: None if t is None else t.cpu().numpy()
    return SimpleNamespace(p=host(tp), m=host(tm), v=host(tv), vmax=host(tvmax), g=host(tg), state=state, state_after=after)


def check_one_step(dev, case, max_norm=None, binding=False):
    n, amsgrad, step, beta1 = case
    inp = inputs(n, step, beta1)
    vmax_in = inp.vmax if amsgrad else nan_pattern(n)
    zero = np.zeros(n, dtype=np.float32)
    out = device_step(dev, inp.g, inp.m, inp.v, vmax_in, zero, step, beta1, amsgrad, max_norm=max_norm)
    g_ref, bar_v, bar_u = inp.g, BAR_V, BAR_U
    if max_norm is not None:
        assert out.state[1] == 0.0 and out.state[3] == 1.0
        assert np.array_equal(out.state.view(np.uint64), out.state_after.view(np.uint64))        # the step kernel reads the state
        if binding:
            assert 0.0 < out.state[2] < 0.26, out.state                   # (n = 1: the 1e-6 beside a norm of 1e-8 ... 10 only lowers it)
            g_ref, bar_v, bar_u = scaled_gradient(inp.g, out.state[2]), BAR_V + GUARD_EXTRA_V, BAR_U + GUARD_EXTRA_U
        else:
            assert out.state[2] == 1.0
    what = case_id(case) + ("" if max_norm is None else " guarded, binding" if binding else " guarded, scale 1")
    ref = adam64(g_ref, inp.m, inp.v, inp.vmax, LR, beta1, BETA2, EPS, step, amsgrad)
    fig = figures(out.m, out.v, -out.p, ref)
    print(show(what, fig))
    print(show(what + " [Python-double betas]",
               figures(out.m, out.v, -out.p, adam64(g_ref, inp.m, inp.v, inp.vmax, LR, beta1, BETA2, EPS, step, amsgrad, fp32_betas=False))))
    assert fig["m"] <= BAR_M and fig["v"] <= bar_v and fig["u"] <= bar_u, (what, {k: x / U for k, x in fig.items()})

    # exact: vmax, the gradient, p from a random start, the elements at rest
    if amsgrad:
        assert np.array_equal(bits(out.vmax), bits(np.maximum(inp.vmax, out.v)))
    else:
        assert np.array_equal(bits(out.vmax), bits(vmax_in))
    assert np.array_equal(bits(out.g), bits(inp.g))
    rest = inp.cls == AT_REST
    again = device_step(dev, inp.g, inp.m, inp.v, vmax_in, inp.p, step, beta1, amsgrad, max_norm=max_norm)
    assert np.array_equal(bits(again.p)[~rest], bits(inp.p + out.p)[~rest])
    assert np.array_equal(bits(again.p)[rest], bits(inp.p)[rest])
    for a, b in ((again.m, out.m), (again.v, out.v), (again.vmax, out.vmax)):
        assert np.array_equal(bits(a), bits(b))
    for a in (out.m, out.v, out.p) + ((out.vmax,) if amsgrad else ()):
        assert not a[rest].any() and not np.signbit(a[rest]).any()
    return out


@pytest.mark.parametrize("case", ONE_STEP, ids=case_id)
def test_one_step_vs_float64(dev, case):
    out = check_one_step(dev, case)
    n, amsgrad, step, beta1 = case
    if not amsgrad:                 # a null vmax is accepted, and gives the same bits
        inp = inputs(n, step, beta1)
        null = device_step(dev, inp.g, inp.m, inp.v, None, np.zeros(n, dtype=np.float32), step, beta1, False)
        for a, b in ((null.p, out.p), (null.m, out.m), (null.v, out.v)):
            assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("binding", [False, True], ids=["scale1", "binding"])
@pytest.mark.parametrize("case", ONE_STEP, ids=case_id)
def test_one_guarded_step_vs_float64(dev, case, binding):
    inp = inputs(case[0], case[2], case[3])
    norm = math.sqrt(float((inp.g.astype(np.float64) ** 2).sum()))
    check_one_step(dev, case, max_norm=0.25 * norm if binding else 1e30, binding=binding)


# ---------------------------------------------------------------------------- 64 steps from zero state
TRAJ_N, TRAJ_STEPS, TRAJ_LR, TRAJ_BETA1 = 4099, 64, 1e-3, 0.75
TRAJ_RUNS = [(amsgrad, guarded) for amsgrad in (True, False) for guarded in (False, True)]
# m, v, vmax: relative 2-norm of the error after the last step; p: max |p - p_ref| over the largest per-element sum of |u_ref|.
# Not derivable in closed form: TRAJ_CPU_FP32 is torch.optim.Adam in fp32 on the CPU against the same float64 loop, the worst of the
# four runs (tests/test_adam_exact_host.py computes and asserts it), and the bar is 3x that.
TRAJ_CPU_FP32 = {"m": 4.25e-8, "v": 1.50e-7, "vmax": 1.50e-7, "p": 3.91e-7}
TRAJ_BARS = {k: 3 * x for k, x in TRAJ_CPU_FP32.items()}
# bars:                       m 1.275e-7, v 4.50e-7, vmax 4.50e-7, p 1.173e-6
# measured on the MI355X, the worst of the four runs: m 5.69e-8, v 1.50e-7, vmax 1.50e-7, p 4.10e-7 (the norm binds on 32 of 64 steps)


@functools.lru_cache(maxsize=None)
def trajectory_gradients():
    """[TRAJ_STEPS, TRAJ_N] fp32: per element a constant signal of magnitude 10^U(-6, 0) plus noise of that size; and the norm that
    clips about half of the steps"""
    rng = np.random.default_rng(64)
    s = _signs(rng, TRAJ_N) * _log_uniform(rng, 1e-6, 1.0, TRAJ_N)
    g = (s + rng.standard_normal((TRAJ_STEPS, TRAJ_N)) * np.abs(s)).astype(np.float32)
    g.setflags(write=False)
    norms = np.sqrt((g.astype(np.float64) ** 2).sum(axis=1))
    return g, float(np.median(norms))


def clip_scale64(g, max_norm):
    """the coefficient of torch.nn.utils.clip_grad_norm_ in float64, for max_norm as the fp32 value the call receives"""
    return min(1.0, widen(max_norm) / (math.sqrt(float((np.asarray(g, dtype=np.float64) ** 2).sum())) + 1e-6))


def trajectory64(amsgrad, scales=None):
    """the float64 loop from zero state; scales: per step, the factor the gradient takes in one fp32 multiply (None: none)"""
    g_all, _ = trajectory_gradients()
    z = np.zeros(TRAJ_N)
    s = SimpleNamespace(m=z, v=z.copy(), vmax=z.copy(), p=z.copy(), path=z.copy())
    for t in range(TRAJ_STEPS):
        g = g_all[t] if scales is None else scaled_gradient(g_all[t], scales[t])
        r = adam64(g, s.m, s.v, s.vmax, TRAJ_LR, TRAJ_BETA1, BETA2, EPS, t + 1, amsgrad)
        s.m, s.v, s.p, s.path = r.m, r.v, s.p - r.u, s.path + np.abs(r.u)
        if amsgrad:
            s.vmax = r.vd
    return s


def trajectory_figures(got, ref, amsgrad):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, dtype=np.float64) - b) / np.linalg.norm(b))
    fig = {"m": rel(got.m, ref.m), "v": rel(got.v, ref.v), "p": float(np.abs(np.asarray(got.p, dtype=np.float64) - ref.p).max() / ref.path.max())}
    if amsgrad:
        fig["vmax"] = rel(got.vmax, ref.vmax)
    return fig


@pytest.mark.parametrize("amsgrad,guarded", TRAJ_RUNS, ids=lambda x: None)
def test_trajectory_vs_float64(dev, amsgrad, guarded):
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    g_all, max_norm = trajectory_gradients()
    tg = torch.zeros(TRAJ_STEPS, TRAJ_N + 1, device=dev)               # rows of 4100 floats: the guard wants 16-byte aligned gradients
    tg[:, :TRAJ_N] = torch.from_numpy(np.array(g_all)).to(dev)
    p, m, v, vmax = (torch.zeros(TRAJ_N, device=dev) for _ in range(4))
    ws = torch.full((lib.nd_grad_guard_workspace_bytes(TRAJ_N),), 0xFF, dtype=torch.uint8, device=dev)
    states = torch.full((TRAJ_STEPS, 4), float("nan"), dtype=torch.float64, device=dev)
    for t in range(TRAJ_STEPS):
        adam = (p.data_ptr(), tg[t].data_ptr(), m.data_ptr(), v.data_ptr(), vmax.data_ptr(), TRAJ_N, TRAJ_LR, TRAJ_BETA1, BETA2, EPS, t + 1,
                int(amsgrad))
        if guarded:
            _lib.check(lib.nd_grad_guard(tg[t].data_ptr(), TRAJ_N, max_norm, 0, states[t].data_ptr(), ws.data_ptr(), ws.numel(), sp),
                       "nd_grad_guard")
            _lib.check(lib.nd_adam_step_guarded(*adam, states[t].data_ptr(), sp), "nd_adam_step_guarded")
        else:
            _lib.check(lib.nd_adam_step(*adam, sp), "nd_adam_step")
    scales = None
    if guarded:
        st = states.cpu().numpy()
        scales = st[:, 2]
        clipped = int((scales < 1.0).sum())
        print(f"adam exact trajectory: the norm binds on {clipped} of {TRAJ_STEPS} steps")
        assert 8 <= clipped <= TRAJ_STEPS - 8 and (st[:, 3] == 1.0).all() and (scales > 0.5).all()
        for t in range(TRAJ_STEPS):      # the guard has its own float64 test: here only that this is the scale that test describes
            want = np.float32(clip_scale64(g_all[t], max_norm))
            assert abs(np.float32(scales[t]) - want) <= np.spacing(want)
    got = SimpleNamespace(m=m.cpu().numpy(), v=v.cpu().numpy(), vmax=vmax.cpu().numpy(), p=p.cpu().numpy())
    assert np.array_equal(bits(tg[:, :TRAJ_N].cpu().numpy()), bits(g_all))
    if not amsgrad:
        assert not got.vmax.any()
    fig = trajectory_figures(got, trajectory64(amsgrad, scales), amsgrad)
    print(f"adam exact trajectory amsgrad {amsgrad} guarded {guarded}: " + ", ".join(f"{k} {x:.3e} (bar {TRAJ_BARS[k]:.3e})" for k, x in fig.items()))
    for k, x in fig.items():
        assert x <= TRAJ_BARS[k], (k, x, TRAJ_BARS[k])


# ---------------------------------------------------------------------------- the trainers
def check_trainer_steps(tr, lr, beta1, beta2, eps, amsgrad, frozen=()):
    """Three optimizer_step() calls on the gradient the trainer holds, the rate halved before the third; each against one float64
    step from the device's previous state, under the one-step measures.  p does not start at 0 here, so the stored parameter carries
    one more rounding: u |p_ref| beside BAR_U's share.  Elements outside the one-step domain (g^2 (1 - b2) or v below 1e-30, not at
    rest) are counted and left out of the three measures.  frozen: index arrays whose parameters must keep their bits.
    Measured on the MI355X: UtNet(8) m 1.40 u, v 2.28 u, p 0.996 of its allowance (485839 of 485853 elements measured, 9 at rest);
    UNet m 1.50 u, v 2.43 u, p 0.990 (14282307 of 14796995 measured, the others at rest).  p sits at its allowance because a parameter
    of size 1 rounds by up to u, a hundred times BAR_U's share of an update of 1e-3: this figure sees a wrong lr, eps, beta or step
    index, not the update's last bits -- the one-step cases from p = 0 see those."""
    snap = lambda: {k: getattr(tr, k).detach().cpu().numpy().copy() for k in ("flat", "grads", "m", "v", "vmax")}
    before = start = snap()
    g = before["grads"]
    g64 = g.astype(np.float64)
    assert tr.steps == 0 and np.isfinite(g).all() and g.any()
    b2 = widen(beta2)
    for step in (1, 2, 3):
        if step == 3:
            tr.update_learning_rate(0.5)
            lr = lr * 0.5
        tr.optimizer_step()
        after = snap()
        assert tr.steps == step and np.array_equal(bits(after["grads"]), bits(g))
        ref = adam64(g, before["m"], before["v"], before["vmax"], lr, beta1, beta2, eps, step, amsgrad)
        rest = (g == 0) & (before["m"] == 0) & (before["v"] == 0) & (before["vmax"] == 0)
        live = (g64 * g64 * (1.0 - b2) >= DENORMAL_EDGE) & ((before["v"] >= DENORMAL_EDGE) | (before["v"] == 0))
        print(f"adam exact {tr.kind} step {step}: {int(live.sum())} of {g.size} elements measured, {int(rest.sum())} at rest")
        assert (live | rest).sum() >= 0.9 * g.size and live.sum() >= 0.5 * g.size
        fig = figures(after["m"], after["v"], ref.u, ref, where=live)
        p_ref = before["flat"].astype(np.float64) - ref.u
        p_err = np.abs(after["flat"].astype(np.float64) - p_ref)
        del fig["u"]
        p_fig = _worst(p_err[live], (BAR_U * ref.uscale + U * np.abs(p_ref))[live])
        print(show(f"{tr.kind} step {step} lr {lr:g}", fig) + f", p {p_fig:.3f} of BAR_U's share + u |p|")
        assert fig["m"] <= BAR_M and fig["v"] <= BAR_V and p_fig <= 1.0, ({k: x / U for k, x in fig.items()}, p_fig)
        for k in ("flat", "m", "v", "vmax"):
            assert np.array_equal(bits(after[k])[rest], bits(before[k])[rest]), k
        if amsgrad:
            assert np.array_equal(bits(after["vmax"]), bits(np.maximum(before["vmax"], after["v"])))
        else:
            assert not after["vmax"].any()
        before = after
    assert not np.array_equal(before["flat"], start["flat"])
    for idx in frozen:
        assert np.array_equal(bits(before["flat"])[idx], bits(start["flat"])[idx])


def _image(n, h, w, seed):
    return torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed))


def test_utnet_trainer_steps_vs_float64(dev):
    from nind_denoise_amd import synth
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    net = UtNet(funit=8)
    net.load_state_dict(synth.make_utnet_state_dict(funit=8, seed=31, gain=1.8))
    hyper = dict(lr=3e-4, beta1=0.9, beta2=0.99, eps=1e-7, amsgrad=False)             # none of them the default
    tr = UtNetTrainer(net, device=dev, weights={"MSE": 0.5, "L1": 0.5}, **hyper)
    tr.forward_backward(_image(1, 104, 104, 3), _image(1, 104, 104, 4))
    check_trainer_steps(tr, **hyper)


def test_unet_trainer_steps_vs_float64(dev):
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    from nind_denoise_amd.train import UNetTrainer
    torch.manual_seed(5)
    net = UNet()
    pre_bn = [f"{prefix}.{i}.bias" for prefix, mod in net.named_modules() if isinstance(mod, torch.nn.Sequential)
              for i, (a, b) in enumerate(zip(list(mod)[:-1], list(mod)[1:]))
              if isinstance(a, torch.nn.Conv2d) and isinstance(b, torch.nn.BatchNorm2d)]
    assert len(pre_bn) == 18
    hyper = dict(lr=1e-3, beta1=0.75, beta2=0.999, eps=1e-8, amsgrad=True)
    tr = UNetTrainer(net, device=dev, weights={"MSE": 1.0}, **hyper)
    stats = [k for k in tr.ranges if k.endswith("running_mean") or k.endswith("running_var")]
    assert len(stats) == 36 and all(k in tr.ranges for k in pre_bn)
    tr.forward_backward(_image(2, 32, 32, 6), _image(2, 32, 32, 7))                    # (2, 32, 32) of test_unet_train.CASES
    frozen = [np.arange(off, off + cnt) for off, cnt in (tr.ranges[k] for k in pre_bn + stats)]
    check_trainer_steps(tr, frozen=frozen, **hyper)
