"""GPU tests of the guarded optimizer step: nd_grad_guard against float64, its count of non-finite entries, its repeatability,
nd_adam_step_guarded against nd_adam_step bit for bit, and the two trainers with max_grad_norm / skip_nonfinite.

Bars.  Sum of g^2: both sides add non-negative doubles (the square of an fp32 value is exact in double), so each is within
(n - 1) 2^-53 of the exact sum relative to it, whatever the order: the two differ by at most 2 n 2^-53.  scale: the float64
restatement, rounded to fp32, within one fp32 ulp.  Everything else is bit equality."""
import copy
import math

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 255, 256, 257, 65537, 1000003]
N_BIG = 1000003


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def wide_gradient(n, seed):
    """n fp32 values with magnitudes from 1e-20 to 1e18, either sign (on the CPU)"""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, dtype=torch.float64, generator=g) * 38.0 - 20.0)
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (mag * sign).float()


def guard(grads, max_norm, skip, ws=None):
    """nd_grad_guard on a device tensor: the four doubles, on the host"""
    lib = _lib.load()
    n = grads.numel()
    nbytes = lib.nd_grad_guard_workspace_bytes(n)
    assert nbytes > 0
    if ws is None:
        ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=grads.device)        # every double a NaN
    state = torch.full((4,), float("nan"), dtype=torch.float64, device=grads.device)
    _lib.check(lib.nd_grad_guard(grads.data_ptr(), n, max_norm, int(skip), state.data_ptr(), ws.data_ptr(), ws.numel(),
                                 _lib.stream_ptr(grads.device)), "nd_grad_guard")
    return state.cpu()


def torch_scale(g64, max_norm):
    """the coefficient of torch.nn.utils.clip_grad_norm_, in float64, for max_norm as the fp32 value the call receives"""
    total = torch.linalg.vector_norm(g64)
    return torch.clamp(float(np.float32(max_norm)) / (total + 1e-6), max=1.0).item()


# ------------------------------------------------------------------ 1. the sums and the scale against float64
@pytest.mark.parametrize("n", SIZES)
def test_grad_guard_vs_float64(dev, n):
    g = wide_gradient(n, seed=n)
    g64 = g.double()
    ref = (g64 * g64).sum().item()
    assert 0 < ref < float("inf")
    for max_norm in (0.0, 0.5 * math.sqrt(ref), 4.0 * math.sqrt(ref)):       # off, binding, not binding
        got = guard(g.to(dev), max_norm, False).tolist()
        rel = abs(got[0] - ref) / ref
        bar = 2 * n * 2.0 ** -53
        want = torch_scale(g64, max_norm) if max_norm > 0 else 1.0
        print(f"n {n} max_norm {max_norm:.6g}: sum g^2 {got[0]!r} (float64 {ref!r}), relative error {rel:.3e}, bar {bar:.3e}; "
              f"scale {got[2]!r}, float64 {want!r}")
        assert rel <= bar
        assert got[1] == 0.0 and got[3] == 1.0
        assert abs(np.float32(got[2]) - np.float32(want)) <= np.spacing(np.float32(want))
        # (the 1e-6 in the denominator decides for a norm far below it: the clamp binds when the float64 restatement says so)
        assert got[2] == 1.0 if want == 1.0 else got[2] < 1.0
        if max_norm == 0.0 or (max_norm > math.sqrt(ref) + 1e-6):
            assert got[2] == 1.0


# ------------------------------------------------------------------ 2. non-finite entries
# n = 1 000 003: 250 000 16-byte elements over 977 workgroups of 256 threads; workgroup 0 takes elements 0..255 in its first round,
# workgroup 1 elements 256..511: floats 1023 | 1024 are a seam.  Floats 1 000 000..1 000 002 are the scalar tail.
NAN, INF = float("nan"), float("inf")
PLANTS = {
    "first-nan": {0: NAN}, "first-inf": {0: INF}, "last-neginf": {N_BIG - 1: -INF}, "seam": {1023: INF, 1024: -INF},
    "tail": {N_BIG - 3: NAN, N_BIG - 2: INF, N_BIG - 1: -INF}, "seam-nan": {1023: NAN, 1024: NAN},
    "all": {0: NAN, 1023: INF, 1024: -INF, N_BIG - 3: INF, N_BIG - 1: NAN},
}


@pytest.fixture(scope="module")
def big_gradient():
    g = torch.Generator().manual_seed(3)
    return torch.randn(N_BIG, generator=g) * 1e-3


@pytest.mark.parametrize("case", sorted(PLANTS))
def test_grad_guard_counts_nonfinite_entries(dev, big_gradient, case):
    g = big_gradient.clone()
    for i, value in PLANTS[case].items():
        g[i] = value
    want = torch_scale(g.double(), 1.0)
    has_nan = any(math.isnan(v) for v in PLANTS[case].values())
    assert math.isnan(want) if has_nan else want == 0.0
    for skip in (False, True):
        got = guard(g.to(dev), 1.0, skip).tolist()
        print(f"{case} skip {skip}: state {got}, torch's coefficient {want}")
        assert got[1] == len(PLANTS[case])
        assert got[3] == (0.0 if skip else 1.0)
        assert math.isnan(got[0]) if has_nan else got[0] == INF
        assert math.isnan(got[2]) if has_nan else got[2] == 0.0
    # clipping off: the scale stays 1 whatever the norm
    got = guard(g.to(dev), 0.0, True).tolist()
    assert got[2] == 1.0 and got[3] == 0.0 and got[1] == len(PLANTS[case])


@pytest.mark.parametrize("n", [5, 1027])
def test_grad_guard_tail_and_small_sizes_count(dev, n):
    """every position of a short buffer, one at a time: vector body and scalar tail"""
    for i in range(n) if n < 10 else (0, 3, 1023, 1024, 1025, 1026):
        g = torch.ones(n)
        g[i] = NAN
        got = guard(g.to(dev), 1.0, True).tolist()
        assert got[1] == 1.0 and got[3] == 0.0 and math.isnan(got[2]), (n, i, got)
    got = guard(torch.ones(n).to(dev), 1.0, True).tolist()
    want = np.float32(torch_scale(torch.ones(n).double(), 1.0))
    assert got[0] == float(n) and got[1] == 0.0 and got[3] == 1.0 and abs(np.float32(got[2]) - want) <= np.spacing(want)


# ------------------------------------------------------------------ 3. repeatability
def test_grad_guard_repeats_its_bits(dev):
    g = wide_gradient(N_BIG, seed=9).to(dev)
    norm = torch.linalg.vector_norm(g.double()).item()
    a = guard(g, 0.3 * norm, True)
    b = guard(g, 0.3 * norm, True)
    # a workspace that held other values, larger than asked for
    ws = torch.zeros(_lib.load().nd_grad_guard_workspace_bytes(N_BIG) + 64, dtype=torch.uint8, device=dev)
    c = guard(g, 0.3 * norm, True, ws=ws)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(a.view(torch.int64), c.view(torch.int64))
    assert not torch.isnan(a).any() and a[2] < 1.0


def test_grad_guard_refuses_bad_arguments(dev):
    lib = _lib.load()
    g = torch.ones(64, device=dev)
    state = torch.zeros(4, dtype=torch.float64, device=dev)
    ws = torch.zeros(lib.nd_grad_guard_workspace_bytes(64), dtype=torch.uint8, device=dev)
    sp = _lib.stream_ptr(dev)
    assert lib.nd_grad_guard_workspace_bytes(0) == 0
    assert lib.nd_grad_guard(g.data_ptr(), 64, 1.0, 0, state.data_ptr(), ws.data_ptr(), ws.numel() - 1, sp) != 0      # short workspace
    assert lib.nd_grad_guard(g.data_ptr() + 4, 60, 1.0, 0, state.data_ptr(), ws.data_ptr(), ws.numel(), sp) != 0      # misaligned
    assert lib.nd_grad_guard(None, 64, 1.0, 0, state.data_ptr(), ws.data_ptr(), ws.numel(), sp) != 0
    assert lib.nd_grad_guard(g.data_ptr(), 0, 1.0, 0, state.data_ptr(), ws.data_ptr(), ws.numel(), sp) != 0
    torch.cuda.synchronize()
    assert state.tolist() == [0.0] * 4


# ------------------------------------------------------------------ 4. nd_adam_step_guarded against nd_adam_step
ADAM = (1e-3, 0.75, 0.999, 1e-8)       # lr, beta1, beta2, eps


class Flat:
    """params, m, v, vmax of n elements, from one seed"""

    def __init__(self, dev, n=N_BIG):
        g = torch.Generator().manual_seed(21)
        self.p = torch.randn(n, generator=g).to(dev)
        self.m, self.v, self.vmax = (torch.zeros(n, device=dev) for _ in range(3))
        self.dev = dev

    def tensors(self):
        return self.p, self.m, self.v, self.vmax

    def plain(self, g, step, amsgrad):
        _lib.check(_lib.load().nd_adam_step(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.vmax.data_ptr(),
                                            g.numel(), *ADAM, step, int(amsgrad), _lib.stream_ptr(self.dev)), "nd_adam_step")

    def guarded(self, g, step, amsgrad, max_norm, skip):
        """guard + guarded step; returns the state (host)"""
        lib = _lib.load()
        ws = torch.full((lib.nd_grad_guard_workspace_bytes(g.numel()),), 0xFF, dtype=torch.uint8, device=self.dev)
        state = torch.zeros(4, dtype=torch.float64, device=self.dev)
        _lib.check(lib.nd_grad_guard(g.data_ptr(), g.numel(), max_norm, int(skip), state.data_ptr(), ws.data_ptr(), ws.numel(),
                                     _lib.stream_ptr(self.dev)), "nd_grad_guard")
        _lib.check(lib.nd_adam_step_guarded(self.p.data_ptr(), g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.vmax.data_ptr(),
                                            g.numel(), *ADAM, step, int(amsgrad), state.data_ptr(), _lib.stream_ptr(self.dev)),
                   "nd_adam_step_guarded")
        return state.cpu()


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def step_gradients(dev):
    g = torch.Generator().manual_seed(22)
    return [(torch.randn(N_BIG, generator=g) * 10.0 ** (-k)).to(dev) for k in range(3)]


@pytest.mark.parametrize("amsgrad", [True, False])
def test_guarded_step_with_a_huge_norm_is_the_plain_step(dev, step_gradients, amsgrad):
    a, b = Flat(dev), Flat(dev)
    for step, g in enumerate(step_gradients, 1):
        a.plain(g, step, amsgrad)
        state = b.guarded(g, step, amsgrad, 1e30, True)
        assert state[2] == 1.0 and state[3] == 1.0
    assert same_bits(a.tensors(), b.tensors())
    assert not torch.equal(a.p, Flat(dev).p)
    assert amsgrad == bool(a.vmax.abs().max() > 0)


@pytest.mark.parametrize("amsgrad", [True, False])
def test_guarded_step_clips_as_the_plain_step_on_scaled_gradients(dev, step_gradients, amsgrad):
    a, b = Flat(dev), Flat(dev)
    for step, g in enumerate(step_gradients, 1):
        keep = g.clone()
        norm = torch.linalg.vector_norm(g.double()).item()
        state = b.guarded(g, step, amsgrad, 0.25 * norm, False)
        assert 0.24 < state[2] < 0.26 and state[3] == 1.0
        assert torch.equal(g.view(torch.int32), keep.view(torch.int32))              # the gradient itself is not clipped
        scaled = g * torch.tensor(state[2].item(), dtype=torch.float32, device=dev)  # the scale rounded to fp32, one fp32 multiply
        a.plain(scaled, step, amsgrad)
    assert same_bits(a.tensors(), b.tensors())


@pytest.mark.parametrize("amsgrad", [True, False])
def test_skipped_step_touches_nothing_and_the_next_one_counts_on(dev, step_gradients, amsgrad):
    g1, g2, g3 = (g.clone() for g in step_gradients)
    g2[N_BIG // 2] = NAN
    a, b = Flat(dev), Flat(dev)
    b.guarded(g1, 1, amsgrad, 0.0, True)
    before = [t.clone() for t in b.tensors()]
    bad = g2.clone()
    state = b.guarded(g2, 2, amsgrad, 0.0, True)
    assert state[1] == 1.0 and state[3] == 0.0
    assert same_bits(before, b.tensors())
    assert torch.equal(bad.view(torch.int32), g2.view(torch.int32))
    state = b.guarded(g3, 3, amsgrad, 0.0, True)
    assert state[3] == 1.0
    a.plain(g1, 1, amsgrad)
    assert same_bits(before, a.tensors())
    a.plain(g3, 3, amsgrad)                           # the unguarded sequence, given the index of the attempt
    assert same_bits(a.tensors(), b.tensors())
    # without skip_nonfinite the NaN goes through, as in nd_adam_step
    c = Flat(dev)
    state = c.guarded(g2, 1, amsgrad, 0.0, False)
    assert state[3] == 1.0 and torch.isnan(c.p[N_BIG // 2]) and torch.isfinite(c.p).sum() == N_BIG - 1


# ------------------------------------------------------------------ 5. UtNetTrainer
FUNIT, CS = 16, 104
WEIGHTS = {"MSE": 0.5, "L1": 0.5}


def image_like(n, h, w, seed):
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    c = F.interpolate(torch.rand(n, 3, h // 8, w // 8, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    return (0.8 * c + 0.1 + 0.05 * torch.randn(n, 3, h, w, generator=g)).clip(0, 1)


@pytest.fixture(scope="module")
def utnet_case():
    from nind_denoise_amd import synth
    sd = synth.make_utnet_state_dict(funit=FUNIT, seed=31, gain=1.8)
    x = image_like(2, CS, CS, seed=3)
    t = (x * 0.9 + 0.05 * image_like(2, CS, CS, seed=4)).clip(0, 1)
    return sd, x, t


def utnet_trainer(dev, sd, **kw):
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    net = UtNet(funit=FUNIT)
    net.load_state_dict(copy.deepcopy(sd))
    return UtNetTrainer(net, lr=1e-3, device=dev, weights=WEIGHTS, **kw)


def bits(t):
    return t.detach().view(torch.int32)


def test_utnet_trainer_options_off_or_huge_are_the_plain_trainer(dev, utnet_case):
    sd, x, t = utnet_case
    plain, off, huge = utnet_trainer(dev, sd), utnet_trainer(dev, sd, max_grad_norm=None, skip_nonfinite=False), \
        utnet_trainer(dev, sd, max_grad_norm=1e30, skip_nonfinite=True)
    assert not plain.guarded and plain.guard_state is None and not off.guarded and huge.guarded
    start = plain.flat.clone()
    for tr in (plain, off, huge):
        for _ in range(2):
            tr.learn(x, t)
    assert torch.equal(bits(plain.flat), bits(off.flat)) and torch.equal(bits(plain.flat), bits(huge.flat))
    assert not torch.equal(plain.flat, start)
    assert huge.guard_state.tolist()[1:] == [0.0, 1.0, 1.0] and huge.guard_state[0] > 0
    assert huge.steps == plain.steps == 2
    with pytest.raises(ValueError):
        utnet_trainer(dev, sd, max_grad_norm=0.0)


def test_utnet_trainer_clips_as_the_prescaled_step(dev, utnet_case):
    sd, x, t = utnet_case
    a, b = utnet_trainer(dev, sd, max_grad_norm=1e-3), utnet_trainer(dev, sd)
    start = a.flat.clone()
    name = "convs1.0.weight"
    for _ in range(2):
        a.learn(x, t)
        scale = a.guard_state[2].item()
        assert 0 < scale < 1, scale
        b.forward_backward(x, t)
        assert torch.equal(bits(a.grads), bits(b.grads))                      # grad_of keeps the unclipped gradient
        assert torch.equal(bits(a.grad_of(name)), bits(b.grad_of(name)))
        norm = torch.linalg.vector_norm(b.grads.double()).item()
        assert abs(scale - float(np.float32(1e-3)) / (norm + 1e-6)) <= 1e-9 * scale
        b.grads.mul_(torch.tensor(scale, dtype=torch.float32, device=dev))
        b.optimizer_step()
        assert torch.equal(bits(a.flat), bits(b.flat))
    assert not torch.equal(a.flat, start)


def test_utnet_trainer_skips_a_nonfinite_step(dev, utnet_case):
    sd, x, t = utnet_case
    tr, plain = utnet_trainer(dev, sd, skip_nonfinite=True), utnet_trainer(dev, sd)
    start = tr.flat.clone()
    generation = tr.model.weights_generation
    bad = x.clone()
    bad[1, 2, 50, 51] = NAN
    tr.learn(bad, t)
    state = tr.guard_state.tolist()
    print(f"guard state after the NaN pixel: {state}")
    assert state[1] > 0 and state[3] == 0.0 and state[2] == 1.0
    assert torch.equal(bits(tr.flat), bits(start))
    assert all(not buf.any() for buf in (tr.m, tr.v, tr.vmax))
    assert tr.steps == 1 and tr.model.weights_generation > generation
    # the next clean step: applied, and the plain step at the index of the attempt
    loss = tr.learn(x, t)
    assert tr.guard_state.tolist()[1:] == [0.0, 1.0, 1.0] and math.isfinite(loss.item())
    plain.steps = 1
    plain.learn(x, t)
    assert torch.equal(bits(tr.flat), bits(plain.flat)) and not torch.equal(tr.flat, start)
    assert torch.isfinite(tr.flat).all()


def test_utnet_trainer_state_dict_round_trip(dev, utnet_case):
    sd, x, t = utnet_case
    a = utnet_trainer(dev, sd, max_grad_norm=1e-3, skip_nonfinite=True)
    a.learn(x, t)
    a.update_learning_rate(0.5)
    state = a.state_dict()
    assert all(state[k].device.type == "cpu" for k in ("flat", "m", "v", "vmax"))
    b = utnet_trainer(dev, sd)
    views = {k: p.data_ptr() for k, p in b.model.named_parameters()}
    generation = b.model.weights_generation
    b.load_state_dict(state)
    assert views == {k: p.data_ptr() for k, p in b.model.named_parameters()} and b.model.weights_generation > generation
    assert (b.steps, b.lr, b.max_grad_norm, b.skip_nonfinite) == (1, 5e-4, 1e-3, True)
    a.learn(x, t)
    b.learn(x, t)
    for key in ("flat", "m", "v", "vmax"):
        assert torch.equal(bits(getattr(a, key)), bits(getattr(b, key))), key
    # the module reads the loaded parameters
    off, cnt = b.ranges["convs1.0.weight"]
    assert torch.equal(dict(b.model.named_parameters())["convs1.0.weight"].detach().reshape(-1), b.flat[off:off + cnt])
    from nind_denoise_amd.networks.UtNet import UtNet
    from nind_denoise_amd.train import UtNetTrainer
    other = UtNetTrainer(UtNet(funit=8), device=dev)
    with pytest.raises(ValueError, match="funit"):
        other.load_state_dict(state)
    broken = dict(state, m=state["m"][:-1])
    with pytest.raises(ValueError, match="parameter"):
        b.load_state_dict(broken)


# ------------------------------------------------------------------ 6. UNetTrainer
def unet_trainer(dev, sd, **kw):
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    from nind_denoise_amd.train import UNetTrainer
    net = UNet()
    net.load_state_dict(copy.deepcopy(sd))
    return UNetTrainer(net, lr=1e-3, device=dev, weights=WEIGHTS, **kw)


@pytest.fixture(scope="module")
def unet_case():
    from nind_denoise_amd.networks.ThirdPartyNets import UNet
    torch.manual_seed(5)
    sd = copy.deepcopy(UNet().state_dict())
    x = image_like(2, 32, 32, seed=6)
    t = (x * 0.9 + 0.05 * image_like(2, 32, 32, seed=7)).clip(0, 1)
    return sd, x, t


def test_unet_trainer_huge_norm_and_binding_norm(dev, unet_case):
    sd, x, t = unet_case
    plain, huge = unet_trainer(dev, sd), unet_trainer(dev, sd, max_grad_norm=1e30, skip_nonfinite=True)
    for tr in (plain, huge):
        for _ in range(2):
            tr.learn(x, t)
    assert torch.equal(bits(plain.flat), bits(huge.flat))
    assert huge.guard_state.tolist()[1:] == [0.0, 1.0, 1.0]
    # binding
    a, b = unet_trainer(dev, sd, max_grad_norm=1e-4), unet_trainer(dev, sd)
    start = a.flat.clone()
    for _ in range(2):
        a.learn(x, t)
        scale = a.guard_state[2].item()
        assert 0 < scale < 1, scale
        b.forward_backward(x, t)
        assert torch.equal(bits(a.grads), bits(b.grads))
        b.grads.mul_(torch.tensor(scale, dtype=torch.float32, device=dev))
        b.optimizer_step()
        assert torch.equal(bits(a.flat), bits(b.flat))
    assert not torch.equal(a.flat, start)
    # state dict: the running statistics travel in the flat buffer, num_batches_tracked beside it
    state = a.state_dict()
    c = unet_trainer(dev, sd)
    c.load_state_dict(state)
    assert torch.equal(bits(c.flat), bits(a.flat)) and [int(v) for v in c._tracked] == [2] * len(c._tracked)
    assert c.max_grad_norm == 1e-4 and c.steps == 2
    from nind_denoise_amd import synth
    with pytest.raises(ValueError, match="UNetTrainer"):
        utnet_trainer(dev, synth.make_utnet_state_dict(funit=FUNIT, seed=1)).load_state_dict(state)
