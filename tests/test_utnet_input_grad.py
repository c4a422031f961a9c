"""UtNet under autograd: the input image's gradient (first layer's data gradient through ReflectionPad2d(2), k_input_grad),
frozen / eval() networks as differentiable stages, rectangular crops through the training path (nd_utnet_train_*_hw).

References: torch autograd on oracle.networks.utnet_forward in float64 on the CPU.  Relative bar as for the parameter
gradients of test_hip_parity.py: max|got - ref| / max|ref| <= 1e-3.  Synthetic weights with gain=1.8 and an MSE criterion
(with an L1 term the sign of g - t flips on pixels where two forwards differ in the last bits).

The input gradient is a per-pixel quantity: unlike a parameter gradient it is not a sum over the whole batch, so a discrete
choice that last-bit differences can flip -- a near-tie inside a MaxPool2d(2) window, a pre-activation at 0 -- moves one
pixel's value by far more than rounding does (seen: UtNet(16) with make_utnet_state_dict seed 7 at 120 pixels, 2e-3 with the
Winograd data gradients, 4e-7 with direct ones).  The cases below use weights and inputs without such near-ties; on them the
HIP input gradient is 4e-7 .. 1e-6 off float64."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from nind_denoise_amd import _lib, synth

REL = 1e-3
BAND = 3      # rows / columns 0 .. 2 and H-3 .. H-1: every pixel the reflection fold touches, plus the edge itself


# ---------------------------------------------------------------------------- CPU: the C ABI's new entry points

def test_abi_version_and_hw_train_workspace_sizes():
    lib = _lib.load()
    assert lib.nd_version() >= 106
    assert lib.nd_utnet_train_workspace_bytes_hw(8, 104, 152, 2) > 0
    assert lib.nd_utnet_train_workspace_bytes_hw(8, 104, 100, 2) == 0       # 100 is not 16k+56
    assert lib.nd_utnet_train_workspace_bytes_hw(8, 110, 104, 2) == 0
    assert lib.nd_utnet_train_workspace_bytes_hw(12, 104, 104, 2) == 0      # funit % 8 != 0
    assert lib.nd_utnet_train_workspace_bytes_hw(8, 104, 104, 0) == 0


# ---------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    _lib.load()
    return torch.device("cuda:0")


def _rel(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all()
    return (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)


def _band(t):
    """The 3-pixel border band of [..., H, W] as one flat tensor."""
    return torch.cat([t[..., :BAND, :].reshape(-1), t[..., -BAND:, :].reshape(-1),
                      t[..., BAND:-BAND, :BAND].reshape(-1), t[..., BAND:-BAND, -BAND:].reshape(-1)])


def _check_input_grad(got, ref, what):
    err = _rel(got, ref)
    assert err <= REL, (what, "x.grad", err)
    berr = _rel(_band(got.detach().cpu()), _band(ref))
    assert berr <= REL, (what, "x.grad border band", berr)
    return err, berr


def assert_close(y, ref, what=""):
    y, ref = y.detach().float().cpu(), ref.detach().float().cpu()
    assert y.shape == ref.shape and torch.isfinite(y).all(), what
    err = (y - ref).abs().max().item()
    assert err <= 1e-3 and err <= 1e-3 * max(ref.abs().max().item(), 1e-6), (what, err)


def _data(B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, h, w, generator=g)
    t = (x * 0.9 + 0.05 * torch.rand(B, 3, h, w, generator=g)).clip(0, 1)
    return x, t


def _oracle(sd, x, t, activation="PReLU", params_grad=True, x_grad=True):
    """float64 CPU autograd: (y, loss, params, x) with .grad set where requested."""
    from oracle import networks as onet
    params = {k: v.clone().double().requires_grad_(params_grad) for k, v in sd.items()}
    x = x.clone().double().requires_grad_(x_grad)
    y = onet.utnet_forward(params, x, activation=activation)
    loss = F.mse_loss(y.clip(0, 1), t.double())
    loss.backward()
    return y.detach(), loss.detach(), params, x


def _net(sd, funit, activation="PReLU"):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=funit, activation=activation)
    net.load_state_dict(sd)
    return net


@pytest.mark.gpu
@pytest.mark.parametrize("activation", ["PReLU", "ELU", "Hardswish"])
def test_input_grad_train_mode(dev, activation):
    funit, B, cs = 8, 2, 104
    sd = synth.make_utnet_state_dict(funit=funit, seed=31, activation=activation, gain=1.8)
    net = _net(sd, funit, activation).to(dev).train()
    x, t = _data(B, cs, cs, 3)
    xd = x.to(dev).requires_grad_()
    out = net(xd)
    loss = F.mse_loss(out.clip(0, 1), t.to(dev))
    loss.backward()
    y_ref, l_ref, params, xr = _oracle(sd, x, t, activation)
    assert_close(out, y_ref, f"forward {activation}")
    assert abs(loss.item() - l_ref.item()) <= 1e-5 * max(1.0, abs(l_ref.item()))
    err, berr = _check_input_grad(xd.grad, xr.grad, activation)
    for name, p in net.named_parameters():
        e = _rel(p.grad, params[name].grad)
        assert e <= REL, (activation, name, e)
    print(f"input grad {activation}: {err:.2e} (band {berr:.2e})")


@pytest.mark.gpu
def test_frozen_eval_network_gives_input_grad(dev):
    funit, B, cs = 16, 2, 120
    sd = synth.make_utnet_state_dict(funit=funit, seed=31, gain=1.8)
    net = _net(sd, funit).to(dev).eval()
    net.requires_grad_(False)
    x, t = _data(B, cs, cs, 5)
    xd = x.to(dev).requires_grad_()
    out = net(xd)
    assert out.requires_grad
    loss = F.mse_loss(out.clip(0, 1), t.to(dev))
    loss.backward()
    y_ref, _, _, xr = _oracle(sd, x, t, params_grad=False)
    assert_close(out, y_ref, "frozen eval forward")
    _check_input_grad(xd.grad, xr.grad, "frozen eval")
    assert all(p.grad is None for p in net.parameters())
    # no input gradient asked for: the inference path, as before (no graph)
    assert not net(x.to(dev)).requires_grad
    with torch.no_grad():
        assert not net(xd).requires_grad


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(104, 152), (152, 104)])
def test_rectangular_crops_under_autograd(dev, h, w):
    funit, B = 8, 2
    sd = synth.make_utnet_state_dict(funit=funit, seed=31, gain=1.8)
    net = _net(sd, funit).to(dev).train()
    x, t = _data(B, h, w, 9)
    xd = x.to(dev).requires_grad_()
    out = net(xd)
    F.mse_loss(out.clip(0, 1), t.to(dev)).backward()
    y_ref, _, params, xr = _oracle(sd, x, t)
    assert_close(out, y_ref, f"forward {h}x{w}")
    _check_input_grad(xd.grad, xr.grad, f"{h}x{w}")
    for name, p in net.named_parameters():
        e = _rel(p.grad, params[name].grad)
        assert e <= REL, (h, w, name, e)


@pytest.mark.gpu
def test_rectangular_fused_step_loss_crop_ssim(dev):
    from nind_denoise_amd.train import UtNetTrainer
    from oracle import losses as olosses
    from oracle import networks as onet
    funit, B, h, w, L = 8, 2, 104, 136, 96
    weights = {"MSE": 0.5, "SSIM": 0.5}
    sd = synth.make_utnet_state_dict(funit=funit, seed=19, gain=1.8)
    tr = UtNetTrainer(_net(sd, funit), device=dev, weights=weights, loss_cs=L)
    x, t = _data(B, h, w, 11)
    y, loss = tr.forward_backward(x, t)
    torch.cuda.synchronize()
    params = {k: v.clone().double().requires_grad_() for k, v in sd.items()}
    yr = onet.utnet_forward(params, x.double())
    y0, x0 = (h - L) // 2, (w - L) // 2            # pt_ops.pt_crop_batch
    g, tc = yr.clip(0, 1)[:, :, y0:y0 + L, x0:x0 + L], t.double()[:, :, y0:y0 + L, x0:x0 + L]
    lref = 0.5 * F.mse_loss(g, tc) + 0.5 * (1 - olosses.ssim(g, tc)).mean()
    lref.backward()
    assert_close(y, yr, "fused step forward")
    assert abs(loss.item() - lref.item()) <= 2e-5 * max(1.0, abs(lref.item())), (loss.item(), lref.item())
    for name, p in params.items():
        e = _rel(tr.grad_of(name), p.grad)
        assert e <= 2e-3, (name, e)     # the bar of test_training_step_loss_center_crop
    with pytest.raises(ValueError):     # the crop must fit the shorter side
        UtNetTrainer(_net(sd, funit), device=dev, weights=weights, loss_cs=h + 8).forward_backward(x, t)


@pytest.mark.gpu
def test_rectangular_autograd_matches_fused_step(dev):
    """Three Adam updates on 104x136 crops: the module under autograd + torch.optim.Adam against UtNetTrainer.  The first
    step's gradients are the same bits; after that the two Adam implementations round differently in the last bits, and Adam's
    per-element normalisation magnifies that on elements whose gradient is near eps (here up3.weight, |g| down to 2e-9)."""
    from nind_denoise_amd.train import UtNetTrainer
    funit, B, h, w, lr = 8, 2, 104, 136, 3e-3
    sd = synth.make_utnet_state_dict(funit=funit, seed=31, gain=1.8)
    ref_net = _net(sd, funit)
    tr = UtNetTrainer(ref_net, device=dev, lr=lr, beta1=0.75, weights={"L1": 0.0, "MSE": 1.0})
    net = _net(sd, funit).to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=lr, betas=(0.75, 0.999), amsgrad=True)
    g = torch.Generator().manual_seed(3)
    for step in range(3):
        x = torch.rand(B, 3, h, w, generator=g)
        t = (x * 0.9 + 0.05 * torch.rand(B, 3, h, w, generator=g)).clip(0, 1)
        y_ref, loss_ref = tr.forward_backward(x, t)
        loss_ref = loss_ref.item()
        opt.zero_grad()
        out = net(x.to(dev))
        loss = F.mse_loss(out.clip(0, 1), t.to(dev))
        loss.backward()
        if step == 0:
            for n, p in net.named_parameters():
                assert torch.equal(p.grad, tr.grad_of(n)), n
        tr.optimizer_step()
        opt.step()
        if step == 0:
            assert torch.equal(out.detach(), y_ref)
        else:
            assert (out.detach() - y_ref).abs().max().item() <= 1e-5, step
        assert abs(loss.item() - loss_ref) <= 1e-6 * max(1.0, abs(loss_ref)), (step, loss.item(), loss_ref)
    worst = max((p1.detach() - p2.detach()).abs().max().item() for p1, p2 in zip(net.parameters(), ref_net.parameters()))
    assert worst <= 0.05 * lr, worst     # (measured 8e-5: 3 % of one step)


def _flat_params(lib, sd, funit, dev):
    flat = torch.zeros(lib.nd_utnet_param_count(funit), dtype=torch.float32)
    for i, name in enumerate(_lib.utnet_tensor_names()):
        off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
        _lib.check(lib.nd_utnet_param_range(funit, i, off, cnt))
        flat[off.value:off.value + cnt.value] = sd[name].reshape(-1)
    return flat.to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, _lib.FLAG_NO_SPLITK])
def test_backward_param_and_input_grads_independent(dev, flags):
    """The backward's parameter gradients and input gradient do not depend on whether the other one was requested: bit for
    bit, and a backward without parameter gradients writes none."""
    lib = _lib.load()
    funit, B, cs = 8, 2, 104
    sd = synth.make_utnet_state_dict(funit=funit, seed=31, gain=1.8)
    params = _flat_params(lib, sd, funit, dev)
    x = _data(B, cs, cs, 3)[0].to(dev)
    nbytes = lib.nd_utnet_train_workspace_bytes_hw(funit, cs, cs, B)
    blobs = torch.empty(lib.nd_utnet_train_blob_bytes(funit), dtype=torch.uint8, device=dev)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    s = _lib.stream_ptr(dev)
    _lib.check(lib.nd_utnet_train_workspace_init_hw(ws.data_ptr(), nbytes, funit, cs, cs, B, s))
    act = _lib.ACT["PReLU"]
    gy = (torch.rand(B, 3, cs, cs, generator=torch.Generator().manual_seed(4)) - 0.5).to(dev)

    def halves(with_grads, with_dx):
        y, grads, dx = torch.empty_like(x), torch.zeros_like(params), torch.zeros_like(x)
        _lib.check(lib.nd_utnet_train_forward_hw(funit, act, flags, params.data_ptr(), blobs.data_ptr(), x.data_ptr(),
                                                 y.data_ptr(), B, cs, cs, ws.data_ptr(), nbytes, s))
        _lib.check(lib.nd_utnet_train_backward_hw(funit, act, flags, params.data_ptr(), grads.data_ptr() if with_grads else None,
                                                  blobs.data_ptr(), gy.data_ptr(), dx.data_ptr() if with_dx else None, B, cs,
                                                  cs, ws.data_ptr(), nbytes, s, None, 0))
        torch.cuda.synchronize()
        return grads, dx

    grads_only, both, dx_only = halves(True, False), halves(True, True), halves(False, True)
    assert torch.equal(both[0], grads_only[0])              # asking for dx leaves the parameter gradients alone
    assert torch.equal(both[1], dx_only[1]) and both[1].abs().max().item() > 0
    assert not dx_only[0].any()                              # grads = NULL: nothing written to a parameter gradient
    with pytest.raises(ValueError):                          # a backward asked for nothing
        _lib.check(lib.nd_utnet_train_backward_hw(funit, act, flags, params.data_ptr(), None, blobs.data_ptr(), gy.data_ptr(),
                                                  None, B, cs, cs, ws.data_ptr(), nbytes, s, None, 0))


@pytest.mark.gpu
def test_stacked_networks_train_end_to_end(dev):
    """net_b(net_a(x)): net_a trains through a frozen eval() net_b -- only possible if d loss / d input leaves net_b."""
    from oracle import networks as onet
    funit, B, cs = 8, 2, 104
    sd_a = synth.make_utnet_state_dict(funit=funit, seed=31, gain=1.8)
    sd_b = synth.make_utnet_state_dict(funit=funit, seed=17, gain=1.8)
    net_a = _net(sd_a, funit).to(dev).train()
    net_b = _net(sd_b, funit).to(dev).eval().requires_grad_(False)
    x, t = _data(B, cs, cs, 13)
    out = net_b(net_a(x.to(dev)))
    F.mse_loss(out.clip(0, 1), t.to(dev)).backward()
    pa = {k: v.clone().double().requires_grad_() for k, v in sd_a.items()}
    pb = {k: v.clone().double() for k, v in sd_b.items()}
    yr = onet.utnet_forward(pb, onet.utnet_forward(pa, x.double()))
    F.mse_loss(yr.clip(0, 1), t.double()).backward()
    assert_close(out, yr, "stacked forward")
    for name, p in net_a.named_parameters():
        assert p.grad is not None, name
        e = _rel(p.grad, pa[name].grad)
        assert e <= REL, (name, e)
    assert all(p.grad is None for p in net_b.parameters())
