"""The reference's own SSIM (libs/pytorch_ssim) on the GPU against the fixture its pytorch_ssim generated on the CPU
(tests/golden/pytorch_ssim.npz, made by tests/golden/make_golden_ssim.py), forward and gradient; loss.gen_score and
denoise_dir --gen_score end to end.

Bars.  The fixture stores, per case, the reference's float32 result, a float64 evaluation of the same functions and their
distance: the reference's own float32 error.  A GPU score may be 10 x the largest such distance from float64 (the margin covers
another summation order: tile partials instead of one mean), a gradient 10 x the largest stored relative distance, relative to
max|g64|.  Constant images are apart: E[x^2] - mu^2 cancels to rounding noise against C2 = 9e-4, and the reference's own float32
is 1e-4 off there; their bar is 5e-4.  MSE: a float32 sum of K = 3 * 70 * 90 non-negative terms in blocks is within about
(log2 K + 5) * 2^-24 = 1.2e-6 of its value, relatively; the bar is 2e-6 relative to the float64 value."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from nind_denoise_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pytorch_ssim.npz")
FX = np.load(GOLDEN)
INDEX = json.loads(bytes(FX["index"]))
GRADS = json.loads(bytes(FX["grads"]))
FILES = json.loads(bytes(FX["files"]))
BAR = 10 * max(float(FX["dist"][i]) for i, c in enumerate(INDEX) if c["group"] == "tight")      # about 2e-6
GRAD_BAR = 10 * max(g["rel"] for g in GRADS)                                                       # about 4e-5, relative
CONST_BAR = 5e-4
MSE_REL_BAR = 2e-6
SCORE_TOL = 2e-5            # the project's bar for fp32 scores (test_eval_harness.py)
ND_EINVAL, ND_ENOMEM = -1, -2

_pairs = {}


def pair(case, dev):
    """the case's inputs on the device, built once per module run and never written"""
    if case["id"] not in _pairs:
        x, y = synth.make_ssim_pair(*case["shape"], case["kind"], case["seed"])
        _pairs[case["id"]] = (torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev))
    return _pairs[case["id"]]


def case_by_id(cid):
    return next((i, c) for i, c in enumerate(INDEX) if c["id"] == cid)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests need a real MI355X")
    from nind_denoise_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def pssim():
    from nind_denoise_amd.libs import pytorch_ssim
    return pytorch_ssim


def test_bars_come_from_the_fixture():
    assert 0 < BAR <= SCORE_TOL and BAR <= 10 * float(FX["tight_cap"])
    assert 0 < GRAD_BAR <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in INDEX])
def test_scores_match_float64(dev, pssim, cid):
    i, c = case_by_id(cid)
    x, y = pair(c, dev)
    n, ws = c["shape"][0], c["window"]
    want_vec, want_mean = FX["score64"][c["off"]:c["off"] + n], float(FX["mean64"][i])
    bar = BAR if c["group"] == "tight" else CONST_BAR
    got = {"fn_vec": pssim.ssim(x, y, window_size=ws, size_average=False), "fn_mean": pssim.ssim(x, y, window_size=ws),
           "mod_vec": pssim.SSIM(window_size=ws, size_average=False)(x, y), "mod_mean": pssim.SSIM(window_size=ws)(x, y)}
    for k, v in got.items():
        assert v.dtype == torch.float32 and v.device == x.device
        if k.endswith("vec"):
            assert tuple(v.shape) == (n,)
            err = float(np.abs(v.cpu().numpy().astype(np.float64) - want_vec).max())
        else:
            assert v.dim() == 0
            err = abs(v.item() - want_mean)
        print(f"{cid} {k}: |gpu - f64| = {err:.3e} (bar {bar:.3e}; the reference's own {float(FX['dist'][i]):.3e})")
        assert err <= bar, (cid, k, err, bar)
    assert torch.equal(got["fn_vec"], got["mod_vec"]) and torch.equal(got["fn_mean"], got["mod_mean"])
    if c["group"] == "tight":
        one = pssim.ssim(x, x, window_size=ws, size_average=False)
        assert (one - 1).abs().max().item() <= 1e-6
        swapped = pssim.ssim(y, x, window_size=ws, size_average=False)
        assert (swapped - got["fn_vec"]).abs().max().item() <= BAR


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRADS, ids=[g["id"] for g in GRADS])
def test_gradients_match_float64(dev, pssim, g):
    _, c = case_by_id(g["id"])
    x, y = pair(c, dev)
    n = c["shape"][0]
    g64 = FX["grad64"][g["off"]:g["off"] + g["count"]].astype(np.float64).reshape(c["shape"])
    scale = np.abs(g64).max()
    wvec = torch.linspace(0.5, 1.5, n).to(dev)
    xr = x.clone().requires_grad_()
    ((1 - pssim.ssim(xr, y, size_average=False)) * wvec).sum().backward()
    assert xr.grad.shape == x.shape and xr.grad.dtype == torch.float32 and torch.isfinite(xr.grad).all()
    err = float(np.abs(xr.grad.cpu().numpy().astype(np.float64) - g64).max() / scale)
    print(f"{g['id']}: max|g - g64| / max|g64| = {err:.3e} (bar {GRAD_BAR:.3e}; the reference's own {g['rel']:.3e})")
    assert err <= GRAD_BAR
    # size_average=True is the vector path with weights 1 / N
    xm = x.clone().requires_grad_()
    pssim.SSIM()(xm, y).backward()
    xv = x.clone().requires_grad_()
    (pssim.ssim(xv, y, size_average=False) * torch.full((n,), 1.0 / n, device=dev)).sum().backward()
    gscale = xv.grad.abs().max().item()
    assert gscale > 0 and (xm.grad - xv.grad).abs().max().item() / gscale <= GRAD_BAR


@pytest.mark.gpu
def test_two_calls_are_bit_equal(dev, pssim):
    for cid in ("n1c3h97w130_ws11_noisy", "n3c3h64w48_ws11_indep"):
        x, y = pair(case_by_id(cid)[1], dev)
        runs = []
        for _ in range(2):
            xr = x.clone().requires_grad_()
            s = pssim.ssim(xr, y, size_average=False)
            (s * torch.linspace(0.5, 1.5, s.numel()).to(dev)).sum().backward()
            runs.append((s.detach().clone(), xr.grad.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.gpu
def test_non_contiguous_and_fp16_inputs(dev, pssim):
    x, y = pair(case_by_id("n1c3h97w130_ws11_noisy")[1], dev)
    xn, yn = x.transpose(2, 3)[..., ::2], y.transpose(2, 3)[..., ::2]          # [1,3,130,49], strided both ways
    assert not xn.is_contiguous()
    assert torch.equal(pssim.ssim(xn, yn, size_average=False), pssim.ssim(xn.contiguous(), yn.contiguous(), size_average=False))
    xh, yh = x.half(), y.half()
    assert torch.equal(pssim.ssim(xh, yh), pssim.ssim(xh.float(), yh.float()))
    xr = xh.clone().requires_grad_()              # the gradient comes back in the input's dtype
    pssim.ssim(xr, yh).backward()
    xf = xh.float().requires_grad_()
    pssim.ssim(xf, yh.float()).backward()
    assert xr.grad.dtype == torch.float16 and torch.equal(xr.grad, xf.grad.half())


@pytest.mark.gpu
def test_img2_gradient_is_refused(dev, pssim):
    x, y = pair(case_by_id("n1c3h5w7_ws11_noisy")[1], dev)
    with pytest.raises(NotImplementedError, match="img2"):
        pssim.ssim(x, y.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="img2"):
        pssim.SSIM()(x.clone().requires_grad_(), y.clone().requires_grad_())
    with pytest.raises(ValueError, match="window_size"):
        pssim.ssim(x, y, window_size=4)


@pytest.mark.gpu
def test_c_abi_argument_checks(dev):
    """a window of 4 or 13 -> ND_EINVAL, a workspace one byte short -> ND_ENOMEM, and nothing is launched: the outputs keep
    their sentinel"""
    from nind_denoise_amd import _lib
    lib = _lib.load()
    x, y = pair(case_by_id("n2c3h32w32_ws11_noisy")[1], dev)
    n, c, h, w = x.shape
    need = lib.nd_ssim_padded_workspace_bytes(n, c, h, w, 11)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((n,), -7.0, device=dev)
    gout = torch.ones(n, device=dev)
    gx = torch.full_like(x, -7.0)
    s = _lib.stream_ptr(dev)

    def fwd(window, nbytes):
        return lib.nd_ssim_padded(x.data_ptr(), y.data_ptr(), n, c, h, w, window, out.data_ptr(), ws.data_ptr(), nbytes, s)

    def bwd(window, nbytes):
        return lib.nd_ssim_padded_grad(x.data_ptr(), y.data_ptr(), n, c, h, w, window, gout.data_ptr(), gx.data_ptr(), ws.data_ptr(),
                                       nbytes, s)
    for call in (fwd, bwd):
        for window in (4, 13, 1, 0, -11):
            assert call(window, need) == ND_EINVAL
            assert b"window" in lib.nd_last_error()
        assert call(11, need - 1) == ND_ENOMEM
        assert b"workspace" in lib.nd_last_error()
    assert lib.nd_ssim_padded(x.data_ptr(), y.data_ptr(), n, c, 0, w, 11, out.data_ptr(), ws.data_ptr(), need, s) == ND_EINVAL
    torch.cuda.synchronize()
    assert (out == -7).all() and (gx == -7).all()
    assert fwd(11, need) == 0 and bwd(11, need) == 0
    torch.cuda.synchronize()
    assert (out != -7).all() and (gx != -7).all()


def _write_png8(path, chw):
    from PIL import Image
    Image.fromarray(np.round(chw * 255).astype(np.uint8).transpose(1, 2, 0)).save(path)


@pytest.mark.gpu
def test_gen_score_end_to_end(dev, tmp_path):
    """two ground-truth sets of three 8-bit PNGs, their noisy files flat in one directory: res.txt holds the reference's numbers"""
    from nind_denoise_amd import loss
    gt_dir, noisy_dir = tmp_path / "gt", tmp_path / "denoised"
    noisy_dir.mkdir()
    want = {}
    for aset, d in FILES.items():
        (gt_dir / aset).mkdir(parents=True)
        gt = None
        for f in d["files"]:
            x, y = synth.make_ssim_pair(1, 3, d["h"], d["w"], "q8", d["seed"], sigma=f["sigma"] or 0.05)
            name = f"NIND_{aset}_{f['iso']}.png"
            if f["sigma"] is None:
                gt = x
                _write_png8(str(gt_dir / aset / name), x[0])
                continue
            h = hashlib.sha256()
            h.update(gt.tobytes())
            h.update(y.tobytes())
            assert h.hexdigest() == f["sha"]
            _write_png8(str(gt_dir / aset / name), y[0])
            _write_png8(str(noisy_dir / name), y[0])
            want[name] = f
    res = loss.gen_score(str(noisy_dir), str(gt_dir), device=dev)
    assert [r[0] for r in res] == sorted(want) and len(res) == 4
    lines = open(noisy_dir / "res.txt").read().splitlines()
    assert len(lines) == 4
    for line, r in zip(lines, res):
        name, s, m = line.split(",")
        assert (name, float(s), float(m)) == r
        f = want[name]
        print(f"{name}: ssim {float(s)!r} (f64 {f['ssim64']!r}, reference fp32 {f['ssim32']!r}); mse {float(m)!r} (f64 {f['mse64']!r})")
        assert abs(float(s) - f["ssim64"]) <= BAR
        assert abs(float(m) - f["mse64"]) <= MSE_REL_BAR * f["mse64"]
    again = loss.gen_score(str(noisy_dir), str(gt_dir), device=dev)       # res.txt is in the directory now and is not scored
    assert again == res and open(noisy_dir / "res.txt").read().splitlines() == lines


@pytest.mark.gpu
def test_denoise_dir_gen_score_flag(dev, pssim, tmp_path):
    """denoise_dir on a one-set directory: with --gen_score it writes res.txt beside the outputs (the score of the written file
    against the set's base ISO), without the flag it does not"""
    from nind_denoise_amd import denoise_dir, loss
    from nind_denoise_amd.common.libs import imgcodec
    sd = synth.make_utnet_state_dict(funit=16, seed=4)
    mdir = tmp_path / "models" / "run_utnet"
    mdir.mkdir(parents=True)
    torch.save(sd, str(mdir / "generator_7.pt"))
    noisy = tmp_path / "ds" / "NIND_120_88"
    (noisy / "bike").mkdir(parents=True)
    clean = synth.make_frame(200, 170, seed=4)      # MS-SSIM of get_losses needs 161 pixels per side
    rng = np.random.default_rng(0)
    for iso, sigma in (("ISO200", 0.0), ("ISO3200", 0.05)):
        img = np.clip(clean + sigma * rng.standard_normal(clean.shape).astype(np.float32), 0, 1)
        imgcodec.write_png(str(noisy / "bike" / f"NIND_bike_{iso}.png"), (img * 65535).round().astype(np.uint16).transpose(1, 2, 0))
    common = ["--model_path", str(mdir / "generator_7.pt"), "--network", "UtNet", "--model_parameters", "funit=16", "--cs", "120",
              "--ucs", "88", "-ol", "16", "--noisy_dir", str(noisy), "--config", "/nonexistent.yaml"]
    denoise_dir.main(common + ["--result_dir", str(tmp_path / "plain")])
    assert sorted(os.listdir(tmp_path / "plain" / "run_utnet")) == ["NIND_bike_ISO3200.png"]
    denoise_dir.main(common + ["--result_dir", str(tmp_path / "scored"), "--gen_score"])
    outdir = tmp_path / "scored" / "run_utnet"
    assert sorted(os.listdir(outdir)) == ["NIND_bike_ISO3200.png", "res.txt"]
    (line,) = open(outdir / "res.txt").read().splitlines()
    name, s, m = line.split(",")
    gt = loss.read_image(str(noisy / "bike" / "NIND_bike_ISO200.png"), dev)
    got = loss.read_image(str(outdir / name), dev)
    assert name == "NIND_bike_ISO3200.png" and float(s) == pssim.ssim(gt, got).item() and 0 < float(s) < 1 and float(m) > 0
