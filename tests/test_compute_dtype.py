"""compute_dtype as a model parameter, on the GPU: the bf16 / fp16 blob packed on the device is the host packer's bit for bit,
and the CLI, the resident worker and denoise_dir run the 16-bit model that `--model_parameters ...,compute_dtype=...` asks for
-- the canvas pipeline.denoise_frame returns for UtNet.set_compute_dtype on the same frame -- and refuse a result that is not
finite.  The accuracy of those canvases is held to its PSNR bars by tests/test_hip_parity.py; nothing here adds a tolerance."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from nind_denoise_amd import _lib, pipeline, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, CS, UCS, OL = 310, 275, 120, 88, 16
GEOM = ["--cs", str(CS), "--ucs", str(UCS), "-ol", str(OL), "--exif_method", "noexif"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _lib.load()
    return torch.device("cuda:0")


def _net(funit, sd, dev, dtype):
    from nind_denoise_amd.networks.UtNet import UtNet
    net = UtNet(funit=funit)
    net.load_state_dict(sd)
    return net.eval().to(dev).set_compute_dtype(dtype)


def _special_weights(shape, seed, overflow=True, scale=1.0):
    """(special_weights of tests/test_compute_dtype_host.py) scale * randn with, planted at fixed strides: bf16 round-to-even
    ties (low 16 bits 0x8000, kept and rounded-up cases alike), fp16
    ties (low 13 bits 0x1000), fp16 subnormals (x 1e-6), values that round to zero in fp16 (x 1e-9), values past the fp16 range
    (x 1e5; optional) and -0.0."""
    w = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale).reshape(-1).contiguous()
    bits = w.view(torch.int32).clone()
    n = w.numel()
    idx = torch.arange(n)
    bits[idx % 11 == 0] = (bits[idx % 11 == 0] & ~0xffff) | 0x8000
    bits[idx % 11 == 1] = (bits[idx % 11 == 1] & ~0x1fff) | 0x1000
    w = bits.view(torch.float32).clone()
    w[idx % 11 == 2] *= 1e-6
    w[idx % 11 == 3] *= 1e-9
    if overflow:
        w[idx % 11 == 4] *= 1e5
    w[idx % 11 == 5] = -0.0
    return w.reshape(shape).contiguous()


def _planted_state_dict(funit, seed):
    """synth.make_utnet_state_dict with the tie / subnormal / underflow / -0.0 values of the host test planted in every weight."""
    sd = synth.make_utnet_state_dict(funit=funit, seed=seed)
    for k, key in enumerate(sorted(sd)):
        if key.endswith(".weight") and sd[key].dim() == 4:
            sp = _special_weights(sd[key].shape, seed=seed + k, overflow=False, scale=sd[key].abs().max().item())
            idx = torch.arange(sp.numel()).reshape(sp.shape) % 11
            sd[key] = torch.where(idx <= 5, sp, sd[key]).contiguous()
    return sd


def _pack(funit, dt, sd, where, dev):
    """The blob through the C ABI itself: nd_utnet_pack_weights (where = 'cpu') or nd_utnet_pack_weights_device."""
    lib = _lib.load()
    names = _lib.utnet_tensor_names()
    keep, ptrs = [], (ctypes.c_void_p * len(names))()
    for i, n in enumerate(names):
        keep.append(sd[n].detach().to(device=where, dtype=torch.float32).contiguous())
        ptrs[i] = keep[-1].data_ptr()
    nbytes = lib.nd_utnet_packed_bytes(funit, dt)
    assert nbytes > 0
    if str(where) == "cpu":
        blob = torch.empty(nbytes // 4, dtype=torch.float32)
        _lib.check(lib.nd_utnet_pack_weights(funit, dt, ptrs, len(names), blob.data_ptr(), nbytes), "nd_utnet_pack_weights")
        return blob
    blob = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.nd_utnet_pack_weights_device(funit, dt, ptrs, len(names), blob.data_ptr(), nbytes, _lib.stream_ptr(dev)),
                   "nd_utnet_pack_weights_device")
        torch.cuda.synchronize()
    return blob.cpu()


@pytest.mark.parametrize("funit", [16, 48, 64])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_device_packed_16bit_blob_is_the_host_blob(dev, dtype, funit):
    """funit 48 (packing only): 48 and 96 output channels are no multiples of 32, 48 input channels make three K blocks."""
    sd = _planted_state_dict(funit, seed=5)
    w = sd["convs2.0.weight"]
    assert ((w.view(torch.int32) & 0xffff) == 0x8000).any() and (w.view(torch.int32) == -2 ** 31).any()      # (planted)
    dt = _lib.DTYPE[dtype]
    b_host = _pack(funit, dt, sd, "cpu", dev).view(torch.int32)
    b_dev = _pack(funit, dt, sd, dev, dev).view(torch.int32)
    same = b_host.shape == b_dev.shape and torch.equal(b_dev, b_host)       # (a plain bool: pytest must not render the blobs)
    assert same, f"{int((b_dev != b_host).sum())} of {b_host.numel()} words differ"
    if funit == 48:
        return
    # the same through the module: pack_on_device governs the 16-bit types too
    net = _net(funit, sd, dev, dtype)
    assert net.pack_on_device
    m_dev = net.packed_weights(dev).cpu().view(torch.int32)
    net.pack_on_device = False
    net._packed.clear()
    m_host = net.packed_weights(dev).cpu().view(torch.int32)
    ok = torch.equal(m_dev, b_host) and torch.equal(m_host, b_host)
    assert ok


@pytest.mark.parametrize("funit,cs", [(16, 120), (64, 264)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_forward_is_the_same_with_either_blob(dev, dtype, funit, cs):
    net = _net(funit, synth.make_utnet_state_dict(funit=funit, seed=3), dev, dtype)
    net.split_k = False
    x = torch.rand(2, 3, cs, cs, generator=torch.Generator().manual_seed(1)).to(dev)
    y_dev = net(x).clone()
    net.pack_on_device = False
    net._packed.clear()
    y_host = net(x).clone()
    ok = bool(torch.isfinite(y_dev).all()) and torch.equal(y_dev, y_host)
    assert ok


# ---------------------------------------------------------------------------- callers

def _fixture(tmp_path, sd=None, seed=8):
    from nind_denoise_amd.common.libs import imgcodec
    sd = synth.make_utnet_state_dict(funit=16, seed=21) if sd is None else sd
    torch.save(sd, tmp_path / "generator_650.pt")
    frame = synth.make_frame(W, H, seed=seed)
    imgcodec.write_tiff(str(tmp_path / "in.tif"), np.ascontiguousarray(frame.transpose(1, 2, 0)))
    return sd, frame


def _cli(tmp_path, out, params, extra=()):
    from nind_denoise_amd import denoise_image as di
    return di.main(["--network", "UtNet", "--model_path", str(tmp_path / "generator_650.pt"), "--model_parameters", params,
                    "--input", str(tmp_path / "in.tif"), "--output", str(tmp_path / out)] + GEOM + list(extra))


def test_cli_runs_the_model_the_parameter_asks_for(dev, tmp_path):
    from nind_denoise_amd.common.libs import np_imgops
    sd, frame = _fixture(tmp_path)
    img = torch.from_numpy(frame).to(dev)
    assert _cli(tmp_path, "f32.tiff", "funit=16") == 0
    f32 = np_imgops.img_path_to_np_flt(str(tmp_path / "f32.tiff"))
    for dtype in ("bf16", "f16"):
        assert _cli(tmp_path, f"{dtype}.tiff", f"funit=16,compute_dtype={dtype}") == 0
        got = np_imgops.img_path_to_np_flt(str(tmp_path / f"{dtype}.tiff"))
        want = pipeline.denoise_frame(_net(16, sd, dev, dtype), img, CS, UCS, OL, batch=64).cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, want), dtype
        assert not np.array_equal(got, f32), f"compute_dtype={dtype} was ignored"
    # --whole_image: the frame's 264 x 248 corner through net(x)
    from nind_denoise_amd.common.libs import imgcodec
    crop = np.ascontiguousarray(frame[:, :248, :264])
    imgcodec.write_tiff(str(tmp_path / "in.tif"), np.ascontiguousarray(crop.transpose(1, 2, 0)))
    assert _cli(tmp_path, "whole.tiff", "funit=16,compute_dtype=bf16", ["--whole_image"]) == 0
    got = np_imgops.img_path_to_np_flt(str(tmp_path / "whole.tiff"))
    want = _net(16, sd, dev, "bf16")(torch.from_numpy(crop).to(dev)[None])[0].cpu().numpy()
    assert np.array_equal(got, want)
    assert _cli(tmp_path, "whole32.tiff", "funit=16", ["--whole_image"]) == 0
    assert not np.array_equal(got, np_imgops.img_path_to_np_flt(str(tmp_path / "whole32.tiff")))


def test_cli_ends_with_a_message_for_a_funit_the_type_cannot_take(dev, tmp_path):
    _fixture(tmp_path, sd=synth.make_utnet_state_dict(funit=8, seed=21))
    with pytest.raises(SystemExit) as e:
        _cli(tmp_path, "out.tiff", "funit=8,compute_dtype=bf16")
    assert "funit=8" in str(e.value.code) and "16" in str(e.value.code) and not os.path.exists(tmp_path / "out.tiff")


class _Worker:
    """One `python -m nind_denoise_amd.serve` process and its thin clients."""

    def __init__(self, tmp_path):
        self.tmp, self.sock = tmp_path, str(tmp_path / "w.sock")
        self.env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        self.proc = subprocess.Popen([sys.executable, "-m", "nind_denoise_amd.serve", "--socket", self.sock], env=self.env, cwd=ROOT,
                                     stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)

    def __enter__(self):
        t0 = time.time()
        while not os.path.exists(self.sock):
            assert self.proc.poll() is None, self.proc.stdout.read()
            assert time.time() - t0 < 180, "worker did not come up"
            time.sleep(0.1)
        return self

    def denoise(self, out, params):
        return subprocess.run([sys.executable, "-m", "nind_denoise_amd.denoise_image", "--network", "UtNet", "--model_path",
                               "generator_650.pt", "--model_parameters", params, "--input", "in.tif", "--output", out] + GEOM
                              + ["--server", self.sock], env=self.env, cwd=self.tmp, capture_output=True, text=True, timeout=300)

    def client(self, what):
        return subprocess.run([sys.executable, "-m", "nind_denoise_amd.client", "--server", self.sock, what], env=self.env,
                              cwd=self.tmp, capture_output=True, text=True, timeout=60)

    def __exit__(self, *exc):
        try:
            if self.proc.poll() is None and exc[0] is None:
                assert self.client("--shutdown").returncode == 0
                assert self.proc.wait(timeout=60) == 0
        finally:
            if self.proc.poll() is None:
                self.proc.kill()
                self.proc.wait()


def _same_file(a, b):
    with open(a, "rb") as f1, open(b, "rb") as f2:
        return f1.read() == f2.read()


def test_worker_keeps_one_model_per_compute_dtype(dev, tmp_path):
    _fixture(tmp_path)
    assert _cli(tmp_path, "cli_f32.tiff", "funit=16") == 0
    assert _cli(tmp_path, "cli_bf16.tiff", "funit=16,compute_dtype=bf16") == 0
    assert not _same_file(tmp_path / "cli_f32.tiff", tmp_path / "cli_bf16.tiff")
    with _Worker(tmp_path) as w:
        for k, (params, ref) in enumerate((("funit=16", "cli_f32.tiff"), ("funit=16,compute_dtype=bf16", "cli_bf16.tiff"),
                                           ("funit=16", "cli_f32.tiff"))):
            r = w.denoise(f"w{k}.tiff", params)
            assert r.returncode == 0, r.stdout + r.stderr
            assert _same_file(tmp_path / f"w{k}.tiff", tmp_path / ref), (k, params)
        r = w.client("--ping")
        assert r.returncode == 0 and "3 request(s) served, 2 model(s) resident" in r.stdout, r.stdout + r.stderr


def test_denoise_dir_scores_the_16bit_model(dev, tmp_path):
    from nind_denoise_amd import denoise_dir, denoise_image
    from nind_denoise_amd.common.libs import imgcodec, pt_helpers, utilities
    sd = synth.make_utnet_state_dict(funit=16, seed=4)
    mdir = tmp_path / "models" / "run_utnet"
    mdir.mkdir(parents=True)
    torch.save(sd, str(mdir / "generator_7.pt"))
    noisy = tmp_path / "ds" / "NIND_120_88"
    rng = np.random.default_rng(0)
    for aset, (w, h) in (("bike", (230, 200)), ("tree", (250, 190))):
        (noisy / aset).mkdir(parents=True)
        clean = synth.make_frame(w, h, seed=len(aset))
        for iso, sigma in (("ISO200", 0.0), ("ISO3200", 0.05), ("ISOH1", 0.1)):
            img = np.clip(clean + sigma * rng.standard_normal(clean.shape).astype(np.float32), 0, 1)
            imgcodec.write_png(str(noisy / aset / f"NIND_{aset}_{iso}.png"), (img * 65535).round().astype(np.uint16).transpose(1, 2, 0))

    def run(params, results):
        return denoise_dir.main(["--model_path", str(mdir / "generator_7.pt"), "--network", "UtNet", "--model_parameters", params,
                                 "--cs", str(CS), "--ucs", str(UCS), "-ol", str(OL), "--noisy_dir", str(noisy),
                                 "--result_dir", str(tmp_path / results), "--config", "/nonexistent.yaml"])
    res16 = run("funit=16,compute_dtype=f16", "r16")
    res32 = run("funit=16", "r32")
    # the same denoise and score functions, handed the model built through the Python API
    net = _net(16, sd, dev, "f16")
    per_set = []
    for aset in ("bike", "tree"):
        per_img = []
        for iso in ("ISO3200", "ISOH1"):
            out = str(tmp_path / f"api_{aset}_{iso}.png")
            denoise_image.denoise_file(net, str(noisy / aset / f"NIND_{aset}_{iso}.png"), out, CS, UCS, OL, batch=64, device=dev,
                                       verbose=False)
            per_img.append(pt_helpers.get_losses(str(noisy / aset / f"NIND_{aset}_ISO200.png"), out, device=dev))
        per_set.append(utilities.avg_listofdicts(per_img))
    want = utilities.avg_listofdicts(per_set)
    assert set(res16) == {"mse", "ssim", "msssim"} and res16 == want, (res16, want)
    assert res16 != res32, "compute_dtype=f16 was ignored"


def test_non_finite_16bit_result_is_refused(dev, tmp_path, capsys):
    """A checkpoint whose first layer lies beyond the fp16 range: its weights become fp16 infinities in the packed blob, bf16 and
    fp32 hold them.  Arithmetic overflow in stored values; no kernel traps."""
    from nind_denoise_amd import denoise_image
    sd = synth.make_utnet_state_dict(funit=16, seed=21)
    w0 = sd["convs1.0.weight"]
    sd["convs1.0.weight"] = w0 * (1e7 / w0.abs().max().item())
    assert (sd["convs1.0.weight"].abs() > 65504).float().mean().item() > 0.5
    _, frame = _fixture(tmp_path, sd=sd)
    img = torch.from_numpy(frame).to(dev)
    # precondition, on the Python-API path
    c16 = pipeline.denoise_frame(_net(16, sd, dev, "f16"), img, CS, UCS, OL, batch=64)
    cbf = pipeline.denoise_frame(_net(16, sd, dev, "bf16"), img, CS, UCS, OL, batch=64)
    bad16, badbf = int((~torch.isfinite(c16)).sum()), int((~torch.isfinite(cbf)).sum())
    with capsys.disabled():
        print(f"non-finite samples of {c16.numel()}: f16 {bad16}, bf16 {badbf}")
    assert bad16 > 0 and badbf == 0, (bad16, badbf)
    with pytest.raises(FloatingPointError, match="use bf16 or f32"):
        denoise_image.denoise_file(_net(16, sd, dev, "f16"), str(tmp_path / "in.tif"), str(tmp_path / "api.tiff"), CS, UCS, OL,
                                   batch=64, device=dev, verbose=False)
    assert not os.path.exists(tmp_path / "api.tiff")
    capsys.readouterr()
    assert _cli(tmp_path, "bad.tiff", "funit=16,compute_dtype=f16") != 0
    err = capsys.readouterr().err
    assert "compute_dtype=f16" in err and f"{bad16} of {c16.numel()}" in err and "use bf16 or f32" in err
    assert not os.path.exists(tmp_path / "bad.tiff")
    assert _cli(tmp_path, "ok.tiff", "funit=16,compute_dtype=bf16") == 0 and os.path.isfile(tmp_path / "ok.tiff")
    with _Worker(tmp_path) as w:
        r = w.denoise("wbad.tiff", "funit=16,compute_dtype=f16")
        assert r.returncode != 0 and "use bf16 or f32" in r.stderr and not os.path.exists(tmp_path / "wbad.tiff"), r.stdout + r.stderr
        r = w.denoise("wok.tiff", "funit=16,compute_dtype=bf16")
        assert r.returncode == 0 and _same_file(tmp_path / "wok.tiff", tmp_path / "ok.tiff"), r.stdout + r.stderr
