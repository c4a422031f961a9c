"""Host-side tests of the guarded optimizer step (no GPU): the three exports in the header and in _lib, what the header says about
them, the argument checks that come before any launch, the workspace size as a function of n alone, the parsing and the refusals
of the command's three options, and the epoch figures computed from the steps' guard states."""
import os
import re

import pytest
import torch

from nind_denoise_amd import _lib, nn_train

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("nd_grad_guard_workspace_bytes", "nd_grad_guard", "nd_adam_step_guarded")
BASE = ["--test_reserve", "0"]


def header():
    with open(os.path.join(ROOT, "include", "nind_hip.h")) as f:
        return f.read()


def test_exports_in_header_and_binding():
    lib = _lib.load()
    assert lib.nd_version() >= 119
    declared = set(re.findall(r"\b(nd_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", header(), flags=re.S)))
    for name in NEW_EXPORTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "nd_adam_step" in declared            # the unguarded step stays


def test_header_states_the_semantics():
    text = " ".join(re.sub(r"\n \* ?", " ", header()).split())
    for phrase in ("GradScaler", "counts attempts", "grads is NOT modified", "clip_grad_norm_", "no atomics", "ok == 0"):
        assert phrase in text, phrase


def test_workspace_is_a_function_of_n():
    lib = _lib.load()
    ws = lib.nd_grad_guard_workspace_bytes
    assert ws(0) == 0
    assert ws(1) == ws(3) == ws(1024) == ws(1027) == 16           # one workgroup of 256 16-byte elements: two doubles
    assert ws(1028) == 32 and ws(1000003) == 977 * 16
    assert ws(31 * 10 ** 6) == ws(10 ** 9) == 1024 * 16           # the grid stops growing at 1024 workgroups


def test_argument_checks_come_before_any_launch():
    lib = _lib.load()
    import ctypes
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    assert lib.nd_grad_guard(None, 8, 1.0, 0, p, p, 512, None) == -1
    assert b"nd_grad_guard" in lib.nd_last_error()
    assert lib.nd_grad_guard(p, 0, 1.0, 0, p, p, 512, None) == -1
    assert lib.nd_grad_guard(p, 8, 1.0, 0, None, p, 512, None) == -1
    assert lib.nd_grad_guard(p, 8, 1.0, 0, p, None, 512, None) == -1
    assert lib.nd_grad_guard(p + 4, 8, 1.0, 0, p, p, 512, None) == -1 and b"aligned" in lib.nd_last_error()
    assert lib.nd_grad_guard(p, 8, 1.0, 0, p, p, 8, None) == -1 and b"workspace" in lib.nd_last_error()
    assert lib.nd_adam_step_guarded(p, p, p, p, p, 8, 1e-3, 0.75, 0.999, 1e-8, 1, 1, None, None) == -1
    assert lib.nd_adam_step_guarded(p, p, p, p, p, 8, 1e-3, 0.75, 0.999, 1e-8, 0, 1, p, None) == -1
    assert lib.nd_adam_step_guarded(p, p, p, p, None, 8, 1e-3, 0.75, 0.999, 1e-8, 1, 1, p, None) == -1
    assert b"nd_adam_step_guarded" in lib.nd_last_error()


def test_options_parse():
    args = nn_train.parse_args(BASE)
    assert args.g_clip_norm is None and args.skip_nonfinite_steps is False and args.max_skipped_steps is None
    assert args.save_state is False and args.resume is None
    nn_train.check_supported(args)
    args = nn_train.parse_args(BASE + ["--g_clip_norm", "0.5", "--skip_nonfinite_steps", "--max_skipped_steps", "3", "--save_state"])
    assert (args.g_clip_norm, args.skip_nonfinite_steps, args.max_skipped_steps, args.save_state) == (0.5, True, 3, True)
    nn_train.check_supported(args)


def test_options_from_a_config_file(tmp_path):
    conf = tmp_path / "conf.yaml"
    conf.write_text("g_clip_norm: 2\nskip_nonfinite_steps: true\nmax_skipped_steps: 0\ntest_reserve: ['0']\n")
    args = nn_train.parse_args(["--config", str(conf)])
    assert args.g_clip_norm == 2.0 and isinstance(args.g_clip_norm, float) and args.skip_nonfinite_steps is True
    assert args.max_skipped_steps == 0
    nn_train.check_supported(args)


@pytest.mark.parametrize("argv,match", [
    (["--max_skipped_steps", "2"], "needs --skip_nonfinite_steps"),
    (["--skip_nonfinite_steps", "--max_skipped_steps", "-1"], "max_skipped_steps -1"),
    (["--g_clip_norm", "0"], "g_clip_norm"),
    (["--g_clip_norm", "-1"], "g_clip_norm"),
    (["--g_clip_norm", "inf"], "g_clip_norm"),
    (["--g_clip_norm", "nan"], "g_clip_norm"),
])
def test_options_refused(argv, match):
    with pytest.raises(ValueError, match=match):
        nn_train.check_supported(nn_train.parse_args(BASE + argv))


def test_guard_summary():
    rows = torch.tensor([[4.0, 0, 0.5, 1],          # norm 2, clipped
                         [float("nan"), 3, float("nan"), 0],    # skipped
                         [16.0, 0, 1.0, 1],         # norm 4, not clipped
                         [float("inf"), 1, 0.0, 0],             # skipped
                         [1.0, 0, 0.25, 1]], dtype=torch.float64)
    assert nn_train.guard_summary(rows) == (3, 2, 2, 7.0 / 3.0, 4.0)
    applied, skipped, clipped, mean, worst = nn_train.guard_summary(rows[[1, 3]])
    assert (applied, skipped, clipped) == (0, 2, 0) and mean != mean and worst != worst


def test_train_epoch_keeps_todays_signature_first():
    """the new argument is last and optional: a caller of today's train_epoch is served as before"""
    import inspect
    params = list(inspect.signature(nn_train.train_epoch).parameters)
    assert params[:11] == ["pool", "trainer", "batch_size", "losses", "ssim_losses", "exp_mult_min", "exp_mult_max", "rank", "world",
                           "log_interval", "log"] and params[11:] == ["guard_log"]
