"""fallback_dtype on the host: the model parameter's spellings and pairs (constructor, setter, instantiate_model), the grouping of
bad tiles into runs, the report and the line the callers print, and the declaration of the checked frame entry.  No GPU call."""
import os
import re

import pytest
import torch

from nind_denoise_amd import _lib, pipeline, synth
from nind_denoise_amd.networks.UtNet import UtNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALLOWED = [("f16", "bf16"), ("f16", "f32"), ("bf16", "f32")]
REFUSED = [("f32", "f32"), ("f32", "bf16"), ("f32", "f16"), ("bf16", "bf16"), ("bf16", "f16"), ("f16", "f16")]
SPELLINGS = {"f32": ("f32", "fp32", "float32"), "bf16": ("bf16", "bfloat16"), "f16": ("f16", "fp16", "float16")}


def test_off_by_default_and_its_spellings():
    assert UtNet(funit=16).fallback_dtype is None
    for off in (None, "", "none", "None"):
        for cd in ("f32", "bf16", "f16"):
            net = UtNet(funit=16, compute_dtype=cd, fallback_dtype=off)
            assert net.fallback_dtype is None and net.checked_fallback_dtype() is None
            assert net.set_fallback_dtype(off) is net and net.fallback_dtype is None


@pytest.mark.parametrize("cd,fb", ALLOWED)
def test_allowed_pairs_in_every_spelling(cd, fb):
    for c in SPELLINGS[cd]:
        for f in SPELLINGS[fb]:
            net = UtNet(funit=16, compute_dtype=c, fallback_dtype=f)
            assert (net.compute_dtype, net.fallback_dtype) == (cd, fb)
            net = UtNet(funit=16, compute_dtype=c)
            assert net.set_fallback_dtype(f) is net and net.fallback_dtype == fb and net.checked_fallback_dtype() == fb
            assert net.compute_dtype == cd                       # (setting the fallback leaves the compute dtype alone)
            assert net.set_fallback_dtype("none").fallback_dtype is None


@pytest.mark.parametrize("cd,fb", REFUSED)
def test_refused_pairs_list_the_choices(cd, fb):
    for make in (lambda: UtNet(funit=16, compute_dtype=cd, fallback_dtype=fb),
                 lambda: UtNet(funit=16, compute_dtype=cd).set_fallback_dtype(fb)):
        with pytest.raises(ValueError) as e:
            make()
        msg = str(e.value)
        assert "f16 -> bf16 | f32" in msg and "bf16 -> f32" in msg and repr(fb) in msg and repr(cd) in msg, msg


def test_unknown_spelling_is_refused():
    with pytest.raises(ValueError, match="unknown compute dtype"):
        UtNet(funit=16, compute_dtype="f16", fallback_dtype="f64")
    with pytest.raises(ValueError, match="unknown compute dtype"):
        UtNet(funit=16, compute_dtype="f16").set_fallback_dtype("half")


def test_pair_is_checked_where_it_is_used():
    """set_compute_dtype can spoil a pair that was fine when it was set: the frame loop asks checked_fallback_dtype."""
    net = UtNet(funit=16, compute_dtype="f16", fallback_dtype="bf16")
    net.set_compute_dtype("bf16")
    with pytest.raises(ValueError, match="bf16 -> f32"):
        net.checked_fallback_dtype()
    net.set_compute_dtype("f32")
    with pytest.raises(ValueError, match="bf16 -> f32"):
        net.checked_fallback_dtype()
    assert net.set_compute_dtype("f16").checked_fallback_dtype() == "bf16"


def test_instantiate_model_takes_the_parameter(tmp_path):
    from nind_denoise_amd.nn_common import Model
    torch.save(synth.make_utnet_state_dict(16, 3), tmp_path / "generator_7.pt")

    def make(params):
        return Model.instantiate_model(model_path=str(tmp_path / "generator_7.pt"), network="UtNet", device="cpu", strparameters=params,
                                       keyword="generator")
    m = make("funit=16,compute_dtype=f16,fallback_dtype=f32")
    assert isinstance(m, UtNet) and (m.compute_dtype, m.fallback_dtype) == ("f16", "f32")
    m = make("funit=16,compute_dtype=bfloat16,fallback_dtype=float32")
    assert (m.compute_dtype, m.fallback_dtype) == ("bf16", "f32")
    assert make("funit=16,compute_dtype=f16,fallback_dtype=none").fallback_dtype is None
    assert make("funit=16,compute_dtype=f16").fallback_dtype is None
    for params in ("funit=16,fallback_dtype=f32", "funit=16,compute_dtype=bf16,fallback_dtype=f16",
                   "funit=16,compute_dtype=f16,fallback_dtype=f16"):
        with pytest.raises(ValueError, match="f16 -> bf16"):
            make(params)


def test_runs_of_bad_tiles():
    runs = pipeline.bad_tile_runs
    assert runs([]) == [] and runs([1, 1, 1, 1]) == []
    assert runs([0]) == [(0, 1)] and runs([0], begin=7) == [(7, 1)]                     # a single tile
    assert runs([1, 1, 0, 1]) == [(2, 1)]
    assert runs([0, 0, 1, 1, 1, 0, 0, 0]) == [(0, 2), (5, 3)]                           # runs at both ends
    assert runs([0, 1, 0, 1, 0, 1]) == [(0, 1), (2, 1), (4, 1)]                         # alternating
    assert runs([1, 0, 1, 0, 1, 0], begin=10) == [(11, 1), (13, 1), (15, 1)]
    assert runs([0, 0, 0, 0]) == [(0, 4)] and runs([0, 0, 0, 0], begin=3) == [(3, 4)]   # every tile
    flags = [1] * 20
    for t in (6, 7, 11, 12):
        flags[t] = 0
    assert runs(flags) == [(6, 2), (11, 2)]
    assert runs(torch.tensor(flags, dtype=torch.uint8)[5:15].tolist(), 5) == [(6, 2), (11, 2)]   # (a tile range's slice)


def test_report_and_printed_line():
    rep = {"stale": 1}
    pipeline._fill_report(rep, 20, [12, 6, 11, 7], "f32")
    assert rep == {"stale": 1, "tiles": 20, "fallback_tiles": [6, 7, 11, 12], "fallback_dtype": "f32"}
    assert pipeline.fallback_line(rep) == "fallback: 4 of 20 tiles recomputed in f32"
    pipeline._fill_report(rep, 12, [0], "bf16")
    assert pipeline.fallback_line(rep) == "fallback: 1 of 12 tiles recomputed in bf16"
    pipeline._fill_report(rep, 20, [], "f32")
    assert rep["fallback_tiles"] == [] and pipeline.fallback_line(rep) is None          # nothing recomputed: nothing printed
    assert pipeline.fallback_line({}) is None and pipeline.fallback_line(None) is None
    pipeline._fill_report(None, 20, [1], "f32")                                         # (no report asked for)


def test_checked_entry_is_declared():
    hdr = open(os.path.join(ROOT, "include", "nind_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"int\s+nd_utnet_denoise_frame_checked\s*\(([^;]*)\)\s*;", code)
    assert m and "unsigned char *tile_ok" in m.group(1)
    plain = re.search(r"int\s+nd_utnet_denoise_frame\s*\(([^;]*)\)\s*;", code)
    squeeze = lambda t: re.sub(r"\s+", " ", t).strip()
    assert squeeze(m.group(1)) == squeeze(plain.group(1)) + ", unsigned char *tile_ok"     # same arguments plus the flags
    assert "nd_utnet_denoise_frame_checked" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "nd_utnet_denoise_frame_checked")
    res, args = _lib._SIGNATURES["nd_utnet_denoise_frame_checked"]
    assert args == _lib._SIGNATURES["nd_utnet_denoise_frame"][1] + [_lib.c_void_p]
    # the argument checks come before any GPU call: a null tile_ok is named
    rc = lib.nd_utnet_denoise_frame_checked(16, 1, 2, 0, None, None, None, 310, 275, 120, 88, 16, 0, 20, 4, None, 0, None, 0, None,
                                            _lib.PROGRESS_FN(), None, None)
    assert rc == -1 and b"tile_ok" in lib.nd_last_error()
