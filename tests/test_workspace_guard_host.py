"""CPU gate of tests/workspace_guard.py: what shows that tests/test_workspace_contract.py can fail.  Three fake entry points written
in torch on CPU tensors -- one correct, one that writes one element past its output, one that adds 0 * scratch[0] to its result --
go through the very helpers the GPU file uses.  The harness must pass the first and report the other two, with the offset of the
stray store and the count of the poisoned values."""
import re

import pytest
import torch

import workspace_guard as G

CPU = torch.device("cpu")
N = 37          # 148 B of float32: no multiple of 512, so the element right after the output lies in the rounding slack


def _at(t, index):
    """A one-element view of t's storage at flat element `index` of t, inside t or not."""
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset() + index, (1,))


def fake_ok(x, y, scratch):
    scratch[:x.numel()] = x * 2          # written before it is read
    y.copy_(scratch[:x.numel()] + 1)


def fake_overrun(x, y, scratch):
    fake_ok(x, y, scratch)
    _at(y, y.numel())[0] = 1.0           # y[N]: the element right after the output


def fake_underrun(x, y, scratch):
    fake_ok(x, y, scratch)
    _at(y, -1)[0] = 1.0


def fake_reads_scratch(x, y, scratch):
    fake_ok(x, y, scratch)
    y.add_(0 * scratch[x.numel()])       # "times zero": harmless on zeroed scratch, NaN on what a caller really passes


def _run(fn, fill=0xFF):
    x = torch.arange(N, dtype=torch.float32) / 8
    gx, hx = G.typed_like(x)
    y, hy = G.typed((N,), torch.float32, CPU, fill=0xFF)
    ws, hw = G.guarded(4 * (N + 3), CPU, fill=fill)
    fn(gx, y, ws.view(torch.float32))
    G.assert_all_guards({"x": hx, "y": hy, "scratch": hw}, fn.__name__)
    want = torch.empty(N)
    fake_ok(x, want, torch.zeros(N + 3))          # the existing way: plain tensors, zeroed scratch
    G.assert_same(y, want, fn.__name__)
    return y


def test_layout_and_fill():
    t, h = G.guarded(1000, CPU, fill=0)
    assert t.numel() == 1000 and h.size == 1024 and h.raw.numel() == 2 * G.GUARD + 1024
    assert t.data_ptr() % G.ALIGN == h.raw.data_ptr() % G.ALIGN and int(t.sum()) == 0
    assert bool((h.raw[:G.GUARD] == 0xFF).all()) and bool((h.raw[G.GUARD + 1000:] == 0xFF).all())      # the 24 B of slack too
    h.raw[G.GUARD + 1000] = 0                                             # the very first byte after the interior is watched
    with pytest.raises(AssertionError, match=r"1 guard bytes written past the end, the first at end \+ 0 "):
        G.assert_guards(h, "slack")
    c, hc = G.typed_like(torch.arange(5, dtype=torch.float32))            # an input's slack is guard as well
    assert bool((hc.raw[G.GUARD + 20:] == 0xFF).all()) and c.tolist() == [0, 1, 2, 3, 4]
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        v, _ = G.typed((3, 5), dtype, CPU, fill=0xFF)
        assert v.shape == (3, 5) and bool(torch.isnan(v).all())          # 0xFF bytes read as NaN in all three
    i, hi = G.typed((7,), torch.int32, CPU, fill=0xFF)
    assert bool((i == -1).all())
    G.assert_guards(hi, "untouched")


def test_correct_entry_point_passes():
    y = _run(fake_ok)
    assert bool(torch.isfinite(y).all())


def test_store_past_the_output_is_reported_with_offset_and_count():
    with pytest.raises(AssertionError) as e:
        _run(fake_overrun)
    msg = str(e.value)
    # y[N] = 1.0 = bytes 00 00 80 3f: four guard bytes change, the first of them is the first byte after the interior's 148 B
    assert re.search(r"fake_overrun: y: 4 guard bytes written past the end, the first at end \+ 0 ", msg), msg
    with pytest.raises(AssertionError) as e:
        _run(fake_underrun)
    assert re.search(r"fake_underrun: y: 4 guard bytes written before the start, the nearest at start - 1$", str(e.value)), str(e.value)


def test_read_of_unwritten_scratch_is_reported_with_count():
    with pytest.raises(AssertionError) as e:
        _run(fake_reads_scratch)
    assert re.search(rf"fake_reads_scratch: {N} of {N} values are not finite \(NaN: {N}\)", str(e.value)), str(e.value)
    _run(fake_reads_scratch, fill=0)     # the existing way -- zeroed scratch -- does not see it: that is the gap


def test_flood_then_reports_carried_state():
    class Obj:
        def __init__(self):
            self.state = torch.zeros(N)

        def ok(self, x):
            self.state.copy_(x)
            return self.state * 2

        def carries(self, x):
            y = x * 2 + 0 * self.state       # reads last call's data before writing this call's
            self.state.copy_(x)
            return y

        def carries_one(self, x):
            y = x * 2
            y[5] += self.state[5] * 0
            self.state.copy_(x)
            return y

    x, nan = torch.arange(N, dtype=torch.float32), torch.full((N,), float("nan"))
    used = Obj()
    G.flood_then(lambda: used.ok(nan), lambda: used.ok(x), lambda: Obj().ok(x))
    for name, count in (("carries", N), ("carries_one", 1)):
        used = Obj()
        with pytest.raises(AssertionError) as e:
            G.flood_then(lambda: getattr(used, name)(nan), lambda: getattr(used, name)(x), lambda: getattr(Obj(), name)(x), name)
        assert re.search(rf"{name} after a NaN call vs a fresh object: {count} of {N} values are not finite \(NaN: {count}\)",
                         str(e.value)), str(e.value)
    # a finite difference is counted too, with its place
    with pytest.raises(AssertionError) as e:
        G.assert_same(torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1.0, 2.5, 3.0]), "t")
    assert "t: 1 of 3 values differ, the first at flat index 1 (NaN: 0)" in str(e.value)
