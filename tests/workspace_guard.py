"""Guard bytes and NaN floods for the buffers the library borrows (imported as tests/exact_net.py is; the CPU gate that proves
these helpers can fail is tests/test_workspace_guard_host.py, their GPU use tests/test_workspace_contract.py).

A store past a tensor's end lands in a neighbouring block of torch's caching allocator and nothing faults; a read of memory that
the call never wrote returns what the last call left there.  guarded() / typed() put a buffer between two runs of 0xFF bytes -- NaN
in fp32, bf16 and fp16, -1 in every integer type -- so that a store outside it is seen byte for byte (assert_guards), and a read
outside it, or of a 0xFF-filled interior, poisons the result.  flood_then() runs a call whose data is all NaN through an object
and then demands of the next call the bits a freshly made object gives."""
import torch

GUARD = 65536
ALIGN = 512     # torch's caching allocator hands out 512-byte aligned blocks; the interior keeps that alignment


class Handle:
    """One guarded allocation: .raw = [guard | interior | slack up to a multiple of ALIGN | guard] as uint8, .interior = the view handed
    out.  The slack is guard too: everything outside the interior's nbytes is 0xFF and watched."""

    def __init__(self, raw, guard, nbytes, size):
        self.raw, self.guard, self.nbytes, self.size = raw, guard, nbytes, size
        self.interior = raw[guard:guard + nbytes]

    def refill(self, fill):
        self.interior.fill_(fill)


def guarded(nbytes, device, fill=None, guard=GUARD):
    """(interior, handle): `nbytes` uint8 between two guards of `guard` 0xFF bytes.  The bytes between nbytes and the next multiple
    of ALIGN, which keep the second guard aligned, are 0xFF and watched like it: the first byte after the interior is guard.  fill:
    None leaves the interior as the allocator gave it; 0xFF / 0 sets every byte of it."""
    assert guard % ALIGN == 0 and nbytes >= 0
    size = (nbytes + ALIGN - 1) // ALIGN * ALIGN
    raw = torch.empty(guard + size + guard, dtype=torch.uint8, device=device)
    raw[:guard].fill_(0xFF)
    raw[guard + nbytes:].fill_(0xFF)
    h = Handle(raw, guard, nbytes, size)
    if fill is not None:
        h.refill(fill)
    assert h.interior.data_ptr() % ALIGN == raw.data_ptr() % ALIGN
    return h.interior, h


def typed(shape, dtype, device, fill=None, guard=GUARD):
    """(tensor, handle): a contiguous tensor of `shape` and `dtype` on a guarded interior (inputs, outputs, packed weights)."""
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    n = 1
    for s in shape:
        n *= s
    interior, h = guarded(n * torch.empty((), dtype=dtype).element_size(), device, fill, guard)
    return interior.view(dtype).view(shape), h


def typed_like(t, device=None, guard=GUARD):
    """(copy, handle): the values of `t` on a guarded interior."""
    out, h = typed(t.shape, t.dtype, t.device if device is None else device, None, guard)
    out.copy_(t)
    return out, h


def assert_guards(handle, what):
    """Both guards of `handle` are still all 0xFF, from the first byte after the interior's nbytes on.  The message names how many
    guard bytes changed and the first one: its offset past the interior's end or before the interior's start."""
    g, raw = handle.guard, handle.raw
    after, before = raw[g + handle.nbytes:] != 0xFF, raw[:g] != 0xFF
    na, nb = int(after.sum()), int(before.sum())
    if na:
        first = int(after.nonzero()[0])
        raise AssertionError(f"{what}: {na} guard bytes written past the end, the first at end + {first} "
                             f"(interior of {handle.nbytes} B)")
    if nb:
        last = int(before.nonzero()[-1])
        raise AssertionError(f"{what}: {nb} guard bytes written before the start, the nearest at start - {g - last}")


def assert_all_guards(handles, what):
    """handles: {name: Handle}."""
    for name, h in handles.items():
        assert_guards(h, f"{what}: {name}")


def mismatch(got, want):
    """tests/test_half_exact.py::_mismatch, with the first differing flat index."""
    ne = got != want
    n = int(ne.sum())
    first = f", the first at flat index {int(ne.reshape(-1).nonzero()[0])}" if n else ""
    nan = f"NaN: {int(torch.isnan(got).sum())}" + (f", in the expected values: {int(torch.isnan(want).sum())}" if torch.isnan(want).any() else "")
    return f"{n} of {want.numel()} values differ{first} ({nan})"


def assert_same(got, want, what):
    """got is finite and bit for bit `want` (tensors, or tuples / lists / dicts of them)."""
    if isinstance(want, dict):
        assert set(got) == set(want), what
        for k in want:
            assert_same(got[k], want[k], f"{what}[{k}]")
        return
    if isinstance(want, (tuple, list)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, f"{what}[{i}]")
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if got.is_floating_point():
        bad = int((~torch.isfinite(got)).sum())
        assert bad == 0, f"{what}: {bad} of {got.numel()} values are not finite (NaN: {int(torch.isnan(got).sum())})"
    assert torch.equal(got, want), f"{what}: {mismatch(got, want)}"


def flood_then(call_flood, call_real, call_fresh, what="result"):
    """call_flood(): the NaN call on the used object; call_real(): the real call on the same object; call_fresh(): the real call on
    a freshly made object.  The two real results must be finite and bit-identical.  Returns the used object's result."""
    call_flood()
    used = call_real()
    fresh = call_fresh()
    assert_same(used, fresh, f"{what} after a NaN call vs a fresh object")
    return used
