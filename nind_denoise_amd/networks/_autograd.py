"""What UtNet and UNet share under torch.autograd: the flat state of one module on one device and the Function that drives the two
halves of include/nind_hip.h (nd_utnet_train_forward_hw / _backward_hw, nd_unet_grad_forward / _backward).

A network supplies `_autograd_state(device)` (its FlatState, cached on the module), two small methods that make its ABI calls,
  `_abi_forward(st, x, y, geom, ws)`              -> the flags the backward must repeat, or None if it reads them from the module
  `_abi_backward(st, flags, grads, gy, dx, geom)`    (grads, dx: data pointers or None; geom = (batch, h, w))
and two attributes: `_autograd_buffers` (its buffers live in the flat layout too and are loaded with the parameters) and
`_autograd_stale` (the RuntimeError text of a backward whose forward is no longer the module's last)."""
import torch

from .. import _lib


class FlatState:
    """Flat parameter / gradient buffers (`ranges`: {tensor name: (offset, count)}), the packed-weight blobs and the workspace of one
    module on one device.  workspace: (size function, init function, leading arguments, name in the error) for _lib.make_workspace;
    one workspace at a time, another shape replaces it."""

    def __init__(self, device, ranges, count, blob_bytes, workspace):
        self.device = device
        self.flat = torch.zeros(count, dtype=torch.float32, device=device)
        self.grads = torch.zeros(count, dtype=torch.float32, device=device)
        self.blobs = torch.empty(blob_bytes, dtype=torch.uint8, device=device)
        self.ranges = ranges
        self._workspace = workspace
        self.ws, self.ws_key = None, None
        self.generation = 0          # bumped by every forward: a backward must follow ITS forward

    def load(self, tensors):
        """Copy {name: tensor} (parameters and buffers) into the flat buffer; num_batches_tracked has no slot."""
        with torch.no_grad():
            for n, t in tensors.items():
                if n.endswith("num_batches_tracked"):
                    continue
                off, cnt = self.ranges[n]
                self.flat[off:off + cnt].copy_(t.detach().reshape(-1))

    def workspace(self, h, w, batch):
        if self.ws_key != (h, w, batch):
            size_fn, init_fn, head, what = self._workspace
            self.ws = _lib.make_workspace(size_fn, init_fn, head + (h, w, batch), self.device, what, drop=lambda: setattr(self, "ws", None))
            self.ws_key = (h, w, batch)
        return self.ws


class NetFunction(torch.autograd.Function):
    """A network's forward under autograd: forward = device-side weight packing + the conv stack with what the backward needs kept,
    backward = the gradients of every layer.  The backward computes only what autograd asks for: the parameter gradients (no
    weight-gradient launch at all when no parameter requires one) and the input's gradient."""

    @staticmethod
    def forward(ctx, model, names, x, *params):
        st = model._autograd_state(x.device)
        st.load(dict(zip(names, params)))
        if model._autograd_buffers:
            st.load(dict(model.named_buffers()))
        geom = (x.size(0), x.size(2), x.size(3))
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            ctx.flags = model._abi_forward(st, x, y, geom, st.workspace(geom[1], geom[2], geom[0]))
        st.generation += 1
        ctx.model, ctx.names, ctx.geom, ctx.generation = model, names, geom, st.generation
        ctx.shapes = [p.shape for p in params]
        return y

    @staticmethod
    def backward(ctx, gy):
        model = ctx.model
        st = model._autograd_state(gy.device)
        if st.generation != ctx.generation:
            raise RuntimeError(model._autograd_stale)
        batch, h, w = ctx.geom
        want_dx, want_p = ctx.needs_input_grad[2], ctx.needs_input_grad[3:]
        gy = gy.to(torch.float32).contiguous()
        dx = torch.empty(batch, 3, h, w, dtype=torch.float32, device=gy.device) if want_dx else None
        if want_dx or any(want_p):
            with torch.cuda.device(gy.device):
                model._abi_backward(st, ctx.flags, st.grads.data_ptr() if any(want_p) else None, gy, dx.data_ptr() if want_dx else None,
                                    ctx.geom)
        grads = []
        for n, shape, want in zip(ctx.names, ctx.shapes, want_p):
            off, cnt = st.ranges[n]
            grads.append(st.grads[off:off + cnt].view(shape).clone() if want else None)
        return (None, None, dx) + tuple(grads)
