"""UNet on MI355X: constructor, parameter/buffer names and call contract of the reference module
(/root/reference/src/nind_denoise/networks/ThirdPartyNets.py:62-169), forward executed by libnind_hip.so
(eval mode: BatchNorm2d running statistics are folded into the convolutions when the weights are packed).

The torch layers below are parameter containers only; ``forward`` never calls them.  No CPU path.

Eval mode is differentiable: an input that requires a gradient gets one, and so do the parameters that require one (fine-tuning
with frozen BatchNorm statistics) -- ``nd_unet_grad_forward`` / ``nd_unet_grad_backward``.  Train mode (batch statistics) raises
here; the training step on batch statistics is ``nind_denoise_amd.train.UNetTrainer``, which drives this module's tensors.
"""
import ctypes

import torch
from torch import nn

from .. import _lib
from .UtNet import canonical_compute_dtype


class _Box(nn.Module):
    """Named container: gives the state-dict the reference's nesting (inc.conv.conv.0.weight, ...)."""

    def __init__(self, **children):
        super().__init__()
        for k, v in children.items():
            self.add_module(k, v)


def _double_conv(in_ch, out_ch):
    return _Box(conv=nn.Sequential(nn.Conv2d(in_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True),
                                   nn.Conv2d(out_ch, out_ch, 3, padding=1), nn.BatchNorm2d(out_ch), nn.ReLU(inplace=True)))


class _GradState:
    """Flat parameter / gradient buffers (parameters AND BatchNorm buffers, nd_unet_tensor_name order), the packed-weight blobs and the
    gradient workspace of one module on one device (nd_unet_grad_forward / nd_unet_grad_backward of include/nind_hip.h)."""

    def __init__(self, device):
        lib = _lib.load()
        self.device = device
        n = lib.nd_unet_param_count()
        self.flat = torch.zeros(n, dtype=torch.float32, device=device)
        self.grads = torch.zeros(n, dtype=torch.float32, device=device)
        self.blobs = torch.empty(lib.nd_unet_grad_blob_bytes(), dtype=torch.uint8, device=device)
        self.ranges = {}
        for i in range(lib.nd_unet_num_tensors()):
            off, cnt = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(lib.nd_unet_param_range(i, off, cnt))
            self.ranges[lib.nd_unet_tensor_name(i).decode()] = (off.value, cnt.value)
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
            lib = _lib.load()
            nbytes = lib.nd_unet_grad_workspace_bytes(h, w, batch)
            if nbytes == 0:
                _lib.check(lib.nd_unet_grad_workspace_init(None, 0, h, w, batch, None), "UNet under autograd")
            self.ws = None
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            _lib.check(lib.nd_unet_grad_workspace_init(self.ws.data_ptr(), nbytes, h, w, batch, _lib.stream_ptr(self.device)),
                       "nd_unet_grad_workspace_init")
            self.ws_key = (h, w, batch)
        return self.ws


class _UNetFunction(torch.autograd.Function):
    """UNet.forward under autograd (eval mode): forward = BatchNorm fold + device-side packing in both roles + the conv stack with every
    activation kept (nd_unet_grad_forward), backward = nd_unet_grad_backward.  The backward computes only what autograd asks for:
    the parameter gradients (no weight-gradient launch at all when no parameter requires one) and the input's gradient."""

    @staticmethod
    def forward(ctx, model, names, x, *params):
        st = model._grad_state(x.device)
        st.load(dict(zip(names, params)))
        st.load(dict(model.named_buffers()))
        batch, h, w = x.size(0), x.size(2), x.size(3)
        y = torch.empty_like(x)
        with torch.cuda.device(x.device):
            ws = st.workspace(h, w, batch)
            _lib.check(_lib.load().nd_unet_grad_forward(model.grad_flags, st.flat.data_ptr(), st.blobs.data_ptr(), x.data_ptr(),
                                                        y.data_ptr(), batch, h, w, ws.data_ptr(), ws.numel(),
                                                        _lib.stream_ptr(x.device)), "nd_unet_grad_forward")
        st.generation += 1
        ctx.model, ctx.names, ctx.geom, ctx.generation, ctx.flags = model, names, (batch, h, w), st.generation, model.grad_flags
        ctx.shapes = [p.shape for p in params]
        return y

    @staticmethod
    def backward(ctx, gy):
        model = ctx.model
        st = model._grad_state(gy.device)
        if st.generation != ctx.generation:
            raise RuntimeError("UNet backward: another forward of this module ran under autograd since this graph was built; its "
                               "activations are gone (one forward/backward in flight per module)")
        batch, h, w = ctx.geom
        want_dx, want_p = ctx.needs_input_grad[2], ctx.needs_input_grad[3:]
        gy = gy.to(torch.float32).contiguous()
        dx = torch.empty(batch, 3, h, w, dtype=torch.float32, device=gy.device) if want_dx else None
        if want_dx or any(want_p):
            with torch.cuda.device(gy.device):
                _lib.check(_lib.load().nd_unet_grad_backward(ctx.flags, st.flat.data_ptr(), st.grads.data_ptr() if any(want_p) else None,
                                                             st.blobs.data_ptr(), gy.data_ptr(), dx.data_ptr() if want_dx else None,
                                                             batch, h, w, st.ws.data_ptr(), st.ws.numel(), _lib.stream_ptr(gy.device)),
                           "nd_unet_grad_backward")
        grads = []
        for n, shape, want in zip(ctx.names, ctx.shapes, want_p):
            off, cnt = st.ranges[n]
            grads.append(st.grads[off:off + cnt].view(shape).clone() if want else None)
        return (None, None, dx) + tuple(grads)


class UNet(nn.Module):
    # arithmetic switches of the frame loop (nd_unet_denoise_frame); class attributes so that a test or a benchmark can flip them
    split_k = True          # False: ND_FLAG_NO_SPLITK (a tile's bits do not depend on the launch it shares)
    useful_only = True      # False: ND_FLAG_FULL_TILES (every decoder layer on the whole tile)
    pack_on_device = True   # False: fold BatchNorm and pack on the host (nd_unet_pack_weights), then upload

    def __init__(self, n_channels=3, n_classes=3, funit=64, find_noise=False, compute_dtype='f32'):
        super().__init__()
        if canonical_compute_dtype(compute_dtype) != 'f32':
            raise NotImplementedError(f"UNet: compute_dtype={compute_dtype!r}: 16-bit storage exists for UtNet only "
                                      "(the UNet executor is fp32)")
        if int(n_channels) != 3 or int(n_classes) != 3:
            raise NotImplementedError("the HIP UNet path is built for RGB in / RGB out (the reference's defaults)")
        self.inc = _Box(conv=_double_conv(3, 64))
        for n, (ci, co) in enumerate([(64, 128), (128, 256), (256, 512), (512, 512)], start=1):
            self.add_module(f"down{n}", _Box(mpconv=nn.Sequential(nn.MaxPool2d(2), _double_conv(ci, co))))
        for n, (ci, co) in enumerate([(1024, 256), (512, 128), (256, 64), (128, 64)], start=1):
            self.add_module(f"up{n}", _Box(up=nn.ConvTranspose2d(ci // 2, ci // 2, 2, stride=2), conv=_double_conv(ci, co)))
        self.outc = _Box(conv=nn.Conv2d(64, 3, 1))
        self.find_noise = find_noise in (True, "True", "true", "1")
        self._packed = None
        self._workspaces = {}

    def _weights_key(self, device):
        return (str(device),) + tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def packed_weights(self, device):
        key = self._weights_key(device)
        if self._packed is not None and self._packed[0] == key:
            return self._packed[1]
        lib = _lib.load()
        sd = self.state_dict()
        n = lib.nd_unet_num_tensors()
        where = device if self.pack_on_device else "cpu"
        keep, ptrs = [], (ctypes.c_void_p * n)()
        for i in range(n):
            t = sd[lib.nd_unet_tensor_name(i).decode()].detach().to(device=where, dtype=torch.float32).contiguous()
            keep.append(t)
            ptrs[i] = t.data_ptr()
        nbytes = lib.nd_unet_packed_bytes(_lib.ND_F32)
        if self.pack_on_device:
            dev_blob = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            with torch.cuda.device(device):
                _lib.check(lib.nd_unet_pack_weights_device(_lib.ND_F32, ptrs, n, dev_blob.data_ptr(), nbytes, _lib.stream_ptr(device)),
                           "nd_unet_pack_weights_device")
                torch.cuda.current_stream(device).synchronize()     # `keep` may be freed after this
        else:
            blob = torch.empty(nbytes // 4, dtype=torch.float32)
            _lib.check(lib.nd_unet_pack_weights(_lib.ND_F32, ptrs, n, blob.data_ptr(), nbytes), "nd_unet_pack_weights")
            dev_blob = blob.to(device)
        self._packed = (key, dev_blob)
        return dev_blob

    @property
    def flags(self):
        return (0 if self.split_k else _lib.FLAG_NO_SPLITK) | (0 if self.useful_only else _lib.FLAG_FULL_TILES)

    @property
    def grad_flags(self):
        """flags of nd_unet_grad_forward / nd_unet_grad_backward"""
        return (0 if self.split_k else _lib.FLAG_NO_SPLITK) | (_lib.FLAG_FIND_NOISE if self.find_noise else 0)

    def _grad_state(self, device):
        st = getattr(self, "_gstate", None)
        if st is None or st.device != device:
            st = self._gstate = _GradState(device)
        return st

    def workspace(self, h, w, batch, device):
        key = (str(device), h, w, batch)
        ws = self._workspaces.get(key)
        if ws is None:
            lib = _lib.load()
            nbytes = lib.nd_unet_workspace_bytes(h, w, batch, _lib.ND_F32)
            if nbytes == 0:
                _lib.check(lib.nd_unet_workspace_init(None, 0, h, w, batch, _lib.ND_F32, None), "UNet")
            self._workspaces.clear()
            ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
            _lib.check(lib.nd_unet_workspace_init(ws.data_ptr(), nbytes, h, w, batch, _lib.ND_F32, _lib.stream_ptr(device)),
                       "nd_unet_workspace_init")
            self._workspaces[key] = ws
        return ws

    def forward(self, x):
        if x.device.type != "cuda":
            raise RuntimeError("nind_denoise_amd.UNet runs on the MI355X HIP path only (no CPU fallback)")
        if self.training:
            raise RuntimeError("nind_denoise_amd.UNet implements eval mode (BatchNorm running statistics) only; call .eval()")
        if x.dim() != 4 or x.size(1) != 3:
            raise ValueError(f"UNet expects [B,3,H,W], got {tuple(x.shape)}")
        if torch.is_grad_enabled() and x.requires_grad:
            # the differentiable path (eval mode: BatchNorm stays on its running statistics).  Parameters that require a gradient
            # get one -- fine-tuning with frozen statistics; an input that needs no gradient takes the inference path below,
            # whose output carries no graph
            named = list(self.named_parameters())
            return _UNetFunction.apply(self, tuple(n for n, _ in named), x.to(torch.float32).contiguous(), *[p for _, p in named])
        x = x.detach().to(torch.float32).contiguous()
        b, _, h, w = x.shape
        lib = _lib.load()
        with torch.cuda.device(x.device):
            blob = self.packed_weights(x.device)
            ws = self.workspace(h, w, b, x.device)
            y = torch.empty_like(x)
            _lib.check(lib.nd_unet_forward(_lib.ND_F32, blob.data_ptr(), x.data_ptr(), y.data_ptr(), b, h, w, ws.data_ptr(),
                                           ws.numel(), _lib.stream_ptr(x.device)), "nd_unet_forward")
        return x - y if self.find_noise else y
