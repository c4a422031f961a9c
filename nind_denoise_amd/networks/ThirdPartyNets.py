"""UNet on MI355X: constructor, parameter/buffer names and call contract of the reference module
(/root/reference/src/nind_denoise/networks/ThirdPartyNets.py:62-169), forward executed by libnind_hip.so
(eval mode: BatchNorm2d running statistics are folded into the convolutions when the weights are packed).

The torch layers below are parameter containers only; ``forward`` never calls them.  No CPU path.

Eval mode is differentiable: an input that requires a gradient gets one, and so do the parameters that require one (fine-tuning
with frozen BatchNorm statistics) -- ``nd_unet_grad_forward`` / ``nd_unet_grad_backward``.  Train mode (batch statistics) raises
here; the training step on batch statistics is ``nind_denoise_amd.train.UNetTrainer``, which drives this module's tensors.

``UNet(winograd=True)`` (``--model_parameters winograd=1``) runs the 3x3 layers of the inference paths -- ``forward`` without a
gradient and the frame loop -- in Winograd forms (ND_FLAG_UNET_WINOGRAD: three-pass F(6x6,3x3) on the wide layers, fused F(4,3) on
the narrow ones).  It is inference only: the autograd halves (``forward`` on an input that requires a gradient, ``frame_grad``) and
``UNetTrainer`` ignore it and run the direct kernels, so their bits do not depend on it.
"""
import ctypes

import torch
from torch import nn

from .. import _lib
from ._autograd import FlatState, NetFunction
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


class UNet(nn.Module):
    # arithmetic switches of the frame loop (nd_unet_denoise_frame); class attributes so that a test or a benchmark can flip them
    split_k = True          # False: ND_FLAG_NO_SPLITK (a tile's bits do not depend on the launch it shares)
    useful_only = True      # False: ND_FLAG_FULL_TILES (every decoder layer on the whole tile)
    pack_on_device = True   # False: fold BatchNorm and pack on the host (nd_unet_pack_weights), then upload

    def __init__(self, n_channels=3, n_classes=3, funit=64, find_noise=False, compute_dtype='f32', winograd=False):
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
        if winograd in (True, "True", "true", "1"):
            self.winograd = True
        elif winograd in (False, "False", "false", "0", None, ""):
            self.winograd = False
        else:
            raise ValueError(f"UNet: winograd={winograd!r}: expected True / 'True' / 'true' / '1' or a false spelling")
        self._packed = None
        self._workspaces = {}

    @property
    def _wino_flag(self):
        return _lib.FLAG_UNET_WINOGRAD if self.winograd else 0

    def _weights_key(self, device):
        return (str(device), self.winograd, self.pack_on_device) + tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

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
        nbytes = lib.nd_unet_packed_bytes_flags(_lib.ND_F32, self._wino_flag)
        if self.pack_on_device:
            dev_blob = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            with torch.cuda.device(device):
                _lib.check(lib.nd_unet_pack_weights_device_flags(_lib.ND_F32, self._wino_flag, ptrs, n, dev_blob.data_ptr(), nbytes,
                                                                 _lib.stream_ptr(device)), "nd_unet_pack_weights_device_flags")
                torch.cuda.current_stream(device).synchronize()     # `keep` may be freed after this
        else:
            blob = torch.empty(nbytes // 4, dtype=torch.float32)
            _lib.check(lib.nd_unet_pack_weights_flags(_lib.ND_F32, self._wino_flag, ptrs, n, blob.data_ptr(), nbytes),
                       "nd_unet_pack_weights_flags")
            dev_blob = blob.to(device)
        self._packed = (key, dev_blob)
        return dev_blob

    @property
    def flags(self):
        return (0 if self.split_k else _lib.FLAG_NO_SPLITK) | (0 if self.useful_only else _lib.FLAG_FULL_TILES) | self._wino_flag

    @property
    def grad_flags(self):
        """flags of nd_unet_grad_forward / nd_unet_grad_backward (``winograd`` is inference only: not among them)"""
        return (0 if self.split_k else _lib.FLAG_NO_SPLITK) | (_lib.FLAG_FIND_NOISE if self.find_noise else 0)

    # ------------------------------------------------------------------ under autograd in eval mode (NetFunction): BatchNorm fold +
    # device-side packing in both roles + the conv stack with every activation kept, then nd_unet_grad_backward
    _autograd_buffers = True       # the running statistics have slots in the flat layout: the fold reads one array
    _autograd_stale = ("UNet backward: another forward of this module ran under autograd since this graph was built; its "
                       "activations are gone (one forward/backward in flight per module)")

    def _grad_state(self, device):
        st = getattr(self, "_gstate", None)
        if st is None or st.device != device:
            lib = _lib.load()
            st = self._gstate = FlatState(device, _lib.unet_ranges(), lib.nd_unet_param_count(), lib.nd_unet_grad_blob_bytes(),
                                          (lib.nd_unet_grad_workspace_bytes, lib.nd_unet_grad_workspace_init, (), "UNet under autograd"))
        return st

    _autograd_state = _grad_state

    def _abi_forward(self, st, x, y, geom, ws):
        flags = self.grad_flags         # recorded: the backward repeats them whatever the module's switches say by then
        _lib.check(_lib.load().nd_unet_grad_forward(flags, st.flat.data_ptr(), st.blobs.data_ptr(), x.data_ptr(), y.data_ptr(), *geom,
                                                    ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device)), "nd_unet_grad_forward")
        return flags

    def _abi_backward(self, st, flags, grads, gy, dx, geom):
        _lib.check(_lib.load().nd_unet_grad_backward(flags, st.flat.data_ptr(), grads, st.blobs.data_ptr(), gy.data_ptr(), dx, *geom,
                                                     st.ws.data_ptr(), st.ws.numel(), _lib.stream_ptr(gy.device)),
                   "nd_unet_grad_backward")

    def workspace(self, h, w, batch, device):
        key = (str(device), h, w, batch, self.winograd)
        ws = self._workspaces.get(key)
        if ws is None:
            lib = _lib.load()
            ws = _lib.make_workspace(lib.nd_unet_workspace_bytes_flags, lib.nd_unet_workspace_init_flags,
                                     (h, w, batch, _lib.ND_F32, self._wino_flag), device, "UNet", drop=self._workspaces.clear)
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
            return NetFunction.apply(self, tuple(n for n, _ in named), x.to(torch.float32).contiguous(), *[p for _, p in named])
        x = x.detach().to(torch.float32).contiguous()
        b, _, h, w = x.shape
        lib = _lib.load()
        with torch.cuda.device(x.device):
            blob = self.packed_weights(x.device)
            ws = self.workspace(h, w, b, x.device)
            y = torch.empty_like(x)
            _lib.check(lib.nd_unet_forward_flags(_lib.ND_F32, self._wino_flag, blob.data_ptr(), x.data_ptr(), y.data_ptr(), b, h, w,
                                                 ws.data_ptr(), ws.numel(), _lib.stream_ptr(x.device)), "nd_unet_forward_flags")
        return x - y if self.find_noise else y
