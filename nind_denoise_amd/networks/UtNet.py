"""UtNet on MI355X: same constructor, parameter names and call contract as the reference module
(/root/reference/src/nind_denoise/networks/UtNet.py:13-109), forward executed by libnind_hip.so.

The torch layers created here are parameter CONTAINERS only (they give the module the reference's
state-dict layout, initialisation and ``load_state_dict`` behaviour); ``forward`` never calls them.
It repacks the weights once into MFMA fragment order, keeps the packed blob and a per-(h, w, batch)
activation workspace resident in HBM, and enqueues the whole conv stack on the current stream
through ``nd_utnet_forward_hw``.  There is no CPU path: a CPU tensor raises.
"""
import ctypes

import torch
from torch import nn

from .. import _lib
from ._autograd import FlatState, NetFunction
from ..synth import utnet_layer_table, utnet_prelu_keys

_ACTIVATIONS = {"PReLU": nn.PReLU, "ELU": nn.ELU, "Hardswish": nn.Hardswish}
_SHORT_DTYPE = {_lib.ND_F32: "f32", _lib.ND_BF16: "bf16", _lib.ND_F16: "f16"}


def canonical_compute_dtype(name):
    """Short form ("f32" | "bf16" | "f16") of any spelling _lib.DTYPE knows; ValueError with the choices otherwise."""
    if name not in _lib.DTYPE:
        raise ValueError(f"unknown compute dtype {name!r}; choose one of {', '.join(_lib.DTYPE)}")
    return _SHORT_DTYPE[_lib.DTYPE[name]]


# compute dtype -> the dtypes with more range that may redo its overflowing tiles (pipeline.denoise_frame)
FALLBACK_DTYPES = {"f16": ("bf16", "f32"), "bf16": ("f32",)}


def canonical_fallback_dtype(name):
    """None for off (None, '' or 'none'), else the short form of any spelling compute_dtype takes."""
    if name is None or (isinstance(name, str) and name.strip().lower() in ("", "none")):
        return None
    return canonical_compute_dtype(name)


def check_fallback_pair(compute_dtype, fallback_dtype):
    """The fallback of a compute dtype has more range than it: f16 -> bf16 | f32, bf16 -> f32.  Returns fallback_dtype (None: off);
    ValueError with the choices otherwise."""
    if fallback_dtype is None or fallback_dtype in FALLBACK_DTYPES.get(compute_dtype, ()):
        return fallback_dtype
    pairs = ", ".join(f"{c} -> {' | '.join(f)}" for c, f in FALLBACK_DTYPES.items())
    raise ValueError(f"fallback_dtype={fallback_dtype!r} cannot serve compute_dtype={compute_dtype!r}; choose one of: {pairs} "
                     "(or none)")


def valid_cs(cs):
    """The network only accepts cs = 16k + 56 (the reference raises in torch.cat otherwise)."""
    return cs >= 104 and (cs - 56) % 16 == 0


def nearest_valid_cs(cs):
    k = (cs - 56 + 8) // 16          # ties go up: 256 -> 264, 512 -> 520, 128 -> 136
    return max(104, 16 * k + 56)


class UtNet(nn.Module):
    # per-call arithmetic flags (nd_flags of include/nind_hip.h), overridable per instance:
    #   split_k = False  -> every output tile whole: a tile's bits do not depend on the batch grouping
    #   winograd = False -> direct convolution on every 3x3 layer
    #   w1d_regs = True  -> A/B switch: the fused 1-D Winograd layers through conv_w1d (transform in registers) instead of conv_w2d
    #   useful_only = False -> the fused denoise loop computes whole tiles in every layer (as forward() always does) instead of
    #                          only what the useful centre of a tile depends on in the last decoder levels (same canvas)
    #   fused_pool = False -> A/B switch: every MaxPool2d(2) as its own kernel instead of from the producing layer's epilogue (same values)
    #   share_encoder = False -> A/B switch: the fused frame loop runs every tile's whole encoder instead of the first two levels
    #                            once per band of tile rows (fp32 useful-region mode; same canvas up to fp32 re-association)
    #   share_level2 = False -> A/B switch: the shared loop keeps the third encoder level (convs3.x) per tile where it would run it
    #                           once per band too (nd_utnet_frame_levels: 3; same canvas up to fp32 re-association)
    #   fold_skips = False -> A/B switch: the shared loop keeps the skip halves of tconvs4.0 / 3.0 / 2.0 in the per-tile sums where it
    #                         would compute their products once per band (nd_utnet_frame_folds; same canvas up to fp32 re-association)
    #   mosaic_wino = False -> A/B switch: every three-pass Winograd layer tiles each image on its own where it would lay one tile grid
    #                          over a mosaic of the launch's images (bottom.2, tconvs1.0; nd_wino_mosaic; fp32 re-association)
    split_k = True
    mosaic_wino = True
    winograd = True
    w1d_regs = False
    useful_only = True
    fused_pool = True
    share_encoder = True
    share_level2 = True
    fold_skips = True

    def __init__(self, funit=64, activation='PReLU', compute_dtype='f32', fallback_dtype=None):
        super().__init__()
        funit = int(funit)
        compute_dtype = canonical_compute_dtype(compute_dtype)
        fallback_dtype = check_fallback_pair(compute_dtype, canonical_fallback_dtype(fallback_dtype))
        if activation not in _ACTIVATIONS:
            exit(f'UtNet: unknown activation function: {activation}')
        self.funit, self.activation = funit, activation
        groups = {}
        for key, kind, cin, cout, k in utnet_layer_table(funit):
            if kind == "conv":
                layer = nn.Conv2d(cin, cout, k)
            elif kind == "convT":
                layer = nn.ConvTranspose2d(cin, cout, k)
            else:
                layer = nn.ConvTranspose2d(cin, cout, k, stride=2)
            if "." in key:
                seq, idx = key.split(".")
                groups.setdefault(seq, {})[int(idx)] = layer
            else:
                groups[key] = layer
        for key in utnet_prelu_keys():
            seq, idx = key.split(".")
            groups[seq][int(idx)] = _ACTIVATIONS[activation]()
        # registration order = the reference's state-dict order (convs1..4, bottom, up1, tconvs1, up2, ...)
        order = ["convs1", "convs2", "convs3", "convs4", "bottom"]
        for n in range(1, 5):
            order += [f"up{n}", f"tconvs{n}"]
        for name in order:
            g = groups[name]
            self.add_module(name, nn.Sequential(*[g[i] for i in sorted(g)]) if isinstance(g, dict) else g)
        self._packed = {}         # dtype -> (key, device blob)
        self.pack_on_device = True   # build the packed blob in HBM (nd_utnet_pack_weights_device); False: host packer
        self._workspaces = {}     # (device, h, w, batch, dtype) -> uint8 tensor
        self.max_cached_workspaces = 2
        self._fallback_workspaces = {}   # the same for a dtype other than compute_dtype (workspace(dtype=...)): one at a time
        self.compute_dtype = compute_dtype   # storage of activations + weights inside the conv stack: "f32" | "bf16" | "f16"
        # the frame loop redoes the tiles whose 16-bit result is not finite in this dtype (None: off; pipeline.denoise_frame)
        self.fallback_dtype = fallback_dtype
        self.weights_generation = 0   # bumped by whoever rewrites the parameters through raw pointers (train.UtNetTrainer)

    def set_compute_dtype(self, name):
        """"f32": fp32 storage, exact-fp32 MFMA (the reference's arithmetic).  "bf16" / "f16": 16-bit storage of
        activations and weights with fp32 accumulation (BASELINE configs 3 / 4); inputs and outputs stay float32.
        Same spellings as the constructor's compute_dtype (the model parameter `--model_parameters compute_dtype=...` sets)."""
        self.compute_dtype = canonical_compute_dtype(name)
        return self

    def set_fallback_dtype(self, name):
        """The dtype in which pipeline.denoise_frame recomputes the tiles whose result is not finite in compute_dtype: f16 -> bf16 or
        f32, bf16 -> f32; None, '' or 'none': off (a non-finite 16-bit frame is then refused by its callers).  Same spellings as
        compute_dtype (the model parameter `--model_parameters compute_dtype=f16,fallback_dtype=f32` sets both).  set_compute_dtype may
        change the pair afterwards, so the frame loop checks it again (checked_fallback_dtype)."""
        self.fallback_dtype = check_fallback_pair(self.compute_dtype, canonical_fallback_dtype(name))
        return self

    def checked_fallback_dtype(self):
        """fallback_dtype (None: off) after checking it against the compute dtype as it stands now."""
        return check_fallback_pair(self.compute_dtype, self.fallback_dtype)

    @property
    def _dt(self):
        return _lib.DTYPE[self.compute_dtype]

    @property
    def flags(self):
        return ((0 if self.split_k else _lib.FLAG_NO_SPLITK) | (0 if self.winograd else _lib.FLAG_DIRECT_CONV) |
                (_lib.FLAG_W1D_REGS if self.w1d_regs else 0) | (0 if self.useful_only else _lib.FLAG_FULL_TILES) |
                (0 if self.fused_pool else _lib.FLAG_UNFUSED_POOL) | (0 if self.share_encoder else _lib.FLAG_TILE_ENCODER) |
                (0 if self.mosaic_wino else _lib.FLAG_TILE_WINO))

    @property
    def frame_flags(self):
        """flags of the frame-loop entry points (nd_utnet_frame_*, nd_utnet_denoise_frame): they alone take FLAG_TILE_LEVEL2 and FLAG_TILE_SKIPS."""
        return self.flags | (0 if self.share_level2 else _lib.FLAG_TILE_LEVEL2) | (0 if self.fold_skips else _lib.FLAG_TILE_SKIPS)

    # ------------------------------------------------------------------ weights
    def _weights_key(self, device):
        return (str(device), self.weights_generation) + tuple((p.data_ptr(), p._version) for p in self.parameters())

    def packed_weights(self, device, dtype=None):
        """Packed blob in HBM (re-packed when a parameter changed or moved).  dtype: pack for another storage type than
        compute_dtype (the fallback's), which stays as it is."""
        dtype = self.compute_dtype if dtype is None else canonical_compute_dtype(dtype)
        dt = _lib.DTYPE[dtype]
        key = self._weights_key(device)
        hit = self._packed.get(dtype)
        if hit is not None and hit[0] == key:
            return hit[1]
        lib = _lib.load()
        sd = self.state_dict()
        names = _lib.utnet_tensor_names()
        nbytes = lib.nd_utnet_packed_bytes(self.funit, dt)
        if nbytes == 0:
            raise ValueError(f"UtNet: funit={self.funit} is not supported by the HIP path for {dtype} "
                             "(multiple of 8 for f32, of 16 for bf16 / f16)")
        on_device = self.pack_on_device
        where = device if on_device else "cpu"     # pack in HBM (device-side packers), or on the host (the yardstick)
        keep = []
        ptrs = (ctypes.c_void_p * len(names))()
        for i, n in enumerate(names):
            if n in sd:
                t = sd[n].detach().to(device=where, dtype=torch.float32).contiguous()
                keep.append(t)
                ptrs[i] = t.data_ptr()
            else:
                ptrs[i] = None  # activation without parameters (ELU / Hardswish)
        if on_device:
            dev_blob = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
            with torch.cuda.device(device):
                _lib.check(lib.nd_utnet_pack_weights_device(self.funit, dt, ptrs, len(names), dev_blob.data_ptr(), nbytes,
                                                            _lib.stream_ptr(device)), "nd_utnet_pack_weights_device")
                torch.cuda.current_stream(device).synchronize()     # `keep` may be freed after this
        else:
            blob = torch.empty(nbytes // 4, dtype=torch.float32)
            _lib.check(lib.nd_utnet_pack_weights(self.funit, dt, ptrs, len(names), blob.data_ptr(), nbytes),
                       "nd_utnet_pack_weights")
            dev_blob = blob.to(device)
        self._packed[dtype] = (key, dev_blob)
        return dev_blob

    def workspace(self, cs, batch, device, width=None, dtype=None):
        """Activation workspace for [batch,3,cs,width or cs] inputs (zero borders initialised once, then cached).  dtype: size it for
        another storage type than compute_dtype (the fallback's); those are cached apart (one at a time), so that the frame
        loop's own workspace stays where it is while a few tiles are redone."""
        h, w = int(cs), int(cs if width is None else width)
        other = dtype is not None and canonical_compute_dtype(dtype) != self.compute_dtype
        dtype = canonical_compute_dtype(dtype) if other else self.compute_dtype
        cache = self._fallback_workspaces if other else self._workspaces
        key = (str(device), h, w, int(batch), dtype)
        ws = cache.get(key)
        if ws is None:
            lib = _lib.load()

            def drop():
                while len(cache) >= (1 if other else self.max_cached_workspaces):
                    cache.pop(next(iter(cache)))
            ws = _lib.make_workspace(lib.nd_utnet_workspace_bytes_hw, lib.nd_utnet_workspace_init_hw,
                                     (self.funit, h, w, batch, _lib.DTYPE[dtype]), device, "UtNet", drop=drop)
            cache[key] = ws
        return ws

    def frame_workspace(self, width, height, cs, ucs, ol, batch, device):
        """Band and strip buffers of the shared encoder for one frame geometry (nd_utnet_frame_workspace_bytes; zero-filled once,
        then cached with the activation workspaces), or None where the frame loop runs every tile's whole encoder."""
        lib = _lib.load()
        nbytes = lib.nd_utnet_frame_workspace_bytes(self.funit, self._dt, self.frame_flags, width, height, cs, ucs, ol, batch)
        if nbytes == 0:
            return None
        key = (str(device), "frame", nbytes)
        ws = self._workspaces.get(key)
        if ws is None:
            for k in [k for k in self._workspaces if k[1] == "frame"]:   # one frame workspace at a time
                del self._workspaces[k]
            ws = torch.zeros(nbytes, dtype=torch.uint8, device=device)
            self._workspaces[key] = ws
        return ws

    # ------------------------------------------------------------------ forward
    def forward(self, l):
        if l.device.type != "cuda":
            raise RuntimeError("nind_denoise_amd.UtNet runs on the MI355X HIP path only (no CPU fallback); "
                               "move the module and its input to the GPU")
        if l.dim() != 4 or l.size(1) != 3:
            raise ValueError(f"UtNet expects [B,3,H,W], got {tuple(l.shape)}")
        batch, h, w = l.size(0), l.size(2), l.size(3)
        for cs in (h, w):
            if not valid_cs(cs):
                raise ValueError(f"UtNet: tile size {cs} is not of the form 16k+56 (e.g. {nearest_valid_cs(cs)}); "
                                 "the reference network fails on it too")
        trainable = self.training and any(p.requires_grad for p in self.parameters())
        if torch.is_grad_enabled() and (trainable or (l.requires_grad and self.compute_dtype == "f32")):
            # the differentiable path: the reference trains through plain autograd (nn_common.py:146 `self.model.train()`,
            # :198-218 forward / backward).  It also serves an input that needs a gradient -- a frozen or eval() network as one
            # differentiable stage of a larger graph -- and then builds the graph whatever the mode, as torch does.  An eval()
            # module whose input needs no gradient (nn_common.py:142, denoise_image.py:229) takes the inference path below,
            # whose output carries no graph
            if self.compute_dtype != "f32":
                raise NotImplementedError("UtNet under autograd runs in fp32 (the training step's arithmetic)")
            named = [(n, p) for n, p in self.named_parameters()]
            return NetFunction.apply(self, tuple(n for n, _ in named), l.to(torch.float32).contiguous(), *[p for _, p in named])
        x = l.detach().to(torch.float32).contiguous()
        lib = _lib.load()
        with torch.cuda.device(x.device):
            blob = self.packed_weights(x.device)
            ws = self.workspace(h, batch, x.device, width=w)
            y = torch.empty_like(x)
            _lib.check(lib.nd_utnet_forward_hw(self.funit, _lib.ACT[self.activation], self._dt, self.flags, blob.data_ptr(),
                                               x.data_ptr(), y.data_ptr(), batch, h, w, ws.data_ptr(), ws.numel(),
                                               _lib.stream_ptr(x.device)), "nd_utnet_forward_hw")
        return y

    # ------------------------------------------------------------------ under autograd (NetFunction): the kernels of the fused
    # training step (csrc/utnet_train.hip); the input's gradient runs through the input's reflection padding
    _autograd_buffers = False
    _autograd_stale = ("UtNet backward: another forward of this module ran under autograd since this graph was built; its "
                       "activations are gone (one forward/backward in flight per module -- as the reference's training loop runs)")

    def _train_state(self, device):
        st = getattr(self, "_tstate", None)
        if st is None or st.device != device:
            lib = _lib.load()
            n = lib.nd_utnet_param_count(self.funit)
            if n == 0:
                raise ValueError(f"UtNet: funit={self.funit} is not supported by the HIP training path (multiple of 8)")
            st = self._tstate = FlatState(device, _lib.utnet_ranges(self.funit), n, lib.nd_utnet_train_blob_bytes(self.funit),
                                          (lib.nd_utnet_train_workspace_bytes_hw, lib.nd_utnet_train_workspace_init_hw, (self.funit,),
                                           "UtNet training"))
        return st

    _autograd_state = _train_state

    def _abi_forward(self, st, x, y, geom, ws):
        _lib.check(_lib.load().nd_utnet_train_forward_hw(self.funit, _lib.ACT[self.activation], self.flags, st.flat.data_ptr(),
                                                         st.blobs.data_ptr(), x.data_ptr(), y.data_ptr(), *geom, ws.data_ptr(),
                                                         ws.numel(), _lib.stream_ptr(x.device)), "nd_utnet_train_forward_hw")

    def _abi_backward(self, st, flags, grads, gy, dx, geom):      # flags: None, the module's are read now; no bucket events
        _lib.check(_lib.load().nd_utnet_train_backward_hw(self.funit, _lib.ACT[self.activation], self.flags, st.flat.data_ptr(), grads,
                                                          st.blobs.data_ptr(), gy.data_ptr(), dx, *geom, st.ws.data_ptr(),
                                                          st.ws.numel(), _lib.stream_ptr(gy.device), None, 0),
                   "nd_utnet_train_backward_hw")

    def flops_per_tile(self, cs):
        return _lib.load().nd_utnet_flops(self.funit, cs)
