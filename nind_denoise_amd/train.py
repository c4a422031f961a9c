"""UtNet training step on MI355X (BASELINE config 5): forward + loss + backward in libnind_hip.so, Adam(amsgrad) on flat
buffers, data parallel over RCCL.

Mirrors the reference's generator update for any activation the network takes (/root/reference/src/nind_denoise/nn_common.py:163-218 and the loop body of
nn_train.py:308-380):  generated = model(noisy).clip(0,1);  loss = sum_k weight_k * criterion_k(generated, clean);
loss.backward();  Adam(lr, betas=(beta1, .999), amsgrad=True).step().   Criteria: L1, MSE, SSIM and MSSSIM (the
reference's SSIM / MS-SSIM criteria come from piqa, which is not installed here: csrc/ssim.hip restates its published
algorithm, forward and backward -- see oracle/losses.py).  Every criterion is reduced with a mean over the batch; the
reference builds its criteria with reduction=None and calls .backward() on the per-sample vector, which torch rejects
for batches larger than one (nn_common.py:170-177, 216), so there is no other reading of "the loss" to reproduce.

The module's parameters are views into ONE flat fp32 buffer in state-dict order; gradients come back in a second flat
buffer with the same layout, so the optimizer is one kernel and the data-parallel reduction runs on nine contiguous level
buckets of that buffer, each all-reduced as soon as the backward pass has finished it (dist.BucketedGradientAverager).

UNetTrainer, below, is the same surface for UNet: BatchNorm on the statistics of the batch (csrc/unet_grad.hip in train mode,
csrc/unet_bn.hip), one GPU.  Both stand on _GuardedStep: the optimizer (csrc/optim.hip), its guard and the trainer's state dict.
"""
import torch

from . import _lib
from .dist import BucketedGradientAverager
from .networks.UtNet import UtNet, valid_cs


class _GuardedStep:
    """The base of UtNetTrainer and UNetTrainer: device and loss-weight checks, Adam's buffers and step (plain or guarded), learn,
    the learning rate, grad_of and the trainer's state dict.  A subclass lays out self.flat and supplies forward_backward and
    _weights_written.

    max_grad_norm (None: off): the gradient is clipped to this global L2 norm, torch.nn.utils.clip_grad_norm_'s coefficient.
    skip_nonfinite: a step whose gradient holds a NaN or an infinity is not applied -- parameters, m, v and vmax keep their bits.
    Both off: optimizer_step is one nd_adam_step launch.  Either on: nd_grad_guard + nd_adam_step_guarded on the same stream,
    behind whatever nd_adam_step would wait for (under a process group: the averaged gradient, so every rank decides alike), and
    `guard_state` holds four doubles on the device: sum g^2, the number of non-finite entries, the scale, ok (include/nind_hip.h).
    Nothing is read back: `steps` counts attempts, so a skipped step still advances Adam's bias-correction index (unlike
    torch.cuda.amp.GradScaler, which skips optimizer.step()).  The clipped gradient is never stored: self.grads and grad_of keep
    the unclipped one."""
    kind, data_parallel = None, True

    def _init_base(self, model, device, process_group, weights, lr, betas, eps, amsgrad, loss_cs):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise RuntimeError(f"{self.kind} needs a GPU (no CPU fallback)")
        if process_group is not None and not self.data_parallel:      # (refused, like the weights, before the device is touched)
            raise NotImplementedError(f"{self.kind}: data-parallel UNet training is not available (the bucketed gradient averager "
                                      "is laid out for UtNet)")
        self.group = process_group
        self.weights = {"L1": 0.0, "MSE": 1.0} if weights is None else dict(weights)
        unknown = set(k for k, v in self.weights.items() if v) - {"L1", "MSE", "SSIM", "MSSSIM"}
        if unknown:   # D1 / D2: the discriminator terms of the reference's GAN mode (nn_common.py:178-182)
            raise NotImplementedError(f"loss terms {sorted(unknown)} are not available (generator losses: L1, MSE, SSIM, MSSSIM)")
        self.model = model.to(self.device)
        self.lib = _lib.load()
        self.lr, self.betas, self.eps, self.amsgrad = lr, betas, eps, amsgrad
        self.loss_cs = loss_cs        # centre crop the criteria see (nn_train.py:319-323 --loss_cs); None: the whole crop

    def _init_optimizer(self, max_grad_norm, skip_nonfinite):
        """Everything sized by self.flat: the gradient buffer (slots nothing writes stay 0), Adam's moments, the guard."""
        self.grads = torch.zeros_like(self.flat)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.vmax = torch.zeros_like(self.flat)
        self.steps = 0
        self._ws = {}
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._init_guard(max_grad_norm, skip_nonfinite)

    def _workspace(self, key, size_fn, init_fn, args, what):
        """The training workspace for `key` (initialised once, then cached; another key replaces it)."""
        ws = self._ws.get(key)
        if ws is None:
            ws = self._ws[key] = _lib.make_workspace(size_fn, init_fn, args, self.device, what, drop=self._ws.clear)
        return ws

    def _init_guard(self, max_grad_norm, skip_nonfinite):
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not (0.0 < max_grad_norm < float("inf")):
                raise ValueError(f"max_grad_norm {max_grad_norm}: a positive finite norm, or None")
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self.guard_state = self._guard_ws = None
        if self.guarded:
            self.guard_state = torch.zeros(4, dtype=torch.float64, device=self.device)
            self._guard_ws = torch.empty(self.lib.nd_grad_guard_workspace_bytes(self.flat.numel()), dtype=torch.uint8, device=self.device)

    @property
    def guarded(self):
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _adam(self):
        """the optimizer launch(es) of one step, self.steps already advanced"""
        adam = (self.flat.data_ptr(), self.grads.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.vmax.data_ptr(),
                self.flat.numel(), self.lr, self.betas[0], self.betas[1], self.eps, self.steps, int(self.amsgrad))
        if not self.guarded:
            _lib.check(self.lib.nd_adam_step(*adam, _lib.stream_ptr(self.device)), "nd_adam_step")
            return
        _lib.check(self.lib.nd_grad_guard(self.grads.data_ptr(), self.grads.numel(), float(self.max_grad_norm or 0.0),
                                          int(self.skip_nonfinite), self.guard_state.data_ptr(), self._guard_ws.data_ptr(),
                                          self._guard_ws.numel(), _lib.stream_ptr(self.device)), "nd_grad_guard")
        _lib.check(self.lib.nd_adam_step_guarded(*adam, self.guard_state.data_ptr(), _lib.stream_ptr(self.device)),
                   "nd_adam_step_guarded")

    def optimizer_step(self):
        self.steps += 1
        with torch.cuda.device(self.device):
            self._adam()      # (UNet's running statistics: gradient and moments 0 -> an update of exactly 0, the slots keep their bits)
        self._weights_written()

    def learn(self, noisy, clean):
        """One generator update (Generator.denoise_batch + learn of the reference); returns the loss as a float tensor."""
        _, loss = self.forward_backward(noisy, clean)
        self.optimizer_step()
        return loss

    def grad_of(self, name):
        off, cnt = self.ranges[name]
        return self.grads[off:off + cnt].view_as(self.model.state_dict()[name])

    def update_learning_rate(self, lr_decay):
        self.lr *= lr_decay
        return self.lr

    def state_dict(self):
        """Everything the next step reads, as CPU copies: the flat parameter buffer (UNet: with the running statistics), Adam's
        m, v and vmax, the step count, the rate and Adam's constants, and the guard's two settings."""
        state = {"kind": self.kind, "funit": getattr(self, "funit", None), "param_count": self.flat.numel(),
                 "steps": self.steps, "lr": self.lr, "betas": tuple(self.betas), "eps": self.eps, "amsgrad": bool(self.amsgrad),
                 "max_grad_norm": self.max_grad_norm, "skip_nonfinite": self.skip_nonfinite}
        for key in ("flat", "m", "v", "vmax"):
            state[key] = getattr(self, key).detach().to("cpu", copy=True)
        return state

    def load_state_dict(self, state):
        """Writes `state` (state_dict of a trainer of the same network) into the existing buffers, so the module's views stay
        valid.  ValueError for another network, funit or parameter count.  The state's max_grad_norm and skip_nonfinite REPLACE
        this trainer's own, and guard_state is allocated anew: a reference to the old tensor no longer sees the steps."""
        if state.get("kind") != self.kind or state.get("funit") != getattr(self, "funit", None):
            raise ValueError(f"{self.kind}.load_state_dict: the state is of {state.get('kind')} funit {state.get('funit')}, this "
                             f"trainer is {self.kind} funit {getattr(self, 'funit', None)}")
        for key in ("flat", "m", "v", "vmax"):
            t = state[key]
            if state.get("param_count") != self.flat.numel() or tuple(t.shape) != tuple(self.flat.shape) or t.dtype != torch.float32:
                raise ValueError(f"{self.kind}.load_state_dict: {key} holds {tuple(t.shape)} {t.dtype} (parameter count "
                                 f"{state.get('param_count')}), this trainer {self.flat.numel()} float32 parameters")
        with torch.no_grad():
            for key in ("flat", "m", "v", "vmax"):
                getattr(self, key).copy_(state[key])
        self.steps, self.lr, self.eps, self.amsgrad = int(state["steps"]), float(state["lr"]), float(state["eps"]), bool(state["amsgrad"])
        self.betas = (float(state["betas"][0]), float(state["betas"][1]))
        self._init_guard(state.get("max_grad_norm"), state.get("skip_nonfinite", False))
        self._weights_written()


class UtNetTrainer(_GuardedStep):
    kind = "UtNetTrainer"

    def __init__(self, model: UtNet, lr=1e-4, beta1=0.75, beta2=0.999, eps=1e-8, amsgrad=True,
                 weights=None, device=None, process_group=None, loss_cs=None, max_grad_norm=None, skip_nonfinite=False):
        self._init_base(model, device, process_group, weights, lr, (beta1, beta2), eps, amsgrad, loss_cs)
        self.funit = model.funit
        n = self.lib.nd_utnet_param_count(self.funit)
        if n == 0:
            raise ValueError(f"funit={self.funit} is not supported")
        self.flat = torch.zeros(n, dtype=torch.float32, device=self.device)
        sd = dict(model.named_parameters())
        self.ranges = {}
        for name, (off, cnt) in _lib.utnet_ranges(self.funit).items():
            if name not in sd:                 # a PReLU slope of a network with another activation: the step ignores its slot
                continue
            p = sd[name]
            assert p.numel() == cnt, (name, p.numel(), cnt)
            view = self.flat[off:off + cnt].view_as(p)
            view.copy_(p.data)
            p.data = view                      # the module now reads / writes the flat buffer
            self.ranges[name] = (off, cnt)
        self.blobs = torch.empty(self.lib.nd_utnet_train_blob_bytes(self.funit), dtype=torch.uint8, device=self.device)
        self._init_optimizer(max_grad_norm, skip_nonfinite)
        # data parallel: the gradient mean runs bucket by bucket (one per network level) under the rest of the backward pass
        self.averager = BucketedGradientAverager(self.funit, self.grads, self.group)

    def workspace(self, h, batch, w=None):
        """Training workspace for [batch,3,h,w or h] crops (zero borders initialised once, then cached)."""
        w = h if w is None else w
        return self._workspace((h, w, batch), self.lib.nd_utnet_train_workspace_bytes_hw, self.lib.nd_utnet_train_workspace_init_hw,
                               (self.funit, h, w, batch), "UtNet training")

    def forward_backward(self, noisy, clean):
        """Forward + loss + backward; fills self.grads (averaged over the process group).  Returns (output, loss tensor)."""
        noisy = noisy.to(self.device, torch.float32).contiguous()
        clean = clean.to(self.device, torch.float32).contiguous()
        if noisy.shape != clean.shape or noisy.dim() != 4 or noisy.size(1) != 3:
            raise ValueError(f"expected two [B,3,H,W] batches, got {tuple(noisy.shape)} and {tuple(clean.shape)}")
        batch, h, w = noisy.size(0), noisy.size(2), noisy.size(3)
        for cs in (h, w):
            if not valid_cs(cs):
                raise ValueError(f"crop side {cs} is not of the form 16k+56 (e.g. 136, 184)")
        y = torch.empty_like(noisy)
        with torch.cuda.device(self.device):
            ws = self.workspace(h, batch, w)
            # loss_cs: an L x L centre crop of the H x W output (pt_ops.pt_crop_batch), 0 = the whole output
            _lib.check(self.lib.nd_utnet_train_step_act_hw(
                self.funit, _lib.ACT[self.model.activation], self.model.flags, self.flat.data_ptr(), self.grads.data_ptr(),
                self.blobs.data_ptr(), noisy.data_ptr(), clean.data_ptr(), y.data_ptr(),
                float(self.weights.get("L1", 0.0)), float(self.weights.get("MSE", 0.0)),
                float(self.weights.get("SSIM", 0.0)), float(self.weights.get("MSSSIM", 0.0)),
                self.loss.data_ptr(), batch, h, w, int(self.loss_cs or 0), ws.data_ptr(),
                ws.numel(), _lib.stream_ptr(self.device), self.averager.event_ptrs,
                len(self.averager.buckets)), "nd_utnet_train_step_act_hw")
            # RCCL: nine all-reduces (0.6 ... 57 MB for UtNet(64)), each behind its bucket's event on a side stream
            self.averager.reduce()
        return y, self.loss

    def evaluate(self, validation_set, batch_size=32, output_to_dir=None, also=()):
        """The validation pass on this trainer's network, weights and loss crop (validation.validate): (mean weighted loss as a
        float, the per-sample weighted losses on the device).  A trainer with a process group shards the set over its ranks."""
        from .validation import validate
        return validate(self.model, validation_set, self.weights, self.loss_cs, batch_size=batch_size, output_to_dir=output_to_dir,
                        also=also, group=self.group)

    def _weights_written(self):
        # the parameters were rewritten through raw pointers (torch's version counters did not move): the inference blob the
        # module cached before this step is stale
        self.model.weights_generation += 1


unet_ranges = _lib.unet_ranges


def unet_flatten(model, flat, ranges):
    """Make every parameter AND every BatchNorm running statistic of `model` a view of `flat` (fp32, on the model's device) at its
    range, keeping the values.  The state-dict keeps its keys and shapes; num_batches_tracked has no slot and stays its own tensor."""
    seen = set()
    with torch.no_grad():
        for prefix, mod in model.named_modules():
            for kind, table in (("p", mod._parameters), ("b", mod._buffers)):
                for key, t in table.items():
                    name = f"{prefix}.{key}" if prefix else key
                    if t is None or name not in ranges:
                        continue
                    off, cnt = ranges[name]
                    assert t.numel() == cnt, (name, t.numel(), cnt)
                    view = flat[off:off + cnt].view(t.shape)
                    view.copy_(t)
                    if kind == "p":
                        t.data = view
                    else:
                        table[key] = view
                    seen.add(name)
    missing = set(ranges) - seen
    assert not missing, sorted(missing)


class UNetTrainer(_GuardedStep):
    """UNet training step on the GPU, with the surface of UtNetTrainer: BatchNorm on the statistics of the batch
    (nd_unet_train_forward / nd_unet_train_backward), the loss of nd_criteria_grad, Adam(amsgrad) in nd_adam_step.

    The module's parameters and its BatchNorm running statistics become views of ONE flat fp32 buffer (nd_unet_param_range).  The
    forward moves the running statistics in that buffer as torch's train-mode BatchNorm does (momentum of the module's BatchNorm
    layers); `num_batches_tracked` advances on the host side of the same call.

    One divergence from torch, on purpose: the bias of a convolution that feeds a BatchNorm gets a gradient of exactly 0 (its exact
    value: BatchNorm removes the channel mean), where torch leaves the rounding noise of a sum that cancels -- which Adam's
    g / (|g| + eps) would turn into full steps.  Those 18 biases therefore never move.

    The module itself is unchanged: `model.train()(x)` still raises, `model.eval()(x)` runs on the trained parameters and running
    statistics (the trainer drops the module's packed inference blob whenever it has written the flat buffer).

    max_grad_norm / skip_nonfinite (_GuardedStep) protect the parameter update only: a non-finite forward has already moved the
    BatchNorm running statistics and num_batches_tracked by the time the gradient is looked at."""
    kind, data_parallel = "UNetTrainer", False

    def __init__(self, model, lr=1e-4, beta1=0.75, beta2=0.999, eps=1e-8, amsgrad=True,
                 weights=None, device=None, process_group=None, loss_cs=None, max_grad_norm=None, skip_nonfinite=False):
        self._init_base(model, device, process_group, weights, lr, (beta1, beta2), eps, amsgrad, loss_cs)
        bns = [m for m in self.model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
        momenta = {m.momentum for m in bns}
        if len(momenta) != 1 or None in momenta:
            raise NotImplementedError(f"UNetTrainer: one numeric BatchNorm momentum for the whole network, got {sorted(map(str, momenta))}")
        self.momentum = float(momenta.pop())
        self._tracked = [m.num_batches_tracked for m in bns]
        self.ranges = unet_ranges()
        self.flat = torch.zeros(self.lib.nd_unet_param_count(), dtype=torch.float32, device=self.device)
        unet_flatten(self.model, self.flat, self.ranges)
        self.blobs = torch.empty(self.lib.nd_unet_train_blob_bytes(), dtype=torch.uint8, device=self.device)
        self._loss_ws = None
        self._init_optimizer(max_grad_norm, skip_nonfinite)      # (grads: the slots of running statistics are never written)

    @property
    def flags(self):
        return self.model.grad_flags

    def workspace(self, h, w, batch):
        """Training workspace for [batch,3,h,w] crops (zeroed once, then cached; another shape replaces it)."""
        return self._workspace((h, w, batch), self.lib.nd_unet_train_workspace_bytes, self.lib.nd_unet_train_workspace_init, (h, w, batch),
                               "UNet training")

    def _loss_workspace(self, batch, h, w):
        nbytes = self.lib.nd_criteria_grad_workspace_bytes(batch, h, w, int(self.loss_cs or 0))
        if nbytes == 0:      # let the library name what is wrong with the shape
            _lib.check(self.lib.nd_criteria_grad(None, None, batch, h, w, int(self.loss_cs or 0), 0.0, 0.0, 0.0, 0.0, None, None, None, 0,
                                                 None), "nd_criteria_grad")
        if self._loss_ws is None or self._loss_ws.numel() < nbytes:
            self._loss_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._loss_ws

    def forward(self, noisy):
        """The train-mode forward alone: output [B,3,H,W]; running statistics and num_batches_tracked advance."""
        noisy = noisy.to(self.device, torch.float32).contiguous()
        if noisy.dim() != 4 or noisy.size(1) != 3:
            raise ValueError(f"expected a [B,3,H,W] batch, got {tuple(noisy.shape)}")
        batch, h, w = noisy.size(0), noisy.size(2), noisy.size(3)
        y = torch.empty_like(noisy)
        with torch.cuda.device(self.device):
            ws = self.workspace(h, w, batch)
            _lib.check(self.lib.nd_unet_train_forward(self.flags, self.flat.data_ptr(), self.blobs.data_ptr(), noisy.data_ptr(),
                                                      y.data_ptr(), batch, h, w, self.momentum, ws.data_ptr(), ws.numel(),
                                                      _lib.stream_ptr(self.device)), "nd_unet_train_forward")
            torch._foreach_add_(self._tracked, 1)
        # the running statistics were rewritten through raw pointers (neither data_ptr nor torch's version counters moved): the
        # inference blob the module cached is stale
        self.model._packed = None
        return y

    def backward(self, gy, want_dx=False):
        """The backward of the last forward from gy = d loss / d output; fills self.grads.  Returns d loss / d input if asked."""
        gy = gy.to(self.device, torch.float32).contiguous()
        batch, h, w = gy.size(0), gy.size(2), gy.size(3)
        ws = self._ws.get((h, w, batch))
        if ws is None:
            raise RuntimeError("UNetTrainer.backward: no forward of this shape came before")
        dx = torch.empty_like(gy) if want_dx else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nd_unet_train_backward(self.flags, self.flat.data_ptr(), self.grads.data_ptr(), self.blobs.data_ptr(),
                                                       gy.data_ptr(), dx.data_ptr() if want_dx else None, batch, h, w, ws.data_ptr(),
                                                       ws.numel(), _lib.stream_ptr(self.device)), "nd_unet_train_backward")
        return dx

    def forward_backward(self, noisy, clean):
        """Forward + loss + backward, enqueued on one stream with no read from the GPU in between; fills self.grads.  Returns
        (output, loss tensor)."""
        noisy = noisy.to(self.device, torch.float32).contiguous()
        clean = clean.to(self.device, torch.float32).contiguous()
        if noisy.shape != clean.shape or noisy.dim() != 4 or noisy.size(1) != 3:
            raise ValueError(f"expected two [B,3,H,W] batches, got {tuple(noisy.shape)} and {tuple(clean.shape)}")
        batch, h, w = noisy.size(0), noisy.size(2), noisy.size(3)
        with torch.cuda.device(self.device):
            lws = self._loss_workspace(batch, h, w)       # refuses a bad loss window before anything runs
            y = self.forward(noisy)
            gy = torch.empty_like(y)
            # (without find_noise the output is a sigmoid: the criteria's clip to [0, 1] is inert)
            _lib.check(self.lib.nd_criteria_grad(y.data_ptr(), clean.data_ptr(), batch, h, w, int(self.loss_cs or 0),
                                                 *[float(self.weights.get(k) or 0.0) for k in ("L1", "MSE", "SSIM", "MSSSIM")],
                                                 self.loss.data_ptr(), gy.data_ptr(), lws.data_ptr(), lws.numel(),
                                                 _lib.stream_ptr(self.device)), "nd_criteria_grad")
            self.backward(gy)
        return y, self.loss

    def _weights_written(self):
        self.model._packed = None      # written through raw pointers: see forward

    def state_dict(self):
        state = super().state_dict()
        state["num_batches_tracked"] = [int(t) for t in self._tracked]      # the one piece of BatchNorm state outside the flat buffer
        return state

    def load_state_dict(self, state):
        super().load_state_dict(state)
        with torch.no_grad():
            for t, value in zip(self._tracked, state["num_batches_tracked"]):
                t.fill_(value)
