"""The validation pass of UtNet training on MI355X: the validation set in HBM, the network on the inference executor in batches,
per-sample criteria from one launch sequence (csrc/criteria.hip, nd_criteria), and the training form of the same criteria, the batch
loss with its gradient (nd_criteria_grad).

Restates validate_generator (nn_train.py:51-71) and ValidationDataset (dataset_torch_3.py:403-428) of the reference, which
validate one image at a time and read every file again every epoch: the loss of a validation pass is the mean over the images of
each image's own weighted loss (Generator.compute_loss on a batch of one, nn_common.py:226-241), so the batched pass needs the
criteria per sample, not per batch.

The set is read once, on the host: ValidationSet(val_tuples, device, cs) opens each path of the list as a crop file;
ValidationSet.from_full_size(val_tuples, dsdirs, ds_cs, ds_stride, device, cs) needs no crop file: it cuts the pairs whose paths
name crops of the full-size dataset dsdirs (crop_pool.crop_source) out of the full-size images, each decoded once, and gives the
same tensors bit for bit for PNG and TIFF sources (JPEG sources are decoded whole; equality with a jpegtran-cropped tree is not
claimed).  Neither runs a kernel: 300 pairs of 256 x 256 are no hot path.
"""
import os

import numpy as np
import torch
import yaml

from . import _lib
from .common.libs import np_imgops

COLUMNS = ("L1", "MSE", "SSIM", "MSSSIM")     # columns 0..3 of nd_criteria; column 4 is the weighted sum
_workspaces = {}                               # device -> uint8 tensor, grown on demand (nothing is carried between two calls)


def _workspace(device, nbytes):
    ws = _workspaces.get(str(device))
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[str(device)] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _checked(generated, target, weights, also=()):
    """The argument checks of criteria and criteria_grad; returns the two batches as contiguous float32 tensors."""
    if generated.shape != target.shape or generated.dim() != 4 or generated.size(1) != 3:
        raise ValueError(f"expected two [B,3,H,W] batches, got {tuple(generated.shape)} and {tuple(target.shape)}")
    if generated.device.type != "cuda" or target.device != generated.device:
        raise RuntimeError("criteria run on the GPU only (no CPU fallback): move both batches to the device")
    unknown = (set(k for k, v in weights.items() if v) | set(also)) - set(COLUMNS)
    if unknown:
        raise NotImplementedError(f"criteria {sorted(unknown)} are not available (L1, MSE, SSIM, MSSSIM)")
    return generated.detach().to(torch.float32).contiguous(), target.detach().to(torch.float32).contiguous()


def criteria(generated, target, weights, loss_cs=None, also=()):
    """Per-sample criteria of a batch: a dict of [B] float32 device tensors with keys L1, MSE, SSIM, MSSSIM and weighted.
    generated: the raw network output (it is clipped to [0, 1] here, Generator.denoise_batch); target: the clean batch; both
    [B,3,H,W] on the GPU.  weights: {name: weight}; a criterion is computed when its weight is not zero or `also` names it
    (--compute_SSIM_anyway), else its entry is zero.  loss_cs: the centre window the criteria see (None or 0: the whole image)."""
    y, t = _checked(generated, target, weights, also)
    n, _, h, w = y.shape
    loss_cs = int(loss_cs or 0)
    bits = sum(1 << COLUMNS.index(k) for k in set(also))
    lib = _lib.load()
    out = torch.empty(n, 5, dtype=torch.float32, device=y.device)
    with torch.cuda.device(y.device):
        nbytes = lib.nd_criteria_workspace_bytes(n, h, w, loss_cs)
        if nbytes == 0:      # let the library name what is wrong with the shape
            _lib.check(lib.nd_criteria(None, None, n, h, w, loss_cs, 0.0, 0.0, 0.0, 0.0, 0, None, None, 0, None), "nd_criteria")
        ws = _workspace(y.device, nbytes)
        _lib.check(lib.nd_criteria(y.data_ptr(), t.data_ptr(), n, h, w, loss_cs, *[float(weights.get(k) or 0.0) for k in COLUMNS],
                                   bits, out.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(y.device)), "nd_criteria")
    res = {k: out[:, i] for i, k in enumerate(COLUMNS)}
    res["weighted"] = out[:, 4]
    return res


def criteria_grad(generated, target, weights, loss_cs=None):
    """The training loss of a batch and its gradient (nd_criteria_grad, the loss section of the fused step): (loss, gy), a float32
    device scalar -- the weighted sum of the batch means of the criteria with a non-zero weight -- and d loss / d generated,
    [B,3,H,W], zero outside the loss_cs window.  Arguments as criteria."""
    y, t = _checked(generated, target, weights)
    n, _, h, w = y.shape
    loss_cs = int(loss_cs or 0)
    lib = _lib.load()
    loss = torch.empty((), dtype=torch.float32, device=y.device)
    gy = torch.empty_like(y)
    with torch.cuda.device(y.device):
        nbytes = lib.nd_criteria_grad_workspace_bytes(n, h, w, loss_cs)
        if nbytes == 0:      # let the library name what is wrong with the shape
            _lib.check(lib.nd_criteria_grad(None, None, n, h, w, loss_cs, 0.0, 0.0, 0.0, 0.0, None, None, None, 0, None), "nd_criteria_grad")
        ws = _workspace(y.device, nbytes)
        _lib.check(lib.nd_criteria_grad(y.data_ptr(), t.data_ptr(), n, h, w, loss_cs, *[float(weights.get(k) or 0.0) for k in COLUMNS],
                                        loss.data_ptr(), gy.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(y.device)),
                   "nd_criteria_grad")
    return loss, gy


def center_crop_pair(ximg, yimg, cs, names=("<clean>", "<noisy>")):
    """np_imgops.np_crop_img_pair(ximg, yimg, cs, CropMethod.CENTER) on two [3,H,W] arrays: x0 = (W - cs) // 2, y0 = (H - cs) // 2.
    ValueError naming the file for differing shapes or a side shorter than cs (the reference fails later, inside the network)."""
    if ximg.shape != yimg.shape:
        raise ValueError(f"ValidationSet: {names[0]} is {ximg.shape[2]}x{ximg.shape[1]} but {names[1]} is {yimg.shape[2]}x{yimg.shape[1]}")
    _, h, w = ximg.shape
    if h < cs or w < cs:
        raise ValueError(f"ValidationSet: {names[0]} is {w}x{h}, smaller than the crop size {cs}")
    x0, y0 = (w - cs) // 2, (h - cs) // 2
    return ximg[:, y0:y0 + cs, x0:x0 + cs], yimg[:, y0:y0 + cs, x0:x0 + cs]


class ValidationSet:
    """The reference's ValidationDataset, read once and kept in HBM: .clean and .noisy, two [N,3,cs,cs] float32 tensors.
    val_tuples: a list of [clean_path, noisy_path] pairs, or the path of a yaml file holding one.  Iterating gives the
    reference's items, (clean, noisy) per pair."""

    def __init__(self, val_tuples, device, cs):
        if isinstance(val_tuples, (str, os.PathLike)):
            with open(val_tuples, 'r') as fp:
                val_tuples = yaml.safe_load(fp)
        if not val_tuples:
            raise ValueError("ValidationSet: no validation pair")
        self.val_tuples = [list(pair) for pair in val_tuples]
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.cs = int(cs)
        clean = np.empty((len(self.val_tuples), 3, self.cs, self.cs), dtype=np.float32)
        noisy = np.empty_like(clean)
        for i, (xpath, ypath) in enumerate(self.val_tuples):
            ximg = np_imgops.img_path_to_np_flt(xpath)
            yimg = np_imgops.img_path_to_np_flt(ypath)
            clean[i], noisy[i] = center_crop_pair(ximg, yimg, self.cs, (xpath, ypath))
        self.clean = torch.from_numpy(clean).to(self.device)
        self.noisy = torch.from_numpy(noisy).to(self.device)

    @classmethod
    def from_full_size(cls, val_tuples, dsdirs, ds_cs=256, ds_stride=192, device=None, cs=None, crops_dir=None):
        """The set ValidationSet(val_tuples, device, cs) would read from the tree the reference's cropper (tools/crop_ds.py --cs
        ds_cs --stride ds_stride) writes for the full-size dataset(s) dsdirs, without that tree.  A pair whose two paths name
        crops of dsdirs (crop_pool.crop_source: by the last four components of the path, never by what exists on disk) is cut out
        of its two full-size images: each read with np_imgops.img_path_to_np_flt, rows [ybeg, ybeg + ds_cs), columns
        [xbeg, xbeg + ds_cs), then center_crop_pair to cs (default ds_cs).  A pair of two other paths is read from disk as the
        constructor reads it; a pair of one of each is ValueError.  A path that names a crop of dsdirs the cropper does not write
        is FileNotFoundError (crop_source), before any image is decoded.
        The pairs are taken file by file: sorted by (clean file, noisy file), two images at most in host memory, so a full-size
        file is decoded once -- once per clean partner, should a noisy file have several.  .clean[i], .noisy[i] and val_tuples
        keep the order and the paths given; n_windows pairs are windows into n_full_size_images files.
        For PNG and TIFF sources a crop file is a rectangle of its image and the float conversion is per sample: the two tensors
        are the constructor's on the cropped tree, bit for bit.  JPEG sources are decoded whole: equality with a jpegtran-cropped
        tree is not claimed, since a decoder upsamples chroma differently at the border of a crop file than inside the whole
        image (CropPool.from_full_size says the same)."""
        from .crop_pool import CropSources
        if isinstance(val_tuples, (str, os.PathLike)):
            with open(val_tuples, 'r') as fp:
                val_tuples = yaml.safe_load(fp)
        if not val_tuples:
            raise ValueError("ValidationSet: no validation pair")
        self = cls.__new__(cls)
        self.val_tuples = [list(pair) for pair in val_tuples]
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        ds_cs = int(ds_cs)
        self.cs = ds_cs if cs is None else int(cs)
        sources = CropSources(dsdirs, ds_cs, ds_stride, crops_dir)
        windows = []                                # (clean file, noisy file, pair, clean (ybeg, xbeg), noisy (ybeg, xbeg))
        clean = np.empty((len(self.val_tuples), 3, self.cs, self.cs), dtype=np.float32)
        noisy = np.empty_like(clean)
        for i, (xpath, ypath) in enumerate(self.val_tuples):
            xsrc, ysrc = sources.source(xpath), sources.source(ypath)
            if (xsrc is None) != (ysrc is None):
                raise ValueError(f"ValidationSet.from_full_size: of the pair {xpath}, {ypath} one path names a crop of {dsdirs} "
                                 f"and the other ({ypath if ysrc is None else xpath}) does not")
            if xsrc is not None:
                windows.append((xsrc[0], ysrc[0], i, xsrc[1:], ysrc[1:]))
        # path -> float32 [3,H,W]: the images of the pair being cut, and none but them (beside any that crop_source had to decode for
        # its size, which stay until they are used: no file is decoded twice)
        held, mine = sources.decoded, set()
        for xfile, yfile, i, (xy, xx), (yy, yx) in sorted(windows):
            for fpath in mine - {xfile, yfile}:
                del held[fpath]
            mine &= {xfile, yfile}
            for fpath in (xfile, yfile):
                if fpath not in held:
                    held[fpath] = np_imgops.img_path_to_np_flt(fpath)
                mine.add(fpath)
            clean[i], noisy[i] = center_crop_pair(held[xfile][:, xy:xy + ds_cs, xx:xx + ds_cs],
                                                  held[yfile][:, yy:yy + ds_cs, yx:yx + ds_cs], self.cs, tuple(self.val_tuples[i]))
        held.clear()
        inside = {w[2] for w in windows}
        for i, (xpath, ypath) in enumerate(self.val_tuples):
            if i not in inside:
                clean[i], noisy[i] = center_crop_pair(np_imgops.img_path_to_np_flt(xpath), np_imgops.img_path_to_np_flt(ypath),
                                                      self.cs, (xpath, ypath))
        self.n_windows = len(windows)
        self.n_full_size_images = len({f for w in windows for f in w[:2]})
        self.clean = torch.from_numpy(clean).to(self.device)
        self.noisy = torch.from_numpy(noisy).to(self.device)
        return self

    @classmethod
    def from_tensors(cls, clean, noisy, device=None):
        """A set from two [N,3,cs,cs] batches that are already cropped (no file is read)."""
        if clean.shape != noisy.shape or clean.dim() != 4 or clean.size(1) != 3 or clean.size(2) != clean.size(3) or not len(clean):
            raise ValueError(f"ValidationSet.from_tensors: expected two [N,3,cs,cs] batches, got {tuple(clean.shape)} and {tuple(noisy.shape)}")
        self = cls.__new__(cls)
        self.val_tuples = None
        self.device = torch.device(device) if device is not None else clean.device
        self.cs = clean.size(2)
        self.clean = clean.to(self.device, torch.float32).contiguous()
        self.noisy = noisy.to(self.device, torch.float32).contiguous()
        return self

    def __len__(self):
        return self.clean.shape[0]

    def __getitem__(self, i):
        return self.clean[i], self.noisy[i]


def shard_indices(n, rank, world):
    """The samples of a set of n that rank `rank` of `world` validates: a contiguous slice, the slices in rank order cover
    range(n) once, and their lengths differ by one at most (empty for some ranks when n < world)."""
    if n < 0 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"shard_indices: n {n}, rank {rank}, world {world}")
    return range(n * rank // world, n * (rank + 1) // world)


def gather_in_order(local, n, group):
    """local: this rank's values for shard_indices(n, rank, world), a 1-D tensor.  Returns the [n] vector in index order, on
    local's device, the same bits on every rank: one all-gather of slices padded to the longest one (through host memory on a
    gloo group), then copies only."""
    import torch.distributed as tdist
    from .dist import _host_staged
    rank, world = tdist.get_rank(group), tdist.get_world_size(group)
    lengths = [len(shard_indices(n, r, world)) for r in range(world)]
    if local.dim() != 1 or local.numel() != lengths[rank]:
        raise ValueError(f"gather_in_order: rank {rank} of {world} holds {tuple(local.shape)} values, its slice of {n} has {lengths[rank]}")
    if world == 1:
        return local
    staged = local.is_cuda and _host_staged(group)
    wire = torch.zeros(max(lengths), dtype=local.dtype, device="cpu" if staged else local.device)
    wire[:lengths[rank]] = local
    parts = [torch.empty_like(wire) for _ in range(world)]
    tdist.all_gather(parts, wire, group=group)
    return torch.cat([part[:length] for part, length in zip(parts, lengths)]).to(local.device)


def validate(model, validation_set, weights, loss_cs, batch_size=32, output_to_dir=None, also=(), group=None):
    """validate_generator (nn_train.py:51-71) with its batch-1 loop batched: the module in eval() mode under no_grad -- the
    inference executor, the arithmetic denoise_image runs on the checkpoint -- over the set in batches (the last one partial), the
    per-sample criteria of each batch, and the mean over all samples of the weighted loss.  Returns (that mean as a Python float,
    the per-sample weighted losses as an [N] device tensor); one host synchronisation per call.  The module is left in train()
    mode, as the reference leaves it.
    output_to_dir (debug option output_val_images): <dir>/<i>.tif, 8-bit, the clipped output with its borders.
    group (a torch.distributed process group; None: this process validates the whole set): every rank of the group calls this
    with the same set and a model with the same parameters; rank r runs the samples shard_indices(N, r, world) (none, when its
    slice is empty) and writes their images, the per-sample values are gathered in index order, and every rank returns the same
    mean and the same [N] vector.  With UtNet.split_k = False a sample's value does not depend on its batch, and both are then
    the single-process ones bit for bit."""
    if batch_size < 1:
        raise ValueError(f"validate: batch_size {batch_size}")
    n = len(validation_set)
    mine = range(n)
    if group is not None:
        import torch.distributed as tdist
        mine = shard_indices(n, tdist.get_rank(group), tdist.get_world_size(group))
    per_sample = torch.empty(len(mine), dtype=torch.float32, device=validation_set.clean.device)
    outputs = []
    model.eval()
    try:
        with torch.no_grad():
            for b0 in range(mine.start, mine.stop, batch_size):
                b1 = min(b0 + batch_size, mine.stop)
                noisy, clean = validation_set.noisy[b0:b1], validation_set.clean[b0:b1]
                y = model(noisy)
                per_sample[b0 - mine.start:b1 - mine.start] = criteria(y, clean, weights, loss_cs, also)["weighted"]
                if output_to_dir is not None:
                    outputs.append(y)
    finally:
        model.train()
    if group is not None:
        per_sample = gather_in_order(per_sample, n, group)
    # the mean in float64 over the fp32 per-sample values, as statistics.mean of the reference's Python floats; one synchronisation
    avgloss = per_sample.double().mean().item()
    if output_to_dir is not None:
        from .denoise_image import _save_dbg_jpg      # torchvision.utils.save_image's conversion: clamp, * 255 + 0.5, uint8
        os.makedirs(output_to_dir, exist_ok=True)
        for i, img in zip(mine, torch.cat(outputs) if outputs else ()):
            _save_dbg_jpg(img, os.path.join(output_to_dir, str(i) + '.tif'))
    return avgloss, per_sample
