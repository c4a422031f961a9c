"""Device-resident crop pool: the data side of UtNet training on MI355X.

Stands in for DenoisingDataset + DataLoader of the reference (dataset_torch_3.py:98-279, nn_train.py:239): the pre-cropped dataset is uploaded once, in the sample type of its files (u8 / u16 / f32), and every training
batch -- random pick of a clean and a noisy image per group, random crop or centred zero padding, rot90, two flips, exposure
multiplier -- is made by one HIP launch (csrc/crop_batch.hip, nd_crop_batch) from a small table of draws that torch ops fill on
the device under one seeded generator.  No file decode, no worker processes and no host-to-device copy per step.

    pool = CropPool.from_directories(["datasets/train/NIND_256_192"], test_reserve=["ursulines-red"])
    for draws in pool.epoch(30, cs=184):
        clean, noisy = pool.batch(draws)          # the reference's batch[0] is the clean one
        trainer.learn(noisy, clean)

Not built: the sigmamin / sigmamax artificial noise and the JPEG re-compression branch of the reference's __getitem__ (the first is
"rarely used / experimental" by its docstring, the second calls .save on a numpy array).
"""
import os

import numpy as np
import torch

from . import _lib
from .common.libs import np_imgops
from .dataset_torch_3 import sortISOs

_TYPES = {np.dtype(np.uint8): _lib.SAMPLE_U8, np.dtype(np.uint16): _lib.SAMPLE_U16, np.dtype(np.float32): _lib.SAMPLE_F32}
_ALIGN = 16


def pack_draws(clean, noisy, x0, y0, nrot, flip1, flip2, u, device=None):
    """The [B, 8] int32 draw table of nd_crop_batch from its eight columns (sequences or tensors); u is stored as float32 bits."""
    cols = [torch.as_tensor(c, device=device).to(torch.int32).reshape(-1) for c in (clean, noisy, x0, y0, nrot, flip1, flip2)]
    ubits = torch.as_tensor(u, device=device).to(torch.float32).reshape(-1).view(torch.int32)
    return torch.stack(cols + [ubits], dim=1).contiguous()


def _to_chw(img):
    """HWC, CHW or HW samples -> contiguous RGB [3, H, W] in the array's own type."""
    img = np.asarray(img)
    if img.dtype not in _TYPES:
        raise TypeError(f"CropPool: samples must be uint8, uint16 or float32, got {img.dtype}")
    if img.ndim == 3 and img.shape[0] == 3 and img.shape[2] != 3:
        return np.ascontiguousarray(img)
    if img.ndim == 2 or (img.ndim == 3 and img.shape[2] in (1, 2, 3, 4)):
        return np.ascontiguousarray(np_imgops.hwc_to_rgb(img).transpose(2, 0, 1))
    raise ValueError(f"CropPool: expected an HWC or CHW image, got shape {img.shape}")


class Draws:
    """One batch of draws a pool made itself: valid by construction, so CropPool.batch takes it without looking at its values."""

    def __init__(self, pool, table, cs, groups):
        self.pool, self.table, self.cs, self.groups = pool, table, cs, groups

    def __len__(self):
        return self.table.shape[0]


class CropPool:
    def __init__(self, device=None, seed=0, cs=None):
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.cs = cs
        self.generator = torch.Generator(device=self.device)
        self.generator.manual_seed(seed)
        self._staged = []        # host arrays not yet uploaded
        self._images = []        # (byte offset, H, W, sample type) per image
        self.sets = []           # from_directories: (datadir, set, crop file, base ISOs, other ISOs) per group
        self._groups = []        # (first clean image, clean images, first noisy image, noisy images, H, W) per group
        self._bytes = 0
        self._pool = self._table = self._gt = None
        self.last_xmax = self.last_mult = None

    # ------------------------------------------------------------------ filling
    def _add_image(self, chw):
        off = self._bytes
        self._staged.append((off, chw))
        self._images.append((off, chw.shape[1], chw.shape[2], _TYPES[chw.dtype]))
        self._bytes = (off + chw.nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        return len(self._images) - 1

    def add_group(self, clean_images, noisy_images):
        """One entry of the reference's self.dataset: the images of its base ISOs and of its other ISOs, all of one size.  When the
        two lists hold the same arrays (a clean-clean entry) they are uploaded once.  Returns the group's index."""
        if self._pool is not None:
            raise RuntimeError("CropPool: the pool was uploaded by its first batch; add every group before that")
        if not len(clean_images) or not len(noisy_images):
            raise ValueError("CropPool.add_group: a group needs at least one clean and one noisy image")
        clean_images, noisy_images = list(clean_images), list(noisy_images)
        same = len(clean_images) == len(noisy_images) and all(c is n for c, n in zip(clean_images, noisy_images))
        lists = [[_to_chw(img) for img in images] for images in ((clean_images,) if same else (clean_images, noisy_images))]
        shapes = {a.shape for images in lists for a in images}
        if len(shapes) != 1:
            raise ValueError(f"CropPool.add_group: the images of a group must have one size, got {sorted(shapes)}")
        # the clean and the noisy images of a group are consecutive in the table: a pick is first + floor(random * count)
        first = [[self._add_image(a) for a in images][0] for images in lists]
        if same:
            first.append(first[0])
        _, h, w = lists[0][0].shape
        self._groups.append((first[0], len(clean_images), first[1], len(noisy_images), h, w))
        self._gt = None
        return len(self._groups) - 1

    def keep_groups(self, count):
        """Drops every group past the first `count` (debug option short_run: DDataset.dataset[:3 * batch_size], nn_train.py:225-226),
        and with them the images no remaining group names.  Only before the first upload."""
        if self._pool is not None:
            raise RuntimeError("CropPool: the pool was uploaded by its first batch; drop groups before that")
        if count < 0:
            raise ValueError(f"CropPool.keep_groups: count {count}")
        if count >= len(self._groups):
            return
        groups, staged = self._groups[:count], dict(self._staged)
        arrays = [staged[off] for off, _, _, _ in self._images]
        self.sets = self.sets[:count]
        self._staged, self._images, self._groups, self._bytes, self._gt = [], [], [], 0, None
        moved = {}
        for c0, nc, n0, nn, h, w in groups:        # images of a group are consecutive: re-add each run once, in the old order
            first = []
            for i0, cnt in ((c0, nc), (n0, nn)):
                if i0 not in moved:
                    moved[i0] = [self._add_image(arrays[i]) for i in range(i0, i0 + cnt)][0]
                first.append(moved[i0])
            self._groups.append((first[0], nc, first[1], nn, h, w))

    @classmethod
    def from_directories(cls, datadirs, test_reserve=(), exact_reserve=False, min_crop_size=None, device=None, seed=0, cs=None):
        """The scan of DenoisingDataset.__init__ (dataset_torch_3.py:166-192) over <datadir>/<set>/ISO*/<crop files>: one group per
        crop file of a set's first noisy ISO, holding that crop at every base ISO and at every other ISO.  Sets named by test_reserve
        are left out (exact_reserve: by equality, else by substring); with min_crop_size, crops with a shorter side are left out.
        cs defaults to the <CS> of a directory named <DSNAME>_<CS>_<UCS>.  Directory listings are taken in sorted order."""
        if isinstance(datadirs, (str, os.PathLike)):
            datadirs = [datadirs]
        if cs is None:
            parts = os.path.basename(os.path.normpath(os.fspath(datadirs[0]))).split('_')
            if len(parts) >= 3 and parts[-2].isdigit() and parts[-1].isdigit():
                cs = int(parts[-2])
        pool = cls(device, seed=seed, cs=cs)

        def reserved(aset):
            if exact_reserve:
                return aset in test_reserve
            return any(s in aset for s in test_reserve)

        def read(fpath):
            try:
                return np_imgops.img_path_to_np_samples(fpath)
            except FileNotFoundError:
                raise
            except Exception as e:
                raise ValueError(f"CropPool.from_directories: cannot read {fpath}: {e}") from e

        for datadir in datadirs:
            datadir = os.fspath(datadir)
            for aset in sorted(os.listdir(datadir)):
                if reserved(aset):
                    continue
                bisos, isos = sortISOs(os.listdir(os.path.join(datadir, aset)))
                if not isos:
                    raise ValueError(f"CropPool.from_directories: {os.path.join(datadir, aset)} has no noisy ISO directory")
                for animg in sorted(os.listdir(os.path.join(datadir, aset, isos[0]))):
                    def path_of(iso):
                        return os.path.join(datadir, aset, iso, animg.replace(isos[0] + '_', iso + '_'))
                    noisy = [read(path_of(iso)) for iso in isos]
                    if min_crop_size is not None and any(d < min_crop_size for d in noisy[0].shape[1:]):
                        continue
                    pool.add_group([read(path_of(iso)) for iso in bisos], noisy)
                    pool.sets.append((datadir, aset, animg, tuple(bisos), tuple(isos)))
        return pool

    @property
    def nbytes(self):
        """Bytes of the pool buffer (images in their own sample type, each aligned to 16 bytes)."""
        return self._bytes

    @property
    def n_groups(self):
        return len(self._groups)

    @property
    def n_images(self):
        return len(self._images)

    def group(self, g):
        """(clean image indices, noisy image indices, H, W) of group g."""
        c0, nc, n0, nn, h, w = self._groups[g]
        return list(range(c0, c0 + nc)), list(range(n0, n0 + nn)), h, w

    def image(self, i):
        """Image i as the pool holds it: a [3, H, W] numpy array of its sample type (read back from the device once uploaded)."""
        off, h, w, typ = self._images[i]
        dtype = [k for k, v in _TYPES.items() if v == typ][0]
        if self._pool is None:
            return dict(self._staged)[off]
        raw = self._pool[off:off + 3 * h * w * dtype.itemsize].cpu().numpy()
        return raw.view(dtype).reshape(3, h, w)

    # ------------------------------------------------------------------ draws
    def seed(self, seed):
        self.generator.manual_seed(seed)

    def _group_table(self):
        if self._gt is None:
            if not self._groups:
                raise ValueError("CropPool: the pool has no group")
            self._gt = torch.tensor(self._groups, dtype=torch.int64).to(self.device)
        return self._gt

    def _cs(self, cs):
        cs = self.cs if cs is None else cs
        if cs is None or int(cs) != cs or not 1 <= cs <= 16384:
            raise ValueError(f"CropPool: crop size {cs!r} (give cs, or set it on the pool)")
        return int(cs)

    def _draw_groups(self, groups, cs):
        gt = self._group_table()[groups]                                   # [B, 6]
        n = groups.shape[0]
        g = self.generator
        r = torch.rand(n, 4, dtype=torch.float64, device=self.device, generator=g)
        bits = torch.randint(0, 16, (n,), device=self.device, generator=g)
        u = torch.rand(n, dtype=torch.float32, device=self.device, generator=g)

        def pick(col, count):       # uniform over [0, count): floor(r * count), clamped against a product that rounds up
            return torch.minimum((r[:, col] * count).to(torch.int64), count - 1)

        clean = gt[:, 0] + pick(0, gt[:, 1])                               # get_x_y_paths: two independent choices
        noisy = gt[:, 2] + pick(1, gt[:, 3])
        x0 = pick(2, (gt[:, 5] - cs).clamp_(min=0) + 1)                    # randint(0, W - cs); a padded side gets 0
        y0 = pick(3, (gt[:, 4] - cs).clamp_(min=0) + 1)
        table = pack_draws(clean, noisy, x0, y0, bits & 3, (bits >> 2) & 1, (bits >> 3) & 1, u)
        return Draws(self, table, cs, groups)

    def draw(self, batch_size, cs=None):
        """Draws for batch_size samples of groups taken uniformly with replacement."""
        cs = self._cs(cs)
        self._group_table()
        if batch_size < 1:
            raise ValueError(f"CropPool.draw: batch_size {batch_size}")
        groups = torch.randint(0, self.n_groups, (batch_size,), device=self.device, generator=self.generator)
        return self._draw_groups(groups, cs)

    def epoch(self, batch_size, cs=None, rank=0, world=1):
        """One pass over the groups in a random order, in full batches (DataLoader(shuffle=True, drop_last=True)).  With world > 1
        every rank must hold a pool with the same groups and generator state: batch k of the single-rank epoch goes to rank
        k % world, each rank gets the same number of batches (the last len(epoch) % world batches are dropped), and the generator
        advances alike on all ranks."""
        cs = self._cs(cs)
        self._group_table()
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"CropPool.epoch: batch_size {batch_size}, rank {rank}, world {world}")
        perm = torch.randperm(self.n_groups, device=self.device, generator=self.generator)
        steps = self.n_groups // batch_size // world
        for k in range(steps * world):
            draws = self._draw_groups(perm[k * batch_size:(k + 1) * batch_size], cs)
            if k % world == rank:
                yield draws

    # ------------------------------------------------------------------ batches
    def device_buffers(self):
        """(pool bytes, image table) as nd_crop_batch takes them: a uint8 tensor and an int64 [images, 4] tensor on the device; the
        first call uploads them."""
        return self._upload()

    def _upload(self):
        if self._pool is None:
            if not self._images:
                raise ValueError("CropPool: the pool has no image")
            if self.device.type != "cuda":
                raise RuntimeError("CropPool.batch needs a GPU (no CPU fallback)")
            host = np.zeros(self._bytes, dtype=np.uint8)
            for off, chw in self._staged:
                host[off:off + chw.nbytes] = chw.reshape(-1).view(np.uint8)
            self._pool = torch.from_numpy(host).to(self.device)
            self._table = torch.tensor(self._images, dtype=torch.int64).to(self.device)
            self._staged = []
        return self._pool, self._table

    def validate(self, draws, cs):
        """Host check of a draw table that did not come from this pool; ValueError names the first thing wrong."""
        t = torch.as_tensor(draws)
        if t.dim() != 2 or t.shape[1] != 8 or t.shape[0] < 1 or t.dtype != torch.int32:
            raise ValueError(f"CropPool: draws must be an int32 [B, 8] table (pack_draws), got {t.dtype} {tuple(t.shape)}")
        d = t.cpu().numpy()
        images = np.asarray(self._images, dtype=np.int64).reshape(-1, 4)
        for name, col in (("clean", 0), ("noisy", 1)):
            if ((d[:, col] < 0) | (d[:, col] >= len(images))).any():
                raise ValueError(f"CropPool: {name} image index outside [0, {len(images)})")
        hc, wc = images[d[:, 0], 1], images[d[:, 0], 2]
        if (hc != images[d[:, 1], 1]).any() or (wc != images[d[:, 1], 2]).any():
            raise ValueError("CropPool: a draw pairs a clean and a noisy image of different sizes")
        if ((d[:, 2] < 0) | (d[:, 2] > np.maximum(wc - cs, 0))).any():
            raise ValueError("CropPool: x0 outside [0, max(W - cs, 0)]")
        if ((d[:, 3] < 0) | (d[:, 3] > np.maximum(hc - cs, 0))).any():
            raise ValueError("CropPool: y0 outside [0, max(H - cs, 0)]")
        if ((d[:, 4] < 0) | (d[:, 4] > 3)).any():
            raise ValueError("CropPool: nrot outside 0..3")
        if ((d[:, 5:7] < 0) | (d[:, 5:7] > 1)).any():
            raise ValueError("CropPool: flip1 / flip2 must be 0 or 1")
        u = np.ascontiguousarray(d[:, 7]).view(np.float32)
        if not ((u >= 0) & (u < 1)).all():
            raise ValueError("CropPool: u outside [0, 1)")
        return t

    def batch(self, draws, cs=None, exp_mult_min=1, exp_mult_max=1, mult=None, out=None):
        """(clean, noisy): two [B,3,cs,cs] float32 tensors on the pool's device, made by one launch on the current stream.
        draws: what draw() / epoch() gave (cs is theirs), or an int32 [B, 8] table (pack_draws), which is checked on the host first.
        The exposure multiplier is drawn when exp_mult_min != 1 (dataset_torch_3.py:271); mult, a float32 [B] tensor, gives it per
        sample instead.  After a batch with a drawn multiplier, last_xmax and last_mult hold the per-sample maxima and multipliers.
        out: a (clean, noisy) pair of tensors to write into."""
        if isinstance(draws, Draws):
            if draws.pool is not self:
                raise ValueError("CropPool.batch: these draws were made by another pool")
            if cs is not None and cs != draws.cs:
                raise ValueError(f"CropPool.batch: the draws were made for cs {draws.cs}, not {cs}")
            cs, table = draws.cs, draws.table
        else:
            cs = self._cs(cs)
            table = self.validate(draws, cs)
        pool, images = self._upload()
        table = table.to(self.device).contiguous()
        n = table.shape[0]
        if not 1 <= n <= 65535:
            raise ValueError(f"CropPool.batch: batch {n} outside [1, 65535]")
        if out is None:
            clean = torch.empty(n, 3, cs, cs, dtype=torch.float32, device=self.device)
            noisy = torch.empty_like(clean)
        else:
            clean, noisy = out
            for t in (clean, noisy):
                if t.shape != (n, 3, cs, cs) or t.dtype != torch.float32 or t.device != self.device or not t.is_contiguous():
                    raise ValueError(f"CropPool.batch: out tensors must be contiguous float32 [{n},3,{cs},{cs}] on {self.device}")
        if mult is not None:
            mult = torch.as_tensor(mult, dtype=torch.float32).to(self.device).contiguous()
            if mult.shape != (n,):
                raise ValueError(f"CropPool.batch: mult must hold {n} values, got {tuple(mult.shape)}")
        xmax = mout = None
        if mult is None and float(exp_mult_min) != 1.0:
            if not exp_mult_min <= exp_mult_max:
                raise ValueError(f"CropPool.batch: exp_mult_min {exp_mult_min} > exp_mult_max {exp_mult_max}")
            xmax, mout = torch.empty(2, n, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().nd_crop_batch(
                pool.data_ptr(), pool.numel(), images.data_ptr(), images.shape[0], table.data_ptr(), n, cs, float(exp_mult_min),
                float(exp_mult_max), None if mult is None else mult.data_ptr(), None if xmax is None else xmax.data_ptr(),
                None if mout is None else mout.data_ptr(), clean.data_ptr(), noisy.data_ptr(), _lib.stream_ptr(self.device)),
                "nd_crop_batch")
        self.last_xmax, self.last_mult = xmax, mout
        return clean, noisy
