"""Device-resident crop pool: the data side of UtNet training on MI355X.

Stands in for DenoisingDataset + DataLoader of the reference (dataset_torch_3.py:98-279, nn_train.py:239): the pre-cropped dataset is uploaded once, in the sample type of its files (u8 / u16 / f32), and every training
batch -- random pick of a clean and a noisy image per group, random crop or centred zero padding, rot90, two flips, exposure
multiplier -- is made by one HIP launch (csrc/crop_batch.hip, nd_crop_batch) from a small table of draws that torch ops fill on
the device under one seeded generator.  No file decode, no worker processes and no host-to-device copy per step.

    pool = CropPool.from_directories(["datasets/train/NIND_256_192"], test_reserve=["ursulines-red"])
    for draws in pool.epoch(30, cs=184):
        clean, noisy = pool.batch(draws)          # the reference's batch[0] is the clean one
        trainer.learn(noisy, clean)

Quality bar (DenoisingDataset.list_content_quality and the docstring of PickyDenoisingDatasetFromList, dataset_torch_3.py:215-298):
score_pairs() gives the MS-SSIM of every (clean, noisy) pair of the resident files, list_content_quality() writes the reference's
csv, and after set_min_quality(q) draws take only pairs whose score is above q.

Without the pre-cropped dataset: CropPool.from_full_size reads the full-size images, keeps each once in HBM as a frame, and makes
of every crop the reference's cropper would have written (crop_grid: tools/crop_img.sh) a window into its frame.  Groups, draws,
batches and scores are those of the pool of crop files, bit for bit (nd_crop_batch_windows, nd_pool_fetch_windows).
crop_source goes the other way, from the path of a crop file to its window of a full-size image (the validation lists name crop
files: validation.ValidationSet.from_full_size); set_images and crop_names are the naming both share.

Not built: the sigmamin / sigmamax artificial noise and the JPEG re-compression branch of the reference's __getitem__ (the first is
"rarely used / experimental" by its docstring, the second calls .save on a numpy array).
"""
import csv
import math
import os
import re

import numpy as np
import torch

from . import _lib
from .common.libs import imgcodec, np_imgops, utilities
from .dataset_torch_3 import sortISOs

_TYPES = {np.dtype(np.uint8): _lib.SAMPLE_U8, np.dtype(np.uint16): _lib.SAMPLE_U16, np.dtype(np.float32): _lib.SAMPLE_F32}
_ALIGN = 16
MS_SSIM_MIN_SIDE = 161      # nd_ms_ssim (include/nind_hip.h): five scales of an 11-tap window; below it piqa raises


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


def _tdiv(a, b):
    """a / b as bash's $(( )) divides: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def crop_grid(width, height, cs, stride):
    """(xcrop, ycrop, xbeg, ybeg) of every crop the reference's cropper writes for a width x height image, in its loop's order
    (rows outer): the arithmetic of tools/crop_img.sh:28-64 as it stands.  The crop is the cs x cs rectangle at (xbeg, ybeg), and its
    file is <basename>_<xcrop>_<ycrop>_<stride>.<ext>.  The loop runs over width / stride + 1 columns and height / stride + 1 rows; a
    crop is written only when it is a full cs x cs, its origin is not negative and its useful size is at least stride, so the first
    column and row (cs - (cs - stride) / 2 wide, unless cs == stride) and the last ones (cut by the image's edge) never are: the
    first crop starts at stride - (cs - stride) / 2, and an image with a side below that plus cs yields nothing.  ValueError unless
    cs and stride are non-negative multiples of 8, where the script exits."""
    for name, v in (("cs", cs), ("stride", stride)):
        if isinstance(v, bool) or int(v) != v or v < 0 or v % 8:
            raise ValueError(f"crop_grid: {name} {v!r} is an invalid crop size, must be a multiple of 8")
    cs, stride, width, height = int(cs), int(stride), int(width), int(height)
    if stride == 0:
        raise ValueError("crop_grid: stride 0 (the script divides by it)")
    margin = _tdiv(cs - stride, 2)
    nx, ny = _tdiv(width, stride) + 1, _tdiv(height, stride) + 1
    crops = []
    for cury in range(ny):
        for curx in range(nx):
            xcs = ycs = cs
            cucs = stride
            xbeg, ybeg = curx * stride - margin, cury * stride - margin
            if curx == 0:
                xcs, xbeg = cs - margin, 0
            if cury == 0:
                ycs, ybeg = cs - margin, 0
            xcs, ycs = min(xcs, width - xbeg), min(ycs, height - ybeg)
            if curx == nx - 1:
                cucs = xcs - margin
            if cury == ny - 1:
                cucs = min(cucs, ycs - margin)
            if xbeg >= 0 and ybeg >= 0 and cucs >= stride and ycs == cs and xcs == cs:
                # every written crop's name ends in _<stride>: another useful size needs a last column or row that is a full cs,
                # and there width % stride + (cs - stride) / 2 < cs
                crops.append((curx, cury, xbeg, ybeg))
    return crops


def findisoval(fn):
    """The ISO value of a full-size file name as the reference's cropper finds it (tools/crop_ds.py:32-39); None if it has none."""
    for part in fn.split('_'):          # the first part that says ISO, GT or NOISY decides
        if 'ISO' in part:
            return part.split('.')[0]
        for word in ('GT', 'NOISY'):    # from the word to the first dot, underscores included
            if word in part:
                return fn[fn.find(word):].split('.')[0]
    return None


def set_images(set_dpath):
    """{ISO: (path of the full-size file, the name the cropper would have cropped it under)} of one set directory of a full-size
    dataset, in sorted file order: the ISO of a file as the cropper finds it (findisoval); a second file with an ISO already seen
    is <iso>-2, a third <iso>-2-2, and named as if it had been renamed so (tools/crop_ds.py:48-55).  No file is opened.
    ValueError for a file that names no ISO value."""
    files = {}
    for image in sorted(os.listdir(set_dpath)):
        iso = old = findisoval(image)
        if iso is None:
            raise ValueError(f"crop_pool.set_images: {os.path.join(set_dpath, image)} names no ISO value "
                             "(ISO<value>, GT... or NOISY... between underscores)")
        while iso in files:
            iso += '-2'
        files[iso] = (os.path.join(set_dpath, image), image.replace(old, iso))
    return files


def crop_names(name, width, height, ds_cs, ds_stride):
    """{crop file name: (xbeg, ybeg)} of the crops the cropper writes for a width x height image it crops under `name`, in its
    loop's order: <name less its last four characters>_<xcrop>_<ycrop>_<ds_stride>.<the last three, in lower case>
    (tools/crop_img.sh:9-10, 26)."""
    stem, ext = name[:-4], name.lower()[-3:]
    return {f'{stem}_{xc}_{yc}_{ds_stride}.{ext}': (xb, yb) for xc, yc, xb, yb in crop_grid(width, height, ds_cs, ds_stride)}


def crops_dirs_of(dsdirs, ds_cs, ds_stride, crops_dir=None):
    """(dsdirs as a list of strings, the directory of each one's cropped tree): crops_dir, one path per dsdir, or the cropper's own
    <root of dsdir>/cropped/<leaf of dsdir>_<ds_cs>_<ds_stride>.  ValueError when the two lists differ in length."""
    if isinstance(dsdirs, (str, os.PathLike)):
        dsdirs = [dsdirs]
    dsdirs = [os.fspath(d) for d in dsdirs]
    if crops_dir is None:
        return dsdirs, [os.path.join(utilities.get_root(d), 'cropped', f'{utilities.get_leaf(d)}_{ds_cs}_{ds_stride}') for d in dsdirs]
    crops_dirs = [os.fspath(crops_dir)] if isinstance(crops_dir, (str, os.PathLike)) else [os.fspath(d) for d in crops_dir]
    if len(crops_dirs) != len(dsdirs):
        raise ValueError(f"crop_pool: {len(crops_dirs)} crops_dir for {len(dsdirs)} dataset directories")
    return dsdirs, crops_dirs


class CropSources:
    """crop_source for many paths of one dataset: the table of a set and the crop names of an image are made once.  decoded holds
    the images that had to be decoded for their size (float32 [3,H,W], by path), for the caller to take instead of decoding again;
    image_size gives the size of every format np_imgops reads from the header, so it stays empty."""

    def __init__(self, dsdirs, ds_cs, ds_stride, crops_dir=None):
        self.dsdirs, self.crops_dirs = crops_dirs_of(dsdirs, ds_cs, ds_stride, crops_dir)
        crop_grid(0, 0, ds_cs, ds_stride)
        self.ds_cs, self.ds_stride = int(ds_cs), int(ds_stride)
        self.leaves = [utilities.get_leaf(d) for d in self.crops_dirs]
        self.decoded = {}
        self._sets, self._names = {}, {}

    def _names_of(self, fpath, name):
        if fpath not in self._names:
            size = imgcodec.image_size(fpath)
            if size is None:
                self.decoded[fpath] = np_imgops.img_path_to_np_flt(fpath)
                size = self.decoded[fpath].shape[2], self.decoded[fpath].shape[1]
            self._names[fpath] = (crop_names(name, size[0], size[1], self.ds_cs, self.ds_stride), size)
        return self._names[fpath]

    def source(self, crop_path):
        given = os.fspath(crop_path)
        parts = [p for p in given.replace(os.sep, '/').split('/') if p and p != '.']
        if len(parts) < 4 or parts[-4] not in self.leaves:
            return None
        leaf, aset, iso, fname = parts[-4:]
        dsdir = self.dsdirs[self.leaves.index(leaf)]
        set_dpath = os.path.join(dsdir, aset)
        if aset in ('.', '..') or not os.path.isdir(set_dpath):
            raise FileNotFoundError(f"{given}: {dsdir} has no set {aset!r}")
        if set_dpath not in self._sets:
            self._sets[set_dpath] = set_images(set_dpath)
        if iso not in self._sets[set_dpath]:
            raise FileNotFoundError(f"{given}: {set_dpath} has no image of ISO {iso!r} (it has {', '.join(self._sets[set_dpath])})")
        fpath, name = self._sets[set_dpath][iso]
        names, (width, height) = self._names_of(fpath, name)
        if fname not in names:
            # the crop of the same indices, where the name shows them and the grid yields them (another extension, stem or stride
            # suffix), else the first one
            m = re.fullmatch(r'.*_(\d+)_(\d+)_\d+\.[^.]*', fname)
            example = m and f'{name[:-4]}_{m[1]}_{m[2]}_{self.ds_stride}.{name.lower()[-3:]}'
            example = example if example in names else next(iter(names), None)
            would = f"it writes {len(names)} crops, such as {example}" if names else "it writes no crop of it"
            raise FileNotFoundError(f"{given}: not a crop the cropper writes for {fpath} ({width} x {height}) at crop size "
                                    f"{self.ds_cs}, stride {self.ds_stride}: {would}")
        xbeg, ybeg = names[fname]
        return fpath, ybeg, xbeg


def crop_source(crop_path, dsdirs, ds_cs, ds_stride, crops_dir=None):
    """Where the crop file crop_path lies in the full-size dataset: (path of the full-size image, ybeg, xbeg) of the ds_cs x ds_cs
    rectangle the reference's cropper (tools/crop_ds.py --cs ds_cs --stride ds_stride) would have written under that name, or None
    when the path is not a crop of this data.  Decided by the path's last four components <crops leaf>/<set>/<iso>/<file name>
    alone; what comes before them is ignored (lists hold paths relative to a working directory the user may not have), and no
    crop file is looked for.  <crops leaf> is the leaf of the cropped tree CropPool.from_full_size derives for one of dsdirs
    (<leaf of dsdir>_<ds_cs>_<ds_stride>, or the leaf of its crops_dir entry); the first dsdir that matches takes the path, and
    None is returned when none does.  From there on a mismatch is FileNotFoundError naming crop_path as given: a set the dsdir
    does not have, an ISO the set does not have (set_images), or a file name other than <stem>_<xcrop>_<ycrop>_<ds_stride>.<ext>
    with the stem and extension of that ISO's image and indices that crop_grid yields for its size; the message then names a
    crop the cropper does write for the image.  Sizes are read from the file header (imgcodec.image_size).
    For many paths make one CropSources and call its source()."""
    return CropSources(dsdirs, ds_cs, ds_stride, crops_dir).source(crop_path)


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
        self._images = []        # (byte offset, H, W, sample type) per image; in a pool of windows (byte offset of the frame, H, W,
        #                          sample type, y, x, frame H, frame W): the rows of the two table formats of nd_crop_batch
        self._frames = None      # a pool of windows: (byte offset, H, W, sample type) per frame; None: a pool of dense images
        self._image_frame = []   # a pool of windows: the frame of each image
        self.sets = []           # from_directories: (datadir, set, crop file, base ISOs, other ISOs) per group
        self.datadirs = None     # from_directories: the directories as given
        self.scores = None       # score_pairs: [pairs] fp32 on the device, in pair order
        self.pairs = None        # score_pairs / set_min_quality: [pairs, 3] int64 on the device (group, clean image, noisy image)
        self.min_quality = None
        self._bar = None         # set_min_quality: (passing pairs [P, 2], first [G], count [G], active groups [A]) on the device
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
        if self._frames is not None:
            raise ValueError("CropPool.add_group: this pool holds frames and windows (add_frame); a pool holds either dense images "
                             "or windows, not both")
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
        self._gt = self.scores = self.pairs = self.min_quality = self._bar = None
        return len(self._groups) - 1

    def add_frame(self, chw):
        """A whole image, stored once, for add_window_group to take windows from (HWC, CHW or HW samples).  Returns the frame's
        index.  A pool holds either dense images (add_group) or frames and windows, not both: ValueError."""
        if self._pool is not None:
            raise RuntimeError("CropPool: the pool was uploaded by its first batch; add every frame before that")
        if self._frames is None:
            if self._images:
                raise ValueError("CropPool.add_frame: this pool holds dense images (add_group); a pool holds either dense images or "
                                 "windows, not both")
            self._frames = []
        chw = _to_chw(chw)
        off = self._bytes
        self._staged.append((off, chw))
        self._frames.append((off, chw.shape[1], chw.shape[2], _TYPES[chw.dtype]))
        self._bytes = (off + chw.nbytes + _ALIGN - 1) // _ALIGN * _ALIGN
        return len(self._frames) - 1

    def add_window_group(self, clean_frames, noisy_frames, y, x, h, w):
        """A group whose images are rows [y, y + h) x columns [x, x + w) of each named frame (indices add_frame gave): what add_group
        makes of that rectangle cut out of each, without a second copy of its samples.  When the two lists are equal (a clean-clean
        entry) the images are shared.  ValueError unless the rectangle lies inside every frame.  Returns the group's index."""
        if self._pool is not None:
            raise RuntimeError("CropPool: the pool was uploaded by its first batch; add every group before that")
        if self._frames is None:
            raise ValueError("CropPool.add_window_group: the pool has no frame (add_frame first; a pool of dense images takes no windows)")
        clean_frames, noisy_frames = [int(f) for f in clean_frames], [int(f) for f in noisy_frames]
        if not clean_frames or not noisy_frames:
            raise ValueError("CropPool.add_window_group: a group needs at least one clean and one noisy frame")
        y, x, h, w = int(y), int(x), int(h), int(w)
        for f in clean_frames + noisy_frames:
            if not 0 <= f < len(self._frames):
                raise ValueError(f"CropPool.add_window_group: frame {f} outside [0, {len(self._frames)})")
            _, fh, fw, _ = self._frames[f]
            if h < 1 or w < 1 or y < 0 or x < 0 or y + h > fh or x + w > fw:
                raise ValueError(f"CropPool.add_window_group: the {h} x {w} window at ({y}, {x}) does not lie inside frame {f} "
                                 f"({fh} x {fw})")

        def add(frames):        # consecutive rows of the table, like the images of a dense group
            first = len(self._images)
            for f in frames:
                off, fh, fw, typ = self._frames[f]
                self._images.append((off, h, w, typ, y, x, fh, fw))
                self._image_frame.append(f)
            return first

        c0 = add(clean_frames)
        n0 = c0 if clean_frames == noisy_frames else add(noisy_frames)
        self._groups.append((c0, len(clean_frames), n0, len(noisy_frames), h, w))
        self._gt = self.scores = self.pairs = self.min_quality = self._bar = None
        return len(self._groups) - 1

    def _keep_window_groups(self, count):
        groups, staged = self._groups[:count], dict(self._staged)
        used = sorted({self._image_frame[i] for c0, nc, n0, nn, _, _ in groups for i0, cnt in ((c0, nc), (n0, nn))
                       for i in range(i0, i0 + cnt)})
        arrays = {f: staged[self._frames[f][0]] for f in used}
        old_images, old_frame = self._images, self._image_frame
        self._staged, self._images, self._image_frame, self._frames, self._groups, self._bytes = [], [], [], [], [], 0
        renumbered = {f: self.add_frame(arrays[f]) for f in used}             # the frames still named, in their old order
        for c0, nc, n0, nn, h, w in groups:
            _, _, _, _, y, x, _, _ = old_images[c0]
            self.add_window_group([renumbered[old_frame[i]] for i in range(c0, c0 + nc)],
                                  [renumbered[old_frame[i]] for i in range(n0, n0 + nn)], y, x, h, w)

    def keep_groups(self, count):
        """Drops every group past the first `count` (debug option short_run: DDataset.dataset[:3 * batch_size], nn_train.py:225-226),
        and with them the images, or in a pool of windows the frames, no remaining group names.  Only before the first upload."""
        if self._pool is not None:
            raise RuntimeError("CropPool: the pool was uploaded by its first batch; drop groups before that")
        if count < 0:
            raise ValueError(f"CropPool.keep_groups: count {count}")
        if count >= len(self._groups):
            return
        if self._frames is not None:
            self.sets = self.sets[:count]
            self._gt = self.scores = self.pairs = self.min_quality = self._bar = None
            return self._keep_window_groups(count)
        groups, staged = self._groups[:count], dict(self._staged)
        arrays = [staged[off] for off, _, _, _ in self._images]
        self.sets = self.sets[:count]
        self._staged, self._images, self._groups, self._bytes, self._gt = [], [], [], 0, None
        self.scores = self.pairs = self.min_quality = self._bar = None
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
        pool.datadirs = [os.fspath(d) for d in datadirs]

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

    @classmethod
    def from_full_size(cls, dsdirs, ds_cs=256, ds_stride=192, test_reserve=(), exact_reserve=False, device=None, seed=0, cs=None,
                       crops_dir=None):
        """The pool from_directories would make of the tree the reference's cropper (tools/crop_ds.py --cs ds_cs --stride ds_stride,
        which runs tools/crop_img.sh on every image) writes for the full-size dataset <dsdir>/<set>/<image files>, without that
        tree: every image of a set that is not reserved is read once and uploaded once as a frame, and every crop is a window into
        its frame.  Groups and their order, sets, pair_paths() and dsname are those of the cropped tree at crops_dir (default: the
        cropper's own <root of dsdir>/cropped/<leaf of dsdir>_<ds_cs>_<ds_stride>; one path per dsdir): sets in sorted order, the ISO
        of a file as the cropper finds it (findisoval), base and other ISOs by sortISOs, one group per crop file name of the first
        noisy ISO in sorted file-name order, <basename>_<xcrop>_<ycrop>_<ds_stride>.<ext> (crop_grid), the crop of another ISO
        named by the same replacement of the ISO in that name.  When an ISO's own image size does not yield that crop,
        FileNotFoundError names the crop file that would be missing, as from_directories raises it on the cropped tree.  A set
        whose images yield no crop contributes nothing.  cs defaults to ds_cs.

        Where this differs from the cropper.  A second file of a set with an ISO value already seen is the ISO <iso>-2, a third
        <iso>-2-2, in sorted file order, and its crops are named as if the file had been renamed so; the cropper renames the user's
        files on disk, in directory order.  This pool renames nothing.  JPEG sources are decoded like any other file: equality with a
        jpegtran-cropped tree is not claimed, since a decoder upsamples chroma differently at the border of a crop file than inside
        the whole image.  For PNG and TIFF a crop file is a rectangle of its image, and the pools are equal bit for bit."""
        dsdirs, crops_dirs = crops_dirs_of(dsdirs, ds_cs, ds_stride, crops_dir)
        crop_grid(0, 0, ds_cs, ds_stride)         # refuses the sizes the script refuses, before any file is read
        pool = cls(device, seed=seed, cs=int(ds_cs) if cs is None else cs)
        pool.datadirs = crops_dirs
        pool._frames = []

        def reserved(aset):
            if exact_reserve:
                return aset in test_reserve
            return any(s in aset for s in test_reserve)

        for dsdir, datadir in zip(dsdirs, crops_dirs):
            for aset in sorted(os.listdir(dsdir)):
                if reserved(aset):
                    continue
                files = set_images(os.path.join(dsdir, aset))
                if not files:
                    continue
                bisos, isos = sortISOs(sorted(files))
                if not isos:
                    raise ValueError(f"CropPool.from_full_size: {os.path.join(dsdir, aset)} has no noisy ISO image")
                samples, crops = {}, {}           # ISO -> its image; ISO -> {crop file name: (xbeg, ybeg)}
                for iso in bisos + isos:
                    fpath, name = files[iso]
                    try:
                        samples[iso] = np_imgops.img_path_to_np_samples(fpath)
                    except FileNotFoundError:
                        raise
                    except Exception as e:
                        raise ValueError(f"CropPool.from_full_size: cannot read {fpath}: {e}") from e
                    _, h, w = samples[iso].shape
                    crops[iso] = crop_names(name, w, h, ds_cs, ds_stride)
                if not crops[isos[0]]:
                    continue
                frames = {iso: pool.add_frame(samples[iso]) for iso in bisos + isos}
                del samples
                for animg in sorted(crops[isos[0]]):
                    xb, yb = crops[isos[0]][animg]
                    for iso in isos + bisos:      # the order in which from_directories opens a group's files
                        theirs = animg.replace(isos[0] + '_', iso + '_')
                        if theirs not in crops[iso]:
                            raise FileNotFoundError(os.path.join(datadir, aset, iso, theirs))
                    pool.add_window_group([frames[iso] for iso in bisos], [frames[iso] for iso in isos], yb, xb, ds_cs, ds_cs)
                    pool.sets.append((datadir, aset, animg, tuple(bisos), tuple(isos)))
        return pool

    @property
    def nbytes(self):
        """Bytes of the pool buffer (images in their own sample type, each aligned to 16 bytes; in a pool of windows the frames,
        each counted once)."""
        return self._bytes

    @property
    def windowed(self):
        """True for a pool of frames and windows (add_frame / add_window_group, from_full_size)."""
        return self._frames is not None

    @property
    def n_frames(self):
        """Frames of a pool of windows; 0 for a pool of dense images."""
        return len(self._frames) if self._frames is not None else 0

    @property
    def n_groups(self):
        return len(self._groups)

    @property
    def n_active_groups(self):
        """Groups that draw() and epoch() take from: all of them, or with a quality bar those with a pair above it."""
        return self.n_groups if self._bar is None else int(self._bar[3].shape[0])

    @property
    def n_images(self):
        return len(self._images)

    def group(self, g):
        """(clean image indices, noisy image indices, H, W) of group g."""
        c0, nc, n0, nn, h, w = self._groups[g]
        return list(range(c0, c0 + nc)), list(range(n0, n0 + nn)), h, w

    def image(self, i):
        """Image i as the pool holds it: a [3, H, W] numpy array of its sample type (read back from the device once uploaded)."""
        off, h, w, typ = self._images[i][:4]
        dtype = [k for k, v in _TYPES.items() if v == typ][0]
        if self._frames is not None:        # a window: its samples, cut out of the frame
            _, _, _, _, y, x, fh, fw = self._images[i]
            if self._pool is None:
                frame = dict(self._staged)[off]
            else:
                frame = self._pool[off:off + 3 * fh * fw * dtype.itemsize].cpu().numpy().view(dtype).reshape(3, fh, fw)
            return np.ascontiguousarray(frame[:, y:y + h, x:x + w])
        if self._pool is None:
            return dict(self._staged)[off]
        raw = self._pool[off:off + 3 * h * w * dtype.itemsize].cpu().numpy()
        return raw.view(dtype).reshape(3, h, w)

    # ------------------------------------------------------------------ draws
    def seed(self, seed):
        self.generator.manual_seed(seed)

    def rng_state(self):
        """The state of the generator behind every draw, as a CPU byte tensor (torch.Generator.get_state): with it, and the same
        groups and quality bar, another pool makes this pool's next draws."""
        return self.generator.get_state().clone()

    def set_rng_state(self, state):
        self.generator.set_state(torch.as_tensor(state, dtype=torch.uint8, device="cpu").contiguous())

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

        if self._bar is None:
            clean = gt[:, 0] + pick(0, gt[:, 1])                           # get_x_y_paths: two independent choices
            noisy = gt[:, 2] + pick(1, gt[:, 3])
        else:                                                              # one choice among the group's pairs above the bar
            passing, first, count, _ = self._bar
            pair = passing[first[groups] + pick(0, count[groups])]
            clean, noisy = pair[:, 0], pair[:, 1]
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
        if self._bar is not None:
            active = self._bar[3]
            return self._draw_groups(active[torch.randint(0, active.shape[0], (batch_size,), device=self.device,
                                                          generator=self.generator)], cs)
        groups = torch.randint(0, self.n_groups, (batch_size,), device=self.device, generator=self.generator)
        return self._draw_groups(groups, cs)

    def epoch(self, batch_size, cs=None, rank=0, world=1):
        """One pass over the groups in a random order, in full batches (DataLoader(shuffle=True, drop_last=True)).  With world > 1
        every rank must hold a pool with the same groups and generator state: batch k of the single-rank epoch goes to rank
        k % world, each rank gets the same number of batches (the last len(epoch) % world batches are dropped), and the generator
        advances alike on all ranks.  With a quality bar the pass is over the active groups, and so are the counts above."""
        cs = self._cs(cs)
        self._group_table()
        if batch_size < 1 or world < 1 or not 0 <= rank < world:
            raise ValueError(f"CropPool.epoch: batch_size {batch_size}, rank {rank}, world {world}")
        if self._bar is None:
            perm = torch.randperm(self.n_groups, device=self.device, generator=self.generator)
        else:
            perm = self._bar[3][torch.randperm(self.n_active_groups, device=self.device, generator=self.generator)]
        steps = perm.shape[0] // batch_size // world
        for k in range(steps * world):
            draws = self._draw_groups(perm[k * batch_size:(k + 1) * batch_size], cs)
            if k % world == rank:
                yield draws

    # ------------------------------------------------------------------ quality
    def pair_table(self):
        """[pairs, 3] int64 numpy rows (group, clean image, noisy image) in the order of get_all_crop_pairs_of_paths
        (dataset_torch_3.py:203-213): groups in pool order, base ISOs outer, other ISOs inner."""
        rows = [(g, c0 + i, n0 + j) for g, (c0, nc, n0, nn, _, _) in enumerate(self._groups) for i in range(nc) for j in range(nn)]
        return np.asarray(rows, dtype=np.int64).reshape(-1, 3)

    def _pairs_on_device(self):
        if self.pairs is None:
            if not self._groups:
                raise ValueError("CropPool: the pool has no group")
            self.pairs = torch.from_numpy(self.pair_table()).to(self.device)
        return self.pairs

    def score_pairs(self, batch_size=64):
        """MS-SSIM (piqa's MS_SSIM(): the similarity, not 1 - it) of every (clean image, noisy image) pair of every group, on the
        files as stored: a [pairs] float32 tensor on the device in the order of pair_table(), kept as self.scores beside
        self.pairs.  Pairs are taken by size (H, W), batch_size at a time: nd_pool_fetch makes the two fp32 batches, nd_ms_ssim
        scores each sample on its own, so no score depends on batch_size.  A pair with a side below 161 gets NaN.  Nothing here waits
        for the GPU."""
        if batch_size < 1 or batch_size > 10922:      # nd_ms_ssim takes 32767 image planes at most
            raise ValueError(f"CropPool.score_pairs: batch_size {batch_size} outside [1, 10922]")
        table = self.pair_table()
        if not len(table):
            raise ValueError("CropPool: the pool has no group")
        pool, images = self._upload()
        sizes = np.asarray([(g[4], g[5]) for g in self._groups], dtype=np.int64)[table[:, 0]]
        order = np.lexsort((np.arange(len(table)), sizes[:, 1], sizes[:, 0]))        # by size, pair order inside a size
        # one upload: the pairs in scoring order, as the kernel's index type, and where each goes in pair order
        up = torch.from_numpy(np.ascontiguousarray(np.stack((table[order, 1], table[order, 2], order)))).to(self.device)
        by_size, place = up[:2].to(torch.int32).contiguous(), up[2]
        assert by_size.stride() == (len(table), 1)                         # rows of the kernel's index type, sliced below
        scored = torch.full((len(table),), float("nan"), dtype=torch.float32, device=self.device)
        lib = _lib.load()
        fetch_name = "nd_pool_fetch" if self._frames is None else "nd_pool_fetch_windows"
        fetch = getattr(lib, fetch_name)
        sorted_sizes = sizes[order]
        bounds = np.flatnonzero((np.diff(sorted_sizes, axis=0) != 0).any(axis=1)) + 1
        with torch.cuda.device(self.device):
            stream = _lib.stream_ptr(self.device)
            for a, b in zip(np.concatenate(([0], bounds)), np.concatenate((bounds, [len(table)]))):
                h, w = (int(v) for v in sorted_sizes[a])
                if min(h, w) < MS_SSIM_MIN_SIDE:
                    continue
                n = int(min(batch_size, b - a))
                x = torch.empty(2, n, 3, h, w, dtype=torch.float32, device=self.device)
                wsb = lib.nd_ssim_workspace_bytes(n, 3, h, w)
                ws = torch.empty(max(wsb, 4096), dtype=torch.uint8, device=self.device)
                for k in range(int(a), int(b), n):
                    m = int(min(n, b - k))
                    for side in (0, 1):
                        _lib.check(fetch(pool.data_ptr(), pool.numel(), images.data_ptr(), images.shape[0],
                                         by_size[side, k:k + m].data_ptr(), m, h, w, x[side].data_ptr(), stream), fetch_name)
                    _lib.check(lib.nd_ms_ssim(x[0].data_ptr(), x[1].data_ptr(), m, 3, h, w, scored[k:k + m].data_ptr(), ws.data_ptr(),
                                              ws.numel(), stream), "nd_ms_ssim")
        scores = torch.empty_like(scored)
        scores[place] = scored
        self.scores = scores
        self._pairs_on_device()
        return scores

    def pair_paths(self):
        """(xpath, ypath) of every pair in pair order, formed as get_all_crop_pairs_of_paths forms them (dataset_torch_3.py:191,
        211-212).  Only for a pool made by from_directories or from_full_size (there: the files of the cropped tree)."""
        if self.datadirs is None or len(self.sets) != len(self._groups):
            raise ValueError("CropPool: file paths are known only for a pool made by from_directories or from_full_size")
        paths = []
        for datadir, aset, animg, bisos, isos in self.sets:
            base = os.path.join(datadir, aset, 'ISOBASE', animg).replace(isos[0] + '_', 'ISOBASE_')
            for biso in bisos:
                for iso in isos:
                    paths.append(tuple(base.replace('ISOBASE_', v + '_').replace('/ISOBASE/', '/' + v + '/') for v in (biso, iso)))
        return paths

    @property
    def dsname(self):
        if self.datadirs is None:
            raise ValueError("CropPool: a dataset name is known only for a pool made by from_directories or from_full_size")
        return '+'.join(utilities.get_leaf(path) for path in self.datadirs)

    def list_content_quality(self, export=False, out_dir='datasets'):
        """(xpath, ypath, score) of every pair, in pair order (DenoisingDataset.list_content_quality, dataset_torch_3.py:215-229);
        the score is a float, NaN where score_pairs gives NaN.  Scores the pool first unless it holds scores.  export: writes
        <out_dir>/<dsname>-msssim.csv with the header xpath,ypath,score; a score is written as repr(float), NaN as an empty field.
        The one read of the scores is the only wait for the GPU."""
        paths = self.pair_paths()
        scores = (self.scores if self.scores is not None else self.score_pairs()).cpu().tolist()
        rows = [(x, y, s) for (x, y), s in zip(paths, scores)]
        if export:
            os.makedirs(out_dir, exist_ok=True)
            outpath = os.path.join(out_dir, self.dsname + '-msssim.csv')
            utilities.list_of_tuples_to_csv([(x, y, '' if math.isnan(s) else repr(s)) for x, y, s in rows],
                                            ('xpath', 'ypath', 'score'), outpath)
            print(f'Quality check exported to {outpath}')
        return rows

    def _scores_from_csv(self, fpath):
        paths = self.pair_paths()
        with open(fpath, 'r', newline='') as fp:
            rows = [(r['xpath'], r['ypath'], r['score']) for r in csv.DictReader(fp)]
        listed, mine = {(x, y): s for x, y, s in rows}, set(paths)
        missing = next((p for p in paths if p not in listed), None)
        extra = next(((x, y) for x, y, _ in rows if (x, y) not in mine), None)
        if missing is not None or extra is not None:
            said = []
            if missing is not None:
                said.append(f"the pool's pair {missing[0]}, {missing[1]} is missing from it")
            if extra is not None:
                said.append(f"it lists the pair {extra[0]}, {extra[1]}, which the pool does not hold")
            raise ValueError(f"CropPool.set_min_quality: {fpath} does not list this pool's pairs: " + "; ".join(said))
        return torch.tensor([float(listed[p]) if listed[p] != '' else float('nan') for p in paths], dtype=torch.float32)

    def set_min_quality(self, q, scores=None):
        """From now on draw() and epoch() take a group's (clean, noisy) pair uniformly among its pairs with score > q (strictly, as
        PickyDenoisingDatasetFromList writes it; NaN never passes), and leave out the groups that have none: n_active_groups says
        how many remain.  scores: a tensor in pair order, the path of a csv that list_content_quality wrote (ValueError unless it
        lists exactly this pool's pairs), or None for the pool's own scores (score_pairs() first if need be).  q None removes the
        bar, and draws are again what a pool without one makes.  Returns the number of pairs above the bar."""
        if q is None:
            self.min_quality = self._bar = None
            return None
        if scores is None:
            scores = self.scores if self.scores is not None else self.score_pairs()
        elif isinstance(scores, (str, os.PathLike)):
            scores = self._scores_from_csv(os.fspath(scores))
        pairs = self._pairs_on_device()
        scores = torch.as_tensor(scores, dtype=torch.float32).to(self.device).reshape(-1)
        if scores.shape[0] != pairs.shape[0]:
            raise ValueError(f"CropPool.set_min_quality: {scores.shape[0]} scores for {pairs.shape[0]} pairs")
        above = pairs[scores > float(q)]                                   # pair order: a group's pairs stay consecutive
        count = torch.bincount(above[:, 0], minlength=self.n_groups)
        first = torch.cumsum(count, 0) - count
        self._bar = (above[:, 1:].contiguous(), first, count, torch.nonzero(count).reshape(-1))
        self.min_quality = float(q)
        return int(above.shape[0])

    # ------------------------------------------------------------------ batches
    def device_buffers(self):
        """(pool bytes, image table) as nd_crop_batch takes them: a uint8 tensor and an int64 [images, 4] tensor on the device; the
        first call uploads them.  A pool of windows: the frames, and the [images, 8] table of nd_crop_batch_windows."""
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
        images = np.asarray(self._images, dtype=np.int64).reshape(len(self._images), -1)     # H, W in columns 1, 2 of both formats
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
            name = "nd_crop_batch" if self._frames is None else "nd_crop_batch_windows"
            _lib.check(getattr(_lib.load(), name)(
                pool.data_ptr(), pool.numel(), images.data_ptr(), images.shape[0], table.data_ptr(), n, cs, float(exp_mult_min),
                float(exp_mult_max), None if mult is None else mult.data_ptr(), None if xmax is None else xmax.data_ptr(),
                None if mout is None else mout.data_ptr(), clean.data_ptr(), noisy.data_ptr(), _lib.stream_ptr(self.device)),
                name)
        self.last_xmax, self.last_mult = xmax, mout
        return clean, noisy
