'''Loss utils used by denoise_dir: SSIM score and MSE loss of every image of a directory against its ground truth, as res.txt.

Interface of the reference's loss.py:14-53 (find_gt_path, files, gen_score, the command line), e.g.
    python -m nind_denoise_amd.loss --noisy_dir ../../results/NIND/test/<model> --gt_dir ../../datasets/test/NIND/ds_fs
The SSIM is the one the reference vendors (libs/pytorch_ssim, zero-padded window), the MSE is nd_mse; both run on the GPU
(no CPU fallback), where the reference scores on whatever device it finds.  Differences: files are visited in sorted order and
the ground-truth extension is that of the first file in sorted order (the reference follows os.listdir order, which the file
system decides); gen_score also returns its lines as a list of (name, ssim, mse).
'''
import argparse
import os

import numpy as np
import torch

from .common.libs import np_imgops, pt_helpers, pt_losses
from .dataset_torch_3 import sortISOs
from .libs import pytorch_ssim

DEFAULT_GT_DIR = '../../datasets/test/NIND/ds_fs'


def find_gt_path(denoised_fn, gt_dir):
    '''<dsname>_<set>_<ISO...>.<ext> -> path of the set's base-ISO image under gt_dir/<set>'''
    dsname, setdir = denoised_fn.split('_')[0:2]
    setfiles = sorted(os.listdir(os.path.join(gt_dir, setdir)))
    ext = setfiles[0].split('.')[-1]
    isos = [fn.split('_')[2][:-4] for fn in setfiles]
    baseiso = sortISOs(isos)[0][0]
    baseiso_fn = dsname + '_' + setdir + '_' + baseiso + '.' + ext
    return os.path.join(gt_dir, setdir, baseiso_fn)


def files(path):
    '''names of the regular files of a directory in sorted order, res.txt left out'''
    for fn in sorted(os.listdir(path)):
        if os.path.isfile(os.path.join(path, fn)) and fn != 'res.txt':
            yield fn


def read_image(path, device):
    '''[1,C,H,W] float32 on the device.  An 8-bit file is read as the reference reads every file (PIL, samples / 255, the
    file's own channels); any other depth goes through np_imgops (16-bit / 65535, float32 as stored), where PIL would keep only
    the high byte of a 16-bit PNG.'''
    raw = np_imgops._read_hwc(path)
    if raw.dtype == np.ubyte:
        from PIL import Image
        arr = np.asarray(Image.open(path))
        if arr.dtype == np.ubyte:
            if arr.ndim == 2:
                arr = arr[:, :, None]
            chw = np.ascontiguousarray(arr.transpose(2, 0, 1)).astype(np.float32) / np.float32(255)
            return torch.from_numpy(chw).to(device).unsqueeze(0)
    return torch.from_numpy(np_imgops.hwc_to_np_flt(raw, path)).to(device).unsqueeze(0)


def gen_score(noisy_dir, gt_dir=DEFAULT_GT_DIR, device=None):
    '''writes noisy_dir/res.txt with one "name,ssim,mse" line per image of noisy_dir; returns [(name, ssim, mse)]'''
    device = pt_helpers.get_device() if device is None else torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError('gen_score needs a GPU (no CPU fallback)')
    SSIM = pytorch_ssim.SSIM()
    results = []
    names = list(files(noisy_dir))
    with open(os.path.join(noisy_dir, 'res.txt'), 'w') as f:
        for noisy_img in names:
            gtimg = read_image(find_gt_path(noisy_img, gt_dir), device)
            noisyimg = read_image(os.path.join(noisy_dir, noisy_img), device)
            MSELoss = pt_losses.mse(gtimg, noisyimg).item()
            SSIMScore = SSIM(gtimg, noisyimg).item()
            res = noisy_img + ',' + str(SSIMScore) + ',' + str(MSELoss)
            print(res)
            f.write(res + '\n')
            results.append((noisy_img, SSIMScore, MSELoss))
    return results


if __name__ == '__main__':
    parser = argparse.ArgumentParser(description='Get SSIM score and MSE loss from test images')
    parser.add_argument('--noisy_dir', type=str, required=True, help='Noisy / denoised data directory')
    parser.add_argument('--gt_dir', type=str, default=DEFAULT_GT_DIR, help='Ground truths directory')
    args, _ = parser.parse_known_args()
    gen_score(args.noisy_dir, args.gt_dir)
