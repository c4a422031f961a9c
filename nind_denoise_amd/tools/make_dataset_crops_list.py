'''
List a dataset's crops under a csv file and list all ms-ssim values
Useful to train above a given quality threshold (nn_train --min_quality Q --quality_csv <the file>)

The reference's tools/make_dataset_crops_list.py on the device-resident crop pool: the options and the default config files are its
own (and nn_train's), the pairs are scored from HBM in batches (crop_pool.CropPool.score_pairs), and the file is
datasets/<dsname>-msssim.csv with the header xpath,ypath,score.

egrun:
    python -m nind_denoise_amd.tools.make_dataset_crops_list --train_data datasets/train/NIND_256_192 --test_reserve configs/test_set_nind.yaml
    python -m nind_denoise_amd.tools.make_dataset_crops_list --full_size_data datasets/NIND --test_reserve configs/test_set_nind.yaml

--full_size_data DIR [--ds_cs 256 --ds_stride 192] (nn_train's options) scores the crops the cropper would cut from the full-size
dataset, as windows into its images (CropPool.from_full_size): the csv is the one the cropped tree gives, paths and scores.
'''
import argparse
import os
import sys
import time

import torch
import yaml

from .. import nn_common, nn_train

OUT_DIR = 'datasets'


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('-c', '--config', help='(yaml) config file path')
    parser.add_argument('--test_reserve', nargs='*', help='Space separated list of image sets to be reserved for testing, or yaml file path containing a list. Set to "0" to use all available data. Required (here or in a config file)')
    parser.add_argument('--train_data', nargs='*', help='(space-separated) Path(s) to the pre-cropped training data')
    parser.add_argument('--cs', '--crop_size', type=int, help='Crop size fed to NN. default: no additional cropping')
    parser.add_argument('--min_crop_size', type=int, help='Minimum crop size. Dataset will be checked if this value is set.')
    parser.add_argument('--loss_cs', '--loss_crop_size', type=int, help='Center crop size used in loss function. default: use stride size from dataset directory name')
    parser.add_argument('--debug_options', '--debug', nargs='*', default=[], help=f'(space-separated) Debug options (available: {nn_train.DEBUG_OPTIONS})')
    nn_train.add_full_size_options(parser)
    return parser


def parse_args(argv=None):
    '''Precedence as nn_train.parse_args: argparse defaults, the two default config files of the working directory if they exist,
    -c/--config, the command line.  Keys of the files that are not options here are ignored, and so are unknown arguments
    (the reference parses with parse_known_args).'''
    argv = sys.argv[1:] if argv is None else list(argv)
    parser = build_parser()
    args, _ = parser.parse_known_args(argv)
    explicit = build_parser()
    for action in explicit._actions:
        action.default = argparse.SUPPRESS
    given = vars(explicit.parse_known_args(argv)[0])
    by_key = {opt.lstrip('-'): action for action in parser._actions for opt in action.option_strings}
    for path, required in ((nn_common.COMMON_CONFIG_FPATH, False), (nn_train.DEFAULT_CONFIG_FPATH, False), (args.config, True)):
        if path is None or (not required and not os.path.isfile(path)):
            continue
        with open(path, 'r') as f:
            conf = yaml.safe_load(f) or {}
        for key, value in conf.items():
            action = by_key.get(key)
            if action is None or action.dest in ('help', 'config'):
                continue
            try:
                setattr(args, action.dest, nn_train._convert(action, value))
            except (TypeError, ValueError) as e:
                parser.error(f'{path}: {key}: {e}')
    for dest, value in given.items():
        setattr(args, dest, value)
    if args.test_reserve is None:
        parser.error('the following arguments are required: --test_reserve (on the command line or in a config file)')
    full, _, _ = nn_train.full_size_options(args, parser)
    if not args.train_data and not full:
        parser.error('the following arguments are required: --train_data or --full_size_data (on the command line or in a config file)')
    return args


def main(argv=None):
    from ..crop_pool import CropPool
    args = parse_args(argv)
    unknown = set(args.debug_options) - set(nn_train.DEBUG_OPTIONS)
    if unknown:
        raise ValueError(f'unknown debug options {sorted(unknown)} (available: {nn_train.DEBUG_OPTIONS})')
    if not torch.cuda.is_available():
        raise RuntimeError('make_dataset_crops_list: no GPU visible; nind_denoise_amd has no CPU fallback')
    if not args.min_crop_size and 'check_dataset' in args.debug_options:
        args.min_crop_size = args.cs
    full, ds_cs, ds_stride = nn_train.full_size_options(args)
    if full:
        pool = CropPool.from_full_size(full, ds_cs=ds_cs, ds_stride=ds_stride, cs=args.cs, device=nn_common.default_device(),
                                       test_reserve=nn_train.get_test_reserve_list(args.test_reserve))
    else:
        pool = CropPool.from_directories(args.train_data, test_reserve=nn_train.get_test_reserve_list(args.test_reserve),
                                         min_crop_size=args.min_crop_size or None, cs=args.cs, device=nn_common.default_device())
    pool.device_buffers()
    torch.cuda.synchronize(pool.device)
    start = time.perf_counter()
    scores = pool.score_pairs()
    unscored = int(torch.isnan(scores).sum())       # the read that waits for the pass
    seconds = time.perf_counter() - start
    print(f'{scores.shape[0]} pairs of {pool.n_groups} groups scored in {seconds:.3f} s '
          f'({scores.shape[0] / max(seconds, 1e-9):.0f} pairs/s); {unscored} left unscored (a side below 161 pixels)')
    pool.list_content_quality(export=True, out_dir=OUT_DIR)     # prints 'Quality check exported to <path>'
    return 0


if __name__ == '__main__':
    sys.exit(main())
