'''
pick validation set:
    should only be done once per test_dir for consistent results
    generates configs/validation_set_<NUM_CROPS>_<TRAIN_DATA>_<leaf of TEST_SET_YAML>

The reference's tools/pick_validation_set.py, with its options and the default config files it (and nn_train) reads: --num_crops
pairs [clean crop path, noisy crop path] drawn at random from the crops of the sets named by --test_reserve, written as the yaml
list nn_train --validation_set_yaml takes.  Candidates follow its loops: the sets whose name is in test_reserve (exact membership,
not the substring rule of the dataset), per set sortISOs, and for each base ISO, each noisy ISO and each crop of the base ISO the
pair [base crop, noisy crop], the noisy one named by crop_fn.replace(base_iso, noisy_iso).

egrun:
    python -m nind_denoise_amd.tools.pick_validation_set --train_data datasets/cropped/NIND_256_192 --test_reserve configs/test_set_nind.yaml
    python -m nind_denoise_amd.tools.pick_validation_set --full_size_data datasets/NIND --test_reserve configs/test_set_nind.yaml

--full_size_data DIR [--ds_cs 256 --ds_stride 192] (nn_train's options) needs no cropped dataset: the crop names are those the
cropper would write for the full-size images (crop_pool.set_images, crop_names), and the paths are <crops dir>/<set>/<iso>/<name>
with the crops dir CropPool.from_full_size derives: the strings --train_data <that crops dir> gives from the same working
directory.  A noisy crop that its own image's grid does not yield is left out, and their number is printed at the end.  The
reference asserts that every chosen crop is a file; that stays for --train_data alone.  No pixel is read.

Where this differs from the reference:
  - directory listings are sorted where it takes os.listdir order, so one seed picks one list on every file system;
  - --seed S draws from a private random.Random(S); without it the module-level random.sample is used, as there;
  - --out PATH names the result file; the default is the reference's name, which needs --test_reserve to be one yaml file.
'''
import argparse
import os
import random
import sys

import yaml

from .. import nn_common, nn_train
from ..common.libs import imgcodec, utilities
from ..crop_pool import crop_names, crops_dirs_of, set_images
from ..dataset_torch_3 import sortISOs


def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--train_data', nargs='*', help='Draw crops randomly from this training image directory')
    parser.add_argument('--num_crops', type=int, default=30)
    parser.add_argument('--test_reserve', nargs='*', help='Space separated list of image sets to be reserved for testing, or yaml file path containing a list. Required (here or in a config file)')
    parser.add_argument('--overwrite', action='store_true', help='Overwrite existing validation set?')
    nn_train.add_full_size_options(parser)
    parser.add_argument('--seed', type=int, help='Draw from a private random.Random(SEED) (default: the module-level random.sample)')
    parser.add_argument('--out', help='Result file (default: configs/validation_set_<num_crops>_<data names joined by +>_<leaf of the test_reserve yaml>)')
    return parser


def parse_args(argv=None):
    '''Precedence as nn_train.parse_args: argparse defaults, the two default config files of the working directory if they exist,
    the command line.  Keys of the files that are not options here are ignored, and so are unknown arguments (the reference
    parses with parse_known_args).'''
    argv = sys.argv[1:] if argv is None else list(argv)
    parser = build_parser()
    args, _ = parser.parse_known_args(argv)
    explicit = build_parser()
    for action in explicit._actions:
        action.default = argparse.SUPPRESS
    given = vars(explicit.parse_known_args(argv)[0])
    by_key = {opt.lstrip('-'): action for action in parser._actions for opt in action.option_strings}
    for path in (nn_common.COMMON_CONFIG_FPATH, nn_train.DEFAULT_CONFIG_FPATH):
        if not os.path.isfile(path):
            continue
        with open(path, 'r') as f:
            conf = yaml.safe_load(f) or {}
        for key, value in conf.items():
            action = by_key.get(key)
            if action is None or action.dest == 'help':
                continue
            try:
                setattr(args, action.dest, nn_train._convert(action, value))
            except (TypeError, ValueError) as e:
                parser.error(f'{path}: {key}: {e}')
    for dest, value in given.items():
        setattr(args, dest, value)
    if not args.test_reserve:
        parser.error('the following arguments are required: --test_reserve (on the command line or in a config file)')
    full, _, _ = nn_train.full_size_options(args, parser)
    if not args.train_data and not full:
        parser.error('the following arguments are required: --train_data or --full_size_data (on the command line or in a config file)')
    if args.out is None and not (len(args.test_reserve) == 1 and args.test_reserve[0].endswith('.yaml')):
        parser.error('the result file is named after the yaml file of --test_reserve: give one, or --out PATH')
    return args


def candidates_of_crops(train_data, test_reserve):
    '''[base crop path, noisy crop path] of every candidate pair of the cropped trees train_data, in the reference's loop order'''
    pairs = []
    for train_data_dpath in train_data:
        for set_name in sorted(os.listdir(train_data_dpath)):
            if set_name not in test_reserve:
                continue
            set_dpath = os.path.join(train_data_dpath, set_name)
            base_isos, isos = sortISOs(sorted(os.listdir(set_dpath)))
            for base_iso in base_isos:
                base_iso_dpath = os.path.join(set_dpath, base_iso)
                crops_filenames = sorted(os.listdir(base_iso_dpath))
                for noisy_iso in isos:
                    noisy_iso_dpath = os.path.join(set_dpath, noisy_iso)
                    for crop_fn in crops_filenames:
                        pairs.append([os.path.join(base_iso_dpath, crop_fn),
                                      os.path.join(noisy_iso_dpath, crop_fn.replace(base_iso, noisy_iso))])
    return pairs


def candidates_of_full_size(dsdirs, crops_dirs, ds_cs, ds_stride, test_reserve):
    '''(the pairs candidates_of_crops finds on the trees the cropper would write at crops_dirs for the full-size datasets dsdirs,
    the number of pairs left out because the noisy image's own grid does not yield the crop).  Sizes come from the file headers.'''
    pairs, skipped = [], 0
    for dsdir, crops_dir in zip(dsdirs, crops_dirs):
        for set_name in sorted(os.listdir(dsdir)):
            if set_name not in test_reserve:
                continue
            names = {}
            for iso, (fpath, name) in set_images(os.path.join(dsdir, set_name)).items():
                size = imgcodec.image_size(fpath)
                if size is None:
                    raise ValueError(f'pick_validation_set: cannot read the size of {fpath} from its header')
                names[iso] = crop_names(name, size[0], size[1], ds_cs, ds_stride)
            set_dpath = os.path.join(crops_dir, set_name)
            base_isos, isos = sortISOs(sorted(names))
            for base_iso in base_isos:
                crops_filenames = sorted(names[base_iso])
                for noisy_iso in isos:
                    for crop_fn in crops_filenames:
                        noisy_fn = crop_fn.replace(base_iso, noisy_iso)
                        if noisy_fn not in names[noisy_iso]:
                            skipped += 1
                            continue
                        pairs.append([os.path.join(set_dpath, base_iso, crop_fn), os.path.join(set_dpath, noisy_iso, noisy_fn)])
    return pairs, skipped


def main(argv=None):
    args = parse_args(argv)
    test_reserve_str = utilities.get_leaf(args.test_reserve[0])
    test_reserve = nn_train.get_test_reserve_list(args.test_reserve)
    full, ds_cs, ds_stride = nn_train.full_size_options(args)
    skipped = None
    if full:
        dsdirs, crops_dirs = crops_dirs_of(full, ds_cs, ds_stride)
        crops_paths, skipped = candidates_of_full_size(dsdirs, crops_dirs, ds_cs, ds_stride, test_reserve)
        data_dnames = [utilities.get_leaf(d) for d in crops_dirs]
    else:
        crops_paths = candidates_of_crops(args.train_data, test_reserve)
        data_dnames = [utilities.get_leaf(d) for d in args.train_data]
    res_fpath = args.out
    if res_fpath is None:
        res_fpath = os.path.join('configs', f'validation_set_{args.num_crops}_{"+".join(data_dnames)}_{test_reserve_str}')
    if os.path.isfile(res_fpath) and not args.overwrite:
        sys.exit(f'{res_fpath} exists and args.overwrite is not set')
    if len(crops_paths) < args.num_crops:
        raise ValueError(f'pick_validation_set: --num_crops {args.num_crops}, but the sets of test_reserve ({test_reserve}) hold '
                         f'{len(crops_paths)} candidate pairs')

    # randomly select crops
    sample = random.sample if args.seed is None else random.Random(args.seed).sample
    chosen_crops = sample(crops_paths, args.num_crops)

    # test that crops exist
    if not full:
        for acrop in chosen_crops:
            assert os.path.isfile(acrop[0]), acrop
            assert os.path.isfile(acrop[1]), acrop

    # write to yaml
    os.makedirs(os.path.dirname(os.path.abspath(res_fpath)), exist_ok=True)
    with open(res_fpath, 'w') as fp:
        yaml.dump(chosen_crops, fp)
    print(f'{chosen_crops=} written to {res_fpath=}')
    if skipped is not None:
        print(f'{skipped} candidate pair(s) left out: the noisy image\'s own grid does not yield the crop')
    return 0


if __name__ == '__main__':
    sys.exit(main())
