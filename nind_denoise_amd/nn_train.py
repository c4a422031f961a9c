'''
Train a denoising UtNet with the NIND (or any dataset of clean-noisy crops) -- MI355X native.

The generator-only reading of the reference's training script (nn_train.py:118-448): option names, defaults, the order of
events of an epoch, the files of a run directory (train.log, config.yaml, trainres.json, generator_<epoch>.pt) and the
learning-rate rule are the reference's; the data side is a device-resident crop pool (crop_pool.CropPool), the update is the
fused HIP step (train.UtNetTrainer) and validation runs in batches from HBM (validation.validate).

egrun:
    python -m nind_denoise_amd.nn_train --config configs/train_conf_utnet_std.yaml --debug_options short_run --epochs 6
then
    python -m nind_denoise_amd.nn_train --config configs/train_conf_utnet_std.yaml
data parallel, one process per GPU (this process starts the ranks and stays off the GPU; or start them with torchrun):
    python -m nind_denoise_amd.nn_train --config configs/train_conf_utnet_std.yaml --gpus 8

Not built, and refused by name: discriminators (--weight_D1 / --weight_D2 and the options that need them), generators other than
UtNet, the CPU whole-image test pass (--test_interval) and clean-clean mixing (--clean_data_ratio).

Quality bar (the cure README.md:140 of the reference names for an unstable start, PickyDenoisingDatasetFromList): --min_quality Q
trains on the pairs whose MS-SSIM is above Q, for the first --min_quality_epochs epochs or for the whole run; the scores are
computed from the resident pool at start, or read from the csv of tools.make_dataset_crops_list with --quality_csv.

Without the pre-cropped dataset: --full_size_data DIR [--ds_cs 256 --ds_stride 192] stands in for --train_data.  The pool holds the
full-size images and takes the cropper's crops as windows into them (CropPool.from_full_size), and the pairs of
--validation_set_yaml are cut out of the full-size images of the reserved sets in the same way (ValidationSet.from_full_size): a
path of the list that names a crop of DIR (crop_pool.crop_source: by its last four components, never by what exists on disk) is a
window, any other pair is read from disk.  tools.pick_validation_set --full_size_data writes such a list.  For PNG and TIFF sources
the run is the run on the cropped tree, byte for byte; JPEG sources are decoded whole, and that equality is not claimed for them.

Long runs: --g_clip_norm X clips the gradient by its global norm and --skip_nonfinite_steps leaves a step with a non-finite
gradient unapplied, both decided on the device (train._GuardedStep); --max_skipped_steps N ends a run that keeps skipping.
--save_state writes train_state.pt after every epoch and --resume RUN_DIR continues that run to the bits the uninterrupted run
would have left (--g_model_path + --start_epoch starts a new optimisation from old weights: "cosmetics", as the reference says).
'''
import argparse
import collections
import datetime
import hashlib
import os
import shutil
import signal
import socket
import subprocess
import sys
import time

import torch
import yaml

from . import nn_common
from .common.libs import json_saver

DEFAULT_CONFIG_FPATH = os.path.join('configs', 'train_conf_defaults.yaml')
DEBUG_OPTIONS = ('short_run', 'check_dataset', 'output_val_images', 'output_test_images', 'keep_all_output_images')
MAX_GPUS = 16         # --gpus: one process per rank, and no more than 16 processes may hold a GPU open at a time
KILL_GRACE_S = 10     # launch(): seconds between SIGTERM and SIGKILL for the ranks that outlive a failed one
STATE_FNAME = 'train_state.pt'      # --save_state / --resume: the latest epoch's training state, in the run directory
STATE_FORMAT = 1
RESUME_OVERRIDES = ('epochs', 'time_limit', 'min_lr', 'log_interval')      # what the command line may set next to --resume


class Printer:
    '''print, and append to a file (nn_common.py:364-378).  prefix: put before every line on stdout (a rank's name); flush: every
    line leaves at once and whole (ranks share one stdout)'''
    def __init__(self, tostdout=True, tofile=True, file_path='log', prefix='', flush=False):
        self.tostdout, self.tofile, self.file_path, self.prefix, self.flush = tostdout, tofile, file_path, prefix, flush

    def print(self, msg):
        if self.tostdout:
            print(self.prefix + str(msg) if self.prefix else msg, flush=self.flush)
        if self.tofile:
            try:
                with open(self.file_path, 'a') as f:
                    f.write(str(msg) + '\n')
            except Exception as e:
                print('Warning: could not write to log: %s' % e)


def get_test_reserve_list(test_reserve):
    '''test_reserve argument (a list, ["0"] for none, or [yaml path]) -> list of set names (nn_common.py:149-160)'''
    if test_reserve is not None and len(test_reserve) == 1:
        if test_reserve[0].endswith('.yaml'):
            with open(test_reserve[0], 'r') as fp:
                return yaml.safe_load(fp)
        elif test_reserve[0] == '0':
            return []
    return test_reserve


# ------------------------------------------------------------------ command line
def build_parser():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('-c', '--config', help='(yaml) config file path')
    parser.add_argument('-c2', '--config2', help='extra (yaml) config file path')
    parser.add_argument('--batch_size', type=int, help='Training batch size')
    parser.add_argument('--time_limit', type=int, help='Time limit in seconds (ends training)')
    parser.add_argument('--g_activation', type=str, default='PReLU', help='Final activation function for generator')
    parser.add_argument('--g_funit', type=int, default=32, help='Filter unit size for generator')
    parser.add_argument('--g_model_path', help='Generator pretrained model path (.pt state dict, or a run directory: its best epoch)')
    parser.add_argument('--models_dpath', help='Directory where all models are saved')
    parser.add_argument('--beta1', type=float, help='beta1 for adam')
    parser.add_argument('--g_lr', type=float, help='Initial learning rate for adam (generator)')
    parser.add_argument('--weight_SSIM', type=float, help='Weight on SSIM term in objective')
    parser.add_argument('--weight_MSSSIM', type=float, help='Weight on MSSSIM term in objective')
    parser.add_argument('--weight_L1', type=float, help='Weight on L1 term in objective')
    parser.add_argument('--weight_MSE', type=float, help='Weight on MSE term in objective')
    parser.add_argument('--test_reserve', nargs='*', help='Space separated list of image sets to be reserved for testing, or yaml file path containing a list. Set to "0" to use all available data. Required (here or in a config file)')
    parser.add_argument('--train_data', nargs='*', help='(space-separated) Path(s) to the pre-cropped training data')
    parser.add_argument('--cs', '--crop_size', type=int, help='Crop size fed to NN. default: no additional cropping')
    parser.add_argument('--min_crop_size', type=int, help='Minimum crop size. Dataset will be checked if this value is set.')
    parser.add_argument('--loss_cs', '--loss_crop_size', type=int, help='Center crop size used in loss function. default: use stride size from dataset directory name')
    parser.add_argument('--debug_options', '--debug', nargs='*', default=[], help=f'(space-separated) Debug options (available: {DEBUG_OPTIONS})')
    parser.add_argument('--g_network', type=str, help='Generator network (UtNet)')
    parser.add_argument('--threads', type=int, default=6, help='Accepted for the reference\'s config files; the crop pool has no loader threads')
    parser.add_argument('--min_lr', type=float, help='Minimum learning rate (ends training)')
    parser.add_argument('--epochs', type=int, default=9001, help='Number of epochs (ends training)')
    parser.add_argument('--compute_SSIM_anyway', action='store_true', help='Compute and display SSIM loss even if not used')
    parser.add_argument('--freeze_generator', action='store_true', help='Freeze generator until discriminator is useful (refused: no discriminator)')
    parser.add_argument('--start_epoch', default=1, type=int, help='Starting epoch (cosmetics)')
    parser.add_argument('--patience', type=int, help='Number of epochs without improvements before the learning rate is updated')
    parser.add_argument('--reduce_lr_factor', type=float, help='LR is multiplied by this factor when model performs poorly for <patience> epochs')
    parser.add_argument('--validation_interval', default=1, type=int, help='Validation interval in # of epochs. Affects learning rate update and helps to keep the best model in the end. 0 = no validation, default=1')
    parser.add_argument('--test_interval', default=0, type=int, help='Refused when > 0: the CPU whole-image test pass is not built (use denoise_dir on a checkpoint)')
    parser.add_argument('--orig_data', help='Location of the originally downloaded train data (before cropping); used when test_interval is set')
    parser.add_argument('--validation_set_yaml', help='Yaml file containing a list of clean/noisy images used for validation.')
    parser.add_argument('--exp_mult_min', type=float, help='Minimum exposure multiplicator (data augmentation)')
    parser.add_argument('--exp_mult_max', type=float, help='Maximum exposure multiplicator (data augmentation)')
    parser.add_argument('--clean_data_dpath', help='Location of the high quality (pre-cropped) clean data which can be used in training')
    parser.add_argument('--clean_data_ratio', type=float, help='Refused when > 0: ratio of clean-clean to clean-noisy training data')
    # discriminator options: parsed so that the reference's command lines and config files load, refused when they ask for one
    parser.add_argument('--d_activation', type=str, default='PReLU')
    parser.add_argument('--d2_activation', type=str, default='PReLU')
    parser.add_argument('--d_funit', type=int, default=32)
    parser.add_argument('--d2_funit', type=int, default=32)
    parser.add_argument('--d_model_path')
    parser.add_argument('--d2_model_path')
    parser.add_argument('--d_loss_function', type=str, default='MSE')
    parser.add_argument('--d2_loss_function', type=str, default='MSE')
    parser.add_argument('--d_lr', type=float)
    parser.add_argument('--d2_lr', type=float)
    parser.add_argument('--weight_D1', type=float, help='Refused when > 0')
    parser.add_argument('--weight_D2', type=float, help='Refused when > 0')
    parser.add_argument('--d_network', type=str)
    parser.add_argument('--d2_network', type=str)
    parser.add_argument('--not_conditional', action='store_true')
    parser.add_argument('--not_conditional_2', action='store_true')
    parser.add_argument('--discriminator_advantage', type=float, default=0.0)
    parser.add_argument('--discriminator2_advantage', type=float, default=0.0)
    # additions
    parser.add_argument('--seed', type=int, default=0, help='Seed of the crop pool\'s draws and of torch\'s generator')
    parser.add_argument('--expname', help='Name of the run directory under models_dpath (default: date and command line)')
    parser.add_argument('--log_interval', type=int, default=50, help='Print an iteration line every N steps (0: never)')
    parser.add_argument('--val_batch_size', type=int, default=32, help='Validation pairs per launch of the network')
    parser.add_argument('--min_quality', type=float, help='Train only on clean-noisy pairs whose MS-SSIM is above this (strictly); groups without such a pair are left out')
    parser.add_argument('--min_quality_epochs', type=int, default=0, help='--min_quality holds for the first N epochs of the run, counted from --start_epoch (0: every epoch)')
    parser.add_argument('--quality_csv', help='Take the pair scores from this csv (python -m nind_denoise_amd.tools.make_dataset_crops_list) instead of scoring the pool at start')
    parser.add_argument('--gpus', type=int, help=f'Data-parallel ranks, one process per GPU (1..{MAX_GPUS}; default 1: this process trains). Each rank takes --batch_size crops per step')
    parser.add_argument('--dist_backend', choices=('nccl', 'gloo'), help='Backend of the process group (default: nccl when every rank has a GPU of its own, else gloo: ranks share GPUs and gradients are staged through the host)')
    parser.add_argument('--g_clip_norm', type=float, help='Clip the generator\'s gradient to this global L2 norm (torch.nn.utils.clip_grad_norm_) before every update')
    parser.add_argument('--skip_nonfinite_steps', action='store_true', help='Do not apply an update whose gradient holds a NaN or an infinity; its loss is left out of the epoch\'s means')
    parser.add_argument('--max_skipped_steps', type=int, help='End the run with an error after an epoch with more skipped steps than this (needs --skip_nonfinite_steps)')
    add_full_size_options(parser)
    parser.add_argument('--save_state', action='store_true', help=f'Write {STATE_FNAME} (parameters, optimizer, learning-rate rule, pool generator) into the run directory after every epoch, for --resume')
    parser.add_argument('--resume', metavar='RUN_DIR', help=f'Continue the run of this directory from its {STATE_FNAME}: options come from its config.yaml; only {", ".join("--" + n for n in RESUME_OVERRIDES)} may be given with it')
    return parser


DS_CS, DS_STRIDE = 256, 192     # the cropper's defaults (tools/crop_ds.py:15-16)


def add_full_size_options(parser):
    '''--full_size_data, --ds_cs, --ds_stride (also of tools.make_dataset_crops_list).  They leave no attribute when they are not
    given, so the result of a command line without them is what it was before they existed: read them with full_size_options.'''
    parser.add_argument('--full_size_data', nargs='+', metavar='DIR', default=argparse.SUPPRESS,
                        help='(space-separated) Path(s) to the full-size dataset (<DIR>/<set>/<image files>), instead of --train_data: '
                             'its images are held whole in HBM and the crops of the cropper (tools/crop_ds.py) are windows into them')
    parser.add_argument('--ds_cs', type=int, default=argparse.SUPPRESS, help=f'Crop size of the cropper with --full_size_data (default: {DS_CS})')
    parser.add_argument('--ds_stride', type=int, default=argparse.SUPPRESS, help=f'Stride (useful crop size) of the cropper with --full_size_data (default: {DS_STRIDE})')


def full_size_options(args, parser=None):
    '''(full_size_data or None, ds_cs, ds_stride) of parsed options.  Refuses --train_data beside --full_size_data: through the
    parser if there is one, else with ValueError.  Without --full_size_data the other two are inert.'''
    full = getattr(args, 'full_size_data', None) or None
    if full and args.train_data:
        msg = '--train_data and --full_size_data are both given: the pool holds either the pre-cropped files or the full-size images'
        if parser is not None:
            parser.error(msg)
        raise ValueError(msg)
    ds_cs, ds_stride = getattr(args, 'ds_cs', None), getattr(args, 'ds_stride', None)
    return full, DS_CS if ds_cs is None else ds_cs, DS_STRIDE if ds_stride is None else ds_stride


def _convert(action, value):
    '''a yaml value as the option would have parsed it: nargs options take lists, typed options their type'''
    if isinstance(action, (argparse._StoreTrueAction, argparse._StoreFalseAction)):
        return bool(value)
    conv = (lambda v: v) if action.type is None or value is None else (lambda v: v if v is None else action.type(v))
    if action.nargs in ('*', '+'):
        if value is None:
            return None
        return [conv(v) for v in (value if isinstance(value, (list, tuple)) else [value])]
    return conv(value)


def parse_args(argv=None):
    '''Precedence, lowest first: argparse defaults, configs/common_conf_default.yaml, configs/train_conf_defaults.yaml (both
    relative to the working directory, if they exist), -c/--config, -c2/--config2, the command line.  Yaml keys are option names
    without their dashes (any alias); unknown keys are ignored.'''
    argv = sys.argv[1:] if argv is None else list(argv)
    parser = build_parser()
    args = parser.parse_args(argv)
    explicit = build_parser()
    for action in explicit._actions:
        action.default = argparse.SUPPRESS
    given = vars(explicit.parse_args(argv))
    if given.get('resume') is not None:
        return resume_args(parser, args, given)
    by_key = {}
    for action in parser._actions:
        for opt in action.option_strings:
            by_key[opt.lstrip('-')] = action
    for path, required in ((nn_common.COMMON_CONFIG_FPATH, False), (DEFAULT_CONFIG_FPATH, False), (args.config, True),
                           (args.config2, True)):
        if path is None or (not required and not os.path.isfile(path)):
            continue
        with open(path, 'r') as f:
            conf = yaml.safe_load(f) or {}
        for key, value in conf.items():
            action = by_key.get(key)
            if action is None or action.dest in ('help', 'config', 'config2'):
                continue
            try:
                setattr(args, action.dest, _convert(action, value))
            except (TypeError, ValueError) as e:
                parser.error(f'{path}: {key}: {e}')
    for dest, value in given.items():
        setattr(args, dest, value)
    if args.test_reserve is None:
        parser.error('the following arguments are required: --test_reserve (on the command line or in a config file)')
    full, _, ds_stride = full_size_options(args, parser)
    if full and args.loss_cs is None:       # the <UCS> of the directory the cropper would have made (nn_train.py:220-222)
        args.loss_cs = ds_stride
    return args


def resume_args(parser, defaults, given):
    '''The options of --resume RUN_DIR: those RUN_DIR/config.yaml recorded (options the file does not know keep their defaults),
    with RESUME_OVERRIDES from the command line.  ValueError naming any other option given beside --resume.  test_reserve comes
    back as the list the first run expanded it to, and start_epoch as that run's: --min_quality_epochs counts from it.'''
    for dest in given:
        if dest != 'resume' and dest not in RESUME_OVERRIDES:
            raise ValueError(f'--{dest} cannot be given with --resume: the options come from the run\'s config.yaml (only '
                             f'{", ".join("--" + n for n in RESUME_OVERRIDES)} may be set)')
    run_dir = os.path.normpath(given['resume'])
    conf_path = os.path.join(run_dir, 'config.yaml')
    if not os.path.isfile(conf_path):
        raise ValueError(f'--resume {given["resume"]}: {conf_path} not found (not a run directory?)')
    with open(conf_path, 'r') as f:
        conf = yaml.safe_load(f) or {}
    args = argparse.Namespace(**vars(defaults))
    for dest, value in conf.items():
        setattr(args, dest, value)
    for dest, value in given.items():
        setattr(args, dest, value)
    args.resume = run_dir
    args.save_state = True
    return args


def check_supported(args):
    '''NotImplementedError naming the first option that asks for something that is not built'''
    if args.g_network is not None and args.g_network != 'UtNet':
        raise NotImplementedError(f'--g_network {args.g_network}: only UtNet trains on the HIP path')
    for name in ('weight_D1', 'weight_D2'):
        if (getattr(args, name) or 0) > 0:
            raise NotImplementedError(f'--{name} > 0: discriminators are not built (generator losses: L1, MSE, SSIM, MSSSIM)')
    for name in ('d_model_path', 'd2_model_path', 'd_network', 'd2_network', 'freeze_generator', 'not_conditional',
                 'not_conditional_2', 'discriminator_advantage', 'discriminator2_advantage'):
        if getattr(args, name):
            raise NotImplementedError(f'--{name} needs a discriminator (--weight_D1 / --weight_D2), and discriminators are not built')
    if (args.test_interval or 0) > 0:
        raise NotImplementedError('--test_interval > 0: the CPU whole-image test pass is not built; run denoise_dir on a checkpoint')
    if (args.clean_data_ratio or 0) > 0:
        raise NotImplementedError('--clean_data_ratio > 0: clean-clean mixing is not built')
    if getattr(args, 'min_quality', None) is None:
        for name in ('min_quality_epochs', 'quality_csv'):
            if getattr(args, name, None):
                raise ValueError(f'--{name} needs --min_quality')
    elif (args.min_quality_epochs or 0) < 0:
        raise ValueError(f'--min_quality_epochs {args.min_quality_epochs} < 0')
    clip = getattr(args, 'g_clip_norm', None)
    if clip is not None and not 0 < clip < float('inf'):
        raise ValueError(f'--g_clip_norm {clip}: a positive finite norm')
    if getattr(args, 'max_skipped_steps', None) is not None:
        if not getattr(args, 'skip_nonfinite_steps', False):
            raise ValueError('--max_skipped_steps needs --skip_nonfinite_steps')
        if args.max_skipped_steps < 0:
            raise ValueError(f'--max_skipped_steps {args.max_skipped_steps} < 0')
    unknown = set(args.debug_options) - set(DEBUG_OPTIONS)
    if unknown:
        raise ValueError(f'unknown debug options {sorted(unknown)} (available: {DEBUG_OPTIONS})')


def get_weights(args):
    '''Loss weights from the weight_* options, as nn_common.py:423-452 means them (its last branches raise as written): a missing
    weight counts as 0, no weight at all means MS-SSIM alone, and weights that do not sum to 1 are divided by their total.'''
    weights = {'MSSSIM': 0, 'L1': 0, 'MSE': 0, 'SSIM': 0, 'D1': 0, 'D2': 0}
    for key in weights:
        weights[key] = getattr(args, 'weight_' + key, None) or 0
    total = sum(weights.values())
    if total == 0:
        weights['MSSSIM'] = 1
        print('Using default weights')
    elif total != 1:
        for key in weights:
            weights[key] /= total
    print(f'Loss weights: {weights}')
    return weights


# ------------------------------------------------------------------ the pieces of an epoch
def set_quality_bar(pool, min_quality, quality_csv, batch_size, world, pfun):
    '''The pool's bar from --min_quality (scores: --quality_csv, or one scoring pass over the pool), with the log lines of it.
    ValueError when the pairs above the bar leave fewer groups than one step of every rank takes.  Returns the steps per epoch.'''
    start = time.time()
    passing = pool.set_min_quality(min_quality, scores=quality_csv)
    source = quality_csv if quality_csv else 'scored on the pool in %.3f s' % (time.time() - start)
    steps = pool.n_active_groups // batch_size // world
    pfun(f'Quality bar: MS-SSIM > {min_quality} ({source}): {passing} of {pool.pairs.shape[0]} pairs pass, '
         f'{pool.n_active_groups} of {pool.n_groups} groups active; {steps} steps per epoch')
    if steps < 1:
        raise ValueError(f'nn_train: --min_quality {min_quality} leaves {pool.n_active_groups} active groups, fewer than the '
                         f'{batch_size * world} one step takes (batch_size {batch_size} x {world} rank(s))')
    return steps


def delete_outperformed_models(dpath, keepers, model_t='generator', keep_all_output_images=False):
    '''Removes the <model_t>_<epoch>.pt files, and the val/<epoch> and testimages/<epoch> directories unless
    keep_all_output_images, whose epoch is not in keepers (nn_train.py:95-116).  Returns what it removed.'''
    removed = []
    for fn in sorted(os.listdir(dpath)):
        fpath = os.path.join(dpath, fn)
        if fn in ('val', 'testimages') and os.path.isdir(fpath):
            if not keep_all_output_images:
                for subdir in sorted(os.listdir(fpath)):
                    if int(subdir) not in keepers:
                        shutil.rmtree(os.path.join(fpath, subdir))
                        removed.append(os.path.join(fpath, subdir))
            continue
        if not fn.startswith(f'{model_t}_'):
            continue
        epoch = int(fn.split('_')[1].split('.')[0])
        if epoch not in keepers:
            os.remove(fpath)
            removed.append(fpath)
    return removed


def update_lr_on_plateau(history, lr_loss, trainer, reduce_lr_factor):
    '''The reference's learning-rate rule (nn_train.py:412-417): when the loss of this epoch is above every loss of the last
    `history.maxlen` epochs, the rate is multiplied by reduce_lr_factor; then the loss joins the history.  Returns the new rate,
    or None when it stays.'''
    decayed = None
    if len(history) > 0 and max(history) < lr_loss:
        decayed = trainer.update_learning_rate(reduce_lr_factor)
    history.append(lr_loss)
    return decayed


def train_epoch(pool, trainer, batch_size, losses, ssim_losses=None, exp_mult_min=1, exp_mult_max=1, rank=0, world=1,
                log_interval=0, log=None, guard_log=None):
    '''One pass over the pool (nn_train.py:308-380 without the discriminators): a batch from the pool, one generator update, the
    step's loss kept on the device in losses[k] (and, with ssim_losses, the mean SSIM loss of the step's output in ssim_losses[k]).
    guard_log ([steps, 4] float64 on the device, for a trainer with a guarded step): row k takes the step's guard_state, and the
    losses of a step that was not applied are stored as 0.
    Nothing here waits for the GPU except an iteration line, every log_interval steps.  Returns the number of steps.'''
    from .validation import criteria
    iteration = 0
    for iteration, draws in enumerate(pool.epoch(batch_size, rank=rank, world=world), 1):
        clean, noisy = pool.batch(draws, exp_mult_min=exp_mult_min, exp_mult_max=exp_mult_max)
        if ssim_losses is not None:
            generated, loss = trainer.forward_backward(noisy, clean)
            trainer.optimizer_step()
            ssim_losses[iteration - 1] = criteria(generated, clean, {}, trainer.loss_cs, also=('SSIM',))['SSIM'].mean()
        else:
            loss = trainer.learn(noisy, clean)
        losses[iteration - 1] = loss[0]        # stays on the device: the epoch's mean is read once
        if guard_log is not None:
            guard_log[iteration - 1] = trainer.guard_state
            applied = trainer.guard_state[3] > 0
            for kept in (losses,) if ssim_losses is None else (losses, ssim_losses):
                kept[iteration - 1] = torch.where(applied, kept[iteration - 1], torch.zeros_like(kept[iteration - 1]))
        if log is not None and log_interval > 0 and iteration % log_interval == 0:
            log(iteration, loss.item())
    return iteration


def save_model(model, model_dir, epoch, name='generator'):
    '''<name>_<epoch>.pt = the module's state dict (Model.save_model, nn_common.py:68-73), as plain CPU tensors: the trainer's
    parameters are views of one flat buffer, which torch.save would otherwise write whole behind every tensor'''
    path = os.path.join(model_dir, '%s_%u.pt' % (name, epoch))
    torch.save({k: v.detach().to('cpu', copy=True).contiguous() for k, v in model.state_dict().items()}, path)
    return path


def file_sha256(path):
    h = hashlib.sha256()
    with open(path, 'rb') as f:
        for block in iter(lambda: f.read(1 << 20), b''):
            h.update(block)
    return h.hexdigest()


def guard_summary(guard_rows):
    '''The figures of an epoch from its steps' guard states ([steps, 4] on the host: sum g^2, non-finite count, scale, ok):
    (applied steps, skipped steps, clipped steps, mean and maximum gradient norm over the applied steps).'''
    ok = guard_rows[:, 3] > 0
    applied = int(ok.sum())
    norms = guard_rows[ok, 0].sqrt()
    clipped = int((guard_rows[ok, 2] < 1).sum())
    mean = norms.mean().item() if applied else float('nan')
    return applied, guard_rows.shape[0] - applied, clipped, mean, (norms.max().item() if applied else float('nan'))


def save_train_state(model_dir, state):
    '''train_state.pt, replaced atomically: written under a temporary name, flushed to the disk, then renamed over the old file.  A
    failure on the way leaves the old file in place.'''
    path = os.path.join(model_dir, STATE_FNAME)
    tmp = path + '.tmp'
    try:
        with open(tmp, 'wb') as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


def load_train_state(run_dir):
    '''The state --save_state left in run_dir.  ValueError when there is none, or when a later version of the program wrote it.'''
    path = os.path.join(run_dir, STATE_FNAME)
    if not os.path.isfile(path):
        raise ValueError(f'--resume {run_dir}: no {STATE_FNAME} there (the run was started without --save_state, or ended before its '
                         'first epoch did)')
    state = torch.load(path, map_location='cpu', weights_only=True)
    if not isinstance(state, dict) or 'format' not in state:
        raise ValueError(f'--resume {run_dir}: {path} is not a training state')
    if state['format'] > STATE_FORMAT:
        raise ValueError(f'--resume {run_dir}: {path} has format {state["format"]}, this program reads up to {STATE_FORMAT}')
    return state


def state_world(run_dir):
    '''The number of ranks of the run whose state file lies in run_dir, read without reading the file's tensors (they are mapped,
    not loaded: the launcher of a data-parallel run asks, and stays a small process).  ValueError as load_train_state.'''
    path = os.path.join(run_dir, STATE_FNAME)
    if not os.path.isfile(path):
        return load_train_state(run_dir)['world']        # raises, with the words of the one refusal
    state = torch.load(path, map_location='cpu', weights_only=True, mmap=True)
    if not isinstance(state, dict) or 'world' not in state:
        raise ValueError(f'--resume {run_dir}: {path} is not a training state')
    return int(state['world'])


def check_resumable(state, run_dir, world, pool_groups):
    '''ValueError unless the run can go on from `state` exactly: the same number of ranks, a pool of the same groups, and, where the
    checkpoint of the state's epoch is still there, the checkpoint the state was written beside.'''
    if state['world'] != world:
        raise ValueError(f'--resume {run_dir}: the state was written by a run of {state["world"]} rank(s), this one has {world}')
    if state['pool_groups'] != pool_groups:
        raise ValueError(f'--resume {run_dir}: the crop pool holds {pool_groups} groups, the state was written with '
                         f'{state["pool_groups"]} (the training data changed)')
    ckpt = os.path.join(run_dir, 'generator_%u.pt' % state['epoch'])
    if os.path.isfile(ckpt) and file_sha256(ckpt) != state['generator_sha256']:
        raise ValueError(f'--resume {run_dir}: {ckpt} is not the checkpoint {STATE_FNAME} was written beside (sha256 differs)')


def restore_trainer(trainer, state, rank=0, group=None):
    '''The trainer as the state file's run left it.  group: rank 0 holds the whole state; its scalars reach the other ranks as one
    object and its four buffers (parameters, m, v, vmax) by broadcast, straight into each trainer's own buffers.'''
    if group is None:
        trainer.load_state_dict(state['trainer'])
        return
    from .dist import broadcast_buffers
    buffers = ('flat', 'm', 'v', 'vmax')
    small = from_rank0({k: v for k, v in state['trainer'].items() if k not in buffers} if rank == 0 else None, group)
    # (a rank other than 0 checks and takes the scalars against its own buffers, which the broadcast then fills)
    trainer.load_state_dict(state['trainer'] if rank == 0 else dict(small, **{k: getattr(trainer, k) for k in buffers}))
    broadcast_buffers([getattr(trainer, k) for k in buffers], 0, group)


def make_expname(argv):
    return (datetime.datetime.now().isoformat()[:-10] + '_' + '_'.join(argv).replace('/', '-'))[0:255]


# ------------------------------------------------------------------ data parallel: what the ranks agree on
def from_rank0(value, group):
    '''rank 0's `value` on every rank of `group` (any picklable object; one broadcast)'''
    import torch.distributed as tdist
    box = [value]
    tdist.broadcast_object_list(box, src=tdist.get_global_rank(group, 0), group=group)
    return box[0]


def combine_epoch_sums(sums, count, group):
    '''The means of an epoch over the steps of every rank.  sums: this rank's sums over its own steps, Python floats (doubles);
    count: the number of those steps.  Every rank gathers every rank's (sums, count) and adds them in rank order, so all ranks
    hold the same bits.  Returns (the list of means, the total count).'''
    import torch.distributed as tdist
    parts = [None] * tdist.get_world_size(group)
    tdist.all_gather_object(parts, ([float(v) for v in sums], int(count)), group=group)
    totals, total_count = [0.0] * len(sums), 0
    for part_sums, part_count in parts:         # rank order
        totals = [a + b for a, b in zip(totals, part_sums)]
        total_count += part_count
    return [t / total_count for t in totals], total_count


def check_agreement(flat, group, epoch):
    '''RuntimeError, on every rank, unless all ranks hold the same parameters: every rank's (sum, sum of magnitudes) of its flat
    parameter buffer, both in double, are gathered and compared with rank 0's as bits.  One small collective.'''
    import struct
    import torch.distributed as tdist
    d = flat.detach().double()
    mine = struct.pack('<2d', *torch.stack((d.sum(), d.abs().sum())).tolist())
    sums = [None] * tdist.get_world_size(group)
    tdist.all_gather_object(sums, mine, group=group)
    bad = [r for r, s in enumerate(sums) if s != sums[0]]
    if bad:
        shown = ', '.join(f'rank {r}: sum {struct.unpack("<2d", sums[r])[0]!r}, sum of magnitudes {struct.unpack("<2d", sums[r])[1]!r}'
                          for r in [0] + bad)
        raise RuntimeError(f'nn_train: after epoch {epoch} the parameters of rank(s) {bad} differ from rank 0\'s ({shown}): '
                           'the ranks have diverged, and no checkpoint was saved for this epoch')


def parameters_digest(state_dict):
    '''SHA-256 over the tensors of a state dict, in its order, as their raw bytes'''
    h = hashlib.sha256()
    for value in state_dict.values():
        h.update(value.detach().to('cpu').contiguous().numpy().tobytes())
    return h.hexdigest()


class _NoResults:
    '''what a rank other than 0 holds in place of the JSONSaver: rank 0 owns trainres.json'''
    def add_res(self, *args, **kwargs):
        pass

    def write(self):
        pass


def record_figures(jsonsaver, epoch, figures):
    '''Figures of an epoch that are no score: they go into the epoch's entry of trainres.json (written with the entry's next write)
    and stay out of best_epoch / best_val, so checkpoint pruning, which keeps the best epochs, does not keep the epoch with the
    smallest gradient norm or the fewest clipped steps.'''
    if isinstance(jsonsaver, json_saver.JSONSaver):
        jsonsaver.results.setdefault(epoch, dict()).update(figures)


# ------------------------------------------------------------------ the run
def run(args, process_group=None, argv=None):
    '''The training run, in the reference's order of events.  Returns the run directory.
    process_group: every rank of the group calls this with the same args.  Rank 0 names the run, its parameters are broadcast,
    it alone writes the run directory's files, its clock decides time_limit; every rank takes batch_size crops per step from its
    own copy of the whole pool, validation is sharded, the epoch's mean loss is over all ranks' steps, and every epoch ends with
    check_agreement.  None: this process alone.'''
    from .crop_pool import CropPool
    from .train import UtNetTrainer
    from .validation import ValidationSet, validate

    check_supported(args)
    if not torch.cuda.is_available():
        raise RuntimeError('nn_train: no GPU visible; nind_denoise_amd has no CPU fallback')
    device = nn_common.default_device()
    argv = ['nn_train.py'] + sys.argv[1:] if argv is None else list(argv)
    full_size_data, ds_cs, ds_stride = full_size_options(args)
    for name in ('models_dpath', 'train_data', 'batch_size', 'g_lr', 'beta1', 'patience', 'reduce_lr_factor'):
        if getattr(args, name) is None and not (name == 'train_data' and full_size_data):
            raise ValueError(f'nn_train: --{name} is not set (on the command line or in a config file)')
    weights = get_weights(args)
    rank, world = 0, 1
    if process_group is not None:
        import torch.distributed as tdist
        rank, world = tdist.get_rank(process_group), tdist.get_world_size(process_group)

    # one run directory, and rank 0 owns every file in it: the other ranks print to stdout under their rank and record nothing
    resume_dir = getattr(args, 'resume', None)
    guard_on = getattr(args, 'g_clip_norm', None) is not None or bool(getattr(args, 'skip_nonfinite_steps', False))
    save_state = bool(getattr(args, 'save_state', False)) or resume_dir is not None
    expname = args.expname if args.expname else make_expname(argv)
    if world > 1:
        expname = from_rank0(expname, process_group)
    model_dir = resume_dir if resume_dir is not None else os.path.join(args.models_dpath, expname)
    state = None
    if resume_dir is not None:      # rank 0 reads the state file; what the other ranks need of it is broadcast below
        refusal = None
        if rank == 0:
            try:
                state = load_train_state(resume_dir)
            except ValueError as e:
                refusal = str(e)
        if world > 1:               # every rank raises rank 0's refusal, none is left waiting for a broadcast
            refusal = from_rank0(refusal, process_group)
        if refusal is not None:
            raise ValueError(refusal)
    if rank == 0:
        os.makedirs(model_dir, exist_ok=True)
        jsonsaver = json_saver.JSONSaver(os.path.join(model_dir, 'trainres.json'), step_type='epoch')
        p = Printer(file_path=os.path.join(model_dir, 'train.log'), flush=world > 1)
    else:
        jsonsaver = _NoResults()
        p = Printer(tofile=False, prefix=f'[rank {rank}] ', flush=True)
    p.print(args)
    p.print('cmd: python3 ' + ' '.join(argv))
    if resume_dir is None:          # (a resumed run's list comes from config.yaml, already expanded)
        args.test_reserve = get_test_reserve_list(args.test_reserve)
    p.print(f'test_reserve: {args.test_reserve}')
    torch.manual_seed(args.seed)

    # Train data
    if not args.min_crop_size and 'check_dataset' in args.debug_options:
        args.min_crop_size = args.cs
    if full_size_data:          # (min_crop_size is inert: every window is ds_cs x ds_cs)
        args.ds_cs, args.ds_stride = ds_cs, ds_stride       # into config.yaml, so that a resumed run rebuilds the same pool
        pool = CropPool.from_full_size(full_size_data, ds_cs=ds_cs, ds_stride=ds_stride, test_reserve=args.test_reserve,
                                       cs=args.cs, device=device, seed=args.seed)
        if args.loss_cs is None:
            args.loss_cs = ds_stride
    else:
        pool = CropPool.from_directories(args.train_data, test_reserve=args.test_reserve, min_crop_size=args.min_crop_size or None,
                                         cs=args.cs, device=device, seed=args.seed)
    if args.loss_cs is None:      # the <UCS> of a directory named <DSNAME>_<CS>_<UCS> (nn_train.py:220-222)
        parts = os.path.basename(os.path.normpath(os.fspath(args.train_data[0]))).split('_')
        if len(parts) < 3 or not parts[-1].isdigit():
            raise ValueError(f'nn_train: --loss_cs is not set and {args.train_data[0]} is not named <DSNAME>_<CS>_<UCS>')
        args.loss_cs = int(parts[-1])
    if args.cs is None:
        args.cs = pool.cs
    if 'short_run' in args.debug_options:
        pool.keep_groups(3 * args.batch_size)
    steps = all_steps = pool.n_groups // args.batch_size // world
    frames = f' (windows into {pool.n_frames} frames)' if pool.windowed else ''
    p.print(f'Crop pool: {pool.n_groups} groups, {pool.n_images} images{frames}, {pool.nbytes / 1e6:.1f} MB in HBM; {steps} steps per epoch')
    validation_set = None
    if full_size_data and args.validation_interval > 0 and args.validation_set_yaml is not None:
        # the crop files the list names are windows into the full-size images of the reserved sets: their names decide which
        # (crop_pool.crop_source), never what happens to exist on disk; every rank builds its own copy
        validation_set = ValidationSet.from_full_size(args.validation_set_yaml, full_size_data, ds_cs, ds_stride, device, cs=args.cs)
        p.print(f'Validation set: {len(validation_set)} pairs, {validation_set.n_windows} of them windows into '
                f'{validation_set.n_full_size_images} full-size images')
    if resume_dir is not None:
        if world > 1:       # the small fields; the trainer's buffers follow once the trainer exists
            small = from_rank0({k: v for k, v in state.items() if k != 'trainer'} if rank == 0 else None, process_group)
            state = state if rank == 0 else small
        check_resumable(state, resume_dir, world, pool.n_groups)
    if args.min_quality is not None and (state is None or state['quality_bar_active']):
        # every rank scores its own identical pool: the kernels are deterministic
        steps = set_quality_bar(pool, args.min_quality, args.quality_csv, args.batch_size, world, p.print)
    if world > 1:
        # CropPool.epoch deals batch k to rank k % world from pools with the same groups and generator state: every rank holds all
        p.print(f'Data parallel: {world} ranks, {args.batch_size} crops per rank and step; every rank read every file and holds '
                f'the whole pool: {pool.nbytes / 1e6:.1f} MB of HBM per rank, {world} readers of the same files')

    # init models
    model = nn_common.Model.instantiate_model(models_dpath=args.models_dpath, model_path=args.g_model_path, network='UtNet',
                                              device=device, pfun=p.print, keyword='generator', funit=args.g_funit,
                                              activation=args.g_activation)
    if world > 1:       # rank 0's parameters on every rank, before the trainer takes them into its flat buffer
        from .dist import broadcast_parameters
        broadcast_parameters(model, 0, process_group)
    trainer = UtNetTrainer(model, lr=args.g_lr, beta1=args.beta1, weights={k: v for k, v in weights.items() if k[0] != 'D'},
                           device=device, process_group=process_group, loss_cs=args.loss_cs,
                           max_grad_norm=getattr(args, 'g_clip_norm', None),
                           skip_nonfinite=bool(getattr(args, 'skip_nonfinite_steps', False)))
    if resume_dir is not None:
        restore_trainer(trainer, state, rank, process_group if world > 1 else None)
        pool.set_rng_state(state['pool_rng_state'])       # every rank restores its own generator: they all held this state
        p.print(f'Resumed from {os.path.join(resume_dir, STATE_FNAME)}: epoch {state["epoch"]} done, {trainer.steps} steps, '
                f'learning rate {trainer.lr}')
    model.train()
    want_ssim = weights['SSIM'] > 0 or args.compute_SSIM_anyway
    exp_mult_min = 1 if args.exp_mult_min is None else args.exp_mult_min
    exp_mult_max = 1 if args.exp_mult_max is None else args.exp_mult_max

    # Validation data
    validation_loss = None if state is None else state['validation_loss']
    if args.validation_interval > 0:
        if args.validation_set_yaml is None:
            raise ValueError('nn_train: --validation_set_yaml is not set (or give --validation_interval 0)')
        if validation_set is None:
            validation_set = ValidationSet(args.validation_set_yaml, device=device, cs=args.cs)

        def get_validation_dpath(epoch):
            return os.path.join(model_dir, 'val', str(epoch)) if 'output_val_images' in args.debug_options else None
        if state is None:       # (a resumed run validated before its first epoch already, and carries the last loss)
            validation_loss, _ = validate(model, validation_set, trainer.weights, args.loss_cs, batch_size=args.val_batch_size,
                                          output_to_dir=get_validation_dpath(0), group=process_group)
            jsonsaver.add_res(0, {'validation_loss': validation_loss}, write=True)
            p.print(f'Validation loss: {validation_loss}')

    if rank == 0 and resume_dir is None:        # (a resumed run keeps the first run's file: its options are that run's)
        with open(os.path.join(model_dir, 'config.yaml'), 'w') as fp:
            yaml.dump({k: v for k, v in vars(args).items() if k != 'resume'}, fp)

    start_time = time.time()
    generator_loss_hist = collections.deque([] if state is None else state['loss_hist'], maxlen=args.patience)
    generator_learning_rate = trainer.lr if state is None else state['gen_lr']
    losses = torch.zeros(max(all_steps, 1), dtype=torch.float32, device=device)
    ssim_losses = torch.zeros_like(losses)
    guard_log = torch.zeros(max(all_steps, 1), 4, dtype=torch.float64, device=device) if guard_on else None

    # Train
    for epoch in range(args.start_epoch if state is None else state['epoch'] + 1, args.epochs):
        epoch_start_time = time.time()
        if pool.min_quality is not None and 0 < args.min_quality_epochs <= epoch - args.start_epoch:
            pool.set_min_quality(None)
            steps = all_steps
            p.print(f'Quality bar lifted after {args.min_quality_epochs} epoch(s): {pool.n_active_groups} groups active; '
                    f'{steps} steps per epoch')
        iteration = train_epoch(pool, trainer, args.batch_size, losses, ssim_losses if want_ssim else None, exp_mult_min,
                                exp_mult_max, rank, world, args.log_interval,
                                lambda it, loss: p.print('Epoch %u batch %u/%u: loss G: weighted: %.3f' % (epoch, it, steps, loss)),
                                **({'guard_log': guard_log} if guard_on else {}))
        applied = iteration
        if guard_on and iteration > 0:
            # the epoch's one read of the guard: under a process group every rank saw the same averaged gradients, so the same rows
            applied, skipped, clipped, norm_mean, norm_max = guard_summary(guard_log[:iteration].cpu())
            if args.max_skipped_steps is not None and skipped > args.max_skipped_steps:
                raise RuntimeError(f'nn_train: epoch {epoch} skipped {skipped} of {iteration} steps for non-finite gradients, more than '
                                   f'--max_skipped_steps {args.max_skipped_steps}; no checkpoint was saved for this epoch')

        # cleanup previous epochs (rank 0 alone: it saved them, and every rank has finished writing the images of earlier epochs)
        if rank == 0:
            removed = delete_outperformed_models(dpath=model_dir, keepers=jsonsaver.get_best_steps(), model_t='generator',
                                                 keep_all_output_images='keep_all_output_images' in args.debug_options)
            p.print(f'delete_outperformed_models removed {removed}')

        # Do validation
        if args.validation_interval > 0 and epoch % args.validation_interval == 0:
            validation_loss, _ = validate(model, validation_set, trainer.weights, args.loss_cs, batch_size=args.val_batch_size,
                                          output_to_dir=get_validation_dpath(epoch), group=process_group)
            jsonsaver.add_res(epoch, {'validation_loss': validation_loss}, write=False)
            p.print(f'Validation loss: {validation_loss}')

        p.print('Epoch %u summary:' % epoch)
        p.print('Time elapsed (s): %u (epoch), %u (total)' % (time.time() - epoch_start_time, time.time() - start_time))
        p.print('Generator:')
        if iteration > 0 and applied == 0:
            p.print(f'Generator learned nothing: all {iteration} steps were skipped for non-finite gradients')
            record_figures(jsonsaver, epoch, {'skipped_steps': skipped, 'clipped_steps': 0})
            jsonsaver.write()
        elif iteration > 0:
            if world > 1:       # the mean over every rank's steps, the same bits on all ranks: the learning-rate rule reads it
                sums = torch.stack((losses[:iteration].double().sum(), ssim_losses[:iteration].double().sum())).tolist()
                means, _ = combine_epoch_sums(sums, applied, process_group)
            elif guard_on:      # the losses of skipped steps are stored as 0: the means run over the applied steps
                means = (torch.stack((losses[:iteration].double().sum(), ssim_losses[:iteration].double().sum())) / applied).tolist()
            else:
                means = torch.stack((losses[:iteration].double().mean(), ssim_losses[:iteration].double().mean())).tolist()
            if guard_on:
                p.print('Gradient norm: mean %f, max %f; clipped steps: %u, skipped steps: %u (of %u)'
                        % (norm_mean, norm_max, clipped, skipped, iteration))
                record_figures(jsonsaver, epoch, {'grad_norm_mean': norm_mean, 'clipped_steps': clipped, 'skipped_steps': skipped})
            if want_ssim:
                p.print('Average SSIM loss: %f' % means[1])
                jsonsaver.add_res(epoch, {'train_SSIM_loss': means[1]}, write=False)
            average_g_weighted_loss = means[0]
            p.print('Average weighted loss: %f' % average_g_weighted_loss)
            jsonsaver.add_res(epoch, {'train_weighted_loss': average_g_weighted_loss}, write=False)
            lr_loss = validation_loss if validation_loss is not None else average_g_weighted_loss
            hist = list(generator_loss_hist)
            if update_lr_on_plateau(generator_loss_hist, lr_loss, trainer, args.reduce_lr_factor) is not None:
                # (the rate the optimizer now uses; the reference reports it multiplied by the factor once more, nn_common.py:252-255)
                generator_learning_rate = trainer.lr
                p.print(f'Generator learning rate updated to {generator_learning_rate} because generator_loss_hist={hist} < lr_loss={lr_loss}')
            jsonsaver.add_res(epoch, {'gen_lr': generator_learning_rate}, write=True)
        else:
            p.print('Generator learned nothing')
        if world > 1:
            check_agreement(trainer.flat, process_group, epoch)
        if rank == 0:
            ckpt = save_model(model, model_dir, epoch, 'generator')
            if save_state:
                save_train_state(model_dir, {
                    'format': STATE_FORMAT, 'epoch': epoch, 'trainer': trainer.state_dict(), 'loss_hist': list(generator_loss_hist),
                    'gen_lr': generator_learning_rate, 'validation_loss': validation_loss, 'pool_rng_state': pool.rng_state(),
                    'quality_bar_active': pool.min_quality is not None, 'world': world, 'pool_groups': pool.n_groups,
                    'generator_sha256': file_sha256(ckpt)})
        time_is_up = bool(args.time_limit and args.time_limit < time.time() - start_time)
        if world > 1 and args.time_limit:       # rank 0's clock decides: no rank may leave while the others wait in an all-reduce
            time_is_up = from_rank0(time_is_up, process_group)
        if time_is_up:
            p.print('Time is up')
            break
        if args.min_lr is not None and generator_learning_rate < args.min_lr:
            p.print('Minimum learning rate reached')
            break
    if world > 1:
        p.print(f'rank {rank} of {world}: parameters sha256 {parameters_digest(model.state_dict())}')
    return model_dir


# ------------------------------------------------------------------ data parallel: starting the ranks
def check_gpus(gpus):
    if not 1 <= gpus <= MAX_GPUS:
        raise ValueError(f'--gpus {gpus}: the number of ranks is between 1 and {MAX_GPUS}')
    return gpus


def strip_option(argv, name):
    '''argv without `name VALUE` and `name=VALUE`'''
    out, skip = [], False
    for arg in argv:
        if skip:
            skip = False
        elif arg == name:
            skip = True
        elif not arg.startswith(name + '='):
            out.append(arg)
    return out


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def launch(argv, gpus, command=None):
    '''Starts `gpus` ranks of this command, each a fresh process running `command` (default: python -m nind_denoise_amd.nn_train)
    with argv less its --gpus option, and RANK, LOCAL_RANK, WORLD_SIZE, MASTER_ADDR and a free MASTER_PORT in its environment, and
    waits for all of them.  When a rank exits with a status other than 0 the others get SIGTERM, SIGKILL after KILL_GRACE_S
    seconds, and that status is returned (128 + the signal for a rank that a signal ended); else 0.  This process never touches
    a GPU: each rank picks its own device (init_rank).'''
    check_gpus(gpus)
    argv = strip_option(list(argv), '--gpus')
    command = [sys.executable, '-m', 'nind_denoise_amd.nn_train'] if command is None else list(command)
    port = _free_port()
    procs = []
    try:            # a SIGTERM to this process ends the ranks too (SystemExit goes through the finally below)
        previous = signal.signal(signal.SIGTERM, lambda signum, frame: sys.exit(128 + signum))
    except ValueError:      # not the main thread: signals cannot be caught here
        previous = None
    try:
        for rank in range(gpus):
            env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(gpus), MASTER_ADDR='127.0.0.1',
                       MASTER_PORT=str(port))
            procs.append(subprocess.Popen(command + argv, env=env))
        status = 0
        while status == 0 and any(proc.returncode is None for proc in procs):
            time.sleep(0.05)
            for proc in procs:
                if proc.poll():
                    status = proc.returncode
                    break
        return status if status >= 0 else 128 - status
    finally:        # a failed rank, or an exception here (Ctrl-C): nothing is left running
        alive = [proc for proc in procs if proc.poll() is None]
        for proc in alive:
            proc.send_signal(signal.SIGTERM)
        deadline = time.monotonic() + KILL_GRACE_S
        for proc in alive:
            try:
                proc.wait(timeout=max(0.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                proc.kill()
                proc.wait()
        if previous is not None:
            signal.signal(signal.SIGTERM, previous)


def world_from_environment():
    '''(rank, local rank, world size) a launcher left in the environment (launch, or torchrun), or None'''
    world = int(os.environ.get('WORLD_SIZE', '1'))
    if world <= 1:
        return None
    rank = int(os.environ['RANK'])
    return rank, int(os.environ.get('LOCAL_RANK', rank)), world


def init_rank(rank, local_rank, world, backend=None):
    '''This process becomes rank `rank` of `world`: its device is LOCAL_RANK % the number of GPUs, set before anything allocates;
    the backend is nccl (RCCL) when every rank has a GPU of its own, else gloo: ranks then share GPUs and every message is staged
    through the host (dist._host_staged), the rehearsal the project runs on one GPU.  Returns the process group.'''
    import torch.distributed as tdist
    if not torch.cuda.is_available():
        raise RuntimeError('nn_train: no GPU visible; nind_denoise_amd has no CPU fallback')
    n_devices = torch.cuda.device_count()
    torch.cuda.set_device(local_rank % n_devices)
    backend = backend or ('nccl' if world <= n_devices else 'gloo')
    if backend == 'nccl' and world > n_devices:
        raise ValueError(f'--dist_backend nccl: {world} ranks on {n_devices} GPU(s), and RCCL refuses two ranks on one device; use gloo')
    tdist.init_process_group(backend, rank=rank, world_size=world)      # MASTER_ADDR, MASTER_PORT from the environment
    return tdist.group.WORLD


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = parse_args(argv)
    if args.gpus is not None:
        check_gpus(args.gpus)
    ranked = world_from_environment()
    if ranked is None and getattr(args, 'resume', None) is not None:
        # a run that `--gpus N` started recorded `gpus: null` (launch() takes the option off every rank's command line, and rank 0
        # writes config.yaml): the state file knows how many ranks wrote it, and that many are started again
        args.gpus = state_world(args.resume)
    if ranked is None:
        if (args.gpus or 1) > 1:
            check_supported(args)       # refuse here what every rank would refuse
            return launch(argv, args.gpus)
        run(args, argv=['nn_train.py'] + argv)
        return 0
    # a rank: started by launch() above, or by an external launcher such as torchrun
    rank, local_rank, world = ranked
    if args.gpus not in (None, world):
        raise ValueError(f'--gpus {args.gpus} inside a rank of a world of {world} (WORLD_SIZE): a rank does not start ranks')
    import torch.distributed as tdist
    group = init_rank(rank, local_rank, world, args.dist_backend)
    try:
        run(args, process_group=group, argv=['nn_train.py'] + argv)     # the trainer is built after the group exists
    finally:
        tdist.destroy_process_group()
    return 0


if __name__ == '__main__':
    sys.exit(main())
