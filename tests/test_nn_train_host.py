"""CPU tests of the training loop's host side (nind_denoise_amd/nn_train.py, validation.py, csrc/criteria.hip's argument checks):
the command line and its yaml precedence, what is refused, the loss weights, the learning-rate rule on a scripted loss sequence,
checkpoint pruning on a temporary tree, the validation set's centre crop, and the two new entry points of the library (which loads
without a GPU).  test_nn_train.py runs the kernels and the loop on the GPU."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import yaml

from nind_denoise_amd import _lib, nn_train, validation
from nind_denoise_amd.common.libs import imgcodec
from nind_denoise_amd.crop_pool import CropPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ parser
def write_yaml(path, conf):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, 'w') as f:
        yaml.dump(conf, f)
    return str(path)


def test_reference_defaults_without_any_file(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    args = nn_train.parse_args(['--test_reserve', '0'])
    assert (args.g_activation, args.g_funit, args.threads, args.epochs, args.start_epoch) == ('PReLU', 32, 6, 9001, 1)
    assert (args.validation_interval, args.test_interval, args.debug_options) == (1, 0, [])
    assert args.batch_size is None and args.g_lr is None and args.loss_cs is None and args.compute_SSIM_anyway is False
    assert (args.seed, args.expname, args.log_interval, args.val_batch_size) == (0, None, 50, 32)
    assert args.test_reserve == ['0'] and nn_train.get_test_reserve_list(args.test_reserve) == []
    with pytest.raises(SystemExit):
        nn_train.parse_args([])                # test_reserve is required, from the command line or from a file


def test_precedence_defaults_files_config_config2_argv(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    write_yaml(tmp_path / 'configs' / 'common_conf_default.yaml',
               {'models_dpath': 'common_models', 'batch_size': 1, 'beta1': 0.1, 'g_lr': 0.1, 'patience': 1, 'cs': 104})
    write_yaml(tmp_path / 'configs' / 'train_conf_defaults.yaml',
               {'batch_size': 2, 'beta1': 0.2, 'g_lr': 0.2, 'patience': 2, 'test_reserve': 'configs/test_set.yaml',
                'compute_SSIM_anyway': True, 'epochs': 321, 'weight_D1': 0, 'train_data': ['a_256_192']})
    c1 = write_yaml(tmp_path / 'c1.yaml', {'batch_size': 3, 'beta1': 0.3, 'g_lr': '3e-4', 'd_lr': 0.0003, 'crop_size': 184,
                                           'an_option_of_another_tool': 7, 'threads': 8, 'time_limit': None})
    c2 = write_yaml(tmp_path / 'c2.yaml', {'batch_size': 4, 'beta1': 0.4, 'debug_options': 'short_run'})
    args = nn_train.parse_args(['-c', c1, '--config2', c2, '--batch_size', '5', '--epochs', '7'])
    assert args.batch_size == 5                                   # argv over every file
    assert args.beta1 == 0.4                                      # config2 over config
    assert args.g_lr == 3e-4 and isinstance(args.g_lr, float)     # config over the default files; typed as the option types it
    assert args.patience == 2                                     # train_conf_defaults over common_conf_default
    assert args.models_dpath == 'common_models'                   # common_conf_default over argparse
    assert args.epochs == 7 and args.g_funit == 32                # argv over a default file; an argparse default nobody set
    assert args.cs == 184                                         # an alias names its option, over the common file's cs
    assert args.test_reserve == ['configs/test_set.yaml']         # a scalar for a list option, as the reference's files write it
    assert args.debug_options == ['short_run'] and args.train_data == ['a_256_192']
    assert args.compute_SSIM_anyway is True and args.threads == 8 and args.time_limit is None and args.d_lr == 0.0003
    assert not hasattr(args, 'an_option_of_another_tool')
    nn_train.check_supported(args)                                # d_lr and weight_D1: 0 ask for nothing
    # the default files are optional, -c is not
    with pytest.raises(FileNotFoundError):
        nn_train.parse_args(['-c', str(tmp_path / 'missing.yaml')])


REFUSED = [(['--g_network', 'UNet'], 'g_network'), (['--weight_D1', '0.1'], 'weight_D1'), (['--weight_D2', '0.2'], 'weight_D2'),
           (['--d_model_path', 'd.pt'], 'd_model_path'), (['--d2_model_path', 'd.pt'], 'd2_model_path'),
           (['--d_network', 'Hul112Disc'], 'd_network'), (['--d2_network', 'Hul112Disc'], 'd2_network'),
           (['--freeze_generator'], 'freeze_generator'), (['--not_conditional'], 'not_conditional'),
           (['--not_conditional_2'], 'not_conditional_2'), (['--discriminator_advantage', '0.1'], 'discriminator_advantage'),
           (['--discriminator2_advantage', '0.1'], 'discriminator2_advantage'), (['--test_interval', '5'], 'test_interval'),
           (['--clean_data_ratio', '0.05'], 'clean_data_ratio')]


@pytest.mark.parametrize('argv,name', REFUSED, ids=[r[1] for r in REFUSED])
def test_refused_options_raise_with_their_name(tmp_path, monkeypatch, argv, name):
    monkeypatch.chdir(tmp_path)
    args = nn_train.parse_args(['--test_reserve', '0'] + argv)
    with pytest.raises(NotImplementedError, match=re.escape('--' + name)) as e:
        nn_train.check_supported(args)
    assert '\n' not in str(e.value)
    with pytest.raises(NotImplementedError):                      # run refuses before it looks for a GPU or a directory
        nn_train.run(args)
    nn_train.check_supported(nn_train.parse_args(['--test_reserve', '0', '--g_network', 'UtNet', '--weight_D1', '0']))
    with pytest.raises(ValueError, match='no_such_option'):
        nn_train.check_supported(nn_train.parse_args(['--test_reserve', '0', '--debug', 'no_such_option']))


# ------------------------------------------------------------------ weights
def weights_of(**kw):
    ns = nn_train.parse_args(['--test_reserve', '0'])
    for k, v in kw.items():
        setattr(ns, k, v)
    return nn_train.get_weights(ns)


def test_get_weights():
    w = weights_of()
    assert {k: v for k, v in w.items() if v} == {'MSSSIM': 1} and set(w) == {'MSSSIM', 'L1', 'MSE', 'SSIM', 'D1', 'D2'}
    assert {k: v for k, v in weights_of(weight_L1=0, weight_MSE=0.0, weight_SSIM=None).items() if v} == {'MSSSIM': 1}
    w = weights_of(weight_L1=1, weight_MSE=3)
    assert {k: v for k, v in w.items() if v} == {'L1': 0.25, 'MSE': 0.75}
    w = weights_of(weight_SSIM=0.2, weight_MSSSIM=0.8)           # a total of 1 is left as it is
    assert (w['SSIM'], w['MSSSIM']) == (0.2, 0.8)
    assert weights_of(weight_MSE=5)['MSE'] == 1


# ------------------------------------------------------------------ learning-rate rule
class StubTrainer:
    def __init__(self, lr):
        self.lr, self.calls = lr, []

    def update_learning_rate(self, lr_decay):
        self.calls.append(lr_decay)
        self.lr *= lr_decay
        return self.lr


def test_lr_rule_on_a_scripted_loss_sequence():
    patience, losses, factor = 3, [.5, .4, .3, .35, .45, .2, .5], 0.5
    # restated: a decay at step k iff the history is not empty and max(the last <= 3 losses before k) < losses[k]
    want = [k for k in range(len(losses)) if k > 0 and max(losses[max(0, k - patience):k]) < losses[k]]
    assert want == [4, 6]
    trainer, hist, decayed_at = StubTrainer(1.0), collections.deque(maxlen=patience), []
    for k, loss in enumerate(losses):
        before = list(hist)
        assert before == losses[max(0, k - patience):k]              # the loss is appended after the test, never before
        ret = nn_train.update_lr_on_plateau(hist, loss, trainer, factor)
        if ret is not None:
            decayed_at.append(k)
            assert ret == trainer.lr                                 # the rate in use, not the rate times the factor once more
        assert hist[-1] == loss and len(hist) == min(k + 1, patience)
    assert decayed_at == want and trainer.calls == [factor] * 2 and trainer.lr == 0.25


# ------------------------------------------------------------------ pruning
def make_run_dir(root):
    for epoch in range(1, 7):
        (root / f'generator_{epoch}.pt').write_bytes(b'g')
        (root / f'discriminator_{epoch}.pt').write_bytes(b'd')
        for sub in ('val', 'testimages'):
            os.makedirs(root / sub / str(epoch))
            (root / sub / str(epoch) / '0.tif').write_bytes(b't')
    for name in ('train.log', 'config.yaml', 'trainres.json', 'notes_generator.txt'):
        (root / name).write_bytes(b'x')
    os.makedirs(root / 'other' / '1')


def test_delete_outperformed_models(tmp_path):
    root = tmp_path / 'run'
    os.makedirs(root)
    make_run_dir(root)
    removed = nn_train.delete_outperformed_models(str(root), keepers={0, 2, 5})
    gone = {1, 3, 4, 6}
    assert sorted(os.listdir(root)) == sorted([f'generator_{e}.pt' for e in (2, 5)] + [f'discriminator_{e}.pt' for e in range(1, 7)]
                                              + ['val', 'testimages', 'other', 'train.log', 'config.yaml', 'trainres.json',
                                                 'notes_generator.txt'])
    for sub in ('val', 'testimages'):
        assert sorted(os.listdir(root / sub)) == ['2', '5']
    assert os.listdir(root / 'other') == ['1']
    assert set(removed) == ({str(root / f'generator_{e}.pt') for e in gone} | {str(root / s / str(e)) for e in gone
                                                                              for s in ('val', 'testimages')})
    assert nn_train.delete_outperformed_models(str(root), keepers={0, 2, 5}) == []

    root2 = tmp_path / 'run2'
    os.makedirs(root2)
    make_run_dir(root2)
    removed = nn_train.delete_outperformed_models(str(root2), keepers={6}, keep_all_output_images=True)
    assert sorted(os.listdir(root2 / 'val')) == [str(e) for e in range(1, 7)]
    assert sorted(os.listdir(root2 / 'testimages')) == [str(e) for e in range(1, 7)]
    assert [f for f in os.listdir(root2) if f.startswith('generator_')] == ['generator_6.pt'] and len(removed) == 5
    nn_train.delete_outperformed_models(str(root2), keepers={6}, model_t='discriminator')
    assert [f for f in os.listdir(root2) if f.startswith('discriminator_')] == ['discriminator_6.pt']


# ------------------------------------------------------------------ validation set
def test_center_crop_matches_numpy_for_even_and_odd_margins():
    rng = np.random.default_rng(0)
    x, y = rng.random((3, 75, 90), dtype=np.float32), rng.random((3, 75, 90), dtype=np.float32)
    cs = 72                                              # margins: 3 rows (odd: 1 above, 2 below), 18 columns (even)
    cx, cy = validation.center_crop_pair(x, y, cs)
    x0, y0 = (90 - cs) // 2, (75 - cs) // 2
    assert (x0, y0) == (9, 1)
    assert np.array_equal(cx, x[:, 1:73, 9:81]) and np.array_equal(cy, y[:, 1:73, 9:81]) and cx.shape == (3, 72, 72)
    xt, yt = x.transpose(0, 2, 1), y.transpose(0, 2, 1)  # 90 x 75: the odd margin on the columns
    cx, cy = validation.center_crop_pair(xt, yt, cs)
    assert np.array_equal(cx, xt[:, 9:81, 1:73]) and np.array_equal(cy, yt[:, 9:81, 1:73])
    cx, _ = validation.center_crop_pair(x[:, :72, :72], y[:, :72, :72], cs)       # no margin
    assert np.array_equal(cx, x[:, :72, :72])
    with pytest.raises(ValueError, match='clean.png'):
        validation.center_crop_pair(x[:, :71], y[:, :71], cs, ('clean.png', 'noisy.png'))
    with pytest.raises(ValueError, match='noisy.png'):
        validation.center_crop_pair(x, y[:, :, :80], cs, ('clean.png', 'noisy.png'))


def test_validation_set_reads_pairs_from_a_yaml_and_names_a_short_file(tmp_path):
    rng = np.random.default_rng(1)
    pairs, imgs = [], []
    for i, shape in enumerate([(75, 90), (72, 72), (80, 73)]):
        c, n = (rng.integers(0, 256, shape + (3,)).astype(np.uint8) for _ in range(2))
        paths = [str(tmp_path / f'{kind}{i}.png') for kind in ('clean', 'noisy')]
        imgcodec.write_png(paths[0], c)
        imgcodec.write_png(paths[1], n)
        pairs.append(paths)
        imgs.append((c, n))
    ypath = write_yaml(tmp_path / 'val.yaml', pairs)
    for source in (ypath, pairs):
        vs = validation.ValidationSet(source, 'cpu', 72)
        assert len(vs) == 3 and vs.clean.shape == (3, 3, 72, 72) and vs.noisy.dtype.is_floating_point
        for i, (c, n) in enumerate(imgs):
            h, w = c.shape[:2]
            y0, x0 = (h - 72) // 2, (w - 72) // 2
            for got, img in ((vs.clean[i], c), (vs.noisy[i], n)):
                want = img.transpose(2, 0, 1)[:, y0:y0 + 72, x0:x0 + 72].astype(np.single) / 255
                assert np.array_equal(got.numpy(), want)
            assert np.array_equal(vs[i][0].numpy(), vs.clean[i].numpy())
    with pytest.raises(ValueError, match=re.escape(pairs[0][0])):
        validation.ValidationSet(pairs, 'cpu', 76)                   # pair 0 is 75 rows high
    with pytest.raises(ValueError):
        validation.ValidationSet([], 'cpu', 72)


# ------------------------------------------------------------------ crop pool: short_run
def test_keep_groups_drops_the_tail_before_the_upload():
    rng = np.random.default_rng(2)

    def fill():
        pool = CropPool('cpu', seed=1, cs=8)
        for g in range(7):
            clean = [rng.integers(0, 255, (10, 12, 3)).astype(np.uint8) for _ in range(1 + g % 2)]
            pool.add_group(clean, clean if g == 2 else [rng.integers(0, 255, (10, 12, 3)).astype(np.uint8) for _ in range(1 + g % 3)])
        return pool
    rng = np.random.default_rng(2)
    full = fill()
    rng = np.random.default_rng(2)
    cut = fill()
    cut.keep_groups(4)
    assert cut.n_groups == 4 and cut.n_images == sum(len(set(full.group(g)[0]) | set(full.group(g)[1])) for g in range(4))
    for g in range(4):
        for ids_cut, ids_full in zip(cut.group(g)[:2], full.group(g)[:2]):
            assert len(ids_cut) == len(ids_full)
            assert all(np.array_equal(cut.image(a), full.image(b)) for a, b in zip(ids_cut, ids_full))
    assert cut.group(2)[0] == cut.group(2)[1]                        # the clean-clean group still holds its images once
    assert cut.nbytes == sum((cut.image(i).nbytes + 15) // 16 * 16 for i in range(cut.n_images))
    assert len(list(cut.epoch(2))) == 2
    cut.keep_groups(9)
    assert cut.n_groups == 4


# ------------------------------------------------------------------ the library
def test_library_exports_the_new_entry_points():
    lib = _lib.load()
    assert lib.nd_version() >= 115
    assert {'nd_criteria', 'nd_criteria_workspace_bytes', 'nd_criteria_grad', 'nd_criteria_grad_workspace_bytes',
            'nd_utnet_train_step_act_hw'} <= set(_lib.EXPORTS)
    assert 'nd_utnet_train_step_hw' not in _lib.EXPORTS           # 115: nd_utnet_train_step_act_hw with ND_ACT_PRELU is that call
    for name in ('nd_criteria', 'nd_criteria_grad', 'nd_criteria_grad_workspace_bytes', 'nd_utnet_train_step_act_hw'):
        assert hasattr(lib, name)
    hdr = open(os.path.join(ROOT, 'include', 'nind_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(nd_[a-z0-9_]+)\s*\(', code)) == set(_lib.EXPORTS)


def test_criteria_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(256)          # never dereferenced: every call below fails its host checks
    ok = dict(y=p, t=p, n=2, h=184, w=168, loss_cs=0, w_l1=0.0, w_mse=1.0, w_ssim=0.0, w_msssim=0.0, also=0, out=p, ws=p,
              ws_bytes=1 << 40, stream=None)
    bads = [dict(y=None), dict(t=None), dict(out=None), dict(ws=None), dict(n=0), dict(loss_cs=185), dict(loss_cs=169),
            dict(loss_cs=-1), dict(also=16),
            dict(w_msssim=1.0, loss_cs=160), dict(also=8, loss_cs=160), dict(w_msssim=0.5, h=160, w=184),
            dict(w_ssim=1.0, loss_cs=10), dict(also=4, h=184, w=10)]
    for bad in bads:
        args = dict(ok, **bad)
        rc = lib.nd_criteria(*args.values())
        assert rc == -1, (bad, rc)
        with pytest.raises(ValueError):
            _lib.check(rc, 'nd_criteria')
    need = lib.nd_criteria_workspace_bytes(2, 184, 168, 0)
    assert need > 2 * 2 * 3 * 184 * 168 * 4
    with pytest.raises(MemoryError):
        _lib.check(lib.nd_criteria(*dict(ok, ws_bytes=need - 1).values()))
    assert lib.nd_criteria_workspace_bytes(2, 184, 168, 185) == 0 and lib.nd_criteria_workspace_bytes(0, 184, 168, 0) == 0
    assert lib.nd_criteria_workspace_bytes(2, 184, 168, 161) < need


def test_criteria_grad_checks_its_arguments_before_any_launch():
    lib = _lib.load()
    p = ctypes.c_void_p(256)          # never dereferenced: every call below fails its host checks
    ok = dict(y=p, t=p, n=2, h=184, w=168, loss_cs=0, w_l1=0.0, w_mse=1.0, w_ssim=0.0, w_msssim=0.0, loss=p, gy=p, ws=p,
              ws_bytes=1 << 40, stream=None)
    bads = [dict(y=None), dict(t=None), dict(loss=None), dict(gy=None), dict(ws=None), dict(n=0), dict(loss_cs=185),
            dict(loss_cs=169), dict(loss_cs=-1),
            dict(w_msssim=1.0, loss_cs=160), dict(w_msssim=0.5, h=160, w=184),
            dict(w_ssim=1.0, loss_cs=10), dict(w_ssim=0.5, h=184, w=10)]
    for bad in bads:
        args = dict(ok, **bad)
        rc = lib.nd_criteria_grad(*args.values())
        assert rc == -1, (bad, rc)
        with pytest.raises(ValueError):
            _lib.check(rc, 'nd_criteria_grad')
    need = lib.nd_criteria_grad_workspace_bytes(2, 184, 168, 0)
    assert need > 2 * 2 * 3 * 184 * 168 * 4
    with pytest.raises(MemoryError):
        _lib.check(lib.nd_criteria_grad(*dict(ok, ws_bytes=need - 1).values()))
    assert lib.nd_criteria_grad_workspace_bytes(2, 184, 168, 185) == 0 and lib.nd_criteria_grad_workspace_bytes(0, 184, 168, 0) == 0
    # one workspace serves a trainer that changes loss_cs between calls: the size for the whole image covers every window
    for cs in (1, 11, 100, 161, 167, 168):
        assert 0 < lib.nd_criteria_grad_workspace_bytes(2, 184, 168, cs) <= need, cs
