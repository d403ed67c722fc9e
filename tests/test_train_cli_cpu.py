"""The training command line (pasta-gan_amd/train_wo_flow_fullbody.py) and the statistics collector, without a GPU.  The
reference's script cannot be run to record a fixture (its line 222 is not valid Python), so the option mapping is checked
against the rows of its ``cfg_specs`` table (train_wo_flow_fullbody.py:166-174), quoted here:

    'stylegan2': ref_gpus=8, kimg=25000, mb=32, mbstd=4, fmaps=0.5, lrate=0.002, gamma=10, ema=10, ramp=None, map=2
    'fashion':   ref_gpus=8, kimg=8000,  mb=32, mbstd=4, fmaps=0.5, lrate=0.002, gamma=10, ema=10, ramp=None, map=1
    'auto':      mb = max(min(gpus * min(4096 // res, 32), 64), gpus), mbstd = min(mb // gpus, 4), fmaps = 1 if res >= 512 else 0.5,
                 lrate = 0.002 if res >= 1024 else 0.0025, gamma = 0.0002 * res ** 2 / mb, ema = mb * 10 / 32, ramp=0.05, map=2
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from conftest import ROOT
from train_grid_tree import PERSONS, make_tree


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('train_cli'))


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_dry_run_fashion_on_eight_gpus(tree, tmp_path):
    outdir = tmp_path / 'runs'
    res = _run(tree, outdir, '--cfg', 'fashion', '--gpus', '8', '--l1_weight', '40', '--mask_weight', '20')
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    assert o['total_kimg'] == 8000 and o['batch_size'] == 32 and o['batch_gpu'] == 4 and o['num_gpus'] == 8
    cfg = o['cfg']
    assert cfg['ema_kimg'] == 10 and cfg['ema_rampup'] is None
    assert cfg['G_opt_kwargs']['lr'] == cfg['D_opt_kwargs']['lr'] == 0.002
    assert cfg['loss_kwargs']['r1_gamma'] == 10 and cfg['loss_kwargs']['l1_weight'] == 40 and cfg['loss_kwargs']['mask_weight'] == 20
    assert cfg['G_kwargs']['mapping_kwargs']['num_layers'] == 1
    assert cfg['D_kwargs']['epilogue_kwargs']['mbstd_group_size'] == 4
    assert cfg['G_kwargs']['synthesis_kwargs']['channel_base'] == cfg['D_kwargs']['channel_base'] == 16384      # fmaps 0.5
    assert cfg['ada_target'] == 0.6 and cfg['augment_kwargs']['xflip'] == 1 and 'imgfilter' not in cfg['augment_kwargs']    # ada, bgc
    assert o['image_snapshot_ticks'] == o['network_snapshot_ticks'] == 50 and o['random_seed'] == 0
    assert o['training_set_kwargs']['max_size'] == len(PERSONS) and o['training_set_kwargs']['resolution'] == 256
    assert re.search(r'00000-[^\n]*-fashion\n', res.output) and 'Dry run; exiting.' in res.output
    assert not outdir.exists()


def test_dry_run_stylegan2_and_overrides(tree, tmp_path):
    res = _run(tree, tmp_path / 'runs', '--cfg', 'stylegan2', '--gpus', '2', '--batch', '16', '--kimg', '100', '--gamma', '2.5', '--aug', 'fixed',
               '--p', '0.25', '--augpipe', 'bg', '--snap', '7', '--seed', '3', '--fp32', 'true', '--workers', '2', '--subset', '4')
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    cfg = o['cfg']
    assert o['total_kimg'] == 100 and o['batch_size'] == 16 and o['batch_gpu'] == 8 and o['random_seed'] == 3
    assert cfg['G_kwargs']['mapping_kwargs']['num_layers'] == 2 and cfg['loss_kwargs']['r1_gamma'] == 2.5
    assert cfg['augment_p'] == 0.25 and 'ada_target' not in cfg and 'brightness' not in cfg['augment_kwargs']
    assert cfg['G_kwargs']['synthesis_kwargs']['num_fp16_res'] == cfg['D_kwargs']['num_fp16_res'] == 0
    assert cfg['G_kwargs']['synthesis_kwargs']['conv_clamp'] is None and cfg['D_kwargs']['conv_clamp'] is None
    assert o['image_snapshot_ticks'] == 7 and o['data_loader_kwargs']['num_workers'] == 2
    assert o['training_set_kwargs']['max_size'] == 4 and o['training_set_kwargs']['random_seed'] == 3
    assert '-stylegan2-gamma2.5-kimg100-batch16-fixed-p0.25-bg' in res.output


def test_cfg_auto_at_256_on_one_gpu(tree, tmp_path):
    res = _run(tree, tmp_path / 'runs')
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    cfg = o['cfg']
    assert o['batch_size'] == 16 and o['batch_gpu'] == 16 and o['total_kimg'] == 25000
    assert cfg['loss_kwargs']['r1_gamma'] == 0.0002 * 256 ** 2 / 16
    assert cfg['G_opt_kwargs']['lr'] == 0.0025 and cfg['ema_kimg'] == 16 * 10 / 32 and cfg['ema_rampup'] == 0.05
    assert cfg['D_kwargs']['epilogue_kwargs']['mbstd_group_size'] == 4 and cfg['G_kwargs']['mapping_kwargs']['num_layers'] == 2
    assert '-auto1' in res.output


@pytest.mark.parametrize('extra, message', [
    (['--cond', 'true'], 'no labels'),
    (['--mirror', 'true'], 'mirrored key points'),
    (['--nhwc', 'true'], 'NCHW'),
    (['--metrics', 'fid50k_full'], 'metric call commented out'),
    (['--cfg', 'paper256'], 'only auto, stylegan2 and fashion'),
    (['--gpus', '3'], 'power of two'),
    (['--aug', 'fixed'], 'requires specifying --p'),
    (['--resume', 'ffhq256'], 'downloads'),
])
def test_refused_options(tree, tmp_path, extra, message):
    res = _run(tree, tmp_path / 'runs', *extra)
    assert res.exit_code != 0
    assert message in res.output, res.output
    assert not (tmp_path / 'runs').exists()


def test_collector_on_cpu_tensors():
    from torch_utils import training_stats as S
    S.report('CliTest/a', torch.tensor([1.0, 2.0, 3.0]))               # before the collector exists: not counted
    c = S.Collector(regex='CliTest/.*')
    other = S.Collector(regex='Other/.*', keep_previous=False)
    assert c.num('CliTest/a') == 0 and np.isnan(c.mean('CliTest/a')) and np.isnan(c.std('CliTest/a'))
    S.report('CliTest/a', torch.tensor([[1.0, 2.0], [3.0, 6.0]]))
    S.report('CliTest/a', 8)
    S.report('CliTest/b', [5.0])
    S.report0('Other/x', 2.0)
    S.report('Elsewhere/y', 1.0)
    c.update()
    other.update()
    assert c.names() == ['CliTest/a', 'CliTest/b'] and other.names() == ['Other/x']
    assert c.num('CliTest/a') == 5 and c.mean('CliTest/a') == 4.0 and c['CliTest/a'] == 4.0
    assert c.std('CliTest/a') == pytest.approx(np.sqrt((1 + 4 + 9 + 36 + 64) / 5 - 16.0), rel=1e-12)     # population deviation
    assert c.num('CliTest/b') == 1 and c.mean('CliTest/b') == 5.0 and c.std('CliTest/b') == 0.0
    d = c.as_dict()
    assert sorted(d) == ['CliTest/a', 'CliTest/b'] and d['CliTest/a'].num == 5 and d['CliTest/b'].mean == 5.0
    assert other['Other/x'] == 2.0
    with pytest.raises(AssertionError):
        c.mean('Other/x')                                               # outside its regex
    # an interval without reports: keep_previous keeps the last figures, the other collector forgets them
    S.report('CliTest/b', [7.0, 9.0])
    c.update()
    other.update()
    assert c.mean('CliTest/a') == 4.0 and c.num('CliTest/a') == 5
    assert c.mean('CliTest/b') == 8.0 and c.num('CliTest/b') == 2 and c.std('CliTest/b') == 1.0
    assert other.num('Other/x') == 0 and np.isnan(other['Other/x'])


def test_abi_carries_the_grid_entries():
    from torch_utils import custom_ops
    text = open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    declared = set(re.findall(r'\b(pasta_[a-z0-9_]+)\s*\(', text))
    lib = ctypes.CDLL(custom_ops.build())
    for name in ('pasta_grid_composite_eroded_u8', 'pasta_grid_assemble', 'pasta_image_grid_tile_u8'):
        assert name in declared and name in custom_ops.ABI and hasattr(lib, name), name
    assert set(custom_ops.ABI) == declared
    assert os.path.exists(os.path.join(ROOT, 'pasta-gan_amd', 'csrc', 'train_grid.hip'))
    # bad arguments are refused on the host, before any launch
    typed = custom_ops.get_plugin()
    assert typed.pasta_image_grid_tile_u8(1, 1, 1, 2, 8, 8, 0, 1, 0, 0, 8, 8, -1.0, 127.5, None) != 0
    assert b'image_grid_tile_u8' in typed.pasta_last_error()
    assert typed.pasta_image_grid_tile_u8(1, 1, 4, 3, 8, 8, 0, 2, 1, 1, 16, 24, -1.0, 127.5, None) != 0      # tiles 2, 3 fall below the canvas
    assert b'leave the' in typed.pasta_last_error()
