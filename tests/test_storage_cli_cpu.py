"""16-bit activation storage from the command lines, without a GPU: ``--storage`` of train_wo_flow_fullbody.py through
``--dry-run`` on the 256 tree and on the 512 tree, its refusals, ``--storage`` of test.py, and ``training.networks.
set_activation_storage`` against modules CONSTRUCTED with the storage: every attribute the two ``_build`` methods and the
Discriminator's constructor decide from it, on every submodule, and an untouched state dict."""
import copy
import json
import os

import pytest
import torch
from click.testing import CliRunner

from oracle import param_fill as PF
from train_grid_tree import make_tree
from tryon_512_train_tree import make_512_train_tree

COMMAND = ('--cfg', 'fashion', '--batch', '2', '--kimg', '5', '--l1_weight', '40', '--mask_weight', '20')
ATTRIBUTES = ('act_dtype', 'use_fp16', 'half_dtype', 'channels_last')


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    return {256: make_tree(tmp_path_factory.mktemp('storage_cli_256')), 512: make_512_train_tree(tmp_path_factory.mktemp('storage_cli_512'))}


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


# ---- the printed options ----

@pytest.mark.parametrize('res', [256, 512])
@pytest.mark.parametrize('cfg', ['auto', 'stylegan2', 'fashion'])
def test_storage_f32_prints_what_no_option_prints(trees, tmp_path, res, cfg):
    plain = _run(trees[res], tmp_path / 'runs', '--cfg', cfg)
    f32 = _run(trees[res], tmp_path / 'runs', '--cfg', cfg, '--storage', 'f32')
    assert plain.exit_code == 0 and f32.exit_code == 0, (plain.output, f32.output)
    assert f32.output == plain.output                   # options, description, run directory: the same text
    text = json.dumps(_options(plain.output)['cfg'])    # no new key
    assert 'act_dtype' not in text and 'half_dtype' not in text and 'storage' not in text


@pytest.mark.parametrize('res, d_fp16_res', [(256, 6), (512, 7)])
@pytest.mark.parametrize('cfg', ['auto', 'stylegan2', 'fashion'])
def test_storage_bf16_sets_what_fashion_config_sets(trees, tmp_path, res, d_fp16_res, cfg):
    from training.training_loop_wo_flow_fullbody import fashion_config
    plain = _run(trees[res], tmp_path / 'runs', '--cfg', cfg)
    bf16 = _run(trees[res], tmp_path / 'runs', '--cfg', cfg, '--storage', 'bf16')
    assert plain.exit_code == 0 and bf16.exit_code == 0, (plain.output, bf16.output)
    a, b = _options(plain.output), _options(bf16.output)
    want = fashion_config(img_resolution=res, act_dtype='bfloat16')
    assert want.D_kwargs.num_fp16_res == d_fp16_res
    # the three keys ...
    assert b['cfg']['G_kwargs']['synthesis_kwargs'].pop('act_dtype') == want.G_kwargs.synthesis_kwargs.act_dtype == 'bfloat16'
    assert b['cfg']['D_kwargs'].pop('half_dtype') == want.D_kwargs.half_dtype == 'bfloat16'
    assert b['cfg']['D_kwargs'].pop('num_fp16_res') == d_fp16_res
    assert a['cfg']['D_kwargs'].pop('num_fp16_res') == 3
    # ... and nothing else but the run's name
    assert b['cfg'] == a['cfg']
    assert b.pop('run_dir') == a.pop('run_dir') + '-bf16'
    assert b == a
    assert ('patch_channels' in b['cfg']['G_kwargs']) == (res == 512)
    if res == 512:
        assert b['cfg']['G_kwargs']['patch_channels'] == 45
        assert b['training_set_kwargs']['class_name'].endswith('UvitonDatasetFull_512')


def test_storage_f16_and_the_description_after_other_suffixes(trees, tmp_path):
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--aug', 'noaug', '--storage', 'f16')
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    assert o['cfg']['G_kwargs']['synthesis_kwargs']['act_dtype'] == o['cfg']['D_kwargs']['half_dtype'] == 'float16'
    assert o['cfg']['D_kwargs']['num_fp16_res'] == 6
    assert o['run_dir'].endswith('-fashion-kimg5-batch2-noaug-f16')


# ---- refusals ----

def test_fp32_and_16_bit_storage_contradict(trees, tmp_path):
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--fp32', 'true', '--storage', 'bf16')
    assert res.exit_code != 0
    assert '--fp32' in res.output and '--storage' in res.output and 'contradict' in res.output, res.output
    assert not (tmp_path / 'runs').exists()
    # --fp32 true with fp32 storage stays what it was
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--fp32', 'true', '--storage', 'f32')
    assert res.exit_code == 0, res.output


def _recorded_run(tree, root, *extra):
    """A run directory as the command leaves it: the options of a real --dry-run and a state file that records them."""
    from training import train_state
    res = _run(tree, root / 'runs', *COMMAND, *extra)
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = root / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    text = json.dumps(options, indent=2)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=2, batch_gpu=2, random_seed=0, options=text,
                 G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    return run_dir, options


def test_continue_refuses_storage_and_carries_the_recorded_one(trees, tmp_path):
    run_dir, options = _recorded_run(trees[256], tmp_path / 'bf16', '--storage', 'bf16')
    for value in ('bf16', 'f32'):
        res = _run(trees[256], tmp_path / 'out', '--continue', str(run_dir), '--storage', value)
        assert res.exit_code != 0
        assert '--storage cannot be given with --continue' in res.output and 'keeps its recorded value' in res.output, res.output
    res = _run(trees[256], tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['cfg'] == options['cfg'] and got['cfg']['G_kwargs']['synthesis_kwargs']['act_dtype'] == 'bfloat16'
    assert os.path.basename(got['run_dir']).endswith('-bf16-continue000000')
    # a state file from before the option has no act_dtype: it continues in fp32
    run_dir, options = _recorded_run(trees[256], tmp_path / 'f32')
    assert 'act_dtype' not in json.dumps(options)
    res = _run(trees[256], tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['cfg'] == options['cfg'] and 'act_dtype' not in got['cfg']['G_kwargs']['synthesis_kwargs'] and 'half_dtype' not in got['cfg']['D_kwargs']


@pytest.mark.parametrize('script', ['test.py', 'test_512.py', 'calc_metrics.py'])
def test_inference_commands_take_the_four_values_only(tmp_path, script):
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location('storage_cli_' + script[:-3], os.path.join(PKG, script))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    command = module.calc_metrics if script == 'calc_metrics.py' else module.generate_images
    (option,) = [p for p in command.params if p.name == 'storage']
    assert list(option.type.choices) == ['snapshot', 'f32', 'bf16', 'f16'] and not option.required
    args = ['--network', str(tmp_path / 'none.pkl')] + ([] if script == 'calc_metrics.py' else ['--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path)])
    res = CliRunner().invoke(command, args + ['--storage', 'int8'])
    assert res.exit_code == 2 and "'--storage'" in res.output and 'int8' in res.output, res.output
    assert not (tmp_path / 'out').exists()


# ---- set_activation_storage ----

def _attributes(module):
    """{submodule path: {attribute: value}} of everything that construction decides from the storage type."""
    return {name: {a: getattr(m, a) for a in ATTRIBUTES if hasattr(m, a)} for name, m in module.named_modules()
            if any(hasattr(m, a) for a in ATTRIBUTES)}


def _with_storage(kind, dtype):
    from training import networks
    if kind == 'D':
        extra = dict() if dtype is None else dict(half_dtype=dtype, num_fp16_res=6)
        return networks.Discriminator(**PF.D_KWARGS, **extra)
    synthesis = dict(PF.G_KWARGS['synthesis_kwargs'], **(dict() if dtype is None else dict(act_dtype=dtype)))
    return getattr(networks, kind)(**dict(PF.G_KWARGS, synthesis_kwargs=synthesis))


@pytest.mark.parametrize('kind', ['GeneratorFull', 'GeneratorV18', 'D'])
def test_switch_sets_what_construction_sets(kind):
    from training.networks import set_activation_storage
    module = _with_storage(kind, None)
    fp32 = _attributes(module)
    blocks = [n for n, a in fp32.items() if 'use_fp16' in a]
    assert len(blocks) == (7 + 1 if kind != 'D' else 6) and not any(fp32[n]['use_fp16'] for n in blocks)
    before = copy.deepcopy(module.state_dict())
    kwargs = module.init_kwargs
    for name, dtype in (('bfloat16', torch.bfloat16), ('float16', torch.float16)):
        want = _attributes(_with_storage(kind, name))
        assert want != fp32 and all(want[n]['use_fp16'] and want[n]['half_dtype'] == dtype for n in blocks)
        for given in (name, dtype):
            assert set_activation_storage(module, given) is module
            assert _attributes(module) == want, (kind, given)
            for value in (None, 'float32', torch.float32):
                set_activation_storage(module, given)
                set_activation_storage(module, value)
                assert _attributes(module) == fp32, (kind, given, value)
    set_activation_storage(module, 'bfloat16')
    after = module.state_dict()
    assert list(after) == list(before)
    assert all(after[k].dtype == before[k].dtype and torch.equal(after[k], before[k]) for k in before)
    assert all(p.dtype == torch.float32 for p in module.parameters())
    assert module.init_kwargs == kwargs                 # a run-time switch: the recorded constructor arguments stay


def test_switch_refusals():
    from training import networks
    from training.networks import set_activation_storage
    with pytest.raises(TypeError, match='MappingNetwork'):
        set_activation_storage(networks.MappingNetwork(z_dim=0, c_dim=8, w_dim=8, num_ws=2, num_layers=1), 'bfloat16')
    with pytest.raises((AssertionError, AttributeError)):
        set_activation_storage(_with_storage('D', None), 'int8')
    # fp16_channels_last: use_fp16 decided the weights' memory format at construction
    D = networks.Discriminator(**PF.D_KWARGS, block_kwargs=dict(fp16_channels_last=True))
    assert not any(m.channels_last for m in D.modules() if hasattr(m, 'use_fp16'))      # num_fp16_res = 0: nothing shows on the blocks
    with pytest.raises(ValueError, match='fp16_channels_last'):
        set_activation_storage(D, 'bfloat16')
    G = networks.GeneratorFull(**dict(PF.G_KWARGS, synthesis_kwargs=dict(PF.G_KWARGS['synthesis_kwargs'], fp16_channels_last=True)))
    with pytest.raises(ValueError, match='fp16_channels_last'):
        set_activation_storage(G, None)
    assert G.synthesis.act_dtype is None and not G.synthesis.b64.use_fp16


@pytest.mark.parametrize('kind', ['GeneratorFull', 'GeneratorV18', 'D'])
@pytest.mark.parametrize('dtype', ['bfloat16', 'float16'])
def test_constructed_storage_survives_copy_and_pickle(kind, dtype):
    """G_ema is a deep copy of G and a snapshot is a pickle: persistence rebuilds every sub-module through its own constructor, so
    the blocks must have recorded their storage type themselves (they came back in float16 while the storage was set on them by the
    parent after construction, and a bf16 generator then met its own fp16 blocks)."""
    import pickle
    module = _with_storage(kind, dtype)
    want = _attributes(module)
    assert any(a.get('half_dtype') == getattr(torch, dtype) for a in want.values())
    assert _attributes(copy.deepcopy(module)) == want
    assert _attributes(pickle.loads(pickle.dumps(module))) == want
    # and a default module records nothing new: its blocks' constructor arguments are what they were
    plain = _with_storage(kind, None)
    assert not any('half_dtype' in m.init_kwargs for m in plain.modules() if hasattr(m, 'use_fp16'))
