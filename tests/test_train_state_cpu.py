"""Continuing a training run, without a GPU: the sampler's ``skip``, the training-state file's round trip, the command line's
``--continue`` / ``--save-state`` through ``--dry-run``, and the signal handlers that end a run at the next tick."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from click.testing import CliRunner

from conftest import PKG
from train_grid_tree import PERSONS, make_tree


# ---- the sampler ----

@pytest.mark.parametrize('shuffle', [True, False])
@pytest.mark.parametrize('n', [7, 50])            # reach = 4 and 25
@pytest.mark.parametrize('replicas', [1, 2, 8])
def test_sampler_skip_continues_the_stream(replicas, n, shuffle):
    from torch_utils.misc import InfiniteSampler
    data = list(range(n))
    skips = [0, replicas, 5 * replicas, n * replicas + replicas]
    for rank in range(replicas):
        take = max(skips) // replicas + 200
        whole = list(itertools.islice(iter(InfiniteSampler(data, rank=rank, num_replicas=replicas, shuffle=shuffle, seed=5)), take))
        assert whole == list(itertools.islice(iter(InfiniteSampler(data, rank=rank, num_replicas=replicas, shuffle=shuffle, seed=5, skip=0)), take))
        for k in skips:
            got = list(itertools.islice(iter(InfiniteSampler(data, rank=rank, num_replicas=replicas, shuffle=shuffle, seed=5, skip=k)), 200))
            assert got == whole[k // replicas:k // replicas + 200], (rank, k)
    if shuffle:
        assert whole[:n] != sorted(whole[:n]) or n < 3


def test_sampler_skip_across_the_replay_blocks():
    """The replay takes its draws 65536 at a time; a skip of three blocks and a bit lands where the one-by-one stream is."""
    from torch_utils.misc import InfiniteSampler
    k = 3 * 65536 + 17
    whole = list(itertools.islice(iter(InfiniteSampler(list(range(50)), seed=2)), k + 200))
    assert list(itertools.islice(iter(InfiniteSampler(list(range(50)), seed=2, skip=k)), 200)) == whole[k:]
    with pytest.raises(AssertionError):
        InfiniteSampler(list(range(5)), skip=-1)


# ---- the state file ----

def _hand_made_state():
    rs = np.random.RandomState(11)
    rs.normal(size=3)                                   # an odd number of normals: has_gauss = 1, a cached value
    from training import train_state
    gen = torch.Generator().manual_seed(4)
    return dict(cur_nimg=12, batch_idx=6, cur_tick=2, elapsed_sec=3.25, num_gpus=1, batch_size=2, batch_gpu=2, random_seed=0, options='{"a": 1}',
                G={'w': torch.randn([3, 2], generator=gen), 'b': torch.arange(4, dtype=torch.float16)}, D={}, G_ema={'w': torch.zeros([3, 2])},
                opt={'G': {'state': {0: {'step': torch.tensor(6.0), 'exp_avg': torch.ones([3, 2])}},
                           'param_groups': [{'lr': 0.0016, 'betas': (0.0, 0.99), 'fused': True, 'foreach': None, 'params': [0]}]}},
                grid_z=torch.zeros([9, 0]),
                ranks=[dict(torch_rng=gen.get_state(), cuda_rng=torch.arange(16, dtype=torch.uint8),
                            numpy_rng=train_state.numpy_rng_to_plain(rs.get_state()), ada_acc=torch.tensor([1.0, 4.0]))]), rs


def test_state_file_round_trip(tmp_path):
    from training import train_state
    state, rs = _hand_made_state()
    path = tmp_path / 'training-state-000000.pt'
    assert train_state.save_state(str(path), None, state) == str(path)
    assert sorted(os.listdir(tmp_path)) == ['training-state-000000.pt']          # the .tmp file is gone
    plain = torch.load(path, map_location='cpu', weights_only=True)             # no pickled classes
    assert plain['format'] == 1
    got = train_state.load_state(str(path))

    def same(a, b, where):
        if isinstance(a, torch.Tensor):
            assert isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), where
        elif isinstance(a, dict):
            assert isinstance(b, dict) and list(a) == list(b), where
            for k in a:
                same(a[k], b[k], where + (k,))
        elif isinstance(a, (list, tuple)):
            assert isinstance(b, list) and len(a) == len(b), where          # a tuple comes back as a list
            for i, (x, y) in enumerate(zip(a, b)):
                same(x, y, where + (i,))
        else:
            assert type(a) is type(b) and a == b, where
    same(state, {k: v for k, v in got.items() if k != 'format'}, ())
    assert got['ranks'][0]['numpy_rng']['keys'].dtype == torch.uint32 and got['ranks'][0]['numpy_rng']['has_gauss'] == 1
    back = np.random.RandomState(0)
    back.set_state(train_state.numpy_rng_from_plain(got['ranks'][0]['numpy_rng']))
    assert np.array_equal(back.normal(size=5), rs.normal(size=5)) and np.array_equal(back.randint(1000, size=5), rs.randint(1000, size=5))
    assert train_state.state_files(str(tmp_path)) == [(0, str(path))]


def test_state_file_refuses_classes_and_other_formats(tmp_path):
    import dnnlib
    from training import train_state
    state, _ = _hand_made_state()
    with pytest.raises(TypeError, match='ndarray'):
        train_state.save_state(str(tmp_path / 'a.pt'), None, dict(state, extra=np.zeros(3)))
    assert os.listdir(tmp_path) == []
    train_state.save_state(str(tmp_path / 'b.pt'), None, dict(state, options=dnnlib.EasyDict(a=1)))       # a dict subclass is stored as a dict
    assert type(train_state.load_state(str(tmp_path / 'b.pt'))['options']) is dict
    torch.save(dict(state, format=2), tmp_path / 'c.pt')
    with pytest.raises(ValueError, match='format 2'):
        train_state.load_state(str(tmp_path / 'c.pt'))
    with pytest.raises(ValueError, match="batch_size=4.*batch_size=2"):
        train_state.check_run(state, num_gpus=1, batch_size=4, batch_gpu=2, random_seed=0)


# ---- the command line ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('train_state_cli'))


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


COMMAND = ('--cfg', 'fashion', '--batch', '2', '--kimg', '5', '--l1_weight', '40', '--mask_weight', '20')


@pytest.fixture(scope='module')
def recorded(tree, tmp_path_factory):
    """A run directory as the command leaves it: the training_options.json of a real --dry-run and a state file made from it."""
    from training import train_state
    root = tmp_path_factory.mktemp('recorded')
    res = _run(tree, root / 'runs', *COMMAND)
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = root / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    text = json.dumps(options, indent=2)
    (run_dir / 'training_options.json').write_text(text)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=2, batch_gpu=2, random_seed=0, options=text,
                 G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    return run_dir, options


def test_save_state_is_the_only_new_option(tree, tmp_path, recorded):
    _, options = recorded
    assert options['save_state'] is True and 'resume_state' not in options
    off = _options(_run(tree, tmp_path / 'runs', *COMMAND, '--save-state', 'false').output)
    assert off['save_state'] is False
    assert sorted(options) == sorted(['num_gpus', 'image_snapshot_ticks', 'network_snapshot_ticks', 'metrics', 'random_seed', 'save_state',
                                      'training_set_kwargs', 'data_loader_kwargs', 'metric_set_kwargs', 'total_kimg', 'batch_size', 'batch_gpu',
                                      'cfg', 'run_dir'])
    for key in options:
        if key not in ('save_state', 'run_dir'):
            assert off[key] == options[key], key


def test_continue_prints_the_recorded_options(tree, tmp_path, recorded):
    run_dir, options = recorded
    outdir = tmp_path / 'elsewhere'
    for path in (run_dir, run_dir / 'training-state-000000.pt'):
        res = _run(tree, outdir, '--continue', str(path), '--kimg', '9')
        assert res.exit_code == 0, res.output
        got = _options(res.output)
        assert got['total_kimg'] == 9 and got['resume_state'] == str(run_dir / 'training-state-000000.pt')
        assert os.path.basename(got['run_dir']) == '00000-' + os.path.basename(options['run_dir'])[len('00000-'):] + '-continue000000'
        for key in options:
            if key not in ('total_kimg', 'run_dir'):
                assert got[key] == options[key], key
        assert 'Dry run; exiting.' in res.output and not outdir.exists()
    assert sorted(os.listdir(run_dir)) == ['training-state-000000.pt', 'training_options.json']
    # the options that may change do; --gpus and --batch may be repeated with their recorded values
    res = _run(tree, outdir, '--continue', str(run_dir), '--snap', '3', '--workers', '2', '--save-state', 'false', '--metrics', 'recon2k',
               '--gpus', '1', '--batch', '2')
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['network_snapshot_ticks'] == got['image_snapshot_ticks'] == 3 and got['data_loader_kwargs']['num_workers'] == 2
    assert got['save_state'] is False and got['metrics'] == ['recon2k'] and got['total_kimg'] == 5


@pytest.mark.parametrize('extra, name', [
    (['--batch', '4'], '--batch'),
    (['--gpus', '2'], '--gpus'),
    (['--cfg', 'auto'], '--cfg'),
    (['--resume', 'x.pkl'], '--resume'),
    (['--aug', 'noaug'], '--aug'),
    (['--seed', '1'], '--seed'),
    (['--allow-tf32', 'true'], '--allow-tf32'),
])
def test_continue_refuses_what_the_run_recorded(tree, tmp_path, recorded, extra, name):
    run_dir, _ = recorded
    res = _run(tree, tmp_path / 'runs', '--continue', str(run_dir), *extra)
    assert res.exit_code != 0
    assert name + ' cannot be given with --continue' in res.output and 'keeps its recorded value' in res.output, res.output
    assert not (tmp_path / 'runs').exists()


def test_continue_refuses_a_directory_without_a_state_file(tree, tmp_path, recorded):
    empty = tmp_path / '00000-empty'
    os.makedirs(empty)
    res = _run(tree, tmp_path / 'runs', '--continue', str(empty))
    assert res.exit_code != 0 and 'holds no training-state-*.pt' in res.output, res.output
    res = _run(tree, tmp_path / 'runs', '--continue', str(tmp_path / 'nowhere'))
    assert res.exit_code != 0 and 'neither a run directory nor' in res.output, res.output


def test_continue_refuses_another_data_set(tmp_path, recorded):
    import PIL.Image
    import shutil
    run_dir, _ = recorded
    bigger = make_tree(tmp_path / 'bigger')
    ds = os.path.join(bigger, 'Zalando_256_192')
    for sub, src, dst in (('image', 'za_0.jpg', 'za_9.jpg'), ('keypoints', 'za_0_keypoints.json', 'za_9_keypoints.json'),
                          ('parsing', 'za_0_label.png', 'za_9_label.png')):
        shutil.copy(os.path.join(ds, sub, src), os.path.join(ds, sub, dst))
    with open(os.path.join(ds, 'train_pairs_front_list_0508.txt'), 'a') as f:
        f.write('za_9.jpg za_9_cloth.jpg\n')
    res = _run(bigger, tmp_path / 'runs', '--continue', str(run_dir))
    assert res.exit_code != 0
    assert f'{len(PERSONS) + 1} people, the run was recorded on {len(PERSONS)}' in res.output, res.output


# ---- signals ----

_SIGNAL_SCRIPT = '''
import os, signal, sys
sys.path.insert(0, %r)
import train_wo_flow_fullbody as T
import torch
aborted = T.install_abort_signals()
assert aborted() is False
os.kill(os.getpid(), getattr(signal, sys.argv[1]))
assert aborted() is True
os.kill(os.getpid(), getattr(signal, sys.argv[1]))      # a second signal changes nothing
assert aborted() is True and not torch.cuda.is_initialized()
print('flag set by', sys.argv[1])
'''


@pytest.mark.parametrize('name', ['SIGUSR1', 'SIGTERM'])
def test_signal_sets_the_abort_flag(tmp_path, name):
    script = tmp_path / 'signals.py'
    script.write_text(_SIGNAL_SCRIPT % PKG)
    r = subprocess.run([sys.executable, str(script), name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'flag set by ' + name in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])
