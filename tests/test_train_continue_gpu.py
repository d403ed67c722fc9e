"""A training run that was cut off and continued from its training-state file equals the uninterrupted run BIT FOR BIT
(training/train_state.py, training_loop's ``save_state`` / ``resume_state``, the command's ``--continue``).

The yardstick is the step's own reproducibility, so the CONTROL comes first: the same run twice from scratch, their state
files compared entry by entry with ``torch.equal``.  Where it passes everything after it is held to ``torch.equal`` as well;
where it fails, to 4 x the control's largest absolute difference of each tensor (``_beyond``), and every entry the control
found equal -- counters, generator states -- to equality.  The loss statistics of stats.jsonl are part of no comparison.

MEASURED (one MI355X): the control passes, 0 tensors differ, and so does every comparison below, bit for bit.  (It failed while
the augmentation pipeline padded with torch's reflect mode, whose GPU gradient scatters with float atomics: two runs from scratch
then differed in all 1068 tensors after 6 iterations, by up to 8.9e-2 in an Adam first moment of magnitude 13, first in the R1
pass of iteration 0.  training/augment.py's ``_reflect_pad`` replaced it)

One item does not show within three iterations, as the issue allows for: ``ada_acc_and_p``.  At the cut p is 0 and the accumulator
holds [0, 4] -- the signs of iterations 5 and 6 sum to 0 -- so with s the sum over iterations 7 and 8 the adjustment after
iteration 8 sees (0 + s) / 8 with the accumulator and s / 4 without, and p, which cannot fall below 0, is 0 afterwards either
way: resetting both changes no tensor of the state.  The case asserts that finding instead of lengthening the run; that the
accumulator and p ARE carried over is held by the exact continuation (its first adjustment after the cut is fed by two iterations
from before it, and p reaches 0.16) and, entry by entry, by ``test_restore_puts_every_entry_back``.

Set-up: the tiny tree, test-size widths, batch 2, ticks of 5 iterations (they close after iterations 1, 6, 11, 16), a snapshot
and a state file every tick; ADA with ``ada_kimg = 0.1`` (p moves by 0.08 per adjustment, every 4th iteration, and the
pipeline draws from the device generator every iteration) and ``ema_rampup = 0.05`` (G_ema depends on cur_nimg)."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

from conftest import PKG, ROOT
from train_grid_tree import make_tree

pytestmark = pytest.mark.gpu

GNUM, BATCH, TICK = 3, 2, 5
IGNORED = ('elapsed_sec',)


def _cfg():
    from training.training_loop_wo_flow_fullbody import augment_options, fashion_config
    cfg = fashion_config(channel_base=2048, mbstd_group_size=2)
    cfg.update(augment_options('ada', 'bgc'))
    cfg.ada_kimg = 0.1
    cfg.ema_rampup = 0.05
    return cfg


def _run(tree, run_dir, iters, batch=BATCH, **kwargs):
    from training.training_loop_wo_flow_fullbody import training_loop
    os.makedirs(run_dir, exist_ok=True)
    args = dict(batch_size=batch, batch_gpu=BATCH, cfg=_cfg(), device=torch.device('cuda'),
                training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree),
                data_loader_kwargs=dict(num_workers=0, pin_memory=True), run_dir=str(run_dir), total_kimg=iters * batch / 1000,
                kimg_per_tick=TICK * batch / 1000, image_snapshot_ticks=None, network_snapshot_ticks=1, snapshot_gnum=GNUM, save_state=True)
    args.update(kwargs)
    return training_loop(**args)


def _file(run_dir):
    from training import train_state
    names = [n for n in os.listdir(run_dir) if n.startswith('training-state-')]
    assert names == ['training-state-000000.pt'], names         # one file, no .tmp beside it
    return os.path.join(str(run_dir), names[0]), train_state.load_state(os.path.join(str(run_dir), names[0]))


def _diff(a, b, where=''):
    """The paths at which two states differ."""
    if isinstance(a, dict) and isinstance(b, dict):
        out = [f'{where}/{k}' for k in set(a) ^ set(b)]
        for k in a:
            if k in b and not (where == '' and k in IGNORED):
                out += _diff(a[k], b[k], f'{where}/{k}')
        return out
    if isinstance(a, list) and isinstance(b, list) and len(a) == len(b):
        return [p for i, (x, y) in enumerate(zip(a, b)) for p in _diff(x, y, f'{where}/{i}')]
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
        return [] if a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b) else [where]
    return [] if type(a) is type(b) and a == b else [where]


def _spread(name, a, b):
    """Print, for the record, the largest absolute difference of every tensor that differs (largest first)."""
    def walk(x, y, where):
        if isinstance(x, dict) and isinstance(y, dict):
            return [r for k in x if k in y for r in walk(x[k], y[k], f'{where}/{k}')]
        if isinstance(x, list) and isinstance(y, list):
            return [r for i, (u, v) in enumerate(zip(x, y)) for r in walk(u, v, f'{where}/{i}')]
        if isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor) and x.shape == y.shape and x.numel() and not torch.equal(x, y):
            return [(float((x.double() - y.double()).abs().max()), float(x.double().abs().max()), where)]
        return []
    rows = sorted(walk(a, b, ''), reverse=True)
    print(f'{name}: {len(rows)} tensors differ' + ''.join(f'\n    {d:.3e} (largest |value| {m:.3e}) {w}' for d, m, w in rows[:6]))


def _spreads(a, b, where=''):
    """{path: largest absolute difference} of the tensors that differ between two states of one structure."""
    if isinstance(a, dict) and isinstance(b, dict):
        return {p: d for k in a if k in b and not (where == '' and k in IGNORED) for p, d in _spreads(a[k], b[k], f'{where}/{k}').items()}
    if isinstance(a, list) and isinstance(b, list):
        return {p: d for i, (x, y) in enumerate(zip(a, b)) for p, d in _spreads(x, y, f'{where}/{i}').items()}
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape and a.numel() and not torch.equal(a, b):
        return {where: float((a.double() - b.double()).abs().max())}
    return {}


def _beyond(a, b, tol):
    """The paths at which two states differ by more than the control allows: ``tol`` is {path: 4 x the control's largest absolute
    difference of that tensor}, empty when the control passed -- then this is ``_diff``, i.e. ``torch.equal``.  Entries that are
    not tensors, and tensors the control found equal (the generator states among them), must be equal."""
    if not tol:
        return _diff(a, b)
    spread = _spreads(a, b)
    return [p for p in _diff(a, b) if not (p in spread and spread[p] <= tol.get(p, 0.0))]


def _differs_in(diff, *entries):
    return any(p == '/' + e or p.startswith('/' + e + '/') for p in diff for e in entries)


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('train_continue'))


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    return tmp_path_factory.mktemp('runs')


@pytest.fixture(scope='module')
def run_a(tree, runs):
    """Run A: from scratch to 6 iterations.  (path of its state file, the state)"""
    _run(tree, runs / '00000-a', 6)
    return _file(runs / '00000-a')


@pytest.fixture(scope='module')
def control(tree, runs, run_a):
    """THE CONTROL: run A once more.  (the second run's state, the tolerance the other tests get from it: {} when the two runs are
    equal, else 4 x the largest absolute difference of every tensor that differs)"""
    _run(tree, runs / '00001-a-again', 6)
    _, again = _file(runs / '00001-a-again')
    _spread('control, A against A again', run_a[1], again)
    return again, {p: 4 * d for p, d in _spreads(run_a[1], again).items()}


@pytest.fixture(scope='module')
def two_more(tree, runs, run_a, control):
    """The exact continuation of A by two iterations: what a continuation with an item dropped is compared with."""
    _run(tree, runs / '00010-two-more', 8, resume_state=run_a[0])
    return _file(runs / '00010-two-more')[1]


# ---- the control ----

def test_control_two_runs_from_scratch_are_equal(run_a, control):
    _, a = run_a
    again, _ = control
    for s in (a, again):
        assert s['format'] == 1 and s['cur_nimg'] == 12 and s['batch_idx'] == 6 and s['cur_tick'] == 2 and s['options'] == ''
        assert (s['num_gpus'], s['batch_size'], s['batch_gpu'], s['random_seed']) == (1, BATCH, BATCH, 0)
        assert sorted(s) == sorted(['format', 'cur_nimg', 'batch_idx', 'cur_tick', 'elapsed_sec', 'num_gpus', 'batch_size', 'batch_gpu', 'random_seed',
                                    'options', 'G', 'D', 'G_ema', 'augment_pipe', 'opt', 'grid_z', 'ranks'])
        assert sorted(s['opt']) == ['D', 'G'] and len(s['ranks']) == 1
        assert sorted(s['ranks'][0]) == ['ada_acc', 'buffers', 'cuda_rng', 'numpy_rng', 'torch_rng']
        assert 'mapping.w_avg' in s['G'] and 'p' in s['augment_pipe'] and any(k.endswith('noise_const') for k in s['G'])
        assert tuple(s['grid_z'].shape) == (GNUM * GNUM, 0)
    assert a['elapsed_sec'] > 0
    assert _diff(a, again) == []


# ---- the exact continuation ----

def test_continued_run_equals_the_uninterrupted_one(tree, runs, run_a, control):
    path_a, a = run_a
    tol = control[1]
    _run(tree, runs / '00002-c', 18)
    step_b = _run(tree, runs / '00003-b', 18, resume_state=path_a)
    _, c = _file(runs / '00002-c')
    _, b = _file(runs / '00003-b')
    assert b['cur_nimg'] == c['cur_nimg'] == 36 and b['batch_idx'] == c['batch_idx'] == 18 and b['cur_tick'] == c['cur_tick'] == 5
    p = float(c['augment_pipe']['p'])
    print('augment p after 18 iterations:', p, 'after 6:', float(a['augment_pipe']['p']), 'ada_acc at the cut:', a['ranks'][0]['ada_acc'].tolist())
    assert p > 0                                               # or ADA never moved and this set-up tests nothing of it
    assert float(a['ranks'][0]['ada_acc'][1]) == 2 * BATCH      # two iterations of signs wait in the accumulator at the cut
    _spread('continued B against uninterrupted C', b, c)
    assert _beyond(b, c, tol) == []
    assert _diff(b, a) != [] and _differs_in(_diff(b, a), 'G') and _differs_in(_diff(b, a), 'opt')
    lines = [json.loads(line) for line in open(runs / '00003-b' / 'stats.jsonl')]
    assert [line['Progress/tick']['mean'] for line in lines] == [2, 3, 4]
    assert lines[0]['Timing/total_sec']['mean'] > a['elapsed_sec']
    assert [json.loads(line)['Progress/tick']['mean'] for line in open(runs / '00002-c' / 'stats.jsonl')] == [0, 1, 2, 3, 4]
    # the fused Adam's step counters are back on the device in their dtype; the buffer versions were left to the first iteration
    for phase in step_b.phases:
        steps = [s['step'] for s in phase.opt.state.values()]
        assert steps and all(t.device.type == 'cuda' and t.dtype == torch.float32 for t in steps)
        assert min(float(t) for t in steps) >= 18
    assert step_b._buf_versions != {}
    assert step_b.cur_nimg == 36 and step_b.batch_idx == 18


# ---- each item of the file is needed ----

def _fresh_cuda_rng(seed=0):
    keep = torch.cuda.get_rng_state('cuda')
    torch.cuda.manual_seed(seed)
    fresh = torch.cuda.get_rng_state('cuda')
    torch.cuda.set_rng_state(keep, 'cuda')
    return fresh


def _drop_opt(s):
    for opt in s['opt'].values():
        opt['state'] = {}


def _drop_batch_idx(s):
    s['batch_idx'] = 0


def _drop_cur_nimg(s):
    s['cur_nimg'] = 0


def _drop_cuda_rng(s):
    s['ranks'][0]['cuda_rng'] = _fresh_cuda_rng(s['random_seed'])


def _drop_ada(s):
    s['ranks'][0]['ada_acc'] = torch.zeros_like(s['ranks'][0]['ada_acc'])
    s['augment_pipe']['p'] = torch.zeros_like(s['augment_pipe']['p'])


@pytest.mark.parametrize('item, drop, entries', [
    ('opt', _drop_opt, ('G', 'D')),
    ('batch_idx', _drop_batch_idx, ('D',)),
    ('cur_nimg', _drop_cur_nimg, ('G_ema',)),
    ('cuda_rng', _drop_cuda_rng, ('G',)),
    ('sampler_skip', None, ('G',)),
    ('ada_acc_and_p', _drop_ada, ('augment_pipe/p',)),
])
def test_each_item_is_needed(tree, runs, run_a, control, two_more, monkeypatch, tmp_path, item, drop, entries):
    """A's file with one item reset to a fresh run's value, continued for two iterations, differs from the exact continuation in
    the entry the item feeds -- beyond the control's tolerance, where there is one.  (``sampler_skip`` is no entry of its own: the position is cur_nimg, so the data order is reset
    where the loop hands it to the sampler.)"""
    from training import train_state
    from training import training_loop_wo_flow_fullbody as loop
    path_a, a = run_a
    state = copy.deepcopy(a)
    if drop is not None:
        drop(state)
    else:
        real = loop._data_batches
        monkeypatch.setattr(loop, '_data_batches', lambda *args, **kwargs: real(*args, **dict(kwargs, cur_nimg=0)))
    path = str(tmp_path / 'training-state-000000.pt')
    train_state.save_state(path, None, state)
    _run(tree, runs / ('00020-without-' + item), state['cur_nimg'] // BATCH + 2, resume_state=path)
    _, got = _file(runs / ('00020-without-' + item))
    assert got['batch_idx'] == state['batch_idx'] + 2
    _spread('without ' + item + ' against the exact continuation', got, two_more)
    diff = _beyond(got, two_more, control[1])
    if item == 'ada_acc_and_p':
        # the finding of the module's docstring: in this set-up the reset values are as good as the real ones for two iterations
        # (and a third would change nothing: the next adjustment is after iteration 12)
        assert float(state['augment_pipe']['p']) == float(run_a[1]['augment_pipe']['p']) == 0 and float(run_a[1]['ranks'][0]['ada_acc'][0]) == 0
        assert float(run_a[1]['ranks'][0]['ada_acc'][1]) == 2 * BATCH and float(got['ranks'][0]['ada_acc'][1]) == 0
        assert diff == [], diff[:8]
        return
    assert _differs_in(diff, *entries), (item, diff[:8])


def test_restore_puts_every_entry_back(tree, runs, run_a, tmp_path):
    """A's file with the accumulator, p and the counters set to values no run here has, continued for no iteration at all
    (``total_kimg`` already reached): the state it writes back holds exactly those values, every other entry as in the file."""
    from training import train_state
    state = copy.deepcopy(run_a[1])
    state['ranks'][0]['ada_acc'] = torch.tensor([-3.0, 6.0])
    state['augment_pipe']['p'] = torch.tensor(0.37)
    path = str(tmp_path / 'training-state-000000.pt')
    train_state.save_state(path, None, state)
    step = _run(tree, runs / '00025-written-back', 6, resume_state=path)
    _, got = _file(runs / '00025-written-back')
    assert step._ada_acc.tolist() == [-3.0, 6.0] and float(step.augment_pipe.p) == float(torch.tensor(0.37))
    state['cur_tick'] += 1                      # the one maintenance round it ran ...
    # ... which moves the host generator on (measured: the only entry that differs; every run's maintenance does the same, so the
    # comparisons of whole runs above are not touched by it, and nothing in the step reads that generator)
    assert torch.equal(got['ranks'][0]['cuda_rng'], state['ranks'][0]['cuda_rng'])
    got['ranks'][0].pop('torch_rng'), state['ranks'][0].pop('torch_rng')
    assert _diff(got, state) == []


# ---- refusals ----

def test_refusals(tree, runs, run_a, tmp_path):
    from training import train_state
    path_a, a = run_a
    with pytest.raises(ValueError, match=r'batch_size=4.*batch_size=2'):
        _run(tree, runs / '00030-refused', 8, batch=4, resume_state=path_a)
    with pytest.raises(ValueError, match=r'random_seed=1.*random_seed=0'):
        _run(tree, runs / '00030-refused', 8, random_seed=1, resume_state=path_a)
    with pytest.raises(ValueError, match='resume_pkl'):
        _run(tree, runs / '00030-refused', 8, resume_state=path_a, resume_pkl=str(runs / '00000-a' / 'network-snapshot-000000.pkl'))
    from training.training_loop_wo_flow_fullbody import training_loop
    with pytest.raises(ValueError, match='run_dir'):
        training_loop(batch_size=BATCH, batch_gpu=BATCH, cfg=_cfg(), device=torch.device('cuda'), resume_state=path_a)
    state = copy.deepcopy(a)
    gone = 'synthesis.b16.conv1.weight' if 'synthesis.b16.conv1.weight' in state['G'] else sorted(state['G'])[0]
    del state['G'][gone]
    path = str(tmp_path / 'training-state-000000.pt')
    train_state.save_state(path, None, state)
    with pytest.raises(ValueError, match=gone.replace('.', r'\.')):
        _run(tree, runs / '00030-refused', 8, resume_state=path)
    assert not any(n.startswith('training-state-') for n in os.listdir(runs / '00030-refused'))


# ---- abort ----

def test_abort_writes_a_state_that_continues_to_the_same_run(tree, runs, run_a, control):
    _, a = run_a
    calls = []
    _run(tree, runs / '00040-aborted', 6, abort_fn=lambda: calls.append(1) or True)
    path, cut = _file(runs / '00040-aborted')
    assert calls == [1] and cut['batch_idx'] == 1 and cut['cur_nimg'] == BATCH and cut['cur_tick'] == 1
    assert 'network-snapshot-000000.pkl' in os.listdir(runs / '00040-aborted')
    _run(tree, runs / '00041-aborted-continued', 6, resume_state=path)
    _, got = _file(runs / '00041-aborted-continued')
    _spread('aborted and continued against A', got, a)
    assert _beyond(got, a, control[1]) == []


# ---- the command line, end to end ----

# train_wo_flow_fullbody.py's own main() in a fresh process, shrunk as tests/test_tryon_512_train_gpu.py shrinks it: test-size widths,
# a 3 x 3 grid, ticks of 3 iterations -- and --kimg N read as N ITERATIONS, since the command counts in thousands of images.
_TRAIN_SCRIPT = '''
import sys
import train_wo_flow_fullbody as T

real_loop = T.training_loop.training_loop

def small_loop(**kwargs):
    cfg = kwargs['cfg']
    cfg.G_kwargs.synthesis_kwargs.channel_base = cfg.D_kwargs.channel_base = 2048
    cfg.D_kwargs.epilogue_kwargs.mbstd_group_size = 2
    kwargs.update(total_kimg=kwargs['total_kimg'] * %d / 1000, kimg_per_tick=3 * %d / 1000, snapshot_gnum=3)
    return real_loop(**kwargs)

T.training_loop.training_loop = small_loop
T.main(sys.argv[1:], standalone_mode=False)
''' % (BATCH, BATCH)


def _process(cmd, seconds, **kwargs):
    r = subprocess.run(['timeout', '-k', '10', str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT, **kwargs)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_command_line_continue_equals_the_straight_command(tree, tmp_path, control):
    import legacy
    from training import train_state
    script = tmp_path / 'train_small.py'
    script.write_text(_TRAIN_SCRIPT)
    env = dict(os.environ, PYTHONPATH=PKG)
    common = ['--data', tree, '--gpus', '1', '--cfg', 'fashion', '--batch', str(BATCH), '--snap', '1', '--aug', 'noaug', '--fp32', 'true',
              '--l1_weight', '40', '--mask_weight', '20']
    cut, straight = tmp_path / 'cut', tmp_path / 'straight'
    out = _process([sys.executable, str(script), '--outdir', str(cut), *common, '--kimg', '3'], 600, env=env)
    assert '"save_state": true' in out
    (first,) = os.listdir(cut)
    assert _file(cut / first)[1]['batch_idx'] == 3
    out = _process([sys.executable, str(script), '--outdir', str(cut), '--data', tree, '--continue', str(cut / first), '--kimg', '6'], 600, env=env)
    assert 'Continuing from' in out
    (second,) = [d for d in os.listdir(cut) if d != first]
    assert second == '00001-' + first[len('00000-'):] + '-continue000000'
    _process([sys.executable, str(script), '--outdir', str(straight), *common, '--kimg', '6'], 600, env=env)
    (third,) = os.listdir(straight)
    _, got = _file(cut / second)
    _, want = _file(straight / third)
    assert got['batch_idx'] == want['batch_idx'] == 6 and got['cur_tick'] == want['cur_tick'] == 3 and 'augment_pipe' not in got
    recorded = json.loads(got['options'])
    assert recorded['resume_state'] == os.path.join(str(cut / first), 'training-state-000000.pt') and recorded['total_kimg'] == 6
    assert json.load(open(cut / second / 'training_options.json')) == recorded
    got.pop('options'), want.pop('options')        # the run directories and --kimg differ, nothing else may
    _spread('command line: continued against straight', got, want)
    assert _beyond(got, want, control[1]) == []
    with open(cut / second / 'network-snapshot-000000.pkl', 'rb') as f:
        data = legacy.load_network_pkl(f)           # test.py's loader
    assert sorted(data) == ['D', 'G', 'G_ema', 'augment_pipe', 'training_set_kwargs']
    for name in ('G', 'D', 'G_ema'):
        named = dict(list(data[name].named_parameters()) + list(data[name].named_buffers()))
        assert sorted(named) == sorted(got[name])
        assert all(torch.equal(named[k].detach().cpu(), got[name][k]) for k in named), name       # the snapshot and the state of one run


# ---- two ranks ----

def _two_rank_worker(rank, world, port, out, tree, root, tol):
    for p in (PKG, ROOT, os.path.join(ROOT, 'tests')):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from torch_utils import training_stats
        from training import train_state
        torch.cuda.set_device(0)
        dev = torch.device('cuda', 0)
        training_stats.init_multiprocessing(rank=rank, sync_device=dev)

        def run(name, iters, **kwargs):
            return _run(tree, os.path.join(root, name), iters, batch=2 * BATCH, num_gpus=world, rank=rank, device=dev,
                        kimg_per_tick=2 * 2 * BATCH / 1000, **kwargs)

        def live(step):
            s = {name: {k: t.detach().cpu().clone() for k, t in list(m.named_parameters()) + list(m.named_buffers())}
                 for name, m in (('G', step.G), ('D', step.D), ('G_ema', step.G_ema))}
            s['opt'] = train_state._plain({p.name[0]: p.opt.state_dict() for p in step.phases})
            s['ada_acc'], s['p'] = step._ada_acc.cpu().clone(), step.augment_pipe.p.cpu().clone()
            return s

        # ticks of 2 iterations close after iterations 1, 3, 5.  Rank 1 alone asks to stop at the second tick: both ranks stop there
        calls = []
        cut = run('00000-cut', 6, abort_fn=lambda: calls.append(1) or (rank == 1 and len(calls) == 2))
        assert calls == [1, 1] and cut.batch_idx == 3 and cut.cur_nimg == 3 * 2 * BATCH, (calls, cut.batch_idx)
        path = os.path.join(root, '00000-cut', 'training-state-000000.pt')
        state = train_state.load_state(path)
        assert len(state['ranks']) == world and state['batch_idx'] == 3 and state['cur_tick'] == 2 and state['num_gpus'] == world
        assert not torch.equal(state['ranks'][0]['torch_rng'], state['ranks'][1]['torch_rng'])          # seeded per rank
        assert not torch.equal(state['ranks'][0]['buffers']['G']['mapping.w_avg'], state['ranks'][1]['buffers']['G']['mapping.w_avg'])
        continued = live(run('00001-continued', 6, resume_state=path))
        straight = live(run('00002-straight', 6))
        _spread(f'rank {rank}, live: continued against straight', continued, straight)
        diff = _beyond(continued, straight, tol)
        assert diff == [], diff[:8]
        if rank == 0:
            diff = _beyond(_file(os.path.join(root, '00001-continued'))[1], _file(os.path.join(root, '00002-straight'))[1], tol)
            assert diff == [], diff[:8]
        out.put((rank, 'ok'))
    except Exception:  # noqa: BLE001
        import traceback
        out.put((rank, 'FAIL: ' + traceback.format_exc()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_continue_exactly_and_stop_together(tree, tmp_path, control):
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = 33000 + os.getpid() % 2000
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, out, tree, str(tmp_path), control[1])) for r in range(2)]
    for p in procs:
        p.start()
    results = [out.get(timeout=500) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    for rank, msg in results:
        assert msg == 'ok', f'rank {rank}: {msg}'
    assert [p.exitcode for p in procs] == [0, 0]
