"""A whole training run on the tiny tree (training_loop with a run directory): the files the reference's loop leaves, a snapshot
that loads and reproduces the in-memory generator, the sample image against the numpy restatement of save_image_grid, resuming,
aborting -- and the unchanged behaviour without a run directory."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch

import train_grid_ref as G
from train_grid_tree import make_tree

pytestmark = pytest.mark.gpu

GNUM, BATCH = 6, 2
ITERS_PER_TICK, TICKS = 3, 2


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('train_run'))


def _loop(tree, **kwargs):
    from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
    cfg = fashion_config(channel_base=2048, mbstd_group_size=2)
    return training_loop(batch_size=BATCH, batch_gpu=BATCH, cfg=cfg, device=torch.device('cuda'),
                         training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree),
                         data_loader_kwargs=dict(num_workers=0, pin_memory=True), **kwargs)


def _run(tree, run_dir, **kwargs):
    os.makedirs(run_dir)
    args = dict(run_dir=str(run_dir), total_kimg=TICKS * ITERS_PER_TICK * BATCH / 1000, kimg_per_tick=ITERS_PER_TICK * BATCH / 1000,
                image_snapshot_ticks=1, network_snapshot_ticks=1, snapshot_gnum=GNUM)
    args.update(kwargs)
    return _loop(tree, **args)


@pytest.fixture(scope='module')
def run(tree, tmp_path_factory):
    run_dir = tmp_path_factory.mktemp('runs') / '00000-run'
    progress = []
    step = _run(tree, run_dir, progress_fn=lambda cur, total: progress.append((cur, total)))
    return step, run_dir, progress


def _state(module):
    from torch_utils import misc
    return {name: t.detach().cpu() for name, t in misc.named_params_and_buffers(module)}


def _same(a, b):
    sa, sb = _state(a), _state(b)
    assert sorted(sa) == sorted(sb)
    for name in sa:
        assert torch.equal(sa[name], sb[name]), name


def _load(path):
    import legacy
    with open(path, 'rb') as f:
        return legacy.load_network_pkl(f)


def test_files_of_a_run(run):
    step, run_dir, progress = run
    names = sorted(os.listdir(run_dir))
    # tick 0 closes after the first iteration (the reference's rule), so the two further ticks make three maintenance rounds
    lines = [json.loads(line) for line in open(run_dir / 'stats.jsonl')]
    fakes = [n for n in names if n.startswith('fakes') and n.endswith('_finetune.png')]
    pkls = [n for n in names if n.startswith('network-snapshot-') and n.endswith('.pkl')]
    ticks = len(lines)
    assert ticks >= TICKS and step.cur_nimg == TICKS * ITERS_PER_TICK * BATCH
    for line in lines:
        assert 'Progress/kimg' in line and 'Timing/sec_per_tick' in line and 'timestamp' in line
        losses = {k: v for k, v in line.items() if k.startswith('Loss/')}
        assert losses and all(np.isfinite(v['mean']) and v['num'] > 0 for v in losses.values()), sorted(losses)
    assert [line['Progress/tick']['mean'] for line in lines] == list(range(ticks))
    for name in ('init_denorm_upper.png', 'init_denorm_lower.png', 'init_retain.png'):
        assert name in names and PIL.Image.open(run_dir / name).size == ((GNUM + 1) * 256, (GNUM + 1) * 256)
    # kimg is far below 1 here, so every tick writes the same file names: one image and one snapshot file, rewritten per tick
    assert fakes == ['fakes000000_finetune.png'] and pkls == ['network-snapshot-000000.pkl']
    assert PIL.Image.open(run_dir / fakes[0]).size == ((GNUM + 1) * 256, (GNUM + 1) * 256)
    assert progress[0] == (0, TICKS * ITERS_PER_TICK * BATCH / 1000) and len(progress) == ticks + 1


def test_snapshot_loads_and_reproduces_g_ema(run):
    step, run_dir, _ = run
    data = _load(run_dir / 'network-snapshot-000000.pkl')
    assert sorted(data) == ['D', 'G', 'G_ema', 'augment_pipe', 'training_set_kwargs']
    _same(data['G_ema'], step.G_ema)
    _same(data['G'], step.G)
    _same(data['D'], step.D)
    grid = step.snapshot_grid
    inputs = grid.inputs(0, BATCH)
    with torch.no_grad():
        want = step.G_ema(z=step.grid_z[0], **inputs, noise_mode='const')[1]
        got = data['G_ema'].to('cuda')(z=step.grid_z[0], **inputs, noise_mode='const')[1]
    assert torch.equal(got, want)


def test_sample_image_equals_save_image_grid(run):
    from training.training_loop_wo_flow_fullbody import sample_images
    step, run_dir, _ = run
    grid = step.snapshot_grid
    images = torch.cat(list(sample_images(step.G_ema, grid, step.grid_z, BATCH))).cpu().numpy()
    assert images.shape == (GNUM * GNUM, 3, 256, 256) and np.isfinite(images).all()
    people = (grid.image.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1).cpu().numpy()          # :121, :364
    side, top = G.frame(people)
    want = G.save_image_grid(side, top, images, [-1, 1], (GNUM, GNUM))
    got = np.array(PIL.Image.open(run_dir / 'fakes000000_finetune.png'))
    assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    assert len(np.unique(want[256:, 256:])) > 8          # a picture, not a constant


def test_resume_restores_the_snapshot(run, tree, tmp_path):
    _, run_dir, _ = run
    pkl = run_dir / 'network-snapshot-000000.pkl'
    data = _load(pkl)
    step = _run(tree, tmp_path / '00001-resumed', resume_pkl=str(pkl), total_kimg=0, random_seed=5)
    assert step.cur_nimg == 0
    for name in ('G', 'D', 'G_ema'):
        _same(getattr(step, name), data[name])
    again = _load(tmp_path / '00001-resumed' / 'network-snapshot-000000.pkl')
    _same(again['G_ema'], data['G_ema'])


def test_abort_after_the_first_tick(tree, tmp_path):
    run_dir = tmp_path / '00002-aborted'
    calls = []
    step = _run(tree, run_dir, abort_fn=lambda: calls.append(1) or True, image_snapshot_ticks=100, network_snapshot_ticks=100)
    assert calls == [1] and step.cur_nimg == BATCH        # tick 0 ends after one iteration
    names = os.listdir(run_dir)
    assert 'fakes000000_finetune.png' in names and 'network-snapshot-000000.pkl' in names
    assert len(open(run_dir / 'stats.jsonl').readlines()) == 1


def test_without_a_run_directory_nothing_is_written(tree, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    progress = []
    step = _loop(tree, total_iters=2, progress_fn=lambda cur, total: progress.append((cur, total)))
    assert step.cur_nimg == 2 * BATCH and progress == [(1, 2), (2, 2)]
    assert os.listdir(tmp_path) == [] and not hasattr(step, 'snapshot_grid')
