"""The reconstruction metric end to end on the tiny tree: ``calc_metric`` against the numpy restatement applied to G_ema's own
outputs, its independence of the batch size, the hook in the training loop, and the command line on a written snapshot.

Figures measured on an MI355X are in DESIGN.md ("Scoring snapshots")."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_ref as R
from conftest import ROOT
from train_grid_tree import PERSONS, make_tree

pytestmark = pytest.mark.gpu

KEYS = ('l1', 'psnr', 'ssim', 'miou', 'pixacc')
SSIM_TOL = R.SSIM_TOL
BATCH = 2
ITERS_PER_TICK, TICKS = 3, 2


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('calc_metrics'))


def _set_kwargs(tree):
    return dict(class_name='training.dataset.UvitonDatasetFull', path=tree)


@pytest.fixture(scope='module')
def generator():
    import dnnlib
    from training.training_loop_wo_flow_fullbody import fashion_config
    torch.manual_seed(7)
    cfg = fashion_config(channel_base=2048)
    return dnnlib.util.construct_class_by_name(**cfg.G_kwargs).eval().requires_grad_(False).cuda()


def _calc(G, tree, **kwargs):
    from metrics import metric_main
    return metric_main.calc_metric('recon_full', G=G, dataset_kwargs=_set_kwargs(tree), num_gpus=1, rank=0, device=torch.device('cuda'),
                                   **kwargs)


def _oracle_sums(G, tree, batch_size):
    """G run directly on FullBodyBatchBuilder batches of ``batch_size`` in data set order, its outputs scored by tests/recon_ref.py:
    (per-item sad, ssd, SSIM sum, windows, bytes; the summed confusion matrix).  z by the rule restated in recon_ref.item_z."""
    import dnnlib
    from training import dataset as dataset_module
    from training.tryon_batch import FullBodyBatchBuilder
    from training.tryon_pairs import images_to_u8
    dataset = dnnlib.util.construct_class_by_name(**_set_kwargs(tree))
    builder = FullBodyBatchBuilder(torch.device('cuda'))
    rows, conf = [], 0
    for lo in range(0, len(dataset), batch_size):
        raw = dataset_module.collate([dataset[i] for i in range(lo, min(lo + batch_size, len(dataset)))])
        batch = builder.build(raw)
        t = batch.tensors
        z = torch.from_numpy(R.item_z(raw['raw_idx'].tolist(), G.z_dim)).cuda()
        with torch.no_grad():
            _, img, parsing = G(z=z, c=t['style_input'], retain=t['retain'], pose=t['pose'], denorm_upper_input=t['denorm_upper_input'],
                                denorm_lower_input=t['denorm_lower_input'], denorm_upper_mask=t['denorm_upper_mask'],
                                denorm_lower_mask=t['denorm_lower_mask'], noise_mode='const')
        photos = raw['image'].numpy()
        h, w = photos.shape[1], photos.shape[2]
        gen = images_to_u8(img.to(torch.float32), (h - w) // 2, w).cpu().numpy()
        sad, ssd, ssim, windows = R.image_stats(gen, photos)
        rows += [(a, b, c, d, h * w * 3) for a, b, c, d in zip(sad, ssd, ssim, windows)]
        conf = conf + R.confusion(parsing.float().cpu().numpy(), t['gt_parsing'].cpu().numpy(), (h - w) // 2, w)
    return tuple(np.array(col) for col in zip(*rows)), conf


def _partials(G, tree, batch_size):
    from metrics import metric_utils, reconstruction
    opts = metric_utils.MetricOptions(G=G, dataset_kwargs=_set_kwargs(tree), num_gpus=1, rank=0, device=torch.device('cuda'),
                                      batch_size=batch_size)
    return reconstruction.compute_partials(opts)


@pytest.mark.parametrize('batch_size', [1, 2, 4, 9])
def test_calc_metric_equals_the_oracle(generator, tree, batch_size):
    """At every batch size the metric scores exactly what G returns at that batch size: the integer sums and the confusion
    matrix are the oracle's, the SSIM sums within the kernel's bound, and the five figures follow."""
    (sad, ssd, ssim, windows, nbytes), conf = _oracle_sums(generator, tree, batch_size)
    assert len(sad) == len(PERSONS)
    p = _partials(generator, tree, batch_size)
    items = p['items'].numpy()
    assert items[:, 0].tolist() == sad.tolist() and items[:, 1].tolist() == ssd.tolist()
    assert items[:, 2].tolist() == windows.tolist() and items[:, 3].tolist() == nbytes.tolist()
    assert np.array_equal(p['confusion'].numpy(), conf)
    assert np.abs(items[:, 4].copy().view(np.float64) / windows - ssim / windows).max() <= SSIM_TOL
    want = R.results(sad, ssd, ssim, windows, nbytes, conf)
    r = _calc(generator, tree, batch_size=batch_size)
    assert sorted(r) == ['metric', 'num_gpus', 'results', 'total_time', 'total_time_str'] and r.metric == 'recon_full' and r.num_gpus == 1
    assert sorted(r.results) == sorted('recon_full_' + k for k in KEYS)
    got = {k: r.results['recon_full_' + k] for k in KEYS}
    print('recon_full on the tiny tree, batch %d:' % batch_size, got, 'oracle:', want)
    assert all(np.isfinite(v) for v in got.values())
    for k in ('l1', 'psnr', 'miou', 'pixacc'):                      # the same integers through a handful of fp64 operations
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    assert abs(got['ssim'] - want['ssim']) <= SSIM_TOL
    assert 0 < got['l1'] < 1 and 0 < got['psnr'] < 100 and -1 <= got['ssim'] < 1 and 0 <= got['miou'] <= got['pixacc'] <= 1


# Ten times the largest deviation from batch size 1 observed on an MI355X: l1 1.2e-8, psnr 2.2e-7 dB,
# ssim 7.3e-8; the confusion matrix did not change at all.
CROSS_BATCH_TOL = dict(l1=1.2e-7, psnr=2.2e-6, ssim=7.3e-7)


def test_result_does_not_depend_on_the_batch_size(generator, tree):
    """z is drawn per item and every item owns its row of the partials, and the test above shows that at each batch size the
    metric is exact on what G returns: what is left between batch sizes is G's own arithmetic.  Observed on an MI355X: G's
    image moves a few bytes by one step between batch sizes (see CROSS_BATCH_TOL), the arg-max of its parsing nowhere, so the
    parsing figures are held to equality and the image figures to ten times what was observed."""
    parts = {b: _partials(generator, tree, b) for b in (1, 2, 9)}
    results = {b: _calc(generator, tree, batch_size=b).results for b in (1, 2, 9)}
    for b in (2, 9):
        moved = (parts[b]['items'][:, 0] - parts[1]['items'][:, 0]).tolist()
        print('batch', b, 'against batch 1:', {k: results[b]['recon_full_' + k] - results[1]['recon_full_' + k] for k in KEYS},
              'sum |d| per item moved by', moved, 'confusion cells moved:', int((parts[b]['confusion'] != parts[1]['confusion']).sum()))
        assert torch.equal(parts[b]['confusion'], parts[1]['confusion'])
        assert torch.equal(parts[b]['items'][:, 2:4], parts[1]['items'][:, 2:4])
        for k in ('miou', 'pixacc'):
            assert results[b]['recon_full_' + k] == results[1]['recon_full_' + k], (b, k)
        for k, tol in CROSS_BATCH_TOL.items():
            assert abs(results[b]['recon_full_' + k] - results[1]['recon_full_' + k]) <= tol, (b, k)


def test_recon2k_on_a_small_tree_is_recon_full(generator, tree):
    from metrics import metric_main
    full = _calc(generator, tree).results
    sub = metric_main.calc_metric('recon2k', G=generator, dataset_kwargs=_set_kwargs(tree), num_gpus=1, rank=0, device=torch.device('cuda')).results
    assert {k[len('recon2k'):]: v for k, v in sub.items()} == {k[len('recon_full'):]: v for k, v in full.items()}


# ---- the training loop ----

def _run(tree, run_dir, **kwargs):
    from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
    os.makedirs(run_dir)
    cfg = fashion_config(channel_base=2048, mbstd_group_size=2)
    return training_loop(batch_size=BATCH, batch_gpu=BATCH, cfg=cfg, device=torch.device('cuda'), training_set_kwargs=_set_kwargs(tree),
                         data_loader_kwargs=dict(num_workers=0, pin_memory=True), run_dir=str(run_dir),
                         total_kimg=TICKS * ITERS_PER_TICK * BATCH / 1000, kimg_per_tick=ITERS_PER_TICK * BATCH / 1000,
                         image_snapshot_ticks=None, network_snapshot_ticks=1, snapshot_gnum=6, **kwargs)


@pytest.fixture(scope='module')
def run(tree, tmp_path_factory):
    run_dir = tmp_path_factory.mktemp('metric_runs') / '00000-run'
    step = _run(tree, run_dir, metrics=['recon_full'])
    return step, run_dir


def test_training_run_reports_every_snapshot(run):
    step, run_dir = run
    snapshots = len(open(run_dir / 'stats.jsonl').readlines())      # network_snapshot_ticks = 1: one snapshot per tick
    lines = [json.loads(line) for line in open(run_dir / 'metric-recon_full.jsonl')]
    assert len(lines) == snapshots >= TICKS
    for line in lines:
        assert line['metric'] == 'recon_full' and line['num_gpus'] == 1 and line['snapshot_pkl'] == 'network-snapshot-000000.pkl'
        assert sorted(line['results']) == sorted('recon_full_' + k for k in KEYS)
        assert all(np.isfinite(v) for v in line['results'].values()), line
        assert 'timestamp' in line and 'total_time' in line and 'total_time_str' in line
    assert [n for n in os.listdir(run_dir) if n.startswith('metric-')] == ['metric-recon_full.jsonl']


def test_training_run_without_metrics_writes_no_metric_file(tree, tmp_path):
    run_dir = tmp_path / '00001-plain'
    _run(tree, run_dir, metrics=None)
    names = os.listdir(run_dir)
    assert 'network-snapshot-000000.pkl' in names and 'stats.jsonl' in names
    assert not [n for n in names if n.startswith('metric-')]


def test_command_line_reproduces_the_loop(run):
    step, run_dir = run
    in_loop = [json.loads(line) for line in open(run_dir / 'metric-recon_full.jsonl')][-1]
    cmd = [sys.executable, os.path.join(ROOT, 'pasta-gan_amd', 'calc_metrics.py'), '--network', str(run_dir / 'network-snapshot-000000.pkl'),
           '--metrics', 'recon_full', '--verbose', 'false']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1 and lines[0]['metric'] == 'recon_full'
    assert lines[0]['results'] == in_loop['results']
    # the run directory was made by training_loop alone (no training_options.json): the command only prints
    assert len(open(run_dir / 'metric-recon_full.jsonl').readlines()) == len(open(run_dir / 'stats.jsonl').readlines())


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')
def test_two_gpus_give_the_sums_of_one(run, tmp_path):
    step, run_dir = run
    out = {}
    for gpus in (1, 2):
        script = tmp_path / ('partials%d.py' % gpus)
        script.write_text(_PARTIALS_SCRIPT)
        dst = tmp_path / ('partials%d.pt' % gpus)
        r = subprocess.run([sys.executable, str(script), str(run_dir / 'network-snapshot-000000.pkl'), str(gpus), str(dst)], capture_output=True,
                           text=True, timeout=900, cwd=ROOT, env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'pasta-gan_amd')))
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        out[gpus] = torch.load(dst)
    one, two = out[1], out[2]
    assert torch.equal(one['items'][:, :4], two['items'][:, :4]) and torch.equal(one['confusion'], two['confusion'])
    a, b = one['items'][:, 4].contiguous().view(torch.float64), two['items'][:, 4].contiguous().view(torch.float64)
    assert float(((a - b).abs() / a.abs()).max()) <= 1e-12
    # and through the command itself
    lines = {}
    for gpus in (1, 2):
        cmd = [sys.executable, os.path.join(ROOT, 'pasta-gan_amd', 'calc_metrics.py'), '--network', str(run_dir / 'network-snapshot-000000.pkl'),
               '--gpus', str(gpus), '--verbose', 'false']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        lines[gpus] = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')][-1]
    assert lines[2]['num_gpus'] == 2
    for k, v in lines[1]['results'].items():
        assert lines[2]['results'][k] == pytest.approx(v, rel=1e-12), k


# One process per GPU computes the combined partials of the snapshot and rank 0 saves them.
_PARTIALS_SCRIPT = '''
import os, sys, tempfile
import torch

def work(rank, pkl, gpus, dst, init):
    import legacy
    from metrics import metric_utils, reconstruction
    if gpus > 1:
        torch.distributed.init_process_group(backend='nccl', init_method='file://' + init, rank=rank, world_size=gpus)
    device = torch.device('cuda', rank)
    torch.cuda.set_device(device)
    with open(pkl, 'rb') as f:
        data = legacy.load_network_pkl(f)
    opts = metric_utils.MetricOptions(G=data['G_ema'], dataset_kwargs=data['training_set_kwargs'], num_gpus=gpus, rank=rank, device=device)
    partials = reconstruction.compute_partials(opts)
    if rank == 0:
        torch.save(partials, dst)
    if gpus > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()

if __name__ == '__main__':
    pkl, gpus, dst = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    with tempfile.TemporaryDirectory() as tmp:
        if gpus == 1:
            work(0, pkl, 1, dst, None)
        else:
            torch.multiprocessing.spawn(fn=work, args=(pkl, gpus, dst, os.path.join(tmp, 'init')), nprocs=gpus)
'''
