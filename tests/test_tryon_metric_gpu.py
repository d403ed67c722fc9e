"""The swapped try-on metric (``tryon_full`` / ``tryon2k``) end to end on the tiny trees: what every block feeds G against
one ``swap_tensors`` call on the whole tree, the indifference of those inputs to the erase mask, the partials and the eighteen
results against the numpy restatement (tests/tryon_fidelity_ref.py) applied to G's own outputs, batch sizes and ranks, the hook
in the training loop with the command line on its snapshot, the 512 x 320 set, and training's own ``swap`` path unchanged.

Figures measured on an MI355X are in DESIGN.md section 8m."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_ref as R
import tryon_fidelity_ref as F
from conftest import ROOT
from train_grid_tree import PERSONS, make_tree
from tryon_512_train_tree import PERSONS as PERSONS_512, make_512_train_tree

pytestmark = pytest.mark.gpu

SSIM_TOL = R.SSIM_TOL           # the bound tests/test_region_stats_gpu.py holds pasta_region_image_stats to
SWAP_FP32 = ['swap_denorm_upper_input', 'swap_denorm_lower_input', 'swap_denorm_upper_mask', 'swap_denorm_lower_mask', 'swap_style_input']
SWAP_U8 = ['swap_denorm_upper', 'swap_denorm_lower']
# what generator_inputs names the five swapped tensors when it hands them to G
G_NAMES = dict(swap_denorm_upper_input='denorm_upper_input', swap_denorm_lower_input='denorm_lower_input',
               swap_denorm_upper_mask='denorm_upper_mask', swap_denorm_lower_mask='denorm_lower_mask', swap_style_input='c')
FIGURES, COUNTS = ('l1', 'psnr', 'share'), ('pairs', 'ssim_pairs')
BATCH = 2
ITERS_PER_TICK, TICKS = 3, 2


def _set_kwargs(tree, res=256):
    return dict(class_name='training.dataset.UvitonDatasetFull' + ('_512' if res == 512 else ''), path=tree)


@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    return {256: make_tree(tmp_path_factory.mktemp('tryon_metric_256')), 512: make_512_train_tree(tmp_path_factory.mktemp('tryon_metric_512'))}


@pytest.fixture(scope='module')
def generators():
    import dnnlib
    from training.training_loop_wo_flow_fullbody import fashion_config
    out = {}
    for res in (256, 512):
        torch.manual_seed(7)
        cfg = fashion_config(channel_base=2048, img_resolution=res)
        if res == 512:
            cfg.G_kwargs.patch_channels = 45
        out[res] = dnnlib.util.construct_class_by_name(**cfg.G_kwargs).eval().requires_grad_(False).cuda()
    return out


def _opts(G, set_kwargs, batch_size):
    from metrics import metric_utils
    return metric_utils.MetricOptions(G=G, dataset_kwargs=dict(set_kwargs, erase_masks='none'), num_gpus=1, rank=0, device=torch.device('cuda'),
                                      batch_size=batch_size)


def _scored(G, set_kwargs, batch_size):
    """``tryon_swapped.compute_partials`` with ``score_block`` recorded: (blocks as the metric fed them to G -- rows, raw_idx, G's
    keyword tensors, the two composites, the keep mask and the photographs of the scored rows, the people loaded --, partials,
    pixels)."""
    from metrics import tryon_swapped
    fed, real = [], tryon_swapped.score_block
    def recording(G, batch, raw_idx, rows, partials):
        n = len(rows)
        inputs = {k: v.clone() for k, v in tryon_swapped.generator_inputs(batch, n).items()}
        assert all(int(v.shape[0]) == n for v in inputs.values())
        fed.append(dict(rows=list(rows), raw_idx=list(raw_idx[:n]), inputs=inputs, loaded=batch.batch, keep=batch.stages['retain_mask'][:n].clone(),
                        image=batch.image[:n].clone(), **{k: batch.stages[k][:n].clone() for k in SWAP_U8}))
        return real(G, batch, raw_idx, rows, partials)
    tryon_swapped.score_block = recording
    try:
        partials, pixels = tryon_swapped.compute_partials(_opts(G, set_kwargs, batch_size))
    finally:
        tryon_swapped.score_block = real
    return fed, partials, pixels


def _fed_tensors(fed):
    """The seven swapped tensors per item, in item order."""
    assert [i for b in fed for i in b['rows']] == list(range(sum(len(b['rows']) for b in fed)))
    out = {k: torch.cat([b['inputs'][G_NAMES[k]] for b in fed]) for k in SWAP_FP32}
    out.update({k: torch.cat([b[k] for b in fed]) for k in SWAP_U8})
    return out


@pytest.fixture(scope='module')
def scored(trees, generators):
    """{batch size: _scored(...)} on the 256 tree, computed once."""
    return {b: _scored(generators[256], _set_kwargs(trees[256]), b) for b in (1, 2, 4, 9)}


def _whole_tree(set_kwargs):
    """One ``swap_tensors`` call on the whole tree built as a single batch, tables (i + 1) % M: the seven tensors."""
    import dnnlib
    from training import dataset as dataset_module, patch_pipeline, swap_outfits
    from training.tryon_batch import builder_for, shift_keypoints
    ds = dnnlib.util.construct_class_by_name(**set_kwargs)
    builder = builder_for(ds, torch.device('cuda'))
    raw = dataset_module.collate([ds[i] for i in range(len(ds))])
    batch = builder.build(raw, keep_stages=True)
    H = int(batch.tensors['real_img'].shape[2])
    keypoints = np.asarray(raw['keypoints'], np.float64)
    if builder.shifted:
        keypoints = shift_keypoints(keypoints, (H - int(raw['image'].shape[2])) // 2)
    _, back, valid = patch_pipeline.part_matrices(keypoints, H, H, builder.box_factor, x_pad=builder.x_pad, shin_fallback=builder.shin_fallback)
    roll = (np.arange(len(ds)) + 1) % len(ds)
    composites = {}
    out = swap_outfits.swap_tensors(batch.stages, back, valid, builder.lower_parts, roll, roll, composites=composites)
    assert sorted(out) == sorted(SWAP_FP32) and sorted(composites) == sorted(SWAP_U8)
    return dict(out, **composites), batch


# ---- 1. the inputs ----

@pytest.mark.parametrize('batch_size', [1, 2, 4, 9])
def test_every_block_feeds_g_the_whole_trees_rows(scored, trees, batch_size):
    fed, _, pixels = scored[batch_size]
    M = len(PERSONS)
    assert pixels == 256 * 192 and len(fed) == (M + batch_size - 1) // batch_size
    assert all(b['loaded'] == min(len(b['rows']) + 1, M) <= batch_size + 1 for b in fed) and [b['raw_idx'] for b in fed] == [b['rows'] for b in fed]
    want, whole = _whole_tree(dict(_set_kwargs(trees[256]), erase_masks='none'))
    got = _fed_tensors(fed)
    for key in SWAP_FP32 + SWAP_U8:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, key
        assert torch.equal(got[key], want[key]), (key, int((got[key] != want[key]).sum()))
    # the person's own tensors and what the regions are scored against
    assert torch.equal(torch.cat([b['inputs']['retain'] for b in fed]), whole.tensors['retain'])
    assert torch.equal(torch.cat([b['inputs']['pose'] for b in fed]), whole.tensors['pose'])
    assert torch.equal(torch.cat([b['keep'] for b in fed]), whole.stages['retain_mask']) and torch.equal(torch.cat([b['image'] for b in fed]), whole.image)
    # a swap it is: nobody wears their own garments
    assert not any(torch.equal(got['swap_denorm_upper'][i], whole.stages['denorm_upper'][i]) for i in range(M))


# ---- 2. the erase mask ----

def test_the_erase_mask_does_not_reach_the_swapped_tensors(scored, trees):
    import dnnlib
    from metrics import tryon_swapped
    from training import dataset as dataset_module
    from training.tryon_batch import builder_for
    ds = dnnlib.util.construct_class_by_name(**dict(_set_kwargs(trees[256]), erase_masks='files'))
    assert ds.erase_masks == 'files' and int(np.count_nonzero(ds[0]['erase_mask'])) > 0
    builder = builder_for(ds, torch.device('cuda'))
    fed = []
    for block in tryon_swapped.blocks(len(ds), 4):
        batch = tryon_swapped.prepare_block(builder, dataset_module.collate([ds[i] for i in block[1]]), block)
        n = len(block[0])
        fed.append(dict(rows=block[0], inputs=tryon_swapped.generator_inputs(batch, n), **{k: batch.stages[k][:n] for k in SWAP_U8}))
    with_files, without = _fed_tensors(fed), _fed_tensors(scored[4][0])
    for key in SWAP_FP32 + SWAP_U8:
        assert torch.equal(with_files[key], without[key]), key
    # while the paired inputs of the same batches do see it
    assert not torch.equal(batch.tensors['denorm_upper_input'], builder.build(dataset_module.collate(
        [dict(ds[i], erase_mask=np.zeros([1, 1], np.uint8)) for i in block[1]])).tensors['denorm_upper_input'])


# ---- 3. the metric against the restatement ----

def _restated(G, fed):
    """G run directly on what the blocks were fed, block by block, its bytes scored by tests/tryon_fidelity_ref.py: rows
    [M, 3, 5] of (sad, ssd, windows, bytes, ssim sum) in fp64 (the integers are far below 2^53)."""
    from training.tryon_pairs import images_to_u8
    rows = []
    for b in fed:
        z = torch.from_numpy(R.item_z(b['raw_idx'], G.z_dim)).cuda()
        with torch.no_grad():
            _, img, _ = G(z=z, noise_mode='const', **b['inputs'])
        h, w = int(b['image'].shape[1]), int(b['image'].shape[2])
        c0 = (h - w) // 2
        gen = images_to_u8(img.to(torch.float32), c0, w).cpu().numpy()
        content = lambda t: t[:, :, c0:c0 + w].cpu().numpy()
        regions = dict(keep=(content(b['keep']), b['image'].cpu().numpy()),
                       upper=(content(b['inputs']['denorm_upper_mask'][:, 0]), content(b['swap_denorm_upper'])),
                       lower=(content(b['inputs']['denorm_lower_mask'][:, 0]), content(b['swap_denorm_lower'])))
        per_region = []
        for region in F.REGIONS:
            mask, ref = regions[region]
            sad, ssd, windows, nbytes, ssim = F.region_stats(gen, ref, mask)
            per_region.append(np.stack([sad, ssd, windows, nbytes, ssim], axis=1).astype(np.float64))
        rows.append(np.stack(per_region, axis=1))
    return np.concatenate(rows)


def _check_against_restatement(G, set_kwargs, fed, partials, pixels, batch_size, count):
    """-> the largest deviation of a per-item mean SSIM from the restatement's."""
    from metrics import metric_main
    want_rows = _restated(G, fed)
    assert want_rows.shape == (count, 3, 5)
    want = F.finish(want_rows, pixels)
    # the tree gives every region pairs and SSIM windows: otherwise this test holds nothing
    assert all(want[r + '_pairs'] >= 1 and want[r + '_ssim_pairs'] >= 1 for r in F.REGIONS), want
    got_rows = partials.numpy()
    assert got_rows.shape == (count, 3, 5) and got_rows.dtype == np.int64
    assert np.array_equal(got_rows[:, :, :4], want_rows[:, :, :4].astype(np.int64))
    ssim_sum, windows = got_rows[:, :, 4].copy().view(np.float64), want_rows[:, :, 2]
    has = windows > 0
    assert np.all(ssim_sum[~has] == 0)
    deviation = float(np.abs(ssim_sum[has] / windows[has] - want_rows[:, :, 4][has] / windows[has]).max())
    print('batch %d: largest deviation of an item\'s mean SSIM over a region: %.3e (bound %.1e)' % (batch_size, deviation, SSIM_TOL))
    assert deviation <= SSIM_TOL
    r = metric_main.calc_metric('tryon_full', G=G, dataset_kwargs=set_kwargs, num_gpus=1, rank=0, device=torch.device('cuda'), batch_size=batch_size)
    assert r.metric == 'tryon_full' and r.num_gpus == 1
    assert sorted(r.results) == sorted('tryon_full_%s_%s' % (region, k) for region in F.REGIONS for k in FIGURES + ('ssim',) + COUNTS)
    print('tryon_full, batch %d:' % batch_size, dict(r.results))
    for region in F.REGIONS:
        for k in FIGURES:                                           # the same integers through a handful of fp64 operations
            assert r.results['tryon_full_%s_%s' % (region, k)] == pytest.approx(want['%s_%s' % (region, k)], rel=1e-12), (region, k)
        assert abs(r.results['tryon_full_%s_ssim' % region] - want[region + '_ssim']) <= SSIM_TOL, region
        for k in COUNTS:
            assert r.results['tryon_full_%s_%s' % (region, k)] == want['%s_%s' % (region, k)], (region, k)
    assert r.results['tryon_full_keep_pairs'] == count
    return deviation


@pytest.mark.parametrize('batch_size', [1, 2, 9])
def test_the_metric_equals_the_restatement(scored, trees, generators, batch_size):
    fed, partials, pixels = scored[batch_size]
    _check_against_restatement(generators[256], _set_kwargs(trees[256]), fed, partials, pixels, batch_size, len(PERSONS))


# ---- 4. batch size and ranks ----

def test_batch_size_moves_only_what_g_moves(scored):
    """Windows and bytes do not depend on G, so they -- and with them every share, pairs and ssim_pairs -- are equal across batch
    sizes.  What is left is G's own arithmetic between batch sizes: printed, not bounded."""
    from metrics import tryon_fidelity
    results = {b: tryon_fidelity.finish(scored[b][1], 'tryon_full', scored[b][2]) for b in (1, 2, 9)}
    for b in (2, 9):
        assert torch.equal(scored[b][1][:, :, 2:4], scored[1][1][:, :, 2:4])
        for key, v in results[b].items():
            if key.rsplit('_', 1)[1] in ('share', 'pairs') or key.endswith('_ssim_pairs'):
                assert v == results[1][key], (b, key)
        moved = (scored[b][1][:, :, 0] - scored[1][1][:, :, 0])
        print('batch', b, 'against batch 1: sum |d| moved per item and region by', moved.tolist(),
              {k: results[b][k] - results[1][k] for k in results[1] if k.rsplit('_', 1)[1] in ('l1', 'psnr', 'ssim') and not k.endswith('_ssim_pairs')})


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason='needs two GPUs')
def test_two_ranks_give_the_partials_of_one(trees, tmp_path):
    out = {}
    for gpus in (1, 2):
        script = tmp_path / ('partials%d.py' % gpus)
        script.write_text(_PARTIALS_SCRIPT)
        dst = tmp_path / ('partials%d.pt' % gpus)
        r = subprocess.run([sys.executable, str(script), trees[256], str(gpus), str(dst)], capture_output=True, text=True, timeout=900, cwd=ROOT,
                           env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, 'pasta-gan_amd')))
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        out[gpus] = torch.load(dst)
    one, two = out[1], out[2]
    assert tuple(one.shape) == (len(PERSONS), 3, 5) and bool((one[:, 0, 3] > 0).all())
    assert torch.equal(one[:, :, :4], two[:, :, :4])
    a, b = one[:, :, 4].contiguous().view(torch.float64), two[:, :, 4].contiguous().view(torch.float64)
    assert float(((a - b).abs() / a.abs().clamp(min=1e-300)).max()) <= 1e-12


# One process per GPU computes the combined partials at batch 2 (five blocks on the tiny tree: three and two per rank); rank 0 saves them.
_PARTIALS_SCRIPT = '''
import os, sys, tempfile
import torch

def work(rank, tree, gpus, dst, init):
    import dnnlib
    from metrics import metric_utils, tryon_swapped
    from training.training_loop_wo_flow_fullbody import fashion_config
    if gpus > 1:
        torch.distributed.init_process_group(backend='nccl', init_method='file://' + init, rank=rank, world_size=gpus)
    device = torch.device('cuda', rank)
    torch.cuda.set_device(device)
    torch.manual_seed(7)
    G = dnnlib.util.construct_class_by_name(**fashion_config(channel_base=2048).G_kwargs).eval().requires_grad_(False).to(device)
    opts = metric_utils.MetricOptions(G=G, dataset_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree, erase_masks='none'),
                                      num_gpus=gpus, rank=rank, device=device, batch_size=2)
    partials, _ = tryon_swapped.compute_partials(opts)
    if rank == 0:
        torch.save(partials, dst)
    if gpus > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()

if __name__ == '__main__':
    tree, gpus, dst = sys.argv[1], int(sys.argv[2]), sys.argv[3]
    with tempfile.TemporaryDirectory() as tmp:
        if gpus == 1:
            work(0, tree, 1, dst, None)
        else:
            torch.multiprocessing.spawn(fn=work, args=(tree, gpus, dst, os.path.join(tmp, 'init')), nprocs=gpus)
'''


# ---- 5. tryon2k ----

def test_tryon2k_on_a_small_tree_is_tryon_full(trees, generators):
    from metrics import metric_main
    kwargs = dict(G=generators[256], dataset_kwargs=_set_kwargs(trees[256]), num_gpus=1, rank=0, device=torch.device('cuda'))
    full, sub = metric_main.calc_metric('tryon_full', **kwargs).results, metric_main.calc_metric('tryon2k', **kwargs).results
    assert len(full) == 18 and all(np.isfinite(v) for v in full.values())
    assert {k[len('tryon2k'):]: v for k, v in sub.items()} == {k[len('tryon_full'):]: v for k, v in full.items()}


# ---- 6. the loop and the command ----

def _run(tree, run_dir, **kwargs):
    from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
    os.makedirs(run_dir)
    cfg = fashion_config(channel_base=2048, mbstd_group_size=2)
    return training_loop(batch_size=BATCH, batch_gpu=BATCH, cfg=cfg, device=torch.device('cuda'), training_set_kwargs=_set_kwargs(tree),
                         data_loader_kwargs=dict(num_workers=0, pin_memory=True), run_dir=str(run_dir),
                         total_kimg=TICKS * ITERS_PER_TICK * BATCH / 1000, kimg_per_tick=ITERS_PER_TICK * BATCH / 1000,
                         image_snapshot_ticks=None, network_snapshot_ticks=1, snapshot_gnum=6, **kwargs)


def test_the_loop_writes_both_files_and_the_command_reproduces_the_last_line(trees, tmp_path):
    run_dir = tmp_path / '00000-run'
    _run(trees[256], run_dir, metrics=['recon_full', 'tryon_full'])
    snapshots = len(open(run_dir / 'stats.jsonl').readlines())          # network_snapshot_ticks = 1: one snapshot per tick
    assert sorted(n for n in os.listdir(run_dir) if n.startswith('metric-')) == ['metric-recon_full.jsonl', 'metric-tryon_full.jsonl']
    assert len(open(run_dir / 'metric-recon_full.jsonl').readlines()) == snapshots >= TICKS
    lines = [json.loads(line) for line in open(run_dir / 'metric-tryon_full.jsonl')]
    assert len(lines) == snapshots
    for line in lines:
        assert line['metric'] == 'tryon_full' and line['num_gpus'] == 1 and line['snapshot_pkl'] == 'network-snapshot-000000.pkl'
        assert len(line['results']) == 18 and line['results']['tryon_full_keep_pairs'] == len(PERSONS)
        assert all(np.isfinite(line['results']['tryon_full_keep_' + k]) for k in ('l1', 'psnr', 'ssim', 'share')), line
    cmd = [sys.executable, os.path.join(ROOT, 'pasta-gan_amd', 'calc_metrics.py'), '--network', str(run_dir / 'network-snapshot-000000.pkl'),
           '--metrics', 'tryon_full', '--verbose', 'false']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    printed = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(printed) == 1 and printed[0]['metric'] == 'tryon_full'
    assert json.dumps(printed[0]['results']) == json.dumps(lines[-1]['results'])         # NaN-proof equality, key order included
    # the run directory was made by training_loop alone (no training_options.json): the command only prints
    assert len(open(run_dir / 'metric-tryon_full.jsonl').readlines()) == snapshots


def test_a_loop_without_metrics_writes_no_metric_file(trees, tmp_path):
    run_dir = tmp_path / '00001-plain'
    _run(trees[256], run_dir, metrics=None)
    names = os.listdir(run_dir)
    assert 'network-snapshot-000000.pkl' in names and 'stats.jsonl' in names and not [n for n in names if n.startswith('metric-')]


# ---- 7. 512 x 320 ----

def test_the_metric_equals_the_restatement_at_512(trees, generators):
    """Five people in blocks of two: the last block holds one person, whose donor is the first of the tree."""
    from training.tryon_regions import FullBodyRegionBatchBuilder
    from training import tryon_batch
    set_kwargs = _set_kwargs(trees[512], 512)
    G = generators[512]
    assert G.patch_channels == 45
    fed, partials, pixels = _scored(G, set_kwargs, 2)
    assert pixels == 512 * 320 and [b['rows'] for b in fed] == [[0, 1], [2, 3], [4]] and [b['loaded'] for b in fed] == [3, 3, 2]
    assert int(fed[0]['inputs']['c'].shape[1]) == 45 and tuple(fed[0]['image'].shape[1:]) == (512, 320, 3)
    import dnnlib
    assert isinstance(tryon_batch.builder_for(dnnlib.util.construct_class_by_name(**set_kwargs), 'cuda'), FullBodyRegionBatchBuilder)
    want, _ = _whole_tree(dict(set_kwargs, erase_masks='none'))
    got = _fed_tensors(fed)
    for key in SWAP_FP32 + SWAP_U8:
        assert torch.equal(got[key], want[key]), key
    _check_against_restatement(G, set_kwargs, fed, partials, pixels, 2, len(PERSONS_512))


# ---- 8. training is unchanged ----

@pytest.mark.parametrize('res', [256, 512])
def test_trainings_swap_is_what_it_was(trees, res):
    """Without ``keep_stages`` the batch is the fifteen tensors, bit for bit those of ``swap_tensors`` called directly with the
    donor rule's tables, and no stage is kept; with it the stages carry the two composites."""
    import dnnlib
    from training import dataset as dataset_module, patch_pipeline, swap_outfits
    from training.tryon_batch import FullBodyBatch, builder_for, shift_keypoints
    ds = dnnlib.util.construct_class_by_name(**_set_kwargs(trees[res], res))
    builder = builder_for(ds, torch.device('cuda'))
    n = 4
    raw = dataset_module.collate([ds[i] for i in range(n)])
    batch = builder.build(raw, swap=dict(region='fullbody', group=n))
    assert batch.stages is None and list(batch.tensors) == FullBodyBatch.KEYS + swap_outfits.SWAP_KEYS and len(batch.tensors) == 15
    kept = builder.build(raw, keep_stages=True)
    assert not any(k in kept.stages for k in SWAP_U8)
    H = int(kept.tensors['real_img'].shape[2])
    keypoints = np.asarray(raw['keypoints'], np.float64)
    if builder.shifted:
        keypoints = shift_keypoints(keypoints, (H - int(raw['image'].shape[2])) // 2)
    _, back, valid = patch_pipeline.part_matrices(keypoints, H, H, builder.box_factor, x_pad=builder.x_pad, shin_fallback=builder.shin_fallback)
    upper_src, lower_src = swap_outfits.source_tables(n, n, 'fullbody')
    composites = {}
    want = swap_outfits.swap_tensors(kept.stages, back, valid, builder.lower_parts, upper_src, lower_src, composites=composites)
    assert list(want) == swap_outfits.SWAP_OUTPUTS
    for key in FullBodyBatch.KEYS:
        assert torch.equal(batch.tensors[key], kept.tensors[key]), key
    for key in swap_outfits.SWAP_OUTPUTS:
        assert torch.equal(batch.tensors[key], want[key]), key
    assert torch.equal(batch.tensors['swap_keep'], kept.stages['retain_mask'])
    # explicit tables through the builder are the same call; kept stages then hold the composites
    both = builder.build(raw, keep_stages=True, swap=dict(upper_src=upper_src, lower_src=lower_src))
    assert sorted(set(both.stages) - set(kept.stages)) == sorted(SWAP_U8)
    for key in swap_outfits.SWAP_KEYS:
        assert torch.equal(both.tensors[key], batch.tensors[key]), key
    for key in SWAP_U8:
        assert torch.equal(both.stages[key], composites[key]) and both.stages[key].dtype == torch.uint8, key
    with pytest.raises(ValueError, match='does not name one of the 4 samples'):
        builder.build(raw, swap=dict(upper_src=[1, 2, 3, 4], lower_src=[1, 2, 3, 0]))
