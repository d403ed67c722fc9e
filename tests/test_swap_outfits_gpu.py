"""Training on swapped outfits: the swapped inputs of a batch against the sample grid's cells, bit for bit, at 256 and
at 512; what a batch carries with and without the option; the unpaired pass of ``StyleGAN2Loss(swap_weight=)`` on stand-in
networks; and one run of train_wo_flow_fullbody.py with ``--swap_weight``, continued once."""
import copy
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import PKG, ROOT
from train_grid_tree import make_tree
from tryon_512_train_tree import make_512_train_tree

pytestmark = pytest.mark.gpu

SWAP_FP32 = ['swap_denorm_upper_input', 'swap_denorm_lower_input', 'swap_denorm_upper_mask', 'swap_denorm_lower_mask', 'swap_style_input']
SWAP_KEYS = SWAP_FP32 + ['swap_keep']


# ---- the swapped inputs ----

@pytest.fixture(scope='module')
def sets(tmp_path_factory):
    """{resolution: (data set, its training builder)} on the tiny trees."""
    from training.dataset import UvitonDatasetFull, UvitonDatasetFull_512
    from training.tryon_batch import builder_for
    a = UvitonDatasetFull(make_tree(tmp_path_factory.mktemp('swap_256')))
    b = UvitonDatasetFull_512(make_512_train_tree(tmp_path_factory.mktemp('swap_512')))
    return {256: (a, builder_for(a, 'cuda')), 512: (b, builder_for(b, 'cuda'))}


def _raw(ds, count):
    from training.dataset import collate
    return collate([ds[i] for i in list(ds.vis_index)[:count]])


@pytest.mark.parametrize('res', [256, 512])
def test_the_swapped_tensors_are_the_grids_cells(sets, res, monkeypatch):
    """Three people, one group.  With gnum = 3 the grid's row 0 swaps the lower garment, row 1 the whole outfit and row 2 the upper
    one; its cells 1, 5, 6 are rows 0, 1, 2 with the donor rule's columns 1, 2, 0."""
    from training import patch_pipeline, swap_outfits
    from training.snapshot_grid import SnapshotGrid
    ds, builder = sets[res]
    assert type(builder).__name__ == ('FullBodyBatchBuilder' if res == 256 else 'FullBodyRegionBatchBuilder')
    raw = _raw(ds, 3)
    solved = []
    real = patch_pipeline.part_matrices
    monkeypatch.setattr(patch_pipeline, 'part_matrices', lambda *a, **k: (solved.append(len(a[0])), real(*a, **k))[1])
    batch = builder.build(raw, keep_stages=True, swap=dict(region='fullbody', group=3))
    assert solved == [3]                                     # the people's 8 x 8 systems are solved once per build
    monkeypatch.undo()

    # the low-level function with arbitrary tables, on the matrices the grid forms for the same people
    from training.tryon_batch import shift_keypoints
    H = int(batch.tensors['real_img'].shape[2])
    keypoints = np.asarray(raw['keypoints'], np.float64)
    if builder.shifted:
        keypoints = shift_keypoints(keypoints, (H - int(raw['image'].shape[2])) // 2)
    _, back, valid = patch_pipeline.part_matrices(keypoints, H, H, builder.box_factor, x_pad=builder.x_pad, shin_fallback=builder.shin_fallback)
    got = swap_outfits.swap_tensors(batch.stages, back, valid, builder.lower_parts, [0, 2, 0], [1, 2, 2])

    grid = SnapshotGrid(raw, batch.stages, torch.device('cuda'), 3, builder)
    for i, c in enumerate((1, 5, 6)):
        want = grid.inputs(c, c + 1)
        want['style_input'] = want.pop('c')
        for key in SWAP_FP32:
            assert got[key].dtype == torch.float32 and got[key][i:i + 1].shape == want[key[len('swap_'):]].shape, key
            assert torch.equal(got[key][i:i + 1], want[key[len('swap_'):]]), (res, c, key, int((got[key][i:i + 1] != want[key[len('swap_'):]]).sum()))
        # the person's own tensors are the paired batch's
        assert torch.equal(batch.tensors['retain'][i:i + 1], want['retain']) and torch.equal(batch.tensors['pose'][i:i + 1], want['pose'])
    assert float(got['swap_denorm_upper_mask'].mean()) > 0 and float(got['swap_denorm_lower_mask'].mean()) > 0
    assert not torch.equal(got['swap_denorm_upper_input'][1], batch.tensors['denorm_upper_input'][1])

    # the batch itself: the full-body roll 1, 2, 0 = the grid's cells (0, 1), (1, 2), (2, 0) by the whole-outfit rule, which the
    # grid applies in its middle row only; the low-level function again, and the region tables through the builder
    full = swap_outfits.swap_tensors(batch.stages, back, valid, builder.lower_parts, [1, 2, 0], [1, 2, 0])
    for key in SWAP_FP32:
        assert torch.equal(batch.tensors[key], full[key]), key
    assert torch.equal(batch.tensors['swap_keep'], batch.stages['retain_mask']) and batch.tensors['swap_keep'].dtype == torch.uint8
    assert torch.equal(batch.tensors['swap_denorm_upper_input'][1:2], grid.inputs(5, 6)['denorm_upper_input'])
    lower = builder.build(raw, swap=dict(region='lowerbody', group=3))
    assert lower.stages is None
    want = grid.inputs(1, 2)
    for key in SWAP_FP32:
        assert torch.equal(lower.tensors[key][0:1], want['c' if key == 'swap_style_input' else key[len('swap_'):]]), key
    upper = builder.build(raw, swap=dict(region='upperbody', group=3))
    want = grid.inputs(6, 7)
    for key in SWAP_FP32:
        assert torch.equal(upper.tensors[key][2:3], want['c' if key == 'swap_style_input' else key[len('swap_'):]]), key


def test_a_batch_of_four_swaps_inside_each_pair_and_splits(sets):
    from training.tryon_batch import FullBodyBatch
    ds, builder = sets[256]
    raw = _raw(ds, 4)
    plain = builder.build(raw, keep_stages=True)
    batch = builder.build(raw, swap=dict(region='fullbody', group=2))
    # without the option: the nine keys; with it: the same nine tensors, bit for bit, and six more
    assert list(plain.tensors) == FullBodyBatch.KEYS and sorted(batch.tensors) == sorted(FullBodyBatch.KEYS + SWAP_KEYS)
    for key in FullBodyBatch.KEYS:
        assert torch.equal(plain.tensors[key], batch.tensors[key]), key
    assert all(list(r) == FullBodyBatch.KEYS for r in plain.split(2))
    # the style channels are the donor's patches as they are: donors 1, 0, 3, 2
    style = plain.tensors['style_input']
    assert torch.equal(batch.tensors['swap_style_input'], style[[1, 0, 3, 2]])
    assert not torch.equal(style[0], style[1]) and not torch.equal(style[2], style[3])
    # and each pair is a batch of two of its own: nothing crosses the rounds
    from training.dataset import collate
    people = [ds[i] for i in list(ds.vis_index)[:4]]
    for g in range(2):
        pair = builder.build(collate(people[2 * g:2 * g + 2]), swap=dict(region='fullbody', group=2))
        for key in SWAP_KEYS:
            assert torch.equal(pair.tensors[key], batch.tensors[key][2 * g:2 * g + 2]), (g, key)
    rounds = batch.split(2)
    assert len(rounds) == 2 and all(list(r) == FullBodyBatch.KEYS + SWAP_KEYS for r in rounds)
    assert torch.equal(rounds[1]['swap_keep'], batch.tensors['swap_keep'][2:])
    with pytest.raises(ValueError, match='groups of at least 2'):
        builder.build(raw, swap=dict(region='fullbody', group=1))
    with pytest.raises(ValueError, match='divide the batch'):
        builder.build(raw, swap=dict(region='fullbody', group=3))


# ---- the loss, on stand-in networks ----

RES, BATCH = 32, 2
REPORTS = ['Loss/G/swap_keep', 'Loss/G/swap_upper', 'Loss/G/swap_lower', 'Loss/G/swap_loss', 'Loss/scores/fake_swap']


@pytest.fixture(scope='module')
def world():
    import tiny_models
    from training.training_loop_wo_flow_fullbody import SyntheticFullBodyBatch
    torch.manual_seed(3)
    dev = torch.device('cuda')
    G, D = tiny_models.TinyG().to(dev), tiny_models.TinyD().to(dev)
    (batch,) = SyntheticFullBodyBatch(BATCH, dev, seed=1, res=RES).split(BATCH)
    # everybody in the other one's garments; the kept parts where retain keeps the photograph
    swap = {'swap_' + k: batch[k].flip(0).contiguous() for k in ('style_input', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask',
                                                                'denorm_lower_mask')}
    # the kept parts on the left, where retain is made the photograph; the garment masks are bands that overlap in the middle rows,
    # so that each of the three regions has pixels whatever the synthetic blobs are
    batch = dict(batch)
    keep = torch.zeros([BATCH, RES, RES], dtype=torch.uint8, device=dev)
    keep[:, :, :RES // 3] = 1
    batch['retain'] = torch.where(keep[:, None] != 0, batch['real_img'], -torch.ones_like(batch['real_img']))
    batch['pose'] = torch.cat([batch['pose'][:, :3], batch['retain']], dim=1)
    rows = torch.arange(RES, device=dev).reshape(1, 1, RES, 1).expand(BATCH, 1, RES, RES)
    swap['swap_denorm_upper_mask'] = (rows < 5 * RES // 8).float().contiguous()
    swap['swap_denorm_lower_mask'] = (rows >= 3 * RES // 8).float().contiguous()
    swap['swap_keep'] = keep
    in1 = (keep == 0) & (swap['swap_denorm_upper_mask'][:, 0] != 0)
    in2 = (keep == 0) & ~in1 & (swap['swap_denorm_lower_mask'][:, 0] != 0)
    assert bool(in1.any()) and bool(in2.any())
    return G, D, batch, swap


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions():
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def _phase(world, phase, with_swap, r1_gamma=10, **loss_kwargs):
    """One accumulate_gradients(phase) on copies of the networks: ({name: gradient} of G and of D, {report: value}, the batch sizes
    D saw)."""
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    G, D, batch, swap = copy.deepcopy(world[0]), copy.deepcopy(world[1]), world[2], world[3]
    reports, d_batches = {}, []
    D.register_forward_pre_hook(lambda module, args: d_batches.append(int(args[0].shape[0])))
    loss = StyleGAN2Loss(torch.device('cuda'), G.mapping, G.synthesis, G.const_encoding, G.style_encoding, D, style_mixing_prob=0, l1_weight=40,
                         vgg_weight=0, contextual_weight=0, mask_weight=20, r1_gamma=r1_gamma,
                         report_fn=lambda name, value: reports.__setitem__(name, value), **loss_kwargs)
    (G if phase.startswith('G') else D).requires_grad_(True)
    (D if phase.startswith('G') else G).requires_grad_(False)
    loss.accumulate_gradients(phase=phase, gen_z=torch.zeros([BATCH, 0], device='cuda'), sync=False, gain=1, **batch, **(swap if with_swap else {}))
    return {n: p.grad for n, p in G.named_parameters()}, {n: p.grad for n, p in D.named_parameters()}, reports, d_batches


def test_gmain_reports_the_pass_and_moves_every_gradient_it_reaches(world):
    """The swapped pass has no parsing term (it has no ground truth), so the parsing head, which only that term reaches, keeps its
    gradient bit for bit; every other generator and style-encoder parameter's gradient changes."""
    with_pass, _, reports, d_batches = _phase(world, 'Gmain', True, swap_weight=1)
    without, _, reports0, d_batches0 = _phase(world, 'Gmain', True, swap_weight=0)
    assert all(name in reports for name in REPORTS) and not any('swap' in name for name in reports0)
    assert d_batches == [4 * BATCH] and d_batches0 == [2 * BATCH]       # one discriminator pass, over four batches of fakes
    for name in REPORTS[:4]:
        value = float(reports[name].detach())
        assert math.isfinite(value) and value > 0, (name, value)
    changed = 0
    for name, g in with_pass.items():
        if without[name] is None:
            assert g is None, name
        elif name.startswith('synthesis.parse.'):
            assert torch.equal(g, without[name]), name
        else:
            assert not torch.equal(g, without[name]), name
            changed += 1
    assert changed >= 14 and any(name.startswith('style_encoding.') for name in with_pass)

    # the reported regions are the op's, times l1_weight, as means over the two images
    from torch_utils.ops.region_l1_loss import region_l1_loss
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    G, D, batch, swap = world
    loss = StyleGAN2Loss(torch.device('cuda'), G.mapping, G.synthesis, G.const_encoding, G.style_encoding, D, style_mixing_prob=0, vgg_weight=0,
                         contextual_weight=0, swap_weight=1)
    with torch.no_grad():
        x_s, x_s_ft, _ = loss._run_G_swapped(torch.zeros([BATCH, 0], device='cuda'), batch['retain'], batch['pose'],
                                             {k[len('swap_'):]: v for k, v in swap.items()}, False, False)
        regions = region_l1_loss((x_s, x_s_ft), batch['retain'], swap['swap_denorm_upper_input'], swap['swap_denorm_lower_input'], swap['swap_keep'],
                                 swap['swap_denorm_upper_mask'], swap['swap_denorm_lower_mask']) * 40
    for r, name in enumerate(REPORTS[:3]):
        assert abs(float(reports[name].detach()) - float(regions[:, r].mean())) <= 1e-5 * float(regions[:, r].mean()), name


def test_weight_zero_is_the_loss_without_the_keyword(world, monkeypatch):
    from torch_utils.ops import region_l1_loss as op
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    def never(*args, **kwargs):
        raise AssertionError('the unpaired pass ran with weight 0')
    monkeypatch.setattr(op, 'region_l1_loss', never)
    monkeypatch.setattr(StyleGAN2Loss, '_run_G_swapped', never)
    for phase in ('Gmain', 'Dmain', 'Dboth'):
        zero = _phase(world, phase, True, swap_weight=0)
        plain = _phase(world, phase, False)
        assert sorted(zero[2]) == sorted(plain[2]) and not any('swap' in name for name in plain[2]) and zero[3] == plain[3]
        for got, want in zip(zero[:2], plain[:2]):
            assert list(got) == list(want)
            for name in want:
                assert (got[name] is None) == (want[name] is None)
                if want[name] is not None:
                    assert torch.equal(got[name], want[name]), (phase, name)


def test_dmain_sees_the_swapped_fakes(world):
    # the fused pass: two paired fakes, two swapped fakes and the photographs
    _, d_with, reports, d_batches = _phase(world, 'Dmain', True, swap_weight=1)
    _, d_without, reports0, d_batches0 = _phase(world, 'Dmain', True, swap_weight=0)
    assert d_batches == [5 * BATCH] and d_batches0 == [3 * BATCH]
    assert 'Loss/scores/fake_swap' in reports and 'Loss/scores/fake_swap' not in reports0
    assert all(not torch.equal(d_with[n], d_without[n]) for n in d_with)
    # Dmain with R1 in the same call: the four fakes in one pass, then the photographs
    _, d_with, reports, d_batches = _phase(world, 'Dboth', True, swap_weight=1)
    _, d_without, _, d_batches0 = _phase(world, 'Dboth', True, swap_weight=0)
    assert d_batches == [4 * BATCH, BATCH] and d_batches0 == [2 * BATCH, BATCH] and 'Loss/scores/fake_swap' in reports
    assert all(not torch.equal(d_with[n], d_without[n]) for n in d_with)
    # Dreg is untouched
    _, reg_with, reports, d_batches = _phase(world, 'Dreg', True, swap_weight=1)
    _, reg_without, _, _ = _phase(world, 'Dreg', True, swap_weight=0)
    assert d_batches == [BATCH] and not any('swap' in name for name in reports)
    assert all(torch.equal(reg_with[n], reg_without[n]) for n in reg_with)


def test_a_positive_weight_needs_the_tensors_and_the_flat_exchange(world, monkeypatch):
    with pytest.raises(ValueError, match='needs the swapped tensors'):
        _phase(world, 'Gmain', False, swap_weight=1)
    # ddp_mode='torch' hands the loss DistributedDataParallel wrappers; here the mapping network's class stands in for the wrapper's
    monkeypatch.setattr(torch.nn.parallel, 'DistributedDataParallel', type(world[0].mapping))
    with pytest.raises(NotImplementedError, match=r"ddp_mode='torch'.*wrapped: G_mapping\).*ddp_mode='flat'"):
        _phase(world, 'Gmain', True, swap_weight=1)


# ---- the command ----

RUN_BATCH = 4
_TRAIN_SCRIPT = '''
import sys
import train_wo_flow_fullbody as T

real_loop = T.training_loop.training_loop

def small_loop(**kwargs):
    cfg = kwargs['cfg']
    cfg.G_kwargs.synthesis_kwargs.channel_base = cfg.D_kwargs.channel_base = 2048
    kwargs.update(total_kimg=kwargs['total_kimg'] * %d / 1000, kimg_per_tick=3 * %d / 1000, snapshot_gnum=3)
    return real_loop(**kwargs)

T.training_loop.training_loop = small_loop
T.main(sys.argv[1:], standalone_mode=False)
''' % (RUN_BATCH, RUN_BATCH)


def _process(cmd, seconds, **kwargs):
    r = subprocess.run(['timeout', '-k', '10', str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT, **kwargs)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _swap_rows(run_dir):
    rows = [json.loads(line) for line in open(os.path.join(run_dir, 'stats.jsonl'))]
    assert rows
    for row in rows:
        for name in REPORTS:
            assert name in row, (name, sorted(row))
            assert row[name]['num'] > 0 and math.isfinite(row[name]['mean']), (name, row[name])
        for name in REPORTS[:3]:
            assert 0 <= row[name]['mean'] <= 80, (name, row[name])         # at most l1_weight times the largest difference
    return rows


def test_a_run_with_the_option_and_its_continuation(tmp_path):
    """The smallest run the run tests use (tests/test_train_continue_gpu.py), at batch 4 with --swap_weight 1, then continued."""
    import legacy
    tree = make_tree(tmp_path / 'tree')
    script = tmp_path / 'train_small.py'
    script.write_text(_TRAIN_SCRIPT)
    env = dict(os.environ, PYTHONPATH=PKG)
    out_dir = tmp_path / 'runs'
    common = ['--data', tree, '--gpus', '1', '--cfg', 'fashion', '--batch', str(RUN_BATCH), '--snap', '1', '--aug', 'noaug', '--fp32', 'true',
              '--l1_weight', '40', '--mask_weight', '20']
    _process([sys.executable, str(script), '--outdir', str(out_dir), *common, '--swap_weight', '1', '--kimg', '2'], 300, env=env)
    (first,) = os.listdir(out_dir)
    assert first.endswith('-swap1')
    options = json.load(open(out_dir / first / 'training_options.json'))
    assert options['cfg']['loss_kwargs']['swap_weight'] == 1 and options['swap_outfits'] == dict(region='fullbody', group=RUN_BATCH)
    _swap_rows(out_dir / first)
    snapshots = sorted(name for name in os.listdir(out_dir / first) if name.startswith('network-snapshot-'))
    assert snapshots
    with open(out_dir / first / snapshots[-1], 'rb') as f:
        data = legacy.load_network_pkl(f)           # test.py's loader
    assert all(torch.isfinite(p).all() for p in data['G_ema'].parameters())
    out = _process([sys.executable, str(script), '--outdir', str(out_dir), '--data', tree, '--continue', str(out_dir / first), '--kimg', '3'],
                   300, env=env)
    assert 'Continuing from' in out
    (second,) = [d for d in os.listdir(out_dir) if d != first]
    kept = json.load(open(out_dir / second / 'training_options.json'))
    assert kept['cfg']['loss_kwargs'] == options['cfg']['loss_kwargs'] and kept['swap_outfits'] == options['swap_outfits']
    _swap_rows(out_dir / second)
