"""Erase strokes on the GPU (--erase-masks strokes; csrc/tryon_inputs.hip's pasta_erase_strokes_u8, training/tryon_batch.py's
strokes_batch) -- EXACT: the entry against the numpy statement (tests/erase_strokes_ref.py) byte for byte at sizes on both of its
paths and on one, two and sixteen tiles; both training builders on a numbered batch against their build of the same people with
the statement's mask handed in as a file mask of the square's size; the numbered stream of a continued run; a short run from the
command line on a tree without a mask directory, continued, and scored twice."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import erase_strokes_ref as ER
from conftest import PKG, ROOT
from train_grid_tree import make_tree as make_grid_tree
from tryon_512_train_tree import make_512_train_tree
from tryon_tree import make_tree

pytestmark = pytest.mark.gpu

SPEC = dict(strokes=5, vertices=4, length=0.2, width=0.1, turn=90.0)
SEED = 5
SIZES = [1, 15, 16, 17, 48, 80, 256]
SPECIAL = 32                        # the segments of _case that are there on purpose; the rest of the 64 are random


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _entry(segments, counts, out, n, S):
    """pasta_erase_strokes_u8 on device tensors (None: a null pointer) -> status."""
    from torch_utils.ops import _native as N
    status = N.lib().pasta_erase_strokes_u8(N.ptr(segments), N.ptr(counts), N.ptr(out), n, S, N.stream())
    torch.cuda.synchronize()
    return status


def _clip(v):
    return int(min(max(v, -8192), 8191))


def _turned(segment, S, quarter_turns):
    """The segment after quarter turns about the square's centre, exact in 1/8 pixel: (x, y) -> (8 (S - 1) - y, x)."""
    x0, y0, x1, y1, r = segment
    for _ in range(quarter_turns):
        x0, y0, x1, y1 = 8 * (S - 1) - y0, x0, 8 * (S - 1) - y1, x1
    return _clip(x0), _clip(y0), _clip(x1), _clip(y1), r


def _case(S):
    """Three items with counts (0, 1, 64).  Item 2 holds, each at all four orientations: a degenerate segment; an axis-aligned
    one; one at 45 degrees; one whose ends both lie outside the square, and so outside every tile it crosses; two inside the
    first tile that reach the next one only through their radius (by the cap, by the side); then eight with ends at the clamps (the
    thinnest half-width and, at S = 256, the widest among them; a narrower one at the small sizes, where 512 would flood the
    square); then random ones up to 64.  Items 0 and 1 carry rows past their counts that
    would mark the square if they were read."""
    u = 8 * S
    base = [(u // 3, u // 3, u // 3, u // 3, 12),
            (u // 8, u // 4, 7 * u // 8, u // 4, 9),
            (u // 5, u // 5, u // 5 + u // 2, u // 5 + u // 2, 11),
            (-100, 8 * 70 * S // 256, u + 350, 8 * 75 * S // 256, 8),
            (8 * 40, 8 * 30, 8 * 61, 8 * 30, 8 * 5),
            (8 * 10, 8 * 62, 8 * 50, 8 * 62, 8 * 4 + 3)]
    rows = [_turned(b, S, q) for b in base for q in range(4)]
    lo, hi, m, wide, mid = -8192, 8191, u // 2, min(512, 8 + u // 6), min(64, 8 + u // 32)
    rows += [(lo, lo, hi, hi, wide), (hi, lo, lo, hi, 8), (hi, hi, lo, lo, wide // 2), (lo, hi, hi, lo, 12),         # both diagonals, both ways
             (lo, m, hi, m + 3, mid), (m, lo, m + 3, hi, mid), (hi, m, lo, m - 3, 8), (m, hi, m - 3, lo, 8)]           # across and down
    assert len(rows) == SPECIAL
    rng = np.random.default_rng(S)
    while len(rows) < 64:
        x, y = rng.integers(-u, 2 * u, 2)                     # many of them miss the square, some tiles, or all but a corner
        dx, dy = rng.integers(-u // 3 - 8, u // 3 + 8, 2)
        rows.append((_clip(x), _clip(y), _clip(x + dx), _clip(y + dy), int(rng.integers(8, 9 + u // 48))))
    seg = np.zeros([3, 64, 5], np.int32)
    seg[2] = rows
    seg[0] = rows                                            # count 0: none of them is read
    seg[1] = rows
    seg[1, 0] = (u // 4, u // 6, 3 * u // 4, u // 2, 8 + u // 40)
    return seg, np.array([0, 1, 64], np.int32)


@pytest.mark.parametrize('S', SIZES)
def test_entry_equals_the_statement(S):
    seg, counts = _case(S)
    want = ER.mask(seg, counts, S, whole_planes=True)
    assert not want[0].any() and want[2].any() and (S < 15 or (0 < want[1].mean() < want[2].mean() and not want[2].all()))
    out = torch.full([3, S, S], 7, dtype=torch.uint8, device='cuda')
    assert out.data_ptr() % 16 == 0
    assert _entry(_cu(seg), _cu(counts), out, 3, S) == 0
    got = out.cpu().numpy()
    for n in range(3):
        assert np.array_equal(got[n], want[n]), (S, n, int((got[n] != want[n]).sum()), np.argwhere(got[n] != want[n])[:4].tolist())
    if S == 256:
        # every tile of item 2 holds set pixels, most hold unset ones too, and the statement restricted to bounding boxes gives these bytes
        tiles = want[2].reshape(4, 64, 4, 64).transpose(0, 2, 1, 3).reshape(16, -1)
        assert tiles.any(axis=1).all() and (~tiles.all(axis=1)).sum() >= 12
        assert np.array_equal(ER.mask(seg, counts, S), want)


def test_entry_each_special_segment_alone():
    """One segment per item, so that a mistake in one of them cannot hide under another one's pixels: the 32 special segments of
    S = 256 as 32 items of count 1, and the empty tiles beside them."""
    S = 256
    seg, _ = _case(S)
    one = np.zeros([SPECIAL, 64, 5], np.int32)
    one[:, 0] = seg[2, :SPECIAL]
    counts = np.ones([SPECIAL], np.int32)
    want = ER.mask(one, counts, S, whole_planes=True)
    out = torch.full([SPECIAL, S, S], 7, dtype=torch.uint8, device='cuda')
    assert _entry(_cu(one), _cu(counts), out, SPECIAL, S) == 0
    got = out.cpu().numpy()
    for n in range(SPECIAL):
        assert np.array_equal(got[n], want[n]), (n, one[n, 0].tolist(), int((got[n] != want[n]).sum()))
    # the two that reach a neighbouring tile only through their radius do reach it, at their first orientation
    assert want[16][:64, 64:128].any() and not want[16][64:, :].any()                   # by the cap: columns 64, 65, 66
    assert want[20][64:128, :64].any() and not want[20][:, 64:].any()                   # by the side: rows 64, 65, 66
    assert (want.reshape(SPECIAL, -1).sum(axis=1) > 0).all()


@pytest.mark.parametrize('S', [16, 48])
def test_entry_into_a_tensor_that_is_not_16_byte_aligned(S):
    """A size of the wide path from an odd address: the byte path, the same bytes, and nothing before or behind them."""
    seg, counts = _case(S)
    want = ER.mask(seg, counts, S, whole_planes=True)
    flat = torch.full([3 * S * S + 32], 7, dtype=torch.uint8, device='cuda')
    out = flat[1:1 + 3 * S * S].view(3, S, S)
    assert out.data_ptr() % 16 == 1
    assert _entry(_cu(seg), _cu(counts), out, 3, S) == 0
    assert np.array_equal(out.cpu().numpy(), want)
    assert int(flat[0]) == 7 and (flat[1 + 3 * S * S:] == 7).all()


def test_entry_reads_a_count_outside_0_64_as_clamped():
    S = 48
    seg, _ = _case(S)
    counts = np.array([-3, 70, 2 ** 31 - 1], np.int32)
    want = ER.mask(seg, np.array([0, 64, 64], np.int32), S, whole_planes=True)
    out = torch.full([3, S, S], 7, dtype=torch.uint8, device='cuda')
    assert _entry(_cu(seg), _cu(counts), out, 3, S) == 0
    assert np.array_equal(out.cpu().numpy(), want) and not want[0].any()


def test_entry_refusals():
    from torch_utils.ops import _native as N
    S = 16
    seg, counts = (_cu(a) for a in _case(S))
    lib = N.lib()
    def refused(words, segments, cnt, with_out, n, size):
        out = torch.full([3, S, S], 7, dtype=torch.uint8, device='cuda')
        assert _entry(segments, cnt, out if with_out else None, n, size) != 0, words
        assert words in lib.pasta_last_error() and b'erase_strokes_u8' in lib.pasta_last_error(), (words, lib.pasta_last_error())
        assert (out == 7).all(), words                                     # nothing was launched
    refused(b'null pointer', None, counts, True, 3, S)
    refused(b'null pointer', seg, None, True, 3, S)
    refused(b'null pointer', seg, counts, False, 3, S)
    for n, size in ((-1, S), (65536, S), (3, 0), (3, -16), (3, 1025)):
        refused(b'bad shape', seg, counts, True, n, size)
    # no item is nothing to do, whatever the pointers
    out = torch.full([3, S, S], 7, dtype=torch.uint8, device='cuda')
    assert _entry(None, None, None, 0, S) == 0 and _entry(seg, counts, out, 0, S) == 0 and (out == 7).all()
    # and the same arguments, complete, are taken
    assert _entry(seg, counts, out, 3, S) == 0 and not (out == 7).any()


# ---- the builders ----

def _equal_batches(got, want):
    from training.tryon_batch import FullBodyBatch
    for k in FullBodyBatch.KEYS:
        g, v = got.tensors[k], want.tensors[k]
        assert g.dtype == torch.float32 and g.shape == v.shape and torch.equal(g, v), (k, int((g != v).sum()))
    assert sorted(got.stages) == sorted(want.stages)
    for k in got.stages:
        g, v = got.stages[k], want.stages[k]
        assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g, v), ('stage', k, int((g != v).sum()))
    assert torch.equal(got.image, want.image)


def _with_masks(samples, masks):
    return [dict(s, erase_mask=m) for s, m in zip(samples, masks)]


def _builder_case(builder, samples, positions):
    """``samples`` of a data set opened with ``strokes`` (1 x 1 zero masks), numbered -> the build of the same people carrying the
    statement's masks as file masks of S x S."""
    from training.dataset import collate
    from training.tryon_batch import attach_strokes
    S = samples[0]['parsing'].shape[0]
    assert all(s['erase_mask'].shape == (1, 1) for s in samples)
    got = builder.build(attach_strokes(collate(samples), SPEC, SEED, positions), keep_stages=True)
    masks = [ER.item_mask(SPEC, SEED, t, S) for t in positions]
    assert all(m.shape == (S, S) and m.max() == 1 for m in masks)
    _equal_batches(got, builder.build(collate(_with_masks(samples, masks)), keep_stages=True))
    # a batch without the key is the plain build: nothing is erased but the arm parts
    plain = builder.build(collate(samples), keep_stages=True)
    _equal_batches(builder.build(dict(collate(samples)), keep_stages=True), plain)
    assert not torch.equal(got.tensors['denorm_upper_input'], plain.tensors['denorm_upper_input']) or \
        not torch.equal(got.tensors['denorm_lower_input'], plain.tensors['denorm_lower_input'])
    for k in ('real_img', 'pose', 'gt_parsing', 'retain'):                 # the erase mask zeroes the two denormalised inputs, nothing else
        assert torch.equal(got.tensors[k], plain.tensors[k]), k
    # 255 in place of 1 erases the same pixels where no arm part lies, and fewer where one does (255 + 1 wraps): never more
    loud = builder.build(collate(_with_masks(samples, [m * np.uint8(255) for m in masks])), keep_stages=True)
    for k in ('denorm_upper_mask', 'denorm_lower_mask'):
        assert (got.tensors[k] <= loud.tensors[k]).all(), k
    return got


def test_builder_256_equals_its_build_with_the_statements_masks(tmp_path_factory):
    from training.dataset import UvitonDatasetFull
    from training.tryon_batch import FullBodyBatchBuilder
    root = make_tree(tmp_path_factory.mktemp('strokes_gpu'))
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    ds = UvitonDatasetFull(root, erase_masks='strokes')
    _builder_case(FullBodyBatchBuilder('cuda'), [ds[i] for i in range(5)], [11, 3, 2 ** 33, 0, 4])


def test_builder_256_draws_after_mirroring_and_jittering_and_never_mirrors_the_mask(tmp_path_factory):
    """Mirrored and jittered people under drawn masks == the same batch with the statement's masks handed in as files, reversed
    along x for the flagged items: the mirror kernel turns those back, so the drawn mask was not mirrored."""
    from training.dataset import UvitonDatasetFull, collate
    from training.tryon_batch import FullBodyBatchBuilder, attach_strokes
    root = make_tree(tmp_path_factory.mktemp('strokes_gpu_mirror'))
    ds = UvitonDatasetFull(root, mirror_people=True, erase_masks='strokes')
    flags = (0, 1, 1)
    samples = [ds[i + 5 * f] for i, f in enumerate(flags)]
    assert [s['xflip'] for s in samples] == list(flags)
    positions = np.array([6, 7, 8], np.int64)
    jitter = dict(spec=dict(scale=0.2, rotate=10.0, shift=0.05, colour=0.2), seed=SEED, positions=positions)
    builder = FullBodyBatchBuilder('cuda')
    got = builder.build(attach_strokes(dict(collate(samples), jitter=jitter), SPEC, SEED, positions), keep_stages=True)
    masks = [ER.item_mask(SPEC, SEED, t, 256) for t in positions.tolist()]
    assert any(not np.array_equal(m, m[:, ::-1]) for m in masks[1:])
    handed = [np.ascontiguousarray(m[:, ::-1]) if f else m for m, f in zip(masks, flags)]
    _equal_batches(got, builder.build(dict(collate(_with_masks(samples, handed)), jitter=jitter), keep_stages=True))


def test_builder_512_equals_its_build_with_the_statements_masks(tmp_path_factory):
    from training.dataset import UvitonDatasetFull_512
    from training.tryon_regions import FullBodyRegionBatchBuilder
    root = make_512_train_tree(tmp_path_factory.mktemp('strokes_gpu_512'))
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    ds = UvitonDatasetFull_512(root, erase_masks='strokes')
    got = _builder_case(FullBodyRegionBatchBuilder('cuda'), [ds[i] for i in ds.vis_index], [1, 12, 5])
    assert got.tensors['denorm_upper_mask'].any() and got.tensors['denorm_lower_mask'].any()


# ---- the stream ----

def test_a_stream_started_at_4_is_the_stream_from_batch_3(tmp_path_factory):
    from training.tryon_batch import FullBodyBatch
    from training.training_loop_wo_flow_fullbody import _data_batches
    root = make_tree(tmp_path_factory.mktemp('strokes_gpu_stream'))
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    def stream(count, cur_nimg, kind='strokes'):
        _, _, batches = _data_batches(1, 0, 2, 0, torch.device('cuda'),
                                      dict(class_name='training.dataset.UvitonDatasetFull', path=root, erase_masks=kind),
                                      dict(num_workers=0, pin_memory=True), cur_nimg=cur_nimg)
        return [next(batches) for _ in range(count)]
    whole, later = stream(4, 0), stream(2, 4)
    for a, b in zip(whole[2:], later):
        for k in FullBodyBatch.KEYS:
            assert torch.equal(a.tensors[k], b.tensors[k]), k
    # the same people without strokes keep more of their garments; and a person who comes round again gets another mask
    plain = stream(4, 0, kind='none')
    kept = lambda batches: sum(float(b.tensors['denorm_upper_mask'].sum() + b.tensors['denorm_lower_mask'].sum()) for b in batches)
    assert kept(whole) < kept(plain)
    assert all(torch.equal(a.tensors['real_img'], b.tensors['real_img']) for a, b in zip(whole, plain))


# ---- the command line, end to end ----

# train_wo_flow_fullbody.py's own main() in a fresh process, shrunk as tests/test_train_continue_gpu.py shrinks it: test-size widths,
# a 3 x 3 grid, ticks of 2 iterations -- and --kimg N read as N ITERATIONS, since the command counts in thousands of images.
BATCH = 2
_TRAIN_SCRIPT = '''
import sys
import train_wo_flow_fullbody as T

real_loop = T.training_loop.training_loop

def small_loop(**kwargs):
    cfg = kwargs['cfg']
    cfg.G_kwargs.synthesis_kwargs.channel_base = cfg.D_kwargs.channel_base = 2048
    cfg.D_kwargs.epilogue_kwargs.mbstd_group_size = 2
    kwargs.update(total_kimg=kwargs['total_kimg'] * %d / 1000, kimg_per_tick=2 * %d / 1000, snapshot_gnum=3)
    return real_loop(**kwargs)

T.training_loop.training_loop = small_loop
T.main(sys.argv[1:], standalone_mode=False)
''' % (BATCH, BATCH)


def _process(cmd, seconds, **kwargs):
    r = subprocess.run(['timeout', '-k', '10', str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT, **kwargs)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _finite_losses(run_dir):
    lines = [json.loads(line) for line in open(os.path.join(run_dir, 'stats.jsonl'))]
    assert lines
    for line in lines:
        losses = {k: v for k, v in line.items() if k.startswith('Loss/')}
        assert losses and all(np.isfinite(v['mean']) and v['num'] > 0 for v in losses.values()), sorted(losses)
    return lines


@pytest.fixture(scope='module')
def command_line_run(tmp_path_factory):
    """Four iterations of ``--erase-masks strokes`` on the grid tree without its mask directory, then two more by ``--continue``.
    (the tree, the first run's directory, the continued run's directory)"""
    root = make_grid_tree(tmp_path_factory.mktemp('strokes_gpu_cli'))
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    tmp = tmp_path_factory.mktemp('strokes_gpu_runs')
    script = tmp / 'train_small.py'
    script.write_text(_TRAIN_SCRIPT)
    env = dict(os.environ, PYTHONPATH=PKG)
    out = _process([sys.executable, str(script), '--outdir', str(tmp / 'runs'), '--data', root, '--gpus', '1', '--cfg', 'fashion', '--batch', str(BATCH),
                    '--snap', '1', '--aug', 'noaug', '--l1_weight', '40', '--mask_weight', '20', '--erase-masks', 'strokes',
                    '--erase-strokes', 'strokes=4,width=0.1', '--kimg', '4'], 600, env=env)
    assert 'Erase masks:        strokes (strokes=4,vertices=6,length=0.25,width=0.1,turn=60)' in out
    (first,) = os.listdir(tmp / 'runs')
    assert '-erasestrokes-fashion' in first
    out = _process([sys.executable, str(script), '--outdir', str(tmp / 'runs'), '--data', root, '--continue', str(tmp / 'runs' / first), '--kimg', '6'],
                   600, env=env)
    assert 'Continuing from' in out and 'Erase masks:        strokes (strokes=4,vertices=6,length=0.25,width=0.1,turn=60)' in out
    (second,) = [d for d in os.listdir(tmp / 'runs') if d != first]
    return root, str(tmp / 'runs' / first), str(tmp / 'runs' / second)


def test_command_line_trains_without_a_mask_directory_and_continues(command_line_run):
    import legacy
    from training import train_state
    root, first, second = command_line_run
    assert not os.path.exists(os.path.join(root, 'train_random_mask_acgpn'))
    lines = _finite_losses(first)
    assert lines[-1]['Progress/kimg']['mean'] * 1000 == pytest.approx(4 * BATCH)
    state = train_state.load_state(os.path.join(first, 'training-state-000000.pt'))
    assert state['batch_idx'] == 4 and state['cur_nimg'] == 4 * BATCH
    recorded = json.load(open(os.path.join(first, 'training_options.json')))
    assert recorded['training_set_kwargs']['erase_masks'] == 'strokes'
    assert recorded['training_set_kwargs']['erase_strokes'] == dict(strokes=4, vertices=6, length=0.25, width=0.1, turn=60.0)
    assert all(os.path.getsize(os.path.join(first, name)) > 1000 for name in ('init_denorm_upper.png', 'init_denorm_lower.png', 'init_retain.png'))
    # the continued run: the same options, two more iterations
    assert second.endswith('-continue000000')
    _finite_losses(second)
    state = train_state.load_state(os.path.join(second, 'training-state-000000.pt'))
    assert state['batch_idx'] == 6 and state['cur_nimg'] == 6 * BATCH
    assert json.load(open(os.path.join(second, 'training_options.json')))['training_set_kwargs'] == recorded['training_set_kwargs']
    with open(os.path.join(second, 'network-snapshot-000000.pkl'), 'rb') as f:
        data = legacy.load_network_pkl(f)
    assert data['training_set_kwargs']['erase_masks'] == 'strokes' and data['training_set_kwargs']['erase_strokes']['strokes'] == 4
    assert all(torch.isfinite(p).all() for p in data['G_ema'].parameters())


def test_calc_metrics_scores_it_twice_with_identical_output(command_line_run):
    root, first, second = command_line_run
    snapshot = os.path.join(second, 'network-snapshot-000000.pkl')
    def score(*extra):
        cmd = [sys.executable, os.path.join(ROOT, 'pasta-gan_amd', 'calc_metrics.py'), '--network', snapshot, '--metrics', 'recon_full', '--verbose', 'false', *extra]
        lines = [json.loads(ln) for ln in _process(cmd, 600).splitlines() if ln.startswith('{')]
        assert len(lines) == 1 and lines[0]['metric'] == 'recon_full' and all(np.isfinite(v) for v in lines[0]['results'].values())
        return lines[0]['results']
    once, twice = score(), score()
    assert once == twice
    # with the holes left out the tree opens as well, and the holes cost something
    bare = score('--data', root, '--erase-masks', 'none')
    print('recon_full with strokes:', once, 'with none:', bare)
    assert bare != once
    reports = [json.loads(line) for line in open(os.path.join(second, 'metric-recon_full.jsonl'))]
    assert len(reports) == 3 and reports[0]['results'] == reports[1]['results'] == once and reports[2]['results'] == bare
