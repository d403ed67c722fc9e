"""People fitted to the canvas on the GPU (--fit-people; csrc/fit_people.hip's pasta_fit_people_u8, training/tryon_batch.py's
fit_batch) -- EXACT: the entry against the numpy statement (tests/fit_ref.py) byte for byte on a ragged batch at a canvas of
each store path; both training builders and both outfit builders on ragged trees (tests/fit_tree.py) against their plain build
of the same people fitted on the host; test.py on a ragged pair tree against a plain run on the host-fitted tree; one tick of a
training run whose snapshot records the option, scored by calc_metrics.py without being told it."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import fit_ref as R
import fit_tree as T

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pasta-gan_amd')
POISON = 0x5A


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sources(H, W):
    """(h, w, forced rectangle or None) of the ragged batch: both passes skipped; an integer factor; an odd ratio; the reduction
    limit; the magnification limit; a vertical pass only and a horizontal pass only (rectangles the two modes never make, so
    they are given)."""
    return [(H, W, None), (2 * H, 2 * W, None), (77, 53, None), (8 * H, 8 * W, None), (H // 4, W // 4, None),
            (2 * H + 1, W, (H, W, 0, 0)), (H, 2 * W + 3, (H, W, 0, 0))]


@functools.lru_cache(maxsize=None)
def _batch(H, W, mode):
    """The ragged batch's arrays and rectangles: random photographs, Voronoi label maps (ties present)."""
    rng = np.random.default_rng(1000 * H + W)
    items = []
    for i, (h, w, forced) in enumerate(_sources(H, W)):
        rect = forced if forced is not None else R.rectangle(h, w, H, W, mode)
        assert not R.refused(h, w, rect[0], rect[1]), (h, w, rect)
        items.append((rng.integers(0, 256, [h, w, 3], dtype=np.uint8), R.voronoi_labels(h, w, 7 * i + H), rect))
    return items


@functools.lru_cache(maxsize=None)
def _want_labels(H, W, mode):
    """The label maps by the statement (they do not depend on the photograph's filter): computed once per canvas and mode."""
    out, tied = [], 0
    for _, lab, (Hc, Wc, oy, ox) in _batch(H, W, mode):
        fitted, t = R.label_mode(lab, Hc, Wc)
        out.append(R.place(fitted, (H, W), oy, ox, 0))
        tied += t
    return out, tied


@pytest.mark.parametrize('filter', ['bilinear', 'box'])
@pytest.mark.parametrize('mode', ['pad', 'crop'])
@pytest.mark.parametrize('H,W', [(40, 24), (64, 48)])
def test_entry_equals_the_statement(H, W, mode, filter):
    from torch_utils.ops import _native as N
    from training import tryon_batch as TB
    items = _batch(H, W, mode)
    hw = np.array([lab.shape for _, lab, _ in items], np.int64)
    offsets = np.concatenate([[0], np.cumsum(hw[:, 0] * hw[:, 1])[:-1]])
    rects = [rect for _, _, rect in items]
    plan = TB.fit_plan(hw, offsets, rects, filter)
    images = _cu(np.concatenate([img.reshape(-1) for img, _, _ in items]))
    labels = _cu(np.concatenate([lab.reshape(-1) for _, lab, _ in items]))
    n = len(items)
    image_out = torch.full([n, H, W, 3], POISON, dtype=torch.uint8, device='cuda')
    parsing_out = torch.full([n, H, W], POISON, dtype=torch.uint8, device='cuda')
    plan_d = _cu(plan)
    status = N.lib().pasta_fit_people_u8(N.ptr(images), N.ptr(labels), int(labels.numel()), N.ptr(plan_d), int(plan.size), N.ptr(image_out),
                                         N.ptr(parsing_out), n, H, W, N.stream())
    torch.cuda.synchronize()
    assert status == 0, N.lib().pasta_last_error()
    got_i, got_p = image_out.cpu().numpy(), parsing_out.cpu().numpy()
    want_p, tied = _want_labels(H, W, mode)
    assert tied > 0                                                  # the tie rule is exercised
    for k, (img, lab, (Hc, Wc, oy, ox)) in enumerate(items):
        want_i = R.place(R.resample(img, Hc, Wc, filter), (H, W), oy, ox, 255)
        assert np.array_equal(got_i[k], want_i), (k, img.shape, 'image', int((got_i[k] != want_i).sum()))
        assert np.array_equal(got_p[k], want_p[k]), (k, lab.shape, 'parsing', int((got_p[k] != want_p[k]).sum()))
    assert np.array_equal(got_i[0], items[0][0]) and np.array_equal(got_p[0], items[0][1])          # the identity is a copy


def test_entry_refuses_and_writes_padding_for_a_foreign_plan():
    """Refusals before any launch leave the outputs alone; a record that points outside the buffers, or at no table, is written
    as padding and nothing outside is read."""
    from torch_utils.ops import _native as N
    from training import tryon_batch as TB
    H, W = 40, 24
    img, lab = np.full([80, 48, 3], 9, np.uint8), np.full([80, 48], 3, np.uint8)
    hw, offsets, rects = np.array([[80, 48]]), np.array([0]), [(40, 24, 0, 0)]
    plan = TB.fit_plan(hw, offsets, rects, 'bilinear')
    images, labels = _cu(img.reshape(-1)), _cu(lab.reshape(-1))
    outs = lambda: (torch.full([1, H, W, 3], POISON, dtype=torch.uint8, device='cuda'), torch.full([1, H, W], POISON, dtype=torch.uint8, device='cuda'))

    def call(plan, image_out, parsing_out, n=1, words=None, pixels=None):
        plan_d = _cu(plan)
        status = N.lib().pasta_fit_people_u8(N.ptr(images), N.ptr(labels), int(labels.numel()) if pixels is None else pixels, N.ptr(plan_d),
                                             int(plan.size) if words is None else words, N.ptr(image_out), N.ptr(parsing_out), n, H, W, N.stream())
        torch.cuda.synchronize()
        return status

    a, b = outs()
    assert call(plan, a, b, n=0) != 0 and call(plan, a, b, words=15) != 0 and call(plan, a, b, pixels=0) != 0
    assert (a == POISON).all() and (b == POISON).all()
    assert call(plan, a, b) == 0 and (a == 9).all() and (b == 3).all()
    for word, value in ((10, 1), (0, 81), (6, int(plan.size) - 1), (7, 3)):          # past the buffer; taller than it; two foreign tables
        bad = plan.copy()
        bad[word] = value
        a, b = outs()
        assert call(bad, a, b) == 0
        if word in (6, 7):
            assert (a == 255).all() and (b == 3).all()               # the label map has its own tables
        else:
            assert (a == 255).all() and (b == 0).all()


# ---- the builders ----

def _same_value(g, v, what):
    if isinstance(g, torch.Tensor):
        assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g, v), (what, int((g != v).sum()))
    else:
        assert np.array_equal(np.asarray(g), np.asarray(v)), what


def _equal_batches(got, want, keys):
    for k in keys:
        assert got.tensors[k].dtype == torch.float32
        _same_value(got.tensors[k], want.tensors[k], k)
    assert sorted(got.tensors) == sorted(want.tensors) and sorted(got.stages) == sorted(want.stages)
    for k in got.stages:
        _same_value(got.stages[k], want.stages[k], 'stage ' + k)
    if getattr(got, 'image', None) is not None:
        assert torch.equal(got.image, want.image)


def _train_world(tmp_path_factory, res):
    from training import dataset as D
    from training.tryon_batch import FullBodyBatchBuilder
    from training.tryon_regions import FullBodyRegionBatchBuilder
    from tryon_512_train_tree import make_512_train_tree
    from tryon_tree import make_tree
    root = tmp_path_factory.mktemp('fit_train_%d' % res)
    make, cls, builder = {256: (make_tree, D.UvitonDatasetFull, FullBodyBatchBuilder), 512: (make_512_train_tree, D.UvitonDatasetFull_512,
                                                                                             FullBodyRegionBatchBuilder)}[res]
    plain = make(root / 'plain')
    sizes = T.ragged_copy(plain, root / 'ragged')
    assert len(set(sizes)) == len(sizes)
    return plain, str(root / 'ragged'), cls, builder('cuda')


@pytest.fixture(scope='module', params=[256, 512])
def train_world(request, tmp_path_factory):
    return _train_world(tmp_path_factory, request.param)


@pytest.mark.parametrize('mode,filter', [('pad', 'bilinear'), ('crop', 'box')])
def test_training_builder_equals_its_build_of_host_fitted_people(train_world, mode, filter):
    from training.dataset import collate
    from training.tryon_batch import FullBodyBatch
    _, ragged, cls, builder = train_world
    ds = cls(ragged, fit=mode, fit_filter=filter)
    samples = [ds[i] for i in range(len(ds))]
    got = builder.build(collate(samples), keep_stages=True)
    host = [T.host_fitted_sample(s) for s in samples]
    want = builder.build(collate(host), keep_stages=True)
    _equal_batches(got, want, FullBodyBatch.KEYS)
    assert torch.equal(got.image.cpu(), torch.from_numpy(np.stack([s['image'] for s in host])))
    assert tuple(got.image.shape[1:3]) == cls.canvas


def test_a_canvas_size_tree_built_with_fit_is_the_plain_build(train_world):
    from training.dataset import collate
    from training.tryon_batch import FullBodyBatch
    plain, _, cls, builder = train_world
    a, b = cls(plain), cls(plain, fit='pad')
    want = builder.build(collate([a[i] for i in range(3)]), keep_stages=True)
    got = builder.build(collate([b[i] for i in range(3)]), keep_stages=True)
    _equal_batches(got, want, FullBodyBatch.KEYS)


def test_fit_comes_before_the_mirror_and_the_jitter(train_world):
    from training.dataset import collate
    from training.tryon_batch import FullBodyBatch
    _, ragged, cls, builder = train_world
    ds = cls(ragged, fit='pad', mirror_people=True)
    samples = [ds[i] for i in (1, 7, 8)]
    assert [s['xflip'] for s in samples] == [0, 1, 1]
    jitter = dict(spec=dict(scale=0.3, rotate=20.0, shift=0.1, colour=0.4), seed=5, positions=np.array([6, 7, 8], np.int64))
    got = builder.build(dict(collate(samples), jitter=jitter), keep_stages=True)
    want = builder.build(dict(collate([T.host_fitted_sample(s) for s in samples]), jitter=jitter), keep_stages=True)
    _equal_batches(got, want, FullBodyBatch.KEYS)


def _outfit_world(tmp_path_factory, res):
    from training import dataset as D
    from training.tryon_pairs import TryOnPairOutfitBatchBuilder
    from training.tryon_regions import TryOnOutfitBatchBuilder
    from tryon_512_tree import make_512_tree
    from tryon_pairs_tree import make_pair_tree
    import test_tryon_outfits_256_gpu as O256
    import test_tryon_outfits_gpu as O512
    root = tmp_path_factory.mktemp('fit_outfits_%d' % res)
    make, cls, builder, helper = {256: (make_pair_tree, D.UvitonOutfits_256_test, TryOnPairOutfitBatchBuilder, O256),
                                  512: (make_512_tree, D.UvitonOutfits_512_test, TryOnOutfitBatchBuilder, O512)}[res]
    T.ragged_copy(make(root / 'plain'), root / 'ragged')
    listing = root / 'outfits.txt'
    listing.write_text(''.join('%s %s %s\n' % tuple(helper._listed(n) for n in line) for line in helper.MIXED))
    return str(root / 'ragged'), str(listing), cls, builder('cuda')


@pytest.mark.parametrize('res', [256, 512])
def test_outfit_builder_equals_its_build_of_host_fitted_people(tmp_path_factory, res):
    from training.dataset import collate_outfits
    ragged, listing, cls, builder = _outfit_world(tmp_path_factory, res)
    ds = cls(path=ragged, outfits_file=listing, fit='pad')
    samples = [ds[i] for i in range(len(ds))]
    assert len({s[p + 'image'].shape for s in samples for p in ('', 'upper_', 'lower_')}) > 2          # a mixed list of several sizes
    got = builder.build(collate_outfits(samples), keep_stages=True)
    host = [T.host_fitted_sample(s, ('', 'upper_', 'lower_')) for s in samples]
    want = builder.build(collate_outfits(host), keep_stages=True)
    _equal_batches(got, want, list(want.tensors))


# ---- the command lines ----

def test_the_try_on_command_on_a_ragged_pair_tree(tmp_path):
    """test.py --fit-people pad on a ragged pair tree writes, byte for byte, the files of a plain run on the host-fitted tree."""
    from click.testing import CliRunner
    import test as test_256
    from test_tryon_pairs_gpu import _snapshot
    from tryon_pairs_tree import make_pair_tree
    plain = make_pair_tree(tmp_path / 'plain')
    T.ragged_copy(plain, tmp_path / 'ragged')
    T.host_fitted_copy(tmp_path / 'ragged', tmp_path / 'fitted', (256, 192), 'pad', 'bilinear')
    pkl = str(tmp_path / 'snapshot.pkl')
    _snapshot(pkl)

    def run(name, tree, *extra):
        args = ['--network', pkl, '--outdir', str(tmp_path / name), '--dataroot', str(tree), '--batchsize', '3', '--workers', '0',
                '--scores', str(tmp_path / (name + '.json')), *extra]
        res = CliRunner().invoke(test_256.generate_images, args, catch_exceptions=False)
        assert res.exit_code == 0, res.output
        files = sorted(os.path.relpath(os.path.join(d, f), tmp_path / name) for d, _, fs in os.walk(tmp_path / name) for f in fs)
        return files, json.loads((tmp_path / (name + '.json')).read_text())
    got, report = run('on', tmp_path / 'ragged', '--fit-people', 'pad')
    want, plain_report = run('off', tmp_path / 'fitted')
    assert got == want and len(got) >= 4
    for name in got:
        assert open(tmp_path / 'on' / name, 'rb').read() == open(tmp_path / 'off' / name, 'rb').read(), name
    assert report['fit_people'] == 'pad' and report['fit_filter'] == 'bilinear' and 'fit_people' not in plain_report
    assert report['results'] == plain_report['results']


def test_a_training_run_on_a_ragged_tree_records_fit_and_is_scored_without_the_option(tmp_path):
    import legacy
    from train_grid_tree import make_tree as make_grid_tree
    from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
    T.ragged_copy(make_grid_tree(tmp_path / 'plain'), tmp_path / 'ragged')
    run_dir = tmp_path / '00000-run'
    os.makedirs(run_dir)
    kwargs = dict(class_name='training.dataset.UvitonDatasetFull', path=str(tmp_path / 'ragged'), fit='pad', fit_filter='bilinear')
    step = training_loop(batch_size=2, batch_gpu=2, cfg=fashion_config(channel_base=2048, mbstd_group_size=2), device=torch.device('cuda'),
                         training_set_kwargs=kwargs, data_loader_kwargs=dict(num_workers=0, pin_memory=True), run_dir=str(run_dir),
                         total_kimg=2 / 1000, kimg_per_tick=2 / 1000, image_snapshot_ticks=1, network_snapshot_ticks=1, snapshot_gnum=3)
    assert step.cur_nimg == 2
    lines = [json.loads(line) for line in open(run_dir / 'stats.jsonl')]
    assert lines and all(np.isfinite(v['mean']) for line in lines for k, v in line.items() if k.startswith('Loss/'))
    assert 'fakes000000_finetune.png' in os.listdir(run_dir)
    pkl = run_dir / 'network-snapshot-000000.pkl'
    with open(pkl, 'rb') as f:
        recorded = legacy.load_network_pkl(f)['training_set_kwargs']
    assert recorded['fit'] == 'pad' and recorded['fit_filter'] == 'bilinear'
    # in this process: the command's own function, which for one GPU scores where it is called
    from click.testing import CliRunner
    import calc_metrics
    res = CliRunner().invoke(calc_metrics.calc_metrics, ['--network', str(pkl), '--metrics', 'recon_full', '--verbose', 'false'], catch_exceptions=False)
    assert res.exit_code == 0, res.output
    results = [json.loads(ln) for ln in res.output.splitlines() if ln.startswith('{')]
    assert len(results) == 1 and results[0]['metric'] == 'recon_full' and all(np.isfinite(v) for v in results[0]['results'].values())
