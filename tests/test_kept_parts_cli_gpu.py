"""--kept-parts photo of the two try-on commands on the tiny trees and snapshots of the existing end-to-end tests: the written
pictures are the numpy restatement's paste (tests/keep_composite_ref.py) of the plain run's bytes, the photograph and the keep
region of the builder's stages; the default writes what it wrote; --scores describes the written bytes.  Every run compared
uses one batch size per model (bytes can differ between batch sizes)."""

import importlib.util
import json
import os

import numpy as np
import PIL.Image
import pytest

import keep_composite_ref as KC
import tryon_fidelity_ref as F
from conftest import ROOT
from test_tryon_512_gpu import _snapshot as _snapshot_512       # the snapshots of the existing end-to-end tests, not copies of them
from test_tryon_outfits_gpu import BATCH as BATCH_512, MIXED, _write_list
from test_tryon_pairs_gpu import _snapshot as _snapshot_256
from tryon_512_tree import make_512_tree
from tryon_pairs_tree import PAIRS as PAIRS_256, make_pair_tree

pytestmark = pytest.mark.gpu

BATCH_256 = 3
SIDE, W512 = 512, 320


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _pixels(path):
    img = PIL.Image.open(path)
    assert img.mode == 'RGB'
    return np.asarray(img)


def _both_kinds(masks, radius):
    """The tree must have kept pixels whose whole window is kept and kept pixels whose window is not: one without both proves nothing."""
    K = (2 * radius + 1) ** 2
    a = [KC.weight(m, radius) for m in masks]
    return any((x == K).any() for x in a), any(((x > 0) & (x < K)).any() for x in a) or radius == 0


class Runs:
    """The runs of one model, made when first asked for and kept: ``get(key, **keywords)`` -> (directory, report or None);
    ``partials[key]``: the int64 partials a scored run handed ``write_scores``."""

    def __init__(self, root, generate):
        self.root, self.generate, self.done, self.partials = root, generate, {}, {}

    def get(self, key, scores=False, **keywords):
        import tryon_cli
        if key not in self.done:
            outdir, report = self.root / key, self.root / (key + '.json')
            write = tryon_cli.write_scores

            def recording(scores_file, partials, *args, **kwargs):
                self.partials[key] = partials.cpu()
                return write(scores_file, partials, *args, **kwargs)
            tryon_cli.write_scores = recording
            try:
                self.generate(str(outdir), str(report) if scores else None, **keywords)
            finally:
                tryon_cli.write_scores = write
            self.done[key] = outdir, json.loads(report.read_text()) if scores else None
        return self.done[key]


# ---- 256 x 192 ----

@pytest.fixture(scope='module')
def world_256(tmp_path_factory):
    import tryon_cli
    root = tmp_path_factory.mktemp('kept256')
    tree, pkl = make_pair_tree(root / 'tree'), str(root / 'snapshot.pkl')
    _snapshot_256(pkl)
    runs = Runs(root, lambda outdir, scores, **kw: tryon_cli.generate_256(pkl, 1, 'const', outdir, tree, BATCH_256, 0, scores_file=scores, **kw))
    # the builder's stages of every pair, as generate_256 builds them, under the name of the pair's file
    from training.dataset import UvitonDatasetV19_test, collate_region_outfits
    from training.tryon_pairs import TryOnPairOutfitBatchBuilder
    ds, builder, stages = UvitonDatasetV19_test(path=tree), TryOnPairOutfitBatchBuilder('cuda'), {}
    for lo in range(0, len(ds), BATCH_256):
        raw = collate_region_outfits('upperbody', [ds[i] for i in range(lo, min(lo + BATCH_256, len(ds)))])
        st = {k: v.cpu().numpy() for k, v in builder.build(raw, keep_stages=True).stages.items() if k in ('image', 'parsing', 'palm', 'denorm_upper', 'denorm_lower')}
        for j, (p, c) in enumerate(zip(raw['person_name'], raw['clothes_name'])):
            name = os.path.join(p.split('/')[0], os.path.basename(p)[:-4] + '__' + os.path.basename(c)[:-4] + '.png')
            stages[name] = dict({k: v[j] for k, v in st.items()}, index=lo + j, keep=F.keep_mask(st['palm'][j], st['parsing'][j]))
    assert len(stages) == len(PAIRS_256)
    return dict(tree=tree, pkl=pkl, runs=runs, stages=stages)


def _check_paste(plain_dir, photo_dir, stages, radius, crop=lambda a: a):
    names = _files(plain_dir)
    assert _files(photo_dir) == names and len(names) == len(stages)
    changed = 0
    for name in names:
        st = stages[name]
        plain, got = crop(_pixels(plain_dir / name)), crop(_pixels(photo_dir / name))
        want = KC.composite(plain[None], st['image'][None], st['keep'][None], radius)[0]
        assert np.array_equal(got, want), (name, radius, int((got != want).sum()))
        changed += int((got != plain).sum())
    assert changed > 0                                              # the generator does not reproduce the photograph by itself
    return names


@pytest.mark.parametrize('radius', [2, 0])
def test_generate_256_pastes_the_photograph(world_256, radius):
    stages = world_256['stages']
    full, partial = _both_kinds([s['keep'] for s in stages.values()], radius)
    assert full and partial, (radius, full, partial)
    plain, _ = world_256['runs'].get('plain', scores=True)
    photo, _ = world_256['runs'].get('photo%d' % radius, scores=radius == 2, kept_parts='photo', kept_feather=radius)
    _check_paste(plain, photo, stages, radius)
    assert PIL.Image.open(photo / _files(photo)[0]).size == (192, 256)


def test_generate_256_default_feather_is_two(world_256):
    two, _ = world_256['runs'].get('photo2', scores=True, kept_parts='photo', kept_feather=2)
    default, _ = world_256['runs'].get('photo_default', kept_parts='photo')
    assert _files(default) == _files(two)
    for name in _files(two):
        assert (default / name).read_bytes() == (two / name).read_bytes(), name


def test_generate_256_generated_is_the_run_without_the_keyword(world_256):
    plain, report = world_256['runs'].get('plain', scores=True)
    same, same_report = world_256['runs'].get('generated', scores=True, kept_parts='generated')
    assert _files(same) == _files(plain) and len(_files(plain)) == len(PAIRS_256)
    for name in _files(plain):
        assert (same / name).read_bytes() == (plain / name).read_bytes(), name
    assert json.dumps(same_report) == json.dumps(report)
    assert sorted(report) == ['dataroot', 'network', 'noise_mode', 'pairs', 'results']      # key for key what it was


def _integer_words(written, ref, mask):
    """The four integer words of tests/tryon_fidelity_ref.region_stats for one image (sum |d|, sum d^2, windows, bytes) without
    its SSIM maps, which take a quarter of a second each at 512 x 320."""
    m = np.asarray(mask) != 0
    d = (written.astype(np.int64) - ref.astype(np.int64)) * m[..., None]
    return [int(np.abs(d).sum()), int((d * d).sum()), 3 * int(F.windows_inside(m).sum()), 3 * int(m.sum())]


def _check_scores(runs, stages, crop=lambda a: a, whole_restatement=True):
    """The scored run with the paste against the scored plain run: the report's new keys, the integer partials against the
    restatement applied to the WRITTEN bytes, and a lower keep_l1."""
    _, plain_report = runs.get('plain', scores=True)
    outdir, report = runs.get('photo2', scores=True, kept_parts='photo', kept_feather=2)
    partials = runs.partials['photo2']
    assert sorted(plain_report) == ['dataroot', 'network', 'noise_mode', 'pairs', 'results']
    assert sorted(report) == ['dataroot', 'kept_feather', 'kept_parts', 'network', 'noise_mode', 'pairs', 'results']
    assert report['kept_parts'] == 'photo' and report['kept_feather'] == 2 and report['pairs'] == len(stages)
    assert sorted(report['results']) == sorted(plain_report['results'])
    rows = np.zeros([len(stages), 3, 4], np.int64)
    for name, st in stages.items():
        regions = F.pair_regions(st['image'], st['parsing'], st['palm'], st['denorm_upper'], st['denorm_lower'])
        written = np.ascontiguousarray(crop(_pixels(outdir / name)))
        for k, region in enumerate(F.REGIONS):
            mask, ref = regions[region]
            rows[st['index'], k] = _integer_words(written, ref, mask)
            if whole_restatement:
                assert rows[st['index'], k].tolist() == [v[0] for v in F.region_stats(written[None], ref[None], mask[None])[:4]]
    print('keep sum |d| per item, pasted:', rows[:, 0, 0].tolist(), 'keep_l1 plain %.6f pasted %.6f'
          % (plain_report['results']['tryon_keep_l1'], report['results']['tryon_keep_l1']))
    assert tuple(partials.shape) == (len(stages), 3, 5)
    assert np.array_equal(partials[:, :, :4].numpy(), rows)          # sum |d|, sum d^2, windows, bytes of the three regions
    assert report['results']['tryon_keep_l1'] < plain_report['results']['tryon_keep_l1']
    for k in ('tryon_keep_share', 'tryon_keep_pairs', 'tryon_upper_share', 'tryon_lower_share'):
        assert report['results'][k] == plain_report['results'][k], k                        # the regions are the same


def test_generate_256_scores_the_written_bytes(world_256):
    _check_scores(world_256['runs'], world_256['stages'])


def test_the_256_command_line_pastes_as_the_keywords_do(world_256, tmp_path):
    from click.testing import CliRunner
    stages = world_256['stages']
    full, partial = _both_kinds([s['keep'] for s in stages.values()], 1)
    assert full and partial
    keyword, _ = world_256['runs'].get('photo1', kept_parts='photo', kept_feather=1)
    plain, _ = world_256['runs'].get('plain', scores=True)
    names = _check_paste(plain, keyword, stages, 1)
    spec = importlib.util.spec_from_file_location('pasta_kept_test_cli', os.path.join(ROOT, 'pasta-gan_amd', 'test.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    result = CliRunner().invoke(module.generate_images, ['--network', world_256['pkl'], '--outdir', str(tmp_path / 'cli'), '--dataroot', world_256['tree'],
                                                         '--batchsize', str(BATCH_256), '--workers', '0', '--kept-parts', 'photo', '--kept-feather', '1'])
    assert result.exit_code == 0, (result.output[-2000:], result.exception)
    assert _files(tmp_path / 'cli') == names
    for name in names:
        assert (tmp_path / 'cli' / name).read_bytes() == (keyword / name).read_bytes(), name


# ---- 512 x 320 ----

@pytest.fixture(scope='module')
def world_512(tmp_path_factory):
    import tryon_cli
    root = tmp_path_factory.mktemp('kept512')
    tree, pkl = make_512_tree(root / 'tree'), str(root / 'snapshot.pkl')
    _snapshot_512(pkl)
    listing = _write_list(root / 'outfits.txt', MIXED)
    runs = Runs(root, lambda outdir, scores, **kw: tryon_cli.generate_512(pkl, 1, 'const', outdir, tree, BATCH_512, None, 0, outfits_file=listing,
                                                                         scores_file=scores, **kw))
    from training.dataset import UvitonOutfits_512_test, collate_outfits
    from training.tryon_regions import TryOnOutfitBatchBuilder
    ds, builder, stages = UvitonOutfits_512_test(path=tree, outfits_file=listing), TryOnOutfitBatchBuilder('cuda'), {}
    for lo in range(0, len(ds), BATCH_512):
        raw = collate_outfits([ds[i] for i in range(lo, min(lo + BATCH_512, len(ds)))])
        st = {k: v.cpu().numpy() for k, v in builder.build(raw, keep_stages=True).stages.items() if k in ('image', 'parsing', 'palm', 'denorm_upper', 'denorm_lower')}
        for j in range(len(raw['person_name'])):
            stages['%03d.png' % (lo + j)] = dict({k: v[j] for k, v in st.items()}, index=lo + j, keep=F.keep_mask(st['palm'][j], st['parsing'][j]))
    assert len(stages) == len(MIXED)
    return dict(runs=runs, stages=stages)


def test_generate_512_pastes_into_the_generated_panel_only(world_512):
    stages = world_512['stages']
    full, partial = _both_kinds([s['keep'] for s in stages.values()], 2)
    assert full and partial
    plain, _ = world_512['runs'].get('plain', scores=True)
    photo, _ = world_512['runs'].get('photo2', scores=True, kept_parts='photo', kept_feather=2)
    c0 = 3 * SIDE + (SIDE - W512) // 2                              # upper donor | lower donor | person | generated
    names = _check_paste(plain, photo, stages, 2, crop=lambda a: a[:, c0:c0 + W512])
    assert names == ['%03d.png' % i for i in range(len(MIXED))]
    for name in names:
        a, b = _pixels(plain / name), _pixels(photo / name)
        assert a.shape == b.shape == (SIDE, 4 * SIDE, 3)
        assert np.array_equal(a[:, :c0], b[:, :c0]) and np.array_equal(a[:, c0 + W512:], b[:, c0 + W512:]), name    # the panels and the padding
    # the encoder on the GPU is handed the same batch
    gpu, _ = world_512['runs'].get('photo2_gpu', kept_parts='photo', kept_feather=2, png_encoder='gpu')
    assert _files(gpu) == names
    for name in names:
        assert np.array_equal(_pixels(gpu / name), _pixels(photo / name)), name
        assert (gpu / name).read_bytes() != (photo / name).read_bytes()


def test_generate_512_scores_the_written_bytes(world_512):
    c0 = 3 * SIDE + (SIDE - W512) // 2
    _check_scores(world_512['runs'], world_512['stages'], crop=lambda a: a[:, c0:c0 + W512], whole_restatement=False)
