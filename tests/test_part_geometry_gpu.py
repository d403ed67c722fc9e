"""``--part-geometry gpu``: pasta_part_geometry against tests/part_geometry_ref.py bit for bit; the 'gpu' form of the
three normalisations, the five builders and the swapped-outfit pass against their 'host' form with the host's solve replaced by
the restatement (so that the one numerical difference, LAPACK, is out of the comparison and every indexing mistake is a hard
failure); no host solve under 'gpu'; and the three command lines."""
import importlib.util
import json
import os
import sys

import numpy as np
import PIL.Image
import pytest
import torch
from click.testing import CliRunner

import part_geometry_ref as ref
from conftest import PKG, ROOT
from train_grid_tree import make_tree
from tryon_512_train_tree import make_512_train_tree
from tryon_512_tree import PAIRS as PAIRS_512, make_512_tree
from tryon_pairs_tree import PAIRS as PAIRS_256, make_pair_tree

pytestmark = pytest.mark.gpu

OUTPUTS = ('quads', 'fwd', 'back', 'fwd_inv', 'back_inv', 'm_inv', 'valid')


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- the kernel ----

def _people(size, m):
    """``m`` people: the edge cases first (all of them from m = 14), then seeded standing people."""
    edge, _ = ref.edge_people(size)
    rest = ref.standing_people(max(m - len(edge), 1), size, seed=m)
    return np.concatenate([edge, rest])[:m] if m >= len(edge) else np.concatenate([edge[3 * m:3 * m + m], rest])[:m]


@pytest.mark.parametrize('size,x_pad,shin', [(256, 32, False), (256, 0, True), (512, 0, False), (512, 32, True)])
@pytest.mark.parametrize('m', [1, 3, 14, 65])
def test_the_kernel_equals_the_restatement_bit_for_bit(size, x_pad, shin, m):
    from training import patch_pipeline
    people = _people(size, m)
    assert people.shape == (m, 18, 3)
    want = ref.geometry(people, size, size // 4, size // 4, x_pad, shin)
    got = patch_pipeline.part_geometry(people, size, size, 2, x_pad, shin, 'cuda')
    assert tuple(got) == OUTPUTS
    for name in OUTPUTS:
        mine = got[name].cpu().numpy()
        assert mine.dtype == want[name].dtype and mine.shape == want[name].shape, name
        differing = np.argwhere(_bits(mine) != _bits(want[name]))
        assert len(differing) == 0, (name, len(differing), differing[:4].tolist())
    if m >= 14:
        valid = want['valid'].astype(bool)
        assert valid.any(axis=0).all() and not valid.all(axis=0).any()
        assert (want['fwd'][valid][:, :8] == 0).all(axis=1).any()           # the singular forward system is among them
    # null outputs: each output alone is what it was among the seven
    for name in OUTPUTS:
        alone = patch_pipeline.part_geometry(people, size, size, 2, x_pad, shin, 'cuda', outputs=(name,))
        assert tuple(alone) == (name,) and torch.equal(alone[name], got[name]), name


def test_part_geometry_refuses_the_cpu_and_unknown_outputs():
    from training import patch_pipeline
    people = _people(256, 1)
    with pytest.raises(RuntimeError, match='no CPU path'):
        patch_pipeline.part_geometry(people, 256, 256, device='cpu')
    with pytest.raises(ValueError, match='unknown output'):
        patch_pipeline.part_geometry(people, 256, 256, device='cuda', outputs=('fwd', 'det'))
    with pytest.raises(ValueError, match='part geometry'):
        patch_pipeline.normalize_batch(*[torch.zeros([1, 256, 256, 3], dtype=torch.uint8, device='cuda')] * 4, people, geometry='fpga')


# ---- exact plumbing: 'gpu' against 'host' with the restatement as the host's solve ----

def _host(x):
    return x.cpu() if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def _same(got, want, what):
    got, want = _host(got), _host(want)
    if want.dtype == torch.bool:
        got = got.to(torch.bool)
    assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), (what, got.dtype, want.dtype, got.shape, want.shape)


def _same_matrices(got, want, what, joints, **solve):
    """``want_matrices``: the device back_inv / valid of either geometry against the back / valid of ``part_matrices`` for the
    persons' ``joints``, solved and inverted here."""
    from training import patch_pipeline
    _, back, valid = patch_pipeline.part_matrices(joints, 256, 256, **solve)
    for name, (back_inv, valid_dev) in (('gpu', got), ('host', want)):
        assert back_inv.is_cuda and valid_dev.is_cuda and valid_dev.dtype == torch.uint8
        _same(back_inv, patch_pipeline.inverse_maps(back, range(10)).reshape(len(back), 10, 9), '%s %s back_inv' % (what, name))
        _same(valid_dev, valid, '%s %s valid' % (what, name))


@pytest.fixture()
def restated(monkeypatch):
    from training import patch_pipeline
    monkeypatch.setattr(patch_pipeline, 'part_matrices', ref.part_matrices)


def _images(rng, n):
    return torch.from_numpy(rng.integers(0, 256, [n, 256, 256, 3], dtype=np.uint8)).cuda()


def _masks(rng, n):
    return torch.from_numpy((rng.integers(0, 4, [n, 256, 256, 1], dtype=np.uint8) > 0).astype(np.uint8).repeat(3, 3) * 255).cuda()


def test_the_three_normalisations_are_the_hosts(restated):
    from training import patch_pipeline as P
    rng = np.random.default_rng(3)
    edge, names = ref.edge_people(256)
    # N = 3 samples over M = 5 people, every index table mixed; the people miss parts the others have
    people = edge[[names.index(k) for k in ('complete', 'no left knee', 'no shoulders, no hips', 'no left ankle', 'zero-length right forearm')]]
    person, upper, lower = [0, 3, 1], [2, 0, 4], [1, 1, 3]

    joints = people[[0, 1, 2]].copy()
    joints[..., 0] -= 32                                                    # normalize_batch adds the padding itself
    sources = [_images(rng, 3), _images(rng, 3), _masks(rng, 3), _masks(rng, 3)]
    want = P.normalize_batch(*sources, joints, want_matrices=True)
    got = P.normalize_batch(*sources, joints, want_matrices=True, geometry='gpu')
    assert len(got) == len(want) == 10 and got[4].is_cuda
    for i in range(8):
        _same(got[i], want[i], 'normalize_batch %d' % i)
    _same_matrices(got[8:], want[8:], 'normalize_batch', joints)
    assert want[2].any() and want[3].any()

    garments, masks, sticks = _images(rng, 6), _masks(rng, 6), _images(rng, 5)
    want = P.normalize_pair_outfit_batch(garments, sticks, masks, people, person, upper, lower)
    got = P.normalize_pair_outfit_batch(garments, sticks, masks, people, person, upper, lower, geometry='gpu')
    assert len(got) == len(want) == 9 and got[5].is_cuda
    for i in range(9):
        _same(got[i], want[i], 'normalize_pair_outfit_batch %d' % i)
    assert want[3].any() and want[4].any() and not all(v.all() for v in want[6:])

    want = P.normalize_outfit_batch(garments, masks, people, person, upper, lower, want_part_masks=True, want_matrices=True)
    got = P.normalize_outfit_batch(garments, masks, people, person, upper, lower, want_part_masks=True, want_matrices=True, geometry='gpu')
    assert len(got) == len(want) == 13 and got[6].is_cuda
    for i in range(11):
        _same(got[i], want[i], 'normalize_outfit_batch %d' % i)
    _same_matrices(got[11:], want[11:], 'normalize_outfit_batch', people[person], x_pad=0)
    assert want[4].any() and want[5].any()


def _listed(pairs, name):
    return name if name == '-' else ['%s/%s.jpg' % (ds, name) for ds, p, c in pairs if name + '.jpg' in (p, c)][0]


def _outfit_list(path, pairs, lines):
    path.write_text(''.join('%s %s %s\n' % tuple(_listed(pairs, n) for n in line) for line in lines))
    return str(path)


def _builds(tmp_path):
    """(name, builder class, constructor arguments, raw batch, build keywords) of the five builders on the tiny trees."""
    from training import dataset as D
    from training.tryon_batch import FullBodyBatchBuilder
    from training.tryon_pairs import TryOnPairOutfitBatchBuilder
    from training.tryon_regions import FullBodyRegionBatchBuilder, TryOnOutfitBatchBuilder, TryOnRegionBatchBuilder
    from test_tryon_outfits_256_gpu import MIXED as MIXED_256
    from test_tryon_outfits_gpu import MIXED as MIXED_512
    train_256 = D.UvitonDatasetFull(make_tree(tmp_path / 'train256'))
    train_512 = D.UvitonDatasetFull_512(make_512_train_tree(tmp_path / 'train512'))
    tree_256, tree_512 = make_pair_tree(tmp_path / 'pairs256'), make_512_tree(tmp_path / 'pairs512')
    outfits_256 = D.UvitonOutfits_256_test(path=tree_256, outfits_file=_outfit_list(tmp_path / 'o256.txt', PAIRS_256, MIXED_256))
    outfits_512 = D.UvitonOutfits_512_test(path=tree_512, outfits_file=_outfit_list(tmp_path / 'o512.txt', PAIRS_512, MIXED_512))
    region = D.UvitonDatasetFull_512_test(path=tree_512, change_region='lowerbody')
    swap = dict(keep_stages=True, swap=dict(region='fullbody', group=3))
    first = lambda ds, count: [ds[i] for i in list(ds.vis_index)[:count]]
    return [('FullBodyBatchBuilder', FullBodyBatchBuilder, (), D.collate(first(train_256, 3)), swap),
            ('FullBodyRegionBatchBuilder', FullBodyRegionBatchBuilder, (), D.collate(first(train_512, 3)), swap),
            ('TryOnPairOutfitBatchBuilder', TryOnPairOutfitBatchBuilder, (), D.collate_outfits([outfits_256[i] for i in range(len(outfits_256))]),
             dict(keep_stages=True)),
            ('TryOnRegionBatchBuilder', TryOnRegionBatchBuilder, ('lowerbody',), D.collate_pairs([region[i] for i in range(len(region))]),
             dict(keep_stages=True)),
            ('TryOnOutfitBatchBuilder', TryOnOutfitBatchBuilder, (), D.collate_outfits([outfits_512[i] for i in range(len(outfits_512))]),
             dict(keep_stages=True))]


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    return _builds(tmp_path_factory.mktemp('part_geometry_builders'))


@pytest.mark.parametrize('which', range(5))
def test_the_builders_and_the_swapped_pass_are_the_hosts(builds, which, restated):
    from training import swap_outfits
    name, cls, args, raw, kwargs = builds[which]
    assert cls('cuda', *args).geometry == 'host'
    want, got = cls('cuda', *args).build(raw, **kwargs), cls('cuda', *args, geometry='gpu').build(raw, **kwargs)
    assert list(got.tensors) == list(want.tensors) and sorted(got.stages) == sorted(want.stages)
    if 'swap' in kwargs:
        assert set(swap_outfits.SWAP_KEYS) <= set(got.tensors) and set(swap_outfits.SWAP_STAGES) <= set(got.stages)
    for key in want.tensors:
        _same(got.tensors[key], want.tensors[key], (name, key))
    for key in want.stages:
        _same(got.stages[key], want.stages[key], (name, 'stage', key))
    assert got.stages['M_invs'].is_cuda and want.stages['denorm_upper'].any() and want.stages['denorm_lower'].any()


@pytest.mark.parametrize('which', range(5))
def test_gpu_builders_solve_nothing_on_the_host(builds, which, monkeypatch):
    from training import patch_pipeline
    name, cls, args, raw, kwargs = builds[which]

    def refuse(*a, **k):
        raise AssertionError('a host solve under geometry=gpu')
    monkeypatch.setattr(patch_pipeline, 'part_matrices', refuse)
    monkeypatch.setattr(patch_pipeline, 'adjugate_inverse', refuse)
    monkeypatch.setattr(np.linalg, 'solve', refuse)
    batch = cls('cuda', *args, geometry='gpu').build(raw, **kwargs)
    assert all(torch.isfinite(t.to(torch.float32)).all() for t in batch.tensors.values())
    with pytest.raises(AssertionError, match='a host solve'):
        cls('cuda', *args).build(raw, **kwargs)                             # the patch does catch the host's path


def test_byte_differences_from_the_unpatched_host(builds):
    """A report, not an assertion on the figures: in how many bytes 'gpu' and the host's own LAPACK solve differ, per tensor."""
    lines = []
    for name, cls, args, raw, kwargs in builds:
        want, got = cls('cuda', *args).build(raw, **kwargs), cls('cuda', *args, geometry='gpu').build(raw, **kwargs)
        for key in want.tensors:
            a, b = _host(got.tensors[key]).contiguous().view(torch.uint8), _host(want.tensors[key]).contiguous().view(torch.uint8)
            lines.append('%s %s: %d of %d bytes differ' % (name, key, int((a != b).sum()), a.numel()))
            assert a.shape == b.shape
    print('\n'.join(['part geometry, gpu against host (LAPACK) on the tiny trees:'] + lines))


# ---- the commands ----

def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs if f.endswith('.png'))


def _command(script):
    spec = importlib.util.spec_from_file_location('pasta_part_geometry_' + script[:-3], os.path.join(PKG, script))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.generate_images


def _three_runs(tmp_path, command, common):
    """The command with --part-geometry gpu, with host and without the option: ({run: report}, the names written)."""
    reports = {}
    for run, extra in (('gpu', ['--part-geometry', 'gpu']), ('host', ['--part-geometry', 'host']), ('plain', [])):
        result = CliRunner().invoke(command, common + ['--outdir', str(tmp_path / run), '--scores', str(tmp_path / (run + '.json'))] + extra)
        assert result.exit_code == 0, (run, result.output[-2000:], result.exception)
        reports[run] = json.loads((tmp_path / (run + '.json')).read_text())
    names = _files(tmp_path / 'plain')
    assert names and _files(tmp_path / 'host') == names and _files(tmp_path / 'gpu') == names
    for name in names:
        assert (tmp_path / 'host' / name).read_bytes() == (tmp_path / 'plain' / name).read_bytes(), name
    assert reports['host'] == reports['plain'] and 'part_geometry' not in reports['plain']
    assert reports['gpu'].pop('part_geometry') == 'gpu' and sorted(reports['gpu']) == sorted(reports['plain'])
    return names


def _generator(pkl):
    import legacy
    with open(pkl, 'rb') as f:
        return legacy.load_network_pkl(f)['G_ema'].cuda().eval().requires_grad_(False)


def test_test_py_writes_the_gpu_builders_images(tmp_path):
    import tryon_cli
    from test_tryon_pairs_gpu import _snapshot
    from training import dataset as D
    from training.tryon_pairs import TryOnPairOutfitBatchBuilder, images_to_u8
    tree, pkl = make_pair_tree(tmp_path / 'tree'), str(tmp_path / 'snapshot.pkl')
    _snapshot(pkl)
    names = _three_runs(tmp_path, _command('test.py'), ['--network', pkl, '--dataroot', tree, '--batchsize', '3', '--workers', '0'])
    assert len(names) == len(PAIRS_256)
    G, ds = _generator(pkl), D.UvitonDatasetV19_test(path=tree)
    builder = TryOnPairOutfitBatchBuilder('cuda', geometry='gpu')
    for lo in range(0, len(ds), 3):
        raw = D.collate_region_outfits('upperbody', [ds[i] for i in range(lo, min(lo + 3, len(ds)))])
        batch = builder.build(raw)
        from metrics import tryon_fidelity
        z = tryon_fidelity.pair_z(raw['raw_idx'].tolist(), G.z_dim, 'cuda')
        want = images_to_u8(tryon_cli.generate(G, batch.tensors, z, 1, 'const'), 32, 192).cpu().numpy()
        for i, (p, c) in enumerate(zip(raw['person_name'], raw['upper_name'])):
            name = os.path.join(p.split('/')[0], os.path.basename(p)[:-4] + '__' + os.path.basename(c)[:-4] + '.png')
            assert np.array_equal(np.asarray(PIL.Image.open(tmp_path / 'gpu' / name)), want[i]), name


def test_test_512_py_writes_the_gpu_builders_images(tmp_path):
    import tryon_cli
    from test_tryon_512_gpu import _snapshot
    from metrics import tryon_fidelity
    from training import dataset as D
    from training.tryon_pairs import images_to_u8
    from training.tryon_regions import TryOnOutfitBatchBuilder
    tree, pkl = make_512_tree(tmp_path / 'tree'), str(tmp_path / 'snapshot.pkl')
    _snapshot(pkl)
    names = _three_runs(tmp_path, _command('test_512.py'), ['--network', pkl, '--dataroot', tree, '--batchsize', '3', '--workers', '0',
                                                            '--change-region', 'lowerbody'])
    assert names == ['%03d.png' % i for i in range(len(PAIRS_512))]
    G, ds = _generator(pkl), D.UvitonDatasetFull_512_test(path=tree, change_region='lowerbody')
    builder = TryOnOutfitBatchBuilder('cuda', geometry='gpu')
    for lo in range(0, len(ds), 3):
        raw = D.collate_region_outfits('lowerbody', [ds[i] for i in range(lo, min(lo + 3, len(ds)))])
        t = builder.build(raw).tensors
        z = tryon_fidelity.pair_z(raw['raw_idx'].tolist(), G.z_dim, 'cuda')
        panels = [t['clothes_lower'], t['image'], tryon_cli.generate(G, t, z, 1, 'const')]
        want = torch.cat([images_to_u8(x, 0, 512) for x in panels], dim=2).cpu().numpy()
        for i in range(want.shape[0]):
            assert np.array_equal(np.asarray(PIL.Image.open(tmp_path / 'gpu' / ('%03d.png' % (lo + i)))), want[i]), lo + i


def test_a_training_run_with_the_option_and_its_continuation(tmp_path):
    """tests/test_swap_outfits_gpu.py's run (the size of tests/test_train_run_gpu.py, batch 4) with --part-geometry gpu --swap_weight 1."""
    import legacy
    from test_swap_outfits_gpu import _TRAIN_SCRIPT, RUN_BATCH, _process, _swap_rows
    tree = make_tree(tmp_path / 'tree')
    script = tmp_path / 'train_small.py'
    script.write_text(_TRAIN_SCRIPT)
    env = dict(os.environ, PYTHONPATH=PKG)
    out_dir = tmp_path / 'runs'
    common = ['--data', tree, '--gpus', '1', '--cfg', 'fashion', '--batch', str(RUN_BATCH), '--snap', '1', '--aug', 'noaug', '--fp32', 'true',
              '--l1_weight', '40', '--mask_weight', '20']
    _process([sys.executable, str(script), '--outdir', str(out_dir), *common, '--part-geometry', 'gpu', '--swap_weight', '1', '--kimg', '2'],
             300, env=env)
    (first,) = os.listdir(out_dir)
    assert first.endswith('-swap1-geomgpu')
    options = json.load(open(out_dir / first / 'training_options.json'))
    assert options['part_geometry'] == 'gpu' and options['swap_outfits'] == dict(region='fullbody', group=RUN_BATCH)
    _swap_rows(out_dir / first)
    snapshots = sorted(name for name in os.listdir(out_dir / first) if name.startswith('network-snapshot-'))
    assert snapshots
    with open(out_dir / first / snapshots[-1], 'rb') as f:
        data = legacy.load_network_pkl(f)
    assert all(torch.isfinite(p).all() for p in data['G_ema'].parameters())
    out = _process([sys.executable, str(script), '--outdir', str(out_dir), '--data', tree, '--continue', str(out_dir / first), '--kimg', '3'],
                   300, env=env)
    assert 'Continuing from' in out and 'Part geometry:      gpu' in out
    (second,) = [d for d in os.listdir(out_dir) if d != first]
    kept = json.load(open(out_dir / second / 'training_options.json'))
    assert kept['part_geometry'] == 'gpu' and kept['swap_outfits'] == options['swap_outfits']
    _swap_rows(out_dir / second)
