"""Erase strokes without a GPU (--erase-masks, --erase-strokes; include/pasta_hip.h, pasta_erase_strokes_u8): the numpy
statement (tests/erase_strokes_ref.py) held to cases whose answer is known without it, the host side of training/tryon_batch.py
against the statement, the draws, the data set without a mask directory, what the loop, the scores and the sample grid attach,
and the command line."""
import json
import os
import shutil

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import erase_strokes_ref as ER
import tryon_tree
from train_grid_tree import make_tree as make_cli_tree

DEFAULTS = dict(strokes=6, vertices=6, length=0.25, width=0.12, turn=60.0)

# ---- the specification ----

def test_spec_defaults_and_refusals():
    from training.tryon_batch import STROKES_RANGES, STROKES_SEGMENTS, STROKES_UNIFORMS, strokes_spec
    assert {k: v[1:] for k, v in STROKES_RANGES.items()} == dict(strokes=(1, 8, 6), vertices=(1, 8, 6), length=(0.01, 0.5, 0.25),
                                                                 width=(0.01, 0.25, 0.12), turn=(0.0, 180.0, 60.0))
    assert STROKES_UNIFORMS == 169 == 1 + 8 * (5 + 2 * 8) and STROKES_SEGMENTS == 64 == 8 * 8
    assert strokes_spec({}) == DEFAULTS == ER.DEFAULTS
    got = strokes_spec(dict(strokes=8.0, turn=0))
    assert got == dict(DEFAULTS, strokes=8, turn=0.0) and type(got['strokes']) is int and type(got['turn']) is float
    assert strokes_spec(dict(strokes=1, vertices=1, length=0.01, width=0.01, turn=180)) == dict(strokes=1, vertices=1, length=0.01, width=0.01, turn=180.0)
    assert strokes_spec(dict(strokes=8, vertices=8, length=0.5, width=0.25)) == dict(strokes=8, vertices=8, length=0.5, width=0.25, turn=60.0)
    for bad, words in ((dict(dots=1), "unknown name 'dots'"), (dict(strokes=0), 'strokes=0 is outside 1..8'), (dict(strokes=9), 'strokes=9 is outside 1..8'),
                       (dict(strokes=2.5), 'strokes=2.5 is not a whole number'), (dict(vertices=9), 'vertices=9 is outside 1..8'),
                       (dict(vertices=float('nan')), 'vertices=nan is not a whole number'), (dict(length=0.0), 'length=0.0 is outside 0.01..0.5'),
                       (dict(length=0.51), 'length=0.51 is outside 0.01..0.5'), (dict(width=0.3), 'width=0.3 is outside 0.01..0.25'),
                       (dict(width=float('nan')), 'width=nan is outside'), (dict(turn=-1), 'turn=-1 is outside 0..180'),
                       (dict(turn=181), 'turn=181 is outside 0..180')):
        with pytest.raises(ValueError, match=words):
            strokes_spec(bad)


# ---- the draws ----

def test_draws_depend_on_seed_and_position_only():
    from training.tryon_batch import jitter_uniforms, strokes_segments, strokes_uniforms
    u = strokes_uniforms(3, 5)
    assert u.shape == (169,) and u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
    assert u.tolist() == ER.uniforms(3, 5) and strokes_uniforms(3, 5).tobytes() == u.tobytes()
    assert not np.array_equal(strokes_uniforms(3, 6), u) and not np.array_equal(strokes_uniforms(4, 5), u)
    assert not np.array_equal(strokes_uniforms(5, 3), u)
    # the third word of the entropy: nothing of the jitter's seven uniforms comes back
    assert not np.isin((jitter_uniforms(3, 5) + 1) / 2, u).any()
    seg, counts = strokes_segments({}, 3, [0, 1, 2, 3, 2 ** 40], 256)
    assert seg.dtype == np.int32 and seg.shape == (5, 64, 5) and counts.dtype == np.int32 and counts.shape == (5,)
    # whatever else is in the batch, whatever the order
    seg2, counts2 = strokes_segments({}, 3, torch.tensor([2 ** 40, 1]), 256)
    assert seg2.tobytes() == seg[[4, 1]].tobytes() and counts2.tolist() == counts[[4, 1]].tolist()
    assert len({seg[i].tobytes() for i in range(5)}) == 5
    assert not np.array_equal(strokes_segments({}, 4, [0], 256)[0], seg[:1])


@pytest.mark.parametrize('S', [256, 512])
def test_segments_equal_the_statement(S):
    from training.tryon_batch import strokes_segments
    for spec in ({}, dict(strokes=8, vertices=8, length=0.5, width=0.25, turn=180), dict(strokes=1, vertices=1, length=0.01, width=0.01, turn=0)):
        seg, counts = strokes_segments(spec, 7, np.arange(40), S)
        want, want_counts = ER.segments(spec, 7, np.arange(40), S)
        assert np.array_equal(seg, want) and np.array_equal(counts, want_counts)
        assert (counts >= 1).all() and (counts <= dict(DEFAULTS, **spec)['strokes'] * dict(DEFAULTS, **spec)['vertices']).all()
        for n in range(40):
            k = int(counts[n])
            assert not seg[n, k:].any()
            assert (np.abs(seg[n, :k, :4]) <= 8192).all() and (seg[n, :k, 4] >= 8).all() and (seg[n, :k, 4] <= 512).all()
    # long straight strokes run into the clamps
    seg, counts = strokes_segments(dict(strokes=8, vertices=8, length=0.5, turn=0), 0, np.arange(100), 512)
    assert counts.max() <= 64 and ((seg[..., :4] == 8191).any() or (seg[..., :4] == -8192).any())


def test_the_largest_draw_fills_all_64_rows(monkeypatch):
    from training import tryon_batch
    top = 1.0 - 2.0 ** -53
    monkeypatch.setattr(tryon_batch, 'strokes_uniforms', lambda seed, position: np.full([169], top))
    monkeypatch.setattr(ER, 'uniforms', lambda seed, position: [top] * 169)
    full = dict(strokes=8, vertices=8, length=0.5, width=0.25, turn=180)
    seg, counts = tryon_batch.strokes_segments(full, 0, [0], 512)
    want, want_counts = ER.segments(full, 0, [0], 512)
    assert counts.tolist() == [64] and np.array_equal(seg, want) and want_counts.tolist() == [64]
    assert (seg[0, :, 4] == 512).all()                       # 0.25 * 512 / 2 = 64 pixels: the clamp of the half-width is its largest value
    assert tryon_batch.strokes_segments({}, 0, [0], 512)[1].tolist() == [36]


def test_a_stroke_is_a_chain_with_one_half_width():
    """Within a stroke a segment starts where the one before it ended, in Q3 too (round joins), and keeps the half-width."""
    for t in range(20):
        strokes = ER.vertices({}, 0, t, 256)
        seg, counts = ER.segments({}, 0, [t], 256)
        assert int(counts[0]) == sum(len(p) - 1 for _, p in strokes)
        k = 0
        for r, points in strokes:
            rows = seg[0, k:k + len(points) - 1]
            assert (rows[1:, :2] == rows[:-1, 2:4]).all() and (rows[:, 4] == rows[0, 4]).all()
            assert 256 * 0.12 / 6 <= r <= 256 * 0.12 / 2
            k += len(points) - 1


def test_a_changed_width_leaves_every_vertex_in_place():
    from training.tryon_batch import strokes_segments
    positions = np.arange(32)
    base, base_counts = strokes_segments({}, 0, positions, 256)
    wide, wide_counts = strokes_segments(dict(width=0.25), 0, positions, 256)
    assert np.array_equal(wide_counts, base_counts) and np.array_equal(wide[..., :4], base[..., :4])
    assert not np.array_equal(wide[..., 4], base[..., 4]) and (wide[..., 4] >= base[..., 4]).all()
    # and the other way: a changed length moves vertices, the counts, the starts and the half-widths stay
    short, short_counts = strokes_segments(dict(length=0.1), 0, positions, 256)
    assert np.array_equal(short_counts, base_counts) and np.array_equal(short[..., 4], base[..., 4])
    assert not np.array_equal(short[..., 2:4], base[..., 2:4])
    assert np.array_equal(short[:, 0, :2], base[:, 0, :2])
    # fewer strokes: the strokes that stay are the first ones, unchanged
    few, few_counts = strokes_segments(dict(strokes=1), 0, positions, 256)
    assert (few_counts <= base_counts).all() and (few_counts < base_counts).any()
    for n in range(32):
        assert np.array_equal(few[n, :few_counts[n]], base[n, :few_counts[n]])


# ---- the mask ----

@pytest.mark.parametrize('S', [256, 512])
def test_every_default_mask_has_a_set_pixel(S):
    """By construction: the start lies within 0.71 pixel of a pixel centre, a quantised half-width is at least one pixel."""
    seg, counts = ER.segments({}, 0, np.arange(256), S)
    masks = ER.mask(seg, counts, S)
    assert masks.dtype == np.uint8 and masks.shape == (256, S, S) and masks.max() == 1           # the value is 1, not 255
    cover = masks.reshape(256, -1).mean(axis=1)
    print('cover of the defaults at S = %d, positions 0..255 of seed 0: mean %.4f, min %.4f, max %.4f' % (S, cover.mean(), cover.min(), cover.max()))
    assert (cover > 0).all()
    # the pixels of a bounding box grown by r are all a segment can reach: the statement on whole planes gives the same bytes
    assert np.array_equal(ER.mask(seg[:6], counts[:6], S, whole_planes=True), masks[:6])
    # the thinnest stroke of the narrowest specification still marks its start
    seg, counts = ER.segments(dict(width=0.01, length=0.01, strokes=1, vertices=1), 0, np.arange(64), S)
    assert (seg[:, 0, 4] >= 8).all() and (ER.mask(seg, counts, S).reshape(64, -1).sum(axis=1) > 0).all()


def _one(segment, S):
    seg = np.zeros([1, 64, 5], np.int32)
    seg[0, 0] = segment
    return ER.mask(seg, np.array([1], np.int32), S)[0]


@pytest.mark.parametrize('r', [8, 16, 20, 37])
def test_a_horizontal_segment_is_a_capsule(r):
    S, xa, xb, y0 = 40, 8 * 12, 8 * 27, 8 * 20
    got = _one((xa, y0, xb, y0, r), S)
    X, Y = np.meshgrid(8 * np.arange(S), 8 * np.arange(S))
    nearest = np.clip(X, xa, xb)
    assert np.array_equal(got, ((X - nearest) ** 2 + (Y - y0) ** 2 <= r * r).astype(np.uint8))
    assert np.array_equal(_one((xb, y0, xa, y0, r), S), got)                     # either direction
    # a pixel at distance exactly r is set; with the segment 1/8 pixel further away it is not, and the pixel on the other side is
    for shift in (0, 1):
        line = y0 + (r % 8) + shift                    # pixel row (line - r) / 8 is at distance r + shift
        m = _one((xa, line, xb, line, r), S)
        above, below = (line - r - shift) // 8, (line + r) // 8
        assert 8 * above == line - r - shift
        assert m[above, 15] == (1 if shift == 0 else 0) and m[above + 1, 15] == 1
        assert m[below, 15] == 1 and m[below + 1, 15] == 0
    # the ends are discs: beside an end the column holds what the disc of radius r around the end holds, and nothing beyond r
    k = r // 8
    assert got[20, 12 - k] == 1 and got[20, 27 + k] == 1 and got[20, 12 - k - 1] == 0 and got[20, 27 + k + 1] == 0
    for side, end in ((slice(0, 12), xa), (slice(28, S), xb)):
        assert np.array_equal(got[:, side], ((X - end) ** 2 + (Y - y0) ** 2 <= r * r).astype(np.uint8)[:, side])
    # a segment of length zero is that disc
    assert np.array_equal(_one((xa, y0, xa, y0, r), S), ((X - xa) ** 2 + (Y - y0) ** 2 <= r * r).astype(np.uint8))


def test_vertices_at_the_clamps_fit_the_integers_the_rule_names():
    """The overflow bound: with both ends at the clamps and r = 512 the int64 statement equals an evaluation in Python's big
    integers, at S = 512 (the largest square of the project) and 1024 (the largest the entry takes); and every dot product and
    cross product stays inside int32, cross^2 below 2^58 (2^60 at 1024), r r L below 2^47."""
    lo, hi = -8192, 8191
    cases = [(lo, lo, hi, hi, 512), (hi, hi, lo, lo, 512), (lo, hi, hi, lo, 512), (hi, lo, lo, hi, 512), (lo, 2000, hi, 2100, 512),
             (1500, lo, 1600, hi, 512), (lo, lo, lo, lo, 512), (hi, hi, hi, hi, 512), (hi, 0, hi, hi, 8), (lo, lo, hi, lo + 1, 512)]
    rng = np.random.default_rng(0)
    for S in (512, 1024):
        seg = np.zeros([len(cases), 64, 5], np.int32)
        seg[:, 0] = cases
        masks = ER.mask(seg, np.ones(len(cases), np.int32), S, whole_planes=True)
        pixels = [(0, 0), (S - 1, S - 1), (0, S - 1), (S - 1, 0)] + [tuple(p) for p in rng.integers(0, S, [400, 2]).tolist()]
        worst32 = worst_cross2 = worst_rrl = 0
        for c, (x0, y0, x1, y1, r) in enumerate(cases):
            on = np.argwhere(masks[c])[::97]
            for py, px in pixels + [(int(a), int(b)) for a, b in on.tolist()]:
                assert bool(masks[c, py, px]) == ER.hit(px, py, x0, y0, x1, y1, r), (S, c, px, py)
                dx, dy, vx, vy, wx, wy = x1 - x0, y1 - y0, 8 * px - x0, 8 * py - y0, 8 * px - x1, 8 * py - y1
                assert max(abs(v) for v in (dx, dy, vx, vy, wx, wy)) < 2 ** 14
                cross = vx * dy - vy * dx
                worst32 = max(worst32, abs(vx * dx + vy * dy), dx * dx + dy * dy, vx * vx + vy * vy, wx * wx + wy * wy, abs(cross))
                worst_cross2, worst_rrl = max(worst_cross2, cross * cross), max(worst_rrl, r * r * (dx * dx + dy * dy))
        assert masks[0].any() and masks[2].any() and not masks[0].all()
        assert worst32 < 2 ** 31 and worst_cross2 < 2 ** 60 and worst_rrl < 2 ** 47, (S, worst32, worst_cross2, worst_rrl)
        if S == 512:
            assert worst_cross2 < 2 ** 58


def test_counts_outside_0_64_are_read_as_clamped():
    seg, _ = ER.segments({}, 1, [0, 1], 64)
    seg[:, :, :] = seg[:, :1, :]
    assert not ER.mask(seg, np.array([-5, 0]), 64).any()
    assert np.array_equal(ER.mask(seg, np.array([1000, 65]), 64), ER.mask(seg, np.array([64, 64]), 64))


# ---- the data set without a mask directory ----

@pytest.fixture(scope='module')
def bare_tree(tmp_path_factory):
    root = tryon_tree.make_tree(tmp_path_factory.mktemp('strokes_cpu'))
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    return root


def test_data_set_without_the_mask_directory(bare_tree):
    from training.dataset import ERASE_MASKS, UvitonDatasetFull, collate
    assert ERASE_MASKS == ('files', 'none', 'strokes')
    with pytest.raises(FileNotFoundError, match='train_random_mask_acgpn'):
        UvitonDatasetFull(bare_tree)
    with pytest.raises(FileNotFoundError, match='train_random_mask_acgpn'):
        UvitonDatasetFull(bare_tree, erase_masks='files')
    for kind, spec, want in (('none', None, None), ('strokes', None, DEFAULTS), ('strokes', dict(turn=10, strokes=2), dict(DEFAULTS, turn=10.0, strokes=2))):
        ds = UvitonDatasetFull(bare_tree, erase_masks=kind, erase_strokes=spec)
        assert ds.erase_masks == kind and ds.erase_strokes == want and len(ds) == len(tryon_tree.PERSONS)
        samples = [ds[i] for i in range(len(ds))]
        for s in samples:
            assert s['erase_mask'].dtype == np.uint8 and s['erase_mask'].shape == (1, 1) and not s['erase_mask'].any()
            assert sorted(s) == ['erase_mask', 'image', 'keypoints', 'parsing', 'raw_idx']
        batch = collate(samples)
        assert tuple(batch['erase_masks'].shape) == (len(ds), 1, 1) and not batch['erase_masks'].any() and (batch['erase_hw'] == 1).all()
        mirrored = UvitonDatasetFull(bare_tree, erase_masks=kind, erase_strokes=spec, mirror_people=True)
        assert len(mirrored) == 2 * len(ds) and mirrored[len(ds)]['xflip'] == 1
    for bad, words in ((dict(erase_masks='lines'), 'erase_masks'), (dict(erase_masks=None), 'erase_masks'),
                       (dict(erase_masks='none', erase_strokes={}), 'erase_strokes'), (dict(erase_strokes=dict(turn=5)), 'erase_strokes'),
                       (dict(erase_masks='strokes', erase_strokes=dict(turn=181)), 'turn=181 is outside')):
        with pytest.raises(ValueError, match=words):
            UvitonDatasetFull(bare_tree, **bad)


def test_data_set_with_files_is_what_it_was(tmp_path):
    from training.dataset import UvitonDatasetFull
    tree = tryon_tree.make_tree(tmp_path / 'tree')
    plain, files = UvitonDatasetFull(tree), UvitonDatasetFull(tree, erase_masks='files')
    assert plain.erase_masks == files.erase_masks == 'files' and plain.erase_strokes is None
    for i in range(len(plain)):
        assert np.array_equal(plain[i]['erase_mask'], files[i]['erase_mask']) and plain[i]['erase_mask'].size > 1
    # with the directory present, none and strokes still do not read it
    assert UvitonDatasetFull(tree, erase_masks='none')[0]['erase_mask'].shape == (1, 1)


def test_the_512_class_takes_the_keywords(tmp_path):
    from training.dataset import UvitonDatasetFull_512
    from tryon_512_train_tree import make_512_train_tree
    root = make_512_train_tree(tmp_path / 'tree')
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    with pytest.raises(FileNotFoundError):
        UvitonDatasetFull_512(root)
    ds = UvitonDatasetFull_512(root, erase_masks='strokes', erase_strokes=dict(width=0.2))
    assert ds.erase_strokes == dict(DEFAULTS, width=0.2) and ds[0]['erase_mask'].shape == (1, 1)


# ---- what the loop, the scores and the grid attach ----

def test_attach_strokes_and_a_batch_without_the_key():
    from training.tryon_batch import attach_strokes, strokes_batch
    raw = dict(raw_idx=torch.arange(3))
    assert attach_strokes(raw, dict(turn=5), 9, [4, 5, 2 ** 40]) is raw
    key = raw['erase_strokes']
    assert key['spec'] == dict(DEFAULTS, turn=5.0) and key['seed'] == 9 and key['positions'].dtype == np.int64
    assert key['positions'].tolist() == [4, 5, 2 ** 40]
    with pytest.raises(AssertionError):
        attach_strokes(dict(raw_idx=torch.arange(3)), {}, 0, [1, 2])
    with pytest.raises(ValueError, match='unknown name'):
        attach_strokes(dict(raw_idx=torch.arange(1)), dict(dots=3), 0, [0])
    erase, erase_hw = torch.zeros([2, 1, 1], dtype=torch.uint8), torch.ones([2, 2], dtype=torch.int32)
    got = strokes_batch(dict(raw_idx=torch.arange(2)), erase, erase_hw, 256)
    assert got[0] is erase and got[1] is erase_hw


class _RawBuilder:
    """Stands in for the GPU builder: the numbered raw batch is what ``_data_batches`` yields."""
    def __init__(self, device):
        pass

    def build(self, raw, keep_stages=False):
        return raw


def _batches(monkeypatch, tree, count, set_kwargs, **kwargs):
    from training import training_loop_wo_flow_fullbody as L
    from training import tryon_batch
    monkeypatch.setattr(tryon_batch, 'builder_for', lambda training_set, device: _RawBuilder(device))
    args = dict(num_gpus=1, rank=0, batch_size=2, random_seed=6, device='cpu',
                training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree, **set_kwargs),
                data_loader_kwargs=dict(num_workers=0))
    args.update(kwargs)
    _, _, batches = L._data_batches(**args)
    return [next(batches) for _ in range(count)]


def test_data_batches_number_the_stream_for_strokes_with_or_without_the_jitter(monkeypatch, bare_tree):
    strokes = dict(erase_masks='strokes', erase_strokes=dict(vertices=3))
    whole = _batches(monkeypatch, bare_tree, 4, strokes)
    assert [b['erase_strokes']['positions'].tolist() for b in whole] == [[0, 1], [2, 3], [4, 5], [6, 7]]
    assert all(b['erase_strokes']['seed'] == 6 and b['erase_strokes']['spec'] == dict(DEFAULTS, vertices=3) and 'jitter' not in b for b in whole)
    later = _batches(monkeypatch, bare_tree, 2, strokes, cur_nimg=3)
    assert [b['erase_strokes']['positions'].tolist() for b in later] == [[3, 4], [5, 6]]
    both = _batches(monkeypatch, bare_tree, 2, strokes, people_jitter=dict(rotate=5.0), cur_nimg=4)
    for b in both:
        assert b['jitter']['positions'].tolist() == b['erase_strokes']['positions'].tolist() and b['jitter']['seed'] == 6
    assert both[0]['jitter']['positions'].tolist() == [4, 5]
    ranks = [_batches(monkeypatch, bare_tree, 2, strokes, num_gpus=2, rank=r, batch_size=4, cur_nimg=2) for r in (0, 1)]
    assert sorted(t for r in ranks for b in r for t in b['erase_strokes']['positions'].tolist()) == list(range(2, 10))
    # none numbers nothing, and neither do files with the jitter alone
    assert all('erase_strokes' not in b and 'jitter' not in b for b in _batches(monkeypatch, bare_tree, 2, dict(erase_masks='none')))
    jittered = _batches(monkeypatch, bare_tree, 1, dict(erase_masks='none'), people_jitter=dict(rotate=5.0))
    assert 'jitter' in jittered[0] and 'erase_strokes' not in jittered[0]


@pytest.mark.parametrize('metric', ['recon_full', 'recon2k'])
def test_scores_draw_by_the_person(monkeypatch, bare_tree, metric):
    """The reconstruction metric numbers its batches with seed 0 and ``raw_idx``: the holes are a function of the person."""
    from metrics import metric_main, reconstruction
    from training import tryon_batch
    seen = []

    class Done(Exception):
        pass

    class Builder:
        def build(self, raw):
            seen.append(raw)
            raise Done
    monkeypatch.setattr(tryon_batch, 'builder_for', lambda dataset, device: Builder())
    monkeypatch.setattr(reconstruction, 'new_partials', lambda *args: None)
    kwargs = dict(class_name='training.dataset.UvitonDatasetFull', path=bare_tree, use_labels=False, max_size=None, xflip=False)
    for extra in (dict(erase_masks='strokes', erase_strokes=dict(turn=20)), dict(erase_masks='none')):
        del seen[:]
        with pytest.raises(Done):
            metric_main.calc_metric(metric, G=torch.nn.Identity(), dataset_kwargs=dict(kwargs, **extra), num_gpus=1, rank=0, device=torch.device('cpu'))
        (raw,) = seen
        if extra['erase_masks'] == 'none':
            assert 'erase_strokes' not in raw
        else:
            key = raw['erase_strokes']
            assert key['seed'] == 0 and key['spec'] == dict(DEFAULTS, turn=20.0) and key['positions'].tolist() == raw['raw_idx'].tolist()
        assert 'jitter' not in raw
    with pytest.raises(FileNotFoundError):
        metric_main.calc_metric(metric, G=torch.nn.Identity(), dataset_kwargs=kwargs, num_gpus=1, rank=0, device=torch.device('cpu'))


def test_sample_grid_draws_by_the_person(monkeypatch, tmp_path):
    from training import snapshot_grid
    from training.dataset import UvitonDatasetFull
    root = make_cli_tree(tmp_path / 'tree')
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    seen = []

    class Done(Exception):
        pass

    class Builder:
        def build(self, raw, keep_stages=False):
            seen.append(raw)
            raise Done
    for kind in ('strokes', 'none'):
        ds = UvitonDatasetFull(root, erase_masks=kind)
        with pytest.raises(Done):
            snapshot_grid.SnapshotGrid.setup(ds, Builder(), 'cpu', gnum=3)
    assert seen[0]['erase_strokes']['seed'] == 0 and seen[0]['erase_strokes']['positions'].tolist() == seen[0]['raw_idx'].tolist()
    assert seen[0]['erase_strokes']['spec'] == DEFAULTS and 'erase_strokes' not in seen[1]


# ---- the command line ----

@pytest.fixture(scope='module')
def cli_tree(tmp_path_factory):
    return make_cli_tree(tmp_path_factory.mktemp('strokes_cli'))


@pytest.fixture(scope='module')
def bare_cli_tree(tmp_path_factory):
    root = make_cli_tree(tmp_path_factory.mktemp('strokes_cli_bare'))
    shutil.rmtree(os.path.join(root, 'train_random_mask_acgpn'))
    return root


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_erase_masks_option(cli_tree, bare_cli_tree, tmp_path):
    plain = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion')
    files = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--erase-masks', 'files')
    assert plain.exit_code == 0 and files.exit_code == 0, (plain.output, files.output)
    a = _options(plain.output)
    # files is today's behaviour: the recorded options and the run's name do not know the option
    assert _options(files.output) == a and 'Erase masks:        files\n' in plain.output
    name = os.path.basename(a.pop('run_dir'))
    assert not any('erase' in k for k in list(a) + list(a['training_set_kwargs'])) and '-erase' not in name
    for kind, extra, strokes, printed in (
            ('none', (), None, 'Erase masks:        none\n'),
            ('strokes', (), DEFAULTS, 'Erase masks:        strokes (strokes=6,vertices=6,length=0.25,width=0.12,turn=60)\n'),
            ('strokes', ('--erase-strokes', 'turn=90, strokes=3'), dict(DEFAULTS, turn=90.0, strokes=3),
             'Erase masks:        strokes (strokes=3,vertices=6,length=0.25,width=0.12,turn=90)\n')):
        for tree in (cli_tree, bare_cli_tree):
            on = _run(tree, tmp_path / 'runs', '--cfg', 'fashion', '--erase-masks', kind, *extra)
            assert on.exit_code == 0, on.output
            b = _options(on.output)
            assert b['training_set_kwargs'].pop('erase_masks') == kind
            assert b['training_set_kwargs'].pop('erase_strokes', None) == strokes
            want_name = name.replace('-fashion', '-erase%s-fashion' % kind).replace(os.path.basename(cli_tree), os.path.basename(tree))
            assert os.path.basename(b.pop('run_dir')) == want_name
            assert b['training_set_kwargs'].pop('path') == tree and printed in on.output
            assert b == dict(a, training_set_kwargs={k: v for k, v in a['training_set_kwargs'].items() if k != 'path'})
    # the tree without masks does not open with files
    res = _run(bare_cli_tree, tmp_path / 'runs', '--cfg', 'fashion')
    assert res.exit_code != 0 and 'train_random_mask_acgpn' in res.output
    # after the mirror and the jitter in the name, as in the batch; the held-out tree inherits the option
    both = _run(bare_cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--mirror-people', 'true', '--jitter-people', 'shift=0.1', '--erase-masks',
                'strokes', '--metrics', 'recon_full', '--metrics_data', bare_cli_tree)
    assert both.exit_code == 0, both.output
    got = _options(both.output)
    assert '-mirrorpeople-jitterpeople-erasestrokes-fashion' in got['run_dir']
    assert got['metric_set_kwargs']['erase_masks'] == 'strokes' and got['metric_set_kwargs']['erase_strokes'] == DEFAULTS


@pytest.mark.parametrize('args,words', [
    (('--erase-masks', 'lines'), "'lines' is not one of"), (('--erase-strokes', 'turn=5'), '--erase-strokes needs --erase-masks strokes (it is files)'),
    (('--erase-masks', 'none', '--erase-strokes', 'turn=5'), '--erase-strokes needs --erase-masks strokes (it is none)'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'dots=5'), "--erase-strokes: unknown name 'dots'"),
    (('--erase-masks', 'strokes', '--erase-strokes', 'turn=5,turn=6'), '--erase-strokes: turn is given twice'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'strokes=9'), '--erase-strokes: strokes=9.0 is outside 1..8'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'vertices=0'), '--erase-strokes: vertices=0.0 is outside 1..8'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'strokes=1.5'), '--erase-strokes: strokes=1.5 is not a whole number'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'length=0.6'), '--erase-strokes: length=0.6 is outside 0.01..0.5'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'width=0'), '--erase-strokes: width=0.0 is outside 0.01..0.25'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'turn=200'), '--erase-strokes: turn=200.0 is outside 0..180'),
    (('--erase-masks', 'strokes', '--erase-strokes', 'turn'), "--erase-strokes: 'turn' is not name=value"),
    (('--erase-masks', 'strokes', '--erase-strokes', 'turn=much'), '--erase-strokes: turn=much is not a number')])
def test_erase_option_refusals(cli_tree, tmp_path, args, words):
    res = _run(cli_tree, tmp_path / 'runs', '--cfg', 'fashion', *args)
    assert res.exit_code != 0 and words in res.output, res.output


def test_continue_keeps_the_options_and_refuses_them_again(bare_cli_tree, tmp_path):
    from training import train_state
    res = _run(bare_cli_tree, tmp_path / 'runs', '--cfg', 'fashion', '--batch', '2', '--kimg', '5', '--erase-masks', 'strokes', '--erase-strokes', 'width=0.2')
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=2, batch_gpu=2, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    res = _run(bare_cli_tree, tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['training_set_kwargs']['erase_masks'] == 'strokes' and got['training_set_kwargs']['erase_strokes'] == dict(DEFAULTS, width=0.2)
    assert 'Erase masks:        strokes (strokes=6,vertices=6,length=0.25,width=0.2,turn=60)' in res.output
    name = os.path.basename(got['run_dir'])
    assert '-erasestrokes-fashion-' in name and name.endswith('-continue000000')
    res = _run(bare_cli_tree, tmp_path / 'out', '--continue', str(run_dir), '--erase-masks', 'strokes')
    assert res.exit_code != 0 and '--erase-masks cannot be given with --continue' in res.output, res.output
    res = _run(bare_cli_tree, tmp_path / 'out', '--continue', str(run_dir), '--erase-strokes', 'width=0.2')
    assert res.exit_code != 0 and '--erase-strokes cannot be given with --continue' in res.output, res.output
    # a held-out tree named at the continuation takes the recorded option
    res = _run(bare_cli_tree, tmp_path / 'out', '--continue', str(run_dir), '--metrics', 'recon_full', '--metrics_data', bare_cli_tree)
    assert res.exit_code == 0, res.output
    assert _options(res.output)['metric_set_kwargs']['erase_masks'] == 'strokes'


def test_calc_metrics_takes_the_options_and_defaults_to_what_the_snapshot_recorded(monkeypatch, cli_tree, bare_cli_tree, tmp_path):
    import calc_metrics
    import legacy
    res = CliRunner().invoke(calc_metrics.calc_metrics, ['--help'])
    text = ' '.join(res.output.split())
    assert res.exit_code == 0 and '--erase-masks' in text and '--erase-strokes' in text and 'as the snapshot recorded' in text
    pkl = tmp_path / 'network-snapshot-000000.pkl'
    pkl.write_bytes(b'stands in for a snapshot')
    seen = []
    monkeypatch.setattr(calc_metrics, 'subprocess_fn', lambda rank, args, temp_dir: seen.append(dict(args.dataset_kwargs)))
    wide = dict(DEFAULTS, width=0.2)

    def run(recorded, *extra):
        monkeypatch.setattr(legacy, 'load_network_pkl', lambda f: dict(training_set_kwargs=dict(
            class_name='training.dataset.UvitonDatasetFull', path=bare_cli_tree, use_labels=False, max_size=9, xflip=False, **recorded)))
        del seen[:]
        res = CliRunner().invoke(calc_metrics.calc_metrics, ['--network', str(pkl), '--verbose', 'false', *extra])
        return res, ({k: v for k, v in seen[0].items() if k.startswith('erase') or k == 'path'} if seen else None)
    strokes = dict(erase_masks='strokes', erase_strokes=wide)
    # the default is what the snapshot recorded, on its own tree and on a tree named
    assert run(strokes)[1] == dict(path=bare_cli_tree, **strokes)
    assert run(strokes, '--data', cli_tree)[1] == dict(path=cli_tree, **strokes)
    assert run({})[1] == dict(path=bare_cli_tree) and run({}, '--data', cli_tree)[1] == dict(path=cli_tree)
    assert run(dict(erase_masks='none'), '--data', cli_tree)[1] == dict(path=cli_tree, erase_masks='none')
    # given, the options replace the recorded ones: a snapshot trained on files is scored on a tree that has none
    assert run({}, '--data', bare_cli_tree, '--erase-masks', 'none')[1] == dict(path=bare_cli_tree, erase_masks='none')
    assert run({}, '--erase-masks', 'strokes')[1] == dict(path=bare_cli_tree, erase_masks='strokes', erase_strokes=DEFAULTS)
    assert run(strokes, '--erase-masks', 'none')[1] == dict(path=bare_cli_tree, erase_masks='none')
    assert run(strokes, '--erase-masks', 'files')[1] == dict(path=bare_cli_tree)
    assert run(strokes, '--erase-masks', 'strokes')[1] == dict(path=bare_cli_tree, erase_masks='strokes', erase_strokes=DEFAULTS)
    assert run(strokes, '--erase-strokes', 'turn=10')[1] == dict(path=bare_cli_tree, erase_masks='strokes', erase_strokes=dict(DEFAULTS, turn=10.0))
    for recorded, extra, words in (({}, ('--erase-strokes', 'turn=10'), '--erase-strokes needs --erase-masks strokes (it is files)'),
                                   (strokes, ('--erase-masks', 'none', '--erase-strokes', 'turn=10'), '--erase-strokes needs --erase-masks strokes (it is none)'),
                                   (strokes, ('--erase-strokes', 'turn=200'), '--erase-strokes: turn=200.0 is outside 0..180'),
                                   ({}, ('--erase-masks', 'lines'), "'lines' is not one of")):
        res, kwargs = run(recorded, *extra)
        assert res.exit_code != 0 and words in res.output and kwargs is None, res.output
