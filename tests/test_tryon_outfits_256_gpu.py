"""Outfits for the 256 x 192 model on the GPU (pasta_patch_composite_eroded_u8 with its radii and pasta_tryon_outfit_masks_u8 with
label 6 in the lower garment, csrc/tryon_pairs.hip, training.tryon_pairs.TryOnPairOutfitBatchBuilder, ``test.py --outfits`` / ``--change-region`` / ``--scores``)
-- EXACT: the per-sample-radius composite against the plain entry and the scalar radius and against a brute-force erode, the masks
entry against a numpy statement of its rule, the builder on (p, c, -) against the pair builder on every pair
of the tree, a truly mixed list against values composed from tests/tryon_pairs_ref.py (tests/tryon_outfits_256_ref.py), and the
command line against an in-process run and the region scores' numpy restatement (tests/tryon_fidelity_ref.py)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_ref as R
import tryon_fidelity_ref as F
import tryon_outfits_256_ref as OR
import tryon_pairs_ref as PR
from conftest import ROOT
from oracle import ref_patches as RP
from test_tryon_pairs_gpu import _snapshot              # the snapshot of the existing 256 end-to-end test, not a second copy of it
from tryon_pairs_tree import PAIRS, make_pair_tree

pytestmark = pytest.mark.gpu

H, W, LP = 256, 192, 32
CLI = os.path.join(ROOT, 'pasta-gan_amd', 'test.py')
BATCH = 4
# (person, upper, lower) by the tree's names.  p0 has no left knee (its thigh falls back to the hip), p1 no right ankle (its shin
# falls back to the knee): as LOWER DONORS in the last two lines they give their fall-back quadrilaterals to somebody else.  c0 has
# no shoulders and no hips; c1 and c2 are of the first sub-dataset, p3, p4 and c4 of the second.
MIXED = [('p0', 'c0', '-'), ('p1', '-', 'c1'), ('p4', 'c4', 'c4'), ('p0', 'c1', 'c2'),          # (p, c, -), (p, -, c), (p, c, c), (p, c1, c2)
         ('p1', '-', '-'), ('p4', 'c2', 'p1'), ('p3', 'c1', 'p0')]                              # (p, -, -), the two fall-back donors
U8_STAGES = ('palm', 'retain_img', 'stick', 'clothes_stick', 'lower_stick', 'lower_img', 'lower_mask', 'upper_img', 'upper_mask', 'denorm_upper',
             'denorm_lower')
PATCH_STAGES = ('patches', 'stick_patches', 'mask_patches')


def _native():
    from torch_utils.ops import _native
    return _native


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- 1. the composite with a radius per sample ----

def _composite_case(rng, n, parts, ph, pw, height, width):
    """Random patches, masks of 255 blocks with holes and near-misses of 254, and random projective maps patch -> image: the
    patch's corners onto a jittered quadrilateral that reaches beyond the image.  Part (0, 1) is invalid, the map of part (2, 3)
    singular (two corners coincide with a third: cv::invert gives zeros, every pixel reads source (0, 0))."""
    from training import patch_pipeline as PP
    patches = rng.integers(0, 256, [n, parts, ph, pw, 3], dtype=np.uint8)
    blocks = rng.uniform(size=[n, parts, ph // 2, pw // 2]) < 0.85
    mask = np.where(blocks.repeat(2, 2).repeat(2, 3), 255, 0).astype(np.uint8)
    mask[rng.uniform(size=mask.shape) < 0.01] = 254
    masks = np.repeat(mask[..., None], 3, axis=-1)
    masks[..., 1] = rng.integers(0, 256, masks.shape[:-1])       # only channel 0 decides
    corners = np.float32([[0, 0], [0, ph], [pw, ph], [pw, 0]])
    back = np.zeros([n, parts, 3, 3])
    for i in range(n):
        for k in range(parts):
            x0, y0 = rng.uniform(-6, width * 0.4), rng.uniform(-6, height * 0.4)
            quad = np.float32([[x0, y0], [x0, y0 + height * 0.6], [x0 + width * 0.6, y0 + height * 0.6], [x0 + width * 0.6, y0]])
            back[i, k] = PP.perspective_matrix(corners, quad + rng.uniform(-5, 5, [4, 2]).astype(np.float32))
    back[2, 3] = PP.perspective_matrix(corners, np.float32([[5, 5], [5, 5], [5, 5], [30, 5]]))
    assert not PP.adjugate_inverse(back[2, 3]).any() and PP.adjugate_inverse(back[2, 2]).any()
    valid = np.ones([n, parts], bool)
    valid[0, 1] = False
    return patches, masks, back, valid


@pytest.mark.parametrize('height, width', [(64, 48), (37, 29)])          # 4 x 3 whole tiles; 3 x 2 tiles with ragged edges
def test_radii_composite_equals_the_plain_and_the_scalar_entries(height, width):
    from training import patch_pipeline as PP
    rng = np.random.default_rng(20)
    n, parts, ph, pw = 3, 4, 16, 12
    radii = [0, 2, 1]
    patches, masks, back, valid = _composite_case(rng, n, parts, ph, pw, height, width)
    order = list(range(parts))
    run = lambda radius: PP.composite(_cu(patches), _cu(masks), back, valid, order, height, width, radius, want_part_masks=True)
    got, got_pm = run(radii)
    assert got.dtype == got_pm.dtype == torch.uint8 and tuple(got.shape) == (n, height, width, 3) and tuple(got_pm.shape) == (n, parts, height, width)
    # every sample against the entry it must equal: radius 0 the plain composite, radius r the scalar eroded entry at r
    scalar = {r: run(None if r == 0 else r) for r in sorted(set(radii))}
    for i, r in enumerate(radii):
        assert torch.equal(got[i], scalar[r][0][i]) and torch.equal(got_pm[i], scalar[r][1][i]), (i, r)
    eroded0 = run(0)                                                  # the scalar entry at 0 is the plain composite as well
    assert torch.equal(eroded0[0], scalar[0][0]) and torch.equal(eroded0[1], scalar[0][1])
    assert not torch.equal(scalar[0][0][1], scalar[2][0][1]) and not torch.equal(scalar[0][0][2], scalar[1][0][2])       # the erosion matters
    out_only, none = PP.composite(_cu(patches), _cu(masks), back, valid, order, height, width, radii)                      # no part masks asked for
    assert none is None and torch.equal(out_only, got)

    # and against the brute-force erode
    out, pm = got.cpu().numpy(), got_pm.cpu().numpy()
    hits = np.zeros(n, np.int64)
    for i, r in enumerate(radii):
        den = np.zeros([height, width, 3], np.uint8)
        for k in range(parts):
            if not valid[i, k]:
                assert not pm[i, k].any()
                continue
            back_img = RP.warp_perspective(patches[i, k], back[i, k], (width, height), RP.BORDER_CONSTANT)
            back_mask = RP.warp_perspective(masks[i, k], back[i, k], (width, height), RP.BORDER_CONSTANT)
            if r:
                back_mask = PR.erode(back_mask, 2 * r + 1)
            hit = (back_mask[..., 0:1] == 255).astype(np.uint8)
            den = back_img * hit + den * (1 - hit)
            assert np.array_equal(pm[i, k], hit[..., 0]), (i, k)
            hits[i] += int(hit.sum())
        assert np.array_equal(out[i], den), (i, int((out[i] != den).sum()))
    assert (hits > 0).all() and (hits < parts * height * width).all()

    # a radius the LDS tiles do not hold is refused, with the sample it belongs to
    for bad in ([0, 9, 1], [0, 2, -1]):
        with pytest.raises(ValueError, match=r'radius -?\d+ of sample [12] \(0\.\.8\)'):
            run(bad)
    with pytest.raises(ValueError, match='2 radii for 3 samples'):
        run([0, 2])
    with pytest.raises(RuntimeError, match='patch_composite_eroded_u8: null pointer'):
        N = _native()
        keep = [_cu(patches), _cu(masks), _cu(PP.inverse_maps(back, order)), _cu(valid.astype(np.uint8)), None]         # no output image
        N.check(N.lib().pasta_patch_composite_eroded_u8(*[N.ptr(t) for t in keep], None, n, parts, ph, pw, height, width, 2, None, N.stream()))


def test_radius_8_is_the_largest_and_equals_the_scalar_entry():
    """The largest halo, with per-sample radii 8 and 0 side by side: the LDS tiles are sized for 8."""
    from training import patch_pipeline as PP
    rng = np.random.default_rng(21)
    patches, masks, back, valid = _composite_case(rng, 3, 4, 16, 12, 64, 48)
    masks[...] = 255                                                  # whole quadrilaterals: something survives a 17 x 17 erosion
    run = lambda radius: PP.composite(_cu(patches), _cu(masks), back, valid, [0, 1, 2, 3], 64, 48, radius, want_part_masks=True)
    got, plain, eight = run([8, 0, 8]), run(None), run(8)
    for i, want in enumerate((eight, plain, eight)):
        assert torch.equal(got[0][i], want[0][i]) and torch.equal(got[1][i], want[1][i]), i
    assert got[1][0].any() and not torch.equal(eight[1][0], plain[1][0])
    # the entry itself with radii AND a scalar radius of 5: the scalar is not read
    N = _native()
    keep = [_cu(patches), _cu(masks), _cu(PP.inverse_maps(back, [0, 1, 2, 3])), _cu(valid.astype(np.uint8)), torch.empty_like(got[0]),
            torch.empty_like(got[1]), _cu(np.array([8, 0, 8], np.uint8))]
    N.check(N.lib().pasta_patch_composite_eroded_u8(*[N.ptr(t) for t in keep[:6]], 3, 4, 16, 12, 64, 48, 5, N.ptr(keep[6]), N.stream()))
    five = run(5)
    for i, want in enumerate((eight, plain, eight)):
        assert torch.equal(keep[4][i], want[0][i]) and torch.equal(keep[5][i], want[1][i]), i
    assert not torch.equal(five[0][0], eight[0][0]) and not torch.equal(five[0][1], plain[0][1])          # radius 5 would have shown


# ---- 2. the label masks with a source per garment ----

OUTPUTS = ('retain_img', 'upper_img', 'upper_mask', 'lower_img', 'lower_mask')


def _masks(entry, ins, n, h, w, six_is_lower):
    N = _native()
    outs = [torch.empty([n, h, h, 3], dtype=torch.uint8, device='cuda') for _ in OUTPUTS]
    N.check(entry(*[N.ptr(t) for t in list(ins) + outs], n, h, w, six_is_lower, N.stream()))
    return [t.cpu().numpy() for t in outs]


def test_pair_outfit_masks_equal_the_pair_entry_and_their_rule():
    """N = 3 at 48 x 30 (9 columns of padding, 2304 pixels = 9 blocks): the person's, a donor's and a third person's stacks."""
    rng = np.random.default_rng(0)
    n, h, w = 3, 48, 30
    lp = (h - w) // 2
    images = [rng.integers(0, 256, [n, h, w, 3], dtype=np.uint8) for _ in range(3)]
    parsings = [rng.integers(0, 20, [n, h, w], dtype=np.uint8) for _ in range(3)]
    pad = lambda a: np.pad(a, ((0, 0), (0, 0), (lp, lp)))
    palm = (np.isin(pad(parsings[0]), (14, 15)) & (rng.uniform(size=[n, h, h]) < 0.5)).astype(np.uint8)      # a palm is a hand pixel
    lib = _native().lib()
    person, a, b = ((_cu(im), _cu(lab)) for im, lab in zip(images, parsings))
    palm_t = _cu(palm)

    def rule(upper, lower):
        """_load_raw_image's expressions (tests/tryon_pairs_ref.load_pair), the upper garment of stack ``upper`` and the lower
        garment of stack ``lower``, on person_stages' padded arrays."""
        want = {k: [] for k in OUTPUTS}
        no_kp = np.zeros([18, 3])
        for i in range(n):
            image, _, parsing, _ = PR.person_stages(images[0][i], parsings[0][i], no_kp)
            u_image, _, u_parsing, _ = PR.person_stages(images[upper][i], parsings[upper][i], no_kp)
            l_image, _, l_parsing, _ = PR.person_stages(images[lower][i], parsings[lower][i], no_kp)
            head = sum((parsing == v).astype(np.uint8) for v in (1, 4, 2, 13))
            shoes = sum((parsing == v).astype(np.uint8) for v in (18, 19))
            up = sum((u_parsing == v).astype(np.uint8) for v in (5, 6, 7))
            low = sum((l_parsing == v).astype(np.uint8) for v in (9, 12, 6))
            want['retain_img'].append(image * (palm[i][..., None] + head + shoes))
            want['upper_img'].append(up * u_image)
            want['lower_img'].append(low * l_image)
            want['upper_mask'].append(np.concatenate([up] * 3, axis=2) * 255)
            want['lower_mask'].append(np.concatenate([low] * 3, axis=2) * 255)
        return [np.stack(want[k]) for k in OUTPUTS]

    stacks = (person, a, b)
    results = {}
    for upper, lower in ((1, 0), (0, 1), (1, 2), (2, 2), (0, 0)):         # the pair, swapped, two third parties, one donor, nobody
        got = _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + stacks[upper] + stacks[lower], n, h, w, 1)
        for name, g, x in zip(OUTPUTS, got, rule(upper, lower)):
            assert g.dtype == x.dtype and np.array_equal(g, x), (upper, lower, name)
            assert g.any() and not g.all(), name
        results[upper, lower] = got
    # (donor, person) is the reference's pair, compared with its rule above
    pair = dict(zip(OUTPUTS, results[1, 0]))
    # label 6 is in BOTH garments here, which six_is_lower = 0 (the 512 x 320 sets) leaves out of the lower garment
    six = _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + a + person, n, h, w, 0)
    assert np.array_equal(six[2], pair['upper_mask']) and not np.array_equal(six[4], pair['lower_mask'])
    assert ((pair['lower_mask'][..., 0] != 0) == np.isin(np.pad(parsings[0], ((0, 0), (0, 0), (lp, lp))), (6, 9, 12))).all()
    assert not np.array_equal(results[1, 2][3], results[1, 0][3]) and not np.array_equal(results[0, 1][1], results[1, 0][1])
    with pytest.raises(RuntimeError, match='tryon_outfit_masks_u8: null pointer'):
        _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + a + (b[0], None), n, h, w, 1)
    with pytest.raises(RuntimeError, match='tryon_outfit_masks_u8: bad shape'):
        _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + a + b, n, w, h, 1)


# ---- 3. and 4. the builder on the tree ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_pair_tree(tmp_path_factory.mktemp('outfits256_gpu'))


def test_the_upper_body_outfit_equals_the_pair_builder(tree):
    """(p, c, -) of every pair of the pair lists, in batches of four and one: all seven tensors and every stage both keep."""
    from training.dataset import UvitonDatasetV19_test, collate_outfits, collate_pairs, pair_as_outfit
    from training.tryon_pairs import TryOnPairBatch, TryOnPairBatchBuilder, TryOnPairOutfitBatch, TryOnPairOutfitBatchBuilder
    assert TryOnPairOutfitBatch.KEYS == TryOnPairBatch.KEYS and len(TryOnPairBatch.KEYS) == 7
    pairs = UvitonDatasetV19_test(path=tree)
    samples = [pairs[i] for i in range(len(pairs))]
    assert len(samples) == len(PAIRS) == 5
    for lo in range(0, len(samples), BATCH):
        chunk = samples[lo:lo + BATCH]
        raw = collate_outfits([pair_as_outfit(s, 'upperbody') for s in chunk])
        assert len(raw['people_name']) == 2 * len(chunk) and raw['lower_idx'].tolist() == raw['person_idx'].tolist()
        got = TryOnPairOutfitBatchBuilder('cuda').build(raw, keep_stages=True)
        want = TryOnPairBatchBuilder('cuda').build(collate_pairs(chunk), keep_stages=True)
        assert got.batch == want.batch == len(chunk) and got.person_name == want.person_name == got.lower_name
        assert got.upper_name == got.clothes_name == want.clothes_name and list(got.tensors) == TryOnPairBatch.KEYS
        for k in TryOnPairBatch.KEYS:
            assert got.tensors[k].shape == want.tensors[k].shape and torch.equal(got.tensors[k], want.tensors[k]), (lo, k)
        assert set(want.stages) <= set(got.stages) and len(want.stages) == 18
        for k, x in want.stages.items():
            if torch.is_tensor(x):
                assert got.stages[k].dtype == x.dtype and torch.equal(got.stages[k], x), (lo, k)
            else:
                assert k.endswith('_valid') and np.array_equal(got.stages[k], x), (lo, k)
        assert np.array_equal(got.stages['person_valid'], want.stages['lower_valid']) and torch.equal(got.stages['lower_stick'], want.stages['stick'])
        assert got.stages['denorm_lower'].any() and got.stages['palm'].any() and (lo > 0 or got.stages['denorm_upper'].any())
    assert TryOnPairOutfitBatchBuilder('cuda').build(raw).stages is None


def test_the_pair_view_equals_the_outfit_builder_on_deduplicated_people(tree):
    """A batch of three with pair 1 twice: TryOnPairBatchBuilder stacks its six people as they come (M = 2N), the outfit builder
    takes the same samples through ``collate_region_outfits`` with every person once (M = 4).  One launch holds a person used
    twice and people used once."""
    from training.dataset import UvitonDatasetV19_test, collate_pairs, collate_region_outfits
    from training.tryon_pairs import TryOnPairBatch, TryOnPairBatchBuilder, TryOnPairOutfitBatchBuilder
    pairs = UvitonDatasetV19_test(path=tree)
    samples = [pairs[1], pairs[0], pairs[1]]
    dedup = collate_region_outfits('upperbody', samples)
    assert len(dedup['people_name']) == 4 < 2 * len(samples)
    want = TryOnPairOutfitBatchBuilder('cuda').build(dedup, keep_stages=True)
    got = TryOnPairBatchBuilder('cuda').build(collate_pairs(samples), keep_stages=True)
    assert type(got) is TryOnPairBatch and got.batch == 3 and got.person_name == want.person_name and got.clothes_name == dedup['clothes_name']
    assert list(got.tensors) == TryOnPairBatch.KEYS
    for k in TryOnPairBatch.KEYS:
        assert got.tensors[k].shape == want.tensors[k].shape and torch.equal(got.tensors[k], want.tensors[k]), k
        assert torch.equal(got.tensors[k][0], got.tensors[k][2]), k                                      # the pair named twice
    assert not torch.equal(got.tensors['retain'][0], got.tensors['retain'][1])
    assert len(got.stages) == 18 and sorted(set(want.stages) - set(got.stages)) == ['lower_stick', 'person_valid']
    u8 = [k for k, x in got.stages.items() if torch.is_tensor(x) and x.dtype == torch.uint8]
    assert len(u8) == 15 and set(U8_STAGES) - {'lower_stick'} <= set(u8) and set(PATCH_STAGES) <= set(u8)
    for k, x in got.stages.items():
        if torch.is_tensor(x):
            assert want.stages[k].dtype == x.dtype and torch.equal(want.stages[k], x), k
        else:
            assert k.endswith('_valid') and np.array_equal(want.stages[k], x), k
    assert got.stages['denorm_upper'].any() and got.stages['denorm_lower'].any() and got.stages['palm'].any()
    assert TryOnPairBatchBuilder('cuda').build(collate_pairs(samples)).stages is None


def _listed(name):
    """'p3' -> 'UPT_subset2_256_192/p3.jpg', '-' -> '-'."""
    if name == '-':
        return name
    return ['%s/%s.jpg' % (ds, name) for ds, p, c in PAIRS if name + '.jpg' in (p, c)][0]


_EXPECTED = {}


def _expected(tree, tmp_path_factory):
    """(the list file, raw outfits, per outfit the uint8 stages of tests/tryon_outfits_256_ref.py), computed once and left as they are."""
    if tree not in _EXPECTED:
        from training.dataset import UvitonOutfits_256_test
        path = tmp_path_factory.mktemp('outfit256_list') / 'outfits.txt'
        path.write_text(''.join('%s %s %s\n' % tuple(_listed(n) for n in line) for line in MIXED))
        ds = UvitonOutfits_256_test(path=tree, outfits_file=str(path))
        samples = [ds[i] for i in range(len(ds))]
        _EXPECTED[tree] = str(path), samples, [OR.load_outfit(s) for s in samples]
    return _EXPECTED[tree]


def _batches(samples):
    from training.dataset import collate_outfits
    for lo in range(0, len(samples), BATCH):
        yield lo, collate_outfits(samples[lo:lo + BATCH])


def test_the_restatement_is_not_vacuous(tree, tmp_path_factory):
    """From the restatement alone, no GPU value: where L is not P the 5 x 5 erosion changes the lower composite; where L is P the
    eroded composite is never formed."""
    _, samples, stages = _expected(tree, tmp_path_factory)
    assert len(samples) == len(MIXED) == 7
    assert [st['own_lower'] for st in stages] == [line[2] == '-' for line in MIXED] == [True, False, False, False, True, False, False]
    changed = 0
    for line, st in zip(MIXED, stages):
        if st['own_lower']:
            assert st['lower_eroded'] is None and st['denorm_lower'] is st['lower_plain'], line
        else:
            assert st['denorm_lower'] is st['lower_eroded'], line
            differing = int((st['lower_eroded'] != st['lower_plain']).any(axis=2).sum())
            # an eroded mask is a subset of the mask, and the parts come in the same order: erosion only ever uncovers what is beneath
            print('%s: the erosion changes %d pixels of the lower composite' % (line, differing))
            changed += differing > 0
    assert changed >= 3
    # the fall-back donors: p1 gives a shin it has no ankle for, p0 a thigh it has no knee for
    assert samples[5]['lower_keypoints'][10, 2] < 0.1 and samples[6]['lower_keypoints'][12, 2] < 0.1
    hwc_part = lambda st, k: st['patches'][:, :, 3 * k:3 * k + 3]
    assert hwc_part(stages[5], 9).any() and hwc_part(stages[6], 6).any()
    assert all(st['denorm_lower'].any() for st in stages) and sum(bool(st['denorm_upper'].any()) for st in stages) >= 5


def test_a_mixed_list_equals_the_restatement(tree, tmp_path_factory, monkeypatch):
    from training import patch_pipeline
    from training.tryon_pairs import TryOnPairOutfitBatch, TryOnPairOutfitBatchBuilder
    _, samples, stages = _expected(tree, tmp_path_factory)
    solved = []
    real = patch_pipeline.part_matrices
    monkeypatch.setattr(patch_pipeline, 'part_matrices', lambda joints, *a, **k: (solved.append(len(joints)), real(joints, *a, **k))[1])
    hwc = lambda t: t.permute(0, 2, 3, 1, 4).reshape(t.shape[0], t.shape[2], t.shape[3], -1)
    builder = TryOnPairOutfitBatchBuilder('cuda')
    people = []
    for lo, raw in _batches(samples):
        del solved[:]
        b = builder.build(raw, keep_stages=True)
        assert solved == [len(raw['people_name'])]                   # one call, over the M distinct people
        people.append(len(raw['people_name']))
        n = b.batch
        assert b.person_name == raw['person_name'] and b.upper_name == raw['upper_name'] and b.lower_name == raw['lower_name']
        want = PR.generator_inputs([PR.getitem(st) for st in stages[lo:lo + n]], 'cuda')
        assert list(b.tensors) == TryOnPairOutfitBatch.KEYS
        for k in TryOnPairOutfitBatch.KEYS:
            assert b.tensors[k].shape == want[k].shape and torch.equal(b.tensors[k], want[k]), (lo, k)
        for i, ref in enumerate(stages[lo:lo + n]):
            for name in U8_STAGES:
                assert np.array_equal(b.stages[name][i].cpu().numpy(), ref[name]), (lo + i, name)
            for name in PATCH_STAGES:
                assert np.array_equal(hwc(b.stages[name])[i].cpu().numpy(), ref[name]), (lo + i, name)
            assert np.array_equal(b.stages['image'][i].cpu().numpy(), samples[lo + i]['image'])
            assert np.array_equal(b.stages['parsing'][i].cpu().numpy(), samples[lo + i]['parsing'])
        assert b.stages['palm'].any() and b.stages['denorm_upper'].any() and b.stages['denorm_lower'].any()
        assert 0 < float(b.tensors['denorm_upper_mask'].mean()) < 1 and 0 < float(b.tensors['denorm_lower_mask'].mean()) < 1
        assert tuple(b.tensors['style_input'].shape) == (n, 60, 64, 64)
        for k in ('upper_valid', 'lower_valid', 'person_valid'):
            assert b.stages[k].shape == (n, 10) and b.stages[k].dtype == bool, k
        if lo == 0:
            # one batch mixes both lower composites: sample 0 wears its own lower garment, the others somebody else's
            assert not b.stages['upper_valid'][0, [0, 1, 2, 4]].any() and b.stages['person_valid'][0, :6].all()       # c0: no shoulders, no hips
            assert np.array_equal(b.stages['lower_valid'][0], b.stages['person_valid'][0])
            assert torch.equal(b.stages['clothes_stick'][1], b.stages['stick'][1]) and not torch.equal(b.stages['lower_stick'][1], b.stages['stick'][1])
            assert torch.equal(b.stages['clothes_stick'][2], b.stages['lower_stick'][2])
        else:
            assert torch.equal(b.stages['lower_stick'][0], b.stages['stick'][0])                   # (p1, -, -)
            assert b.stages['lower_valid'][1, 9] and b.stages['lower_valid'][2, 6]                 # the shin and the thigh that fall back
    assert people == [7, 6]                                           # of 12 and 9 roles


# ---- 5. the command line ----

def _generate(G, t, z):
    """test.py's call sequence (:119-128)."""
    with torch.no_grad():
        gen_c, cat_feat_list = G.style_encoding(t['style_input'], t['retain'])
        pose_feat = G.const_encoding(t['pose'])
        ws = G.mapping(z, gen_c, truncation_psi=1)
        cat_feats = {str(c.shape[2]): c for c in cat_feat_list}
        _, gen_imgs, _, _ = G.synthesis(ws, pose_feat, cat_feats, t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                                        t['denorm_lower_mask'], noise_mode='const')
    return gen_imgs


def _files(root):
    return {os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs}


def test_cli_writes_and_scores_outfits_and_regions(tree, tmp_path, tmp_path_factory):
    import PIL.Image
    import legacy
    from metrics import tryon_fidelity as M
    listing, samples, stages = _expected(tree, tmp_path_factory)
    pkl = str(tmp_path / 'snapshot.pkl')
    _snapshot(pkl)

    # the plain command and an explicit --change-region upperbody, in this process: the same names and the same bytes
    spec = importlib.util.spec_from_file_location('pasta_test_cli_256', CLI)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    common = dict(network_pkl=pkl, seeds=None, truncation_psi=1, class_idx=None, noise_mode='const', projected_w=None, dataroot=tree,
                  batchsize=BATCH, workers=0, scores_file=None)
    plain, upper = tmp_path / 'plain', tmp_path / 'upper'
    module.generate_images.callback(outdir=str(plain), **common)
    module.generate_images.callback(outdir=str(upper), change_region='upperbody', **common)
    names = {os.path.join(ds, p[:-4] + '__' + c[:-4] + '.png') for ds, p, c in PAIRS}
    assert _files(plain) == _files(upper) == names
    for name in names:
        assert (plain / name).read_bytes() == (upper / name).read_bytes(), name
    # the other two regions keep the names and write other pictures
    lower, scores = tmp_path / 'lower', tmp_path / 'lower.json'
    module.generate_images.callback(outdir=str(lower), change_region='lowerbody', **dict(common, scores_file=str(scores)))
    assert _files(lower) == names and any((lower / name).read_bytes() != (plain / name).read_bytes() for name in names)
    report = json.loads(scores.read_text())
    assert report['mode'] == 'change-region lowerbody' and report['pairs'] == len(PAIRS) and len(report['results']) == 18

    # --outfits with --scores, in a fresh child process
    outdir, scores = tmp_path / 'out', tmp_path / 'scores' / 'scores.json'
    cmd = [sys.executable, CLI, '--network', pkl, '--dataroot', tree, '--batchsize', str(BATCH), '--workers', '0', '--outdir', str(outdir),
           '--outfits', listing, '--scores', str(scores)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    stem = lambda s, role: os.path.basename(s[role + '_name'])[:-4]
    written = [os.path.join(s['person_name'].split('/')[0], '%s__%s__%s.png' % tuple(stem(s, role) for role in ('person', 'upper', 'lower')))
               for s in samples]
    assert written[0] == os.path.join('UPT_subset1_256_192', 'p0__c0__p0.png') and written[4] == os.path.join('UPT_subset1_256_192', 'p1__p1__p1.png')
    assert written[6] == os.path.join('UPT_subset2_256_192', 'p3__c1__p0.png')                    # under the PERSON's sub-dataset
    assert _files(outdir) == set(written) and len(set(written)) == len(MIXED)
    report = json.loads(scores.read_text())
    assert sorted(report) == ['dataroot', 'mode', 'network', 'noise_mode', 'pairs', 'results']
    assert report['mode'] == 'outfits' and report['pairs'] == len(MIXED) and report['network'] == pkl and report['dataroot'] == tree
    printed = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(printed) == 1 and json.dumps(printed[0]) == json.dumps(report)       # the same line printed and written

    # the restated inputs through legacy-loaded G_ema in this process, in the same batches, with the per-item z
    with open(pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].cuda().eval().requires_grad_(False)
    rows = np.zeros([len(MIXED), 3, 5])
    differing, total = 0, 0
    for lo in range(0, len(samples), BATCH):
        index = list(range(lo, min(lo + BATCH, len(samples))))
        t = PR.generator_inputs([PR.getitem(stages[i]) for i in index], 'cuda')
        gen_imgs = _generate(G, t, M.pair_z(index, G.z_dim, 'cuda')).cpu().numpy()
        for j, i in enumerate(index):
            img = PIL.Image.open(outdir / written[i])
            assert img.mode == 'RGB' and img.size == (W, H)
            got, want = np.asarray(img), PR.image_to_u8(gen_imgs[j])
            differing, total = differing + int((got != want).sum()), total + got.size
            # the restated scores of the bytes the command line wrote
            regions = F.pair_regions(samples[i]['image'], samples[i]['parsing'], stages[i]['palm'], stages[i]['denorm_upper'],
                                     stages[i]['denorm_lower'])
            rows[i] = [[v[0] for v in F.region_stats(got[None], regions[name][1][None], regions[name][0][None])] for name in F.REGIONS]
    print('e2e outfits at 256: %d of %d values differ' % (differing, total))
    assert differing == 0, (differing, total)
    oracle, got = F.finish(rows, H * W), report['results']
    print('tryon fidelity of the outfits at 256:', got)
    assert sorted(got) == sorted('tryon_' + k for k in oracle) and len(got) == 18
    for k, v in oracle.items():
        assert np.isfinite(v), k
        assert got['tryon_' + k] == pytest.approx(v, rel=1e-12, abs=R.SSIM_TOL if k.endswith('_ssim') else 0), k
    upper_pairs, lower_pairs = (sum(bool(st[k].any()) for st in stages) for k in ('denorm_upper', 'denorm_lower'))
    assert got['tryon_keep_pairs'] == len(MIXED) and got['tryon_upper_pairs'] == upper_pairs and got['tryon_lower_pairs'] == lower_pairs == len(MIXED)
    assert 0 < got['tryon_upper_share'] < 1 and 0 < got['tryon_lower_share'] < 1 and 0 < got['tryon_keep_share'] < 1
