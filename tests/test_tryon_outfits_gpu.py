"""Outfits at 512 x 320 on the GPU (pasta_tryon_outfit_masks_u8 / pasta_tryon_outfit_assemble of csrc/tryon_pairs.hip,
training.tryon_regions.TryOnOutfitBatchBuilder, ``test_512.py --outfits`` and ``--scores``) -- EXACT: the entries against a numpy
statement of their rule and test_512.py's expressions, the builder against the region builder on the three
degenerate outfits of every pair and on a batch that names a pair twice, a truly mixed list against values composed from tests/tryon_512_ref.py, and the command line
against an in-process run and the region scores' numpy restatement (tests/tryon_fidelity_ref.py)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_ref as R
import tryon_512_ref as FR
import tryon_fidelity_ref as F
from conftest import ROOT
from test_tryon_512_gpu import G512_45, _snapshot       # the snapshot of the existing 512 end-to-end test, not a second copy of it
from tryon_512_tree import PAIRS, make_512_tree

pytestmark = pytest.mark.gpu

H, W, LP = 512, 320, 96
CLI = os.path.join(ROOT, 'pasta-gan_amd', 'test_512.py')
OUTPUTS = ('retain_img', 'upper_img', 'upper_mask', 'lower_img', 'lower_mask')
# (person, upper, lower) by the tree's names: 'p3' has an empty ``people``, and so has 'c4'; c2 is Zalora's, c3 Deepfashion's
MIXED = [('p0', 'c0', 'c1'), ('p0', 'c2', 'c3'), ('p1', '-', '-'), ('p3', 'c1', 'c0'), ('p4', 'c4', 'c2'), ('p2', 'c0', 'c0'), ('p1', 'c0', '-')]
BATCH = 4                                                            # seven lines: batches of 4 and 3


def _native():
    from torch_utils.ops import _native
    return _native


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _listed(name):
    """'p3' -> 'Deepfashion_512_320/p3.jpg', '-' -> '-'."""
    if name == '-':
        return name
    return ['%s/%s.jpg' % (ds, name) for ds, p, c in PAIRS if name + '.jpg' in (p, c)][0]


def _write_list(path, outfits):
    path.write_text(''.join('%s %s %s\n' % tuple(_listed(n) for n in line) for line in outfits))
    return str(path)


# ---- 1. the entries ----

def _masks(entry, ins, n, h, w, *extra):
    N = _native()
    outs = [torch.empty([n, h, h, 3], dtype=torch.uint8, device='cuda') for _ in OUTPUTS]
    N.check(entry(*[N.ptr(t) for t in list(ins) + outs], n, h, w, *extra, N.stream()))
    return [t.cpu().numpy() for t in outs]


def test_outfit_masks_equal_their_rule_and_the_region_entry():
    """N = 3 at 48 x 30 (9 columns of padding, 2304 pixels = 9 blocks): three distinct source stacks."""
    rng = np.random.default_rng(0)
    n, h, w = 3, 48, 30
    lp = (h - w) // 2
    image, a_image, b_image = (rng.integers(0, 256, [n, h, w, 3], dtype=np.uint8) for _ in range(3))
    parsing, a_parsing, b_parsing = (rng.integers(0, 20, [n, h, w], dtype=np.uint8) for _ in range(3))
    pad = lambda a, v: np.pad(a, ((0, 0), (0, 0), (lp, lp)) + ((0, 0),) * (a.ndim - 3), constant_values=v)
    palm = (np.isin(pad(parsing, 0), (14, 15)) & (rng.uniform(size=[n, h, h]) < 0.5)).astype(np.uint8)      # a palm is a hand pixel
    lib = _native().lib()
    person, a, b = (_cu(image), _cu(parsing)), (_cu(a_image), _cu(a_parsing)), (_cu(b_image), _cu(b_parsing))
    palm_t = _cu(palm)
    got = _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + a + b, n, h, w, 0)

    # the rule: labels and images padded with 0 and 255; retain from the person, upper and lower from a source each
    label = pad(parsing, 0)
    keep = np.isin(label, (18, 19)).astype(np.uint8) + palm + np.isin(label, (1, 2, 4, 13)).astype(np.uint8)
    mask3 = lambda m: np.repeat(m[..., None], 3, axis=3).astype(np.uint8) * 255

    def rule(up, low):
        upper, lower = np.isin(pad(up[1], 0), (5, 6, 7)), np.isin(pad(low[1], 0), (9, 12))
        return [keep[..., None] * pad(image, 255), upper[..., None] * pad(up[0], 255), mask3(upper), lower[..., None] * pad(low[0], 255),
                mask3(lower)]
    host = dict(person=(image, parsing), a=(a_image, a_parsing), b=(b_image, b_parsing))
    want = rule(host['a'], host['b'])
    assert keep.max() == 1
    for name, g, x in zip(OUTPUTS, got, want):
        assert g.dtype == x.dtype and np.array_equal(g, x), name
        assert g.any() and not g.all(), name
    assert not got[0][:, :, :lp].any() and not got[0][:, :, lp + w:].any()                # label 0 and no palm there: nothing is kept
    assert not got[2][:, :, :lp].any() and not got[4][:, :, lp + w:].any()                # label 0 there: no garment

    # one donor: the three regions (full, upper, lower body) are three choices of the two sources, the person's own pointers among them
    device = dict(person=person, a=a)
    for up, low in (('a', 'a'), ('a', 'person'), ('person', 'a')):
        outfit = _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + device[up] + device[low], n, h, w, 0)
        for name, g, x in zip(OUTPUTS, outfit, rule(host[up], host[low])):
            assert np.array_equal(g, x), (up, low, name)
    assert not np.array_equal(got[3], outfit[3])                     # B's lower garment is not A's
    with pytest.raises(RuntimeError, match='tryon_outfit_masks_u8: null pointer'):
        _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + a + (b[0], None), n, h, w, 0)
    with pytest.raises(RuntimeError, match='tryon_outfit_masks_u8: bad shape'):
        _masks(lib.pasta_tryon_outfit_masks_u8, person + (palm_t,) + a + b, n, w, h, 0)


def test_outfit_assemble_equals_two_region_assembles():
    """All ten outputs against test_512.py's expressions (tests/tryon_512_ref.generator_inputs): the nine of the pair (person,
    upper donor), and clothes_lower = the restatement's ``clothes`` of the pair (person, lower donor)."""
    from training.tryon_regions import TryOnOutfitBatch, TryOnRegionBatch
    assert TryOnOutfitBatch.KEYS == TryOnRegionBatch.KEYS + ['clothes_lower']
    rng = np.random.default_rng(1)
    n, h, w, pu, pl, ph, pw = 3, 48, 30, 3, 2, 6, 5
    lp = (h - w) // 2
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    pad = lambda a: np.pad(a, ((0, 0), (0, 0), (lp, lp), (0, 0)), constant_values=255)
    image, a_image, b_image, stick = u8(n, h, w, 3), u8(n, h, w, 3), u8(n, h, w, 3), u8(n, h, h, 3)
    retain_mask = (rng.uniform(size=[n, h, h, 1]) < 0.5).astype(np.uint8)
    patches, patches_l, den_u, den_l = u8(n, pu, ph, pw, 3), u8(n, pl, ph, pw, 3), u8(n, h, h, 3), u8(n, h, h, 3)

    def restated(clothes):
        stages = [dict(image=pad(image)[i], clothes=pad(clothes)[i], stick=stick[i], retain_mask=retain_mask[i],
                       patches=patches[i].transpose(1, 2, 0, 3).reshape(ph, pw, 3 * pu),
                       patches_lower=patches_l[i].transpose(1, 2, 0, 3).reshape(ph, pw, 3 * pl), denorm_upper=den_u[i], denorm_lower=den_l[i])
                  for i in range(n)]
        return FR.generator_inputs([FR.getitem(s) for s in stages], 'cuda')
    want = dict(restated(a_image), clothes_lower=restated(b_image)['clothes'])
    assert list(want) == TryOnOutfitBatch.KEYS
    N = _native()
    lib = N.lib()
    photos = [_cu(x) for x in (image, a_image, b_image)]
    rest = [_cu(x) for x in (retain_mask * pad(image), stick, patches, patches_l, den_u, den_l)]
    outfit = {k: torch.full_like(want[k], float('nan')) for k in TryOnOutfitBatch.KEYS}
    outs = (ctypes.c_void_p * 10)(*[outfit[k].data_ptr() for k in TryOnOutfitBatch.KEYS])
    N.check(lib.pasta_tryon_outfit_assemble(*[N.ptr(x) for x in photos + rest], outs, n, h, w, pu, pl, ph, pw, N.stream()))
    for k in TryOnOutfitBatch.KEYS:
        assert torch.equal(outfit[k], want[k]) and not torch.isnan(outfit[k]).any(), k
    assert not torch.equal(outfit['clothes_lower'], outfit['clothes'])
    assert float(outfit['clothes_lower'][..., :lp].min()) == 1.0                             # white padding
    with pytest.raises(RuntimeError, match='tryon_outfit_assemble: null photograph'):
        N.check(lib.pasta_tryon_outfit_assemble(*[N.ptr(x) for x in photos[:2] + [None] + rest], outs, n, h, w, pu, pl, ph, pw, N.stream()))
    with pytest.raises(RuntimeError, match='tryon_outfit_assemble: output 8 is null'):
        outs = (ctypes.c_void_p * 10)(*[outfit[k].data_ptr() for k in TryOnOutfitBatch.KEYS[:8]], None, outfit['clothes_lower'].data_ptr())
        N.check(lib.pasta_tryon_outfit_assemble(*[N.ptr(x) for x in photos + rest], outs, n, h, w, pu, pl, ph, pw, N.stream()))


# ---- 2. and 3. the builder on the tree ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_512_tree(tmp_path_factory.mktemp('outfits512_gpu'))


def _outfits(tree, listing):
    from training.dataset import UvitonOutfits_512_test
    ds = UvitonOutfits_512_test(path=tree, outfits_file=listing)
    return [ds[i] for i in range(len(ds))]


def test_degenerate_outfits_equal_the_region_builder(tree, tmp_path):
    """(p, c, c), (p, c, -) and (p, -, c) of every pair of the pair lists are full body, upper body and lower body."""
    from training.dataset import UvitonDatasetFull_512_test, collate_outfits, collate_pairs
    from training.tryon_regions import TryOnOutfitBatchBuilder, TryOnRegionBatch, TryOnRegionBatchBuilder
    stem = lambda f: f[:-len('.jpg')]
    forms = dict(fullbody=lambda p, c: (p, c, c), upperbody=lambda p, c: (p, c, '-'), lowerbody=lambda p, c: (p, '-', c))
    for region, form in forms.items():
        listing = _write_list(tmp_path / (region + '.txt'), [form(stem(p), stem(c)) for _, p, c in PAIRS])
        raw = collate_outfits(_outfits(tree, listing))
        assert len(raw['people_name']) == 2 * len(PAIRS)
        got = TryOnOutfitBatchBuilder('cuda').build(raw, keep_stages=True)
        pairs = UvitonDatasetFull_512_test(path=tree, change_region=region)
        want = TryOnRegionBatchBuilder('cuda', region).build(collate_pairs([pairs[i] for i in range(len(pairs))]), keep_stages=True)
        assert got.batch == want.batch == len(PAIRS) and got.person_name == want.person_name
        assert got.upper_name == (want.person_name if region == 'lowerbody' else want.clothes_name)
        assert got.lower_name == (want.person_name if region == 'upperbody' else want.clothes_name)
        donor = want.tensors['clothes']
        for k in TryOnRegionBatch.KEYS:
            x = want.tensors['image'] if (k == 'clothes' and region == 'lowerbody') else want.tensors[k]     # the upper garment's owner
            assert torch.equal(got.tensors[k], x), (region, k)
        assert torch.equal(got.tensors['clothes_lower'], want.tensors['image'] if region == 'upperbody' else donor), region
        shared = [k for k in want.stages if k in got.stages and torch.is_tensor(want.stages[k]) and want.stages[k].dtype == torch.uint8]
        assert len(shared) == 15 and {'image', 'parsing', 'palm', 'patches_lower', 'denorm_lower'} <= set(shared)
        for k in shared:
            assert torch.equal(got.stages[k], want.stages[k]), (region, k)
        assert torch.equal(got.stages['M_invs'], want.stages['M_invs'])
        assert np.array_equal(got.stages['person_valid'], want.stages['person_valid'])
        donor_valid = got.stages['lower_valid' if region == 'lowerbody' else 'upper_valid']
        assert np.array_equal(donor_valid, want.stages['clothes_valid'])
        assert got.stages['denorm_upper'].any() and got.stages['denorm_lower'].any() and not torch.equal(got.tensors['image'], donor)


def test_the_pair_view_equals_the_outfit_builder_on_deduplicated_people(tree):
    """A batch of three with pair 0 twice: TryOnRegionBatchBuilder stacks its six people as they come (M = 2N), the outfit builder
    takes the same samples through ``collate_region_outfits`` with every person once (M = 4).  One launch holds a person used
    twice and people used once.  The pair view has the nine tensors and no tenth, and its ``clothes`` is the donor's photograph
    in every region."""
    from training.dataset import UvitonDatasetFull_512_test, collate_pairs, collate_region_outfits
    from training.tryon_regions import TryOnOutfitBatchBuilder, TryOnRegionBatch, TryOnRegionBatchBuilder
    donors = {}
    for region in ('fullbody', 'upperbody', 'lowerbody'):
        pairs = UvitonDatasetFull_512_test(path=tree, change_region=region)
        samples = [pairs[0], pairs[1], pairs[0]]
        dedup = collate_region_outfits(region, samples)
        assert len(dedup['people_name']) == 4 < 2 * len(samples)
        want = TryOnOutfitBatchBuilder('cuda').build(dedup, keep_stages=True)
        builder = TryOnRegionBatchBuilder('cuda', region)
        plain, got = builder.build(collate_pairs(samples)), builder.build(collate_pairs(samples), keep_stages=True)
        assert list(plain.tensors) == list(got.tensors) == TryOnRegionBatch.KEYS and len(TryOnRegionBatch.KEYS) == 9       # no tenth tensor
        assert plain.stages is None and got.batch == 3 and got.person_name == want.person_name and got.clothes_name == dedup['clothes_name']
        for k in TryOnRegionBatch.KEYS:
            x = want.tensors['clothes_lower'] if (k == 'clothes' and region == 'lowerbody') else want.tensors[k]        # the donor's
            assert got.tensors[k].shape == x.shape and torch.equal(got.tensors[k], x), (region, k)
            assert torch.equal(plain.tensors[k], x), (region, k)
            assert torch.equal(got.tensors[k][0], got.tensors[k][2]), (region, k)                                           # the pair named twice
        shared = [k for k in got.stages if k in want.stages and torch.is_tensor(got.stages[k]) and got.stages[k].dtype == torch.uint8]
        assert len(shared) == 15 and {'image', 'parsing', 'palm', 'patches_lower', 'denorm_lower'} <= set(shared)
        for k in shared:
            assert torch.equal(got.stages[k], want.stages[k]), (region, k)
        assert torch.equal(got.stages['M_invs'], want.stages['M_invs']) and np.array_equal(got.stages['person_valid'], want.stages['person_valid'])
        assert np.array_equal(got.stages['clothes_valid'], want.stages['lower_valid' if region == 'lowerbody' else 'upper_valid'])
        assert sorted(set(got.stages) - set(want.stages)) == ['clothes_valid']
        assert got.stages['denorm_upper'].any() and got.stages['denorm_lower'].any() and got.stages['palm'].any()
        donors[region] = got.tensors['clothes']
        assert not torch.equal(got.tensors['clothes'], got.tensors['image'])
    assert torch.equal(donors['lowerbody'], donors['fullbody']) and torch.equal(donors['upperbody'], donors['fullbody'])


_EXPECTED = {}


def _expected(tree, tmp_path_factory):
    """(the list file, raw outfits, per outfit the uint8 stages composed from tests/tryon_512_ref.py), computed once: the upper
    side from the upper-body preparation of (person, upper donor), the lower side from the lower-body preparation of (person,
    lower donor), everything else the person's."""
    if tree in _EXPECTED:
        return _EXPECTED[tree]
    listing = _write_list(tmp_path_factory.mktemp('outfit_list') / 'outfits.txt', MIXED)
    samples = _outfits(tree, listing)
    sides = {}

    def side(s, prefix, region):
        key = (s['person_name'], s[prefix + 'name'], region)
        if key not in sides:
            raw = dict(image=s['image'], parsing=s['parsing'], keypoints=s['keypoints'], clothes_image=s[prefix + 'image'],
                       clothes_parsing=s[prefix + 'parsing'], clothes_keypoints=s[prefix + 'keypoints'])
            st = FR.label_stages(raw, region)
            st['normalized'] = FR.normalize_region(region, st['upper_img'], st['lower_img'], st['upper_mask'], st['lower_mask'], st['clothes_kp'],
                                                   st['kp'])
            sides[key] = st
        return sides[key]

    stages = []
    for s in samples:
        up, lo = side(s, 'upper_', 'upperbody'), side(s, 'lower_', 'lowerbody')
        assert np.array_equal(up['retain_img'], lo['retain_img']) and np.array_equal(up['stick'], lo['stick'])      # the person's, either way
        stages.append(dict(image=up['image'], clothes=up['clothes'], clothes_lower=lo['clothes'], stick=up['stick'], palm=up['palm'],
                           retain_mask=up['retain_mask'], retain_img=up['retain_img'], upper_img=up['upper_img'], upper_mask=up['upper_mask'],
                           lower_img=lo['lower_img'], lower_mask=lo['lower_mask'], patches=up['normalized'][0], mask_patches=up['normalized'][2],
                           denorm_upper=up['normalized'][4], patches_lower=lo['normalized'][1], mask_patches_lower=lo['normalized'][3],
                           denorm_lower=lo['normalized'][5]))
    _EXPECTED[tree] = listing, samples, stages
    return _EXPECTED[tree]


def _expected_tensors(stages):
    """The ten fp32 tensors of a batch of expected stages: test_512.py's expressions as tests/tryon_512_ref.py states them;
    ``clothes_lower`` is ``clothes`` of the same items with the lower donor's photograph."""
    want = FR.generator_inputs([FR.getitem(st) for st in stages], 'cuda')
    want['clothes_lower'] = FR.generator_inputs([FR.getitem(dict(st, clothes=st['clothes_lower'])) for st in stages], 'cuda')['clothes']
    return want


def _batches(samples):
    from training.dataset import collate_outfits
    for lo in range(0, len(samples), BATCH):
        yield lo, collate_outfits(samples[lo:lo + BATCH])


def test_a_mixed_list_equals_the_restatement(tree, tmp_path_factory, monkeypatch):
    from training import patch_pipeline
    from training.tryon_regions import TryOnOutfitBatch, TryOnOutfitBatchBuilder
    _, samples, stages = _expected(tree, tmp_path_factory)
    assert len(samples) == len(MIXED) == 7
    solved = []
    real = patch_pipeline.part_matrices
    monkeypatch.setattr(patch_pipeline, 'part_matrices', lambda joints, *a, **k: (solved.append(len(joints)), real(joints, *a, **k))[1])
    hwc = lambda t: t.permute(0, 2, 3, 1, 4).reshape(t.shape[0], t.shape[2], t.shape[3], -1)
    builder = TryOnOutfitBatchBuilder('cuda')
    people = []
    for lo, raw in _batches(samples):
        del solved[:]
        b = builder.build(raw, keep_stages=True)
        assert solved == [len(raw['people_name'])]                   # one call, over the M distinct people
        people.append(len(raw['people_name']))
        n = b.batch
        assert b.person_name == raw['person_name'] and b.upper_name == raw['upper_name'] and b.lower_name == raw['lower_name']
        want = _expected_tensors(stages[lo:lo + n])
        assert list(b.tensors) == TryOnOutfitBatch.KEYS
        for k in TryOnOutfitBatch.KEYS:
            assert b.tensors[k].shape == want[k].shape and torch.equal(b.tensors[k], want[k]), (lo, k)
        for i, ref in enumerate(stages[lo:lo + n]):
            for name in ('stick', 'palm', 'retain_img', 'upper_img', 'upper_mask', 'lower_img', 'lower_mask', 'denorm_upper', 'denorm_lower'):
                assert np.array_equal(b.stages[name][i].cpu().numpy(), ref[name]), (lo + i, name)
            for name in ('patches', 'patches_lower', 'mask_patches', 'mask_patches_lower'):
                assert np.array_equal(hwc(b.stages[name])[i].cpu().numpy(), ref[name]), (lo + i, name)
            assert np.array_equal(b.stages['image'][i].cpu().numpy(), samples[lo + i]['image'])
            assert np.array_equal(b.stages['parsing'][i].cpu().numpy(), samples[lo + i]['parsing'])
        # nothing passes vacuously
        assert b.stages['palm'].any() and b.stages['denorm_upper'].any() and b.stages['denorm_lower'].any()
        assert 0 < float(b.tensors['denorm_upper_mask'].mean()) < 1 and 0 < float(b.tensors['denorm_lower_mask'].mean()) < 1
        assert tuple(b.tensors['style_input'].shape) == (n, 45, 128, 128)
        if lo == 0:
            pv = b.stages['person_valid']
            assert not pv[3].any() and pv[0].all()                   # p3: empty ``people``; nothing is warped back onto it
            assert not b.stages['denorm_upper'][3].any() and not b.stages['denorm_lower'][3].any()
            assert b.stages['upper_valid'][3].any() and b.stages['patches'][3].any()        # its donors' patches still enter the style
            assert not torch.equal(b.tensors['clothes'][0], b.tensors['clothes_lower'][0])
            assert torch.equal(b.tensors['clothes'][2], b.tensors['image'][2]) and torch.equal(b.tensors['clothes_lower'][2], b.tensors['image'][2])
        else:
            assert not b.stages['upper_valid'][0].any() and b.stages['lower_valid'][0].any()       # c4: empty ``people``
            assert not b.stages['patches'][0].any() and float(b.tensors['style_input'][0, :30].max()) == -1.0
            assert b.stages['patches_lower'][0].any() and b.stages['denorm_lower'][0].any() and not b.stages['denorm_upper'][0].any()
            assert torch.equal(b.tensors['clothes_lower'][2], b.tensors['image'][2])               # (p1, c0, -)
    assert people == [7, 6]                                           # of 12 and 9 roles


# ---- 4. the command line ----

def _generate(G, t, z):
    """test_512.py's call sequence (:134-142)."""
    with torch.no_grad():
        gen_c, cat_feat_list = G.style_encoding(t['style_input'], t['retain'])
        pose_feat = G.const_encoding(t['pose'])
        ws = G.mapping(z, gen_c, truncation_psi=1)
        cat_feats = {str(c.shape[2]): c for c in cat_feat_list}
        _, gen_imgs, _ = G.synthesis(ws, pose_feat, cat_feats, t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                                     t['denorm_lower_mask'], noise_mode='const')
    return gen_imgs


def _oracle_row(gen_u8, sample, stages):
    """One item's [3, 5] row of the numpy restatement: the written content bytes [512, 320, 3] against its three regions."""
    regions = F.pair_regions(sample['image'], sample['parsing'], stages['palm'], stages['denorm_upper'], stages['denorm_lower'])
    return [[v[0] for v in F.region_stats(gen_u8[None], regions[name][1][None], regions[name][0][None])] for name in F.REGIONS]


def _run_cli(*args):
    return subprocess.run([sys.executable, CLI, *args], capture_output=True, text=True, timeout=600, cwd=ROOT)


def test_cli_writes_and_scores_the_outfits(tree, tmp_path, tmp_path_factory):
    import PIL.Image
    import legacy
    from metrics import tryon_fidelity as M
    from training.tryon_pairs import images_to_u8
    from training.tryon_regions import TryOnOutfitBatch, TryOnOutfitBatchBuilder
    listing, samples, stages = _expected(tree, tmp_path_factory)
    pkl, outdir, scores = str(tmp_path / 'snapshot.pkl'), tmp_path / 'out', tmp_path / 'out' / 'scores.json'
    _snapshot(pkl)
    common = ['--network', pkl, '--dataroot', tree, '--batchsize', str(BATCH), '--workers', '0']
    r = _run_cli(*common, '--outdir', str(outdir), '--outfits', listing, '--scores', str(scores))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert sorted(os.listdir(outdir)) == ['%03d.png' % i for i in range(len(MIXED))] + ['scores.json']
    report = json.loads(scores.read_text())
    assert sorted(report) == ['dataroot', 'network', 'noise_mode', 'pairs', 'results']
    assert report['pairs'] == len(MIXED) and report['network'] == pkl and report['dataroot'] == tree and report['noise_mode'] == 'const'
    printed = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(printed) == 1 and json.dumps(printed[0]) == json.dumps(report)       # the same line printed and written

    # the same outfits in the same batches in this process, scored by score_batch
    with open(pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].cuda().eval().requires_grad_(False)
    assert G512_45['patch_channels'] == 45 and G.z_dim == 0
    builder = TryOnOutfitBatchBuilder('cuda')
    partials = M.new_partials(len(MIXED), 'cuda')
    rows, cli_rows = np.zeros([len(MIXED), 3, 5]), np.zeros([len(MIXED), 3, 5])
    worst, differing, total = 0, 0, 0
    for lo, raw in _batches(samples):
        batch = builder.build(raw, keep_stages=True)
        index = list(range(lo, lo + batch.batch))
        assert raw['raw_idx'].tolist() == index
        want = _expected_tensors(stages[lo:lo + batch.batch])
        for k in TryOnOutfitBatch.KEYS:
            assert torch.equal(batch.tensors[k], want[k]), (lo, k)
        gen_imgs = _generate(G, batch.tensors, M.pair_z(index, G.z_dim, 'cuda'))
        M.score_batch(gen_imgs, batch, index, partials)
        content = images_to_u8(gen_imgs, LP, W).cpu().numpy()
        gen_imgs = gen_imgs.cpu().numpy()
        panels = {k: want[k].cpu().numpy() for k in ('clothes', 'clothes_lower', 'image')}
        for j, i in enumerate(index):
            img = PIL.Image.open(outdir / ('%03d.png' % i))
            assert img.mode == 'RGB' and img.size == (4 * H, H)
            got = np.asarray(img)
            inputs = np.concatenate([FR.panel(panels[k][j], False) for k in ('clothes', 'clothes_lower', 'image')], axis=1)
            assert np.array_equal(got[:, :3 * H], inputs), (i, 'input panels')         # upper donor | lower donor | person
            generated = FR.panel(gen_imgs[j], True)
            assert np.array_equal(generated[:, LP:LP + W], content[j])
            diff = np.abs(got[:, 3 * H:].astype(np.int32) - generated.astype(np.int32))
            worst, differing, total = max(worst, int(diff.max())), differing + int((diff > 0).sum()), total + diff.size
            # the restated scores of the bytes this process would write, and of the bytes the command line wrote
            rows[i] = _oracle_row(content[j], samples[i], stages[i])
            written = np.ascontiguousarray(got[:, 3 * H + LP:3 * H + LP + W])
            cli_rows[i] = rows[i] if np.array_equal(written, content[j]) else _oracle_row(written, samples[i], stages[i])
    print('e2e outfits: max |diff| %d LSB, %d of %d values differ' % (worst, differing, total))
    # the same inputs in the same batches through the same kernels: at most 1 LSB anywhere, and in at most 0.1 % of the values
    assert worst <= 1 and differing <= total // 1000, (worst, differing, total)

    # score_batch against the restatement, as tests/test_tryon_fidelity_gpu.py holds the 256 ones: integer words equal, SSIM to its bound
    partials = partials.cpu()
    assert np.array_equal(partials[:, :, :4].numpy(), rows[:, :, :4].astype(np.int64))
    kernel = partials.numpy().astype(np.float64)
    kernel[:, :, 4] = partials[:, :, 4].contiguous().numpy().view(np.float64)
    has = rows[:, :, 2] > 0
    assert has.any(axis=0).all() and (kernel[:, :, 4][~has] == 0.0).all()
    dev = np.abs(kernel[:, :, 4][has] / rows[:, :, 2][has] - rows[:, :, 4][has] / rows[:, :, 2][has])
    print('mean SSIM of the outfits, kernel against oracle: largest deviation %.3e over %d regions with windows' % (dev.max(), has.sum()))
    assert dev.max() <= R.SSIM_TOL
    mine, oracle = M.finish(partials, 'tryon', pixels=H * W), F.finish(rows, H * W)
    written = F.finish(cli_rows, H * W)
    got = report['results']
    print('tryon fidelity of the outfits:', got)
    assert sorted(got) == sorted(mine) == sorted('tryon_' + k for k in oracle) and len(got) == 18
    for k, v in oracle.items():
        tol = dict(rel=1e-12, abs=R.SSIM_TOL if k.endswith('_ssim') else 0)
        assert np.isfinite(v), k
        assert mine['tryon_' + k] == pytest.approx(v, **tol), k
        assert got['tryon_' + k] == pytest.approx(written[k], **tol), k            # the report describes the files next to it
    # who has a region at all, by the restatement: nothing is warped back onto p3 (empty ``people``), c4 (empty ``people``) gives p4 no
    # upper garment
    upper_pairs, lower_pairs = (sum(bool(st[k].any()) for st in stages) for k in ('denorm_upper', 'denorm_lower'))
    assert not stages[3]['denorm_upper'].any() and not stages[3]['denorm_lower'].any() and not stages[4]['denorm_upper'].any()
    assert 0 < upper_pairs < lower_pairs < len(MIXED)
    assert got['tryon_keep_pairs'] == len(MIXED) and got['tryon_upper_pairs'] == upper_pairs and got['tryon_lower_pairs'] == lower_pairs
    assert 0 < got['tryon_upper_share'] < 1 and 0 < got['tryon_lower_share'] < 1 and 0 < got['tryon_keep_share'] < 1

    # a pair list with a region takes --scores as well; the two modes exclude each other
    short = tmp_path / 'pairs'
    r = _run_cli(*common, '--outdir', str(short), '--change-region', 'upperbody', '--scores', str(short / 'scores.json'))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    pairs = json.loads((short / 'scores.json').read_text())
    assert sorted(pairs) == sorted(report) and sorted(pairs['results']) == sorted(got) and pairs['pairs'] == len(PAIRS)
    assert sorted(os.listdir(short)) == ['%03d.png' % i for i in range(len(PAIRS))] + ['scores.json']
    assert pairs['results']['tryon_keep_pairs'] == len(PAIRS) and np.isfinite(pairs['results']['tryon_upper_l1'])
    # the command's function called without --scores, as a plain run, writes the same files for the same pairs (z_dim = 0: the
    # per-pair z is the plain run's z)
    import importlib.util
    spec = importlib.util.spec_from_file_location('pasta_test_512_cli', CLI)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    plain = tmp_path / 'plain'
    module.generate_images.callback(network_pkl=pkl, seeds=None, truncation_psi=1, class_idx=None, noise_mode='const', projected_w=None,
                                    outdir=str(plain), dataroot=tree, batchsize=BATCH, change_region='upperbody', workers=0)
    assert sorted(os.listdir(plain)) == ['%03d.png' % i for i in range(len(PAIRS))]
    for name in os.listdir(plain):
        assert (plain / name).read_bytes() == (short / name).read_bytes(), name
    r = _run_cli(*common, '--outdir', str(tmp_path / 'both'), '--outfits', listing, '--change-region', 'fullbody')
    assert r.returncode != 0 and '--outfits' in r.stderr and '--change-region' in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / 'both').exists()
