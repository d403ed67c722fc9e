"""Training at 512 x 320 on the GPU (the two training entries of csrc/tryon_pairs.hip, training/tryon_regions.py's
FullBodyRegionBatchBuilder, the snapshot grid and the commands) -- EXACT: the entries and the builder against the numpy
restatement (tests/tryon_512_train_ref.py) bit for bit; the builder against TryOnRegionBatchBuilder('fullbody') on the pair
(person, person), which is the rule the feature rests on; every cell of the 3 x 3 grid against TryOnRegionBatchBuilder on the
pair (row, col); and one run of the training command whose snapshot test_512.py loads and calc_metrics.py scores."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import recon_ref as RR
import tryon_512_train_ref as TR
from conftest import ROOT
from tryon_512_train_tree import PERSONS, make_512_train_tree
from tryon_512_tree import PAIRS, make_512_tree

pytestmark = pytest.mark.gpu

H, W = 512, 320
STAGES = ('stick', 'palm', 'retain_mask', 'gt_parsing', 'upper_img', 'lower_img', 'upper_mask', 'lower_mask', 'norm_img', 'norm_img_lower',
          'norm_clothes_mask', 'norm_clothes_mask_lower', 'denorm_upper', 'denorm_lower', 'arm_masks', 'M_invs')


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_512_train_tree(tmp_path_factory.mktemp('train512_gpu'))


@pytest.fixture(scope='module')
def cases(tree):
    return TR.cases(tree)


@pytest.fixture(scope='module')
def built(cases):
    from training.dataset import collate
    from training.tryon_regions import FullBodyRegionBatchBuilder
    samples, _, _ = cases
    return FullBodyRegionBatchBuilder('cuda').build(collate(samples), keep_stages=True)


def _assemble(stages, erase_masks, h, w, arm_a, arm_b):
    """pasta_tryon_train_region_assemble on restated uint8 stages, the restatement's arm masks 2 and 3 as planes arm_a and
    arm_b of the part masks: the nine tensors."""
    from torch_utils.ops import _native as N
    from training.dataset import collate
    from training.tryon_batch import FullBodyBatch
    n, lp = len(stages), (h - w) // 2
    ph, pw = stages[0]['norm_img'].shape[:2]
    per_part = lambda key: np.stack([st[key].reshape(ph, pw, -1, 3).transpose(2, 0, 1, 3) for st in stages])
    patches, patches_l = per_part('norm_img'), per_part('norm_img_lower')
    pu, pl = patches.shape[1], patches_l.shape[1]
    part_masks = np.full([n, pu, h, h], 1, np.uint8)   # the other planes must not matter
    part_masks[:, arm_a], part_masks[:, arm_b] = (np.stack([st['arm_masks'][k] for st in stages]) for k in (2, 3))
    raw = collate([dict(image=st['image'][:, lp:lp + w], parsing=st['gt_parsing'][:, lp:lp + w], keypoints=np.zeros([18, 3]), erase_mask=m,
                        raw_idx=i) for i, (st, m) in enumerate(zip(stages, erase_masks))])
    stack = lambda key: np.stack([st[key] for st in stages])
    ins = [_cu(a) for a in (raw['image'].numpy(), stack('stick'), stack('retain_mask'), stack('gt_parsing'), patches, patches_l,
                            stack('denorm_upper'), stack('denorm_lower'), part_masks)]
    erase, erase_hw = raw['erase_masks'].cuda(), raw['erase_hw'].cuda()
    planes = dict(pose=6, denorm_upper_mask=1, denorm_lower_mask=1, gt_parsing=1)
    t = {k: torch.empty([n, 3 * (pu + pl), ph, pw] if k == 'style_input' else [n, planes.get(k, 3), h, h], device='cuda')
         for k in FullBodyBatch.KEYS}
    outs = (ctypes.c_void_p * 9)(*[t[k].data_ptr() for k in FullBodyBatch.KEYS])
    N.check(N.lib().pasta_tryon_train_region_assemble(*[N.ptr(a) for a in ins], arm_a, arm_b, N.ptr(erase), N.ptr(erase_hw), outs, n, h, w,
                                                      pu, pl, ph, pw, int(erase.shape[1]), int(erase.shape[2]), N.stream()))
    return t


def test_masks_entry_equals_the_restatement(cases):
    from torch_utils.ops import _native as N
    samples, stages, _ = cases
    n = len(samples)
    ins = [_cu(np.stack(a)) for a in ([s['image'] for s in samples], [s['parsing'] for s in samples], [st['palm'] for st in stages])]
    u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device='cuda')
    retain, gt, img, mask = u8(n, H, H), u8(n, H, H), u8(2 * n, H, H, 3), u8(2 * n, H, H, 3)
    # the 256 training set's entry in its own order (both images, then both masks), on the halves of the stacked tensors
    N.check(N.lib().pasta_tryon_masks_u8(*[N.ptr(a) for a in ins], N.ptr(retain), N.ptr(gt), N.ptr(img[:n]), N.ptr(img[n:]),
                                         N.ptr(mask[:n]), N.ptr(mask[n:]), n, H, W, N.stream()))
    got = dict(retain_mask=retain, gt_parsing=gt, upper_img=img[:n], upper_mask=mask[:n], lower_img=img[n:], lower_mask=mask[n:])
    for k, v in got.items():
        v = v.cpu().numpy()
        for i in range(n):
            assert np.array_equal(v[i], stages[i][k]), (k, i)
        assert v.any()
    assert int(retain.max()) == 1                       # a 0 / 1 mask, not an image


def test_assemble_entry_equals_the_restatement(cases):
    """On the restated stages of the three people (erase masks of 512 x 512 with the wrap pixel, 256 x 192 and 37 x 23), and on
    random stages at 20 x 12 with 3 and 2 parts of 5 x 4, where the 400 pixels and the five style_input threads meet inside one
    block of 256 and the erase mask (7 x 5) is stretched along both axes."""
    samples, stages, wrap = cases
    masks = [s['erase_mask'] for s in samples]
    got, want = _assemble(stages, masks, H, W, 4, 5), TR.training_tensors(stages, masks, 'cuda')
    for k, v in want.items():
        assert got[k].shape == v.shape and torch.equal(got[k], v), (k, int((got[k] != v).sum()))
    assert float(got['denorm_upper_input'][0, :, wrap[0], wrap[1]].max()) > -1        # the wrap pixel is kept

    rng = np.random.default_rng(4)
    h, w, pu, pl, ph, pw, lp = 20, 12, 3, 2, 5, 4, 4
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    bit = lambda *shape: (rng.uniform(size=shape) < 0.5).astype(np.uint8)
    small = [dict(image=np.pad(u8(h, w, 3), ((0, 0), (lp, lp), (0, 0)), constant_values=255), stick=u8(h, h, 3), retain_mask=bit(h, h),
                  gt_parsing=rng.integers(0, 6, [h, h]).astype(np.uint8), norm_img=u8(ph, pw, 3 * pu), norm_img_lower=u8(ph, pw, 3 * pl),
                  denorm_upper=u8(h, h, 3) * bit(h, h, 1), denorm_lower=u8(h, h, 3) * bit(h, h, 1), arm_masks=bit(4, h, h))
             for _ in range(2)]
    small_masks = [(rng.uniform(size=[7, 5]) < 0.3).astype(np.uint8) * np.uint8(255), u8(3, 9)]
    got, want = _assemble(small, small_masks, h, w, 1, 2), TR.training_tensors(small, small_masks, 'cuda')
    for k, v in want.items():
        assert got[k].shape == v.shape and torch.equal(got[k], v), ('small', k, int((got[k] != v).sum()))
    assert 0 < float(want['denorm_upper_mask'].mean()) < 1


def test_builder_equals_the_restatement(cases, built):
    from training.tryon_batch import FullBodyBatch
    samples, stages, wrap = cases
    want = TR.training_tensors(stages, [s['erase_mask'] for s in samples], 'cuda')
    assert list(built.tensors) == FullBodyBatch.KEYS and built.batch == 3 and len(built.split(2)) == 2
    for k in FullBodyBatch.KEYS:
        g, v = built.tensors[k], want[k]
        assert g.dtype == torch.float32 and g.shape == v.shape and torch.equal(g, v), (k, int((g != v).sum()))
    assert tuple(built.tensors['style_input'].shape) == (3, 45, 128, 128)
    assert sorted(built.stages) == sorted(STAGES)
    for i, st in enumerate(stages):
        for k in STAGES:
            assert np.array_equal(built.stages[k][i].cpu().numpy(), st[k]), (i, k)
    assert torch.equal(built.image.cpu(), torch.from_numpy(np.stack([s['image'] for s in samples])))
    assert tuple(built.stages['norm_img'].shape) == (3, 128, 128, 30) and tuple(built.stages['norm_img_lower'].shape) == (3, 128, 128, 15)


def test_a_sample_is_the_test_sets_preparation_of_the_pair_person_person(cases, built):
    """The rule of the feature, bit for bit: retain, pose and style_input are what test_512.py would feed the generator for the
    pair (person, person); real_img is its image; the denormalised inputs and masks are its own outside the erase mask and -1
    and 0 inside."""
    from training.dataset import collate_pairs
    from training.tryon_regions import TryOnRegionBatchBuilder
    samples, stages, _ = cases
    pairs = []
    for i, s in enumerate(samples):
        pairs.append(dict(image=s['image'], parsing=s['parsing'], keypoints=s['keypoints'], clothes_image=s['image'],
                          clothes_parsing=s['parsing'], clothes_keypoints=s['keypoints'], person_name='p%d' % i, clothes_name='p%d' % i,
                          raw_idx=i))
    pair = TryOnRegionBatchBuilder('cuda', 'fullbody').build(collate_pairs(pairs)).tensors
    t = built.tensors
    for k in ('retain', 'pose', 'style_input'):
        assert torch.equal(t[k], pair[k]), k
    assert torch.equal(t['real_img'], pair['image'])
    erase = _cu(np.stack([TR.erased(st, s['erase_mask'])[0] for st, s in zip(stages, samples)]))[:, None].bool()
    assert 0.01 < float(erase.float().mean()) < 0.5
    for k, gone in (('denorm_upper_input', -1.0), ('denorm_lower_input', -1.0), ('denorm_upper_mask', 0.0), ('denorm_lower_mask', 0.0)):
        e = erase.expand_as(t[k])
        assert torch.equal(t[k][~e], pair[k][~e]), k
        assert bool((t[k][e] == gone).all()), k
        assert not torch.equal(t[k], pair[k]), k        # the erase mask removed something that was there


def test_grid_cells_equal_the_test_sets_pairs(tree):
    """gnum = 3, gap = 1: row 0 swaps the lower garment, row 1 the whole outfit, row 2 the upper garment.  The seven tensors of
    every cell equal TryOnRegionBatchBuilder on the pair (person = row, donor = col) of that region."""
    from training.dataset import UvitonDatasetFull_512, collate_pairs
    from training.snapshot_grid import INPUT_KEYS, SnapshotGrid
    from training.tryon_batch import builder_for
    from training.tryon_regions import TryOnRegionBatchBuilder
    ds = UvitonDatasetFull_512(tree)
    grid = SnapshotGrid.setup(ds, builder_for(ds, 'cuda'), 'cuda', gnum=3)
    assert grid.cells == 9 and grid.H == 512
    people = [ds[i] for i in ds.vis_index[:3]]
    got = grid.inputs(0, 9)
    got['style_input'] = got.pop('c')
    seen = set()
    for row, region in enumerate(('lowerbody', 'fullbody', 'upperbody')):
        pairs = [dict(image=people[row]['image'], parsing=people[row]['parsing'], keypoints=people[row]['keypoints'],
                      clothes_image=people[col]['image'], clothes_parsing=people[col]['parsing'], clothes_keypoints=people[col]['keypoints'],
                      person_name='r%d' % row, clothes_name='c%d' % col, raw_idx=row * 3 + col) for col in range(3)]
        want = TryOnRegionBatchBuilder('cuda', region).build(collate_pairs(pairs)).tensors
        for k in INPUT_KEYS:
            for col in range(3):
                assert torch.equal(got[k][row * 3 + col], want[k][col]), (row, col, k, int((got[k][row * 3 + col] != want[k][col]).sum()))
        seen.add(tuple(want['style_input'].shape[1:]))
        assert not torch.equal(want['denorm_upper_input'][0], want['denorm_upper_input'][1]) or region == 'lowerbody'
        assert not torch.equal(want['denorm_lower_input'][0], want['denorm_lower_input'][1]) or region == 'upperbody'
    assert seen == {(45, 128, 128)} and float(got['denorm_upper_mask'].mean()) > 0 and float(got['denorm_lower_mask'].mean()) > 0


# ---- end to end: train at 512, load the snapshot in test_512.py, score it ----

BATCH = 4
# train_wo_flow_fullbody.py's own main() in a fresh process, with the run shrunk as tests/test_train_run_gpu.py shrinks it: test-size
# widths (channel_base 2048), one tick of one iteration, a 3 x 3 sample grid.  The command line has no options for these.
_TRAIN_SCRIPT = '''
import sys
import train_wo_flow_fullbody as T

real_loop = T.training_loop.training_loop

def small_loop(**kwargs):
    cfg = kwargs['cfg']
    cfg.G_kwargs.synthesis_kwargs.channel_base = cfg.D_kwargs.channel_base = 2048
    kwargs.update(total_kimg=%d / 1000, kimg_per_tick=%d / 1000, snapshot_gnum=3)
    return real_loop(**kwargs)

T.training_loop.training_loop = small_loop
T.main(sys.argv[1:], standalone_mode=False)
''' % (BATCH, BATCH)


def _process(cmd, seconds, **kwargs):
    r = subprocess.run(['timeout', '-k', '10', str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT, **kwargs)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def test_train_then_try_on_then_score(tree, tmp_path):
    import PIL.Image
    import legacy
    from training.dataset import UvitonDatasetFull_512, collate
    from training.tryon_batch import builder_for
    from training.tryon_pairs import images_to_u8
    code = os.path.join(ROOT, 'pasta-gan_amd')
    script = tmp_path / 'train_small.py'
    script.write_text(_TRAIN_SCRIPT)
    out = _process([sys.executable, str(script), '--outdir', str(tmp_path / 'runs'), '--data', tree, '--gpus', '1', '--cfg', 'fashion',
                    '--batch', str(BATCH), '--snap', '1', '--aug', 'noaug', '--fp32', 'true', '--l1_weight', '40', '--mask_weight', '20'], 600,
                   env=dict(os.environ, PYTHONPATH=code))
    assert 'UvitonDatasetFull_512' in out and '"patch_channels": 45' in out
    (run_dir,) = [tmp_path / 'runs' / d for d in os.listdir(tmp_path / 'runs')]
    names = os.listdir(run_dir)
    pkl = str(run_dir / 'network-snapshot-000000.pkl')
    assert 'network-snapshot-000000.pkl' in names and 'training_options.json' in names
    for name in ('fakes000000_finetune.png', 'init_denorm_upper.png', 'init_denorm_lower.png', 'init_retain.png'):
        assert PIL.Image.open(run_dir / name).size == (4 * 512, 4 * 512), name
    with open(pkl, 'rb') as f:
        data = legacy.load_network_pkl(f)
    assert data['training_set_kwargs']['class_name'] == 'training.dataset.UvitonDatasetFull_512'
    G = data['G_ema'].eval().requires_grad_(False).cuda()
    assert G.style_encoding.model[0].weight.shape[1] == 45

    # test_512.py loads the snapshot and writes clothes | person | generated for every pair of a 512 x 320 pair tree
    pair_tree = make_512_tree(tmp_path / 'pairs512')
    _process([sys.executable, os.path.join(code, 'test_512.py'), '--network', pkl, '--outdir', str(tmp_path / 'tryon'), '--dataroot', pair_tree,
              '--batchsize', '2', '--noise-mode', 'const', '--workers', '0', '--change-region', 'upperbody'], 600)
    assert sorted(os.listdir(tmp_path / 'tryon')) == ['%03d.png' % i for i in range(len(PAIRS))]
    for i in range(len(PAIRS)):
        img = PIL.Image.open(tmp_path / 'tryon' / ('%03d.png' % i))
        assert img.mode == 'RGB' and img.size == (3 * 512, 512)
        assert len(np.unique(np.asarray(img)[:, 2 * 512:])) > 1

    # calc_metrics.py scores it on the 512 tree through builder_for: the figures of tests/recon_ref.py on the builder's outputs
    out = _process([sys.executable, os.path.join(code, 'calc_metrics.py'), '--network', pkl, '--metrics', 'recon_full', '--data', tree,
                    '--verbose', 'false'], 600)
    (line,) = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{')]
    assert line['metric'] == 'recon_full'
    ds = UvitonDatasetFull_512(tree)
    raw = collate([ds[i] for i in range(len(ds))])      # one batch, as the command's default batch size makes it
    t = builder_for(ds, 'cuda').build(raw).tensors
    z = torch.from_numpy(RR.item_z(raw['raw_idx'].tolist(), G.z_dim)).cuda()
    with torch.no_grad():
        _, img, parsing = G(z=z, c=t['style_input'], retain=t['retain'], pose=t['pose'], denorm_upper_input=t['denorm_upper_input'],
                            denorm_lower_input=t['denorm_lower_input'], denorm_upper_mask=t['denorm_upper_mask'],
                            denorm_lower_mask=t['denorm_lower_mask'], noise_mode='const')
    photos = raw['image'].numpy()
    gen = images_to_u8(img.to(torch.float32), (H - W) // 2, W).cpu().numpy()
    sad, ssd, ssim, windows = RR.image_stats(gen, photos)
    conf = RR.confusion(parsing.float().cpu().numpy(), t['gt_parsing'].cpu().numpy(), (H - W) // 2, W)
    want = RR.results(sad, ssd, ssim, windows, np.full(len(PERSONS), H * W * 3), conf)
    got = {k: line['results']['recon_full_' + k] for k in want}
    print('recon_full on the tiny 512 tree:', got, 'oracle:', want)
    for k in ('l1', 'psnr', 'miou', 'pixacc'):
        assert got[k] == pytest.approx(want[k], rel=1e-12), k
    assert abs(got['ssim'] - want['ssim']) <= RR.SSIM_TOL
