"""Row f4 for the 512 x 320 try-on pairs with a change region on the GPU (the region entries of csrc/tryon_pairs.hip, the generalised stick-figure
and palm entries, training/tryon_regions.py, pasta-gan_amd/test_512.py) against the numpy restatement of the reference
(tests/tryon_512_ref.py) -- EXACT: every uint8 stage bit for bit, the nine fp32 tensors equal to test_512.py's own expressions
evaluated by torch on the GPU, and the written images against an in-process run."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import tryon_512_ref as FR
from conftest import ROOT
from oracle import param_fill as PF
from tryon_512_tree import PAIRS, make_512_tree

pytestmark = pytest.mark.gpu

H, W, LP = 512, 320, 96


def _lib():
    from torch_utils.ops import _native
    return _native


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keypoints(rng, n, h=H, w=W):
    kp = np.zeros([n, 18, 3])
    kp[..., 0] = rng.uniform(-50, w + 60, [n, 18])
    kp[..., 1] = rng.uniform(-50, h + 60, [n, 18])
    kp[..., 2] = rng.uniform(0, 1, [n, 18])
    kp[:, 2:8, 2] = 0.9
    kp[0, 4, :2] = kp[0, 3, :2]                                  # zero-length right forearm
    kp[1, 7, :2] = (3000.5, -2000.25)                            # left wrist far outside
    kp[2, 0, :2] = kp[2, 1, :2]                                  # zero-length neck-nose limb
    kp[2, :2, 2] = 0.9
    return kp


def _labels(rng, kp, h=H, w=W):
    n = kp.shape[0]
    lab = rng.integers(0, 20, [n, h // 16, w // 16]).repeat(16, 1).repeat(16, 2).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    for i in range(n):
        for j, label in ((7, 14), (6, 14), (5, 14), (4, 15), (3, 15), (2, 15)):
            lab[i][(yy - kp[i, j, 1]) ** 2 + (xx - kp[i, j, 0]) ** 2 < rng.uniform(20, 60) ** 2] = label
    return lab


def _stick(entry, kp, h, w, *args):
    from training import tryon_batch as TB
    N = _lib()
    limbs, joints = (_cu(a) for a in TB.stick_tables(kp))
    out = torch.empty([kp.shape[0], h, h, 3], dtype=torch.uint8, device='cuda')
    N.check(entry(N.ptr(limbs), N.ptr(joints), N.ptr(out), kp.shape[0], h, w, *args, N.stream()))
    return out.cpu().numpy()


def _palm(entry, parsing, kp, h, w, *boxes):
    from training import tryon_batch as TB
    N = _lib()
    quads, present = TB.palm_quads(kp, (h - w) // 2)
    out = torch.empty([kp.shape[0], h, h], dtype=torch.uint8, device='cuda')
    lab, quads, present = _cu(parsing), _cu(quads), _cu(present)
    N.check(entry(N.ptr(lab), N.ptr(quads), N.ptr(present), N.ptr(out), kp.shape[0], h, w, *boxes, N.stream()))
    return out.cpu().numpy()


def test_thick_stick_figure_equals_the_restatement():
    rng = np.random.default_rng(0)
    kp = _keypoints(rng, 4)
    lib = _lib().lib()
    got = _stick(lib.pasta_pose_stickman_u8, kp, H, W, 5, 5)
    for i in range(len(kp)):
        ref = np.pad(FR.draw_pose_from_cords(kp[i], (H, W)), ((0, 0), (LP, LP), (0, 0)))
        assert np.array_equal(got[i], ref), (i, int((got[i] != ref).any(axis=2).sum()))
    assert got.any() and not got[:, :, :LP].any() and not got[:, :, LP + W:].any()
    thin = _stick(lib.pasta_pose_stickman_u8, kp, H, W, 2, 2)
    assert (got.any(axis=3).sum() > 2 * thin.any(axis=3).sum())  # thickness 5 covers far more than thickness 2


def test_generalised_entries_with_the_old_constants_equal_the_old_entries():
    """The 256 x 192 sets' constants through the one stick-figure and the one palm entry, each against its restatement: the
    thickness-2 figure of tests/tryon_ref.py, and the palm rule on the 256 square with the training set's boxes, the test set's
    and a pair of small ones."""
    import tryon_ref as R
    rng = np.random.default_rng(1)
    kp = _keypoints(rng, 4, 256, 192)
    kp[1, 7, :2] = (300.5, -20.25)
    lib = _lib().lib()
    thin = _stick(lib.pasta_pose_stickman_u8, kp, 256, 192, 2, 2)
    for i in range(len(kp)):
        assert np.array_equal(thin[i], np.pad(R.draw_pose_from_cords(kp[i], (256, 192)), ((0, 0), (32, 32), (0, 0)))), i
    assert thin.any()
    parsing = _labels(rng, kp, 256, 192)
    padded = np.pad(parsing, ((0, 0), (0, 0), (32, 32)))
    shifted = kp.copy()
    shifted[..., 0] += 32
    seen = []
    for boxes in ((25, 15), (25, 16), (7, 4)):
        got = _palm(lib.pasta_palm_mask_u8, parsing, kp, 256, 192, *boxes)
        for i in range(len(kp)):
            assert np.array_equal(got[i], FR.palm_mask(shifted[i], padded[i], boxes)), (boxes, i)
        assert got.any()
        seen.append(got)
    assert (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any()          # the boxes matter
    with pytest.raises(RuntimeError, match='bad shape'):
        _palm(lib.pasta_palm_mask_u8, np.zeros([1, 520, 320], np.uint8), kp[:1], 520, 320, 35, 20)


def test_palm_512_and_region_masks_equal_the_restatement():
    rng = np.random.default_rng(2)
    n = 3
    kp, d_kp = _keypoints(rng, n), _keypoints(rng, n)
    kp[1, 7, :2] = (330.5, -20.25)
    parsing, d_parsing = _labels(rng, kp), _labels(rng, d_kp)
    image, d_image = (rng.integers(0, 256, [n, H, W, 3], dtype=np.uint8) for _ in range(2))
    N = _lib()
    lib = N.lib()
    palm = _palm(lib.pasta_palm_mask_u8, parsing, kp, H, W, 35, 20)
    other = _palm(lib.pasta_palm_mask_u8, parsing, kp, H, W, 25, 15)
    raws = [dict(image=image[i], parsing=parsing[i], keypoints=kp[i], clothes_image=d_image[i], clothes_parsing=d_parsing[i],
                 clothes_keypoints=d_kp[i]) for i in range(n)]
    person = [_cu(a) for a in (image, parsing, palm)]     # held: a freed input's memory would be reused by the next one
    own, donor = person[:2], [_cu(a) for a in (d_image, d_parsing)]
    seen = {}
    for region in FR.REGIONS:
        upper_donor, lower_donor = FR.region_sources(region)
        ins = person + (donor if upper_donor else own) + (donor if lower_donor else own)
        outs = [torch.empty([n, H, H, 3], dtype=torch.uint8, device='cuda') for _ in range(5)]
        N.check(lib.pasta_tryon_outfit_masks_u8(*[N.ptr(t) for t in ins + outs], n, H, W, 0, N.stream()))
        outs = [t.cpu().numpy() for t in outs]
        for i in range(n):
            ref = FR.label_stages(raws[i], region)
            assert np.array_equal(palm[i], ref['palm']), (i, 'palm')
            for k, name in enumerate(('retain_img', 'upper_img', 'upper_mask', 'lower_img', 'lower_mask')):
                assert np.array_equal(outs[k][i], ref[name]), (region, i, name)
        seen[region] = outs
        assert all(o.any() for o in outs)
    assert palm.any() and (palm != other).any()
    assert not np.array_equal(seen['fullbody'][3], seen['upperbody'][3]) and np.array_equal(seen['fullbody'][1], seen['upperbody'][1])
    assert not np.array_equal(seen['fullbody'][1], seen['lowerbody'][1]) and np.array_equal(seen['fullbody'][3], seen['lowerbody'][3])
    with pytest.raises(RuntimeError, match='six_is_lower 3'):
        outs = [torch.empty([n, H, H, 3], dtype=torch.uint8, device='cuda') for _ in range(5)]
        N.check(lib.pasta_tryon_outfit_masks_u8(*[N.ptr(t) for t in ins + outs], n, H, W, 3, N.stream()))


def test_region_assemble_equals_test_512_expressions():
    """On random uint8 stages (a 0 / 1 retain mask times the image, patches, composites with all-zero pixels and with pixels
    whose channels sum past 255): the nine tensors equal test_512.py's torch expressions bit for bit.  At 512 x 320, and at
    20 x 12 with 3 and 2 parts of 5 x 5, where the 400 pixels and the style_input tail meet inside one block of 256."""
    import ctypes
    from training.tryon_regions import TryOnRegionBatch
    rng = np.random.default_rng(3)
    for h, w, pu, pl, ph, pw in ((H, W, 10, 5, 128, 128), (20, 12, 3, 2, 5, 5)):
        n, lp = 2, (h - w) // 2
        u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
        image, clothes, stick = u8(n, h, w, 3), u8(n, h, w, 3), u8(n, h, h, 3)
        pad = lambda a: np.pad(a, ((0, 0), (0, 0), (lp, lp), (0, 0)), constant_values=255)
        retain_mask = (rng.uniform(size=[n, h, h, 1]) < 0.5).astype(np.uint8)
        patches, patches_l = u8(n, pu, ph, pw, 3), u8(n, pl, ph, pw, 3)
        den_u, den_l = (u8(n, h, h, 3) * (rng.uniform(size=[n, h, h, 1]) < 0.6).astype(np.uint8) for _ in range(2))
        den_u[0, :8, :8] = (128, 64, 64)                          # sums to 256: a wrapping uint8 sum would call it empty
        stages = [dict(image=pad(image)[i], clothes=pad(clothes)[i], stick=stick[i], retain_mask=retain_mask[i],
                       patches=patches[i].transpose(1, 2, 0, 3).reshape(ph, pw, 3 * pu),
                       patches_lower=patches_l[i].transpose(1, 2, 0, 3).reshape(ph, pw, 3 * pl), denorm_upper=den_u[i], denorm_lower=den_l[i])
                  for i in range(n)]
        want = FR.generator_inputs([FR.getitem(s) for s in stages], 'cuda')
        N = _lib()
        t = {k: torch.empty_like(want[k]) for k in TryOnRegionBatch.KEYS}
        outs = (ctypes.c_void_p * 10)(*[t[k].data_ptr() for k in TryOnRegionBatch.KEYS], None)       # no clothes_lower, no third photograph
        ins = [_cu(a) for a in (image, clothes)] + [None] + [_cu(a) for a in (retain_mask * pad(image), stick, patches, patches_l, den_u, den_l)]
        N.check(N.lib().pasta_tryon_outfit_assemble(*[N.ptr(a) for a in ins], outs, n, h, w, pu, pl, ph, pw, N.stream()))
        for k in TryOnRegionBatch.KEYS:
            assert torch.equal(t[k], want[k]), (h, k)
        assert tuple(t['style_input'].shape) == (n, 3 * (pu + pl), ph, pw) and tuple(t['pose'].shape) == (n, 6, h, h)
        assert t['denorm_upper_mask'][0, 0, :8, :8].all() and 0 < float(t['denorm_upper_mask'].mean()) < 1
        assert float(t['retain'].min()) == -1.0 and float(t['image'][..., :lp].min()) > 0.99      # zeros outside the mask, white padding


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_512_tree(tmp_path_factory.mktemp('pairs512_gpu'))


_RESTATED = {}


def _restated(tree, region):
    """(raw pairs, restated stages) of the whole tree for one region, computed once."""
    from training.dataset import UvitonDatasetFull_512_test
    if (tree, region) not in _RESTATED:
        ds = UvitonDatasetFull_512_test(path=tree, change_region=region)
        samples = [ds[i] for i in range(len(ds))]
        _RESTATED[tree, region] = samples, [FR.load_pair(r, region) for r in samples]
    return _RESTATED[tree, region]


def test_builder_equals_the_restatement_on_the_tree(tree):
    from training.dataset import collate_pairs
    from training.tryon_regions import TryOnRegionBatch, TryOnRegionBatchBuilder
    hwc = lambda t: t.permute(0, 2, 3, 1, 4).reshape(t.shape[0], t.shape[2], t.shape[3], -1)
    style = {}
    for region in FR.REGIONS:
        samples, stages = _restated(tree, region)
        raw = collate_pairs(samples)
        b = TryOnRegionBatchBuilder('cuda', region).build(raw, keep_stages=True)
        assert b.batch == len(PAIRS) and b.person_name == raw['person_name'] and b.clothes_name == raw['clothes_name']
        want = FR.generator_inputs([FR.getitem(s) for s in stages], 'cuda')
        assert list(b.tensors) == TryOnRegionBatch.KEYS
        for k in TryOnRegionBatch.KEYS:
            assert b.tensors[k].shape == want[k].shape and torch.equal(b.tensors[k], want[k]), (region, k)
        for i, ref in enumerate(stages):
            for name in ('stick', 'palm', 'retain_img', 'upper_img', 'upper_mask', 'lower_img', 'lower_mask', 'denorm_upper', 'denorm_lower'):
                assert np.array_equal(b.stages[name][i].cpu().numpy(), ref[name]), (region, i, name)
            for name in ('patches', 'patches_lower', 'mask_patches', 'mask_patches_lower'):
                assert np.array_equal(hwc(b.stages[name])[i].cpu().numpy(), ref[name]), (region, i, name)
        # nothing passes vacuously
        assert b.stages['palm'].any() and b.stages['denorm_upper'].any() and b.stages['denorm_lower'].any()
        assert 0 < float(b.tensors['denorm_upper_mask'].mean()) < 1 and 0 < float(b.tensors['denorm_lower_mask'].mean()) < 1
        cv, pv = b.stages['clothes_valid'], b.stages['person_valid']
        assert not cv[0, [0, 1, 2, 4, 6, 8]].any() and pv[0].all()   # pair 0: the donor has no shoulders or hips, the person has all
        assert not pv[1, 9] and pv[1, 8]                             # pair 1: the shin without its ankle is invalid here
        assert pv[2, 6] and not pv[2, 7]                             # pair 2: the thigh without its knee falls back, its shin is missing
        assert not pv[3].any() and not cv[4].any()                   # empty ``people``: the person of pair 3, the donor of pair 4
        assert not b.stages['denorm_upper'][3].any() and not b.stages['denorm_lower'][3].any()
        style[region] = b.tensors['style_input']
    assert tuple(style['fullbody'].shape) == (len(PAIRS), 45, 128, 128)
    for a, c in (('fullbody', 'upperbody'), ('fullbody', 'lowerbody'), ('upperbody', 'lowerbody')):
        assert not torch.equal(style[a], style[c]), (a, c)
    assert torch.equal(style['fullbody'][:, :30], style['upperbody'][:, :30]) and torch.equal(style['fullbody'][:, 30:], style['lowerbody'][:, 30:])


G512_45 = dict(z_dim=0, c_dim=512, w_dim=512, img_resolution=512, img_channels=3, patch_channels=45, mapping_kwargs=dict(num_layers=1),
               synthesis_kwargs=dict(channel_base=2048, channel_max=512, conv_clamp=256))


def _snapshot(path):
    from training import networks
    G = PF.fill_module(networks.GeneratorFull(**G512_45)).eval().requires_grad_(False)
    D = networks.Discriminator(c_dim=512, img_resolution=256, img_channels=3, channel_base=512, channel_max=32)
    with open(path, 'wb') as f:
        pickle.dump(dict(G=G, D=D, G_ema=G), f)


@pytest.mark.parametrize('region', [None, 'lowerbody'])
def test_cli_writes_the_images_of_an_in_process_run(tree, tmp_path, region):
    """``region`` None: no --change-region, which must mean full body."""
    import PIL.Image
    import legacy
    from training.dataset import collate_pairs
    pkl, outdir = str(tmp_path / 'snapshot.pkl'), tmp_path / 'out'
    _snapshot(pkl)
    cmd = [sys.executable, os.path.join(ROOT, 'pasta-gan_amd', 'test_512.py'), '--network', pkl, '--outdir', str(outdir), '--dataroot', tree,
           '--batchsize', '2', '--noise-mode', 'const', '--workers', '0'] + (['--change-region', region] if region else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert sorted(os.listdir(outdir)) == ['%03d.png' % i for i in range(len(PAIRS))]

    with open(pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].cuda()
    assert G.style_encoding.model[0].weight.shape[1] == 45
    samples, stages = _restated(tree, region or 'fullbody')
    worst, differing, total = 0, 0, 0
    for s in range(0, len(samples), 2):
        t = FR.generator_inputs([FR.getitem(st) for st in stages[s:s + 2]], 'cuda')
        n = t['image'].shape[0]
        with torch.no_grad():                                    # test_512.py:134-142
            gen_c, cat_feat_list = G.style_encoding(t['style_input'], t['retain'])
            pose_feat = G.const_encoding(t['pose'])
            ws = G.mapping(torch.randn([n, 0], device='cuda'), gen_c)
            cat_feats = {str(c.shape[2]): c for c in cat_feat_list}
            _, gen_imgs, _ = G.synthesis(ws, pose_feat, cat_feats, t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                                         t['denorm_lower_mask'], noise_mode='const')
        gen_imgs, image, clothes = gen_imgs.cpu().numpy(), t['image'].cpu().numpy(), t['clothes'].cpu().numpy()
        for i in range(n):
            want = FR.result_image(clothes[i], image[i], gen_imgs[i])
            img = PIL.Image.open(os.path.join(outdir, '%03d.png' % (s + i)))
            assert img.mode == 'RGB' and img.size == (3 * H, H)
            got = np.asarray(img)
            assert np.array_equal(got[:, :2 * H], want[:, :2 * H]), (s + i, 'input panels')
            diff = np.abs(got[:, 2 * H:].astype(np.int32) - want[:, 2 * H:].astype(np.int32))
            worst, differing, total = max(worst, int(diff.max())), differing + int((diff > 0).sum()), total + diff.size
    print('e2e %s: max |diff| %d LSB, %d of %d values differ' % (region or 'fullbody', worst, differing, total))
    # the same inputs in the same batches through the same kernels: at most 1 LSB anywhere, and in at most 0.1 % of the values
    assert worst <= 1 and differing <= total // 1000, (worst, differing, total)
