"""Row f4 for the try-on TEST pairs on the GPU (csrc/tryon_pairs.hip, training/tryon_pairs.py, pasta-gan_amd/test.py) against
the numpy restatement of the reference (tests/tryon_pairs_ref.py) -- EXACT: every uint8 stage bit for bit, the seven fp32
tensors equal to test.py's own expressions evaluated by torch on the GPU, and the written images against an in-process run."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch

import tryon_pairs_ref as PR
from conftest import ROOT
from oracle import param_fill as PF
from oracle import ref_patches as RP
from tryon_pairs_tree import PAIRS, make_pair_tree

pytestmark = pytest.mark.gpu


def _lib():
    from torch_utils.ops import _native
    return _native


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keypoints(rng, n):
    kp = np.zeros([n, 18, 3])
    kp[..., 0] = rng.uniform(-30, 230, [n, 18])
    kp[..., 1] = rng.uniform(-30, 290, [n, 18])
    kp[..., 2] = rng.uniform(0, 1, [n, 18])
    kp[:, 2:8, 2] = 0.9
    kp[0, 4, :2] = kp[0, 3, :2]                                  # zero-length right forearm
    kp[1, 7, :2] = (300.5, -20.25)                               # left wrist far outside
    return kp


def _labels(rng, kp):
    n = kp.shape[0]
    lab = rng.integers(0, 20, [n, 32, 24]).repeat(8, 1).repeat(8, 2).astype(np.uint8)
    yy, xx = np.mgrid[0:256, 0:192]
    for i in range(n):
        for j, label in ((7, 14), (6, 14), (5, 14), (4, 15), (3, 15), (2, 15)):
            lab[i][(yy - kp[i, j, 1]) ** 2 + (xx - kp[i, j, 0]) ** 2 < rng.uniform(10, 30) ** 2] = label
    return lab


def _palm(entry, parsing, kp, *boxes):
    from training import tryon_batch as TB
    N = _lib()
    quads, present = TB.palm_quads(kp, 32)
    out = torch.empty([kp.shape[0], 256, 256], dtype=torch.uint8, device='cuda')
    lab, quads, present = _cu(parsing), _cu(quads), _cu(present)
    N.check(entry(N.ptr(lab), N.ptr(quads), N.ptr(present), N.ptr(out), kp.shape[0], 256, 192, *boxes, N.stream()))
    return out.cpu().numpy()


def test_palm_box_and_pair_masks_equal_the_restatement():
    rng = np.random.default_rng(0)
    n = 5
    kp, d_kp = _keypoints(rng, n), _keypoints(rng, n)
    parsing, d_parsing = _labels(rng, kp), _labels(rng, d_kp)
    parsing[:, 200:230, 40:150] = 6
    image, d_image = (rng.integers(0, 256, [n, 256, 192, 3], dtype=np.uint8) for _ in range(2))
    lib = _lib().lib()
    palm15, palm16 = _palm(lib.pasta_palm_mask_u8, parsing, kp, 25, 15), _palm(lib.pasta_palm_mask_u8, parsing, kp, 25, 16)
    N = _lib()
    u8 = lambda: torch.empty([n, 256, 256, 3], dtype=torch.uint8, device='cuda')
    outs = [u8() for _ in range(5)]                               # retain, upper img, upper mask, lower img, lower mask
    # the pair: the upper garment's source is the donor, the lower garment's the person, label 6 in the lower garment
    ins = [_cu(a) for a in (image, parsing, palm15, d_image, d_parsing)]  # held: a freed input's memory would be reused by the next one
    N.check(lib.pasta_tryon_outfit_masks_u8(*[N.ptr(t) for t in ins + ins[:2] + outs], n, 256, 192, 1, N.stream()))
    outs = [t.cpu().numpy() for t in outs]
    differs = 0
    for i in range(n):
        raw = dict(image=image[i], parsing=parsing[i], keypoints=kp[i], clothes_image=d_image[i], clothes_parsing=d_parsing[i], clothes_keypoints=d_kp[i])
        ref = PR.load_pair(raw)
        _, _, pad_parsing, shifted = PR.person_stages(image[i], parsing[i], kp[i])
        ref16 = PR.palm_mask(shifted, pad_parsing[..., 0], 16)
        differs += int((ref16 != ref['palm']).sum())
        assert np.array_equal(palm15[i], ref['palm']) and np.array_equal(palm16[i], ref16), (i, 'palm')
        for k, name in enumerate(('retain_img', 'upper_img', 'upper_mask', 'lower_img', 'lower_mask')):
            assert np.array_equal(outs[k][i], ref[name]), (i, name)
    assert palm15.any() and differs > 0 and (outs[3] > 0).any()


def _composite_case(rng, n, parts):
    """Random patches and masks (255 blocks with holes and near-misses of 254) and random perspective maps of body-part quadrilaterals."""
    from training import patch_pipeline as PP
    ph, pw = 64, 64
    patches = rng.integers(0, 256, [n, parts, ph, pw, 3], dtype=np.uint8)
    blocks = rng.uniform(size=[n, parts, ph // 4, pw // 4]) < 0.7
    mask = np.where(blocks.repeat(4, 2).repeat(4, 3), 255, 0).astype(np.uint8)
    mask[rng.uniform(size=mask.shape) < 0.02] = 254
    masks = np.repeat(mask[..., None], 3, axis=-1)
    masks[..., 1] = rng.integers(0, 256, masks.shape[:-1])       # only channel 0 decides
    kp = _keypoints(rng, n)
    kp[..., 0] = rng.uniform(20, 170, [n, 18])
    kp[..., 1] = rng.uniform(10, 245, [n, 18])
    _, back, valid = PP.part_matrices(kp, 256, 256)
    back, valid = back[:, :parts], valid[:, :parts].copy()
    valid[0, 1] = False
    return patches, masks, back, valid


@pytest.mark.parametrize('radius', [0, 1, 2, 3])
def test_eroded_composite_equals_the_restatement(radius):
    from training import patch_pipeline as PP
    rng = np.random.default_rng(10 + radius)
    n, parts = 3, 6
    patches, masks, back, valid = _composite_case(rng, n, parts)
    N = _lib()
    lib = N.lib()
    inv = _cu(np.stack([PP.adjugate_inverse(back[i, k]) for i in range(n) for k in range(parts)]).reshape(n * parts, 9))
    val = _cu(valid.astype(np.uint8))
    patches_t, masks_t = _cu(patches), _cu(masks)
    out = torch.empty([n, 256, 256, 3], dtype=torch.uint8, device='cuda')
    pm = torch.empty([n, parts, 256, 256], dtype=torch.uint8, device='cuda')
    N.check(lib.pasta_patch_composite_eroded_u8(N.ptr(patches_t), N.ptr(masks_t), N.ptr(inv), N.ptr(val), N.ptr(out), N.ptr(pm), n, parts,
                                                64, 64, 256, 256, radius, None, N.stream()))
    out, pm = out.cpu().numpy(), pm.cpu().numpy()
    hits = 0
    for i in range(n):
        den = np.zeros([256, 256, 3], np.uint8)
        for k in range(parts):
            if not valid[i, k]:
                assert not pm[i, k].any()
                continue
            back_img = RP.warp_perspective(patches[i, k], back[i, k], (256, 256), RP.BORDER_CONSTANT)
            back_mask = RP.warp_perspective(masks[i, k], back[i, k], (256, 256), RP.BORDER_CONSTANT)
            if radius:
                back_mask = PR.erode(back_mask, 2 * radius + 1)
            hit = (back_mask[..., 0:1] == 255).astype(np.uint8)
            den = back_img * hit + den * (1 - hit)
            assert np.array_equal(pm[i, k], hit[..., 0]), (i, k)
            hits += int(hit.sum())
        assert np.array_equal(out[i], den), (i, int((out[i] != den).sum()))
    assert hits > 0
    if radius == 0:                                              # the plain composite, bit for bit, part masks included
        out0 = torch.empty([n, 256, 256, 3], dtype=torch.uint8, device='cuda')
        pm0 = torch.empty([n, parts, 256, 256], dtype=torch.uint8, device='cuda')
        N.check(lib.pasta_patch_composite_u8(N.ptr(patches_t), N.ptr(masks_t), N.ptr(inv), N.ptr(val), N.ptr(out0), N.ptr(pm0), n, parts, 64, 64,
                                             256, 256, N.stream()))
        assert np.array_equal(out0.cpu().numpy(), out) and np.array_equal(pm0.cpu().numpy(), pm)


def test_images_to_u8_equals_test_py_conversion():
    from training.tryon_pairs import images_to_u8
    rng = np.random.default_rng(3)
    steps = (np.arange(256, dtype=np.float64) + 0.5) / 127.5 - 1           # (x + 1) * 127.5 at exact .5 steps (as near as fp32 gets)
    eps = np.float32(1e-7)
    special = np.float32([-1, 1, -1 - eps, -1 + eps, 1 - eps, 1 + eps, np.nextafter(np.float32(-1), 0), np.nextafter(np.float32(1), 2),
                          -1.5, 1.5, 0, -0.0, 3e38, -3e38, np.inf, -np.inf])
    values = np.concatenate([special, steps.astype(np.float32), np.float32(np.nextafter(steps.astype(np.float32), 2)),
                             np.float32(np.nextafter(steps.astype(np.float32), -2)), rng.uniform(-1.2, 1.2, 3 * 2 * 256 * 256 - 16 - 3 * 256).astype(np.float32)])
    gen = values.reshape(2, 3, 256, 256).copy()
    gen[1, 2, 7, 40] = np.nan
    got = images_to_u8(_cu(gen), 32, 192).cpu().numpy()
    for i in range(2):
        with np.errstate(all='ignore'):
            ref = PR.image_to_u8(np.nan_to_num(gen[i], nan=-1.0))
        assert np.array_equal(got[i], ref), (i, int((got[i] != ref).sum()))
    assert got[1, 7, 40 - 32, 2] == 0                            # NaN -> 0
    assert got.min() == 0 and got.max() == 255


def test_pair_assemble_equals_test_py_expressions():
    """The seven-tensor form of pasta_tryon_outfit_assemble (outputs 0, 1 and 9 null, no photographs) on its own, on random
    uint8 stages (composites with all-zero pixels and one pixel whose channels sum to 256): the seven tensors equal test.py's
    torch expressions bit for bit.  N = 2, H = 20, P = 3 parts of 5 x 5: the 400 pixels do not fill whole blocks of 256, so the
    image part and the style_input tail meet inside one block.  The width is not read without photographs: W = 12, what the
    builder passes for such a square's canvas, and W = 20 give the same bits."""
    import ctypes
    from training.tryon_pairs import TryOnPairBatch
    rng = np.random.default_rng(4)
    n, h, parts, ph, pw = 2, 20, 3, 5, 5
    u8 = lambda *shape: rng.integers(0, 256, shape, dtype=np.uint8)
    retain_img = u8(n, h, h, 3) * (rng.uniform(size=[n, h, h, 1]) < 0.5).astype(np.uint8)
    stick, patches, stick_patches = u8(n, h, h, 3), u8(n, parts, ph, pw, 3), u8(n, parts, ph, pw, 3)
    den_u, den_l = (u8(n, h, h, 3) * (rng.uniform(size=[n, h, h, 1]) < 0.6).astype(np.uint8) for _ in range(2))
    den_u[1, 7, 13] = (128, 64, 64)                               # sums to 256: a wrapping uint8 sum would call it empty
    hwc = lambda a: a.transpose(1, 2, 0, 3).reshape(ph, pw, 3 * parts)
    stages = [dict(retain_img=retain_img[i], stick=stick[i], patches=hwc(patches[i]), stick_patches=hwc(stick_patches[i]),
                   denorm_upper=den_u[i], denorm_lower=den_l[i]) for i in range(n)]
    want = PR.generator_inputs([PR.getitem(s) for s in stages], 'cuda')
    N = _lib()
    # contiguous NaN-filled outputs (the restated tensors keep the strides of getitem's transposed views)
    from training.tryon_batch import OUTFIT_OUTPUTS
    assert OUTFIT_OUTPUTS[2:9] == TryOnPairBatch.KEYS
    ins = [None] * 3 + [_cu(a) for a in (retain_img, stick, patches, stick_patches, den_u, den_l)]
    for w in (12, 20):
        t = {k: torch.full(want[k].shape, float('nan'), device='cuda') for k in TryOnPairBatch.KEYS}
        outs = (ctypes.c_void_p * 10)(None, None, *[t[k].data_ptr() for k in TryOnPairBatch.KEYS], None)
        N.check(N.lib().pasta_tryon_outfit_assemble(*[N.ptr(a) for a in ins], outs, n, h, w, parts, parts, ph, pw, N.stream()))
        for k in TryOnPairBatch.KEYS:
            assert not torch.isnan(t[k]).any(), (w, k)            # every element was written
            assert t[k].shape == want[k].shape and torch.equal(t[k], want[k]), (w, k)
    assert tuple(t['style_input'].shape) == (n, 6 * parts, ph, pw) and tuple(t['pose'].shape) == (n, 6, h, h)
    assert t['denorm_upper_mask'][1, 0, 7, 13] == 1
    for k in ('denorm_upper_mask', 'denorm_lower_mask'):
        assert 0 < float(t[k].mean()) < 1, k                      # neither all 0 nor all 1


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_pair_tree(tmp_path_factory.mktemp('pairs_gpu'))


def _restated_batches(tree, batch):
    from training.dataset import UvitonDatasetV19_test, collate_pairs
    ds = UvitonDatasetV19_test(path=tree)
    for s in range(0, len(ds), batch):
        samples = [ds[i] for i in range(s, min(s + batch, len(ds)))]
        yield collate_pairs(samples), [PR.load_pair(r) for r in samples]


def test_builder_equals_the_restatement_on_the_tree(tree):
    from training.tryon_pairs import TryOnPairBatch, TryOnPairBatchBuilder
    builder = TryOnPairBatchBuilder('cuda')
    (raw, stages), = list(_restated_batches(tree, len(PAIRS)))
    b = builder.build(raw, keep_stages=True)
    assert b.batch == len(PAIRS) and b.person_name == raw['person_name'] and b.clothes_name == raw['clothes_name']
    want = PR.generator_inputs([PR.getitem(s) for s in stages], 'cuda')
    for k in TryOnPairBatch.KEYS:
        assert b.tensors[k].shape == want[k].shape and torch.equal(b.tensors[k], want[k]), k
    hwc = lambda t: t.permute(0, 2, 3, 1, 4).reshape(t.shape[0], t.shape[2], t.shape[3], -1)
    for i, ref in enumerate(stages):
        for name in ('palm', 'retain_img', 'stick', 'clothes_stick', 'lower_img', 'lower_mask', 'upper_img', 'upper_mask', 'denorm_upper', 'denorm_lower'):
            assert np.array_equal(b.stages[name][i].cpu().numpy(), ref[name]), (i, name)
        for name in ('patches', 'stick_patches', 'mask_patches'):
            assert np.array_equal(hwc(b.stages[name])[i].cpu().numpy(), ref[name]), (i, name)
    # pair 0: the donor has no shoulders or hips, so its torso, head and upper arms are blank while the person's exist
    no_shoulders = [0, 1, 2, 4]
    assert not b.stages['upper_valid'][0, no_shoulders].any() and b.stages['lower_valid'][0, :6].all()
    assert not b.stages['stick_patches'][0, no_shoulders].any() and b.stages['stick_patches'][0, 3].any()     # the forearm needs no shoulder
    assert b.stages['lower_valid'][1, 9]                         # the shin without its ankle falls back to the knee
    assert not b.stages['lower_valid'][2].any()                  # empty ``people``
    assert b.stages['denorm_upper'][1:].any() and b.stages['denorm_lower'].any()


def _snapshot(path):
    from training import networks
    G = PF.fill_module(networks.GeneratorV18(**PF.G_KWARGS)).eval().requires_grad_(False)
    D = networks.Discriminator(c_dim=512, img_resolution=256, img_channels=3, channel_base=512, channel_max=32)
    with open(path, 'wb') as f:
        pickle.dump(dict(G=G, D=D, G_ema=G), f)


def test_cli_writes_the_images_of_an_in_process_run(tree, tmp_path):
    import PIL.Image
    import legacy
    pkl, outdir = str(tmp_path / 'snapshot.pkl'), tmp_path / 'out'
    _snapshot(pkl)
    cmd = [sys.executable, os.path.join(ROOT, 'pasta-gan_amd', 'test.py'), '--network', pkl, '--outdir', str(outdir), '--dataroot', tree,
           '--batchsize', '2', '--noise-mode', 'const', '--workers', '0']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    names = {os.path.join(ds, p[:-4] + '__' + c[:-4] + '.png') for ds, p, c in PAIRS}
    found = {os.path.relpath(os.path.join(d, f), outdir) for d, _, fs in os.walk(outdir) for f in fs}
    assert found == names

    with open(pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].cuda()
    worst, differing, total = 0, 0, 0
    for raw, stages in _restated_batches(tree, 2):
        t = PR.generator_inputs([PR.getitem(s) for s in stages], 'cuda')
        n = len(stages)
        with torch.no_grad():                                    # test.py:119-128
            gen_c, cat_feat_list = G.style_encoding(t['style_input'], t['retain'])
            pose_feat = G.const_encoding(t['pose'])
            ws = G.mapping(torch.randn([n, 0], device='cuda'), gen_c)
            cat_feats = {str(c.shape[2]): c for c in cat_feat_list}
            _, gen_imgs, _, _ = G.synthesis(ws, pose_feat, cat_feats, t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                                            t['denorm_lower_mask'], noise_mode='const')
        gen_imgs = gen_imgs.cpu().numpy()
        for i in range(n):
            want = PR.image_to_u8(gen_imgs[i])
            p, c = raw['person_name'][i], raw['clothes_name'][i]
            img = PIL.Image.open(os.path.join(outdir, p.split('/')[0], os.path.basename(p)[:-4] + '__' + os.path.basename(c)[:-4] + '.png'))
            assert img.mode == 'RGB' and img.size == (192, 256)
            diff = np.abs(np.asarray(img).astype(np.int32) - want.astype(np.int32))
            worst, differing, total = max(worst, int(diff.max())), differing + int((diff > 0).sum()), total + diff.size
    print('e2e: max |diff| %d LSB, %d of %d values differ' % (worst, differing, total))
    # the same inputs in the same batches through the same kernels: at most 1 LSB anywhere, and in at most 0.1 % of the values
    assert worst <= 1 and differing <= total // 1000, (worst, differing, total)
