"""Row f4, the try-on data set's per-sample preparation on the GPU (csrc/tryon_inputs.hip, training/tryon_batch.py) against the
numpy restatement of the reference (tests/tryon_ref.py) -- EXACT: the uint8 stages bit for bit, the fp32 tensors equal to the
reference loop's own expressions (x / 127.5 - 1 evaluated by torch on the GPU, as training_loop...:425-456 does)."""
import numpy as np
import pytest
import torch

import tryon_ref as R
from oracle import ref_patches as RP
from tryon_tree import make_tree

pytestmark = pytest.mark.gpu


def _keypoints(rng, n):
    """Random poses with every oddity: missing joints, coincident endpoints, negative and out-of-canvas coordinates."""
    kp = np.zeros([n, 18, 3])
    kp[..., 0] = rng.uniform(-30, 230, [n, 18])
    kp[..., 1] = rng.uniform(-30, 290, [n, 18])
    kp[..., 2] = rng.uniform(0, 1, [n, 18])
    kp[rng.uniform(size=[n, 18]) < 0.15, 2] = 0.1 - 1e-9
    for i in range(n):
        a, b = rng.integers(0, 18, 2)
        kp[i, b, :2] = kp[i, a, :2]                          # coincident endpoints
        kp[i, 3, :2] = kp[i, 2, :2] + rng.integers(-3, 4, 2)  # a very short upper arm
    kp[0, 2:8, 2] = 0.9
    kp[0, 6, :2] = kp[0, 5, :2]                               # left upper arm of length zero
    kp[1, 4, :2] = (300.5, -20.25)                            # right wrist far outside
    return kp


def _labels(rng, kp):
    n = kp.shape[0]
    lab = rng.integers(0, 20, [n, 32, 24]).repeat(8, 1).repeat(8, 2).astype(np.uint8)
    yy, xx = np.mgrid[0:256, 0:192]
    for i in range(n):
        for j, label in ((7, 14), (6, 14), (5, 14), (4, 15), (3, 15), (2, 15)):
            lab[i][(yy - kp[i, j, 1]) ** 2 + (xx - kp[i, j, 0]) ** 2 < rng.uniform(10, 30) ** 2] = label
    return lab


def _launch_front(image, parsing, kp):
    """The three uint8 kernels before the warps, through the builder's own host code."""
    from torch_utils.ops import _native
    from training import tryon_batch as TB
    n = image.shape[0]
    limbs, joints = TB.stick_tables(kp)
    quads, present = TB.palm_quads(kp, 32)
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    img, lab, limbs, joints, quads, present = cu(image), cu(parsing), cu(limbs), cu(joints), cu(quads), cu(present)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device='cuda')
    stick, palm, retain, gt = u8(n, 256, 256, 3), u8(n, 256, 256), u8(n, 256, 256), u8(n, 256, 256)
    g = [u8(n, 256, 256, 3) for _ in range(4)]
    lib, P, s = _native.lib(), _native.ptr, _native.stream()
    _native.check(lib.pasta_pose_stickman_u8(P(limbs), P(joints), P(stick), n, 256, 192, 2, 2, s))
    _native.check(lib.pasta_palm_mask_u8(P(lab), P(quads), P(present), P(palm), n, 256, 192, 25, 16, s))
    _native.check(lib.pasta_tryon_masks_u8(P(img), P(lab), P(palm), P(retain), P(gt), *[P(t) for t in g], n, 256, 192, s))
    out = [t.cpu().numpy() for t in (stick, palm, retain, gt, *g)]
    return out


@pytest.mark.parametrize('seed', [0, 1])
def test_uint8_kernels_equal_the_restatement(seed):
    rng = np.random.default_rng(seed)
    n = 6
    kp = _keypoints(rng, n)
    parsing = _labels(rng, kp)
    image = rng.integers(0, 256, [n, 256, 192, 3], dtype=np.uint8)
    stick, palm, retain, gt, ui, li, um, lm = _launch_front(image, parsing, kp)
    palms = 0
    for i in range(n):
        ref = R.label_masks(image[i], parsing[i], kp[i])
        assert np.array_equal(stick[i], ref[1]), (i, 'stick figure')
        assert np.array_equal(palm[i], ref[8]), (i, 'palm', int((palm[i] != ref[8]).sum()))
        for k, got in ((2, retain), (3, gt), (4, ui), (5, li), (6, um), (7, lm)):
            assert np.array_equal(got[i], ref[k]), (i, k)
        palms += int(ref[8].sum())
    assert palms > 0 and stick.any() and set(np.unique(gt)) == {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize('box', [25, 16])
def test_palm_dilation_equals_a_brute_force_max_filter(box):
    """All labels 14 (left hand) and one left segment whose fill lands in the image, the other one off the canvas (empty fill):
    the palm is then exactly the complement of the one dilated fill."""
    from torch_utils.ops import _native
    from training import tryon_batch as TB
    rng = np.random.default_rng(box)
    for trial in range(4):
        quads = np.zeros([1, 4, 4, 2])
        present = np.array([[1, 1, 0, 0]], np.uint8)
        p, q = rng.uniform(10, 246, 2), rng.uniform(10, 246, 2)
        lit = 0 if box == 25 else 1
        corners = TB.rectangle_corners(p[0], p[1], q[0], q[1])
        quads[0, lit] = corners
        quads[0, 1 - lit] = [[-500, -500], [-480, -500], [-480, -480], [-500, -480]]
        lab = np.full([1, 256, 192], 14, np.uint8)
        cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        out = torch.empty([1, 256, 256], dtype=torch.uint8, device='cuda')
        lab_t, quads_t, present_t = cu(lab), cu(quads), cu(present)       # held: the kernel runs after the pointers are taken
        _native.check(_native.lib().pasta_palm_mask_u8(_native.ptr(lab_t), _native.ptr(quads_t), _native.ptr(present_t),
                                                      _native.ptr(out), 1, 256, 192, 25, 16, _native.stream()))
        fill = R.rle_fr_poly([float(v) for v in corners.reshape(-1)], 256, 256)
        want = 1 - R.dilate(fill, box)
        want[:, :32] = 0
        want[:, 224:] = 0                                 # the padding carries label 0
        assert fill.any()
        assert np.array_equal(out[0].cpu().numpy(), want), (box, trial)


def _reference_batch(samples):
    """_load_raw_image -> normalize -> __getitem__ per sample, then the loop's conversions evaluated by torch on the GPU."""
    per = []
    for s in samples:
        image, pose, retain, gt, ui, li, um, lm, palm = R.label_masks(s['image'], s['parsing'], s['keypoints'])
        ni, nl, du, dl, _, hands, _, _ = RP.normalize(ui, li, um, lm, s['keypoints'])
        erase = R.erase_mask(hands, s['erase_mask'])[None]
        du = du.transpose(2, 0, 1) * (1 - erase)
        dl = dl.transpose(2, 0, 1) * (1 - erase)
        per.append(dict(real=image.transpose(2, 0, 1), pose=pose.transpose(2, 0, 1), ni=ni.transpose(2, 0, 1), nl=nl.transpose(2, 0, 1),
                        du=du, dl=dl, gt=gt[None], dum=(np.sum(du, axis=0, keepdims=True) > 0).astype(np.uint8),
                        dlm=(np.sum(dl, axis=0, keepdims=True) > 0).astype(np.uint8), retain=retain[None],
                        stages=dict(stick=pose, retain_mask=retain, gt_parsing=gt, upper_img=ui, lower_img=li, upper_mask=um, lower_mask=lm,
                                    norm_img=ni, norm_img_lower=nl)))
    b = {k: torch.from_numpy(np.stack([p[k] for p in per])).cuda() for k in per[0] if k != 'stages'}
    real = b['real'].to(torch.float32) / 127.5 - 1
    head = b['retain'] * real - (1 - b['retain'])
    t = dict(real_img=real,
             style_input=torch.cat([b['ni'].to(torch.float32) / 127.5 - 1, b['nl'].to(torch.float32) / 127.5 - 1], dim=1),
             retain=head, pose=torch.cat((b['pose'].to(torch.float32) / 127.5 - 1, head), dim=1),
             denorm_upper_input=b['du'].to(torch.float32) / 127.5 - 1, denorm_lower_input=b['dl'].to(torch.float32) / 127.5 - 1,
             denorm_upper_mask=b['dum'].to(torch.float32), denorm_lower_mask=b['dlm'].to(torch.float32), gt_parsing=b['gt'].to(torch.float32))
    return t, [p['stages'] for p in per]


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('tryon_gpu'))


def test_builder_equals_the_reference_pipeline(tree):
    from training.dataset import UvitonDatasetFull, collate
    from training.tryon_batch import FullBodyBatchBuilder
    ds = UvitonDatasetFull(tree)
    rng = np.random.default_rng(5)
    samples = [ds[i] for i in range(len(ds))]
    # erase masks of several sizes: the tree's two, an integer factor, a 2x reduction and an odd size
    for s, hw in zip(samples[2:], [(128, 128), (512, 384), (77, 131)]):
        s['erase_mask'] = (rng.uniform(size=hw) < 0.3).astype(np.uint8) * np.uint8(255)
    samples[1]['erase_mask'] = rng.integers(0, 256, [256, 192], dtype=np.uint8)
    got = FullBodyBatchBuilder('cuda').build(collate(samples), keep_stages=True)
    want, stages = _reference_batch(samples)
    for k, v in want.items():
        g = got.tensors[k]
        assert g.dtype == torch.float32 and g.shape == v.shape, (k, g.shape, v.shape)
        assert torch.equal(g, v), (k, int((g != v).sum()))
    for i, st in enumerate(stages):
        for k, v in st.items():
            assert np.array_equal(got.stages[k][i].cpu().numpy(), v), (i, k)
    assert got.batch == len(samples) and len(got.split(2)) == 3
    assert got.tensors['denorm_upper_mask'].any() and not torch.equal(got.tensors['retain'], -torch.ones_like(got.tensors['retain']))


def test_training_step_on_the_tiny_tree(tree):
    from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
    cfg = fashion_config(channel_base=2048, mbstd_group_size=2)
    step = training_loop(batch_size=2, batch_gpu=2, total_iters=2, cfg=cfg, device=torch.device('cuda'),
                         training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree),
                         data_loader_kwargs=dict(num_workers=0, pin_memory=True))
    assert step.cur_nimg == 4
    # one more iteration by hand: losses finite, parameters move
    from training.dataset import UvitonDatasetFull, collate
    from training.tryon_batch import FullBodyBatchBuilder
    ds = UvitonDatasetFull(tree)
    data = FullBodyBatchBuilder('cuda').build(collate([ds[3], ds[4]]))
    log = {}
    step.loss.report = lambda name, value: log.__setitem__(name, value)
    before = [p.detach().clone() for p in step.G.parameters()] + [p.detach().clone() for p in step.D.parameters()]
    step.run(data)
    after = list(step.G.parameters()) + list(step.D.parameters())
    assert any(not torch.equal(a, b) for a, b in zip(after, before))
    losses = {k: v for k, v in log.items() if k.startswith('Loss/')}
    assert losses and all(torch.isfinite(torch.as_tensor(v).float()).all() for v in losses.values()), sorted(losses)
