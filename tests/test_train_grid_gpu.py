"""The training run's sample grid on the GPU (csrc/train_grid.hip, training/snapshot_grid.py) against the numpy restatement of
the reference loop (tests/train_grid_ref.py) -- EXACT: the uint8 cells bit for bit, the fp32 minibatch tensors torch.equal to the
reference loop's own expressions evaluated by torch on the GPU, every byte of the tiled canvas."""
import numpy as np
import pytest
import torch

import train_grid_ref as G
from train_grid_tree import VIS_COUNT, make_tree

pytestmark = pytest.mark.gpu

GNUM = 6            # gap = 2: two rows in each third


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('train_grid'))


@pytest.fixture(scope='module')
def prepared(tree):
    from training.dataset import UvitonDatasetFull
    from training.snapshot_grid import SnapshotGrid
    from training.tryon_batch import FullBodyBatchBuilder
    ds = UvitonDatasetFull(tree)
    assert len(ds.vis_index) == VIS_COUNT
    ref = G.setup_snapshot_image_grid([ds[i] for i in ds.vis_index], GNUM)
    grid = SnapshotGrid.setup(ds, FullBodyBatchBuilder('cuda'), 'cuda', gnum=GNUM)
    return ds, ref, grid


def test_inputs_do_real_work(prepared):
    """Checked on the restatement alone.  'Differs from the whole-outfit cell of the same pair': in the first and last third the
    cell of (person, donor) is compared with the composite the whole-outfit rule would give that pair; in the middle third, where
    the cell IS that composite, with the person wearing their own clothes -- so each third's source rule changes the picture."""
    _, ref, _ = prepared
    gap = GNUM // 3
    args = (ref['norm_img'], ref['norm_img_lower'], ref['m_invs'], ref['masks'], ref['masks_lower'])
    for third in range(3):
        differs = 0
        for row in range(third * gap, (third + 1) * gap):
            for col in range(GNUM):
                src = row if third == 1 else col
                u, l, _ = G.denorm_from(*args, src, src, row)
                i = row * GNUM + col
                differs += not (np.array_equal(u.transpose(2, 0, 1), ref['denorm_upper'][i]) and
                                np.array_equal(l.transpose(2, 0, 1), ref['denorm_lower'][i]))
        assert differs > 0, third
    assert max(ref['skipped']) > 0 and min(ref['skipped']) == 0
    assert ref['denorm_lower'].any() and ref['denorm_upper'].any()
    assert ref['denorm_upper_mask'].any() and not ref['denorm_upper_mask'].all()


def test_every_cell_equals_the_restatement(prepared):
    _, ref, grid = prepared
    assert grid.denorm_upper.dtype == grid.denorm_lower.dtype == torch.uint8
    got_u = grid.denorm_upper.permute(0, 3, 1, 2).cpu().numpy()
    got_l = grid.denorm_lower.permute(0, 3, 1, 2).cpu().numpy()
    for i in range(GNUM * GNUM):
        assert np.array_equal(got_u[i], ref['denorm_upper'][i]), ('upper', divmod(i, GNUM), int((got_u[i] != ref['denorm_upper'][i]).sum()))
        assert np.array_equal(got_l[i], ref['denorm_lower'][i]), ('lower', divmod(i, GNUM), int((got_l[i] != ref['denorm_lower'][i]).sum()))


def test_minibatch_tensors_equal_the_loops_expressions(prepared):
    _, ref, grid = prepared
    batch = 7                                   # does not divide 36: the last minibatch has one cell
    seen = 0
    for lo in range(0, GNUM * GNUM, batch):
        hi = min(lo + batch, GNUM * GNUM)
        got = grid.inputs(lo, hi)
        want = G.generator_inputs(ref, GNUM, lo, hi, 'cuda')
        assert sorted(got) == sorted(want)
        for k, v in want.items():
            assert got[k].dtype == torch.float32 and got[k].shape == v.shape, (k, got[k].shape, v.shape)
            assert torch.equal(got[k], v), (k, lo, int((got[k] != v).sum()))
        seen += hi - lo
    assert seen == GNUM * GNUM


def test_identity_index_equals_the_eroded_composite():
    from oracle import ref_patches as RP
    from torch_utils.ops import _native
    rng = np.random.default_rng(11)
    n, P, ph, pw, H, W = 3, 5, 64, 64, 256, 256
    patches = torch.from_numpy(rng.integers(0, 256, [n, P, ph, pw, 3], dtype=np.uint8)).cuda()
    masks = torch.from_numpy(((rng.uniform(size=[n, P, ph // 8, pw // 8, 1]) < 0.8) * 255).astype(np.uint8).repeat(8, 2).repeat(8, 3)
                             .repeat(3, 4)).cuda().contiguous()
    corners = np.float32([[0, 0], [0, ph], [pw, ph], [pw, 0]])
    minv = np.zeros([n, P, 9])
    for i in range(n):
        for k in range(P):
            quad = np.float32(rng.uniform(20, 236, [4, 2]))
            minv[i, k] = RP.invert3x3(RP.get_perspective_transform(corners, quad)).reshape(9)
    valid = np.ones([n, P], np.uint8)
    valid[1, 2] = valid[2, 0] = 0
    minv_t, valid_t = torch.from_numpy(minv).cuda(), torch.from_numpy(valid).cuda()
    index = torch.arange(n * P, dtype=torch.int32, device='cuda')
    lib, p, s = _native.lib(), _native.ptr, _native.stream()
    for radius in (0, 2):
        want, got = (torch.full([n, H, W, 3], 7, dtype=torch.uint8, device='cuda') for _ in range(2))
        _native.check(lib.pasta_patch_composite_eroded_u8(p(patches), p(masks), p(minv_t), p(valid_t), p(want), None, n, P, ph, pw, H, W, radius, None, s))
        _native.check(lib.pasta_grid_composite_eroded_u8(p(patches), p(masks), p(index), p(minv_t), p(valid_t), p(got), n, P, n * P, ph, pw, H, W,
                                                         radius, s))
        assert torch.equal(got, want), radius
        assert want.any()


def _tiling_inputs(C):
    """[n, C, H, W] fp32 in drange [-1, 1] (scale 127.5): exact .5 ties of both parities, values beyond both ends, a NaN."""
    rng = np.random.default_rng(C)
    g, H = 3, 8
    img = rng.uniform(-1.2, 1.2, [g * g, C, H, H]).astype(np.float32)
    # (x + 1) * 127.5 = k + .5 exactly for x = (2 k + 1) / 255 - 1 when that is representable: take the ones that are
    ties = [np.float32((2 * k + 1) / 255 - 1) for k in range(255)]
    ties = [t for t in ties if float((t - np.float32(-1)) * np.float32(127.5)) % 1 == 0.5]
    parities = {int(float((t + np.float32(1)) * np.float32(127.5))) % 2 for t in ties}
    assert parities == {0, 1}, 'ties that round down to an even and up from an odd integer'
    img.reshape(-1)[:len(ties)] = ties
    img[1, 0, 0, :4] = [-1.5, 1.5, -1.0, 1.0]
    img[2, 0, 1, 1] = np.nan
    people = rng.uniform(-1, 1, [g, C, H, H]).astype(np.float32)
    return g, H, img, people


@pytest.mark.parametrize('C', [3, 1])
def test_tiling_equals_save_image_grid(C):
    from training.snapshot_grid import SnapshotGrid
    g, H, img, people = _tiling_inputs(C)
    side, top = G.frame(people)
    want = G.save_image_grid(side, top, img, [-1, 1], (g, g))
    grid = SnapshotGrid.__new__(SnapshotGrid)           # the tiling alone: no data set behind it
    grid.device, grid.gnum, grid.cells, grid.H = torch.device('cuda'), g, g * g, H
    canvas = torch.full([(g + 1) * H, (g + 1) * H, C], 99, dtype=torch.uint8, device='cuda')
    dev = lambda a: torch.from_numpy(a).cuda()
    grid._tile(canvas, torch.zeros([1, C, H, H], device='cuda'), 0, 1, 0, 0, (-1, 1))
    grid._tile(canvas, dev(people), 0, 1, 0, 1, (-1, 1))
    grid._tile(canvas, dev(people), 0, g, 1, 0, (-1, 1))
    for lo in range(0, g * g, 4):                       # minibatches of 4, 4 and 1
        grid._tile(canvas, dev(img[lo:lo + 4]), lo, g, 1, 1, (-1, 1))
    got = canvas.cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).sum())
    assert (want[:H, :H] == 128).all()                  # the corner tile: zeros in [-1, 1] are 127.5, which rounds to even


def test_frame_equals_the_reference_side_and_top(prepared):
    _, ref, grid = prepared
    images, _, _ = G.person_tensors(ref, 'cuda')
    side, top = G.frame(images.cpu().numpy())
    H = grid.H
    got = grid.frame(3).cpu().numpy()
    blank = np.zeros([GNUM * GNUM, 3, H, H], np.float32)
    want = G.save_image_grid(side, top, blank, [-1, 1], (GNUM, GNUM))
    assert np.array_equal(got[:H], want[:H]) and np.array_equal(got[:, :H], want[:, :H])


def test_too_few_listed_people(prepared):
    from training.snapshot_grid import SnapshotGrid
    from training.tryon_batch import FullBodyBatchBuilder
    ds, _, _ = prepared
    with pytest.raises(IOError, match=r'needs 23 people .* has %d' % VIS_COUNT):
        SnapshotGrid.setup(ds, FullBodyBatchBuilder('cuda'), 'cuda', gnum=23)
