"""pasta_region_image_stats (csrc/recon_metrics.hip) against the numpy fp64 restatement (tests/tryon_fidelity_ref.py), against
pasta_recon_image_stats under a mask of ones, and its refusals.

The bytes are taken from ``images_to_u8`` on the GPU, so what is compared is the statistics alone: the integer sums and the window
counts must be equal, SSIM is evaluated in fp32 on the GPU and held to SSIM_TOL on the per-image mean over the counted windows."""
import ctypes

import numpy as np
import pytest
import torch

import recon_ref as R
import tryon_fidelity_ref as F

pytestmark = pytest.mark.gpu

# Bound on |per-image mean SSIM of the kernel - the fp64 restatement| over the counted windows: the bound
# tests/test_recon_metrics_gpu.py holds the unmasked kernel to (ten times its largest deviation on an MI355X, which came from
# images of 11 x 11, three windows, as the block masks here have).  The masked kernel evaluates the same expression on the same
# moments; the test prints every case's deviation (DESIGN.md section 8d says what to do with the largest).
SSIM_TOL = R.SSIM_TOL

N = 3
SHAPES = [(11, 11), (12, 13), (33, 43), (45, 75)]       # 33 x 43: one position past a tile of 22 x 32 in both directions


def _inputs(rng, h, w):
    """Random images in [-1.2, 1.2] with a few NaN in a wider square, and a wider random reference: (images [N,3,h,wt], c0,
    ref [N,h,wr,3], r0)."""
    wt, c0, wr, r0 = w + 9, 4, w + 6, 5
    images = rng.uniform(-1.2, 1.2, [N, 3, h, wt]).astype(np.float32)
    images[rng.random(images.shape) < 0.003] = np.nan
    images[0, 1, h // 2, c0 + w // 2] = np.nan
    ref = rng.integers(0, 256, [N, h, wr, 3], dtype=np.uint8)
    return images, c0, ref, r0


def _block(h, w, y, x, hole=False):
    m = np.zeros([N, h, w], np.uint8)
    m[:, y:y + 11, x:x + 11] = 1
    if hole:
        m[:, y + 4, x + 7] = 0
    return m


def _masks(rng, h, w):
    """name -> (mask [N, h, w] of 0 and nonzero bytes, expected windows per image or None)."""
    one = np.zeros([N, h, w], np.uint8)
    one[:, h // 2, w // 3] = 255
    per_image = np.stack([np.ones([h, w], np.uint8), (rng.random([h, w]) < 0.9).astype(np.uint8) * 7, np.zeros([h, w], np.uint8)])
    per_image[2, :h // 2 + 6, : w // 2 + 6] = 1
    masks = dict(ones=(np.ones([N, h, w], np.uint8), 3 * (h - 10) * (w - 10)), zeros=(np.zeros([N, h, w], np.uint8), 0), one_pixel=(one, 0),
                 dense=((rng.random([N, h, w]) < 0.97).astype(np.uint8) * 255, None), per_image=(per_image, None))
    # a block of 11 x 11 has one window: at the first position of the next tile, (22, 32), where the image reaches that far;
    # with its pixels on both sides of the tiles' boundary rows and columns; in the corner otherwise
    places = [(22, 32), (17, 27)] if h >= 33 and w >= 43 else [(h - 11, w - 11)]
    for y, x in places:
        masks['block_%d_%d' % (y, x)] = (_block(h, w, y, x), 3)
        masks['hole_%d_%d' % (y, x)] = (_block(h, w, y, x, hole=True), 0)
    return masks


def _wide(mask, wm, m0, rng):
    """The mask inside a wider tensor whose other columns hold noise."""
    out = rng.integers(0, 256, [mask.shape[0], mask.shape[1], wm], dtype=np.uint8)
    out[:, :, m0:m0 + mask.shape[2]] = mask
    return out


@pytest.mark.parametrize('h, w', SHAPES)
def test_region_stats_against_the_oracle(h, w):
    from metrics.metric_utils import region_image_stats
    from training.tryon_pairs import images_to_u8
    rng = np.random.default_rng(100 * h + w)
    images, c0, ref, r0 = _inputs(rng, h, w)
    d_images, d_ref = torch.from_numpy(images).cuda(), torch.from_numpy(ref).cuda()
    gen = images_to_u8(d_images, c0, w).cpu().numpy()
    crop = ref[:, :, r0:r0 + w]
    worst = 0.0
    for name, (mask, expect_windows) in _masks(rng, h, w).items():
        wm, m0 = w + 3, 2
        d_mask = torch.from_numpy(_wide(mask, wm, m0, rng)).cuda()
        sums, ssim = region_image_stats(d_images, d_ref, d_mask, c0, r0, m0, w)
        sums2, ssim2 = region_image_stats(d_images.clone(), d_ref.clone(), d_mask.clone(), c0, r0, m0, w)
        assert torch.equal(sums, sums2) and torch.equal(ssim.view(torch.int64), ssim2.view(torch.int64)), name     # bit-identical
        sad, ssd, windows, nbytes, want = F.region_stats(gen, crop, mask)
        sums, ssim = sums.cpu().numpy(), ssim.cpu().numpy()
        assert sums[:, 0].tolist() == sad.tolist() and sums[:, 1].tolist() == ssd.tolist(), name
        assert sums[:, 2].tolist() == windows.tolist() and sums[:, 3].tolist() == nbytes.tolist(), name
        if expect_windows is not None:
            assert windows.tolist() == [expect_windows] * N, name
        if name.startswith('block'):
            assert nbytes.tolist() == [3 * 121] * N
        if name.startswith('hole'):
            assert nbytes.tolist() == [3 * 120] * N
        if name == 'zeros':
            assert not sums.any()
        has = windows > 0
        assert (ssim[~has] == 0.0).all() and np.isfinite(ssim).all(), name
        dev = np.abs(ssim[has] / windows[has] - want[has] / windows[has]).max() if has.any() else 0.0
        print('region_image_stats %dx%d %-12s windows %s largest deviation %.3e' % (h, w, name, windows.tolist(), dev))
        worst = max(worst, dev)
        assert dev <= SSIM_TOL, (name, dev)
    print('region_image_stats %dx%d: largest deviation of the mean SSIM over all masks %.3e' % (h, w, worst))


@pytest.mark.parametrize('h, w, wt', [(33, 43, 50), (256, 192, 256)])
def test_a_mask_of_ones_gives_the_bits_of_recon_image_stats(h, w, wt):
    from metrics.metric_utils import recon_image_stats, region_image_stats
    rng = np.random.default_rng(h)
    c0 = (wt - w) // 2
    images = rng.uniform(-1.2, 1.2, [2, 3, h, wt]).astype(np.float32)
    images[rng.random(images.shape) < 0.001] = np.nan
    d_images = torch.from_numpy(images).cuda()
    photos = torch.from_numpy(rng.integers(0, 256, [2, h, w, 3], dtype=np.uint8)).cuda()
    ones = torch.ones([2, h, w], dtype=torch.uint8, device='cuda')
    sums, ssim = region_image_stats(d_images, photos, ones, c0, 0, 0, w)
    sums0, ssim0 = recon_image_stats(d_images, photos, c0)
    assert torch.equal(sums[:, :3], sums0) and sums[:, 3].tolist() == [3 * h * w] * 2
    assert torch.equal(ssim.view(torch.int64), ssim0.view(torch.int64))
    assert float(ssim0.abs().min()) > 0


def test_two_calls_give_the_same_bits():
    from metrics.metric_utils import region_image_stats
    rng = np.random.default_rng(3)
    images = torch.from_numpy(rng.uniform(-1.2, 1.2, [N, 3, 70, 90]).astype(np.float32)).cuda()
    ref = torch.from_numpy(rng.integers(0, 256, [N, 70, 70, 3], dtype=np.uint8)).cuda()
    mask = torch.from_numpy((rng.random([N, 70, 80]) < 0.98).astype(np.uint8)).cuda()
    a = region_image_stats(images, ref, mask, 10, 0, 5, 70)
    b = region_image_stats(images, ref, mask, 10, 0, 5, 70)
    assert int(a[0][:, 2].min()) > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


def test_refusals_launch_nothing():
    from metrics.metric_utils import region_image_stats
    from torch_utils.ops import _native
    z = lambda *s: torch.zeros(s, device='cuda')
    u = lambda *s: torch.zeros(s, dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11 SSIM window'):
        region_image_stats(z(1, 3, 10, 64), u(1, 10, 64, 3), u(1, 10, 64), 0, 0, 0, 64)
    with pytest.raises(RuntimeError, match='bad crop of the mask'):
        region_image_stats(z(1, 3, 32, 40), u(1, 32, 40, 3), u(1, 32, 30), 0, 0, 7, 24)
    with pytest.raises(RuntimeError, match='bad crop of the reference'):
        region_image_stats(z(1, 3, 32, 40), u(1, 32, 26, 3), u(1, 32, 40), 0, 3, 0, 24)
    with pytest.raises(RuntimeError, match='bad shape or crop of the images'):
        region_image_stats(z(1, 3, 32, 40), u(1, 32, 40, 3), u(1, 32, 40), 17, 0, 0, 24)
    # a workspace one byte short, through the C entry: an error return, and the outputs keep their canaries
    lib, P = _native.lib(), _native.ptr
    need = int(lib.pasta_region_image_stats_workspace(2, 40, 50))
    assert need == 2 * 3 * 2 * 2 * 40 and int(lib.pasta_region_image_stats_workspace(2, 10, 50)) == 0
    images, ref, mask = z(2, 3, 40, 50), u(2, 40, 50, 3), u(2, 40, 50)
    work = torch.zeros([need], dtype=torch.uint8, device='cuda')
    sums = torch.full([2, 4], -7, dtype=torch.int64, device='cuda')
    ssim = torch.full([2], -7.0, dtype=torch.float64, device='cuda')
    args = (P(images), P(ref), P(mask), P(sums), P(ssim), P(work))
    assert lib.pasta_region_image_stats(*args, need - 1, 2, 40, 50, 0, 50, 0, 50, 0, 50, _native.stream()) != 0
    assert b'workspace' in lib.pasta_last_error()
    assert lib.pasta_region_image_stats(*args, need, 2, 10, 50, 0, 50, 0, 50, 0, 50, _native.stream()) != 0
    torch.cuda.synchronize()
    assert (sums == -7).all() and (ssim == -7.0).all() and not work.any()
    assert lib.pasta_region_image_stats(*args, need, 2, 40, 50, 0, 50, 0, 50, 0, 50, _native.stream()) == 0
    torch.cuda.synchronize()
    assert sums.tolist() == [[0, 0, 0, 0]] * 2 and ssim.tolist() == [0.0, 0.0]
