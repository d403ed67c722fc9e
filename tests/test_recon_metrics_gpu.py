"""The two statistics kernels of csrc/recon_metrics.hip against the numpy fp64 restatement (tests/recon_ref.py).

The byte rule is taken from ``images_to_u8`` on the GPU, so what is compared is the statistics alone.  The difference sums
are integers and must be equal; SSIM is evaluated in fp32 on the GPU and held to SSIM_TOL on the per-image mean."""
import numpy as np
import pytest
import torch

import recon_ref as R

pytestmark = pytest.mark.gpu

SSIM_TOL = R.SSIM_TOL

SHAPES = [(256, 192, 256), (512, 320, 512), (37, 23, 40), (11, 11, 11)]       # H, W, Wt


def _photos(rng, n, h, w):
    # blocks of 4 x 4 with noise on top: structure at the scale of the window, every byte value in reach
    coarse = rng.integers(0, 256, [n, (h + 3) // 4, (w + 3) // 4, 3]).repeat(4, 1).repeat(4, 2)[:, :h, :w]
    return np.clip(coarse + rng.integers(-20, 21, [n, h, w, 3]), 0, 255).astype(np.uint8)


def _images(kind, rng, photos, wt, c0):
    n, h, w, _ = photos.shape
    x = rng.uniform(-1, 1, [n, 3, h, wt]).astype(np.float32)                   # the padding holds noise: it must not be scored
    inner = x[..., c0:c0 + w]
    p = photos.transpose(0, 3, 1, 2).astype(np.float64)
    if kind == 'random':
        pass
    elif kind == 'near':                                                        # the photograph with a generator's kind of error
        inner[:] = ((p + rng.normal(0, 6, p.shape)) / 127.5 - 1).astype(np.float32)
    elif kind == 'equal':                                                       # mid-bucket values: the bytes are the photograph's
        inner[:] = ((p + 0.5) / 127.5 - 1).astype(np.float32)
    elif kind == 'constant':
        for i in range(n):
            inner[i] = np.float32([-1.0, 1.0, 0.25, -0.4, 0.0][i % 5])
    elif kind == 'wild':                                                        # outside [-1, 1], infinities and NaNs
        inner[:] = (rng.normal(0, 2, inner.shape)).astype(np.float32)
        inner[:, 0, 0, 0] = np.nan
        inner[:, 0, 0, 5] = np.inf
        inner[:, 1, h // 2, w // 2] = np.nan
        inner[:, 2, h - 1, w - 1] = -np.inf
    else:
        raise AssertionError(kind)
    return x


def _check(kind, n, h, w, wt, seed):
    from metrics.metric_utils import recon_image_stats
    from training.tryon_pairs import images_to_u8
    rng = np.random.default_rng(seed)
    c0 = (wt - w) // 2
    photos = _photos(rng, n, h, w)
    if kind == 'constant':
        photos[0] = 255                                                         # constant against constant as well
    images = _images(kind, rng, photos, wt, c0)
    d_images, d_photos = torch.from_numpy(images).cuda(), torch.from_numpy(photos).cuda()
    sums, ssim = recon_image_stats(d_images, d_photos, c0)
    sums2, ssim2 = recon_image_stats(d_images.clone(), d_photos.clone(), c0)
    assert torch.equal(sums, sums2) and torch.equal(ssim.view(torch.int64), ssim2.view(torch.int64))        # bit-identical
    gen = images_to_u8(d_images, c0, w).cpu().numpy()
    if kind == 'equal':
        assert np.array_equal(gen, photos)
    sad, ssd, want, windows = R.image_stats(gen, photos)
    sums, ssim = sums.cpu().numpy(), ssim.cpu().numpy()
    assert sums[:, 0].tolist() == sad.tolist() and sums[:, 1].tolist() == ssd.tolist() and sums[:, 2].tolist() == windows.tolist()
    dev = np.abs(ssim / windows - want / windows)
    print('recon_image_stats %-8s N=%d %dx%d in %d: mean SSIM %s, largest deviation %.3e' % (kind, n, h, w, wt,
          np.array2string(want / windows, precision=4), dev.max()))
    assert np.isfinite(ssim).all() and dev.max() <= SSIM_TOL, dev
    if kind == 'equal':
        assert (sums[:, :2] == 0).all() and np.abs(ssim / windows - 1).max() <= 1e-6
    return dev.max()


@pytest.mark.parametrize('kind', ['random', 'near', 'equal', 'constant', 'wild'])
@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('h, w, wt', SHAPES)
def test_image_stats_against_the_oracle(kind, n, h, w, wt):
    _check(kind, n, h, w, wt, seed=h * 7 + n)


def test_image_stats_with_the_content_at_the_left_edge_and_odd_padding():
    _check('near', 2, 50, 33, 64, seed=1)                                       # c0 = 15
    from metrics.metric_utils import recon_image_stats
    x = torch.zeros([1, 3, 40, 64], device='cuda')
    p = torch.zeros([1, 40, 30, 3], dtype=torch.uint8, device='cuda')
    a = recon_image_stats(x, p, 0)
    b = recon_image_stats(x, p, 34)
    assert torch.equal(a[0], b[0]) and int(a[0][0, 0]) == 127 * 40 * 30 * 3


@pytest.mark.parametrize('h, w', [(10, 64), (64, 10), (10, 10)])
def test_image_stats_refuse_an_image_smaller_than_the_window(h, w):
    from metrics.metric_utils import recon_image_stats
    x = torch.zeros([1, 3, h, w], device='cuda')
    p = torch.zeros([1, h, w, 3], dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11 SSIM window'):
        recon_image_stats(x, p, 0)


def test_image_stats_refuse_a_crop_outside_the_square():
    from metrics.metric_utils import recon_image_stats
    x = torch.zeros([1, 3, 32, 40], device='cuda')
    p = torch.zeros([1, 32, 24, 3], dtype=torch.uint8, device='cuda')
    with pytest.raises(RuntimeError, match='bad shape or crop'):
        recon_image_stats(x, p, 17)


# ---- confusion ----

def _confusion_case(rng, n, c, h, wt):
    logits = (np.round(rng.normal(0, 1.5, [n, c, h, wt]) * 2) / 2).astype(np.float32)        # half-integer steps: many ties
    logits[rng.random(logits.shape) < 0.1] = np.nan
    logits[rng.random(logits.shape) < 0.01] = np.inf
    logits[rng.random(logits.shape) < 0.01] = -np.inf
    logits[:, :, rng.random([h, wt]) < 0.03] = np.nan                                        # pixels without any number
    labels = rng.integers(0, c, [n, 1, h, wt]).astype(np.float32)
    other = rng.random(labels.shape)
    for value, lo in [(255.0, 0.00), (float(c), 0.05), (-1.0, 0.10), (np.nan, 0.13), (c - 0.5, 0.15), (-0.5, 0.17)]:
        labels[(other >= lo) & (other < lo + 0.02)] = value
    return logits, labels


@pytest.mark.parametrize('n, c, h, w, wt, c0', [(3, 6, 37, 23, 40, 8), (2, 6, 256, 192, 256, 32), (1, 32, 16, 16, 16, 0), (2, 1, 9, 5, 12, 7),
                                                (1, 6, 512, 320, 512, 96)])
def test_confusion_against_the_oracle(n, c, h, w, wt, c0):
    from metrics.metric_utils import parsing_confusion
    logits, labels = _confusion_case(np.random.default_rng(n * 100 + c), n, c, h, wt)
    want = R.confusion(logits, labels, c0, w)
    assert want.sum() > 0 and (c == 1 or (np.diag(want).sum() < want.sum()))
    d_logits, d_labels = torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()
    got = parsing_confusion(d_logits, d_labels, c0, w)
    assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), want)
    again = parsing_confusion(d_logits, d_labels, c0, w, out=got)                               # accumulates
    assert again is got and np.array_equal(got.cpu().numpy(), 2 * want)


def test_confusion_refuses_more_than_32_classes():
    from metrics.metric_utils import parsing_confusion
    with pytest.raises(RuntimeError, match='33 classes'):
        parsing_confusion(torch.zeros([1, 33, 4, 4], device='cuda'), torch.zeros([1, 1, 4, 4], device='cuda'), 0, 4)
