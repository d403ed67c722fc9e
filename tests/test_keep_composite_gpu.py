"""pasta_images_keep_to_u8 (training.tryon_pairs.images_keep_to_u8) against the numpy restatement tests/keep_composite_ref.py,
byte for byte: both kernels (four pixels per thread where the widths allow it, one otherwise), every radius that takes another
path, masks that put the window on tile borders and image borders."""

import numpy as np
import pytest
import torch

import keep_composite_ref as KC

pytestmark = pytest.mark.gpu

# (N, H, W, Wt, c0).  The first two take the one-pixel kernel (16 x 16 tiles), the last two the four-pixel kernel (64 x 16 tiles):
# W = 40 leaves its only tile ragged in both directions, 256 x 192 is the test set's size.
SHAPES = [(3, 19, 17, 19, 1), (2, 45, 35, 50, 7), (2, 21, 40, 48, 4), (1, 256, 192, 256, 32)]
RADII = (0, 1, 2, 8)


def _generated(rng, n, h, wt):
    x = rng.uniform(-1.2, 1.2, size=[n, 3, h, wt]).astype(np.float32)
    flat = x.reshape(-1)
    k = np.arange(256)
    cand = (k / 127.5 - 1).astype(np.float32)
    exact = cand[(cand + np.float32(1)) * np.float32(127.5) == k.astype(np.float32)]     # (x + 1) * 127.5 is an integer in fp32
    assert len(exact) >= 10
    planted = np.concatenate([np.float32([-1, 1, np.nan, -1.2, 1.2, 0]), exact])
    flat[rng.choice(flat.size, size=len(planted), replace=False)] = planted
    return x


def _masks(rng, n, h, w):
    """name -> uint8 [n, h, w]; non-zero values other than 1 are kept as 1 is."""
    z = lambda: np.zeros([n, h, w], np.uint8)
    masks = dict(zeros=z(), ones=np.full([n, h, w], 255, np.uint8))
    m = z(); m[:, h // 2, w // 2] = 1; masks['interior pixel'] = m
    m = z(); m[:, 0, 0] = 1; m[:, h - 1, w - 1] = 3; masks['corner pixels'] = m
    m = z(); m[:, :h // 2, :w // 2] = 1; masks['block at the top left'] = m
    m = z(); m[:, 11:20, 11:20] = 1; m[:, 27:36, 27:36] = 1; m[:, 11:20, 59:68] = 1; masks['9 x 9 blocks across 15/16, 31/32 and 63/64'] = m
    masks['random 0.9'] = (rng.rand(n, h, w) < 0.9).astype(np.uint8) * rng.choice(np.uint8([1, 2, 255]), size=[n, h, w])
    m = np.stack([(rng.rand(h, w) < d).astype(np.uint8) for d in np.linspace(0.5, 0.97, n)]); m[0, :, : w // 3] = 1
    masks['one mask per image'] = m
    return masks


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def case(request):
    n, h, w, wt, c0 = request.param
    rng = np.random.RandomState(n * 1000 + h)
    x = _generated(rng, n, h, wt)
    photo = rng.randint(0, 256, size=[n, h, w, 3]).astype(np.uint8)
    return dict(shape=request.param, x=x, photo=photo, masks=_masks(rng, n, h, w), g=KC.images_to_u8(x, c0, w),
                x_gpu=torch.from_numpy(x).cuda(), photo_gpu=torch.from_numpy(photo).cuda())


@pytest.mark.parametrize('radius', RADII)
def test_entry_equals_the_restatement(case, radius):
    from training.tryon_pairs import images_keep_to_u8, images_to_u8
    n, h, w, wt, c0 = case['shape']
    plain = images_to_u8(case['x_gpu'], c0, w)
    assert np.array_equal(plain.cpu().numpy(), case['g'])            # the restated quantiser is the entry's, NaN and exact integers included
    K = (2 * radius + 1) ** 2
    for name, mask in case['masks'].items():
        keep = torch.from_numpy(mask).cuda()
        got = images_keep_to_u8(case['x_gpu'], c0, w, case['photo_gpu'], keep, radius)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w, 3)
        want = KC.composite(case['g'], case['photo'], mask, radius)
        bad = np.argwhere(got.cpu().numpy() != want)
        assert len(bad) == 0, (name, radius, len(bad), bad[:5].tolist())
        # without the restatement
        if name == 'zeros':
            assert torch.equal(got, plain)
        if name == 'ones':
            assert torch.equal(got, case['photo_gpu'])
        full = torch.from_numpy(KC.weight(mask, radius) == K).cuda()
        assert torch.equal(got[full], case['photo_gpu'][full]), name
        assert torch.equal(got[keep == 0], plain[keep == 0]), name
    w_all = [KC.weight(m, radius) for m in case['masks'].values()]
    assert any((a == K).any() for a in w_all) and (radius == 0 or any(((a > 0) & (a < K)).any() for a in w_all))


def test_a_tensor_that_is_not_aligned_takes_the_narrow_kernel():
    """The four-pixel kernel needs 16-byte rows of ``images``; a view that starts 4 bytes into its storage is made contiguous by
    the front-end and so keeps it, but the entry itself, handed such a pointer, must fall back: the same bytes either way."""
    from torch_utils.ops import _native
    rng = np.random.RandomState(5)
    n, h, w, wt, c0, r = 2, 18, 24, 32, 4, 2
    x = _generated(rng, n, h, wt)
    photo = rng.randint(0, 256, size=[n, h, w, 3]).astype(np.uint8)
    mask = (rng.rand(n, h, w) < 0.8).astype(np.uint8)
    want = KC.composite(KC.images_to_u8(x, c0, w), photo, mask, r)
    store = torch.zeros([x.size + 1], dtype=torch.float32, device='cuda')
    store[1:] = torch.from_numpy(x).cuda().reshape(-1)
    shifted = store[1:].view(n, 3, h, wt)
    assert shifted.data_ptr() % 16 == 4
    out = torch.empty([n, h, w, 3], dtype=torch.uint8, device='cuda')
    P = _native.ptr
    photo_gpu, keep_gpu = torch.from_numpy(photo).cuda(), torch.from_numpy(mask).cuda()      # named: a pointer does not keep a tensor alive
    _native.check(_native.lib().pasta_images_keep_to_u8(P(shifted), P(photo_gpu), P(keep_gpu), P(out), n, h, wt, c0, w, r, _native.stream()))
    assert np.array_equal(out.cpu().numpy(), want)


def test_refusals():
    from torch_utils.ops import _native
    from training.tryon_pairs import images_keep_to_u8
    x = torch.zeros([2, 3, 8, 12], device='cuda')
    photo = torch.zeros([2, 8, 8, 3], dtype=torch.uint8, device='cuda')
    keep = torch.zeros([2, 8, 8], dtype=torch.uint8, device='cuda')
    assert images_keep_to_u8(x, 2, 8, photo, keep, 8).shape == (2, 8, 8, 3)
    for args, words in (((x, 2, 8, photo, keep, 9), 'radius'), ((x, 2, 8, photo, keep, -1), 'radius'), ((x, 2, 8, photo, keep, 1.0), 'radius'),
                        ((x.cpu(), 2, 8, photo, keep, 2), 'GPU'), ((x, 2, 8, photo.cpu(), keep, 2), 'GPU'), ((x, 2, 8, photo, keep.cpu(), 2), 'GPU'),
                        ((x, 2, 8, photo[:, :7], keep, 2), 'photo'), ((x, 2, 8, photo[:1], keep, 2), 'photo'),
                        ((x, 2, 8, photo, keep[:, :, :7], 2), 'keep'), ((x, 5, 8, photo, keep, 2), 'columns'), ((x, -1, 8, photo, keep, 2), 'columns'),
                        ((x.double(), 2, 8, photo, keep, 2), 'fp32'), ((x, 2, 8, photo.float(), keep, 2), 'uint8'),
                        ((x, 2, 8, photo, keep.bool(), 2), 'uint8'), ((x[:, :2], 2, 8, photo, keep, 2), r'\[N, 3, H, Wt\]')):
        with pytest.raises(ValueError, match=words):
            images_keep_to_u8(*args)
    # the entry's own refusals, before any launch
    lib, P = _native.lib(), _native.ptr
    out = torch.empty_like(photo)
    for args, words in (((P(x), P(photo), P(keep), P(out), 2, 8, 12, 2, 8, 9), b'radius 9'),
                        ((P(x), P(photo), P(keep), P(out), 2, 8, 12, 5, 8, 2), b'columns 5 + 8 of 12'),
                        ((P(x), P(photo), P(keep), P(out), 0, 8, 12, 2, 8, 2), b'bad shape'),
                        ((P(x), P(None), P(keep), P(out), 2, 8, 12, 2, 8, 2), b'null pointer')):
        assert lib.pasta_images_keep_to_u8(*args, _native.stream()) != 0
        assert words in lib.pasta_last_error() and b'images_keep_to_u8' in lib.pasta_last_error()
