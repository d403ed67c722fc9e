"""The three restated primitives of tests/tryon_ref.py (cv2.line with thickness 2, pycocotools' rleFrPoly, cv2.resize INTER_LINEAR
on uint8) on cases whose answer does not depend on a rasteriser's tie-breaking, and the host geometry of training/tryon_batch.py."""
import numpy as np

import tryon_ref as R


def test_thick_line_axis_aligned_and_45_degrees():
    img = np.zeros([20, 30, 3], np.uint8)
    R.thick_line(img, (5, 10), (15, 10), (1, 2, 3))
    want = np.zeros([20, 30], bool)
    want[9:12, 5:16] = True                        # three rows over the segment ...
    want[10, 4] = want[10, 16] = True              # ... and the round caps
    assert np.array_equal(img[..., 0] > 0, want) and (img[want] == (1, 2, 3)).all()
    img = np.zeros([20, 20, 3], np.uint8)
    R.thick_line(img, (3, 3), (10, 10), (9, 9, 9))
    ys, xs = np.mgrid[0:20, 0:20]
    band = (abs(xs - ys) <= 1) & (xs + ys >= 6) & (xs + ys <= 20)
    band |= ((xs - 3) ** 2 + (ys - 3) ** 2 <= 1) | ((xs - 10) ** 2 + (ys - 10) ** 2 <= 1)
    assert np.array_equal(img[..., 0] > 0, band)
    img = np.zeros([9, 9, 3], np.uint8)
    R.thick_line(img, (4, 4), (4, 4), (5, 5, 5))   # a point: the plus-shaped cap
    assert (img[..., 0] > 0).sum() == 5


def test_rle_fill_of_integer_rectangles():
    for x0, y0, x1, y1 in [(3, 4, 20, 9), (0, 0, 7, 7), (-5, 10, 12, 40), (250, 250, 300, 300)]:
        m = R.rle_fr_poly([x0, y0, x0, y1, x1, y1, x1, y0], 32 if y1 < 32 else 256, 32 if x1 < 32 else 256)
        want = np.zeros_like(m)
        want[max(y0, 0):y1, max(x0, 0):x1] = 1      # pixels [x0, x1) x [y0, y1)
        assert np.array_equal(m, want), (x0, y0, x1, y1)
    assert not R.rle_fr_poly([5.0, 5.0] * 4, 16, 16).any()        # coincident corners: empty


def test_resize_integer_factors():
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, [64, 48], dtype=np.uint8)
    assert np.array_equal(R.resize_linear_u8(src, 64, 48), src)                     # identity
    big = rng.integers(0, 256, [128, 96], dtype=np.uint8)
    quad = big.astype(np.int64).reshape(64, 2, 48, 2).sum((1, 3))
    assert np.array_equal(R.resize_linear_u8(big, 64, 48), ((quad + 2) >> 2).astype(np.uint8))    # 2x down = 2 x 2 mean, rounded
    assert (R.resize_linear_u8(np.full([17, 5], 93, np.uint8), 256, 256) == 93).all()
    up = R.resize_linear_u8(src, 128, 96)         # 2x up: odd outputs weigh their two nearest sources 3 : 1 per axis
    s = src.astype(np.int64)
    want = ((9 * s[:-1, :-1] + 3 * s[1:, :-1] + 3 * s[:-1, 1:] + s[1:, 1:]) + 8) >> 4
    assert np.array_equal(up[1:-1:2, 1:-1:2], want.astype(np.uint8))
    assert np.array_equal(up[0, 0], src[0, 0]) and np.array_equal(up[-1, -1], src[-1, -1])


def test_dilation_anchor():
    m = np.zeros([40, 40], np.uint8)
    m[20, 20] = 1
    d16 = R.dilate(m, 16)
    assert np.array_equal(np.argwhere(d16)[[0, -1]], [[13, 13], [28, 28]])       # window offsets -8 .. +7: a point spreads 7 up / left, 8 down / right
    d25 = R.dilate(m, 25)
    assert np.array_equal(np.argwhere(d25)[[0, -1]], [[8, 8], [32, 32]])


def test_host_geometry_matches_the_restatement():
    from training import tryon_batch as TB
    kp = np.zeros([1, 18, 3])
    kp[0, :, 0] = np.arange(18) * 7.9 - 3.2
    kp[0, :, 1] = np.arange(18) * 11.6 + 0.7
    kp[0, :, 2] = 0.5
    kp[0, 3, 2] = 0.05
    limbs, joints = TB.stick_tables(kp)
    assert limbs.shape == (1, 19, 5) and joints.shape == (1, 18, 3)
    assert joints[0, 0].tolist() == [-3, 0, 1] and joints[0, 3, 2] == 0
    assert limbs[0, 2].tolist() == [int(kp[0, 2, 0]), int(kp[0, 2, 1]), int(kp[0, 3, 0]), int(kp[0, 3, 1]), 0]
    quads, present = TB.palm_quads(kp, 32)
    assert present[0].tolist() == [1, 1, 0, 0]          # right elbow missing
    a, b, c, d = kp[0, 5, 0] + 32, kp[0, 5, 1], kp[0, 6, 0] + 32, kp[0, 6, 1]
    m = R.rle_fr_poly([float(v) for v in quads[0, 0].reshape(-1)], 256, 256)
    assert np.array_equal(m * 255.0, R.get_rectangle_mask(a, b, c, d, 256, 256))
