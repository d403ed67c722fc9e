"""The try-on region scores without a GPU: partials -> figures on CPU tensors (metrics/tryon_fidelity.py) against the numpy
restatement (tests/tryon_fidelity_ref.py), the restatement's window rule, and the metric registry left as it was."""
import numpy as np
import pytest
import torch

import tryon_fidelity_ref as F

PIXELS = 256 * 192


def _partials(num_pairs, rng):
    from metrics import tryon_fidelity as M
    p = M.new_partials(num_pairs)
    for k in range(3):
        pixels = torch.from_numpy(rng.integers(200, 20000, num_pairs))
        windows = 3 * torch.from_numpy(rng.integers(1, 150, num_pairs))
        p[:, k, 0] = torch.from_numpy(rng.integers(0, 255 * 600, num_pairs))
        p[:, k, 1] = torch.from_numpy(rng.integers(0, 255 * 255 * 600, num_pairs))
        p[:, k, 2] = windows
        p[:, k, 3] = 3 * pixels
        p[:, k, 4] = (torch.from_numpy(rng.uniform(-0.2, 1.0, num_pairs)) * windows).view(torch.int64)
    p[2, 0, 1] = 0                                  # a pair at the PSNR cap
    p[4, 1] = 0                                     # a pair without an upper garment
    p[5, 1, 2] = 0                                  # a pair whose upper garment holds no window
    p[5, 1, 4] = 0
    p[:, 2] = 0                                     # no pair has a lower garment
    return p


def _as_rows(p):
    rows = p.numpy().astype(np.float64)
    rows[:, :, 4] = p[:, :, 4].contiguous().numpy().view(np.float64)
    return rows


def _same(a, b):
    return a.keys() == b.keys() and all((a[k] == b[k]) or (a[k] != a[k] and b[k] != b[k]) for k in a)


@pytest.mark.parametrize('ways', [1, 2, 3])
def test_results_do_not_depend_on_how_the_partials_are_split(ways):
    from metrics import tryon_fidelity as M
    whole = _partials(11, np.random.default_rng(5))
    want = M.finish(whole, 'tryon')
    parts = []
    for r in range(ways):
        p = M.new_partials(11)
        p[r::ways] = whole[r::ways]
        parts.append(p)
    combined = M.combine_partials(parts)
    assert torch.equal(combined, whole) and _same(M.finish(combined, 'tryon'), want)        # bit for bit
    assert torch.equal(whole, _partials(11, np.random.default_rng(5)))                        # inputs untouched
    assert sorted(want) == sorted('tryon_%s_%s' % (r, k) for r in M.REGIONS for k in M.FIGURES + M.COUNTS) and len(want) == 18


def test_figures_against_the_oracle_formulas_and_an_absent_region():
    from metrics import tryon_fidelity as M
    p = _partials(9, np.random.default_rng(9))
    got, want = M.finish(p, 'x'), F.finish(_as_rows(p), PIXELS)
    for k, v in want.items():
        if np.isnan(v):
            assert np.isnan(got['x_' + k]), k
        else:
            assert got['x_' + k] == pytest.approx(v, rel=1e-13), k
    assert got['x_keep_pairs'] == got['x_keep_ssim_pairs'] == 9 and got['x_upper_pairs'] == 8 and got['x_upper_ssim_pairs'] == 7
    assert all(np.isfinite(got['x_%s_%s' % (r, k)]) for r in ('keep', 'upper') for k in M.FIGURES)
    # the region no pair has: NaN figures, no pairs, no share -- and no error
    assert all(np.isnan(got['x_lower_' + k]) for k in ('l1', 'psnr', 'ssim'))
    assert got['x_lower_pairs'] == 0 and got['x_lower_ssim_pairs'] == 0 and got['x_lower_share'] == 0
    assert got['x_keep_share'] == pytest.approx(int(p[:, 0, 3].sum()) / (3 * PIXELS * 9), rel=1e-15)
    assert M.finish(p, 'x', pixels=2 * PIXELS)['x_keep_share'] == pytest.approx(got['x_keep_share'] / 2, rel=1e-15)


def test_figures_by_hand_and_the_psnr_cap():
    from metrics import tryon_fidelity as M
    from metrics.reconstruction import PSNR_CAP_DB
    # pair 0: 100 region pixels, every byte off by 2 -> MSE 4; pair 1: 50 identical pixels -> MSE floored: the cap
    p = M.new_partials(3)
    ssim = torch.tensor([15.0, 6.0], dtype=torch.float64)
    p[:2, 0, 0] = torch.tensor([600, 0])
    p[:2, 0, 1] = torch.tensor([1200, 0])
    p[:2, 0, 2] = torch.tensor([30, 6])
    p[:2, 0, 3] = torch.tensor([300, 150])
    p[:2, 0, 4] = ssim.view(torch.int64)
    r = M.finish(p, 'm', pixels=1000)
    assert r['m_keep_psnr'] == pytest.approx((10 * np.log10(255.0 ** 2 / 4.0) + PSNR_CAP_DB) / 2, rel=1e-13)
    assert r['m_keep_l1'] == pytest.approx(600 / 450 / 255, rel=1e-15)
    assert r['m_keep_ssim'] == pytest.approx((0.5 + 1.0) / 2, rel=1e-15)
    assert r['m_keep_share'] == pytest.approx(450 / (3 * 1000 * 3), rel=1e-15)
    assert r['m_keep_pairs'] == 2 and r['m_keep_ssim_pairs'] == 2
    p[0, 0, 1] = 0                                   # both at the cap: the mean is the cap, not infinity
    assert M.finish(p, 'm', pixels=1000)['m_keep_psnr'] == pytest.approx(PSNR_CAP_DB, rel=1e-13)


def test_window_rule_of_the_oracle():
    block = np.zeros([33, 43], np.uint8)
    block[22:33, 32:43] = 1
    inside = F.windows_inside(block)
    assert inside.shape == (23, 33) and inside.sum() == 1 and inside[22, 32]
    hole = block.copy()
    hole[26, 39] = 0
    assert F.windows_inside(hole).sum() == 0
    rng = np.random.default_rng(0)
    gen, ref = (rng.integers(0, 256, [1, 33, 43, 3], dtype=np.uint8) for _ in range(2))
    sad, ssd, windows, nbytes, ssim = F.region_stats(gen, ref, block[None])
    assert windows.tolist() == [3] and nbytes.tolist() == [3 * 121]
    d = gen[0, 22:, 32:].astype(np.int64) - ref[0, 22:, 32:]
    assert sad[0] == np.abs(d).sum() and ssd[0] == (d * d).sum()
    holed = F.region_stats(gen, ref, hole[None])
    assert holed[2].tolist() == [0] and holed[3].tolist() == [3 * 120] and holed[4].tolist() == [0.0]
    # a mask of ones is tests/recon_ref.py's image_stats
    import recon_ref as R
    full = F.region_stats(gen, ref, np.ones([1, 33, 43], np.uint8))
    sad0, ssd0, ssim0, windows0 = R.image_stats(gen, ref)
    assert (full[0], full[1], full[2]) == (sad0, ssd0, windows0) and full[4][0] == pytest.approx(ssim0[0], rel=1e-13)
    assert F.region_stats(gen, ref, np.zeros([1, 33, 43], np.uint8))[3].tolist() == [0]


def test_keep_mask_of_the_oracle():
    parsing = np.arange(20, dtype=np.uint8).reshape(4, 5).repeat(3, 0)[:, :5]         # [12, 5]: padded square 12 x 12, c0 = 3
    palm = np.zeros([12, 12], np.uint8)
    palm[0, 3] = 1                                  # content column 0
    palm[0, 2] = 1                                  # in the padding: not a content pixel
    m = F.keep_mask(palm, parsing)
    want = np.isin(parsing, [1, 2, 4, 13, 18, 19])
    want[0, 0] = True
    assert m.shape == (12, 5) and np.array_equal(m, want)


def test_registry_untouched():
    from metrics import metric_main
    import metrics.tryon_fidelity  # noqa: F401
    assert metric_main.list_valid_metrics() == ['recon_full', 'recon2k']
    assert not metric_main.is_valid_metric('tryon_fidelity') and not metric_main.is_valid_metric('tryon')
