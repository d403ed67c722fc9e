"""The try-on region scores in numpy fp64 (include/pasta_hip.h, pasta_region_image_stats; metrics/tryon_fidelity.py): the
statistics inside a mask with the rule that an SSIM window counts when all its 121 pixels are in the region, the three regions
of a pair, and the figures computed from the partials.  SSIM itself is tests/recon_ref.py's."""
import numpy as np

import recon_ref as R

REGIONS = ('keep', 'upper', 'lower')
KEEP_LABELS = (1, 2, 4, 13, 18, 19)


def windows_inside(mask):
    """mask [H, W] -> bool [H - 10, W - 10]: the valid 11 x 11 positions whose pixels are all in the region."""
    return np.lib.stride_tricks.sliding_window_view(np.asarray(mask) != 0, (R.K, R.K)).all(axis=(2, 3))


def region_stats(gen_u8, ref_u8, mask):
    """uint8 [N, H, W, 3] each and mask [N, H, W] -> (sad, ssd, windows, bytes int64 [N]; ssim_sum fp64 [N])."""
    g, p = np.asarray(gen_u8).astype(np.int64), np.asarray(ref_u8).astype(np.int64)
    m = np.asarray(mask) != 0
    assert g.shape == p.shape and g.shape[3] == 3 and m.shape == g.shape[:3]
    d = (g - p) * m[..., None]
    sad, ssd = np.abs(d).sum(axis=(1, 2, 3)), (d * d).sum(axis=(1, 2, 3))
    windows, ssim = np.zeros([g.shape[0]], np.int64), np.zeros([g.shape[0]])
    for n in range(g.shape[0]):
        inside = windows_inside(m[n])
        windows[n] = 3 * int(inside.sum())
        if windows[n]:
            ssim[n] = sum(R.ssim_map(g[n, :, :, c], p[n, :, :, c])[inside].sum() for c in range(3))
    return sad, ssd, windows, 3 * m.sum(axis=(1, 2)).astype(np.int64), ssim


def keep_mask(palm, parsing):
    """palm [H, H] (padded) and the person's parsing [H, W] -> bool [H, W]: palm, head and shoes."""
    h, w = parsing.shape
    c0 = (h - w) // 2
    return (palm[:, c0:c0 + w] != 0) | np.isin(parsing, KEEP_LABELS)


def pair_regions(photo, parsing, palm, denorm_upper, denorm_lower):
    """One pair's (mask [H, W], reference bytes [H, W, 3]) per region, from the uint8 stages (the denorm stages are padded squares)."""
    h, w = parsing.shape
    c0 = (h - w) // 2
    du, dl = denorm_upper[:, c0:c0 + w], denorm_lower[:, c0:c0 + w]
    return dict(keep=(keep_mask(palm, parsing), photo), upper=(du.astype(np.int64).sum(axis=2) > 0, du),
                lower=(dl.astype(np.int64).sum(axis=2) > 0, dl))


def finish(rows, pixels):
    """rows [pairs, 3, 5] (sad, ssd, windows, bytes, ssim sum; any real dtype) -> the figures of metrics.tryon_fidelity.finish
    without a prefix: ``<region>_<name>``."""
    rows = np.asarray(rows, np.float64)
    out = {}
    for k, region in enumerate(REGIONS):
        sad, ssd, windows, nbytes, ssim = (rows[:, k, j] for j in range(5))
        has, has_w = nbytes > 0, windows > 0
        mse = np.maximum(ssd[has] / nbytes[has], 255.0 ** 2 * 1e-10)
        out[region + '_l1'] = sad.sum() / nbytes.sum() / 255.0 if has.any() else np.nan
        out[region + '_psnr'] = float(np.mean(10 * np.log10(255.0 ** 2 / mse))) if has.any() else np.nan
        out[region + '_ssim'] = float(np.mean(ssim[has_w] / windows[has_w])) if has_w.any() else np.nan
        out[region + '_share'] = nbytes.sum() / (3.0 * pixels * rows.shape[0])
        out[region + '_pairs'], out[region + '_ssim_pairs'] = int(has.sum()), int(has_w.sum())
    return out
