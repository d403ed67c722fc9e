"""Unpaired try-on scored by region: what PASTA-GAN's design tells the generator to reproduce, measured on the bytes test.py writes.

Three regions of every output have a known answer, so they need no detector network:

    keep     head, palms and shoes -- the pixels ``retain`` carries (``pasta_tryon_outfit_masks_u8``'s mask: palm != 0 or the
             person's label in KEEP_LABELS) -- against the person's photograph;
    upper    where the donor's upper-garment patches were warped onto the person (``denorm_upper_mask``) against those
             warped patches (stage ``denorm_upper``);
    lower    the same for the lower garment (``denorm_lower_mask``, stage ``denorm_lower``).

Per region and pair, ``pasta_region_image_stats`` (csrc/recon_metrics.hip) gives sum |d|, sum d^2 and the bytes of the region's
pixels, and the SSIM sum and count of the 11 x 11 windows lying wholly inside it.  These are this project's own figures, not
the reference's (which scores try-on by FID and KID).  They are an option of test.py and test_512.py (``finish`` with
``pixels=512 * 320``), which score the pairs of a test tree's lists, and the registered metrics ``tryon_full`` and ``tryon2k``
(metrics/tryon_swapped.py), which score a training-layout tree with every person in the next person's garments and share
``score_regions``, ``new_partials`` and ``finish`` with the option.

Partials are ``int64 [num_pairs, 3, 5]``: per region sum |d|, sum d^2, SSIM windows, bytes and the bits of the fp64 SSIM sum.
Row i belongs to pair i of the pair lists and is written by whoever scores it (zeros elsewhere), the scheme of
metrics/reconstruction.py: adding partials as integers only ever adds zeros to a row, the fp64 word included."""

import math

import torch

from metrics.reconstruction import PSNR_CAP_DB, item_z

REGIONS = ('keep', 'upper', 'lower')
WORDS = 5                               # sum |d|, sum d^2, SSIM windows, bytes, bits of the fp64 SSIM sum
KEEP_LABELS = (1, 2, 4, 13, 18, 19)     # head (1, 2, 4, 13) and shoes (18, 19)
FIGURES = ('l1', 'psnr', 'ssim', 'share')
COUNTS = ('pairs', 'ssim_pairs')
PIXELS = 256 * 192                      # content pixels of a pair of the test set (UPT_subset*_256_192)

#----------------------------------------------------------------------------

def new_partials(num_pairs, device='cpu'):
    return torch.zeros([num_pairs, len(REGIONS), WORDS], dtype=torch.int64, device=device)

def combine_partials(parts):
    """Several scorers' partials -> one: integer sums (exact for the fp64 word too, see the module docstring)."""
    parts = list(parts)
    out = parts[0].clone()
    for p in parts[1:]:
        out += p
    return out

def pair_z(pair_index, z_dim, device):
    """z of every pair from its own index in the pair lists (``np.random.RandomState(pair_index)``, as reconstruction.item_z)."""
    return item_z(pair_index, z_dim, device)

def finish(partials, prefix, pixels=PIXELS):
    """Combined partials -> per region r ``<prefix>_<r>_l1`` (pooled), ``_psnr`` (mean over the pairs that have the region, the
    MSE floored as PSNR_CAP_DB says), ``_ssim`` (mean over the pairs with a window of the pair's mean SSIM), ``_share`` (of the
    ``pixels`` content pixels of a pair), ``_pairs`` and ``_ssim_pairs``; in fp64 on the host.  A region no pair has gives NaN
    figures (share 0), not an error."""
    p = partials.to('cpu', torch.int64)
    assert p.ndim == 3 and tuple(p.shape[1:]) == (len(REGIONS), WORDS)
    pairs = int(p.shape[0])
    nan = float('nan')
    out = {}
    for k, region in enumerate(REGIONS):
        sad, ssd, windows, nbytes = (p[:, k, j] for j in range(4))
        ssim_sum = p[:, k, 4].contiguous().view(torch.float64)
        has, has_w = nbytes > 0, windows > 0
        total = int(nbytes.sum())
        mse = (ssd[has].double() / nbytes[has].double()).clamp(min=255.0 ** 2 * 10.0 ** (-PSNR_CAP_DB / 10.0))
        r = dict(l1=int(sad.sum()) / total / 255.0 if total > 0 else nan,
                 psnr=float((10.0 * torch.log10(255.0 ** 2 / mse)).mean()) if total > 0 else nan,
                 ssim=float((ssim_sum[has_w] / windows[has_w].double()).mean()) if bool(has_w.any()) else nan,
                 share=total / (3.0 * pixels * pairs) if pairs > 0 else nan,
                 pairs=int(has.sum()), ssim_pairs=int(has_w.sum()))
        for name, v in r.items():
            out['%s_%s_%s' % (prefix, region, name)] = v
    return out

#----------------------------------------------------------------------------

def keep_mask(stages):
    """uint8 [N, H, W]: the content columns of the mask ``pasta_tryon_outfit_masks_u8`` multiplies ``retain_img`` with."""
    parsing, palm = stages['parsing'], stages['palm']
    H, W = int(parsing.shape[1]), int(parsing.shape[2])
    c0 = (H - W) // 2
    m = palm[:, :, c0:c0 + W] != 0
    for label in KEEP_LABELS:
        m = m | (parsing == label)
    return m.to(torch.uint8)

def score_batch(images, batch, rows, partials):
    """G's fine-tuned output fp32 [N, 3, H, H] (before images_to_u8; the kernel quantises as that does) of a ``TryOnPairBatch``, or
    of a 512 x 320 ``TryOnRegionBatch`` or ``TryOnOutfitBatch``, built with ``keep_stages=True``, scored into rows ``rows`` of
    ``partials``.  It reads the stages every one of them keeps: the person's unpadded ``image`` and ``parsing``, ``palm``,
    ``denorm_upper`` and ``denorm_lower``; the retain rule (``keep_mask``) is the same at both sizes."""
    st, t = batch.stages, batch.tensors
    assert st is not None, 'tryon_fidelity.score_batch: build the batch with keep_stages=True'
    photos = st['image']
    H, W = int(photos.shape[1]), int(photos.shape[2])
    c0 = (H - W) // 2
    score_regions(images, dict(keep=(keep_mask(st), 0, photos, 0),
                               upper=(garment_mask(t['denorm_upper_mask']), c0, st['denorm_upper'], c0),
                               lower=(garment_mask(t['denorm_lower_mask']), c0, st['denorm_lower'], c0)), c0, W, rows, partials)

def garment_mask(mask):
    """fp32 [N, 1, H, H], a ``denorm_*_mask`` input of G -> uint8 [N, H, H]: where it is not zero."""
    return (mask[:, 0] != 0).to(torch.uint8)

def score_regions(images, regions, c0, W, rows, partials):
    """images [N, 3, H, Wt], content columns c0 .. c0 + W - 1, scored per region of REGIONS into rows ``rows`` of ``partials``.
    ``regions[name]`` = (mask uint8 [N, H, Wm], the mask's first content column, reference uint8 [N, H, Wr, 3], the reference's
    first content column).  One ``pasta_region_image_stats`` launch per region; shared with metrics/tryon_swapped.py."""
    from metrics import metric_utils
    images = images.to(torch.float32)
    words = []
    for region in REGIONS:
        mask, m0, ref, r0 = regions[region]
        sums, ssim = metric_utils.region_image_stats(images, ref, mask, c0, r0, m0, W)
        words.append(torch.cat([sums, ssim.view(torch.int64).unsqueeze(1)], dim=1))
    rows = torch.as_tensor(rows, dtype=torch.int64, device=partials.device)
    partials[rows] = torch.stack(words, dim=1).to(partials.device)

#----------------------------------------------------------------------------
