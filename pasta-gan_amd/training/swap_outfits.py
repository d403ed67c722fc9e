"""The swapped inputs of training's unpaired pass (``--swap_weight``): every person of a training batch dressed in a
batch-mate's garments, prepared on the GPU from the stages the batch builder has just made.

    donors          the donor rule: a deterministic roll inside each group of ``batch_gpu`` consecutive samples
    source_tables   whose upper and whose lower patches every sample wears, by swap region
    swap_tensors    pasta_grid_composite_eroded_u8 twice (upper, lower) and pasta_swap_assemble (csrc/train_grid.hip): the five fp32
                    tensors, by the sample grid's rule (training/snapshot_grid.py) -- the donor's patches warped back with the
                    PERSON's M_inv, every mask eroded 5 x 5
    attach          what both training builders call: the six extra tensors of a batch, by the donor rule or by explicit tables
                    (metrics/tryon_swapped.py takes its donors over the data set, not over the batch)

The warp-back matrices are the float64 ones the builder's normalisation has already solved (``want_matrices`` of
``patch_pipeline.normalize_batch`` / ``normalize_outfit_batch``): the people's 8 x 8 systems are not solved a second time.
A builder with ``geometry='gpu'`` hands over the device ``back_inv`` and flags of ``patch_pipeline.part_geometry`` instead: nothing
is inverted or uploaded here, and the lower garment's parts are gathered on the device.
``retain`` and ``pose`` of the swapped pass are the paired batch's own tensors; no erase mask is applied."""

import ctypes

import numpy as np
import torch

from torch_utils.ops import _native
from training import patch_pipeline

ERODE_RADIUS = 2            # every part, as training/snapshot_grid.py's cells
REGIONS = ('fullbody', 'upperbody', 'lowerbody')
# the five tensors pasta_swap_assemble writes, in its order, and the keep mask of the region L1 term
SWAP_OUTPUTS = ['swap_denorm_upper_input', 'swap_denorm_lower_input', 'swap_denorm_upper_mask', 'swap_denorm_lower_mask', 'swap_style_input']
SWAP_KEYS = SWAP_OUTPUTS + ['swap_keep']
SWAP_STAGES = ('swap_denorm_upper', 'swap_denorm_lower')       # the two uint8 composites [N, H, H, 3], kept with the stages


def donors(n, group):
    """int64 [n]: the donor of every sample of a rank's batch.  The swap group is ``group`` consecutive samples (one accumulation
    round); inside it the donor of sample i is its successor, the last one's the first.  No random numbers: the sampler shuffles."""
    n, b = int(n), int(group)
    if b < 2 or n % b != 0:
        raise ValueError('swapped outfits need groups of at least 2 samples that divide the batch: %d samples, groups of %d' % (n, b))
    i = np.arange(n, dtype=np.int64)
    g = i // b
    return g * b + (i - g * b + 1) % b


def source_tables(n, group, region='fullbody'):
    """(upper_src, lower_src) int64 [n]: whose upper and whose lower patches sample i wears."""
    if region not in REGIONS:
        raise ValueError('swap region %s is invalid.' % region)
    own, donor = np.arange(int(n), dtype=np.int64), donors(n, group)
    return (donor if region != 'lowerbody' else own), (donor if region != 'upperbody' else own)


def _composite(pool, mask_pool, index, minv, valid, ph, pw, H):
    dev = pool.device
    n, parts = index.shape
    index_t = torch.from_numpy(np.ascontiguousarray(index, dtype=np.int32)).to(dev, non_blocking=True)
    if isinstance(minv, torch.Tensor):              # already on the device (geometry='gpu')
        minv_t, valid_t = minv.contiguous(), valid.contiguous()
    else:
        minv_t = torch.from_numpy(np.ascontiguousarray(minv, dtype=np.float64)).to(dev, non_blocking=True)
        valid_t = torch.from_numpy(np.ascontiguousarray(valid).astype(np.uint8)).to(dev, non_blocking=True)
    out = torch.empty([n, H, H, 3], dtype=torch.uint8, device=dev)
    P = _native.ptr
    with torch.cuda.device(dev):
        _native.check(_native.lib().pasta_grid_composite_eroded_u8(P(pool), P(mask_pool), P(index_t), P(minv_t), P(valid_t), P(out), n, parts,
                                                                   int(pool.shape[0]), ph, pw, H, H, ERODE_RADIUS, _native.stream()))
    return out


def swap_tensors(stages, back, valid, lower_parts, upper_src, lower_src, composites=None):
    """The five fp32 tensors of SWAP_OUTPUTS for arbitrary source tables.  ``stages``: the builder's kept stages (``norm_img``,
    ``norm_img_lower`` [N, ph, pw, 3 p], ``norm_clothes_mask*``, ``retain_mask``); ``back`` float64 [N, 10, 3, 3] / ``valid``
    [N, 10]: the people's patch -> image maps as ``patch_pipeline.part_matrices`` returned them; ``lower_parts``: the parts also
    cut from the lower garment (the builder's).  Or ``back`` float64 [N, 10, 9] / ``valid`` uint8 [N, 10] on the device: the INVERTED
    maps and flags of ``patch_pipeline.part_geometry`` (``back_inv``), used as they are.  Three launches.  ``composites``: a dict that receives the two uint8 composites
    [N, H, H, 3] the assemble reads (SWAP_STAGES: the donor's patches on the person, eroded), which are otherwise dropped."""
    norm_img, norm_lower = stages['norm_img'], stages['norm_img_lower']
    dev = norm_img.device
    n, ph, pw = int(norm_img.shape[0]), int(norm_img.shape[1]), int(norm_img.shape[2])
    cu, cl = int(norm_img.shape[3]), int(norm_lower.shape[3])
    pu, pl = cu // 3, cl // 3
    H = int(stages['retain_mask'].shape[1])
    upper_src, lower_src = (np.asarray(t, np.int64).reshape(-1) for t in (upper_src, lower_src))
    lower_parts = np.asarray(lower_parts)
    assert upper_src.shape == (n,) and lower_src.shape == (n,) and len(lower_parts) == pl and back.shape[:2] == (n, 10)
    assert upper_src.min() >= 0 and upper_src.max() < n and lower_src.min() >= 0 and lower_src.max() < n, 'a source outside the batch'

    # the pool of patches [T, ph, pw, 3]: part k of person i at i * pu + k, lower part k at n * pu + i * pl + k (SnapshotGrid's)
    per_part = lambda t, p: t.reshape(n, ph, pw, p, 3).permute(0, 3, 1, 2, 4).reshape(n * p, ph, pw, 3)
    pool = torch.cat([per_part(norm_img, pu), per_part(norm_lower, pl)]).contiguous()
    mask_pool = torch.cat([per_part(stages['norm_clothes_mask'], pu), per_part(stages['norm_clothes_mask_lower'], pl)]).contiguous()
    if isinstance(back, torch.Tensor):
        assert pu == 10 and back.shape == (n, 10, 9) and back.dtype == torch.float64 and valid.shape == (n, 10) and valid.dtype == torch.uint8
        lower_t = torch.from_numpy(lower_parts.astype(np.int64)).to(dev, non_blocking=True)
        inv, inv_l, valid_l = back, back.index_select(1, lower_t), valid.index_select(1, lower_t)
    else:
        inv = patch_pipeline.inverse_maps(back, range(pu)).reshape(n, pu, 9)
        inv_l, valid_l = inv[:, lower_parts], valid[:, lower_parts]
    index_u = upper_src[:, None] * pu + np.arange(pu)
    index_l = n * pu + lower_src[:, None] * pl + np.arange(pl)
    den_u = _composite(pool, mask_pool, index_u, inv, valid, ph, pw, H)
    den_l = _composite(pool, mask_pool, index_l, inv_l, valid_l, ph, pw, H)

    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    t = dict(swap_denorm_upper_input=f32(n, 3, H, H), swap_denorm_lower_input=f32(n, 3, H, H), swap_denorm_upper_mask=f32(n, 1, H, H),
             swap_denorm_lower_mask=f32(n, 1, H, H), swap_style_input=f32(n, cu + cl, ph, pw))
    outs = (ctypes.c_void_p * 5)(*[t[k].data_ptr() for k in SWAP_OUTPUTS])
    up_t = torch.from_numpy(upper_src.astype(np.int32)).to(dev, non_blocking=True)
    low_t = torch.from_numpy(lower_src.astype(np.int32)).to(dev, non_blocking=True)
    norm_img, norm_lower = norm_img.contiguous(), norm_lower.contiguous()
    P = _native.ptr
    with torch.cuda.device(dev):
        _native.check(_native.lib().pasta_swap_assemble(P(den_u), P(den_l), P(norm_img), P(norm_lower), P(up_t), P(low_t), outs, n, n, H, ph, pw,
                                                        cu, cl, _native.stream()))
    if composites is not None:
        composites.update(zip(SWAP_STAGES, (den_u, den_l)))
    return t


def attach(tensors, stages, back, valid, builder, swap, keep_stages=False):
    """``tensors`` with the six SWAP_KEYS added: the five swapped tensors and ``swap_keep``, the ``retain_mask`` stage (uint8
    [N, H, H]).  ``swap`` is dict(region=, group=), the donor rule inside the batch, or dict(upper_src=, lower_src=), explicit
    tables of batch indices [N].  With ``keep_stages`` the two composites join ``stages`` under SWAP_STAGES."""
    n = int(stages['retain_mask'].shape[0])
    if 'upper_src' in swap or 'lower_src' in swap:
        if set(swap) != {'upper_src', 'lower_src'}:
            raise ValueError('swap takes region= and group=, or upper_src= and lower_src=, not %s' % ', '.join(sorted(swap)))
        upper_src, lower_src = (np.asarray(swap[k], np.int64).reshape(-1) for k in ('upper_src', 'lower_src'))
        for name, table in (('upper_src', upper_src), ('lower_src', lower_src)):
            if table.shape != (n,) or table.min() < 0 or table.max() >= n:
                raise ValueError('swap %s %s does not name one of the %d samples of the batch for each of them' % (name, table.tolist(), n))
    else:
        upper_src, lower_src = source_tables(n, swap['group'], swap.get('region', 'fullbody'))
    tensors.update(swap_tensors(stages, back, valid, builder.lower_parts, upper_src, lower_src, composites=stages if keep_stages else None))
    tensors['swap_keep'] = stages['retain_mask']
    return tensors
