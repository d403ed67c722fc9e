"""The swapped inputs of training's unpaired pass (``--swap_weight``): every person of a training batch dressed in a
batch-mate's garments, prepared on the GPU from the stages the batch builder has just made.

    donors          the donor rule: a deterministic roll inside each group of ``batch_gpu`` consecutive samples
    source_tables   whose upper and whose lower patches every sample wears, by swap region
    grid_composites pasta_grid_composite_eroded_u8 twice (upper, lower): the package's one launcher of it, the sample grid's as well
    swap_tensors    grid_composites and pasta_swap_assemble (csrc/train_grid.hip): the five fp32
                    tensors, by the sample grid's rule (training/snapshot_grid.py) -- the donor's patches warped back with the
                    PERSON's M_inv, every mask eroded 5 x 5
    attach          what both training builders call: the six extra tensors of a batch, by the donor rule or by explicit tables
                    (metrics/tryon_swapped.py takes its donors over the data set, not over the batch)

The warp-back maps are the device ``back_inv`` and flags the builder's normalisation already holds (``want_matrices`` of
``patch_pipeline.normalize_batch`` / ``normalize_outfit_batch``, whichever geometry made them): the people are not solved a second
time and nothing is inverted here.
``retain`` and ``pose`` of the swapped pass are the paired batch's own tensors; no erase mask is applied."""

import ctypes

import numpy as np
import torch

from torch_utils.ops import _native
from training import patch_pipeline

ERODE_RADIUS = 2            # cv2.erode(..., np.ones((5, 5))) of every warped-back mask, upper and lower, of the reference's grid
                            # (training_loop_wo_flow_fullbody.py:63, :91, :98)
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


def grid_composites(stages, back, valid, lower_parts, upper_src, lower_src, rows):
    """(upper, lower) uint8 [C, H, H, 3], pasta_grid_composite_eroded_u8 twice: output c wears the upper patches of person
    ``upper_src[c]`` and the lower ones of ``lower_src[c]``, warped back with the maps of person ``rows[c]`` and eroded 5 x 5 -- the
    swapped pass (``rows`` = arange(n)) and the sample grid (training/snapshot_grid.py: repeat(arange(g), g)) alike.  ``stages``: the
    builder's kept stages of the n people; ``back`` / ``valid``: their maps as ``patch_pipeline.composite`` takes them (PartMaps'
    device ``back_inv`` [n, 10, 9] and ``valid`` [n, 10], or the host's, converted here); ``lower_parts``: the parts also cut from
    the lower garment (the builder's)."""
    norm_img, norm_lower = stages['norm_img'], stages['norm_img_lower']
    dev = norm_img.device
    n, ph, pw = int(norm_img.shape[0]), int(norm_img.shape[1]), int(norm_img.shape[2])
    pu, pl = int(norm_img.shape[3]) // 3, int(norm_lower.shape[3]) // 3
    H = int(stages['retain_mask'].shape[1])
    upper_src, lower_src, rows = (np.asarray(t, np.int64).reshape(-1) for t in (upper_src, lower_src, rows))
    assert pu == 10 and len(lower_parts) == pl and 0 <= min(lower_parts) and max(lower_parts) < pu
    assert upper_src.shape == lower_src.shape == rows.shape and all(t.min() >= 0 and t.max() < n for t in (upper_src, lower_src, rows)), 'a source outside the batch'
    back = patch_pipeline.on_device(back, torch.float64, dev, (n, 10, 9), invert=True)
    valid = patch_pipeline.on_device(valid, torch.uint8, dev, (n, 10))

    # the pool of patches [T, ph, pw, 3]: part k of person i at i * pu + k, lower part k at n * pu + i * pl + k
    per_part = lambda t, p: t.reshape(n, ph, pw, p, 3).permute(0, 3, 1, 2, 4).reshape(n * p, ph, pw, 3)
    pool = torch.cat([per_part(norm_img, pu), per_part(norm_lower, pl)]).contiguous()
    mask_pool = torch.cat([per_part(stages['norm_clothes_mask'], pu), per_part(stages['norm_clothes_mask_lower'], pl)]).contiguous()
    upload = lambda table, dtype: torch.from_numpy(np.ascontiguousarray(table, dtype=dtype)).to(dev, non_blocking=True)
    rows_t, lower_t = upload(rows, np.int64), upload(lower_parts, np.int64)
    back, valid = back.index_select(0, rows_t), valid.index_select(0, rows_t)

    def launch(index, minv_t, valid_t):
        index_t = upload(index, np.int32)
        out = torch.empty([len(rows), H, H, 3], dtype=torch.uint8, device=dev)
        P = _native.ptr
        with torch.cuda.device(dev):
            _native.check(_native.lib().pasta_grid_composite_eroded_u8(P(pool), P(mask_pool), P(index_t), P(minv_t), P(valid_t), P(out), len(rows),
                                                                       index.shape[1], int(pool.shape[0]), ph, pw, H, H, ERODE_RADIUS,
                                                                       _native.stream()))
        return out
    return (launch(upper_src[:, None] * pu + np.arange(pu), back, valid),
            launch(n * pu + lower_src[:, None] * pl + np.arange(pl), back.index_select(1, lower_t).contiguous(),
                   valid.index_select(1, lower_t).contiguous()))


def swap_tensors(stages, back, valid, lower_parts, upper_src, lower_src, composites=None):
    """The five fp32 tensors of SWAP_OUTPUTS for arbitrary source tables.  ``stages``: the builder's kept stages (``norm_img``,
    ``norm_img_lower`` [N, ph, pw, 3 p], ``norm_clothes_mask*``, ``retain_mask``); ``back`` / ``valid``: the people's patch -> image
    maps, as grid_composites takes them (the builders hand over the device pair of their normalisation); ``lower_parts``: the parts
    also cut from the lower garment (the builder's).  Three launches.  ``composites``: a dict that receives the two uint8 composites
    [N, H, H, 3] the assemble reads (SWAP_STAGES: the donor's patches on the person, eroded), which are otherwise dropped."""
    norm_img, norm_lower = stages['norm_img'], stages['norm_img_lower']
    dev = norm_img.device
    n, ph, pw = int(norm_img.shape[0]), int(norm_img.shape[1]), int(norm_img.shape[2])
    cu, cl = int(norm_img.shape[3]), int(norm_lower.shape[3])
    H = int(stages['retain_mask'].shape[1])
    upper_src, lower_src = (np.asarray(t, np.int64).reshape(-1) for t in (upper_src, lower_src))
    assert upper_src.shape == (n,) and lower_src.shape == (n,)
    den_u, den_l = grid_composites(stages, back, valid, lower_parts, upper_src, lower_src, np.arange(n))

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
