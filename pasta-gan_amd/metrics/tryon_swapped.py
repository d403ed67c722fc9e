"""Unpaired try-on as a registered metric (``tryon_full``, ``tryon2k``): every person of a training-layout tree dressed
in the next person's garments by G_ema, scored by the regions of metrics/tryon_fidelity.py.

The rule.  The M items of the data set in data-set order; item i wears the upper and the lower garment of item (i + 1) % M (the
``fullbody`` swap of training/swap_outfits.py, rolled over the data set and not over a batch: no random numbers, and nothing
depends on the batch size or on the number of ranks).  The items are cut into blocks of ``batch_size`` consecutive items; block k
belongs to rank k % num_gpus.  A block is prepared as one batch of the data set's training builder with explicit source tables
(``build(raw, keep_stages=True, swap=dict(upper_src=, lower_src=))``); the donor of its last item is loaded with it when the block
does not already hold that item, wears its own garments and is never scored.  G runs on the scored rows only.

Per scored row the three regions of tryon_fidelity: ``keep`` is the ``retain_mask`` stage against the photograph, ``upper`` and
``lower`` are where the swapped garment masks G is given are not zero, against the bytes of the two composites those inputs were
made from (stages ``swap_denorm_upper`` / ``swap_denorm_lower``).  Partials are tryon_fidelity's ``int64 [M, 3, 5]``; row i is
written by the rank that scores item i and the ranks add them as integers.  No erase mask is applied (``erase_masks='none'`` is
forced): none of the stages read here depends on it, and a held-out tree needs no mask directory."""

import copy

import torch

import dnnlib
from metrics import tryon_fidelity
from metrics.reconstruction import item_z

#----------------------------------------------------------------------------

def blocks(num_items, batch_size, num_gpus=1, rank=0):
    """This rank's blocks, [(rows, load, upper_src, lower_src)]: ``rows`` the items the block scores, ``load`` the items it loads
    (``rows``, then the donor of the last row when it is not among them) and the two source tables over ``load`` as positions in
    ``load``: row j wears ``load[upper_src[j]]`` = (rows[j] + 1) % M, an extra person its own garments.  Pure: no data set, no GPU."""
    M, B, G, r = int(num_items), int(batch_size), int(num_gpus), int(rank)
    if M < 2:
        raise ValueError('swapped outfits need at least 2 items to take a donor from: %d' % M)
    if B < 1 or G < 1 or not 0 <= r < G:
        raise ValueError('blocks of %d items for rank %d of %d' % (B, r, G))
    out = []
    for k in range(r, (M + B - 1) // B, G):
        rows = list(range(k * B, min((k + 1) * B, M)))
        donor = (rows[-1] + 1) % M
        load = rows if donor in rows else rows + [donor]
        place = {item: j for j, item in enumerate(load)}
        src = [place[(i + 1) % M] for i in rows] + list(range(len(rows), len(load)))
        out.append((rows, load, list(src), list(src)))
    return out

def generator_inputs(batch, count):
    """The keyword tensors G is given for the first ``count`` rows of a batch built with the swap: the swapped garments, the
    person's own ``retain`` and ``pose``."""
    t = batch.tensors
    names = dict(c='swap_style_input', retain='retain', pose='pose', denorm_upper_input='swap_denorm_upper_input',
                 denorm_lower_input='swap_denorm_lower_input', denorm_upper_mask='swap_denorm_upper_mask',
                 denorm_lower_mask='swap_denorm_lower_mask')
    return {k: t[v][:count] for k, v in names.items()}

def prepare_block(builder, raw, block):
    """One loaded block (``raw``: ``collate`` of the items ``block[1]``) -> the prepared batch, stages kept."""
    _, load, upper_src, lower_src = block
    assert int(raw['raw_idx'].shape[0]) == len(load)
    return builder.build(raw, keep_stages=True, swap=dict(upper_src=upper_src, lower_src=lower_src))

def score_block(G, batch, raw_idx, rows, partials):
    """The first ``len(rows)`` people of a prepared block through G and the three statistics launches, into rows ``rows``."""
    n = len(rows)
    photos, st = batch.image[:n], batch.stages
    H, W = int(photos.shape[1]), int(photos.shape[2])
    c0 = (H - W) // 2
    inputs = generator_inputs(batch, n)
    with torch.no_grad():
        out = G(z=item_z(raw_idx[:n], G.z_dim, photos.device), noise_mode='const', **inputs)
    mask = tryon_fidelity.garment_mask
    regions = dict(keep=(st['retain_mask'][:n], c0, photos, 0),
                   upper=(mask(inputs['denorm_upper_mask']), c0, st['swap_denorm_upper'][:n], c0),
                   lower=(mask(inputs['denorm_lower_mask']), c0, st['swap_denorm_lower'][:n], c0))
    tryon_fidelity.score_regions(out[1], regions, c0, W, rows, partials)

def open_set(opts):
    """The data set of ``opts.dataset_kwargs``.  Fewer than two items: an error that names the tree."""
    dataset = dnnlib.util.construct_class_by_name(**opts.dataset_kwargs)
    if len(dataset) < 2:
        raise ValueError('swapped outfits need at least 2 items to take a donor from: %s has %d' % (opts.dataset_kwargs.get('path'), len(dataset)))
    return dataset

def compute_partials(opts):
    """This rank's blocks scored into device partials, combined over the ranks by one all_reduce -> (int64 [M, 3, 5] on the host,
    the content pixels H * W of an item)."""
    from training import dataset as dataset_module
    from training.tryon_batch import builder_for
    dataset = open_set(opts)
    num_items = len(dataset)
    mine = blocks(num_items, opts.batch_size, opts.num_gpus, opts.rank)
    G = copy.deepcopy(opts.G).eval().requires_grad_(False).to(opts.device)
    # a copy is rebuilt from the recorded constructor arguments: a storage switched at run time (calc_metrics.py --storage) is handed on
    from training.networks import activation_storage, set_activation_storage
    if activation_storage(G) != activation_storage(opts.G):
        set_activation_storage(G, activation_storage(opts.G))
    builder = builder_for(dataset, opts.device)
    loader = torch.utils.data.DataLoader(dataset, batch_sampler=[load for _, load, _, _ in mine], collate_fn=dataset_module.collate,
                                         **opts.data_loader_kwargs)
    partials = tryon_fidelity.new_partials(num_items, opts.device)       # a rank without a block still takes part in the exchange
    progress = opts.progress.sub(tag='swapped try-on', num_items=sum(len(rows) for rows, _, _, _ in mine))
    done = 0
    for block, raw in zip(mine, loader):
        batch = prepare_block(builder, raw, block)
        score_block(G, batch, raw['raw_idx'].tolist(), block[0], partials)
        done += len(block[0])
        progress.update(done)
    if opts.num_gpus > 1:
        torch.distributed.all_reduce(partials)
    return partials.cpu(), int(dataset.resolution) * int(dataset.content_width)

def finish(partials, prefix, pixels):
    """Combined partials -> the eighteen results of ``tryon_fidelity.finish``.  Every person has kept parts (a head, or the tree is
    broken) and the ``keep`` region's bytes do not depend on G, so an item whose ``keep`` bytes are 0 was not scored: an error,
    as in ``reconstruction.finish``.  A garment region nobody has is NaN figures and share 0, not an error."""
    keep_bytes = partials[:, tryon_fidelity.REGIONS.index('keep'), 3]
    if partials.shape[0] == 0 or not bool((keep_bytes > 0).all()):
        raise ValueError('swapped try-on metric: %d of %d items were not scored (no kept pixels)' % (int((keep_bytes <= 0).sum()), partials.shape[0]))
    return tryon_fidelity.finish(partials, prefix, pixels=pixels)

def compute(opts, prefix):
    partials, pixels = compute_partials(opts)
    return finish(partials, prefix, pixels)

#----------------------------------------------------------------------------
