"""Paired reconstruction: G_ema re-dresses every person of a data set in patches of their own garments -- the task the loss's L1
and parsing terms train -- and its fine-tuned image and predicted parsing are scored against the person's photograph and label
map: L1, PSNR and SSIM over the bytes test.py would write, mIoU and pixel accuracy over the parsing classes.

Per batch: the data set's training builder (training/tryon_batch.py ``builder_for``), G in eval mode with ``noise_mode='const'`` and z drawn per item from
``np.random.RandomState(raw_idx)``, then the two statistics kernels of csrc/recon_metrics.hip.  Nothing but the statistics is
kept: five 8-byte words per item and the confusion matrix.

The partial sums of a rank are ``dict(items=int64 [num_items, 5], confusion=int64 [C, C])``.  Row i of ``items`` belongs to item i
of the data set and is written by the one rank that scores it (zeros elsewhere): sum |d|, sum d^2, SSIM windows, bytes, and the
bits of the fp64 SSIM sum.  Adding the ranks' tensors as integers therefore only ever adds zeros to a row, the fp64 word
included: the combined partials, and with them every result, do not depend on the number of GPUs or on the batch size."""

import copy

import numpy as np
import torch

import dnnlib

ITEM_WORDS = 5      # sum |d|, sum d^2, SSIM windows, bytes, bits of the fp64 SSIM sum
PSNR_CAP_DB = 100.0
NUM_CLASSES = 6     # the parsing head's classes (networks.py: SynthesisNetworkFull)

#----------------------------------------------------------------------------

def new_partials(num_items, num_classes, device='cpu'):
    return dict(items=torch.zeros([num_items, ITEM_WORDS], dtype=torch.int64, device=device),
                confusion=torch.zeros([num_classes, num_classes], dtype=torch.int64, device=device))

def combine_partials(parts):
    """The ranks' partials -> one: integer sums (see the module docstring for why that is exact for the fp64 word too)."""
    parts = list(parts)
    out = {k: parts[0][k].clone() for k in ('items', 'confusion')}
    for p in parts[1:]:
        for k in out:
            out[k] += p[k]
    return out

def confusion_scores(confusion):
    """(mIoU over the classes whose union is not empty, pixel accuracy) of an int64 [C, C] matrix, row = label, column = prediction;
    NaN where nothing was counted."""
    m = confusion.to('cpu', torch.int64)
    hit = m.diagonal()
    union = m.sum(dim=1) + m.sum(dim=0) - hit
    seen = union > 0
    miou = float((hit[seen].double() / union[seen].double()).mean()) if bool(seen.any()) else float('nan')
    total = int(m.sum())
    return miou, (int(hit.sum()) / total if total > 0 else float('nan'))

def finish(partials, prefix):
    """Combined partials (CPU or device tensors) -> the metric's results, in fp64 on the host."""
    items = partials['items'].to('cpu', torch.int64)
    sad, ssd, windows, nbytes = (items[:, k] for k in range(4))
    ssim_sum = items[:, 4].contiguous().view(torch.float64)
    if items.shape[0] == 0 or not bool((nbytes > 0).all()):
        raise ValueError('reconstruction metric: %d of %d items were not scored' % (int((nbytes <= 0).sum()), items.shape[0]))
    l1 = int(sad.sum()) / int(nbytes.sum()) / 255.0
    mse = (ssd.double() / nbytes.double()).clamp(min=255.0 ** 2 * 10.0 ** (-PSNR_CAP_DB / 10.0))
    psnr = float((10.0 * torch.log10(255.0 ** 2 / mse)).mean())
    ssim = float((ssim_sum / windows.double()).mean())
    miou, pixacc = confusion_scores(partials['confusion'])
    return {prefix + '_l1': l1, prefix + '_psnr': psnr, prefix + '_ssim': ssim, prefix + '_miou': miou, prefix + '_pixacc': pixacc}

#----------------------------------------------------------------------------

def item_z(raw_idx, z_dim, device):
    """z of every item from its own index in the tree: no dependence on the batch size or on which rank scores it."""
    z = np.stack([np.random.RandomState(int(i)).randn(z_dim) for i in raw_idx]).astype(np.float32)
    return torch.from_numpy(z).to(device)

def score_batch(G, batch, raw_idx, rows, partials):
    """One prepared batch (``FullBodyBatch``) through G and the two kernels, into rows ``rows`` of ``partials``."""
    from metrics import metric_utils
    t, photos = batch.tensors, batch.image
    n, H, W = int(photos.shape[0]), int(photos.shape[1]), int(photos.shape[2])
    c0 = (H - W) // 2
    with torch.no_grad():
        out = G(z=item_z(raw_idx, G.z_dim, photos.device), c=t['style_input'], retain=t['retain'], pose=t['pose'],
                denorm_upper_input=t['denorm_upper_input'], denorm_lower_input=t['denorm_lower_input'],
                denorm_upper_mask=t['denorm_upper_mask'], denorm_lower_mask=t['denorm_lower_mask'], noise_mode='const')
    assert out[2].shape[1] == partials['confusion'].shape[0]
    sums, ssim = metric_utils.recon_image_stats(out[1].to(torch.float32), photos, c0)
    metric_utils.parsing_confusion(out[2].to(torch.float32), t['gt_parsing'], c0, W, out=partials['confusion'])
    rows = torch.as_tensor(rows, dtype=torch.int64, device=photos.device)
    nbytes = torch.full([n, 1], H * W * 3, dtype=torch.int64, device=photos.device)
    partials['items'][rows] = torch.cat([sums, nbytes, ssim.view(torch.int64).unsqueeze(1)], dim=1)

def compute_partials(opts):
    """This rank's items -- (i * num_gpus + rank) % num_items as the reference's metrics take theirs, without the repeats of the
    wrap-around, so that each item is scored once -- scored into device partials, combined over the ranks by one all_reduce."""
    from training import dataset as dataset_module
    from training.tryon_batch import attach_strokes, builder_for
    dataset = dnnlib.util.construct_class_by_name(**opts.dataset_kwargs)
    num_items = len(dataset)
    rounds = (num_items - 1) // opts.num_gpus + 1
    subset = [i * opts.num_gpus + opts.rank for i in range(rounds) if i * opts.num_gpus + opts.rank < num_items]
    G = copy.deepcopy(opts.G).eval().requires_grad_(False).to(opts.device)
    # a copy is rebuilt from the recorded constructor arguments: a storage switched at run time (calc_metrics.py --storage) is handed on
    from training.networks import activation_storage, set_activation_storage
    if activation_storage(G) != activation_storage(opts.G):
        set_activation_storage(G, activation_storage(opts.G))
    builder = builder_for(dataset, opts.device)
    loader = torch.utils.data.DataLoader(dataset, sampler=subset, batch_size=opts.batch_size, collate_fn=dataset_module.collate,
                                         **opts.data_loader_kwargs)
    partials = new_partials(num_items, NUM_CLASSES, opts.device)      # a rank without items still takes part in the exchange
    progress = opts.progress.sub(tag='reconstruction', num_items=len(subset))
    done = 0
    for raw in loader:
        if getattr(dataset, 'erase_masks', 'files') == 'strokes':       # drawn by the person, not by a visit: scores stay comparable
            attach_strokes(raw, dataset.erase_strokes, 0, raw['raw_idx'].numpy())
        batch = builder.build(raw)
        score_batch(G, batch, raw['raw_idx'].tolist(), subset[done:done + batch.batch], partials)
        done += batch.batch
        progress.update(done)
    cut = partials['items'].numel()
    flat = torch.cat([partials['items'].flatten(), partials['confusion'].flatten()])
    if opts.num_gpus > 1:
        torch.distributed.all_reduce(flat)
    flat = flat.cpu()
    return dict(items=flat[:cut].reshape(num_items, ITEM_WORDS), confusion=flat[cut:].reshape(NUM_CLASSES, NUM_CLASSES))

def compute(opts, prefix):
    return finish(compute_partials(opts), prefix)

#----------------------------------------------------------------------------
