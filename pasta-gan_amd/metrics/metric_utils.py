"""What every metric is handed (``MetricOptions``, as the reference's metrics/metric_utils.py:25-41 without its detector cache),
a progress printer, and the statistics kernels of csrc/recon_metrics.hip."""

import copy
import time

import torch

import dnnlib
from torch_utils.ops import _native

#----------------------------------------------------------------------------

class MetricOptions:
    def __init__(self, G=None, G_kwargs={}, dataset_kwargs={}, num_gpus=1, rank=0, device=None, progress=None, batch_size=16,
                 data_loader_kwargs=None):
        assert 0 <= rank < num_gpus
        self.G = G
        self.G_kwargs = dnnlib.EasyDict(G_kwargs)
        self.dataset_kwargs = dnnlib.EasyDict(copy.deepcopy(dict(dataset_kwargs)))
        self.num_gpus = num_gpus
        self.rank = rank
        self.device = device if device is not None else torch.device('cuda', rank)
        self.progress = progress.sub() if progress is not None and rank == 0 else ProgressMonitor()
        self.batch_size = batch_size
        self.data_loader_kwargs = dict(data_loader_kwargs if data_loader_kwargs is not None else dict(num_workers=0, pin_memory=True))

#----------------------------------------------------------------------------

class ProgressMonitor:
    """``update(cur_items)`` prints ``tag items n/total`` with the time since the start when ``verbose``; silent otherwise."""

    def __init__(self, tag=None, num_items=None, verbose=False):
        self.tag, self.num_items, self.verbose = tag, num_items, verbose
        self.start_time = time.time()

    def update(self, cur_items):
        if self.verbose and self.tag is not None:
            total = '?' if self.num_items is None else str(self.num_items)
            print(f'{self.tag:<19s} items {cur_items:<7d}/{total:<7s} time {dnnlib.util.format_time(time.time() - self.start_time)}', flush=True)

    def sub(self, tag=None, num_items=None):
        return ProgressMonitor(tag=tag if tag is not None else self.tag, num_items=num_items, verbose=self.verbose)

#----------------------------------------------------------------------------

def recon_image_stats(images, photos, c0):
    """images fp32 [N, 3, H, Wt] against photos uint8 [N, H, W, 3], columns c0 .. c0 + W - 1 (pasta_recon_image_stats):
    (sums int64 [N, 3] = sum |d|, sum d^2, SSIM windows; ssim fp64 [N] = the sum of SSIM over those windows)."""
    _native.require_gpu(images, 'recon_image_stats')
    assert images.dtype == torch.float32 and images.ndim == 4 and images.shape[1] == 3
    assert photos.dtype == torch.uint8 and photos.ndim == 4 and photos.shape[3] == 3 and photos.device == images.device
    images, photos = images.contiguous(), photos.contiguous()
    n, _, h, wt = images.shape
    w = int(photos.shape[2])
    assert tuple(photos.shape[:2]) == (n, h)
    lib = _native.lib()
    nbytes = int(lib.pasta_recon_image_stats_workspace(n, h, w))
    work = torch.empty([max(nbytes, 8)], dtype=torch.uint8, device=images.device)
    sums = torch.empty([n, 3], dtype=torch.int64, device=images.device)
    ssim = torch.empty([n], dtype=torch.float64, device=images.device)
    with torch.cuda.device(images.device):
        _native.check(lib.pasta_recon_image_stats(_native.ptr(images), _native.ptr(photos), _native.ptr(sums), _native.ptr(ssim),
                                                  _native.ptr(work), nbytes, n, h, wt, int(c0), w, _native.stream()))
    return sums, ssim

def region_image_stats(images, ref, mask, c0, r0, m0, W):
    """images fp32 [N, 3, H, Wt] against ref uint8 [N, H, Wr, 3] inside the region mask uint8 [N, H, Wm] != 0, over W columns that
    start at c0, r0 and m0 of the three tensors (pasta_region_image_stats): (sums int64 [N, 4] = sum |d|, sum d^2, SSIM windows
    wholly inside the region, bytes; ssim fp64 [N] = the sum of SSIM over those windows)."""
    _native.require_gpu(images, 'region_image_stats')
    assert images.dtype == torch.float32 and images.ndim == 4 and images.shape[1] == 3
    assert ref.dtype == torch.uint8 and ref.ndim == 4 and ref.shape[3] == 3 and ref.device == images.device
    assert mask.dtype == torch.uint8 and mask.ndim == 3 and mask.device == images.device
    images, ref, mask = images.contiguous(), ref.contiguous(), mask.contiguous()
    n, _, h, wt = images.shape
    assert tuple(ref.shape[:2]) == (n, h) and tuple(mask.shape[:2]) == (n, h)
    w = int(W)
    lib = _native.lib()
    nbytes = int(lib.pasta_region_image_stats_workspace(n, h, w))
    work = torch.empty([max(nbytes, 8)], dtype=torch.uint8, device=images.device)
    sums = torch.empty([n, 4], dtype=torch.int64, device=images.device)
    ssim = torch.empty([n], dtype=torch.float64, device=images.device)
    with torch.cuda.device(images.device):
        _native.check(lib.pasta_region_image_stats(_native.ptr(images), _native.ptr(ref), _native.ptr(mask), _native.ptr(sums),
                                                   _native.ptr(ssim), _native.ptr(work), nbytes, n, h, wt, int(c0), int(ref.shape[2]), int(r0),
                                                   int(mask.shape[2]), int(m0), w, _native.stream()))
    return sums, ssim

def parsing_confusion(logits, labels, c0, width, out=None):
    """logits fp32 [N, C, H, Wt] against labels fp32 [N, 1, H, Wt], columns c0 .. c0 + width - 1 (pasta_parsing_confusion): added
    to ``out`` (int64 [C, C], row = label, column = prediction; a zeroed one when None), which is returned."""
    _native.require_gpu(logits, 'parsing_confusion')
    assert logits.dtype == torch.float32 and logits.ndim == 4 and labels.dtype == torch.float32 and labels.device == logits.device
    logits, labels = logits.contiguous(), labels.contiguous()
    n, c, h, wt = logits.shape
    assert tuple(labels.shape) == (n, 1, h, wt)
    if out is None:
        out = torch.zeros([c, c], dtype=torch.int64, device=logits.device)
    assert out.dtype == torch.int64 and tuple(out.shape) == (c, c) and out.is_contiguous() and out.device == logits.device
    with torch.cuda.device(logits.device):
        _native.check(_native.lib().pasta_parsing_confusion(_native.ptr(logits), _native.ptr(labels), _native.ptr(out), n, c, h, wt, int(c0),
                                                            int(width), _native.stream()))
    return out

#----------------------------------------------------------------------------
