"""Timings of the unpaired (swapped-outfit) pass of training on one GPU:

    python tools/bench_region_l1.py [--iters 200] [--step-cost] [--builder]

Device-event times per call, after a warm-up, of the region L1 term's forward (with its reduce launch; value only, and with the
byte maps the backward reads) and of its backward launch, for K = 2 images at [16, 3, 256, 256] and at [8, 3, 512, 512], next to
their memory floor at the HBM rate a float4 copy reaches (6.29 TB/s).  --step-cost also times the Gmain and Dmain phases of
bench.py's configuration (fashion_config, batch 16, 256 x 256, synthetic batch) with and without ``swap_weight=1``, alternating in
one process through the loss object of one TrainingStep; the swapped tensors are the synthetic batch's own, rolled by one.
--builder times the 256 batch builder on the tests' tiny tree (eight people per batch), with and without the swapped preparation."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools'), ROOT]

HBM_RATE = 6.29e12
K = 2


class SwappedSyntheticBatch:
    """A SyntheticFullBodyBatch that also carries the six swapped tensors when ``swapped`` is set: everybody in the next one's
    synthetic garments, the kept parts where the synthetic retain keeps the photograph."""

    def __init__(self, data):
        import torch
        self.data, self.batch, self.swapped = data, data.batch, False
        t = data.tensors
        self.extra = {'swap_' + k: t[k].roll(-1, 0).contiguous() for k in ('style_input', 'denorm_upper_input', 'denorm_lower_input',
                                                                            'denorm_upper_mask', 'denorm_lower_mask')}
        self.extra['swap_keep'] = (t['retain'] == t['real_img']).all(dim=1).to(torch.uint8)

    def split(self, batch_gpu):
        rounds = self.data.split(batch_gpu)
        if self.swapped:
            for i, r in enumerate(rounds):
                r.update({k: v.split(batch_gpu)[i] for k, v in self.extra.items()})
        return rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--step-cost', action='store_true')
    ap.add_argument('--builder', action='store_true')
    ap.add_argument('--steps', type=int, default=6, help='--step-cost: iterations per window (four windows: without, with, without, with)')
    opt = ap.parse_args()

    import ctypes
    import numpy as np
    import torch
    from torch_utils.ops import _native
    from torch_utils.ops.region_l1_loss import region_l1_loss
    device = torch.device('cuda')

    def timed(fn, iters):
        for _ in range(10):
            fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        times = []
        for _ in range(5):
            start.record()
            for _ in range(iters):
                fn()
            end.record()
            end.synchronize()
            times.append(start.elapsed_time(end) / iters * 1e3)
        return float(np.median(times)), min(times), max(times)

    def row(name, fn, nbytes, iters, shape):
        med, lo, hi = timed(fn, iters)
        floor = '' if nbytes is None else '; %.1f MB at %.2f TB/s = %.1f us floor, %.1f x' % (nbytes / 1e6, HBM_RATE / 1e12, nbytes / HBM_RATE * 1e6,
                                                                                             med / (nbytes / HBM_RATE * 1e6))
        print('%-50s %-18s %8.1f us per call (min %.1f, max %.1f over 5 windows of %d)%s' % (name, shape, med, lo, hi, iters, floor))

    for n, res in ((16, 256), (8, 512)):
        shape = '[%d, 3, %d, %d]' % (n, res, res)
        gen = torch.Generator(device='cpu').manual_seed(0)
        u = lambda *s: (torch.rand(s, generator=gen) * 2 - 1).to(device)
        blobs = lambda p: (torch.nn.functional.interpolate(torch.rand([n, 1, res // 16, res // 16], generator=gen), size=(res, res),
                                                           mode='bilinear', align_corners=False) < p).to(device)
        images = [u(n, 3, res, res).requires_grad_(True) for _ in range(K)]
        retain, upper, lower = u(n, 3, res, res), u(n, 3, res, res), u(n, 3, res, res)
        keep, um, lm = blobs(0.5)[:, 0].to(torch.uint8).contiguous(), blobs(0.35).float(), blobs(0.35).float()
        out = region_l1_loss(images, retain, upper, lower, keep, um, lm)
        torch.autograd.grad(out.sum(), images)
        region = torch.where(keep != 0, 0, torch.where(um[:, 0] != 0, 1, torch.where(lm[:, 0] != 0, 2, -1)))
        share = [float((region == r).float().mean()) for r in range(3)]
        print('%s K = %d: regions cover %.2f / %.2f / %.2f of the pixels; out = %s' % (shape, K, *share, [[round(v, 5) for v in r] for r in out.tolist()]))

        # the launches on their own, through the C ABI with preallocated buffers
        lib, P = _native.lib(), _native.ptr
        pointers = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        nbytes = int(lib.pasta_region_l1_loss_workspace(n, res))
        work = torch.empty([nbytes], dtype=torch.uint8, device=device)
        val = torch.empty([K, 3], dtype=torch.float32, device=device)
        maps = torch.empty([K, n, res, res], dtype=torch.uint8, device=device)
        dx = [torch.empty_like(x) for x in images]
        g = torch.ones([K, 3], dtype=torch.float32, device=device)
        xs = [x.detach() for x in images]
        x_ptrs, map_ptrs, dx_ptrs = pointers(xs), pointers(list(maps)), pointers(dx)
        pixels = n * res * res
        # what a launch moves: the keep byte, the two masks, the K images, and the targets of the pixels that have a region (a thread
        # reads a target's 16 bytes when one of its four pixels needs it: counted as the covered share, a lower bound)
        read = pixels * (1 + 8 + 12 * K + 12 * sum(share))

        def forward(with_maps):
            _native.check(lib.pasta_region_l1_loss(x_ptrs, P(retain), P(upper), P(lower), P(keep), P(um), P(lm), P(val), map_ptrs if with_maps else None,
                                                   P(work), nbytes, K, n, res, _native.stream()))

        def backward():
            _native.check(lib.pasta_region_l1_loss_backward(map_ptrs, P(g), dx_ptrs, K, n, res, _native.stream()))

        def op_both():
            return torch.autograd.grad(region_l1_loss(images, retain, upper, lower, keep, um, lm).sum(), images)

        def torch_both():
            in0 = (keep != 0)[:, None]
            in1 = ~in0 & (um != 0)
            in2 = ~in0 & ~in1 & (lm != 0)
            total = sum(((x - t).abs() * w).sum() for x in images for t, w in ((retain, in0), (upper, in1), (lower, in2))) / (3 * pixels)
            return torch.autograd.grad(total, images)

        row('pasta_region_l1_loss, value only (+ reduce)', lambda: forward(False), read, opt.iters, shape)
        row('pasta_region_l1_loss with the byte maps (+ reduce)', lambda: forward(True), read + pixels * K, opt.iters, shape)
        row('pasta_region_l1_loss_backward', backward, pixels * K * (1 + 12), opt.iters, shape)
        print('%-50s %-18s %8.1f us floor (it would move %.1f MB: masks, one region\'s targets, x and dx of K images)' % (
            '  a backward that re-read the inputs instead', shape, pixels * (1 + 8 + 12 * sum(share) + 24 * K) / HBM_RATE * 1e6,
            pixels * (1 + 8 + 12 * sum(share) + 24 * K) / 1e6))
        row('region_l1_loss + autograd.grad (the op, allocating)', op_both, None, opt.iters, shape)
        row('the same values and gradients from stock torch ops', torch_both, None, max(opt.iters // 10, 5), shape)

    if opt.step_cost:
        from training.training_loop_wo_flow_fullbody import SyntheticFullBodyBatch, TrainingStep, fashion_config
        step = TrainingStep(device, cfg=fashion_config(mbstd_group_size=4), num_gpus=1, rank=0, batch_size=16, batch_gpu=16)
        data = SwappedSyntheticBatch(SyntheticFullBodyBatch(16, device, seed=0, res=256))
        phases = [p for p in step.phases if p.name in ('Gmain', 'Dmain')]
        for _ in range(3):
            step.run(data)
        times = {(w, p.name): [] for w in (0, 1) for p in phases}
        for weight in (0, 1, 0, 1):
            step.loss.swap_weight, data.swapped = weight, weight > 0
            step.run(data)      # the first iteration after a change is not timed
            for _ in range(opt.steps):
                for p in phases:
                    p.start_event, p.end_event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                step.run(data)
                for p in phases:
                    p.end_event.synchronize()
                    times[weight, p.name].append(p.start_event.elapsed_time(p.end_event))
            for p in phases:
                p.start_event = p.end_event = None
        for p in phases:
            for weight in (0, 1):
                t = times[weight, p.name]
                print('%s phase, batch 16 at 256 x 256, swap_weight %d: median %.2f ms (min %.2f, max %.2f over %d iterations in two windows)' % (
                    p.name, weight, float(np.median(t)), min(t), max(t), len(t)))
            print('%s: difference of the medians %.2f ms' % (p.name, float(np.median(times[1, p.name])) - float(np.median(times[0, p.name]))))
        print('peak device memory %.2f GB' % (torch.cuda.max_memory_allocated(device) / 2 ** 30))

    if opt.builder:
        from train_grid_tree import make_tree
        from training.dataset import UvitonDatasetFull, collate
        from training.tryon_batch import builder_for
        with tempfile.TemporaryDirectory() as tmp:
            ds = UvitonDatasetFull(make_tree(os.path.join(tmp, 'tree')))
            raw = collate([ds[i] for i in range(8)])
        builder = builder_for(ds, device)
        for name, kwargs in (('without the swapped preparation', {}), ('with it (fullbody, groups of 8)', dict(swap=dict(region='fullbody', group=8)))):
            for _ in range(3):
                builder.build(raw, **kwargs)
            torch.cuda.synchronize()
            times = []
            for _ in range(20):
                t0 = time.perf_counter()
                builder.build(raw, **kwargs)
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            print('FullBodyBatchBuilder.build, 8 people at 256 x 192, %s: median %.2f ms (min %.2f, max %.2f over 20 calls, wall clock with a '
                  'synchronisation)' % (name, float(np.median(times)), min(times), max(times)))


if __name__ == '__main__':
    main()
