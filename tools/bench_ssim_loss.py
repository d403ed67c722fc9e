"""Timings of the SSIM loss's launches on one GPU:

    python tools/bench_ssim_loss.py [--iters 200] [--step-cost]

Device-event times per call, after a warm-up, of the forward (value and derivative maps, with its reduce launch), of the
value-only forward and of the backward launch at [16, 3, 256, 256] with the crop 32 + 192 and at [8, 3, 512, 512] with the crop
96 + 320; in the same process, on the same inputs, the same loss and gradient composed from stock torch ops (conv2d with the
11 x 11 Gaussian over five stacked maps, the formula, autograd) -- a yardstick that lives in this tool only.  Next to each
launch its memory floor at the HBM rate a float4 copy reaches (6.29 TB/s).  --step-cost also times the Gmain phase of bench.py's
configuration (fashion_config, batch 16, 256 x 256, synthetic batch) with and without the term, alternating in one process
through the loss object of one TrainingStep."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools'), ROOT]

HBM_RATE = 6.29e12
C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2


def torch_ssim_loss(x, y, c0, width, window):
    """The loss from stock torch ops, differentiable by autograd."""
    import torch
    n, _, h, _ = x.shape
    a, b = x[..., c0:c0 + width], y[..., c0:c0 + width]
    maps = torch.stack([a, b, a * a, b * b, a * b], dim=1).reshape(n * 15, 1, h, width)
    e = torch.nn.functional.conv2d(maps, window).reshape(n, 5, 3, h - 10, width - 10)
    mx, my = e[:, 0] + 1, e[:, 1] + 1
    sxx, syy, sxy = e[:, 2] - e[:, 0] * e[:, 0], e[:, 3] - e[:, 1] * e[:, 1], e[:, 4] - e[:, 0] * e[:, 1]
    return 1 - ((2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--step-cost', action='store_true')
    ap.add_argument('--steps', type=int, default=6, help='--step-cost: iterations per window (four windows: without, with, without, with)')
    opt = ap.parse_args()

    import numpy as np
    import torch
    from torch_utils.ops import _native
    from torch_utils.ops.ssim_loss import ssim_loss
    device = torch.device('cuda')
    g = np.exp(-0.5 * (np.arange(11) - 5.0) ** 2 / 1.5 ** 2)
    window = torch.from_numpy(np.outer(g, g) / np.outer(g, g).sum()).float().reshape(1, 1, 11, 11).to(device)

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
        print('%-44s %-18s %8.1f us per call (min %.1f, max %.1f over 5 windows of %d)%s' % (name, shape, med, lo, hi, iters, floor))

    for n, res, c0, width in ((16, 256, 32, 192), (8, 512, 96, 320)):
        shape = '[%d, 3, %d, %d]' % (n, res, res)
        gen = torch.Generator(device='cpu').manual_seed(0)
        y = (torch.rand([n, 3, res // 4, res // 4], generator=gen) * 2 - 1).repeat_interleave(4, 2).repeat_interleave(4, 3)
        x = (y + 0.05 * torch.randn([n, 3, res, res], generator=gen)).to(device).requires_grad_(True)
        y = y.contiguous().to(device)
        y[..., :c0] = 1.0
        y[..., c0 + width:] = 1.0

        loss = ssim_loss(x, y, c0, width)
        (grad,) = torch.autograd.grad(loss, x)
        ref = torch_ssim_loss(x, y, c0, width, window)
        (ref_grad,) = torch.autograd.grad(ref, x)
        print('%s crop %d + %d: loss %.6f; |loss (HIP) - loss (torch, fp32)| %.3e; largest gradient difference %.3e of %.3e' % (
            shape, c0, width, float(loss.detach()), abs(float(loss.detach()) - float(ref.detach())), float((grad - ref_grad).abs().max()), float(ref_grad.abs().max())))

        # the three launches on their own, through the C ABI with preallocated buffers
        lib = _native.lib()
        nbytes = int(lib.pasta_ssim_loss_workspace(n, res, width))
        work = torch.empty([nbytes], dtype=torch.uint8, device=device)
        out = torch.empty([], dtype=torch.float32, device=device)
        dmaps = torch.empty([n, 3, 3, res - 10, width - 10], dtype=torch.float32, device=device)
        dx = torch.empty_like(x)
        one = torch.ones([], dtype=torch.float32, device=device)
        xd = x.detach()
        content = n * 3 * res * width * 4

        def forward(maps):
            _native.check(lib.pasta_ssim_loss(_native.ptr(xd), _native.ptr(y), _native.ptr(out), _native.ptr(maps), _native.ptr(work), nbytes, n, res,
                                              res, c0, width, _native.stream()))

        def backward():
            _native.check(lib.pasta_ssim_loss_backward(_native.ptr(xd), _native.ptr(y), _native.ptr(dmaps), _native.ptr(one), _native.ptr(dx), n, res,
                                                       res, c0, width, _native.stream()))

        def op_both():
            (g,) = torch.autograd.grad(ssim_loss(x, y, c0, width), x)
            return g

        def torch_both():
            (g,) = torch.autograd.grad(torch_ssim_loss(x, y, c0, width, window), x)
            return g

        row('pasta_ssim_loss, value only (+ reduce)', lambda: forward(None), 2 * content, opt.iters, shape)
        row('pasta_ssim_loss with the maps (+ reduce)', lambda: forward(dmaps), 2 * content + dmaps.numel() * 4, opt.iters, shape)
        row('pasta_ssim_loss_backward', backward, 2 * content + dmaps.numel() * 4 + dx.numel() * 4, opt.iters, shape)
        row('ssim_loss + autograd.grad (the op, allocating)', op_both, None, opt.iters, shape)
        row('the same loss and gradient from stock torch ops', torch_both, None, max(opt.iters // 10, 5), shape)

    if opt.step_cost:
        from training.training_loop_wo_flow_fullbody import SyntheticFullBodyBatch, TrainingStep, fashion_config
        step = TrainingStep(device, cfg=fashion_config(mbstd_group_size=4), num_gpus=1, rank=0, batch_size=16, batch_gpu=16)
        data = SyntheticFullBodyBatch(16, device, seed=0, res=256)
        (gmain,) = [p for p in step.phases if p.name == 'Gmain']
        for _ in range(3):
            step.run(data)
        times = {0: [], 5: []}
        for weight in (0, 5, 0, 5):
            step.loss.ssim_weight, step.loss.ssim_width = weight, 192
            step.run(data)      # the first iteration after a change is not timed
            for _ in range(opt.steps):
                gmain.start_event, gmain.end_event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                step.run(data)
                gmain.end_event.synchronize()
                times[weight].append(gmain.start_event.elapsed_time(gmain.end_event))
            gmain.start_event = gmain.end_event = None
        for weight in (0, 5):
            t = times[weight]
            print('Gmain phase, batch 16 at 256 x 256, ssim_weight %d: median %.2f ms (min %.2f, max %.2f over %d iterations in two windows)' % (
                weight, float(np.median(t)), min(t), max(t), len(t)))
        print('difference of the medians: %.0f us' % ((float(np.median(times[5])) - float(np.median(times[0]))) * 1e3))


if __name__ == '__main__':
    main()
