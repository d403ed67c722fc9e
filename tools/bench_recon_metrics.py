"""Timings of the reconstruction metric's kernels and of the try-on region statistics on one GPU (sections 8c and 8d):

    python tools/bench_recon_metrics.py --prepare DIR [--people 256]     # a tree of --people persons and DIR/snapshot.pkl
    python tools/bench_recon_metrics.py [--batch 16] [--iters 200]       # the kernels, a stock-torch yardstick, G_ema's forward

--prepare writes what a kernel trace of the command needs:
    rocprofv3 --kernel-trace --stats -d OUT -- python pasta-gan_amd/calc_metrics.py --network DIR/snapshot.pkl --verbose false
Without it: device-event times per call at 256 x 192 in 256 after a warm-up, for pasta_recon_image_stats, pasta_parsing_confusion,
the same image statistics from stock torch ops (quantisation, five stacked maps through conv2d with the 11 x 11 Gaussian, the
SSIM formula, the sums) in the same process on the same batch, and the full-width G_ema's forward pass; next to each kernel
its memory floor at the HBM rate a float4 copy reaches (6.29 TB/s).  A loop over one batch keeps its 15 MB in the caches, so the
image kernel is also timed on inputs that rotate through 360 MB."""
import argparse
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tools'), ROOT]

HBM_RATE = 6.29e12


def prepare(root, people):
    import dnnlib
    from bench_train_grid import make_tree
    from training.training_loop_wo_flow_fullbody import fashion_config
    tree = make_tree(os.path.join(root, 'tree'), people)
    G = dnnlib.util.construct_class_by_name(**fashion_config().G_kwargs).eval().requires_grad_(False)
    D = dnnlib.util.construct_class_by_name(**fashion_config().D_kwargs).eval().requires_grad_(False)
    with open(os.path.join(root, 'snapshot.pkl'), 'wb') as f:
        pickle.dump(dict(G=G, D=D, G_ema=G, training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree)), f)
    print('wrote', os.path.join(root, 'snapshot.pkl'), 'and a tree of', people, 'people')


def torch_image_stats(images, photos, c0, window, mask=None):
    """pasta_recon_image_stats from stock torch ops: (sums [N, 2], ssim sums [N]); with ``mask`` (uint8 [N, H, W])
    pasta_region_image_stats: the differences of the region's pixels, SSIM over the windows wholly inside it (a min-pool)."""
    import torch
    n, h, w, _ = photos.shape
    v = (images[..., c0:c0 + w] + 1.0) * 127.5
    x = torch.where(v != v, torch.zeros_like(v), v.clamp(0, 255)).floor()
    y = photos.permute(0, 3, 1, 2).to(torch.float32)
    d = x - y
    if mask is not None:
        m = (mask != 0).to(torch.float32).unsqueeze(1)
        d = d * m
        inside = -torch.nn.functional.max_pool2d(-m, 11, stride=1)
    sums = torch.stack([d.abs().sum(dim=(1, 2, 3), dtype=torch.float64), (d * d).sum(dim=(1, 2, 3), dtype=torch.float64)], dim=1)
    a, b = x - 127.5, y - 127.5
    maps = torch.stack([a, b, a * a, b * b, a * b], dim=1).reshape(n * 15, 1, h, w)
    e = torch.nn.functional.conv2d(maps, window).reshape(n, 5, 3, h - 10, w - 10)
    mx, my = e[:, 0] + 127.5, e[:, 1] + 127.5
    sxx, syy, sxy = e[:, 2] - e[:, 0] * e[:, 0], e[:, 3] - e[:, 1] * e[:, 1], e[:, 4] - e[:, 0] * e[:, 1]
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ssim = (2 * mx * my + c1) * (2 * sxy + c2) / ((mx * mx + my * my + c1) * (sxx + syy + c2))
    if mask is not None:
        ssim = ssim * inside
    return sums, ssim.sum(dim=(1, 2, 3), dtype=torch.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--prepare', metavar='DIR')
    ap.add_argument('--people', type=int, default=256)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=200)
    opt = ap.parse_args()
    if opt.prepare:
        os.makedirs(opt.prepare, exist_ok=True)
        return prepare(opt.prepare, opt.people)

    import numpy as np
    import torch
    import dnnlib
    from metrics import metric_utils
    from training.training_loop_wo_flow_fullbody import SyntheticFullBodyBatch, fashion_config
    device = torch.device('cuda')
    n, H, W, c0 = opt.batch, 256, 192, 32
    gen = torch.Generator(device='cpu').manual_seed(0)
    photos = torch.randint(0, 256, [n, H // 4, W // 4, 3], generator=gen, dtype=torch.uint8).repeat_interleave(4, 1).repeat_interleave(4, 2)
    images = photos.permute(0, 3, 1, 2).float() / 127.5 - 1 + 0.05 * torch.randn([n, 3, H, W], generator=gen)
    images = torch.nn.functional.pad(images, [c0, H - W - c0], value=1.0).contiguous().to(device)
    photos = photos.contiguous().to(device)
    logits = torch.randn([n, 6, H, H], generator=gen).to(device)
    labels = torch.randint(0, 6, [n, 1, H, H], generator=gen).float().to(device)
    g = np.exp(-0.5 * (np.arange(11) - 5.0) ** 2 / 1.5 ** 2)
    window = torch.from_numpy(np.outer(g, g) / np.outer(g, g).sum()).float().reshape(1, 1, 11, 11).to(device)
    conf = torch.zeros([6, 6], dtype=torch.int64, device=device)

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

    hip_sums, hip_ssim = metric_utils.recon_image_stats(images, photos, c0)
    ref_sums, ref_ssim = torch_image_stats(images, photos, c0, window)
    assert torch.equal(hip_sums[:, :2].double(), ref_sums), 'the yardstick computes other sums'
    print('largest |mean SSIM (HIP) - mean SSIM (torch, fp32)|: %.3e' % float(((hip_ssim - ref_ssim) / hip_sums[:, 2]).abs().max()))

    # the region kernel on a blocky mask (8 x 8 blocks, three in four inside), against the same torch ops with a mask
    mask = (torch.rand([n, H // 8, W // 8], generator=gen) < 0.75).to(torch.uint8).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous().to(device)
    reg_sums, reg_ssim = metric_utils.region_image_stats(images, photos, mask, c0, 0, 0, W)
    ref_sums, ref_ssim_m = torch_image_stats(images, photos, c0, window, mask)
    assert torch.equal(reg_sums[:, :2].double(), ref_sums) and int(reg_sums[:, 2].min()) > 0, 'the masked yardstick computes other sums'
    print('the same under a mask (%.0f %% of the windows count): %.3e' % (100.0 * float(reg_sums[:, 2].sum()) / float(hip_sums[:, 2].sum()),
          float(((reg_ssim - ref_ssim_m) / reg_sums[:, 2]).abs().max())))

    # the same call on inputs that cannot stay in the 256 MiB Infinity Cache: 24 copies (360 MB) taken in turn
    copies = [(images.clone(), photos.clone()) for _ in range(24)]
    turn = [0]

    def rotating():
        a, b = copies[turn[0] % len(copies)]
        turn[0] += 1
        return metric_utils.recon_image_stats(a, b, c0)

    rows = [('pasta_recon_image_stats (+ its reduce launch)', lambda: metric_utils.recon_image_stats(images, photos, c0),
             images.numel() * 4 + photos.numel()),
            ('  the same, inputs rotating through 360 MB', rotating, images.numel() * 4 + photos.numel()),
            ('the same statistics from stock torch ops', lambda: torch_image_stats(images, photos, c0, window), None),
            ('pasta_region_image_stats (+ its reduce launch)', lambda: metric_utils.region_image_stats(images, photos, mask, c0, 0, 0, W),
             images.numel() * 4 + photos.numel() + mask.numel()),
            ('the region statistics from stock torch ops', lambda: torch_image_stats(images, photos, c0, window, mask), None),
            ('pasta_parsing_confusion', lambda: metric_utils.parsing_confusion(logits, labels, c0, W, out=conf), (logits.numel() + labels.numel()) * 4)]
    for name, fn, nbytes in rows:
        med, lo, hi = timed(fn, opt.iters)
        floor = '' if nbytes is None else '; %.1f MB at %.2f TB/s = %.1f us floor, %.1f x' % (nbytes / 1e6, HBM_RATE / 1e12, nbytes / HBM_RATE * 1e6,
                                                                                             med / (nbytes / HBM_RATE * 1e6))
        print('%-48s batch %d: %8.1f us per call (min %.1f, max %.1f over 5 windows of %d)%s' % (name, n, med, lo, hi, opt.iters, floor))

    G = dnnlib.util.construct_class_by_name(**fashion_config().G_kwargs).eval().requires_grad_(False).to(device)
    t = SyntheticFullBodyBatch(n, device).tensors
    z = torch.zeros([n, G.z_dim], device=device)

    def forward():
        with torch.no_grad():
            G(z=z, c=t['style_input'], retain=t['retain'], pose=t['pose'], denorm_upper_input=t['denorm_upper_input'],
              denorm_lower_input=t['denorm_lower_input'], denorm_upper_mask=t['denorm_upper_mask'], denorm_lower_mask=t['denorm_lower_mask'],
              noise_mode='const')
    med, lo, hi = timed(forward, max(opt.iters // 10, 5))
    print('%-48s batch %d: %8.1f us per call (min %.1f, max %.1f)' % ('G_ema forward (full width, 256 x 256)', n, med, lo, hi))


if __name__ == '__main__':
    main()
