"""Timings of the kept-parts paste on one GPU:

    python tools/bench_keep_composite.py [--iters 200] [--radius 2] [--out FILE]

Per size -- (16, 256, 192) in 256 columns, test.py's batch, and (8, 512, 320) in 512 columns, test_512.py's -- in one process,
device-event times per call after a warm-up, the median of five windows, on a blocky mask (8 x 8 blocks, three in four kept):

    images_keep_to_u8                       the fused entry (pasta_images_keep_to_u8): quantise, crop and paste in one launch
    images_to_u8                            the conversion alone (pasta_images_to_u8), what a run without --kept-parts photo launches
    images_to_u8 + the paste from torch ops the same bytes from stock torch ops after the conversion: a box sum of the mask padded
                                            with ones through avg_pool2d, then the integer blend

The two composites are compared byte for byte before anything is timed.  Next to each kernel its memory floor at the HBM rate a
float4 copy reaches (6.29 TB/s); a loop over one batch keeps its bytes in the caches, so the fused entry is also timed on inputs
that rotate through more than the 256 MiB Infinity Cache."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), ROOT]

HBM_RATE = 6.29e12


def torch_keep_composite(images, c0, width, photo, keep, radius):
    """images_keep_to_u8 from stock torch ops after images_to_u8 (include/pasta_hip.h states the rule)."""
    import torch
    from training.tryon_pairs import images_to_u8
    g = images_to_u8(images, c0, width).to(torch.int32)
    k = (keep != 0)
    K = (2 * radius + 1) ** 2
    if radius > 0:
        padded = torch.nn.functional.pad(k.to(torch.float32).unsqueeze(1), [radius] * 4, value=1.0)
        s = torch.nn.functional.avg_pool2d(padded, 2 * radius + 1, stride=1, divisor_override=1).squeeze(1).round().to(torch.int32)
    else:
        s = torch.ones_like(k, dtype=torch.int32)
    a = torch.where(k, s, torch.zeros_like(s)).unsqueeze(3)
    return torch.div(g * (K - a) + photo.to(torch.int32) * a + K // 2, K, rounding_mode='floor').to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--radius', type=int, default=2)
    ap.add_argument('--out', metavar='FILE', help='also write the lines to FILE')
    opt = ap.parse_args()

    import numpy as np
    import torch
    from training.tryon_pairs import images_keep_to_u8, images_to_u8
    device = torch.device('cuda')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

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

    say('%s, torch %s, radius %d, %d calls per window' % (torch.cuda.get_device_name(0), torch.__version__, opt.radius, opt.iters))
    for n, H, W in ((16, 256, 192), (8, 512, 320)):
        c0, r = (H - W) // 2, opt.radius
        gen = torch.Generator(device='cpu').manual_seed(0)
        photo = torch.randint(0, 256, [n, H // 4, W // 4, 3], generator=gen, dtype=torch.uint8).repeat_interleave(4, 1).repeat_interleave(4, 2)
        images = photo.permute(0, 3, 1, 2).float() / 127.5 - 1 + 0.05 * torch.randn([n, 3, H, W], generator=gen)
        images = torch.nn.functional.pad(images, [c0, H - W - c0], value=1.0).contiguous().to(device)
        photo = photo.contiguous().to(device)
        keep = (torch.rand([n, H // 8, W // 8], generator=gen) < 0.75).to(torch.uint8).repeat_interleave(8, 1).repeat_interleave(8, 2).contiguous().to(device)

        fused, stock = images_keep_to_u8(images, c0, W, photo, keep, r), torch_keep_composite(images, c0, W, photo, keep, r)
        assert torch.equal(fused, stock), 'the yardstick pastes other bytes'
        plain = images_to_u8(images, c0, W)
        say('(%d, %d, %d) in %d columns: the two composites agree; %.1f %% of the bytes differ from the plain conversion'
            % (n, H, W, H, 100.0 * float((fused != plain).float().mean())))

        need = 256 * 2 ** 20 * 1.4 / (images.numel() * 4 + photo.numel() + keep.numel())      # past the 256 MiB Infinity Cache
        copies = [(images.clone(), photo.clone(), keep.clone()) for _ in range(int(need) + 1)]
        turn = [0]

        def rotating():
            a, b, c = copies[turn[0] % len(copies)]
            turn[0] += 1
            return images_keep_to_u8(a, c0, W, b, c, r)

        read = n * 3 * H * W * 4                                    # the content columns of the three planes
        rows = [('images_keep_to_u8', lambda: images_keep_to_u8(images, c0, W, photo, keep, r), read + 7 * n * H * W),
                ('  the same, inputs rotating through %d MB' % (len(copies) * (images.numel() * 4 + photo.numel() + keep.numel()) // 10 ** 6),
                 rotating, read + 7 * n * H * W),
                ('images_to_u8', lambda: images_to_u8(images, c0, W), read + 3 * n * H * W),
                ('images_to_u8 + the paste from torch ops', lambda: torch_keep_composite(images, c0, W, photo, keep, r), None)]
        for name, fn, nbytes in rows:
            med, lo, hi = timed(fn, opt.iters)
            floor = '' if nbytes is None else '; %.1f MB at %.2f TB/s = %.1f us floor, %.1f x' % (nbytes / 1e6, HBM_RATE / 1e12, nbytes / HBM_RATE * 1e6,
                                                                                                 med / (nbytes / HBM_RATE * 1e6))
            say('  %-46s %8.1f us per call (min %.1f, max %.1f over 5 windows)%s' % (name, med, lo, hi, floor))
        del copies
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
