"""Timings of the paste mask on one GPU:

    python tools/bench_paste_mask.py [--iters 200] [--out FILE]

Per size -- (16, 256, 192) in 256 columns, test.py's batch, and (8, 512, 320) in 512 columns, test_512.py's -- and per kind of
heads (the six parsing logits of GeneratorFull, the two sigmoid planes of GeneratorV18), in one process, device-event times per
call after a warm-up, the median of five windows, with the rule table of all three options and the palm mask:

    photo_paste_mask             the entry (pasta_photo_paste_mask_u8): labels, palm, rule row and heads in one launch
    the mask from torch ops      the same mask from stock torch ops: argmax or two comparisons, a gather in the rule table, a
                                 shift, the palm term

The two masks are compared byte for byte before anything is timed.  Next to the entry its memory floor at the HBM rate a float4
copy reaches (6.29 TB/s); a loop over one batch keeps its bytes in the caches."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), ROOT]

HBM_RATE = 6.29e12


def torch_paste_mask(parsing, palm, rule, heads, c0):
    """photo_paste_mask from stock torch ops (include/pasta_hip.h states the rule)."""
    import torch
    n, h, w = parsing.shape
    crop = lambda x: x[:, :, :h, c0:c0 + w]
    if len(heads) == 1:
        s = torch.tensor([0, 1, 2, 3, 3, 3], device=parsing.device)[torch.argmax(crop(heads[0]), dim=1)]
    elif len(heads) == 2:
        u, l = (crop(x)[:, 0] for x in heads)
        s = torch.where(u > 0.5, 1, torch.where(l > 0.5, 2, 0))
    else:
        s = torch.zeros([n, h, w], dtype=torch.int64, device=parsing.device)
    allowed = torch.gather(rule.to(torch.int64), 1, parsing.reshape(n, h * w).to(torch.int64)).reshape(n, h, w)
    m = ((allowed >> s) & 1) != 0
    if palm is not None:
        m = m | (palm[:, :, c0:c0 + w] != 0)
    return m.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--out', metavar='FILE', help='also write the lines to FILE')
    opt = ap.parse_args()

    import numpy as np
    import torch
    from training.tryon_pairs import paste_rules, photo_paste_mask
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

    say('%s, torch %s, %d calls per window' % (torch.cuda.get_device_name(0), torch.__version__, opt.iters))
    for n, H, W in ((16, 256, 192), (8, 512, 320)):
        c0 = (H - W) // 2
        gen = torch.Generator(device='cpu').manual_seed(0)
        blocky = lambda t: t.repeat_interleave(8, -2).repeat_interleave(8, -1).contiguous()
        parsing = blocky(torch.randint(0, 20, [n, H // 8, W // 8], generator=gen, dtype=torch.uint8)).to(device)
        palm = blocky((torch.rand([n, H // 8, H // 8], generator=gen) < 0.05).to(torch.uint8)).to(device)
        own = torch.arange(n)
        rule = paste_rules(True, True, True, own, torch.where(own % 2 == 0, own, (own + 1) % n), torch.where(own % 3 == 0, own, (own + 1) % n), H).to(device)
        logits = (blocky(torch.randn([n, 6, H // 8, H // 8], generator=gen)) + 0.1 * torch.randn([n, 6, H, H], generator=gen)).to(device)
        sigmoids = tuple(torch.sigmoid(blocky(torch.randn([n, 1, H // 8, H // 8], generator=gen)) + 0.1 * torch.randn([n, 1, H, H], generator=gen)).to(device)
                         for _ in range(2))
        for kind, heads in (('six logit planes', (logits,)), ('two sigmoid planes', sigmoids)):
            fused, stock = photo_paste_mask(parsing, palm, rule, heads, c0), torch_paste_mask(parsing, palm, rule, heads, c0)
            assert torch.equal(fused, stock), 'the yardstick forms another mask'
            say('(%d, %d, %d) in %d columns, %s: the two masks agree; %.1f %% of the pixels are pasted'
                % (n, H, W, H, kind, 100.0 * float(fused.float().mean())))
            nbytes = n * H * W * (3 + 4 * sum(int(x.shape[1]) for x in heads))          # labels, palm, mask; the planes' content columns
            rows = [('photo_paste_mask', lambda: photo_paste_mask(parsing, palm, rule, heads, c0), nbytes),
                    ('the mask from torch ops', lambda: torch_paste_mask(parsing, palm, rule, heads, c0), None)]
            for name, fn, floor_bytes in rows:
                med, lo, hi = timed(fn, opt.iters)
                floor = '' if floor_bytes is None else '; %.1f MB at %.2f TB/s = %.1f us floor, %.1f x' % (
                    floor_bytes / 1e6, HBM_RATE / 1e12, floor_bytes / HBM_RATE * 1e6, med / (floor_bytes / HBM_RATE * 1e6))
                say('  %-28s %8.1f us per call (min %.1f, max %.1f over 5 windows)%s' % (name, med, lo, hi, floor))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
