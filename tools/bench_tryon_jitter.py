"""What jittered people cost a training batch on one GPU:

    python tools/bench_tryon_jitter.py [--runs 30] [--warmup 5] [--out FILE]

Per case -- 16 people at 256 x 192 (FullBodyBatchBuilder), 8 and 16 people at 512 x 320 (FullBodyRegionBatchBuilder; 8 is the
batch the 512 model trains with, 16 the batch profiles/tryon_mirror_bench.txt measured) -- in one process: ``build()`` of the same
collated people (the five of the tests' tiny trees, repeated) as they are and numbered for ``--jitter-people`` at the top of every
range, wall clock from before the upload to after a device synchronisation, the median of ``--runs`` runs after ``--warmup``
warm-ups, the two kinds of batch taking turns.  The comparison is the plain build of the same process; its own spread (min, max)
is printed next to it.  Below them, the parts the jittered build adds, each on its own: the launch of pasta_tryon_jitter_u8
(device events around 200 calls, next to the bytes it writes and at least reads at the HBM rate a float4 copy reaches,
6.29 TB/s), the host's draws, integers and joints, and ``jitter_batch`` as the builder calls it."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), ROOT]

HBM_RATE = 6.29e12
SPEC = dict(scale=0.5, rotate=45.0, shift=0.25, colour=0.5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', metavar='FILE', help='also write the lines to FILE')
    opt = ap.parse_args()

    import numpy as np
    import torch
    from torch_utils.ops import _native
    from training import tryon_batch
    from training.dataset import UvitonDatasetFull, UvitonDatasetFull_512, collate
    from tryon_512_train_tree import make_512_train_tree
    from tryon_tree import make_tree
    device = torch.device('cuda')
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def stats(times):
        return float(np.median(times)), min(times), max(times)

    say('%s, torch %s, %d runs after %d warm-ups' % (torch.cuda.get_device_name(0), torch.__version__, opt.runs, opt.warmup))
    with tempfile.TemporaryDirectory() as tmp:
        ds256 = UvitonDatasetFull(make_tree(os.path.join(tmp, 't256')))
        ds512 = UvitonDatasetFull_512(make_512_train_tree(os.path.join(tmp, 't512')))
        for size, ds, people in (('256 x 192', ds256, 16), ('512 x 320', ds512, 8), ('512 x 320', ds512, 16)):
            builder = tryon_batch.builder_for(ds, device)
            plain_raw = collate([ds[i % len(ds)] for i in range(people)])
            batches = {0: plain_raw, 1: dict(plain_raw, jitter=dict(spec=SPEC, seed=0, positions=np.arange(people, dtype=np.int64)))}
            times = {0: [], 1: []}
            for run in range(opt.warmup + opt.runs):
                for kind in (0, 1):
                    t = wall(lambda: builder.build(batches[kind]))
                    if run >= opt.warmup:
                        times[kind].append(t)
            plain, jittered = stats(times[0]), stats(times[1])
            say('%s, build() of %d people' % (size, people))
            say('  as they are       %8.3f ms (min %.3f, max %.3f)' % plain)
            say('  jittered          %8.3f ms (min %.3f, max %.3f)' % jittered)
            say('  difference        %8.3f ms of the medians; the plain runs spread over %.3f ms' % (jittered[0] - plain[0], plain[2] - plain[1]))

            # the parts, each on its own
            raw = batches[1]
            image, parsing, keypoints = tryon_batch.upload_person(raw, device, 'bench')
            n, H, W, _ = image.shape
            geometry, tone = tryon_batch.jitter_parameters(SPEC, 0, raw['jitter']['positions'], H, W)
            affine = torch.from_numpy(tryon_batch.jitter_affine_q16(geometry, H, W)).to(device)
            matrix = torch.from_numpy(tryon_batch.jitter_colour_q8(tone)).to(device)
            outs = [torch.empty_like(t) for t in (image, parsing)]
            lib, P = _native.lib(), _native.ptr
            def launch():
                _native.check(lib.pasta_tryon_jitter_u8(P(image), P(parsing), P(affine), P(matrix), *[P(t) for t in outs], n, H, W, _native.stream()))
            for _ in range(10):
                launch()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            windows = []
            for _ in range(5):
                start.record()
                for _ in range(200):
                    launch()
                end.record()
                end.synchronize()
                windows.append(start.elapsed_time(end) / 200 * 1e3)
            nbytes = 2 * (image.numel() + parsing.numel())
            say('  pasta_tryon_jitter_u8 alone %6.1f us per call (min %.1f, max %.1f over 5 windows of 200); %.1f MB written and at least read, %.1f us at %.2f TB/s'
                % (*stats(windows), nbytes / 1e6, nbytes / HBM_RATE * 1e6, HBM_RATE / 1e12))
            host = [0.0] * opt.runs
            for i in range(opt.runs):
                t0 = time.perf_counter()
                g, c = tryon_batch.jitter_parameters(SPEC, 0, raw['jitter']['positions'], H, W)
                tryon_batch.jitter_affine_q16(g, H, W), tryon_batch.jitter_colour_q8(c), tryon_batch.jitter_keypoints(keypoints, g, H, W)
                host[i] = (time.perf_counter() - t0) * 1e3
            say('  draws, integers, joints (host) %6.3f ms (min %.3f, max %.3f)' % stats(host))
            helper = [wall(lambda: tryon_batch.jitter_batch(raw, image, parsing, keypoints)) for _ in range(opt.warmup + opt.runs)][opt.warmup:]
            say('  jitter_batch as called      %6.3f ms (min %.3f, max %.3f)' % stats(helper))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
