"""What mirrored people cost a training batch on one GPU:

    python tools/bench_tryon_mirror.py [--runs 30] [--warmup 5] [--out FILE]

Per size -- 256 x 192 (FullBodyBatchBuilder) and 512 x 320 (FullBodyRegionBatchBuilder) -- in one process: ``build()`` of the same
16 collated people (the five of the tests' tiny trees, repeated) with no flag set and with every flag set, wall clock from before
the upload to after a device synchronisation, the median of ``--runs`` runs after ``--warmup`` warm-ups, the two kinds of batch
taking turns.  The comparison is the unmirrored build of the same process; its own spread (min, max) is printed next to it.
Below them, the parts the mirrored build adds, each on its own: the launch of pasta_tryon_mirror_u8 (device events around 200
calls, next to the bytes it moves at the HBM rate a float4 copy reaches, 6.29 TB/s), ``mirror_keypoints`` on the host, and
``mirror_batch`` as the builder calls it (two small uploads, three allocations, the launch)."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), ROOT]

HBM_RATE = 6.29e12
PEOPLE = 16


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

    say('%s, torch %s, %d runs after %d warm-ups, %d people per batch' % (torch.cuda.get_device_name(0), torch.__version__, opt.runs, opt.warmup, PEOPLE))
    with tempfile.TemporaryDirectory() as tmp:
        sets = (('256 x 192', UvitonDatasetFull(make_tree(os.path.join(tmp, 't256')), mirror_people=True)),
                ('512 x 320', UvitonDatasetFull_512(make_512_train_tree(os.path.join(tmp, 't512')), mirror_people=True)))
        for size, ds in sets:
            people = len(ds) // 2
            builder = tryon_batch.builder_for(ds, device)
            batches = {flag: collate([ds[i % people + people * flag] for i in range(PEOPLE)]) for flag in (0, 1)}
            assert batches[0]['xflip'].tolist() == [0] * PEOPLE and batches[1]['xflip'].tolist() == [1] * PEOPLE
            times = {0: [], 1: []}
            for run in range(opt.warmup + opt.runs):
                for flag in (0, 1):
                    t = wall(lambda: builder.build(batches[flag]))
                    if run >= opt.warmup:
                        times[flag].append(t)
            plain, mirrored = stats(times[0]), stats(times[1])
            say('%s, build() of %d people' % (size, PEOPLE))
            say('  no flag set       %8.3f ms (min %.3f, max %.3f)' % plain)
            say('  every flag set    %8.3f ms (min %.3f, max %.3f)' % mirrored)
            say('  difference        %8.3f ms of the medians; the unmirrored runs spread over %.3f ms' % (mirrored[0] - plain[0], plain[2] - plain[1]))

            # the parts, each on its own
            raw = batches[1]
            image, parsing, keypoints = tryon_batch.upload_person(raw, device, 'bench')
            n, H, W, _ = image.shape
            erase, erase_hw = tryon_batch.upload_erase(raw, device, n)
            flip, lut = raw['xflip'].to(device), torch.from_numpy(tryon_batch.mirror_lut()).to(device)
            outs = [torch.empty_like(t) for t in (image, parsing, erase)]
            lib, P = _native.lib(), _native.ptr
            def launch():
                _native.check(lib.pasta_tryon_mirror_u8(P(image), P(parsing), P(erase), P(erase_hw), P(flip), P(lut), *[P(t) for t in outs], n, H, W,
                                                        int(erase.shape[1]), int(erase.shape[2]), _native.stream()))
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
            nbytes = 2 * (image.numel() + parsing.numel() + erase.numel())
            say('  pasta_tryon_mirror_u8 alone %6.1f us per call (min %.1f, max %.1f over 5 windows of 200); %.1f MB read and written, %.1f us at %.2f TB/s'
                % (*stats(windows), nbytes / 1e6, nbytes / HBM_RATE * 1e6, HBM_RATE / 1e12))
            host = [0.0] * opt.runs
            for i in range(opt.runs):
                t0 = time.perf_counter()
                tryon_batch.mirror_keypoints(keypoints, W, raw['xflip'])
                host[i] = (time.perf_counter() - t0) * 1e3
            say('  mirror_keypoints (host)     %6.3f ms (min %.3f, max %.3f)' % stats(host))
            helper = [wall(lambda: tryon_batch.mirror_batch(raw, image, parsing, keypoints, erase, erase_hw)) for _ in range(opt.warmup + opt.runs)][opt.warmup:]
            say('  mirror_batch as called      %6.3f ms (min %.3f, max %.3f)' % stats(helper))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
