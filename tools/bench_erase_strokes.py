"""What drawn erase masks cost a training batch on one GPU:

    python tools/bench_erase_strokes.py [--runs 30] [--warmup 5] [--out FILE]

Per size -- 16 people at 256 x 192 (FullBodyBatchBuilder) and 16 at 512 x 320 (FullBodyRegionBatchBuilder) -- in one process:
``build()`` of the same 16 collated people (the tests' tiny trees, repeated) with the masks of their files (``--erase-masks
files``) and numbered for ``--erase-masks strokes`` at the default strengths with 1 x 1 masks, wall clock from before the upload
to after a device synchronisation, the median of ``--runs`` runs after ``--warmup`` warm-ups, the two kinds of batch taking turns.
The bar: the strokes build's median is not above the files build's median by more than the spread (max - min) of the files runs
of this process.  Below them the launch of pasta_erase_strokes_u8 alone (device events around 200 calls, at the defaults and with
all 64 segments of the widest specification), the host's draws, and ``strokes_batch`` as the builder calls it."""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), ROOT]

PEOPLE = 16
WIDEST = dict(strokes=8, vertices=8, length=0.5, width=0.25, turn=180.0)


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
        trees = (('256 x 192', UvitonDatasetFull, make_tree(os.path.join(tmp, 't256'))),
                 ('512 x 320', UvitonDatasetFull_512, make_512_train_tree(os.path.join(tmp, 't512'))))
        for size, cls, tree in trees:
            files, drawn = cls(tree), cls(tree, erase_masks='strokes')
            builder = tryon_batch.builder_for(files, device)
            positions = np.arange(PEOPLE, dtype=np.int64)
            batches = {0: collate([files[i % len(files)] for i in range(PEOPLE)]),
                       1: tryon_batch.attach_strokes(collate([drawn[i % len(drawn)] for i in range(PEOPLE)]), drawn.erase_strokes, 0, positions)}
            times = {0: [], 1: []}
            for run in range(opt.warmup + opt.runs):
                for kind in (0, 1):
                    t = wall(lambda: builder.build(batches[kind]))
                    if run >= opt.warmup:
                        times[kind].append(t)
            plain, strokes = stats(times[0]), stats(times[1])
            spread = plain[2] - plain[1]
            say('%s, build() of %d people' % (size, PEOPLE))
            say('  masks from files  %8.3f ms (min %.3f, max %.3f)' % plain)
            say('  masks drawn       %8.3f ms (min %.3f, max %.3f)' % strokes)
            say('  difference        %8.3f ms of the medians; the files runs spread over %.3f ms: the bar is %s'
                % (strokes[0] - plain[0], spread, 'met' if strokes[0] - plain[0] <= spread else 'MISSED'))

            # the parts, each on its own
            S = int(batches[1]['image'].shape[1])
            out = torch.empty([PEOPLE, S, S], dtype=torch.uint8, device=device)
            lib, P = _native.lib(), _native.ptr
            for name, spec in (('defaults', drawn.erase_strokes), ('widest specification', WIDEST)):
                segments, counts = tryon_batch.strokes_segments(spec, 0, positions, S)
                if spec is WIDEST:                   # every item's own segments, repeated up to all 64 rows
                    for n in range(PEOPLE):
                        segments[n] = np.resize(segments[n, :counts[n]], [64, 5])
                    counts[:] = 64
                seg_d, cnt_d = torch.from_numpy(segments).to(device), torch.from_numpy(counts).to(device)
                def launch():
                    _native.check(lib.pasta_erase_strokes_u8(P(seg_d), P(cnt_d), P(out), PEOPLE, S, _native.stream()))
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
                say('  pasta_erase_strokes_u8 alone, %s (%d to %d segments, %.1f %% set) %6.1f us per call (min %.1f, max %.1f over 5 windows of 200); %.2f MB written'
                    % (name, counts.min(), counts.max(), 100 * float(out.float().mean()), *stats(windows), out.numel() / 1e6))
            host = [0.0] * opt.runs
            for i in range(opt.runs):
                t0 = time.perf_counter()
                tryon_batch.strokes_segments(drawn.erase_strokes, 0, positions, S)
                host[i] = (time.perf_counter() - t0) * 1e3
            say('  draws and segments (host)   %6.3f ms (min %.3f, max %.3f)' % stats(host))
            erase, erase_hw = tryon_batch.upload_erase(batches[1], device, PEOPLE)
            helper = [wall(lambda: tryon_batch.strokes_batch(batches[1], erase, erase_hw, S)) for _ in range(opt.warmup + opt.runs)][opt.warmup:]
            say('  strokes_batch as called     %6.3f ms (min %.3f, max %.3f)' % stats(helper))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
