"""Timings of the test builders on one GPU, the figures of DESIGN.md section 9 (outfits), at 512 x 320:

    python tools/bench_tryon_builders.py [--batch 16] [--warmup 5] [--repeats 30] [--rounds 1]

  1. TryOnOutfitBatchBuilder.build for --batch fully mixed outfits (three distinct people each: M = 3 * batch);
  2. the same for --batch (p, c, -) outfits (M = 2 * batch);
  3. TryOnRegionBatchBuilder('fullbody').build for --batch pairs (M = 2 * batch as well);
and at 256 x 192, with the people of tests/tryon_pairs_tree.py:
  4. TryOnPairOutfitBatchBuilder.build for --batch fully mixed outfits (M = 3 * batch);
  5. the same for --batch (p, c, -) outfits (M = 2 * batch);
  6. TryOnPairBatchBuilder.build for --batch pairs (M = 2 * batch), which 5 equals bit for bit.
Each line is the median wall time around build() and torch.cuda.synchronize() after the warm-ups, and the median host time
spent inside patch_pipeline.part_matrices (the 8 x 8 solves) with its share.  Every builder is measured twice, ``geometry`` 'host'
and, on the next line, 'gpu' (patch_pipeline.part_geometry's one launch: DESIGN 8n; its part_matrices time is 0 by construction);
--rounds repeats the whole list in the same process on the same batches.  The people are those of the tiny trees that have
key points, repeated under distinct names: only the count of distinct people matters to the timing."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), ROOT]


def outfit_batch(people, idx):
    """The batch of training.dataset.collate_outfits for ``idx`` [N, 3] (person, upper, lower) into a stack of idx.max() + 1 people."""
    import torch
    m = int(idx.max()) + 1
    pick = [people[i % len(people)] for i in range(m)]
    names = ['person%d' % i for i in range(m)]
    out = dict(people_image=torch.from_numpy(np.stack([p[0] for p in pick])), people_parsing=torch.from_numpy(np.stack([p[1] for p in pick])),
               people_keypoints=torch.from_numpy(np.stack([p[2] for p in pick])), people_name=names, raw_idx=torch.arange(len(idx)))
    for k, role in enumerate(('person', 'upper', 'lower')):
        out[role + '_idx'] = torch.from_numpy(np.ascontiguousarray(idx[:, k]))
        out[role + '_name'] = [names[i] for i in idx[:, k]]
    return out


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--batch', type=int, default=16)
    parser.add_argument('--warmup', type=int, default=5)
    parser.add_argument('--repeats', type=int, default=30)
    parser.add_argument('--rounds', type=int, default=1)
    args = parser.parse_args()

    import torch
    from training import patch_pipeline
    from training.dataset import UvitonDatasetFull_512_test, UvitonDatasetV19_test, collate_pairs
    from training.tryon_pairs import TryOnPairBatchBuilder, TryOnPairOutfitBatchBuilder
    from training.tryon_regions import TryOnOutfitBatchBuilder, TryOnRegionBatchBuilder
    from tryon_512_tree import make_512_tree
    from tryon_pairs_tree import make_pair_tree

    with tempfile.TemporaryDirectory() as root:
        pairs = UvitonDatasetFull_512_test(path=make_512_tree(root), change_region='fullbody')
        pairs = [pairs[i] for i in (0, 1, 2)]                    # both people of these pairs have key points
    with tempfile.TemporaryDirectory() as root:
        pairs_256 = UvitonDatasetV19_test(path=make_pair_tree(root))
        pairs_256 = [pairs_256[i] for i in (0, 1, 4)]            # both people of these pairs have key points
    stack = lambda chosen: [(p[k + 'image'], p[k + 'parsing'], p[k + 'keypoints']) for p in chosen for k in ('', 'clothes_')]
    people, people_256 = stack(pairs), stack(pairs_256)
    n = args.batch
    mixed = np.arange(3 * n, dtype=np.int64).reshape(n, 3)
    own_lower = np.stack([np.arange(0, 2 * n, 2), np.arange(1, 2 * n, 2), np.arange(0, 2 * n, 2)], axis=1).astype(np.int64)

    solving = [0.0]
    solve = patch_pipeline.part_matrices

    def timed_solve(*a, **k):
        t = time.perf_counter()
        out = solve(*a, **k)
        solving[0] += time.perf_counter() - t
        return out
    patch_pipeline.part_matrices = timed_solve

    def measure(name, build, raw, geometry):
        for _ in range(args.warmup):
            build(raw)
            torch.cuda.synchronize()
        total, host = [], []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            solving[0] = 0.0
            t = time.perf_counter()
            build(raw)
            torch.cuda.synchronize()
            total.append(time.perf_counter() - t)
            host.append(solving[0])
        ms, solve_ms = 1e3 * float(np.median(total)), 1e3 * float(np.median(host))
        print(json.dumps(dict(name=name, geometry=geometry, median_ms=round(ms, 2), part_matrices_ms=round(solve_ms, 2), part_matrices_share=round(solve_ms / ms, 3),
                              min_ms=round(1e3 * min(total), 2), max_ms=round(1e3 * max(total), 2))), flush=True)

    cases = [('outfits, fully mixed (M = %d)' % (3 * n), TryOnOutfitBatchBuilder, (), outfit_batch(people, mixed)),
             ('outfits (p, c, -) (M = %d)' % (2 * n), TryOnOutfitBatchBuilder, (), outfit_batch(people, own_lower)),
             ('region builder, fullbody (M = %d)' % (2 * n), TryOnRegionBatchBuilder, ('fullbody',),
              collate_pairs([pairs[i % len(pairs)] for i in range(n)])),
             ('256: outfits, fully mixed (M = %d)' % (3 * n), TryOnPairOutfitBatchBuilder, (), outfit_batch(people_256, mixed)),
             ('256: outfits (p, c, -) (M = %d)' % (2 * n), TryOnPairOutfitBatchBuilder, (), outfit_batch(people_256, own_lower)),
             ('256: pair builder (M = %d)' % (2 * n), TryOnPairBatchBuilder, (), collate_pairs([pairs_256[i % len(pairs_256)] for i in range(n)]))]
    for _ in range(args.rounds):
        for name, cls, extra, raw in cases:
            for geometry in ('host', 'gpu'):
                measure(name, cls('cuda', *extra, geometry=geometry).build, raw, geometry)


if __name__ == '__main__':
    main()
