"""Timings of the training run's sample grid and statistics on one GPU (profiles/train_grid.txt):

    python tools/bench_train_grid.py [--gnum 23] [--batch 16] [--iters 16] [--repeats 5]

  1. SnapshotGrid.setup at gnum people (full-width fashion_config, a synthetic tree in the data set's layout);
  2. one snapshot image: G_ema over all gnum^2 cells in --batch minibatches, tiled, copied to the host, PNG written;
  3. --iters training iterations on a device-resident synthetic batch with the run's bookkeeping (statistics routed through
     training_stats.report, phase events recorded) and without it, interleaved, --repeats windows each; no tick (no
     Collector.update) falls inside a window.
Every figure is a wall time around torch.cuda.synchronize(), after a warm-up."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), ROOT]


def make_tree(root, people, seed=0):
    """`people` Zalando persons, all listed in train_img_vis (tests/tryon_tree.py's key points and label maps)."""
    import PIL.Image
    from tryon_tree import H, W, label_map, person_keypoints
    rng = np.random.default_rng(seed)
    for ds in ('Zalando_256_192', 'Zalora_256_192', 'Deepfashion_256_192', 'MPV_256_192'):
        for sub in ('image', 'keypoints', 'parsing'):
            os.makedirs(os.path.join(root, ds, sub))
        open(os.path.join(root, ds, 'train_pairs_front_list_0508.txt'), 'w').close()
    os.makedirs(os.path.join(root, 'train_img_vis'))
    os.makedirs(os.path.join(root, 'train_random_mask_acgpn'))
    PIL.Image.fromarray(np.zeros([H, W], np.uint8), mode='L').save(os.path.join(root, 'train_random_mask_acgpn', 'm0.png'))
    ds = 'Zalando_256_192'
    with open(os.path.join(root, ds, 'train_pairs_front_list_0508.txt'), 'w') as f:
        for i in range(people):
            name = 'p_%03d' % i
            img = rng.integers(0, 256, [H // 4, W // 4, 3]).repeat(4, 0).repeat(4, 1).astype(np.uint8)
            PIL.Image.fromarray(img).save(os.path.join(root, ds, 'image', name + '.jpg'), quality=95)
            kp = person_keypoints(10 + i, rng)
            with open(os.path.join(root, ds, 'keypoints', name + '_keypoints.json'), 'w') as g:
                json.dump({'version': 1.3, 'people': [{'pose_keypoints_2d': [float(v) for v in kp.reshape(-1)]}]}, g)
            PIL.Image.fromarray(label_map(rng, kp), mode='L').save(os.path.join(root, ds, 'parsing', name + '_label.png'))
            PIL.Image.fromarray(np.zeros([8, 8, 3], np.uint8)).save(os.path.join(root, 'train_img_vis', name + '.jpg'))
            f.write('%s.jpg %s_cloth.jpg\n' % (name, name))
    return root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gnum', type=int, default=23)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--iters', type=int, default=16)
    ap.add_argument('--repeats', type=int, default=5)
    opt = ap.parse_args()
    import torch
    import dnnlib
    from torch_utils import training_stats
    from training import training_loop_wo_flow_fullbody as TL
    from training.dataset import UvitonDatasetFull
    from training.snapshot_grid import SnapshotGrid
    from training.tryon_batch import FullBodyBatchBuilder
    device = torch.device('cuda')
    sync = torch.cuda.synchronize

    def wall(fn):
        sync(); t = time.perf_counter(); fn(); sync()
        return time.perf_counter() - t

    with tempfile.TemporaryDirectory() as tmp:
        ds = UvitonDatasetFull(make_tree(os.path.join(tmp, 'tree'), opt.gnum))
        builder = FullBodyBatchBuilder(device)
        grids = []
        setup = [wall(lambda: grids.append(SnapshotGrid.setup(ds, builder, device, gnum=opt.gnum))) for _ in range(1 + opt.repeats)]
        grid = grids[-1]
        del grids
        print('SnapshotGrid.setup gnum=%d: first %.3f s (cold), then %s s' % (opt.gnum, setup[0], ' '.join('%.3f' % t for t in setup[1:])))

        def step_of(stats):
            cfg = TL.fashion_config(mbstd_group_size=min(opt.batch, 4))
            if stats:
                cfg.loss_kwargs = dnnlib.EasyDict(cfg.loss_kwargs, report_fn=training_stats.report)
            step = TL.TrainingStep(device, cfg=cfg, batch_size=opt.batch, batch_gpu=opt.batch)
            if stats:
                for phase in step.phases:
                    phase.start_event, phase.end_event = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            return step
        plain, with_stats = step_of(False), step_of(True)
        grid_z = torch.randn([grid.cells, plain.G.z_dim], device=device).split(opt.batch)
        image = lambda: grid.save(TL.sample_images(plain.G_ema, grid, grid_z, opt.batch), os.path.join(tmp, 'fakes.png'))
        times = [wall(image) for _ in range(1 + opt.repeats)]
        print('one snapshot image (%d cells, minibatches of %d, %d x %d PNG): first %.3f s, then %s s'
              % (grid.cells, opt.batch, (opt.gnum + 1) * 256, (opt.gnum + 1) * 256, times[0], ' '.join('%.3f' % t for t in times[1:])))
        device_part = [wall(lambda: grid.canvas(TL.sample_images(plain.G_ema, grid, grid_z, opt.batch))) for _ in range(3)]
        print('  of which G_ema + assemble + tiling on the device: %s s (the rest is the copy to the host and PIL\'s PNG encoder)'
              % ' '.join('%.3f' % t for t in device_part))

        data = TL.SyntheticFullBodyBatch(opt.batch, device)
        window = lambda step: wall(lambda: [step.run(data) for _ in range(opt.iters)])
        for step in (plain, with_stats):
            window(step)                                   # warm-up: 16 iterations cover every lazy-regularisation phase
        collector = training_stats.Collector('.*')
        a, b = [], []
        for _ in range(opt.repeats):
            a.append(window(plain))
            b.append(window(with_stats))
        collector.update()
        fmt = lambda xs: ' '.join('%.4f' % x for x in xs)
        print('%d iterations, batch %d, without run bookkeeping: %s s  (median %.4f, spread max - min %.4f)'
              % (opt.iters, opt.batch, fmt(a), float(np.median(a)), max(a) - min(a)))
        print('%d iterations, batch %d, statistics + phase events:  %s s  (median %.4f, spread max - min %.4f)'
              % (opt.iters, opt.batch, fmt(b), float(np.median(b)), max(b) - min(b)))
        print('difference of the medians: %+.4f s per window = %+.3f ms per iteration; %d names collected, e.g. Loss/G/loss num %d'
              % (float(np.median(b) - np.median(a)), float(np.median(b) - np.median(a)) / opt.iters * 1e3, len(collector.names()),
                 collector.num('Loss/G/loss')))


if __name__ == '__main__':
    main()
