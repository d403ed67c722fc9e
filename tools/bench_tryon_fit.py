"""What fitting people to the canvas costs on one GPU:

    python tools/bench_tryon_fit.py [--runs 30] [--warmup 5] [--train-iters 0] [--out FILE]

16 photographs of 1024 x 768 with their label maps, packed as ``training.dataset.collate`` packs them, into each canvas
(256 x 192 and 512 x 320), for each mode (pad, crop) and filter (bilinear, box), in one process:

  fit_batch     ``training.tryon_batch.fit_batch`` from the host's packed batch to the fitted tensors: tap tables, three uploads,
                two launches, joints; wall clock around a device synchronisation, the median of ``--runs`` after ``--warmup``;
  upload        the bare upload of the packed batch (photographs and label maps), the same way;
  kernels       the two launches of pasta_fit_people_u8 alone, device events around windows of 50 calls, next to the bytes they
                read at least once and write, as a share of the HBM peak (8 TB/s);
  PIL           ``PIL.Image.resize`` of the same 16 photographs (the same filter) and label maps (NEAREST: PIL has no mode) with the
                placing on the canvas, on one host core.

``--train-iters K`` (K > 0) adds two short training runs each on a canvas-size tree and on its ragged copy opened with
``fit='pad'`` (tests/fit_tree.py), taking turns: sec/kimg of K iterations of batch 2 after the first tick."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), ROOT]

HBM_PEAK = 8.0e12
PEOPLE, SOURCE = 16, (1024, 768)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--runs', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--train-iters', type=int, default=0)
    ap.add_argument('--out', metavar='FILE', help='also write the lines to FILE')
    opt = ap.parse_args()

    import numpy as np
    import PIL.Image
    import torch
    import fit_ref
    from torch_utils.ops import _native
    from training import tryon_batch
    from training.dataset import pack_people
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

    def timed(fn):
        return stats([wall(fn) for _ in range(opt.warmup + opt.runs)][opt.warmup:])

    say('%s, torch %s, %d runs after %d warm-ups; %d people of %d x %d' % (torch.cuda.get_device_name(0), torch.__version__, opt.runs, opt.warmup,
                                                                         PEOPLE, *SOURCE))
    rng = np.random.default_rng(0)
    labels = fit_ref.voronoi_labels(*SOURCE, 0)
    people = [(rng.integers(0, 256, [*SOURCE, 3], dtype=np.uint8), np.roll(labels, 17 * i, axis=1)) for i in range(PEOPLE)]
    image, parsing, image_hw, image_offsets = pack_people(people)
    keypoints = np.concatenate([rng.uniform(0, 700, [PEOPLE, 18, 2]), np.ones([PEOPLE, 18, 1])], axis=2)
    say('  upload of the packed batch (%.1f MB)  %8.3f ms (min %.3f, max %.3f)'
        % ((image.numel() + parsing.numel()) / 1e6, *timed(lambda: (image.to(device, non_blocking=True), parsing.to(device, non_blocking=True)))))
    image_d, parsing_d = image.to(device), parsing.to(device)
    lib, P = _native.lib(), _native.ptr
    for canvas in ((256, 192), (512, 320)):
        for mode in tryon_batch.FIT_MODES:
            for filter in tryon_batch.FIT_FILTERS:
                raw = dict(image=image, parsing=parsing, image_hw=image_hw, image_offsets=image_offsets, keypoints=keypoints,
                           fit=dict(mode=mode, filter=filter, canvas=canvas))
                whole = timed(lambda: tryon_batch.fit_batch(raw, device))
                rectangles = tryon_batch.fit_rectangles(image_hw.numpy(), canvas, mode)
                t0 = time.perf_counter()
                tryon_batch.fit_taps.cache_clear()
                plan = tryon_batch.fit_plan(image_hw.numpy(), image_offsets.numpy(), rectangles, filter)
                cold = (time.perf_counter() - t0) * 1e3
                plan_d = torch.from_numpy(plan).to(device)
                H, W = canvas
                outs = torch.empty([PEOPLE, H, W, 3], dtype=torch.uint8, device=device), torch.empty([PEOPLE, H, W], dtype=torch.uint8, device=device)

                def launch():
                    _native.check(lib.pasta_fit_people_u8(P(image_d), P(parsing_d), int(parsing_d.numel()), P(plan_d), int(plan.size), P(outs[0]),
                                                          P(outs[1]), PEOPLE, H, W, _native.stream()))
                for _ in range(5):
                    launch()
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                windows = []
                for _ in range(5):
                    start.record()
                    for _ in range(50):
                        launch()
                    end.record()
                    end.synchronize()
                    windows.append(start.elapsed_time(end) / 50 * 1e3)
                # crop reads only the window it shows: count the source bytes under the canvas
                shown = [min(1.0, H / r[0]) * min(1.0, W / r[1]) for r in rectangles]
                nbytes = sum(4 * h * w * s for (h, w), s in zip(image_hw.tolist(), shown)) + outs[0].numel() + outs[1].numel()
                kernel = stats(windows)
                t0 = time.perf_counter()
                for (img, lab), (Hc, Wc, oy, ox) in zip(people, rectangles):
                    a = np.asarray(PIL.Image.fromarray(img).resize((Wc, Hc), PIL.Image.BOX if filter == 'box' else PIL.Image.BILINEAR))
                    b = np.asarray(PIL.Image.fromarray(lab).resize((Wc, Hc), PIL.Image.NEAREST))
                    fit_ref.place(a, canvas, oy, ox, 255), fit_ref.place(b, canvas, oy, ox, 0)
                pil = (time.perf_counter() - t0) * 1e3
                say('%d x %d %-4s %-8s fit_batch %7.3f ms (min %.3f, max %.3f) | kernels %7.1f us (min %.1f, max %.1f), %.1f MB, %.1f%% of %.0f TB/s | '
                    'plan from a cold cache %.2f ms, %d words | PIL on one core %.1f ms'
                    % (H, W, mode, filter, *whole, *kernel, nbytes / 1e6, 100.0 * nbytes / (kernel[0] * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12, cold,
                       plan.size, pil))

    if opt.train_iters > 0:
        import fit_tree
        from train_grid_tree import make_tree
        from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
        with tempfile.TemporaryDirectory() as tmp:
            plain = make_tree(os.path.join(tmp, 'plain'))
            fit_tree.ragged_copy(plain, os.path.join(tmp, 'ragged'))
            sets = {'canvas-size tree': dict(path=plain), "ragged tree, fit='pad'": dict(path=os.path.join(tmp, 'ragged'), fit='pad')}
            for turn in range(2):
                for name, kwargs in sets.items():
                    run_dir = os.path.join(tmp, 'run%d_%d' % (turn, len(os.listdir(tmp))))
                    os.makedirs(run_dir)
                    training_loop(batch_size=2, batch_gpu=2, cfg=fashion_config(channel_base=2048, mbstd_group_size=2), device=device,
                                  training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', **kwargs),
                                  data_loader_kwargs=dict(num_workers=0, pin_memory=True), run_dir=run_dir, total_kimg=(1 + opt.train_iters) * 2 / 1000,
                                  kimg_per_tick=opt.train_iters * 2 / 1000, image_snapshot_ticks=None, network_snapshot_ticks=None, snapshot_gnum=3)
                    with open(os.path.join(run_dir, 'stats.jsonl')) as f:
                        ticks = [json.loads(line) for line in f]
                    say('training, %-24s run %d: %8.2f sec/kimg over the last tick of %d iterations of batch 2'
                        % (name, turn, ticks[-1]['Timing/sec_per_kimg']['mean'], opt.train_iters))
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
