"""Measurements of DESIGN 8g (profiles/png_encoder_bench.txt).  Needs a GPU.

  batch     torch_utils.ops.png_encode.encode next to the PIL loop it replaces, on the same uint8 tensors: host clock around the
            call and a synchronise, median of --repeats after --warmup; then the encoder's steps, each ended by a synchronise.
  prepare   a 65-pair tree per size (the test tree makers, pair i drawn like pair i % 5 of the tiny trees) and a full-width,
            untrained fp32 snapshot per size under --dir.
  command   tryon_cli.generate_512 / generate_256 of the package under --package twice in one process, the second call timed:
            seconds, images/s, bytes written; --phases adds where the second call's time went.

One JSON line per result on stdout."""

import argparse
import io
import json
import os
import pickle
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _median_ms(fn, warmup, repeats):
    import torch
    laps = []
    for i in range(warmup + repeats):
        torch.cuda.synchronize()
        start = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        laps.append((time.perf_counter() - start) * 1e3)
    laps = laps[warmup:]
    return round(statistics.median(laps), 3), round(min(laps), 3), round(max(laps), 3)


def run_batch(args):
    sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests')]
    import numpy as np
    import PIL.Image
    import torch
    import png_ref
    from torch_utils.ops import png_encode

    def panels(n, squares):         # squares of 512 with 320 columns of photograph in each: a panel of test_512.py
        out = np.full((n, 512, 512 * squares, 3), 255, np.uint8)
        for i in range(n):
            for k in range(squares):
                out[i, :, 512 * k + 96:512 * k + 416] = png_ref.photograph(512, 320, 100 * i + k)
        return out
    shapes = {'[8, 512, 1536, 3] panels': lambda: panels(8, 3), '[8, 512, 2048, 3] panels': lambda: panels(8, 4),
              '[16, 256, 192, 3] photographs': lambda: np.stack([png_ref.photograph(256, 192, i) for i in range(16)])}
    for name, make in shapes.items():
        host = make()
        images = torch.from_numpy(host).cuda()

        def pil_loop():
            sizes = []
            for img in images.cpu().numpy():
                b = io.BytesIO()
                PIL.Image.fromarray(np.ascontiguousarray(img)).save(b, format='PNG')
                sizes.append(b.tell())
            return sizes
        files = png_encode.encode(images)
        for img, data in zip(host, files):
            assert np.array_equal(np.asarray(PIL.Image.open(io.BytesIO(data))), img)
        gpu = _median_ms(lambda: png_encode.encode(images), args.warmup, args.repeats)
        pil = _median_ms(pil_loop, args.warmup, args.repeats)
        steps = []
        for i in range(args.warmup + args.repeats):
            times = {}
            png_encode.encode(images, times)
            steps.append(times)
        steps = {k: round(statistics.median(s[k] for s in steps[args.warmup:]) * 1e3, 3) for k in steps[0]}
        print(json.dumps(dict(name=name, gpu_median_ms=gpu[0], gpu_min_ms=gpu[1], gpu_max_ms=gpu[2], pil_median_ms=pil[0], pil_min_ms=pil[1],
                              pil_max_ms=pil[2], steps_ms=steps, raw_bytes=int(host.size), gpu_bytes=sum(len(f) for f in files),
                              pil_bytes=sum(pil_loop()))), flush=True)


def run_prepare(args):
    sys.path[:0] = [os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests'), ROOT]
    import torch
    import tryon_512_tree
    import tryon_pairs_tree
    from training import networks
    os.makedirs(args.dir, exist_ok=True)
    for size, module, files in (
            (512, tryon_512_tree, dict(shape=(512, 320), block=8, label_map=tryon_512_tree.label_map, any_person=tryon_512_tree.standing_person)),
            (256, tryon_pairs_tree, dict(shape=(tryon_pairs_tree.H, tryon_pairs_tree.W), block=4, label_map=tryon_pairs_tree.label_map,
                                         any_person=lambda rng: tryon_pairs_tree.person_keypoints(0, rng)))):
        pairs = [(module.PAIRS[i % 5][0], 'p%d.jpg' % i, 'c%d.jpg' % i) for i in range(65)]
        tryon_pairs_tree.make_tree(os.path.join(args.dir, 'tree%d' % size), 0, module.SUBSETS, pairs, lambda i, rng: module.pair_keypoints(i % 5, rng),
                                   files, person_lower_six=size == 256)
        common = dict(z_dim=0, c_dim=512, w_dim=512, img_resolution=size, img_channels=3, mapping_kwargs=dict(num_layers=1),
                      synthesis_kwargs=dict(channel_base=16384, channel_max=512, conv_clamp=256))
        torch.manual_seed(0)
        G = (networks.GeneratorFull(patch_channels=45, **common) if size == 512 else networks.GeneratorV18(**common)).eval().requires_grad_(False)
        D = networks.Discriminator(c_dim=512, img_resolution=256, img_channels=3, channel_base=512, channel_max=32)
        with open(os.path.join(args.dir, 'snapshot%d.pkl' % size), 'wb') as f:
            pickle.dump(dict(G=G, D=D, G_ema=G), f)
        print(json.dumps(dict(prepared=size, pairs=len(pairs))), flush=True)


def run_command(args):
    package = os.path.abspath(args.package)
    sys.path[:0] = [package]
    import torch
    import tryon_cli
    phases = {}
    if args.phases:
        from torch_utils.ops import png_encode
        from training import tryon_pairs, tryon_regions

        def timed(owner, attr, name):
            inner = getattr(owner, attr)

            def wrapper(*a, **k):
                torch.cuda.synchronize()
                start = time.perf_counter()
                try:
                    return inner(*a, **k)
                finally:
                    torch.cuda.synchronize()
                    phases[name] = phases.get(name, 0.0) + time.perf_counter() - start
            setattr(owner, attr, wrapper)
        timed(tryon_cli, 'load_generator', 'load_snapshot')
        timed(tryon_cli, 'generate', 'generator')
        timed(png_encode, 'save', 'encode_and_write')
        timed(tryon_regions.TryOnOutfitBatchBuilder if args.size == 512 else tryon_pairs.TryOnPairOutfitBatchBuilder, 'build', 'builder')
    tree, pkl = os.path.join(args.dir, 'tree%d' % args.size), os.path.join(args.dir, 'snapshot%d.pkl' % args.size)
    extra = {} if args.encoder == 'parent' else dict(png_encoder=args.encoder)
    if args.geometry != 'parent':
        extra['part_geometry'] = args.geometry

    def call(outdir):
        if args.size == 512:
            tryon_cli.generate_512(pkl, 1, 'const', outdir, tree, 8, None, 4, **extra)
        else:
            tryon_cli.generate_256(pkl, 1, 'const', outdir, tree, 16, 4, **extra)
    outdir = os.path.join(args.dir, 'out_%s_%d_%d' % (args.encoder, args.size, os.getpid()))
    real_stdout, sys.stdout = sys.stdout, sys.stderr
    try:
        call(outdir + '_first')
        phases.clear()
        torch.cuda.synchronize()
        start = time.perf_counter()
        call(outdir)
        torch.cuda.synchronize()
        seconds = time.perf_counter() - start
    finally:
        sys.stdout = real_stdout
    files = [os.path.join(d, f) for d, _, fs in os.walk(outdir) for f in fs]
    line = dict(package=os.path.relpath(package, ROOT), size=args.size, encoder=args.encoder, geometry=args.geometry, seconds=round(seconds, 3), images=65,
                images_per_s=round(65 / seconds, 2), files=len(files), bytes_written=sum(os.path.getsize(f) for f in files))
    if args.phases:
        line['phases_s'] = {k: round(v, 3) for k, v in phases.items()}
        line['phases_s']['rest (loader wait, start-up of the workers, scores, names)'] = round(seconds - sum(phases.values()), 3)
    print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest='what', required=True)
    b = sub.add_parser('batch')
    b.add_argument('--warmup', type=int, default=5)
    b.add_argument('--repeats', type=int, default=30)
    p = sub.add_parser('prepare')
    p.add_argument('--dir', required=True)
    c = sub.add_parser('command')
    c.add_argument('--dir', required=True)
    c.add_argument('--package', default=os.path.join(ROOT, 'pasta-gan_amd'))
    c.add_argument('--size', type=int, choices=[256, 512], required=True)
    c.add_argument('--encoder', choices=['parent', 'pil', 'gpu'], required=True, help="'parent': a tree from before the option, called without it")
    c.add_argument('--geometry', choices=['parent', 'host', 'gpu'], default='parent',
                   help="the commands' part_geometry keyword (DESIGN 8n); 'parent': a tree from before that option, called without it")
    c.add_argument('--phases', action='store_true')
    args = ap.parse_args()
    dict(batch=run_batch, prepare=run_prepare, command=run_command)[args.what](args)


if __name__ == '__main__':
    main()
