"""Unpaired try-on images from the test pairs of a trained snapshot (the reference's test.py, test.sh mode 1).

For every line ``person clothes`` of the pair lists of ``UPT_subset1_256_192`` and ``UPT_subset2_256_192`` under --dataroot,
the person is dressed in the donor's upper garment and the image is written to
``<outdir>/<sub-dataset>/<person stem>__<clothes stem>.png`` (RGB, 256 x 192: columns 32..223 of the generator's square).

Loader workers only decode files (training.dataset.collate_pairs).  Everything on the GPU runs in this process: the batch
preparation (training.tryon_pairs.TryOnPairBatchBuilder), the call sequence of the reference's test.py:119-128
(style_encoding, const_encoding, mapping, synthesis) and the conversion to uint8 (pasta_images_to_u8).

Differences from the reference, on purpose:
  --noise-mode is forwarded to G.synthesis and --trunc to G.mapping.  The reference declares both and forwards neither, so its
  images use random noise and no truncation: ``--noise-mode random`` reproduces that.  The default, ``const``, makes the
  output a function of the inputs alone.
  --network must name a local file: URLs are refused (nothing is downloaded).
  --workers sets the loader's processes (the reference: 4).
  --seeds, --class and --projected-w are accepted and unused, as in the reference.
  --scores FILE scores every image by region against what the generator was told to reproduce (metrics/tryon_fidelity.py: kept
  body parts against the photograph, garment patches against themselves; L1, PSNR, SSIM) and writes one JSON object.  These are
  this project's own figures; the reference has none for test.py.
"""

import json
import os
import re
from typing import List, Optional

import click


def num_range(s: str) -> List[int]:
    """Either a comma-separated list 'a,b,c' or a range 'a-c'."""
    first, dash, last = s.partition('-')
    if dash and first.isdigit() and last.isdigit():
        return list(range(int(first), int(last) + 1))
    return [int(x) for x in s.split(',')]


def _local_snapshot(path):
    if re.match(r'^[A-Za-z][A-Za-z0-9+.-]*://', path):
        raise click.BadParameter('%r is a URL: give the path of a local snapshot file' % path, param_hint='--network')
    if not os.path.isfile(path):
        raise click.BadParameter('%r is not a file' % path, param_hint='--network')
    return path


@click.command()
@click.option('--network', 'network_pkl', help='Network pickle filename (a local file)', required=True)
@click.option('--seeds', type=num_range, help='List of random seeds (unused, as in the reference)')
@click.option('--trunc', 'truncation_psi', type=float, help='Truncation psi, forwarded to G.mapping', default=1, show_default=True)
@click.option('--class', 'class_idx', type=int, help='Class label (unused, as in the reference)')
@click.option('--noise-mode', help='Noise mode, forwarded to G.synthesis', type=click.Choice(['const', 'random', 'none']), default='const',
              show_default=True)
@click.option('--projected-w', help='Projection result file (unused, as in the reference)', type=str, metavar='FILE')
@click.option('--outdir', help='Where to save the output images', type=str, required=True, metavar='DIR')
@click.option('--dataroot', help='Root of the test data set', type=str, required=True)
@click.option('--batchsize', help='Pairs per batch', type=click.IntRange(min=1), default=16, show_default=True)
@click.option('--workers', help='Loader processes (file decoding only)', type=click.IntRange(min=0), default=4, show_default=True)
@click.option('--scores', 'scores_file', help='Score the written images by region (kept body parts, upper and lower garment patches: L1, PSNR, '
              'SSIM) and write the results to FILE as JSON. With this option z of pair i is np.random.RandomState(i).randn(z_dim), so that '
              'the figures describe the images whatever the batch size [default: no scores]', type=str, metavar='FILE')
def generate_images(network_pkl: str, seeds: Optional[List[int]], truncation_psi: float, class_idx: Optional[int], noise_mode: str,
                    projected_w: Optional[str], outdir: str, dataroot: str, batchsize: int, workers: int, scores_file: Optional[str]):
    """Generate unpaired try-on images from the test pairs with a trained snapshot.

    \b
    python test.py --network snapshot.pkl --outdir out --dataroot PASTA_UPT_256 --batchsize 16
    """
    del seeds, class_idx, projected_w
    _local_snapshot(network_pkl)

    import numpy as np
    import PIL.Image
    import torch

    import legacy
    from training import dataset as custom_dataset
    from training.tryon_pairs import TryOnPairBatchBuilder, images_to_u8

    device = torch.device('cuda')
    print('Loading networks from "%s"...' % network_pkl)
    with open(network_pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].to(device).eval().requires_grad_(False)  # type: ignore

    os.makedirs(outdir, exist_ok=True)
    dataset = custom_dataset.UvitonDatasetV19_test(path=dataroot, use_labels=True, max_size=None, xflip=False)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batchsize, shuffle=False, num_workers=workers, pin_memory=True,
                                         collate_fn=custom_dataset.collate_pairs)
    print(len(dataset))
    builder = TryOnPairBatchBuilder(device)
    if scores_file is not None:
        from metrics import tryon_fidelity
        partials = tryon_fidelity.new_partials(len(dataset), device)
        pixels = tryon_fidelity.PIXELS                              # content pixels of a pair; every batch brings its own
    written = 0
    for raw in loader:
        batch = builder.build(raw, keep_stages=scores_file is not None)
        t, n = batch.tensors, batch.batch
        height, width = raw['image'].shape[1], raw['image'].shape[2]
        gen_z = torch.empty([n, 0], device=device)
        if scores_file is not None:
            pair_index = raw['raw_idx'].tolist()                    # the pairs' positions in the pair lists
            gen_z = tryon_fidelity.pair_z(pair_index, G.z_dim, device)
        with torch.no_grad():
            gen_c, cat_feat_list = G.style_encoding(t['style_input'], t['retain'])
            pose_feat = G.const_encoding(t['pose'])
            ws = G.mapping(gen_z, gen_c, truncation_psi=truncation_psi)
            cat_feats = {str(feat.shape[2]): feat for feat in cat_feat_list}
            _, gen_imgs, _, _ = G.synthesis(ws, pose_feat, cat_feats, t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                                            t['denorm_lower_mask'], noise_mode=noise_mode)
        images = images_to_u8(gen_imgs, (height - width) // 2, width).cpu().numpy()
        if scores_file is not None:
            tryon_fidelity.score_batch(gen_imgs, batch, pair_index, partials)
            pixels = height * width
        for img, person, clothes in zip(images, batch.person_name, batch.clothes_name):
            save_dir = os.path.join(outdir, person.split('/')[0])
            os.makedirs(save_dir, exist_ok=True)
            name = os.path.basename(person)[:-4] + '__' + os.path.basename(clothes)[:-4] + '.png'
            PIL.Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(save_dir, name))
            written += 1
    print('finish: %d images under %s' % (written, outdir))
    if scores_file is not None:
        results = tryon_fidelity.finish(partials, 'tryon', pixels=pixels)
        line = json.dumps(dict(results=results, pairs=written, network=network_pkl, dataroot=dataroot, noise_mode=noise_mode))
        print(line)
        os.makedirs(os.path.dirname(os.path.abspath(scores_file)), exist_ok=True)
        with open(scores_file, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    generate_images()  # pylint: disable=no-value-for-parameter
