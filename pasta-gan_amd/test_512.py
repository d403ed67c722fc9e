"""Unpaired try-on images at 512 x 320 from the test pairs of a trained snapshot (the reference's test_512.py).

For every line ``person clothes`` of the pair lists of ``Zalando_512_320``, ``Zalora_512_320``, ``Deepfashion_512_320`` and
``MPV_512_320`` under --dataroot, the person is dressed in the donor's garments of --change-region and one image is written to
``<outdir>/<count>.png`` (count zero-filled to three digits, in loader order): ``clothes | person | generated`` side by side,
RGB, 512 x 1536, each the generator's whole padded square.  The two input panels are the reference's float round trip,
``(x / 127.5 - 1 + 1) * 127.5`` truncated, not copies of the files.

Loader workers only decode files (training.dataset.collate_pairs).  Everything on the GPU runs in this process: the batch
preparation (training.tryon_regions.TryOnRegionBatchBuilder), the call sequence of the reference's test_512.py:134-142
(style_encoding, const_encoding, mapping, synthesis with three return values) and the conversion to uint8
(pasta_images_to_u8).

Differences from the reference, on purpose:
  --change-region selects full-body, upper-body or lower-body try-on.  The reference makes the user edit the source.
  --noise-mode is forwarded to G.synthesis and --trunc to G.mapping.  The reference declares both and forwards neither, so its
  images use random noise and no truncation: ``--noise-mode random`` reproduces that.  The default, ``const``, makes the
  output a function of the inputs alone.
  --network must name a local file: URLs are refused (nothing is downloaded).
  --workers sets the loader's processes (the reference: 4).
  --seeds, --class and --projected-w are accepted and unused, as in the reference.
  The images are written with PIL as RGB; the reference's BGR swap followed by cv2.imwrite stores the same picture.
"""

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
@click.option('--dataroot', help='Root of the 512 x 320 test data set', type=str, required=True)
@click.option('--batchsize', help='Pairs per batch', type=click.IntRange(min=1), default=8, show_default=True)
@click.option('--change-region', help='Which garments the person takes from the donor', type=click.Choice(['fullbody', 'upperbody', 'lowerbody']),
              default='fullbody', show_default=True)
@click.option('--workers', help='Loader processes (file decoding only)', type=click.IntRange(min=0), default=4, show_default=True)
def generate_images(network_pkl: str, seeds: Optional[List[int]], truncation_psi: float, class_idx: Optional[int], noise_mode: str,
                    projected_w: Optional[str], outdir: str, dataroot: str, batchsize: int, change_region: str, workers: int):
    """Generate unpaired try-on images at 512 x 320 from the test pairs with a trained snapshot.

    \b
    python test_512.py --network snapshot.pkl --outdir out --dataroot PASTA_UPT_512 --batchsize 8 --change-region fullbody
    """
    del seeds, class_idx, projected_w
    _local_snapshot(network_pkl)

    import numpy as np
    import PIL.Image
    import torch

    import legacy
    from training import dataset as custom_dataset
    from training.tryon_pairs import images_to_u8
    from training.tryon_regions import TryOnRegionBatchBuilder

    device = torch.device('cuda')
    print('Loading networks from "%s"...' % network_pkl)
    with open(network_pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].to(device).eval().requires_grad_(False)  # type: ignore

    os.makedirs(outdir, exist_ok=True)
    dataset = custom_dataset.UvitonDatasetFull_512_test(path=dataroot, change_region=change_region, use_labels=True, max_size=None, xflip=False)
    loader = torch.utils.data.DataLoader(dataset, batch_size=batchsize, shuffle=False, num_workers=workers, pin_memory=True,
                                         collate_fn=custom_dataset.collate_pairs)
    print(len(dataset))
    builder = TryOnRegionBatchBuilder(device, change_region)
    count = 0
    for raw in loader:
        batch = builder.build(raw)
        t, n = batch.tensors, batch.batch
        side = t['image'].shape[2]
        gen_z = torch.empty([n, 0], device=device)
        with torch.no_grad():
            gen_c, cat_feat_list = G.style_encoding(t['style_input'], t['retain'])
            pose_feat = G.const_encoding(t['pose'])
            ws = G.mapping(gen_z, gen_c, truncation_psi=truncation_psi)
            cat_feats = {str(feat.shape[2]): feat for feat in cat_feat_list}
            _, gen_imgs, _ = G.synthesis(ws, pose_feat, cat_feats, t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                                         t['denorm_lower_mask'], noise_mode=noise_mode)
        panels = torch.cat([images_to_u8(x, 0, side) for x in (t['clothes'], t['image'], gen_imgs)], dim=2).cpu().numpy()
        for result in panels:
            PIL.Image.fromarray(np.ascontiguousarray(result)).save(os.path.join(outdir, str(count).zfill(3) + '.png'))
            count += 1
    print('finish: %d images under %s' % (count, outdir))


if __name__ == '__main__':
    generate_images()  # pylint: disable=no-value-for-parameter
