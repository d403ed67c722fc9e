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
from typing import List, Optional

import click

import tryon_cli


@click.command()
@tryon_cli.shared_options('Root of the 512 x 320 test data set', 8)
@click.option('--change-region', help='Which garments the person takes from the donor', type=click.Choice(['fullbody', 'upperbody', 'lowerbody']),
              default='fullbody', show_default=True)
@tryon_cli.workers_option
def generate_images(network_pkl: str, seeds: Optional[List[int]], truncation_psi: float, class_idx: Optional[int], noise_mode: str,
                    projected_w: Optional[str], outdir: str, dataroot: str, batchsize: int, change_region: str, workers: int):
    """Generate unpaired try-on images at 512 x 320 from the test pairs with a trained snapshot.

    \b
    python test_512.py --network snapshot.pkl --outdir out --dataroot PASTA_UPT_512 --batchsize 8 --change-region fullbody
    """
    del seeds, class_idx, projected_w
    tryon_cli._local_snapshot(network_pkl)

    import numpy as np
    import PIL.Image
    import torch

    from training import dataset as custom_dataset
    from training.tryon_pairs import images_to_u8
    from training.tryon_regions import TryOnRegionBatchBuilder

    device = torch.device('cuda')
    G = tryon_cli.load_generator(network_pkl, device)
    os.makedirs(outdir, exist_ok=True)
    dataset = custom_dataset.UvitonDatasetFull_512_test(path=dataroot, change_region=change_region, use_labels=True, max_size=None, xflip=False)
    loader = tryon_cli.pair_loader(dataset, batchsize, workers)
    builder = TryOnRegionBatchBuilder(device, change_region)
    count = 0
    for raw in loader:
        batch = builder.build(raw)
        t, n = batch.tensors, batch.batch
        side = t['image'].shape[2]
        gen_z = torch.empty([n, 0], device=device)
        gen_imgs = tryon_cli.generate(G, t, gen_z, truncation_psi, noise_mode)
        panels = torch.cat([images_to_u8(x, 0, side) for x in (t['clothes'], t['image'], gen_imgs)], dim=2).cpu().numpy()
        for result in panels:
            PIL.Image.fromarray(np.ascontiguousarray(result)).save(os.path.join(outdir, str(count).zfill(3) + '.png'))
            count += 1
    print('finish: %d images under %s' % (count, outdir))


if __name__ == '__main__':
    generate_images()  # pylint: disable=no-value-for-parameter
