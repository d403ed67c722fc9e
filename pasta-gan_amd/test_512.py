"""Unpaired try-on images at 512 x 320 from the test pairs of a trained snapshot (the reference's test_512.py).

For every line ``person clothes`` of the pair lists of ``Zalando_512_320``, ``Zalora_512_320``, ``Deepfashion_512_320`` and
``MPV_512_320`` under --dataroot, the person is dressed in the donor's garments of --change-region and one image is written to
``<outdir>/<count>.png`` (count zero-filled to three digits, in loader order): ``clothes | person | generated`` side by side,
RGB, 512 x 1536, each the generator's whole padded square.  The two input panels are the reference's float round trip,
``(x / 127.5 - 1 + 1) * 127.5`` truncated, not copies of the files.

Loader workers only decode files and stack every distinct person of a batch once (training.dataset.collate_region_outfits: a
pair is the outfit of its change region).  Everything on the GPU runs in this process, in ``tryon_cli.generate_512``: the
batch preparation (training.tryon_regions.TryOnOutfitBatchBuilder), the call sequence of the reference's test_512.py:134-142
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
  --storage f32 | bf16 | f16 runs the generator in that activation storage, whatever it was pickled with.
  --scores FILE scores every image by region (metrics/tryon_fidelity.py) and writes one JSON object; z of item i is then
  ``pair_z(i)``.
  --outfits FILE dresses every line ``person upper lower`` of FILE instead of the pair lists, ``-`` for a garment the person
  keeps (training.dataset.UvitonOutfits_512_test), written as ``upper donor | lower donor | person | generated``.  It excludes
  an explicit --change-region.  These three options are this project's own.
"""

from typing import List, Optional

import click

import tryon_cli


@click.command()
@tryon_cli.shared_options('Root of the 512 x 320 test data set', 8)
@tryon_cli.scores_option
@tryon_cli.outfits_option
@click.option('--change-region', help='Which garments the person takes from the donor', type=click.Choice(['fullbody', 'upperbody', 'lowerbody']),
              default='fullbody', show_default=True)
@tryon_cli.workers_option
def generate_images(network_pkl: str, seeds: Optional[List[int]], truncation_psi: float, class_idx: Optional[int], noise_mode: str,
                    projected_w: Optional[str], outdir: str, dataroot: str, batchsize: int, change_region: str, workers: int,
                    outfits_file: Optional[str] = None, scores_file: Optional[str] = None, storage: Optional[str] = None):
    """Generate unpaired try-on images at 512 x 320 from the test pairs with a trained snapshot.

    \b
    python test_512.py --network snapshot.pkl --outdir out --dataroot PASTA_UPT_512 --batchsize 8 --change-region fullbody
    """
    del seeds, class_idx, projected_w
    # the default region, 'fullbody', does not count as given: --outfits excludes only a region the user named
    tryon_cli.generate_512(network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, tryon_cli._explicit_region(change_region),
                           workers, outfits_file, scores_file, storage)


if __name__ == '__main__':
    generate_images()  # pylint: disable=no-value-for-parameter
