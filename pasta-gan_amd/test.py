"""Unpaired try-on images from the test pairs of a trained snapshot (the reference's test.py, test.sh mode 1).

For every line ``person clothes`` of the pair lists of ``UPT_subset1_256_192`` and ``UPT_subset2_256_192`` under --dataroot,
the person is dressed in the donor's upper garment and the image is written to
``<outdir>/<sub-dataset>/<person stem>__<clothes stem>.png`` (RGB, 256 x 192: columns 32..223 of the generator's square).

Loader workers only decode files and stack every distinct person of a batch once (training.dataset.collate_region_outfits: a
pair is the outfit (person, donor, -)).  Everything on the GPU runs in this process, in ``tryon_cli.generate_256``: the batch
preparation (training.tryon_pairs.TryOnPairOutfitBatchBuilder), the call sequence of the reference's test.py:119-128
(style_encoding, const_encoding, mapping, synthesis) and the conversion to uint8 (pasta_images_to_u8).

Differences from the reference, on purpose:
  --noise-mode is forwarded to G.synthesis and --trunc to G.mapping.  The reference declares both and forwards neither, so its
  images use random noise and no truncation: ``--noise-mode random`` reproduces that.  The default, ``const``, makes the
  output a function of the inputs alone.
  --network must name a local file: URLs are refused (nothing is downloaded).
  --workers sets the loader's processes (the reference: 4).
  --seeds, --class and --projected-w are accepted and unused, as in the reference.
  --storage f32 | bf16 | f16 runs the generator in that activation storage, whatever it was pickled with.
  --scores FILE scores every image by region against what the generator was told to reproduce (metrics/tryon_fidelity.py: kept
  body parts against the photograph, garment patches against themselves; L1, PSNR, SSIM) and writes one JSON object.  These are
  this project's own figures; the reference has none for test.py.
  --change-region upperbody | lowerbody | fullbody takes the donor's upper garment (what a run without the option does, and the
  same bytes), the donor's lower garment over the person's own top, or both.  The reference's 256 test set knows the first only.
  --outfits FILE dresses every line ``person upper lower`` of FILE instead of the pair lists: the upper garment of one donor,
  the lower garment of another, ``-`` for a garment the person keeps (training.dataset.UvitonOutfits_256_test), written to
  ``<outdir>/<person's sub-dataset>/<person stem>__<upper stem>__<lower stem>.png``.  Both options are this project's own
  (include/pasta_hip.h lists the rules) and exclude each other.
  --part-geometry host | gpu (tryon_cli.part_geometry_option; default host, the bytes this command always wrote): with gpu the body
  parts' matrices of a batch are solved in one launch on the GPU instead of numpy on the host, a second rule that prepares almost
  exactly the same bytes; --scores then says ``part_geometry: gpu``.
  --fit-people pad | crop with --fit-filter bilinear | box (tryon_cli.fit_people_option; default: none) takes photographs of any
  size, which need not match within a pair or an outfit: every person is fitted to the model's canvas on the GPU before anything
  else (training.tryon_batch.fit_batch), padded so that all of the photograph shows or centre-cropped so that it fills
  the canvas; --scores then names both options.
"""

from typing import List, Optional

import click

import tryon_cli


@click.command()
@tryon_cli.shared_options('Root of the test data set', 16)
@tryon_cli.region_option
@tryon_cli.pair_outfits_option
@tryon_cli.workers_option
@tryon_cli.scores_option
def generate_images(network_pkl: str, seeds: Optional[List[int]], truncation_psi: float, class_idx: Optional[int], noise_mode: str,
                    projected_w: Optional[str], outdir: str, dataroot: str, batchsize: int, workers: int, scores_file: Optional[str],
                    storage: Optional[str] = None, change_region: Optional[str] = None, outfits_file: Optional[str] = None):
    """Generate unpaired try-on images from the test pairs with a trained snapshot.

    \b
    python test.py --network snapshot.pkl --outdir out --dataroot PASTA_UPT_256 --batchsize 16
    """
    del seeds, class_idx, projected_w
    tryon_cli.generate_256(network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, workers, outfits_file, change_region,
                           scores_file, storage)


if __name__ == '__main__':
    generate_images()  # pylint: disable=no-value-for-parameter
