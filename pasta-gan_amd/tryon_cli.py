"""What the two try-on command lines, test.py and test_512.py, share: the options the reference declares, the refusal of a
snapshot that is not a local file, loading ``G_ema``, the loader over a pair data set, the generator's call sequence and the
--scores report.

test.py's --outfits and --change-region are served by ``generate_256`` below; a run with neither is test.py's own loop.

test_512.py's --outfits and --scores are declared and served HERE, not in that file, which stays the reference's command line
as it was (``shared_options`` says how): ``generate_512`` is the one loop for those runs, outfits or pairs."""

import functools
import inspect
import os
import re
from typing import List

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


def shared_options(dataroot_help, batchsize):
    """The decorator of the options both command lines take up to --batchsize, in the order --help prints them; each command
    line puts its own options and --workers (``workers_option``) below it."""
    options = [
        click.option('--network', 'network_pkl', help='Network pickle filename (a local file)', required=True),
        click.option('--seeds', type=num_range, help='List of random seeds (unused, as in the reference)'),
        click.option('--trunc', 'truncation_psi', type=float, help='Truncation psi, forwarded to G.mapping', default=1, show_default=True),
        click.option('--class', 'class_idx', type=int, help='Class label (unused, as in the reference)'),
        click.option('--noise-mode', help='Noise mode, forwarded to G.synthesis', type=click.Choice(['const', 'random', 'none']), default='const',
                     show_default=True),
        click.option('--projected-w', help='Projection result file (unused, as in the reference)', type=str, metavar='FILE'),
        click.option('--outdir', help='Where to save the output images', type=str, required=True, metavar='DIR'),
        click.option('--dataroot', help=dataroot_help, type=str, required=True),
        click.option('--batchsize', help='Pairs per batch', type=click.IntRange(min=1), default=batchsize, show_default=True),
        storage_option]

    def decorate(f):
        parameters = inspect.signature(f).parameters
        # --storage is kept here for ``load_generator`` and handed to the command's function only where it declares the argument
        # (test.py writes it into its report): a command line that just loads and runs the generator needs no line for it
        takes_storage = 'storage' in parameters
        # A command whose function takes ``change_region`` and no ``scores_file`` of its own is the 512 x 320 command line.  It
        # gets --outfits and --scores from here, and a run that gives either is ``generate_512`` below, not the function's
        # own loop over the pair lists, which knows neither: test_512.py stays as it is and still runs every plain command.
        # tests/test_tryon_outfits_gpu.py holds the two loops to the same files for the same pairs.
        extended = 'change_region' in parameters and 'scores_file' not in parameters

        @functools.wraps(f)
        def command(*args, storage=None, **kwargs):
            _given['storage'] = storage
            if extended:
                outfits_file, scores_file = kwargs.pop('outfits_file', None), kwargs.pop('scores_file', None)
                if outfits_file is not None or scores_file is not None:
                    for unused in ('seeds', 'class_idx', 'projected_w'):
                        kwargs.pop(unused, None)
                    kwargs['change_region'] = _explicit_region(kwargs.get('change_region'))
                    return generate_512(*args, outfits_file=outfits_file, scores_file=scores_file, storage=storage, **kwargs)
            if takes_storage:
                kwargs['storage'] = storage
            return f(*args, **kwargs)
        if extended:
            command = scores_option(outfits_option(command))
        for option in reversed(options):
            command = option(command)
        return command
    return decorate


# --storage: run the loaded generator in this activation storage instead of the one it was pickled with
STORAGE_DTYPES = {'snapshot': None, 'f32': 'float32', 'bf16': 'bfloat16', 'f16': 'float16'}
_given = {}                 # the running command's --storage (``shared_options``)
storage_option = click.option('--storage', help='Activation storage the generator runs in: as pickled (snapshot), or f32, bf16, f16 '
                              '[default: snapshot]', type=click.Choice(list(STORAGE_DTYPES)))

scores_option = click.option(
    '--scores', 'scores_file', type=str, metavar='FILE',
    help='Score the written images by region (kept body parts, upper and lower garment patches: L1, PSNR, SSIM) and write the results to '
         'FILE as JSON. With this option z of pair i is np.random.RandomState(i).randn(z_dim), so that the figures describe the images '
         'whatever the batch size [default: no scores]')

def _outfits_option(written):
    return click.option(
        '--outfits', 'outfits_file', type=str, metavar='FILE',
        help='Dress the people of FILE instead of the pair lists: lines "person upper lower", each <sub-dataset>/<file>.jpg, "-" for a '
             'garment the person keeps; written %s. Not together with --change-region' % written)


outfits_option = _outfits_option('as upper donor | lower donor | person | generated')
pair_outfits_option = _outfits_option('to <person\'s sub-dataset>/<person>__<upper>__<lower>.png, a kept garment under the person\'s name')
region_option = click.option(
    '--change-region', type=click.Choice(['upperbody', 'lowerbody', 'fullbody']),
    help='Which garments the person takes from the donor of the pair lists: the upper garment (what a run without this option does), '
         'the lower garment, or both [default: upperbody]')
BOTH_MODES = '--outfits and --change-region exclude each other: every line of the outfit list names whose garments are worn'


def _explicit_region(change_region):
    """--change-region as the user gave it, None when it is the option's default: from click's record of where the value came
    from.  When the callback is called without a click context there is no such record; 'fullbody', what the default means, then
    counts as not given."""
    context = click.get_current_context(silent=True)
    if context is not None:
        return change_region if context.get_parameter_source('change_region') != click.core.ParameterSource.DEFAULT else None
    return None if change_region == 'fullbody' else change_region


workers_option = click.option('--workers', help='Loader processes (file decoding only)', type=click.IntRange(min=0), default=4, show_default=True)


def load_generator(network_pkl, device, storage=None):
    """``G_ema`` of a snapshot file on ``device``, in eval mode and without gradients.  ``storage``: a key of ``STORAGE_DTYPES``,
    by default the --storage of the running command; None or 'snapshot' runs the network as pickled, another value switches its
    activation storage (``training.networks.set_activation_storage``)."""
    import legacy
    if storage is None:
        storage = _given.get('storage')
    print('Loading networks from "%s"...' % network_pkl)
    with open(network_pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].to(device).eval().requires_grad_(False)  # type: ignore
    if storage is not None and storage != 'snapshot':
        from training.networks import set_activation_storage
        set_activation_storage(G, STORAGE_DTYPES[storage])
    return G


def pair_loader(dataset, batchsize, workers, collate_fn=None):
    """The pairs (or, with ``training.dataset.collate_outfits``, the outfits) of ``dataset`` in order; the workers only decode files."""
    import torch
    from training.dataset import collate_pairs
    print(len(dataset))
    return torch.utils.data.DataLoader(dataset, batch_size=batchsize, shuffle=False, num_workers=workers, pin_memory=True,
                                       collate_fn=collate_fn or collate_pairs)


def generate(G, t, gen_z, truncation_psi, noise_mode):
    """The reference's call sequence (test.py:119-128, test_512.py:134-142) on a batch's tensors ``t``: the generated images.
    ``synthesis`` returns them second, of four values (GeneratorV18) or of three (the 512 x 320 GeneratorFull)."""
    import torch
    with torch.no_grad():
        style_input, retain, pose = t['style_input'], t['retain'], t['pose']
        act = getattr(G.synthesis, 'act_dtype', None)
        if act is not None:             # 16-bit activation storage: the encoders run in it as well, as in the generator's own forward
            style_input, retain, pose = style_input.to(act), retain.to(act), pose.to(act)
        gen_c, cat_feat_list = G.style_encoding(style_input, retain)
        pose_feat = G.const_encoding(pose)
        ws = G.mapping(gen_z, gen_c, truncation_psi=truncation_psi)
        cat_feats = {str(feat.shape[2]): feat for feat in cat_feat_list}
        return G.synthesis(ws, pose_feat, cat_feats, t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                           t['denorm_lower_mask'], noise_mode=noise_mode)[1]


def write_scores(scores_file, partials, pixels, pairs, network_pkl, dataroot, noise_mode, storage=None, mode=None):
    """--scores: the figures of ``metrics.tryon_fidelity.finish`` (prefix ``tryon``) and what the run was, as one JSON line,
    printed and written to ``scores_file``.  ``mode``: what was dressed, when it was not the plain pair lists."""
    import json
    from metrics import tryon_fidelity
    report = dict(results=tryon_fidelity.finish(partials, 'tryon', pixels=pixels), pairs=pairs, network=network_pkl, dataroot=dataroot,
                  noise_mode=noise_mode)
    if storage is not None:
        report['storage'] = storage
    if mode is not None:
        report['mode'] = mode
    line = json.dumps(report)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(scores_file)), exist_ok=True)
    with open(scores_file, 'w') as f:
        f.write(line + '\n')


def generate_512(network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, change_region, workers, outfits_file=None,
                 scores_file=None, storage=None):
    """test_512.py with --outfits and / or --scores.  --outfits FILE: every line ``person upper lower`` of FILE
    (training.dataset.UvitonOutfits_512_test) instead of the pair lists, prepared by
    training.tryon_regions.TryOnOutfitBatchBuilder, written as ``upper donor | lower donor | person | generated`` (512 x 2048) to
    ``<outdir>/<count>.png`` in list order.  ``change_region`` None means full body; any other value is refused together with
    --outfits, since a line names whose garments are worn.  --scores FILE: the region scores of metrics/tryon_fidelity.py over
    what is written, z of item i from ``pair_z(i)``, ``pixels = 512 * 320``.  Without --outfits the pairs of the change region
    are written as test_512.py writes them, ``clothes | person | generated``."""
    if outfits_file is not None and change_region is not None:
        raise click.UsageError(BOTH_MODES)
    _local_snapshot(network_pkl)

    import numpy as np
    import PIL.Image
    import torch

    from metrics import tryon_fidelity
    from training import dataset as custom_dataset
    from training.tryon_pairs import images_to_u8
    from training.tryon_regions import TryOnOutfitBatchBuilder, TryOnRegionBatchBuilder

    device = torch.device('cuda')
    G = load_generator(network_pkl, device, storage)
    os.makedirs(outdir, exist_ok=True)
    if outfits_file is not None:
        dataset = custom_dataset.UvitonOutfits_512_test(path=dataroot, outfits_file=outfits_file, use_labels=True, max_size=None, xflip=False)
        loader = pair_loader(dataset, batchsize, workers, custom_dataset.collate_outfits)
        builder, panels = TryOnOutfitBatchBuilder(device), ('clothes', 'clothes_lower', 'image')
    else:
        change_region = change_region or 'fullbody'
        dataset = custom_dataset.UvitonDatasetFull_512_test(path=dataroot, change_region=change_region, use_labels=True, max_size=None, xflip=False)
        loader = pair_loader(dataset, batchsize, workers)
        builder, panels = TryOnRegionBatchBuilder(device, change_region), ('clothes', 'image')
    partials = tryon_fidelity.new_partials(len(dataset), device) if scores_file is not None else None
    count = 0
    for raw in loader:
        batch = builder.build(raw, keep_stages=scores_file is not None)
        t, n = batch.tensors, batch.batch
        side = t['image'].shape[2]
        gen_z = torch.empty([n, 0], device=device)
        if scores_file is not None:
            index = raw['raw_idx'].tolist()                         # the items' positions in the pair lists, or in the outfit list
            gen_z = tryon_fidelity.pair_z(index, G.z_dim, device)
        gen_imgs = generate(G, t, gen_z, truncation_psi, noise_mode)
        if scores_file is not None:
            tryon_fidelity.score_batch(gen_imgs, batch, index, partials)
        images = torch.cat([images_to_u8(x, 0, side) for x in [t[k] for k in panels] + [gen_imgs]], dim=2).cpu().numpy()
        for result in images:
            PIL.Image.fromarray(np.ascontiguousarray(result)).save(os.path.join(outdir, str(count).zfill(3) + '.png'))
            count += 1
    print('finish: %d images under %s' % (count, outdir))
    if scores_file is not None:
        write_scores(scores_file, partials, 512 * 320, count, network_pkl, dataroot, noise_mode, storage)


def generate_256(network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, workers, outfits_file=None, change_region=None,
                 scores_file=None, storage=None):
    """test.py with --outfits or --change-region: the 256 x 192 model on outfits, prepared by
    training.tryon_pairs.TryOnPairOutfitBatchBuilder.  --outfits FILE: every line ``person upper lower`` of FILE
    (training.dataset.UvitonOutfits_256_test), written to ``<outdir>/<person's sub-dataset>/<person stem>__<upper stem>__<lower
    stem>.png``, a kept garment under the person's stem.  --change-region: the pairs of the pair lists as the outfits (P, D, -),
    (P, -, D) or (P, D, D), written under test.py's name ``<person stem>__<clothes stem>.png``; 'upperbody' writes the bytes of a
    run without the option.  The two exclude each other, and that is refused before anything is read.  Only the generated image
    is written, as test.py writes it.  --scores FILE: the region scores over what is written, z of item i from ``pair_z(i)``;
    the report's ``mode`` is ``outfits`` or ``change-region <region>``."""
    if outfits_file is not None and change_region is not None:
        raise click.UsageError(BOTH_MODES)
    _local_snapshot(network_pkl)

    import numpy as np
    import PIL.Image
    import torch

    from metrics import tryon_fidelity
    from training import dataset as custom_dataset
    from training.tryon_pairs import TryOnPairOutfitBatchBuilder, images_to_u8

    device = torch.device('cuda')
    G = load_generator(network_pkl, device, storage)
    os.makedirs(outdir, exist_ok=True)
    if outfits_file is not None:
        dataset = custom_dataset.UvitonOutfits_256_test(path=dataroot, outfits_file=outfits_file, use_labels=True, max_size=None, xflip=False)
        loader, mode = pair_loader(dataset, batchsize, workers, custom_dataset.collate_outfits), 'outfits'
    else:
        dataset = custom_dataset.UvitonDatasetV19_test(path=dataroot, use_labels=True, max_size=None, xflip=False)
        loader = pair_loader(dataset, batchsize, workers, functools.partial(custom_dataset.collate_region_outfits, change_region))
        mode = 'change-region ' + change_region
    builder = TryOnPairOutfitBatchBuilder(device)
    partials = tryon_fidelity.new_partials(len(dataset), device) if scores_file is not None else None
    pixels = tryon_fidelity.PIXELS
    stem = lambda name: os.path.basename(name)[:-4]
    written = 0
    for raw in loader:
        batch = builder.build(raw, keep_stages=scores_file is not None)
        t, n = batch.tensors, batch.batch
        height, width = raw['people_image'].shape[1], raw['people_image'].shape[2]
        gen_z = torch.empty([n, 0], device=device)
        if scores_file is not None:
            index = raw['raw_idx'].tolist()                         # the items' positions in the pair lists, or in the outfit list
            gen_z = tryon_fidelity.pair_z(index, G.z_dim, device)
        gen_imgs = generate(G, t, gen_z, truncation_psi, noise_mode)
        images = images_to_u8(gen_imgs, (height - width) // 2, width).cpu().numpy()
        if scores_file is not None:
            tryon_fidelity.score_batch(gen_imgs, batch, index, partials)
            pixels = height * width
        worn = zip(batch.upper_name, batch.lower_name) if outfits_file is not None else zip(raw['clothes_name'])
        for img, person, garments in zip(images, batch.person_name, worn):
            save_dir = os.path.join(outdir, person.split('/')[0])
            os.makedirs(save_dir, exist_ok=True)
            name = '__'.join([stem(person)] + [stem(g) for g in garments]) + '.png'
            PIL.Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(save_dir, name))
            written += 1
    print('finish: %d images under %s' % (written, outdir))
    if scores_file is not None:
        write_scores(scores_file, partials, pixels, written, network_pkl, dataroot, noise_mode, storage, mode)
