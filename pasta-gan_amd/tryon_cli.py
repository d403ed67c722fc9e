"""What the two try-on command lines, test.py and test_512.py, share (and, of the options, the training and scoring command lines:
--storage, --erase-masks, --erase-strokes): the options the reference declares and this project's own
(each command line lists its options itself, in the order --help prints them), the refusal of a snapshot that is not a local
file, loading ``G_ema``, the loader over a test data set, the generator's call sequence, the --scores report, and the ONE loop
that dresses a data set (``dress``): build, z, generate, score, convert, write.

Every run dresses OUTFITS.  ``generate_256`` (test.py) and ``generate_512`` (test_512.py) choose the data set, the collate
function, the builder and how an item is written; pair lists become the outfits of the change region in the loader's workers
(``training.dataset.collate_region_outfits``), where a person named twice in a batch is stacked, uploaded and solved once."""

import functools
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
    """The decorator of the options both command lines take up to --storage, --png-encoder, the two --kept options, --background,
    --kept-garments, --part-geometry, --fit-people and --fit-filter, in the order --help prints them; each command line puts its own options and --workers (``workers_option``) below it."""
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
        storage_option, png_encoder_option, kept_parts_option, kept_feather_option, background_option, kept_garments_option,
        part_geometry_option, fit_people_option, fit_filter_option]

    def decorate(f):
        for option in reversed(options):
            f = option(f)
        return f
    return decorate


# --storage: run the loaded generator in this activation storage instead of the one it was pickled with
STORAGE_DTYPES = {'snapshot': None, 'f32': 'float32', 'bf16': 'bfloat16', 'f16': 'float16'}
storage_option = click.option('--storage', help='Activation storage the generator runs in: as pickled (snapshot), or f32, bf16, f16 '
                              '[default: snapshot]', type=click.Choice(list(STORAGE_DTYPES)))

# --erase-masks, --erase-strokes: where a training item's erase mask comes from.  train_wo_flow_fullbody.py records
# them with the run; calc_metrics.py's default is what the snapshot recorded.  ``erase_options`` decorates both commands.
ERASE_STROKES_HELP = ('With --erase-masks strokes: comma-separated strokes=1..8, vertices=1..8, length=0.01..0.5, width=0.01..0.25 '
                      '(of the square\'s side), turn=0..180 (degrees) [default: strokes=6,vertices=6,length=0.25,width=0.12,turn=60]')


def erase_options(erase_masks_default):
    options = [
        click.option('--erase-masks', help='Erase masks: the files of train_random_mask_acgpn, none, or strokes drawn on the GPU '
                     '[default: %s]' % erase_masks_default, type=click.Choice(['files', 'none', 'strokes'])),
        click.option('--erase-strokes', help=ERASE_STROKES_HELP, metavar='SPEC')]

    def decorate(f):
        for option in reversed(options):
            f = option(f)
        return f
    return decorate


def parse_name_values(text):
    """``name=value,name=value`` -> a dict of floats; a ValueError names what is not name=value, a name given twice or a value
    that is no number."""
    spec = {}
    for pair in text.split(','):
        name, eq, value = pair.partition('=')
        name = name.strip()
        if not eq or not name:
            raise ValueError(f'{pair!r} is not name=value')
        if name in spec:
            raise ValueError(f'{name} is given twice')
        try:
            spec[name] = float(value)
        except ValueError:
            raise ValueError(f'{name}={value.strip()} is not a number')
    return spec


def erase_mask_kwargs(erase_masks, erase_strokes):
    """``--erase-masks`` and ``--erase-strokes`` (None where not given) -> the keyword arguments they add to the training data set:
    none for ``files``, so that such a run records what it always did.  A ValueError carries the option's name."""
    from training.tryon_batch import strokes_spec
    erase_masks = 'files' if erase_masks is None else erase_masks
    if erase_strokes is not None and erase_masks != 'strokes':
        raise ValueError(f'--erase-strokes needs --erase-masks strokes (it is {erase_masks})')
    if erase_masks == 'files':
        return {}
    if erase_masks == 'none':
        return dict(erase_masks='none')
    try:
        spec = strokes_spec(parse_name_values(erase_strokes) if erase_strokes is not None else {})
    except ValueError as err:
        raise ValueError(f'--erase-strokes: {err}')
    return dict(erase_masks='strokes', erase_strokes=spec)


# --png-encoder: who turns the uint8 batch into PNG files: PIL in this process, one image at a time, or the GPU.  The
# option comes with ``shared_options`` and hands the commands' callbacks no argument: its value is recorded in the click context,
# where ``generate_256`` and ``generate_512`` find it (``_chosen_encoder``), as ``_explicit_region`` finds where a region came from.
_ENCODER_KEY = 'pasta.png_encoder'


def _record_encoder(context, param, value):
    context.meta[_ENCODER_KEY] = value
    return value


png_encoder_option = click.option('--png-encoder', help='Who encodes the PNG files: PIL on the host, one image at a time, or the GPU, a batch '
                                  'at a time (torch_utils/ops/png_encode.py; the same pixels in larger files)',
                                  type=click.Choice(['pil', 'gpu']), default='pil', show_default=True, expose_value=False,
                                  callback=_record_encoder)


def _chosen_encoder(png_encoder):
    """The ``png_encoder`` keyword of ``generate_256`` / ``generate_512``; left at 'pil' under a running command line, it is what
    that command line's --png-encoder said.  A call without a click context has only the keyword."""
    context = click.get_current_context(silent=True)
    if png_encoder == 'pil' and context is not None:
        return context.meta.get(_ENCODER_KEY, png_encoder)
    return png_encoder


# --part-geometry: where the body parts' quadrilaterals, 8 x 8 systems and inverses are solved: numpy on the host, one
# part at a time, or one launch per batch (training.patch_pipeline.part_geometry), a second rule that prepares almost exactly the
# same bytes.  Recorded in the click context like --png-encoder; train_wo_flow_fullbody.py declares its own option of this name.
_GEOMETRY_KEY = 'pasta.part_geometry'
PART_GEOMETRY_HELP = ('Where the body-part matrices are solved: numpy on the host, or one launch per batch on the GPU (almost exactly the '
                      'same bytes: DESIGN 8n)')


def _record_geometry(context, param, value):
    context.meta[_GEOMETRY_KEY] = value
    return value


part_geometry_option = click.option('--part-geometry', help=PART_GEOMETRY_HELP, type=click.Choice(['host', 'gpu']), default='host',
                                    show_default=True, expose_value=False, callback=_record_geometry)


def _chosen_geometry(part_geometry):
    """The ``part_geometry`` keyword of ``generate_256`` / ``generate_512``; left at 'host' under a running command line, it is what
    that command line's --part-geometry said (``_chosen_encoder``)."""
    context = click.get_current_context(silent=True)
    if part_geometry == 'host' and context is not None:
        return context.meta.get(_GEOMETRY_KEY, part_geometry)
    return part_geometry


def _record(key):
    def record(context, param, value):
        context.meta[key] = value
        return value
    return record


# --fit-people pad | crop, --fit-filter bilinear | box: photographs of any size, fitted to the model's canvas per batch on the GPU
# (training.tryon_batch.fit_batch; include/pasta_hip.h has the rule).  Arguments of the data set.  test.py and
# test_512.py get them with ``shared_options``, recorded in the click context like --png-encoder; train_wo_flow_fullbody.py and
# calc_metrics.py declare them with ``fit_options`` and take their values.
_FIT_KEY, _FIT_FILTER_KEY = 'pasta.fit_people', 'pasta.fit_filter'
FIT_PEOPLE_HELP = ('Take photographs of any size: fit each to the canvas on the GPU, padded to show all of it or centre-cropped to fill the '
                   'canvas [default: %s]')
FIT_FILTER_HELP = 'With --fit-people: how the photographs are resampled, as PIL\'s BILINEAR or BOX [default: %s]'


def fit_options(fit_default='none: every photograph has the canvas size', filter_default='bilinear'):
    options = [click.option('--fit-people', help=FIT_PEOPLE_HELP % fit_default, type=click.Choice(['pad', 'crop'])),
               click.option('--fit-filter', help=FIT_FILTER_HELP % filter_default, type=click.Choice(['bilinear', 'box']))]

    def decorate(f):
        for option in reversed(options):
            f = option(f)
        return f
    return decorate


def fit_kwargs(fit_people, fit_filter):
    """``--fit-people`` and ``--fit-filter`` (None where not given) -> the keyword arguments they add to a data set: none without
    --fit-people, so that such a run records what it always did.  A ValueError carries the option's name."""
    if fit_people is None:
        if fit_filter is not None:
            raise ValueError('--fit-filter needs --fit-people pad or crop')
        return {}
    from training.tryon_batch import fit_check
    try:
        mode, filter = fit_check(fit_people, 'bilinear' if fit_filter is None else fit_filter)
    except ValueError as err:
        raise ValueError(f'--fit-people / --fit-filter: {err}')
    return dict(fit=mode, fit_filter=filter)


fit_people_option = click.option('--fit-people', help=FIT_PEOPLE_HELP % 'none: every photograph has the canvas size',
                                 type=click.Choice(['pad', 'crop']), expose_value=False, callback=_record(_FIT_KEY))
fit_filter_option = click.option('--fit-filter', help=FIT_FILTER_HELP % 'bilinear', type=click.Choice(['bilinear', 'box']), expose_value=False,
                                 callback=_record(_FIT_FILTER_KEY))


def _chosen_fit(fit_people, fit_filter):
    """The data set's ``fit`` keywords of ``generate_256`` / ``generate_512`` (``fit_kwargs``); keywords both left at None under a
    running command line are what that command line's options said (``_chosen_encoder``)."""
    context = click.get_current_context(silent=True)
    if fit_people is None and fit_filter is None and context is not None:
        fit_people, fit_filter = context.meta.get(_FIT_KEY), context.meta.get(_FIT_FILTER_KEY)
    try:
        return fit_kwargs(fit_people, fit_filter)
    except ValueError as err:
        raise click.UsageError(str(err))


def canvas_of(raw):
    """(height, width) of the people of a batch of ``collate_outfits``: the stack's, or a packed batch's canvas."""
    if 'fit' in raw:
        return tuple(int(v) for v in raw['fit']['canvas'])
    return int(raw['people_image'].shape[1]), int(raw['people_image'].shape[2])


# --kept-parts photo: the photograph's head, palms and shoes (metrics.tryon_fidelity.keep_mask, the region `retain` carries) are
# pasted into the generated picture where its bytes are made (training.tryon_pairs.images_keep_to_u8), feathered over
# --kept-feather pixels.  Both options come with ``shared_options`` and, like --png-encoder, hand the commands' callbacks no
# argument (test.py and test_512.py are untouched): their values are recorded in the click context, where ``_paste_plan`` finds
# them when the keywords ``kept_parts`` / ``kept_feather`` of ``generate_256`` / ``generate_512`` are left at their defaults.
_KEPT_PARTS_KEY, _KEPT_FEATHER_KEY = 'pasta.kept_parts', 'pasta.kept_feather'
KEPT_PARTS = ('generated', 'photo')
KEPT_FEATHER_DEFAULT = 2            # the 5 x 5 window of the project's erosions
KEPT_FEATHER_MAX = 8


kept_parts_option = click.option('--kept-parts', help='Where the written head, palms and shoes come from: the generator, or the person\'s '
                                 'photograph, pasted in on the GPU', type=click.Choice(list(KEPT_PARTS)), default='generated', show_default=True,
                                 expose_value=False, callback=_record(_KEPT_PARTS_KEY))
kept_feather_option = click.option('--kept-feather', help='With --kept-parts, --background or --kept-garments photo: the paste fades over R '
                                   'pixels inside the pasted region, 0 for a hard edge [default: %d]' % KEPT_FEATHER_DEFAULT,
                                   type=click.IntRange(0, KEPT_FEATHER_MAX), metavar='R', expose_value=False, callback=_record(_KEPT_FEATHER_KEY))

# --background photo and --kept-garments photo widen the pasted region: the photograph's background, and the garment(s)
# of the person's own that an item's outfit keeps, each only where the generator's own region heads agree with the photograph's
# label map (training.tryon_pairs.photo_paste_mask).  Recorded in the click context as the --kept options are; the keywords are
# ``background`` / ``kept_garments`` of ``generate_256`` / ``generate_512``.
_BACKGROUND_KEY, _KEPT_GARMENTS_KEY = 'pasta.background', 'pasta.kept_garments'
PASTE_OPTIONS = ('kept_parts', 'background', 'kept_garments')      # by keyword; the options are --kept-parts, --background, --kept-garments
background_option = click.option('--background', help='Where the written background comes from: the generator, or the person\'s photograph '
                                 'where the generator claims neither garment nor skin, pasted in on the GPU', type=click.Choice(list(KEPT_PARTS)),
                                 default='generated', show_default=True, expose_value=False, callback=_record(_BACKGROUND_KEY))
kept_garments_option = click.option('--kept-garments', help='Where a garment the outfit does not change comes from: the generator, or the '
                                    'person\'s photograph where the generator puts that garment, pasted in on the GPU',
                                    type=click.Choice(list(KEPT_PARTS)), default='generated', show_default=True, expose_value=False,
                                    callback=_record(_KEPT_GARMENTS_KEY))


def _paste_plan(kept_parts, kept_feather, background='generated', kept_garments='generated'):
    """(feather radius, the PASTE_OPTIONS that are 'photo') of a run; (None, ()) for a run that writes the generator's own
    pixels.  A feather without any paste is a usage error; the two generate functions raise it before anything is read.  Keywords
    all left at their defaults ('generated', None) under a running command line are what that command line's options said; a call
    without a click context has only the keywords."""
    context = click.get_current_context(silent=True)
    if context is not None and kept_parts == background == kept_garments == 'generated' and kept_feather is None:
        kept_parts = context.meta.get(_KEPT_PARTS_KEY, kept_parts)
        kept_feather = context.meta.get(_KEPT_FEATHER_KEY, kept_feather)
        background = context.meta.get(_BACKGROUND_KEY, background)
        kept_garments = context.meta.get(_KEPT_GARMENTS_KEY, kept_garments)
    chosen = dict(kept_parts=kept_parts, background=background, kept_garments=kept_garments)
    for name, value in chosen.items():
        if value not in KEPT_PARTS:
            raise click.BadParameter('%r is not one of %s' % (value, ', '.join(KEPT_PARTS)), param_hint='--' + name.replace('_', '-'))
    if kept_feather is not None and (isinstance(kept_feather, bool) or not isinstance(kept_feather, int)
                                     or not 0 <= kept_feather <= KEPT_FEATHER_MAX):
        raise click.BadParameter('%r is not an integer 0..%d' % (kept_feather, KEPT_FEATHER_MAX), param_hint='--kept-feather')
    pasted = tuple(name for name in PASTE_OPTIONS if chosen[name] == 'photo')
    if not pasted:
        if kept_feather is not None:
            raise click.UsageError('--kept-feather needs --kept-parts photo, --background photo or --kept-garments photo: '
                                   'without one of them nothing is pasted')
        return None, ()
    return (KEPT_FEATHER_DEFAULT if kept_feather is None else kept_feather), pasted


def _kept_radius(kept_parts, kept_feather, background='generated', kept_garments='generated'):
    """The feather radius of a run that pastes from the photograph, None for one that does not (``_paste_plan``)."""
    return _paste_plan(kept_parts, kept_feather, background, kept_garments)[0]


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
    the command's --storage; None or 'snapshot' runs the network as pickled, another value switches its activation storage
    (``training.networks.set_activation_storage``)."""
    import legacy
    print('Loading networks from "%s"...' % network_pkl)
    with open(network_pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].to(device).eval().requires_grad_(False)  # type: ignore
    if storage is not None and storage != 'snapshot':
        from training.networks import set_activation_storage
        set_activation_storage(G, STORAGE_DTYPES[storage])
    return G


def pair_loader(dataset, batchsize, workers, collate_fn):
    """The items of ``dataset`` in order, collated by ``collate_fn`` (``training.dataset.collate_outfits``, or
    ``collate_region_outfits`` for a pair list); the workers only decode files and stack."""
    import torch
    print(len(dataset))
    return torch.utils.data.DataLoader(dataset, batch_size=batchsize, shuffle=False, num_workers=workers, pin_memory=True,
                                       collate_fn=collate_fn)


def generate_outputs(G, t, gen_z, truncation_psi, noise_mode):
    """The reference's call sequence (test.py:119-128, test_512.py:134-142) on a batch's tensors ``t``: everything ``synthesis``
    returns.  The generated images are second, of four values (GeneratorV18: then the two sigmoid garment heads) or of three
    (the 512 x 320 GeneratorFull: then the six parsing logits)."""
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
                           t['denorm_lower_mask'], noise_mode=noise_mode)


def generate(G, t, gen_z, truncation_psi, noise_mode):
    """The generated images of ``generate_outputs``: same launches, same value."""
    return generate_outputs(G, t, gen_z, truncation_psi, noise_mode)[1]


def write_scores(scores_file, partials, pixels, pairs, network_pkl, dataroot, noise_mode, storage=None, mode=None, kept_radius=None,
                 pasted=('kept_parts',), part_geometry='host', fit=None):
    """--scores: the figures of ``metrics.tryon_fidelity.finish`` (prefix ``tryon``) and what the run was, as one JSON line,
    printed and written to ``scores_file``.  ``mode``: what was dressed, when it was not the plain pair lists; ``kept_radius``:
    the feather of a run that pastes from the photograph, whose report says so and names each of ``pasted`` (PASTE_OPTIONS);
    ``part_geometry``: named in the report only when it is not the host's; ``fit``: the data set's fit keywords (``fit_kwargs``),
    named as ``fit_people`` and ``fit_filter`` when the run had the option."""
    import json
    from metrics import tryon_fidelity
    report = dict(results=tryon_fidelity.finish(partials, 'tryon', pixels=pixels), pairs=pairs, network=network_pkl, dataroot=dataroot,
                  noise_mode=noise_mode)
    if storage is not None:
        report['storage'] = storage
    if mode is not None:
        report['mode'] = mode
    if kept_radius is not None:
        report.update([(name, 'photo') for name in pasted if name == 'kept_parts'], kept_feather=kept_radius)
        report.update((name, 'photo') for name in pasted if name != 'kept_parts')
    if part_geometry != 'host':
        report['part_geometry'] = part_geometry
    if fit:
        report.update(fit_people=fit['fit'], fit_filter=fit['fit_filter'])
    line = json.dumps(report)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(scores_file)), exist_ok=True)
    with open(scores_file, 'w') as f:
        f.write(line + '\n')


def dress(choose, network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, workers, scores_file, storage, mode=None,
          kept_radius=None, pasted=('kept_parts',), part_geometry='host', fit=None, png_encoder='pil'):
    """The loop of both command lines.  ``choose(device)`` -> (data set, collate function, builder, ``pictures``), called once the
    snapshot is loaded; ``pictures(batch, raw, gen_imgs, count, content)`` -> (uint8 [N, h, w, 3] on the GPU, the N file names
    under ``outdir``): what is written for the items of a batch, ``count`` items having been written before it.  --scores FILE: z of
    item i is ``pair_z(i)`` and the region scores of metrics/tryon_fidelity.py over what is written go to FILE (``write_scores``).
    ``kept_radius`` (``_paste_plan``; None: the generator's own pixels, and ``content`` is None): the batches keep their stages,
    and ``content``, uint8 [N, H, W, 3], is the generated picture's content columns with the photograph pasted in by
    ``images_keep_to_u8`` over the region of ``pasted`` (PASTE_OPTIONS: the kept parts, the background, the person's own
    garments), which ``photo_paste_mask`` forms once per batch from the builder's stages, ``paste_rules`` and, for the last two,
    the generator's own region heads; with the kept parts alone it is ``tryon_fidelity.keep_mask``.  The scores are
    then those of these bytes, handed to
    ``score_batch`` as the centres (b + 0.5) / 127.5 - 1 of the bytes' intervals, which ``unit_to_u8`` returns to b.
    ``png_encoder``: 'pil' copies the batch to the host and saves image by image; 'gpu' encodes the batch where it is
    (torch_utils.ops.png_encode.save) and copies back the compressed bytes.  Names, layout and scores are settled before either.
    ``part_geometry``: 'host' or 'gpu', handed to ``choose(device, part_geometry)`` for its builder and named in the scores report
    when 'gpu'."""
    _local_snapshot(network_pkl)
    if png_encoder not in ('pil', 'gpu'):
        raise click.BadParameter('%r is not one of pil, gpu' % (png_encoder,), param_hint='--png-encoder')
    if part_geometry not in ('host', 'gpu'):
        raise click.BadParameter('%r is not one of host, gpu' % (part_geometry,), param_hint='--part-geometry')

    import numpy as np
    import PIL.Image
    import torch

    from metrics import tryon_fidelity
    from torch_utils.ops import png_encode
    from training.tryon_pairs import images_keep_to_u8, paste_rules, photo_paste_mask

    device = torch.device('cuda')
    G = load_generator(network_pkl, device, storage)
    os.makedirs(outdir, exist_ok=True)
    dataset, collate_fn, builder, pictures = choose(device, part_geometry)
    loader = pair_loader(dataset, batchsize, workers, collate_fn)
    scoring = scores_file is not None
    partials = tryon_fidelity.new_partials(len(dataset), device) if scoring else None
    pixels = tryon_fidelity.PIXELS                                  # content pixels of an item; every batch brings its own
    count = 0
    for raw in loader:
        batch = builder.build(raw, keep_stages=scoring or kept_radius is not None)
        gen_z = torch.empty([batch.batch, 0], device=device)
        if scoring:
            index = raw['raw_idx'].tolist()                         # the items' positions in the pair lists, or in the outfit list
            gen_z = tryon_fidelity.pair_z(index, G.z_dim, device)
        _, gen_imgs, *heads = generate_outputs(G, batch.tensors, gen_z, truncation_psi, noise_mode)
        content, scored = None, gen_imgs
        if kept_radius is not None:
            photo = batch.stages['image']
            c0, width = (photo.shape[1] - photo.shape[2]) // 2, photo.shape[2]
            rule = paste_rules('kept_parts' in pasted, 'background' in pasted, 'kept_garments' in pasted, raw['person_idx'], raw['upper_idx'],
                               raw['lower_idx'], int(photo.shape[1])).to(device)
            region = photo_paste_mask(batch.stages['parsing'], batch.stages['palm'] if 'kept_parts' in pasted else None, rule,
                                      heads if pasted != ('kept_parts',) else (), c0)       # the kept parts need no statement
            content = images_keep_to_u8(gen_imgs, c0, width, photo, region, kept_radius)
            if scoring:
                scored = gen_imgs.to(torch.float32).clone()
                scored[:, :, :, c0:c0 + width] = ((content.to(torch.float32) + 0.5) / 127.5 - 1).permute(0, 3, 1, 2)
        if scoring:
            tryon_fidelity.score_batch(scored, batch, index, partials)
            pixels = canvas_of(raw)[0] * canvas_of(raw)[1]
        images, names = pictures(batch, raw, gen_imgs, count, content)
        if png_encoder == 'gpu':
            png_encode.save(images, [os.path.join(outdir, name) for name in names])
            count += len(names)
            continue
        for img, name in zip(images.cpu().numpy(), names):
            os.makedirs(os.path.dirname(os.path.join(outdir, name)), exist_ok=True)
            PIL.Image.fromarray(np.ascontiguousarray(img)).save(os.path.join(outdir, name))
            count += 1
    print('finish: %d images under %s' % (count, outdir))
    if scoring:
        write_scores(scores_file, partials, pixels, count, network_pkl, dataroot, noise_mode, storage, mode, kept_radius, pasted, part_geometry, fit)


def generate_512(network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, change_region, workers, outfits_file=None,
                 scores_file=None, storage=None, kept_parts='generated', kept_feather=None, background='generated',
                 kept_garments='generated', part_geometry='host', fit_people=None, fit_filter=None, png_encoder='pil'):
    """test_512.py: the 512 x 320 model on outfits, prepared by training.tryon_regions.TryOnOutfitBatchBuilder and written to
    ``<outdir>/<count>.png`` in list order.  --outfits FILE: every line ``person upper lower`` of FILE
    (training.dataset.UvitonOutfits_512_test), written as ``upper donor | lower donor | person | generated`` (512 x 2048).
    Without it: the pairs of the pair lists as the outfits of ``change_region`` (None means full body), written as the reference
    writes them, ``clothes | person | generated`` with the DONOR as ``clothes``, who for 'lowerbody' owns the lower garment.
    A ``change_region`` other than None is refused together with --outfits, since a line names whose garments are worn, and that
    is refused before anything is read.  ``kept_parts`` 'photo' with ``kept_feather`` (None: 2): the ``generated`` panel's content
    columns carry the photograph's kept parts (``dress``), the other panels and the panel's padding are untouched; ``background``
    / ``kept_garments`` 'photo' widen the pasted region to the photograph's background and to the garment(s) of the person's own
    that an item keeps; a feather with none of the three is refused like the two modes.  ``png_encoder``: who writes the files (``dress``, ``_chosen_encoder``);
    ``part_geometry``: where the builder solves the body parts (``_chosen_geometry``)."""
    if outfits_file is not None and change_region is not None:
        raise click.UsageError(BOTH_MODES)
    kept_radius, pasted = _paste_plan(kept_parts, kept_feather, background, kept_garments)
    fit = _chosen_fit(fit_people, fit_filter)          # photographs of any size, fitted to the canvas on the GPU

    def choose(device, geometry='host'):
        import torch
        from training import dataset as custom_dataset
        from training.tryon_pairs import images_to_u8
        from training.tryon_regions import TryOnOutfitBatchBuilder
        if outfits_file is not None:
            dataset = custom_dataset.UvitonOutfits_512_test(path=dataroot, outfits_file=outfits_file, use_labels=True, max_size=None, xflip=False, **fit)
            collate_fn, panels = custom_dataset.collate_outfits, ('clothes', 'clothes_lower', 'image')
        else:
            region = change_region or 'fullbody'
            dataset = custom_dataset.UvitonDatasetFull_512_test(path=dataroot, change_region=region, use_labels=True, max_size=None, xflip=False,
                                                                **fit)
            collate_fn = functools.partial(custom_dataset.collate_region_outfits, region)
            panels = ('clothes_lower' if region == 'lowerbody' else 'clothes', 'image')

        def pictures(batch, raw, gen_imgs, count, content):
            t = batch.tensors
            side = t['image'].shape[2]
            images = torch.cat([images_to_u8(x, 0, side) for x in [t[k] for k in panels] + [gen_imgs]], dim=2)
            if content is not None:             # the last panel's content columns; its padding stays the generator's
                c0 = len(panels) * side + (side - content.shape[2]) // 2
                images[:, :, c0:c0 + content.shape[2]] = content
            return images, [str(count + i).zfill(3) + '.png' for i in range(batch.batch)]
        return dataset, collate_fn, TryOnOutfitBatchBuilder(device, geometry=geometry), pictures
    dress(choose, network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, workers, scores_file, storage,
          kept_radius=kept_radius, pasted=pasted, png_encoder=_chosen_encoder(png_encoder), part_geometry=_chosen_geometry(part_geometry), fit=fit)


def generate_256(network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, workers, outfits_file=None, change_region=None,
                 scores_file=None, storage=None, kept_parts='generated', kept_feather=None, background='generated',
                 kept_garments='generated', part_geometry='host', fit_people=None, fit_filter=None, png_encoder='pil'):
    """test.py: the 256 x 192 model on outfits, prepared by training.tryon_pairs.TryOnPairOutfitBatchBuilder; only the generated
    image is written, columns 32..223 of the generator's square.  --outfits FILE: every line ``person upper lower`` of FILE
    (training.dataset.UvitonOutfits_256_test), written to ``<outdir>/<person's sub-dataset>/<person stem>__<upper stem>__<lower
    stem>.png``, a kept garment under the person's stem.  Without it: the pairs of the pair lists as the outfits (P, D, -),
    (P, -, D) or (P, D, D) of ``change_region`` (None: upper body, the reference's run), written to ``<person stem>__<clothes
    stem>.png``.  The two exclude each other, and that is refused before anything is read.  The --scores report's ``mode`` is
    ``outfits`` or ``change-region <region>``; a run with neither option has none.  ``kept_parts`` 'photo' with ``kept_feather``
    (None: 2): the written image carries the photograph's kept parts (``dress``); ``background`` / ``kept_garments`` 'photo' widen
    the pasted region to the photograph's background and to the garment(s) of the person's own that an item keeps; a
    feather with none of the three is refused like the two modes.  ``png_encoder``: who writes the files (``dress``, ``_chosen_encoder``);
    ``part_geometry``: where the builder solves the body parts (``_chosen_geometry``)."""
    if outfits_file is not None and change_region is not None:
        raise click.UsageError(BOTH_MODES)
    kept_radius, pasted = _paste_plan(kept_parts, kept_feather, background, kept_garments)
    fit = _chosen_fit(fit_people, fit_filter)          # photographs of any size, fitted to the canvas on the GPU

    def choose(device, geometry='host'):
        from training import dataset as custom_dataset
        from training.tryon_pairs import TryOnPairOutfitBatchBuilder, images_to_u8
        if outfits_file is not None:
            dataset = custom_dataset.UvitonOutfits_256_test(path=dataroot, outfits_file=outfits_file, use_labels=True, max_size=None, xflip=False, **fit)
            collate_fn, worn = custom_dataset.collate_outfits, ('upper_name', 'lower_name')
        else:
            dataset = custom_dataset.UvitonDatasetV19_test(path=dataroot, use_labels=True, max_size=None, xflip=False, **fit)
            collate_fn, worn = functools.partial(custom_dataset.collate_region_outfits, change_region or 'upperbody'), ('clothes_name',)
        stem = lambda name: os.path.basename(name)[:-4]

        def pictures(batch, raw, gen_imgs, count, content):
            height, width = canvas_of(raw)
            names = [os.path.join(who[0].split('/')[0], '__'.join(stem(name) for name in who) + '.png')
                     for who in zip(raw['person_name'], *[raw[k] for k in worn])]
            return (images_to_u8(gen_imgs, (height - width) // 2, width) if content is None else content), names
        return dataset, collate_fn, TryOnPairOutfitBatchBuilder(device, geometry=geometry), pictures
    mode = 'outfits' if outfits_file is not None else change_region and 'change-region ' + change_region
    dress(choose, network_pkl, truncation_psi, noise_mode, outdir, dataroot, batchsize, workers, scores_file, storage, mode,
          kept_radius=kept_radius, pasted=pasted, png_encoder=_chosen_encoder(png_encoder), part_geometry=_chosen_geometry(part_geometry), fit=fit)
