"""Train PASTA-GAN's full-body model from the command line: the reference's train_wo_flow_fullbody.py (options :33-75 and
:424-470, their mapping onto the training loop's arguments :76-385, the run directory and process start :472-567).

    python train_wo_flow_fullbody.py --outdir=runs --data=<training tree> --gpus=8 --cfg=fashion --batch=64 \\
        --l1_weight=40 --vgg_weight=0 --mask_weight=20 --aug=noaug

The G / D / optimiser / loss options are ``training_loop_wo_flow_fullbody.fashion_config``'s and the augmentation options
``augment_options``'s; a base config contributes the figures of the reference's ``cfg_specs`` table below.  Options this
package cannot honour are refused with the reason, not ignored.

A run writes ``training-state-<kimg>.pt`` next to every network snapshot (``--save-state``) and stops at the next tick on SIGTERM
or SIGUSR1 with snapshot and state written; ``--continue=<run directory or state file>`` goes on from there, bit for bit, with
the options the state file recorded:

    python train_wo_flow_fullbody.py --outdir=runs --data=<training tree> --continue=runs/00000-...

``--mirror-people=true`` doubles the training set with every person as a mirror shows them: photograph, label map and erase mask
reversed, left and right labels and joints exchanged, per batch on the GPU before the preparation (the reference's
``--mirror`` stays refused).

``--jitter-people=scale=0.1,rotate=5,shift=0.03,colour=0.2`` trains on every person under a random similarity map (scale, rotation,
shift) and colour change, drawn anew at every visit from the run's seed and the sample's position in the sampler's stream, and
resampled per batch on the GPU before the preparation, after the mirroring.  ``--fit-people pad|crop`` with
``--fit-filter bilinear|box`` trains on a tree whose photographs have sizes of their own: every batch is fitted to the canvas on the
GPU before the mirroring; recorded with the run, so the sample grid, the metrics and --continue see the same people.  The sample grid and the metrics see the
people as photographed.

``--ssim_weight=5`` adds ``5 * (1 - mean SSIM)`` of each of the generator's two images against the photograph to its loss: the
windows and constants ``recon_full`` reports, on the un-quantised images, value and gradient on the GPU.

``--swap_weight=1`` adds an unpaired second pass: within every per-GPU round each person is also dressed in a batch-mate's garments
(``--swap-region`` fullbody, upperbody or lowerbody), prepared on the GPU from the batch's own stages; both images of that pass go to
the discriminator and are held to the regions with a known answer -- the kept parts against the photograph, each garment region
against its warped patches -- by a region L1 term scaled by ``--l1_weight``.  ``--swap_cx_weight=W`` adds, inside
that pass, a contextual term on the garment regions: VGG-19 relu3_1 / relu4_1 features of the swapped images against those of the
warped patches, matched wherever they lie, value and gradient on the GPU without an N x N matrix.

``--erase-masks=strokes`` trains without the mask files of ``train_random_mask_acgpn``: every item's erase mask is drawn on the GPU,
random thick polylines on the padded square, anew at every visit from the run's seed and the item's position in the sampler's
stream (``--erase-strokes=strokes=6,vertices=6,length=0.25,width=0.12,turn=60`` sets their strengths); ``--erase-masks=none`` erases
only what the arm-part rule erases.  With either the tree needs no mask directory.

``--storage=bf16`` (or ``f16``) keeps the activations of G and of every block of D in that type; parameters, demodulation,
statistics, the images and the loss stay fp32.

``--part-geometry=gpu`` solves the body parts' quadrilaterals, 8 x 8 systems and inverses of every training batch in one launch
(``training.patch_pipeline.part_geometry``) instead of numpy on the host, one part at a time; with ``--swap_weight`` the swapped pass
uses the same device maps.  A second rule that prepares almost exactly the same bytes; recorded with the run only when
given as ``gpu``.  The sample grid and the metrics keep the host's geometry.
"""

import json
import os
import re
import signal
import tempfile

import click
import torch

import dnnlib
import tryon_cli
from training import training_loop_wo_flow_fullbody as training_loop
from training.dataset import training_set_class

#----------------------------------------------------------------------------

class UserError(Exception):
    pass

# train_wo_flow_fullbody.py:166-174.  'auto' is filled in from the resolution and the GPU count (:178-187).
CFG_SPECS = {
    'auto':      dict(ref_gpus=-1, kimg=25000, mb=-1, mbstd=-1, fmaps=-1,  lrate=-1,    gamma=-1, ema=-1, ramp=0.05, map=2),
    'stylegan2': dict(ref_gpus=8,  kimg=25000, mb=32, mbstd=4,  fmaps=0.5, lrate=0.002, gamma=10, ema=10, ramp=None, map=2),
    'fashion':   dict(ref_gpus=8,  kimg=8000,  mb=32, mbstd=4,  fmaps=0.5, lrate=0.002, gamma=10, ema=10, ramp=None, map=1),
}
UNSUPPORTED_CFGS = ('paper256', 'paper512', 'paper1024', 'cifar')
STORAGE_DTYPES = {None: None, 'f32': None, 'bf16': 'bfloat16', 'f16': 'float16'}      # --storage -> fashion_config's act_dtype
SUPPORTED_METRICS = ('recon_full', 'recon2k', 'tryon_full', 'tryon2k')     # metrics/metric_main.py; the reference's detector metrics are refused

def parse_jitter_people(text):
    """``--jitter-people``'s SPEC, comma-separated ``name=value`` pairs -> the specification ``training_loop(people_jitter=)``
    takes: all four names (scale 0..0.5, rotate 0..45 degrees, shift 0..0.25 of the canvas side, colour 0..0.5), absent ones 0."""
    from training.tryon_batch import jitter_spec
    try:
        return jitter_spec(tryon_cli.parse_name_values(text))
    except ValueError as err:
        raise UserError(f'--jitter-people: {err}')

def setup_training_loop_kwargs(gpus=None, snap=None, metrics=None, metrics_data=None, seed=None, data=None, cond=None, subset=None, mirror=None, cfg=None,
                               gamma=None, kimg=None, batch=None, aug=None, p=None, target=None, augpipe=None, resume=None, freezed=None,
                               fp32=None, nhwc=None, allow_tf32=None, nobench=None, workers=None, l1_weight=0, vgg_weight=0, pl_weight=0,
                               mask_weight=0, contextual_weight=0, use_noise_const_branch=False, save_state=None, storage=None,
                               mirror_people=None, jitter_people=None, ssim_weight=None, erase_masks=None, erase_strokes=None,
                               swap_weight=None, swap_region=None, swap_cx_weight=None, part_geometry=None, fit_people=None, fit_filter=None):
    """The command line's options -> (run description, keyword arguments of ``training_loop``)."""
    args = dnnlib.EasyDict()

    # General options: gpus, snap, metrics, seed (:82-109)
    gpus = 1 if gpus is None else gpus
    if not (gpus >= 1 and gpus & (gpus - 1) == 0):
        raise UserError('--gpus must be a power of two')
    args.num_gpus = gpus
    snap = 50 if snap is None else snap
    if snap < 1:
        raise UserError('--snap must be at least 1')
    args.image_snapshot_ticks = args.network_snapshot_ticks = snap
    metrics = list(metrics) if metrics else []
    refused = [m for m in metrics if m not in SUPPORTED_METRICS]
    if refused:
        raise UserError('--metrics must be none: metrics are not evaluated (the reference loop has its metric call commented out, and '
                        'this package has no metrics/ with the Inception and VGG weights it needs); refused: ' + ', '.join(refused) +
                        ' (evaluated without those weights: ' + ', '.join(SUPPORTED_METRICS) + ')')
    args.metrics = metrics
    args.random_seed = 0 if seed is None else seed
    args.save_state = True if save_state is None else bool(save_state)

    # Dataset: data, cond, subset, mirror (:115-155)
    assert isinstance(data, str)
    # a tree of *_512_320 folders (and no Zalando_256_192) is the 512 x 320 training set, whose batches carry 45 patch channels
    args.training_set_kwargs = dnnlib.EasyDict(class_name=training_set_class(data), path=data, use_labels=False, max_size=None, xflip=False)
    args.data_loader_kwargs = dnnlib.EasyDict(pin_memory=True, num_workers=0)
    # --erase-masks, --erase-strokes (own options): where the erase masks come from.  Arguments of the data set, set before it is
    # opened: with none or strokes it never looks for train_random_mask_acgpn.  The scores and the sample grid inherit them
    try:
        erase_kwargs = dnnlib.EasyDict(tryon_cli.erase_mask_kwargs(erase_masks, erase_strokes))
    except ValueError as err:
        raise UserError(str(err))
    args.training_set_kwargs.update(erase_kwargs)
    # --fit-people, --fit-filter (own options): photographs of any size, fitted to the canvas per batch on the GPU before the
    # mirroring.  Arguments of the data set, recorded only when given: the scores, the sample grid and --continue inherit them
    try:
        fit_kwargs = dnnlib.EasyDict(tryon_cli.fit_kwargs(fit_people, fit_filter))
    except ValueError as err:
        raise UserError(str(err))
    args.training_set_kwargs.update(fit_kwargs)
    try:
        training_set = dnnlib.util.construct_class_by_name(**args.training_set_kwargs)
        args.training_set_kwargs.resolution = training_set.resolution
        args.training_set_kwargs.max_size = len(training_set)
        desc = training_set.name
        content_width = training_set.content_width
        del training_set
    except IOError as err:
        raise UserError(f'--data: {err}')
    # --metrics_data: a held-out tree of the same layout for the metrics (own option; default: the training tree)
    args.metric_set_kwargs = None
    if metrics_data is not None:
        if not metrics:
            raise UserError('--metrics_data needs --metrics')
        args.metric_set_kwargs = dnnlib.EasyDict(class_name=training_set_class(metrics_data), path=metrics_data, use_labels=False,
                                                 max_size=None, xflip=False, **erase_kwargs, **fit_kwargs)
        try:
            metric_set = dnnlib.util.construct_class_by_name(**args.metric_set_kwargs)
            if metric_set.resolution != args.training_set_kwargs.resolution:
                raise UserError(f'--metrics_data: resolution {metric_set.resolution}, the training data has {args.training_set_kwargs.resolution}')
            del metric_set
        except IOError as err:
            raise UserError(f'--metrics_data: {err}')
    if cond:
        raise UserError('--cond=true is not supported: the try-on data set has no labels (the generator is conditioned on the garment patches)')
    if subset is not None:
        if not 1 <= subset <= args.training_set_kwargs.max_size:
            raise UserError(f'--subset must be between 1 and {args.training_set_kwargs.max_size}')
        desc += f'-subset{subset}'
        if subset < args.training_set_kwargs.max_size:
            args.training_set_kwargs.max_size = subset
            args.training_set_kwargs.random_seed = args.random_seed
    if mirror:
        raise UserError('--mirror=true is not supported: a mirrored person would need mirrored key points and left / right labels, '
                        'which the data set does not provide (the reference flips the prepared tuple; --mirror-people=true trains on '
                        'people mirrored before the preparation, by this package\'s own rule)')
    # --mirror-people (own option): every person a second time as a mirror shows them, mirrored per batch on the GPU.  Set after
    # max_size, which stays the number of people (:154-155 does the same with xflip)
    if mirror_people:
        desc += '-mirrorpeople'
        args.training_set_kwargs.mirror_people = True
    # --jitter-people (own option): a random scale, rotation, shift and colour change per person and visit, resampled per batch on
    # the GPU after the mirroring.  An argument of the loop, not of the data set: the sample grid and the scores build without it
    if jitter_people is not None:
        desc += '-jitterpeople'
        args.people_jitter = dnnlib.EasyDict(parse_jitter_people(jitter_people))
    if erase_kwargs:
        desc += '-erase' + erase_kwargs['erase_masks']
    if fit_kwargs:
        desc += '-fit' + fit_kwargs['fit']

    # Base config: cfg, gamma, kimg, batch (:161-246)
    cfg = 'auto' if cfg is None else cfg
    desc += f'-{cfg}'
    if cfg in UNSUPPORTED_CFGS:
        raise UserError(f'--cfg={cfg} is not supported: only auto, stylegan2 and fashion are; the others are the image-synthesis '
                        'presets of the code the reference was derived from')
    spec = dnnlib.EasyDict(CFG_SPECS[cfg])
    res = args.training_set_kwargs.resolution
    if cfg == 'auto':
        desc += f'{gpus:d}'
        spec.ref_gpus = gpus
        spec.mb = max(min(gpus * min(4096 // res, 32), 64), gpus)
        spec.mbstd = min(spec.mb // gpus, 4)
        spec.fmaps = 1 if res >= 512 else 0.5
        spec.lrate = 0.002 if res >= 1024 else 0.0025
        spec.gamma = 0.0002 * (res ** 2) / spec.mb
        spec.ema = spec.mb * 10 / 32
    # mixed precision as the reference enables it (:195-196): the three highest resolutions of G and of D in fp16
    # --storage: 16-bit activation storage in G and in every block of D, as fashion_config(act_dtype=) states it
    if storage not in STORAGE_DTYPES:
        raise UserError(f'--storage={storage} not supported')
    config = training_loop.fashion_config(channel_base=int(spec.fmaps * 32768), d_fp16_res=3, mbstd_group_size=spec.mbstd, img_resolution=res,
                                          act_dtype=STORAGE_DTYPES[storage])
    config.G_kwargs.mapping_kwargs.num_layers = spec.map
    if args.training_set_kwargs.class_name.endswith('UvitonDatasetFull_512'):
        config.G_kwargs.patch_channels = 45     # ten parts of the upper garment and five of the lower one (training/tryon_regions.py)
    config.G_kwargs.synthesis_kwargs.use_noise = bool(use_noise_const_branch)
    config.G_opt_kwargs.lr = config.D_opt_kwargs.lr = spec.lrate
    config.loss_kwargs.update(r1_gamma=spec.gamma, l1_weight=l1_weight or 0, vgg_weight=vgg_weight or 0, pl_weight=pl_weight or 0,
                              contextual_weight=contextual_weight or 0, mask_weight=mask_weight or 0)
    # --ssim_weight (own option): 1 - mean SSIM of both generated images against the photograph, over the content columns the
    # batch builder pads from.  Absent or 0 adds no key: the recorded options of every other command stay what they were
    if ssim_weight is not None and not ssim_weight >= 0:
        raise UserError('--ssim_weight must be non-negative')
    if ssim_weight:
        config.loss_kwargs.update(ssim_weight=ssim_weight, ssim_width=content_width)
    # --swap_weight, --swap-region (own options): the unpaired pass on every person in a batch-mate's garments.  Absent or 0 adds no
    # key, here or below
    if swap_weight is not None and not swap_weight >= 0:
        raise UserError('--swap_weight must be non-negative')
    if swap_region is not None and not swap_weight:
        raise UserError('--swap-region needs a positive --swap_weight: without one nobody is dressed in another\'s garments')
    if swap_weight:
        config.loss_kwargs.update(swap_weight=swap_weight)
    # --swap_cx_weight (own option): the contextual term of the unpaired pass, same texture without asking where
    if swap_cx_weight is not None and not swap_cx_weight >= 0:
        raise UserError('--swap_cx_weight must be non-negative')
    if swap_cx_weight and not swap_weight:
        raise UserError('--swap_cx_weight needs a positive --swap_weight: it is a term of the unpaired pass')
    if swap_cx_weight:
        config.loss_kwargs.update(swap_cx_weight=swap_cx_weight)
    config.ema_kimg, config.ema_rampup = spec.ema, spec.ramp
    args.total_kimg = spec.kimg
    args.batch_size = spec.mb
    args.batch_gpu = spec.mb // spec.ref_gpus
    if gamma is not None:
        if not gamma >= 0:
            raise UserError('--gamma must be non-negative')
        desc += f'-gamma{gamma:g}'
        config.loss_kwargs.r1_gamma = gamma
    if kimg is not None:
        if not kimg >= 1:
            raise UserError('--kimg must be at least 1')
        desc += f'-kimg{kimg:d}'
        args.total_kimg = kimg
    if batch is not None:
        if not (batch >= 1 and batch % gpus == 0):
            raise UserError('--batch must be at least 1 and divisible by --gpus')
        desc += f'-batch{batch}'
        args.batch_size = batch
        args.batch_gpu = batch // gpus

    # Discriminator augmentation: aug, p, target, augpipe (:252-313)
    if aug is None:
        aug = 'ada'
    else:
        desc += f'-{aug}'
    if aug not in ('ada', 'noaug', 'fixed'):
        raise UserError(f'--aug={aug} not supported')
    if aug == 'fixed' and p is None:
        raise UserError(f'--aug={aug} requires specifying --p')
    if p is not None:
        if aug != 'fixed':
            raise UserError('--p can only be specified with --aug=fixed')
        if not 0 <= p <= 1:
            raise UserError('--p must be between 0 and 1')
        desc += f'-p{p:g}'
    if target is not None:
        if aug != 'ada':
            raise UserError('--target can only be specified with --aug=ada')
        if not 0 <= target <= 1:
            raise UserError('--target must be between 0 and 1')
        desc += f'-target{target:g}'
    if augpipe is None:
        augpipe = 'bgc'
    else:
        if aug == 'noaug':
            raise UserError('--augpipe cannot be specified with --aug=noaug')
        desc += f'-{augpipe}'
    config.update(training_loop.augment_options(aug=aug, augpipe=augpipe, p=p, target=target))

    # Transfer learning: resume, freezed (:327-348)
    if resume is None or resume == 'noresume':
        desc += '-noresume' if resume is not None else ''
    else:
        if not os.path.isfile(resume):
            raise UserError(f'--resume={resume}: not a file (the reference\'s named source networks and URLs are downloads, which are '
                            'not supported; give the path of a network pickle)')
        desc += '-resumecustom'
        args.resume_pkl = resume
        config.ada_kimg = 100       # make ADA react faster at the beginning
        config.ema_rampup = None
    if freezed is not None:
        if not freezed >= 0:
            raise UserError('--freezed must be non-negative')
        desc += f'-freezed{freezed:d}'
        config.D_kwargs.block_kwargs.freeze_layers = freezed

    # Performance options: fp32, nhwc, allow_tf32, workers (:354-383); --nobench is accepted and means nothing here (no cuDNN)
    if STORAGE_DTYPES[storage] is not None:
        if fp32:
            raise UserError(f'--fp32=true and --storage={storage} contradict: --fp32 asks for fp32 activations in every block, '
                            '--storage for 16-bit ones')
        desc += f'-{storage}'
    if ssim_weight:
        desc += f'-ssim{ssim_weight:g}'
    if swap_weight:
        # the swap group is one per-GPU round: the donors of a round come from that round, so accumulation does not change them
        if args.batch_gpu < 2:
            raise UserError(f'--swap_weight needs at least 2 samples per GPU round, --batch={args.batch_size} on {gpus} GPUs gives '
                            f'{args.batch_gpu}: a person\'s donor is a batch-mate of the same round')
        swap_region = 'fullbody' if swap_region is None else swap_region
        desc += f'-swap{swap_weight:g}' + (swap_region if swap_region != 'fullbody' else '') + (f'-cx{swap_cx_weight:g}' if swap_cx_weight else '')
        args.swap_outfits = dnnlib.EasyDict(region=swap_region, group=args.batch_gpu)
    # --part-geometry (own option): the body parts' matrices in one launch per batch instead of numpy on the host.  Absent
    # or host records nothing, so that such a run's options and launches are what they always were.
    if part_geometry not in (None, 'host', 'gpu'):
        raise UserError(f'--part-geometry must be host or gpu, not {part_geometry}')
    if part_geometry == 'gpu':
        desc += '-geomgpu'
        args.part_geometry = 'gpu'
    if fp32:
        config.G_kwargs.synthesis_kwargs.num_fp16_res = config.D_kwargs.num_fp16_res = 0
        config.G_kwargs.synthesis_kwargs.conv_clamp = config.D_kwargs.conv_clamp = None
    if nhwc:
        raise UserError('--nhwc=true is not supported: the HIP convolution kernels take NCHW tensors')
    if allow_tf32:
        config.allow_tf32 = True
    if workers is not None:
        if not workers >= 1:
            raise UserError('--workers must be at least 1')
        args.data_loader_kwargs.num_workers = workers
        args.data_loader_kwargs.prefetch_factor = 2

    args.cfg = config
    return desc, args

#----------------------------------------------------------------------------

# what --continue may be combined with (besides --outdir and --data): these replace the recorded values, everything else is the run's
CONTINUE_MAY_CHANGE = ('kimg', 'snap', 'metrics', 'metrics_data', 'workers', 'save_state')

def find_state_file(path):
    """``--continue``'s PATH -> the state file: the path itself, or the one with the highest kimg of a run directory."""
    from training import train_state
    if os.path.isdir(path):
        found = train_state.state_files(path)
        if not found:
            raise UserError(f'--continue={path}: the directory holds no training-state-*.pt (was the run started with --save-state=false?)')
        return found[-1][1]
    if not os.path.isfile(path):
        raise UserError(f'--continue={path}: neither a run directory nor a training-state-*.pt file')
    return path

def setup_continue_kwargs(continue_path, data=None, **given):
    """``--continue``: (run description, keyword arguments of ``training_loop``) from the options the state file recorded."""
    from training import train_state
    state_file = os.path.abspath(find_state_file(continue_path))
    try:
        state = train_state.load_state(state_file, mmap=True)      # the options and the counters; no tensor is read
    except (ValueError, RuntimeError, OSError) as err:
        raise UserError(f'--continue: {err}')
    if not state.get('options'):
        raise UserError(f'--continue={continue_path}: the state file records no options (it was not written by this command)')
    args = json.loads(state['options'], object_hook=dnnlib.EasyDict)
    kimg_done = int(state['cur_nimg']) // 1000
    del state

    given = {name: value for name, value in given.items() if value is not None}
    for name, value in given.items():
        recorded = {'gpus': args.num_gpus, 'batch': args.batch_size}.get(name)
        if name in CONTINUE_MAY_CHANGE or (recorded is not None and value == recorded):
            continue
        option = '--' + {'allow_tf32': 'allow-tf32', 'mirror_people': 'mirror-people', 'jitter_people': 'jitter-people', 'erase_masks': 'erase-masks',
                         'erase_strokes': 'erase-strokes', 'swap_region': 'swap-region', 'part_geometry': 'part-geometry',
                         'fit_people': 'fit-people', 'fit_filter': 'fit-filter'}.get(name, name)
        raise UserError(f'{option} cannot be given with --continue: a continued run keeps its recorded value' +
                        (f' ({recorded})' if recorded is not None else ''))

    # the data: the tree may have moved; it must still be the recorded set
    assert isinstance(data, str)
    recorded = args.training_set_kwargs
    class_name = training_set_class(data)
    try:
        # the people are counted unmirrored: max_size was recorded before --mirror-people doubled the set
        training_set = dnnlib.util.construct_class_by_name(**dict(recorded, class_name=class_name, path=data, max_size=None, mirror_people=False))
        people, resolution = len(training_set), training_set.resolution
        del training_set
    except IOError as err:
        raise UserError(f'--data: {err}')
    if class_name != recorded.class_name:
        raise UserError(f'--data: a tree of {class_name.rsplit(".", 1)[-1]}, the run was recorded on {recorded.class_name.rsplit(".", 1)[-1]}')
    if resolution != recorded.resolution:
        raise UserError(f'--data: resolution {resolution}, the run was recorded at {recorded.resolution}')
    subset = 'random_seed' in recorded          # --subset: max_size is the subset's size, the tree's own size was not recorded
    if (people < recorded.max_size) if subset else (people != recorded.max_size):
        raise UserError(f'--data: {people} people, the run was recorded on {"a subset of " if subset else ""}{recorded.max_size}')
    recorded.path = data

    if 'kimg' in given:
        if not given['kimg'] >= 1:
            raise UserError('--kimg must be at least 1')
        args.total_kimg = given['kimg']
    if 'snap' in given:
        if given['snap'] < 1:
            raise UserError('--snap must be at least 1')
        args.image_snapshot_ticks = args.network_snapshot_ticks = given['snap']
    if 'metrics' in given:
        refused = [m for m in given['metrics'] if m not in SUPPORTED_METRICS]
        if refused:
            raise UserError('--metrics: not evaluated: ' + ', '.join(refused) + ' (evaluated: ' + ', '.join(SUPPORTED_METRICS) + ')')
        args.metrics = list(given['metrics'])
        if not args.metrics:
            args.metric_set_kwargs = None
    if 'metrics_data' in given:
        if not args.metrics:
            raise UserError('--metrics_data needs --metrics')
        metrics_data = given['metrics_data']
        args.metric_set_kwargs = dnnlib.EasyDict(class_name=training_set_class(metrics_data), path=metrics_data, use_labels=False,
                                                 max_size=None, xflip=False,
                                                 **{k: recorded[k] for k in ('erase_masks', 'erase_strokes', 'fit', 'fit_filter') if k in recorded})
        try:
            metric_set = dnnlib.util.construct_class_by_name(**args.metric_set_kwargs)
            if metric_set.resolution != recorded.resolution:
                raise UserError(f'--metrics_data: resolution {metric_set.resolution}, the training data has {recorded.resolution}')
            del metric_set
        except IOError as err:
            raise UserError(f'--metrics_data: {err}')
    if 'workers' in given:
        if not given['workers'] >= 1:
            raise UserError('--workers must be at least 1')
        args.data_loader_kwargs.num_workers = given['workers']
        args.data_loader_kwargs.prefetch_factor = 2
    if 'save_state' in given:
        args.save_state = bool(given['save_state'])

    # <recorded description>-continue<kimg>; a run continued twice keeps one suffix
    desc = re.sub(r'^\d+-', '', os.path.basename(os.path.normpath(args.pop('run_dir', '') or 'run')))
    desc = re.sub(r'-continue\d{6}$', '', desc) + f'-continue{kimg_done:06d}'
    args.pop('resume_pkl', None)        # the networks come from the state file; cfg stays as that run had it
    args.resume_state = state_file
    return desc, args

#----------------------------------------------------------------------------

def install_abort_signals(signals=(signal.SIGTERM, signal.SIGUSR1)):
    """Handlers that set a flag; returns the flag's reader, which is the loop's ``abort_fn``: the run ends at the next tick
    boundary with image, snapshot and state written.  A second signal changes nothing."""
    flag = []
    def handler(signum, frame):
        flag.append(signum)
    for signum in signals:
        signal.signal(signum, handler)
    return lambda: bool(flag)

def subprocess_fn(rank, args, temp_dir):
    from torch_utils import training_stats
    abort_fn = install_abort_signals()
    dnnlib.util.Logger(file_name=os.path.join(args.run_dir, 'log.txt'), file_mode='a', should_flush=True)
    if args.num_gpus > 1:
        init_file = os.path.abspath(os.path.join(temp_dir, '.torch_distributed_init'))
        torch.distributed.init_process_group(backend='nccl', init_method=f'file://{init_file}', rank=rank, world_size=args.num_gpus)
    sync_device = torch.device('cuda', rank) if args.num_gpus > 1 else None
    training_stats.init_multiprocessing(rank=rank, sync_device=sync_device)
    training_loop.training_loop(rank=rank, abort_fn=abort_fn, **args)

#----------------------------------------------------------------------------

class CommaSeparatedList(click.ParamType):
    name = 'list'

    def convert(self, value, param, ctx):
        if value is None or value.lower() == 'none' or value == '':
            return []
        return value.split(',')

@click.command()
@click.pass_context
# General options.
@click.option('--outdir', help='Where to save the results', required=True, metavar='DIR')
@click.option('--gpus', help='Number of GPUs to use [default: 1]', type=int, metavar='INT')
@click.option('--snap', help='Snapshot interval [default: 50 ticks]', type=int, metavar='INT')
@click.option('--metrics', help='Comma-separated list of recon_full, recon2k, tryon_full, tryon2k, or "none" [default: none]', type=CommaSeparatedList())
@click.option('--metrics_data', help='Tree the metrics are evaluated on [default: the training data]', metavar='PATH')
@click.option('--seed', help='Random seed [default: 0]', type=int, metavar='INT')
@click.option('-n', '--dry-run', help='Print training options and exit', is_flag=True)
@click.option('--save-state', help='Write a training-state file with every network snapshot [default: true]', type=bool, metavar='BOOL')
@click.option('--continue', 'continue_path', help='Continue the run of this directory or training-state-*.pt file, with its recorded options',
              metavar='PATH')
# Dataset.
@click.option('--data', help='Training data (directory)', metavar='PATH', required=True)
@click.option('--cond', help='Not supported [default: false]', type=bool, metavar='BOOL')
@click.option('--subset', help='Train with only N images [default: all]', type=int, metavar='INT')
@click.option('--mirror', help='Not supported [default: false]', type=bool, metavar='BOOL')
@click.option('--mirror-people', help='Train on every person a second time, mirrored on the GPU [default: false]', type=bool, metavar='BOOL')
@click.option('--jitter-people', help='Train on people jittered on the GPU: comma-separated scale=0..0.5, rotate=0..45 (degrees), '
              'shift=0..0.25 (of the canvas side), colour=0..0.5 [default: none]', metavar='SPEC')
@tryon_cli.erase_options('files')
@tryon_cli.fit_options()
# Base config.
@click.option('--cfg', help='Base config [default: auto]', type=click.Choice(list(CFG_SPECS) + list(UNSUPPORTED_CFGS)))
@click.option('--gamma', help='Override R1 gamma', type=float)
@click.option('--kimg', help='Override training duration', type=int, metavar='INT')
@click.option('--batch', help='Override batch size', type=int, metavar='INT')
# Discriminator augmentation.
@click.option('--aug', help='Augmentation mode [default: ada]', type=click.Choice(['noaug', 'ada', 'fixed']))
@click.option('--p', help='Augmentation probability for --aug=fixed', type=float)
@click.option('--target', help='ADA target value for --aug=ada', type=float)
@click.option('--augpipe', help='Augmentation pipeline [default: bgc]', type=click.Choice(sorted(training_loop.AUGPIPE_SPECS)))
# Transfer learning.
@click.option('--resume', help='Resume from a network pickle [default: noresume]', metavar='PKL')
@click.option('--freezed', help='Freeze-D [default: 0 layers]', type=int, metavar='INT')
# Performance options.
@click.option('--fp32', help='Disable mixed-precision training', type=bool, metavar='BOOL')
@click.option('--nhwc', help='Not supported', type=bool, metavar='BOOL')
@click.option('--nobench', help='Accepted for compatibility; no effect', type=bool, metavar='BOOL')
@click.option('--allow-tf32', help='Use the three-product split-bf16 convolution arithmetic', type=bool, metavar='BOOL')
@click.option('--workers', help='Override number of DataLoader workers', type=int, metavar='INT')
@click.option('--storage', help='Activation storage of G and D: f32, or 16-bit (bf16, f16) with fp32 parameters and statistics [default: f32]',
              type=click.Choice(['f32', 'bf16', 'f16']))
# Loss weights.
@click.option('--pl_weight', type=float)
@click.option('--l1_weight', help='G L1 loss weight', type=float)
@click.option('--ssim_weight', help='G SSIM loss weight: 1 - mean SSIM against the photograph, the windows recon_full reports [default: 0]',
              type=float)
@click.option('--swap_weight', help='Weight of the unpaired pass: every person also in a batch-mate\'s garments, through D and a region L1 '
              'term [default: 0]', type=float)
@click.option('--swap-region', help='What the donor gives in the unpaired pass [default: fullbody]',
              type=click.Choice(['fullbody', 'upperbody', 'lowerbody']))
@click.option('--swap_cx_weight', help='Weight, within the unpaired pass, of a contextual term on its garment regions: VGG-19 relu3_1 and relu4_1 '
              'features of the swapped images against those of the warped patches, matched wherever they lie.  Needs --swap_weight.  The '
              'features come from ./checkpoints/vgg19-dcbb9e9d.pth when it exists, otherwise from seeded RANDOM weights, whose values mean '
              'only what random features mean [default: 0]', type=float)
@click.option('--part-geometry', help='Where the body-part matrices of a batch are solved: numpy on the host, or one launch on the GPU (almost '
              'exactly the same bytes: DESIGN 8n) [default: host]', type=click.Choice(['host', 'gpu']))
@click.option('--vgg_weight', help='vgg loss weight (runs from random weights: the checkpoint cannot be obtained; --ssim_weight is the '
              'structural term that needs none)', type=float)
@click.option('--contextual_weight', help='contextual loss weight (refused unless 0: its checkpoint cannot be obtained; see --ssim_weight)',
              type=float)
@click.option('--mask_weight', type=float)
@click.option('--use_noise_const_branch', help='Enable const_branch noise input?', type=bool, metavar='BOOL')
def main(ctx, outdir, dry_run, continue_path, **config_kwargs):
    """Train PASTA-GAN's full-body try-on model on the reference's training tree."""
    try:
        if continue_path is not None:
            run_desc, args = setup_continue_kwargs(continue_path, **config_kwargs)
        else:
            run_desc, args = setup_training_loop_kwargs(**config_kwargs)
    except UserError as err:
        ctx.fail(str(err))

    # Pick output directory (:525-532).
    prev_run_dirs = []
    if os.path.isdir(outdir):
        prev_run_dirs = [x for x in os.listdir(outdir) if os.path.isdir(os.path.join(outdir, x))]
    prev_run_ids = [re.match(r'^\d+', x) for x in prev_run_dirs]
    prev_run_ids = [int(x.group()) for x in prev_run_ids if x is not None]
    cur_run_id = max(prev_run_ids, default=-1) + 1
    args.run_dir = os.path.join(outdir, f'{cur_run_id:05d}-{run_desc}')
    assert not os.path.exists(args.run_dir)

    print()
    print('Training options:')
    print(json.dumps(args, indent=2))
    print()
    print(f'Output directory:   {args.run_dir}')
    print(f'Training data:      {args.training_set_kwargs.path}')
    print(f'Data set class:     {args.training_set_kwargs.class_name.rsplit(".", 1)[-1]}')
    print(f'Training duration:  {args.total_kimg} kimg')
    print(f'Number of GPUs:     {args.num_gpus}')
    print(f'Number of images:   {args.training_set_kwargs.max_size}')
    print(f'Mirrored people:    {bool(args.training_set_kwargs.get("mirror_people", False))}')
    jitter = args.get('people_jitter')
    print(f'Jittered people:    {",".join(f"{k}={v:g}" for k, v in jitter.items()) if jitter else False}')
    strokes = args.training_set_kwargs.get('erase_strokes')
    print(f'Erase masks:        {args.training_set_kwargs.get("erase_masks", "files")}' +
          (f' ({",".join(f"{k}={v:g}" for k, v in strokes.items())})' if strokes else ''))
    swap = args.get('swap_outfits')
    if swap:
        print(f'Swapped outfits:    weight {args.cfg.loss_kwargs.swap_weight:g}, {swap.region}, groups of {swap.group}' +
              (f', contextual weight {args.cfg.loss_kwargs.swap_cx_weight:g}' if args.cfg.loss_kwargs.get('swap_cx_weight') else ''))
    if args.get('part_geometry'):
        print(f'Part geometry:      {args.part_geometry}')
    if args.training_set_kwargs.get('fit'):
        print(f'Fitted people:      {args.training_set_kwargs.fit} ({args.training_set_kwargs.fit_filter})')
    print(f'Image resolution:   {args.training_set_kwargs.resolution}')
    print()
    if dry_run:
        print('Dry run; exiting.')
        return

    print('Creating output directory...')
    os.makedirs(args.run_dir)
    with open(os.path.join(args.run_dir, 'training_options.json'), 'wt') as f:
        json.dump(args, f, indent=2)

    # One process for one GPU; fresh children (spawn) joined through a file for more.
    print('Launching processes...')
    with tempfile.TemporaryDirectory() as temp_dir:
        if args.num_gpus == 1:
            subprocess_fn(rank=0, args=args, temp_dir=temp_dir)
        else:
            # the children's handlers end the run; this process hands both signals on to them and waits
            context = torch.multiprocessing.spawn(fn=subprocess_fn, args=(args, temp_dir), nprocs=args.num_gpus, join=False)
            def forward(signum, frame):
                for pid in context.pids():
                    try:
                        os.kill(pid, signum)
                    except ProcessLookupError:
                        pass
            for signum in (signal.SIGTERM, signal.SIGUSR1):
                signal.signal(signum, forward)
            while not context.join():
                pass

#----------------------------------------------------------------------------

if __name__ == '__main__':
    main()  # pylint: disable=no-value-for-parameter
