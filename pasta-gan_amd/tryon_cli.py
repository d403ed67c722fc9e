"""What the two try-on command lines, test.py and test_512.py, share: the options the reference declares, the refusal of a
snapshot that is not a local file, loading ``G_ema``, the loader over a pair data set and the generator's call sequence."""

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
        # --storage is kept here for ``load_generator`` and handed to the command's function only where it declares the argument
        # (test.py writes it into its report): a command line that just loads and runs the generator needs no line for it
        takes_storage = 'storage' in inspect.signature(f).parameters

        @functools.wraps(f)
        def command(*args, storage=None, **kwargs):
            _given['storage'] = storage
            if takes_storage:
                kwargs['storage'] = storage
            return f(*args, **kwargs)
        for option in reversed(options):
            command = option(command)
        return command
    return decorate


# --storage: run the loaded generator in this activation storage instead of the one it was pickled with
STORAGE_DTYPES = {'snapshot': None, 'f32': 'float32', 'bf16': 'bfloat16', 'f16': 'float16'}
_given = {}                 # the running command's --storage (``shared_options``)
storage_option = click.option('--storage', help='Activation storage the generator runs in: as pickled (snapshot), or f32, bf16, f16 '
                              '[default: snapshot]', type=click.Choice(list(STORAGE_DTYPES)))

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


def pair_loader(dataset, batchsize, workers):
    """The pairs of ``dataset`` in order; the workers only decode files."""
    import torch
    from training.dataset import collate_pairs
    print(len(dataset))
    return torch.utils.data.DataLoader(dataset, batch_size=batchsize, shuffle=False, num_workers=workers, pin_memory=True, collate_fn=collate_pairs)


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
