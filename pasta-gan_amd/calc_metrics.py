"""Score a network snapshot with the metrics of ``metrics/`` (the reference's calc_metrics.py, restricted to what this package
registers: the paired-reconstruction metrics ``recon_full`` and ``recon2k``, and the unpaired try-on metrics ``tryon_full`` and
``tryon2k``, every person in the next person's garments scored by region -- DESIGN 8m).

    python calc_metrics.py --network runs/00000-x/network-snapshot-000200.pkl                  # on the snapshot's training tree
    python calc_metrics.py --network snapshot.pkl --metrics recon2k --data held_out_tree --gpus 8
    python calc_metrics.py --network snapshot.pkl --metrics recon2k,tryon2k --data held_out_tree

Without --data the snapshot's own ``training_set_kwargs`` name the tree; --data names another one of the same layout (a held-out
tree; a tree of ``*_512_320`` folders is read as the 512 x 320 training set).  When the snapshot lies in a training run's directory (one with training_options.json), the result is also appended to
that directory's ``metric-<name>.jsonl``.  --network must name a local file: URLs are refused (nothing is downloaded).
--storage f32 | bf16 | f16 scores the generator in that activation storage, whatever it was pickled with; the result line then
carries a ``storage`` field.  --erase-masks files | none | strokes and --erase-strokes SPEC say where the erase masks of
the scored batches come from, as train_wo_flow_fullbody.py's options do; their default is what the snapshot recorded, and
``--erase-masks none`` scores a snapshot trained on mask files on a tree that has none; the ``tryon_*`` metrics
apply no erase mask and never look for one.  --fit-people pad | crop and --fit-filter bilinear | box score a tree whose photographs
have sizes of their own, fitted to the canvas on the GPU; their default, too, is what the snapshot recorded.  One
process per GPU; for more than one GPU fresh processes are spawned, each loading the snapshot itself."""

import json
import os
import re
import tempfile

import click

import tryon_cli

#----------------------------------------------------------------------------

def subprocess_fn(rank, args, temp_dir):
    import torch
    import legacy
    from metrics import metric_main, metric_utils
    if args.num_gpus > 1:
        init_file = os.path.abspath(os.path.join(temp_dir, '.torch_distributed_init'))
        torch.distributed.init_process_group(backend='nccl', init_method=f'file://{init_file}', rank=rank, world_size=args.num_gpus)
    device = torch.device('cuda', rank)
    torch.cuda.set_device(device)
    verbose = args.verbose and rank == 0
    if verbose:
        print(f'Loading network from "{args.network_pkl}"...')
    with open(args.network_pkl, 'rb') as f:
        G = legacy.load_network_pkl(f)['G_ema'].eval().requires_grad_(False).to(device)
    if args.storage is not None and args.storage != 'snapshot':
        from training.networks import set_activation_storage
        set_activation_storage(G, tryon_cli.STORAGE_DTYPES[args.storage])
    for metric in args.metrics:
        if verbose:
            print(f'Calculating {metric}...')
        progress = metric_utils.ProgressMonitor(verbose=verbose)
        result_dict = metric_main.calc_metric(metric=metric, G=G, dataset_kwargs=args.dataset_kwargs, num_gpus=args.num_gpus, rank=rank,
                                              device=device, progress=progress, batch_size=args.batch_size,
                                              data_loader_kwargs=dict(num_workers=args.workers, pin_memory=True))
        if args.storage is not None:
            result_dict.storage = args.storage
        if rank == 0:
            metric_main.report_metric(result_dict, run_dir=args.run_dir, snapshot_pkl=args.network_pkl)
        if verbose:
            print()
    if args.num_gpus > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if verbose:
        print('Exiting...')

#----------------------------------------------------------------------------

class CommaSeparatedList(click.ParamType):
    name = 'list'

    def convert(self, value, param, ctx):
        if value is None or value.lower() == 'none' or value == '':
            return []
        return value.split(',')

@click.command()
@click.pass_context
@click.option('network_pkl', '--network', help='Network pickle filename (a local file)', metavar='PATH', required=True)
@click.option('--metrics', help='Comma-separated list of recon_full, recon2k, tryon_full, tryon2k, or "none"', type=CommaSeparatedList(), default='recon_full', show_default=True)
@click.option('--data', help='Tree to score against (directory) [default: the snapshot\'s training data]', metavar='PATH')
@click.option('--gpus', help='Number of GPUs to use', type=click.IntRange(min=1), default=1, metavar='INT', show_default=True)
@click.option('--verbose', help='Print optional information', type=bool, default=True, metavar='BOOL', show_default=True)
@click.option('--batch', 'batch_size', help='Items per batch and GPU (the results do not depend on it)', type=click.IntRange(min=1), default=16,
              show_default=True)
@click.option('--workers', help='Loader processes (file decoding only)', type=click.IntRange(min=0), default=0, show_default=True)
@tryon_cli.storage_option
@tryon_cli.erase_options('as the snapshot recorded')
@tryon_cli.fit_options('as the snapshot recorded', 'as the snapshot recorded, else bilinear')
def calc_metrics(ctx, network_pkl, metrics, data, gpus, verbose, batch_size, workers, storage, erase_masks, erase_strokes, fit_people, fit_filter):
    """Calculate quality metrics of a network snapshot on a tree of the training set's layout."""
    import dnnlib
    from metrics import metric_main
    args = dnnlib.EasyDict(metrics=metrics, num_gpus=gpus, network_pkl=network_pkl, verbose=verbose, batch_size=batch_size, workers=workers,
                           storage=storage)
    unknown = [m for m in args.metrics if not metric_main.is_valid_metric(m)]
    if unknown:
        ctx.fail('\n'.join(['--metrics: unknown metric ' + ', '.join(unknown), 'valid metrics: ' + ', '.join(metric_main.list_metrics())]))
    if re.match(r'^[A-Za-z][A-Za-z0-9+.-]*://', network_pkl):
        ctx.fail('--network: %r is a URL: give the path of a local snapshot file' % network_pkl)
    if not os.path.isfile(network_pkl):
        ctx.fail('--network: %r is not a file' % network_pkl)

    # Data set options: the tree given, else the one the snapshot was trained on.  Where the erase masks come from: as given,
    # else as the snapshot recorded (a snapshot trained on files can be scored on a tree that has none: --erase-masks none).
    import legacy
    with open(network_pkl, 'rb') as f:
        kwargs = legacy.load_network_pkl(f).get('training_set_kwargs')
    if data is not None:
        if not os.path.isdir(data):
            ctx.fail('--data: %r is not a directory' % data)
        from training.dataset import training_set_class
        args.dataset_kwargs = dnnlib.EasyDict(class_name=training_set_class(data), path=data)
        args.dataset_kwargs.update({k: kwargs[k] for k in ('erase_masks', 'erase_strokes', 'fit', 'fit_filter') if kwargs is not None and k in kwargs})
    else:
        if kwargs is None:
            ctx.fail('Could not look up dataset options; please specify --data')
        args.dataset_kwargs = dnnlib.EasyDict(kwargs)
    if erase_masks is not None or erase_strokes is not None:
        if erase_masks is None:
            erase_masks = args.dataset_kwargs.get('erase_masks', 'files')       # --erase-strokes alone: new strengths for recorded strokes
        try:
            given = tryon_cli.erase_mask_kwargs(erase_masks, erase_strokes)
        except ValueError as err:
            ctx.fail(str(err))
        for k in ('erase_masks', 'erase_strokes'):
            args.dataset_kwargs.pop(k, None)
        args.dataset_kwargs.update(given)
    if fit_people is not None or fit_filter is not None:
        # --fit-filter alone: another filter for the recorded mode
        try:
            given = tryon_cli.fit_kwargs(args.dataset_kwargs.get('fit') if fit_people is None else fit_people,
                                         args.dataset_kwargs.get('fit_filter') if fit_filter is None else fit_filter)
        except ValueError as err:
            ctx.fail(str(err))
        args.dataset_kwargs.update(given)
    args.dataset_kwargs.update(use_labels=False, xflip=False, mirror_people=False)
    if args.verbose:
        print('Dataset options:')
        print(json.dumps(args.dataset_kwargs, indent=2))

    # A snapshot inside a training run's directory reports into that directory.
    args.run_dir = None
    pkl_dir = os.path.dirname(os.path.abspath(network_pkl))
    if os.path.isfile(os.path.join(pkl_dir, 'training_options.json')):
        args.run_dir = pkl_dir

    if args.verbose:
        print('Launching processes...')
    with tempfile.TemporaryDirectory() as temp_dir:
        if args.num_gpus == 1:
            subprocess_fn(rank=0, args=args, temp_dir=temp_dir)
        else:
            import torch
            torch.multiprocessing.spawn(fn=subprocess_fn, args=(args, temp_dir), nprocs=args.num_gpus)

#----------------------------------------------------------------------------

if __name__ == '__main__':
    calc_metrics()  # pylint: disable=no-value-for-parameter
