"""The metric registry, ``calc_metric`` and ``report_metric`` with the reference's call signatures and report format
(metrics/metric_main.py:24-77), holding the metrics this package can compute without a pretrained detector network."""

import json
import os
import time

import dnnlib

from . import metric_utils
from . import reconstruction
from . import tryon_swapped

#----------------------------------------------------------------------------

# Two families, each name -> function of MetricOptions returning {result key: float}.  ``_metrics`` holds the paired metrics and
# is what ``register_metric`` and ``list_valid_metrics`` have dealt with since DESIGN 8c: both keep that meaning, so that nothing
# which lists or registers paired metrics changes.  ``_unpaired`` holds the swapped try-on metrics of DESIGN 8m.  A name of either
# family is valid for ``calc_metric``, ``report_metric`` and the commands; ``list_metrics`` names them all.
_metrics = dict()
_unpaired = dict()

def register_metric(fn):
    assert callable(fn)
    _metrics[fn.__name__] = fn
    return fn

def register_unpaired_metric(fn):
    assert callable(fn) and fn.__name__ not in _metrics
    _unpaired[fn.__name__] = fn
    return fn

def is_valid_metric(metric):
    return metric in _metrics or metric in _unpaired

def list_valid_metrics():
    """The paired metrics, in the order they were registered."""
    return list(_metrics)

def list_unpaired_metrics():
    return list(_unpaired)

def list_metrics():
    """Every name ``is_valid_metric`` accepts: the paired metrics, then the unpaired ones."""
    return list_valid_metrics() + list_unpaired_metrics()

#----------------------------------------------------------------------------

def calc_metric(metric, **kwargs):
    """``calc_metric(metric, G=, dataset_kwargs=, num_gpus=, rank=, device=, progress=None)`` (the arguments of
    ``metric_utils.MetricOptions``) on every rank -> EasyDict(results, metric, total_time, total_time_str, num_gpus).  Every rank
    ends with the same results: they are computed from partial sums that the ranks have exchanged."""
    if not is_valid_metric(metric):
        raise ValueError('unknown metric %r; valid metrics: %s' % (metric, ', '.join(list_metrics())))
    opts = metric_utils.MetricOptions(**kwargs)
    start_time = time.time()
    results = (_metrics[metric] if metric in _metrics else _unpaired[metric])(opts)
    total_time = time.time() - start_time
    return dnnlib.EasyDict(results=dnnlib.EasyDict({k: float(v) for k, v in results.items()}), metric=metric, total_time=total_time,
                           total_time_str=dnnlib.util.format_time(total_time), num_gpus=opts.num_gpus)

def report_metric(result_dict, run_dir=None, snapshot_pkl=None):
    """Print the result as one JSON line, with the snapshot's path relative to ``run_dir`` and a timestamp, and append the line to
    ``<run_dir>/metric-<name>.jsonl`` when the directory exists."""
    metric = result_dict['metric']
    assert is_valid_metric(metric)
    if run_dir is not None and snapshot_pkl is not None:
        snapshot_pkl = os.path.relpath(snapshot_pkl, run_dir)
    line = json.dumps(dict(result_dict, snapshot_pkl=snapshot_pkl, timestamp=time.time()))
    print(line)
    if run_dir is not None and os.path.isdir(run_dir):
        with open(os.path.join(run_dir, f'metric-{metric}.jsonl'), 'at') as f:
            f.write(line + '\n')

#----------------------------------------------------------------------------
# Paired reconstruction (metrics/reconstruction.py).  Scored on the people as photographed: a snapshot's training_set_kwargs may carry
# mirror_people, which is forced off where xflip is.

@register_metric
def recon_full(opts):
    opts.dataset_kwargs.update(max_size=None, xflip=False, mirror_people=False)
    return reconstruction.compute(opts, 'recon_full')

@register_metric
def recon2k(opts):
    opts.dataset_kwargs.update(max_size=2000, random_seed=0, xflip=False, mirror_people=False)
    return reconstruction.compute(opts, 'recon2k')

#----------------------------------------------------------------------------
# Unpaired try-on (metrics/tryon_swapped.py): every person in the next person's garments, scored by region.  The swapped pass
# applies no erase mask, so none is loaded (and a recorded strokes specification goes with it): a held-out tree needs no masks.

def _swapped_set(opts, **subset):
    opts.dataset_kwargs.pop('erase_strokes', None)
    opts.dataset_kwargs.update(xflip=False, mirror_people=False, erase_masks='none', **subset)

@register_unpaired_metric
def tryon_full(opts):
    _swapped_set(opts, max_size=None)
    return tryon_swapped.compute(opts, 'tryon_full')

@register_unpaired_metric
def tryon2k(opts):
    _swapped_set(opts, max_size=2000, random_seed=0)
    return tryon_swapped.compute(opts, 'tryon2k')

#----------------------------------------------------------------------------
