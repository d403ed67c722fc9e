"""The metric registry, ``calc_metric`` and ``report_metric`` with the reference's call signatures and report format
(metrics/metric_main.py:24-77), holding the metrics this package can compute without a pretrained detector network."""

import json
import os
import time

import dnnlib

from . import metric_utils
from . import reconstruction

#----------------------------------------------------------------------------

_metrics = dict()       # name -> function of MetricOptions returning {result key: float}

def register_metric(fn):
    assert callable(fn)
    _metrics[fn.__name__] = fn
    return fn

def is_valid_metric(metric):
    return metric in _metrics

def list_valid_metrics():
    return list(_metrics)

#----------------------------------------------------------------------------

def calc_metric(metric, **kwargs):
    """``calc_metric(metric, G=, dataset_kwargs=, num_gpus=, rank=, device=, progress=None)`` (the arguments of
    ``metric_utils.MetricOptions``) on every rank -> EasyDict(results, metric, total_time, total_time_str, num_gpus).  Every rank
    ends with the same results: they are computed from partial sums that the ranks have exchanged."""
    if not is_valid_metric(metric):
        raise ValueError('unknown metric %r; valid metrics: %s' % (metric, ', '.join(list_valid_metrics())))
    opts = metric_utils.MetricOptions(**kwargs)
    start_time = time.time()
    results = _metrics[metric](opts)
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
