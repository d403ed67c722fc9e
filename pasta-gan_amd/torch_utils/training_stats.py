"""Training statistics with the interface of the reference's torch_utils/training_stats.py (``init_multiprocessing``,
``report``, ``report0``, ``Collector``): any part of the training code reports named scalars, a ``Collector`` turns what was
reported since its last ``update()`` into count, mean and standard deviation, summed over all ranks.

Kept off the hot path: the moments (count, sum, sum of squares) of values that live on the GPU accumulate in one float64
table on that GPU, a row per name; ``report`` queues a few tiny launches and never synchronises.  ``Collector.update()`` is
the only read-back -- one copy of the table to the host, after one all-reduce when there are several ranks.  Values that are
already on the host (the loop's timings) accumulate in a host table."""

import re

import numpy as np
import torch

import dnnlib

_NUM_MOMENTS = 3                # count, sum, sum of squares
_rank = 0
_sync_device = None             # the device of the all-reduce; None: one process
_names = []                     # row order of every table, the same on all ranks (they run the same program)
_rows = {}                      # name -> row
_host = np.zeros([0, _NUM_MOMENTS], np.float64)     # moments reported from the host since the last synchronisation
_device = {}                    # torch.device -> [rows, 3] float64 table on that device, same meaning
_cumulative = np.zeros([0, _NUM_MOMENTS], np.float64)       # everything ever synchronised, all ranks

#----------------------------------------------------------------------------

def init_multiprocessing(rank, sync_device):
    """Call once per process before anything is reported: ``rank`` of this process and the device its all-reduces run on
    (None when there is only one process)."""
    global _rank, _sync_device
    assert not _names, 'init_multiprocessing() after the first report()'
    _rank = rank
    _sync_device = sync_device

def _row(name):
    global _host, _cumulative
    row = _rows.get(name)
    if row is None:
        row = _rows[name] = len(_names)
        _names.append(name)
        grow = np.zeros([1, _NUM_MOMENTS], np.float64)
        _host, _cumulative = np.concatenate([_host, grow]), np.concatenate([_cumulative, grow])
    return row

def _table(device, rows):
    table = _device.get(device)
    if table is None or table.shape[0] < rows:
        grown = torch.zeros([max(rows, 64), _NUM_MOMENTS], dtype=torch.float64, device=device)      # grows during the first iteration only
        if table is not None:
            grown[:table.shape[0]] = table
        table = _device[device] = grown
    return table

@torch.no_grad()
def report(name, value):
    """Add ``value`` (a scalar, a sequence or a tensor; every element counts) to the statistics of ``name``.  Returns ``value``.
    All ranks must report the same names in the same order."""
    assert re.fullmatch(r'[A-Za-z0-9_./]+', name), name
    row = _row(name)
    if isinstance(value, torch.Tensor) and value.device.type != 'cpu':
        if value.numel() > 0:
            elems = value.detach().flatten().to(torch.float64)
            table = _table(value.device, row + 1)
            table[row, 0] += elems.numel()          # a kernel argument: nothing is copied to the device
            table[row, 1:] += torch.stack([elems.sum(), elems.square().sum()])
        return value
    elems = np.asarray(value.detach().numpy() if isinstance(value, torch.Tensor) else value, np.float64).reshape(-1)
    if elems.size > 0:
        _host[row] += [elems.size, elems.sum(), np.square(elems).sum()]
    return value

def report0(name, value):
    """``report`` by rank 0 alone (the other ranks register the name and add nothing).  Returns ``value``."""
    report(name, value if _rank == 0 else [])
    return value

def _sync():
    """Move everything reported since the last call, from all ranks, into ``_cumulative``: one read-back."""
    global _host
    rows = len(_names)
    delta = _host.copy()
    _host[:] = 0
    for device in list(_device):
        _table(device, rows)                # names registered since the table was made
    if _sync_device is not None:            # host moments ride in the same all-reduce
        flat = torch.from_numpy(np.concatenate([delta, [[rows, 0, 0]]])).to(_sync_device)      # the last row: the number of names
        for device, table in _device.items():
            flat[:rows] += table[:rows].to(_sync_device)
            table.zero_()
        torch.distributed.all_reduce(flat)
        flat = flat.cpu().numpy()           # the read-back
        assert flat[rows, 0] == rows * torch.distributed.get_world_size(), 'the ranks reported different names'
        delta = flat[:rows]
    elif _device:
        tables = list(_device.values())
        flat = tables[0][:rows] if len(tables) == 1 else sum(t[:rows].to(tables[0].device) for t in tables)
        delta += flat.cpu().numpy()        # the read-back
        for table in tables:
            table.zero_()
    _cumulative[:rows] += delta

#----------------------------------------------------------------------------

class Collector:
    """Statistics of the names matching ``regex`` over the interval between the last two ``update()`` calls.  With
    ``keep_previous``, a name nobody reported during an interval keeps the figures of the interval before."""

    def __init__(self, regex='.*', keep_previous=True):
        self._regex = re.compile(regex)
        self._keep_previous = keep_previous
        self._seen = {}         # name -> cumulative moments at the last update
        self._moments = {}      # name -> moments of the last interval
        self.update()
        self._moments.clear()

    def names(self):
        return [name for name in _names if self._regex.fullmatch(name)]

    def update(self):
        """Close the interval: synchronises with the other ranks and reads the counters back (once)."""
        if not self._keep_previous:
            self._moments.clear()
        _sync()
        for name in self.names():
            total = _cumulative[_rows[name]].copy()
            delta = total - self._seen.get(name, 0.0)
            self._seen[name] = total
            if delta[0] != 0:
                self._moments[name] = delta

    def _get(self, name):
        assert self._regex.fullmatch(name), name
        return self._moments.get(name, np.zeros([_NUM_MOMENTS], np.float64))

    def num(self, name):
        return int(self._get(name)[0])

    def mean(self, name):
        m = self._get(name)
        return float(m[1] / m[0]) if int(m[0]) != 0 else float('nan')

    def std(self, name):
        m = self._get(name)
        if int(m[0]) == 0 or not np.isfinite(float(m[1])):
            return float('nan')
        if int(m[0]) == 1:
            return 0.0
        mean = float(m[1] / m[0])
        return float(np.sqrt(max(float(m[2] / m[0]) - np.square(mean), 0)))

    def as_dict(self):
        return dnnlib.EasyDict((name, dnnlib.EasyDict(num=self.num(name), mean=self.mean(name), std=self.std(name))) for name in self.names())

    def __getitem__(self, name):
        return self.mean(name)

#----------------------------------------------------------------------------
