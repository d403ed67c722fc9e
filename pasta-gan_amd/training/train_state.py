"""The training-state file: everything an interrupted run needs to go on bit for bit.

A network snapshot (``network-snapshot-*.pkl``) holds G, D, G_ema and the augmentation pipeline, which is what ``--resume``
warm-starts from.  ``training-state-*.pt`` is self-contained and adds what a continuation needs: both Adam optimisers'
moments and step counts, ``cur_nimg`` / ``batch_idx`` / ``cur_tick``, the wall clock so far, the ADA accumulator, the sample
grid's latents and every rank's random generators (and its ``w_avg`` buffers, which the ranks do not share).

The file is written with ``torch.save`` and read with ``torch.load(..., map_location='cpu', weights_only=True)``: tensors,
numbers, strings, lists and dicts, no pickled classes."""

import io
import os

import numpy as np
import torch

from torch_utils import misc

FORMAT = 1
MODULES = ('G', 'D', 'G_ema', 'augment_pipe')
CHECKED = ('num_gpus', 'batch_size', 'batch_gpu', 'random_seed')       # a continued run must have these as the file has them

#----------------------------------------------------------------------------
# plain containers

def _plain(obj, where='state'):
    """``obj`` with every dict subclass as a dict and every tuple as a list; anything that would need a pickled class is refused."""
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    if isinstance(obj, (np.integer, np.floating, np.bool_)):
        return obj.item()
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu()
    if isinstance(obj, dict):
        for key in obj:
            if not isinstance(key, (int, str)):
                raise TypeError(f'{where}: key {key!r} is neither an integer nor a string')
        return {key: _plain(value, f'{where}[{key!r}]') for key, value in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_plain(value, f'{where}[{i}]') for i, value in enumerate(obj)]
    raise TypeError(f'{where}: {type(obj).__name__} cannot be stored in a training-state file')

def numpy_rng_to_plain(state):
    """``np.random.get_state()`` / ``RandomState.get_state()`` as its key string, a uint32 tensor and plain numbers."""
    kind, keys, pos, has_gauss, cached_gaussian = state
    return dict(kind=str(kind), keys=torch.from_numpy(np.array(keys, dtype=np.uint32)), pos=int(pos), has_gauss=int(has_gauss),
                cached_gaussian=float(cached_gaussian))

def numpy_rng_from_plain(plain):
    return (plain['kind'], plain['keys'].numpy().astype(np.uint32), int(plain['pos']), int(plain['has_gauss']), float(plain['cached_gaussian']))

#----------------------------------------------------------------------------
# what a TrainingStep contributes

def _optimizers(step):
    """{'G': optimiser, 'D': optimiser}: one entry per distinct optimiser (Gmain and Greg share one)."""
    opts = {}
    for phase in step.phases:
        opts.setdefault(phase.name[0], phase.opt)
        assert opts[phase.name[0]] is phase.opt
    return opts

def _modules(step):
    return {name: getattr(step, name) for name in MODULES if getattr(step, name) is not None}

def _own_buffers(step):
    """The buffers every rank keeps for itself (``w_avg``: a running mean over the rank's own batches, exempt from the
    replica check of the snapshots): {module name: {tensor name: tensor}}."""
    return {name: {k: t.detach().cpu() for k, t in module.named_buffers() if k.rsplit('.', 1)[-1] == 'w_avg'}
            for name, module in _modules(step).items() if name in ('G', 'G_ema')}

def rank_entry(step):
    """This rank's own part of the state: its three random generators, its ADA accumulator, its ``w_avg`` buffers."""
    entry = dict(torch_rng=torch.get_rng_state(), numpy_rng=numpy_rng_to_plain(np.random.get_state()), buffers=_own_buffers(step))
    if step.device.type == 'cuda':
        entry['cuda_rng'] = torch.cuda.get_rng_state(step.device)
    if getattr(step, '_ada_acc', None) is not None:
        entry['ada_acc'] = step._ada_acc.detach().cpu()
    return entry

def _gather_entries(step, entry):
    """Every rank's entry on rank 0 (None elsewhere): the serialised entries as int32 rows of one all-reduced table, which
    the training step's transports (RCCL, and gloo on device tensors) both carry."""
    buf = io.BytesIO()
    torch.save(entry, buf)
    mine = torch.frombuffer(bytearray(buf.getvalue()), dtype=torch.uint8)
    size = torch.tensor([mine.numel()], dtype=torch.int64, device=step.device)
    longest = size.clone()
    torch.distributed.all_reduce(longest, op=torch.distributed.ReduceOp.MAX)
    table = torch.zeros([step.num_gpus, int(longest) + 1], dtype=torch.int32, device=step.device)
    table[step.rank, 0] = mine.numel()
    table[step.rank, 1:1 + mine.numel()] = mine.to(step.device)
    torch.distributed.all_reduce(table)
    if step.rank != 0:
        return None
    table = table.cpu()
    entries = []
    for row in table:
        data = row[1:1 + int(row[0])].to(torch.uint8).numpy().tobytes()
        entries.append(torch.load(io.BytesIO(data), map_location='cpu', weights_only=True))
    return entries

def collect(step):
    """The entries of the state file that come from the step.  A collective with more than one rank: every rank calls it,
    rank 0 gets the state and the others None."""
    entry = _plain(rank_entry(step), 'ranks')
    ranks = _gather_entries(step, entry) if step.num_gpus > 1 else [entry]
    if step.rank != 0:
        return None
    state = dict(cur_nimg=int(step.cur_nimg), batch_idx=int(step.batch_idx), num_gpus=int(step.num_gpus), batch_size=int(step.batch_size),
                 batch_gpu=int(step.batch_gpu), ranks=ranks)
    for name, module in _modules(step).items():
        state[name] = {k: t.detach().cpu() for k, t in misc.named_params_and_buffers(module)}
    state['opt'] = {name: opt.state_dict() for name, opt in _optimizers(step).items()}
    return state

#----------------------------------------------------------------------------
# the file

def save_state(path, step, extras):
    """Write ``extras`` (a dict: cur_tick, elapsed_sec, random_seed, options, grid_z, ...) and, with a ``step``, what
    ``collect`` takes from it, to ``path``; atomically (``<path>.tmp``, then ``os.replace``).  With more than one rank every
    rank calls this and rank 0 writes.  Returns the path, or None on the ranks that do not write."""
    state = dict(extras)
    if step is not None:
        collected = collect(step)
        if collected is None:
            return None
        state.update(collected)
    state['format'] = FORMAT
    state = _plain(state)
    tmp = str(path) + '.tmp'
    torch.save(state, tmp)
    os.replace(tmp, path)
    return path

def load_state(path, mmap=False):
    """The state of ``path``, every tensor on the host.  ``mmap``: tensors are mapped, not read (for a look at the numbers)."""
    state = torch.load(path, map_location='cpu', weights_only=True, mmap=bool(mmap))
    if not isinstance(state, dict) or state.get('format') != FORMAT:
        found = state.get('format') if isinstance(state, dict) else None
        raise ValueError(f'{path}: training-state format {found!r}, this code reads format {FORMAT}')
    return state

def check_run(state, **given):
    """A continued run keeps the number of GPUs, the batch sizes and the seed of the run it continues."""
    for name in CHECKED:
        if name in given and given[name] != state[name]:
            raise ValueError(f'resume_state: {name}={given[name]!r}, but the state file was written with {name}={state[name]!r}')

#----------------------------------------------------------------------------
# back into a TrainingStep

def _copy_named(source, named, where):
    """``source`` {name: tensor} into the tensors of ``named`` [(name, tensor)]: the same names and shapes on both sides."""
    named = list(named)
    missing = [name for name, _ in named if name not in source]
    extra = sorted(set(source) - {name for name, _ in named})
    if missing or extra:
        raise ValueError(f'{where}: ' + '; '.join(part for part in ('missing from the state file: ' + ', '.join(missing) if missing else '',
                                                                  'not in this run\'s module: ' + ', '.join(extra) if extra else '') if part))
    with torch.no_grad():
        for name, dst in named:
            src = source[name]
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f'{where}.{name}: {tuple(src.shape)} {src.dtype} in the state file, {tuple(dst.shape)} {dst.dtype} in this run')
            dst.copy_(src)

def restore(step, state):
    """Everything but the random generators: modules, optimisers, counters, this rank's ADA accumulator and ``w_avg``.
    ``step._buf_versions`` stays empty, so the first iteration copies G's (equal) buffers into G_ema once more."""
    modules = _modules(step)
    for name in MODULES:
        if (name in modules) != (name in state):
            raise ValueError(f'{name}: ' + ('missing from the state file' if name in modules else 'in the state file, but this run has none'))
    for name, module in modules.items():
        _copy_named(state[name], misc.named_params_and_buffers(module), name)
    opts = _optimizers(step)
    if sorted(opts) != sorted(state['opt']):
        raise ValueError(f'opt: {sorted(state["opt"])} in the state file, {sorted(opts)} in this run')
    for name, opt in opts.items():
        opt.load_state_dict(state['opt'][name])
    step.cur_nimg, step.batch_idx = int(state['cur_nimg']), int(state['batch_idx'])
    step._buf_versions = {}
    entry = state['ranks'][step.rank]
    for name, buffers in entry['buffers'].items():
        own = [(k, t) for k, t in modules[name].named_buffers() if k.rsplit('.', 1)[-1] == 'w_avg']
        _copy_named(buffers, own, f'ranks[{step.rank}].buffers.{name}')
    has_acc = getattr(step, '_ada_acc', None) is not None
    if has_acc != ('ada_acc' in entry):
        raise ValueError('ada_acc: ' + ('missing from the state file' if has_acc else 'in the state file, but this run does not adapt p'))
    if has_acc:
        step._ada_acc.copy_(entry['ada_acc'])

def restore_rng(step, state):
    """This rank's generators; the last thing before the first ``step.run``."""
    entry = state['ranks'][step.rank]
    np.random.set_state(numpy_rng_from_plain(entry['numpy_rng']))
    torch.set_rng_state(entry['torch_rng'])
    if 'cuda_rng' in entry:
        torch.cuda.set_rng_state(entry['cuda_rng'], step.device)

#----------------------------------------------------------------------------
# the files of a run directory

def state_files(run_dir):
    """[(kimg, path)] of the ``training-state-<kimg>.pt`` files of a directory, lowest kimg first."""
    import re
    found = []
    for name in os.listdir(run_dir):
        m = re.fullmatch(r'training-state-(\d+)\.pt', name)
        if m:
            found.append((int(m.group(1)), os.path.join(run_dir, name)))
    return sorted(found)

#----------------------------------------------------------------------------
