"""Record what the convolution planners answer over a grid of descriptors -> tests/golden/conv_plan_table.npz.

The planners (pasta_conv2d_plan, pasta_conv2d_workspace, pasta_conv2d_wgrad_plan, pasta_conv2d_wgrad_workspace,
pasta_conv2d_wgrad_modulated_workspace; include/pasta_hip.h) are pure host arithmetic on a descriptor, so the table is recorded and compared
without a device.  tests/test_conv_plan_table_cpu.py holds the library to the stored table: a refactor of the planner must not move one entry,
and a pull request that changes a plan on purpose records the table again with this tool and says so.

The grid: the six shapes of tests/test_conv_plan_cpu.py (with and without a second input tensor), every launch of tests/conv16_cases.py, and
the shapes of EXTRA below, which reach the forward kernels 0 - 13 and the weight-gradient kernels 0 - 6 that those leave out; each crossed
with the three storage types, the math codes and both x_layout values.

    python tools/conv_plan_table.py            # record
    python tools/conv_plan_table.py --check    # compare the library of this tree with the stored table (what the test does)
"""

import argparse
import ctypes
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, 'pasta-gan_amd'), os.path.join(ROOT, 'tests')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PATH = os.path.join(ROOT, 'tests', 'golden', 'conv_plan_table.npz')
IO_CODES = (0, 1, 3)                      # PASTA_F32, PASTA_F16, PASTA_BF16
MATH_CODES = (0, 1, 2, 3, 4, 5)           # PASTA_MATH_DEFAULT (= F16X3), F32, BF16X6, BF16X3, BF16, F16X3
INT_FIELDS = ('N', 'C_in', 'H', 'W', 'C_out', 'OH', 'OW', 'kh', 'kw', 'stride', 'pad_h', 'pad_w', 'groups', 'transposed', 'flip', 'math',
              'io_dtype', 'x2', 'C1', 'x_layout')     # x2: set or null (the planners never read through it)
FWD_COLUMNS = ('ok', 'tile', 'ksplit', 'math', 'launches', 'kernel')
NFLAGS = 32

# (transposed, stride, pad, outpad, groups), (N, C_in, H, W), C_out, k
EXTRA = [
    ((False, 1, 3, 0, 1), (1, 3, 96, 96), 64, 7),          # 7x7 RGB stem: the packed-K mode with a padded copy
    ((False, 1, 0, 0, 1), (1, 3, 102, 102), 64, 7),        # ... without padding: the input itself serves
    ((False, 1, 1, 0, 1), (4, 512, 4, 4), 512, 3),         # 4x4 and 8x8 layers: K slices
    ((False, 1, 1, 0, 1), (1, 64, 8, 8), 64, 3),
    ((False, 1, 1, 0, 1), (16, 512, 8, 8), 512, 3),
    ((True, 2, 1, 1, 1), (2, 32, 32, 32), 64, 3),          # stride-2 transposed onto 2H: the pair launch
    ((True, 2, 0, 0, 1), (2, 32, 32, 32), 64, 3),          # onto 2H + 1 below 128 x 128
    ((True, 2, 0, 0, 1), (8, 16, 32, 32), 64, 3),          # ... the one-pass kernel's smallest planes
    ((True, 2, 0, 0, 1), (2, 32, 30, 32), 64, 3),          # ... planes the one-pass kernel does not tile: merged classes
    ((True, 2, 0, 0, 1), (1, 32, 128, 128), 64, 3),        # onto 2H + 1 at 128 x 128
    ((True, 2, 0, 0, 1), (1, 32, 132, 128), 64, 3),        # ... planes the one-pass kernel does not tile: the pair launch with its remainder
    ((True, 2, 0, 0, 1), (1, 128, 132, 128), 128, 3),
    ((True, 3, 1, 0, 1), (2, 24, 11, 9), 72, 3),           # stride-3 transposed: one launch per class
    ((True, 4, 0, 0, 1), (1, 32, 9, 9), 64, 4),
    ((False, 1, 1, 0, 1), (3, 24, 16, 16), 40, 3),         # 16-pixel rows: wide16
    ((False, 1, 1, 0, 1), (16, 512, 16, 16), 512, 3),
    ((False, 1, 0, 0, 1), (2, 8, 64, 64), 16, 1),          # 1x1 with <= 16 channels on either side
    ((False, 1, 0, 0, 1), (2, 16, 64, 64), 8, 1),
    ((False, 1, 0, 0, 1), (2, 64, 64, 64), 3, 1),
    ((True, 1, 0, 0, 1), (2, 3, 64, 64), 64, 1),
    ((False, 1, 1, 0, 2), (1, 48, 95, 93), 80, 3),         # grouped
    ((False, 1, 1, 0, 4), (2, 64, 32, 32), 64, 3),
    ((False, 1, 1, 0, 1), (2, 3, 32, 32), 32, 3),          # few input channels, 3x3: the small-cin weight gradient
    ((False, 1, 1, 0, 1), (2, 32, 32, 32), 64, 3),         # the shapes of tests/test_conv_workspace_gpu.py
    ((False, 1, 1, 0, 1), (2, 32, 32, 32), 32, 3),
    ((False, 2, 1, 0, 1), (2, 32, 64, 64), 64, 3),         # 3x3 stride 2, pad 1
    ((False, 1, 2, 0, 1), (2, 32, 24, 24), 32, 5),         # 5x5: the fp32-MFMA weight gradient
    ((False, 1, 0, 0, 1), (2, 32, 31, 31), 32, 4),         # 4x4
]


def _base_descs():
    """(N, C_in, H, W, C_out, OH, OW, kh, kw, stride, pad_h, pad_w, groups, transposed, wscale, x2) of every shape of the grid, once each."""
    import conv16_cases as cc
    import test_conv_plan_cpu as tp
    from torch_utils.ops import conv2d_gradfix as cg
    seen, out = set(), []

    def add(d, x2=False):
        key = (d.N, d.C_in, d.H, d.W, d.C_out, d.OH, d.OW, d.kh, d.kw, d.stride, d.pad_h, d.pad_w, d.groups, d.transposed, float(d.wscale), bool(x2))
        if key not in seen:
            seen.add(key)
            out.append(key)

    for cfg, xs, c_out, k in tp.SHAPES:
        oh, ow = cg._out_hw(cfg, xs[2], xs[3], k, k)
        for x2 in (False, True):
            add(cg._desc(cfg, xs, c_out, oh, ow, k, k), x2)
    for case in cc.CASES:
        for _, d, _ in cc.launch_descs(case, cc.DTYPES[0]).values():
            add(d)
    for (tr, stride, pad, outpad, groups), xs, c_out, k in EXTRA:
        cfg = cg._Cfg((tr, stride, pad, pad, outpad, outpad, groups, 1.0))
        oh, ow = cg._out_hw(cfg, xs[2], xs[3], k, k)
        d = cg._desc(cfg, xs, c_out, oh, ow, k, k)
        add(d)
        gcfg = cg._grad_cfg(cfg, xs[2:], (oh, ow), k, k)       # ... and its input-gradient launch
        add(cg._desc(gcfg, (xs[0], c_out, oh, ow), xs[1], xs[2], xs[3], k, k))
    return out


def grid():
    """-> (int32 [n, len(INT_FIELDS)], float32 [n]): every descriptor of the grid."""
    rows, wscale = [], []
    for base, io, math, layout in itertools.product(_base_descs(), IO_CODES, MATH_CODES, (0, 1)):
        n, c_in, h, w, c_out, oh, ow, kh, kw, stride, ph, pw, groups, tr, ws, x2 = base
        rows.append((n, c_in, h, w, c_out, oh, ow, kh, kw, stride, ph, pw, groups, tr, 0, math, io, int(x2), c_in // 2 if x2 else 0, layout))
        wscale.append(ws)
    return np.asarray(rows, dtype=np.int32), np.asarray(wscale, dtype=np.float32)


def make_desc(row, wscale):
    from torch_utils import custom_ops
    f = dict(zip(INT_FIELDS, (int(v) for v in row)))
    x2 = f.pop('x2')
    d = custom_ops.ConvDesc(wscale=float(wscale), **f)
    if x2:
        d.x2 = 0x1000
    return d


def answers(lib, descs, wscale):
    """The planners' answers: fwd int32 [n, NFLAGS, 6] (fields the planner did not write: -1), ws int64 [n, 5] = forward workspace,
    weight-gradient plan accepted, its kernel (-1: not written), weight-gradient workspace, modulated weight-gradient workspace."""
    fwd = np.full((len(descs), NFLAGS, len(FWD_COLUMNS)), -1, dtype=np.int32)
    ws = np.zeros((len(descs), 5), dtype=np.int64)
    for i, (row, s) in enumerate(zip(descs, wscale)):
        d = make_desc(row, s)
        ref = ctypes.byref(d)
        for flags in range(NFLAGS):
            out = [ctypes.c_int(-1) for _ in range(5)]
            status = lib.pasta_conv2d_plan(ref, flags, *(ctypes.byref(o) for o in out))
            fwd[i, flags] = [int(status == 0)] + [o.value for o in out]
        kernel = ctypes.c_int(-1)
        status = lib.pasta_conv2d_wgrad_plan(ref, ctypes.byref(kernel))
        ws[i] = (lib.pasta_conv2d_workspace(ref), int(status == 0), kernel.value, lib.pasta_conv2d_wgrad_workspace(ref),
                 lib.pasta_conv2d_wgrad_modulated_workspace(ref))
    return fwd, ws


def load():
    with np.load(PATH) as z:
        manifest = json.loads(bytes(z['manifest']).decode())
        assert tuple(manifest['int_fields']) == INT_FIELDS and tuple(manifest['fwd_columns']) == FWD_COLUMNS
        return z['desc'], z['wscale'], z['fwd'], z['ws']


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--check', action='store_true', help='compare with the stored table instead of writing it')
    args = ap.parse_args()
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()
    if args.check:
        descs, wscale, fwd0, ws0 = load()
        fwd, ws = answers(lib, descs, wscale)
        bad = np.flatnonzero((fwd != fwd0).any(axis=(1, 2)) | (ws != ws0).any(axis=1))
        for i in bad[:20]:
            print('differs:', dict(zip(INT_FIELDS, descs[i].tolist())))
        print('%d of %d descriptors differ' % (len(bad), len(descs)))
        sys.exit(1 if len(bad) else 0)
    descs, wscale = grid()
    fwd, ws = answers(lib, descs, wscale)
    manifest = {'int_fields': INT_FIELDS, 'fwd_columns': FWD_COLUMNS,
                'ws_columns': ['conv2d_workspace', 'wgrad_plan ok', 'wgrad_plan kernel', 'wgrad_workspace', 'wgrad_modulated_workspace'],
                'flags': 'axis 1 of fwd: the launch_flags value (PASTA_PLAN_*) 0 .. 31', 'abi': custom_ops.EXPECTED_ABI}
    np.savez_compressed(PATH, desc=descs, wscale=wscale, fwd=fwd, ws=ws, manifest=np.frombuffer(json.dumps(manifest).encode(), dtype=np.uint8))
    ok = fwd[:, :, 0] == 1
    print('%d descriptors, %d bytes' % (len(descs), os.path.getsize(PATH)))
    print('forward kernels:', sorted(set(fwd[:, :, 5][ok].tolist())), ' weight-gradient kernels:', sorted(set(ws[:, 2][ws[:, 1] == 1].tolist())))


if __name__ == '__main__':
    main()
