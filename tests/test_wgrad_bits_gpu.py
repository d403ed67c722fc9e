"""The weight-gradient kernels keep their bits: for the smallest shapes at which each shared piece of the family can go wrong (slice bounds,
chunk walker, ring slots, operand scales, the split, the slab store, the reductions), the SHA-256 of the fp32 bytes ``cg._launch_wgrad`` /
``cg._launch_wgrad_modulated`` return must equal the digest in tests/golden/wgrad_bits.npz, recorded on the MI355X from the kernels as they
stood before their staging, slicing and slab stores were single-sourced.  Each case also holds the planner to its kernel id and K-slice count
(that test carries no gpu mark and runs without one; where the table says "as planned" -- kernels 1, 5 and 6 -- the slice count is the one
the fixture recorded, so for those four cases it pins the planner against its own earlier answer, not against an independent figure).

The fixture is tied to the compiler: what it fuses and in which order it schedules fp32 additions is part of the bits.  When the toolchain
changes, re-record it from a tree whose fp64 accuracy tests pass:  python tests/test_wgrad_bits_gpu.py --record
(every case is launched twice; nothing is written if two runs differ)."""
import contextlib
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'wgrad_bits.npz')

# (id, kind, k, stride, pad, transposed, groups, N, C_in, C_out, H, kernel id, K slices or None = as planned (held by the fixture))
SHAPES = [
    ('s1-2x40-72@32', 'plain', 3, 1, 1, False, 1, 2, 40, 72, 32, 2, 8),        # a tail in a and b, slices beginning mid-column, XCD order
    ('s1-3x40-72@32', 'plain', 3, 1, 1, False, 1, 3, 40, 72, 32, 2, 12),       # workgroup order 0, a slice crossing an image
    ('s1-1x24-40@64', 'plain', 3, 1, 1, False, 1, 1, 24, 40, 64, 2, 16),       # two column blocks per row
    ('s1-5x72-40@16', 'plain', 3, 1, 1, False, 1, 5, 72, 40, 16, 2, 10),       # half-filled chunks, two b tiles
    ('s1-g2-2x48-80@32', 'plain', 3, 1, 1, False, 2, 2, 48, 80, 32, 2, 8),     # group offsets of S, L and slab
    ('s2-2x32-64@33', 'plain', 3, 2, 0, False, 1, 2, 32, 64, 33, 3, 4),        # odd plane, dword halo loads
    ('s2-2x40-72@65', 'plain', 3, 2, 0, False, 1, 2, 40, 72, 65, 3, 16),       # two column blocks, channel tails
    ('s2-p1-1x24-130@64', 'plain', 3, 2, 1, False, 1, 1, 24, 130, 64, 3, 8),   # pad 1, three a tiles
    ('s2-t-2x72-40@32', 'plain', 3, 2, 0, True, 1, 2, 72, 40, 32, 3, 16),      # operand roles swapped
    ('1x1-2x64-40@32', 'plain', 1, 1, 0, False, 1, 2, 64, 40, 32, 4, 8),       # 64 x 64 tile
    ('1x1-2x192-130@32', 'plain', 1, 1, 0, False, 1, 2, 192, 130, 32, 4, 8),   # 128 x 128 tile, both tails
    ('1x1-3x130-130@16', 'plain', 1, 1, 0, False, 1, 3, 130, 130, 16, 4, 3),   # slices not a multiple of 8
    ('f32-2x24-72@24', 'plain', 3, 1, 1, False, 1, 2, 24, 72, 24, 0, 6),       # fp32 MFMA: slice bounds, tap groups
    ('f32-7x7-1x16-40@24', 'plain', 7, 1, 3, False, 1, 1, 16, 40, 24, 0, 3),   # 1 x 7 tap groups
    ('small-7x7-2x3-40@32', 'plain', 7, 1, 3, False, 1, 2, 3, 40, 32, 1, None),
    ('few-1x1-2x3-40@32', 'plain', 1, 1, 0, False, 1, 2, 3, 40, 32, 5, None),
    ('pieces-5x24-48@128', 'pieces', 3, 2, 0, False, 1, 5, 24, 48, 129, 6, None),     # H: the blurred plane (128 + 2 + 2 - 3)
    ('mod-4x40-72@32', 'modulated', 3, 1, 1, False, 1, 4, 40, 72, 32, 2, 16),   # sample-aligned slices
]
SPLIT = [('bf16x6', 'f32'), ('bf16x3', 'f32'), ('bf16', 'f32'), ('f16x3', 'f32'), ('default', 'f16'), ('default', 'bf16')]   # (arithmetic, storage)
DTYPES = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}


def _variants(shape):
    kind, kernel = shape[1], shape[11]
    if kind != 'plain' or kernel == 6:
        return [('f16x3', 'f32')]
    return {0: [('f32', 'f32')], 1: [('f32', 'f32')], 5: [('f32', 'f32'), ('default', 'f16')]}.get(kernel, SPLIT)


CASES = [(s, v) for s in SHAPES for v in _variants(s)]
_key = lambda case: '%s|%s|%s' % (case[0][0], case[1][0], case[1][1])


@contextlib.contextmanager
def _arith(name):
    from torch_utils.ops import conv2d_gradfix as cg
    old, cg.conv_math = cg.conv_math, name
    try:
        yield cg
    finally:
        cg.conv_math = old


def _geometry(shape):
    """cfg, x shape, dy shape, weight shape of one table row."""
    from torch_utils.ops import conv2d_gradfix as cg
    _, kind, k, st, pad, tr, groups, n, ci, co, h = shape[:11]
    cfg = cg._Cfg((tr, st, pad, pad, 0, 0, groups, 1.0))
    oh, ow = cg._out_hw(cfg, h, h, k, k)
    w_shape = (ci, co // groups, k, k) if tr else (co, ci // groups, k, k)
    return cfg, (n, ci, h, h), (n, co, oh, ow), w_shape


def plan_of(case):
    """(kernel id, K slices) the planner gives the case: the slab part of the workspace is ksplit . G . kh kw . padded A . padded B floats
    (kernels 1 and 5: ksplit . padded C_out . padded C_in kh kw)."""
    shape, (arith, store) = case
    kind, k, groups, n, ci, co, kernel = shape[1], shape[2], shape[6], shape[7], shape[8], shape[9], shape[11]
    with _arith(arith) as cg:
        cfg, xs, ys, _ = _geometry(shape)
        desc = cg._desc(cfg, xs, ys[1], ys[2], ys[3], k, k, DTYPES[store])
        desc.x_layout = int(kind == 'pieces')
        plan = cg._plan('wgrad', desc)
        floats = plan.workspace // 4 - 2 * cg.AMAX_PARTS
        if kind == 'modulated':
            floats = cg._plan('wgrad_modulated', desc).workspace // 4 - 2 * cg.AMAX_PARTS
    up = lambda v, m: (v + m - 1) // m * m
    if kernel in (1, 5):
        per = up(co, 64) * up(ci * k * k, 32)
    else:
        ag, bg = (ci // groups, co // groups) if cfg.transposed else (co // groups, ci // groups)
        tile = 128 if k == 1 and ag > 64 and bg > 64 else 64
        ap, bp = up(ag, tile), up(bg, tile)
        per = groups * k * k * ap * bp
        if kind == 'modulated':     # the partial style gradients follow the slabs: one [N][C_in] block per (4 or 16 rows a) x tap
            rows = 16 if (bp // 64) * (ap // 16) * k * k >= 512 else 4
            floats -= ap // rows * k * k * n * ci
    assert floats % per == 0, (floats, per)
    return plan.kernel, floats // per


def compute(case):
    """SHA-256 digests of what the launch returns: (dw,) or (dw, ds)."""
    shape, (arith, store) = case
    kind, k = shape[1], shape[2]
    rng = np.random.default_rng(sum(shape[2:11]) * 131 + len(shape[0]))
    with _arith(arith) as cg:
        cfg, xs, ys, w_shape = _geometry(shape)
        dy = torch.from_numpy((rng.standard_normal(ys) * 0.013).astype(np.float32)).cuda().to(DTYPES[store])
        if kind == 'pieces':
            from torch_utils.ops import upfirdn2d
            x = torch.from_numpy((rng.standard_normal((xs[0], xs[1], xs[2] - 1, xs[3] - 1)) * 1.7).astype(np.float32)).cuda()
            pieces, bound, lshape = cg.blur_pieces(x, upfirdn2d.setup_filter([1, 3, 3, 1]).cuda(), (2, 2, 2, 2))
            assert tuple(lshape) == xs
            outs = (cg._launch_wgrad(pieces, dy, cfg, w_shape, torch.float32, pieces=(bound, lshape)),)
        else:
            x = torch.from_numpy((rng.standard_normal(xs) * 1.7).astype(np.float32)).cuda().to(DTYPES[store])
            if kind == 'modulated':
                s = torch.from_numpy(rng.uniform(0.5, 2.0, xs[:2]).astype(np.float32)).cuda()
                w = torch.from_numpy((rng.standard_normal(w_shape) * 0.05).astype(np.float32)).cuda()
                outs = cg._launch_wgrad_modulated(x, dy, cfg, s, w)
            else:
                outs = (cg._launch_wgrad(x, dy, cfg, w_shape, torch.float32),)
    for o in outs:
        assert o.dtype == torch.float32 and bool(torch.isfinite(o).all()) and float(o.abs().max()) > 0
    return tuple(np.frombuffer(hashlib.sha256(o.contiguous().cpu().numpy().tobytes()).digest(), dtype=np.uint8) for o in outs)


@pytest.mark.parametrize('case', CASES, ids=_key)
def test_planner_gives_the_tabled_kernel_and_slices(case):
    kernel, slices = plan_of(case)
    want = case[0][12] if case[0][12] is not None else int(np.load(GOLDEN)[_key(case) + '|slices'])
    assert (kernel, slices) == (case[0][11], want)


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=_key)
def test_weight_gradient_returns_the_recorded_bits(case):
    golden = np.load(GOLDEN)
    got = compute(case)
    for name, digest in zip(('dw', 'ds'), got):
        assert np.array_equal(digest, golden[_key(case) + '|' + name]), (name, 'arithmetic order changed')


if __name__ == '__main__':
    assert sys.argv[1:] == ['--record'], 'usage: test_wgrad_bits_gpu.py --record'
    out = {}
    for case in CASES:
        kernel, slices = plan_of(case)
        assert kernel == case[0][11] and case[0][12] in (None, slices), (_key(case), kernel, slices)
        first, second = compute(case), compute(case)
        assert len(first) == len(second) and all(np.array_equal(a, b) for a, b in zip(first, second)), (_key(case), 'two runs differ: nothing written')
        out[_key(case) + '|slices'] = np.int32(slices)
        for name, digest in zip(('dw', 'ds'), first):
            out[_key(case) + '|' + name] = digest
        print(_key(case), kernel, slices, first[0][:4].tobytes().hex())
    np.savez(GOLDEN, **out)
    print('recorded', len(CASES), 'cases ->', GOLDEN)
