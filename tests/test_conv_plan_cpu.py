"""conv2d_gradfix._plan, the one memoised query of the convolution planners: its answers are the planners' own, and its cache never
lets two descriptors that differ in a field the planners read share an entry.  Host-only entry points of the library; no device."""

import ctypes
import itertools

import pytest

from torch_utils import custom_ops
from torch_utils.ops import conv2d_gradfix as cg

SHAPES = [   # cfg, (N, C_in, H, W), C_out, kh
    (cg._Cfg((False, 1, 1, 1, 0, 0, 1, 1.0)), (16, 128, 128, 128), 128, 3),   # 3x3 stride 1: the eight-wave tile (pieces)
    (cg._Cfg((False, 2, 0, 0, 0, 0, 1, 1.0)), (16, 64, 257, 257), 128, 3),    # 3x3 stride 2, pad 0: the stride-2 kernel (pieces)
    (cg._Cfg((False, 1, 0, 0, 0, 0, 1, 1.0)), (16, 128, 64, 64), 128, 1),     # pointwise (second input tensor)
    (cg._Cfg((False, 1, 0, 0, 0, 0, 1, 1.0)), (4, 3, 64, 64), 64, 1),         # few input channels
    (cg._Cfg((True, 2, 0, 0, 0, 0, 1, 1.0)), (16, 128, 64, 64), 64, 3),       # transposed stride 2: the one-pass kernel
    (cg._Cfg((False, 1, 1, 1, 0, 0, 4, 0.5)), (1, 64, 8, 8), 64, 3),          # grouped, weight gain
]


def _descs():
    for (cfg, x_shape, c_out, k), layout, x2, io, math in itertools.product(SHAPES, (0, 1), (False, True), cg.IO_CODES, cg.MATH_CODES.values()):
        oh, ow = cg._out_hw(cfg, x_shape[2], x_shape[3], k, k)
        d = cg._desc(cfg, x_shape, c_out, oh, ow, k, k, io)
        d.math, d.x_layout = math, layout
        if x2:
            d.x2, d.C1 = 0x1000, x_shape[1] // 2       # the planners read whether x2 is set, never through it
        yield d


def _direct(lib, kind, d, flags):
    kernel, math = ctypes.c_int(), ctypes.c_int()
    if kind == 'conv':
        ok = lib.pasta_conv2d_plan(ctypes.byref(d), flags, None, None, ctypes.byref(math), None, ctypes.byref(kernel)) == 0
        return ok, kernel.value if ok else None, math.value if ok else None, lib.pasta_conv2d_workspace(ctypes.byref(d))
    if kind == 'wgrad':
        ok = lib.pasta_conv2d_wgrad_plan(ctypes.byref(d), ctypes.byref(kernel)) == 0
        return ok, kernel.value if ok else None, None, lib.pasta_conv2d_wgrad_workspace(ctypes.byref(d))
    nbytes = lib.pasta_conv2d_wgrad_modulated_workspace(ctypes.byref(d))
    return nbytes >= 0, None, None, nbytes


def test_plan_answers_as_the_planners(monkeypatch):
    monkeypatch.setattr(cg, '_plan_cache', {})
    lib = custom_ops.get_plugin()
    seen = set()
    for d in _descs():
        queries = [('conv', f) for f in range(32)] + [('wgrad', 0), ('wgrad_modulated', 0)]
        for kind, flags in queries:
            want = _direct(lib, kind, d, flags)
            assert tuple(cg._plan(kind, d, flags)) == want, (kind, flags, cg._desc_key(d))
            assert tuple(cg._plan(kind, d, flags)) == want         # ... and again from the cache
            seen.add((kind, want[0], want[1]))
    # the grid reaches accepted and refused descriptors, and the kernels of the pieces layout and of the second input tensor
    assert {('conv', True, 7), ('conv', True, 9), ('conv', True, 10), ('conv', True, 13), ('wgrad', True, 6), ('conv', False, None)} <= seen


@pytest.mark.parametrize('field', [f for f, _ in custom_ops.ConvDesc._fields_])
def test_plan_cache_keys_on_every_field(monkeypatch, field):
    monkeypatch.setattr(cg, '_plan_cache', {})
    cfg, x_shape, c_out, k = SHAPES[0]
    base = cg._desc(cfg, x_shape, c_out, x_shape[2], x_shape[3], k, k)
    other = custom_ops.ConvDesc.from_buffer_copy(base)
    value = getattr(base, field)
    if field in cg._DESC_PTRS:
        setattr(other, field, 0x1000)
    elif isinstance(value, float):
        setattr(other, field, value * 2)
    else:
        setattr(other, field, value + 1)
    assert cg._desc_key(other) != cg._desc_key(base)
    for d in (base, other):
        cg._plan('conv', d, 4)
    assert len(cg._plan_cache) == 2
    # a pointer field enters the key as null / non-null only: another address is the same entry
    if field in cg._DESC_PTRS:
        setattr(other, field, 0x2000)
        cg._plan('conv', other, 4)
        assert len(cg._plan_cache) == 2
