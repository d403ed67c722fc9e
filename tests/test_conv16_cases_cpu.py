"""The case table of the 16-bit-storage convolution tests (tests/conv16_cases.py), checked on the host: the planners give every case the
kernel the table names, the table reaches every kernel cell the planners can answer for a 16-bit descriptor, and the references make the
bitwise comparison meaningful (their outputs need rounding, are not zero, and the generic data's own fp32 evaluation rounds to the
reference almost everywhere).  Host-only entry points of the library; no device."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import conv16_cases as C
import storage_ref as sr

IDS = [c.name for c in C.CASES]


@pytest.mark.parametrize('dtype', C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_planner_gives_each_case_the_kernel_the_table_names(case, dtype):
    got = {k: C.plan(*v) for k, v in C.launch_descs(case, dtype).items()}
    assert got == case.expect


def _cells(kind, desc, answer):
    return (kind, answer[0], answer[1], bool(desc.transposed))


def test_table_reaches_every_16bit_kernel_cell_the_planners_answer():
    """Sweep 16-bit descriptors; every accepted (launch kind, kernel, K sliced?, transposed?) must be the cell of some table case's launch."""
    from torch_utils import custom_ops
    from torch_utils.ops import conv2d_gradfix as cg
    lib = custom_ops.get_plugin()
    covered = set()
    for case in C.CASES:
        for dtype in C.DTYPES:
            for kind, desc, flags in C.launch_descs(case, dtype).values():
                a = C.plan(kind, desc, flags)
                if a is not None:
                    covered.add(_cells(kind, desc, a))
    planes = sorted({c.xs[2:] for c in C.CASES} | {C.out_hw(c) for c in C.CASES})
    flag_sets = sorted({C.plan_flags(c) for c in C.CASES if 'iscale' not in c.ops})
    assert len(flag_sets) >= 6
    found = {}
    kernel, ks = ctypes.c_int(), ctypes.c_int()
    for transposed, stride, (kh, kw), pad, groups in itertools.product((False, True), (1, 2, 3), ((1, 1), (1, 3), (3, 3)), (0, 1), (1, 2)):
        if pad >= stride + max(kh, kw) - 1:
            continue
        cfg = cg._Cfg((transposed, stride, pad if kh > 1 else 0, pad, 0, 0, groups, 1.0))      # (a 1 x 3 kernel pads its rows only)
        for (h, w), n in itertools.product(planes, (1, 3, 16)):
            oh, ow = cg._out_hw(cfg, h, w, kh, kw)
            if oh < 1 or ow < 1:
                continue
            for ci, co, dtype in itertools.product((8, 16, 24, 64), (8, 24, 40, 72, 136), C.DTYPES):
                d = cg._desc(cfg, (n, ci * groups, h, w), co * groups, oh, ow, kh, kw, dtype)
                ref = ctypes.byref(d)
                for flags in flag_sets:
                    if lib.pasta_conv2d_plan(ref, flags, None, ctypes.byref(ks), None, None, ctypes.byref(kernel)) == 0:
                        found.setdefault(('conv', kernel.value, ks.value > 1, transposed), (cg._desc_key(d), flags))
                a = C.plan('wgrad', d)
                if a is not None:
                    found.setdefault(_cells('wgrad', d, a), (cg._desc_key(d), 0))
    assert len(found) >= 10
    missing = {cell: where for cell, where in found.items() if cell not in covered}
    assert not missing, f'16-bit kernel cells without a case in tests/conv16_cases.py: {missing}'


@pytest.mark.parametrize('dtype', C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_exact_reference_is_exact_and_not_vacuous(case, dtype):
    """The premises of the bitwise comparison, from the reference alone: operands representable in the storage type, every fp32 step exact
    (``reference(exact=True)`` asserts it), at least a quarter of the outputs in need of rounding, at least 90 % nonzero before the activation."""
    d, ref = C.exact_reference(case.name, dtype)
    for key in ('x', 'dy_x', 'dy_w', 'res'):
        if key in d:
            assert torch.equal(sr.rounded(d[key], dtype), d[key]), key
    w = C.effective_weights(case, d)
    assert torch.equal(sr.rounded(w, dtype), w), 'the weights the matrix cores multiply are not representable in the operand type'
    if case.kind == 'conv':
        assert float((ref.pre != 0).double().mean()) >= 0.9
        assert C.needs_rounding(ref.y, dtype) >= 0.25
        if ref.clamp is not None:
            share = float((ref.y.abs() == ref.clamp).double().mean())
            assert 0 < share < 0.5, share                       # some outputs exceed the clamp, most do not
            assert torch.equal(sr.rounded(torch.tensor([ref.clamp]), dtype), torch.tensor([ref.clamp], dtype=torch.float64))
    if ref.dx is not None:
        assert C.needs_rounding(ref.dx, dtype) >= 0.25
    if ref.dw is not None:
        assert float((ref.dw != 0).double().mean()) >= 0.9


@pytest.mark.parametrize('dtype', C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize('name', C.GENERIC)
def test_generic_data_rounds_to_the_reference_almost_everywhere(name, dtype):
    """torch's own fp32 convolution of the generic data, rounded once, equals the rounded fp64 reference on at least 0.995 of the elements:
    the 0.99 the GPU test demands of the kernels is then a demand on their store, not on the data."""
    case = C.BY_NAME[name]
    d, ref = C.generic_reference(name, dtype)
    w = C.effective_weights(case, d, C.generic_operand_dtype(case, dtype, case.expect['fwd'][0]))
    y32 = C._conv(case, d['x'].to(torch.float32), w.to(torch.float32)).to(torch.float64)
    same = float((sr.rne(y32, dtype) == sr.rne(ref.y, dtype)).mean())
    assert same >= 0.995, same
    sr.assert_stored(torch.from_numpy(sr.rne(y32, dtype)), ref.y, dtype, ref.scale, k=C.products(case, 'fwd') + 4, what=name)
    if case.expect.get('dx') is not None:           # the input gradient the GPU test judges the same way
        x32 = d['x'].to(torch.float32).requires_grad_(True)
        dx32, = torch.autograd.grad(C._conv(case, x32, w.to(torch.float32)), x32, d['dy_x'].to(torch.float32))
        dx32 = dx32.to(torch.float64)
        same = float((sr.rne(dx32, dtype) == sr.rne(ref.dx, dtype)).mean())
        assert same >= 0.995, same
        sr.assert_stored(torch.from_numpy(sr.rne(dx32, dtype)), ref.dx, dtype, ref.dx_scale, k=C.products(case, 'dx') + 4, what=name + ' dx')


def _forward_cells(names):
    return {(C.BY_NAME[n].expect['fwd'], C.BY_NAME[n].transposed) for n in names if C.BY_NAME[n].expect.get('fwd') is not None}


def test_generic_leg_reaches_every_forward_cell_of_the_table():
    """(kernel, K sliced?, transposed?) of the native forward launches: the generic cases cover what the table covers, and one of them is modulated."""
    assert _forward_cells(C.GENERIC) == _forward_cells(c.name for c in C.CASES)
    assert any('wmodd' in C.BY_NAME[n].ops for n in C.GENERIC)
