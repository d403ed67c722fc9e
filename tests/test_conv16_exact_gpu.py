"""16-bit-storage convolutions (io_dtype fp16 / bf16) against an fp64 CPU reference, at channel tails, partial pixel tiles, odd planes, K
slices, transposed remainder rows and with every epilogue operand (tests/conv16_cases.py holds the cases, the data and the reference).

Exact leg, NO tolerance: the data lie on dyadic grids such that every product and every partial sum is exact in fp32, so whatever the kernel's
summation order its fp32 value is the mathematically exact one: every 16-bit output (forward, input gradient) must equal the fp64 reference
rounded once, bit for bit, and every weight-gradient element the reference itself.  One dropped, doubled or misplaced term, or a store that
truncates or rounds twice, fails.

Generic leg: normal activations and unrounded fp32 weights (the packing kernels' rounding, which integers hide), held to
``storage_ref.assert_stored`` / ``assert_reduced``.

Every launch is recorded through ``conv2d_gradfix.launch_hook`` and checked against the planner: the launch judged was the 16-bit kernel the
table names (or, for the refused descriptors, a converted fp32 launch)."""

import numpy as np
import pytest
import torch

import conv16_cases as C
import storage_ref as sr

pytestmark = pytest.mark.gpu

IDS = [c.name for c in C.CASES]
ACT_CODE = {'linear': 1, 'relu': 2, 'lrelu': 3}         # bias_act.activation_funcs[...].cuda_idx


class _Recorder:
    """conv2d_gradfix.launch_hook for the duration of a ``with`` block: keeps (kind, a copy of the descriptor, flags) of every launch."""

    def __enter__(self):
        from torch_utils.ops import conv2d_gradfix as cg
        self.cg, self.old, self.launches = cg, cg.launch_hook, []
        cg.launch_hook = self._hook
        return self

    def _hook(self, kind, desc, launch, flags):
        self.launches.append((kind, type(desc).from_buffer_copy(desc), flags))
        launch()

    def __exit__(self, *exc):
        self.cg.launch_hook = self.old
        return False


def _check_launches(case, dtype, launches, keys):
    """The recorded launches are the table's ``keys`` ('fwd', 'dx': forward-type launches; 'dw': the weight gradient), in order: native ones carry
    the storage type and get the table's kernel from the planner, refused ones were converted to fp32 tensors."""
    from torch_utils.ops import conv2d_gradfix as cg
    kinds = ['wgrad' if l[0] == 'wgrad' else 'conv' for l in launches]
    assert kinds == ['wgrad' if k == 'dw' else 'conv' for k in keys], (kinds, keys)
    for key, (kind, desc, flags) in zip(keys, launches):
        if case.expect[key] is None:
            assert desc.io_dtype == cg.IO_CODES[torch.float32], f'{key}: the planner refuses this descriptor, the launch must be a converted one'
        else:
            assert desc.io_dtype == cg.IO_CODES[dtype], f'{key}: converted to fp32 tensors, the table says native'
            assert C.plan('wgrad' if kind == 'wgrad' else 'conv', desc, flags) == case.expect[key], key


def _run(case, d, dtype):
    """-> (y, dx, dw) with every launch checked against the table.  An autograd node computes the gradient of every input that required one when it
    was recorded, whichever is asked for, so the two gradients -- which take different output gradients (conv16_cases.exact_data) -- come from
    two forward passes: one with x alone requiring a gradient, one with w alone."""
    dx = dw = None
    with _Recorder() as rec:
        y, x, _ = _forward(case, d, dtype, 'dx' in case.expect, False)
        if 'dx' in case.expect:
            dx, = torch.autograd.grad(y, x, _dev(d['dy_x'], dtype))
        torch.cuda.synchronize()
    _check_launches(case, dtype, rec.launches, [k for k in ('fwd', 'dx') if k in case.expect])
    if 'dw' in case.expect:
        with _Recorder() as rec:
            y2, _, w = _forward(case, d, dtype, False, True)
            dw, = torch.autograd.grad(y2, w, _dev(d['dy_w'], dtype))
            torch.cuda.synchronize()
        _check_launches(case, dtype, rec.launches, ['fwd', 'dw'])
        assert torch.equal(y2, y)
    return y, dx, dw


def _dev(t, dtype):
    return t.to(dtype).cuda()


def _forward(case, d, dtype, x_grad, w_grad):
    """-> (y, x, w) through the public operators (plain cases) or conv2d_gradfix._launch_conv (the operand cases)."""
    from torch_utils.ops import conv2d_gradfix as cg
    x = _dev(d['x'], dtype).requires_grad_(x_grad)
    w = _dev(d['w'], torch.float32).requires_grad_(w_grad)
    if not case.ops:
        if case.transposed:
            y = cg.conv_transpose2d(x, w, stride=case.stride, padding=case.pad, output_padding=case.outpad, groups=case.groups, wgain=case.wgain)
        else:
            y = cg.conv2d(x, w, stride=case.stride, padding=case.pad, groups=case.groups, wgain=case.wgain)
        return y, x, w
    kw = {}
    if 'iscale' in d:
        kw['iscale'] = _dev(d['iscale'], torch.float32)
    if 'oscale' in d:
        kw['oscale'] = _dev(d['oscale'], torch.float32)
    if any(k in d for k in ('bias', 'res', 'noise')):
        act = ('lrelu', d['alpha'], d['gain'], C.exact_reference(case.name, dtype)[1].clamp) if 'act' in d else ('linear', 0.0, 1.0, -1.0)
        kw['epilogue'] = (_dev(d['bias'], torch.float32) if 'bias' in d else None, ACT_CODE[act[0]], act[1], act[2], act[3],
                          _dev(d['res'], dtype) if 'res' in d else None)
    if 'noise' in d:
        kw['noise'] = (_dev(d['noise'], torch.float32), _dev(d['strength'], torch.float32))
    if 'styles' in d:
        kw['wmod'] = (_dev(d['styles'], torch.float32), _dev(d['dcoefs'], torch.float32) if 'dcoefs' in d else None)
    with torch.no_grad():
        return cg._launch_conv(x, w, C.cfg_of(case), **kw), x, w


def _assert_bitwise(got, ref, dtype, what):
    assert got.dtype == dtype, (what, got.dtype)
    g, r = got.detach().cpu().to(torch.float64).numpy(), sr.rne(ref.numpy(), dtype)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = ~(g == r)
    if bad.any():
        i = np.flatnonzero(bad.ravel())
        j = np.unravel_index(int(i[0]), g.shape)
        raise AssertionError(f'{what}: {len(i)} of {g.size} elements differ from the fp64 reference rounded once to {dtype}; first at {j}: '
                             f'got {g[j]!r}, want {r[j]!r} (reference {float(ref[j])!r})')


def _assert_equal_f32(got, ref, what):
    assert got.dtype == torch.float32, (what, got.dtype)
    g, r = got.detach().cpu().to(torch.float64), ref
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bad = ~(g == r)
    if bool(bad.any()):
        j = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {g.numel()} elements differ from the fp64 reference; first at {j}: got {float(g[j])!r}, want {float(r[j])!r}')


@pytest.mark.parametrize('dtype', C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize('case', C.CASES, ids=IDS)
def test_exact_data_gives_the_reference_bit_for_bit(case, dtype):
    from torch_utils.ops import conv2d_gradfix as cg
    d, ref = C.exact_reference(case.name, dtype)
    if case.kind == 'wgrad':
        with _Recorder() as rec:
            dw = cg._launch_wgrad(_dev(d['x'], dtype), _dev(d['dy_w'], dtype), C.cfg_of(case), C.w_shape(case), out_dtype=torch.float32)
            torch.cuda.synchronize()
        _check_launches(case, dtype, rec.launches, ['dw'])
        y = dx = None
    else:
        y, dx, dw = _run(case, d, dtype)
    for key, got, want, scale in (('fwd', y, ref.y, ref.scale), ('dx', dx, ref.dx, ref.dx_scale)):
        if got is None:
            continue
        if case.expect[key] is not None:
            _assert_bitwise(got, want, dtype, f'{case.name} {key}')
        else:       # a converted launch (fp32 copies, the fp32-equivalent arithmetic): held to the storage bound of the generic leg
            assert got.dtype == dtype
            sr.assert_stored(got, want, dtype, scale, k=C.products(case, key) + 4, what=f'{case.name} {key} (converted)')
    if dw is not None:
        _assert_equal_f32(dw, ref.dw, f'{case.name} dw')       # (exact in the converted launches too: the grids fit every arithmetic's operand pieces)


@pytest.mark.parametrize('dtype', C.DTYPES, ids=C.DTYPE_IDS)
@pytest.mark.parametrize('name', C.GENERIC)
def test_generic_data_within_one_fp32_evaluation_and_one_rounding(name, dtype):
    case = C.BY_NAME[name]
    d, ref = C.generic_reference(name, dtype)
    y, dx, dw = _run(case, d, dtype)
    # Only native 16-bit launches are judged here (the forward launch of every generic case is one; ``_run`` has checked it).  A gradient the
    # planner refuses runs as a converted launch in the fp32-equivalent three-product arithmetic, whose operand pieces are not one rounding of
    # the operand: the bounds below do not describe it, and the fp32-storage tests (tests/test_conv_precision_gpu.py) are what holds it.
    # a sum of K exact products in any order has at most K - 1 roundings on its longest chain; the epilogue adds at most four
    sr.assert_stored(y, ref.y, dtype, ref.scale, k=C.products(case, 'fwd') + 4, what=f'{name} fwd')
    if dx is not None and case.expect['dx'] is not None:
        sr.assert_stored(dx, ref.dx, dtype, ref.dx_scale, k=C.products(case, 'dx') + 4, what=f'{name} dx')
    if dw is not None and case.expect['dw'] is not None:
        # n = N P Q exact products per element.  The split kernels sum a chunk of 32 pixels inside one matrix-core instruction, chunks one after
        # another within a K slice, slices in a second kernel: the depth is far below n, but the order inside the instruction is not documented,
        # so the bound taken is the one valid for ANY order, lanes = 1 (a chain of n additions), extra = 2 for the reduce kernel's sum and the
        # weight gain.
        assert dw.dtype == torch.float32
        n = case.xs[0] * (case.xs[2] * case.xs[3] if case.transposed else int(np.prod(C.out_hw(case))))
        sr.assert_reduced(dw, ref.dw, ref.dw_scale, n=n, lanes=1, extra=2, what=f'{name} dw')
