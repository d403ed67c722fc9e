"""Cases, data and fp64 references for the 16-bit-storage convolutions (io_dtype fp16 / bf16: the stored element is the matrix-core
operand, one product per multiply-add, fp32 accumulation and epilogue, one rounding on the way out).

EXACT data: activations, weights and every epilogue operand lie on short dyadic grids, such that every operand is representable in the
storage type and every partial sum, in any order, in fp32 (``sum |x||w|`` over the grid unit stays below 2^24; ``reference`` checks
it).  The fp32 value a kernel forms is then the mathematically exact one whatever its summation order, K slicing, tile or parity
class, and the stored result must equal the fp64 reference rounded once -- bit for bit, no tolerance.  Weight gradients stay fp32 and
must equal the reference exactly.

GENERIC data (``generic_data``): normal activations rounded to the storage type and unrounded fp32 weights, which exercise the weight
rounding of the packing kernels that integers hide; held to ``storage_ref.assert_stored``.

Each case names the plan kernel (include/pasta_hip.h: pasta_conv2d_plan / pasta_conv2d_wgrad_plan) and whether K is sliced, for its
forward, input-gradient and weight-gradient launch; tests/test_conv16_cases_cpu.py holds the planners to the table and shows that the
table reaches every (launch kind, kernel, K-sliced, transposed) cell the planners can answer for a 16-bit descriptor.

A plain module imported by the tests (no fixtures)."""

import collections
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

import storage_ref as sr

DTYPES = [torch.float16, torch.bfloat16]
DTYPE_IDS = ['fp16', 'bf16']

# ``ops``: what the forward launch carries besides x, w (through conv2d_gradfix._launch_conv)
#   'oscale'  a per-(sample, channel) output scale          'epi'     bias, lrelu (alpha 0.25), gain, clamp
#   'res'     a residual (with a linear epilogue)            'noise1'  one noise plane      'noiseN'  one noise plane per sample
#   'wmod'    modulated weights (styles)                     'wmodd'   modulated weights (styles and dcoefs)
#   'iscale'  an input scale (no 16-bit kernel takes one: the launch is converted)
# ``expect``: {'fwd' | 'dx' | 'dw': (plan kernel id, K sliced?)}; None in place of the pair = the planner refuses the 16-bit descriptor and
# the wrapper converts that launch to fp32 tensors.  A case without 'dx' / 'dw' runs the forward launch only; kind 'wgrad' cases run the
# weight gradient only (conv2d_gradfix._launch_wgrad).  The K-sliced flag of weight-gradient kernel 5 is None (it has no split workspace
# to tell it from).
Case = collections.namedtuple('Case', 'name kind transposed xs cout k stride pad outpad groups wgain ops expect')


def _c(name, xs, cout, expect, kind='conv', transposed=False, k=3, stride=1, pad=1, outpad=0, groups=1, wgain=1.0, ops=()):
    return Case(name, kind, transposed, tuple(xs), cout, k, stride, pad, outpad, groups, wgain, tuple(ops), expect)


OPS_ALL = ('oscale', 'epi', 'res', 'noiseN')                       # everything a plain-weight launch can carry at once
OPS_ALL_MOD = ('epi', 'res', 'noise1', 'wmodd')                    # ... and a modulated one (it takes no scale vectors)
OPERAND_SETS = [('oscale',), ('epi',), ('res',), ('noise1',), ('noiseN',), ('wmod',), ('wmodd',), OPS_ALL, OPS_ALL_MOD]

CASES = []


def _add(*a, **kw):
    CASES.append(_c(*a, **kw))


def _operand_cases(base, xs, cout, fwd, **kw):
    """``base`` with each operand set; the forward launch only.  ``fwd``: the expectation, or {ops: expectation} with a default under None."""
    for ops in OPERAND_SETS:
        e = fwd.get(ops, fwd[None]) if isinstance(fwd, dict) else fwd
        _add(f'{base}+{"+".join(ops)}', xs, cout, {'fwd': e}, ops=ops, **kw)


# ---- forward-type launches (3x3, pad 1, stride 1 unless said otherwise) -------------------------------------------------------------------
# F1: base kernel on the 64 x 256 tile; 24 -> 40 channels (both with tails) over an odd plane whose last pixel tile is partial
_add('F1_base_64x256', [1, 24, 95, 93], 40, {'fwd': (1, False), 'dx': (1, False), 'dw': None}, wgain=0.5)
# F2: 17..32 output channels take the 64-row tile half empty (so that 16-bit tensors are not converted)
_add('F2_base_64x256_half', [1, 24, 95, 93], 24, {'fwd': (1, False), 'dx': (1, False), 'dw': None})
# F3: base kernel on the 128 x 128 tile with K slices: the reduce kernel's 16-bit store
_add('F3_base_128_ksplit', [1, 48, 17, 13], 72, {'fwd': (1, True), 'dx': None, 'dw': None}, wgain=2.0)
# F4: row-reuse kernel, both tiles
_add('F4_rows_128', [2, 16, 33, 128], 72, {'fwd': (2, False), 'dx': None, 'dw': (2, True)})
_add('F4_rows_64x256', [11, 16, 12, 64], 40, {'fwd': (2, False), 'dx': None, 'dw': (2, True)})
# F5: the three 2-D row tiles
_add('F5_rows2d_r4', [3, 24, 44, 64], 72, {'fwd': (4, False), 'dx': (2, False), 'dw': (2, True)})
_add('F5_rows2d_r2', [2, 24, 66, 64], 72, {'fwd': (5, False), 'dx': (1, False), 'dw': (2, True)})
_add('F5_rows2d_r8', [3, 16, 88, 32], 40, {'fwd': (6, False), 'dx': None, 'dw': (2, True)})
# F6: a 2-D tile shape under K slices
_add('F6_small_plane_ksplit', [1, 32, 8, 32], 72, {'fwd': (4, True), 'dx': None, 'dw': (2, False)})
_add('F6_rows_ksplit', [1, 32, 3, 128], 72, {'fwd': (2, True), 'dx': None, 'dw': (2, False)})               # an odd number of 128-pixel rows: no 2-D tile
_add('F6_rows2d_r2_ksplit', [1, 32, 6, 64], 72, {'fwd': (5, True), 'dx': None, 'dw': (2, False)})
# ... and the 2-D tiles as conv_transpose2d (stride 1: one lattice, mirrored taps)
_add('F5_rows2d_r4_transposed', [3, 24, 44, 64], 72, {'fwd': (4, False), 'dx': (2, False), 'dw': (2, True)}, transposed=True)
_add('F5_rows2d_r2_transposed', [2, 24, 66, 64], 72, {'fwd': (5, False), 'dx': (1, False), 'dw': (2, True)}, transposed=True)
_add('F5_rows2d_r8_transposed', [3, 16, 88, 32], 40, {'fwd': (6, False), 'dx': None, 'dw': (2, True)}, transposed=True)
# F7: the few-channel 1x1 kernels, both directions
_add('F7_fewch_in', [1, 8, 91, 92], 40, {'fwd': (11, False), 'dx': (12, False), 'dw': (5, None)}, k=1, pad=0)
_add('F7_fewch_out', [3, 24, 52, 53], 8, {'fwd': (12, False), 'dx': (11, False), 'dw': None}, k=1, pad=0)
# F8: groups
_add('F8_groups', [1, 48, 95, 93], 80, {'fwd': (1, False), 'dx': (1, False), 'dw': None}, groups=2)
# F9: conv_transpose2d stride 2, the four parity classes in one grid
_add('F9_t2_pad0_odd', [4, 24, 47, 45], 40, {'fwd': (1, False), 'dx': (1, False), 'dw': None}, transposed=True, stride=2, pad=0)
_add('F9_t2_pad1_outpad', [4, 24, 47, 45], 40, {'fwd': (1, False), 'dx': (1, False), 'dw': None}, transposed=True, stride=2, pad=1, outpad=1)
_add('F9_t2_small_ksplit', [1, 128, 9, 7], 72, {'fwd': (1, True), 'dx': (1, True), 'dw': None}, transposed=True, stride=2, pad=0)
# F10: conv_transpose2d stride 3: one launch per class
_add('F10_t3_per_class', [2, 24, 11, 9], 72, {'fwd': (1, False), 'dx': None, 'dw': None}, transposed=True, stride=3, pad=1)
# F11: stride-2 conv2d, pad 0, odd plane; its input gradient is a transposed launch with output padding
_add('F11_s2_pad0_odd', [4, 24, 96, 94], 40, {'fwd': (1, False), 'dx': (1, False), 'dw': None}, stride=2, pad=0)
# F12: descriptors the planner refuses: the wrapper converts the launch
_add('F12_iscale', [1, 24, 95, 93], 40, {'fwd': None}, ops=('iscale',))
_add('F12_tile64', [1, 24, 17, 13], 40, {'fwd': None, 'dx': None, 'dw': None})

_operand_cases('F1', [1, 24, 95, 93], 40, (1, False), wgain=0.5)
_operand_cases('F3', [1, 48, 17, 13], 72, (1, True), wgain=2.0)
_operand_cases('F5r4', [3, 24, 44, 64], 72, (4, False))
_operand_cases('F9', [4, 24, 47, 45], 40, (1, False), transposed=True, stride=2, pad=0)
_add('F8_groups+wmodd', [1, 48, 95, 93], 80, {'fwd': (1, False)}, groups=2, ops=('wmodd',))

# ---- weight gradients (dw stays fp32) -----------------------------------------------------------------------------------------------------
_add('W1_3x3', [2, 24, 12, 32], 40, {'dw': (2, True)}, kind='wgrad')
_add('W1_3x3_tiles', [2, 80, 12, 32], 72, {'dw': (2, True)}, kind='wgrad')
_add('W2_3x3_wide16', [3, 24, 16, 16], 40, {'dw': (2, True)}, kind='wgrad')
_add('W3_3x3s2_pad0', [2, 24, 33, 33], 40, {'dw': (3, True)}, kind='wgrad', stride=2, pad=0)
_add('W3_3x3s2_pad1', [2, 24, 32, 32], 40, {'dw': (3, True)}, kind='wgrad', stride=2, pad=1)
_add('W4_1x1', [1, 24, 17, 32], 40, {'dw': (4, True)}, kind='wgrad', k=1, pad=0)
_add('W4_1x1_2x2', [1, 80, 34, 16], 72, {'dw': (4, True)}, kind='wgrad', k=1, pad=0)
_add('W5_1x1_fewcin', [3, 8, 10, 6], 40, {'dw': (5, None)}, kind='wgrad', k=1, pad=0)
_add('W6_transposed_s1', [2, 24, 12, 32], 40, {'dw': (2, True)}, kind='wgrad', transposed=True)
_add('W6_transposed_s2', [2, 24, 16, 16], 40, {'dw': (3, True)}, kind='wgrad', transposed=True, stride=2, pad=1, outpad=1)
_add('W3_3x3s2_single', [1, 24, 8, 32], 40, {'dw': (3, False)}, kind='wgrad', stride=2, pad=1)
_add('W4_1x1_single', [1, 24, 5, 32], 40, {'dw': (4, False)}, kind='wgrad', k=1, pad=0)
_add('W6_transposed_s1_single', [1, 24, 8, 32], 40, {'dw': (2, False)}, kind='wgrad', transposed=True)
_add('W6_transposed_1x1', [1, 24, 17, 32], 40, {'dw': (4, True)}, kind='wgrad', transposed=True, k=1, pad=0)
_add('W6_transposed_1x1_single', [1, 24, 5, 32], 40, {'dw': (4, False)}, kind='wgrad', transposed=True, k=1, pad=0)
_add('W6_transposed_s2_single', [1, 24, 4, 16], 40, {'dw': (3, False)}, kind='wgrad', transposed=True, stride=2, pad=0)
_add('W7_refused_row24', [2, 24, 12, 24], 40, {'dw': None}, kind='wgrad')

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# one case per forward kernel cell for the generic leg (plus a modulated launch)
GENERIC = ['F1_base_64x256', 'F1+wmodd', 'F3_base_128_ksplit', 'F4_rows_128', 'F4_rows_64x256', 'F5_rows2d_r4', 'F5_rows2d_r2', 'F5_rows2d_r8',
           'F6_small_plane_ksplit', 'F6_rows_ksplit', 'F6_rows2d_r2_ksplit',
           'F5_rows2d_r4_transposed', 'F5_rows2d_r2_transposed', 'F5_rows2d_r8_transposed', 'F7_fewch_in', 'F7_fewch_out', 'F9_t2_pad0_odd', 'F9_t2_small_ksplit', 'F10_t3_per_class', 'F11_s2_pad0_odd']

# ---- shapes and descriptors ---------------------------------------------------------------------------------------------------------------


def _cg():
    from torch_utils.ops import conv2d_gradfix as cg
    return cg


def cfg_of(case):
    return _cg()._Cfg((case.transposed, case.stride, case.pad, case.pad, case.outpad, case.outpad, case.groups, float(case.wgain)))


def out_hw(case):
    return _cg()._out_hw(cfg_of(case), case.xs[2], case.xs[3], case.k, case.k)


def w_shape(case):
    """The weight tensor; with modulated weights ONE group's weights, shared by the groups."""
    g = case.groups
    shared = g if any(o in case.ops for o in ('wmod', 'wmodd')) else 1
    if case.transposed:
        return (case.xs[1] // shared, case.cout // g, case.k, case.k)
    return (case.cout // shared, case.xs[1] // g, case.k, case.k)


def products(case, key):
    """Products per output element of the 'fwd' or 'dx' launch, at most: the input channels of a group times the taps that reach one output --
    all k x k of a conv2d, ceil(k / stride)^2 of a transposed launch (one output parity class)."""
    c = case.cout if key == 'dx' else case.xs[1]
    transposed = case.transposed if key == 'fwd' else not case.transposed
    taps = (-(-case.k // case.stride)) ** 2 if transposed else case.k ** 2
    return c // case.groups * taps


def plan_flags(case):
    cg = _cg()
    f = 0
    for o in case.ops:
        f |= {'oscale': cg.PLAN_OSCALE, 'epi': cg.PLAN_EPILOGUE, 'res': cg.PLAN_EPILOGUE, 'noise1': cg.PLAN_EPILOGUE | cg.PLAN_NOISE,
              'noiseN': cg.PLAN_EPILOGUE | cg.PLAN_NOISE, 'wmod': cg.PLAN_MODULATED, 'wmodd': cg.PLAN_MODULATED, 'iscale': cg.PLAN_ISCALE}[o]
    return f


def launch_descs(case, dtype):
    """{'fwd' | 'dx' | 'dw': (planner kind, descriptor, flags)} for the launches of ``case`` in storage type ``dtype``."""
    cg = _cg()
    cfg = cfg_of(case)
    n, c_in, h, w = case.xs
    oh, ow = out_hw(case)
    k = case.k
    out = {}
    if case.kind == 'conv':
        out['fwd'] = ('conv', cg._desc(cfg, case.xs, case.cout, oh, ow, k, k, dtype), plan_flags(case))
        if 'dx' in case.expect:
            gcfg = cg._grad_cfg(cfg, (h, w), (oh, ow), k, k)
            out['dx'] = ('conv', cg._desc(gcfg, (n, case.cout, oh, ow), c_in, h, w, k, k, dtype), 0)
    if 'dw' in case.expect:
        out['dw'] = ('wgrad', cg._desc(cfg, case.xs, case.cout, oh, ow, k, k, dtype), 0)
    return out


def plan(kind, desc, flags=0):
    """The planner's own answer: None where it refuses, else (kernel id, K sliced?)."""
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()
    kernel, ks = ctypes.c_int(), ctypes.c_int()
    if kind == 'conv':
        if lib.pasta_conv2d_plan(ctypes.byref(desc), int(flags), None, ctypes.byref(ks), None, None, ctypes.byref(kernel)) != 0:
            return None
        return kernel.value, ks.value > 1
    if lib.pasta_conv2d_wgrad_plan(ctypes.byref(desc), ctypes.byref(kernel)) != 0:
        return None
    if kernel.value not in (2, 3, 4):
        return kernel.value, None           # (16-bit: kernel 5 only; it has no split workspace to read its slices from)
    # the K slices of the split kernels, from the workspace layout include/pasta_hip.h states (pasta_conv2d_wgrad_plan): 2 x 256 maxima, then one
    # slab per slice of G kh kw (A padded) (B padded) floats, channel tiles of 64, or 128 where kernel 4 has more than 64 channels on both sides
    ag, bg = desc.C_out // desc.groups, desc.C_in // desc.groups
    t = 128 if kernel.value == 4 and ag > 64 and bg > 64 else 64
    slab = desc.groups * desc.kh * desc.kw * (-(-ag // t) * t) * (-(-bg // t) * t)
    floats = lib.pasta_conv2d_wgrad_workspace(ctypes.byref(desc)) // 4 - 512
    assert floats >= slab and floats % slab == 0, (floats, slab)
    return kernel.value, floats // slab > 1


# ---- data ---------------------------------------------------------------------------------------------------------------------------------

# activations k * 2^-e with |k| <= kmax: bf16 has 8 significand bits, fp16 11; the finer fp16 grid is what makes its outputs need rounding
_XGRID = {torch.float16: (6, 1023), torch.bfloat16: (3, 127)}


def _ints(g, shape, kmax):
    return torch.randint(-kmax, kmax + 1, tuple(shape), generator=g).to(torch.float64)


def _pick(g, shape, values):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), tuple(shape), generator=g)]


def _seed(case):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(case.name)) % (2 ** 31)


def exact_data(case, dtype):
    """fp64 CPU tensors on the dyadic grids: x, w, the operands ``case.ops`` names, and two output gradients -- ``dy_x`` on the activation
    grid (for the input gradient, whose 16-bit result must need rounding) and ``dy_w`` on a coarse one (for the weight gradient, a sum over
    every pixel of the batch that has to stay below 2^24 grid units)."""
    g = torch.Generator().manual_seed(_seed(case))
    e, kmax = _XGRID[dtype]
    n, c_in, h, w = case.xs
    oh, ow = out_hw(case)
    d = {'x': _ints(g, case.xs, kmax) * 2.0 ** -e, 'w': _ints(g, w_shape(case), 7)}
    ys = (n, case.cout, oh, ow)
    d['dy_x'] = _ints(g, ys, kmax) * 2.0 ** -e
    d['dy_w'] = _ints(g, ys, 3) * 2.0 ** -3
    ops = case.ops
    if 'oscale' in ops:
        d['oscale'] = _pick(g, (n, case.cout), [0.5, 1.0, 2.0, -1.0, 1.5, -0.5])
    if 'iscale' in ops:
        d['iscale'] = _pick(g, (n, c_in), [0.5, 1.0, 2.0, -1.0])
    if 'epi' in ops:
        d['bias'] = _ints(g, (case.cout,), 63) / 4
        d['act'], d['alpha'], d['gain'], d['clamp'] = 'lrelu', 0.25, (2.0, 0.5)[int(torch.randint(0, 2, (1,), generator=g))], 'auto'
    if 'res' in ops:
        d['res'] = _ints(g, ys, kmax) * 2.0 ** -e
    if 'noise1' in ops:
        d['noise'], d['strength'] = _ints(g, (oh, ow), 15) / 2, torch.tensor(0.5, dtype=torch.float64)
    if 'noiseN' in ops:
        d['noise'], d['strength'] = _ints(g, (n, 1, oh, ow), 15) / 2, torch.tensor(2.0, dtype=torch.float64)
    if 'wmod' in ops or 'wmodd' in ops:
        d['styles'] = _pick(g, (case.groups, c_in // case.groups), [0.5, 1.0, 1.5, 2.0, -1.0, -0.5])
        if 'wmodd' in ops:
            d['dcoefs'] = _pick(g, (case.groups, case.cout // case.groups), [0.5, 1.0, 2.0, -1.0])
    return d


def generic_data(case, dtype):
    """Normal activations (and output gradients) rounded to ``dtype``, fp32 weights of scale 1 / sqrt(K) that are NOT on the 16-bit grid."""
    g = torch.Generator().manual_seed(_seed(case) + 1)
    n, c_in, h, w = case.xs
    oh, ow = out_hw(case)
    ws = w_shape(case)
    fan = (ws[0] if case.transposed else ws[1]) * case.k * case.k / (case.stride ** 2 if case.transposed else 1)
    d = {'x': sr.rounded(torch.randn(case.xs, generator=g), dtype),
         'w': (torch.randn(ws, generator=g) / np.sqrt(fan)).to(torch.float32).to(torch.float64)}
    d['dy_x'] = d['dy_w'] = sr.rounded(torch.randn((n, case.cout, oh, ow), generator=g), dtype)
    if 'wmodd' in case.ops:
        d['styles'] = (1 + 0.5 * torch.randn((case.groups, c_in // case.groups), generator=g)).to(torch.float32).to(torch.float64)
        d['dcoefs'] = (1 + 0.5 * torch.randn((case.groups, case.cout // case.groups), generator=g)).to(torch.float32).to(torch.float64)
    return d


# ---- reference ----------------------------------------------------------------------------------------------------------------------------

def _f32_exact(t, what):
    assert torch.equal(t.to(torch.float32).to(torch.float64), t), f'{what} is not representable in fp32'


def effective_weights(case, d, operand_dtype=None):
    """The weights the matrix cores multiply, [C_out, C_in / G, k, k] ([C_in, C_out / G, k, k] transposed), fp64: w * wgain, modulated per group
    ((w * wgain) * s) * d as the packing kernels form it (csrc/conv_pack.h).  ``operand_dtype``: the product is formed in fp32 and rounded
    once to that type (generic data; on the exact grids nothing rounds)."""
    w = d['w']
    lo = (lambda t: t.to(torch.float32)) if operand_dtype is not None else (lambda t: t)
    v = lo(w) * lo(torch.tensor(case.wgain, dtype=torch.float64))
    if 'styles' in d:
        g = case.groups
        v = v.unsqueeze(0).expand(g, *v.shape).clone()                       # [G, O | I, I | O, k, k]
        s, dc = lo(d['styles']), (lo(d['dcoefs']) if 'dcoefs' in d else None)
        if case.transposed:
            v = v * s[:, :, None, None, None]
            v = v * dc[:, None, :, None, None] if dc is not None else v
        else:
            v = v * s[:, None, :, None, None]
            v = v * dc[:, :, None, None, None] if dc is not None else v
        v = v.reshape(-1, *v.shape[2:])
    v = v.to(torch.float64)
    if operand_dtype is not None and operand_dtype != torch.float32:
        v = sr.rounded(v, operand_dtype)
    return v


def _conv(case, x, w):
    if case.transposed:
        return F.conv_transpose2d(x, w, stride=case.stride, padding=case.pad, output_padding=case.outpad, groups=case.groups)
    return F.conv2d(x, w, stride=case.stride, padding=case.pad, groups=case.groups)


Ref = collections.namedtuple('Ref', 'y pre scale dx dx_scale dw dw_scale clamp')


def reference(case, d, exact=True, operand_dtype=None, grads=True):
    """fp64 on the CPU, the epilogue in the order of pasta_conv_epilogue (include/pasta_hip.h; csrc/conv_common.h conv_store_subtile): modulated
    weights, output scale, noise times strength, residual, bias, activation, gain, clamp.  -> Ref(y, pre = the value the activation sees,
    scale = conv(|x|, |w|), dx, its scale, dw, its scale, the clamp used).  ``exact``: every step is checked to be exact in fp32 -- the premise
    of the bitwise comparison."""
    x = d['x'] * d['iscale'][:, :, None, None] if 'iscale' in d else d['x']
    w = effective_weights(case, d, operand_dtype)
    v = _conv(case, x, w)
    scale = _conv(case, x.abs(), w.abs())
    if exact:
        # every partial sum, in any order, is a multiple of the product grid's unit below 2^24 units
        unit = grid_unit(x) * grid_unit(w)
        assert float(scale.max()) < 2.0 ** 24 * unit, (case.name, float(scale.max()) / unit)
    steps = [('sum', v)]
    if 'oscale' in d or 'noise' in d:
        nz = 0.0
        if 'noise' in d:
            nz = (d['noise'] * d['strength']).reshape(-1, 1, *v.shape[2:])
            steps.append(('noise * strength', nz))
        v = v * (d['oscale'][:, :, None, None] if 'oscale' in d else 1.0) + nz          # one fused multiply-add
        steps.append(('scale and noise', v))
    if 'res' in d:
        v = v + d['res']
        steps.append(('residual', v))
    clamp = None
    if 'bias' in d:
        v = v + d['bias'].reshape(1, -1, 1, 1)
        steps.append(('bias', v))
    pre = v
    if 'act' in d:
        assert d['act'] == 'lrelu'
        v = torch.where(v > 0, v, v * d['alpha']) * d['gain']
        steps.append(('activation and gain', v))
        clamp = d['clamp']
        if clamp == 'auto':         # a power of two that the outputs of the top two binades exceed
            clamp = 2.0 ** (int(np.floor(np.log2(float(v.abs().max())))) - 1)
        v = v.clamp(-clamp, clamp)
    if exact:
        for what, t in steps:
            _f32_exact(t, f'{case.name}: {what}')
    dx = dxs = dw = dws = None
    if grads and not case.ops:
        # the gradients of the plain convolution: linear in each operand, so autograd of the fp64 operator gives them
        # (the input gradient multiplies the weights as the forward does; the weight gradient never sees them: d/dw of conv(x, w * wgain))
        def grad_pair(x0, w_eff, w0, dy_x, dy_w):
            xg, wg = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
            gx, = torch.autograd.grad(_conv(case, xg, w_eff), xg, dy_x)
            gw, = torch.autograd.grad(_conv(case, x0, wg * case.wgain), wg, dy_w)
            return gx, gw
        dx, dw = grad_pair(d['x'], w, d['w'], d['dy_x'], d['dy_w'])
        dxs, dws = grad_pair(d['x'].abs(), w.abs(), d['w'].abs(), d['dy_x'].abs(), d['dy_w'].abs())
        if exact:
            assert float(dxs.max()) < 2.0 ** 24 * grid_unit(d['dy_x']) * grid_unit(w), case.name
            assert float(dws.max()) < 2.0 ** 24 * grid_unit(d['dy_w']) * grid_unit(d['x']) * case.wgain, case.name
            _f32_exact(dw, f'{case.name}: dw')
    return Ref(v, pre, scale, dx, dxs, dw, dws, clamp)


def grid_unit(t):
    """The largest power of two that divides every element of ``t`` (fp64)."""
    a = t.abs().reshape(-1)
    a = a[a > 0]
    u = 1.0
    for _ in range(64):
        if bool(((a / u) == (a / u).round()).all()):
            return u
        u /= 2
    raise AssertionError('not a dyadic grid')


def needs_rounding(ref, dtype):
    """Share of ``ref`` (fp64 tensor) that is not representable in ``dtype``."""
    r = ref.numpy()
    return float((sr.rne(r, dtype) != r).mean())


@functools.lru_cache(maxsize=None)
def exact_reference(name, dtype):
    """(data, Ref) of the exact leg, computed once per (case, storage type) and shared by the tests (they leave it unchanged)."""
    case = BY_NAME[name]
    d = exact_data(case, dtype)
    return d, reference(case, d, exact=True)


def generic_operand_dtype(case, dtype, fwd_kernel):
    """The type the weights are rounded to on their way to the multiply: the storage type on the matrix-core kernels; the few-channel 1x1 kernels
    (plan kernels 11, 12; csrc/conv_fwd_fewch.h) stream the raw fp32 weights through fp32 FMAs."""
    return torch.float32 if fwd_kernel in (11, 12) else dtype


@functools.lru_cache(maxsize=None)
def generic_reference(name, dtype):
    case = BY_NAME[name]
    d = generic_data(case, dtype)
    kernel = case.expect['fwd'][0]
    return d, reference(case, d, exact=False, operand_dtype=generic_operand_dtype(case, dtype, kernel))
