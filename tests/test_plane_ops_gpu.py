"""The per-plane HBM kernels (csrc/planes.hip, bias_act.hip) against fp64 references in fp32, fp16 and bf16 storage.

Every reference is computed in fp64 from the rounded inputs the kernel reads (tests/storage_ref.py).  Inputs plant large
values in the last element of each plane, so a lost tail, a skipped last chunk or a wrong plane / sample index shows as a
gross error.  Shapes reach every code path the launchers choose: 16-byte packs and the scalar loops (HW % 4 != 0, or a
contiguous view at an element offset), grid-strides past 65535 planes and past 64 workgroups of a plane, multi-chunk planes
with a ragged last chunk, and the register-resident and generic SPADE kernels.

Masks follow the reference's CUDA semantics (torch_utils/ops/bias_act.cu): the backward's slope and clamp mask come from the
STORED forward output, strictly inside +-clamp, so the reference takes them from the kernel's y.  spade_norm_bwd recomputes
its pre-activation in fp32 from x instead; there the upstream gradient is zeroed on the elements whose fp64 pre-activation
lies within a band of 2^-16 (|x_hat| |1 + gamma| + |beta|) -- 256 fp32 ulps -- of the ReLU or clamp edge, where fp32 and fp64
may legitimately take different sides.
"""

import math
import zlib

import numpy as np
import pytest
import torch

import storage_ref as S

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
DT_ID = {torch.float32: 'f32', torch.float16: 'f16', torch.bfloat16: 'bf16'}
PLANT = 24.0


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def host(shape, gen, dtype, plant=PLANT, scale=1.0):
    """fp64 CPU data already rounded to ``dtype``; the last element of every [H, W] plane carries +-plant."""
    t = torch.randn(shape, generator=gen, dtype=torch.float64) * scale
    if plant:
        flat = t.view(-1, shape[-2] * shape[-1])
        sign = torch.where(torch.arange(flat.shape[0]) % 2 == 0, 1.0, -1.0).to(torch.float64)
        flat[:, -1] = plant * sign * (1 + torch.arange(flat.shape[0], dtype=torch.float64) / flat.shape[0])
    return S.rounded(t, dtype)


def dev(t64, dtype, offset=0, grad=False):
    """A contiguous GPU tensor holding ``t64`` (exactly representable in ``dtype``) at element ``offset`` of its storage."""
    buf = torch.empty([t64.numel() + offset], dtype=dtype, device='cuda')
    v = buf[offset:].view(t64.shape).detach()
    v.copy_(t64.to(dtype))
    assert v.is_contiguous() and v.storage_offset() == offset
    return v.requires_grad_(grad)


def c64(t):
    return t.detach().cpu().to(torch.float64)


def f32(v):
    """A scalar parameter as the kernel receives it (a C float)."""
    return None if v is None else float(np.float32(v))


# ----------------------------------------------------------------------------- scale_add: fma.scale_planes, fma.fma, networks.scale_planes

SCALE_CASES = [       # (N, C, H, W, offset): vector path, scalar path (HW % 4), scalar path (offset), > 65535 planes, HW > 65536
    (2, 3, 8, 8, 0), (2, 3, 5, 7, 0), (2, 3, 8, 8, 1), (2, 40000, 2, 2, 0), (1, 2, 320, 512, 0), (2, 2, 320, 512, 3),
]
NOISE = [None, 'hw', '11hw', 'n1hw']


def _noise_shape(kind, n, h, w):
    return {'hw': [h, w], '11hw': [1, 1, h, w], 'n1hw': [n, 1, h, w]}[kind]


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', SCALE_CASES, ids=str)
@pytest.mark.parametrize('noise', NOISE, ids=str)
def test_scale_planes(case, noise, dtype):
    from torch_utils.ops import fma
    n, c, h, w, off = case
    gen = _gen('scale', case, noise, DT_ID[dtype])
    x = host([n, c, h, w], gen, dtype)
    s = S.rounded(torch.randn([n, c], generator=gen, dtype=torch.float64), torch.float32)
    s[-1, -1] = -3.0                                                        # last plane's scale planted
    nz = host(_noise_shape(noise, n, h, w), gen, dtype) if noise else None
    ref = x * s.reshape(n, c, 1, 1)
    scale = ref.abs()
    if nz is not None:
        nb = nz.reshape(-1, 1, h, w)
        ref, scale = ref + nb, scale + nb.abs()
    y = fma.scale_planes(dev(x, dtype, off), dev(s, torch.float32), dev(nz, dtype, off) if nz is not None else None)
    assert y.dtype == dtype and y.shape == x.shape
    S.assert_stored(y, ref, dtype, scale, k=2, what='scale_add y')
    if noise is None:               # the autograd wrapper of the activation-side modulation: same launch
        from training import networks
        y2 = networks.scale_planes(dev(x, dtype, off), dev(s, torch.float32))
        assert torch.equal(y2, y)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('case', [(2, 3, 8, 8, 0), (2, 3, 5, 7, 0), (3, 4, 16, 16, 1), (1, 3, 16, 16, 2)], ids=str)
@pytest.mark.parametrize('noise', ['hw', '11hw', 'n1hw'], ids=str)
@pytest.mark.parametrize('b16', [False, True], ids=['b_f32', 'b_like_a'])
def test_fma_gradients(case, noise, dtype, b16):
    """fma.fma(a, b, c) on the plane pattern: y, and da / db / dc against fp64 autograd.  ``offset`` puts a and dy at an element
    offset (the backward's plane_dot then takes its scalar loop)."""
    from torch_utils.ops import fma
    n, c, h, w, off = case
    gen = _gen('fma', case, noise, DT_ID[dtype], b16)
    bdt = dtype if b16 else torch.float32
    a = host([n, c, h, w], gen, dtype)
    b = S.rounded(torch.randn([n, c, 1, 1], generator=gen, dtype=torch.float64), bdt)
    nz = host(_noise_shape(noise, n, h, w), gen, dtype)
    dy = host([n, c, h, w], gen, dtype)
    ar, br, cr = (t.clone().requires_grad_(True) for t in (a, b, nz))
    yr = ar * br + cr
    dar, dbr, dcr = torch.autograd.grad(yr, [ar, br, cr], dy)
    ag, bg, cg = dev(a, dtype, off, True), dev(b, bdt, 0, True), dev(nz, dtype, 0, True)
    y = fma.fma(ag, bg, cg)
    da, db, dc = torch.autograd.grad(y, [ag, bg, cg], dev(dy, dtype, off))
    S.assert_stored(y, yr, dtype, (a * b).abs() + nz.abs().expand_as(a), k=2, what='y')
    S.assert_stored(da, dar, dtype, (dy * b).abs(), k=2, what='da')
    hw = h * w
    dbs = (dy * a).abs().sum(dim=[2, 3], keepdim=True)
    if bdt == torch.float32:
        S.assert_reduced(db, dbr, dbs, hw, extra=6, what='db')
    else:                           # an fp32 plane sum stored once in the 16-bit type of b
        S.assert_stored(db, dbr, bdt, dbs, k=S.reduction_depth(hw, 256, 6), bitwise=None, what='db')
    dcs, = torch.autograd.grad(ar * br + cr, [cr], dy.abs())             # sum of |dy| over what c was broadcast across
    S.assert_stored(dc, dcr, dtype, dcs, k=n * c + 2, bitwise=None, what='dc')


# ----------------------------------------------------------------------------- plane_dot

DOT_CASES = [(2, 3, 16, 16), (2, 3, 5, 4), (2, 3, 3, 5), (1, 2, 64, 96), (2, 40000, 2, 2)]


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('shape', DOT_CASES, ids=str)
@pytest.mark.parametrize('offsets', [(0, 0), (1, 0), (0, 2), (3, 3)], ids=str)
@pytest.mark.parametrize('with_q', [True, False], ids=['pq', 'p'])
def test_plane_dot(shape, offsets, with_q, dtype):
    from torch_utils.ops import fma
    n, c, h, w = shape
    gen = _gen('dot', shape, offsets, with_q, DT_ID[dtype])
    p = host(shape, gen, dtype)
    q = host(shape, gen, dtype, plant=-PLANT) if with_q else None
    terms = p * q if with_q else p
    out = fma.plane_dot(dev(p, dtype, offsets[0]), dev(q, dtype, offsets[1]) if with_q else None)
    assert out.dtype == torch.float32 and out.shape == (n, c)
    S.assert_reduced(out, terms.sum(dim=[2, 3]), terms.abs().sum(dim=[2, 3]), h * w, extra=6, what='plane_dot')


# ----------------------------------------------------------------------------- mod_bias_act

MBA_SHAPES = [(2, 3, 8, 8), (2, 3, 5, 7), (2, 2, 64, 64), (2, 2, 64, 65), (2, 2, 67, 67), (2, 2, 320, 512)]
MBA_CFGS = [          # (dcoefs, noise, act, clamp)
    (True, 'hw', 'lrelu', 0.75), (True, 'n1hw', 'lrelu', None), (False, None, 'linear', None), (True, None, 'linear', 1.0),
    (False, 'n1hw', 'lrelu', 0.75),
]


def _mba_inputs(shape, dtype, cfg, gen):
    n, c, h, w = shape
    use_d, noise, act, clamp = cfg
    u = host(shape, gen, dtype, plant=6.0, scale=0.5)
    d = S.rounded(0.5 + torch.rand([n, c], generator=gen, dtype=torch.float64), torch.float32) if use_d else None
    nz = host([n, 1, h, w] if noise == 'n1hw' else [h, w], gen, torch.float32, plant=5.0) if noise else None
    if nz is not None and noise == 'n1hw':
        nz[-1] *= 2                                                         # the last sample's noise differs grossly from sample 0's
    st = S.rounded(torch.tensor(0.3 + 0.1 * n, dtype=torch.float64), torch.float32) if noise else None
    b = S.rounded(torch.randn([c], generator=gen, dtype=torch.float64) * 0.2, torch.float32)
    dy = host(shape, gen, dtype, plant=-8.0)
    return u, d, nz, st, b, dy


def _mba_ref(u, d, nz, st, b, act, gain, clamp, y_stored, dy):
    n, c, h, w = u.shape
    alpha = f32(0.2) if act == 'lrelu' else 1.0
    pre = u * (d.reshape(n, c, 1, 1) if d is not None else 1.0) + b.reshape(1, c, 1, 1)
    scale = (u * (d.reshape(n, c, 1, 1) if d is not None else 1.0)).abs() + b.abs().reshape(1, c, 1, 1)
    if nz is not None:
        nb = nz.reshape(-1, 1, h, w) * st
        pre, scale = pre + nb, scale + nb.abs()
    y = torch.where(pre > 0, pre, pre * alpha) * gain
    scale = scale * gain
    if clamp is not None:
        y = y.clamp(-clamp, clamp)
    # backward: slope and mask from the kernel's stored y
    ys = c64(y_stored)
    dz = dy * gain * torch.where(ys > 0, 1.0, alpha)
    if clamp is not None:
        dz = torch.where((ys > -clamp) & (ys < clamp), dz, torch.zeros_like(dz))
    du = dz * (d.reshape(n, c, 1, 1) if d is not None else 1.0)
    sums = dict(dd=((dz * u).sum(dim=[2, 3]), (dz * u).abs().sum(dim=[2, 3])), db=(dz.sum(dim=[0, 2, 3]), dz.abs().sum(dim=[0, 2, 3])))
    if nz is not None:
        t = dz * nz.reshape(-1, 1, h, w)
        sums['dstrength'] = (t.sum(), t.abs().sum())
    return y, scale, du, dz.abs(), sums


def _mba_run(shape, dtype, cfg, gen, offs=(0, 0, 0)):
    """Forward and backward through networks.mod_bias_act; ``offs`` = element offsets of (u, dy, noise)."""
    from training import networks
    use_d, noise, act, clamp = cfg
    u, d, nz, st, b, dy = _mba_inputs(shape, dtype, cfg, gen)
    ug = dev(u, dtype, offs[0], True)
    dg = dev(d, torch.float32, 0, True) if d is not None else None
    ng = dev(nz, torch.float32, offs[2]) if nz is not None else None
    sg = dev(st.reshape([]), torch.float32, 0, True) if st is not None else None
    bg = dev(b, torch.float32, 0, True)
    gain = f32(np.sqrt(2)) if act == 'lrelu' else 1.0
    y = networks.mod_bias_act(ug, dg, ng, sg, bg, act=act, gain=gain, clamp=clamp)
    wrt = [t for t in (ug, dg, sg, bg) if t is not None]
    grads = torch.autograd.grad(y, wrt, dev(dy, dtype, offs[1]))
    g = dict(zip(['du'] + (['dd'] if d is not None else []) + (['dstrength'] if st is not None else []) + ['db'], grads))
    return (u, d, nz, st, b, dy, gain), y, g


def _mba_check(shape, dtype, cfg, inputs, y, g):
    n, c, h, w = shape
    use_d, noise, act, clamp = cfg
    u, d, nz, st, b, dy, gain = inputs
    yr, ys, dur, dus, sums = _mba_ref(u, d, nz, st, b, act, gain, clamp, y, dy)
    S.assert_stored(y, yr, dtype, ys, k=5, what='y')
    S.assert_stored(g['du'], dur, dtype, dus * (d.reshape(n, c, 1, 1) if d is not None else 1.0), k=3, what='du')
    chunks = math.ceil(h * w / 4096)
    extra = chunks + n * c + 8          # four-term packs, the workgroup's four wave partials, the host's chunk and plane sums, dz
    for name, (ref, scale) in sums.items():
        if name in g:
            S.assert_reduced(g[name], ref, scale, min(h * w, 4096), extra=extra, what=name)
    assert set(g) - {'du'} == set(k for k in sums if k in g)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('shape', MBA_SHAPES, ids=str)
def test_mod_bias_act(shape, dtype):
    for cfg in MBA_CFGS:
        inputs, y, g = _mba_run(shape, dtype, cfg, _gen('mba', shape, cfg, DT_ID[dtype]))
        _mba_check(shape, dtype, cfg, inputs, y, g)


def test_mod_bias_act_side_operands_are_read_as_fp32():
    """dcoefs, noise, strength and bias of another type or device are converted (with their gradients), not read as fp32 bits;
    wrong sizes are refused."""
    from training import networks
    shape, cfg = (2, 3, 16, 20), (True, 'n1hw', 'lrelu', 0.75)
    inputs, y, g = _mba_run(shape, torch.bfloat16, cfg, _gen('mba16'))
    u, d, nz, st, b, dy, gain = inputs
    ug = dev(u, torch.bfloat16, 0, True)
    side = [dev(d, torch.bfloat16, 0, True), dev(nz, torch.bfloat16), st.reshape(1).to(torch.bfloat16).requires_grad_(True),   # strength on the CPU
            dev(b, torch.float16, 0, True)]
    y2 = networks.mod_bias_act(ug, side[0], side[1], side[2], side[3], act='lrelu', gain=gain, clamp=0.75)
    # the side operands above are the fp32 values rounded to 16 bits: reference from those
    d16, nz16, st16, b16 = (c64(t) for t in side)
    yr, ys, dur, dus, sums = _mba_ref(u, d16, nz16, st16.reshape([]), b16, 'lrelu', gain, 0.75, y2, dy)
    S.assert_stored(y2, yr, torch.bfloat16, ys, k=5, what='y')
    grads = torch.autograd.grad(y2, [ug, side[0], side[2], side[3]], dev(dy, torch.bfloat16))
    for t, gr in zip([ug, side[0], side[2], side[3]], grads):
        assert gr.dtype == t.dtype and gr.shape == t.shape and gr.device == t.device
    assert torch.isfinite(grads[1]).all() and torch.isfinite(grads[3]).all()
    with pytest.raises(RuntimeError, match='bias'):
        networks.mod_bias_act(ug, None, None, None, dev(torch.zeros(4), torch.float32))
    with pytest.raises(RuntimeError, match='noise'):
        networks.mod_bias_act(ug, None, dev(torch.zeros(7), torch.float32), side[2], None)
    with pytest.raises(RuntimeError, match='dcoefs'):
        networks.mod_bias_act(ug, torch.ones([2, 3], dtype=torch.int32, device='cuda'), None, None, None)


# ----------------------------------------------------------------------------- spade_modulate

SPADE_HW = [(128, 128, 0), (64, 64, 0), (17, 13, 0), (128, 128, 1)]       # EPT 16, EPT 4, generic, generic by misalignment
SPADE_GRADS = [('x',), ('g',), ('b',), ('x', 'g', 'b')]


def _spade_ref(x, g, b, eps, relu_gain, clamp):
    n, c, h, w = x.shape
    mean = x.mean(dim=[2, 3], keepdim=True)
    var = ((x - mean) ** 2).mean(dim=[2, 3], keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    xh = (x - mean) * rstd
    v = xh * (1 + g) + b
    vscale = (xh.abs() + (mean.abs() + x.abs()) * rstd) * (1 + g).abs() + b.abs()
    if relu_gain is None:
        return xh, rstd, v, v, vscale, None
    out = torch.clamp(torch.relu(v) * relu_gain, max=clamp) if clamp is not None else torch.relu(v) * relu_gain
    band = 2.0 ** -16 * (xh.abs() * (1 + g).abs() + b.abs())
    near = v.abs() <= band
    if clamp is not None:
        near |= (v * relu_gain - clamp).abs() <= band * relu_gain
    return xh, rstd, v, out, vscale * relu_gain, near


def _spade_case(hw, dtype, mode, post, wanted, passthrough, gen):
    """Runs networks.spade_modulate on planted data and checks out and the requested gradients against fp64.  The ReLU gain is
    the model's sqrt(2): a gain like 1.3 (fp32 0x3fa66666) puts dout * gain exactly on a 16-bit tie after its fp32 rounding for
    ~2.6 % of 16-bit dout, and the bitwise check would measure that double rounding instead of the store."""
    from training import networks
    h, w, off = hw
    n, c = 2, 3
    relu_gain, clamp = f32(post[0]), f32(post[1])
    x = host([n, c, h, w], gen, dtype, plant=6.0, scale=0.7)
    x = x + S.rounded(torch.randn([n, c, 1, 1], generator=gen, dtype=torch.float64), torch.float64)     # per-plane means
    x = S.rounded(x, dtype)
    g = host([n, c, h, w], gen, dtype, plant=2.0, scale=0.3)
    b = host([n, c, h, w], gen, dtype, plant=-3.0, scale=0.3)
    dout = host([n, c, h, w], gen, dtype, plant=5.0)
    dxp = host([n, c, h, w], gen, dtype) if passthrough else None
    eps = f32(1e-5)
    xh, rstd, v, outr, oscale, near = _spade_ref(x, g, b, eps, relu_gain, clamp)
    if near is not None:
        dout = torch.where(near, torch.zeros_like(dout), dout)             # no gradient where fp32 may take the other side of an edge
    need = dict(x='x' in wanted, g='g' in wanted, b='b' in wanted)
    xg = dev(x, dtype, off, need['x'])
    if mode == 'separate':
        gg, bg = dev(g, dtype, 0, need['g']), dev(b, dtype, 0, need['b'])
        args, wrt = (xg, gg, bg), [t for t, k in ((xg, 'x'), (gg, 'g'), (bg, 'b')) if need[k]]
    else:
        gb = torch.cat([g, b], dim=1)
        if mode == 'slice':             # gamma | beta as channels [2, 2 + 2C) of a wider tensor: read at its sample stride
            wide = torch.cat([host([n, 2, h, w], gen, dtype), gb, host([n, 1, h, w], gen, dtype)], dim=1)
            gbg = dev(wide, dtype, 0, need['g'] or need['b'])
            gbv = gbg.narrow(1, 2, 2 * c)
            assert gbv.stride(0) > 2 * c * h * w
        else:
            gbg = gbv = dev(gb, dtype, 0, need['g'] or need['b'])
        args, wrt = (xg, gbv, None), [t for t, k in ((xg, 'x'), (gbg, 'g')) if need[k] or (k == 'g' and need['b'])]
    kw = dict(relu_gain=relu_gain, clamp=clamp)
    if passthrough:
        out, xp = networks.spade_modulate(*args, passthrough=True, **kw)
        assert torch.equal(xp, xg) and xp.requires_grad
        grads = torch.autograd.grad([out, xp], wrt, [dev(dout, dtype, off), dev(dxp, dtype)])
    else:
        out = networks.spade_modulate(*args, **kw)
        grads = torch.autograd.grad(out, wrt, dev(dout, dtype, off))
    HW = h * w
    kst = S.reduction_depth(HW, 1024, 8)          # statistics: 1024-lane sums of x and (x - mean)^2, rsqrt, the normalisation
    S.assert_stored(out, outr, dtype, oscale, k=kst, what='out')
    gain = relu_gain if relu_gain is not None else 1.0
    d = dout * gain
    if relu_gain is not None:
        d = torch.where(v > 0, d, torch.zeros_like(d))
        if clamp is not None:
            d = torch.where(v * relu_gain < clamp, d, torch.zeros_like(d))
    t = d * (1 + g)
    m1, m2 = t.mean(dim=[2, 3], keepdim=True), (t * xh).mean(dim=[2, 3], keepdim=True)
    dxr = rstd * (t - m1 - xh * m2)
    dxs = rstd * (t.abs() + t.abs().mean(dim=[2, 3], keepdim=True) +
                  (xh.abs() + 1) * (t * xh).abs().mean(dim=[2, 3], keepdim=True)) * (1 + (xh.abs() + 1))
    if passthrough:
        dxr, dxs = dxr + dxp, dxs + dxp.abs()
    hs = (xh.abs() + (x.abs() + x.mean(dim=[2, 3], keepdim=True).abs()) * rstd)         # |x_hat| and its statistics' error
    gi = iter(grads)
    if need['x']:
        S.assert_stored(next(gi), dxr, dtype, dxs, k=kst, bitwise=None, what='dx')
    if mode == 'separate':
        if need['g']:
            S.assert_stored(next(gi), d * xh, dtype, d.abs() * hs, k=kst, what='dgamma')
        if need['b']:
            S.assert_stored(next(gi), d, dtype, d.abs(), k=2, what='dbeta')
    elif need['g'] or need['b']:
        dgb = next(gi)
        full = dgb if mode == 'halves' else dgb[:, 2:2 + 2 * c]
        if mode == 'slice':
            assert not bool(dgb[:, :2].any()) and not bool(dgb[:, 2 + 2 * c:].any())
        S.assert_stored(full[:, :c], d * xh, dtype, d.abs() * hs, k=kst, what='dgamma half')
        S.assert_stored(full[:, c:], d, dtype, d.abs(), k=2, what='dbeta half')


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('hw', SPADE_HW, ids=str)
@pytest.mark.parametrize('mode', ['separate', 'halves', 'slice'])
@pytest.mark.parametrize('post', [(None, None), (2 ** 0.5, None), (2 ** 0.5, 1.2)], ids=['none', 'relu', 'relu_clamp'])
def test_spade_modulate(hw, mode, post, dtype):
    for wanted in SPADE_GRADS:
        if mode != 'separate' and wanted == ('b',):
            continue                    # gamma | beta is one tensor: ('g',) already asks for its gradient
        _spade_case(hw, dtype, mode, post, wanted, False, _gen('spade', hw, mode, post, wanted, DT_ID[dtype]))


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('hw', SPADE_HW, ids=str)
@pytest.mark.parametrize('mode', ['separate', 'halves'])
def test_spade_modulate_passthrough_joins_both_gradients(hw, mode, dtype):
    """passthrough=True: the gradient of the pass-through output is added to dx by the backward kernel (dx_add)."""
    for wanted in [('x',), ('x', 'g', 'b')]:
        _spade_case(hw, dtype, mode, (2 ** 0.5, 1.2), wanted, True, _gen('spade_pt', hw, mode, wanted, DT_ID[dtype]))


# ----------------------------------------------------------------------------- element offsets: same values as the aligned call

def _same_per_element(got, want, dtype, what):
    """Bitwise equal, except for fp16: there the compiler contracts the scalar loops' fp32 multiply-add and fp16 store into ONE
    v_fma_mixlo_f16 (a single rounding of the exact value), while the packed path rounds to fp32 first and then converts with
    v_cvt_pk_f16_f32.  The two differ by one fp16 ulp where the fp32 result lands exactly on an fp16 tie; both are within the
    storage bound, checked against fp64 elsewhere in this file."""
    if dtype != torch.float16:
        assert torch.equal(got, want), what
        return
    diff = got != want
    assert float(diff.float().mean()) < 0.01, what
    g, w = c64(got)[c64(diff).bool()], c64(want)[c64(diff).bool()]
    assert bool(((g - w).abs() <= torch.from_numpy(S.ulp(w, torch.float16))).all()), what

@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('offset', [1, 2, 3])
def test_element_offsets_scale_planes_and_fma(offset, dtype):
    """scale_add does the same fp32 arithmetic per element on both paths: equal (see _same_per_element for fp16).  plane_dot
    sums in another order."""
    from torch_utils.ops import fma
    n, c, h, w = 2, 3, 16, 16
    gen = _gen('off_fma', offset, DT_ID[dtype])
    a, dy = host([n, c, h, w], gen, dtype), host([n, c, h, w], gen, dtype)
    b = S.rounded(torch.randn([n, c, 1, 1], generator=gen, dtype=torch.float64), torch.float32)
    nz = host([n, 1, h, w], gen, dtype)
    outs = []
    for oa, od, on in [(0, 0, 0), (offset, 0, 0), (0, offset, 0), (0, 0, offset)]:
        ag, bg = dev(a, dtype, oa, True), dev(b, torch.float32, 0, True)
        y = fma.fma(ag, bg, dev(nz, dtype, on))
        da, db = torch.autograd.grad(y, [ag, bg], dev(dy, dtype, od))
        outs.append((y, da, db))
    for y, da, db in outs[1:]:
        _same_per_element(y, outs[0][0], dtype, 'y')
        _same_per_element(da, outs[0][1], dtype, 'da')
        S.assert_reduced(db, c64(outs[0][2]), (dy * a).abs().sum(dim=[2, 3], keepdim=True) * 2, h * w, extra=6, what='db')


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('act,clamp', [('lrelu', 1.5), ('linear', 1.0)])
def test_element_offsets_bias_act(offset, act, clamp, dtype):
    """bias_act with x or grad_output at an element offset: the fused (dx, db) kernel moves 16-byte packs, so the backward
    takes the two-launch path; y and dx are the same fp32 arithmetic per element (bitwise equal), db sums in another order."""
    from torch_utils.ops import bias_act
    shape = [2, 3, 64, 64]
    gen = _gen('off_ba', offset, act, DT_ID[dtype])
    x, dy = host(shape, gen, dtype), host(shape, gen, dtype)
    b = S.rounded(torch.randn([3], generator=gen, dtype=torch.float64), dtype)
    outs = []
    for ox, od in [(0, 0), (offset, 0), (0, offset)]:
        xg, bg = dev(x, dtype, ox, True), dev(b, dtype, 0, True)
        y = bias_act.bias_act(xg, bg, act=act, clamp=clamp)
        dx, db = torch.autograd.grad(y, [xg, bg], dev(dy, dtype, od))
        outs.append((y, dx, db))
    for y, dx, db in outs[1:]:
        assert torch.equal(y, outs[0][0]) and torch.equal(dx, outs[0][1])
        scale = c64(outs[0][1]).abs().sum(dim=[0, 2, 3]) * 2
        if dtype == torch.float32:
            S.assert_reduced(db, c64(outs[0][2]), scale, 2 * 64 * 64, extra=8, what='db')
        else:
            S.assert_stored(db, c64(outs[0][2]), dtype, scale, k=S.reduction_depth(2 * 64 * 64, 256, 8), bitwise=None, what='db')


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('offset', [1, 2, 3])
@pytest.mark.parametrize('shape', [(2, 3, 16, 16), (2, 2, 64, 65)], ids=str)
def test_element_offsets_mod_bias_act(shape, offset, dtype):
    """u, dy and noise in turn at an element offset: y and du equal to the aligned call (same fp32 arithmetic per element on
    the scalar path; see _same_per_element for fp16); dd, dstrength and db within the reduction bound against fp64."""
    cfg = (True, 'n1hw', 'lrelu', 0.75)
    base = _mba_run(shape, dtype, cfg, _gen('off_mba', shape, DT_ID[dtype]))
    for offs in [(offset, 0, 0), (0, offset, 0), (0, 0, offset)]:
        inputs, y, g = _mba_run(shape, dtype, cfg, _gen('off_mba', shape, DT_ID[dtype]), offs)
        _same_per_element(y, base[1], dtype, f'y {offs}')
        _same_per_element(g['du'], base[2]['du'], dtype, f'du {offs}')
        _mba_check(shape, dtype, cfg, inputs, y, g)


@pytest.mark.parametrize('dtype', DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize('offset', [1, 2, 3])
def test_element_offsets_spade(offset, dtype):
    """x / dout at an element offset (the 128x128 plane then runs on the generic kernel): checked against fp64 like the aligned
    call, whose statistics are summed in another order."""
    _spade_case((128, 128, offset), dtype, 'halves', (2 ** 0.5, 1.2), ('x', 'g'), True, _gen('off_spade', offset, DT_ID[dtype]))
    _spade_case((64, 64, offset), dtype, 'separate', (None, None), ('x', 'g', 'b'), False, _gen('off_spade4', offset, DT_ID[dtype]))
