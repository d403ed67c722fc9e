"""grid_sample_gradfix on the HIP kernels (csrc/grid_sample.hip) under general sampling grids: forward, image gradient,
grid gradient (alone and fused with the image gradient), second derivative in the image, 16-bit storage, a model-level
R1 case, the absence of ATen's sampler, and a > 2^31-element image.  References: F.grid_sample in fp64 on the CPU."""

import math

import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _ref_sample(x, grid):
    return F.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False)


def _off_kinks(grid, ih, iw):
    """Move fp32 grid points off the pixel lattice.  grad_grid jumps where a source coordinate crosses an integer (the sampler's
    kinks); there one ulp of the fp32 coordinate arithmetic picks a side the fp64 reference may not pick."""
    g = grid.double()
    for k, size in ((0, iw), (1, ih)):
        pix = ((g[..., k] + 1) * size - 1) / 2
        near = (pix - pix.round()).abs() < 1e-3
        g[..., k] = torch.where(near, g[..., k] + 4e-3 / size, g[..., k])
    return g.float()


def _grid(kind, n, oh, ow, ih, iw, gen):
    """Grids of several kinds, fp32 on the CPU."""
    if kind == 'random':        # includes points outside [-1, 1]
        return torch.rand([n, oh, ow, 2], generator=gen) * 2.8 - 1.4
    if kind == 'lattice':       # pixel centres, image borders (+-1) and the centres of the pixels just outside
        xs = torch.tensor([(2 * j + 1) / iw - 1 for j in range(-1, iw + 1)] + [-1.0, 1.0])
        ys = torch.tensor([(2 * i + 1) / ih - 1 for i in range(-1, ih + 1)] + [-1.0, 1.0])
        gx = xs[torch.randint(len(xs), [n, oh, ow], generator=gen)]
        gy = ys[torch.randint(len(ys), [n, oh, ow], generator=gen)]
        return torch.stack([gx, gy], dim=-1)
    theta = torch.tensor([[0.08, 0.01, 0.05], [-0.01, 0.07, -0.1]]) if kind == 'zoom_out' else torch.tensor([[2.7, 0.3, 0.2], [-0.2, 2.4, 0.1]])
    base = F.affine_grid(theta.expand(n, 2, 3), [n, 1, oh, ow], align_corners=False)
    return base + 0.002 * torch.randn(base.shape, generator=gen)


CASES = [
    # zoom_out: the whole output grid falls on a few input pixels -- every dx element takes hundreds of atomic adds
    dict(kind='random', n=2, c=3, ih=17, iw=9, oh=23, ow=31),
    dict(kind='lattice', n=3, c=1, ih=17, iw=9, oh=23, ow=31),
    dict(kind='zoom_out', n=16, c=3, ih=17, iw=9, oh=23, ow=31),
    dict(kind='zoom_in', n=4, c=64, ih=17, iw=9, oh=23, ow=31),
    dict(kind='random', n=16, c=64, ih=33, iw=40, oh=19, ow=70),
]


def _setup(case, seed=0):
    gen = torch.Generator().manual_seed(seed)
    n, c, ih, iw, oh, ow = (case[k] for k in ('n', 'c', 'ih', 'iw', 'oh', 'ow'))
    x = torch.randn([n, c, ih, iw], generator=gen)
    grid = _grid(case['kind'], n, oh, ow, ih, iw, gen)
    if case['kind'] != 'lattice':
        grid = _off_kinks(grid, ih, iw)
    dy = torch.randn([n, c, oh, ow], generator=gen)
    return x, grid, dy


@pytest.mark.parametrize('case', CASES, ids=lambda c: '{kind}-{n}x{c}x{ih}x{iw}-{oh}x{ow}'.format(**c))
def test_forward(case):
    from torch_utils.ops import grid_sample_gradfix as gs
    x, grid, _ = _setup(case)
    y = gs.grid_sample(x.cuda(), grid.cuda())
    assert y.dtype == torch.float32 and y.shape == (case['n'], case['c'], case['oh'], case['ow'])
    assert rel_err(y, _ref_sample(x.double(), grid.double())) <= TOL
    # within a few ulp of ATen's own GPU sampler (same coordinate arithmetic, up to fused multiply-adds)
    assert rel_err(y, _ref_sample(x.cuda(), grid.cuda())) <= 8 * torch.finfo(torch.float32).eps


# grad_grid jumps on the pixel lattice, so the lattice grid checks the image gradient only
GRAD_CASES = [(c, w) for c in CASES for w in ('dx', 'grid', 'both') if c['kind'] != 'lattice' or w == 'dx']


@pytest.mark.parametrize('case,wanted', GRAD_CASES, ids=['{kind}-{n}x{c}x{ih}x{iw}-{oh}x{ow}-'.format(**c) + w for c, w in GRAD_CASES])
def test_gradients(case, wanted):
    """dx alone (the atomic scatter), grad_grid alone, and both from one pass, against fp64 autograd of F.grid_sample."""
    from torch_utils.ops import grid_sample_gradfix as gs
    x, grid, dy = _setup(case, seed=1)
    x64, g64 = x.double().requires_grad_(wanted != 'grid'), grid.double().requires_grad_(wanted != 'dx')
    inputs = [t for t in (x64, g64) if t.requires_grad]
    ref = torch.autograd.grad(_ref_sample(x64, g64), inputs, dy.double())
    xg, gg = x.cuda().requires_grad_(wanted != 'grid'), grid.cuda().requires_grad_(wanted != 'dx')
    got = torch.autograd.grad(gs.grid_sample(xg, gg), [t for t in (xg, gg) if t.requires_grad], dy.cuda())
    for a, b in zip(got, ref):
        assert a.dtype == torch.float32 and a.device.type == 'cuda'
        assert rel_err(a, b) <= TOL


@pytest.mark.parametrize('case', CASES[:4], ids=lambda c: c['kind'])
def test_second_derivative_and_adjoint_identity(case):
    """d/d(dy) of S^T dy contracted with e is S e; and <S x, dy> = <x, S^T dy> in the kernels' own arithmetic."""
    from torch_utils.ops import grid_sample_gradfix as gs
    x, grid, dy = _setup(case, seed=2)
    xg, gc = x.cuda().requires_grad_(True), grid.cuda()
    y = gs.grid_sample(xg, gc)
    dyg = dy.cuda().requires_grad_(True)
    g, = torch.autograd.grad(y, xg, dyg, create_graph=True)
    e = torch.randn(x.shape, generator=torch.Generator().manual_seed(3))
    dd, = torch.autograd.grad(g, dyg, e.cuda())
    assert rel_err(dd, _ref_sample(e.double(), grid.double())) <= TOL
    lhs, rhs = float((y.detach().double() * dyg.detach().double()).sum()), float((xg.detach().double() * g.detach().double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.0)


# 16-bit storage: the kernels read the stored values exactly, compute in fp32 and round each result once, so against an fp64 reference
# built from the SAME stored inputs the error is half an ulp of the storage type at the result's magnitude plus fp32 noise.  Bounds are
# relative to the largest reference value: 2^-10 for fp16 (one ulp at the top of the range, twice the rounding) and 2^-7 for bf16.
TOL16 = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7}


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
@pytest.mark.parametrize('grid_in_dtype', [False, True], ids=['grid_fp32', 'grid_16bit'])
@pytest.mark.parametrize('case', [CASES[0], CASES[2], CASES[4]], ids=lambda c: c['kind'] + str(c['c']))
def test_16bit_storage(case, dtype, grid_in_dtype):
    from torch_utils.ops import grid_sample_gradfix as gs
    x, grid, dy = _setup(case, seed=4)
    x, dy = x.to(dtype), dy.to(dtype)
    if grid_in_dtype:
        grid = grid.to(dtype)       # the coordinates of a 16-bit grid are exact in both fp32 and fp64: no kink ambiguity
    xg, gg = x.cuda().requires_grad_(True), grid.cuda().requires_grad_(True)
    y = gs.grid_sample(xg, gg)
    dx, dgrid = torch.autograd.grad(y, [xg, gg], dy.cuda())
    assert y.dtype == dtype and dx.dtype == dtype and dgrid.dtype == grid.dtype
    x64, g64 = x.double().requires_grad_(True), grid.double().requires_grad_(True)
    y64 = _ref_sample(x64, g64)
    dx64, dg64 = torch.autograd.grad(y64, [x64, g64], dy.double())
    tol = TOL16[dtype]
    assert rel_err(y, y64) <= tol
    assert rel_err(dx, dx64) <= tol
    assert rel_err(dgrid, dg64) <= tol


def test_float64_tensors():
    """fp64 GPU tensors stay on the HIP path (fp64 arithmetic, global_atomic_add_f64 for dx), differentiable as before."""
    from torch_utils.ops import grid_sample_gradfix as gs
    x, grid, dy = (t.double() for t in _setup(CASES[4], seed=9))
    xg, gg = x.cuda().requires_grad_(True), grid.cuda().requires_grad_(True)
    y = gs.grid_sample(xg, gg)
    dx, dgrid = torch.autograd.grad(y, [xg, gg], dy.cuda())
    x64, g64 = x.clone().requires_grad_(True), grid.clone().requires_grad_(True)
    y64 = _ref_sample(x64, g64)
    dx64, dg64 = torch.autograd.grad(y64, [x64, g64], dy)
    for a, b in ((y, y64), (dx, dx64), (dgrid, dg64)):
        assert a.dtype == torch.float64 and rel_err(a, b) <= 1e-12


def test_model_level_r1_and_grid_gradient():
    """conv2d_gradfix.conv2d + bias_act(lrelu) on grid_sample(img, learned_grid): an R1-style double backward in the image and a
    first-order gradient to the grid, against the same graph in fp64 on the CPU.  ATen's grid sampler has no second derivative, so
    the CPU image path writes S as the dense matrix F.grid_sample makes of the unit images (linear in the image to any order); the
    grid gradient uses F.grid_sample itself."""
    from torch_utils.ops import bias_act, conv2d_gradfix
    from torch_utils.ops import grid_sample_gradfix as gs
    gen = torch.Generator().manual_seed(5)
    n, c, ih, iw, oh, ow, co = 2, 4, 12, 10, 14, 11, 8
    img = torch.randn([n, c, ih, iw], generator=gen)
    theta = torch.tensor([[[0.9, 0.25, 0.05], [-0.2, 1.1, -0.1]], [[1.2, -0.1, 0.1], [0.15, 0.8, 0.05]]])
    grid = _off_kinks(F.affine_grid(theta, [n, c, oh, ow], align_corners=False) + 0.05 * torch.randn([n, oh, ow, 2], generator=gen), ih, iw)
    w = torch.randn([co, c, 3, 3], generator=gen) / 6
    b = torch.randn([co], generator=gen) * 0.1
    r = torch.randn([n, co, oh, ow], generator=gen)

    def head(s, conv, act):
        return (act(conv(s, w_), b_) * r_).sum()

    # GPU: the product's ops
    w_, b_, r_ = w.cuda(), b.cuda(), r.cuda()
    xg, gg = img.cuda().requires_grad_(True), grid.cuda().requires_grad_(True)
    score = head(gs.grid_sample(xg, gg), lambda s, w: conv2d_gradfix.conv2d(s, w, padding=1),
                 lambda t, bb: bias_act.bias_act(t, bb, act='lrelu', gain=math.sqrt(2)))
    g_img, g_grid = torch.autograd.grad(score, [xg, gg], create_graph=True)
    r1, = torch.autograd.grad(g_img.square().sum(), [xg])

    # CPU fp64: plain torch
    w_, b_, r_ = w.double(), b.double(), r.double()
    conv = lambda s, w: F.conv2d(s, w, padding=1)
    act = lambda t, bb: F.leaky_relu(t + bb.reshape(1, -1, 1, 1), 0.2) * math.sqrt(2)
    x64, g64 = img.double().requires_grad_(True), grid.double().requires_grad_(True)
    eye = torch.eye(ih * iw, dtype=torch.float64).reshape(ih * iw, 1, ih, iw)
    smat = torch.stack([_ref_sample(eye, g64.detach()[k:k + 1].expand(ih * iw, oh, ow, 2)).reshape(ih * iw, oh * ow).t() for k in range(n)])
    s_dense = torch.einsum('npq,ncq->ncp', smat, x64.reshape(n, c, ih * iw)).reshape(n, c, oh, ow)
    g_img64, = torch.autograd.grad(head(s_dense, conv, act), [x64], create_graph=True)
    r1_64, = torch.autograd.grad(g_img64.square().sum(), [x64])
    g_grid64, = torch.autograd.grad(head(_ref_sample(x64.detach(), g64), conv, act), [g64])
    assert rel_err(g_img, g_img64) <= 1e-4
    assert rel_err(r1, r1_64) <= 1e-4
    assert rel_err(g_grid, g_grid64) <= 1e-4


def test_no_aten_sampler_on_gpu_tensors(monkeypatch):
    from torch_utils.ops import grid_sample_gradfix as gs

    def refuse(name, real):
        def f(*args, **kwargs):
            if any(isinstance(a, torch.Tensor) and a.is_cuda for a in list(args) + list(kwargs.values())):
                raise AssertionError(f'{name} ran on a GPU tensor')
            return real(*args, **kwargs)
        return f
    monkeypatch.setattr(torch.nn.functional, 'grid_sample', refuse('F.grid_sample', torch.nn.functional.grid_sample))
    monkeypatch.setattr(torch, 'grid_sampler', refuse('torch.grid_sampler', torch.grid_sampler))
    monkeypatch.setattr(torch, 'grid_sampler_2d', refuse('torch.grid_sampler_2d', torch.grid_sampler_2d))
    monkeypatch.setattr(torch.ops.aten, 'grid_sampler_2d_backward',
                        refuse('aten::grid_sampler_2d_backward', torch.ops.aten.grid_sampler_2d_backward))
    x, grid, dy = _setup(CASES[0], seed=6)
    xg, gg, dyg = x.cuda().requires_grad_(True), grid.cuda().requires_grad_(True), dy.cuda().requires_grad_(True)
    y = gs.grid_sample(xg, gg)
    dx, dgrid = torch.autograd.grad(y, [xg, gg], dyg, create_graph=True)
    dd, = torch.autograd.grad(dx, dyg, torch.ones_like(dx))
    assert torch.isfinite(dd).all() and torch.isfinite(dgrid).all()
    # and the same patches do catch a GPU call
    with pytest.raises(AssertionError, match='ran on a GPU tensor'):
        torch.nn.functional.grid_sample(xg, gg, align_corners=False)


def test_image_past_two_gig_elements():
    """An fp16 image of more than 2^31 elements (about 4.4 GB): forward, image and grid gradient read and write with 64-bit offsets.
    Checked on a few channels of every sample; dy is zero outside them, so the grid gradient's channel sum is checkable too."""
    from torch_utils.ops import grid_sample_gradfix as gs
    n, c, ih, iw, oh, ow = 2, 260, 2048, 2048, 40, 56
    assert n * c * ih * iw > 2 ** 31
    gen = torch.Generator(device='cuda').manual_seed(7)
    x = torch.randn([n, c, ih, iw], device='cuda', dtype=torch.float16, generator=gen)
    grid = _off_kinks(torch.rand([n, oh, ow, 2], generator=torch.Generator().manual_seed(8)) * 2.2 - 1.1, ih, iw).cuda()
    chans = [0, 1, 129, 258, 259]
    dy = torch.zeros([n, c, oh, ow], device='cuda', dtype=torch.float16)
    dy[:, chans] = torch.randn([n, len(chans), oh, ow], device='cuda', generator=gen).half()
    xg, gg = x.requires_grad_(True), grid.requires_grad_(True)
    y = gs.grid_sample(xg, gg)
    dx, dgrid = torch.autograd.grad(y, [xg, gg], dy)
    xs = x.detach()[:, chans].double().cpu().requires_grad_(True)
    g64 = grid.detach().double().cpu().requires_grad_(True)
    y64 = _ref_sample(xs, g64)
    dx64, dg64 = torch.autograd.grad(y64, [xs, g64], dy[:, chans].double().cpu())
    # at 2048 pixels an fp32 source coordinate resolves 2.4e-4 of a pixel (ATen's arithmetic, ((g + 1) * W - 1) / 2, has the same
    # limit): that much weight error comes on top of the fp16 rounding
    assert rel_err(y[:, chans], y64) <= 2e-3
    assert rel_err(dx[:, chans], dx64) <= 2e-3
    assert rel_err(dgrid, dg64) <= 2e-3
    assert float(dx[:, 2:129].abs().max()) == 0.0
