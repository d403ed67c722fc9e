"""``grid_sample`` with a second derivative (reference: torch_utils/ops/grid_sample_gradfix.py:22-83).

Bilinear sampling, zero padding, ``align_corners=False``: for a fixed grid a linear map of the image, ``y = S(grid) x``.
ADA's geometric step resamples the discriminator's input, and R1 differentiates ``D(augment(real))`` twice with respect
to the image, so the image gradient ``S^T dy`` must itself be differentiable; the gradient of THAT with respect to ``dy``
is ``S`` again, i.e. the forward sampler -- two Functions that call each other, to any order.

The gradient with respect to the grid is the reference's ``grad_grid`` (:61-67; ``aten::grid_sampler_2d_backward``):
first order only.  The reference drops ``grad2_grad_grid`` and asserts on the term through the grid (:70-81); here a
second-order request that would need either raises ``NotImplementedError`` instead of returning a zero.

GPU tensors run on this package's kernels (``csrc/grid_sample.hip``: forward; image and grid gradients in one pass over
``dy``); the image may be float32, float16, bfloat16 or float64 and the grid has its dtype (or float32 for a 16-bit image).  ``dx`` is accumulated with
float atomics and is not bitwise reproducible from run to run (ATen's is not either); ``grad_grid`` is.  CPU tensors use
ATen's sampler.
"""

import torch

enabled = False  # kept for API compatibility: the differentiable path is always on

def grid_sample(input, grid):
    return _Sample.apply(input, grid)

#----------------------------------------------------------------------------
# The launches: HIP for GPU tensors, ATen for CPU tensors.

_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64)

def _check_args(x_shape, x_dtype, x_device, grid, what):
    from . import _native
    if len(x_shape) != 4 or grid.ndim != 4 or grid.shape[0] != x_shape[0] or grid.shape[3] != 2:
        raise RuntimeError(f'{what}: expected input [N, C, H, W] and grid [N, H_out, W_out, 2], got {tuple(x_shape)} and {tuple(grid.shape)}')
    if x_dtype not in _DTYPES or not (grid.dtype == x_dtype or (grid.dtype == torch.float32 and x_dtype in (torch.float16, torch.bfloat16))):
        raise RuntimeError(f'{what}: input must be float32, float16, bfloat16 or float64 and the grid of its dtype (or float32 for a 16-bit '
                           f'input), got {x_dtype}, {grid.dtype}')
    if grid.device != x_device:
        raise RuntimeError(f'{what}: input on {x_device}, grid on {grid.device}')
    return _native.DTYPE_CODE[x_dtype], _native.DTYPE_CODE[grid.dtype]

def _forward(x, grid):
    if x.device.type != 'cuda':
        return torch.nn.functional.grid_sample(input=x, grid=grid, mode='bilinear', padding_mode='zeros', align_corners=False)
    from . import _native
    dt, gdt = _check_args(x.shape, x.dtype, x.device, grid, 'grid_sample')
    x, grid = x.contiguous(), grid.contiguous()
    n, c, ih, iw = x.shape
    oh, ow = grid.shape[1], grid.shape[2]
    y = torch.empty([n, c, oh, ow], dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device):
        st = _native.lib().pasta_grid_sample(_native.ptr(x), _native.ptr(grid), _native.ptr(y), n, c, ih, iw, oh, ow, dt, gdt, _native.stream())
    _native.check(st)
    return y

def _backward(dy, x, grid, x_shape, want_dx, want_dgrid):
    """(dx or None, dgrid or None) in one pass over dy; x is read only for the grid gradient."""
    if dy.device.type != 'cuda':
        image = x if want_dgrid else dy.new_empty(x_shape)      # without the grid gradient only the image's shape / dtype / device is read
        dx, dgrid = torch.ops.aten.grid_sampler_2d_backward(dy.contiguous(), image, grid, 0, 0, False, [want_dx, want_dgrid])
        return (dx if want_dx else None), (dgrid if want_dgrid else None)
    from . import _native
    n, c, ih, iw = x_shape
    dt, gdt = _check_args(x_shape, dy.dtype, dy.device, grid, 'grid_sample_backward')
    oh, ow = grid.shape[1], grid.shape[2]
    if dy.shape != (n, c, oh, ow) or (want_dgrid and (x.shape != x_shape or x.dtype != dy.dtype)):
        raise RuntimeError(f'grid_sample_backward: dy {tuple(dy.shape)} {dy.dtype} does not match the image {tuple(x_shape)} '
                           f'and the grid {tuple(grid.shape)}')
    dy, grid = dy.contiguous(), grid.contiguous()
    x = x.contiguous() if want_dgrid else None
    dx = torch.empty([n, c, ih, iw], dtype=dy.dtype, device=dy.device) if want_dx else None
    dgrid = torch.empty_like(grid) if want_dgrid else None
    lib = _native.lib()
    ws = None
    if want_dx:
        nbytes = lib.pasta_grid_sample_backward_workspace(n, c, ih, iw, dt)
        if nbytes < 0:
            _native.check(1)
        ws = torch.empty([nbytes // 4], dtype=torch.float32, device=dy.device) if nbytes > 0 else None
    with torch.cuda.device(dy.device):
        st = lib.pasta_grid_sample_backward(_native.ptr(dy), _native.ptr(x), _native.ptr(grid), _native.ptr(dx), _native.ptr(dgrid), _native.ptr(ws),
                                            n, c, ih, iw, oh, ow, dt, gdt, _native.stream())
    _native.check(st)
    return dx, dgrid

#----------------------------------------------------------------------------
# Autograd.

_NO_GRID_SECOND_ORDER = ('grid_sample_gradfix: the derivative of the image gradient S(grid)^T dy with respect to the sampling grid is not '
                         'implemented (the grid gradient is first order only, as in the reference)')

class _GridGuard(torch.autograd.Function):
    """An empty token that carries the grid into the graph of an image gradient.  The engine runs this node only when a
    gradient with respect to the grid is requested through that image gradient, and then the term is missing: raise."""
    @staticmethod
    def forward(ctx, grid):
        ctx.set_materialize_grads(False)
        return grid.new_empty([0])

    @staticmethod
    def backward(ctx, g):
        if g is not None:
            raise NotImplementedError(_NO_GRID_SECOND_ORDER)
        return None

def _engine_wants(ctx, i):
    """Whether the running backward pass uses the gradient of input i.  ``ctx.needs_input_grad`` only says the input requires one:
    ``autograd.grad(loss, [x])`` with a grid that requires a gradient would otherwise compute the grid gradient for nothing."""
    if not ctx.needs_input_grad[i]:
        return False
    node = ctx.next_functions[i][0]
    if node is None:
        return False
    try:
        return torch._C._will_engine_execute_node(node)
    except (AttributeError, RuntimeError):
        return True         # no such query in this torch, or outside a backward pass: compute it

def _guard(grid):
    """The token, when the image gradient is being built into a graph (create_graph) and the grid requires a gradient."""
    return _GridGuard.apply(grid) if torch.is_grad_enabled() and grid.requires_grad else None

class _Sample(torch.autograd.Function):
    """y = S(grid) x"""
    @staticmethod
    def forward(ctx, x, grid):
        assert x.ndim == 4 and grid.ndim == 4
        ctx.save_for_backward(x if grid.requires_grad else None, grid)      # the image is read only by the grid gradient
        ctx.x_shape = x.shape
        return _forward(x, grid)

    @staticmethod
    def backward(ctx, dy):
        x, grid = ctx.saved_tensors
        want_dx, want_dgrid = _engine_wants(ctx, 0), _engine_wants(ctx, 1)
        if want_dgrid:
            dx, dgrid = _SampleGrad.apply(dy, x, grid, _guard(grid), ctx.x_shape, want_dx)
            return (dx if want_dx else None), dgrid
        dx = _SampleAdjoint.apply(dy, grid, _guard(grid), ctx.x_shape) if want_dx else None
        return dx, None

class _SampleAdjoint(torch.autograd.Function):
    """dx = S(grid)^T dy"""
    @staticmethod
    def forward(ctx, dy, grid, token, x_shape):
        ctx.save_for_backward(grid)
        ctx.has_token = token is not None
        dx, _ = _backward(dy, None, grid, x_shape, True, False)
        return dx

    @staticmethod
    def backward(ctx, ddx):
        grid, = ctx.saved_tensors
        ddy = _Sample.apply(ddx, grid) if ctx.needs_input_grad[0] else None
        # the term through the grid is not computed: the token's node raises if the engine needs it
        return ddy, None, (grid.new_empty([0]) if ctx.has_token else None), None

class _SampleGrad(torch.autograd.Function):
    """(dx = S(grid)^T dy, grad_grid) from one launch; grad_grid is first order only."""
    @staticmethod
    def forward(ctx, dy, x, grid, token, x_shape, want_dx):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(grid)
        ctx.has_token = token is not None
        dx, dgrid = _backward(dy, x, grid, x_shape, want_dx, True)
        if dx is None:
            dx = dy.new_empty([0])
            ctx.mark_non_differentiable(dx)
        return dx, dgrid

    @staticmethod
    def backward(ctx, ddx, ddgrid):
        if ddgrid is not None:
            raise NotImplementedError('grid_sample_gradfix: grad_grid is not differentiable (no second derivative through the gradient with '
                                      'respect to the sampling grid, as in the reference)')
        grid, = ctx.saved_tensors
        used = ddx is not None and ddx.numel() > 0
        ddy = _Sample.apply(ddx, grid) if (used and ctx.needs_input_grad[0]) else None
        # dx depends on the grid whether or not dy requires a gradient: the token's node raises if the engine needs that term
        token_grad = grid.new_empty([0]) if (ctx.has_token and used) else None
        return ddy, None, None, token_grad, None, None

#----------------------------------------------------------------------------
# The affine special case on this package's own kernels (ADA's geometric step, training/augment.py).

def affine_sample(x, theta, out_hw):
    """``grid_sample(x, affine_grid(theta, [N, C, *out_hw], align_corners=False))`` (bilinear, zero padding) without the
    grid tensor, differentiable to any order in ``x``: forward ``pasta_affine_sample``; gradient ``pasta_affine_sample_adjoint``,
    a gather over the output lattice points whose footprint covers an input pixel (no atomics); the gradient of the
    gradient is the forward again."""
    return _AffineSample.apply(x, theta, (int(out_hw[0]), int(out_hw[1])))

def _affine_launch(name, src, theta, dst_shape, in_hw, out_hw):
    from . import _native
    _native.require_gpu(src, name)
    if src.dtype != torch.float32 or theta.dtype != torch.float32:
        raise RuntimeError(f'{name}: float32 only')
    n, c = src.shape[0], src.shape[1]
    if theta.shape != (n, 2, 3):
        raise RuntimeError(f'{name}: theta must be [{n}, 2, 3], got {tuple(theta.shape)}')
    src, theta = src.contiguous(), theta.contiguous()
    dst = torch.empty(dst_shape, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        st = getattr(_native.lib(), name)(_native.ptr(src), _native.ptr(theta), _native.ptr(dst), n, c, in_hw[0], in_hw[1], out_hw[0], out_hw[1],
                                          _native.stream())
    _native.check(st)
    return dst

class _AffineSample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, theta, out_hw):
        assert x.ndim == 4
        ctx.save_for_backward(theta)
        ctx.in_hw, ctx.out_hw = (x.shape[2], x.shape[3]), out_hw
        return _affine_launch('pasta_affine_sample', x, theta, [x.shape[0], x.shape[1], *out_hw], ctx.in_hw, out_hw)

    @staticmethod
    def backward(ctx, dy):
        theta, = ctx.saved_tensors
        if ctx.needs_input_grad[1]:
            raise NotImplementedError('affine_sample: no gradient with respect to theta')
        dx = _AffineSampleAdjoint.apply(dy, theta, ctx.in_hw) if ctx.needs_input_grad[0] else None
        return dx, None, None

class _AffineSampleAdjoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, theta, in_hw):
        ctx.save_for_backward(theta)
        ctx.in_hw, ctx.out_hw = in_hw, (dy.shape[2], dy.shape[3])
        return _affine_launch('pasta_affine_sample_adjoint', dy, theta, [dy.shape[0], dy.shape[1], *in_hw], in_hw, ctx.out_hw)

    @staticmethod
    def backward(ctx, ddx):
        theta, = ctx.saved_tensors
        ddy = _AffineSample.apply(ddx, theta, ctx.out_hw) if ctx.needs_input_grad[0] else None
        return ddy, None, None
