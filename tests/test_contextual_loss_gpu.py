"""The contextual loss on the GPU (csrc/contextual_loss.hip) against the fp64 statement of tests/contextual_ref.py.

The bound is not a constant: per quantity it is 8 x the largest deviation, over the table ``contextual_ref.CASES``, of the fp32
statement evaluated on the CPU from the fp64 one (``contextual_ref.bounds``).  1 / ((m + 1e-3) h) multiplies an error in a
distance by up to 1e4, and the fp32 statement pays that too; the factor 8 covers what it does not share with the kernels, the
MFMA's summation order and the hardware exponential.  The value deviation is relative per sample, the gradient's relative to the
largest gradient magnitude of the case (floors for the cases whose exact answer is 0: contextual_ref.VALUE_FLOOR, GRAD_FLOOR)."""
import pytest
import torch

import contextual_ref as R

pytestmark = pytest.mark.gpu


def _cu(t, dtype=None):
    return None if t is None else (t if dtype is None else t.to(dtype)).cuda()


def _run(x, y, xv, yv, upstream):
    """(loss, dx) of the op on the GPU for fp64 / uint8 CPU inputs."""
    from torch_utils.ops.contextual_loss import contextual_loss
    xg = _cu(x, torch.float32).requires_grad_(True)
    loss = contextual_loss(xg, _cu(y, torch.float32), _cu(xv), _cu(yv))
    assert loss.dtype == torch.float32 and loss.shape == (x.shape[0],) and loss.is_cuda
    dx, = torch.autograd.grad((loss * _cu(upstream, torch.float32)).sum(), xg)
    return loss.detach(), dx


@pytest.mark.parametrize('name', list(R.CASES))
def test_value_and_gradient(name):
    case, v64, g64 = R.references()[name]
    bound_v, bound_g = R.bounds()
    loss, dx = _run(*case)
    dv, dg = R.deviations(loss, dx, v64, g64)
    print('%s: value deviation %.3e (bound %.3e), gradient deviation %.3e (bound %.3e)' % (name, dv, bound_v, dg, bound_g))
    assert torch.isfinite(dx).all()
    assert dv <= bound_v and dg <= bound_g
    x, y, xv, yv, up = case
    if name == 'empty':       # no valid row (sample 0), no valid column (sample 1): exactly 0, value and gradient
        assert loss[0].item() == 0 and loss[1].item() == 0 and not dx[:2].any()
    if xv is not None:        # an invalid row gets no gradient from the N x N part; what is left is exactly 0
        rows = (xv != 0)[:, None].expand_as(x)
        assert not dx.cpu()[~rows].any()


def test_last_tile_case_is_what_it_says():
    (x, y, xv, yv, up), _, _ = R.references()['last_tile']
    xh, yh = R.normalized(x, y)
    jstar = (1 - xh.transpose(1, 2) @ yh).argmin(dim=-1)
    assert int(jstar.min()) >= 192 and xh.shape[2] == 207


@pytest.mark.parametrize('name', ['ragged', 'masked'])
def test_repeats_to_the_bit(name):
    case = R.references()[name][0]
    a, b = _run(*case), _run(*case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('name', ['plain', 'ragged'])
def test_none_is_all_ones(name):
    x, y, _, _, up = R.references()[name][0]
    ones = torch.ones([x.shape[0], x.shape[2], x.shape[3]], dtype=torch.uint8)
    a, b = _run(x, y, None, None, up), _run(x, y, ones, ones, up)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_no_n_by_n_tensor():
    """B N N fp32 would be 128 MiB here; the op's workspace and its peak allocation stay far below an eighth of that."""
    from torch_utils.ops import _native
    from torch_utils.ops.contextual_loss import contextual_loss
    b, c, hh = 2, 64, 64
    n = hh * hh
    limit = b * n * n * 4 // 8
    assert 0 < int(_native.lib().pasta_contextual_loss_workspace(b, c, n)) < limit
    gen = torch.Generator().manual_seed(3)
    x = torch.randn([b, c, hh, hh], generator=gen).abs().cuda().requires_grad_(True)
    y = torch.randn([b, c, hh, hh], generator=gen).abs().cuda()
    inputs = 2 * x.numel() * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = contextual_loss(x, y)
    dx, = torch.autograd.grad(loss.sum(), x)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print('peak %d bytes over the inputs, limit %d + %d' % (peak, limit, inputs))
    assert torch.isfinite(loss).all() and torch.isfinite(dx).all()
    assert peak < limit + inputs


def test_refusals():
    from torch_utils.ops.contextual_loss import contextual_loss
    x = torch.rand([1, 4, 3, 3]).cuda()
    y = torch.rand([1, 4, 3, 3]).cuda()
    with pytest.raises(RuntimeError):
        contextual_loss(x.cpu(), y)
    with pytest.raises(RuntimeError):
        contextual_loss(x, y.cpu())
    with pytest.raises(NotImplementedError):
        contextual_loss(x, y.clone().requires_grad_(True))
    xg = x.clone().requires_grad_(True)
    dx, = torch.autograd.grad(contextual_loss(xg, y).sum(), xg, create_graph=True)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad(dx.sum(), xg)
