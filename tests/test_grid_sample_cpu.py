"""grid_sample_gradfix under a general sampling grid, host side: the C ABI of the HIP kernels, and the gradient with respect
to the grid on CPU tensors (ATen's sampler), including the second-order requests that must raise."""

import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ('pasta_grid_sample', 'pasta_grid_sample_backward', 'pasta_grid_sample_backward_workspace')


def _case(seed=0, n=2, c=3, ih=5, iw=7, oh=4, ow=6):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn([n, c, ih, iw], generator=gen, dtype=torch.float64)
    # points outside [-1, 1] too; no point lands on a pixel boundary, where the sampler has a kink and finite differences disagree
    grid = torch.rand([n, oh, ow, 2], generator=gen, dtype=torch.float64) * 2.6 - 1.3
    return x, grid


def test_header_declares_and_loader_types_the_grid_sample_entries():
    from torch_utils import custom_ops
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read(), flags=re.S)
    for name in ENTRIES:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in custom_ops.ABI
    assert custom_ops.ABI['pasta_grid_sample'][0] is ctypes.c_int
    assert custom_ops.ABI['pasta_grid_sample_backward_workspace'][0] is ctypes.c_int64
    assert len(custom_ops.ABI['pasta_grid_sample'][1]) == 12 and len(custom_ops.ABI['pasta_grid_sample_backward'][1]) == 15
    assert custom_ops.EXPECTED_ABI == 22


def test_workspace_query_and_argument_guards():
    """Host-only entry points and the guards that run before any launch."""
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()
    assert lib.pasta_grid_sample_backward_workspace(16, 64, 128, 128, 0) == 0                     # fp32 dx accumulates in place
    assert lib.pasta_grid_sample_backward_workspace(16, 64, 128, 128, 1) == 16 * 64 * 128 * 128 * 4
    assert lib.pasta_grid_sample_backward_workspace(0, 64, 128, 128, 3) == -1
    null = ctypes.c_void_p(0)
    assert lib.pasta_grid_sample(null, null, null, 1, 1, 4, 4, 4, 4, 0, 0, null) != 0
    assert b'null pointer' in lib.pasta_last_error()
    one = ctypes.c_void_p(16)       # never dereferenced: the dtype guard refuses first
    assert lib.pasta_grid_sample(one, one, one, 1, 1, 4, 4, 4, 4, 1, 3, null) != 0
    assert b'dtype' in lib.pasta_last_error()
    assert lib.pasta_grid_sample_backward(one, null, one, null, one, null, 1, 1, 4, 4, 4, 4, 0, 0, null) != 0
    assert b'needs the image' in lib.pasta_last_error()


def test_library_without_the_entries_fails_on_first_use(monkeypatch):
    """A library built before an entry that was added without moving the version (an A/B build) still loads; calling the entry
    raises and asks for a rebuild.  No entry is late at present, so the test names one."""
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()
    monkeypatch.setattr(custom_ops, '_cached_plugins', {})
    monkeypatch.setattr(custom_ops, 'LATE_ENTRIES', frozenset(['pasta_grid_sample']))
    real_hasattr = hasattr

    def no_grid_sample(obj, name):
        return False if (obj is not lib and isinstance(obj, ctypes.CDLL) and name in custom_ops.LATE_ENTRIES) else real_hasattr(obj, name)
    monkeypatch.setattr(custom_ops, 'hasattr', no_grid_sample, raising=False)
    old = custom_ops.get_plugin()
    assert old is not lib
    with pytest.raises(RuntimeError, match='rebuild'):
        old.pasta_grid_sample()


def test_grid_gradient_on_cpu_matches_autograd_of_f_grid_sample():
    from torch_utils.ops import grid_sample_gradfix as gs
    x, grid = _case()
    x.requires_grad_(True)
    grid.requires_grad_(True)
    assert torch.autograd.gradcheck(gs.grid_sample, (x, grid))
    dy = torch.randn([2, 3, 4, 6], dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    got = torch.autograd.grad(gs.grid_sample(x, grid), [x, grid], dy)
    ref = torch.autograd.grad(torch.nn.functional.grid_sample(x, grid, mode='bilinear', padding_mode='zeros', align_corners=False), [x, grid], dy)
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)
    # the grid gradient alone (image without requires_grad)
    g_only, = torch.autograd.grad(gs.grid_sample(x.detach(), grid), [grid], dy)
    assert torch.allclose(g_only, ref[1], rtol=1e-12, atol=1e-12)


def test_second_order_through_the_grid_raises():
    from torch_utils.ops import grid_sample_gradfix as gs
    x, grid = _case(seed=2)
    x.requires_grad_(True)
    grid.requires_grad_(True)
    y = gs.grid_sample(x, grid)
    dx, dgrid = torch.autograd.grad(y.square().sum(), [x, grid], create_graph=True)
    with pytest.raises(NotImplementedError, match='grad_grid'):
        torch.autograd.grad(dgrid.square().sum(), [x], retain_graph=True)
    with pytest.raises(NotImplementedError, match='sampling grid'):
        torch.autograd.grad(dx.square().sum(), [grid], retain_graph=True)
    # the image gradient alone, taken while the grid requires a gradient
    dx2, = torch.autograd.grad(gs.grid_sample(x, grid).square().sum(), [x], create_graph=True)
    with pytest.raises(NotImplementedError, match='sampling grid'):
        torch.autograd.grad(dx2.sum(), [grid], retain_graph=True)
    # what stays differentiable: R1-style, the image gradient's gradient with respect to the image
    r1, = torch.autograd.grad(dx.square().sum(), [x])
    r1b, = torch.autograd.grad(dx2.square().sum(), [x])
    assert torch.equal(r1, r1b)
    assert torch.autograd.gradgradcheck(lambda t: gs.grid_sample(t, grid.detach()), (x,))


@pytest.mark.parametrize('loss', ['linear', 'square'])
@pytest.mark.parametrize('wrt', ['x', 'x_grid'])
def test_second_order_through_the_grid_raises_for_any_loss(loss, wrt):
    """A loss linear in y makes dy a constant, so nothing differentiates dy -- the term of dx through the grid is still needed and
    must raise, for grad(...) and for .backward() into a parameter that produced the grid."""
    from torch_utils.ops import grid_sample_gradfix as gs
    x, base = _case(seed=3)
    x.requires_grad_(True)
    p = torch.zeros_like(base, requires_grad=True)
    grid = base + 0.1 * p
    y = gs.grid_sample(x, grid)
    out = y.sum() if loss == 'linear' else (y * y).sum()
    dx = torch.autograd.grad(out, [x] if wrt == 'x' else [x, grid], create_graph=True)[0]
    with pytest.raises(NotImplementedError, match='sampling grid'):
        torch.autograd.grad(dx.square().sum(), [grid], allow_unused=True, retain_graph=True)
    with pytest.raises(NotImplementedError, match='sampling grid'):
        dx.square().sum().backward(retain_graph=True)
    assert p.grad is None


def test_backward_computes_only_the_requested_gradients(monkeypatch):
    """A grid that requires a gradient does not make an image-only request compute the grid gradient, nor the reverse."""
    from torch_utils.ops import grid_sample_gradfix as gs
    calls = []
    real = gs._backward
    monkeypatch.setattr(gs, '_backward', lambda dy, x, grid, x_shape, want_dx, want_dgrid:
                        (calls.append((want_dx, want_dgrid)), real(dy, x, grid, x_shape, want_dx, want_dgrid))[1])
    x, grid = _case(seed=4)
    x.requires_grad_(True)
    grid.requires_grad_(True)
    for inputs, expect in (([x], (True, False)), ([grid], (False, True)), ([x, grid], (True, True))):
        calls.clear()
        torch.autograd.grad(gs.grid_sample(x, grid).sum(), inputs)
        assert calls == [expect], (len(inputs), calls)
