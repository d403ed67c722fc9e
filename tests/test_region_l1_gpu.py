"""The region L1 term on the GPU (csrc/region_l1.hip) against the fp64 reference of tests/region_l1_ref.py.

Value: |out - ref64| <= 2^-22 |ref64|.  A difference of two fp32 values is exact in fp64 and the kernel rounds it once to fp32
(2^-24 of a non-negative term, so 2^-24 of the sum), the sums are fp64, and the quotient rounds once more to fp32 (2^-24):
2^-23 and a little, bounded by 2^-22.  An empty region gives exactly 0.
Gradient: bit for bit ``torch.where(x > t, q, torch.where(x < t, -q, 0))`` with q = g[k][r] / M as ONE fp32 division, evaluated by
torch on the GPU (a tensor by a tensor: torch multiplies by the reciprocal when the divisor is a Python number)."""
import numpy as np
import pytest
import torch

import region_l1_ref as R

pytestmark = pytest.mark.gpu


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope='module')
def cases():
    """{(shape, content): (the numpy case, its tensors on the GPU, the fp64 values)}: computed once and left unchanged."""
    out = {}
    for shape in R.CASES:
        for content in R.CONTENTS:
            case = R.make_case(shape, content)
            out[shape, content] = (case, ([_cu(x) for x in case[0]],) + tuple(_cu(a) for a in case[1:]), R.values(*case))
    return out


def _upstream(K):
    """Three different entries per image, none a power of two."""
    return (torch.arange(1, 3 * K + 1, dtype=torch.float32).reshape(K, 3) * 0.37 - 1.0).cuda()


def _expected_gradients(dev, g):
    images, retain, upper, lower, keep, um, lm = dev
    n, _, h, _ = images[0].shape
    M = torch.full([], float(3 * n * h * h), dtype=torch.float32, device='cuda')
    in0 = (keep != 0)[:, None]
    in1 = ~in0 & (um != 0)
    in2 = ~in0 & ~in1 & (lm != 0)
    zero = torch.zeros([], device='cuda')
    want = []
    for k, x in enumerate(images):
        dx = torch.zeros_like(x)
        for r, (t, inside) in enumerate(((retain, in0), (upper, in1), (lower, in2))):
            q = g[k, r] / M
            dx = torch.where(inside, torch.where(x > t, q, torch.where(x < t, -q, zero)), dx)
        want.append(dx)
    return want


@pytest.mark.parametrize('shape', R.CASES)
def test_values_and_gradients(cases, shape):
    from torch_utils.ops.region_l1_loss import region_l1_loss
    K = shape[0]
    g = _upstream(K)
    for content in R.CONTENTS:
        case, dev, ref = cases[shape, content]
        images = [x.clone().requires_grad_(True) for x in dev[0]]
        out = region_l1_loss(images, *dev[1:])
        assert out.shape == (K, 3) and out.dtype == torch.float32 and out.is_cuda
        got = out.detach().cpu().double().numpy()
        err = np.abs(got - ref)
        print(f'{shape} {content}: largest |out - ref| / |ref| = {(err / np.maximum(ref, 1e-300)).max():.3e}')
        assert (err <= R.VALUE_RTOL * np.abs(ref)).all(), (content, got, ref)
        assert (got[ref == 0] == 0).all()
        region = R.regions(*case[4:])
        for r in range(3):
            assert ((region == r).any() or not ref[:, r].any())
        if content == 'none':
            assert not got.any()
        if content in ('keep', 'overlap'):
            assert not got[:, 1:].any() and got[:, 0].all()
        grads = torch.autograd.grad((out * g).sum(), images)
        for k, (dx, want) in enumerate(zip(grads, _expected_gradients(dev, g))):
            assert dx.dtype == torch.float32 and torch.equal(dx, want), (content, k, int((dx != want).sum()))
        if content == 'equal':
            assert any(bool(((dx == 0) & torch.from_numpy(region >= 0).cuda()[:, None]).any()) for dx in grads)
        # a value-only call returns the bits of the call that also saves the byte map
        with torch.no_grad():
            assert torch.equal(region_l1_loss(dev[0], *dev[1:]), out.detach())


def test_the_value_is_the_part_of_l1_loss_in_the_regions(cases):
    from torch_utils.ops.region_l1_loss import region_l1_loss
    _, dev, _ = cases[(2, 3, 12), 'overlap']
    out = region_l1_loss(dev[0], *dev[1:])
    for k, x in enumerate(dev[0]):
        want = torch.nn.functional.l1_loss(x.double(), dev[1].double())
        assert abs(float(out[k, 0]) - float(want)) <= 2.0 ** -22 * float(want)


def test_two_calls_give_equal_bits(cases):
    from torch_utils.ops.region_l1_loss import region_l1_loss
    shape = (2, 2, 64)
    _, dev, _ = cases[shape, 'blobs']
    g = _upstream(shape[0])
    runs = []
    for _ in range(2):
        images = [x.clone().requires_grad_(True) for x in dev[0]]
        out = region_l1_loss(images, *dev[1:])
        runs.append((out.detach(),) + torch.autograd.grad((out * g).sum(), images))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_only_the_asked_gradients_are_returned(cases):
    from torch_utils.ops.region_l1_loss import region_l1_loss
    _, dev, _ = cases[(2, 3, 12), 'blobs']
    first = dev[0][0].clone().requires_grad_(True)
    out = region_l1_loss([first, dev[0][1]], *dev[1:])
    (dx,) = torch.autograd.grad(out.sum(), [first])
    assert torch.equal(dx, _expected_gradients(dev, torch.ones([2, 3], device='cuda'))[0])


def test_the_refusals(cases):
    from torch_utils.ops.region_l1_loss import region_l1_loss
    _, dev, _ = cases[(2, 3, 12), 'blobs']
    images, rest = dev[0], list(dev[1:])
    names = ['retain', 'upper', 'lower', 'keep', 'upper_mask', 'lower_mask']
    # no gradient with respect to a target or a mask
    for i in (0, 1, 2, 4, 5):
        args = list(rest)
        args[i] = args[i].clone().requires_grad_(True)
        with pytest.raises(NotImplementedError, match='no gradient with respect to ' + names[i]):
            region_l1_loss(images, *args)
    # no second derivative
    x = [t.clone().requires_grad_(True) for t in images]
    out = region_l1_loss(x, *rest)
    (dx, _) = torch.autograd.grad(out.sum(), x, create_graph=True)
    assert dx.requires_grad
    with pytest.raises(NotImplementedError, match='no second derivative'):
        torch.autograd.grad(dx.square().sum(), x)
    # a CPU tensor, another dtype, H % 4 != 0, too many images, another shape
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):
        region_l1_loss([images[0].cpu(), images[1]], *rest)
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):
        region_l1_loss(images, rest[0].cpu(), *rest[1:])
    for dtype in (torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(RuntimeError, match='expected torch.float32'):
            region_l1_loss([images[0].to(dtype), images[1]], *rest)
    with pytest.raises(RuntimeError, match='keep is torch.float32, expected torch.uint8'):
        region_l1_loss(images, rest[0], rest[1], rest[2], rest[3].float(), rest[4], rest[5])
    with pytest.raises(RuntimeError, match='upper_mask is torch.uint8, expected torch.float32'):
        region_l1_loss(images, rest[0], rest[1], rest[2], rest[3], rest[4].to(torch.uint8), rest[5])
    odd = lambda t: t[..., :10, :10].contiguous()
    with pytest.raises(RuntimeError, match='H = 10 is not a multiple of 4'):
        region_l1_loss([odd(t) for t in images], *[odd(t) for t in rest])
    with pytest.raises(RuntimeError, match=r'5 images \(1..4\)'):
        region_l1_loss([images[0]] * 5, *rest)
    with pytest.raises(RuntimeError, match=r'0 images \(1..4\)'):
        region_l1_loss([], *rest)
    with pytest.raises(RuntimeError, match='lower_mask is'):
        region_l1_loss(images, *rest[:5], rest[5][:, 0])
