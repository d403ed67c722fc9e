"""The SSIM loss on the GPU (csrc/ssim_loss.hip through torch_utils/ops/ssim_loss.py) against the fp64 reference of
tests/ssim_loss_ref.py: value and gradient on every shape and content of its table, repeatability, the crop, the upstream
gradient, the refusals, and the loss's kernel against the metric's on byte-grid images."""
import functools

import numpy as np
import pytest
import torch

import recon_ref
import ssim_loss_ref as R

pytestmark = pytest.mark.gpu

ALL = [(shape, content) for shape in R.CASES for content in R.CONTENTS]
CROPPED = (2, 23, 40, 3, 25)


@functools.lru_cache(maxsize=None)
def _reference(shape, content):
    """(x, y, loss64, grad64) of a case: computed once, shared and left unchanged."""
    x, y = R.make_case(shape, content)
    loss, grad = R.loss_and_grad(x, y, shape[3], shape[4])
    for a in (x, y, grad):
        a.setflags(write=False)
    return x, y, loss, grad


def _gpu(shape, content):
    x, y, _, _ = _reference(shape, content)
    return torch.from_numpy(x.copy()).cuda().requires_grad_(True), torch.from_numpy(y.copy()).cuda()


def _loss_and_grad(x, y, shape):
    from torch_utils.ops.ssim_loss import ssim_loss
    loss = ssim_loss(x, y, shape[3], shape[4])
    (grad,) = torch.autograd.grad(loss, x)
    return loss, grad


@pytest.mark.parametrize('shape, content', ALL, ids=['%s-%s' % ('x'.join(map(str, s)), c) for s, c in ALL])
def test_value_and_gradient_against_fp64(shape, content):
    _, _, loss64, grad64 = _reference(shape, content)
    x, y = _gpu(shape, content)
    loss, grad = _loss_and_grad(x, y, shape)
    assert loss.dtype == torch.float32 and loss.shape == () and grad.shape == x.shape and grad.dtype == torch.float32
    value = abs(float(loss.detach()) - loss64)
    gradient = R.grad_error(grad.cpu().numpy(), grad64, R.windows(shape))
    print(f'{shape} {content}: value {value:.3e} gradient {gradient:.3e}')
    assert value <= R.VALUE_TOL, (value, R.VALUE_TOL)
    assert gradient <= R.GRAD_TOL, (gradient, R.GRAD_TOL)


@pytest.mark.parametrize('shape', [R.CASES[3], CROPPED, R.CASES[5]])
def test_two_calls_give_the_same_bits(shape):
    for content in ('noise', 'near_white'):
        x, y = _gpu(shape, content)
        loss_a, grad_a = _loss_and_grad(x, y, shape)
        loss_b, grad_b = _loss_and_grad(x.detach().clone().requires_grad_(True), y.clone(), shape)
        assert torch.equal(loss_a, loss_b)
        assert torch.equal(grad_a.view(torch.int32), grad_b.view(torch.int32))        # the bits: NaN-proof and sign-of-zero-proof


@pytest.mark.parametrize('shape', [CROPPED, R.CASES[5]])
def test_the_gradient_is_zero_outside_the_crop_and_finite(shape):
    _, _, wt, c0, w = shape
    for content in R.CONTENTS:
        x, y = _gpu(shape, content)
        assert torch.isnan(x[..., :c0]).all() and torch.isnan(x[..., c0 + w:]).all() and torch.isnan(y[..., :c0]).all()
        loss, grad = _loss_and_grad(x, y, shape)
        assert torch.isfinite(loss) and torch.isfinite(grad).all()
        outside = torch.cat([grad[..., :c0], grad[..., c0 + w:]], dim=3)
        assert outside.numel() == grad.numel() // wt * (wt - w) and (outside.view(torch.int32) == 0).all()          # +0.0 exactly


def test_an_upstream_gradient_on_the_device_scales_the_gradient():
    from torch_utils.ops.ssim_loss import ssim_loss
    shape = R.CASES[5]
    x, y = _gpu(shape, 'close')
    _, base = _loss_and_grad(x, y, shape)
    inside = slice(shape[3], shape[3] + shape[4])

    def close(got, factor):
        want = (base[..., inside].double() * factor).float()                           # the scalar product, rounded once
        ulp = torch.maximum((torch.nextafter(want.abs(), want.abs() + 1) - want.abs()), torch.full_like(want, 2.0 ** -149))
        assert ((got[..., inside] - want).abs() <= ulp).all()

    x1 = x.detach().clone().requires_grad_(True)
    (2.5 * ssim_loss(x1, y, shape[3], shape[4])).backward()
    close(x1.grad, 2.5)
    x2 = x.detach().clone().requires_grad_(True)
    g = torch.tensor(-0.3, device='cuda')
    ssim_loss(x2, y, shape[3], shape[4]).backward(g)
    close(x2.grad, float(g))
    x3 = x.detach().clone().requires_grad_(True)
    weight = torch.tensor(7.0, device='cuda', requires_grad=True)                       # a graph through the factor: still no host read
    (ssim_loss(x3, y, shape[3], shape[4]) * weight * 0.5).backward()
    close(x3.grad, 3.5)


def test_value_only_and_non_contiguous_inputs():
    from torch_utils.ops.ssim_loss import ssim_loss
    shape = R.CASES[3]
    x, y = _gpu(shape, 'sinusoid')
    loss, grad = _loss_and_grad(x, y, shape)
    value = ssim_loss(x.detach(), y, shape[3], shape[4])
    assert not value.requires_grad and value.grad_fn is None and torch.equal(value, loss.detach())
    with torch.no_grad():
        assert torch.equal(ssim_loss(x, y, shape[3], shape[4]), loss.detach())
    # x and y as transposed views of [N, 3, Wt, H] storage
    xt = x.detach().transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)
    yt = y.transpose(2, 3).contiguous().transpose(2, 3)
    assert not xt.is_contiguous() and not yt.is_contiguous()
    loss_t, grad_t = _loss_and_grad(xt, yt, shape)
    assert torch.equal(loss_t, loss) and torch.equal(grad_t, grad)
    # the default crop is the whole width
    assert torch.equal(ssim_loss(x.detach(), y), value)


def test_refusals():
    from torch_utils.ops.ssim_loss import ssim_loss
    x = torch.rand([1, 3, 16, 16], device='cuda')
    y = torch.rand([1, 3, 16, 16], device='cuda')
    with pytest.raises(RuntimeError, match='fp32'):
        ssim_loss(x.half(), y.half())
    with pytest.raises(RuntimeError, match='fp32'):
        ssim_loss(x, y.double())
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):
        ssim_loss(x.cpu(), y.cpu())
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):
        ssim_loss(x, y.cpu())
    with pytest.raises(NotImplementedError, match='no gradient with respect to the target'):
        ssim_loss(x, y.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='smaller than the 11 x 11 SSIM window'):
        ssim_loss(x[:, :, :10], y[:, :, :10])
    with pytest.raises(RuntimeError, match='bad shape or crop'):
        ssim_loss(x, y, 4, 13)
    with pytest.raises(RuntimeError, match=r'two \[N, 3, H, W\] tensors'):
        ssim_loss(x, y[:, :, :12])
    # a second derivative is refused, not returned as zeros
    xg = x.clone().requires_grad_(True)
    (grad,) = torch.autograd.grad(ssim_loss(xg, y), xg, create_graph=True)
    assert grad.requires_grad
    with pytest.raises(NotImplementedError, match='no second derivative'):
        torch.autograd.grad(grad.square().sum(), xg)


def test_the_loss_kernel_against_the_metric_kernel_on_the_byte_grid():
    """On images that lie on the byte grid, 1 - loss is the mean over the images of recon_image_stats' ssim / windows."""
    from metrics import metric_utils
    from torch_utils.ops.ssim_loss import ssim_loss
    n, h, wt, c0, w = 2, 40, 64, 8, 48
    rng = np.random.RandomState(11)
    photo = rng.randint(0, 256, [n, h, w, 3])
    smooth = np.clip(128 + 100 * np.sin(np.arange(h).reshape(1, h, 1, 1) * 0.2 + np.arange(w).reshape(1, 1, w, 1) * 0.15), 0, 255).astype(np.int64)
    photo[1] = smooth[0] + rng.randint(0, 4, [h, w, 3])
    gen = np.clip(photo + rng.randint(-12, 13, photo.shape), 0, 255)
    x = np.full([n, 3, h, wt], np.nan, np.float32)
    y = np.full([n, 3, h, wt], np.nan, np.float32)
    x[..., c0:c0 + w] = R.from_bytes(gen).transpose(0, 3, 1, 2)
    y[..., c0:c0 + w] = R.from_bytes(photo).transpose(0, 3, 1, 2)
    assert (recon_ref.to_u8(x[..., c0:c0 + w]).transpose(0, 2, 3, 1) == gen).all()
    x, y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    sums, ssim = metric_utils.recon_image_stats(x, torch.from_numpy(photo.astype(np.uint8)).cuda(), c0)
    metric = float((ssim / sums[:, 2].double()).mean())
    loss = float(ssim_loss(x, y, c0, w))
    want = float(np.mean([recon_ref.ssim_map(gen[i, :, :, c], photo[i, :, :, c]).mean() for i in range(n) for c in range(3)]))
    print(f'byte grid: 1 - loss {1 - loss:.9f} metric {metric:.9f} fp64 {want:.9f}')
    assert abs(metric - want) <= recon_ref.SSIM_TOL
    assert abs((1 - loss) - metric) <= recon_ref.SSIM_TOL + R.VALUE_TOL
