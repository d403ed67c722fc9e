"""The SSIM term of the generator's loss on the GPU (csrc/ssim_loss.hip; include/pasta_hip.h states the definition, DESIGN 8j
the numerics and what it costs).

``ssim_loss(x, y, c0=0, width=None)``: 1 - mean SSIM of the generated images ``x`` against the photographs ``y`` (fp32
[N, 3, H, Wt], the networks' own values: dynamic range 2, not clipped, not quantised) over the content columns
c0 .. c0 + width - 1, as an fp32 scalar on the device, differentiable once with respect to ``x``.  The forward launch saves
three derivative maps per window position ([N, 3, 3, H - 10, width - 10]); the backward launch gathers from them and reads the
upstream gradient from device memory.  Nothing is read back to the host.  There is no CPU path: a CPU tensor is refused."""

import torch

from . import _native

WINDOW = 11


def _check(x, y, c0, width):
    _native.require_gpu(x, 'ssim_loss')
    _native.require_gpu(y, 'ssim_loss')
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise RuntimeError('ssim_loss: expected fp32 tensors, got %s and %s' % (x.dtype, y.dtype))
    if x.ndim != 4 or x.shape[1] != 3 or x.shape != y.shape or x.device != y.device:
        raise RuntimeError('ssim_loss: expected two [N, 3, H, W] tensors on one device, got %s and %s' % (list(x.shape), list(y.shape)))
    width = int(x.shape[3]) - int(c0) if width is None else int(width)
    return int(c0), width


def _forward(x, y, c0, width, want_maps):
    n, _, h, wt = x.shape
    lib = _native.lib()
    nbytes = int(lib.pasta_ssim_loss_workspace(n, h, width))
    work = torch.empty([max(nbytes, 8)], dtype=torch.uint8, device=x.device)
    loss = torch.empty([], dtype=torch.float32, device=x.device)
    dmaps = torch.empty([n, 3, 3, max(h - WINDOW + 1, 0), max(width - WINDOW + 1, 0)], dtype=torch.float32, device=x.device) if want_maps else None
    with torch.cuda.device(x.device):
        _native.check(lib.pasta_ssim_loss(_native.ptr(x), _native.ptr(y), _native.ptr(loss), _native.ptr(dmaps), _native.ptr(work), nbytes,
                                          n, h, wt, c0, width, _native.stream()))
    return loss, dmaps


class _SsimLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, c0, width):
        x, y = x.contiguous(), y.contiguous()
        want_maps = ctx.needs_input_grad[0]
        loss, dmaps = _forward(x, y, c0, width, want_maps)
        if want_maps:
            ctx.save_for_backward(x, y, dmaps)
            ctx.crop = (c0, width)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        x, y, dmaps = ctx.saved_tensors
        return _SsimLossBackward.apply(x, y, dmaps, grad_loss, *ctx.crop), None, None, None


class _SsimLossBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, dmaps, grad_loss, c0, width):
        n, _, h, wt = x.shape
        grad_loss = grad_loss.to(device=x.device, dtype=torch.float32).contiguous()      # stays on the device: the kernel reads it
        dx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            _native.check(_native.lib().pasta_ssim_loss_backward(_native.ptr(x), _native.ptr(y), _native.ptr(dmaps), _native.ptr(grad_loss),
                                                                 _native.ptr(dx), n, h, wt, c0, width, _native.stream()))
        return dx

    @staticmethod
    def backward(ctx, grad_dx):
        raise NotImplementedError('ssim_loss: no second derivative (the gradient of the gradient is not implemented)')


def ssim_loss(x, y, c0=0, width=None):
    """1 - mean SSIM of ``x`` against ``y`` over columns c0 .. c0 + width - 1 (to the last column when ``width`` is None)."""
    c0, width = _check(x, y, c0, width)
    if y.requires_grad:
        raise NotImplementedError('ssim_loss: no gradient with respect to the target; detach it')
    return _SsimLoss.apply(x, y, c0, width)
