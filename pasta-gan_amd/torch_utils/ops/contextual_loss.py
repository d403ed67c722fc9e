"""The contextual loss on the GPU (csrc/contextual_loss.hip; include/pasta_hip.h states the definition, DESIGN 8l what is exact and
what it costs): "the same texture, not necessarily in the same place".

``contextual_loss(x, y, x_valid=None, y_valid=None, h=0.1)``: for fp32 [B, C, H, W] feature maps, N = H W positions each, both
centred on y's channel mean per position and scaled to unit length, d_ij = 1 - x^_i . y^_j, and per sample
-log(mean_i max_j softmax-like affinity of row i) as an fp32 [B] tensor on the device, differentiable once with respect to ``x``.
``x_valid`` / ``y_valid`` (uint8 [B, H, W] or None) remove rows from the mean and columns from existence; None is all valid and
gives the same bits as all-ones masks.  The centring and the normalisation are torch ops here (O(B C N), autograd gives their
backward); everything N x N is HIP: no B N N tensor is ever allocated, the forward saves five numbers per row, the upstream
gradient is read from device memory, nothing is read back to the host.  There is no CPU path, no gradient with respect to ``y`` or
a mask, and no second derivative: each of them raises."""

import torch

from . import _native

EPS = 2.220446049250313e-16      # the reference's feature_normalize adds sys.float_info.epsilon to the norm
MAX_C, MAX_N = 512, 16384


def _check(x, y, x_valid, y_valid, h):
    for name, t in (('x', x), ('y', y), ('x_valid', x_valid), ('y_valid', y_valid)):
        if t is None:
            continue
        _native.require_gpu(t, 'contextual_loss (%s)' % name)
        want = torch.float32 if name in ('x', 'y') else torch.uint8
        if t.dtype != want:
            raise RuntimeError('contextual_loss: %s is %s, expected %s' % (name, t.dtype, want))
        if t.device != x.device:
            raise RuntimeError('contextual_loss: %s is on %s, x on %s' % (name, t.device, x.device))
    if x.ndim != 4 or x.shape != y.shape:
        raise RuntimeError('contextual_loss: expected x and y of one shape [B, C, H, W], got %s and %s' % (list(x.shape), list(y.shape)))
    b, c, hh, ww = x.shape
    if not (b >= 1 and 1 <= c <= MAX_C and 1 <= hh * ww <= MAX_N):
        raise RuntimeError('contextual_loss: bad shape %s (C <= %d, H W <= %d)' % (list(x.shape), MAX_C, MAX_N))
    for name, t in (('x_valid', x_valid), ('y_valid', y_valid)):
        if t is not None and tuple(t.shape) != (b, hh, ww):
            raise RuntimeError('contextual_loss: %s is %s, expected %s' % (name, list(t.shape), [b, hh, ww]))
    if y.requires_grad:
        raise NotImplementedError('contextual_loss: no gradient with respect to y; detach it')
    if not float(h) > 0:
        raise ValueError('contextual_loss: the bandwidth h must be positive')


class _Contextual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xh, yh, x_valid, y_valid, h):
        xh, yh = xh.contiguous(), yh.contiguous()
        x_valid = None if x_valid is None else x_valid.contiguous()
        y_valid = None if y_valid is None else y_valid.contiguous()
        b, c, n = xh.shape
        lib = _native.lib()
        nbytes = int(lib.pasta_contextual_loss_workspace(b, c, n))
        work = torch.empty([max(nbytes, 8)], dtype=torch.uint8, device=xh.device)
        loss = torch.empty([b], dtype=torch.float32, device=xh.device)
        P = _native.ptr
        with torch.cuda.device(xh.device):
            _native.check(lib.pasta_contextual_loss(P(xh), P(yh), P(x_valid), P(y_valid), P(loss), P(work), nbytes, b, c, n, h, _native.stream()))
        ctx.h = h
        ctx.masks = (x_valid, y_valid)
        ctx.save_for_backward(xh, yh, work)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        xh, yh, work = ctx.saved_tensors
        return _ContextualBackward.apply(xh, yh, work, grad_loss, ctx.masks[0], ctx.masks[1], ctx.h), None, None, None, None


class _ContextualBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xh, yh, work, grad_loss, x_valid, y_valid, h):
        b, c, n = xh.shape
        grad_loss = grad_loss.to(device=xh.device, dtype=torch.float32).contiguous()      # stays on the device: the kernel reads it
        yht = yh.transpose(1, 2).contiguous()          # [B, N, C]: the second product's operand rows
        dxh = torch.empty_like(xh)
        P = _native.ptr
        with torch.cuda.device(xh.device):
            _native.check(_native.lib().pasta_contextual_loss_backward(P(xh), P(yh), P(yht), P(x_valid), P(y_valid), P(work), P(grad_loss), P(dxh),
                                                                       b, c, n, h, _native.stream()))
        return dxh

    @staticmethod
    def backward(ctx, grad_dxh):
        raise NotImplementedError('contextual_loss: no second derivative (the gradient of the gradient is not implemented)')


def normalized(x, y):
    """x^ and y^ as [B, C, N]: both centred on y's channel mean per position, then scaled to unit length."""
    b, c = x.shape[:2]
    mu = y.mean(dim=1, keepdim=True)
    x, y = x - mu, y - mu
    x = x / (x.norm(dim=1, keepdim=True) + EPS)
    y = y / (y.norm(dim=1, keepdim=True) + EPS)
    return x.reshape(b, c, -1), y.reshape(b, c, -1)


def contextual_loss(x, y, x_valid=None, y_valid=None, h=0.1):
    """fp32 [B] on the device: per sample -log of the mean over the valid rows of CX_i."""
    _check(x, y, x_valid, y_valid, h)
    xh, yh = normalized(x, y)
    return _Contextual.apply(xh, yh, x_valid, y_valid, float(h))
