"""The region L1 term of training's unpaired pass on the GPU (csrc/region_l1.hip; include/pasta_hip.h states the definition,
DESIGN 8k what is exact and what it costs).

``region_l1_loss(images, retain, upper, lower, keep, upper_mask, lower_mask)``: for K (1 .. 4) generated images ``x_k`` (fp32
[N, 3, H, H]) the part of ``F.l1_loss`` that falls into each of three regions -- 0 where ``keep`` (uint8 [N, H, H]) is set,
against ``retain``; else 1 where ``upper_mask`` (fp32 [N, 1, H, H]) is set, against ``upper``; else 2 where ``lower_mask`` is
set, against ``lower`` -- as an fp32 [K, 3] tensor on the device, differentiable once with respect to the images.  One forward
launch serves all K images; it saves one byte per pixel and image (region and signs), from which the backward launch writes
every gradient; the upstream gradient is read from device memory.  Nothing is read back to the host.  There is no CPU path, no
gradient with respect to a target or a mask, and no second derivative: each of them raises."""

import ctypes

import torch

from . import _native

MAX_IMAGES = 4


def _check(images, retain, upper, lower, keep, upper_mask, lower_mask):
    images = tuple(images)
    if not 1 <= len(images) <= MAX_IMAGES:
        raise RuntimeError('region_l1_loss: %d images (1..%d)' % (len(images), MAX_IMAGES))
    named = [('images[%d]' % i, x) for i, x in enumerate(images)] + [('retain', retain), ('upper', upper), ('lower', lower), ('keep', keep),
                                                                     ('upper_mask', upper_mask), ('lower_mask', lower_mask)]
    for name, t in named:
        _native.require_gpu(t, 'region_l1_loss (%s)' % name)
        want = torch.uint8 if name == 'keep' else torch.float32
        if t.dtype != want:
            raise RuntimeError('region_l1_loss: %s is %s, expected %s' % (name, t.dtype, want))
        if t.device != images[0].device:
            raise RuntimeError('region_l1_loss: %s is on %s, the images on %s' % (name, t.device, images[0].device))
    x = images[0]
    if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise RuntimeError('region_l1_loss: expected [N, 3, H, H] images, got %s' % list(x.shape))
    n, _, h, _ = x.shape
    if h % 4 != 0:
        raise RuntimeError('region_l1_loss: H = %d is not a multiple of 4' % h)
    shapes = dict(keep=(n, h, h), upper_mask=(n, 1, h, h), lower_mask=(n, 1, h, h))
    for name, t in named:
        if tuple(t.shape) != shapes.get(name, (n, 3, h, h)):
            raise RuntimeError('region_l1_loss: %s is %s, expected %s' % (name, list(t.shape), list(shapes.get(name, (n, 3, h, h)))))
    for name, t in named[len(images):]:
        if t.requires_grad:
            raise NotImplementedError('region_l1_loss: no gradient with respect to %s; detach it' % name)
    return images


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class _RegionL1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, retain, upper, lower, keep, upper_mask, lower_mask, token, *images):
        images = [x.contiguous() for x in images]
        retain, upper, lower, keep, upper_mask, lower_mask = (t.contiguous() for t in (retain, upper, lower, keep, upper_mask, lower_mask))
        k, (n, _, h, _) = len(images), images[0].shape
        dev = images[0].device
        want_maps = any(ctx.needs_input_grad[7:])
        lib = _native.lib()
        nbytes = int(lib.pasta_region_l1_loss_workspace(n, h))
        work = torch.empty([max(nbytes, 8)], dtype=torch.uint8, device=dev)
        out = torch.empty([k, 3], dtype=torch.float32, device=dev)
        maps = torch.empty([k, n, h, h], dtype=torch.uint8, device=dev) if want_maps else None
        P = _native.ptr
        with torch.cuda.device(dev):
            _native.check(lib.pasta_region_l1_loss(_pointers(images), P(retain), P(upper), P(lower), P(keep), P(upper_mask), P(lower_mask), P(out),
                                                   _pointers(list(maps)) if want_maps else None, P(work), nbytes, k, n, h, _native.stream()))
        if want_maps:
            ctx.save_for_backward(maps, token)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        maps, token = ctx.saved_tensors
        grads = _RegionL1Backward.apply(maps, grad_out, token)
        return (None,) * 7 + tuple(g if need else None for g, need in zip(grads, ctx.needs_input_grad[7:]))


class _RegionL1Backward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, maps, grad_out, token):
        k, n, h, _ = maps.shape
        grad_out = grad_out.to(device=maps.device, dtype=torch.float32).contiguous()     # stays on the device: the kernel reads it
        dx = [torch.empty([n, 3, h, h], dtype=torch.float32, device=maps.device) for _ in range(k)]
        with torch.cuda.device(maps.device):
            _native.check(_native.lib().pasta_region_l1_loss_backward(_pointers(list(maps)), _native.ptr(grad_out), _pointers(dx), k, n, h,
                                                                      _native.stream()))
        return tuple(dx)

    @staticmethod
    def backward(ctx, *grad_dx):
        raise NotImplementedError('region_l1_loss: no second derivative (the gradient of the gradient is not implemented)')


def region_l1_loss(images, retain, upper, lower, keep, upper_mask, lower_mask):
    """fp32 [K, 3] on the device: row k the three region sums of ``images[k]`` divided by M = 3 N H H."""
    images = _check(images, retain, upper, lower, keep, upper_mask, lower_mask)
    # one element of every image: it ties the gradients to the images in the graph, so that a second derivative reaches
    # _RegionL1Backward.backward and raises instead of coming back as zeros; the kernels never read it
    token = torch.cat([x.reshape(-1)[:1] for x in images])
    return _RegionL1.apply(retain, upper, lower, keep, upper_mask, lower_mask, token, *images)
