"""The input-activation mask in the store of the FIR kernels (pasta_upfirdn2d_masked): the filter's transpose that ends the backward of a
low-pass in front of a stride-2 convolution, with the low-pass's saved input as the mask, against launch + stand-alone pass
(``upfirdn2d.input_grad`` with the protocol on / off).  Results must be ``torch.equal``: same fp32 value, same rule (csrc/common.h act_grad1).

Cases (dy -> dx planes, 4 x 4 filter): the issue's -- onto 32 x 32 from 33 x 33 (the tile kernel; the forward of that launch is the blur with the
remainder strip), onto 8 x 8 (the small-plane kernel), an odd plane count (one plane per work item) -- and, for the code the mask adds to the
other instances: 4096 planes (the plane-pair instance of the tile kernel takes them from 2048 work items on), 4097 planes (odd again, at that
size), and onto 33 x 33 from 32 x 32, whose last column, row and corner are stored by the remainder strip of the tile kernel.  A separable
filter and a channels-last gradient have no masked kernel: they fall back to the pass and stay equal."""

import numpy as np
import pytest
import torch

from act_grad_cases import count_passes, protocol

pytestmark = pytest.mark.gpu

SQRT2 = float(np.sqrt(2))
# name: (N, C, dy plane, pads of the transposed launch (x0, x1, y0, y1)) -> dx plane = dy + x0 + x1 - 3
CASES = {
    'tile_32_from_33':   (2, 6, (33, 33), (1, 1, 1, 1)),
    'small_8_from_9':    (2, 6, (9, 9), (1, 1, 1, 1)),
    'tile_odd_planes':   (1, 5, (33, 33), (1, 1, 1, 1)),
    'small_odd_planes':  (1, 5, (9, 9), (1, 1, 1, 1)),
    'tile_pairs_4096':   (16, 256, (33, 33), (1, 1, 1, 1)),
    'tile_odd_4097':     (1, 4097, (33, 33), (1, 1, 1, 1)),
    'tile_rem_33_from_32': (2, 6, (32, 32), (2, 2, 2, 2)),
    'tile_rem_pairs':    (16, 256, (32, 32), (2, 2, 2, 2)),
    'tile_20x65':        (1, 3, (17, 62), (3, 3, 3, 3)),
}


def _run(name, act, gain, clamp, add, f=None, channels_last=False):
    from torch_utils.ops import bias_act, upfirdn2d
    n, c, (h, w), (px0, px1, py0, py1) = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    dy = torch.randn(n, c, h, w, generator=gen).cuda()
    if f is None:
        f = upfirdn2d.setup_filter([1, 3, 3, 1]).cuda()
    fh, fw = (f.shape[0], f.shape[0]) if f.ndim == 1 else f.shape
    oh, ow = h + py0 + py1 - fh + 1, w + px0 + px1 - fw + 1
    x = (torch.randn(n, c, oh, ow, generator=gen) * 0.7).cuda()          # the low-pass's input: the activated tensor
    x = bias_act.bias_act(x, None, act=act, gain=gain, clamp=clamp)
    dxp = torch.randn(n, c, oh, ow, generator=gen).cuda() if add else None
    if channels_last:
        dy = dy.contiguous(memory_format=torch.channels_last)
    gcfg = (1, 1, 1, 1, px0, px1, py0, py1, True, 1.0)
    cfg = bias_act.act_cfg(act, None, gain, clamp)
    out = []
    for on in (False, True):
        with protocol(on), torch.no_grad(), count_passes() as cnt:
            out.append((upfirdn2d.input_grad(dy, f, gcfg, dxp, x, cfg), cnt.passes))
    if clamp is not None:
        hit = int((x.abs() >= clamp).sum())
        assert 0 < hit < x.numel(), hit
    return out, x


@pytest.mark.parametrize('add', [False, True], ids=['plain', 'addend'])
@pytest.mark.parametrize('act,gain,clamp', [('lrelu', SQRT2, 0.5), ('relu', 1.0, None), ('lrelu', 1.0, None), ('relu', SQRT2, 0.5)])
@pytest.mark.parametrize('name', list(CASES))
def test_masked_fir_equals_launch_and_pass(name, act, gain, clamp, add):
    ((ref, passes_ref), (got, passes)), x = _run(name, act, gain, clamp, add)
    assert (passes_ref, passes) == (1, 0)           # every case above has a masked kernel
    assert got.shape == x.shape and torch.equal(got, ref)
    assert float(got.abs().max()) > 0
    if act == 'relu':
        assert 0 < int((got == 0).sum()) < got.numel()


def test_what_no_kernel_masks_falls_back():
    from torch_utils.ops import upfirdn2d
    ((ref, passes_ref), (got, passes)), _ = _run('tile_32_from_33', 'lrelu', SQRT2, 0.5, True, channels_last=True)
    assert (passes_ref, passes) == (1, 1) and torch.equal(got, ref)
    f1 = upfirdn2d.setup_filter([1, 3, 3, 1], separable=True).cuda()
    assert f1.ndim == 1
    ((ref, passes_ref), (got, passes)), _ = _run('tile_32_from_33', 'lrelu', SQRT2, 0.5, False, f=f1)
    assert (passes_ref, passes) == (1, 1) and torch.equal(got, ref)


def test_masked_entry_refuses_the_generic_kernel():
    """A 5 x 5 filter runs on the generic kernel, which does not apply the mask: the predicate says so and the entry point refuses."""
    from torch_utils.ops import bias_act, upfirdn2d
    dy = torch.randn(1, 2, 40, 40).cuda()
    f = torch.ones(5, 5).cuda() / 25
    gcfg = (1, 1, 1, 1, 2, 2, 2, 2, True, 1.0)
    assert not upfirdn2d._mask_launch_ok(dy, f, gcfg)
    with pytest.raises(RuntimeError, match='input-activation mask'):
        upfirdn2d._launch(dy, f, 1, 1, 1, 1, 2, 2, 2, 2, True, 1.0, mask=(torch.randn(1, 2, 40, 40).cuda(), bias_act.act_cfg('relu', None, 1, None)))
