"""The input-activation mask in the store of the input-gradient convolutions (include/pasta_hip.h, pasta_act_mask; conv2d_gradfix
``_ACT_GRAD_IN_WRITER``): a producer ``y = bias_act(conv(x, w0), b0)`` and its one reader ``z = conv(y, w1)``, gradients with the protocol on
against the protocol off (every layer runs its own pass).

The gradient dz at the producer's convolution and every input / weight gradient must be ``torch.equal``: the fused store multiplies the same
fp32 value by the same slope (csrc/common.h, act_grad1).  The bias gradient is summed from the same dz by a read-only pass and is held to the
bound of the existing bias-gradient test (tests/test_ops_gpu.py test_bias_act_large: rel_err < 1e-4).  Seen on the MI355X: 0 in every case.
The sum has the partial-sum shape the unfused path has for the same tensor -- ``pasta_bias_sum_db`` (the order of the pass with the bias
sum folded in) where that pass would have run (planes of at least 256 sixteen-byte packs: the 100 x 100 case here), ``pasta_bias_grad``
otherwise -- so it is bit-identical; summed by ``pasta_bias_grad`` throughout, the 100 x 100 case differed by up to 2.1e-7.

Shapes.  A case names the MASKED launch, ``dz [N, c_z, H, W] -> [N, c_y, H, W]``.  The issue's cases come first, as stated: N = 1 on planes of
8 x 32, 8 x 64, 16 x 32 (128 -> 128), three groups of 16 -> 128, 64 -> 64 on 8 x 32 and 16 -> 32 on 4 x 4.  With one sample all of them have
at most 512 pixels, where the planner slices K (plan kernel 7, two slices: the 128 -> 128 planes) or takes the fp32 tile (plan kernel 0: 64 -> 64
and 16 -> 32): those do not qualify and check the fall-back (launch + pass, still equal) -- the forced K-sliced launch among them.  Only the three
groups of 16 input channels (144 channel-taps: too few to slice) run the mask in the store at N = 1.  What the planner reports is asserted
for every case, so that a change of the planner shows here.  The
cases that run the mask in the store are the same planes with enough samples for more than 8192 pixels (no K slices): the eight-wave tile
(plan kernel 7; 8 x 64 and 16 x 32 planes put two tiles on one halo; three groups of 16 input channels leave the last K chunk partial) and the
64 x 256 tile (plan kernel 6).  The base kernel was asked for as well and is left out (BASE_CASES below says why): its launches fall back."""

import numpy as np
import pytest
import torch

from act_grad_cases import count_passes, dgrad_plan, protocol
from conftest import rel_err

pytestmark = pytest.mark.gpu

SQRT2 = float(np.sqrt(2))
# name: (N, c_z, c_y, groups, H, W, k), expected (plan kernel, K slices > 1, mask in the store)
ISSUE_CASES = {
    'issue_wide_8x32':    ((1, 128, 128, 1, 8, 32, 3), (7, True, False)),
    'issue_wide_8x64':    ((1, 128, 128, 1, 8, 64, 3), (7, True, False)),
    'issue_wide_16x32':   ((1, 128, 128, 1, 16, 32, 3), (7, True, False)),
    'issue_wide_groups3': ((1, 48, 384, 3, 8, 32, 3), (7, False, True)),
    'issue_r8_8x32':      ((1, 64, 64, 1, 8, 32, 3), (0, False, False)),
    'issue_base_4x4':     ((1, 16, 32, 1, 4, 4, 3), (0, False, False)),
}
FUSED_CASES = {
    'wide_8x32':    ((36, 128, 128, 1, 8, 32, 3), (7, False, True)),
    'wide_8x64':    ((18, 128, 128, 1, 8, 64, 3), (7, False, True)),
    'wide_16x32':   ((18, 128, 128, 1, 16, 32, 3), (7, False, True)),
    'wide_groups3': ((36, 48, 384, 3, 8, 32, 3), (7, False, True)),
    'r8_8x32':      ((36, 64, 64, 1, 8, 32, 3), (6, False, True)),
}
# the base kernel (plan kernel 1) does not apply the mask -- its three-workgroup instances went to scratch with the masked store --: these
# launches, without K slices, fall back as well.  A 4 x 4 plane with pointwise weights 16 -> 80, and a 100 x 100 plane that no 2-D tile divides,
# 128 -> 80: both leave the 128-row tile partly empty.
BASE_CASES = {
    'base_4x4_pointwise': ((1, 16, 80, 1, 4, 4, 1), (1, False, False)),
    'base_100x100': ((1, 128, 80, 1, 100, 100, 3), (1, False, False)),
}
CASES = {**ISSUE_CASES, **FUSED_CASES, **BASE_CASES}
ACTS = [(act, gain, clamp) for act in ('relu', 'lrelu') for gain in (1.0, SQRT2) for clamp in (None, 0.5)]
# the whole activation matrix on one shape per kernel; one clamped lrelu and one plain relu on the others
PARAMS = [(name, act, gain, clamp) for name in ('wide_8x32', 'r8_8x32', 'issue_wide_8x32') for act, gain, clamp in ACTS] + \
         [(name, act, gain, clamp) for name in CASES if name not in ('wide_8x32', 'r8_8x32', 'issue_wide_8x32')
          for act, gain, clamp in (('lrelu', SQRT2, 0.5), ('relu', 1.0, None))]

worst_db = [0.0]


def _tensors(name):
    (n, c_z, c_y, groups, h, w, k), _ = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    r = lambda *s: torch.randn(*s, generator=gen)
    c_x = 16
    return dict(x=r(n, c_x, h, w).cuda(), w0=(r(c_y, c_x, 3, 3) / np.sqrt(c_x * 9)).cuda(), b0=(r(c_y) * 0.3).cuda(),
                w1=(r(c_z, c_y // groups, k, k) / np.sqrt(c_y // groups * k * k)).cuda(), gz=r(n, c_z, h, w).cuda(), gy=r(n, c_y, h, w).cuda())


def _pair(t, name, act, gain, clamp, join):
    """Gradients of producer and reader; ``join``: y has a second reader whose gradient gy arrives through ``passthrough``."""
    from torch_utils.ops import bias_act, conv2d_gradfix
    (n, c_z, c_y, groups, h, w, k), _ = CASES[name]
    x, w0, b0, w1 = (t[key].clone().requires_grad_(True) for key in ('x', 'w0', 'b0', 'w1'))
    pair = conv2d_gradfix.act_grad_pair_ok(x, act)
    cfg = bias_act.act_cfg(act, None, gain, clamp) if pair else None
    y = conv2d_gradfix.conv2d_bias_act(x, w0, b0, padding=1, act=act, gain=gain, clamp=clamp, defer_act_grad=pair)
    if join:
        z, y2 = conv2d_gradfix.conv2d_bias_act(y, w1, None, padding=k // 2, groups=groups, act='linear', passthrough=True, input_act=cfg)
        loss = (z * t['gz']).sum() + (y2 * t['gy']).sum()
    else:
        z = conv2d_gradfix.conv2d(y, w1, padding=k // 2, groups=groups, input_act=cfg)
        loss = (z * t['gz']).sum()
    with count_passes() as c:
        grads = torch.autograd.grad(loss, [x, w0, b0, w1])
    return y.detach(), grads, c.passes


def _dz(t, name, y, act, gain, clamp, join):
    """The masked launch on its own: dz of the producer from the reader's input-gradient launch (``_input_grad``)."""
    from torch_utils.ops import bias_act, conv2d_gradfix
    (n, c_z, c_y, groups, h, w, k), _ = CASES[name]
    cfg = conv2d_gradfix._Cfg((False, 1, k // 2, k // 2, 0, 0, groups, 1.0))
    gcfg = conv2d_gradfix._grad_cfg(cfg, (h, w), (h, w), k, k)
    with torch.no_grad(), count_passes() as c:
        dz = conv2d_gradfix._input_grad(t['gz'], t['w1'], gcfg, t['gy'] if join else None, y, bias_act.act_cfg(act, None, gain, clamp), None)
    return dz, c.passes


@pytest.mark.parametrize('join', [False, True], ids=['plain', 'join'])
@pytest.mark.parametrize('name,act,gain,clamp', PARAMS, ids=[f'{p[0]}-{p[1]}-g{p[2]:.2f}-c{p[3]}' for p in PARAMS])
def test_masked_input_gradient_equals_launch_and_pass(name, act, gain, clamp, join):
    (n, c_z, c_y, groups, h, w, k), (want_kernel, want_sliced, want_mask) = CASES[name]
    kernel, ksplit, mask_ok = dgrad_plan(n, c_z, c_y, groups, h, w, k)
    assert (kernel, ksplit > 1, mask_ok) == (want_kernel, want_sliced, want_mask), (kernel, ksplit, mask_ok)
    t = _tensors(name)
    with protocol(False):
        y_ref, g_ref, passes_ref = _pair(t, name, act, gain, clamp, join)
        dz_ref, dz_passes_ref = _dz(t, name, y_ref, act, gain, clamp, join)
    with protocol(True):
        y, g, passes = _pair(t, name, act, gain, clamp, join)
        dz, dz_passes = _dz(t, name, y, act, gain, clamp, join)
    assert torch.equal(y, y_ref)
    if clamp is not None:                       # the clamp bites on some elements, not on all
        hit = int((y.abs() >= clamp).sum())
        assert 0 < hit < y.numel(), hit
    assert 0 < int((y > 0).sum()) < y.numel()
    # the pass runs exactly where no kernel applies the mask (K slices, the fp32 tile); the unfused side always runs it
    assert (passes_ref, dz_passes_ref) == (1, 1)
    assert (passes, dz_passes) == ((0, 0) if mask_ok else (1, 1))
    assert torch.equal(dz, dz_ref)
    assert float(dz.abs().max()) > 0
    for got, ref, what in zip(g, g_ref, ('dx', 'dw0', 'db0', 'dw1')):
        if what == 'db0':
            err = rel_err(got, ref)
            worst_db[0] = max(worst_db[0], err)
            print(f'{name} {act} gain {gain:.3f} clamp {clamp} join {join}: db rel_err {err:.3g} (largest so far {worst_db[0]:.3g})')
            assert err < 1e-4, err
        else:
            assert torch.equal(got, ref), (what, rel_err(got, ref))


def test_masked_launch_refuses_what_it_cannot_apply():
    """The entry point itself refuses a K-sliced launch (the front-end asks pasta_conv2d_mask_available first and runs the pass)."""
    from torch_utils.ops import bias_act, conv2d_gradfix
    name = 'issue_wide_8x32'
    (n, c_z, c_y, groups, h, w, k), _ = CASES[name]
    t = _tensors(name)
    gcfg = conv2d_gradfix._grad_cfg(conv2d_gradfix._Cfg((False, 1, 1, 1, 0, 0, 1, 1.0)), (h, w), (h, w), k, k)
    with pytest.raises(RuntimeError, match='no kernel applies the input-activation mask'):
        conv2d_gradfix._launch_conv(t['gz'], t['w1'], gcfg, epilogue=conv2d_gradfix._act_epilogue(None, conv2d_gradfix._LINEAR_EPILOGUE, None),
                                    mask=(t['gy'], bias_act.act_cfg('relu', None, 1, None)))
