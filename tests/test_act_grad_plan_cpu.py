"""Where the input-activation mask (include/pasta_hip.h, pasta_act_mask) is served, as the library's own predicates answer -- host only, no
device work: the 2-D tiles of the default arithmetic on fp32 tensors without K slices for the convolutions, the tile and small-plane kernels
on fp32 tensors for the filter."""

import ctypes

from act_grad_cases import PLAN_EPILOGUE, dgrad_plan


def _desc(**kw):
    from torch_utils import custom_ops
    base = dict(N=36, C_in=128, H=8, W=32, C_out=128, OH=8, OW=32, kh=3, kw=3, stride=1, pad_h=1, pad_w=1, groups=1, transposed=1, flip=0, math=0,
                wscale=1.0)
    base.update(kw)
    return custom_ops.ConvDesc(**base)


def test_convolution_predicate():
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()
    assert custom_ops.has_entry(lib, 'pasta_conv2d_masked') and custom_ops.has_entry(lib, 'pasta_bias_sum_db')
    ok = lambda d, flags=PLAN_EPILOGUE: lib.pasta_conv2d_mask_available(ctypes.byref(d), flags)
    assert ok(_desc()) == 1 and ok(_desc(), 0) == 1                      # the eight-wave tile, with and without the residual's epilogue
    assert ok(_desc(C_in=64, C_out=64)) == 1                              # the 64 x 256 tile
    assert ok(_desc(N=1)) == 0                                            # K slices
    assert ok(_desc(io_dtype=3)) == 0 and ok(_desc(io_dtype=1)) == 0      # 16-bit storage
    for math in (1, 2, 3, 4):                                             # the other arithmetics
        assert ok(_desc(math=math)) == 0, math
    assert ok(_desc(N=1, H=100, W=100, OH=100, OW=100, C_out=80)) == 0   # the base kernel
    assert ok(_desc(C_in=32, C_out=16)) == 0                              # the fp32 tile
    assert ok(_desc(), PLAN_EPILOGUE | 1) == 0 and ok(_desc(), PLAN_EPILOGUE | 2) == 0       # scale vectors
    assert ok(_desc(OH=7)) == -1                                          # a descriptor the library refuses
    assert dgrad_plan(36, 128, 128, 1, 8, 32, 3) == (7, 1, True)


def test_filter_predicate():
    from torch_utils import custom_ops
    from torch_utils.ops import _native
    lib = custom_ops.get_plugin()
    ok = lambda dtype, shape, f, *cfg: lib.pasta_upfirdn2d_mask_available(dtype, _native.i32x(*shape), _native.i32x(*f), *cfg)
    blur_t = (1, 1, 1, 1, 1, 1, 1, 1)                                     # the transpose of the blur in front of a stride-2 convolution
    assert ok(0, (2, 6, 33, 33), (4, 4), *blur_t) == 1                    # tile kernel
    assert ok(0, (2, 6, 9, 9), (4, 4), *blur_t) == 1                      # small-plane kernel
    assert ok(0, (1, 2, 40, 40), (5, 5), 1, 1, 1, 1, 2, 2, 2, 2) == 0     # generic kernel
    assert ok(1, (2, 6, 33, 33), (4, 4), *blur_t) == 0 and ok(3, (2, 6, 33, 33), (4, 4), *blur_t) == 0       # 16-bit storage
    assert ok(0, (2, 6, 2, 2), (4, 4), 1, 1, 1, 1, 0, 0, 0, 0) == 0       # no output
