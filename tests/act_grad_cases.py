"""Shared by the tests of the input-activation mask (tests/test_act_grad_*): the planner's answer for a masked launch, a counter of the
stand-alone activation-gradient passes, and the switch of the protocol."""

import contextlib
import ctypes

PLAN_EPILOGUE = 4


def dgrad_plan(n, c_z, c_y, groups, h, w, k):
    """(plan kernel, K slices, does a kernel apply the mask) for the input-gradient launch of a stride-1 k x k convolution c_y -> c_z:
    conv_transpose2d of dz [n, c_z, h, w] onto [n, c_y, h, w], with the linear epilogue every masked launch carries."""
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()
    d = custom_ops.ConvDesc(N=n, C_in=c_z, H=h, W=w, C_out=c_y, OH=h, OW=w, kh=k, kw=k, stride=1, pad_h=k // 2, pad_w=k // 2, groups=groups,
                            transposed=1, flip=0, math=0, wscale=1.0)
    kernel, ksplit = ctypes.c_int(), ctypes.c_int()
    assert lib.pasta_conv2d_plan(ctypes.byref(d), PLAN_EPILOGUE, None, ctypes.byref(ksplit), None, None, ctypes.byref(kernel)) == 0
    return kernel.value, ksplit.value, lib.pasta_conv2d_mask_available(ctypes.byref(d), PLAN_EPILOGUE) == 1


class PassCounter:
    """Counts the launches of the stand-alone first-derivative pass (pasta_bias_act with grad = 1, and its form with the bias sum)."""
    def __init__(self):
        self.passes = 0


@contextlib.contextmanager
def count_passes():
    from torch_utils.ops import bias_act
    c = PassCounter()
    launch, launch_db = bias_act._launch, bias_act._launch_grad_db

    def counted(x, b, xref, yref, dy, grad, *rest):
        c.passes += int(grad == 1)
        return launch(x, b, xref, yref, dy, grad, *rest)

    def counted_db(*args):
        c.passes += 1
        return launch_db(*args)

    bias_act._launch, bias_act._launch_grad_db = counted, counted_db
    try:
        yield c
    finally:
        bias_act._launch, bias_act._launch_grad_db = launch, launch_db


@contextlib.contextmanager
def protocol(on):
    """conv2d_gradfix._ACT_GRAD_IN_WRITER = on inside the block."""
    from torch_utils.ops import conv2d_gradfix
    old, conv2d_gradfix._ACT_GRAD_IN_WRITER = conv2d_gradfix._ACT_GRAD_IN_WRITER, on
    try:
        yield
    finally:
        conv2d_gradfix._ACT_GRAD_IN_WRITER = old
