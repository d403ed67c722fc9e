"""Environment switches and the forward planner's flags.  Settled A/B switches are retired: the default is the code.  What stays is a
short list, and this test keeps it short.  No device work is launched here."""

import ctypes
import os
import re

from conftest import ROOT

# the arithmetic; debug aids; tooling; two test-only routing overrides (csrc/conv_igemm.hip, choose_fwd)
KEPT = {'PASTA_CONV_MATH', 'PASTA_CHECK_FINITE', 'PASTA_AMAX_TRACE', 'PASTA_LIB_AB', 'PASTA_BUILD_JOBS', 'PASTA_DIST_BACKEND',
        'PASTA_ROWS2D', 'PASTA_T2_PAIR'}

_READ = re.compile(r'''(?:getenv|environ\.get|environ\[)\s*\(?\s*["'](PASTA_[A-Z0-9_]+)["']''')


def _switches_read():
    files = [os.path.join(ROOT, 'bench.py'), os.path.join(ROOT, '__graft_entry__.py')]
    for top, _, names in os.walk(os.path.join(ROOT, 'pasta-gan_amd')):
        files += [os.path.join(top, n) for n in names if n.endswith(('.py', '.hip', '.h'))]
    found = {}
    for path in files:
        for name in _READ.findall(open(path, encoding='utf-8', errors='replace').read()):
            found.setdefault(name, []).append(os.path.relpath(path, ROOT))
    return found


def test_only_the_kept_switches_are_read():
    found = _switches_read()
    extra = {k: v for k, v in found.items() if k not in KEPT}
    assert not extra, f'environment switches outside the kept list: {extra}'
    assert set(found) == KEPT, f'kept switches no longer read: {sorted(KEPT - set(found))}'


def test_planner_takes_noise_into_account():
    """A pointwise layer with few input channels over more than 8192 pixels runs on conv1x1_fewcin_kernel (plan kernel 11) -- unless its
    epilogue adds noise, which that kernel does not take."""
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()
    header = open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read()
    flag = {n: int(v) for n, v in re.findall(r'#define (PASTA_PLAN_[A-Z]+)\s+(\d+)', header)}
    assert flag['PASTA_PLAN_NOISE'] == 16
    d = custom_ops.ConvDesc(N=1, C_in=8, H=128, W=128, C_out=64, OH=128, OW=128, kh=1, kw=1, stride=1, pad_h=0, pad_w=0, groups=1,
                            transposed=0, flip=0, math=0)
    kernel = ctypes.c_int()
    assert lib.pasta_conv2d_plan(ctypes.byref(d), flag['PASTA_PLAN_EPILOGUE'], None, None, None, None, ctypes.byref(kernel)) == 0
    assert kernel.value == 11
    assert lib.pasta_conv2d_plan(ctypes.byref(d), flag['PASTA_PLAN_EPILOGUE'] | flag['PASTA_PLAN_NOISE'], None, None, None, None,
                                 ctypes.byref(kernel)) == 0
    assert kernel.value != 11
