"""The convolution launches stay inside the workspace they ask for.  One layout function per family (csrc/conv_plan.h: fwd_workspace,
wgrad_workspace) sizes the buffer and forms every pointer into it; here each region of those layouts is reached by a launch whose workspace is
EXACTLY the reported byte count, carved out of the middle of a larger tensor whose flanks (4096 floats on either side, memory this test owns)
hold a fixed bit pattern: the flanks must come back bit-unchanged, and the output must equal, bit for bit, that of the same launch on a
separate, generously sized workspace.

Shapes: the smallest that reach each region under the planner's thresholds (tests/golden/conv_plan_table.npz holds them all); every case first
asserts the kernel it means to reach.  The split kernels want lattices above 8192 pixels, hence the batches of 8 - 10; the pair launch with a
remainder runs in a child process under PASTA_T2_PAIR=2, as in tests/test_conv_pairs_gpu.py, on planes (12 x 64) that the one-pass kernel,
which would take precedence, does not tile."""

import ctypes
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

FLANK = 4096                    # floats
FLANK_BITS = 0x5A5AA5A5
FILL_BITS = 0x7FC0BEEF          # a NaN: whatever a launch reads from the workspace without having written it shows in the output


def _lib():
    from torch_utils.ops import _native
    return _native.lib()


def _desc(transposed, stride, pad, xs, cout, k, math='default'):
    from torch_utils.ops import conv2d_gradfix as cg
    cfg = cg._Cfg((transposed, stride, pad, pad, 0, 0, 1, 1.0))
    oh, ow = cg._out_hw(cfg, xs[2], xs[3], k, k)
    d = cg._desc(cfg, xs, cout, oh, ow, k, k)
    d.math = cg.MATH_CODES[math]
    return cfg, d


def _plan(d, flags=0):
    ks, launches, kernel = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert _lib().pasta_conv2d_plan(ctypes.byref(d), flags, None, ctypes.byref(ks), None, ctypes.byref(launches), ctypes.byref(kernel)) == 0
    return kernel.value, ks.value, launches.value


class Carved:
    """A workspace of exactly ``nbytes`` between two flanks."""

    def __init__(self, nbytes):
        assert nbytes > 0 and nbytes % 16 == 0
        self.n = nbytes // 4
        self.buf = torch.full([FLANK + self.n + FLANK], FILL_BITS, dtype=torch.int32, device='cuda')
        self.buf[:FLANK] = FLANK_BITS
        self.buf[FLANK + self.n:] = FLANK_BITS
        self.ws = self.buf[FLANK:FLANK + self.n]
        self.ptr, self.nbytes = self.ws.data_ptr(), nbytes
        assert self.ptr % 16 == 0

    def assert_flanks(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:FLANK] == FLANK_BITS).all()) and bool((self.buf[FLANK + self.n:] == FLANK_BITS).all()), 'a launch wrote outside its workspace'


class Generous:
    def __init__(self, nbytes):
        self.ws = torch.full([nbytes // 4 + (1 << 18)], FILL_BITS, dtype=torch.int32, device='cuda')
        self.ptr, self.nbytes = self.ws.data_ptr(), self.ws.numel() * 4

    def assert_flanks(self):
        pass


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _check(status):
    assert status == 0, _lib().pasta_last_error().decode(errors='replace')


def _both(nbytes, launch):
    """``launch(workspace) -> tensors`` on the carved workspace and on the generous one: the flanks intact, the results bit-equal."""
    carved = Carved(nbytes)
    got = launch(carved)
    carved.assert_flanks()
    want = launch(Generous(nbytes))
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert not bool(torch.isnan(a).any())
        assert torch.equal(a, b)
    return carved


def _tensors(d, seed, transposed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn([d.N, d.C_in, d.H, d.W], generator=g).cuda()
    ws = [d.C_in, d.C_out, d.kh, d.kw] if transposed else [d.C_out, d.C_in, d.kh, d.kw]
    w = (torch.randn(ws, generator=g) / (d.C_in * d.kh * d.kw) ** 0.5).cuda()
    return g, x, w


def _forward(d, x, w, iscale=None, oscale=None):
    lib = _lib()
    nbytes = lib.pasta_conv2d_workspace(ctypes.byref(d))

    def launch(ws):
        y = torch.empty([d.N, d.C_out, d.OH, d.OW], device='cuda')
        _check(lib.pasta_conv2d_ex(x.data_ptr(), w.data_ptr(), y.data_ptr(), iscale.data_ptr() if iscale is not None else None,
                                   oscale.data_ptr() if oscale is not None else None, None, ctypes.byref(d), ws.ptr, ws.nbytes, _stream()))
        return (y,)
    return _both(nbytes, launch)


# name: (transposed, stride, pad, x shape, C_out, k), expected (kernel, K sliced, launches)
FORWARD = {
    'k_sliced': ((False, 1, 1, (1, 64, 8, 8), 64, 3), (0, True, 1)),                  # partial sums behind the packed weights
    'packed_k_padded_copy': ((False, 1, 3, (1, 3, 96, 96), 64, 7), (8, False, 1)),     # the offset table and the zero-padded input copy
    'one_pass_column': ((True, 2, 0, (8, 16, 32, 32), 64, 3), (13, False, 1)),         # the gathered last column, 32 x 32 -> 65 x 65
}


@pytest.mark.parametrize('name', sorted(FORWARD))
def test_forward_launch_stays_inside_its_workspace(name):
    (transposed, stride, pad, xs, cout, k), (kernel, sliced, launches) = FORWARD[name]
    _, d = _desc(transposed, stride, pad, xs, cout, k)
    got = _plan(d)
    assert (got[0], got[1] > 1, got[2]) == (kernel, sliced, launches)
    _, x, w = _tensors(d, 1, transposed)
    _forward(d, x, w)


def test_input_scale_launch_stays_inside_its_workspace():
    """A modulated convolution as input and output scales: the operand bound of x * iscale is formed in the workspace's leading rows."""
    from torch_utils.ops import conv2d_gradfix as cg
    _, d = _desc(False, 1, 1, (9, 32, 32, 32), 64, 3)
    assert _plan(d, cg.PLAN_ISCALE | cg.PLAN_OSCALE)[0] == 6
    g, x, w = _tensors(d, 2, False)
    iscale = (1 + 0.5 * torch.randn([9, 32], generator=g)).cuda()
    oscale = (1 + 0.5 * torch.randn([9, 64], generator=g)).cuda()
    _forward(d, x, w, iscale, oscale)


def test_prepacked_pair_stays_inside_both_workspaces():
    """pasta_conv2d_pack_pair packs a convolution's weights into the workspaces of the convolution and of its input gradient; both launches then
    run on them with w_prepacked = 1."""
    from torch_utils.ops import conv2d_gradfix as cg
    lib = _lib()
    cfg, da = _desc(False, 1, 1, (9, 32, 32, 32), 64, 3)
    gcfg = cg._grad_cfg(cfg, (32, 32), (32, 32), 3, 3)
    db = cg._desc(gcfg, (9, 64, 32, 32), 32, 32, 32, 3, 3)
    assert _plan(da)[0] == 6 and _plan(db)[0] == 6
    g, x, w = _tensors(da, 3, False)
    dy = torch.randn([9, 64, 32, 32], generator=g).cuda()
    na, nb = lib.pasta_conv2d_workspace(ctypes.byref(da)), lib.pasta_conv2d_workspace(ctypes.byref(db))

    def run(wa, wb, prepacked):
        da.w_prepacked = db.w_prepacked = 0
        if prepacked:
            mask = ctypes.c_int(0)
            _check(lib.pasta_conv2d_pack_pair(w.data_ptr(), ctypes.byref(da), wa.ptr, wa.nbytes, ctypes.byref(db), wb.ptr, wb.nbytes, _stream(), ctypes.byref(mask)))
            assert mask.value == 3
            da.w_prepacked = db.w_prepacked = 1
        y, dx = torch.empty([9, 64, 32, 32], device='cuda'), torch.empty([9, 32, 32, 32], device='cuda')
        _check(lib.pasta_conv2d_ex(x.data_ptr(), w.data_ptr(), y.data_ptr(), None, None, None, ctypes.byref(da), wa.ptr, wa.nbytes, _stream()))
        _check(lib.pasta_conv2d_ex(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), None, None, None, ctypes.byref(db), wb.ptr, wb.nbytes, _stream()))
        torch.cuda.synchronize()
        da.w_prepacked = db.w_prepacked = 0
        return y, dx

    ca, cb = Carved(na), Carved(nb)
    got = run(ca, cb, True)
    ca.assert_flanks()
    cb.assert_flanks()
    for want in (run(Generous(na), Generous(nb), True), run(Generous(na), Generous(nb), False)):
        for a, b in zip(got, want):
            assert not bool(torch.isnan(a).any()) and torch.equal(a, b)


PAIR_SHAPE = (True, 2, 0, (10, 32, 12, 64), 64, 3)         # 12 x 64 -> 25 x 129: remainder row and column


def test_pair_launch_with_remainder_stays_inside_its_workspace():
    """PASTA_T2_PAIR=2 (read once by the planner) sends planes under 128 x 128 with a remainder to the pair launch: a child process."""
    if os.environ.get('PASTA_WORKSPACE_CHILD'):
        _, d = _desc(*PAIR_SHAPE)
        assert _plan(d) == (3, 1, 2)
        _, x, w = _tensors(d, 4, True)
        _forward(d, x, w)
        return
    env = dict(os.environ, PASTA_T2_PAIR='2', PASTA_WORKSPACE_CHILD='1')
    out = subprocess.run([sys.executable, '-m', 'pytest', os.path.abspath(__file__), '-x', '-q', '-k', 'test_pair_launch_with_remainder'],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and '1 passed' in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]


# name: (x shape, C_out), kernel
WGRAD = {'split_3x3': (((2, 32, 32, 32), 32), 2), 'small_cin': (((2, 3, 32, 32), 32), 1)}


@pytest.mark.parametrize('name', sorted(WGRAD))
def test_weight_gradient_stays_inside_its_workspace(name):
    lib = _lib()
    (xs, cout), kernel = WGRAD[name]
    _, d = _desc(False, 1, 1, xs, cout, 3)
    k = ctypes.c_int()
    assert lib.pasta_conv2d_wgrad_plan(ctypes.byref(d), ctypes.byref(k)) == 0 and k.value == kernel
    g, x, _ = _tensors(d, 5, False)
    dy = torch.randn([d.N, d.C_out, d.OH, d.OW], generator=g).cuda()

    def launch(ws):
        dw = torch.empty([d.C_out, d.C_in, 3, 3], device='cuda')
        _check(lib.pasta_conv2d_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ctypes.byref(d), ws.ptr, ws.nbytes, _stream()))
        return (dw,)
    _both(lib.pasta_conv2d_wgrad_workspace(ctypes.byref(d)), launch)


def test_modulated_weight_gradient_stays_inside_its_workspace():
    """... and its partial style gradients are the last region of the workspace: one [N][C_in] block per workgroup row of the reduction
    (64 padded rows in blocks of 4, times 9 taps), which sum_blocks_kernel adds up on four interleaved accumulators."""
    lib = _lib()
    _, d = _desc(False, 1, 1, (2, 32, 32, 32), 32, 3)
    k = ctypes.c_int()
    assert lib.pasta_conv2d_wgrad_plan(ctypes.byref(d), ctypes.byref(k)) == 0 and k.value == 2
    nbytes = lib.pasta_conv2d_wgrad_modulated_workspace(ctypes.byref(d))
    assert nbytes > 0
    g, x, w = _tensors(d, 6, False)
    dy = torch.randn([2, 32, 32, 32], generator=g).cuda()
    styles = (1 + 0.5 * torch.randn([2, 32], generator=g)).cuda()

    def launch(ws):
        dw, ds = torch.empty([32, 32, 3, 3], device='cuda'), torch.empty([2, 32], device='cuda')
        _check(lib.pasta_conv2d_wgrad_modulated(x.data_ptr(), dy.data_ptr(), styles.data_ptr(), w.data_ptr(), dw.data_ptr(), ds.data_ptr(), ctypes.byref(d),
                                                ws.ptr, ws.nbytes, _stream()))
        return dw, ds
    carved = _both(nbytes, launch)
    _, ds = launch(carved)
    torch.cuda.synchronize()
    blocks, n = 64 // 4 * 9, 2 * 32
    part = carved.ws[carved.n - blocks * n:].view(torch.float32).view(blocks, n)
    assert not bool(torch.isnan(part).any())                    # every block was written
    v = [torch.zeros(n, device='cuda') for _ in range(4)]
    for b in range(blocks):
        v[b % 4] = v[b % 4] + part[b]
    assert torch.equal(((v[0] + v[1]) + (v[2] + v[3])).view(2, 32), ds)
