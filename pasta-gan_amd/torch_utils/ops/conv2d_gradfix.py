"""``conv2d`` / ``conv_transpose2d`` on the MI355X implicit-GEMM kernels, with gradients of any order.

Public surface mirrors the reference module torch_utils/ops/conv2d_gradfix.py (``enabled`` :22,
``weight_gradients_disabled`` :23, ``no_weight_gradients`` :25-31, ``conv2d`` :35-38,
``conv_transpose2d`` :40-43). Where the reference forwards to ATen/cuDNN, this module launches
``pasta_conv2d`` / ``pasta_conv2d_wgrad`` (csrc/conv_igemm.hip, fp32 matrix cores). The autograd
structure is the reference's (:107-165): the input gradient is the transposed operator applied
to ``dy``; the weight gradient is its own Function whose backward is again expressed with the
forward operators, so R1's double backward works.
"""

import collections
import contextlib
import ctypes
import operator

import torch

from . import _native
from .. import custom_ops

#----------------------------------------------------------------------------

enabled = True                      # Kept for API compatibility; the HIP path is always used for GPU tensors.
# Matrix-core arithmetic of the convolutions (include/pasta_hip.h PASTA_MATH_*): 'f16x3' (= 'default': fp32-equivalent
# products from three fp16 MFMAs with power-of-two operand scales), 'bf16x6' (fp32-equivalent from six bf16 MFMAs; the default
# until round 3) or 'f32' (fp32 MFMA, bit-exact fp32 FMA chains); 'bf16x3' / 'bf16' are opt-in reduced modes.  Overridable
# with PASTA_CONV_MATH.
import os as _os
MATH_CODES = {'default': 0, 'f32': 1, 'bf16x6': 2, 'bf16x3': 3, 'bf16': 4, 'f16x3': 5}
conv_math = _os.environ.get('PASTA_CONV_MATH', 'default')
assert conv_math in MATH_CODES, f'PASTA_CONV_MATH must be one of {sorted(MATH_CODES)}'
weight_gradients_disabled = False   # Forcefully disable computation of gradients with respect to the weights.

@contextlib.contextmanager
def no_weight_gradients():
    """Skip weight gradients inside the block (used around R1 / path-length ``autograd.grad``)."""
    global weight_gradients_disabled
    old = weight_gradients_disabled
    weight_gradients_disabled = True
    try:
        yield
    finally:
        weight_gradients_disabled = old

#----------------------------------------------------------------------------

def _pair(v):
    v = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    assert len(v) == 2 and all(isinstance(e, int) for e in v)
    return v

class _Cfg(tuple):
    """(transposed, stride, pad_h, pad_w, outpad_h, outpad_w, groups[, wgain]) -- hashable op configuration.
    ``wgain``: the weights enter every launch of the family as ``w * wgain`` (folded into the weight packing, and
    into the weight gradient's reduction), so a layer's ``self.weight * self.weight_gain`` needs no kernel of its own."""
    __slots__ = ()
    wgain = property(lambda s: s[7] if len(s) > 7 else 1.0)
    transposed = property(lambda s: s[0]); stride = property(lambda s: s[1])
    pad_h = property(lambda s: s[2]); pad_w = property(lambda s: s[3])
    outpad_h = property(lambda s: s[4]); outpad_w = property(lambda s: s[5]); groups = property(lambda s: s[6])

def _out_hw(cfg, h, w, kh, kw):
    if cfg.transposed:
        return ((h - 1) * cfg.stride - 2 * cfg.pad_h + kh + cfg.outpad_h,
                (w - 1) * cfg.stride - 2 * cfg.pad_w + kw + cfg.outpad_w)
    return ((h + 2 * cfg.pad_h - kh) // cfg.stride + 1, (w + 2 * cfg.pad_w - kw) // cfg.stride + 1)

IO_CODES = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 3}      # pasta_conv_desc.io_dtype (PASTA_F32 / _F16 / _BF16)

def _desc(cfg, x_shape, c_out, oh, ow, kh, kw, io=torch.float32):
    n, c_in, h, w = x_shape
    return custom_ops.ConvDesc(N=n, C_in=c_in, H=h, W=w, C_out=c_out, OH=oh, OW=ow, kh=kh, kw=kw, stride=cfg.stride,
                               pad_h=cfg.pad_h, pad_w=cfg.pad_w, groups=cfg.groups, transposed=int(cfg.transposed), flip=0,
                               math=MATH_CODES[conv_math], wscale=float(cfg.wgain), io_dtype=IO_CODES[io])

# The planners (include/pasta_hip.h): pasta_conv2d_plan / pasta_conv2d_wgrad_plan name the kernel a descriptor gets, and whether one exists --
# 16-bit storage (fp16 / bf16 tensors in HBM, one matrix-core product per multiply-add, fp32 accumulation; pasta_conv_desc.io_dtype) exists for
# the shapes the matrix-core kernel family covers, everything else -- the few-channel stems and heads -- is converted to fp32 for that launch
# and back.  ``_plan`` is the one place that asks them.
PLAN_ISCALE, PLAN_OSCALE, PLAN_EPILOGUE, PLAN_MODULATED, PLAN_NOISE = 1, 2, 4, 8, 16      # PASTA_PLAN_*: what a forward launch passes besides x, w
_Plan = collections.namedtuple('_Plan', 'ok kernel math workspace')
_DESC_PTRS = ('x_amax', 'x2', 'x2_amax', 'dy_amax')
_desc_values = operator.attrgetter(*(f for f, _ in custom_ops.ConvDesc._fields_ if f not in _DESC_PTRS))
_desc_ptrs = operator.attrgetter(*_DESC_PTRS)

def _desc_key(desc):
    """Every field of ``desc`` as the planners see it: the pointers as null / non-null."""
    a, b, c, d = _desc_ptrs(desc)
    return _desc_values(desc) + (a is not None, b is not None, c is not None, d is not None)

_plan_cache = {}

def _plan(kind, desc, flags=0):
    """The planner's answer for ``desc``, memoised: (accepted, kernel id, math actually used, workspace bytes).  ``kind`` 'conv' asks
    pasta_conv2d_plan with the launch's PLAN_* ``flags``; 'wgrad' pasta_conv2d_wgrad_plan (no math); 'wgrad_modulated' the sample-aligned weight
    gradient, which exists where its workspace query answers (no kernel, no math).  kernel and math are None where the planner refuses."""
    key = (kind, flags, _desc_key(desc))
    hit = _plan_cache.get(key)
    if hit is None:
        lib, d = _native.lib(), ctypes.byref(desc)
        kernel, math = ctypes.c_int(), ctypes.c_int()
        if kind == 'conv':
            ok = lib.pasta_conv2d_plan(d, int(flags), None, None, ctypes.byref(math), None, ctypes.byref(kernel)) == 0
            hit = _Plan(ok, kernel.value, math.value, lib.pasta_conv2d_workspace(d))
        elif kind == 'wgrad':
            ok = lib.pasta_conv2d_wgrad_plan(d, ctypes.byref(kernel)) == 0
            hit = _Plan(ok, kernel.value, None, lib.pasta_conv2d_wgrad_workspace(d))
        else:
            nbytes = lib.pasta_conv2d_wgrad_modulated_workspace(d)
            hit = _Plan(nbytes >= 0, None, None, nbytes)
        if not hit.ok:
            hit = hit._replace(kernel=None, math=None)
        _plan_cache[key] = hit
    return hit

def _native16(kind, desc, has_iscale=False):
    """Does a 16-bit-storage kernel take ``desc`` (io_dtype fp16 / bf16)?"""
    return _plan(kind, desc, PLAN_ISCALE if has_iscale else 0).ok

# PASTA_MATH_F16X3 (include/pasta_hip.h): the power-of-two operand scales of the ACTIVATIONS come from the tensors' largest
# magnitudes (the weights are scaled per output row by their packing kernel at every launch: nothing about a weight is cached).
# A tensor is scanned by ``pasta_tensor_amax`` (256 partial maxima, one pass at HBM rate) or arrives with the maxima its
# producer kernel left behind (_native.amax_attach), and the result travels with the Python tensor object while its version
# stands: a forward input serves the forward launch and, from the saved tensor, the weight gradient; a gradient serves the
# input-gradient and the weight-gradient launch of the same backward.
#
# What may be cached (round 4): the key (t._version, t.data_ptr()) cannot see a write that goes
# around the version counter (``t.data.mul_()``, numpy / DLPack aliases).  The tensors such idioms are applied to are LEAVES a
# caller holds: parameters (no longer scanned at all) and input batches.  So a scan result is attached only to
#   * tensors with a ``grad_fn`` (results of recorded operations: only autograd-visible code writes them), and
#   * tensors met inside a backward pass (gradients, saved activations being differentiated),
# and a leaf met outside a backward pass -- an input batch, a parameter used as an activation, a no-grad intermediate of a
# torch operator -- is scanned at every use (its maxima are never read from the object: ``tensor_amax`` applies the same predicate
# when it READS a scan result, so a result attached to a leaf inside a backward pass is not found by a later forward).  Producer rows are written by the
# kernel that wrote the tensor and are trusted for that version.  Inference tensors (``torch.inference_mode()``) track no
# version: nothing is cached on them or read back from them.
AMAX_PARTS = 256
_SCAN_TRACE = {} if _os.environ.get('PASTA_AMAX_TRACE') else None
if _SCAN_TRACE is not None:
    import atexit as _atexit
    def _dump_scans():
        import sys
        rows = sorted(_SCAN_TRACE.items(), key=lambda kv: -kv[1] * max(1, int(torch.Size(kv[0][0]).numel())))
        for (shape, src), n in rows[:60]:
            print(f'amax scan x{n:5d}  {str(shape):22s} {src}', file=sys.stderr)
    _atexit.register(_dump_scans)

# PASTA_CHECK_FINITE=1 (debug; synchronises): every convolution under the three-product arithmetic checks its output for
# inf / NaN and raises -- what an operand scale taken from stale maxima (|v S| > 65504) or a non-finite operand produces.
_CHECK_FINITE = _os.environ.get('PASTA_CHECK_FINITE', '0') == '1'

_graph_task_id = getattr(torch._C, '_current_graph_task_id', None)

def _in_backward():
    return _graph_task_id is not None and _graph_task_id() != -1

def _amax_cacheable(t):
    """May a scan of ``t`` be attached to the tensor object (see the note above)?"""
    if t.is_inference():
        return False
    return t.grad_fn is not None or _in_backward()

def tensor_amax(t):
    """[256] partial |max| of a contiguous fp32 GPU tensor; cached on the tensor only where no write can bypass the key."""
    hit = None if t.is_inference() else getattr(t, '_pasta_amax', None)
    # the read side applies the rule of the write side: a SCAN result found on a leaf outside a backward pass is not trusted --
    # it may have been attached while the leaf was met inside one (an image batch whose forward ran a kernel that takes no maxima, scanned by
    # the weight gradient), and a `.data` write since then is invisible to the key.  Producer rows (hit[3]) stand for their version.
    if hit is not None and hit[0] == t._version and hit[1] == t.data_ptr() and (len(hit) > 3 or _amax_cacheable(t)):
        return hit[2]
    if _SCAN_TRACE is not None:                        # diagnostic (PASTA_AMAX_TRACE=1): which tensors still cost a scan
        import sys as _sys
        fr, chain = _sys._getframe(1), []
        while fr is not None and len(chain) < 8:           # the callers inside this package, innermost first
            if 'pasta-gan_amd' in fr.f_code.co_filename and fr.f_code.co_name not in ('apply', '_call_impl', '_wrapped_call_impl'):
                chain.append(f'{fr.f_code.co_name}:{fr.f_lineno}')
            fr = fr.f_back
        key = (tuple(t.shape), (type(t.grad_fn).__name__ if t.grad_fn is not None else ('param' if t.requires_grad else 'plain'))
               + ' <- ' + ' <- '.join(chain) + (' [stale attr]' if hit is not None else ''))
        _SCAN_TRACE[key] = _SCAN_TRACE.get(key, 0) + 1
    parts = torch.empty([AMAX_PARTS], dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        _native.check(_native.lib().pasta_tensor_amax(_native.ptr(t), t.numel(), 0, _native.ptr(parts), _native.stream()))
    if _amax_cacheable(t):
        try:
            t._pasta_amax = (t._version, t.data_ptr(), parts)
        except AttributeError:
            pass
    return parts

def _check_finite(y, what):
    if _CHECK_FINITE and not bool(torch.isfinite(y).all()):
        raise RuntimeError(f'{what}: non-finite output under PASTA_MATH_F16X3 -- a non-finite operand, or an operand scale taken '
                           f'from maxima that no longer describe the tensor (written behind the version counter?)')

def _runs_f16x3(kind, desc, flags=0):
    """Does this launch run the three-product fp16 arithmetic (then it wants the operands' partial maxima)?"""
    if desc.math not in (0, MATH_CODES['f16x3']) or desc.io_dtype != 0:
        return False
    p = _plan(kind, desc, flags)
    return p.math == MATH_CODES['f16x3'] if kind == 'conv' else p.kernel in (custom_ops.WGRAD_3X3, custom_ops.WGRAD_3X3S2, custom_ops.WGRAD_1X1)

# Optional measurement hook (bench.py): when set, called as hook(kind, desc, launch, flags) around every native
# convolution launch; ``launch()`` performs it. None = no overhead.
launch_hook = None

def _f32(t):
    return t if t.dtype == torch.float32 else t.float()

def _workspace(nbytes, device):
    """The workspace of a launch (``_plan(...).workspace``; negative for a descriptor the library refuses: the launch then says why)."""
    return torch.empty([max(nbytes // 4, 4)], dtype=torch.float32, device=device)

def _issue(kind, flags, entry, args, desc, work, device):
    """``entry(*args, desc, workspace, bytes, stream)`` -- the tail every convolution entry point shares --, through ``launch_hook`` when set.
    ``kind`` ('conv', 'conv_isc' = with an input scale, 'wgrad') and ``flags`` (PLAN_*) are what the hook is told."""
    def launch():
        with torch.cuda.device(device):
            _native.check(entry(*args, ctypes.byref(desc), _native.ptr(work), work.numel() * 4, _native.stream()))
    if launch_hook is None:
        launch()
    else:
        launch_hook(kind, desc, launch, flags)

def _epilogue(epilogue, noise, y):
    """The ``pasta_conv_epilogue`` of a launch onto ``y`` -> (ConvEpilogue, the producer row of y's maxima or None, the tensors it points to)."""
    bias, act_code, alpha, gain, clamp = epilogue[:5]
    res = epilogue[5] if len(epilogue) > 5 else None
    bias = _f32(bias).contiguous() if bias is not None else None
    if res is not None:
        res = res.to(y.dtype).contiguous()
        if res.shape != y.shape:
            raise RuntimeError(f'conv2d: residual {tuple(res.shape)} does not match the output {tuple(y.shape)}')
    nz = nstr = None
    if noise is not None:
        nz, nstr = _f32(noise[0]).contiguous(), _f32(noise[1]).reshape(1).contiguous()
        n, _, oh, ow = y.shape
        if nz.numel() not in (oh * ow, n * oh * ow):
            raise RuntimeError(f'conv2d: noise {tuple(nz.shape)} is neither one {oh}x{ow} plane nor one per sample')
    ep = custom_ops.ConvEpilogue(bias=bias.data_ptr() if bias is not None else None, act=int(act_code), alpha=float(alpha),
                                 gain=float(gain), clamp=float(clamp), res=res.data_ptr() if res is not None else None,
                                 noise=nz.data_ptr() if nz is not None else None, noise_strength=nstr.data_ptr() if nz is not None else None,
                                 noise_per_sample=int(nz is not None and nz.numel() != y.shape[2] * y.shape[3]))
    y_row = _native.amax_slot(y)            # the layer's output usually feeds the next convolution
    if y_row is not None:
        ep.y_amax = y_row.data_ptr()
    return ep, y_row, (bias, res, nz, nstr)

def _launch_conv(x, w, cfg, iscale=None, oscale=None, epilogue=None, wmod=None, noise=None, x2=None, used=None, pieces=None, prepacked=None, mask=None):
    """y = conv(x * iscale[n,c]) * oscale[n,c'] through ``pasta_conv2d_ex``; fp32 accumulation.  fp32 tensors run the
    split-bf16 (fp32-equivalent) or fp32 matrix-core kernels; fp16 / bf16 tensors stay 16-bit in HBM where a kernel exists
    (``_native16``) and are converted for the launch otherwise.
    ``epilogue`` = (bias or None, act code 1..3, alpha, gain, clamp[, residual or None]) fuses Conv2dLayer's bias_act into the
    store; the residual ([N, C_out, OH, OW]) is added to the convolution before the bias.
    ``noise`` = (plane(s) [OH, OW] or [N, 1, OH, OW] fp32, strength scalar tensor): added after ``oscale`` (needs ``epilogue``).
    ``wmod`` = (styles [G, I], dcoefs [G, O] or None): ``w`` is ONE group's weight shared by all ``cfg.groups`` groups and
    modulated per group by the packing kernel (``pasta_conv2d_modulated``).
    ``x2`` ([N, C2, H, W], pointwise convolutions only -- ``cat1x1_available``): the convolution runs over the channel concatenation
    ``cat([x, x2], 1)`` without forming it (``pasta_conv_desc.x2``).
    ``used`` (dict, optional): receives ``'x_amax'`` / ``'x2_amax'`` = the partial maxima the launch took for its activations, so that the
    autograd node can hand them to the weight gradient of the SAME saved tensor (a saved non-leaf tensor comes back from autograd as a new
    Python object without the attribute the maxima travel on: it would be scanned a second time).
    ``pieces`` = (bound row [256], logical shape (N, C, H, W)): ``x`` is not an NCHW tensor but the producer-written operand of the three-product
    arithmetic (``blur_pieces``: PASTA_LAYOUT_PIECES16, include/pasta_hip.h) -- the launch copies its sixteen-byte pieces instead of splitting.
    ``prepacked`` = (descriptor key, workspace) from ``_pack_pair``: the weights packed for the descriptor of that key; a launch of that very
    descriptor runs on it without a packing kernel, any other packs for itself.
    ``mask`` = (m, (act, alpha, gain, clamp)): the input-activation mask of an input-gradient launch (``pasta_conv2d_masked``; ``_mask_launch_ok``
    says where a kernel applies it) -- the store multiplies by the derivative of the activation that produced ``m`` (shape of the output)."""
    _native.require_gpu(x, 'conv2d')
    if pieces is not None:
        assert iscale is None and oscale is None and wmod is None and noise is None and x2 is None
        bound, x_shape = pieces
        out_dtype = torch.float32
    else:
        if x.ndim != 4 or w.ndim != 4:
            raise RuntimeError('conv2d: x and w must be rank 4')
        x_shape, out_dtype = tuple(x.shape), x.dtype
    n, h, wd = x_shape[0], x_shape[2], x_shape[3]
    w = _f32(w).contiguous()
    kh, kw = w.shape[2], w.shape[3]
    shared = cfg.groups if wmod is not None else 1        # the weight tensor holds one group
    c_in = x_shape[1] + (x2.shape[1] if x2 is not None else 0)
    if cfg.transposed:
        if w.shape[0] * shared != c_in:
            raise RuntimeError(f'conv_transpose2d: weight {tuple(w.shape)} does not match input channels {c_in}')
        c_out = w.shape[1] * cfg.groups
    else:
        if w.shape[1] * cfg.groups != c_in:
            raise RuntimeError(f'conv2d: weight {tuple(w.shape)} does not match input channels {c_in} (groups={cfg.groups})')
        c_out = w.shape[0] * shared
    oh, ow = _out_hw(cfg, h, wd, kh, kw)
    if oh < 1 or ow < 1:
        raise RuntimeError('conv2d: output must be at least 1x1')
    if x.numel() == 0 or c_out * oh * ow == 0:
        return torch.zeros([n, c_out, oh, ow], dtype=out_dtype, device=x.device)
    if noise is not None and epilogue is None:
        raise RuntimeError('conv2d: the noise operand is part of the fused epilogue')
    # the launch's PASTA_PLAN_* flags, as the library derives them from what it is passed (the kernel it runs depends on them)
    flags = ((PLAN_ISCALE if iscale is not None else 0) | (PLAN_OSCALE if oscale is not None else 0) | (PLAN_EPILOGUE if epilogue is not None else 0)
             | (PLAN_MODULATED if wmod is not None else 0) | (PLAN_NOISE if noise is not None else 0))
    io = torch.float32
    if x.dtype in (torch.float16, torch.bfloat16) and _native16('conv', _desc(cfg, x_shape, c_out, oh, ow, kh, kw, x.dtype), iscale is not None):
        io = x.dtype
    if pieces is None:
        x = x.contiguous() if io is not torch.float32 else _f32(x).contiguous()
    y = torch.empty([n, c_out, oh, ow], dtype=io, device=x.device)
    desc = _desc(cfg, (n, c_in, h, wd), c_out, oh, ow, kh, kw, io)
    if x2 is not None:
        if io is not torch.float32 or x2.dtype != torch.float32 or x2.shape[0] != n or x2.shape[2:] != x.shape[2:]:
            raise RuntimeError('conv2d: the second input tensor must be fp32 and match the first in batch and plane size')
        x2 = x2.contiguous()
        desc.x2, desc.C1 = x2.data_ptr(), int(x.shape[1])
    if pieces is not None:
        desc.x_layout, desc.x_amax = 1, bound.data_ptr()
    f16x3 = pieces is not None or _runs_f16x3('conv', desc, flags)
    if prepacked is not None and prepacked[0] == _desc_key(desc):
        assert iscale is None and oscale is None and wmod is None
        work = prepacked[1]
        desc.w_prepacked = 1
    else:
        work = _workspace(_plan('conv', desc, flags).workspace, x.device)
    if iscale is not None:
        iscale = _f32(iscale).contiguous()
        assert iscale.shape == (n, x_shape[1])
    if oscale is not None:
        oscale = _f32(oscale).contiguous()
        assert oscale.shape == (n, c_out)
    ep = y_row = None
    if epilogue is not None:
        ep, y_row, ep_tensors = _epilogue(epilogue, noise, y)        # (ep_tensors: what ep points to, held until the launch is issued)
    x_amax = x2_amax = None
    if f16x3 and pieces is None:
        x_amax = tensor_amax(x)                 # the weights are scaled per output row by their packing kernel: nothing to pass
        desc.x_amax = x_amax.data_ptr()
        if x2 is not None:
            x2_amax = tensor_amax(x2)
            desc.x2_amax = x2_amax.data_ptr()
        if used is not None:
            used['x_amax'], used['x2_amax'] = x_amax, x2_amax
    ep_ref = ctypes.byref(ep) if ep is not None else None
    lib = _native.lib()
    if mask is not None:
        from . import bias_act as ba
        assert iscale is None and oscale is None and wmod is None and noise is None and io is torch.float32
        m, (m_act, m_alpha, m_gain, m_clamp) = mask
        if m.dtype != torch.float32 or tuple(m.shape) != tuple(y.shape):
            raise RuntimeError(f'conv2d: the input-activation mask {tuple(m.shape)} {m.dtype} does not match the fp32 output {tuple(y.shape)}')
        m = m.contiguous()
        am = custom_ops.ActMask(m=m.data_ptr(), act=int(ba.activation_funcs[m_act].cuda_idx), alpha=float(m_alpha), gain=float(m_gain), clamp=float(m_clamp))
        args = (_native.ptr(x), _native.ptr(w), _native.ptr(y), None, None, ep_ref, ctypes.byref(am))
        _issue('conv', flags, lib.pasta_conv2d_masked, args, desc, work, x.device)
    elif wmod is not None:
        assert iscale is None and oscale is None
        mod_s = _f32(wmod[0]).contiguous()
        mod_d = _f32(wmod[1]).contiguous() if wmod[1] is not None else None
        assert mod_s.numel() == x.shape[1] and (mod_d is None or mod_d.numel() == c_out)
        args = (_native.ptr(x), _native.ptr(w), _native.ptr(mod_s), _native.ptr(mod_d), _native.ptr(y), ep_ref)
        _issue('conv', flags, lib.pasta_conv2d_modulated, args, desc, work, x.device)
    else:
        args = (_native.ptr(x), _native.ptr(w), _native.ptr(y), _native.ptr(iscale), _native.ptr(oscale), ep_ref)
        _issue('conv' if iscale is None else 'conv_isc', flags, lib.pasta_conv2d_ex, args, desc, work, x.device)
    if f16x3:
        _check_finite(y, 'conv2d')
    if y_row is not None and y.dtype == out_dtype:
        _native.amax_attach(y, y_row)
    return y.to(out_dtype)

# ---- producer-written operand pieces (round 5; csrc/pieces.hip, include/pasta_hip.h "Producer-written operand pieces") --------------------
# The low-pass in front of a stride-2 convolution (reference conv2d_resample.py:119-122) has ONE reader besides that convolution's weight
# gradient, and its magnitude is bounded by its input's: it can write its output once as the fp16 pieces h | l' of the three-product
# arithmetic (16-byte units of eight channels, [N][C / 8][H][piece][W]), and both consumers copy pieces instead of fetching fp32 with eight
# channel-strided loads per unit and splitting it -- in every launch that touches the tensor.
_PIECES = True       # False: the blurred tensor in fp32, as the reference (tests compare the two)

def pieces_available(x, f, weight, pad4, groups=1):
    """Can ``conv2d(upfirdn2d(x, f, padding=pad4), weight, stride=2)`` run on the blurred tensor as producer-written pieces (forward kernel 10 and
    weight-gradient kernel 6 of the planners)?  fp32 tensors, the default arithmetic, a 4 x 4 filter, whole channel octets."""
    if not (_PIECES and x.device.type == 'cuda' and x.dtype == torch.float32 and weight.dtype == torch.float32 and conv_math in ('default', 'f16x3')
            and groups == 1 and f is not None and f.ndim == 2 and tuple(f.shape) == (4, 4) and x.ndim == 4 and x.shape[1] % 8 == 0
            and tuple(weight.shape[2:]) == (3, 3) and weight.shape[1] == x.shape[1] and x.numel() > 0):
        return False
    px0, px1, py0, py1 = pad4
    n, c, h, wd = (int(v) for v in x.shape)
    bh, bw = h + py0 + py1 - 3, wd + px0 + px1 - 3
    if bh < 3 or bw < 3:
        return False
    cfg = _Cfg((False, 2, 0, 0, 0, 0, 1, 1.0))
    oh, ow = _out_hw(cfg, bh, bw, 3, 3)
    desc = _desc(cfg, (n, c, bh, bw), int(weight.shape[0]), oh, ow, 3, 3)
    desc.x_layout = 1
    return _plan('conv', desc, PLAN_EPILOGUE).kernel == custom_ops.FWD_3X3S2 and _plan('wgrad', desc).kernel == custom_ops.WGRAD_3X3S2_PIECES

def blur_pieces(x, f, pad4, flip_filter=False, gain=1.0, x_amax=None):
    """``upfirdn2d(x, f, padding=pad4, flip_filter, gain)`` for a 4 x 4 filter, written as PASTA_LAYOUT_PIECES16.  Returns (pieces -- a uint8
    tensor of N * C / 8 * OH * OW * 32 bytes --, bound row [256] fp32, logical shape (N, C, OH, OW)); the bound row is ``x_amax`` (the partial
    maxima of x: its producer's row, or one scan) times gain * sum |f| and fixes the operand's power-of-two scale on both sides."""
    _native.require_gpu(x, 'blur_pieces')
    x = x.contiguous()
    n, c, h, wd = (int(v) for v in x.shape)
    px0, px1, py0, py1 = pad4
    oh, ow = h + py0 + py1 - 3, wd + px0 + px1 - 3
    lib = _native.lib()
    nbytes = lib.pasta_pieces_bytes(n, c, oh, ow)
    if nbytes < 0 or oh < 1 or ow < 1:
        raise RuntimeError(f'blur_pieces: {tuple(x.shape)} -> {oh} x {ow}: the channel count must be a multiple of 8 and the output at least 1 x 1')
    parts = tensor_amax(x) if x_amax is None else x_amax
    pieces = torch.empty([nbytes], dtype=torch.uint8, device=x.device)
    bound = torch.empty([AMAX_PARTS], dtype=torch.float32, device=x.device)
    f = f.contiguous()
    def launch():
        with torch.cuda.device(x.device):
            _native.check(lib.pasta_blur_pieces(_native.ptr(x), _native.ptr(f), _native.ptr(pieces), _native.ptr(parts), _native.ptr(bound), n, c, h, wd,
                                                int(px0), int(px1), int(py0), int(py1), int(bool(flip_filter)), float(gain), _native.stream()))
    from . import upfirdn2d as _up
    if _up.launch_hook is None:
        launch()
    else:       # algorithmic bytes: fp32 in, 4 bytes per element out (two fp16 pieces)
        _up.launch_hook((x.numel() + n * c * oh * ow) * 4, (tuple(x.shape), 1, 1, 4, 'pieces'), launch)
    return pieces, bound, (n, c, oh, ow)

def pieces_pack(x, x_amax=None):
    """An fp32 NCHW tensor as PASTA_LAYOUT_PIECES16, split exactly as the consuming kernels split it in their staging (``pasta_pieces_pack``).
    Returns (pieces, bound row, shape) like ``blur_pieces``; the bound row is x's own partial maxima."""
    _native.require_gpu(x, 'pieces_pack')
    x = x.float().contiguous()
    n, c, h, wd = (int(v) for v in x.shape)
    lib = _native.lib()
    nbytes = lib.pasta_pieces_bytes(n, c, h, wd)
    if nbytes < 0:
        raise RuntimeError(f'pieces_pack: {tuple(x.shape)}: the channel count must be a multiple of 8')
    parts = tensor_amax(x) if x_amax is None else x_amax
    pieces = torch.empty([nbytes], dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _native.check(lib.pasta_pieces_pack(_native.ptr(x), _native.ptr(parts), _native.ptr(pieces), n, c, h, wd, _native.stream()))
    return pieces, parts, (n, c, h, wd)

# ---- one operand, several 3x3 layers (round 5): a tensor that several stride-1 3x3 convolutions read (the SPADE feature map: three
# conv_mlp batches per generator pass, networks.py Spade_ResBlockV2) is packed ONCE and every forward launch copies the pieces (plan kernel 7
# with x_layout = PASTA_LAYOUT_PIECES16: +10 % on 256 -> 384 at 128 x 128, profiles/r5_s1_pieces_microbench.txt).  The pieces ride on the tensor
# object, keyed by version and address like the maxima rows; the weight gradients keep reading the fp32 tensor.

def _shared_pieces_ok(x, weight, cfg, has_epilogue):
    """Does the eight-wave stride-1 tile kernel take conv2d(x, weight) with x as pieces?"""
    if not (_PIECES and x.device.type == 'cuda' and x.dtype == torch.float32 and weight.dtype == torch.float32
            and conv_math in ('default', 'f16x3') and cfg.groups == 1 and cfg.stride == 1 and not cfg.transposed
            and tuple(weight.shape[2:]) == (3, 3) and x.ndim == 4 and x.shape[1] % 8 == 0):
        return False
    n, c, h, wd = (int(v) for v in x.shape)
    oh, ow = _out_hw(cfg, h, wd, 3, 3)
    desc = _desc(cfg, (n, c, h, wd), int(weight.shape[0]), oh, ow, 3, 3)
    desc.x_layout = 1
    return _plan('conv', desc, PLAN_EPILOGUE if has_epilogue else 0).kernel == custom_ops.FWD_ROWS2D_WIDE

def share_pieces(x):
    """Pack ``x`` for the stride-1 3x3 layers that will read it (a no-op where none of them could use the pieces); returns ``x``."""
    if (_PIECES and x.device.type == 'cuda' and x.dtype == torch.float32 and x.ndim == 4 and x.shape[1] % 8 == 0 and x.shape[1] >= 16
            and conv_math in ('default', 'f16x3') and not x.is_inference() and x.is_contiguous()
            and not torch.cuda.is_current_stream_capturing() and _shared_lookup(x) is None):
        pieces, bound, shape = pieces_pack(x)
        try:
            x._pasta_pieces = (x._version, x.data_ptr(), pieces, bound, shape)
        except AttributeError:
            pass
    return x

def _shared_lookup(x):
    hit = getattr(x, '_pasta_pieces', None)
    if hit is not None and hit[0] == x._version and hit[1] == x.data_ptr():
        return hit
    return None

def pieces_unpack(pieces, bound, shape):
    """(h + 2^-11 l') / S as an fp32 NCHW tensor (tests, diagnostics): the 22 bits the consumers multiply."""
    n, c, h, wd = shape
    y = torch.empty([n, c, h, wd], dtype=torch.float32, device=pieces.device)
    with torch.cuda.device(pieces.device):
        _native.check(_native.lib().pasta_pieces_unpack(_native.ptr(pieces), _native.ptr(bound), _native.ptr(y), n, c, h, wd, _native.stream()))
    return y

def _launch_wgrad(x, dy, cfg, w_shape, out_dtype=None, x_amax=None, pieces=None):
    """dw of ``conv(x, w)`` given dy through ``pasta_conv2d_wgrad``; the gradient comes out fp32 (weights are fp32 masters)
    and is returned as ``out_dtype`` (default: dy's).  ``pieces`` = (bound row, logical shape) as for ``_launch_conv``: x is a
    producer-written operand (``blur_pieces``; pasta_conv2d_wgrad_plan kernel 6)."""
    _native.require_gpu(x, 'conv2d_wgrad')
    out_dtype = dy.dtype if out_dtype is None else out_dtype
    kh, kw = w_shape[2], w_shape[3]
    dw = torch.empty(list(w_shape), dtype=torch.float32, device=x.device)
    if dw.numel() == 0:
        return dw.to(out_dtype)
    if x.numel() == 0 or dy.numel() == 0:
        return dw.zero_().to(out_dtype)
    io = torch.float32
    if pieces is not None:
        x_amax, x_shape = pieces
    else:
        x_shape = tuple(x.shape)
        if x.dtype == dy.dtype and x.dtype in (torch.float16, torch.bfloat16) and \
                _native16('wgrad', _desc(cfg, x_shape, dy.shape[1], dy.shape[2], dy.shape[3], kh, kw, x.dtype)):
            io = x.dtype
        x = x.contiguous() if io is not torch.float32 else _f32(x).contiguous()
    dy = dy.contiguous() if io is not torch.float32 else _f32(dy).contiguous()
    desc = _desc(cfg, x_shape, dy.shape[1], dy.shape[2], dy.shape[3], kh, kw, io)
    if pieces is not None:
        desc.x_layout = 1
    f16x3 = pieces is not None or _runs_f16x3('wgrad', desc)
    _wgrad_issue('wgrad', desc, x, dy, x_amax, f16x3, _native.lib().pasta_conv2d_wgrad, (x, dy, dw), dw)
    return dw.to(out_dtype)

def _wgrad_issue(kind, desc, x, dy, x_amax, f16x3, entry, tensors, dw):
    """What every weight-gradient launch does around its entry point: workspace, the operands' maxima under the three-product arithmetic
    (``x_amax``: the maxima the forward launch took for this very tensor -- autograd has checked that it was not written since -- or the
    pieces' bound row), the launch, the finite check."""
    work = _workspace(_plan(kind, desc).workspace, dy.device)
    if f16x3:
        amax_x, amax_dy = (x_amax if x_amax is not None else tensor_amax(x)), tensor_amax(dy)
        desc.x_amax, desc.dy_amax = amax_x.data_ptr(), amax_dy.data_ptr()
    _issue('wgrad', 0, entry, tuple(_native.ptr(t) for t in tensors), desc, work, dy.device)
    if f16x3:
        _check_finite(dw, 'conv2d_wgrad')

#----------------------------------------------------------------------------

def _grad_cfg(cfg, x_hw, y_hw, kh, kw):
    """Configuration of the operator that maps dy back to dx (reference :95-104, :125-128)."""
    if cfg.transposed:
        return _Cfg((False, cfg.stride, cfg.pad_h, cfg.pad_w, 0, 0, cfg.groups, cfg.wgain))
    oph = x_hw[0] - ((y_hw[0] - 1) * cfg.stride - 2 * cfg.pad_h + kh)
    opw = x_hw[1] - ((y_hw[1] - 1) * cfg.stride - 2 * cfg.pad_w + kw)
    return _Cfg((True, cfg.stride, cfg.pad_h, cfg.pad_w, oph, opw, cfg.groups, cfg.wgain))

# ---- one packing launch for a convolution and its input gradient (round 5; include/pasta_hip.h, pasta_conv2d_pack_pair) -------------------
# Every forward convolution whose input needs a gradient is followed, in the backward pass, by the same weights packed the other way round
# (transposed and mirrored): 120 of the 310 packing launches of a training step.  The forward packs BOTH orientations with one kernel and the
# autograd node carries the second workspace to its backward.
_PACK_PAIR = True       # False: every launch packs for itself (tests compare the two)

def _pack_pair(x, w, cfg):
    """-> the forward launch's and its input-gradient launch's (descriptor key, workspace) with the weights packed in it, or (None, None).  The
    input-gradient launch takes its workspace only if its own descriptor has that key (the arithmetic may have been switched in between)."""
    if not (_PACK_PAIR and x.device.type == 'cuda' and x.dtype == torch.float32 and w.dtype == torch.float32 and conv_math in ('default', 'f16x3')
            and x.ndim == 4 and w.ndim == 4 and x.numel() > 0 and not torch.cuda.is_current_stream_capturing()):
        return None, None
    kh, kw = int(w.shape[2]), int(w.shape[3])
    n, c_in, h, wd = (int(v) for v in x.shape)
    c_out = int(w.shape[1]) * cfg.groups if cfg.transposed else int(w.shape[0])
    oh, ow = _out_hw(cfg, h, wd, kh, kw)
    if oh < 1 or ow < 1:
        return None, None
    gcfg = _grad_cfg(cfg, (h, wd), (oh, ow), kh, kw)
    da = _desc(cfg, (n, c_in, h, wd), c_out, oh, ow, kh, kw)
    db = _desc(gcfg, (n, c_out, oh, ow), c_in, h, wd, kh, kw)
    na, nb = _plan('conv', da).workspace, _plan('conv', db).workspace
    if na < 0 or nb < 0:
        return None, None
    wa, wb = _workspace(na, x.device), _workspace(nb, x.device)
    mask = ctypes.c_int(0)
    wc = w.contiguous()
    with torch.cuda.device(x.device):
        _native.check(_native.lib().pasta_conv2d_pack_pair(_native.ptr(wc), ctypes.byref(da), _native.ptr(wa), wa.numel() * 4, ctypes.byref(db),
                                                           _native.ptr(wb), wb.numel() * 4, _native.stream(), ctypes.byref(mask)))
    return ((_desc_key(da), wa), (_desc_key(db), wb)) if mask.value == 3 else (None, None)

def _act_epilogue(b, act_cfg, res=None):
    """The ``epilogue`` operand of ``_launch_conv`` for the bias ``b``, ``act_cfg`` = (act, alpha, gain, clamp) and the residual ``res``."""
    from . import bias_act as ba
    act, alpha, gain, clamp = act_cfg
    return (b, ba.activation_funcs[act].cuda_idx, alpha, gain, clamp, res)

def _save_epilogue_output(ctx, y, act_cfg, inputs, extra=(), passthrough=None, tape=True, keep_y=True):
    """Saves ``inputs``, the epilogue's output y and ``extra`` for the backward and returns the forward's result.  y is needed there only as
    the activation / clamp mask: a linear, unclamped layer (the residual skips, whose output the blocks then update in place) must not pin it.
    ``tape``: y passes the test instrument bias_act.SlopeTape first.  ``passthrough`` (the input x): returns (y, x).  ``keep_y=False``: the
    layer defers its activation gradient to the reader of y, which holds y itself."""
    from . import bias_act as ba
    act, _, _, clamp = act_cfg
    if tape and ba.slope_tape is not None:
        y = ba.slope_tape.visit(y, act)
    ctx.save_for_backward(*inputs, y if keep_y and (act != 'linear' or clamp >= 0) else None, *extra)
    if passthrough is None:
        return y
    ctx.set_materialize_grads(False)        # an unused output's gradient arrives as None, not as a tensor of zeros
    return y, passthrough

def _epilogue_grad(dy, y, bias, act_cfg, want_db):
    """(dz, db): the gradient at the convolution's output given the epilogue's dy, and the bias gradient (None unless ``want_db`` and a bias) --
    in one pass where the epilogue has a derivative of its own."""
    from . import bias_act as ba
    act, alpha, gain, clamp = act_cfg
    want_db = want_db and bias is not None
    dz, db = dy, None
    if act != 'linear' or gain != 1 or clamp >= 0:
        if want_db:
            dz, db = ba.grad_with_bias_grad(dy.contiguous(), y, (1, act, alpha, gain, clamp))
        else:
            dz = ba._BiasActHipGrad.apply(dy.contiguous(), None, None, y, (1, act, alpha, gain, clamp))
    if want_db and db is None:
        db = ba._BiasSum.apply(dz, 1)
    return dz, db

def _output_grad(dy, y, bias, act_cfg, want_db, deferred):
    """``_epilogue_grad``, or -- ``deferred``: the reader of y has applied this layer's activation gradient, ``dy`` IS dz -- the bias sum alone."""
    if not deferred:
        return _epilogue_grad(dy, y, bias, act_cfg, want_db)
    from . import bias_act as ba
    return dy, (ba._BiasSum.apply(dy.contiguous(), 1, True) if want_db and bias is not None else None)

def _hand_over(x, again, pieces=False):
    """``again`` is the pass-through output autograd made of ``x``: the same data at the same version, so x's maxima -- and with ``pieces`` its
    packed pieces (``share_pieces``) -- go along for the next reader."""
    if again.is_inference():
        return again
    hit = getattr(x, '_pasta_amax', None)
    if hit is not None:
        again._pasta_amax = hit
    hit = _shared_lookup(x) if pieces else None
    if hit is not None:
        again._pasta_pieces = (again._version, again.data_ptr()) + hit[2:]
    return again

# ---- an input's activation gradient in the launch that writes its gradient (include/pasta_hip.h, pasta_act_mask) --------------------------------
# A layer whose input x is the activated output y of the layer in front holds, in its backward, everything the activation gradient of THAT layer
# needs: dz = dx * act'(y) depends on y alone (relu / lrelu, gain, clamp).  So the launch that writes dx applies it in its store, from its own
# saved tensor, and the layer in front skips its stand-alone pass (two reads and a write of the activation per pair).  The protocol:
#   consumer  ``input_act=(act, alpha, gain, clamp)``: "my x is the activated output of a layer that will not apply its own activation gradient" --
#             the backward returns dz of that layer instead of dx: in the store of the input-gradient launch where a kernel does it and no graph
#             of the backward is recorded, by the differentiable stand-alone pass otherwise (R1's double backward, K-sliced launches, 16-bit
#             storage, the other arithmetics), so that what the producer receives is ALWAYS dz;
#   producer  ``defer_act_grad=True``: its backward takes the incoming gradient as dz and only sums the bias gradient from it.
# Both flags are set together, by the module that owns both layers, for a tensor with no other reader (or whose other reader's gradient joins
# through ``passthrough``, in front of the mask).  Results are bit-identical to the passes: same fp32 value, same rule (csrc/common.h act_grad1).
_ACT_GRAD_IN_WRITER = True      # False: nobody defers, every layer runs its own pass (tests and the A/B compare the two)

def act_grad_pair_ok(x, act):
    """May a module set ``defer_act_grad`` on the layer that writes ``act(.)`` from the fp32 GPU tensor ``x`` and ``input_act`` on its reader?"""
    return (_ACT_GRAD_IN_WRITER and act in ('relu', 'lrelu') and x.device.type == 'cuda' and x.dtype == torch.float32 and x.numel() > 0
            and custom_ops.has_entry(_native.lib(), 'pasta_conv2d_masked'))         # (a library that predates the mask: nobody defers)

def input_act_pass(dx, x, input_act):
    """dz = dx * act'(x) by the stand-alone pass (differentiable to any order): the consumer's fallback."""
    from . import bias_act as ba
    return ba._BiasActHipGrad.apply(dx.contiguous(), None, None, x, (1,) + tuple(input_act))

def mask_store_allowed(dy, x):
    """What every store-side mask asks of the backward it runs in: the protocol on, no graph being recorded, fp32 GPU tensors, a library that has it."""
    return (_ACT_GRAD_IN_WRITER and not torch.is_grad_enabled() and dy.device.type == 'cuda' and dy.dtype == torch.float32 and x.dtype == torch.float32
            and dy.numel() > 0 and custom_ops.has_entry(_native.lib(), 'pasta_conv2d_masked'))

def _mask_launch_ok(dz, w, gcfg):
    """Does a kernel apply the input-activation mask in the store of ``conv(dz, w)`` under ``gcfg`` (pasta_conv2d_mask_available)?"""
    n, c_in, h, wd = (int(v) for v in dz.shape)
    kh, kw = int(w.shape[2]), int(w.shape[3])
    c_out = int(w.shape[1]) * gcfg.groups if gcfg.transposed else int(w.shape[0])
    oh, ow = _out_hw(gcfg, h, wd, kh, kw)
    if oh < 1 or ow < 1:
        return False
    desc = _desc(gcfg, (n, c_in, h, wd), c_out, oh, ow, kh, kw)
    key = ('mask', PLAN_EPILOGUE, _desc_key(desc))
    hit = _plan_cache.get(key)
    if hit is None:
        hit = _plan_cache[key] = _native.lib().pasta_conv2d_mask_available(ctypes.byref(desc), PLAN_EPILOGUE) == 1
    return hit

def _input_grad(dz, w, gcfg, dxp, x, input_act, ws):
    """The gradient at a convolution's input ``x`` given ``dz`` at its output, plus ``dxp`` (another consumer's gradient of ``x``, joined in the
    launch's epilogue where the types agree); with ``input_act`` the result is the gradient at the OUTPUT of the convolution in front of ``x``:
    mask in the store, or launch and pass.  ``ws``: the prepacked workspace of the launch (``_pack_pair``)."""
    join = dxp is not None and dxp.dtype == dz.dtype
    if input_act is not None and (dxp is None or join) and mask_store_allowed(dz, x) and w.dtype == torch.float32 and _mask_launch_ok(dz, w, gcfg):
        return _launch_conv(dz, w, gcfg, epilogue=_act_epilogue(None, _LINEAR_EPILOGUE, dxp), mask=(x, input_act), prepacked=ws)
    if join:
        dx = _ConvBiasActHip.apply(dz, w, None, gcfg, _LINEAR_EPILOGUE, dxp, False, ws)
    else:
        dx = _ConvHip.apply(dz, w, gcfg, ws)
        if dxp is not None:
            dx = dx + dxp
    return dx if input_act is None else input_act_pass(dx, x, input_act)

class _ConvHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, cfg, prepacked=None, input_act=None):
        used = {}
        ctx.dgrad_ws = None
        ctx.input_act = input_act
        if prepacked is None and ctx.needs_input_grad[0]:
            prepacked, ctx.dgrad_ws = _pack_pair(x, w, cfg)
        y = _launch_conv(x, w, cfg, used=used, prepacked=prepacked)
        ctx.save_for_backward(x, w)
        ctx.cfg, ctx.x_amax = cfg, (used.get('x_amax') if x.dtype == torch.float32 else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        cfg = ctx.cfg
        dx = dw = None
        if ctx.needs_input_grad[0]:
            gcfg = _grad_cfg(cfg, x.shape[2:], dy.shape[2:], w.shape[2], w.shape[3])
            dx = _input_grad(dy, w, gcfg, None, x, ctx.input_act, ctx.dgrad_ws)
            assert dx.shape == x.shape
        if ctx.needs_input_grad[1] and not weight_gradients_disabled:
            dw = _ConvWgradHip.apply(dy, x, cfg, tuple(w.shape), w.dtype, ctx.x_amax)
        return dx, dw, None, None, None

class _ConvBiasActHip(torch.autograd.Function):
    """y = bias_act(conv(x, w), b) with the bias / activation / gain / clamp applied in the convolution's epilogue.
    The backward is assembled from the stand-alone differentiable pieces (bias_act gradient kernel, input- and
    weight-gradient convolutions), so gradients of any order keep working.

    ``passthrough=True`` returns ``(y, x)``: the second output is the input again, to be handed to the OTHER consumers of ``x`` (a
    residual block's skip branch).  Their gradient then arrives here as ``dxp`` and joins this layer's input gradient in the epilogue of
    the input-gradient launch (one read of it) -- instead of autograd adding two full tensors afterwards (two reads and a write).
    ``input_act`` / ``defer_act_grad``: the protocol above ``_ACT_GRAD_IN_WRITER`` (this layer as consumer / as producer)."""
    @staticmethod
    def forward(ctx, x, w, b, cfg, act_cfg, res=None, passthrough=False, prepacked=None, input_act=None, defer_act_grad=False):
        used = {}
        ctx.dgrad_ws = None
        ctx.input_act, ctx.defer_act_grad = input_act, bool(defer_act_grad)
        shared = _shared_lookup(x) if not x.is_inference() else None
        if shared is not None and _shared_pieces_ok(x, w, cfg, True):
            # x was packed for its several readers (share_pieces): this launch copies the pieces; its maxima are the pack's bound row
            y = _launch_conv(shared[2], w, cfg, epilogue=_act_epilogue(b, act_cfg, res), pieces=(shared[3], shared[4]))
            used['x_amax'] = shared[3]
        else:
            if prepacked is None and ctx.needs_input_grad[0]:
                prepacked, ctx.dgrad_ws = _pack_pair(x, w, cfg)
            y = _launch_conv(x, w, cfg, epilogue=_act_epilogue(b, act_cfg, res), used=used, prepacked=prepacked)
        ctx.cfg, ctx.act_cfg, ctx.x_amax = cfg, act_cfg, (used.get('x_amax') if x.dtype == torch.float32 else None)
        return _save_epilogue_output(ctx, y, act_cfg, (x, w, b), passthrough=x if passthrough else None, keep_y=not defer_act_grad)

    @staticmethod
    def backward(ctx, dy, dxp=None):
        x, w, b, y = ctx.saved_tensors
        if dy is None:                              # only the pass-through output was differentiated
            if dxp is not None and ctx.input_act is not None:
                dxp = input_act_pass(dxp, x, ctx.input_act)
            return (dxp,) + (None,) * 9
        cfg = ctx.cfg
        dx = dw = None
        dz, db = _output_grad(dy, y, b, ctx.act_cfg, ctx.needs_input_grad[2], ctx.defer_act_grad)
        if ctx.needs_input_grad[0]:
            gcfg = _grad_cfg(cfg, x.shape[2:], dz.shape[2:], w.shape[2], w.shape[3])
            dx = _input_grad(dz, w, gcfg, dxp, x, ctx.input_act, ctx.dgrad_ws)
            assert dx.shape == x.shape
        if ctx.needs_input_grad[1] and not weight_gradients_disabled:
            dw = _ConvWgradHip.apply(dz, x, cfg, tuple(w.shape), w.dtype, ctx.x_amax)
        dres = dz if ctx.needs_input_grad[5] else None     # the residual enters before the activation
        return dx, dw, db, None, None, dres, None, None, None, None

class _BlurConvS2Hip(torch.autograd.Function):
    """``bias_act(conv2d(upfirdn2d(x, f, padding), w, stride=2) [+ res], b)`` -- the down path of conv2d_resample (reference :119-122 followed by the
    layer's bias_act) -- with the blurred tensor written once as the operand pieces of the default arithmetic (``blur_pieces``) instead of as an
    fp32 tensor: the forward convolution and, in the backward, the weight gradient copy pieces.  The backward is assembled from the stand-alone
    differentiable operators (conv_transpose2d for the input gradient, the mirrored filter behind it), so gradients of any order keep working;
    where a gradient OF the weight gradient may be asked for (a backward pass that records a graph: R1), the weight gradient is formed from the
    fp32 blurred tensor recomputed from ``x`` by the differentiable operators instead.  ``passthrough`` as in ``_ConvBiasActHip``: the filter is
    what reads ``x``, and the other consumers' gradient is the addend of its backward launch."""
    @staticmethod
    def forward(ctx, x, f, w, b, ucfg, cfg, act_cfg, res=None, passthrough=False, input_act=None):
        px0, px1, py0, py1, flip, ugain = ucfg
        ctx.input_act = input_act        # (consumer side of the protocol above ``_ACT_GRAD_IN_WRITER``: the mask rides in the filter's transpose)
        pieces, bound, shape = blur_pieces(x, f, (px0, px1, py0, py1), flip, ugain)
        y = _launch_conv(pieces, w, cfg, epilogue=_act_epilogue(b, act_cfg, res), pieces=(bound, shape))
        ctx.ucfg, ctx.cfg, ctx.act_cfg, ctx.shape = ucfg, cfg, act_cfg, shape
        return _save_epilogue_output(ctx, y, act_cfg, (x, f, w, b), (pieces, bound), passthrough=x if passthrough else None)

    @staticmethod
    def backward(ctx, dy, dxp=None):
        from . import upfirdn2d as up
        x, f, w, b, y, pieces, bound = ctx.saved_tensors
        if dy is None:
            if dxp is not None and ctx.input_act is not None:
                dxp = input_act_pass(dxp, x, ctx.input_act)
            return (dxp,) + (None,) * 9
        cfg, shape = ctx.cfg, ctx.shape
        px0, px1, py0, py1, flip, ugain = ctx.ucfg
        dx = dw = None
        dz, db = _epilogue_grad(dy, y, b, ctx.act_cfg, ctx.needs_input_grad[3])
        if ctx.needs_input_grad[0]:
            gcfg = _grad_cfg(cfg, shape[2:], dz.shape[2:], w.shape[2], w.shape[3])
            dxb = _ConvHip.apply(dz, w, gcfg)                   # gradient of the blurred tensor
            assert tuple(dxb.shape) == tuple(shape)
            ih, iw = x.shape[2], x.shape[3]
            ucfg_t = (1, 1, 1, 1, 3 - px0, iw - shape[3] + px0, 3 - py0, ih - shape[2] + py0, not flip, ugain)      # upfirdn2d._Upfirdn2dHip.backward, up = down = 1, 4 taps
            dx = up.input_grad(dxb, f, ucfg_t, dxp, x, ctx.input_act)
            assert dx.shape == x.shape
        elif dxp is not None:
            dx = dxp if ctx.input_act is None else input_act_pass(dxp, x, ctx.input_act)
        if ctx.needs_input_grad[2] and not weight_gradients_disabled:
            if torch.is_grad_enabled():             # a graph of this backward pass is being recorded: keep everything differentiable
                xb = up._Upfirdn2dHip.apply(x, f, (1, 1, 1, 1, px0, px1, py0, py1, flip, ugain))
                dw = _ConvWgradHip.apply(dz, xb, cfg, tuple(w.shape), w.dtype, None)
            else:
                dw = _launch_wgrad(pieces, dz, cfg, tuple(w.shape), w.dtype, pieces=(bound, shape))
        dres = dz if ctx.needs_input_grad[7] else None
        return dx, None, dw, db, None, None, None, dres, None, None

def blur_conv2d_s2_bias_act(x, f, weight, pad4, flip_filter=False, bias=None, act='linear', alpha=None, gain=None, clamp=None, wgain=1.0,
                            residual=None, passthrough=False, input_act=None):
    """``bias_act(conv2d(upfirdn2d(x, f, padding=pad4, flip_filter=flip_filter), weight, stride=2) [+ residual], bias, ...)`` with the blurred
    tensor as producer-written operand pieces (``pieces_available`` says whether the kernels exist for these shapes)."""
    from . import bias_act as ba
    act_cfg = ba.act_cfg(act, alpha, gain, clamp)
    assert act in FUSABLE_ACTS
    cfg = _Cfg((False, 2, 0, 0, 0, 0, 1, float(wgain)))
    ucfg = (int(pad4[0]), int(pad4[1]), int(pad4[2]), int(pad4[3]), bool(flip_filter), 1.0)
    if passthrough and torch.is_grad_enabled() and x.requires_grad:
        y, again = _BlurConvS2Hip.apply(x, f, weight, bias, ucfg, cfg, act_cfg, residual, True, input_act)
        return y, _hand_over(x, again)
    y = _BlurConvS2Hip.apply(x, f, weight, bias, ucfg, cfg, act_cfg, residual, False, input_act)
    return (y, x) if passthrough else y

_LINEAR_EPILOGUE = ('linear', 0.0, 1.0, -1.0)      # (act, alpha, gain, clamp) of an epilogue that only adds the residual

FUSABLE_ACTS = ('linear', 'relu', 'lrelu')

def cat1x1_available(x, x2, weight):
    """Will ``conv2d_cat1x1_bias_act`` run as ONE launch over the two tensors (the pointwise kernel, pasta_conv2d_plan kernel 9)?"""
    if not (x.device.type == 'cuda' and x.dtype == torch.float32 and x2.dtype == torch.float32 and x.ndim == 4 and x2.shape[0] == x.shape[0]
            and x2.shape[2:] == x.shape[2:] and tuple(weight.shape[2:]) == (1, 1) and weight.shape[1] == x.shape[1] + x2.shape[1]
            and conv_math in ('default', 'f16x3') and x.numel() > 0):
        return False
    n, h, w_ = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
    desc = _desc(_Cfg((False, 1, 0, 0, 0, 0, 1, 1.0)), (n, int(x.shape[1]) + int(x2.shape[1]), h, w_), int(weight.shape[0]), h, w_, 1, 1)
    return _plan('conv', desc, PLAN_EPILOGUE).kernel == custom_ops.FWD_1X1

class _CatConv1x1BiasActHip(torch.autograd.Function):
    """``bias_act(conv2d(cat([x, x2], 1), w), b)`` for a 1x1 weight in one launch over the two tensors; the backward is assembled from the
    stand-alone differentiable pieces -- the two input gradients are two pointwise launches on the weight's channel slices (two
    contiguous tensors, where the concatenation's backward hands out channel slices of one), the weight gradient two launches whose
    results are concatenated (a few hundred KB)."""
    @staticmethod
    def forward(ctx, x, x2, w, b, wgain, act_cfg):
        cfg = _Cfg((False, 1, 0, 0, 0, 0, 1, float(wgain)))
        used = {}
        y = _launch_conv(x, w, cfg, epilogue=_act_epilogue(b, act_cfg), x2=x2, used=used)
        ctx.cfg, ctx.act_cfg, ctx.amax = cfg, act_cfg, (used.get('x_amax'), used.get('x2_amax'))
        return _save_epilogue_output(ctx, y, act_cfg, (x, x2, w, b), tape=False)

    @staticmethod
    def backward(ctx, dy):
        x, x2, w, b, y = ctx.saved_tensors
        cfg = ctx.cfg
        dx = dx2 = dw = None
        dz, db = _epilogue_grad(dy, y, b, ctx.act_cfg, ctx.needs_input_grad[3])
        c1 = x.shape[1]
        gcfg = _grad_cfg(cfg, x.shape[2:], dz.shape[2:], 1, 1)
        if ctx.needs_input_grad[0]:
            dx = _ConvHip.apply(dz, w[:, :c1], gcfg)
        if ctx.needs_input_grad[1]:
            dx2 = _ConvHip.apply(dz, w[:, c1:], gcfg)
        if ctx.needs_input_grad[2] and not weight_gradients_disabled:
            dw = torch.cat([_ConvWgradHip.apply(dz, x, cfg, (w.shape[0], c1, 1, 1), w.dtype, ctx.amax[0]),
                            _ConvWgradHip.apply(dz, x2, cfg, (w.shape[0], w.shape[1] - c1, 1, 1), w.dtype, ctx.amax[1])], dim=1)
        return dx, dx2, dw, db, None, None

def conv2d_cat1x1_bias_act(x, x2, weight, bias=None, act='linear', alpha=None, gain=None, clamp=None, wgain=1.0):
    """``bias_act(conv2d(torch.cat([x, x2], 1), weight), bias, ...)`` for a 1x1 ``weight`` without the concatenated tensor
    (``cat1x1_available`` says whether the one-launch form exists for these shapes; otherwise the concatenation is formed)."""
    from . import bias_act as ba
    act_cfg = ba.act_cfg(act, alpha, gain, clamp)
    if act in FUSABLE_ACTS and cat1x1_available(x, x2, weight):
        return _CatConv1x1BiasActHip.apply(x, x2, weight, bias, float(wgain), act_cfg)
    return conv2d_bias_act(torch.cat([x, x2], dim=1), weight, bias, act=act, alpha=act_cfg[1], gain=act_cfg[2], clamp=clamp, wgain=wgain)

def conv2d_bias_act(input, weight, bias=None, stride=1, padding=0, groups=1, act='linear', alpha=None, gain=None, clamp=None, wgain=1.0,
                    residual=None, passthrough=False, input_act=None, defer_act_grad=False):
    """``bias_act(conv2d(input, weight) [+ residual], bias, act, alpha, gain, clamp)`` in one launch (fp32 GPU tensors,
    act in FUSABLE_ACTS); other cases run the ops separately.  ``passthrough=True`` returns ``(y, input')`` where ``input'`` is the
    input again, for its other consumers: see ``_ConvBiasActHip``.  ``input_act`` / ``defer_act_grad``: the protocol above
    ``_ACT_GRAD_IN_WRITER`` (fused launches only: ``act_grad_pair_ok`` is what a module asks before it sets them)."""
    from . import bias_act as ba
    act_cfg = ba.act_cfg(act, alpha, gain, clamp)
    if act in FUSABLE_ACTS and input.dtype in IO_CODES and input.device.type == 'cuda' and input.numel() > 0:
        sh, sw = _pair(stride)
        ph, pw = _pair(padding)
        assert sh == sw
        cfg = _Cfg((False, sh, ph, pw, 0, 0, int(groups), float(wgain)))
        if passthrough and torch.is_grad_enabled() and input.requires_grad:
            y, again = _ConvBiasActHip.apply(input, weight, bias, cfg, act_cfg, residual, True, None, input_act, defer_act_grad)
            return y, _hand_over(input, again, pieces=True)
        y = _ConvBiasActHip.apply(input, weight, bias, cfg, act_cfg, residual, False, None, input_act, defer_act_grad)
        return (y, input) if passthrough else y
    assert input_act is None and not defer_act_grad, 'input_act / defer_act_grad belong to the fused launches (act_grad_pair_ok)'
    y = conv2d(input, weight, stride=stride, padding=padding, groups=groups, wgain=wgain)
    if residual is not None:
        y = y + residual
    y = ba.bias_act(y, bias, act=act, alpha=act_cfg[1], gain=act_cfg[2], clamp=clamp)
    return (y, input) if passthrough else y

def modulated_conv2d_forward(x, weight, styles, dcoefs=None, stride=1, padding=0, transposed=False, per_sample=False, tail=None):
    """FORWARD-ONLY modulated convolution (networks.py:36-94) in one launch -- no autograd graph is recorded; the training
    path keeps its differentiable pieces.  ``x`` [N,I,H,W], ``weight`` [O,I,kh,kw] ([I,O,kh,kw] when ``transposed``),
    ``styles`` [N,I], ``dcoefs`` [N,O] or None.

    ``per_sample=False``: ``conv(x * styles) * dcoefs`` with the shared weight.  fp32 tensors: the styles ride in the
    kernel's activation staging (``iscale``), no modulated copy of ``x`` is written; 16-bit tensors are scaled by a pass of
    their own first.  ``per_sample=True``: the reference's grouped form (groups = N), each sample's weights
    ``w * styles[n] * dcoefs[n]`` formed by the weight-packing kernel.
    ``tail`` = dict(noise=unit plane(s) or None, strength=scalar tensor, bias, act, alpha, gain, clamp): the rest of
    SynthesisLayer / ToRGBLayer -- ``+ noise * strength``, bias, activation, gain, clamp -- in the convolution's epilogue
    (act in FUSABLE_ACTS).  Without ``tail`` the plain (for ``per_sample``: demodulated) convolution is returned and
    ``dcoefs`` of the shared form must be applied by the caller (an upsampling layer filters first)."""
    from . import bias_act as ba
    from . import fma
    assert not (torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, weight, styles, dcoefs))), \
        'modulated_conv2d_forward records no graph'
    n, o = int(x.shape[0]), int(weight.shape[1] if transposed else weight.shape[0])
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    assert sh == sw
    epilogue = noise = None
    if tail is not None:
        assert tail['act'] in FUSABLE_ACTS
        bias = tail.get('bias')
        if bias is not None and per_sample:
            bias = bias.repeat(n)                       # the grouped launch has N * O output channels
        epilogue = _act_epilogue(bias, ba.act_cfg(tail['act'], tail.get('alpha'), tail.get('gain'), tail.get('clamp')))
        if tail.get('noise') is not None:
            noise = (tail['noise'], tail['strength'])
    if per_sample:
        if noise is not None and noise[0].numel() != noise[0].shape[-1] * noise[0].shape[-2]:
            raise NotImplementedError('modulated_conv2d_forward: per-sample noise with per-sample weights')
        cfg = _Cfg((bool(transposed), sh, ph, pw, 0, 0, n, 1.0))
        y = _launch_conv(x.reshape(1, -1, *x.shape[2:]), weight, cfg, epilogue=epilogue, wmod=(styles, dcoefs), noise=noise)
        return y.reshape(n, o, *y.shape[2:])
    cfg = _Cfg((bool(transposed), sh, ph, pw, 0, 0, 1, 1.0))
    if x.dtype != torch.float32:
        x, styles = fma.scale_planes(x, styles), None
    if tail is None:
        return _launch_conv(x, weight, cfg, iscale=styles)
    return _launch_conv(x, weight, cfg, iscale=styles, oscale=dcoefs, epilogue=epilogue, noise=noise)

#----------------------------------------------------------------------------
# Shared-weight modulated convolution of the TRAINING path, y = conv(x * s[n, i], w)  (networks.py:72-76), without the tensor x * s:
#   forward          conv(x, w) with the styles multiplied onto the activations in the kernel's staging (``iscale``),
#   input gradient   conv^T(dy, w) with the styles as the output scale of the launch's epilogue (``oscale``),
#   weight gradient  the plain weight-gradient kernels on the UNMODULATED x with sample-aligned K slices, whose reduction forms
#                    dw = sum_n s[n, i] Dw_n and ds[n, i] = sum_{o, taps} w Dw_n  (pasta_conv2d_wgrad_modulated),
# instead of scale_planes (a read and a write of the activation) + a scan of x * s for its operand scale + scale_planes of the input
# gradient + plane_dot(dx, x) (two reads): seven passes over the activation per modulated layer.  

_MODCONV = True         # False: scale_planes + the plain convolution, as the reference (tests compare the two)

def modconv_available(x, weight, styles, stride=1, padding=0, transposed=False):
    """Does ``modulated_conv2d_shared`` run natively for these operands (else the caller scales the planes itself)?"""
    if not (_MODCONV and x.device.type == 'cuda' and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.ndim == 4 and x.numel() > 0
            and conv_math in ('default', 'f16x3') and not transposed and stride == 1):
        return False
    ph, pw = _pair(padding)
    cfg = _Cfg((False, 1, ph, pw, 0, 0, 1, 1.0))
    kh, kw = int(weight.shape[2]), int(weight.shape[3])
    oh, ow = _out_hw(cfg, x.shape[2], x.shape[3], kh, kw)
    return _plan('wgrad_modulated', _desc(cfg, x.shape, int(weight.shape[0]), oh, ow, kh, kw)).ok

def _launch_wgrad_modulated(x, dy, cfg, styles, w, x_amax=None):
    """(dw, dstyles) of ``conv(x * styles, w)`` given dy: pasta_conv2d_wgrad_modulated (``modconv_available`` says where it exists)."""
    _native.require_gpu(x, 'conv2d_wgrad_modulated')
    x, dy = _f32(x).contiguous(), _f32(dy).contiguous()
    styles, w32 = _f32(styles).contiguous(), _f32(w).contiguous()
    desc = _desc(cfg, x.shape, dy.shape[1], dy.shape[2], dy.shape[3], int(w.shape[2]), int(w.shape[3]))
    dw = torch.empty(list(w.shape), dtype=torch.float32, device=x.device)
    ds = torch.empty([x.shape[0], x.shape[1]], dtype=torch.float32, device=x.device)
    _wgrad_issue('wgrad_modulated', desc, x, dy, x_amax, True, _native.lib().pasta_conv2d_wgrad_modulated, (x, dy, styles, w32, dw, ds), dw)
    return dw, ds

class _ModConvHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, s, cfg):
        used = {}
        y = _launch_conv(x, w, cfg, iscale=s, used=used)
        ctx.save_for_backward(x, w, s)
        ctx.cfg, ctx.x_amax = cfg, used.get('x_amax')
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, w, s = ctx.saved_tensors
        cfg = ctx.cfg
        dx = dw = ds = None
        dy = dy.contiguous()
        if ctx.needs_input_grad[0]:
            dx = _launch_conv(dy, w, _grad_cfg(cfg, x.shape[2:], dy.shape[2:], w.shape[2], w.shape[3]), oscale=s)
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            dw, ds = _launch_wgrad_modulated(x, dy, cfg, s, w, x_amax=ctx.x_amax)
            dw = dw.to(w.dtype) if ctx.needs_input_grad[1] and not weight_gradients_disabled else None
            ds = ds.to(s.dtype) if ctx.needs_input_grad[2] else None
        return dx, dw, ds, None

def modulated_conv2d_shared(x, weight, styles, padding=0):
    """``conv2d(x * styles[:, :, None, None], weight, padding=padding)`` for the training path (where ``modconv_available``); first derivatives only,
    like the reference's own fused op would be used (the generator has no second-order phase: networks.py / loss_wo_flow_fullbody.py run no
    path-length regularisation).  ``styles``: [N, C_in]."""
    ph, pw = _pair(padding)
    cfg = _Cfg((False, 1, ph, pw, 0, 0, 1, 1.0))
    return _ModConvHip.apply(x, weight, styles.to(torch.float32).reshape(x.shape[0], x.shape[1]), cfg)

def demod_coefs(weight, styles):
    """``rsqrt(sum_{i,kh,kw} (weight[o,i] * styles[n,i])^2 + 1e-8)`` [N, O] (networks.py:65-68) by ``pasta_demod_coefs``: one
    workgroup per output channel, wavefront-shuffle reduction; differentiable to any order (the backward is written in
    differentiable torch operations on the small [N,I] / [O,I] matrices)."""
    return _DemodCoefs.apply(weight, styles)

class _DemodCoefs(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, styles):
        _native.require_gpu(weight, 'demod_coefs')
        o, i = int(weight.shape[0]), int(weight.shape[1])
        n = int(styles.shape[0])
        assert styles.shape == (n, i)
        w32, s32 = _f32(weight).contiguous(), _f32(styles).contiguous()
        d = torch.empty([n, o], dtype=torch.float32, device=weight.device)
        with torch.cuda.device(weight.device):
            _native.check(_native.lib().pasta_demod_coefs(_native.ptr(w32), _native.ptr(s32), _native.ptr(d), n, o, i,
                                                          int(weight[0, 0].numel()), 1e-8, _native.stream()))
        ctx.save_for_backward(weight, styles, d)
        return d.to(styles.dtype)

    @staticmethod
    def backward(ctx, g):
        weight, styles, d = ctx.saved_tensors
        if torch.is_grad_enabled():         # a graph of this backward is being recorded: d has to be a function of the inputs again
            d = _DemodCoefs.apply(weight, styles).to(torch.float32)
        # d = q^-1/2, q[n,o] = sum_i s[n,i]^2 W2[o,i] + eps, W2 = sum_taps w^2
        dq = -0.5 * g.to(torch.float32) * d * d * d
        ds = dw = None
        if ctx.needs_input_grad[1]:
            ds = (2 * styles * (dq @ weight.square().sum(dim=[2, 3]).to(torch.float32))).to(styles.dtype)
        if ctx.needs_input_grad[0]:
            dw = (2 * weight * (dq.t() @ styles.square().to(torch.float32))[:, :, None, None]).to(weight.dtype)
        return dw, ds

class _ConvWgradHip(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dy, x, cfg, w_shape, w_dtype=None, x_amax=None):
        dw = _launch_wgrad(x, dy, cfg, w_shape, w_dtype, x_amax=x_amax)
        ctx.save_for_backward(dy, x)
        ctx.cfg = cfg
        return dw

    @staticmethod
    def backward(ctx, d_dw):
        dy, x = ctx.saved_tensors
        cfg = ctx.cfg
        d_dy = d_x = None
        if ctx.needs_input_grad[0]:     # y is linear in w: d_dy = conv(x, d_dw)
            d_dy = _ConvHip.apply(x, d_dw, cfg)
            assert d_dy.shape == dy.shape
        if ctx.needs_input_grad[1]:     # and dx is linear in w as well
            gcfg = _grad_cfg(cfg, x.shape[2:], dy.shape[2:], d_dw.shape[2], d_dw.shape[3])
            d_x = _ConvHip.apply(dy, d_dw, gcfg)
            assert d_x.shape == x.shape
        return d_dy, d_x, None, None, None, None

#----------------------------------------------------------------------------

def _check_common(input, weight, dilation):
    assert isinstance(input, torch.Tensor) and isinstance(weight, torch.Tensor)
    if _pair(dilation) != (1, 1):
        raise NotImplementedError('conv2d_gradfix: dilation != 1 is not on the PASTA-GAN path and is not implemented')

def _add_bias(y, bias):
    return y if bias is None else y + bias.to(y.dtype).reshape(1, -1, 1, 1)

def conv2d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, wgain=1.0, input_act=None):
    """Same contract as ``torch.nn.functional.conv2d`` (reference :35-38); equal strides in x and y.
    ``wgain`` (extension): convolve with ``weight * wgain`` without materialising the product.  ``input_act`` (extension): this layer as
    consumer in the protocol above ``_ACT_GRAD_IN_WRITER``."""
    _check_common(input, weight, dilation)
    sh, sw = _pair(stride)
    if sh != sw:
        raise NotImplementedError('conv2d_gradfix: anisotropic stride is not implemented')
    ph, pw = _pair(padding)
    cfg = _Cfg((False, sh, ph, pw, 0, 0, int(groups), float(wgain)))
    return _add_bias(_ConvHip.apply(input, weight, cfg, None, input_act), bias)

def conv_transpose2d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1, wgain=1.0):
    """Same contract as ``torch.nn.functional.conv_transpose2d`` (reference :40-43)."""
    _check_common(input, weight, dilation)
    sh, sw = _pair(stride)
    if sh != sw:
        raise NotImplementedError('conv2d_gradfix: anisotropic stride is not implemented')
    ph, pw = _pair(padding)
    oph, opw = _pair(output_padding)
    cfg = _Cfg((True, sh, ph, pw, oph, opw, int(groups), float(wgain)))
    return _add_bias(_ConvHip.apply(input, weight, cfg), bias)

#----------------------------------------------------------------------------
