"""Build and load the native HIP library behind ``torch_utils.ops``.

Stands where the reference's JIT plugin loader stands (torch_utils/custom_ops.py:46-124,
``get_plugin(module_name, sources, **build_kwargs)``), but for one ahead-of-time library:
``csrc/*.hip`` -> ``hipcc --offload-arch=gfx950`` -> ``lib/libpasta_hip.so`` kept in-tree,
loaded with ``ctypes`` through the C ABI declared in ``include/pasta_hip.h``.

There is no fallback: if the library cannot be built or loaded, every op raises.
"""

import ctypes
import fcntl
import hashlib
import os
import shutil
import subprocess
import threading
import time
import warnings

# PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so) and puts it in the process-global symbol scope.
# Importing torch BEFORE loading libpasta_hip.so makes the library's HIP calls bind to that same runtime, so its
# kernels and PyTorch's share devices, streams and allocations. Loaded the other way round the process ends up with
# two HIP runtimes and the second one finds no device.
import torch  # noqa: F401  (must precede ctypes.CDLL below)

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # .../pasta-gan_amd
_CSRC = os.path.join(_ROOT, 'csrc')
_LIBDIR = os.path.join(_ROOT, 'lib')
_OBJDIR = os.path.join(_ROOT, 'build')
_INCLUDE = os.path.join(os.path.dirname(_ROOT), 'include')
LIB_NAME = 'libpasta_hip.so'
EXPECTED_ABI = 22                   # pasta_abi_version() of include/pasta_hip.h and csrc/common.hip
ARCH = 'gfx950'

# The kernels as the planners name them: PASTA_FWD_* (pasta_conv2d_plan) and PASTA_WGRAD_* (pasta_conv2d_wgrad_plan) of include/pasta_hip.h
(FWD_F32, FWD_BASE, FWD_ROWS, FWD_PAIR, FWD_ROWS2D_R4, FWD_ROWS2D_R2, FWD_ROWS2D_R8, FWD_ROWS2D_WIDE, FWD_PACKED_K, FWD_1X1, FWD_3X3S2,
 FWD_FEWCIN, FWD_FEWCOUT, FWD_T2) = range(14)
WGRAD_F32, WGRAD_SMALLCIN, WGRAD_3X3, WGRAD_3X3S2, WGRAD_1X1, WGRAD_FEWCIN, WGRAD_3X3S2_PIECES = range(7)

_lock = threading.Lock()
_cached_plugins = dict()

#----------------------------------------------------------------------------

def _sources():
    return sorted(os.path.join(_CSRC, f) for f in os.listdir(_CSRC) if f.endswith('.hip'))

def _digest(sources, extra_flags=()):
    h = hashlib.md5()
    # the compile flags are part of what the library IS: a build with extra -D flags must never carry the default stamp
    h.update(repr([str(f) for f in extra_flags]).encode())
    extra = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC)) if f.endswith('.h')]
    extra.append(os.path.join(_INCLUDE, 'pasta_hip.h'))
    for path in list(sources) + extra:
        h.update(os.path.basename(path).encode())
        with open(path, 'rb') as f:
            h.update(f.read())
    return h.hexdigest()

def _hipcc():
    return shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)

def _stamp_matches(lib_path, stamp, digest):
    if not (os.path.exists(lib_path) and os.path.exists(stamp)):
        return False
    with open(stamp) as f:
        return f.read().strip() == digest

def build(force=False, verbose=False, extra_flags=()):
    """Compile every ``csrc/*.hip`` for gfx950 and link ``lib/libpasta_hip.so``.

    Skips the work when the stored source digest matches. Returns the library path.  Concurrent callers (several ranks
    importing the ops at once) are serialised by an exclusive lock on ``lib/.build.lock`` -- the reference loader does
    the same with a file baton (custom_ops.py:86-92) -- and whoever gets the lock second finds the stamp up to date."""
    sources = _sources()
    lib_path = os.path.join(_LIBDIR, LIB_NAME)
    stamp = lib_path + '.md5'
    digest = _digest(sources, extra_flags)
    if not force and _stamp_matches(lib_path, stamp, digest):
        return lib_path
    hipcc = _hipcc()
    if hipcc is None:
        raise RuntimeError('hipcc not found: cannot build ' + LIB_NAME)
    os.makedirs(_LIBDIR, exist_ok=True)
    os.makedirs(_OBJDIR, exist_ok=True)
    with open(os.path.join(_LIBDIR, '.build.lock'), 'w') as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and _stamp_matches(lib_path, stamp, digest):
                return lib_path
            return _compile_and_link(hipcc, sources, lib_path, stamp, digest, verbose, extra_flags)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)

def _unit_weight(src):
    """Rough compile cost of a translation unit, for the build order: the kernel instances are in the conv_tu_* units and in bias_act."""
    name = os.path.basename(src)
    return (4 if name.startswith(('conv_tu_fwd_rows', 'conv_tu_rows2d', 'conv_tu_fwd_base', 'bias_act')) else 2 if name.startswith(('conv_tu_', 'upfirdn2d')) else 1)

def _compile_and_link(hipcc, sources, lib_path, stamp, digest, verbose, extra_flags):
    flags = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-ffp-contract=fast', '-I', _INCLUDE] + list(extra_flags)
    # one hipcc per translation unit, at most one per core at a time, the large units first (the convolution family is nineteen
    # units, csrc/conv_launch.h: a forced build takes about a minute on eight cores)
    objs = [os.path.join(_OBJDIR, os.path.basename(src)[:-4] + '.o') for src in sources]
    queue = sorted(zip(sources, objs), key=lambda so: -_unit_weight(so[0]))
    # PASTA_BUILD_JOBS, else MAX_JOBS (the usual cap for extension builds), else the CPUs this process may run on
    jobs = int(os.environ.get('PASTA_BUILD_JOBS') or os.environ.get('MAX_JOBS') or 0) or len(os.sched_getaffinity(0))
    jobs = max(1, min(len(queue), jobs))
    running, failed = [], None
    while (queue and failed is None) or running:
        while queue and failed is None and len(running) < jobs:
            src, obj = queue.pop(0)
            cmd = [hipcc] + flags + ['-c', src, '-o', obj]
            if verbose:
                print(' '.join(cmd))
            log = open(obj[:-2] + '.log', 'wb')      # a file, not a pipe: a unit that prints many warnings must not block on a full pipe
            running.append((src, log, subprocess.Popen(cmd, stdout=log, stderr=subprocess.STDOUT)))
        for item in list(running):
            src, log, proc = item
            if proc.poll() is None:
                continue
            running.remove(item)
            log.close()
            if proc.returncode != 0 and failed is None:
                with open(log.name, 'rb') as f:
                    failed = 'hipcc failed on %s:\n%s' % (src, f.read().decode(errors='replace'))
        if running:
            time.sleep(0.05)
    if failed is not None:
        raise RuntimeError(failed)
    tmp = lib_path + '.tmp%d' % os.getpid()
    cmd = [hipcc, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', tmp] + objs
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if res.returncode != 0:
        raise RuntimeError('link failed:\n' + res.stdout.decode(errors='replace'))
    os.replace(tmp, lib_path)
    with open(stamp, 'w') as f:
        f.write(digest)
    return lib_path

#----------------------------------------------------------------------------

_c_i32 = ctypes.c_int32
_c_i64 = ctypes.c_int64
_c_f32 = ctypes.c_float
_c_ptr = ctypes.c_void_p

class ConvDesc(ctypes.Structure):
    """Mirror of ``pasta_conv_desc`` (include/pasta_hip.h)."""
    _fields_ = [(name, _c_i32) for name in (
        'N', 'C_in', 'H', 'W', 'C_out', 'OH', 'OW', 'kh', 'kw', 'stride',
        'pad_h', 'pad_w', 'groups', 'transposed', 'flip', 'math')] + [('wscale', _c_f32), ('io_dtype', _c_i32),
                                                                      ('x_amax', _c_ptr), ('x2', _c_ptr), ('x2_amax', _c_ptr), ('C1', _c_i32), ('dy_amax', _c_ptr), ('x_layout', _c_i32), ('w_prepacked', _c_i32)]

class ConvEpilogue(ctypes.Structure):
    """Mirror of ``pasta_conv_epilogue`` (include/pasta_hip.h)."""
    _fields_ = [('bias', _c_ptr), ('act', _c_i32), ('alpha', _c_f32), ('gain', _c_f32), ('clamp', _c_f32), ('res', _c_ptr),
                ('noise', _c_ptr), ('noise_strength', _c_ptr), ('noise_per_sample', _c_i32), ('y_amax', _c_ptr)]

class ActMask(ctypes.Structure):
    """Mirror of ``pasta_act_mask`` (include/pasta_hip.h)."""
    _fields_ = [('m', _c_ptr), ('act', _c_i32), ('alpha', _c_f32), ('gain', _c_f32), ('clamp', _c_f32)]

class AdaConfig(ctypes.Structure):
    """Mirror of ``pasta_ada_config`` (include/pasta_hip.h)."""
    _fields_ = [(name, _c_f32) for name in (
        'xflip', 'rotate90', 'xint', 'xint_max', 'scale', 'rotate', 'aniso', 'xfrac', 'scale_std', 'rotate_max', 'aniso_std',
        'xfrac_std', 'brightness', 'contrast', 'lumaflip', 'hue', 'saturation', 'brightness_std', 'contrast_std', 'hue_max',
        'saturation_std')]

# name -> (restype, argtypes); exactly the symbols include/pasta_hip.h declares.
ABI = {
    'pasta_last_error':   (ctypes.c_char_p, []),
    'pasta_abi_version':  (ctypes.c_int, []),
    'pasta_build_info':   (ctypes.c_char_p, []),
    'pasta_upfirdn2d':    (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, ctypes.c_int,
                                          ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i32),
                                          ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i64)] + [ctypes.c_int] * 9 + [_c_f32, _c_ptr, _c_ptr, _c_ptr]),
    'pasta_bias_act':     (ctypes.c_int, [_c_ptr] * 6 + [ctypes.c_int, _c_i64, ctypes.c_int, _c_i64, ctypes.c_int, ctypes.c_int,
                                                           _c_f32, _c_f32, _c_f32, _c_ptr, _c_ptr]),
    'pasta_bias_grad_workspace': (_c_i64, [_c_i64, ctypes.c_int, _c_i64]),
    'pasta_bias_grad':    (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, ctypes.c_int, _c_i64, ctypes.c_int, _c_i64, _c_ptr]),
    'pasta_bias_act_grad_db_workspace': (_c_i64, [ctypes.c_int, _c_i64, ctypes.c_int, _c_i64, ctypes.c_int]),
    'pasta_bias_act_grad_db': (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, _c_ptr, _c_ptr, ctypes.c_int, _c_i64, ctypes.c_int, _c_i64, ctypes.c_int,
                                              ctypes.c_float, ctypes.c_float, ctypes.c_float, _c_ptr, _c_ptr]),
    'pasta_bias_sum_db':   (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, ctypes.c_int, _c_i64, ctypes.c_int, _c_i64, _c_ptr]),
    'pasta_pieces_bytes':  (_c_i64, [ctypes.c_int] * 4),
    'pasta_blur_pieces':   (ctypes.c_int, [_c_ptr] * 5 + [ctypes.c_int] * 9 + [_c_f32, _c_ptr]),
    'pasta_pieces_unpack': (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int] * 4 + [_c_ptr]),
    'pasta_pieces_pack': (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int] * 4 + [_c_ptr]),
    'pasta_conv2d_pack_pair': (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, ctypes.c_int64, _c_ptr, _c_ptr, ctypes.c_int64, _c_ptr, _c_ptr]),
    'pasta_conv2d_workspace':       (_c_i64, [ctypes.POINTER(ConvDesc)]),
    'pasta_conv2d_wgrad_workspace': (_c_i64, [ctypes.POINTER(ConvDesc)]),
    'pasta_conv2d_tile':  (ctypes.c_int, [ctypes.POINTER(ConvDesc)]),
    'pasta_conv2d_plan':  (ctypes.c_int, [ctypes.POINTER(ConvDesc), ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 5),
    'pasta_conv2d_wgrad_plan': (ctypes.c_int, [ctypes.POINTER(ConvDesc), ctypes.POINTER(ctypes.c_int)]),
    'pasta_conv2d':       (ctypes.c_int, [_c_ptr] * 5 + [ctypes.POINTER(ConvDesc), _c_ptr, _c_i64, _c_ptr]),
    'pasta_conv2d_ex':    (ctypes.c_int, [_c_ptr] * 5 + [ctypes.POINTER(ConvEpilogue), ctypes.POINTER(ConvDesc), _c_ptr, _c_i64, _c_ptr]),
    'pasta_conv2d_masked': (ctypes.c_int, [_c_ptr] * 5 + [ctypes.POINTER(ConvEpilogue), ctypes.POINTER(ActMask), ctypes.POINTER(ConvDesc), _c_ptr, _c_i64, _c_ptr]),
    'pasta_conv2d_mask_available': (ctypes.c_int, [ctypes.POINTER(ConvDesc), ctypes.c_int]),
    'pasta_upfirdn2d_masked': (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, ctypes.c_int,
                                              ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i32),
                                              ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i64)] + [ctypes.c_int] * 9 + [_c_f32, _c_ptr, _c_ptr, _c_ptr,
                                                                                                                      ctypes.POINTER(ActMask)]),
    'pasta_upfirdn2d_mask_available': (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i32)] + [ctypes.c_int] * 8),
    'pasta_conv2d_wgrad': (ctypes.c_int, [_c_ptr] * 3 + [ctypes.POINTER(ConvDesc), _c_ptr, _c_i64, _c_ptr]),
    'pasta_conv2d_wgrad_modulated': (ctypes.c_int, [_c_ptr] * 6 + [ctypes.POINTER(ConvDesc), _c_ptr, _c_i64, _c_ptr]),
    'pasta_conv2d_wgrad_modulated_workspace': (_c_i64, [ctypes.POINTER(ConvDesc)]),
    'pasta_conv2d_modulated': (ctypes.c_int, [_c_ptr] * 5 + [ctypes.POINTER(ConvEpilogue), ctypes.POINTER(ConvDesc), _c_ptr, _c_i64, _c_ptr]),
    'pasta_tensor_amax':  (ctypes.c_int, [_c_ptr, _c_i64, ctypes.c_int, _c_ptr, _c_ptr]),
    'pasta_demod_coefs':  (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int] * 4 + [_c_f32, _c_ptr]),
    'pasta_scale_add':    (ctypes.c_int, [_c_ptr] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i64, ctypes.c_int, _c_ptr, _c_ptr]),
    'pasta_plane_dot':    (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int, _c_i64, _c_i64, _c_ptr]),
    'pasta_mod_bias_act': (ctypes.c_int, [_c_ptr] * 6 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                          ctypes.c_float, ctypes.c_float, _c_ptr, _c_ptr]),
    'pasta_mod_bias_act_bwd_workspace': (_c_i64, [ctypes.c_int, ctypes.c_int, _c_i64]),
    'pasta_mod_bias_act_bwd': (ctypes.c_int, [_c_ptr] * 7 + [ctypes.c_int, ctypes.c_int, ctypes.c_int, _c_i64, ctypes.c_int, ctypes.c_int, ctypes.c_float,
                                              ctypes.c_float, ctypes.c_float, _c_ptr, _c_ptr]),
    'pasta_masked_mean_fill': (ctypes.c_int, [_c_ptr] * 5 + [ctypes.c_int, ctypes.c_int, _c_i64, _c_i64, _c_i64, ctypes.c_int, _c_ptr, _c_ptr]),
    'pasta_spade_norm':   (ctypes.c_int, [_c_ptr] * 5 + [ctypes.c_int, _c_i64, _c_i64, _c_f32, ctypes.c_int, _c_f32, _c_f32, ctypes.c_int, _c_i64, _c_ptr, _c_ptr]),
    'pasta_spade_norm_bwd': (ctypes.c_int, [_c_ptr] * 7 + [ctypes.c_int, _c_i64, _c_i64, _c_ptr, ctypes.c_int, _c_f32, _c_f32, ctypes.c_int, _c_i64, _c_i64, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'pasta_ada_matrices': (ctypes.c_int, [_c_ptr, _c_ptr, _c_i64, ctypes.c_int, ctypes.c_int, _c_ptr, ctypes.POINTER(AdaConfig)] +
                                         [ctypes.c_int] * 4 + [_c_f32, _c_ptr, _c_ptr, _c_ptr, _c_ptr]),
    'pasta_ada_theta':    (ctypes.c_int, [_c_ptr, _c_i64, ctypes.POINTER(_c_f32), ctypes.POINTER(_c_f32), _c_ptr, _c_ptr]),
    'pasta_color_affine': (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64, _c_i64, ctypes.c_int, _c_ptr]),
    'pasta_ada_grid':     (ctypes.c_int, [_c_ptr, _c_i64, ctypes.c_int, ctypes.c_int, _c_ptr, _c_ptr]),
    'pasta_affine_sample': (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64] + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_affine_sample_adjoint': (ctypes.c_int, [_c_ptr, _c_ptr, _c_ptr, _c_i64] + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_grid_sample':  (ctypes.c_int, [_c_ptr] * 3 + [_c_i64] + [ctypes.c_int] * 7 + [_c_ptr]),
    'pasta_grid_sample_backward_workspace': (_c_i64, [_c_i64] + [ctypes.c_int] * 4),
    'pasta_grid_sample_backward': (ctypes.c_int, [_c_ptr] * 6 + [_c_i64] + [ctypes.c_int] * 7 + [_c_ptr]),
    'pasta_nan_to_num_multi': (ctypes.c_int, [ctypes.POINTER(_c_ptr), ctypes.POINTER(_c_i64), ctypes.c_int, _c_f32, _c_f32, _c_f32, _c_ptr]),
    'pasta_warp_perspective_u8': (ctypes.c_int, [_c_ptr] * 5 + [ctypes.c_int] * 7 + [_c_ptr]),
    'pasta_patch_composite_u8': (ctypes.c_int, [_c_ptr] * 6 + [ctypes.c_int] * 6 + [_c_ptr]),
    'pasta_pose_stickman_u8': (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_palm_mask_u8': (ctypes.c_int, [_c_ptr] * 4 + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_tryon_masks_u8': (ctypes.c_int, [_c_ptr] * 9 + [ctypes.c_int] * 3 + [_c_ptr]),
    'pasta_tryon_assemble': (ctypes.c_int, [_c_ptr] * 11 + [ctypes.POINTER(_c_ptr)] + [ctypes.c_int] * 9 + [_c_ptr]),
    'pasta_tryon_mirror_u8': (ctypes.c_int, [_c_ptr] * 9 + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_tryon_jitter_u8': (ctypes.c_int, [_c_ptr] * 6 + [ctypes.c_int] * 3 + [_c_ptr]),
    'pasta_erase_strokes_u8': (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int] * 2 + [_c_ptr]),
    'pasta_tryon_outfit_masks_u8': (ctypes.c_int, [_c_ptr] * 12 + [ctypes.c_int] * 4 + [_c_ptr]),
    'pasta_patch_composite_eroded_u8': (ctypes.c_int, [_c_ptr] * 6 + [ctypes.c_int] * 7 + [_c_ptr] * 2),
    'pasta_tryon_outfit_assemble': (ctypes.c_int, [_c_ptr] * 9 + [ctypes.POINTER(_c_ptr)] + [ctypes.c_int] * 7 + [_c_ptr]),
    'pasta_images_to_u8': (ctypes.c_int, [_c_ptr] * 2 + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_images_keep_to_u8': (ctypes.c_int, [_c_ptr] * 4 + [ctypes.c_int] * 6 + [_c_ptr]),
    'pasta_photo_paste_mask_u8': (ctypes.c_int, [_c_ptr] * 5 + [ctypes.c_int] + [_c_ptr] + [ctypes.c_int] * 4 + [_c_ptr]),
    'pasta_tryon_train_region_assemble': (ctypes.c_int, [_c_ptr] * 9 + [ctypes.c_int] * 2 + [_c_ptr] * 2 + [ctypes.POINTER(_c_ptr)] +
                                                        [ctypes.c_int] * 9 + [_c_ptr]),
    'pasta_grid_composite_eroded_u8': (ctypes.c_int, [_c_ptr] * 6 + [ctypes.c_int] * 8 + [_c_ptr]),
    'pasta_grid_assemble': (ctypes.c_int, [_c_ptr] * 7 + [ctypes.POINTER(_c_ptr)] + [ctypes.c_int] * 8 + [_c_ptr]),
    'pasta_image_grid_tile_u8': (ctypes.c_int, [_c_ptr] * 2 + [ctypes.c_int] * 10 + [_c_f32, _c_f32, _c_ptr]),
    'pasta_recon_image_stats_workspace': (_c_i64, [ctypes.c_int] * 3),
    'pasta_recon_image_stats': (ctypes.c_int, [_c_ptr] * 5 + [_c_i64] + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_parsing_confusion': (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int] * 6 + [_c_ptr]),
    'pasta_region_image_stats_workspace': (_c_i64, [ctypes.c_int] * 3),
    'pasta_region_image_stats': (ctypes.c_int, [_c_ptr] * 6 + [_c_i64] + [ctypes.c_int] * 9 + [_c_ptr]),
    'pasta_png_filter': (ctypes.c_int, [_c_ptr] * 3 + [ctypes.c_int] * 4 + [_c_ptr]),
    'pasta_png_code_lengths': (ctypes.c_int, [_c_ptr, ctypes.c_int, ctypes.c_int, _c_ptr]),
    'pasta_png_segment_tables': (ctypes.c_int, [_c_ptr, _c_i64, _c_ptr, _c_ptr]),
    'pasta_png_encode': (ctypes.c_int, [_c_ptr] * 4 + [_c_i64] + [ctypes.c_int] * 3 + [_c_ptr]),
    'pasta_ssim_loss_workspace': (_c_i64, [ctypes.c_int] * 3),
    'pasta_ssim_loss': (ctypes.c_int, [_c_ptr] * 5 + [_c_i64] + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_ssim_loss_backward': (ctypes.c_int, [_c_ptr] * 5 + [ctypes.c_int] * 5 + [_c_ptr]),
    'pasta_swap_assemble': (ctypes.c_int, [_c_ptr] * 6 + [ctypes.POINTER(_c_ptr)] + [ctypes.c_int] * 7 + [_c_ptr]),
    'pasta_region_l1_loss_workspace': (_c_i64, [ctypes.c_int] * 2),
    'pasta_region_l1_loss': (ctypes.c_int, [ctypes.POINTER(_c_ptr)] + [_c_ptr] * 7 + [ctypes.POINTER(_c_ptr), _c_ptr, _c_i64] + [ctypes.c_int] * 3 + [_c_ptr]),
    'pasta_region_l1_loss_backward': (ctypes.c_int, [ctypes.POINTER(_c_ptr), _c_ptr, ctypes.POINTER(_c_ptr)] + [ctypes.c_int] * 3 + [_c_ptr]),
    'pasta_contextual_loss_workspace': (_c_i64, [ctypes.c_int] * 3),
    'pasta_contextual_loss': (ctypes.c_int, [_c_ptr] * 6 + [_c_i64] + [ctypes.c_int] * 3 + [_c_f32, _c_ptr]),
    'pasta_contextual_loss_backward': (ctypes.c_int, [_c_ptr] * 8 + [ctypes.c_int] * 3 + [_c_f32, _c_ptr]),
    'pasta_part_geometry': (ctypes.c_int, [_c_ptr] + [ctypes.c_int] * 6 + [_c_ptr] * 8),
    'pasta_fit_people_u8': (ctypes.c_int, [_c_ptr, _c_ptr, _c_i64, _c_ptr, _c_i64, _c_ptr, _c_ptr] + [ctypes.c_int] * 3 + [_c_ptr]),
}

# Entries added to the current ABI after its first release (purely additive, so the version did not move): a library built before
# them (an old PASTA_LIB_AB build) still loads, and the first call of a missing one raises instead of the import.  At 22: the PNG
# encoder's four entries (csrc/png_encode.hip), pasta_images_keep_to_u8 and pasta_photo_paste_mask_u8 (csrc/tryon_pairs.hip), the five
# entries of the input-activation mask (pasta_act_mask: csrc/conv_igemm.hip, csrc/upfirdn2d.hip; pasta_bias_sum_db: csrc/bias_act.hip),
# pasta_tryon_mirror_u8, pasta_tryon_jitter_u8 and pasta_erase_strokes_u8 (csrc/tryon_inputs.hip), the three entries of the SSIM loss
# (csrc/ssim_loss.hip), pasta_swap_assemble (csrc/train_grid.hip), the three entries of the region L1 loss (csrc/region_l1.hip) and the
# three of the contextual loss (csrc/contextual_loss.hip), pasta_part_geometry (csrc/part_geometry.hip) and pasta_fit_people_u8
# (csrc/fit_people.hip).
LATE_ENTRIES = frozenset(['pasta_png_filter', 'pasta_png_code_lengths', 'pasta_png_segment_tables', 'pasta_png_encode',
                          'pasta_images_keep_to_u8', 'pasta_photo_paste_mask_u8', 'pasta_conv2d_masked', 'pasta_conv2d_mask_available', 'pasta_upfirdn2d_masked',
                          'pasta_upfirdn2d_mask_available', 'pasta_bias_sum_db', 'pasta_tryon_mirror_u8',
                          'pasta_tryon_jitter_u8', 'pasta_ssim_loss_workspace', 'pasta_ssim_loss', 'pasta_ssim_loss_backward',
                          'pasta_erase_strokes_u8', 'pasta_swap_assemble', 'pasta_region_l1_loss_workspace', 'pasta_region_l1_loss',
                          'pasta_region_l1_loss_backward', 'pasta_contextual_loss_workspace', 'pasta_contextual_loss',
                          'pasta_contextual_loss_backward', 'pasta_part_geometry', 'pasta_fit_people_u8'])

def _missing_entry(lib_path, name):
    def missing(*args, **kwargs):
        raise RuntimeError('%s has no %s: it predates this tree, rebuild it from this tree' % (lib_path, name))
    missing.pasta_missing = True
    return missing

def has_entry(lib, name):
    """Does the loaded library export the late entry ``name`` (an older PASTA_LIB_AB build may not)?"""
    return not getattr(getattr(lib, name), 'pasta_missing', False)

def get_plugin(module_name='pasta_hip', sources=None, **build_kwargs):
    """Return the loaded library (a ``ctypes.CDLL`` with typed entry points).

    ``sources`` is accepted for signature compatibility with the reference loader and
    ignored: the library always contains every kernel under ``csrc/``."""
    del sources
    with _lock:
        if module_name in _cached_plugins:
            return _cached_plugins[module_name]
        lib_path = build(**build_kwargs)
        # same-box A/B of two builds (tools/ab_lib.sh): PASTA_LIB_AB names another library built from THIS tree with other compile flags
        ab = os.environ.get('PASTA_LIB_AB')
        if ab:
            if not os.path.isfile(ab):
                raise RuntimeError('PASTA_LIB_AB names %r, which does not exist' % ab)
            warnings.warn('PASTA_LIB_AB: loading %s instead of %s (same-box A/B measurement)' % (ab, lib_path))
            lib_path = ab
        lib = ctypes.CDLL(lib_path)
        for name, (restype, argtypes) in ABI.items():
            if name in LATE_ENTRIES and not hasattr(lib, name):
                setattr(lib, name, _missing_entry(lib_path, name))
                continue
            fn = getattr(lib, name)       # AttributeError here = header/library mismatch
            fn.restype = restype
            fn.argtypes = argtypes
        # the structure layouts above (ConvDesc, ConvEpilogue, ...) are those of ONE ABI revision: a library of another one -- a stale A/B
        # build, a copy from another checkout -- would read pointer fields at the wrong offsets
        if lib.pasta_abi_version() != EXPECTED_ABI:
            raise RuntimeError('%s reports ABI %d, this tree expects %d (include/pasta_hip.h): rebuild it from this tree'
                               % (lib_path, lib.pasta_abi_version(), EXPECTED_ABI))
        _cached_plugins[module_name] = lib
        return lib

def check(lib, status):
    """Turn a non-zero status into the RuntimeError the reference's TORCH_CHECK raises."""
    if status != 0:
        raise RuntimeError(lib.pasta_last_error().decode(errors='replace'))

#----------------------------------------------------------------------------
