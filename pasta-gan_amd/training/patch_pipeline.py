"""Body-part patch pipeline of the data loader on the GPU (reference training/dataset.py:751-836 ``get_crop`` and :838-927
``normalize``), batched: the reference warps ten body-part quadrilaterals of every sample into (W/4) x (H/4) patches, warps
them back and composites them where the warped garment mask is 255 -- about 28 ``cv2.warpPerspective`` calls per sample on the
host (the reason the reference's loader, not its networks, bounds real-data throughput).  Here the ten (or
fourteen) forward warps of a whole batch are ONE launch of ``pasta_warp_perspective_u8`` per source tensor and the warp-back
+ mask test + compositing of all parts one launch of ``pasta_patch_composite_u8`` per garment.

The projective matrices are 8 x 8 solves on eighteen key points -- host work, numpy float64, as in the reference -- or, with
``geometry='gpu'``, ONE launch of ``pasta_part_geometry`` per batch (part_geometry below): a second, documented rule.
Either way every consumer takes one form, PartMaps: the INVERTED maps and the flags on the device, made once per batch by
``part_maps``; host matrices handed to a launch wrapper are converted at its entry by ``on_device``.  Image
tensors stay uint8 HWC as the reference's arrays.  Numerics: OpenCV's fixed-point bilinear interpolation restated from its
published algorithm (csrc/patches.hip); OpenCV is not installed here, so parity with cv2 is UNPINNED;
the kernels are held bit for bit to oracle/ref_patches.py in tests/test_patches_gpu.py."""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from torch_utils.ops import _native

# dataset.py:846-861
BODY_PARTS = (('lshoulder', 'lhip', 'rhip', 'rshoulder'), ('lshoulder', 'rshoulder', 'cnose'), ('lshoulder', 'lelbow'), ('lelbow', 'lwrist'),
              ('rshoulder', 'relbow'), ('relbow', 'rwrist'), ('lhip', 'lknee'), ('lknee', 'lankle'), ('rhip', 'rknee'), ('rknee', 'rankle'))
JOINT_ORDER = ('cnose', 'cneck', 'rshoulder', 'relbow', 'rwrist', 'lshoulder', 'lelbow', 'lwrist', 'rhip', 'rknee', 'rankle', 'lhip', 'lknee',
               'lankle', 'reye', 'leye', 'rear', 'lear')
_JOINT = {name: i for i, name in enumerate(JOINT_ORDER)}
LOWER_FROM = 6              # parts 6..9 (the legs) are also cut from the lower garment (dataset.py:890)
ARM_PARTS = (2, 3, 4, 5)    # whose warped-back masks the reference returns as denorm_hand_masks (:906-910)


def _seen(joints, names):
    return all(joints[_JOINT[n], 2] >= 0.1 for n in names)              # dataset.py:748-749


def _box_around(p, q, half_width_ratio):
    """Rectangle around the segment p -> q, ``half_width_ratio`` of its length to either side (corner order of dataset.py:821-829)."""
    seg = q - p
    normal = np.array([-seg[1], seg[0]], dtype=seg.dtype) * half_width_ratio
    return np.float32([p + normal, p - normal, q - normal, q + normal])


def part_quadrilateral(joints, part, image_height, aspect=0.5, x_pad=32, shin_fallback=False):
    """Source quadrilateral [4, 2] float32 of one body part, or None when its key points are missing (dataset.py:751-829).
    ``joints`` [18, 3] = (x, y, confidence) in the unpadded 192-wide image; ``x_pad`` shifts into the padded square.
    ``shin_fallback``: a shin without its ankle goes straight down from the knee, as the test set's get_crop does (:1355-1362;
    the training set's has it commented out)."""
    names = list(part)
    if not _seen(joints, names):
        if names[0] in ('lhip', 'rhip') and names[1] in ('lknee', 'rknee') and names[0][0] == names[1][0]:
            names = names[:1]                                   # thigh without its knee: straight down from the hip
        elif shin_fallback and names[0] in ('lknee', 'rknee') and names[1] in ('lankle', 'rankle') and names[0][0] == names[1][0]:
            names = names[:1]                                   # shin without its ankle: straight down from the knee
        elif names == ['lshoulder', 'rshoulder', 'cnose']:
            names = ['lshoulder', 'rshoulder', 'rshoulder']     # head without the nose: a square above the shoulders
        if not _seen(joints, names):
            return None
    pts = np.float32([[joints[_JOINT[n], 0], joints[_JOINT[n], 1]] for n in names])
    pts[:, 0] = pts[:, 0] + x_pad                       # in float32, after the conversion (dataset.py:780)
    if len(pts) == 4:
        return pts
    if len(pts) == 1:
        return _box_around(pts[0], np.float32([pts[0][0], image_height - 1]), aspect / 2.0)
    if len(pts) == 2:
        return _box_around(pts[0], pts[1], aspect / 2.0)
    if names[2] == 'rshoulder':
        seg = pts[1] - pts[0]
        normal = np.array([-seg[1], seg[0]])
        if normal[1] > 0.0:
            normal = -normal
        return np.float32([pts[0] + normal, pts[0], pts[1], pts[1] + normal])
    neck = 0.5 * (pts[0] + pts[1])
    top = np.float32(neck + 2 * (pts[2] - neck))
    a, b, c, d = _box_around(top, np.float32(neck), 0.5)
    return np.float32([b, c, d, a])


def perspective_matrix(src, dst):
    """3 x 3 float64 map taking the four ``src`` points onto the four ``dst`` points (cv2.getPerspectiveTransform's system)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    rows, rhs = [], []
    for (x, y), (u, v) in zip(src, dst):
        rows.append([x, y, 1, 0, 0, 0, -x * u, -y * u])
        rhs.append(u)
    for (x, y), (u, v) in zip(src, dst):
        rows.append([0, 0, 0, x, y, 1, -x * v, -y * v])
        rhs.append(v)
    try:
        h = np.linalg.solve(np.array(rows), np.array(rhs))
    except np.linalg.LinAlgError:
        h = np.zeros(8)
    return np.append(h, 1.0).reshape(3, 3)


def adjugate_inverse(m):
    """Inverses of 3 x 3 float64 matrices [..., 3, 3] by cofactors (what cv2.warpPerspective applies to its argument), all of them in
    one pass; zeros where singular."""
    m = np.asarray(m, np.float64)
    m00, m01, m02, m10, m11, m12, m20, m21, m22 = (m[..., i, j] for i in range(3) for j in range(3))
    with np.errstate(all='ignore'):
        c = np.stack([m11 * m22 - m12 * m21, m02 * m21 - m01 * m22, m01 * m12 - m02 * m11,
                      m12 * m20 - m10 * m22, m00 * m22 - m02 * m20, m02 * m10 - m00 * m12,
                      m10 * m21 - m11 * m20, m01 * m20 - m00 * m21, m00 * m11 - m01 * m10], axis=-1)
        det = m00 * (m11 * m22 - m12 * m21) - m01 * (m10 * m22 - m12 * m20) + m02 * (m10 * m21 - m11 * m20)
        det = det[..., None]
        return np.where(det != 0, c * (1.0 / det), 0.0).reshape(m.shape)


def part_matrices(joints, width, height, box_factor=2, x_pad=32, shin_fallback=False):
    """For a batch of key points [N, 18, 3]: (M [N,10,3,3], M_inv [N,10,3,3], valid [N,10]) float64 / bool -- image -> patch and
    patch -> image maps of the ten parts (dataset.py:831-836); zeros where a part is missing.  ``x_pad`` and ``shin_fallback``
    go to part_quadrilateral (the test set passes key points already shifted in float64, x_pad = 0, and its fall-back)."""
    joints = np.asarray(joints, np.float64)
    n = joints.shape[0]
    pw, ph = width // 2 ** box_factor, height // 2 ** box_factor
    corners = np.float32([[0, 0], [0, ph], [pw, ph], [pw, 0]])
    fwd, back, valid = np.zeros([n, 10, 3, 3]), np.zeros([n, 10, 3, 3]), np.zeros([n, 10], bool)
    for i in range(n):
        for k, part in enumerate(BODY_PARTS):
            quad = part_quadrilateral(joints[i], part, height, x_pad=x_pad, shin_fallback=shin_fallback)
            if quad is not None:
                fwd[i, k], back[i, k], valid[i, k] = perspective_matrix(quad, corners), perspective_matrix(corners, quad), True
    return fwd, back, valid


GEOMETRIES = ('host', 'gpu')
GEOMETRY_OUTPUTS = ('quads', 'fwd', 'back', 'fwd_inv', 'back_inv', 'm_inv', 'valid')       # pasta_part_geometry's, in its order


def check_geometry(geometry):
    if geometry not in GEOMETRIES:
        raise ValueError('part geometry %r is invalid (one of %s).' % (geometry, ', '.join(GEOMETRIES)))
    return geometry


def part_geometry(joints, width, height, box_factor=2, x_pad=32, shin_fallback=False, device='cuda', outputs=GEOMETRY_OUTPUTS):
    """part_matrices and the inverses the warps take, on the GPU in one launch (csrc/part_geometry.hip; include/pasta_hip.h states
    the rule): ``joints`` [M, 18, 3] (host, uploaded once, or a float64 tensor already on ``device``) -> dict of device tensors
    ``quads`` float32 [M,10,4,2], ``fwd`` / ``back`` / ``fwd_inv`` / ``back_inv`` float64 [M,10,9], ``m_inv`` float32 [M,10,9]
    (``back`` cast, zeros where invalid: the M_invs tensor) and ``valid`` uint8 [M,10]; ``outputs`` names the ones wanted.  Nothing
    is read back."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('part_geometry needs a GPU device (there is no CPU path), not %s' % dev)
    unknown = [k for k in outputs if k not in GEOMETRY_OUTPUTS]
    if unknown:
        raise ValueError('part_geometry: unknown output %s' % ', '.join(unknown))
    if isinstance(joints, torch.Tensor):
        kp = joints.to(dev, torch.float64).contiguous()
    else:
        kp = torch.from_numpy(np.ascontiguousarray(joints, dtype=np.float64)).to(dev, non_blocking=True)
    assert kp.ndim == 3 and kp.shape[1:] == (18, 3), 'key points [M, 18, 3]'
    m = int(kp.shape[0])
    shapes = dict(quads=([m, 10, 4, 2], torch.float32), m_inv=([m, 10, 9], torch.float32), valid=([m, 10], torch.uint8))
    shaped = lambda size, dtype: torch.empty(size, dtype=dtype, device=dev)
    out = {k: shaped(*shapes.get(k, ([m, 10, 9], torch.float64))) for k in outputs}
    if m == 0:
        return out
    pw, ph = width // 2 ** box_factor, height // 2 ** box_factor
    with torch.cuda.device(dev):
        _native.check(_native.lib().pasta_part_geometry(_native.ptr(kp), m, int(height), pw, ph, int(x_pad), 1 if shin_fallback else 0,
                                                        *[_native.ptr(out.get(k)) for k in GEOMETRY_OUTPUTS], _native.stream()))
    return out


_PART_JOINTS = [[_JOINT[name] for name in part] for part in BODY_PARTS]


def part_valid(joints, shin_fallback=False):
    """bool [N, 10]: part_matrices' valid flags for key points [N, 18, 3], the _seen / fall-back rule of part_quadrilateral
    vectorised -- no solve (the builders' upper_valid / lower_valid / person_valid under ``geometry='gpu'``)."""
    seen = np.asarray(joints, np.float64)[..., 2] >= 0.1                                # [N, 18]
    first = np.stack([seen[:, j[0]] for j in _PART_JOINTS], axis=1)
    everything = np.stack([seen[:, j].all(axis=1) for j in _PART_JOINTS], axis=1)
    valid = everything.copy()
    valid[:, 1] = seen[:, _JOINT['lshoulder']] & seen[:, _JOINT['rshoulder']]          # head without the nose
    alone = [6, 8] + ([7, 9] if shin_fallback else [])                                  # thigh without knee, shin without ankle
    valid[:, alone] = first[:, alone]
    return valid


def _u8(t):
    assert t.dtype == torch.uint8 and t.is_cuda and t.ndim == 4 and t.shape[-1] == 3, 'uint8 [N, H, W, 3] tensors on the GPU'
    return t.contiguous()


class PartMaps(NamedTuple):
    """The body-part maps of M people, the one form every consumer takes, whoever solved them."""
    fwd_inv: torch.Tensor       # float64 [M, 10, 9] on the device: what the forward warp launches take (the image -> patch maps, inverted)
    back_inv: torch.Tensor      # float64 [M, 10, 9] on the device: what the composites take (the patch -> image maps, inverted)
    valid: torch.Tensor         # uint8 [M, 10] on the device: the part flags
    m_invs: torch.Tensor        # float32 [M, 10, 3, 3]: the patch -> image maps cast, zeros where invalid (the M_invs tensor); a host
                                # tensor under 'host', a device tensor under 'gpu'
    flags: np.ndarray           # bool [M, 10] on the host: what upper_valid / lower_valid / person_valid are cut from


def host_part_maps(joints, width, height, box_factor=2, x_pad=32, shin_fallback=False):
    """PartMaps' five fields as numpy arrays, no GPU: ONE part_matrices call for the M people and one batched inverse each of
    their forward and back maps."""
    fwd, back, flags = part_matrices(joints, width, height, box_factor, x_pad, shin_fallback)
    m = len(flags)
    return PartMaps(adjugate_inverse(fwd).reshape(m, 10, 9), adjugate_inverse(back).reshape(m, 10, 9), flags.astype(np.uint8),
                    np.where(flags[..., None, None], back, 0.0).astype(np.float32), flags)


def part_maps(joints, width, height, box_factor=2, x_pad=32, shin_fallback=False, device='cuda', geometry='host'):
    """PartMaps of the people ``joints`` [M, 18, 3] (host) on ``device``.  ``geometry='host'``: host_part_maps and three uploads;
    ``'gpu'``: part_geometry's one launch, nothing solved or inverted in Python, the host flags from part_valid."""
    dev = torch.device(device)
    if check_geometry(geometry) == 'gpu':
        g = part_geometry(joints, width, height, box_factor, x_pad, shin_fallback, dev, ('fwd_inv', 'back_inv', 'm_inv', 'valid'))
        return PartMaps(g['fwd_inv'], g['back_inv'], g['valid'], g['m_inv'].reshape(-1, 10, 3, 3), part_valid(joints, shin_fallback))
    h = host_part_maps(joints, width, height, box_factor, x_pad, shin_fallback)
    return PartMaps(*[torch.from_numpy(a).to(dev) for a in h[:3]], torch.from_numpy(h.m_invs), h.flags)


def on_device(t, dtype, dev, shape=None, invert=False):
    """An argument of a launch, the ONE place host arguments are converted: a tensor already on the device is checked (device, dtype,
    ``shape``) and made contiguous; a host array is cast and uploaded.  ``invert``: host 3 x 3 float64 matrices [..., 3, 3], inverted
    here, all at once, into the [..., 9] the kernels read -- a device tensor is taken as inverted already."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = np.asarray(t, torch.empty(0, dtype=dtype).numpy().dtype)
        if invert:
            t = adjugate_inverse(t).reshape(*t.shape[:-2], 9)
        t = torch.from_numpy(np.ascontiguousarray(t)).to(dev)
    assert t.device == dev and t.dtype == dtype and (shape is None or t.shape == tuple(shape)), \
        'a %s tensor %s on %s, not %s %s on %s' % (dtype, shape, dev, t.dtype, list(t.shape), t.device)
    return t.contiguous()


def _upload(table, dtype, dev):
    return torch.from_numpy(np.ascontiguousarray(table, dtype=dtype)).to(dev, non_blocking=True)


def warp_perspective(src, matrices, out_hw, border='constant', src_index=None, valid=None):
    """Batched ``cv2.warpPerspective(src[i], M, (w, h), borderMode=...)`` for uint8 [*, H, W, C] GPU tensors: ``matrices``
    [B, 3, 3] float64 on the host, or the INVERTED ones [B, 9] float64 already on the device (PartMaps' ``fwd_inv``); one output
    per matrix.  ``src_index`` [B] int32 picks the source of each (default: i) and ``valid`` [B] uint8 flags it; host or device."""
    _native.require_gpu(src, 'warp_perspective')
    dev = src.device
    b = int(len(matrices))
    inv_t = on_device(matrices, torch.float64, dev, (b, 9), invert=True)
    idx_t, val_t = on_device(src_index, torch.int32, dev, (b,)), on_device(valid, torch.uint8, dev, (b,))
    oh, ow = out_hw
    dst = torch.empty([b, oh, ow, src.shape[-1]], dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().pasta_warp_perspective_u8(_native.ptr(src), _native.ptr(idx_t), _native.ptr(inv_t), _native.ptr(val_t),
                                                              _native.ptr(dst), b, int(src.shape[1]), int(src.shape[2]), oh, ow,
                                                              int(src.shape[-1]), 1 if border == 'replicate' else 0, _native.stream()))
    return dst


def inverse_maps(back, parts):
    """[n * p, 9] float64: the inverse cv2.warpPerspective applies to ``back[i, k]`` for every sample i and every k of ``parts``,
    sample-major."""
    return np.ascontiguousarray(adjugate_inverse(np.asarray(back)[:, list(parts)]).reshape(-1, 9))


MAX_ERODE_RADIUS = 8        # ER_MAX_R of csrc/patch_erode.h: the halo its LDS tiles hold


def composite(patches, masks, back, valid, parts, height, width, radius=None, want_part_masks=False):
    """patch -> image (BORDER_CONSTANT) + mask test + compositing of ``patches`` / ``masks`` [N, p, h, w, 3] in order, one launch:
    index j is part ``parts[j]`` of ``back`` / ``valid``, the maps of the people the result is drawn on: PartMaps' ``back_inv``
    [N, 10, 9] float64 and ``valid`` [N, 10] uint8 on the device, or the host's ``back`` [N, 10, 3, 3] and flags [N, 10], converted
    on entry; the parts are gathered on the device.
    ``radius`` None: pasta_patch_composite_u8, the mask tested as warped; a value: pasta_patch_composite_eroded_u8, the mask eroded
    (2 * radius + 1) square first; a sequence [N]: the same entry with its ``radii``, sample i eroded by ``radius[i]`` (0: as warped),
    still one launch.  A radius outside 0 .. 8 raises ValueError.  Returns (image uint8 [N, height, width, 3], part masks uint8
    [N, p, height, width] or None)."""
    n, p, ph, pw = patches.shape[:4]
    dev = patches.device
    lib = _native.lib()
    if radius is None:
        entry, extra = lib.pasta_patch_composite_u8, ()
    elif np.ndim(radius) == 0:
        entry, extra = lib.pasta_patch_composite_eroded_u8, (radius, None)
    else:
        radii = np.asarray(radius).reshape(-1)
        if radii.shape != (n,):
            raise ValueError('composite: %d radii for %d samples' % (len(radii), n))
        bad = np.flatnonzero((radii < 0) | (radii > MAX_ERODE_RADIUS))
        if len(bad):
            raise ValueError('composite: radius %d of sample %d (0..%d)' % (radii[bad[0]], bad[0], MAX_ERODE_RADIUS))
        radius_t = torch.from_numpy(radii.astype(np.uint8)).to(dev)       # held until the launch is queued
        entry, extra = lib.pasta_patch_composite_eroded_u8, (0, _native.ptr(radius_t))
    back = on_device(back, torch.float64, dev, invert=True)
    assert back.ndim == 3 and back.shape[0] == n and back.shape[2] == 9 and len(parts) == p and 0 <= min(parts) and max(parts) < back.shape[1]
    valid = on_device(valid, torch.uint8, dev, back.shape[:2])
    parts_t = torch.as_tensor(np.asarray(parts, np.int64), device=dev)
    inv_t, val_t = back.index_select(1, parts_t).contiguous(), valid.index_select(1, parts_t).contiguous()
    out = torch.empty([n, height, width, 3], dtype=torch.uint8, device=dev)
    pm = torch.empty([n, p, height, width], dtype=torch.uint8, device=dev) if want_part_masks else None
    patches, masks = patches.contiguous(), masks.contiguous()             # held until the launch is queued
    with torch.cuda.device(dev):
        _native.check(entry(_native.ptr(patches), _native.ptr(masks), _native.ptr(inv_t), _native.ptr(val_t), _native.ptr(out), _native.ptr(pm),
                            n, p, ph, pw, height, width, *extra, _native.stream()))
    return out, pm


def normalize_batch(upper_img, lower_img, upper_mask, lower_mask, joints, box_factor=2, want_matrices=False, geometry='host'):
    """``normalize`` (dataset.py:838-927) for a batch on the GPU.  Images and 3-channel masks: uint8 [N, H, W, 3] CUDA tensors;
    ``joints`` [N, 18, 3] (host).  Returns the reference's tuple, batched:
    (norm_img [N,h,w,30], norm_img_lower [N,h,w,12], denorm_upper [N,H,W,3], denorm_lower [N,H,W,3], M_invs [N,10,3,3] float32,
     denorm_hand_masks [N,4,H,W,1], clothes_masks [N,h,w,30], clothes_masks_lower [N,h,w,12]).  M_invs is PartMaps' ``m_invs``: a
    host tensor under ``geometry='host'``, a device tensor under ``'gpu'``.  ``want_matrices``: two more values, PartMaps' device
    ``back_inv`` [N,10,9] float64 and ``valid`` [N,10] uint8 (training/swap_outfits.py warps a batch-mate's patches back with them
    instead of solving the people again)."""
    upper_img, lower_img, upper_mask, lower_mask = _u8(upper_img), _u8(lower_img), _u8(upper_mask), _u8(lower_mask)
    n, height, width, _ = upper_img.shape
    ph, pw = height // 2 ** box_factor, width // 2 ** box_factor
    dev = upper_img.device
    maps = part_maps(joints, width, height, box_factor, device=dev, geometry=geometry)
    sample = _upload(np.repeat(np.arange(n), 10), np.int32, dev).reshape(n, 10)

    def cut(t, which):                  # [n, 10, ...] -> the items of a forward launch, flat
        t = t if which == 'all' else t[:, LOWER_FROM:]
        return t.reshape(-1, *t.shape[2:])
    # image -> patch (BORDER_REPLICATE): all ten parts of every sample in one launch per source tensor
    warp = lambda src, which: warp_perspective(src, cut(maps.fwd_inv, which), (ph, pw), 'replicate', cut(sample, which), cut(maps.valid, which))
    p_img = warp(upper_img, 'all').reshape(n, 10, ph, pw, 3)
    p_mask = warp(upper_mask, 'all').reshape(n, 10, ph, pw, 3)
    p_img_l = warp(lower_img, 'legs').reshape(n, 10 - LOWER_FROM, ph, pw, 3)
    p_mask_l = warp(lower_mask, 'legs').reshape(n, 10 - LOWER_FROM, ph, pw, 3)

    # patch -> image + mask test + compositing, all parts in order, one launch per garment
    den_u, part_masks = composite(p_img, p_mask, maps.back_inv, maps.valid, list(range(10)), height, width, want_part_masks=True)
    den_l, _ = composite(p_img_l, p_mask_l, maps.back_inv, maps.valid, list(range(LOWER_FROM, 10)), height, width)
    hwc = lambda t: t.permute(0, 2, 3, 1, 4).reshape(n, ph, pw, -1)            # parts concatenated along the channel axis (:918-921)
    hand_masks = part_masks[:, list(ARM_PARTS)].unsqueeze(-1)
    out = (hwc(p_img), hwc(p_img_l), den_u, den_l, maps.m_invs, hand_masks, hwc(p_mask), hwc(p_mask_l))
    return out + (maps.back_inv, maps.valid) if want_matrices else out


def _gathered(maps, items, person_idx, dev):
    """What the outfit normalisers take from the M people's ``maps``, gathered on the device by two tables uploaded once: the forward
    launches' inverse maps and flags by ``items`` (flat: owner * 10 + part) and the PERSONS' maps by ``person_idx``:
    (minv [B, 9], flags [B], back_inv [N, 10, 9], valid [N, 10] uint8, M_invs [N, 10, 3, 3] float32, where ``maps.m_invs`` lives)."""
    m = len(maps.flags)
    assert items.min() >= 0 and items.max() < 10 * m and person_idx.min() >= 0 and person_idx.max() < m, 'an index outside the %d people' % m
    items_t, person_t = _upload(items, np.int64, dev), _upload(person_idx, np.int64, dev)
    return (maps.fwd_inv.reshape(-1, 9).index_select(0, items_t), maps.valid.reshape(-1).index_select(0, items_t),
            maps.back_inv.index_select(0, person_t), maps.valid.index_select(0, person_t),
            maps.m_invs.index_select(0, person_t if maps.m_invs.is_cuda else torch.from_numpy(person_idx)))


UPPER_PARTS = 6             # the test set: parts 0..5 from the clothes donor, 6..9 from the person (dataset.py:1470-1478)
ERODE_RADIUS = 2            # cv2.erode(..., np.ones((5, 5))) of the warped-back masks of parts 0..5 (:1460, :1484-1485)


def normalize_pair_outfit_batch(garment_img, people_stick, garment_mask, people_joints, person_idx, upper_idx, lower_idx, box_factor=2,
                                geometry='host'):
    """The test set's ``normalize`` (dataset.py:1430-1500) for a batch of OUTFITS on the GPU (include/pasta_hip.h lists the
    rules).  ``garment_img`` / ``garment_mask``: uint8 [2N, H, W, 3] CUDA tensors, the N upper garments (image, 3-channel mask)
    followed by the N lower garments.  ``people_stick`` [M, H, W, 3]: the stick figures of the batch's M DISTINCT people;
    ``people_joints`` [M, 18, 3] float64 (host), already shifted by the padding (x_pad = 0 below).  ``person_idx`` /
    ``upper_idx`` / ``lower_idx`` [N]: who sample i is and whose upper and lower garment it wears.
    ONE part_matrices call solves the M people.  Parts 0..5 are cut from the upper garment, its owner's stick figure and its mask
    with the owner's matrices, parts 6..9 from the lower garment's likewise: three forward-warp launches (image, stick figure,
    mask).  All ten parts are warped back with the PERSON's M_inv: parts 0..5 into denorm_upper through the eroded composite,
    parts 6..9 into denorm_lower in one launch whose radius is per sample, 0 (the plain composite) where the person wears their
    own lower garment and ERODE_RADIUS where it is somebody else's.  Returns (patches, stick_patches, mask_patches
    [N,10,h,w,3], denorm_upper, denorm_lower [N,H,W,3], M_invs [N,10,3,3] float32 (the person's; where PartMaps' ``m_invs``
    lives), upper_valid, lower_valid, person_valid [N,10] bool).  ``geometry``: part_maps'; the owner and person tables are
    index_select on the device."""
    garment_img, people_stick, garment_mask = _u8(garment_img), _u8(people_stick), _u8(garment_mask)
    n2, height, width, _ = garment_img.shape
    n = n2 // 2
    assert n2 == 2 * n and garment_mask.shape == garment_img.shape and people_stick.shape[1:] == garment_img.shape[1:]
    person_idx, upper_idx, lower_idx = (np.asarray(ix, np.int64).reshape(n) for ix in (person_idx, upper_idx, lower_idx))
    ph, pw = height // 2 ** box_factor, width // 2 ** box_factor
    dev = garment_img.device
    from_upper = np.arange(10) < UPPER_PARTS
    owner = np.where(from_upper[None, :], upper_idx[:, None], lower_idx[:, None])      # [N, 10]: whose matrices and stick figure part k takes
    maps = part_maps(people_joints, width, height, box_factor, 0, True, dev, geometry)
    minv, valid, back, valid_p, m_invs = _gathered(maps, (owner * 10 + np.arange(10)[None, :]).reshape(-1), person_idx, dev)
    # item (i, k) reads garment i of the upper ones (0..N-1) for k < 6 and of the lower ones (N..2N-1) otherwise
    garment = _upload((np.arange(n)[:, None] + np.where(from_upper, 0, n)[None, :]).reshape(-1), np.int32, dev)
    warp = lambda src, index: warp_perspective(src, minv, (ph, pw), 'replicate', index, valid).reshape(n, 10, ph, pw, 3)
    patches, mask_patches = warp(garment_img, garment), warp(garment_mask, garment)
    stick_patches = warp(people_stick, _upload(owner.reshape(-1), np.int32, dev))

    upper, lower = list(range(UPPER_PARTS)), list(range(UPPER_PARTS, 10))
    den_u, _ = composite(patches[:, upper], mask_patches[:, upper], back, valid_p, upper, height, width, ERODE_RADIUS)
    radius = np.where(lower_idx != person_idx, ERODE_RADIUS, 0)
    den_l, _ = composite(patches[:, lower], mask_patches[:, lower], back, valid_p, lower, height, width, radius)
    return patches, stick_patches, mask_patches, den_u, den_l, m_invs, maps.flags[upper_idx], maps.flags[lower_idx], maps.flags[person_idx]


LOWER_PARTS_512 = (0, 6, 7, 8, 9)       # the 512 x 320 set: the torso and the legs are also cut from the lower garment (dataset.py:2023)


def normalize_outfit_batch(garment_img, garment_mask, people_joints, person_idx, upper_idx, lower_idx, box_factor=2, want_part_masks=False,
                           want_matrices=False, geometry='host'):
    """``normalize_full`` / ``normalize_upper`` / ``normalize_lower`` of the 512 x 320 set (dataset.py:1967-2193) for a batch of
    OUTFITS on the GPU.  ``garment_img`` / ``garment_mask``: uint8 [2N, H, W, 3] CUDA tensors, the N upper garments (image,
    3-channel mask) followed by the N lower garments.  ``people_joints`` [M, 18, 3] float64 (host): the batch's DISTINCT people,
    already shifted by the padding (x_pad = 0); get_crop here has no shin fall-back (:1893-1900).  ``person_idx`` / ``upper_idx``
    / ``lower_idx`` [N]: who sample i is and whose upper and lower garment it wears (a pair with a change region: full body
    (P, D, D), upper body (P, D, P), lower body (P, P, D); a training sample: all three the person).
    ONE part_matrices call solves the M people, whatever the number of samples that use them.  All ten parts of the upper
    garment and parts 0, 6, 7, 8, 9 of the lower one are warped forward with their owner's matrices (one launch for the images,
    one for the masks) and back with the PERSON's M_inv through the eroded composite, every part 5 x 5.  A part whose forward
    matrix is missing is zeros; a part whose M_inv is missing is skipped.  Returns (patches [N,10,h,w,3], patches_lower
    [N,5,h,w,3], mask_patches, mask_patches_lower, denorm_upper, denorm_lower [N,H,W,3], M_invs [N,10,3,3] float32 (the
    person's), upper_valid, lower_valid, person_valid [N,10] bool).  ``want_part_masks``: an eleventh value, the eroded 0 / 1
    masks [N,10,H,W] of the upper composite's parts.  ``want_matrices``: two last values, the PERSONS' device ``back_inv`` [N,10,9]
    float64 and ``valid`` [N,10] uint8 (training/swap_outfits.py).  ``geometry`` and M_invs: as normalize_pair_outfit_batch's."""
    garment_img, garment_mask = _u8(garment_img), _u8(garment_mask)
    n2, height, width, _ = garment_img.shape
    n = n2 // 2
    assert n2 == 2 * n and garment_mask.shape == garment_img.shape
    person_idx, upper_idx, lower_idx = (np.asarray(ix, np.int64).reshape(n) for ix in (person_idx, upper_idx, lower_idx))
    ph, pw = height // 2 ** box_factor, width // 2 ** box_factor
    dev = garment_img.device
    low = list(LOWER_PARTS_512)
    pu, pl = 10, len(low)
    # items: (i, k) of the upper garments, then (i, k) of the lower garments, which read source N + i
    items = np.concatenate([(upper_idx[:, None] * 10 + np.arange(pu)).reshape(-1), (lower_idx[:, None] * 10 + np.asarray(low)).reshape(-1)])
    maps = part_maps(people_joints, width, height, box_factor, 0, False, dev, geometry)
    minv, valid, back, valid_p, m_invs = _gathered(maps, items, person_idx, dev)
    src_index = _upload(np.concatenate([np.repeat(np.arange(n), pu), np.repeat(np.arange(n, 2 * n), pl)]), np.int32, dev)
    warp = lambda src: warp_perspective(src, minv, (ph, pw), 'replicate', src_index, valid)
    split = lambda t: (t[:n * pu].reshape(n, pu, ph, pw, 3), t[n * pu:].reshape(n, pl, ph, pw, 3))
    (patches, patches_l), (mask_patches, mask_patches_l) = split(warp(garment_img)), split(warp(garment_mask))

    den_u, part_masks = composite(patches, mask_patches, back, valid_p, list(range(pu)), height, width, ERODE_RADIUS, want_part_masks)
    den_l, _ = composite(patches_l, mask_patches_l, back, valid_p, low, height, width, ERODE_RADIUS)
    out = (patches, patches_l, mask_patches, mask_patches_l, den_u, den_l, m_invs, maps.flags[upper_idx], maps.flags[lower_idx],
           maps.flags[person_idx])
    out = out + (part_masks,) if want_part_masks else out
    return out + (back, valid_p) if want_matrices else out
