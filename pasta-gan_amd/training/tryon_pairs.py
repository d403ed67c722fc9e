"""A batch of the try-on TEST pairs prepared on the GPU: what the reference's ``UvitonDatasetV19_test._load_raw_image`` /
``normalize`` / ``__getitem__`` (training/dataset.py:1085-1525) and test.py's conversions (test.py:104-117) do per sample on
the host in four loader processes, as a few launches per batch:

    pasta_pose_stickman_u8            the stick figures of the batch's people, thickness 2 and radius 2, one launch
                                      (csrc/tryon_inputs.hip)
    pasta_palm_mask_u8                the person's palm mask, boxes 25 and 15 (csrc/tryon_pairs.hip)
    pasta_tryon_outfit_masks_u8       retain image, the lower garment (labels 6, 9, 12) and the upper garment, a source per garment
    patch_pipeline.normalize_pair_outfit_batch   three forward warps + the eroded composite and the one with a radius per
                                                 sample (csrc/patches.hip, csrc/tryon_pairs.hip)
    pasta_tryon_outfit_assemble       the seven fp32 tensors G takes (its outputs 2..8)

and, after the generator, ``images_to_u8`` (pasta_images_to_u8: the bytes test.py writes) or, with --kept-parts photo,
``images_keep_to_u8`` (pasta_images_keep_to_u8: those bytes with the photograph's kept parts pasted in, one launch).

The host keeps the file decoding (training/dataset.py), the key-point geometry and the 8 x 8 solves of the warps.  Key points
are shifted by the padding in float64 before get_crop's float32 conversion (dataset.py:1100, :1129), so the quadrilaterals are
formed with x_pad = 0 from pre-shifted joints; the palm quadrilaterals add the same float64 shift (tryon_batch.palm_quads).

The implementation is the OUTFIT form, this project's own: a person with the upper garment of one donor and the lower garment of
another (``training.dataset.UvitonOutfits_256_test``, ``collate_outfits``; include/pasta_hip.h lists the rules).  The lower
composite erodes a sample's masks 5 x 5 exactly where the lower garment is somebody else's (pasta_patch_composite_eroded_u8's radii); the
batch's distinct people are uploaded once, drawn once and their matrices solved once.  ``TryOnPairOutfitBatchBuilder`` is that
body; the reference's pair (P, D) is the outfit (P, D, -), and ``TryOnPairBatchBuilder`` is the same body behind
``training.dataset.pairs_batch_as_outfits``.  Lower-body and full-body try-on are (P, -, D) and (P, D, D)."""

import numpy as np
import torch

from torch_utils.ops import _native
from training import patch_pipeline
from training.dataset import pairs_batch_as_outfits
from training.tryon_batch import (OUTFIT_OUTPUTS, STICK_RADIUS, STICK_THICKNESS, allocator, device_tables, output_tensors, shift_keypoints,
                                  upload_images, upload_person)

PALM_BOXES = (25, 15)       # get_hand_mask of the test set: upper arm 25 x 25, forearm 15 x 15 (dataset.py:1240-1253)
SIX_IS_LOWER = 1            # the lower garment is labels 6, 9, 12 (dataset.py:1113)


class TryOnPairBatch:
    """``tensors``: the seven inputs of test.py's generator calls (KEYS); ``person_name`` / ``clothes_name``: the data set's
    relative paths; ``stages``: the uint8 intermediates (and the person's unpadded ``image`` and ``parsing``, which
    metrics.tryon_fidelity scores against) when the builder was asked to keep them.  training.tryon_regions.TryOnRegionBatch is
    this class with the nine KEYS of test_512.py."""
    KEYS = ['retain', 'pose', 'style_input', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask', 'denorm_lower_mask']

    def __init__(self, tensors, person_name, clothes_name, stages=None):
        self.tensors = tensors
        self.batch = int(tensors['retain'].shape[0])
        self.person_name = list(person_name)
        self.clothes_name = list(clothes_name)
        self.stages = stages


class TryOnPairOutfitBatch(TryOnPairBatch):
    """``tensors``: the seven of TryOnPairBatch; ``person_name`` / ``upper_name`` / ``lower_name``: the data set's relative paths
    (``clothes_name`` is ``upper_name``); ``stages`` as TryOnPairBatch's (``clothes_stick`` the upper garment's owner's), with
    ``lower_stick`` and ``upper_valid`` / ``lower_valid`` / ``person_valid`` [N, 10]."""

    def __init__(self, tensors, person_name, upper_name, lower_name, stages=None):
        super().__init__(tensors, person_name, upper_name, stages)
        self.upper_name = self.clothes_name
        self.lower_name = list(lower_name)


class TryOnPairOutfitBatchBuilder:
    """``build(raw_batch)``: a batch of ``training.dataset.collate_outfits`` at 256 x 192 -> TryOnPairOutfitBatch on ``device``.
    The batch's M distinct people are uploaded once, their stick figures drawn once and their matrices solved once; the
    per-sample views (the person, the owner of the upper garment, the owner of the lower one) are gathered on the device."""

    def __init__(self, device, box_factor=2):
        self.device = torch.device(device)
        self.box_factor = box_factor

    def build(self, raw, keep_stages=False):
        dev = self.device
        people_image, people_parsing, people_kp = upload_person(raw, dev, type(self).__name__, 'people_')
        m, H, W, _ = people_image.shape
        lp = (H - W) // 2
        host_idx = [np.asarray(raw[k], np.int64) for k in ('person_idx', 'upper_idx', 'lower_idx')]
        n = len(host_idx[0])
        assert all(ix.shape == (n,) and ix.min() >= 0 and ix.max() < m for ix in host_idx), 'outfit indices outside the people stack'
        person_ix, upper_ix, lower_ix = (torch.from_numpy(ix).to(dev, non_blocking=True) for ix in host_idx)
        (image, parsing), (u_image, u_parsing), (l_image, l_parsing) = (
            (people_image.index_select(0, ix), people_parsing.index_select(0, ix)) for ix in (person_ix, upper_ix, lower_ix))
        limbs, joints, quads, present = device_tables(people_kp, people_kp[host_idx[0]], lp, dev)      # M stick figures, N palms
        u8 = allocator(torch.uint8, dev)
        sticks, palm, retain_img = u8(m, H, H, 3), u8(n, H, H), u8(n, H, H, 3)
        garment_img, garment_mask = u8(2 * n, H, H, 3), u8(2 * n, H, H, 3)   # the upper garments, then the lower garments
        lib, P = _native.lib(), _native.ptr
        with torch.cuda.device(dev):
            s = _native.stream()
            _native.check(lib.pasta_pose_stickman_u8(P(limbs), P(joints), P(sticks), m, H, W, STICK_THICKNESS, STICK_RADIUS, s))
            _native.check(lib.pasta_palm_mask_u8(P(parsing), P(quads), P(present), P(palm), n, H, W, *PALM_BOXES, s))
            _native.check(lib.pasta_tryon_outfit_masks_u8(P(image), P(parsing), P(palm), P(u_image), P(u_parsing), P(l_image), P(l_parsing),
                                                          P(retain_img), P(garment_img[:n]), P(garment_mask[:n]), P(garment_img[n:]),
                                                          P(garment_mask[n:]), n, H, W, SIX_IS_LOWER, s))
        patches, stick_patches, mask_patches, den_u, den_l, m_invs, valid_u, valid_l, valid_p = patch_pipeline.normalize_pair_outfit_batch(
            garment_img, sticks, garment_mask, shift_keypoints(people_kp, lp), *host_idx, self.box_factor)
        stick = sticks.index_select(0, person_ix)
        parts, ph, pw = patches.shape[1], patches.shape[2], patches.shape[3]
        t, outs = output_tensors(TryOnPairOutfitBatch.KEYS, n, H, (6 * parts, ph, pw), dev, OUTFIT_OUTPUTS)
        with torch.cuda.device(dev):             # no image / clothes tensors, so no photographs; the stick patches are the second list
            _native.check(lib.pasta_tryon_outfit_assemble(None, None, None, P(retain_img), P(stick), P(patches), P(stick_patches), P(den_u),
                                                          P(den_l), outs, n, H, W, parts, parts, ph, pw, _native.stream()))
        stages = None
        if keep_stages:
            stages = dict(image=image, parsing=parsing, stick=stick, clothes_stick=sticks.index_select(0, upper_ix),
                          lower_stick=sticks.index_select(0, lower_ix), palm=palm, retain_img=retain_img, lower_img=garment_img[n:],
                          lower_mask=garment_mask[n:], upper_img=garment_img[:n], upper_mask=garment_mask[:n], patches=patches,
                          stick_patches=stick_patches, mask_patches=mask_patches, denorm_upper=den_u, denorm_lower=den_l, M_invs=m_invs,
                          upper_valid=valid_u, lower_valid=valid_l, person_valid=valid_p)
        return TryOnPairOutfitBatch(t, raw['person_name'], raw['upper_name'], raw['lower_name'], stages)


class TryOnPairBatchBuilder(TryOnPairOutfitBatchBuilder):
    """``build(raw_batch)``: a batch of ``training.dataset.collate_pairs`` -> TryOnPairBatch on ``device``: the pairs as the
    upper-body outfits (P, D, -), stacked on the device after the upload.  Its stages are the reference's eighteen: the person is
    the owner of the lower garment, so ``lower_stick`` is ``stick`` and ``person_valid`` is ``lower_valid``."""

    def build(self, raw, keep_stages=False):
        batch = super().build(pairs_batch_as_outfits(upload_images(raw, self.device), 'upperbody'), keep_stages)
        if keep_stages:
            del batch.stages['lower_stick'], batch.stages['person_valid']
        return TryOnPairBatch(batch.tensors, raw['person_name'], raw['clothes_name'], batch.stages)


def images_to_u8(images, c0, width):
    """test.py:133-137 on the GPU: fp32 [N, 3, H, Wt] in [-1, 1] -> uint8 [N, H, width, 3] (RGB) of columns c0 .. c0 + width - 1:
    (x + 1) * 127.5 rounded per operation, clipped to [0, 255], truncated; a NaN becomes 0."""
    _native.require_gpu(images, 'images_to_u8')
    assert images.dtype == torch.float32 and images.ndim == 4 and images.shape[1] == 3
    images = images.contiguous()
    n, _, h, wt = images.shape
    out = torch.empty([n, h, width, 3], dtype=torch.uint8, device=images.device)
    with torch.cuda.device(images.device):
        _native.check(_native.lib().pasta_images_to_u8(_native.ptr(images), _native.ptr(out), n, h, wt, c0, width, _native.stream()))
    return out


KEEP_MAX_RADIUS = 8         # the largest feather of images_keep_to_u8: a 17 x 17 window (csrc/tryon_pairs.hip's KC_MAX_R)


def images_keep_to_u8(images, c0, width, photo, keep, radius):
    """``images_to_u8`` with the photograph's kept parts pasted in, in the same launch (include/pasta_hip.h,
    pasta_images_keep_to_u8; this project's own rule): fp32 [N, 3, H, Wt], ``photo`` uint8 [N, H, width, 3], ``keep`` uint8
    [N, H, width] (non-zero: kept, metrics.tryon_fidelity.keep_mask) -> uint8 [N, H, width, 3].  Where the whole
    (2 radius + 1)^2 window round a kept pixel is kept (or outside the image) the byte is the photograph's, outside the kept
    region it is ``images_to_u8``'s, in between a weighted mean of the two; radius 0 is a hard paste.  Refuses with ValueError."""
    for name, t in (('images', images), ('photo', photo), ('keep', keep)):
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise ValueError('images_keep_to_u8: %s is not a tensor on the GPU (there is no CPU path)' % name)
    if images.dtype != torch.float32 or photo.dtype != torch.uint8 or keep.dtype != torch.uint8:
        raise ValueError('images_keep_to_u8: images fp32, photo and keep uint8, not %s, %s, %s' % (images.dtype, photo.dtype, keep.dtype))
    if images.ndim != 4 or images.shape[1] != 3:
        raise ValueError('images_keep_to_u8: images [N, 3, H, Wt], not %s' % (list(images.shape),))
    n, _, h, wt = images.shape
    c0, width = int(c0), int(width)
    if width < 1 or c0 < 0 or c0 + width > wt:
        raise ValueError('images_keep_to_u8: columns %d + %d of %d' % (c0, width, wt))
    if tuple(photo.shape) != (n, h, width, 3) or tuple(keep.shape) != (n, h, width):
        raise ValueError('images_keep_to_u8: photo %s and keep %s for images %s and width %d'
                         % (list(photo.shape), list(keep.shape), list(images.shape), width))
    if photo.device != images.device or keep.device != images.device:
        raise ValueError('images_keep_to_u8: tensors on different devices')
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= KEEP_MAX_RADIUS:
        raise ValueError('images_keep_to_u8: radius %r (an integer 0..%d)' % (radius, KEEP_MAX_RADIUS))
    images, photo, keep = images.contiguous(), photo.contiguous(), keep.contiguous()
    out = torch.empty([n, h, width, 3], dtype=torch.uint8, device=images.device)
    with torch.cuda.device(images.device):
        _native.check(_native.lib().pasta_images_keep_to_u8(_native.ptr(images), _native.ptr(photo), _native.ptr(keep), _native.ptr(out), n, h,
                                                            wt, c0, width, radius, _native.stream()))
    return out
