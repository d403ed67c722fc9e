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
``images_keep_to_u8`` (pasta_images_keep_to_u8: those bytes with the photograph's kept parts pasted in, one launch) over the
region of ``photo_paste_mask`` (pasta_photo_paste_mask_u8: the kept parts, and with --background / --kept-garments photo the
background and the person's own garments where the generator's region heads agree; ``paste_rules`` fills its table).

The host keeps the file decoding (training/dataset.py), the key-point geometry and the 8 x 8 solves of the warps
(patch_pipeline.part_maps; a builder with geometry='gpu': one launch instead).  Key points
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
    per-sample views (the person, the owner of the upper garment, the owner of the lower one) are gathered on the device.
    ``geometry`` = 'host' or 'gpu': where the matrices are solved (patch_pipeline.part_maps: DESIGN 8n)."""

    def __init__(self, device, box_factor=2, geometry='host'):
        self.device = torch.device(device)
        self.box_factor = box_factor
        self.geometry = patch_pipeline.check_geometry(geometry)

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
            garment_img, sticks, garment_mask, shift_keypoints(people_kp, lp), *host_idx, self.box_factor, geometry=self.geometry)
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


# ---- where the photograph may be pasted: kept parts, background, the person's own garments ----

# The label sets of pasta_tryon_outfit_masks_u8 (csrc/tryon_pairs.hip's tryon_pair_masks_kernel): the upper garment, the lower
# garment, and label 6, which belongs to the lower garment as well where a size's SIX_IS_LOWER says so.  paste_rules takes them
# from here, the one statement on the host.
UPPER_LABELS = (5, 6, 7)
LOWER_LABELS = (9, 12)
SHARED_LABEL = 6
# the bits of a rule row, by the generator's statement (include/pasta_hip.h, pasta_photo_paste_mask_u8)
STATE_OTHER, STATE_UPPER, STATE_LOWER, STATE_SKIN = 0, 1, 2, 3
PASTE_SIZES = (256, 512)    # the heights of the two try-on models: 256 x 192 and 512 x 320


def garment_labels(size):
    """(upper labels, lower labels) of the masks entry as the builder of ``size`` (256 or 512, the height) calls it."""
    if size == 256:
        six_is_lower = SIX_IS_LOWER
    elif size == 512:
        from training.tryon_regions import SIX_IS_LOWER as six_is_lower
    else:
        raise ValueError('paste_rules: size %r (one of %s)' % (size, ', '.join(map(str, PASTE_SIZES))))
    return UPPER_LABELS, LOWER_LABELS + ((SHARED_LABEL,) if six_is_lower else ())


def paste_rules(kept_parts, background, kept_garments, person_idx, upper_idx, lower_idx, size):
    """The rule table of ``photo_paste_mask``: uint8 [N, 256] on the host, row n for item n of a batch of ``collate_outfits``
    (``person_idx`` / ``upper_idx`` / ``lower_idx``: whose photograph, upper and lower garment).  Entry [n, L] is the set of the
    generator's statements (bit 0 other, 1 upper, 2 lower, 3 skin) under which label L of the photograph may be pasted:
    ``kept_parts``: every statement at metrics.tryon_fidelity.KEEP_LABELS; ``background``: 'other' at label 0;
    ``kept_garments``: 'upper' at the upper labels of an item that wears its own upper garment, 'lower' at the lower labels of
    one that wears its own lower garment (``garment_labels(size)``; a label in both sets gets both bits)."""
    from metrics.tryon_fidelity import KEEP_LABELS
    upper_labels, lower_labels = garment_labels(size)
    person, upper, lower = (np.asarray(ix, np.int64).reshape(-1) for ix in (person_idx, upper_idx, lower_idx))
    if not person.shape == upper.shape == lower.shape:
        raise ValueError('paste_rules: %d people, %d upper and %d lower garments' % (len(person), len(upper), len(lower)))
    rule = np.zeros([len(person), 256], np.uint8)
    if kept_parts:
        rule[:, list(KEEP_LABELS)] |= 0b1111
    if background:
        rule[:, 0] |= 1 << STATE_OTHER
    if kept_garments:
        for labels, owner, state in ((upper_labels, upper, STATE_UPPER), (lower_labels, lower, STATE_LOWER)):
            own = np.flatnonzero(owner == person)
            rule[np.ix_(own, list(labels))] |= 1 << state
    return torch.from_numpy(rule)


def photo_paste_mask(parsing, palm, rule, heads, c0):
    """Where the photograph is pasted (include/pasta_hip.h, pasta_photo_paste_mask_u8; this project's own rule), one launch:
    ``parsing`` uint8 [N, H, W], the person's labels; ``palm`` uint8 [N, H, Ht] or None; ``rule`` uint8 [N, 256]
    (``paste_rules``); ``heads``: what the synthesis network returned after its images -- () for no statement, one tensor
    [N, 6, Ht, Ht] (the parsing logits of GeneratorFull) or two [N, 1, Ht, Ht] (the sigmoid heads of GeneratorV18), cast to fp32
    here (16-bit storage); ``c0`` = (Ht - W) // 2, the content's first column in the heads and the palm mask.
    -> uint8 [N, H, W], 0 / 1.  Refuses with ValueError."""
    heads = tuple(heads) if isinstance(heads, (tuple, list)) else (heads,)
    named = [('parsing', parsing), ('rule', rule)] + ([('palm', palm)] if palm is not None else []) + [('heads[%d]' % i, h) for i, h in enumerate(heads)]
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.device.type != 'cuda':
            raise ValueError('photo_paste_mask: %s is not a tensor on the GPU (there is no CPU path)' % name)
    if parsing.dtype != torch.uint8 or rule.dtype != torch.uint8 or (palm is not None and palm.dtype != torch.uint8):
        raise ValueError('photo_paste_mask: parsing, palm and rule uint8, not %s, %s, %s'
                         % (parsing.dtype, None if palm is None else palm.dtype, rule.dtype))
    if any(not h.dtype.is_floating_point for h in heads):
        raise ValueError('photo_paste_mask: floating-point heads, not %s' % ', '.join(str(h.dtype) for h in heads))
    if parsing.ndim != 3:
        raise ValueError('photo_paste_mask: parsing [N, H, W], not %s' % (list(parsing.shape),))
    n, h, w = (int(v) for v in parsing.shape)
    c0 = int(c0)
    if len(heads) not in (0, 1, 2) or any(x.ndim != 4 or int(x.shape[1]) != (6, 1)[len(heads) - 1] for x in heads):
        raise ValueError('photo_paste_mask: heads are none, one tensor of 6 planes or two of 1 plane, not %s' % ([list(x.shape) for x in heads],))
    ht = int(palm.shape[2]) if palm is not None and palm.ndim == 3 else int(heads[0].shape[3]) if heads else w + 2 * c0
    if c0 < 0 or ht < w or c0 != (ht - w) // 2:
        raise ValueError('photo_paste_mask: c0 %d for a width of %d in %d columns (their centred position)' % (c0, w, ht))
    if tuple(rule.shape) != (n, 256):
        raise ValueError('photo_paste_mask: rule %s for %d items (one row of 256 per item)' % (list(rule.shape), n))
    if palm is not None and tuple(palm.shape) != (n, h, ht):
        raise ValueError('photo_paste_mask: palm %s for parsing %s (the rows padded to %d)' % (list(palm.shape), list(parsing.shape), ht))
    if h > ht or any(tuple(x.shape) != (n, x.shape[1], ht, ht) for x in heads):
        raise ValueError('photo_paste_mask: heads %s for parsing %s in a square of %d' % ([list(x.shape) for x in heads], list(parsing.shape), ht))
    if any(t.device != parsing.device for _, t in named):
        raise ValueError('photo_paste_mask: tensors on different devices')
    parsing, rule = parsing.contiguous(), rule.contiguous()
    palm = None if palm is None else palm.contiguous()
    heads = [x.to(torch.float32).contiguous() for x in heads]
    a, b = (heads + [None, None])[:2]
    out = torch.empty([n, h, w], dtype=torch.uint8, device=parsing.device)
    with torch.cuda.device(parsing.device):
        _native.check(_native.lib().pasta_photo_paste_mask_u8(_native.ptr(parsing), _native.ptr(palm), _native.ptr(rule), _native.ptr(a),
                                                              _native.ptr(b), (0, 6, 1)[len(heads)], _native.ptr(out), n, h, w, ht,
                                                              _native.stream()))
    return out
