"""A batch of the 512 x 320 try-on pairs with a change region prepared on the GPU: what the reference's
``UvitonDatasetFull_512_test._load_raw_image`` / ``normalize_full`` / ``normalize_upper`` / ``normalize_lower`` /
``__getitem__`` (training/dataset.py:1605-2214) and test_512.py's conversions (test_512.py:115-131) do per sample on the host
in four loader processes, as a few launches per batch:

    pasta_pose_stickman_u8            the person's stick figure, thickness 5 and radius 5   (csrc/tryon_inputs.hip)
    pasta_palm_mask_u8                the person's palm mask on the 512 square, boxes 35 and 20 (csrc/tryon_pairs.hip)
    pasta_tryon_outfit_masks_u8       retain image, upper and lower garment (labels 9, 12), a source per garment
    patch_pipeline.normalize_outfit_batch   two forward warps + two eroded composites (csrc/patches.hip, csrc/tryon_pairs.hip)
    pasta_tryon_outfit_assemble       the nine fp32 tensors of test_512.py (its outputs 0..8)

The host keeps the file decoding (training/dataset.py), the key-point geometry and the 8 x 8 solves of the warps
(patch_pipeline.part_maps; a builder with geometry='gpu': one launch instead).  Key points
are shifted by the padding in float64 before get_crop's float32 conversion (dataset.py:1623, :1660), so the quadrilaterals are
formed with x_pad = 0 from pre-shifted joints; the stick figure is drawn from the unshifted ones (:1621).

The implementation is the OUTFIT form, this project's own: a person with the upper garment of one donor and the lower garment of
another (``training.dataset.UvitonOutfits_512_test``, ``collate_outfits``).  The batch's distinct people are uploaded once and
``patch_pipeline.normalize_outfit_batch`` solves their matrices once.  ``TryOnOutfitBatchBuilder`` is that body, with
``clothes_lower`` as a tenth tensor.  A pair with a change region is the outfit (P, D, D), (P, D, P)
or (P, P, D), and ``TryOnRegionBatchBuilder`` is the same body behind ``training.dataset.pairs_batch_as_outfits``, told whose
photograph ``clothes`` is.

``FullBodyRegionBatchBuilder`` prepares TRAINING batches at 512 x 320 (``training.dataset.UvitonDatasetFull_512``).  The
reference has no 512 training set, so the rule is this project's own: the generator is trained on exactly the inputs
test_512.py will later feed it.  A sample is the full-body preparation above of the pair (person, person), plus the 256
training set's photograph as target, ``gt_parsing`` and erase mask (include/pasta_hip.h lists the rules):

    pasta_fit_people_u8                   the people of a packed ``fit`` batch on their canvas (training/tryon_batch.py, fit_batch)
    pasta_tryon_mirror_u8                 the mirrored people of a ``mirror_people`` batch (training/tryon_batch.py, mirror_batch)
    pasta_tryon_jitter_u8                 the jittered people of a numbered batch (training/tryon_batch.py, jitter_batch)
    pasta_erase_strokes_u8                the drawn erase masks of a batch with ``erase_strokes`` (training/tryon_batch.py, strokes_batch)
    pasta_pose_stickman_u8, pasta_palm_mask_u8     as above
    pasta_tryon_masks_u8                  retain mask, gt_parsing and the person's own two garments in one pass, the 256 set's entry
    patch_pipeline.normalize_outfit_batch everyone their own donor: N solves; the eroded part masks of the upper composite kept
    pasta_tryon_train_region_assemble     the erase mask and the nine fp32 tensors of FullBodyBatch.KEYS"""

import numpy as np
import torch

from torch_utils.ops import _native
from training import patch_pipeline
from training.dataset import pairs_batch_as_outfits
from training.swap_outfits import attach as attach_swap
from training.tryon_batch import (OUTFIT_OUTPUTS, FullBodyBatch, allocator, device_tables, jitter_batch, mirror_batch, output_tensors, shift_keypoints,
                                  strokes_batch, upload_erase, upload_images, upload_person)
from training.tryon_pairs import TryOnPairBatch

PALM_BOXES = (35, 20)       # get_hand_mask of the 512 set: upper arm 35 x 35, forearm 20 x 20 (dataset.py:1790, :1795)
STICK_THICKNESS = 5         # cv2.line(..., 5) (dataset.py:1851)
STICK_RADIUS = 5            # circle(..., radius=5) (dataset.py:1832, :1861)
SIX_IS_LOWER = 0            # the lower garment is labels 9, 12 (dataset.py:1639, :1669)
# change region -> (its index in training.dataset.CHANGE_REGIONS, upper garment from the donor, lower garment from the donor)
# (:1679-1690); the builders take the garments' owners from the outfit's indices
REGIONS = dict(fullbody=(0, True, True), upperbody=(1, True, False), lowerbody=(2, False, True))


class TryOnRegionBatch(TryOnPairBatch):
    """``tensors``: the nine tensors test_512.py forms (KEYS; the generator takes all but ``image`` and ``clothes``, which
    test_512.py writes next to the result); ``person_name`` / ``clothes_name``: the data set's relative paths; ``stages``: the
    uint8 intermediates when the builder was asked to keep them."""
    KEYS = ['image', 'clothes', 'retain', 'pose', 'style_input', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask',
            'denorm_lower_mask']


def _person_launches(parsing, kp, n, H, W, dev):
    """What the test builders' body does first: the person's thick stick figure and palm mask, launched, and the uint8 tensors the
    label-masks entry fills: (stick, palm, retain_img [n,H,H,3], garment_img, garment_mask [2n,H,H,3]: the upper garments, then
    the lower garments)."""
    limbs, joints, quads, present = device_tables(kp, kp, (H - W) // 2, dev)
    u8 = allocator(torch.uint8, dev)
    stick, palm, retain_img = u8(n, H, H, 3), u8(n, H, H), u8(n, H, H, 3)
    garment_img, garment_mask = u8(2 * n, H, H, 3), u8(2 * n, H, H, 3)
    lib, P = _native.lib(), _native.ptr
    with torch.cuda.device(dev):
        s = _native.stream()
        _native.check(lib.pasta_pose_stickman_u8(P(limbs), P(joints), P(stick), n, H, W, STICK_THICKNESS, STICK_RADIUS, s))
        _native.check(lib.pasta_palm_mask_u8(P(parsing), P(quads), P(present), P(palm), n, H, W, *PALM_BOXES, s))
    return stick, palm, retain_img, garment_img, garment_mask


def _stages(image, parsing, stick, palm, retain_img, garment_img, garment_mask, normalized, **valid):
    """The uint8 intermediates the test builders keep: the person's unpadded ``image`` and ``parsing`` (which
    metrics.tryon_fidelity scores against), the label stages and ``normalized``, normalize_outfit_batch's first seven values."""
    n = image.shape[0]
    patches, patches_l, mask_patches, mask_patches_l, den_u, den_l, m_invs = normalized
    return dict(image=image, parsing=parsing, stick=stick, palm=palm, retain_img=retain_img, upper_img=garment_img[:n],
                upper_mask=garment_mask[:n], lower_img=garment_img[n:], lower_mask=garment_mask[n:], patches=patches, patches_lower=patches_l,
                mask_patches=mask_patches, mask_patches_lower=mask_patches_l, denorm_upper=den_u, denorm_lower=den_l, M_invs=m_invs, **valid)


class TryOnOutfitBatch(TryOnRegionBatch):
    """``tensors``: the nine of TryOnRegionBatch, ``clothes`` being the upper garment's donor, and ``clothes_lower``, the lower
    garment's donor; ``person_name`` / ``upper_name`` / ``lower_name``: the data set's relative paths (``clothes_name`` is
    ``upper_name``); ``stages`` as TryOnRegionBatch's, with ``upper_valid`` / ``lower_valid`` / ``person_valid`` [N, 10]."""
    KEYS = TryOnRegionBatch.KEYS + ['clothes_lower']

    def __init__(self, tensors, person_name, upper_name, lower_name, stages=None):
        super().__init__(tensors, person_name, upper_name, stages)
        self.upper_name = self.clothes_name
        self.lower_name = list(lower_name)


class TryOnOutfitBatchBuilder:
    """``build(raw_batch)``: a batch of ``training.dataset.collate_outfits`` -> TryOnOutfitBatch on ``device``.  The batch's M
    distinct people are uploaded once and their matrices solved once; the per-sample views (the person, the owner of the upper
    garment, the owner of the lower one) are gathered on the device.  ``geometry`` = 'host' or 'gpu': where the matrices are solved
    (patch_pipeline.part_maps: DESIGN 8n)."""

    def __init__(self, device, box_factor=2, geometry='host'):
        self.device = torch.device(device)
        self.box_factor = box_factor
        self.geometry = patch_pipeline.check_geometry(geometry)

    def build(self, raw, keep_stages=False):
        t, stages = self._prepare(raw, ('upper', 'lower'), dict(upper='upper_valid', lower='lower_valid', person='person_valid'), keep_stages)
        return TryOnOutfitBatch(t, raw['person_name'], raw['upper_name'], raw['lower_name'], stages)

    def _prepare(self, raw, panels, valid_stages, keep_stages):
        """The one body of the test builders: (fp32 tensors, stages or None) of a batch of ``collate_outfits``.  ``panels``: whose
        photographs follow ``image``, by role: two give ``clothes`` and ``clothes_lower``, one gives ``clothes`` alone (no tenth
        output and no third photograph).  ``valid_stages``: the name under which the stages keep the [N, 10] valid flags of a
        role's matrices."""
        dev = self.device
        people_image, people_parsing, people_kp = upload_person(raw, dev, type(self).__name__, 'people_')
        m, H, W, _ = people_image.shape
        lp = (H - W) // 2
        host_idx = [np.asarray(raw[k], np.int64) for k in ('person_idx', 'upper_idx', 'lower_idx')]
        n = len(host_idx[0])
        assert all(ix.shape == (n,) and ix.min() >= 0 and ix.max() < m for ix in host_idx), 'outfit indices outside the people stack'
        (image, parsing), (u_image, u_parsing), (l_image, l_parsing) = (
            (people_image.index_select(0, ix), people_parsing.index_select(0, ix))
            for ix in (torch.from_numpy(ix).to(dev, non_blocking=True) for ix in host_idx))
        stick, palm, retain_img, garment_img, garment_mask = _person_launches(parsing, people_kp[host_idx[0]], n, H, W, dev)
        lib, P = _native.lib(), _native.ptr
        with torch.cuda.device(dev):
            _native.check(lib.pasta_tryon_outfit_masks_u8(P(image), P(parsing), P(palm), P(u_image), P(u_parsing), P(l_image), P(l_parsing),
                                                          P(retain_img), P(garment_img[:n]), P(garment_mask[:n]), P(garment_img[n:]),
                                                          P(garment_mask[n:]), n, H, W, SIX_IS_LOWER, _native.stream()))
        *normalized, valid_u, valid_l, valid_p = patch_pipeline.normalize_outfit_batch(
            garment_img, garment_mask, shift_keypoints(people_kp, lp), *host_idx, self.box_factor, geometry=self.geometry)
        patches, patches_l, _, _, den_u, den_l, _ = normalized
        pu, pl, ph, pw = patches.shape[1], patches_l.shape[1], patches.shape[2], patches.shape[3]
        photograph = dict(upper=u_image, lower=l_image)
        clothes, clothes_lower = photograph[panels[0]], photograph[panels[1]] if len(panels) == 2 else None
        keys = TryOnOutfitBatch.KEYS if len(panels) == 2 else TryOnRegionBatch.KEYS
        t, outs = output_tensors(keys, n, H, (3 * (pu + pl), ph, pw), dev, OUTFIT_OUTPUTS)
        with torch.cuda.device(dev):
            _native.check(lib.pasta_tryon_outfit_assemble(P(image), P(clothes), P(clothes_lower), P(retain_img), P(stick), P(patches),
                                                          P(patches_l), P(den_u), P(den_l), outs, n, H, W, pu, pl, ph, pw, _native.stream()))
        stages = None
        if keep_stages:
            valid = dict(upper=valid_u, lower=valid_l, person=valid_p)
            stages = _stages(image, parsing, stick, palm, retain_img, garment_img, garment_mask, normalized,
                             **{name: valid[role] for role, name in valid_stages.items()})
        return t, stages


class TryOnRegionBatchBuilder(TryOnOutfitBatchBuilder):
    """``build(raw_batch)``: a batch of ``training.dataset.collate_pairs`` -> TryOnRegionBatch on ``device`` for
    ``change_region`` = 'fullbody', 'upperbody' or 'lowerbody': the pairs as the outfits (P, D, D), (P, D, -) or (P, -, D),
    stacked on the device after the upload.  ``clothes`` is always the DONOR's photograph, which at 'lowerbody' is not the upper
    garment's owner, and there is no ``clothes_lower``."""

    def __init__(self, device, change_region, box_factor=2, geometry='host'):
        if change_region not in REGIONS:
            raise ValueError('change region %s is invalid.' % change_region)
        super().__init__(device, box_factor, geometry)
        self.change_region = change_region

    def build(self, raw, keep_stages=False):
        donor = 'lower' if self.change_region == 'lowerbody' else 'upper'
        t, stages = self._prepare(pairs_batch_as_outfits(upload_images(raw, self.device), self.change_region), (donor,),
                                  {donor: 'clothes_valid', 'person': 'person_valid'}, keep_stages)
        return TryOnRegionBatch(t, raw['person_name'], raw['clothes_name'], stages)


class FullBodyRegionBatchBuilder:
    """``build(raw_batch)``: a batch of ``training.dataset.collate`` at 512 x 320 -> FullBodyBatch on ``device``, which
    TrainingStep.run consumes as the 256 builder's.  ``stages`` (``keep_stages``) carry the 256 builder's names, so that
    training/snapshot_grid.py has one code path.  ``swap`` = dict(region=, group=) or dict(upper_src=, lower_src=), as the 256
    builder's: the batch also carries the swapped inputs of training/swap_outfits.py."""

    # see FullBodyBatchBuilder: parts 0, 6..9 are also cut from the lower garment; key points shifted in float64, x_pad = 0
    lower_parts, x_pad, shin_fallback, shifted = patch_pipeline.LOWER_PARTS_512, 0, False, True

    def __init__(self, device, box_factor=2, geometry='host'):
        self.device = torch.device(device)
        self.box_factor = box_factor
        self.geometry = patch_pipeline.check_geometry(geometry)

    def build(self, raw, keep_stages=False, swap=None):
        dev = self.device
        image, parsing, kp = upload_person(raw, dev, 'FullBodyRegionBatchBuilder')
        n, H, W, _ = image.shape
        lp = (H - W) // 2
        erase, erase_hw = upload_erase(raw, dev, n)
        image, parsing, kp, erase = mirror_batch(raw, image, parsing, kp, erase, erase_hw)
        image, parsing, kp = jitter_batch(raw, image, parsing, kp)
        erase, erase_hw = strokes_batch(raw, erase, erase_hw, H)
        limbs, joints, quads, present = device_tables(kp, kp, lp, dev)
        u8 = allocator(torch.uint8, dev)
        stick, palm, retain_mask, gt = u8(n, H, H, 3), u8(n, H, H), u8(n, H, H), u8(n, H, H)
        garment_img, garment_mask = u8(2 * n, H, H, 3), u8(2 * n, H, H, 3)  # the upper garments, then the lower garments
        lib, P = _native.lib(), _native.ptr
        with torch.cuda.device(dev):
            s = _native.stream()
            _native.check(lib.pasta_pose_stickman_u8(P(limbs), P(joints), P(stick), n, H, W, STICK_THICKNESS, STICK_RADIUS, s))
            _native.check(lib.pasta_palm_mask_u8(P(parsing), P(quads), P(present), P(palm), n, H, W, *PALM_BOXES, s))
            # pasta_tryon_masks_u8's order: both images, then both masks
            _native.check(lib.pasta_tryon_masks_u8(P(image), P(parsing), P(palm), P(retain_mask), P(gt), P(garment_img[:n]), P(garment_img[n:]),
                                                   P(garment_mask[:n]), P(garment_mask[n:]), n, H, W, s))
        own = np.arange(n)                  # everyone wears their own garments: the N people are solved once
        patches, patches_l, mask_patches, mask_patches_l, den_u, den_l, m_invs, _, _, _, part_masks, back, valid = patch_pipeline.normalize_outfit_batch(
            garment_img, garment_mask, shift_keypoints(kp, lp), own, own, own, self.box_factor, want_part_masks=True, want_matrices=True,
            geometry=self.geometry)
        pu, pl, ph, pw = patches.shape[1], patches_l.shape[1], patches.shape[2], patches.shape[3]
        arm_a, arm_b = patch_pipeline.ARM_PARTS[2], patch_pipeline.ARM_PARTS[3]
        t, outs = output_tensors(FullBodyBatch.KEYS, n, H, (3 * (pu + pl), ph, pw), dev)
        with torch.cuda.device(dev):
            _native.check(lib.pasta_tryon_train_region_assemble(P(image), P(stick), P(retain_mask), P(gt), P(patches), P(patches_l), P(den_u),
                                                                P(den_l), P(part_masks), arm_a, arm_b, P(erase), P(erase_hw), outs, n, H, W,
                                                                pu, pl, ph, pw, int(erase.shape[1]), int(erase.shape[2]), _native.stream()))
        stages = None
        if keep_stages or swap is not None:
            hwc = lambda x: x.permute(0, 2, 3, 1, 4).reshape(n, ph, pw, -1).contiguous()       # parts along the channel axis, as at 256
            stages = dict(stick=stick, palm=palm, retain_mask=retain_mask, gt_parsing=gt, upper_img=garment_img[:n], lower_img=garment_img[n:],
                          upper_mask=garment_mask[:n], lower_mask=garment_mask[n:], norm_img=hwc(patches), norm_img_lower=hwc(patches_l),
                          denorm_upper=den_u, denorm_lower=den_l, arm_masks=part_masks[:, list(patch_pipeline.ARM_PARTS)].contiguous(),
                          M_invs=m_invs, norm_clothes_mask=hwc(mask_patches), norm_clothes_mask_lower=hwc(mask_patches_l))
        if swap is not None:
            attach_swap(t, stages, back, valid, self, swap, keep_stages)
        return FullBodyBatch(t, stages if keep_stages else None, image)
