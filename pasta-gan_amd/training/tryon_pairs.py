"""A batch of the try-on TEST pairs prepared on the GPU: what the reference's ``UvitonDatasetV19_test._load_raw_image`` /
``normalize`` / ``__getitem__`` (training/dataset.py:1085-1525) and test.py's conversions (test.py:104-117) do per sample on
the host in four loader processes, as a few launches per batch:

    pasta_pose_stickman_u8            both people's stick figures, one launch  (csrc/tryon_inputs.hip)
    pasta_palm_mask_box_u8            the person's palm mask, boxes 25 and 15 (csrc/tryon_pairs.hip)
    pasta_tryon_pair_masks_u8         retain image, the person's lower garment, the donor's upper garment
    patch_pipeline.normalize_pair_batch   three forward warps + the eroded and the plain composite (csrc/patches.hip,
                                          csrc/tryon_pairs.hip)
    pasta_tryon_pair_assemble         the seven fp32 tensors G takes

The host keeps the file decoding (training/dataset.py), the key-point geometry and the 8 x 8 solves of the warps.  Key points
are shifted by the padding in float64 before get_crop's float32 conversion (dataset.py:1100, :1129), so the quadrilaterals are
formed with x_pad = 0 from pre-shifted joints; the palm quadrilaterals add the same float64 shift (tryon_batch.palm_quads)."""

import ctypes

import numpy as np
import torch

from torch_utils.ops import _native
from training import patch_pipeline
from training.tryon_batch import palm_quads, stick_tables

PALM_BOXES = (25, 15)       # get_hand_mask of the test set: upper arm 25 x 25, forearm 15 x 15 (dataset.py:1240-1253)


class TryOnPairBatch:
    """``tensors``: the seven inputs of test.py's generator calls (KEYS); ``person_name`` / ``clothes_name``: the data set's
    relative paths; ``stages``: the uint8 intermediates (and the person's unpadded ``image`` and ``parsing``, which
    metrics.tryon_fidelity scores against) when the builder was asked to keep them."""
    KEYS = ['retain', 'pose', 'style_input', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask', 'denorm_lower_mask']

    def __init__(self, tensors, person_name, clothes_name, stages=None):
        self.tensors = tensors
        self.batch = int(tensors['retain'].shape[0])
        self.person_name = list(person_name)
        self.clothes_name = list(clothes_name)
        self.stages = stages


class TryOnPairBatchBuilder:
    """``build(raw_batch)``: a batch of ``training.dataset.collate_pairs`` -> TryOnPairBatch on ``device``."""

    def __init__(self, device, box_factor=2):
        self.device = torch.device(device)
        self.box_factor = box_factor

    def build(self, raw, keep_stages=False):
        dev = self.device
        up = lambda t: torch.as_tensor(t).to(dev, non_blocking=True).contiguous()
        image, parsing = up(raw['image']), up(raw['parsing'])
        d_image, d_parsing = up(raw['clothes_image']), up(raw['clothes_parsing'])
        kp = np.asarray(raw['keypoints'], np.float64)
        d_kp = np.asarray(raw['clothes_keypoints'], np.float64)
        _native.require_gpu(image, 'TryOnPairBatchBuilder')
        assert all(t.dtype == torch.uint8 for t in (image, parsing, d_image, d_parsing))
        n, H, W, _ = image.shape
        assert H >= W and tuple(d_image.shape) == (n, H, W, 3) and tuple(parsing.shape) == tuple(d_parsing.shape) == (n, H, W)
        assert kp.shape == d_kp.shape == (n, 18, 3)
        lp = (H - W) // 2
        limbs, joints = stick_tables(np.concatenate([d_kp, kp]))          # stick figures from the UNSHIFTED key points
        quads, present = palm_quads(kp, lp)
        limbs, joints, quads, present = (torch.from_numpy(a).to(dev, non_blocking=True) for a in (limbs, joints, quads, present))
        u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
        sticks, palm = u8(2 * n, H, H, 3), u8(n, H, H)                     # sticks: the donors, then the persons
        retain_img, lower_img, lower_mask, upper_img, upper_mask = (u8(n, H, H, 3) for _ in range(5))
        lib, P = _native.lib(), _native.ptr
        with torch.cuda.device(dev):
            s = _native.stream()
            _native.check(lib.pasta_pose_stickman_u8(P(limbs), P(joints), P(sticks), 2 * n, H, W, s))
            _native.check(lib.pasta_palm_mask_box_u8(P(parsing), P(quads), P(present), P(palm), n, H, W, *PALM_BOXES, s))
            _native.check(lib.pasta_tryon_pair_masks_u8(P(image), P(parsing), P(palm), P(d_image), P(d_parsing), P(retain_img), P(lower_img),
                                                        P(lower_mask), P(upper_img), P(upper_mask), n, H, W, s))
        d_stick, stick = sticks[:n], sticks[n:]
        shift = lambda k: np.concatenate([k[..., :1] + lp, k[..., 1:]], axis=-1)     # float64, as keypoints[:, 0] += left_padding
        patches, stick_patches, mask_patches, den_u, den_l, m_invs, valid_u, valid_l = patch_pipeline.normalize_pair_batch(
            upper_img, d_stick, upper_mask, shift(d_kp), lower_img, stick, lower_mask, shift(kp), self.box_factor)
        parts, ph, pw = patches.shape[1], patches.shape[2], patches.shape[3]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        t = dict(retain=f32(n, 3, H, H), pose=f32(n, 6, H, H), style_input=f32(n, 6 * parts, ph, pw), denorm_upper_input=f32(n, 3, H, H),
                 denorm_lower_input=f32(n, 3, H, H), denorm_upper_mask=f32(n, 1, H, H), denorm_lower_mask=f32(n, 1, H, H))
        outs = (ctypes.c_void_p * 7)(*[t[k].data_ptr() for k in TryOnPairBatch.KEYS])
        with torch.cuda.device(dev):
            _native.check(lib.pasta_tryon_pair_assemble(P(retain_img), P(stick), P(patches), P(stick_patches), P(den_u), P(den_l), outs, n, H,
                                                        parts, ph, pw, _native.stream()))
        stages = None
        if keep_stages:
            stages = dict(image=image, parsing=parsing, stick=stick, clothes_stick=d_stick, palm=palm, retain_img=retain_img, lower_img=lower_img, lower_mask=lower_mask,
                          upper_img=upper_img, upper_mask=upper_mask, patches=patches, stick_patches=stick_patches, mask_patches=mask_patches,
                          denorm_upper=den_u, denorm_lower=den_l, M_invs=m_invs, upper_valid=valid_u, lower_valid=valid_l)
        return TryOnPairBatch(t, raw['person_name'], raw['clothes_name'], stages)


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
