"""A batch of the try-on data set prepared on the GPU: what the reference's ``UvitonDatasetFull._load_raw_image`` /
``__getitem__`` (training/dataset.py:515-568, 619-736, 929-993) and its training loop (training_loop_wo_flow_fullbody.py:425-456)
do per sample on the host, as a few launches per batch:

    pasta_pose_stickman_u8   stick figure                       (csrc/tryon_inputs.hip)
    pasta_palm_mask_u8       palm part of the retain mask
    pasta_tryon_masks_u8     retain mask, gt_parsing, garment images and masks
    patch_pipeline.normalize_batch   the ten body-part warps    (csrc/patches.hip)
    pasta_tryon_assemble     erase mask and every float conversion, into the nine tensors of SyntheticFullBodyBatch.KEYS

The host keeps the file decoding (training/dataset.py), the key-point geometry below and the 8 x 8 solves of the warps."""

import ctypes
import math

import numpy as np
import torch

from torch_utils.ops import _native
from training import patch_pipeline

# dataset.py:43-52 (1-based joint pairs)
LIMBSEQ = ((2, 3), (2, 6), (3, 4), (4, 5), (6, 7), (7, 8), (2, 9), (9, 10), (10, 11), (2, 12), (12, 13), (13, 14), (2, 1), (1, 15),
           (15, 17), (1, 16), (16, 18), (3, 17), (6, 18))
ARMS = ((5, 6, 7), (2, 3, 4))       # left, right: shoulder, elbow, wrist (get_palm :683-684)
COORD_LIMIT = 4096                  # stick-figure coordinates are clamped to +-COORD_LIMIT (integer arithmetic in the kernel)
QUAD_LIMIT = 1e5                    # palm quadrilateral corners are clamped to +-QUAD_LIMIT


def stick_tables(keypoints):
    """[N, 18, 3] key points (unpadded x, y, confidence) -> (limbs int32 [N, 19, 5] = x0, y0, x1, y1, drawn;
    joints int32 [N, 18, 3] = x, y, drawn) of draw_pose_from_cords (:704-736): int()-truncated, drawn when confidence >= 0.1."""
    kp = np.asarray(keypoints, np.float64)
    xy = np.clip(np.trunc(np.nan_to_num(kp[..., :2])), -COORD_LIMIT, COORD_LIMIT).astype(np.int32)
    seen = kp[..., 2] >= 0.1
    f = np.array([a - 1 for a, _ in LIMBSEQ])
    t = np.array([b - 1 for _, b in LIMBSEQ])
    limbs = np.concatenate([xy[:, f], xy[:, t], (seen[:, f] & seen[:, t])[..., None].astype(np.int32)], axis=2)
    joints = np.concatenate([xy, seen[..., None].astype(np.int32)], axis=2)
    return np.ascontiguousarray(limbs), np.ascontiguousarray(joints)


def rectangle_corners(a, b, c, d):
    """The polygon of get_rectangle_mask(a, b, c, d) (:626-650), float64 [4, 2], in its corner order."""
    a, b, c, d = (np.float64(v) for v in (a, b, c, d))
    x1, y1 = a + (b - d) / 4, b + (c - a) / 4
    x2, y2 = a - (b - d) / 4, b - (c - a) / 4
    x3, y3 = c + (b - d) / 4, d + (c - a) / 4
    x4, y4 = c - (b - d) / 4, d - (c - a) / 4
    v0_x, v0_y = c - a, d - b
    v1_x, v1_y = x3 - x1, y3 - y1
    v2_x, v2_y = x4 - x1, y4 - y1
    with np.errstate(divide='ignore', invalid='ignore'):
        cos1 = (v0_x * v1_x + v0_y * v1_y) / (math.sqrt(v0_x * v0_x + v0_y * v0_y) * math.sqrt(v1_x * v1_x + v1_y * v1_y))
        cos2 = (v0_x * v2_x + v0_y * v2_y) / (math.sqrt(v0_x * v0_x + v0_y * v0_y) * math.sqrt(v2_x * v2_x + v2_y * v2_y))
    tail = [x3, y3, x4, y4] if cos1 < cos2 else [x4, y4, x3, y3]
    return np.array([x1, y1, x2, y2] + tail, np.float64).reshape(4, 2)


def palm_quads(keypoints, left_padding):
    """(quads float64 [N, 4, 4, 2], present uint8 [N, 4]) for the left upper arm, left forearm, right upper arm, right forearm
    (get_hand_mask :652-672: key points shifted by the padding; a segment needs both confidences > 0.1)."""
    kp = np.asarray(keypoints, np.float64)
    n = kp.shape[0]
    quads, present = np.zeros([n, 4, 4, 2]), np.zeros([n, 4], np.uint8)
    for i in range(n):
        for side, (s, e, w) in enumerate(ARMS):
            arm = kp[i, [s, e, w]].copy()
            arm[:, 0] += left_padding
            for k, (p, q) in enumerate(((0, 1), (1, 2))):
                if arm[p, 2] > 0.1 and arm[q, 2] > 0.1:
                    quads[i, 2 * side + k] = rectangle_corners(arm[p, 0], arm[p, 1], arm[q, 0], arm[q, 1])
                    present[i, 2 * side + k] = 1
    return np.ascontiguousarray(np.clip(np.nan_to_num(quads), -QUAD_LIMIT, QUAD_LIMIT)), present


class FullBodyBatch:
    """The interface TrainingStep.run consumes (as SyntheticFullBodyBatch): ``tensors`` (the nine KEYS), ``batch``, ``split``.
    ``stages`` holds the uint8 intermediates when the builder was asked to keep them; ``image`` is the photographs' uint8 batch
    [N, H, W, 3] as the builder uploaded it (the reconstruction metric scores against it)."""
    KEYS = ['real_img', 'style_input', 'retain', 'pose', 'denorm_upper_input', 'denorm_lower_input',
            'denorm_upper_mask', 'denorm_lower_mask', 'gt_parsing']

    def __init__(self, tensors, stages=None, image=None):
        self.tensors = tensors
        self.batch = int(tensors['real_img'].shape[0])
        self.stages = stages
        self.image = image

    def split(self, batch_gpu):
        parts = {k: v.split(batch_gpu) for k, v in self.tensors.items()}
        return [{k: parts[k][i] for k in self.KEYS} for i in range(len(parts['real_img']))]


class FullBodyBatchBuilder:
    """``build(raw_batch)``: a batch of ``training.dataset.collate`` -> FullBodyBatch on ``device``."""

    def __init__(self, device, box_factor=2):
        self.device = torch.device(device)
        self.box_factor = box_factor

    def build(self, raw, keep_stages=False):
        dev = self.device
        up = lambda t: torch.as_tensor(t).to(dev, non_blocking=True).contiguous()
        image, parsing = up(raw['image']), up(raw['parsing'])
        erase, erase_hw = up(raw['erase_masks']), up(torch.as_tensor(raw['erase_hw'], dtype=torch.int32))
        keypoints = np.asarray(raw['keypoints'], np.float64)
        _native.require_gpu(image, 'FullBodyBatchBuilder')
        assert image.dtype == torch.uint8 and parsing.dtype == torch.uint8 and erase.dtype == torch.uint8
        n, H, W, _ = image.shape
        assert H >= W and tuple(parsing.shape) == (n, H, W) and keypoints.shape == (n, 18, 3) and erase.ndim == 3
        hw = np.asarray(raw['erase_hw'])
        assert hw.shape == (n, 2) and (hw >= 1).all() and (hw[:, 0] <= erase.shape[1]).all() and (hw[:, 1] <= erase.shape[2]).all()
        lp = (H - W) // 2
        limbs, joints = stick_tables(keypoints)
        quads, present = palm_quads(keypoints, lp)
        limbs, joints, quads, present = (torch.from_numpy(a).to(dev, non_blocking=True) for a in (limbs, joints, quads, present))
        u8 = lambda *shape: torch.empty(shape, dtype=torch.uint8, device=dev)
        stick, palm, retain_mask, gt = u8(n, H, H, 3), u8(n, H, H), u8(n, H, H), u8(n, H, H)
        garments = [u8(n, H, H, 3) for _ in range(4)]          # upper image, lower image, upper mask, lower mask
        lib, P = _native.lib(), _native.ptr
        with torch.cuda.device(dev):
            s = _native.stream()
            _native.check(lib.pasta_pose_stickman_u8(P(limbs), P(joints), P(stick), n, H, W, s))
            _native.check(lib.pasta_palm_mask_u8(P(parsing), P(quads), P(present), P(palm), n, H, W, s))
            _native.check(lib.pasta_tryon_masks_u8(P(image), P(parsing), P(palm), P(retain_mask), P(gt), *[P(g) for g in garments], n, H, W, s))
        norm_img, norm_lower, den_u, den_l, m_invs, hand_masks, norm_mask, norm_mask_lower = patch_pipeline.normalize_batch(
            *garments, keypoints, self.box_factor)
        norm_img, norm_lower, den_u, den_l = (t.contiguous() for t in (norm_img, norm_lower, den_u, den_l))
        arm = hand_masks.reshape(n, 4, H, H).contiguous()
        ph, pw, cu, cl = norm_img.shape[1], norm_img.shape[2], norm_img.shape[3], norm_lower.shape[3]
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        t = dict(real_img=f32(n, 3, H, H), style_input=f32(n, cu + cl, ph, pw), retain=f32(n, 3, H, H), pose=f32(n, 6, H, H),
                 denorm_upper_input=f32(n, 3, H, H), denorm_lower_input=f32(n, 3, H, H), denorm_upper_mask=f32(n, 1, H, H),
                 denorm_lower_mask=f32(n, 1, H, H), gt_parsing=f32(n, 1, H, H))
        outs = (ctypes.c_void_p * 9)(*[t[k].data_ptr() for k in FullBodyBatch.KEYS])
        with torch.cuda.device(dev):
            _native.check(lib.pasta_tryon_assemble(P(image), P(stick), P(retain_mask), P(gt), P(norm_img), P(norm_lower), P(den_u), P(den_l),
                                                   P(arm), P(erase), P(erase_hw), outs, n, H, W, ph, pw, cu, cl,
                                                   int(erase.shape[1]), int(erase.shape[2]), _native.stream()))
        stages = None
        if keep_stages:
            stages = dict(stick=stick, palm=palm, retain_mask=retain_mask, gt_parsing=gt, upper_img=garments[0], lower_img=garments[1],
                          upper_mask=garments[2], lower_mask=garments[3], norm_img=norm_img, norm_img_lower=norm_lower,
                          denorm_upper=den_u, denorm_lower=den_l, arm_masks=arm, M_invs=m_invs, norm_clothes_mask=norm_mask.contiguous(),
                          norm_clothes_mask_lower=norm_mask_lower.contiguous())
        return FullBodyBatch(t, stages, image)
