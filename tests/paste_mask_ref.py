"""Where the photograph may be pasted, in numpy (include/pasta_hip.h, pasta_photo_paste_mask_u8), written directly
from the rule: the generator's statement from its heads, the lookup in the item's rule row, the palm term."""
import numpy as np

OTHER, UPPER, LOWER, SKIN = 0, 1, 2, 3
CLASS_STATEMENT = np.array([OTHER, UPPER, LOWER, SKIN, SKIN, SKIN], np.int64)       # gt_parsing's classes 0..5


def argmax_planes(planes):
    """fp32 [N, 6, H, W] -> int64 [N, H, W] as torch.argmax(dim=1): the first NaN where there is one, else the first of the
    largest values (numpy's argmax does the same; this is the rule spelled out, plane after plane)."""
    planes = np.asarray(planes, np.float32)
    best, c = planes[:, 0].copy(), np.zeros(planes[:, 0].shape, np.int64)
    for k in range(1, planes.shape[1]):
        t = planes[:, k]
        with np.errstate(invalid='ignore'):
            take = ~np.isnan(best) & (np.isnan(t) | (t > best))
        best, c = np.where(take, t, best), np.where(take, k, c)
    return c


def statement(heads, c0, width, shape):
    """heads: () | (fp32 [N, 6, Ht, Ht],) | (u, l: fp32 [N, 1, Ht, Ht]) -> int64 ``shape`` = [N, H, W] in {0, 1, 2, 3}, read at
    rows 0 .. H - 1 and columns c0 .. c0 + W - 1 of the heads."""
    n, h, w = shape
    assert w == width
    crop = lambda x: np.asarray(x, np.float32)[:, :, :h, c0:c0 + w]
    if len(heads) == 0:
        return np.zeros(shape, np.int64)
    if len(heads) == 1:
        assert heads[0].shape[1] == 6
        return CLASS_STATEMENT[argmax_planes(crop(heads[0]))]
    u, l = (crop(x)[:, 0] for x in heads)
    with np.errstate(invalid='ignore'):                 # IEEE: a comparison with a NaN is false
        return np.where(u > np.float32(0.5), UPPER, np.where(l > np.float32(0.5), LOWER, OTHER)).astype(np.int64)


def paste_mask(parsing, palm, rule, heads, c0):
    """parsing uint8 [N, H, W], palm uint8 [N, H, Ht] or None, rule uint8 [N, 256], heads as ``statement`` -> uint8 [N, H, W]."""
    parsing, rule = np.asarray(parsing), np.asarray(rule)
    n, h, w = parsing.shape
    assert parsing.dtype == np.uint8 and rule.dtype == np.uint8 and rule.shape == (n, 256)
    s = statement(heads, c0, w, (n, h, w))
    allowed = rule[np.arange(n)[:, None, None], parsing.astype(np.int64)].astype(np.int64)
    m = ((allowed >> s) & 1) != 0
    if palm is not None:
        assert np.asarray(palm).shape[:2] == (n, h) and c0 == (np.asarray(palm).shape[2] - w) // 2
        m = m | (np.asarray(palm)[:, :, c0:c0 + w] != 0)
    return m.astype(np.uint8)


def kept_parts_rule(n, keep_labels):
    rule = np.zeros([n, 256], np.uint8)
    rule[:, list(keep_labels)] = 0b1111
    return rule
