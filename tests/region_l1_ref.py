"""fp64 reference of the region L1 term (include/pasta_hip.h, "region L1"), the cases its tests share, and the donor
rule restated.

A pixel belongs to exactly one region: 0 where keep != 0, else 1 where upper_mask != 0, else 2 where lower_mask != 0, else none;
the targets are retain, upper, lower.  out[k][r] = (1 / M) sum over the region's pixels and 3 channels of |x_k - t_r|, M = 3 N H H.
With upstream g [K, 3], dx_k = q sign(x_k - t_r) on region r, q = g[k][r] / M, and 0 where the pixel has no region."""
import numpy as np
import torch

# (K, N, H): a single four-pixel group per row, sizes that are no multiple of any tile, more than one workgroup per image (64 x 64
# = 4096 pixels = four workgroups of 256 threads x 4 pixels), the most images
CASES = [(1, 1, 4), (2, 3, 12), (1, 2, 20), (2, 2, 64), (4, 1, 36)]
CONTENTS = ['none', 'keep', 'overlap', 'blobs', 'equal']
VALUE_RTOL = 2.0 ** -22     # |x - t| rounds once in fp32 (2^-24, the terms non-negative), the quotient once more (2^-24); fp64 sums


def make_case(shape, content, seed=0):
    """numpy inputs: images [K] fp32 [N,3,H,H], retain, upper, lower fp32 [N,3,H,H], keep uint8 [N,H,H], upper_mask, lower_mask fp32
    [N,1,H,H]."""
    K, N, H = shape
    rng = np.random.RandomState(1000 * seed + 100 * K + 10 * N + H + 7 * CONTENTS.index(content))
    u = lambda *s: (rng.rand(*s) * 2 - 1).astype(np.float32)
    images = [u(N, 3, H, H) for _ in range(K)]
    retain, upper, lower = u(N, 3, H, H), u(N, 3, H, H), u(N, 3, H, H)
    zeros_u8, zeros = np.zeros([N, H, H], np.uint8), np.zeros([N, 1, H, H], np.float32)
    if content == 'none':
        keep, um, lm = zeros_u8, zeros, zeros.copy()
    elif content == 'keep':
        keep, um, lm = (rng.rand(N, H, H) < 0.6).astype(np.uint8) * 255, zeros, zeros.copy()
    elif content == 'overlap':
        keep, um, lm = np.ones([N, H, H], np.uint8), np.ones([N, 1, H, H], np.float32), np.ones([N, 1, H, H], np.float32)
    else:
        def blobs(p):
            c = max(H // 4, 1)
            coarse = rng.rand(N, c, c) < p
            return np.repeat(np.repeat(coarse, H // c, axis=1), H // c, axis=2)[:, :H, :H] if H % c == 0 else rng.rand(N, H, H) < p
        keep = blobs(0.4).astype(np.uint8)
        um = (rng.rand(N, 1, H, H) < 0.5).astype(np.float32)
        lm = blobs(0.6).astype(np.float32).reshape(N, 1, H, H)
    if content == 'equal':          # x == t on half the pixels, of every region
        region = regions(keep, um, lm)
        same = rng.rand(N, 1, H, H) < 0.5
        for x in images:
            for r, t in enumerate((retain, upper, lower)):
                np.copyto(x, t, where=same & (region == r)[:, None])
    return images, retain, upper, lower, keep, um, lm


def regions(keep, upper_mask, lower_mask):
    """int [N,H,H]: 0, 1, 2 or -1 by the priority rule."""
    return np.where(keep != 0, 0, np.where(upper_mask[:, 0] != 0, 1, np.where(lower_mask[:, 0] != 0, 2, -1)))


def values(images, retain, upper, lower, keep, upper_mask, lower_mask):
    """float64 [K, 3]."""
    region = regions(keep, upper_mask, lower_mask)
    M = 3.0 * region.size
    out = np.zeros([len(images), 3])
    for k, x in enumerate(images):
        for r, t in enumerate((retain, upper, lower)):
            d = np.abs(x.astype(np.float64) - t.astype(np.float64))
            out[k, r] = (d * (region == r)[:, None]).sum() / M
    return out


def gradients(images, retain, upper, lower, keep, upper_mask, lower_mask, g):
    """The closed form: [K] float64 [N,3,H,H] for upstream ``g`` [K, 3]."""
    region = regions(keep, upper_mask, lower_mask)
    M = 3.0 * region.size
    out = []
    for k, x in enumerate(images):
        dx = np.zeros(x.shape)
        for r, t in enumerate((retain, upper, lower)):
            dx += (g[k][r] / M) * np.sign(x.astype(np.float64) - t.astype(np.float64)) * (region == r)[:, None]
        out.append(dx)
    return out


def values_torch(images, retain, upper, lower, keep, upper_mask, lower_mask, dtype=torch.float64):
    """A torch restatement that autograd differentiates: [K, 3] from tensors (or arrays) in ``dtype``."""
    as_t = lambda a: a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    keep, um, lm = as_t(keep), as_t(upper_mask), as_t(lower_mask)
    in0 = keep != 0
    in1 = ~in0 & (um[:, 0] != 0)
    in2 = ~in0 & ~in1 & (lm[:, 0] != 0)
    M = 3.0 * keep.numel()
    rows = []
    for x in images:
        x = as_t(x).to(dtype)
        rows.append(torch.stack([((x - as_t(t).to(dtype)).abs() * w[:, None].to(dtype)).sum() / M
                                 for t, w in ((retain, in0), (upper, in1), (lower, in2))]))
    return torch.stack(rows)


def donors(n, b):
    """The donor rule restated: with g = i // b the donor of sample i is g b + (i - g b + 1) % b."""
    return [(i // b) * b + (i - (i // b) * b + 1) % b for i in range(n)]
