"""Rounding-aware fp64 references for kernels that compute in fp32 and store fp32, fp16 or bf16.

A reference is computed in fp64 from ``rounded`` inputs (what the kernel actually reads), and the kernel's output is
held to what one fp32 evaluation and one round-to-nearest-even store can give:

* ``assert_stored``: element-wise outputs.  Each element within half a storage ulp plus an fp32 term, and (16-bit) almost
  every element bitwise equal to the fp64 reference rounded once: a truncating or doubly-rounding store misses on about
  half of them.
* ``assert_reduced``: fp32 sums, with a bound derived from the depth of the kernel's summation tree.

A plain module imported by the tests (no fixtures).
"""

import math

import numpy as np
import torch

U32 = 2.0 ** -24        # unit roundoff of fp32

# (significand bits including the implicit one, smallest normal exponent)
_FORMAT = {torch.float16: (11, -14), torch.bfloat16: (8, -126), torch.float32: (24, -126)}


def _np64(t):
    return np.asarray(t.detach().cpu().to(torch.float64).numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)


def ulp(ref, dtype):
    """Spacing of ``dtype`` (fp16 / bf16 / fp32) at |ref| (fp64 numpy array): the distance from the binade's lower end to the next
    representable value; subnormals and zero get the subnormal spacing."""
    p, emin = _FORMAT[dtype]
    a = np.abs(_np64(ref))
    _, e = np.frexp(a)                      # a = m * 2**e, m in [0.5, 1): the binade is [2**(e-1), 2**e)
    e = np.where(a == 0, emin, np.maximum(e - 1, emin))
    return np.ldexp(1.0, e - p + 1)


def rne(ref, dtype):
    """fp64 values rounded ONCE to ``dtype`` (round to nearest, ties to even), returned as fp64.  Done on the fp64 value
    directly: torch's double -> bfloat16 conversion goes through fp32 and so rounds twice."""
    r = _np64(ref)
    s = ulp(r, dtype)
    return np.round(r / s) * s              # r / s and the product are exact (s is a power of two); np.round ties to even


def rounded(t, dtype):
    """CPU data rounded to the storage type ``dtype`` and back to fp64 (a torch tensor): the inputs a kernel reading
    ``dtype`` sees."""
    t = t.detach().cpu()
    if dtype == torch.float64:
        return t.to(torch.float64)
    return torch.from_numpy(np.asarray(rne(t, dtype)))


def assert_stored(got, ref, dtype, scale, k=4, bitwise=0.99, what=''):
    """``got`` (stored as ``dtype``) against the fp64 ``ref`` of an output made by one fp32 evaluation and one rounding.

    ``scale`` (>= 0, broadcastable) is the fp64 sum of the magnitudes of the terms that made each element, ``k`` the number
    of fp32 roundings along the way.  Every element must satisfy

        |got - ref| <= 1/2 ulp_dtype(|ref| + d) + d,    d = k 2^-24 scale

    (the fp32 value v has |v - ref| <= d; storing it adds at most half a spacing at |v|).  For 16-bit ``dtype`` at least
    ``bitwise`` of the elements must also equal ``rne(ref, dtype)`` bit for bit; pass ``bitwise=None`` where the fp32 error
    is not far below the storage spacing (cancellation)."""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    d = k * U32 * np.broadcast_to(_np64(scale), r.shape)
    bound = 0.5 * ulp(np.abs(r) + d, dtype) + d
    err = np.abs(g - r)
    bad = ~(err <= bound)                   # NaN counts as bad
    if bad.any():
        i = np.flatnonzero(bad.ravel())
        j = int(i[np.argmax((err / bound).ravel()[i])]) if np.isfinite(err.ravel()[i]).any() else int(i[0])
        raise AssertionError(f'{what}: {len(i)} of {r.size} elements outside the storage bound; worst at flat index {j}: '
                             f'got {g.ravel()[j]!r}, ref {r.ravel()[j]!r}, bound {bound.ravel()[j]!r}')
    if bitwise is not None and dtype in (torch.float16, torch.bfloat16):
        same = float((g == rne(r, dtype)).mean())
        assert same >= bitwise, f'{what}: only {same:.4f} of the elements equal the reference rounded once to {dtype} (want >= {bitwise})'


def reduction_depth(n, lanes, extra=2):
    """c(n) for ``assert_reduced``: the depth of the fp32 summation tree of a kernel that sums ``n`` terms in ``lanes``
    parallel partial sums (each over at most ceil(n / lanes) terms, one after another), combines the partials by a tree of
    ceil(log2 lanes) levels, and spends ``extra`` roundings on forming each term (a product, a conversion) and on the final
    combination (the four wave partials of a workgroup, the host-side sum of chunk partials)."""
    return math.ceil(n / lanes) + math.ceil(math.log2(max(lanes, 1))) + extra


def assert_reduced(got, ref, scale, n, lanes=256, extra=2, what=''):
    """fp32 reductions: |got - ref| <= c(n) 2^-24 scale, with ``scale`` the fp64 sum of |term| per output.

    Derivation: a sum evaluated in floating point along any binary tree of depth d (the longest chain of roundings from
    one term to the result) satisfies |s_hat - s| <= gamma_d sum |x_i|, gamma_d = d u / (1 - d u)  (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., section 4.2).  A term's own relative error (the product p*q, the dz of an
    activation) adds its roundings to d.  The kernels here have a lane of ``lanes`` threads sum its share of ceil(n/lanes)
    terms in sequence (d grows by one per term), then combine lanes by wavefront shuffles and workgroup partials:
    d <= reduction_depth(n, lanes, extra) = c(n).  For d u << 1, gamma_d <= 1.01 d u, and the bound is taken as
    1.01 c(n) u sum |x_i|."""
    g, r = _np64(got), _np64(ref)
    assert g.shape == r.shape, (what, g.shape, r.shape)
    bound = 1.01 * reduction_depth(n, lanes, extra) * U32 * np.broadcast_to(_np64(scale), r.shape)
    err = np.abs(g - r)
    bad = ~(err <= bound)
    if bad.any():
        i = np.flatnonzero(bad.ravel())
        j = int(i[0])
        raise AssertionError(f'{what}: {len(i)} of {r.size} sums outside c(n) u scale; first at flat index {j}: '
                             f'got {g.ravel()[j]!r}, ref {r.ravel()[j]!r}, bound {bound.ravel()[j]!r}')
