"""The SSIM loss's definition and gradient in fp64 (include/pasta_hip.h, "The SSIM term of the generator's loss"), the cases the
kernels are held to, and the bounds.

x (generated) and y (photograph) are [N, 3, H, Wt] with values v in nominally [-1, 1], taken as intensities v + 1 of dynamic
range L = 2; only columns c0 .. c0 + W - 1 count.  Per channel and valid position of an explicit 11 x 11 Gaussian window (sigma
1.5, normalised; ``recon_ref.window``), with mx = E[x] + 1, my = E[y] + 1 and the (shift-free) second moments of x and y:
    S = (2 mx my + C1) (2 sxy + C2) / ((mx^2 + my^2 + C1) (sxx + syy + C2)),   loss = 1 - mean S.
The intensities are a pure scaling of the bytes the metric scores, b = (v + 1) * 127.5, and SSIM does not change under a scaling
when C1 and C2 scale with L^2: on byte-grid images this is ``recon_ref.ssim_map``.  (Means of v itself would not do: SSIM's
luminance factor is not invariant under a shift.)
The gradient with respect to x is given twice: by the closed form (``loss_and_grad``) and by autograd through a torch restatement
(``loss_and_grad_autograd``), which also runs in fp32 to show that the inputs are fair."""
import numpy as np
import torch

import recon_ref

K = recon_ref.K
L = 2.0
C1, C2 = (0.01 * L) ** 2, (0.03 * L) ** 2

# The project's parity figure (README): the ceiling for both measures below.
CEILING = 1e-3
# Bounds: ten times the largest deviation of the HIP kernels from ``loss_and_grad`` measured on an MI355X over CASES x CONTENTS
# (tests/test_ssim_loss_gpu.py prints every figure).  VALUE_TOL bounds |loss - loss64|, GRAD_TOL bounds ``grad_error``.
#   value:    4.98e-7 on (2, 12, 14, 0, 14) 'sinusoid'; 6e-8 or less on every other content
#   gradient: 1.92e-5 on (1, 64, 64, 8, 48) 'sinusoid'; then 1.6e-6 ('close'), 3.6e-7 ('noise'), 3.2e-7 ('near_white')
# Both are below 1e-4, the figure above which the kernels' numerics would have to change.  (Without the per-tile centring the same
# kernels measured 7.98e-6 and 2.54e-4, both on 'near_white': DESIGN 8j.)
VALUE_TOL = 5.0e-6
GRAD_TOL = 1.9e-4

# (N, H, Wt, c0, W): the smallest shapes at which the tiling can go wrong.
CASES = [
    (1, 11, 11, 0, 11),     # one window
    (2, 12, 14, 0, 14),     # a handful of windows, two images
    (1, 32, 42, 0, 42),     # exactly one 22 x 32 tile of positions, no sliver
    (1, 33, 43, 0, 43),     # one row and one column past a tile: four workgroups, three of them slivers
    (2, 23, 40, 3, 25),     # odd crop inside wider rows; the columns outside it are NaN and must not be read
    (1, 64, 64, 8, 48),     # 3 x 2 tiles, interior pixels that gather all 121 windows
]
CONTENTS = ['noise', 'close', 'equal', 'opposite', 'sinusoid', 'near_white', 'out_of_range']


def make_case(shape, content, seed=0):
    """fp32 x, y [N, 3, H, Wt] of a case; the columns outside the crop are NaN in both."""
    n, h, wt, c0, w = shape
    rng = np.random.RandomState(1000 * CASES.index(tuple(shape)) + 10 * CONTENTS.index(content) + seed) if tuple(shape) in CASES \
        else np.random.RandomState(seed)
    size = [n, 3, h, wt]
    if content == 'noise':
        x, y = rng.uniform(-1, 1, size), rng.uniform(-1, 1, size)
    elif content == 'close':
        y = rng.uniform(-1, 1, size)
        x = np.clip(y + 0.05 * rng.standard_normal(size), -1, 1)
    elif content == 'equal':
        x, y = np.full(size, 0.3), np.full(size, 0.3)
    elif content == 'opposite':
        x, y = np.full(size, -1.0), np.full(size, 1.0)
    elif content == 'sinusoid':
        i, j, c = np.arange(h).reshape(1, 1, h, 1), np.arange(wt).reshape(1, 1, 1, wt), np.arange(3).reshape(1, 3, 1, 1)
        y = 0.8 * np.sin(0.3 * i + 0.2 * j + c) * np.ones([n, 1, 1, 1])
        x = y + 0.01 * rng.standard_normal(size)
    elif content == 'near_white':
        x, y = 1 - 0.002 * rng.uniform(0, 1, size), np.ones(size)
    elif content == 'out_of_range':
        x, y = 3 * rng.standard_normal(size), rng.uniform(-1, 1, size)
    else:
        raise ValueError(content)
    x, y = x.astype(np.float32), y.astype(np.float32)
    for a in (x, y):
        a[..., :c0] = np.nan
        a[..., c0 + w:] = np.nan
    return x, y


def _mean(a):
    """Weighted mean of every valid 11 x 11 window of the last two axes, explicit window."""
    view = np.lib.stride_tricks.sliding_window_view(a, (K, K), axis=(-2, -1))
    return np.einsum('...kl,kl->...', view, recon_ref.window())


def _parts(x, y):
    ex, ey = _mean(x), _mean(y)
    sxx, syy, sxy = _mean(x * x) - ex * ex, _mean(y * y) - ey * ey, _mean(x * y) - ex * ey
    mx, my = ex + 1, ey + 1                             # means of the intensities v + 1 in [0, L]; the second moments do not move
    return mx, my, 2 * mx * my + C1, 2 * sxy + C2, mx * mx + my * my + C1, sxx + syy + C2


def ssim_map(x, y):
    """x, y [..., H, W] (values of dynamic range 2) -> SSIM [..., H - 10, W - 10] in fp64."""
    _, _, a1, a2, b1, b2 = _parts(np.asarray(x, np.float64), np.asarray(y, np.float64))
    return a1 * a2 / (b1 * b2)


def _transposed(f):
    """(w (*) F)[q] = sum over the valid positions p with q - 10 <= p <= q of w[q - p] F[p]: [..., Hp, Wp] -> [..., Hp + 10, Wp + 10]."""
    w = recon_ref.window()
    hp, wp = f.shape[-2:]
    out = np.zeros(f.shape[:-2] + (hp + K - 1, wp + K - 1))
    for dy in range(K):
        for dx in range(K):
            out[..., dy:dy + hp, dx:dx + wp] += w[dy, dx] * f
    return out


def loss_and_grad(x, y, c0, width):
    """The closed form in numpy fp64: (loss, dloss/dx [N, 3, H, Wt], exactly 0 outside the crop)."""
    xc = np.asarray(x, np.float64)[..., c0:c0 + width]
    yc = np.asarray(y, np.float64)[..., c0:c0 + width]
    mx, my, a1, a2, b1, b2 = _parts(xc, yc)
    s = a1 * a2 / (b1 * b2)
    d_mx = 2 * my * a2 / (b1 * b2) - 2 * mx * s / b1
    b = -s / b2
    c = 2 * a1 / (b1 * b2)
    a = d_mx - 2 * mx * b - my * c
    grad = np.zeros(np.shape(x))
    grad[..., c0:c0 + width] = -(_transposed(a) + 2 * (xc + 1) * _transposed(b) + (yc + 1) * _transposed(c)) / s.size
    return 1 - s.mean(), grad


def loss_and_grad_autograd(x, y, c0, width, dtype=torch.float64):
    """The same through autograd: a torch restatement of the definition with F.conv2d, evaluated in ``dtype`` on the CPU."""
    xc = torch.as_tensor(np.asarray(x)[..., c0:c0 + width].copy()).to(dtype).requires_grad_(True)
    yc = torch.as_tensor(np.asarray(y)[..., c0:c0 + width].copy()).to(dtype)
    w = torch.as_tensor(recon_ref.window()).to(dtype).reshape(1, 1, K, K)
    mean = lambda a: torch.nn.functional.conv2d(a.reshape(-1, 1, a.shape[2], a.shape[3]), w)
    ex, ey = mean(xc), mean(yc)
    sxx, syy, sxy = mean(xc * xc) - ex * ex, mean(yc * yc) - ey * ey, mean(xc * yc) - ex * ey
    mx, my = ex + 1, ey + 1
    s = (2 * mx * my + C1) * (2 * sxy + C2) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    loss = 1 - s.mean()
    (g,) = torch.autograd.grad(loss, xc)
    grad = np.zeros(np.shape(x))
    grad[..., c0:c0 + width] = g.double().numpy()
    return float(loss.detach()), grad


def windows(shape):
    n, h, _, _, w = shape
    return n * 3 * (h - K + 1) * (w - K + 1)


def grad_error(g, g64, m):
    """max |g - g64| / max(max |g64|, 1 / M): 1 / M is the weight of one SSIM value in the loss; a gradient below it everywhere is
    a difference of terms of that size, and an error relative to the gradient alone would mean nothing."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return float(np.abs(g - g64).max() / max(np.abs(g64).max(), 1.0 / m))


def grid(b):
    """A byte's place on the grid in fp64: b / 127.5 - 1, so that the intensity v + 1 is b / 127.5 exactly."""
    return np.asarray(b).astype(np.float64) / 127.5 - 1


def from_bytes(b):
    """A byte as an fp32 value the networks could have produced: the least fp32 >= ``grid(b)`` that ``recon_ref.to_u8`` takes back
    to b (the fp32 nearest to the grid point often truncates to b - 1), so it is the inverse of ``to_u8`` on the grid and lies
    within two fp32 steps of the grid point."""
    b = np.asarray(b)
    v = grid(b).astype(np.float32)
    for _ in range(4):
        low = recon_ref.to_u8(v) < b
        if not low.any():
            break
        v = np.where(low, np.nextafter(v, np.float32(2)), v).astype(np.float32)
    assert (recon_ref.to_u8(v) == b).all()
    return v
