"""The contextual loss as plain torch, the yardstick of torch_utils.ops.contextual_loss (include/pasta_hip.h states the definition).

``statement`` follows the reference's ``ContextualLoss_forward`` (training/loss_wo_flow_fullbody.py:503-541 with PONO and feature
centring) in its operation order -- centre on the channel mean of y, normalise, ``1 - matmul``, divide by the row minimum plus
1e-3, exponentiate, normalise the rows, take the row maxima, average, ``-log`` -- in whatever floating type the inputs have, and
adds this project's masks: a column with ``y_valid == 0`` does not exist, a row with ``x_valid == 0`` does not enter the mean, and
a sample without a valid row or column has loss 0.  It materialises the N x N matrices, which is what the op exists to avoid.

``closed_form_grad`` is the gradient the kernels implement, written out from the per-row quantities m, j*, S, E."""

import torch

EPS = 2.220446049250313e-16     # sys.float_info.epsilon, the reference's feature_normalize


def normalized(x, y):
    """x^ and y^ as [B, C, N]: both centred on y's channel mean per position, then scaled to unit length."""
    b, c = x.shape[:2]
    mu = y.mean(dim=1).unsqueeze(dim=1)
    x = x - mu
    y = y - mu
    x = torch.div(x, torch.norm(x, 2, 1, keepdim=True) + EPS).view(b, c, -1)
    y = torch.div(y, torch.norm(y, 2, 1, keepdim=True) + EPS).view(b, c, -1)
    return x, y


def _masks(xh, x_valid, y_valid):
    b, _, n = xh.shape
    rows = torch.ones([b, n], dtype=torch.bool, device=xh.device) if x_valid is None else x_valid.reshape(b, n) != 0
    cols = torch.ones([b, n], dtype=torch.bool, device=xh.device) if y_valid is None else y_valid.reshape(b, n) != 0
    return rows, cols


def statement_normalized(xh, yh, x_valid=None, y_valid=None, h=0.1):
    """The statement from unit vectors on: [B] losses."""
    rows, cols = _masks(xh, x_valid, y_valid)
    count = rows.sum(dim=1)
    ok = (count > 0) & (cols.sum(dim=1) > 0)
    cols = cols | ~ok[:, None]              # an empty sample is evaluated on all columns and then replaced by 0: no 0 / 0 on the way
    d = 1 - torch.matmul(xh.permute(0, 2, 1), yh)                                # [B, N, N]
    big = torch.finfo(d.dtype).max
    d_min = torch.min(torch.where(cols[:, None, :], d, torch.full_like(d, big)), dim=-1, keepdim=True)[0]
    d_norm = d / (d_min + 1e-3)
    w = torch.where(cols[:, None, :], torch.exp((1 - d_norm) / h), torch.zeros_like(d))
    a = w / torch.sum(w, dim=-1, keepdim=True)
    cx_rows = torch.max(a, dim=-1)[0]                                            # [B, N]
    cx = torch.where(rows, cx_rows, torch.zeros_like(cx_rows)).sum(dim=1) / count.clamp(min=1).to(d.dtype)
    return torch.where(ok, -torch.log(torch.where(ok, cx, torch.ones_like(cx))), torch.zeros_like(cx))


def statement(x, y, x_valid=None, y_valid=None, h=0.1):
    xh, yh = normalized(x, y.detach())
    return statement_normalized(xh, yh, x_valid, y_valid, h)


def closed_form_grad(xh, yh, x_valid=None, y_valid=None, h=0.1, grad_out=None):
    """d(sum_b grad_out[b] loss_b) / d x^ as [B, C, N], from m, j*, S, E per row (no autograd)."""
    rows, cols = _masks(xh, x_valid, y_valid)
    ok = ((rows.sum(dim=1) > 0) & (cols.sum(dim=1) > 0))[:, None]
    cols = cols | ~ok
    b, c, n = xh.shape
    grad_out = torch.ones([b], dtype=xh.dtype, device=xh.device) if grad_out is None else grad_out
    d = 1 - torch.matmul(xh.permute(0, 2, 1), yh)
    big = torch.finfo(d.dtype).max
    m, jstar = torch.min(torch.where(cols[:, None, :], d, torch.full_like(d, big)), dim=-1)      # [B, N]
    ci = 1 / (m + 1e-3)
    w = torch.where(cols[:, None, :], torch.exp((1 - d * ci[..., None]) / h), torch.zeros_like(d))
    s = w.sum(dim=-1)
    a = w / s[..., None]
    e = (a * d).sum(dim=-1)
    cx_rows = torch.where(rows, torch.exp((1 - m * ci) / h) / s, torch.zeros_like(s))
    total = cx_rows.sum(dim=1, keepdim=True)                                      # R mean CX
    coef = torch.where(ok & rows, grad_out[:, None] * cx_rows / torch.where(ok, total, torch.ones_like(total)), torch.zeros_like(s))
    g = torch.matmul(a, yh.permute(0, 2, 1))                                      # [B, N, C]: sum_j A_ij y^_j
    ys = torch.gather(yh.permute(0, 2, 1), 1, jstar[..., None].expand(b, n, c))   # y^_{j*}
    out = coef[..., None] * ((ci / h)[..., None] * (g - ys) - (ci * ci * (e - m) / h)[..., None] * ys)
    return out.permute(0, 2, 1)


# ---- the table of tests/test_contextual_loss_gpu.py and the bound that goes with it -------------------------------------------
# name: (B, C, H, W).  Inputs are |randn| (relu-like), from one seeded generator per case.
CASES = {
    'plain': (2, 6, 5, 7),
    'single': (2, 3, 1, 1),
    'one_tile': (1, 2, 8, 8),            # N = 64: exactly one column tile, one row block
    'ragged': (2, 130, 9, 23),           # C over one 128-channel stretch and odd; N = 207: four column tiles, the last ragged
    'masked': (2, 6, 5, 7),              # about half of the rows and of the columns, different per sample
    'empty': (3, 8, 8, 9),               # sample 0 without a valid row, sample 1 without a valid column, sample 2 masked at random
    'last_tile': (2, 6, 9, 23),          # every row's nearest column is in the last, ragged tile (columns 192 .. 206)
    'block_invalid': (2, 6, 9, 23),      # rows 64 .. 127, one whole row block, invalid
    'near': (2, 6, 5, 7),                # x = y + 0.3 noise: m_i around 1e-1, 1 / ((m + 1e-3) h) around 1e2
    'nearer': (2, 6, 5, 7),              # x = y + 0.1 noise: m_i around 1e-2, 1 / ((m + 1e-3) h) around 1e3
}
VALUE_FLOOR = 1e-2      # a loss that is 0 (N = 1, or x = y) has no relative error: below this the deviation is absolute / floor
GRAD_FLOOR = 1e-3       # likewise for a gradient that is identically 0 (N = 1, an empty sample)


def make_case(name):
    """(x, y, x_valid, y_valid, upstream) as fp64 / uint8 CPU tensors; the masks are None where the case has none."""
    b, c, hh, ww = CASES[name]
    n = hh * ww
    gen = torch.Generator().manual_seed(sorted(CASES).index(name) + 1)
    x = torch.randn([b, c, hh, ww], generator=gen, dtype=torch.float64).abs()
    y = torch.randn([b, c, hh, ww], generator=gen, dtype=torch.float64).abs()
    xv = yv = None
    if name in ('masked', 'empty'):
        xv = (torch.rand([b, hh, ww], generator=gen) < 0.5).to(torch.uint8)
        yv = (torch.rand([b, hh, ww], generator=gen) < 0.5).to(torch.uint8)
    if name == 'empty':
        xv[0] = 0
        yv[1] = 0
    if name == 'last_tile':
        first = (n - 1) // 64 * 64
        idx = first + torch.arange(n) % (n - first)
        noise = torch.randn([b, c, n], generator=gen, dtype=torch.float64)
        x = (y.reshape(b, c, n)[:, :, idx] + 0.02 * noise).abs().reshape(b, c, hh, ww)
    if name == 'block_invalid':
        xv = torch.ones([b, n], dtype=torch.uint8)
        xv[:, 64:128] = 0
        xv = xv.reshape(b, hh, ww)
    if name in ('near', 'nearer'):
        x = (y + (0.3 if name == 'near' else 0.1) * torch.randn([b, c, hh, ww], generator=gen, dtype=torch.float64)).abs()
    upstream = torch.arange(1, b + 1, dtype=torch.float64) * 0.37 + 0.5
    return x, y, xv, yv, upstream


def value_and_grad(x, y, xv, yv, upstream, fn=None):
    """(loss [B], d(sum_b upstream_b loss_b)/dx) of ``fn`` (default: the statement), detached."""
    fn = statement if fn is None else fn
    x = x.detach().clone().requires_grad_(True)
    loss = fn(x, y, xv, yv)
    grad, = torch.autograd.grad((loss * upstream.to(loss.dtype)).sum(), x)
    return loss.detach(), grad.detach()


def deviations(value, grad, ref_value, ref_grad):
    """(value deviation, gradient deviation) of fp32 results against fp64 ones: the value relative per sample, the gradient relative
    to the largest gradient magnitude of the case, each denominator no smaller than its floor."""
    value, grad = value.double().cpu(), grad.double().cpu()
    dv = ((value - ref_value).abs() / ref_value.abs().clamp(min=VALUE_FLOOR)).max().item()
    dg = ((grad - ref_grad).abs().max() / ref_grad.abs().max().clamp(min=GRAD_FLOOR)).item()
    return dv, dg


_cache = {}


def references():
    """{name: (case, fp64 value, fp64 gradient)}: computed once and left unchanged."""
    if 'ref' not in _cache:
        _cache['ref'] = {name: (make_case(name),) + value_and_grad(*make_case(name)) for name in CASES}
    return _cache['ref']


def fp32_deviation():
    """The largest deviation over the table of the fp32 statement, evaluated on the CPU, from the fp64 one: (value, gradient)."""
    if 'dev' not in _cache:
        worst_v = worst_g = 0.0
        for name, ((x, y, xv, yv, up), v64, g64) in references().items():
            v32, g32 = value_and_grad(x.float(), y.float(), xv, yv, up.float())
            dv, dg = deviations(v32, g32, v64, g64)
            worst_v, worst_g = max(worst_v, dv), max(worst_g, dg)
        _cache['dev'] = (worst_v, worst_g)
    return _cache['dev']


def bounds():
    """What the kernels are held to: 8 x the fp32 statement's own deviation per quantity.  The factor covers the MFMA's summation
    order and the hardware exponential, which the statement does not share."""
    dv, dg = fp32_deviation()
    return 8 * dv, 8 * dg
