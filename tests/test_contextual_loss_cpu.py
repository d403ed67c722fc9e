"""The contextual loss's statement (tests/contextual_ref.py; include/pasta_hip.h) on the CPU: answers that are known
without computing, the closed-form gradient the kernels implement against autograd in fp64, and ``--swap_cx_weight`` through
``--dry-run`` and the loss class."""
import json
import os

import pytest
import torch
from click.testing import CliRunner

import contextual_ref as R
from train_grid_tree import make_tree

COMMAND = ('--cfg', 'fashion', '--batch', '4', '--kimg', '5', '--l1_weight', '40', '--mask_weight', '20')


def _inputs(b=2, c=6, hh=5, ww=7, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn([b, c, hh, ww], generator=gen, dtype=torch.float64).abs(),
            torch.randn([b, c, hh, ww], generator=gen, dtype=torch.float64).abs())


# ---- known answers ---------------------------------------------------------------------------------------------------------------

def test_equal_inputs_give_zero():
    """x = y: m_i = 0 at j = i, every other column's weight is exp(-1000 d_ij / h) of the row's: CX_i = 1 to far below 1e-6."""
    x, _ = _inputs()
    assert R.statement(x, x).abs().max().item() < 1e-6


def test_a_permutation_of_the_columns_changes_nothing():
    """Once mu is out of the way (pre-centred y: channel mean 0 at every position) the loss sees y's positions as a set."""
    x, y = _inputs()
    y = y - y.mean(dim=1, keepdim=True)
    perm = torch.randperm(y.shape[2] * y.shape[3], generator=torch.Generator().manual_seed(1))
    shuffled = y.flatten(2)[:, :, perm].reshape(y.shape)
    a, b = R.statement(x, y), R.statement(x, shuffled)
    assert (a - b).abs().max().item() < 1e-12 and a.min().item() > 0.01


def test_all_ones_masks_are_none():
    x, y = _inputs()
    ones = torch.ones([2, 5, 7], dtype=torch.uint8)
    assert torch.equal(R.statement(x, y), R.statement(x, y, ones, ones))
    xh, yh = R.normalized(x, y)
    assert torch.equal(R.closed_form_grad(xh, yh), R.closed_form_grad(xh, yh, ones, ones))


def test_a_far_column_can_be_masked_without_effect():
    """x close to y: a column that is nobody's nearest and whose weight exp((1 - d c) / h) underflows to 0 adds exactly nothing."""
    _, y = _inputs()
    x = y + 1e-4 * torch.randn(y.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    xh, yh = R.normalized(x, y)
    d = 1 - xh.transpose(1, 2) @ yh
    m, jstar = d.min(dim=-1)
    off_diagonal = d + 9 * torch.eye(d.shape[1], dtype=d.dtype)
    far = int(off_diagonal.min(dim=1)[0].min(dim=0)[0].argmax())      # the column farthest from every row but its own, in both samples
    w = torch.exp((1 - d[:, :, far] / (m + 1e-3)) / 0.1)
    rows = torch.arange(d.shape[1]) != far
    assert (jstar[:, rows] != far).all() and (w[:, rows] == 0).all()
    valid = torch.ones([2, 5, 7], dtype=torch.uint8)
    valid.view(2, -1)[:, far] = 0
    rows_only = torch.ones([2, 5, 7], dtype=torch.uint8)
    rows_only.view(2, -1)[:, far] = 0           # row `far` itself has the column as its nearest: keep it out of both means
    assert torch.equal(R.statement(x, y, rows_only, valid), R.statement(x, y, rows_only, None))


def test_the_empty_mask_rule():
    x, y = _inputs(b=3)
    xv = torch.ones([3, 5, 7], dtype=torch.uint8)
    yv = torch.ones([3, 5, 7], dtype=torch.uint8)
    xv[0] = 0
    yv[1] = 0
    xg = x.clone().requires_grad_(True)
    loss = R.statement(xg, y, xv, yv)
    grad, = torch.autograd.grad(loss.sum(), xg)
    assert loss[0].item() == 0 and loss[1].item() == 0 and loss[2].item() > 0
    assert not grad[:2].any() and grad[2].any() and torch.isfinite(grad).all()
    xh, yh = R.normalized(x, y)
    closed = R.closed_form_grad(xh, yh, xv, yv)
    assert not closed[:2].any() and torch.isfinite(closed).all()


# ---- the gradient the kernels implement --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(R.CASES))
def test_closed_form_gradient_is_autograds(name):
    x, y, xv, yv, up = R.make_case(name)
    xh, yh = R.normalized(x, y)
    xh = xh.detach().requires_grad_(True)
    loss = R.statement_normalized(xh, yh, xv, yv)
    want, = torch.autograd.grad((loss * up).sum(), xh)
    got = R.closed_form_grad(xh.detach(), yh, xv, yv, grad_out=up)
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    print('%s: absolute %.3e, relative to max|grad| %.3e' % (name, err, err / max(scale, 1e-300)))
    assert err <= 1e-12 and (scale == 0 or err / scale <= 1e-12 or err <= 1e-15)


def test_the_bound_is_computed_and_small():
    bound_v, bound_g = R.bounds()
    print('bounds: value %.3e, gradient %.3e' % (bound_v, bound_g))
    assert 0 < bound_v < 1e-2 and 0 < bound_g < 1e-1


# ---- the option and the class -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('cx_cli'))


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def test_the_option_needs_a_swap_weight(tree, tmp_path):
    for extra in ((), ('--swap_weight', '0')):
        res = _run(tree, tmp_path / 'runs', *COMMAND, '--swap_cx_weight', '2', *extra)
        assert res.exit_code != 0 and '--swap_cx_weight needs a positive --swap_weight' in res.output, res.output
    res = _run(tree, tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--swap_cx_weight', '-1')
    assert res.exit_code != 0 and '--swap_cx_weight must be non-negative' in res.output, res.output


def test_the_option_is_recorded_and_zero_records_nothing(tree, tmp_path):
    swap = _run(tree, tmp_path / 'runs', *COMMAND, '--swap_weight', '1')
    zero = _run(tree, tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--swap_cx_weight', '0')
    cx = _run(tree, tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--swap_cx_weight', '2')
    assert swap.exit_code == 0 and zero.exit_code == 0 and cx.exit_code == 0, (swap.output, zero.output, cx.output)
    assert zero.output == swap.output and 'swap_cx' not in swap.output and 'contextual weight' not in swap.output
    a, b = _options(swap.output), _options(cx.output)
    assert b['cfg']['loss_kwargs']['swap_cx_weight'] == 2 and b['run_dir'].endswith('-swap1-cx2')
    assert 'contextual weight 2' in cx.output
    b['cfg']['loss_kwargs'].pop('swap_cx_weight')
    b['run_dir'] = b['run_dir'][:-len('-cx2')]
    assert a == b


def test_continue_keeps_the_option(tree, tmp_path):
    from training import train_state
    import train_wo_flow_fullbody as T
    res = _run(tree, tmp_path / 'runs', *COMMAND, '--swap_weight', '1', '--swap_cx_weight', '2')
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=4, batch_gpu=4, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    res = _run(tree, tmp_path / 'out', '--continue', str(run_dir), '--swap_cx_weight', '2')
    assert res.exit_code != 0 and '--swap_cx_weight cannot be given with --continue' in res.output, res.output
    res = _run(tree, tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    assert _options(res.output)['cfg']['loss_kwargs']['swap_cx_weight'] == 2
    assert 'swap_cx_weight' not in T.CONTINUE_MAY_CHANGE


def test_the_class_refuses_what_it_must():
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    make = lambda **kw: StyleGAN2Loss(torch.device('cpu'), None, None, None, None, None, vgg_weight=0, **kw)
    with pytest.raises(ValueError, match='swap_cx_weight must not be negative'):
        make(contextual_weight=0, swap_weight=1, swap_cx_weight=-1)
    with pytest.raises(ValueError, match='needs a positive swap_weight'):
        make(contextual_weight=0, swap_cx_weight=1)
    with pytest.raises(NotImplementedError, match='contextual term needs'):
        make(contextual_weight=1, swap_weight=1, swap_cx_weight=1)
    assert make(contextual_weight=0).swap_cx_weight == 0
