"""The SSIM loss without a GPU: the fp64 reference against itself and against the metric's, the fairness of the
chosen inputs, the three entries' declarations and host guards, and ``--ssim_weight`` of train_wo_flow_fullbody.py through
``--dry-run``."""
import json
import os
import re

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import recon_ref
import ssim_loss_ref as R
from train_grid_tree import make_tree
from tryon_512_train_tree import make_512_train_tree

COMMAND = ('--cfg', 'fashion', '--batch', '2', '--kimg', '5', '--l1_weight', '40', '--mask_weight', '20')


# ---- the reference ----

@pytest.mark.parametrize('shape', R.CASES)
def test_closed_form_gradient_equals_autograd_in_fp64(shape):
    for content in R.CONTENTS:
        x, y = R.make_case(shape, content)
        loss, grad = R.loss_and_grad(x, y, shape[3], shape[4])
        loss_ag, grad_ag = R.loss_and_grad_autograd(x, y, shape[3], shape[4])
        assert abs(loss - loss_ag) <= 1e-12, (content, loss, loss_ag)
        assert np.abs(grad - grad_ag).max() <= 1e-8 * max(np.abs(grad_ag).max(), 1.0 / R.windows(shape)), content
        assert np.isfinite(grad).all() and not grad[..., :shape[3]].any() and not grad[..., shape[3] + shape[4]:].any()
        if content == 'equal':      # S = 1 everywhere
            assert abs(loss) <= 1e-12 and np.abs(grad).max() * R.windows(shape) <= 1e-9


def test_the_byte_grid_maps_agree_with_the_metric():
    """On the byte grid the loss's SSIM is the metric's.  The mapping is ``ssim_loss_ref.grid``: v = b / 127.5 - 1 in fp64, so that
    the intensity v + 1 is the byte scaled by 1 / 127.5; ``from_bytes`` is its fp32 form that ``recon_ref.to_u8`` inverts."""
    rng = np.random.RandomState(5)
    for bx, by in ((rng.randint(0, 256, [24, 30]), rng.randint(0, 256, [24, 30])), (np.full([11, 13], 255), np.full([11, 13], 254)),
                   (np.zeros([12, 11], np.int64), rng.randint(0, 3, [12, 11]))):
        assert np.abs(R.ssim_map(R.grid(bx), R.grid(by)) - recon_ref.ssim_map(bx, by)).max() <= 1e-12
    b = np.arange(256)
    v = R.from_bytes(b)
    assert v.dtype == np.float32 and (recon_ref.to_u8(v) == b).all()
    assert np.abs(v.astype(np.float64) - R.grid(b)).max() <= 2.0 ** -22           # two steps of fp32 at 1
    # and the constants are the metric's, scaled with L^2
    assert R.C1 == pytest.approx(recon_ref.C1 / 127.5 ** 2, rel=1e-15) and R.C2 == pytest.approx(recon_ref.C2 / 127.5 ** 2, rel=1e-15)


@pytest.mark.parametrize('shape', R.CASES)
def test_the_inputs_are_fair_an_fp32_evaluation_stays_under_the_ceiling(shape):
    for content in R.CONTENTS:
        x, y = R.make_case(shape, content)
        loss, grad = R.loss_and_grad(x, y, shape[3], shape[4])
        loss32, grad32 = R.loss_and_grad_autograd(x, y, shape[3], shape[4], dtype=torch.float32)
        value, gradient = abs(loss32 - loss), R.grad_error(grad32, grad, R.windows(shape))
        print(f'{shape} {content}: fp32 restatement value {value:.2e} gradient {gradient:.2e}')
        assert value < R.CEILING and gradient < R.CEILING, (content, value, gradient)


def test_the_bounds_are_under_the_ceiling():
    assert 0 < R.VALUE_TOL <= R.CEILING and 0 < R.GRAD_TOL <= R.CEILING


# ---- the entries ----

def test_the_entries_are_declared_typed_and_late():
    from conftest import ROOT
    from torch_utils import custom_ops
    header = open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read()
    lib = custom_ops.get_plugin()
    for name, kind, args in (('pasta_ssim_loss_workspace', 'int64_t', 3), ('pasta_ssim_loss', 'int', 12), ('pasta_ssim_loss_backward', 'int', 11)):
        assert re.search(r'\b%s %s\(' % (kind, name), header), name
        assert name in custom_ops.ABI and len(custom_ops.ABI[name][1]) == args and name in custom_ops.LATE_ENTRIES
        assert custom_ops.has_entry(lib, name)
    assert lib.pasta_abi_version() == custom_ops.EXPECTED_ABI == 22


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """Pointers are the never-dereferenced value 1: every call is refused with the entry's own text before anything is launched."""
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()

    def refused(status, text):
        assert status != 0 and text in lib.pasta_last_error(), lib.pasta_last_error()

    assert lib.pasta_ssim_loss_workspace(2, 10, 40) == 0 and lib.pasta_ssim_loss_workspace(2, 40, 10) == 0 and lib.pasta_ssim_loss_workspace(0, 40, 40) == 0
    assert lib.pasta_ssim_loss_workspace(2, 33, 43) == 2 * 3 * 2 * 2 * 8
    need = lib.pasta_ssim_loss_workspace(2, 23, 25)
    forward = lambda x=1, y=1, loss=1, work=1, nbytes=need, H=23, Wt=40, c0=3, W=25, N=2: \
        lib.pasta_ssim_loss(x, y, loss, 1, work, nbytes, N, H, Wt, c0, W, None)
    backward = lambda x=1, y=1, maps=1, g=1, dx=1, H=23, Wt=40, c0=3, W=25, N=2: lib.pasta_ssim_loss_backward(x, y, maps, g, dx, N, H, Wt, c0, W, None)
    for null in ('x', 'y', 'loss', 'work'):
        refused(forward(**{null: None}), b'ssim_loss: null pointer')
    for null in ('x', 'y', 'maps', 'g', 'dx'):
        refused(backward(**{null: None}), b'ssim_loss_backward: null pointer')
    refused(forward(H=10), b'ssim_loss: 10 x 25 is smaller than the 11 x 11 SSIM window')
    refused(backward(H=10), b'ssim_loss_backward: 10 x 25 is smaller than the 11 x 11 SSIM window')
    refused(forward(W=10), b'smaller than the 11 x 11 SSIM window')
    refused(forward(c0=16), b'ssim_loss: bad shape or crop (columns 16 + 25 of 40)')
    refused(backward(c0=16), b'ssim_loss_backward: bad shape or crop (columns 16 + 25 of 40)')
    refused(forward(c0=-1), b'bad shape or crop')
    refused(forward(N=65536, nbytes=1 << 40), b'bad shape or crop')
    refused(forward(H=4097, nbytes=1 << 40), b'bad shape or crop')
    refused(forward(nbytes=need - 1), b'ssim_loss: workspace of %d bytes, %d needed' % (need - 1, need))


# ---- the command line ----

@pytest.fixture(scope='module')
def trees(tmp_path_factory):
    return {256: make_tree(tmp_path_factory.mktemp('structure_cli_256')), 512: make_512_train_tree(tmp_path_factory.mktemp('structure_cli_512'))}


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def _run(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


@pytest.mark.parametrize('res, width', [(256, 192), (512, 320)])
def test_the_option_sets_weight_and_content_width(trees, tmp_path, res, width):
    plain = _run(trees[res], tmp_path / 'runs', *COMMAND)
    ssim = _run(trees[res], tmp_path / 'runs', *COMMAND, '--ssim_weight', '5')
    assert plain.exit_code == 0 and ssim.exit_code == 0, (plain.output, ssim.output)
    a, b = _options(plain.output), _options(ssim.output)
    assert 'ssim' not in json.dumps(a['cfg']) and 'ssim' not in os.path.basename(a['run_dir'])      # no ssim_* key, no suffix
    assert b['cfg']['loss_kwargs'].pop('ssim_weight') == 5 and b['cfg']['loss_kwargs'].pop('ssim_width') == width
    assert b.pop('run_dir') == a.pop('run_dir') + '-ssim5'
    assert b == a                                               # and nothing else


def test_weight_zero_is_no_option_and_a_negative_one_is_refused(trees, tmp_path):
    plain = _run(trees[256], tmp_path / 'runs', *COMMAND)
    zero = _run(trees[256], tmp_path / 'runs', *COMMAND, '--ssim_weight', '0')
    assert plain.exit_code == 0 and zero.output == plain.output
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--ssim_weight', '-1')
    assert res.exit_code != 0 and '--ssim_weight must be non-negative' in res.output, res.output
    assert not (tmp_path / 'runs').exists()
    half = _run(trees[256], tmp_path / 'runs', *COMMAND, '--ssim_weight', '0.5')
    assert half.exit_code == 0 and _options(half.output)['run_dir'].endswith('-ssim0.5')


def test_continue_keeps_the_recorded_weight_and_refuses_another(trees, tmp_path):
    from training import train_state
    res = _run(trees[256], tmp_path / 'runs', *COMMAND, '--ssim_weight', '5')
    assert res.exit_code == 0, res.output
    options = _options(res.output)
    run_dir = tmp_path / 'runs' / os.path.basename(options['run_dir'])
    os.makedirs(run_dir)
    empty = dict(cur_nimg=0, batch_idx=0, cur_tick=1, elapsed_sec=0.0, num_gpus=1, batch_size=2, batch_gpu=2, random_seed=0,
                 options=json.dumps(options, indent=2), G={}, D={}, G_ema={}, opt={}, grid_z=torch.zeros([0, 0]), ranks=[])
    train_state.save_state(str(run_dir / 'training-state-000000.pt'), None, empty)
    for value in ('5', '0', '7'):
        res = _run(trees[256], tmp_path / 'out', '--continue', str(run_dir), '--ssim_weight', value)
        assert res.exit_code != 0
        assert '--ssim_weight cannot be given with --continue' in res.output and 'keeps its recorded value' in res.output, res.output
    res = _run(trees[256], tmp_path / 'out', '--continue', str(run_dir))
    assert res.exit_code == 0, res.output
    got = _options(res.output)
    assert got['cfg'] == options['cfg'] and got['cfg']['loss_kwargs']['ssim_weight'] == 5 and got['cfg']['loss_kwargs']['ssim_width'] == 192
    import train_wo_flow_fullbody as T
    assert 'ssim_weight' not in T.CONTINUE_MAY_CHANGE


def test_the_loss_class_takes_the_term_only_with_a_width():
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    kw = dict(device=torch.device('cpu'), G_mapping=None, G_synthesis=None, G_const_encoding=None, G_style_encoding=None, D=None,
              vgg_weight=0, contextual_weight=0)
    assert StyleGAN2Loss(**kw).ssim_weight == 0
    assert StyleGAN2Loss(ssim_weight=2, ssim_width=192, **kw).ssim_width == 192
    with pytest.raises(ValueError, match='ssim_width'):
        StyleGAN2Loss(ssim_weight=2, **kw)
    with pytest.raises(ValueError, match='negative'):
        StyleGAN2Loss(ssim_weight=-1, ssim_width=192, **kw)
    with pytest.raises(NotImplementedError, match='ssim_weight'):
        StyleGAN2Loss(**dict(kw, contextual_weight=1))


def test_the_op_refuses_a_cpu_tensor():
    from torch_utils.ops.ssim_loss import ssim_loss
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):
        ssim_loss(torch.zeros([1, 3, 12, 12]), torch.zeros([1, 3, 12, 12]))
