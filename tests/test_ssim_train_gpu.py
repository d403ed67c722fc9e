"""The SSIM term in training: ``StyleGAN2Loss(ssim_weight=, ssim_width=)`` through one Gmain on stand-in networks --
what it reports, what it adds to every generator gradient, and that weight 0 is the loss without the keyword -- and one run of
train_wo_flow_fullbody.py with ``--ssim_weight``, continued once."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import PKG, ROOT, rel_err
from train_grid_tree import make_tree

pytestmark = pytest.mark.gpu

RES, WIDTH, BATCH = 32, 24, 2       # SyntheticFullBodyBatch pads RES // 8 columns on each side


@pytest.fixture(scope='module')
def world():
    import tiny_models
    from training.training_loop_wo_flow_fullbody import SyntheticFullBodyBatch
    torch.manual_seed(3)
    dev = torch.device('cuda')
    G, D = tiny_models.TinyG().to(dev), tiny_models.TinyD().to(dev)
    (batch,) = SyntheticFullBodyBatch(BATCH, dev, seed=1, res=RES).split(BATCH)
    return G, D, batch


@pytest.fixture(autouse=True)
def deterministic_stock_convolutions():
    """The stand-in networks are stock torch convolutions, whose weight gradients may be summed with atomics: ask for the
    deterministic algorithms, so that two equal steps give equal bits."""
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def _gmain(world, **loss_kwargs):
    """One accumulate_gradients('Gmain') on copies of the networks: (the loss object, its G, {name: gradient}, {report name: value})."""
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    G, D, batch = copy.deepcopy(world[0]), copy.deepcopy(world[1]), world[2]
    reports = {}
    loss = StyleGAN2Loss(torch.device('cuda'), G.mapping, G.synthesis, G.const_encoding, G.style_encoding, D, style_mixing_prob=0, l1_weight=40,
                         vgg_weight=0, contextual_weight=0, mask_weight=20, report_fn=lambda name, value: reports.__setitem__(name, value),
                         **loss_kwargs)
    G.requires_grad_(True)
    D.requires_grad_(False)
    loss.accumulate_gradients(phase='Gmain', gen_z=torch.zeros([BATCH, 0], device='cuda'), sync=False, gain=1, **batch)
    return loss, G, {name: p.grad for name, p in G.named_parameters()}, reports


def _images(loss, G, batch):
    """The two images Gmain formed, again (the stand-ins are deterministic without style mixing)."""
    real_c, cat_feats = G.style_encoding(batch['style_input'], batch['retain'])
    gen_img, gen_finetune_img, _, _ = loss.run_G(torch.zeros([BATCH, 0], device='cuda'), real_c, batch['pose'], cat_feats, batch['denorm_upper_mask'],
                                                 batch['denorm_lower_mask'], batch['denorm_upper_input'], batch['denorm_lower_input'], sync=False)
    return gen_img, gen_finetune_img


def test_gmain_reports_the_term_and_adds_its_gradient(world):
    from torch_utils.ops.ssim_loss import ssim_loss
    batch = world[2]
    c0 = (RES - WIDTH) // 2
    loss, G, with_term, reports = _gmain(world, ssim_weight=3, ssim_width=WIDTH)
    _, _, without, reports0 = _gmain(world, ssim_weight=0)
    assert 'Loss/G/ssim' in reports and 'Loss/G/ssim_finetune' in reports
    assert 'Loss/G/ssim' not in reports0 and 'Loss/G/ssim_finetune' not in reports0

    for p in G.parameters():
        p.grad = None
    gen_img, gen_finetune_img = _images(loss, G, batch)
    term = 3 * ssim_loss(gen_img, batch['real_img'], c0, WIDTH)
    term_finetune = 3 * ssim_loss(gen_finetune_img, batch['real_img'], c0, WIDTH)
    assert abs(float(reports['Loss/G/ssim'].detach()) - float(term.detach())) <= 1e-6 and abs(float(reports['Loss/G/ssim_finetune'].detach()) - float(term_finetune.detach())) <= 1e-6
    assert 0 < float(term.detach()) < 6 and 0 < float(term_finetune.detach()) < 6
    names = [name for name, p in G.named_parameters()]
    alone = torch.autograd.grad((term + term_finetune) / 2, [p for _, p in G.named_parameters()], allow_unused=True)
    touched = 0
    for name, g in zip(names, alone):
        if with_term[name] is None:
            assert without[name] is None and g is None, name
            continue
        want = without[name] if g is None else without[name] + g
        err = rel_err(with_term[name], want)
        print(f'{name}: {err:.2e}' + ('' if g is None else f' (the term alone: {float(g.abs().max()):.2e} of {float(want.abs().max()):.2e})'))
        assert err < 1e-3, (name, err)
        if g is not None and float(g.abs().max()) > 1e-3 * float(want.abs().max()):
            touched += 1
            assert not torch.equal(with_term[name], without[name]), name
    assert touched >= 6         # the term reaches the synthesis layers and the encoders


def test_weight_zero_is_the_loss_without_the_keyword(world, monkeypatch):
    from torch_utils.ops import ssim_loss as op
    def never(*args, **kwargs):
        raise AssertionError('ssim_loss ran with weight 0')
    monkeypatch.setattr(op, 'ssim_loss', never)
    _, _, zero, reports_zero = _gmain(world, ssim_weight=0)
    _, _, plain, reports_plain = _gmain(world)
    assert sorted(reports_zero) == sorted(reports_plain) and not any('ssim' in name for name in reports_plain)
    assert list(zero) == list(plain)
    for name in plain:
        assert (zero[name] is None) == (plain[name] is None)
        if plain[name] is not None:
            assert torch.equal(zero[name], plain[name]), name


# ---- the command ----

_TRAIN_SCRIPT = '''
import sys
import train_wo_flow_fullbody as T

real_loop = T.training_loop.training_loop

def small_loop(**kwargs):
    cfg = kwargs['cfg']
    cfg.G_kwargs.synthesis_kwargs.channel_base = cfg.D_kwargs.channel_base = 2048
    cfg.D_kwargs.epilogue_kwargs.mbstd_group_size = 2
    kwargs.update(total_kimg=kwargs['total_kimg'] * %d / 1000, kimg_per_tick=3 * %d / 1000, snapshot_gnum=3)
    return real_loop(**kwargs)

T.training_loop.training_loop = small_loop
T.main(sys.argv[1:], standalone_mode=False)
''' % (BATCH, BATCH)


def _process(cmd, seconds, **kwargs):
    r = subprocess.run(['timeout', '-k', '10', str(seconds)] + cmd, capture_output=True, text=True, cwd=ROOT, **kwargs)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout


def _ssim_rows(run_dir):
    rows = [json.loads(line) for line in open(os.path.join(run_dir, 'stats.jsonl'))]
    assert rows
    for row in rows:
        for name in ('Loss/G/ssim', 'Loss/G/ssim_finetune'):
            assert name in row, (name, sorted(row))
            assert row[name]['num'] > 0 and 0 <= row[name]['mean'] <= 10, (name, row[name])
    return rows


def test_a_run_with_the_option_and_its_continuation(tmp_path):
    """The smallest run the run tests use (tests/test_train_continue_gpu.py), with --ssim_weight 5, then continued."""
    tree = make_tree(tmp_path / 'tree')
    script = tmp_path / 'train_small.py'
    script.write_text(_TRAIN_SCRIPT)
    env = dict(os.environ, PYTHONPATH=PKG)
    out_dir = tmp_path / 'runs'
    common = ['--data', tree, '--gpus', '1', '--cfg', 'fashion', '--batch', str(BATCH), '--snap', '1', '--aug', 'noaug', '--fp32', 'true',
              '--l1_weight', '40', '--mask_weight', '20']
    _process([sys.executable, str(script), '--outdir', str(out_dir), *common, '--ssim_weight', '5', '--kimg', '2'], 300, env=env)
    (first,) = os.listdir(out_dir)
    assert first.endswith('-ssim5')
    options = json.load(open(out_dir / first / 'training_options.json'))
    assert options['cfg']['loss_kwargs']['ssim_weight'] == 5 and options['cfg']['loss_kwargs']['ssim_width'] == 192
    _ssim_rows(out_dir / first)
    out = _process([sys.executable, str(script), '--outdir', str(out_dir), '--data', tree, '--continue', str(out_dir / first), '--kimg', '3'],
                   300, env=env)
    assert 'Continuing from' in out
    (second,) = [d for d in os.listdir(out_dir) if d != first]
    kept = json.load(open(out_dir / second / 'training_options.json'))
    assert kept['cfg']['loss_kwargs'] == options['cfg']['loss_kwargs']
    _ssim_rows(out_dir / second)
