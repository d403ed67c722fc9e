"""``StyleGAN2Loss(swap_cx_weight=)``: one Gmain call of ``accumulate_gradients`` on the stand-in networks and the
synthetic batch of tests/test_swap_outfits_gpu.py (32 x 32, two people).  What it reports against the fp32 statement of
tests/contextual_ref.py on VGG features and masks built here with torch ops, within the bound of
tests/test_contextual_loss_gpu.py; that the term moves the generator; and that a weight of 0 is the loss without the keyword."""
import copy

import pytest
import torch

import contextual_ref as R

pytestmark = pytest.mark.gpu

RES, BATCH = 32, 2


@pytest.fixture(scope='module')
def world():
    import tiny_models
    from training.training_loop_wo_flow_fullbody import SyntheticFullBodyBatch
    torch.manual_seed(3)
    dev = torch.device('cuda')
    G, D = tiny_models.TinyG().to(dev), tiny_models.TinyD().to(dev)
    (batch,) = SyntheticFullBodyBatch(BATCH, dev, seed=1, res=RES).split(BATCH)
    swap = {'swap_' + k: batch[k].flip(0).contiguous() for k in ('style_input', 'denorm_upper_input', 'denorm_lower_input', 'denorm_upper_mask',
                                                                'denorm_lower_mask')}
    # the kept parts on the left; the garment masks are bands that overlap in the middle rows: all three regions have pixels
    batch = dict(batch)
    keep = torch.zeros([BATCH, RES, RES], dtype=torch.uint8, device=dev)
    keep[:, :, :RES // 3] = 1
    batch['retain'] = torch.where(keep[:, None] != 0, batch['real_img'], -torch.ones_like(batch['real_img']))
    batch['pose'] = torch.cat([batch['pose'][:, :3], batch['retain']], dim=1)
    rows = torch.arange(RES, device=dev).reshape(1, 1, RES, 1).expand(BATCH, 1, RES, RES)
    swap['swap_denorm_upper_mask'] = (rows < 5 * RES // 8).float().contiguous()
    swap['swap_denorm_lower_mask'] = (rows >= 3 * RES // 8).float().contiguous()
    swap['swap_keep'] = keep
    return G, D, batch, swap


@pytest.fixture(scope='module', autouse=True)
def deterministic_stock_convolutions():
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def _loss(G, D, reports, **loss_kwargs):
    from training.loss_wo_flow_fullbody import StyleGAN2Loss
    return StyleGAN2Loss(torch.device('cuda'), G.mapping, G.synthesis, G.const_encoding, G.style_encoding, D, style_mixing_prob=0, l1_weight=40,
                         vgg_weight=0, contextual_weight=0, mask_weight=20, report_fn=lambda name, value: reports.__setitem__(name, value),
                         **loss_kwargs)


def _gmain(world, **loss_kwargs):
    """One accumulate_gradients('Gmain') on copies of the networks: ({name: gradient} of G, {report: value})."""
    G, D, batch, swap = copy.deepcopy(world[0]), copy.deepcopy(world[1]), world[2], world[3]
    reports = {}
    loss = _loss(G, D, reports, **loss_kwargs)
    G.requires_grad_(True)
    D.requires_grad_(False)
    loss.accumulate_gradients(phase='Gmain', gen_z=torch.zeros([BATCH, 0], device='cuda'), sync=False, gain=1, **batch, **swap)
    return {n: p.grad for n, p in G.named_parameters()}, reports


@pytest.fixture(scope='module')
def runs(world, deterministic_stock_convolutions):
    return {key: _gmain(world, **kw) for key, kw in (('cx', dict(swap_weight=1, swap_cx_weight=2)), ('zero', dict(swap_weight=1, swap_cx_weight=0)),
                                                    ('plain', dict(swap_weight=1)))}


def test_the_reports_are_the_statement_on_the_same_features(world, runs):
    G, D, batch, swap = world
    reports = runs['cx'][1]
    loss = _loss(G, D, {}, swap_weight=1, swap_cx_weight=2)
    s = {k[len('swap_'):]: v for k, v in swap.items()}
    bound_v, _ = R.bounds()          # differentiates the statement: outside no_grad
    with torch.no_grad():
        x_s, x_s_ft, _ = loss._run_G_swapped(torch.zeros([BATCH, 0], device='cuda'), batch['retain'], batch['pose'], s, False, False)
        kept = s['keep'][:, None] != 0
        upper = ~kept & (s['denorm_upper_mask'] != 0)
        lower = ~kept & ~upper & (s['denorm_lower_mask'] != 0)
        assert bool(upper.any()) and bool(lower.any())
        target = s['denorm_upper_input'] * upper + s['denorm_lower_input'] * lower
        union = (upper | lower).float()
        feats = [loss.cx_vgg(x.float() * union)[2:4] for x in (x_s, x_s_ft)]
        target_feats = loss.cx_vgg(target)[2:4]
        assert [tuple(f.shape[1:]) for f in target_feats] == [(256, RES // 4, RES // 4), (512, RES // 8, RES // 8)]
        for name, region in (('upper', upper), ('lower', lower)):
            values = []
            for tap, stride in ((0, 4), (1, 8)):
                valid = (torch.nn.functional.avg_pool2d(region.float(), stride) >= 0.5)[:, 0].to(torch.uint8)
                assert bool(valid.any())
                for image in feats:
                    values.append(R.statement(image[tap], target_feats[tap], valid, valid))
            want = float(torch.stack(values).mean())
            got = float(reports['Loss/G/swap_cx_' + name].detach())
            print('%s: reported %.8g, statement %.8g, deviation %.3e (bound %.3e)' % (name, got, want, abs(got - want) / max(abs(want), R.VALUE_FLOOR),
                                                                                     bound_v))
            assert want > 0 and abs(got - want) <= bound_v * max(abs(want), R.VALUE_FLOOR), name


def test_the_term_moves_the_generator(runs):
    with_term, without = runs['cx'][0], runs['zero'][0]
    assert not any('swap_cx' in name for name in runs['zero'][1])
    changed = [name for name, g in with_term.items() if g is not None and not torch.equal(g, without[name])]
    assert changed and all(torch.isfinite(g).all() for g in with_term.values() if g is not None)


def test_weight_zero_is_the_loss_without_the_keyword(runs):
    (zero, zero_reports), (plain, plain_reports) = runs['zero'], runs['plain']
    assert list(zero) == list(plain) and sorted(zero_reports) == sorted(plain_reports)
    for name in plain:
        assert (zero[name] is None) == (plain[name] is None)
        if plain[name] is not None:
            assert torch.equal(zero[name], plain[name]), name
    for name in plain_reports:
        assert torch.equal(torch.as_tensor(zero_reports[name]).detach().cpu(), torch.as_tensor(plain_reports[name]).detach().cpu()), name
