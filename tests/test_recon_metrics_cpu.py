"""The reconstruction metric without a GPU: the numpy restatement (tests/recon_ref.py) against closed forms, the registry and
the report format of metrics/metric_main.py, the partials -> results step on CPU tensors, and the two command lines."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from click.testing import CliRunner

import recon_ref as R
from conftest import ROOT
from train_grid_tree import make_tree

KEYS = ('l1', 'psnr', 'ssim', 'miou', 'pixacc')


# ---- the oracle against closed forms ----

def test_ssim_of_an_image_with_itself_is_one():
    x = np.random.default_rng(0).integers(0, 256, [29, 23])
    assert np.allclose(R.ssim_map(x, x), 1.0, rtol=0, atol=1e-12)
    assert R.ssim_map(x, x).shape == (19, 13)
    assert abs(R.window().sum() - 1) < 1e-15 and R.window().shape == (11, 11)


@pytest.mark.parametrize('a, b', [(0, 255), (10, 200), (128, 128), (255, 254)])
def test_ssim_of_two_constant_images(a, b):
    got = R.ssim_map(np.full([12, 15], a), np.full([12, 15], b))
    want = (2.0 * a * b + R.C1) / (a * a + b * b + R.C1)        # the variances vanish: the second factor is C2 / C2
    assert got.shape == (2, 5) and np.allclose(got, want, rtol=0, atol=1e-9)


def test_byte_rule():
    x = np.array([-1.0, 1.0, 0.0, -3.0, 7.0, np.nan, np.inf, -np.inf, 2.5 / 127.5 - 1, 0.999], np.float32)
    assert R.to_u8(x).tolist() == [0, 255, 127, 0, 255, 0, 255, 0, 2, 254]


def test_psnr_by_hand():
    from metrics import reconstruction as M
    # image 0: every one of its 300 bytes off by 2 -> MSE 4; image 1: identical -> MSE floored at 255^2 * 1e-10 = 100 dB
    p = M.new_partials(2, 6)
    ssim = torch.tensor([75.0, 150.0], dtype=torch.float64)
    p['items'][:, 0] = torch.tensor([600, 0])
    p['items'][:, 1] = torch.tensor([1200, 0])
    p['items'][:, 2] = 150
    p['items'][:, 3] = 300
    p['items'][:, 4] = ssim.view(torch.int64)
    p['confusion'][0, 0] = 1
    r = M.finish(p, 'm')
    assert sorted(r) == sorted('m_' + k for k in KEYS)
    assert r['m_psnr'] == pytest.approx((10 * np.log10(255.0 ** 2 / 4.0) + 100.0) / 2, rel=1e-13)
    assert r['m_psnr'] == pytest.approx((42.110204 + 100) / 2, abs=1e-6)        # 20 log10(255 / 2)
    assert r['m_l1'] == pytest.approx(600 / 600 / 255, rel=1e-15)
    assert r['m_ssim'] == pytest.approx(0.75, rel=1e-15)


def test_miou_of_a_matrix_with_an_empty_class():
    from metrics import reconstruction as M
    #            predicted 0  1  2  3
    m = torch.tensor([[5, 1, 0, 0],      # label 0
                      [2, 6, 0, 0],      # label 1
                      [0, 0, 0, 0],      # label 2: never labelled, never predicted -> no union, left out
                      [0, 3, 0, 0]])     # label 3: never predicted -> IoU 0
    miou, pixacc = M.confusion_scores(m)
    assert miou == pytest.approx((5 / 8 + 6 / 12 + 0 / 3) / 3, rel=1e-15)
    assert pixacc == pytest.approx(11 / 17, rel=1e-15)
    want = R.results([1], [1], [1], [1], [1], m.numpy())
    assert miou == pytest.approx(want['miou'], rel=1e-15) and pixacc == pytest.approx(want['pixacc'], rel=1e-15)
    assert all(np.isnan(v) for v in M.confusion_scores(torch.zeros([4, 4], dtype=torch.int64)))


def test_confusion_rules_of_the_oracle():
    nan = np.nan
    logits = np.array([[1, 1, 0], [nan, 2, 2], [nan, nan, nan], [0, nan, 3], [-np.inf, nan, -np.inf], [4, 0, 0], [0, 5, 0]], np.float64)
    labels = np.array([2, 0, 1, 1, 2, 255, 3], np.float64)
    lg = logits.T.reshape(1, 3, 1, 7)
    m = R.confusion(lg, labels.reshape(1, 1, 1, 7), 0, 7)
    want = np.zeros([3, 3], np.int64)
    for lab, pred in [(2, 0), (0, 1), (1, 0), (1, 2), (2, 0)]:      # ties -> lowest; NaN never wins; all NaN -> 0; 255 and 3 skipped
        want[lab, pred] += 1
    assert np.array_equal(m, want)
    assert np.array_equal(R.confusion(lg, labels.reshape(1, 1, 1, 7), 2, 3), np.array([[0, 0, 0], [1, 0, 1], [1, 0, 0]]))


def test_z_is_drawn_per_item_from_its_raw_index():
    from metrics import reconstruction as M
    z = M.item_z([7, 0, 123456, 7], 5, 'cpu')
    assert z.dtype == torch.float32 and tuple(z.shape) == (4, 5)
    want = np.stack([np.random.RandomState(i).randn(5) for i in (7, 0, 123456, 7)]).astype(np.float32)
    assert np.array_equal(z.numpy(), want) and np.array_equal(z.numpy(), R.item_z([7, 0, 123456, 7], 5))
    assert torch.equal(z[0], z[3]) and torch.equal(M.item_z([123456], 5, 'cpu')[0], z[2])      # no dependence on the batch
    assert np.random.RandomState(7).randn(5)[0] == pytest.approx(1.6905257)                    # the generator meant, by its first draw
    assert tuple(M.item_z([1, 2], 0, 'cpu').shape) == (2, 0) and R.item_z([1, 2], 0).shape == (2, 0)


# ---- registry and report ----

def test_registry():
    from metrics import metric_main
    assert metric_main.list_valid_metrics() == ['recon_full', 'recon2k']
    assert metric_main.is_valid_metric('recon_full') and metric_main.is_valid_metric('recon2k')
    for name in ('fid50k_full', 'kid50k_full', 'pr50k3_full', 'ppl2_wend', 'is50k', 'recon', ''):
        assert not metric_main.is_valid_metric(name)
    with pytest.raises(ValueError, match='recon_full, recon2k'):
        metric_main.calc_metric('fid50k_full', G=None, dataset_kwargs={}, num_gpus=1, rank=0, device=torch.device('cpu'))

    @metric_main.register_metric
    def recon_test_only(opts):
        return dict(recon_test_only_x=opts.num_gpus + 0.5)
    try:
        r = metric_main.calc_metric('recon_test_only', G=None, dataset_kwargs=dict(path='x'), num_gpus=1, rank=0, device=torch.device('cpu'))
        assert sorted(r) == ['metric', 'num_gpus', 'results', 'total_time', 'total_time_str'] and r.results == dict(recon_test_only_x=1.5)
        assert r.metric == 'recon_test_only' and r.num_gpus == 1 and isinstance(r.total_time_str, str)
    finally:
        del metric_main._metrics['recon_test_only']


def test_report_metric_writes_the_line(tmp_path, capsys):
    import dnnlib
    from metrics import metric_main
    run_dir = tmp_path / '00000-run'
    run_dir.mkdir()
    result = dnnlib.EasyDict(results=dnnlib.EasyDict(recon_full_l1=0.25, recon_full_psnr=12.5), metric='recon_full', total_time=1.5,
                             total_time_str='1s', num_gpus=1)
    metric_main.report_metric(result, run_dir=str(run_dir), snapshot_pkl=str(run_dir / 'network-snapshot-000123.pkl'))
    metric_main.report_metric(result, run_dir=str(run_dir), snapshot_pkl=str(run_dir / 'network-snapshot-000246.pkl'))
    lines = (run_dir / 'metric-recon_full.jsonl').read_text().splitlines()
    assert capsys.readouterr().out.splitlines() == lines and len(lines) == 2
    first, second = (json.loads(line) for line in lines)
    assert sorted(first) == ['metric', 'num_gpus', 'results', 'snapshot_pkl', 'timestamp', 'total_time', 'total_time_str']
    assert first['results'] == dict(recon_full_l1=0.25, recon_full_psnr=12.5) and first['metric'] == 'recon_full'
    assert first['snapshot_pkl'] == 'network-snapshot-000123.pkl' and second['snapshot_pkl'] == 'network-snapshot-000246.pkl'
    assert isinstance(first['timestamp'], float)
    # without a run directory: printed only, the path as given
    metric_main.report_metric(result, snapshot_pkl='/somewhere/s.pkl')
    assert json.loads(capsys.readouterr().out)['snapshot_pkl'] == '/somewhere/s.pkl'
    assert sorted(os.listdir(run_dir)) == ['metric-recon_full.jsonl']


# ---- combining ----

def _partials(num_items, rng):
    from metrics import reconstruction as M
    p = M.new_partials(num_items, 6)
    nbytes = 256 * 192 * 3
    p['items'][:, 0] = torch.from_numpy(rng.integers(0, 255 * nbytes, num_items))
    p['items'][:, 1] = torch.from_numpy(rng.integers(0, 255 * 255 * nbytes, num_items))
    p['items'][:, 2] = 3 * 246 * 182
    p['items'][:, 3] = nbytes
    p['items'][:, 4] = torch.from_numpy(rng.uniform(-0.2, 1.0, num_items) * 3 * 246 * 182).view(torch.int64)
    p['items'][3, 1] = 0                                             # one image at the PSNR cap
    p['confusion'] += torch.from_numpy(rng.integers(0, 10 ** 6, [6, 6]))
    p['confusion'][4] = 0
    p['confusion'][:, 4] = 0
    return p


@pytest.mark.parametrize('ways', [1, 2, 3])
def test_results_do_not_depend_on_how_the_partials_are_split(ways):
    from metrics import reconstruction as M
    rng = np.random.default_rng(5)
    whole = _partials(11, rng)
    want = M.finish(whole, 'recon_full')
    assert all(np.isfinite(v) for v in want.values())
    # rank r of `ways` owns items r, r + ways, ...; the confusion matrix splits into arbitrary integer shares
    parts = []
    left = whole['confusion'].clone()
    for r in range(ways):
        p = M.new_partials(11, 6)
        p['items'][r::ways] = whole['items'][r::ways]
        share = left if r == ways - 1 else left // (r + 2)
        p['confusion'] += share
        left = left - share
        parts.append(p)
    combined = M.combine_partials(parts)
    assert torch.equal(combined['items'], whole['items']) and torch.equal(combined['confusion'], whole['confusion'])
    assert M.finish(combined, 'recon_full') == want                 # bit for bit
    assert torch.equal(whole['items'], _partials(11, np.random.default_rng(5))['items'])     # inputs untouched
    with pytest.raises(ValueError, match='not scored'):
        M.finish(parts[0] if ways > 1 else M.new_partials(11, 6), 'recon_full')


def test_results_against_the_oracle_formulas():
    from metrics import reconstruction as M
    p = _partials(7, np.random.default_rng(9))
    items = p['items'].numpy()
    want = R.results(items[:, 0], items[:, 1], items[:, 4].view(np.float64), items[:, 2], items[:, 3], p['confusion'].numpy())
    got = M.finish(p, 'x')
    for k in KEYS:
        assert got['x_' + k] == pytest.approx(want[k], rel=1e-13), k


# ---- command lines ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('recon_cli'))


def _train(tree, outdir, *extra):
    import train_wo_flow_fullbody as T
    return CliRunner().invoke(T.main, ['--outdir', str(outdir), '--data', tree, '--dry-run', *extra])


def _options(output):
    text = output[output.index('Training options:') + len('Training options:'):output.index('Output directory:')]
    return json.loads(text)


def test_train_accepts_and_records_the_metrics(tree, tmp_path):
    res = _train(tree, tmp_path / 'runs', '--metrics', 'recon_full,recon2k', '--metrics_data', tree)
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    assert o['metrics'] == ['recon_full', 'recon2k']
    assert o['metric_set_kwargs']['path'] == tree and o['metric_set_kwargs']['class_name'] == 'training.dataset.UvitonDatasetFull'
    res = _train(tree, tmp_path / 'runs', '--metrics', 'recon_full')
    assert res.exit_code == 0, res.output
    o = _options(res.output)
    assert o['metrics'] == ['recon_full'] and o['metric_set_kwargs'] is None
    for none in ([], ['--metrics', 'none']):
        res = _train(tree, tmp_path / 'runs', *none)
        assert res.exit_code == 0 and _options(res.output)['metrics'] == []


def test_train_loop_takes_the_recorded_options(tree, tmp_path):
    import inspect
    from training.training_loop_wo_flow_fullbody import training_loop
    o = _options(_train(tree, tmp_path / 'runs', '--metrics', 'recon_full').output)
    params = inspect.signature(training_loop).parameters
    assert set(o) - {'run_dir'} <= set(params) and params['metrics'].default is None and params['metric_set_kwargs'].default is None


@pytest.mark.parametrize('extra, message', [
    (['--metrics', 'fid50k_full'], 'metric call commented out'),
    (['--metrics', 'recon_full,kid50k_full'], 'kid50k_full'),
    (['--metrics_data', 'x'], 'needs --metrics'),
    (['--metrics', 'recon_full', '--metrics_data', '/nonexistent/tree'], '--metrics_data'),
])
def test_train_still_refuses(tree, tmp_path, extra, message):
    res = _train(tree, tmp_path / 'runs', *extra)
    assert res.exit_code != 0
    assert message in res.output, res.output


def test_calc_metrics_refuses_an_unknown_metric(tmp_path):
    cli = os.path.join(ROOT, 'pasta-gan_amd', 'calc_metrics.py')
    r = subprocess.run([sys.executable, cli, '--metrics', 'nope', '--network', str(tmp_path / 'none.pkl')], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert 'nope' in r.stderr and 'recon_full' in r.stderr and 'recon2k' in r.stderr, r.stderr
    r = subprocess.run([sys.executable, cli, '--network', 'https://example.com/snapshot.pkl'], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert r.returncode != 0 and 'URL' in r.stderr, r.stderr
    r = subprocess.run([sys.executable, cli, '--help'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0
    for opt in ('--network', '--metrics', '--data', '--gpus', '--verbose'):
        assert opt in r.stdout
    assert 'recon_full' in r.stdout                                 # the default
