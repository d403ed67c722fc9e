"""16-bit activation storage through the real commands: train_wo_flow_fullbody.py ``--storage bf16`` on the tiny 256 tree
and on the tiny 512 tree -- batches from the builders, ADA (the command's default), the sample grid, the snapshot, the state
file, ``--continue`` and ``--resume`` -- and ``--storage`` of test.py, test_512.py and calc_metrics.py.  Every command runs in a
child process, shrunk as tests/test_train_continue_gpu.py and tests/test_tryon_512_train_gpu.py shrink it (their scripts: test-size
widths, a 3 x 3 grid, ``--kimg N`` read as N iterations at 256, one tick of one iteration at 512).

Continuing is held to what tests/test_train_continue_gpu.py holds the fp32 command to, and that file's control passes bit for bit:
the state of the continued run against the straight run's, entry by entry with ``torch.equal`` (every parameter and buffer of G, D
and G_ema, the optimisers, the generators' states, ADA's accumulator), excluding what it excludes -- ``elapsed_sec`` and the
recorded options, which name the run directories -- and no more.

test.py reads pairs whose patch stack has 60 channels, the released ``GeneratorV18``'s; the 256 training generator takes 42.  So
test.py's snapshots here are pickles of a filled ``GeneratorV18``, one constructed in bf16 storage ("the bf16 snapshot") and one in
fp32 with the same parameters, as tests/test_tryon_fidelity_gpu.py makes its own; the TRAINED bf16 snapshot goes through
test_512.py (512 tree) and the trained fp32 one through calc_metrics.py."""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
from oracle import param_fill as PF
import recon_ref as RR
from test_calc_metrics_gpu import _oracle_sums
from test_train_continue_gpu import _TRAIN_SCRIPT, _diff, _file, _process, _spread
from test_tryon_fidelity_gpu import _same
from test_tryon_512_train_gpu import _TRAIN_SCRIPT as _TRAIN_SCRIPT_512
from train_grid_tree import make_tree
from tryon_512_train_tree import make_512_train_tree
from tryon_512_tree import PAIRS as PAIRS_512, make_512_tree
from tryon_pairs_tree import PAIRS, make_pair_tree

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
BATCH = 2                       # of _TRAIN_SCRIPT
ENV = dict(os.environ, PYTHONPATH=PKG)
LOSSES = ('--l1_weight', '40', '--mask_weight', '20')


def _load(path):
    import legacy
    with open(path, 'rb') as f:
        return legacy.load_network_pkl(f)


def _only_run(outdir, but=()):
    (name,) = [d for d in os.listdir(outdir) if d not in but]
    return outdir / name


def _stats(run_dir):
    return [json.loads(line) for line in open(run_dir / 'stats.jsonl')]


def _finite_losses(line):
    losses = {k: v['mean'] for k, v in line.items() if k.startswith('Loss/')}
    assert losses and all(np.isfinite(v) for v in losses.values()), losses
    return losses


def _in_bf16_storage(data, top):
    for name in ('G', 'G_ema'):
        syn = data[name].synthesis
        assert syn.act_dtype == BF16, name
        blocks = [getattr(syn, f'b{2 ** k}') for k in range(2, int(np.log2(top)) + 1)] + [getattr(syn, f'texture_b{top}')]
        assert all(b.use_fp16 and b.half_dtype == BF16 for b in blocks), name
    assert all(getattr(data['D'], f'b{2 ** k}').use_fp16 and getattr(data['D'], f'b{2 ** k}').half_dtype == BF16 for k in range(3, int(np.log2(top)) + 1))
    for name in ('G', 'G_ema', 'D'):
        assert all(p.dtype == torch.float32 for p in data[name].parameters()), name         # fp32 masters


# ---- training at 256: the run, its continuation, --resume ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('storage_run_256'))


@pytest.fixture(scope='module')
def script(tmp_path_factory):
    path = tmp_path_factory.mktemp('storage_run_scripts') / 'train_small.py'
    path.write_text(_TRAIN_SCRIPT)
    return str(path)


def _train(script, outdir, tree, *extra):
    return _process([sys.executable, script, '--outdir', str(outdir), '--data', tree, '--gpus', '1', '--cfg', 'fashion', '--batch', str(BATCH),
                     '--snap', '1', *LOSSES, *extra], 600, env=ENV)


@pytest.fixture(scope='module')
def straight(script, tree, tmp_path_factory):
    """``--storage bf16`` with the default augmentation (ADA) for 6 iterations: ticks close after iterations 1, 4 and 6."""
    outdir = tmp_path_factory.mktemp('storage_straight')
    out = _train(script, outdir, tree, '--storage', 'bf16', '--kimg', '6')
    return out, _only_run(outdir)


@pytest.fixture(scope='module')
def cut(script, tree, tmp_path_factory):
    """The same command stopped after 3 iterations."""
    outdir = tmp_path_factory.mktemp('storage_cut')
    _train(script, outdir, tree, '--storage', 'bf16', '--kimg', '3')
    return outdir, _only_run(outdir)


@pytest.fixture(scope='module')
def fp32_run(script, tree, tmp_path_factory):
    """The command without the option (fp32 storage) for one tick: the snapshot that --resume and calc_metrics.py take."""
    outdir = tmp_path_factory.mktemp('storage_fp32')
    _train(script, outdir, tree, '--kimg', '1')
    return _only_run(outdir)


def test_training_run_in_bf16_storage(straight, cut):
    import PIL.Image
    out, run_dir = straight
    assert '"act_dtype": "bfloat16"' in out and '"half_dtype": "bfloat16"' in out and '"ada_target"' in out
    assert os.path.basename(run_dir).endswith('-bf16')
    lines = _stats(run_dir)
    assert [line['Progress/tick']['mean'] for line in lines] == [0, 1, 2]
    for line in lines:
        _finite_losses(line)
    assert PIL.Image.open(run_dir / 'fakes000000_finetune.png').size == (4 * 256, 4 * 256)
    data = _load(run_dir / 'network-snapshot-000000.pkl')
    assert sorted(data) == ['D', 'G', 'G_ema', 'augment_pipe', 'training_set_kwargs']
    _in_bf16_storage(data, 256)
    state = _file(run_dir)[1]
    assert data['augment_pipe'] is not None and 'augment_pipe' in state and float(state['ranks'][0]['ada_acc'][1]) > 0       # ADA ran
    assert json.loads(state['options'])['cfg']['G_kwargs']['synthesis_kwargs']['act_dtype'] == 'bfloat16'
    for name in ('G', 'G_ema', 'D'):
        named = dict(list(data[name].named_parameters()) + list(data[name].named_buffers()))
        assert all(torch.equal(named[k].detach().cpu(), state[name][k]) for k in named), name
        assert all(bool(torch.isfinite(t).all()) for t in named.values()), name
    # every parameter of D has moved: between the third iteration (the cut run's state) and the sixth
    earlier = _file(cut[1])[1]['D']
    stuck = [k for k, p in data['D'].named_parameters() if torch.equal(p.detach().cpu(), earlier[k])]
    assert stuck == [], stuck


def test_continued_bf16_run_equals_the_straight_one(script, tree, straight, cut):
    outdir, first = cut
    assert _file(first)[1]['batch_idx'] == 3
    out = _process([sys.executable, script, '--outdir', str(outdir), '--data', tree, '--continue', str(first), '--kimg', '6'], 600, env=ENV)
    assert 'Continuing from' in out and '"act_dtype": "bfloat16"' in out
    second = _only_run(outdir, but=(os.path.basename(first),))
    assert os.path.basename(second) == '00001-' + os.path.basename(first)[len('00000-'):] + '-continue000000'
    got, want = _file(second)[1], _file(straight[1])[1]
    assert got['batch_idx'] == want['batch_idx'] == 6 and got['cur_tick'] == want['cur_tick'] == 3 and 'augment_pipe' in got
    got.pop('options'), want.pop('options')             # the run directories and --kimg differ, nothing else may
    _spread('bf16 storage, command line: continued against straight', got, want)
    assert _diff(got, want) == []
    assert sorted(got['G']) == sorted(want['G']) and sorted(got['D']) == sorted(want['D']) and sorted(got['G_ema']) == sorted(want['G_ema'])
    _in_bf16_storage(_load(second / 'network-snapshot-000000.pkl'), 256)


def test_resume_an_fp32_snapshot_in_bf16_storage(script, tree, fp32_run, tmp_path):
    pkl = fp32_run / 'network-snapshot-000000.pkl'
    before = _load(pkl)
    assert before['G'].synthesis.act_dtype is None and not before['D'].b8.use_fp16 and before['D'].b256.use_fp16     # mixed precision as before
    out = _train(script, tmp_path / 'runs', tree, '--storage', 'bf16', '--kimg', '1', '--resume', str(pkl))
    assert 'Resuming from' in out
    run_dir = _only_run(tmp_path / 'runs')
    assert os.path.basename(run_dir).endswith('-resumecustom-bf16')
    (line,) = _stats(run_dir)
    assert line['Progress/tick']['mean'] == 0
    _finite_losses(line)
    _in_bf16_storage(_load(run_dir / 'network-snapshot-000000.pkl'), 256)


# ---- training at 512, and test_512.py on its snapshot ----

def test_training_at_512_in_bf16_storage_then_try_on(tmp_path):
    import PIL.Image
    tree = make_512_train_tree(tmp_path / 'train512')
    script = tmp_path / 'train_small_512.py'
    script.write_text(_TRAIN_SCRIPT_512)
    out = _process([sys.executable, str(script), '--outdir', str(tmp_path / 'runs'), '--data', tree, '--gpus', '1', '--cfg', 'fashion', '--batch', '4',
                    '--snap', '1', *LOSSES, '--storage', 'bf16'], 600, env=ENV)
    assert 'UvitonDatasetFull_512' in out and '"patch_channels": 45' in out and '"act_dtype": "bfloat16"' in out and '"num_fp16_res": 7' in out
    run_dir = _only_run(tmp_path / 'runs')
    (line,) = _stats(run_dir)
    _finite_losses(line)
    assert PIL.Image.open(run_dir / 'fakes000000_finetune.png').size == (4 * 512, 4 * 512)
    pkl = run_dir / 'network-snapshot-000000.pkl'
    data = _load(pkl)
    _in_bf16_storage(data, 512)
    assert data['G_ema'].style_encoding.model[0].weight.shape[1] == 45
    pair_tree = make_512_tree(tmp_path / 'pairs512')
    for name, extra in (('as_pickled', []), ('f32', ['--storage', 'f32'])):
        _process([sys.executable, os.path.join(PKG, 'test_512.py'), '--network', str(pkl), '--outdir', str(tmp_path / name), '--dataroot', pair_tree,
                  '--batchsize', '2', '--noise-mode', 'const', '--workers', '0', '--change-region', 'upperbody', *extra], 600)
        assert sorted(os.listdir(tmp_path / name)) == ['%03d.png' % i for i in range(len(PAIRS_512))]
    differ = 0
    for i in range(len(PAIRS_512)):
        a, b = (np.asarray(PIL.Image.open(tmp_path / name / ('%03d.png' % i))) for name in ('as_pickled', 'f32'))
        assert a.shape == b.shape == (512, 3 * 512, 3) and len(np.unique(a[:, 2 * 512:])) > 1
        assert np.array_equal(a[:, :2 * 512], b[:, :2 * 512])           # clothes | person: the inputs
        differ += int(not np.array_equal(a[:, 2 * 512:], b[:, 2 * 512:]))
    assert differ > 0                                                   # the snapshot ran in bf16 as pickled, in fp32 with the option


# ---- test.py ----

@pytest.fixture(scope='module')
def pair_tree(tmp_path_factory):
    return make_pair_tree(tmp_path_factory.mktemp('storage_pairs'))


def _v18(dtype=None):
    from training import networks
    synthesis = dict(PF.G_KWARGS['synthesis_kwargs'], **(dict() if dtype is None else dict(act_dtype=dtype)))
    return PF.fill_module(networks.GeneratorV18(**dict(PF.G_KWARGS, synthesis_kwargs=synthesis))).eval().requires_grad_(False)


@pytest.fixture(scope='module')
def snapshots(tmp_path_factory):
    """{'f32' | 'bf16': path of a snapshot file whose GeneratorV18 was constructed in that storage}: the same parameters in both."""
    from training import networks
    root = tmp_path_factory.mktemp('storage_snapshots')
    D = networks.Discriminator(c_dim=512, img_resolution=256, img_channels=3, channel_base=512, channel_max=32)
    paths = {}
    for name, dtype in (('f32', None), ('bf16', 'bfloat16')):
        G = _v18(dtype)
        paths[name] = str(root / (name + '.pkl'))
        with open(paths[name], 'wb') as f:
            pickle.dump(dict(G=G, D=D, G_ema=G), f)
    return paths


def _images_in_process(G, pair_tree):
    """{file name relative to --outdir: the image} of test.py's call sequence on the builder's tensors, one batch of all pairs, z per pair."""
    import tryon_cli
    from metrics import tryon_fidelity as M
    from training.dataset import UvitonDatasetV19_test, collate_pairs
    from training.tryon_pairs import TryOnPairBatchBuilder, images_to_u8
    ds = UvitonDatasetV19_test(path=pair_tree)
    index = list(range(len(ds)))
    batch = TryOnPairBatchBuilder('cuda').build(collate_pairs([ds[i] for i in index]))
    t, z = batch.tensors, M.pair_z(index, G.z_dim, 'cuda')
    gen = tryon_cli.generate(G, t, z, 1, 'const')
    assert gen.dtype == torch.float32
    # the command's call sequence is the generator's own forward, the encoders in the storage type included
    with torch.no_grad():
        whole = G(z, t['style_input'], t['retain'], t['pose'], t['denorm_upper_input'], t['denorm_lower_input'], t['denorm_upper_mask'],
                  t['denorm_lower_mask'], noise_mode='const')[1]
    assert torch.equal(gen, whole)
    images = images_to_u8(gen, 32, 192).cpu().numpy()
    return {os.path.join(sub, p[:-4] + '__' + c[:-4] + '.png'): images[i] for i, (sub, p, c) in enumerate(PAIRS)}


def _test_py(pkl, outdir, pair_tree, *extra):
    import PIL.Image
    out = _process([sys.executable, os.path.join(PKG, 'test.py'), '--network', pkl, '--outdir', str(outdir), '--dataroot', pair_tree,
                    '--batchsize', str(len(PAIRS)), '--workers', '0', *extra], 600)
    names = {os.path.relpath(os.path.join(d, f), outdir) for d, _, fs in os.walk(outdir) for f in fs}
    return out, {name: np.asarray(PIL.Image.open(outdir / name)) for name in names}


def test_test_py_runs_a_bf16_snapshot_as_pickled(snapshots, pair_tree, tmp_path):
    G = _load(snapshots['bf16'])['G_ema'].cuda().eval().requires_grad_(False)
    assert G.synthesis.act_dtype == BF16 and G.synthesis.b256.use_fp16
    want = _images_in_process(G, pair_tree)
    _, got = _test_py(snapshots['bf16'], tmp_path / 'out', pair_tree)
    assert sorted(got) == sorted(want) and len(got) == len(PAIRS)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


def test_test_py_switches_an_fp32_snapshot(snapshots, pair_tree, tmp_path):
    from training.networks import set_activation_storage
    G = _load(snapshots['f32'])['G_ema'].cuda().eval().requires_grad_(False)
    assert G.synthesis.act_dtype is None
    want = _images_in_process(set_activation_storage(G, 'bfloat16'), pair_tree)
    out, got = _test_py(snapshots['f32'], tmp_path / 'bf16', pair_tree, '--storage', 'bf16', '--scores', str(tmp_path / 'bf16.json'))
    assert sorted(got) == sorted(want) and len(got) == len(PAIRS)
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    report = json.loads((tmp_path / 'bf16.json').read_text())
    assert report['storage'] == 'bf16' and sorted(report) == ['dataroot', 'network', 'noise_mode', 'pairs', 'results', 'storage']
    (printed,) = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{')]
    assert _same(printed, report)                       # the same line printed and written
    # without the option: other images, and the report's keys are exactly what they were
    _, plain = _test_py(snapshots['f32'], tmp_path / 'plain', pair_tree, '--scores', str(tmp_path / 'plain.json'))
    assert sorted(plain) == sorted(got)
    assert any(not np.array_equal(plain[name], got[name]) for name in got)
    plain_report = json.loads((tmp_path / 'plain.json').read_text())
    assert sorted(plain_report) == ['dataroot', 'network', 'noise_mode', 'pairs', 'results']
    assert sorted(plain_report['results']) == sorted(report['results']) and plain_report['pairs'] == report['pairs'] == len(PAIRS)


# ---- calc_metrics.py ----

def test_calc_metrics_scores_the_switched_generator(fp32_run, tree, monkeypatch):
    from metrics import metric_main, reconstruction
    from training.networks import set_activation_storage
    pkl = fp32_run / 'network-snapshot-000000.pkl'
    lines = {}
    for name, extra in (('bf16', ['--storage', 'bf16']), ('plain', [])):
        out = _process([sys.executable, os.path.join(PKG, 'calc_metrics.py'), '--network', str(pkl), '--metrics', 'recon_full', '--data', tree,
                        '--verbose', 'false', *extra], 600)
        (lines[name],) = [json.loads(ln) for ln in out.splitlines() if ln.startswith('{')]
    assert lines['bf16']['storage'] == 'bf16' and sorted(lines['bf16']) == sorted(list(lines['plain']) + ['storage'])
    assert sorted(lines['plain']) == ['metric', 'num_gpus', 'results', 'snapshot_pkl', 'timestamp', 'total_time', 'total_time_str']
    written = [json.loads(ln) for ln in open(fp32_run / 'metric-recon_full.jsonl')]
    assert written == [lines['bf16'], lines['plain']]                   # the run directory's file gets the same lines
    # the figures are those of the switched generator, scored in this process by the numpy restatement on G's own outputs (one batch of all
    # people, as the command's default batch size makes it) -- not through calc_metric, whose copy of G has to be handed the switch
    G = _load(pkl)['G_ema'].eval().requires_grad_(False).cuda()
    for name, dtype in (('plain', None), ('bf16', 'bfloat16')):
        set_activation_storage(G, dtype)
        (sad, ssd, ssim, windows, nbytes), conf = _oracle_sums(G, tree, 16)
        want = RR.results(sad, ssd, ssim, windows, nbytes, conf)
        got = {k: lines[name]['results']['recon_full_' + k] for k in want}
        print('recon_full of one snapshot, storage', name, got, 'oracle:', want)
        for k in ('l1', 'psnr', 'miou', 'pixacc'):
            assert got[k] == pytest.approx(want[k], rel=1e-12), (name, k)
        assert abs(got['ssim'] - want['ssim']) <= RR.SSIM_TOL, name
    # and the metric's own copy of the generator runs in the storage of the one it was given
    seen = []
    real = reconstruction.score_batch
    monkeypatch.setattr(reconstruction, 'score_batch', lambda G_, *args: (seen.append(G_.synthesis.b64.half_dtype if G_.synthesis.b64.use_fp16 else None),
                                                                          real(G_, *args))[1])
    kwargs = dict(dataset_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree), num_gpus=1, rank=0, device=torch.device('cuda'),
                  batch_size=16)
    switched = metric_main.calc_metric('recon_full', G=G, **kwargs).results
    plain = metric_main.calc_metric('recon_full', G=set_activation_storage(G, None), **kwargs).results
    assert seen == [BF16, None]
    assert lines['bf16']['results'] == dict(switched) and lines['plain']['results'] == dict(plain)
