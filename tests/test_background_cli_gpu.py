"""--background photo and --kept-garments photo of the two try-on commands on the tiny trees and snapshots of the
existing end-to-end tests: generate_256 with --change-region lowerbody (GeneratorV18: sigmoid heads) and generate_512 with an
outfit list that has a ``-`` in each position (GeneratorFull: parsing logits).  The written pictures are the numpy restatement's
paste (tests/keep_composite_ref.py) of the plain run's decoded bytes under the restated mask (tests/paste_mask_ref.py), formed
from the builder's stages and the heads of an in-process ``generate_outputs`` on the same batches; the defaults write what they
wrote; --scores describes the written bytes.  Every run compared uses one batch size per model."""

import importlib.util
import json
import os
import pickle

import numpy as np
import PIL.Image
import pytest
import torch

import keep_composite_ref as KC
import paste_mask_ref as PM
import tryon_fidelity_ref as F
from conftest import ROOT
from test_kept_parts_cli_gpu import Runs, _files, _integer_words, _pixels     # the helpers of the kept-parts test, not copies of them
from test_tryon_512_gpu import _snapshot as _snapshot_512
from test_tryon_outfits_gpu import _write_list
from test_tryon_pairs_gpu import _snapshot as _snapshot_256
from tryon_512_tree import make_512_tree
from tryon_pairs_tree import PAIRS as PAIRS_256, make_pair_tree

pytestmark = pytest.mark.gpu

BATCH_256 = 3
SIDE, W512 = 512, 320
# the person keeps the lower garment, the upper garment, both, neither: one batch
OUTFITS_512 = [('p0', 'c0', '-'), ('p1', '-', 'c1'), ('p2', '-', '-'), ('p0', 'c2', 'c3')]
BATCH_512 = 4
UPPER = (5, 6, 7)
LOWER = {256: (6, 9, 12), 512: (9, 12)}
# what a run pastes -> (the keywords, paste_rules' three flags: kept parts, background, kept garments)
OPTIONS = dict(background=(dict(background='photo'), (False, True, False)),
               garments=(dict(kept_garments='photo'), (False, False, True)),
               parts=(dict(kept_parts='photo'), (True, False, False)),
               everything=(dict(kept_parts='photo', background='photo', kept_garments='photo'), (True, True, True)))
PLAIN_KEYS = ['dataroot', 'network', 'noise_mode', 'pairs', 'results']
# The heads of the filled (untrained) test generators are all but constant: at 256 x 192 the upper head's pre-activation lies in
# 0.050 .. 0.167 and the lower head's in 1.139 .. 1.179 over the content of these trees, so every pixel says "upper garment"; at
# 512 x 320 logit plane 3 (0.04 .. 0.12) is the largest everywhere, so every pixel says "skin".  Neither gives a pixel that is
# pasted.  As the conditions below need both kinds of pixel, the snapshots are the existing tests' with a constant added to the
# biases of those heads (``m_bias1`` / ``m_bias2`` of the last ToRGB layer), fixed here once.  The constants are read off the
# quantiles of the pre-activations, not off the code under test:
#   256: -0.11 puts the upper head's threshold near its 90th percentile (0.114), -1.17 the lower head's at its 90th (1.170), so
#        most pixels say "other" and a tenth each says "upper" or "lower";
#   512: plane 0 ("other") is raised by its median to 0, plane 1 ("upper"), whose upper half lies within 0.0057 .. 0.0068, is
#        lowered to just under that, plane 2 by its 95th percentile, and the three skin planes by 1, out of reach.
# test_the_*_tree_has_every_kind_of_pixel asserts from the stages and the heads of a run that these constants do give the kinds.
HEAD_BIAS_SHIFT_256 = dict(m_bias1=(-0.11,), m_bias2=(-1.17,))
HEAD_BIAS_SHIFT_512 = dict(m_bias1=(0.1005, -0.0078, -0.0212, -1.0, -1.0, -1.0))


def _shifted_snapshot(make, path, resolution, shifts):
    """The snapshot ``make`` writes, with constants added to the head biases of the top block's ToRGB layer."""
    make(path)
    with open(path, 'rb') as f:
        data = pickle.load(f)
    assert data['G'] is data['G_ema']
    torgb = getattr(data['G_ema'].synthesis, 'b%d' % resolution).torgb
    with torch.no_grad():
        for name, constants in shifts.items():
            getattr(torgb, name).add_(torch.tensor(constants, dtype=torch.float32))
    with open(path, 'wb') as f:
        pickle.dump(data, f)


def _expectations(pkl, builder, raws, names_of, size):
    """Per written file: the builder's stages, the in-process run's bytes and the restated mask of every option."""
    import tryon_cli
    from training.tryon_pairs import images_to_u8, paste_rules
    G = tryon_cli.load_generator(pkl, torch.device('cuda'))
    items = {}
    for raw in raws:
        batch = builder.build(raw, keep_stages=True)
        n = batch.batch
        outs = tryon_cli.generate_outputs(G, batch.tensors, torch.empty([n, 0], device='cuda'), 1, 'const')      # z_dim is 0
        assert len(outs) == (4 if size == 256 else 3)
        heads = tuple(x.float().cpu().numpy() for x in outs[2:])
        st = {k: batch.stages[k].cpu().numpy() for k in ('image', 'parsing', 'palm', 'denorm_upper', 'denorm_lower')}
        h, w = st['parsing'].shape[1:]
        c0 = (h - w) // 2
        in_process = images_to_u8(outs[1].float(), c0, w).cpu().numpy()
        state = PM.statement(heads, c0, w, st['parsing'].shape)
        masks = {}
        for key, (_, flags) in OPTIONS.items():
            rule = paste_rules(*flags, raw['person_idx'], raw['upper_idx'], raw['lower_idx'], size)
            masks[key] = PM.paste_mask(st['parsing'], st['palm'] if flags[0] else None, np.asarray(rule), heads, c0)
        own_upper = (np.asarray(raw['upper_idx']) == np.asarray(raw['person_idx']))
        own_lower = (np.asarray(raw['lower_idx']) == np.asarray(raw['person_idx']))
        for j, name in enumerate(names_of(raw)):
            items[name] = dict({k: v[j] for k, v in st.items()}, index=int(raw['raw_idx'][j]), in_process=in_process[j], state=state[j],
                               masks={k: m[j] for k, m in masks.items()}, own_upper=bool(own_upper[j]), own_lower=bool(own_lower[j]))
    return items


# ---- the checks both models share ----

def _run(world, option, radius=2, **more):
    """The run of ``option`` at ``radius``, made once; the two runs whose reports are read are scored."""
    key = '%s%d%s' % (option, radius, ''.join('_' + str(v) for v in more.values()))
    return world['runs'].get(key, scores=(radius == 2 and option in ('everything', 'background') and not more), kept_feather=radius,
                             **OPTIONS[option][0], **more)


def _check_option(world, option, radius, crop):
    plain, _ = world['runs'].get('plain', scores=True)
    got_dir, _ = _run(world, option, radius)
    names = _files(plain)
    assert _files(got_dir) == names and sorted(world['items']) == names
    changed = 0
    for name in names:
        item = world['items'][name]
        whole_plain, whole_got = _pixels(plain / name), _pixels(got_dir / name)
        a, b = crop(whole_plain), crop(whole_got)
        assert np.array_equal(a, item['in_process']), name               # the in-process run is the run: its heads are the run's heads
        want = KC.composite(a[None], item['image'][None], item['masks'][option][None], radius)[0]
        assert np.array_equal(b, want), (name, option, radius, int((b != want).sum()))
        outside = np.ones(whole_plain.shape[:2], bool)
        crop(outside)[...] = False
        assert np.array_equal(whole_plain[outside], whole_got[outside]), name      # the other panels and the padding
        changed += int((b != a).sum())
    assert changed > 0
    return got_dir, names


def _check_kinds(world, size):
    """Asserted from the stages and the heads, not assumed: background pixels pasted with a fully kept window, background pixels
    refused because the generator claims them, own-garment pixels pasted and refused."""
    pasted_whole = refused_background = own_pasted = own_refused = 0
    for name, item in world['items'].items():
        L, s = item['parsing'], item['state']
        background = item['masks']['background']
        assert np.array_equal(background != 0, (L == 0) & (s == PM.OTHER))
        pasted_whole += int(((KC.weight(background, 2) == 25) & (L == 0)).sum())
        refused_background += int(((L == 0) & (s != PM.OTHER)).sum())
        for labels, own, state in ((UPPER, item['own_upper'], PM.UPPER), (LOWER[size], item['own_lower'], PM.LOWER)):
            mine = np.isin(L, labels) & own
            own_pasted += int((mine & (s == state)).sum())
            own_refused += int((mine & (s != state)).sum())
        garments = item['masks']['garments']
        assert garments.any() == bool((item['own_upper'] and (np.isin(L, UPPER) & (s == PM.UPPER)).any())
                                      or (item['own_lower'] and (np.isin(L, LOWER[size]) & (s == PM.LOWER)).any()))
        if not (item['own_upper'] or item['own_lower']):
            assert not garments.any()                                   # an item that changes both: a no-op
    print('%d: background pasted with a whole window %d, background refused %d, own garment pasted %d, refused %d'
          % (size, pasted_whole, refused_background, own_pasted, own_refused))
    assert pasted_whole > 0 and refused_background > 0 and own_pasted > 0 and own_refused > 0


def _check_same_files(a, b, names):
    assert _files(a) == _files(b) == names
    for name in names:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name


def _check_defaults(world, plain_keys):
    plain, report = world['runs'].get('plain', scores=True)
    same, same_report = world['runs'].get('generated', scores=True, kept_parts='generated', background='generated', kept_garments='generated')
    _check_same_files(plain, same, sorted(world['items']))
    assert json.dumps(same_report) == json.dumps(report)
    assert sorted(report) == plain_keys                                 # key for key what it was


def _check_scores(world, crop, plain_keys):
    _, plain_report = world['runs'].get('plain', scores=True)
    outdir, report = _run(world, 'everything')
    partials, items = world['runs'].partials['everything2'], world['items']
    assert sorted(report) == sorted(plain_keys + ['background', 'kept_feather', 'kept_garments', 'kept_parts'])
    assert report['background'] == report['kept_garments'] == report['kept_parts'] == 'photo' and report['kept_feather'] == 2
    _, one = _run(world, 'background')
    assert sorted(one) == sorted(plain_keys + ['background', 'kept_feather'])         # only what is 'photo' is named
    rows = np.zeros([len(items), 3, 4], np.int64)
    for name, st in items.items():
        regions = F.pair_regions(st['image'], st['parsing'], st['palm'], st['denorm_upper'], st['denorm_lower'])
        written = np.ascontiguousarray(crop(_pixels(outdir / name)))
        for k, region in enumerate(F.REGIONS):
            mask, ref = regions[region]
            rows[st['index'], k] = _integer_words(written, ref, mask)
    assert tuple(partials.shape) == (len(items), 3, 5)
    assert np.array_equal(partials[:, :, :4].numpy(), rows)             # sum |d|, sum d^2, windows, bytes of the three regions
    for k in ('tryon_keep_share', 'tryon_keep_pairs', 'tryon_upper_share', 'tryon_lower_share'):
        assert report['results'][k] == plain_report['results'][k], k    # the three scored regions are the same


def _describe(world, size, crop):
    """Figures of an untrained generator, printed and not asserted beyond their direction: the L1 between the written bytes and
    the photograph over the label-0 pixels and over the pixels of the garments the person keeps."""
    dirs = dict(plain=world['runs'].get('plain', scores=True)[0],
                pasted=_run(world, 'everything')[0])
    figures = {}
    for key, outdir in dirs.items():
        sums = np.zeros([2, 2])
        for name, item in world['items'].items():
            d = np.abs(crop(_pixels(outdir / name)).astype(np.int64) - item['image'].astype(np.int64)).sum(axis=2)
            L = item['parsing']
            own = (np.isin(L, UPPER) & item['own_upper']) | (np.isin(L, LOWER[size]) & item['own_lower'])
            for k, region in enumerate((L == 0, own)):
                sums[k] += (d[region].sum(), 3 * region.sum())
        figures[key] = sums[:, 0] / sums[:, 1] / 255.0
    print('%d: L1 to the photograph, label 0: plain %.6f pasted %.6f; own garments: plain %.6f pasted %.6f'
          % (size, figures['plain'][0], figures['pasted'][0], figures['plain'][1], figures['pasted'][1]))
    assert (figures['pasted'] < figures['plain']).all()


def _command(name):
    spec = importlib.util.spec_from_file_location('pasta_background_test_cli_' + name[:-3], os.path.join(ROOT, 'pasta-gan_amd', name))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.generate_images


PHOTO_FLAGS = ['--kept-parts', 'photo', '--background', 'photo', '--kept-garments', 'photo', '--kept-feather', '2']


# ---- 256 x 192, --change-region lowerbody: everyone keeps their upper garment ----

@pytest.fixture(scope='module')
def world_256(tmp_path_factory):
    import tryon_cli
    from training.dataset import UvitonDatasetV19_test, collate_region_outfits
    from training.tryon_pairs import TryOnPairOutfitBatchBuilder
    root = tmp_path_factory.mktemp('background256')
    tree, pkl = make_pair_tree(root / 'tree'), str(root / 'snapshot.pkl')
    _shifted_snapshot(_snapshot_256, pkl, 256, HEAD_BIAS_SHIFT_256)
    runs = Runs(root, lambda outdir, scores, **kw: tryon_cli.generate_256(pkl, 1, 'const', outdir, tree, BATCH_256, 0, change_region='lowerbody',
                                                                         scores_file=scores, **kw))
    ds = UvitonDatasetV19_test(path=tree)
    raws = [collate_region_outfits('lowerbody', [ds[i] for i in range(lo, min(lo + BATCH_256, len(ds)))]) for lo in range(0, len(ds), BATCH_256)]
    stem = lambda p: os.path.basename(p)[:-4]
    names_of = lambda raw: [os.path.join(p.split('/')[0], stem(p) + '__' + stem(c) + '.png') for p, c in zip(raw['person_name'], raw['clothes_name'])]
    items = _expectations(pkl, TryOnPairOutfitBatchBuilder('cuda'), raws, names_of, 256)
    assert len(items) == len(PAIRS_256) and all(i['own_upper'] and not i['own_lower'] for i in items.values())
    return dict(tree=tree, pkl=pkl, runs=runs, items=items)


KEYS_256 = sorted(PLAIN_KEYS + ['mode'])


def test_the_256_tree_has_every_kind_of_pixel(world_256):
    _check_kinds(world_256, 256)


@pytest.mark.parametrize('radius', [2, 0])
@pytest.mark.parametrize('option', list(OPTIONS))
def test_generate_256_pastes_under_the_restated_mask(world_256, option, radius):
    got, names = _check_option(world_256, option, radius, crop=lambda a: a)
    assert PIL.Image.open(got / names[0]).size == (192, 256)


def test_generate_256_defaults_write_what_they_wrote(world_256):
    _check_defaults(world_256, KEYS_256)


def test_generate_256_scores_the_written_bytes(world_256):
    _check_scores(world_256, lambda a: a, KEYS_256)
    _describe(world_256, 256, lambda a: a)


def test_the_256_command_line_and_the_gpu_encoder(world_256, tmp_path):
    from click.testing import CliRunner
    keyword, _ = _run(world_256, 'everything')
    names = sorted(world_256['items'])
    result = CliRunner().invoke(_command('test.py'), ['--network', world_256['pkl'], '--outdir', str(tmp_path / 'cli'), '--dataroot', world_256['tree'],
                                                      '--batchsize', str(BATCH_256), '--workers', '0', '--change-region', 'lowerbody'] + PHOTO_FLAGS)
    assert result.exit_code == 0, (result.output[-2000:], result.exception)
    _check_same_files(tmp_path / 'cli', keyword, names)
    gpu, _ = _run(world_256, 'everything', png_encoder='gpu')
    assert _files(gpu) == names
    for name in names:
        assert np.array_equal(_pixels(gpu / name), _pixels(keyword / name)), name
        assert (gpu / name).read_bytes() != (keyword / name).read_bytes()


# ---- 512 x 320, an outfit list with a ``-`` in each position ----

C0_512 = 3 * SIDE + (SIDE - W512) // 2                                  # upper donor | lower donor | person | generated
_crop_512 = lambda a: a[:, C0_512:C0_512 + W512]


@pytest.fixture(scope='module')
def world_512(tmp_path_factory):
    import tryon_cli
    from training.dataset import UvitonOutfits_512_test, collate_outfits
    from training.tryon_regions import TryOnOutfitBatchBuilder
    root = tmp_path_factory.mktemp('background512')
    tree, pkl = make_512_tree(root / 'tree'), str(root / 'snapshot.pkl')
    _shifted_snapshot(_snapshot_512, pkl, 512, HEAD_BIAS_SHIFT_512)
    listing = _write_list(root / 'outfits.txt', OUTFITS_512)
    runs = Runs(root, lambda outdir, scores, **kw: tryon_cli.generate_512(pkl, 1, 'const', outdir, tree, BATCH_512, None, 0, outfits_file=listing,
                                                                         scores_file=scores, **kw))
    ds = UvitonOutfits_512_test(path=tree, outfits_file=listing)
    raws = [collate_outfits([ds[i] for i in range(lo, min(lo + BATCH_512, len(ds)))]) for lo in range(0, len(ds), BATCH_512)]
    items = _expectations(pkl, TryOnOutfitBatchBuilder('cuda'), raws, lambda raw: ['%03d.png' % i for i in raw['raw_idx'].tolist()], 512)
    assert [(i['own_upper'], i['own_lower']) for _, i in sorted(items.items())] == [(False, True), (True, False), (True, True), (False, False)]
    return dict(tree=tree, pkl=pkl, listing=listing, runs=runs, items=items)


KEYS_512 = sorted(PLAIN_KEYS)                                           # generate_512 names no mode


def test_the_512_tree_has_every_kind_of_pixel(world_512):
    _check_kinds(world_512, 512)


@pytest.mark.parametrize('radius', [2, 0])
@pytest.mark.parametrize('option', list(OPTIONS))
def test_generate_512_pastes_into_the_generated_panel_only(world_512, option, radius):
    got, names = _check_option(world_512, option, radius, crop=_crop_512)
    assert _pixels(got / names[0]).shape == (SIDE, 4 * SIDE, 3)


def test_generate_512_defaults_write_what_they_wrote(world_512):
    _check_defaults(world_512, KEYS_512)


def test_generate_512_scores_the_written_bytes(world_512):
    _check_scores(world_512, _crop_512, KEYS_512)
    _describe(world_512, 512, _crop_512)


def test_the_512_command_line_and_the_gpu_encoder(world_512, tmp_path):
    from click.testing import CliRunner
    keyword, _ = _run(world_512, 'everything')
    names = sorted(world_512['items'])
    result = CliRunner().invoke(_command('test_512.py'), ['--network', world_512['pkl'], '--outdir', str(tmp_path / 'cli'), '--dataroot', world_512['tree'],
                                                          '--batchsize', str(BATCH_512), '--workers', '0', '--outfits', world_512['listing']] + PHOTO_FLAGS)
    assert result.exit_code == 0, (result.output[-2000:], result.exception)
    _check_same_files(tmp_path / 'cli', keyword, names)
    gpu, _ = _run(world_512, 'everything', png_encoder='gpu')
    assert _files(gpu) == names
    for name in names:
        assert np.array_equal(_pixels(gpu / name), _pixels(keyword / name)), name
        assert (gpu / name).read_bytes() != (keyword / name).read_bytes()
