"""The paste region of --background / --kept-garments / --kept-parts photo without a GPU: the rule table the host
fills (training.tryon_pairs.paste_rules), the numpy restatement (tests/paste_mask_ref.py) against the kept region the scores
use, and the options' refusals on both command lines."""

import importlib.util
import os

import numpy as np
import pytest

import paste_mask_ref as PM
import tryon_fidelity_ref as F
from conftest import ROOT

KEEP = (1, 2, 4, 13, 18, 19)
UPPER = (5, 6, 7)
LOWER = {256: (6, 9, 12), 512: (9, 12)}
# (person, upper, lower) as positions in the people stack: both kept, upper changed, lower changed, both changed
PERSON, UPPER_IDX, LOWER_IDX = [0, 0, 1, 3], [0, 2, 1, 4], [0, 0, 3, 4]


def _rules(size, kept_parts=False, background=False, kept_garments=False):
    from training.tryon_pairs import paste_rules
    rule = paste_rules(kept_parts, background, kept_garments, PERSON, UPPER_IDX, LOWER_IDX, size)
    rule = rule.numpy() if hasattr(rule, 'numpy') else np.asarray(rule)
    assert rule.dtype == np.uint8 and rule.shape == (4, 256)
    return rule


def _expected(size, kept_parts, background, kept_garments):
    want = np.zeros([4, 256], np.uint8)
    if kept_parts:
        want[:, list(KEEP)] |= 0b1111
    if background:
        want[:, 0] |= 0b0001
    if kept_garments:
        want[np.ix_([0, 2], list(UPPER))] |= 0b0010            # items 0 and 2 wear their own upper garment
        want[np.ix_([0, 1], list(LOWER[size]))] |= 0b0100      # items 0 and 1 their own lower garment
    return want


@pytest.mark.parametrize('size', [256, 512])
def test_paste_rules_give_the_stated_bits(size):
    from metrics.tryon_fidelity import KEEP_LABELS
    assert tuple(KEEP_LABELS) == KEEP
    for flags in ((True, False, False), (False, True, False), (False, False, True), (True, True, True), (False, False, False)):
        assert np.array_equal(_rules(size, *flags), _expected(size, *flags)), (size, flags)
    garments = _rules(size, kept_garments=True)
    assert not garments[3].any()                                # an item that changes both: a no-op
    assert (garments[:, 20:] == 0).all() and (_rules(size, True, True, True)[:, 20:] == 0).all()


def test_label_six_belongs_to_both_garments_at_256():
    from training.tryon_pairs import paste_rules
    six = lambda upper, lower: int(np.asarray(paste_rules(False, False, True, [0], [upper], [lower], 256))[0, 6])
    assert six(0, 0) == 0b0110                                  # (P, -, -)
    assert six(1, 0) == 0b0100                                  # (P, D, -)
    assert six(0, 1) == 0b0010                                  # (P, -, D)
    assert six(1, 1) == 0
    at_512 = lambda upper, lower: int(np.asarray(paste_rules(False, False, True, [0], [upper], [lower], 512))[0, 6])
    assert at_512(0, 0) == 0b0010 and at_512(1, 0) == 0 and at_512(0, 1) == 0b0010      # the upper garment's alone at 512 x 320


def test_the_label_sets_are_the_builders():
    """paste_rules takes the sets from next to the builders: what each size passes the masks entry as six_is_lower."""
    from training import tryon_pairs, tryon_regions
    assert tryon_pairs.garment_labels(256) == (UPPER, (9, 12, 6)) and tryon_pairs.SIX_IS_LOWER == 1
    assert tryon_pairs.garment_labels(512) == (UPPER, (9, 12)) and tryon_regions.SIX_IS_LOWER == 0
    with pytest.raises(ValueError):
        tryon_pairs.garment_labels(384)


def test_kept_parts_rules_without_heads_are_the_keep_mask():
    rng = np.random.RandomState(3)
    n, h, w = 3, 40, 24
    c0 = (h - w) // 2
    parsing = rng.randint(0, 20, size=[n, h, w]).astype(np.uint8)
    parsing[0, 0, :3] = (200, 255, 20)
    palm = (rng.rand(n, h, h) < 0.1).astype(np.uint8) * rng.choice(np.uint8([1, 255]), size=[n, h, h])
    got = PM.paste_mask(parsing, palm, _rules(256, kept_parts=True)[:n], (), c0)
    want = np.stack([F.keep_mask(palm[i], parsing[i]) for i in range(n)]).astype(np.uint8)
    assert got.dtype == np.uint8 and np.array_equal(got, want) and 0 < got.sum() < got.size
    # the heads change nothing under 0b1111, and without the palm pointer the palm term is gone
    heads = (rng.uniform(-3, 3, size=[n, 6, h, h]).astype(np.float32),)
    assert np.array_equal(PM.paste_mask(parsing, palm, _rules(256, kept_parts=True)[:n], heads, c0), want)
    assert np.array_equal(PM.paste_mask(parsing, None, _rules(256, kept_parts=True)[:n], (), c0), np.isin(parsing, KEEP).astype(np.uint8))


def test_the_restated_statement():
    nan = np.float32(np.nan)
    planes = np.zeros([1, 6, 1, 8], np.float32)
    #                  tie 0/1  largest 4  NaN first  NaN later  all NaN   tie 2/5   -0 / +0   class 3
    planes[0, :, 0] = [[1, 0, nan, 0, nan, -1, -0.0, 0],
                       [1, 0, 5, 0, nan, -1, 0.0, 0],
                       [0, 1, 9, nan, nan, 2, 0, 0],
                       [0, 0, 0, 9, nan, 0, 0, 3],
                       [0, 3, 0, nan, nan, 0, 0, 0],
                       [0, 3, 0, 0, nan, 2, 0, 0]]
    assert PM.argmax_planes(planes)[0, 0].tolist() == [0, 4, 0, 2, 0, 2, 0, 3]
    assert PM.statement((planes,), 0, 8, (1, 1, 8))[0, 0].tolist() == [0, 3, 0, 2, 0, 2, 0, 3]
    u = np.float32([[[[0.5, 0.50001, 0.9, nan, 0.1, nan, 0.2, 0.5]]]])
    l = np.float32([[[[0.9, 0.9, 0.9, 0.9, 0.5, nan, 0.50001, nan]]]])
    assert PM.statement((u, l), 0, 8, (1, 1, 8))[0, 0].tolist() == [2, 1, 1, 2, 0, 0, 2, 0]
    assert not PM.statement((), 0, 8, (1, 1, 8)).any()


# ---- the options ----

def _command(name):
    spec = importlib.util.spec_from_file_location('pasta_paste_cli_' + name[:-3], os.path.join(ROOT, 'pasta-gan_amd', name))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.generate_images


@pytest.mark.parametrize('name', ['test.py', 'test_512.py'])
def test_both_commands_declare_and_refuse(name, tmp_path):
    import click
    from click.testing import CliRunner
    command = _command(name)
    for keyword, flag in (('background', '--background'), ('kept_garments', '--kept-garments')):
        option, = [p for p in command.params if p.name == keyword]
        assert option.opts == [flag] and isinstance(option.type, click.Choice) and list(option.type.choices) == ['generated', 'photo']
        assert option.default == 'generated' and not option.required
    common = ['--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path)]
    for extra, words in ((['--kept-feather', '3'], ('--kept-feather', '--background photo', '--kept-garments photo')),
                         (['--background', 'generated', '--kept-garments', 'generated', '--kept-feather', '0'], ('--kept-feather', '--background photo')),
                         (['--background', 'studio'], ("'studio' is not one of", '--background')),
                         (['--kept-garments', 'both'], ("'both' is not one of", '--kept-garments')),
                         (['--background', 'photo', '--kept-feather', '9'], ('--kept-feather', '9'))):
        result = CliRunner().invoke(command, common + extra)
        assert result.exit_code == 2, (extra, result.output)
        assert all(w in result.output for w in words) and 'none.pkl' not in result.output, (extra, result.output)
        assert not (tmp_path / 'out').exists(), extra


@pytest.mark.parametrize('name', ['test.py', 'test_512.py'])
def test_the_values_reach_the_loop(name, tmp_path, monkeypatch):
    """``dress`` is replaced by a recorder, so nothing is loaded or launched."""
    import click
    import tryon_cli
    from click.testing import CliRunner
    seen = []
    monkeypatch.setattr(tryon_cli, 'dress', lambda *args, **kwargs: seen.append((kwargs.get('kept_radius'), tuple(kwargs.get('pasted', ())))))
    common = ['--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path)]
    for extra, want in (([], (None, ())),
                        (['--background', 'photo'], (2, ('background',))),
                        (['--kept-garments', 'photo', '--kept-feather', '0'], (0, ('kept_garments',))),
                        (['--kept-feather', '8', '--background', 'photo', '--kept-parts', 'photo', '--kept-garments', 'photo'],
                         (8, ('kept_parts', 'background', 'kept_garments'))),
                        (['--kept-parts', 'photo'], (2, ('kept_parts',)))):
        result = CliRunner().invoke(_command(name), common + extra)
        assert result.exit_code == 0, result.output
        assert seen.pop() == want and not seen
    generate = tryon_cli.generate_256 if name == 'test.py' else tryon_cli.generate_512
    first = ('none.pkl', 1, 'const', 'out', 'root', 2) + ((0,) if name == 'test.py' else (None, 0))
    generate(*first)
    generate(*first, background='photo')
    generate(*first, kept_garments='photo', kept_feather=1)
    generate(*first, kept_parts='photo', background='photo', kept_garments='photo', kept_feather=0)
    assert seen == [(None, ()), (2, ('background',)), (1, ('kept_garments',)), (0, ('kept_parts', 'background', 'kept_garments'))]
    with pytest.raises(click.UsageError, match='--background photo'):
        generate(*first, kept_feather=1)
    for bad in (dict(background='studio'), dict(kept_garments='both'), dict(background='photo', kept_feather=9)):
        with pytest.raises(click.BadParameter):
            generate(*first, **bad)
    assert len(seen) == 4


def test_generate_is_the_second_of_generate_outputs(monkeypatch):
    import tryon_cli
    monkeypatch.setattr(tryon_cli, 'generate_outputs', lambda *args: ('img', 'fine', 'head_a', 'head_b'))
    assert tryon_cli.generate(None, None, None, 1, 'const') == 'fine'


def test_photo_paste_mask_refuses_cpu_tensors():
    import torch
    from training.tryon_pairs import photo_paste_mask
    parsing, rule = torch.zeros([1, 4, 4], dtype=torch.uint8), torch.zeros([1, 256], dtype=torch.uint8)
    with pytest.raises(ValueError, match='not a tensor on the GPU'):
        photo_paste_mask(parsing, None, rule, (), 0)
