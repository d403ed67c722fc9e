"""--png-encoder gpu of the two try-on commands: the same names, the same pixels and the same --scores report as the default,
on the tiny trees and snapshots of the existing end-to-end tests."""

import json
import os

import numpy as np
import PIL.Image
import pytest

from test_tryon_512_gpu import _snapshot as _snapshot_512       # the snapshots of the existing end-to-end tests, not copies of them
from test_tryon_pairs_gpu import _snapshot as _snapshot_256
from tryon_512_tree import PAIRS as PAIRS_512, make_512_tree
from tryon_pairs_tree import PAIRS as PAIRS_256, make_pair_tree

pytestmark = pytest.mark.gpu


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _same_pictures(tmp_path, generate, pairs):
    """``generate(outdir, scores_file, png_encoder)`` once per encoder: what the two runs wrote."""
    reports = {}
    for encoder in ('pil', 'gpu'):
        generate(str(tmp_path / encoder), str(tmp_path / (encoder + '.json')), encoder)
        reports[encoder] = json.loads((tmp_path / (encoder + '.json')).read_text())
    names = _files(tmp_path / 'pil')
    assert len(names) == pairs and _files(tmp_path / 'gpu') == names
    larger = 0
    for name in names:
        PIL.Image.open(tmp_path / 'gpu' / name).verify()
        mine, twin = PIL.Image.open(tmp_path / 'gpu' / name), PIL.Image.open(tmp_path / 'pil' / name)
        assert mine.mode == twin.mode == 'RGB' and np.array_equal(np.asarray(mine), np.asarray(twin)), name
        larger += (tmp_path / 'gpu' / name).read_bytes() != (tmp_path / 'pil' / name).read_bytes()
    assert larger == len(names)                                     # the option did choose another writer
    assert reports['gpu'] == reports['pil'] and reports['pil']['pairs'] == pairs
    return names


def test_generate_512_writes_the_same_panels(tmp_path):
    import tryon_cli
    tree, pkl = make_512_tree(tmp_path / 'tree'), str(tmp_path / 'snapshot.pkl')
    _snapshot_512(pkl)
    names = _same_pictures(tmp_path, lambda outdir, scores, encoder: tryon_cli.generate_512(
        pkl, 1, 'const', outdir, tree, 3, None, 0, scores_file=scores, png_encoder=encoder), len(PAIRS_512))
    assert names == ['%03d.png' % i for i in range(len(PAIRS_512))]
    assert PIL.Image.open(tmp_path / 'gpu' / names[0]).size == (1536, 512)

    # the command line itself: its option reaches the loop through the click context and writes the files of the keyword
    import importlib.util
    from click.testing import CliRunner
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('pasta_png_test_512_cli', os.path.join(ROOT, 'pasta-gan_amd', 'test_512.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    result = CliRunner().invoke(module.generate_images, ['--network', pkl, '--outdir', str(tmp_path / 'cli'), '--dataroot', tree, '--batchsize', '3',
                                                         '--workers', '0', '--png-encoder', 'gpu'])
    assert result.exit_code == 0, (result.output[-2000:], result.exception)
    assert _files(tmp_path / 'cli') == names
    for name in names:
        assert (tmp_path / 'cli' / name).read_bytes() == (tmp_path / 'gpu' / name).read_bytes(), name


def test_generate_256_writes_the_same_images(tmp_path):
    import tryon_cli
    tree, pkl = make_pair_tree(tmp_path / 'tree'), str(tmp_path / 'snapshot.pkl')
    _snapshot_256(pkl)
    names = _same_pictures(tmp_path, lambda outdir, scores, encoder: tryon_cli.generate_256(
        pkl, 1, 'const', outdir, tree, 3, 0, scores_file=scores, png_encoder=encoder), len(PAIRS_256))
    assert set(names) == {os.path.join(ds, p[:-4] + '__' + c[:-4] + '.png') for ds, p, c in PAIRS_256}
    assert PIL.Image.open(tmp_path / 'gpu' / names[0]).size == (192, 256)
