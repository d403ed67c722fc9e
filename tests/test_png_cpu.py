"""The parts of the PNG encoder that need no GPU: the host-only code-length entry (complete, length-limited codes), the numpy
restatement of the stream (tests/png_ref.py) judged by zlib and PIL, the host-only table entry against the restatement, and the
--png-encoder option of the two try-on command lines."""

import heapq
import importlib.util
import inspect
import io
import os
import zlib

import numpy as np
import PIL.Image
import pytest

import png_ref as R
from conftest import ROOT


def _fibonacci(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def _huffman_total(counts):
    """Total bits of the unlimited Huffman code: the sum of the merged weights."""
    heap = [int(c) for c in counts if c > 0]
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        merged = heapq.heappop(heap) + heapq.heappop(heap)
        total += merged
        heapq.heappush(heap, merged)
    return total


# counts, by limit: the Fibonacci-like ones are as long as still fit the limit's 2^limit leaves with a Huffman depth above it
# (depth n - 1 for n Fibonacci counts: 39 > 15 and 18 > 7)
CASES = {
    'flat': lambda limit: [5] * 64,
    'two symbols': lambda limit: [0, 3, 0, 9],
    'zero counts': lambda limit: [0, 7, 0, 0, 2, 1, 0, 30, 0],
    'fibonacci': lambda limit: _fibonacci(40 if limit == 15 else 19),
}
# the limited code's total over the unlimited Huffman total, measured on the Fibonacci counts: 1.0055 at 15 bits over 40
# counts, 1.1253 at 7 bits over 19 counts (the code-length alphabet, where it is at most a few bytes of a header); none elsewhere
SLACK = {('fibonacci', 15): 1.006, ('fibonacci', 7): 1.126}


@pytest.mark.parametrize('limit', [15, 7])
@pytest.mark.parametrize('case', list(CASES))
def test_code_lengths_are_limited_and_complete(case, limit):
    from torch_utils.ops import png_encode
    counts = np.array(CASES[case](limit), np.uint32)
    lengths = png_encode.code_lengths(counts, limit).astype(np.int64)
    assert lengths.max() <= limit
    assert np.array_equal(lengths == 0, counts == 0)
    assert sum(2 ** (limit - int(l)) for l in lengths if l) == 2 ** limit          # Kraft sum exactly 1, in units of 2^-limit
    total, unlimited = int((lengths * counts).sum()), _huffman_total(counts)
    print('%s at %d bits: %d bits, unlimited Huffman %d (%.4f)' % (case, limit, total, unlimited, total / unlimited))
    assert unlimited <= total <= unlimited * SLACK.get((case, limit), 1.0)
    if case == 'fibonacci':
        assert lengths.max() == limit and total > unlimited                         # the limit did bind


def test_code_lengths_stay_complete_on_many_histograms():
    """Skewed, sparse and power-of-two counts over both alphabets: the repair ends on a complete code every time."""
    from torch_utils.ops import png_encode
    rng = np.random.RandomState(0)
    fib = np.array(_fibonacci(40), np.int64)
    for it in range(600):
        n, limit = (rng.randint(2, 287), 15) if it % 2 else (rng.randint(2, 20), 7)
        counts = [rng.randint(0, 100, n), (rng.exponential(1, n) ** 8 * 10).astype(np.int64), fib[np.minimum(np.arange(n), 39)] * rng.randint(0, 2, n),
                  2 ** rng.randint(0, 31, n).astype(np.int64) * rng.randint(0, 2, n)][it // 2 % 4]
        counts = np.minimum(counts, 2 ** 32 - 1).astype(np.uint32)
        if (counts > 0).sum() < 2:
            continue
        lengths = png_encode.code_lengths(counts, limit).astype(np.int64)
        assert lengths.max() <= limit and np.array_equal(lengths == 0, counts == 0), (it, counts)
        assert sum(2 ** (limit - int(l)) for l in lengths if l) == 2 ** limit, (it, counts, lengths)


def test_code_lengths_refusals_and_the_lone_symbol():
    from torch_utils.ops import png_encode
    assert png_encode.code_lengths([0, 0, 6], 15).tolist() == [0, 0, 1]
    with pytest.raises(RuntimeError, match='every one of the 3 counts is zero'):
        png_encode.code_lengths([0, 0, 0], 15)
    with pytest.raises(RuntimeError, match='9 symbols do not fit codes of at most 3 bits'):
        png_encode.code_lengths([1] * 9, 3)
    with pytest.raises(RuntimeError, match='limit of 16 bits'):
        png_encode.code_lengths([1, 1], 16)


def _images():
    rng = np.random.RandomState(11)
    halves = rng.randint(0, 256, (40, 60, 3)).astype(np.uint8)
    halves[:, :30] = 255
    return {'1x1': np.full((1, 1, 3), 200, np.uint8), '5x7 zeros': np.zeros((5, 7, 3), np.uint8),
            '37x53 noise': rng.randint(0, 256, (37, 53, 3)).astype(np.uint8), '53x37 noise': rng.randint(0, 256, (53, 37, 3)).astype(np.uint8),
            '40x60 halves': halves, '128x384 panel': R.panel(128, 384, 80, 1)}


@pytest.fixture(scope='module')
def restated():
    from torch_utils.ops import png_encode
    return {name: (img, R.encode(img, png_encode.code_lengths)) for name, img in _images().items()}


@pytest.mark.parametrize('name', list(_images()))
def test_the_restatement_writes_png(name, restated):
    img, e = restated[name]
    kinds = R.chunks(e['file'])
    assert [k for k, _, _ in kinds] == [b'IHDR', b'IDAT', b'IEND'] and kinds[1][1] == e['idat']
    for kind, body, crc in kinds:
        assert zlib.crc32(kind + body) == crc, kind
    assert zlib.decompress(e['idat']) == e['filtered'].tobytes()                    # inflate checks the Adler-32 as well
    PIL.Image.open(io.BytesIO(e['file'])).verify()
    back = PIL.Image.open(io.BytesIO(e['file']))
    assert back.mode == 'RGB' and back.size == (img.shape[1], img.shape[0]) and np.array_equal(np.asarray(back), img)
    assert e['sizes'].sum() + 6 == len(e['idat'])


def test_the_restated_cases_hold_what_they_are_for(restated):
    assert restated['5x7 zeros'][1]['meta'][0, :256].nonzero()[0].tolist() == [0, 4]       # literals of one value, and the filter byte
    assert restated['5x7 zeros'][1]['meta'][0, R.MATCH] == 0
    assert (restated['40x60 halves'][1]['meta'][:, R.MATCH] > 0).all() and (restated['128x384 panel'][1]['meta'][:, R.MATCH] > 0).all()
    # ragged last segments of five rows; rows of 160 bytes fill their tiles, rows of 112 leave the last tile of 5 x 112 bytes half full
    assert restated['37x53 noise'][1]['meta'].shape[0] == 3 and restated['53x37 noise'][1]['meta'].shape[0] == 4 and (5 * 112) % 32 == 16


@pytest.mark.parametrize('name', list(_images()))
def test_segment_tables_equal_the_restatement(name, restated):
    """The host-only table entry: the tables and the sizes known before encoding are the restatement's."""
    from torch_utils.ops import png_encode
    e = restated[name][1]
    tables, sizes = png_encode.segment_tables(e['meta'])
    assert np.array_equal(tables, e['tables']) and np.array_equal(sizes, e['sizes'])


def test_encode_refuses_a_cpu_tensor():
    import torch
    from torch_utils.ops import png_encode
    with pytest.raises(RuntimeError, match='tensor is on cpu'):
        png_encode.encode(torch.zeros([1, 4, 4, 3], dtype=torch.uint8))


# ---- the option ----

def _command(name):
    spec = importlib.util.spec_from_file_location('pasta_png_cli_' + name[:-3], os.path.join(ROOT, 'pasta-gan_amd', name))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module.generate_images


@pytest.mark.parametrize('name', ['test.py', 'test_512.py'])
def test_both_commands_declare_the_option(name, tmp_path):
    import click
    from click.testing import CliRunner
    command = _command(name)
    option, = [p for p in command.params if p.name == 'png_encoder']
    assert option.opts == ['--png-encoder'] and isinstance(option.type, click.Choice) and list(option.type.choices) == ['pil', 'gpu']
    assert option.default == 'pil' and not option.required
    result = CliRunner().invoke(command, ['--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path),
                                          '--png-encoder', 'cpu'])
    assert result.exit_code == 2 and "'cpu' is not one of" in result.output and not (tmp_path / 'out').exists()


@pytest.mark.parametrize('name', ['test.py', 'test_512.py'])
def test_the_command_lines_value_reaches_the_loop(name, tmp_path, monkeypatch):
    """The option hands the callbacks no argument: generate_256 / generate_512 find its value in the click context.  ``dress`` is
    replaced by a recorder, so nothing is loaded or launched."""
    import tryon_cli
    from click.testing import CliRunner
    seen = []
    monkeypatch.setattr(tryon_cli, 'dress', lambda *args, **kwargs: seen.append(kwargs.get('png_encoder', args[-1])))
    common = ['--network', str(tmp_path / 'none.pkl'), '--outdir', str(tmp_path / 'out'), '--dataroot', str(tmp_path)]
    for extra, want in (([], 'pil'), (['--png-encoder', 'pil'], 'pil'), (['--png-encoder', 'gpu'], 'gpu')):
        result = CliRunner().invoke(_command(name), common + extra)
        assert result.exit_code == 0, result.output
        assert seen.pop() == want and not seen
    # without a command line there is only the keyword
    generate = tryon_cli.generate_256 if name == 'test.py' else tryon_cli.generate_512
    first = ('none.pkl', 1, 'const', 'out', 'root', 2) + ((0,) if name == 'test.py' else (None, 0))
    generate(*first)
    generate(*first, png_encoder='gpu')
    assert seen == ['pil', 'gpu']


def test_the_generate_functions_take_the_encoder_last():
    import tryon_cli
    for fn in (tryon_cli.generate_256, tryon_cli.generate_512, tryon_cli.dress):
        names = list(inspect.signature(fn).parameters)
        assert names[-1] == 'png_encoder' and inspect.signature(fn).parameters['png_encoder'].default == 'pil', fn
    with pytest.raises(click_bad_parameter(), match='is not one of pil, gpu'):
        tryon_cli.dress(None, __file__, 1, 'const', 'unused', 'unused', 1, 0, None, None, png_encoder='cpu')


def click_bad_parameter():
    import click
    return click.BadParameter
