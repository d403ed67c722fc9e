"""The PNG encoder on the GPU (csrc/png_encode.hip, torch_utils/ops/png_encode.py) against its numpy restatement
(tests/png_ref.py), byte for byte; every file against zlib and PIL; determinism; the size conditions; the refusals."""

import io
import zlib

import numpy as np
import PIL.Image
import pytest
import torch

import png_ref as R

pytestmark = pytest.mark.gpu


def _noise(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _halves(h, w, seed):
    img = _noise(h, w, seed)
    img[:, :w // 2] = 255
    return img


def _batches():
    """name -> [N, H, W, 3] uint8.  Rows per segment 16, tile 32: the shapes name which edge they sit on."""
    three = np.stack([R.photograph(40, 24, 7), _halves(40, 24, 8), np.zeros((40, 24, 3), np.uint8)])
    return {
        '1x1': np.full((1, 1, 1, 3), 200, np.uint8),
        '5x7 zeros': np.zeros((1, 5, 7, 3), np.uint8),                  # the stream's first tile; literals of one value
        '37x53 noise': _noise(37, 53, 1)[None],                         # ragged last segment of whole tiles (rows of 160 bytes)
        '53x37 noise': _noise(53, 37, 9)[None],                         # ragged last segment, ragged last tile (rows of 112 bytes)
        '40x60 halves': _halves(40, 60, 2)[None],                       # matches next to literals
        '128x384 panel': R.panel(128, 384, 80, 1)[None],                # white padding between content
        'three of 40x24': three,                                        # a batch in one call
        '33x11 noise': _noise(33, 11, 3)[None],                         # a row of 34 bytes: rows and tiles drift apart by two
        '33x9 halves': _halves(33, 9, 4)[None],                         # a row of 28 bytes, shorter than a tile
        '17x20 white': np.full((1, 17, 20, 3), 255, np.uint8),          # H = R + 1: a one-row last segment
        '17x683 halves': _halves(17, 683, 5)[None],                     # a row of 2050 bytes, no multiple of 32
        '20x2800 halves': _halves(20, 2800, 6)[None],                   # 134 416 bytes in a segment: seventeen rounds of 256 tiles
    }


@pytest.fixture(scope='module')
def batches():
    return _batches()


@pytest.fixture(scope='module')
def restated(batches):
    from torch_utils.ops import png_encode
    return {name: [R.encode(img, png_encode.code_lengths) for img in batch] for name, batch in batches.items()}


@pytest.fixture(scope='module')
def encoded(batches):
    from torch_utils.ops import png_encode
    out = {}
    for name, batch in batches.items():
        images = torch.from_numpy(batch).cuda()
        filtered, meta = png_encode.filter_pass(images)
        out[name] = (filtered.cpu().numpy(), meta.cpu().numpy().view(np.uint32), png_encode.encode(images))
    return out


@pytest.mark.parametrize('name', list(_batches()))
def test_device_equals_the_restatement(name, batches, restated, encoded):
    filtered, meta, files = encoded[name]
    assert len(files) == len(batches[name])
    for i, want in enumerate(restated[name]):
        assert np.array_equal(filtered[i], want['filtered']), (name, i, 'filtered stream')
        assert np.array_equal(meta[i, :, :R.SYMS], want['meta'][:, :R.SYMS]), (name, i, 'token counts')
        assert np.array_equal(meta[i, :, R.SYMS:], want['meta'][:, R.SYMS:]), (name, i, 'Adler parts')
        assert files[i] == want['file'], (name, i, len(files[i]), len(want['file']))


@pytest.mark.parametrize('name', list(_batches()))
def test_files_decode_to_the_input(name, batches, encoded):
    for img, data in zip(batches[name], encoded[name][2]):
        kinds = R.chunks(data)
        assert [k for k, _, _ in kinds] == [b'IHDR', b'IDAT', b'IEND']
        for kind, body, crc in kinds:
            assert zlib.crc32(kind + body) == crc, (name, kind)
        assert zlib.decompress(kinds[1][1]) == R.filtered(img).tobytes(), name        # inflate checks the Adler-32 as well
        PIL.Image.open(io.BytesIO(data)).verify()
        back = PIL.Image.open(io.BytesIO(data))
        assert back.mode == 'RGB' and np.array_equal(np.asarray(back), img), name


def test_the_cases_reach_both_kinds_of_token(restated):
    """The restatement's counts say what the cases above exercise: segments with matches and segments without."""
    for name in ('1x1', '5x7 zeros', '37x53 noise', '33x9 halves'):         # rows of 22 and 28 bytes: every tile holds a filter byte
        assert restated[name][0]['meta'][:, R.MATCH].sum() == 0, name
    for name in ('40x60 halves', '128x384 panel', '17x683 halves', '20x2800 halves', '17x20 white'):
        assert restated[name][0]['meta'][0, R.MATCH] > 0, name
    assert restated['three of 40x24'][2]['meta'][:, R.MATCH].sum() > 0
    assert restated['17x20 white'][0]['sizes'].shape == (2,)


def test_encoding_twice_gives_the_same_bytes(batches, encoded):
    from torch_utils.ops import png_encode
    for name in ('128x384 panel', 'three of 40x24', '20x2800 halves'):
        assert png_encode.encode(torch.from_numpy(batches[name]).cuda()) == encoded[name][2], name


def _pil_bytes(img):
    b = io.BytesIO()
    PIL.Image.fromarray(img).save(b, format='PNG')
    return len(b.getvalue())


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_sizes_stay_within_their_conditions(seed):
    """Conditions of the feature, not measurements: a photograph within 1.05 x PIL's default save, a panel within 1.15 x, uniform
    noise within 1.03 x its raw bytes.  (Measured with 16 rows per segment: 1.004, 1.124 and 1.018.)"""
    from torch_utils.ops import png_encode
    size = lambda img: len(png_encode.encode(torch.from_numpy(img[None]).cuda())[0])
    photograph, panel, noise = R.photograph(128, 384, seed), R.panel(128, 384, 80, seed), _noise(64, 96, seed)
    figures = size(photograph) / _pil_bytes(photograph), size(panel) / _pil_bytes(panel), size(noise) / noise.size
    print('seed %d: photograph %.4f x PIL, panel %.4f x PIL, noise %.4f x raw' % ((seed,) + figures))
    assert figures[0] <= 1.05 and figures[1] <= 1.15 and figures[2] <= 1.03, figures


def test_refusals(monkeypatch):
    from torch_utils.ops import _native, png_encode
    launches = []
    real = _native.lib().pasta_png_encode
    monkeypatch.setattr(_native.lib(), 'pasta_png_encode', lambda *a: launches.append(a) or real(*a))
    with pytest.raises(RuntimeError, match='tensor is on cpu'):
        png_encode.encode(torch.zeros([1, 4, 4, 3], dtype=torch.uint8))
    with pytest.raises(RuntimeError, match='png_filter: 4 channels'):
        png_encode.encode(torch.zeros([1, 4, 4, 4], dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError, match=r'png_filter: width 0 \(1 \.\. 8192\)'):
        png_encode.encode(torch.zeros([1, 4, 0, 3], dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError, match=r'png_filter: width 8193 \(1 \.\. 8192\)'):
        png_encode.encode(torch.zeros([1, 1, 8193, 3], dtype=torch.uint8, device='cuda'))
    with pytest.raises(RuntimeError, match='expected a uint8'):
        png_encode.encode(torch.zeros([1, 4, 4, 3], device='cuda'))
    with pytest.raises(RuntimeError, match='2 images and 1 paths'):
        png_encode.save(torch.zeros([2, 4, 4, 3], dtype=torch.uint8, device='cuda'), ['a.png'])
    assert not launches                                             # the filter entry refused before its launch, and nothing went on
