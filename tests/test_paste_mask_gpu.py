"""pasta_photo_paste_mask_u8 (training.tryon_pairs.photo_paste_mask) against the numpy restatement tests/paste_mask_ref.py, byte
for byte: both forms of the kernel (four pixels per thread where the widths and pointers allow it, one otherwise), the three
kinds of heads, with and without the palm mask; the six-plane statement against torch.argmax on the device; the kept-parts
rules against metrics.tryon_fidelity.keep_mask; the refusals."""

import numpy as np
import pytest
import torch

import paste_mask_ref as PM

pytestmark = pytest.mark.gpu

# (N, H, W, Ht).  c0 = 1 and 5: one pixel per thread; (2, 40, 24) in 48 (c0 = 12, H < Ht) and the test set's 256 x 192: four.
SHAPES = [(3, 19, 17, 19), (2, 45, 35, 45), (2, 40, 24, 48), (1, 256, 192, 256)]
KINDS = ('logits', 'sigmoids', 'none')
KEEP = (1, 2, 4, 13, 18, 19)


def _content_pixels(rng, count, n, h, w, c0):
    """``count`` distinct pixels of the content region as (item, row, column in the heads)."""
    flat = rng.choice(n * h * w, size=count, replace=False)
    return flat // (h * w), (flat // w) % h, c0 + flat % w


def _logits(rng, n, h, w, ht):
    c0 = (ht - w) // 2
    x = rng.uniform(-3, 3, size=[n, 6, ht, ht]).astype(np.float32)
    i, y, c = _content_pixels(rng, 60, n, h, w, c0)
    top = x[i, :, y, c].max(axis=1)
    for lo, (a, b) in zip(range(0, 30, 5), ((0, 1), (1, 2), (2, 5), (3, 4), (0, 5), (4, 5))):     # exact ties of the largest value
        s = slice(lo, lo + 5)
        x[i[s], a, y[s], c[s]] = top[s]
        x[i[s], b, y[s], c[s]] = top[s]
    x[i[30:33], :, y[30:33], c[30:33]] = 1.5                         # all six equal
    x[i[33:36], 0, y[33:36], c[33:36]] = -0.0                        # -0 and +0 tie
    x[i[33:36], 1:, y[33:36], c[33:36]] = 0.0
    x[i[36:42], 0, y[36:42], c[36:42]] = np.nan                      # NaN in plane 0
    for k, j in zip((1, 2, 3, 4, 5, 3), range(42, 48)):              # NaN in a later plane
        x[i[j], k, y[j], c[j]] = np.nan
    x[i[48:51], 2, y[48:51], c[48:51]] = np.nan                      # two NaN: the first wins
    x[i[48:51], 4, y[48:51], c[48:51]] = np.nan
    x[i[51:56], :, y[51:56], c[51:56]] = np.nan                      # NaN in every plane
    x[i[56:60], 3, y[56:60], c[56:60]] = np.inf
    return x


def _sigmoids(rng, n, h, w, ht):
    c0 = (ht - w) // 2
    u, l = (rng.uniform(0, 1, size=[n, 1, ht, ht]).astype(np.float32) for _ in range(2))
    i, y, c = _content_pixels(rng, 40, n, h, w, c0)
    u[i[:8], 0, y[:8], c[:8]] = 0.5                                  # exactly 0.5 is not "upper"
    l[i[4:12], 0, y[4:12], c[4:12]] = 0.5
    u[i[12:20], 0, y[12:20], c[12:20]] = np.nan
    l[i[16:24], 0, y[16:24], c[16:24]] = np.nan
    u[i[24:28], 0, y[24:28], c[24:28]] = np.nextafter(np.float32(0.5), np.float32(1))
    l[i[28:32], 0, y[28:32], c[28:32]] = np.nextafter(np.float32(0.5), np.float32(1))
    u[i[32:36], 0, y[32:36], c[32:36]] = 0.9                         # both claim: upper
    l[i[32:36], 0, y[32:36], c[32:36]] = 0.9
    return u, l


def _rules(rng, n):
    ones = np.full([n, 256], 0b1111, np.uint8)
    mixed = rng.randint(0, 16, size=[n, 256]).astype(np.uint8)
    mixed[0] = 0
    mixed[-1, ::2] = 0b1111
    return {'random': rng.randint(0, 16, size=[n, 256]).astype(np.uint8), 'zero': np.zeros([n, 256], np.uint8), 'all': ones,
            'a row of each': mixed}


@pytest.fixture(scope='module', params=SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def case(request):
    n, h, w, ht = request.param
    rng = np.random.RandomState(n * 1000 + h)
    parsing = rng.randint(0, 20, size=[n, h, w]).astype(np.uint8)
    parsing.reshape(-1)[rng.choice(parsing.size, size=6, replace=False)] = (200, 255, 200, 255, 20, 128)
    palm = (rng.rand(n, h, ht) < 0.08).astype(np.uint8) * rng.choice(np.uint8([1, 2, 255]), size=[n, h, ht])
    heads = dict(logits=(_logits(rng, n, h, w, ht),), sigmoids=_sigmoids(rng, n, h, w, ht), none=())
    cu = lambda a: torch.from_numpy(a).cuda()
    return dict(shape=request.param, c0=(ht - w) // 2, parsing=parsing, palm=palm, heads=heads, rules=_rules(rng, n),
                parsing_gpu=cu(parsing), palm_gpu=cu(palm), heads_gpu={k: tuple(cu(x) for x in v) for k, v in heads.items()})


@pytest.mark.parametrize('with_palm', [True, False], ids=['palm', 'no palm'])
@pytest.mark.parametrize('kind', KINDS)
def test_entry_equals_the_restatement(case, kind, with_palm):
    from training.tryon_pairs import photo_paste_mask
    n, h, w, ht = case['shape']
    palm, palm_gpu = (case['palm'], case['palm_gpu']) if with_palm else (None, None)
    seen = set()
    for name, rule in case['rules'].items():
        got = photo_paste_mask(case['parsing_gpu'], palm_gpu, torch.from_numpy(rule).cuda(), case['heads_gpu'][kind], case['c0'])
        assert got.dtype == torch.uint8 and tuple(got.shape) == (n, h, w)
        want = PM.paste_mask(case['parsing'], palm, rule, case['heads'][kind], case['c0'])
        bad = np.argwhere(got.cpu().numpy() != want)
        assert len(bad) == 0, (name, kind, with_palm, len(bad), bad[:5].tolist())
        seen |= set(np.unique(want).tolist())
        if name == 'zero':                                      # without the restatement: only the palm term is left
            assert torch.equal(got, (palm_gpu[:, :, case['c0']:case['c0'] + w] != 0).to(torch.uint8) if with_palm else torch.zeros_like(got))
        if name == 'all':
            assert bool((got == 1).all())
    assert seen == {0, 1}


def test_the_statement_is_torch_argmax(case):
    """Rule rows that allow exactly statement k turn the entry's output into (s == k): held to torch.argmax on the device and
    the class table, not to the restatement."""
    from training.tryon_pairs import photo_paste_mask
    n, h, w, ht = case['shape']
    c0 = case['c0']
    logits, = case['heads_gpu']['logits']
    label = torch.argmax(logits, dim=1)[:, :h, c0:c0 + w]
    s = torch.tensor([0, 1, 2, 3, 3, 3], device='cuda')[label]
    assert np.array_equal(s.cpu().numpy(), PM.statement(case['heads']['logits'], c0, w, (n, h, w)))        # and so is the restatement
    assert len(torch.unique(label)) == 6
    u, l = (x[:, 0, :h, c0:c0 + w] for x in case['heads_gpu']['sigmoids'])
    s2 = torch.where(u > 0.5, 1, torch.where(l > 0.5, 2, 0))
    for k in range(4):
        rule = torch.full([n, 256], 1 << k, dtype=torch.uint8, device='cuda')
        assert torch.equal(photo_paste_mask(case['parsing_gpu'], None, rule, (logits,), c0), (s == k).to(torch.uint8)), k
        assert torch.equal(photo_paste_mask(case['parsing_gpu'], None, rule, case['heads_gpu']['sigmoids'], c0), (s2 == k).to(torch.uint8)), k
        assert torch.equal(photo_paste_mask(case['parsing_gpu'], None, rule, (), c0), torch.full_like(s, int(k == 0), dtype=torch.uint8)), k


def test_sixteen_bit_heads_are_cast(case):
    from training.tryon_pairs import photo_paste_mask
    rule = torch.from_numpy(case['rules']['random']).cuda()
    for kind in ('logits', 'sigmoids'):
        half = tuple(x.to(torch.bfloat16) for x in case['heads_gpu'][kind])
        got = photo_paste_mask(case['parsing_gpu'], case['palm_gpu'], rule, half, case['c0'])
        assert torch.equal(got, photo_paste_mask(case['parsing_gpu'], case['palm_gpu'], rule, tuple(x.float() for x in half), case['c0']))


def test_kept_parts_rules_without_heads_are_keep_mask(case):
    from metrics import tryon_fidelity
    from training.tryon_pairs import paste_rules, photo_paste_mask
    n, h, w, ht = case['shape']
    assert tuple(tryon_fidelity.KEEP_LABELS) == KEEP
    own = list(range(n))
    rule = paste_rules(True, False, False, own, own, own, 256).cuda()
    if h == ht:
        want = tryon_fidelity.keep_mask(dict(parsing=case['parsing_gpu'], palm=case['palm_gpu']))
    else:                                   # keep_mask reads the palm mask of a padded square: its expression with this c0
        want = (case['palm_gpu'][:, :, case['c0']:case['c0'] + w] != 0) | torch.isin(case['parsing_gpu'], torch.tensor(KEEP, dtype=torch.uint8, device='cuda'))
        want = want.to(torch.uint8)
    assert torch.equal(photo_paste_mask(case['parsing_gpu'], case['palm_gpu'], rule, (), case['c0']), want)
    assert torch.equal(photo_paste_mask(case['parsing_gpu'], case['palm_gpu'], rule, case['heads_gpu']['logits'], case['c0']), want)
    assert 0 < int(want.sum()) < want.numel()


@pytest.mark.parametrize('kind', ['logits', 'sigmoids'])
def test_a_plane_pointer_that_is_not_aligned_takes_the_scalar_form(kind):
    """The four-pixel form loads 16 bytes of a plane at a time; the entry, handed planes that start 4 bytes off a 16-byte boundary,
    must take the other form: the same bytes either way."""
    from torch_utils.ops import _native
    n, h, w, ht = 2, 40, 24, 48
    c0 = (ht - w) // 2
    rng = np.random.RandomState(11)
    parsing = rng.randint(0, 20, size=[n, h, w]).astype(np.uint8)
    palm = (rng.rand(n, h, ht) < 0.08).astype(np.uint8)
    rule = rng.randint(0, 16, size=[n, 256]).astype(np.uint8)
    heads = (_logits(rng, n, h, w, ht),) if kind == 'logits' else _sigmoids(rng, n, h, w, ht)
    want = PM.paste_mask(parsing, palm, rule, heads, c0)
    shifted = []
    for x in heads:
        store = torch.zeros([x.size + 1], dtype=torch.float32, device='cuda')
        store[1:] = torch.from_numpy(x).cuda().reshape(-1)
        shifted.append(store[1:].view(*x.shape))
        assert shifted[-1].data_ptr() % 16 == 4
    P = _native.ptr
    parsing_gpu, palm_gpu, rule_gpu = (torch.from_numpy(a).cuda() for a in (parsing, palm, rule))     # named: a pointer keeps no tensor alive
    out = torch.empty([n, h, w], dtype=torch.uint8, device='cuda')
    a, b = (shifted + [None])[:2]
    _native.check(_native.lib().pasta_photo_paste_mask_u8(P(parsing_gpu), P(palm_gpu), P(rule_gpu), P(a), P(b), 6 if kind == 'logits' else 1, P(out),
                                                          n, h, w, ht, _native.stream()))
    assert np.array_equal(out.cpu().numpy(), want)


def test_refusals():
    from torch_utils.ops import _native
    from training.tryon_pairs import photo_paste_mask
    n, h, w, ht, c0 = 2, 8, 6, 8, 1
    parsing = torch.zeros([n, h, w], dtype=torch.uint8, device='cuda')
    palm = torch.zeros([n, h, ht], dtype=torch.uint8, device='cuda')
    rule = torch.zeros([n, 256], dtype=torch.uint8, device='cuda')
    six = torch.zeros([n, 6, ht, ht], device='cuda')
    one = torch.zeros([n, 1, ht, ht], device='cuda')
    assert photo_paste_mask(parsing, palm, rule, (six,), c0).shape == (n, h, w)
    assert photo_paste_mask(parsing, None, rule, (one, one), c0).shape == (n, h, w)
    for args, words in (((parsing.cpu(), palm, rule, (six,), c0), 'GPU'), ((parsing, palm.cpu(), rule, (six,), c0), 'GPU'),
                        ((parsing, palm, rule.cpu(), (six,), c0), 'GPU'), ((parsing, palm, rule, (six.cpu(),), c0), 'GPU'),
                        ((parsing.float(), palm, rule, (), c0), 'uint8'), ((parsing, palm.bool(), rule, (), c0), 'uint8'),
                        ((parsing, palm, rule.int(), (), c0), 'uint8'), ((parsing, palm, rule, (six.long(),), c0), 'floating'),
                        ((parsing[0], palm, rule, (), c0), r'\[N, H, W\]'), ((parsing, palm, rule[:1], (), c0), 'rule'),
                        ((parsing, palm, rule[:, :255], (), c0), 'rule'), ((parsing, palm[:1], rule, (), c0), 'palm'),
                        ((parsing, palm[:, :7], rule, (), c0), 'palm'), ((parsing, palm, rule, (six,), 0), 'c0'),
                        ((parsing, None, rule, (six,), 2), 'c0'), ((parsing, palm, rule, (one,), c0), 'heads'),
                        ((parsing, palm, rule, (six, six), c0), 'heads'), ((parsing, palm, rule, (one, one, one), c0), 'heads'),
                        ((parsing, palm, rule, (six[:, :5],), c0), 'heads'), ((parsing, palm, rule, (six[:1],), c0), 'heads'),
                        ((parsing, palm, rule, (one, one[:, :, :7]), c0), 'heads'), ((parsing, palm, rule, (six[0],), c0), 'heads')):
        with pytest.raises(ValueError, match=words):
            photo_paste_mask(*args)
    # the entry's own refusals, before any launch
    lib, P = _native.lib(), _native.ptr
    out = torch.empty_like(parsing)
    N = P(None)
    for args, words in (((N, P(palm), P(rule), P(six), N, 6, P(out), n, h, w, ht), b'null pointer'),
                        ((P(parsing), P(palm), N, P(six), N, 6, P(out), n, h, w, ht), b'null pointer'),
                        ((P(parsing), P(palm), P(rule), P(six), N, 6, N, n, h, w, ht), b'null pointer'),
                        ((P(parsing), P(palm), P(rule), P(six), N, 3, P(out), n, h, w, ht), b'head_planes 3'),
                        ((P(parsing), P(palm), P(rule), P(six), N, -1, P(out), n, h, w, ht), b'head_planes -1'),
                        ((P(parsing), P(palm), P(rule), N, N, 6, P(out), n, h, w, ht), b'6 head planes'),
                        ((P(parsing), P(palm), P(rule), P(six), P(one), 6, P(out), n, h, w, ht), b'6 head planes'),
                        ((P(parsing), P(palm), P(rule), P(one), N, 1, P(out), n, h, w, ht), b'1 head planes'),
                        ((P(parsing), P(palm), P(rule), P(one), N, 0, P(out), n, h, w, ht), b'0 head planes'),
                        ((P(parsing), P(palm), P(rule), N, P(one), 0, P(out), n, h, w, ht), b'0 head planes'),
                        ((P(parsing), P(palm), P(rule), N, N, 0, P(out), n, h, ht + 1, ht), b'bad shape'),
                        ((P(parsing), P(palm), P(rule), N, N, 0, P(out), n, ht + 1, w, ht), b'bad shape'),
                        ((P(parsing), P(palm), P(rule), N, N, 0, P(out), 0, h, w, ht), b'bad shape'),
                        ((P(parsing), P(palm), P(rule), N, N, 0, P(out), n, h, 0, ht), b'bad shape'),
                        ((P(parsing), P(palm), P(rule), N, N, 0, P(out), n, h, w, 4097), b'bad shape')):
        assert lib.pasta_photo_paste_mask_u8(*args, _native.stream()) != 0, words
        assert words in lib.pasta_last_error() and b'photo_paste_mask_u8' in lib.pasta_last_error(), (words, lib.pasta_last_error())
