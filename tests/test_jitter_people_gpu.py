"""Jittered people on the GPU (--jitter-people; csrc/tryon_inputs.hip's pasta_tryon_jitter_u8, training/tryon_batch.py's
jitter_batch) -- EXACT: the entry against the numpy statement (tests/jitter_ref.py) byte for byte at widths on both of its
paths; both training builders on a numbered batch against their plain build of the same people jittered on the host; the
numbered stream of a continued run; a short training run whose sample grid does not see the option."""
import json
import os

import numpy as np
import pytest
import torch

import jitter_ref as JR
from train_grid_tree import make_tree as make_grid_tree
from tryon_512_train_tree import erase_masks, make_512_train_tree
from tryon_tree import make_tree

pytestmark = pytest.mark.gpu

SPEC = dict(scale=0.3, rotate=20.0, shift=0.1, colour=0.4)
SEED = 5


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _entry(image, parsing, affine, colour, outs=None, shape=None):
    """pasta_tryon_jitter_u8 on device tensors -> (status, image_out, parsing_out); the outputs start as 7 everywhere."""
    from torch_utils.ops import _native as N
    n, h, w, _ = image.shape if shape is None else (*shape, 3)
    image_out, parsing_out = outs if outs is not None else (torch.full_like(image, 7), torch.full_like(parsing, 7))
    status = N.lib().pasta_tryon_jitter_u8(N.ptr(image), N.ptr(parsing), N.ptr(affine), N.ptr(colour), N.ptr(image_out), N.ptr(parsing_out),
                                           n, h, w, N.stream())
    torch.cuda.synchronize()
    return status, image_out, parsing_out


def _kernel_case(h, w, seed):
    """Three items: random parameters at the top of every range; the identity; scale 0.5 with a shift of several canvases, so
    that every tap and every label read clamps."""
    rng = np.random.default_rng(seed)
    n = 3
    image = rng.integers(0, 256, [n, h, w, 3], dtype=np.uint8)
    parsing = rng.permutation(np.arange(n * h * w) % 256).astype(np.uint8).reshape(n, h, w)       # every byte value when there is room
    sign = lambda: float(rng.choice([-1.0, 1.0]))
    top = ((1.5 ** sign(), 45.0 * sign(), 0.25 * w * sign(), 0.25 * h * sign()), (1.5 ** sign(), 1.5 ** sign(), 32.0 * sign()))
    far = ((0.5, 0.0, 4.0 * w + 7.3, -(4.0 * h + 3.7)), JR.IDENTITY_TONE)
    items = (top, (JR.IDENTITY_GEOMETRY, JR.IDENTITY_TONE), far)
    affine = np.array([JR.affine_q16(g, h, w) for g, _ in items], np.int64)
    colour = np.array([JR.colour_q8(t) for _, t in items], np.int32)
    return image, parsing, affine, colour


@pytest.mark.parametrize('h,w', [(5, 1), (6, 2), (7, 15), (8, 16), (9, 17), (5, 48), (6, 192)])
def test_entry_equals_the_statement(h, w):
    image, parsing, affine, colour = _kernel_case(h, w, 16 * h + w)
    if parsing.size >= 256:
        assert len(np.unique(parsing)) == 256
    assert affine[1].tolist() == list(JR.IDENTITY_AFFINE) and colour[1].tolist() == list(JR.IDENTITY_COLOUR)
    want_i, want_p = JR.resample_arrays(image, parsing, affine, colour)
    status, got_i, got_p = _entry(_cu(image), _cu(parsing), _cu(affine), _cu(colour))
    assert status == 0
    got_i, got_p = got_i.cpu().numpy(), got_p.cpu().numpy()
    for n in range(3):
        assert np.array_equal(got_i[n], want_i[n]), (h, w, n, 'image', int((got_i[n] != want_i[n]).sum()))
        assert np.array_equal(got_p[n], want_p[n]), (h, w, n, 'parsing', int((got_p[n] != want_p[n]).sum()))
    # the identity item is the input
    assert np.array_equal(got_i[1], image[1]) and np.array_equal(got_p[1], parsing[1])
    # the far item reads the clamped corner everywhere: x far to the left, y far below
    assert (got_i[2] == image[2, h - 1, 0]).all() and (got_p[2] == parsing[2, h - 1, 0]).all()
    if w > 2:
        assert not np.array_equal(got_i[0], image[0])


def test_entry_quarter_turn_is_rot90():
    rng = np.random.default_rng(1)
    image, parsing = rng.integers(0, 256, [2, 7, 7, 3], dtype=np.uint8), rng.integers(0, 256, [2, 7, 7], dtype=np.uint8)
    affine = np.array([JR.affine_q16((1.0, 90.0, 0.0, 0.0), 7, 7), JR.affine_q16((1.0, -90.0, 0.0, 0.0), 7, 7)], np.int64)
    colour = np.array([JR.IDENTITY_COLOUR] * 2, np.int32)
    status, got_i, got_p = _entry(_cu(image), _cu(parsing), _cu(affine), _cu(colour))
    assert status == 0
    for n, k in ((0, -1), (1, 1)):
        assert np.array_equal(got_i[n].cpu().numpy(), np.rot90(image[n], k)) and np.array_equal(got_p[n].cpu().numpy(), np.rot90(parsing[n], k))


@pytest.mark.parametrize('w', [16, 48])
def test_entry_on_tensors_that_are_not_16_byte_aligned(w):
    """A width of the wide path from an odd address: the pixel-by-pixel path, the same bytes."""
    image, parsing, affine, colour = _kernel_case(6, w, 99)
    want_i, want_p = JR.resample_arrays(image, parsing, affine, colour)
    odd = lambda a: torch.cat([torch.zeros(1, dtype=torch.uint8, device='cuda'), _cu(a).reshape(-1)])[1:].view(a.shape)
    src_i, src_p = odd(image), odd(parsing)
    outs = (odd(np.full_like(image, 7)), odd(np.full_like(parsing, 7)))
    assert src_i.data_ptr() % 16 == 1 and outs[0].data_ptr() % 16 == 1 and outs[1].data_ptr() % 16 == 1
    status, got_i, got_p = _entry(src_i, src_p, _cu(affine), _cu(colour), outs=outs)
    assert status == 0
    assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(got_p.cpu().numpy(), want_p)
    # only one tensor off: aligned inputs, an output from an odd address
    status, got_i, got_p = _entry(_cu(image), _cu(parsing), _cu(affine), _cu(colour), outs=(torch.full_like(_cu(image), 7), odd(np.full_like(parsing, 7))))
    assert status == 0
    assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(got_p.cpu().numpy(), want_p)


@pytest.mark.parametrize('w', [13, 32])
def test_entry_colour_clamps_at_0_and_255(w):
    rng = np.random.default_rng(3)
    image, parsing = rng.integers(0, 256, [3, 6, w, 3], dtype=np.uint8), rng.integers(0, 256, [3, 6, w], dtype=np.uint8)
    steep = [1024, 0, 0, -384 * 256, 0, 1024, 0, -384 * 256, 0, 0, 1024, -384 * 256]           # 4 v - 384: below 0 and above 255
    negative = [-256, 0, 0, 255 * 256, 0, -256, 0, 255 * 256, 0, 0, -256, 255 * 256]           # 255 - v
    mixed = [256, 256, 256, 0, -256, -256, 0, 64 * 256, 77, 150, 29, 0]                        # R+G+B; 64-R-G; the luma
    affine = np.array([JR.IDENTITY_AFFINE, JR.IDENTITY_AFFINE, JR.affine_q16((1.1, 10.0, 0.5, -0.25), 6, w)], np.int64)
    colour = np.array([steep, negative, mixed], np.int32)
    want_i, want_p = JR.resample_arrays(image, parsing, affine, colour)
    v = image[0].astype(np.int32)
    assert np.array_equal(want_i[0], np.clip(4 * v - 384, 0, 255)) and (4 * v - 384 < 0).any() and (4 * v - 384 > 255).any()
    assert (want_i[0] == 0).any() and (want_i[0] == 255).any()
    assert np.array_equal(want_i[1], 255 - image[1])
    assert (want_i[2][..., 0] == 255).any() and (want_i[2][..., 1] == 0).any()
    status, got_i, got_p = _entry(_cu(image), _cu(parsing), _cu(affine), _cu(colour))
    assert status == 0
    assert np.array_equal(got_i.cpu().numpy(), want_i) and np.array_equal(got_p.cpu().numpy(), want_p)


def test_entry_past_2_to_the_31_bytes():
    """Four items of 16384 x 16384, the largest canvas: the fourth item's bytes start past 2^31.  Items 0-2 are the identity (the
    copy), item 3 an integer shift, checked against the clamped index shift on the device."""
    side, tx, ty = 16384, 3, -5
    gen = torch.Generator(device='cuda').manual_seed(0)
    image = torch.randint(0, 256, [4, side, side, 3], dtype=torch.uint8, device='cuda', generator=gen)
    parsing = torch.randint(0, 256, [4, side, side], dtype=torch.uint8, device='cuda', generator=gen)
    assert 3 * side * side * 3 > 2 ** 31
    affine = np.array([JR.IDENTITY_AFFINE] * 3 + [JR.affine_q16((1.0, 0.0, float(tx), float(ty)), side, side)], np.int64)
    status, got_i, got_p = _entry(image, parsing, _cu(affine), _cu(np.array([JR.IDENTITY_COLOUR] * 4, np.int32)),
                                  outs=(torch.empty_like(image), torch.empty_like(parsing)))
    assert status == 0
    assert torch.equal(got_i[:3], image[:3]) and torch.equal(got_p[:3], parsing[:3])
    ys = (torch.arange(side, device='cuda') - ty).clamp(0, side - 1)
    xs = (torch.arange(side, device='cuda') - tx).clamp(0, side - 1)
    assert torch.equal(got_p[3], parsing[3][ys][:, xs])
    assert torch.equal(got_i[3], image[3][ys][:, xs])


def test_entry_refusals():
    from torch_utils.ops import _native as N
    image, parsing, affine, colour = (_cu(a) for a in _kernel_case(5, 16, 3))
    lib = N.lib()
    fresh = lambda: (torch.full_like(image, 7), torch.full_like(parsing, 7))
    def refused(words, *args, **kwargs):
        outs = kwargs['outs']
        status, *_ = _entry(*args, **kwargs)
        assert status != 0, words
        assert words in lib.pasta_last_error() and b'tryon_jitter_u8' in lib.pasta_last_error(), (words, lib.pasta_last_error())
        for o, src in zip(outs, (image, parsing)):          # nothing was launched: an output that is no input still holds its 7s
            if o is not None and o is not src:
                assert (o == 7).all(), words
    refused(b'null pointer', None, parsing, affine, colour, outs=fresh(), shape=(3, 5, 16))
    refused(b'null pointer', image, None, affine, colour, outs=fresh())
    refused(b'null pointer', image, parsing, None, colour, outs=fresh())
    refused(b'null pointer', image, parsing, affine, None, outs=fresh())
    refused(b'null pointer', image, parsing, affine, colour, outs=(None, fresh()[1]))
    refused(b'null pointer', image, parsing, affine, colour, outs=(fresh()[0], None))
    before = (image.clone(), parsing.clone())
    refused(b'an output is its input', image, parsing, affine, colour, outs=(image, fresh()[1]))
    refused(b'an output is its input', image, parsing, affine, colour, outs=(fresh()[0], parsing))
    assert torch.equal(image, before[0]) and torch.equal(parsing, before[1])
    for shape in ((0, 5, 16), (65536, 5, 16), (3, 0, 16), (3, 16385, 16), (3, 5, 0), (3, 5, 16385), (3, 5, -16)):
        refused(b'bad shape', image, parsing, affine, colour, outs=fresh(), shape=shape)
    # and the same arguments, complete, are taken
    assert _entry(image, parsing, affine, colour, outs=fresh())[0] == 0


# ---- the builders ----

def _equal_batches(got, want):
    from training.tryon_batch import FullBodyBatch
    for k in FullBodyBatch.KEYS:
        g, v = got.tensors[k], want.tensors[k]
        assert g.dtype == torch.float32 and g.shape == v.shape and torch.equal(g, v), (k, int((g != v).sum()))
    assert sorted(got.stages) == sorted(want.stages)
    for k in got.stages:
        g, v = got.stages[k], want.stages[k]
        assert g.dtype == v.dtype and g.shape == v.shape and torch.equal(g, v), ('stage', k, int((g != v).sum()))
    assert torch.equal(got.image, want.image)


def _builder_case(builder, samples, positions, monkeypatch):
    from training import tryon_batch
    from training.dataset import collate
    H, W = samples[0]['parsing'].shape
    numbered = dict(collate(samples), jitter=dict(spec=SPEC, seed=SEED, positions=np.asarray(positions, np.int64)))
    got = builder.build(numbered, keep_stages=True)
    host = [JR.jitter_raw(s, *JR.parameters(SPEC, SEED, t, H, W)) for s, t in zip(samples, positions)]
    want = builder.build(collate(host), keep_stages=True)
    _equal_batches(got, want)
    assert torch.equal(got.image.cpu(), torch.from_numpy(np.stack([s['image'] for s in host])))
    plain = builder.build(collate(samples), keep_stages=True)
    for k in ('real_img', 'pose', 'gt_parsing', 'style_input'):
        assert not torch.equal(got.tensors[k], plain.tensors[k]), k
    # the erase masks belong to the canvas: the same file, the same place
    assert all(np.array_equal(h['erase_mask'], s['erase_mask']) for h, s in zip(host, samples))
    # drawn parameters replaced by the identity: the plain build, bit for bit
    n = len(samples)
    monkeypatch.setattr(tryon_batch, 'jitter_parameters',
                        lambda spec, seed, positions, H, W: (np.tile(JR.IDENTITY_GEOMETRY, (n, 1)), np.tile(JR.IDENTITY_TONE, (n, 1))))
    _equal_batches(builder.build(numbered, keep_stages=True), plain)
    monkeypatch.undo()
    return got


def test_builder_256_equals_its_build_of_host_jittered_people(tmp_path_factory, monkeypatch):
    """The five people of the tiny tree (the empty ``people``, joints off the canvas, the forearm of length zero) at fixed
    positions, erase masks of the tree's two sizes and two more."""
    from training.dataset import UvitonDatasetFull
    from training.tryon_batch import FullBodyBatchBuilder
    ds = UvitonDatasetFull(make_tree(tmp_path_factory.mktemp('jitter_gpu')))
    samples = [ds[i] for i in range(5)]
    rng = np.random.default_rng(7)
    samples[2]['erase_mask'] = (rng.uniform(size=[77, 131]) < 0.3).astype(np.uint8) * np.uint8(255)
    samples[4]['erase_mask'] = rng.integers(0, 256, [256, 192], dtype=np.uint8)
    _builder_case(FullBodyBatchBuilder('cuda'), samples, [11, 3, 2 ** 33, 0, 4], monkeypatch)


def test_builder_256_mirrors_first_then_jitters(tmp_path_factory):
    import mirror_ref as MR
    from training.dataset import UvitonDatasetFull, collate
    from training.tryon_batch import FullBodyBatchBuilder
    ds = UvitonDatasetFull(make_tree(tmp_path_factory.mktemp('jitter_gpu_mirror')), mirror_people=True)
    flags = (0, 1, 1)
    samples = [ds[i + 5 * f] for i, f in enumerate(flags)]
    assert [s['xflip'] for s in samples] == list(flags)
    positions = [6, 7, 8]
    builder = FullBodyBatchBuilder('cuda')
    got = builder.build(dict(collate(samples), jitter=dict(spec=SPEC, seed=SEED, positions=np.asarray(positions, np.int64))), keep_stages=True)
    mirrored = [MR.mirror_raw(s) if s['xflip'] else {k: v for k, v in s.items() if k != 'xflip'} for s in samples]
    host = [JR.jitter_raw(s, *JR.parameters(SPEC, SEED, t, 256, 192)) for s, t in zip(mirrored, positions)]
    _equal_batches(got, builder.build(collate(host), keep_stages=True))


def test_builder_512_equals_its_build_of_host_jittered_people(tmp_path_factory, monkeypatch):
    """The three listed people of the 512 tree (the folded arm, the missing wrist and ankle, the elbow far outside) with erase
    masks of three sizes."""
    from training.dataset import UvitonDatasetFull_512
    from training.tryon_regions import FullBodyRegionBatchBuilder
    ds = UvitonDatasetFull_512(make_512_train_tree(tmp_path_factory.mktemp('jitter_gpu_512')))
    samples = [ds[i] for i in ds.vis_index]
    for s, m in zip(samples, erase_masks()):
        s['erase_mask'] = m
    got = _builder_case(FullBodyRegionBatchBuilder('cuda'), samples, [1, 12, 5], monkeypatch)
    assert got.tensors['denorm_upper_mask'].any() and got.tensors['denorm_lower_mask'].any()


# ---- the stream and the loop ----

def test_a_stream_started_at_4_is_the_stream_from_batch_3(tmp_path_factory):
    from training.tryon_batch import FullBodyBatch
    from training.training_loop_wo_flow_fullbody import _data_batches
    tree = make_tree(tmp_path_factory.mktemp('jitter_gpu_stream'))
    def stream(count, cur_nimg):
        _, _, batches = _data_batches(1, 0, 2, 0, torch.device('cuda'), dict(class_name='training.dataset.UvitonDatasetFull', path=tree),
                                      dict(num_workers=0, pin_memory=True), cur_nimg=cur_nimg, people_jitter=SPEC)
        return [next(batches) for _ in range(count)]
    whole, later = stream(4, 0), stream(2, 4)
    for a, b in zip(whole[2:], later):
        for k in FullBodyBatch.KEYS:
            assert torch.equal(a.tensors[k], b.tensors[k]), k
        assert torch.equal(a.image, b.image)
    # the people come round again within these batches (five people, eight items), jittered anew
    _, _, plain = _data_batches(1, 0, 2, 0, torch.device('cuda'), dict(class_name='training.dataset.UvitonDatasetFull', path=tree),
                                dict(num_workers=0, pin_memory=True))
    assert not torch.equal(next(plain).tensors['real_img'], whole[0].tensors['real_img'])


def test_training_run_on_jittered_people_and_its_sample_grid(tmp_path_factory, tmp_path, monkeypatch):
    """Four iterations of batch 2 with the option: finite losses and parameters, four numbered batches through ``jitter_batch``.
    The sample grid written before the first iteration is byte for byte the one of a run without the option."""
    from training import tryon_batch
    from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
    tree = make_grid_tree(tmp_path_factory.mktemp('jitter_gpu_loop'))
    calls = []
    real = tryon_batch.jitter_batch
    def spy(raw, *args):
        calls.append(raw['jitter']['positions'].tolist() if 'jitter' in raw else None)
        return real(raw, *args)
    monkeypatch.setattr(tryon_batch, 'jitter_batch', spy)
    def run(run_dir, iters, **kwargs):
        os.makedirs(run_dir)
        return training_loop(batch_size=2, batch_gpu=2, cfg=fashion_config(channel_base=2048, mbstd_group_size=2), device=torch.device('cuda'),
                             training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree),
                             data_loader_kwargs=dict(num_workers=0, pin_memory=True), run_dir=str(run_dir), total_kimg=iters * 2 / 1000,
                             image_snapshot_ticks=None, network_snapshot_ticks=None, snapshot_gnum=3, **kwargs)
    step = run(tmp_path / 'on', 4, people_jitter=SPEC)
    assert step.cur_nimg == 8
    assert [c for c in calls if c is not None] == [[0, 1], [2, 3], [4, 5], [6, 7]]
    grid_calls = calls.count(None)
    assert grid_calls >= 1                                       # the grid's people went through the builder unnumbered
    lines = [json.loads(line) for line in open(tmp_path / 'on' / 'stats.jsonl')]
    assert lines
    for line in lines:
        losses = {k: v for k, v in line.items() if k.startswith('Loss/')}
        assert losses and all(np.isfinite(v['mean']) and v['num'] > 0 for v in losses.values()), sorted(losses)
    assert all(torch.isfinite(p).all() for p in step.G.parameters()) and all(torch.isfinite(p).all() for p in step.D.parameters())
    del calls[:]
    run(tmp_path / 'off', 0)
    assert calls == [None] * grid_calls
    for name in ('init_denorm_upper.png', 'init_denorm_lower.png', 'init_retain.png'):
        a, b = open(tmp_path / 'on' / name, 'rb').read(), open(tmp_path / 'off' / name, 'rb').read()
        assert len(a) > 1000 and a == b, name
