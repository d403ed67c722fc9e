"""Mirrored people on the GPU (--mirror-people; csrc/tryon_inputs.hip's pasta_tryon_mirror_u8, training/tryon_batch.py's
mirror_batch) -- EXACT: the entry against the numpy statement (tests/mirror_ref.py) bit for bit at widths on both of its paths;
both training builders on a batch with mixed flags against their build of the same people mirrored on the host with no flag set
(256 x 192) and against the unchanged restatement evaluated on mirrored raw samples (512 x 320); a short training loop on a
mirrored data set."""
import numpy as np
import pytest
import torch

import mirror_ref as MR
import tryon_512_train_ref as TR
from tryon_512_train_tree import erase_masks, make_512_train_tree
from tryon_tree import make_tree

pytestmark = pytest.mark.gpu

EH, EW = 40, 32                          # the erase stack of the kernel cases
ERASE_SIZES = ((1, 1), (EH, EW), (37, 23))


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _entry(image, parsing, erase, erase_hw, flags, lut, outs=None, shape=None):
    """pasta_tryon_mirror_u8 on device tensors (erase may be None) -> (status, image_out, parsing_out, erase_out)."""
    from torch_utils.ops import _native as N
    n, h, w, _ = image.shape if shape is None else (*shape, 3)
    image_out, parsing_out, erase_out = outs if outs is not None else (
        torch.full_like(image, 7), torch.full_like(parsing, 7), None if erase is None else torch.full_like(erase, 7))
    eh, ew = (0, 0) if erase is None else (int(erase.shape[1]), int(erase.shape[2]))
    status = N.lib().pasta_tryon_mirror_u8(N.ptr(image), N.ptr(parsing), N.ptr(erase), N.ptr(erase_hw), N.ptr(flags), N.ptr(lut), N.ptr(image_out),
                                           N.ptr(parsing_out), N.ptr(erase_out), n, h, w, eh, ew, N.stream())
    torch.cuda.synchronize()
    return status, image_out, parsing_out, erase_out


def _kernel_case(w, seed):
    rng = np.random.default_rng(seed)
    n, h = 3, 5
    image = rng.integers(0, 256, [n, h, w, 3], dtype=np.uint8)
    parsing = rng.permutation(np.arange(n * h * w) % 256).astype(np.uint8).reshape(n, h, w)       # every byte value when there is room
    erase, hw = np.zeros([n, EH, EW], np.uint8), np.array(ERASE_SIZES, np.int32)
    for i, (eh, ew) in enumerate(ERASE_SIZES):
        erase[i, :eh, :ew] = rng.integers(0, 256, [eh, ew], dtype=np.uint8)       # the padding is 0, as collate leaves it
    return image, parsing, erase, hw, np.array([1, 0, 1], np.uint8)


@pytest.mark.parametrize('w', [1, 2, 15, 16, 17, 48, 192])
def test_entry_equals_the_statement(w):
    image, parsing, erase, hw, flags = _kernel_case(w, w)
    if parsing.size >= 256:
        assert len(np.unique(parsing)) == 256
    lut = _cu(MR.lut())
    want = MR.mirror_arrays(image, parsing, erase, hw, flags)
    status, *got = _entry(_cu(image), _cu(parsing), _cu(erase), _cu(hw), _cu(flags), lut)
    assert status == 0
    for name, g, v in zip(('image', 'parsing', 'erase'), got, want):
        assert np.array_equal(g.cpu().numpy(), v), (w, name, int((g.cpu().numpy() != v).sum()))
    # the unflagged item is the input, the table not applied (it holds labels 14..19 wherever there is room)
    assert np.array_equal(got[0][1].cpu().numpy(), image[1]) and np.array_equal(got[1][1].cpu().numpy(), parsing[1])
    assert np.array_equal(got[2][1].cpu().numpy(), erase[1])
    assert not got[2][0, 1:].any() and not got[2][2, 37:].any() and not got[2][2, :, 23:].any()      # the padding stays 0
    if w > 1:
        assert not np.array_equal(want[0][0], image[0])
    # without erase masks
    status, image_out, parsing_out, none = _entry(_cu(image), _cu(parsing), None, None, _cu(flags), lut)
    assert status == 0 and none is None
    assert np.array_equal(image_out.cpu().numpy(), want[0]) and np.array_equal(parsing_out.cpu().numpy(), want[1])
    # a table that is not the identity elsewhere is applied as it is, to flagged items only
    odd = np.random.default_rng(1).permutation(256).astype(np.uint8)
    status, _, parsing_out, _ = _entry(_cu(image), _cu(parsing), None, None, _cu(flags), _cu(odd))
    assert status == 0
    for i in range(3):
        assert np.array_equal(parsing_out[i].cpu().numpy(), odd[parsing[i][:, ::-1]] if flags[i] else parsing[i]), i


def test_entry_on_tensors_that_are_not_16_byte_aligned():
    """W = 16 from an odd address: the pixel-by-pixel path, the same bytes."""
    image, parsing, erase, hw, flags = _kernel_case(16, 99)
    want = MR.mirror_arrays(image, parsing, erase, hw, flags)
    odd = lambda a: torch.cat([torch.zeros(1, dtype=torch.uint8, device='cuda'), _cu(a).reshape(-1)])[1:].view(a.shape)
    src_i, src_p = odd(image), odd(parsing)
    outs = (odd(np.full_like(image, 7)), odd(np.full_like(parsing, 7)), torch.full([3, EH, EW], 7, dtype=torch.uint8, device='cuda'))
    assert src_i.data_ptr() % 16 == 1 and outs[1].data_ptr() % 16 == 1
    status, *got = _entry(src_i, src_p, _cu(erase), _cu(hw), _cu(flags), _cu(MR.lut()), outs=outs)
    assert status == 0
    for g, v in zip(got, want):
        assert np.array_equal(g.cpu().numpy(), v)


def test_entry_all_flags_and_no_flags():
    image, parsing, erase, hw, _ = _kernel_case(48, 5)
    lut = _cu(MR.lut())
    for flags in (np.zeros(3, np.uint8), np.ones(3, np.uint8)):
        want = MR.mirror_arrays(image, parsing, erase, hw, flags)
        status, *got = _entry(_cu(image), _cu(parsing), _cu(erase), _cu(hw), _cu(flags), lut)
        assert status == 0
        for g, v in zip(got, want):
            assert np.array_equal(g.cpu().numpy(), v), flags


def test_entry_refusals():
    from torch_utils.ops import _native as N
    image, parsing, erase, hw, flags = (_cu(a) for a in _kernel_case(16, 3))
    lut = _cu(MR.lut())
    lib = N.lib()
    fresh = lambda: (torch.empty_like(image), torch.empty_like(parsing), torch.empty_like(erase))
    def refused(words, *args, **kwargs):
        status, *_ = _entry(*args, **kwargs)
        assert status != 0, words
        assert words in lib.pasta_last_error() and b'tryon_mirror_u8' in lib.pasta_last_error(), (words, lib.pasta_last_error())
    refused(b'null pointer', None, parsing, erase, hw, flags, lut, outs=fresh(), shape=(3, 5, 16))
    refused(b'null pointer', image, None, erase, hw, flags, lut, outs=fresh(), shape=(3, 5, 16))
    refused(b'null pointer', image, parsing, erase, hw, None, lut, outs=fresh())
    refused(b'null pointer', image, parsing, erase, hw, flags, None, outs=fresh())
    refused(b'null pointer', image, parsing, erase, hw, flags, lut, outs=(None, fresh()[1], fresh()[2]))
    a, b, c = fresh()
    refused(b'an output is its input', image, parsing, erase, hw, flags, lut, outs=(image, b, c))
    refused(b'an output is its input', image, parsing, erase, hw, flags, lut, outs=(a, parsing, c))
    refused(b'an output is its input', image, parsing, erase, hw, flags, lut, outs=(a, b, erase))
    for shape in ((0, 5, 16), (3, 0, 16), (3, 5, 0), (3, 5, -16)):
        refused(b'bad shape', image, parsing, erase, hw, flags, lut, outs=fresh(), shape=shape)
    refused(b'null together', image, parsing, erase, hw, flags, lut, outs=(a, b, None))
    refused(b'null together', image, parsing, None, hw, flags, lut, outs=(a, b, c))
    refused(b'erase masks need erase_hw', image, parsing, erase, None, flags, lut, outs=fresh())
    # and the same arguments, complete, are taken
    assert _entry(image, parsing, erase, hw, flags, lut, outs=fresh())[0] == 0


# ---- the builder at 256 x 192 ----

@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return make_tree(tmp_path_factory.mktemp('mirror_gpu'))


def _equal_batches(got, want, items=None):
    from training.tryon_batch import FullBodyBatch
    pick = (lambda t: t) if items is None else (lambda t: t[items])
    for k in FullBodyBatch.KEYS:
        g, v = pick(got.tensors[k]), pick(want.tensors[k])
        assert g.dtype == torch.float32 and g.shape == v.shape and torch.equal(g, v), (k, int((g != v).sum()))
    assert sorted(got.stages) == sorted(want.stages)
    for k in got.stages:
        g, v = pick(got.stages[k]), pick(want.stages[k])
        assert g.dtype == v.dtype and torch.equal(g, v), ('stage', k, int((g != v).sum()))
    assert torch.equal(pick(got.image), pick(want.image))


def test_builder_256_mixed_flags_equal_the_host_mirrored_people(tree):
    """The five people of the tiny tree (the empty ``people``, joints off the canvas, the forearm of length zero), three of them
    flagged, erase masks of the tree's two sizes and two more."""
    from training.dataset import UvitonDatasetFull, collate
    from training.tryon_batch import FullBodyBatchBuilder
    ds = UvitonDatasetFull(tree, mirror_people=True)
    flags = (0, 1, 1, 0, 1)
    samples = [ds[i + 5 * f] for i, f in enumerate(flags)]
    assert [s['xflip'] for s in samples] == list(flags) and [s['raw_idx'] for s in samples] == [0, 1, 2, 3, 4]
    rng = np.random.default_rng(7)
    samples[2]['erase_mask'] = (rng.uniform(size=[77, 131]) < 0.3).astype(np.uint8) * np.uint8(255)
    samples[4]['erase_mask'] = rng.integers(0, 256, [256, 192], dtype=np.uint8)
    builder = FullBodyBatchBuilder('cuda')
    got = builder.build(collate(samples), keep_stages=True)
    host = [MR.mirror_raw(s) if s['xflip'] else {k: v for k, v in s.items() if k != 'xflip'} for s in samples]
    assert all('xflip' not in s for s in host)
    want = builder.build(collate(host), keep_stages=True)
    _equal_batches(got, want)
    assert torch.equal(got.image.cpu(), torch.from_numpy(np.stack([s['image'] for s in host])))
    plain = builder.build(collate([{k: v for k, v in s.items() if k != 'xflip'} for s in samples]), keep_stages=True)
    _equal_batches(got, plain, items=[0, 3])
    for k in ('real_img', 'pose', 'gt_parsing', 'style_input'):
        assert not torch.equal(got.tensors[k][1], plain.tensors[k][1]), k
    # flags all 0: the plain build, bit for bit
    zeros = collate([dict(s, xflip=0) for s in samples])
    assert zeros['xflip'].tolist() == [0] * 5
    _equal_batches(builder.build(zeros, keep_stages=True), plain)


# ---- the builder at 512 x 320 ----

def test_builder_512_mixed_flags_equal_the_restatement_on_mirrored_samples(tmp_path_factory):
    """The three listed people of the 512 tree (the folded arm, the missing wrist and ankle, the elbow far outside) with erase
    masks of three sizes, flags (1, 0, 1): the nine tensors equal the unchanged restatement evaluated on mirrored raw samples."""
    from training.dataset import UvitonDatasetFull_512, collate
    from training.tryon_batch import FullBodyBatch
    from training.tryon_regions import FullBodyRegionBatchBuilder
    tree = make_512_train_tree(tmp_path_factory.mktemp('mirror_gpu_512'))
    ds = UvitonDatasetFull_512(tree, mirror_people=True)
    flags = (1, 0, 1)
    samples = [ds[i + 5 * f] for i, f in zip(ds.vis_index, flags)]
    for s, m in zip(samples, erase_masks()):
        s['erase_mask'] = m
    assert [s['xflip'] for s in samples] == list(flags)
    got = FullBodyRegionBatchBuilder('cuda').build(collate(samples))
    host = [MR.mirror_raw(s) if s['xflip'] else s for s in samples]
    stages = [TR.person_training_stages(s) for s in host]
    want = TR.training_tensors(stages, [s['erase_mask'] for s in host], 'cuda')
    for k in FullBodyBatch.KEYS:
        g, v = got.tensors[k], want[k]
        assert g.dtype == torch.float32 and g.shape == v.shape and torch.equal(g, v), (k, int((g != v).sum()))
    assert torch.equal(got.image.cpu(), torch.from_numpy(np.stack([s['image'] for s in host])))
    assert got.tensors['denorm_upper_mask'].any() and got.tensors['denorm_lower_mask'].any()


# ---- the loop ----

def test_training_loop_on_mirrored_people(tree):
    """Four iterations of batch 2 on the mirrored tiny tree.  With the default seed 0 the first four raw batches of the loop's own
    loader hold both flag values (checked here on a second loader built the same way)."""
    from torch_utils import misc
    from training.dataset import UvitonDatasetFull, collate
    from training.training_loop_wo_flow_fullbody import fashion_config, training_loop
    ds = UvitonDatasetFull(tree, mirror_people=True)
    loader = iter(torch.utils.data.DataLoader(dataset=ds, sampler=misc.InfiniteSampler(dataset=ds, rank=0, num_replicas=1, seed=0), batch_size=2,
                                              collate_fn=collate, num_workers=0))
    seen = torch.cat([next(loader)['xflip'] for _ in range(4)]).tolist()
    assert 0 in seen and 1 in seen, seen
    log = []
    cfg = fashion_config(channel_base=2048, mbstd_group_size=2)
    cfg.loss_kwargs = dict(cfg.loss_kwargs, report_fn=lambda name, value: log.append((name, value)))
    step = training_loop(batch_size=2, batch_gpu=2, total_iters=4, cfg=cfg, device=torch.device('cuda'),
                         training_set_kwargs=dict(class_name='training.dataset.UvitonDatasetFull', path=tree, mirror_people=True),
                         data_loader_kwargs=dict(num_workers=0, pin_memory=True))
    assert step.cur_nimg == 8
    losses = [(k, v) for k, v in log if k.startswith('Loss/')]
    assert losses and all(torch.isfinite(torch.as_tensor(v).float()).all() for _, v in losses), sorted({k for k, _ in losses})
    assert all(torch.isfinite(p).all() for p in step.G.parameters())
