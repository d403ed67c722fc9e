"""The one device-resident form of the body-part maps on the GPU: ``part_maps`` under 'host' against
``host_part_maps`` and, with the host's solve replaced by the restatement, against 'gpu', bit for bit; how often a build inverts;
and the launch wrappers handed host matrices against the same wrappers handed the converted device form."""
import numpy as np
import pytest
import torch

import part_geometry_ref as ref
from test_part_geometry_gpu import _builds

pytestmark = pytest.mark.gpu

SIZE = 256


def _edge_five():
    """tests/test_part_geometry_gpu.py's case: N = 3 samples over M = 5 edge people who miss parts the others have."""
    edge, names = ref.edge_people(SIZE)
    people = edge[[names.index(k) for k in ('complete', 'no left knee', 'no shoulders, no hips', 'no left ankle', 'zero-length right forearm')]]
    return people, [0, 3, 1], [2, 0, 4], [1, 1, 3]


def _equal(got, want, what):
    """Bit for bit: a tensor against a numpy array or another tensor."""
    got = got.cpu()
    want = want.cpu() if isinstance(want, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(want))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    as_bytes = lambda t: t.contiguous().view(torch.uint8)
    assert torch.equal(as_bytes(got), as_bytes(want)), what


@pytest.mark.parametrize('x_pad,shin', [(0, True), (32, False)])
def test_host_part_maps_uploaded_is_host_part_maps(x_pad, shin):
    from training import patch_pipeline as P
    people = _edge_five()[0]
    want = P.host_part_maps(people, SIZE, SIZE, 2, x_pad, shin)
    got = P.part_maps(people, SIZE, SIZE, 2, x_pad, shin, 'cuda', 'host')
    assert type(got) is P.PartMaps
    for name in ('fwd_inv', 'back_inv', 'valid'):
        assert getattr(got, name).is_cuda, name
        _equal(getattr(got, name), getattr(want, name), name)
    assert not got.m_invs.is_cuda and isinstance(got.flags, np.ndarray) and got.flags.dtype == bool
    _equal(got.m_invs, want.m_invs, 'm_invs')
    assert np.array_equal(got.flags, want.flags) and want.flags.any() and not want.flags.all()


@pytest.mark.parametrize('x_pad,shin', [(0, True), (32, False)])
def test_host_and_gpu_part_maps_agree_under_the_restated_solve(x_pad, shin, monkeypatch):
    from training import patch_pipeline as P
    monkeypatch.setattr(P, 'part_matrices', ref.part_matrices)
    people = _edge_five()[0]
    host, gpu = (P.part_maps(people, SIZE, SIZE, 2, x_pad, shin, 'cuda', geometry) for geometry in ('host', 'gpu'))
    assert gpu.m_invs.is_cuda and not host.m_invs.is_cuda
    for name in ('fwd_inv', 'back_inv', 'valid', 'm_invs'):
        _equal(getattr(gpu, name), getattr(host, name), name)
    assert gpu.flags.dtype == bool and np.array_equal(gpu.flags, host.flags)


@pytest.fixture(scope='module')
def builds(tmp_path_factory):
    return _builds(tmp_path_factory.mktemp('part_maps_builders'))


@pytest.mark.parametrize('which', range(5))
def test_a_build_inverts_twice_under_host_and_never_under_gpu(builds, which, monkeypatch):
    """Once for the forward maps and once for the back maps of all the people, whatever the number of launches, the swapped pass
    included where the case has one."""
    from training import patch_pipeline
    name, cls, args, raw, kwargs = builds[which]
    calls = []
    real = patch_pipeline.adjugate_inverse
    monkeypatch.setattr(patch_pipeline, 'adjugate_inverse', lambda m: (calls.append(np.shape(m)), real(m))[1])
    cls('cuda', *args).build(raw, **kwargs)
    assert len(calls) == 2 and calls[0] == calls[1] and calls[0][1:] == (10, 3, 3), (name, calls)
    del calls[:]
    cls('cuda', *args, geometry='gpu').build(raw, **kwargs)
    assert calls == [], (name, calls)


def test_the_launch_wrappers_take_host_matrices_and_the_device_form_alike():
    from training import patch_pipeline as P
    rng = np.random.default_rng(11)
    people, person, upper, _ = _edge_five()
    fwd, back, flags = P.part_matrices(people, SIZE, SIZE, x_pad=0, shin_fallback=True)
    maps = P.part_maps(people, SIZE, SIZE, 2, 0, True, 'cuda', 'host')
    images = torch.from_numpy(rng.integers(0, 256, [5, SIZE, SIZE, 3], dtype=np.uint8)).cuda()

    # ten parts of three owners: host matrices, index and flags against the gathered device rows
    items = (np.asarray(upper)[:, None] * 10 + np.arange(10)).reshape(-1)
    index = np.repeat(np.asarray(upper, np.int32), 10)
    items_t = torch.from_numpy(items).cuda()
    by_host = P.warp_perspective(images, fwd.reshape(-1, 3, 3)[items], (64, 64), 'replicate', index, flags.reshape(-1)[items])
    by_device = P.warp_perspective(images, maps.fwd_inv.reshape(-1, 9).index_select(0, items_t), (64, 64), 'replicate',
                                   torch.from_numpy(index).cuda(), maps.valid.reshape(-1).index_select(0, items_t))
    assert by_host.shape == (30, 64, 64, 3) and torch.equal(by_host, by_device) and by_host.any()
    valid_items = torch.from_numpy(flags.reshape(-1)[items])
    assert not valid_items.all() and not by_host[~valid_items].any()            # a missing part is zeros either way

    patches = by_host.reshape(3, 10, 64, 64, 3)
    masks = torch.from_numpy(np.where(rng.uniform(size=[3, 10, 32, 32, 1]) < 0.85, 255, 0).astype(np.uint8).repeat(2, 2).repeat(2, 3).repeat(3, 4)).cuda()
    person_t = torch.from_numpy(np.asarray(person)).cuda()
    for parts, radius in ((list(range(10)), None), ([0, 6, 7, 8, 9], 2), ([6, 7, 8, 9], [0, 2, 1])):
        args = (patches[:, parts], masks[:, parts])
        want = P.composite(*args, back[person], flags[person], parts, SIZE, SIZE, radius, want_part_masks=True)
        got = P.composite(*args, maps.back_inv.index_select(0, person_t), maps.valid.index_select(0, person_t), parts, SIZE, SIZE, radius,
                          want_part_masks=True)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and want[0].any() and want[1].any(), (parts, radius)
