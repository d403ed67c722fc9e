"""The one form of the body-part maps without a GPU: the batched ``patch_pipeline.adjugate_inverse`` against the
per-matrix expressions it replaced, restated here, and ``host_part_maps`` against ``part_matrices`` plus those per-matrix
inverses and against tests/part_geometry_ref.py's ``geometry`` -- all bit for bit."""
import numpy as np
import pytest

import part_geometry_ref as ref
from training import patch_pipeline

CASES = [(256, 32, False), (256, 0, True), (512, 0, False), (512, 32, True)]       # size, x_pad, shin_fallback


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    differing = np.argwhere(_bits(got) != _bits(want))
    assert len(differing) == 0, (what, len(differing), differing[:4].tolist())


def _one_inverse(m):
    """adjugate_inverse as it was, one 3 x 3 matrix at a time."""
    with np.errstate(all='ignore'):                # the hand matrices overflow on purpose
        m = np.asarray(m, np.float64)
        c = np.empty([3, 3])
        c[0, 0] = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]; c[0, 1] = m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2]; c[0, 2] = m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]
        c[1, 0] = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]; c[1, 1] = m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0]; c[1, 2] = m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]
        c[2, 0] = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]; c[2, 1] = m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1]; c[2, 2] = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
        det = (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]) +
               m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
        return c * (1.0 / det) if det != 0 else np.zeros([3, 3])


def _each_inverse(mats):
    return np.stack([_one_inverse(m) for m in mats.reshape(-1, 3, 3)]).reshape(mats.shape)


def _people(size):
    return np.concatenate([ref.edge_people(size)[0], ref.standing_people(40, size, seed=size)])


@pytest.mark.parametrize('size', [256, 512])
@pytest.mark.parametrize('solver', ['lapack', 'restated'])
def test_the_batched_inverse_is_the_per_matrix_one_bit_for_bit(size, solver):
    solve = patch_pipeline.part_matrices if solver == 'lapack' else ref.part_matrices
    fwd, back, valid = solve(_people(size), size, size, x_pad=0)
    assert valid.any(axis=0).all() and not valid.all(axis=0).any()          # present and missing parts (zeros) alike
    for name, mats in (('fwd', fwd), ('back', back)):
        got = patch_pipeline.adjugate_inverse(mats)
        _same(got, _each_inverse(mats), (solver, size, name))
        assert got.flags['C_CONTIGUOUS']
        _same(patch_pipeline.adjugate_inverse(mats[3, 2]), _one_inverse(mats[3, 2]), (solver, size, name, 'one matrix'))
    parts = [0, 6, 7, 8, 9]
    want = np.stack([_one_inverse(back[i, k]) for i in range(len(back)) for k in parts]).reshape(-1, 9)
    _same(patch_pipeline.inverse_maps(back, parts), want, 'inverse_maps')


def test_the_batched_inverse_on_singular_and_non_finite_matrices():
    hand = np.array([[[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [1.0, 0.0, 1.0]],                       # det == 0 with non-zero entries
                     [[1.0, np.nan, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],                     # a NaN
                     [[np.inf, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]],                     # an inf
                     [[1e200, 0.0, 0.0], [0.0, 1e200, 0.0], [0.0, 0.0, 1.0]]])                   # an overflow to inf
    got = patch_pipeline.adjugate_inverse(hand)
    _same(got, _each_inverse(hand), 'hand matrices')
    assert not got[0].any() and np.isnan(got[1]).any() and np.isnan(got[2]).any() and not got[3, :2, :2].any()
    _same(patch_pipeline.adjugate_inverse(hand.reshape(2, 2, 3, 3)), got.reshape(2, 2, 3, 3), 'two leading axes')


@pytest.mark.parametrize('size,x_pad,shin', CASES)
def test_host_part_maps_is_part_matrices_and_its_inverses(size, x_pad, shin):
    people = _people(size)
    fwd, back, valid = patch_pipeline.part_matrices(people, size, size, 2, x_pad, shin)
    got = patch_pipeline.host_part_maps(people, size, size, 2, x_pad, shin)
    assert type(got) is patch_pipeline.PartMaps and got._fields == ('fwd_inv', 'back_inv', 'valid', 'm_invs', 'flags')
    m = len(people)
    _same(got.fwd_inv, _each_inverse(fwd).reshape(m, 10, 9), 'fwd_inv')
    _same(got.back_inv, _each_inverse(back).reshape(m, 10, 9), 'back_inv')
    _same(got.valid, valid.astype(np.uint8), 'valid')
    _same(got.m_invs, np.where(valid[..., None, None], back, 0).astype(np.float32), 'm_invs')
    _same(got.flags, patch_pipeline.part_valid(people, shin), 'flags')
    assert got.flags.dtype == bool and np.array_equal(got.flags, valid)
    missing = ~valid
    assert missing.any() and not got.fwd_inv[missing].any() and not got.back_inv[missing].any() and not got.m_invs[missing].any()


@pytest.mark.parametrize('size,x_pad,shin', CASES)
def test_host_part_maps_under_the_restated_solve_is_the_kernels_rule(size, x_pad, shin, monkeypatch):
    people = _people(size)
    monkeypatch.setattr(patch_pipeline, 'part_matrices', ref.part_matrices)         # looked up when called
    got = patch_pipeline.host_part_maps(people, size, size, 2, x_pad, shin)
    want = ref.geometry(people, size, size // 4, size // 4, x_pad, shin)
    _same(got.fwd_inv, want['fwd_inv'], 'fwd_inv')
    _same(got.back_inv, want['back_inv'], 'back_inv')
    _same(got.m_invs, want['m_inv'].reshape(-1, 10, 3, 3), 'm_inv')
    _same(got.valid, want['valid'], 'valid')
    flags = want['valid'].astype(bool)
    assert (want['fwd'][flags][:, :8] == 0).all(axis=1).any()                       # a valid part whose forward system is singular
    assert not got.fwd_inv[flags][(want['fwd'][flags][:, :8] == 0).all(axis=1)].any()
