"""The rounding-aware reference helper (tests/storage_ref.py) bites on synthetic data: a truncating bf16 store, a sum that
drops one planted term, and correct round-to-nearest-even data that must pass."""

import numpy as np
import pytest
import torch

import storage_ref as S


def _data(n=1 << 14, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn([n], generator=gen, dtype=torch.float64) * 3


def _truncate_bf16(x64):
    """fp64 -> fp32 -> bf16 by dropping the low 16 bits (a truncating store)."""
    b = x64.float().view(torch.int32) & -65536
    return b.view(torch.float32).double()


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16, torch.float32])
def test_ulp_and_rne_match_torch_where_torch_rounds_once(dtype):
    x = _data()
    # from fp32 data torch rounds once to fp16 / bf16 (RNE); the helper must agree bit for bit
    x32 = x.float()
    assert np.array_equal(S.rne(x32.double(), dtype), x32.to(dtype).double().numpy())
    nxt = torch.nextafter(x32.to(dtype).float() if dtype != torch.float32 else x32, torch.tensor(float('inf')))
    if dtype == torch.float32:
        sp = (nxt.double() - x32.double()).abs().numpy()
        assert np.array_equal(S.ulp(x32.double(), dtype)[x32.numpy() > 0], sp[x32.numpy() > 0])
    assert S.ulp(np.array([0.0]), torch.float16)[0] == 2.0 ** -24
    assert S.ulp(np.array([1.0]), torch.bfloat16)[0] == 2.0 ** -7
    assert S.ulp(np.array([0.75]), torch.float16)[0] == 2.0 ** -11


def test_rne_rounds_once_from_fp64():
    # 1 + 2^-8 + 2^-30: fp64 -> bf16 directly is 1 + 2^-7 (above the tie); through fp32 (torch's conversion) the 2^-30 is lost
    # first and the tie goes to even, 1.0.  The helper must give the single rounding.
    v = np.array([1 + 2.0 ** -8 + 2.0 ** -30])
    assert S.rne(v, torch.bfloat16)[0] == 1 + 2.0 ** -7
    assert float(torch.from_numpy(v).to(torch.bfloat16)) == 1.0


def test_correct_rne_storage_passes():
    ref = _data()
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        got = torch.from_numpy(S.rne(ref, dtype))
        S.assert_stored(got, ref, dtype, ref.abs(), what=str(dtype))
    # an fp32 evaluation error of a few ulps of fp32 stays inside the bound and almost never moves the 16-bit result
    jitter = ref * (1 + 3 * S.U32 * torch.sign(torch.randn(ref.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)))
    S.assert_stored(torch.from_numpy(S.rne(jitter, torch.bfloat16)), ref, torch.bfloat16, ref.abs())


def test_truncating_bf16_store_fails():
    ref = _data()
    with pytest.raises(AssertionError):
        S.assert_stored(_truncate_bf16(ref), ref, torch.bfloat16, ref.abs())


def test_double_rounding_fails_the_bitwise_check():
    # values above a bf16 tie by less than an fp32 ulp: once-rounded they go up; through fp32 they land on the tie, which goes to
    # even, i.e. down for half of them
    gen = torch.Generator().manual_seed(2)
    base = torch.from_numpy(S.rne(_data(), torch.bfloat16))
    ref = base + torch.from_numpy(S.ulp(base, torch.bfloat16)) * (0.5 + 2.0 ** -20 * torch.rand(base.shape, generator=gen, dtype=torch.float64))
    twice = ref.float().to(torch.bfloat16).double()
    with pytest.raises(AssertionError):
        S.assert_stored(twice, ref, torch.bfloat16, ref.abs(), k=0)


def test_one_dropped_planted_term_fails_the_reduction_bound():
    terms = _data(1 << 14)
    terms[-1] = 1000.0                                  # planted in the last element
    ref = terms.sum().reshape(1)
    scale = terms.abs().sum().reshape(1)
    ok = terms.float().sum().double().reshape(1)
    S.assert_reduced(ok, ref, scale, terms.numel())
    dropped = terms[:-1].float().sum().double().reshape(1)
    with pytest.raises(AssertionError):
        S.assert_reduced(dropped, ref, scale, terms.numel())


def test_a_lost_element_fails_the_storage_bound():
    ref = _data()
    got = torch.from_numpy(S.rne(ref, torch.float32))
    got[-1] = 0.0
    with pytest.raises(AssertionError):
        S.assert_stored(got, ref, torch.float32, ref.abs())
