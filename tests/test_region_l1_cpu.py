"""The region L1 term and the swapped-outfit tables without a GPU: the fp64 reference's closed-form gradient against
autograd, the priority rule, the declarations and host guards of the four new entries, and the donor rule."""
import os
import re

import numpy as np
import pytest
import torch

import region_l1_ref as R


# ---- the reference ----

@pytest.mark.parametrize('shape', R.CASES)
def test_closed_form_gradient_equals_autograd_in_fp64(shape):
    K, N, H = shape
    g = np.arange(1, 3 * K + 1, dtype=np.float64).reshape(K, 3) * 0.37 - 1.0
    for content in R.CONTENTS:
        case = R.make_case(shape, content)
        images = [torch.from_numpy(x).double().requires_grad_(True) for x in case[0]]
        out = R.values_torch(images, *case[1:])
        assert np.abs(out.detach().numpy() - R.values(*case)).max() <= 1e-14, content
        grads = torch.autograd.grad((out * torch.from_numpy(g)).sum(), images)
        for got, want in zip(grads, R.gradients(*case, g)):
            # |.|'s derivative at 0 is 0 in torch, as in the definition
            assert np.abs(got.numpy() - want).max() <= 1e-15, content
        region = R.regions(*case[4:])
        if content == 'none':
            assert (region == -1).all() and not out.detach().numpy().any()
        if content == 'equal':
            assert any(((x == t) & (region == r)[:, None]).any() for x in case[0] for r, t in enumerate(case[1:4]))


def test_the_priority_rule_where_all_three_masks_overlap():
    case = R.make_case((2, 2, 12), 'overlap')
    images, retain, upper, lower, keep, um, lm = case
    assert keep.all() and um.all() and lm.all() and (R.regions(keep, um, lm) == 0).all()
    out = R.values(*case)
    assert not out[:, 1:].any()                 # everything is keep's
    for k, x in enumerate(images):
        assert out[k, 0] == pytest.approx(np.abs(x.astype(np.float64) - retain).mean(), rel=1e-14)      # F.l1_loss against retain
    # taking keep away hands every pixel to the upper region, then to the lower one
    nobody = np.zeros_like(keep)
    assert (R.regions(nobody, um, lm) == 1).all() and (R.regions(nobody, np.zeros_like(um), lm) == 2).all()
    out = R.values(images, retain, upper, lower, nobody, um, lm)
    assert not out[:, 0].any() and not out[:, 2].any() and out[:, 1].all()
    # and the three regions partition what F.l1_loss sums
    blobs = R.make_case((1, 2, 12), 'blobs')
    region = R.regions(*blobs[4:])
    assert set(np.unique(region)) == {-1, 0, 1, 2}
    total = sum(np.abs(blobs[0][0].astype(np.float64) - t)[np.broadcast_to((region == r)[:, None], t.shape)].sum()
                for r, t in enumerate(blobs[1:4])) / blobs[0][0].size
    assert R.values(*blobs).sum() == pytest.approx(total, rel=1e-13)


# ---- the entries ----

ENTRIES = (('pasta_region_l1_loss_workspace', 'int64_t', 2), ('pasta_region_l1_loss', 'int', 15), ('pasta_region_l1_loss_backward', 'int', 7),
           ('pasta_swap_assemble', 'int', 15))


def test_the_entries_are_declared_typed_and_late():
    from conftest import ROOT
    from torch_utils import custom_ops
    header = open(os.path.join(ROOT, 'include', 'pasta_hip.h')).read()
    lib = custom_ops.get_plugin()
    for name, kind, args in ENTRIES:
        assert re.search(r'\b%s %s\(' % (kind, name), header), name
        assert name in custom_ops.ABI and len(custom_ops.ABI[name][1]) == args and name in custom_ops.LATE_ENTRIES, name
        assert custom_ops.has_entry(lib, name), name
    assert lib.pasta_abi_version() == custom_ops.EXPECTED_ABI == 22
    # pasta_grid_assemble keeps its signature
    assert len(custom_ops.ABI['pasta_grid_assemble'][1]) == 17


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """Pointers are the never-dereferenced value 1 (the pointer arrays hold it too): every call is refused with the entry's own text
    before anything is launched."""
    import ctypes
    from torch_utils import custom_ops
    lib = custom_ops.get_plugin()

    def refused(status, text):
        assert status != 0 and text in lib.pasta_last_error(), lib.pasta_last_error()

    ones = lambda n: (ctypes.c_void_p * n)(*[1] * n)
    assert lib.pasta_region_l1_loss_workspace(2, 10) == 0 and lib.pasta_region_l1_loss_workspace(0, 8) == 0
    assert lib.pasta_region_l1_loss_workspace(2, 4100) == 0
    assert lib.pasta_region_l1_loss_workspace(2, 64) == 2 * 4 * 12 * 8          # four workgroups per image, twelve fp64 slots each
    need = lib.pasta_region_l1_loss_workspace(2, 12)
    forward = lambda images=ones(4), t=1, out=1, work=1, nbytes=need, K=2, N=2, H=12: \
        lib.pasta_region_l1_loss(images, t, 1, 1, 1, 1, 1, out, ones(4), work, nbytes, K, N, H, None)
    backward = lambda maps=ones(4), g=1, dx=ones(4), K=2, N=2, H=12: lib.pasta_region_l1_loss_backward(maps, g, dx, K, N, H, None)
    for null in ('images', 't', 'out', 'work'):
        refused(forward(**{null: None}), b'region_l1_loss: null pointer')
    for null in ('maps', 'g', 'dx'):
        refused(backward(**{null: None}), b'region_l1_loss_backward: null pointer')
    refused(forward(K=0), b'region_l1_loss: 0 images (1..4)')
    refused(forward(K=5), b'region_l1_loss: 5 images (1..4)')
    refused(backward(K=5), b'region_l1_loss_backward: 5 images (1..4)')
    refused(forward(H=10, nbytes=1 << 30), b'region_l1_loss: bad shape (N 2, H 10: H a multiple of 4)')
    refused(backward(H=10), b'region_l1_loss_backward: bad shape (N 2, H 10: H a multiple of 4)')
    refused(forward(N=65536, nbytes=1 << 40), b'bad shape')
    refused(forward(nbytes=need - 1), b'region_l1_loss: workspace of %d bytes, %d needed' % (need - 1, need))
    holes = (ctypes.c_void_p * 4)(1, None, 1, 1)
    refused(forward(images=holes), b'region_l1_loss: image 1 is null')
    refused(backward(dx=holes), b'region_l1_loss_backward: map or gradient 1 is null')

    swap = lambda den=1, src=1, outs=ones(5), n=3, T=3, H=16, pw=4: lib.pasta_swap_assemble(den, 1, 1, 1, src, 1, outs, n, T, H, 4, pw, 30, 12, None)
    refused(swap(den=None), b'swap_assemble: null pointer')
    refused(swap(src=None), b'swap_assemble: null pointer')
    refused(swap(outs=None), b'swap_assemble: null pointer')
    refused(swap(n=0), b'swap_assemble: 0 samples of 3 people')
    refused(swap(H=18), b'swap_assemble: bad shape (H and pw multiples of 4)')
    refused(swap(pw=6), b'swap_assemble: bad shape')
    refused(swap(outs=(ctypes.c_void_p * 5)(1, 1, None, 1, 1)), b'swap_assemble: output 2 is null')


def test_the_op_refuses_cpu_tensors():
    from torch_utils.ops.region_l1_loss import region_l1_loss
    case = R.make_case((1, 1, 4), 'blobs')
    tensors = [torch.from_numpy(a) for a in case[1:]]
    with pytest.raises(RuntimeError, match='needs a GPU tensor'):
        region_l1_loss([torch.from_numpy(case[0][0])], *tensors)


# ---- the donor rule ----

@pytest.mark.parametrize('b', [2, 3, 4])
def test_the_donor_rule_and_the_region_tables(b):
    from training import swap_outfits as S
    for groups in (1, 2):
        n = groups * b
        donor = S.donors(n, b)
        assert donor.tolist() == R.donors(n, b)
        own = np.arange(n)
        assert (donor != own).all() and (donor // b == own // b).all()              # a batch-mate of the same round
        assert sorted(donor.tolist()) == own.tolist()                               # a roll: everybody gives once
        for region, want in (('fullbody', (donor, donor)), ('upperbody', (donor, own)), ('lowerbody', (own, donor))):
            upper_src, lower_src = S.source_tables(n, b, region)
            assert upper_src.tolist() == want[0].tolist() and lower_src.tolist() == want[1].tolist(), region
    assert S.donors(4, 2).tolist() == [1, 0, 3, 2] and S.donors(6, 3).tolist() == [1, 2, 0, 4, 5, 3] and S.donors(4, 4).tolist() == [1, 2, 3, 0]
    with pytest.raises(ValueError, match='at least 2'):
        S.donors(4, 1)
    with pytest.raises(ValueError, match='divide the batch'):
        S.donors(5, 2)
    with pytest.raises(ValueError, match='swap region'):
        S.source_tables(4, 2, 'hat')
