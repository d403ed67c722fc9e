"""pasta_recon_image_stats keeps its bits: the sums and the fp64 SSIM sums of fixed inputs, recorded from the library as it stood
before pasta_region_image_stats joined its kernel template (tests/golden/recon_image_stats_bits.npz), must come back equal.
The SSIM sum is fp32 arithmetic whose rounding depends on what the compiler fuses; this holds it still."""
import os

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'recon_image_stats_bits.npz')
CASES = [(2, 37, 23, 40, 'random'), (2, 64, 48, 64, 'near'), (3, 33, 43, 50, 'constant'), (1, 256, 192, 256, 'near'), (2, 11, 11, 11, 'random')]


def case_inputs(n, h, w, wt, kind):
    """Seeded inputs of one case: (images fp32 [n, 3, h, wt], photos uint8 [n, h, w, 3], c0)."""
    rng = np.random.default_rng(1000 * h + w + n)
    c0 = (wt - w) // 2
    x = rng.uniform(-1.2, 1.2, [n, 3, h, wt]).astype(np.float32)
    p = rng.integers(0, 256, [n, h, w, 3], dtype=np.uint8)
    if kind == 'near':
        x[..., c0:c0 + w] = ((p.transpose(0, 3, 1, 2) + rng.normal(0, 6, [n, 3, h, w])) / 127.5 - 1).astype(np.float32)
    if kind == 'constant':
        for i in range(n):
            x[i] = np.float32([-1.0, 0.25, -0.4][i % 3])
            p[i] = [255, 17, 128][i % 3]
    return x, p, c0


def compute(case):
    from metrics.metric_utils import recon_image_stats
    x, p, c0 = case_inputs(*case)
    sums, ssim = recon_image_stats(torch.from_numpy(x).cuda(), torch.from_numpy(p).cuda(), c0)
    return sums.cpu().numpy(), ssim.cpu().numpy().view(np.int64)


@pytest.mark.parametrize('case', CASES, ids=lambda c: '%dx%d-%s' % (c[1], c[2], c[4]))
def test_recon_image_stats_returns_the_recorded_bits(case):
    golden = np.load(GOLDEN)
    key = '%d_%d_%d_%d_%s' % case
    sums, bits = compute(case)
    assert np.array_equal(sums, golden[key + '_sums'])
    assert np.array_equal(bits, golden[key + '_ssim']), (bits.view(np.float64), golden[key + '_ssim'].view(np.float64))
