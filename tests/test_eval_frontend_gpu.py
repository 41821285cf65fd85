"""-m gpu: ``ops.surface_distances`` after its table and counts became two views of one packed buffer (``kernels.surface_layout``) that
one copy brings to the host - the only op whose copy path changed when the packed tables got one layout each.

16 x 16 masks, B = 1 and B = 3 (the counts then start at word 12 and at word 36 of the buffer), with an empty plane, a full plane and a
pair of single pixels in the first image.  Against tests/surface_ref.py by the criterion of tests/test_surface_gpu.py: the integers (n,
the max squared distance, the Dice counts) exactly, the NaN pattern exactly, the sum of distances s within (n + 2) * 2^-52 * s_ref - one
ulp per square root plus the (n - 1) * 2^-53 * sum bound of any summation order.  Two calls in a row give identical arrays."""
import numpy as np
import pytest
import torch

import surface_ref as sr
from uda_clr_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52
S = 16


def _masks(B, kind):
    """bool pred, gt [B,2,16,16]: ellipses, and in image 0 the special planes of ``kind``"""
    rng = np.random.default_rng(B)
    pred, gt = np.zeros((B, 2, S, S), bool), np.zeros((B, 2, S, S), bool)
    for b in range(B):
        for c, r in enumerate((3.0, 6.0)):
            pred[b, c] = sr.ellipse(S, S, 8 + rng.uniform(-1, 1), 8 + rng.uniform(-1, 1), r, r + rng.uniform(0, 1.5))
            gt[b, c] = sr.ellipse(S, S, 8 + rng.uniform(-1, 1), 8 + rng.uniform(-1, 1), r + rng.uniform(0, 1.5), r)
    if kind == "empty":
        pred[0, 0] = False                                                    # no predicted cup: NaN sums, -1 maxima, n of the truth kept
    elif kind == "full":
        pred[0, 1] = True                                                     # the disc everywhere: its border is the image's frame
    else:
        pred[0, 0], gt[0, 0] = False, False
        pred[0, 0, 2, 3], gt[0, 0, 13, 11] = True, True                       # one pixel each: n = 1, s = sqrt(11^2 + 8^2) both ways
    return pred, gt


@pytest.mark.parametrize("kind", ["empty", "full", "single"])
@pytest.mark.parametrize("B", [1, 3])
def test_surface_distances_through_the_packed_buffer(B, kind):
    pred, gt = _masks(B, kind)
    table, counts = ops.surface_distances(torch.from_numpy(pred), torch.from_numpy(gt).to(DEV))
    rt, rc = sr.surface_distances(pred, gt)
    assert table.dtype == np.float64 and table.shape == (B, 2, 2, 3) and counts.dtype == np.int64 and counts.shape == (B, 2, 3)
    assert np.array_equal(counts, rc)
    assert np.array_equal(table[..., 0], rt[..., 0]) and np.array_equal(table[..., 2], rt[..., 2])
    s, s_ref, n = table[..., 1], rt[..., 1], rt[..., 0]
    assert np.array_equal(np.isnan(s), np.isnan(s_ref))
    ok = ~np.isnan(s_ref)
    err, bound = np.abs(s - s_ref)[ok], ((n + 2) * EPS * s_ref)[ok]
    print("s: worst error / bound = %.3f over %d entries" % (float((err / np.maximum(bound, 1e-300)).max()), int(ok.sum())))
    assert (err <= bound).all(), (err, bound)
    if kind == "empty":
        assert np.isnan(table[0, 0, :, 1]).all() and (table[0, 0, :, 2] == -1).all() and table[0, 0, 0, 0] == 0 and table[0, 0, 1, 0] > 0
    elif kind == "full":
        assert counts[0, 1, 1] == S * S and table[0, 1, 0, 0] == 4 * S - 4
    else:
        assert (table[0, 0, :, 0] == 1).all() and (table[0, 0, :, 2] == 185).all() and counts[0, 0].tolist() == [0, 1, 1]
    again = ops.surface_distances(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    assert np.array_equal(again[0], table, equal_nan=True) and np.array_equal(again[1], counts)
    assert again[0].tobytes() == table.tobytes()
