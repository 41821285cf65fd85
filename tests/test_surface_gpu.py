"""-m gpu: uda_surface_distance (csrc/surface.hip) against the scipy oracle (tests/surface_ref.py), its determinism and argument
checks, and evaluate() on the device against the stepwise scipy chain.

Integers (the squared distance maps, n, the max, the Dice counts) are compared exactly.  The sum of distances s is compared
within (n + 2) * 2^-52 * s_ref: one ulp per square root, plus the (n - 1) * 2^-53 * sum bound that holds for ANY order of
summing n non-negative terms (the oracle's fsum rounds once).  The bound is derived, not measured."""
import math

import numpy as np
import pytest
import torch

import surface_ref as sr
from kernel_cases import _scipy_postprocess
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops
from uda_clr_amd.utils import metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
EPS = 2.0 ** -52


def _run(pred, gt, want_d2=True):
    out = ops.kernels().surface_distance(torch.from_numpy(pred.astype(np.uint8)).to(DEV), torch.from_numpy(gt.astype(np.uint8)).to(DEV), want_d2)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check_against_oracle(pred, gt):
    table, counts, d2 = _run(pred, gt)
    rt, rc, rd = sr.reference(pred, gt)
    assert d2.dtype == np.int32 and np.array_equal(d2, rd), "squared distance maps differ in %d pixels" % int((d2 != rd).sum())
    assert np.array_equal(counts, rc)
    assert np.array_equal(table[..., 0], rt[..., 0]) and np.array_equal(table[..., 2], rt[..., 2])
    s, s_ref, n = table[..., 1], rt[..., 1], rt[..., 0]
    assert np.array_equal(np.isnan(s), np.isnan(s_ref))
    ok = ~np.isnan(s_ref)
    err, bound = np.abs(s - s_ref)[ok], ((n + 2) * EPS * s_ref)[ok]
    print("s: worst error / bound = %.3f over %d entries" % (float((err / np.maximum(bound, 1e-300)).max()), int(ok.sum())))
    assert (err <= bound).all(), (err, bound)
    return table, counts


def test_special_masks_96x80():
    """non-square, W no multiple of 64 or 16, H none of 32 or 128: every kind of mask the border rule has a corner case for"""
    _check_against_oracle(*sr.special_96x80())


@pytest.mark.parametrize("B,H,W", [(1, 33, 17), (2, 512, 512), (1, 1024, 40)], ids=["33x17", "512x512", "1024x40"])
def test_ellipses_against_oracle(B, H, W):
    """one partial strip and one partial row block; the workload's column length; the longest supported column"""
    _check_against_oracle(*sr.random_pairs(100 + H, B, H, W))


def test_empty_sets_follow_the_nan_convention():
    pred, gt = sr.empty_96x80()
    table, counts = _check_against_oracle(pred, gt)
    assert np.isnan(table[:, 0, :, 1]).all() and (table[:, 0, :, 2] == -1).all()
    assert table[0, 0, 0, 0] == 0 and table[0, 0, 1, 0] > 0 and table[1, 0, 0, 0] > 0 and table[1, 0, 1, 0] == 0 and (table[2, 0, :, 0] == 0).all()
    assert np.isfinite(table[:, 1]).all()
    got = metrics.surface_metrics_from_table(table)
    assert np.isnan(got["assd"][:, 0]).all() and np.isfinite(got["assd"][:, 1]).all()
    # the public front end on the same masks: bool and float inputs, host arrays, one table
    t2, c2 = ops.surface_distances(torch.from_numpy(pred), torch.from_numpy(gt).float().to(DEV))
    assert isinstance(t2, np.ndarray) and t2.dtype == np.float64 and c2.dtype == np.int64
    assert np.array_equal(t2, table, equal_nan=True) and np.array_equal(c2, counts)
    cup, disc = metrics.assd_2label(torch.from_numpy(pred), torch.from_numpy(gt))
    assert np.isnan(cup).all() and np.array_equal(disc, got["assd"][:, 1])
    cup, disc = metrics.hd_2label(torch.from_numpy(pred), torch.from_numpy(gt))
    assert np.isnan(cup).all() and np.array_equal(disc, got["hd"][:, 1])


def test_table_is_deterministic_and_independent_of_the_batch():
    pred, gt = sr.special_96x80()
    K = ops.kernels()
    p, g = torch.from_numpy(pred.astype(np.uint8)).to(DEV), torch.from_numpy(gt.astype(np.uint8)).to(DEV)
    t1, c1 = K.surface_distance(p, g)
    t2, c2 = K.surface_distance(p, g)
    assert torch.equal(t1, t2) and torch.equal(c1, c2)
    for b in range(3):
        tb, cb = K.surface_distance(p[b:b + 1].contiguous(), g[b:b + 1].contiguous())
        assert torch.equal(tb[0], t1[b]) and torch.equal(cb[0], c1[b]), b
    # the optional distance map does not change the table either
    t3, _, _ = K.surface_distance(p, g, want_d2=True)
    assert torch.equal(t1, t3)


@pytest.mark.parametrize("case", ["H=1025", "W=0", "short workspace"])
def test_bad_arguments_return_an_error_and_write_nothing(case):
    K = ops.kernels()
    B, H, W = 1, 64, 48
    pred = torch.ones(B, 2, 1025, W, dtype=torch.uint8, device=DEV)          # large enough for the rejected H as well
    table = torch.full((B, 2, 2, 3), 12345.0, dtype=torch.float64, device=DEV)
    counts = torch.full((B, 2, 3), -77, dtype=torch.int64, device=DEV)
    need = K.lib.uda_surface_distance_workspace_bytes(B, H, W)
    assert need > 4 * B * H * W * 7
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    h, w, nbytes = {"H=1025": (1025, W, need), "W=0": (H, 0, need), "short workspace": (H, W, need - 1)}[case]
    rc = K.lib.uda_surface_distance(pred.data_ptr(), pred.data_ptr(), B, h, w, table.data_ptr(), counts.data_ptr(), None, ws.data_ptr(),
                                    nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_surface_distance" in K.lib.uda_last_error()
    assert bool((table == 12345.0).all()) and bool((counts == -77).all()) and bool((ws == 0xA5).all())


def test_evaluate_matches_the_stepwise_scipy_chain():
    """4 images of 128 x 128 in 2 batches.  Dice, n and HD exactly; ASSD within (max n + 4) * 2^-52 * assd_ref: each directed sum
    within (n + 2) * 2^-52 relative (above), and the division and the addition that follow round once on either side."""
    batches, logits = sr.eval_batches(n_images=4, batch=2, S=128)
    res = ev.evaluate(sr.standin_model(logits), batches)
    assert res["n_images"] == 4 and res["n_undefined"] == {"cup": 0, "disc": 0}
    assert [r["img_name"] for r in res["per_image"]] == ["img_%02d.png" % i for i in range(4)]
    for i, r in enumerate(res["per_image"]):
        b, k = divmod(i, 2)
        mask = _scipy_postprocess(torch.sigmoid(logits[i]).numpy(), 0.75, 0.75).astype(bool)
        gt = batches[b]["map"][k].numpy() > 0.5
        rt, rc, _ = sr.reference(mask[None], gt[None])
        dt, dc = ops.surface_distances(torch.from_numpy(mask[None]), torch.from_numpy(gt[None]))
        assert np.array_equal(dt[..., 0], rt[..., 0]) and np.array_equal(dc, rc)
        want, dice = metrics.surface_metrics_from_table(rt), metrics.dice_per_image(rc)
        for c, name in enumerate(("cup", "disc")):
            assert r[name + "_dice"] == dice[0, c] and r[name + "_hd"] == want["hd"][0, c]
            bound = (rt[0, c, :, 0].max() + 4) * EPS * want["assd"][0, c]
            print("%s %s assd %.6f (oracle %.6f, bound %.1e) hd %.4f dice %.4f" % (r["img_name"], name, r[name + "_assd"], want["assd"][0, c],
                                                                                   bound, r[name + "_hd"], r[name + "_dice"]))
            assert abs(r[name + "_assd"] - want["assd"][0, c]) <= bound
    for key in ev.FIELDS:
        assert res["mean"][key] == float(np.nanmean([r[key] for r in res["per_image"]]))


def test_evaluate_runs_a_deeplab():
    """plumbing only: a seeded MobileNetV2 DeepLab at 64 x 64, untrained - shapes, names, finite-or-NaN values"""
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    torch.manual_seed(0)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(DEV)
    batches, _ = sr.eval_batches(n_images=4, batch=2, S=64, seed=5)
    res = ev.evaluate(model, batches, postprocess=False)
    assert res["n_images"] == 4 and len(res["per_image"]) == 4 and model.training        # the caller's mode is restored
    for r in res["per_image"]:
        assert set(r) == {"img_name"} | set(ev.FIELDS)
        assert 0.0 < r["cup_dice"] <= 1.0 and 0.0 < r["disc_dice"] <= 1.0
        for key in ("cup_assd", "disc_assd", "cup_hd", "disc_hd"):
            assert math.isnan(r[key]) or (0.0 <= r[key] < 64 * math.sqrt(2.0))
    assert 0 <= res["n_undefined"]["cup"] <= 4 and 0 <= res["n_undefined"]["disc"] <= 4
    res = ev.evaluate(model, batches)                       # and through the post-processing
    assert res["n_images"] == 4
