"""not-gpu: the host side of the per-image evaluation - the scipy oracle against a brute-force integer minimum, the closed
forms of utils/metrics.py against the definitions' own mean / max, and evaluate() with the device stages replaced by the oracle."""
import math
import os

import numpy as np
import pytest
import torch

import surface_ref as sr
from kernel_cases import _scipy_postprocess
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops
from uda_clr_amd.utils import Utils, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _masks(H, W):
    """planes of one size: ellipses, a mask on the image edge, a single pixel"""
    rng = np.random.default_rng(H * 1000 + W)
    edge = sr.ellipse(H, W, 1, 2, 0.3 * H, 0.35 * W, 0.4)
    one = np.zeros((H, W), bool)
    one[H // 3, W // 2] = True
    return [sr.random_ellipse(rng, H, W), sr.random_ellipse(rng, H, W), edge, one]


@pytest.mark.parametrize("H,W", [(33, 17), (96, 80)])
def test_oracle_d2_is_the_integer_minimum(H, W):
    for m in _masks(H, W):
        assert m.any()
        assert np.array_equal(sr.d2_to_border(m), sr.d2_brute(m))


def test_special_masks_are_what_they_claim():
    pred, gt = sr.special_96x80()
    assert pred[1, 0].sum() == 1 and pred[1, 1].all()
    assert ndimage_label_count(pred[2, 0]) == 2 and ndimage_label_count(gt[2, 0]) == 1
    for b in range(3):
        for c in range(2):
            assert sr.border(pred[b, c]).any() and sr.border(gt[b, c]).any()
    pe, ge = sr.empty_96x80()
    assert not pe[0, 0].any() and ge[0, 0].any() and pe[1, 0].any() and not ge[1, 0].any() and not pe[2, 0].any() and not ge[2, 0].any()


def ndimage_label_count(m):
    from scipy import ndimage
    return ndimage.label(m)[1]


@pytest.mark.parametrize("H,W", [(33, 17), (96, 80)])
def test_metrics_from_table_match_the_definitions(H, W):
    ms = _masks(H, W)
    pred = np.stack([np.stack([ms[0], ms[2]]), np.stack([ms[3], ms[1]])])
    gt = np.stack([np.stack([ms[1], ms[0]]), np.stack([ms[0], ms[2]])])
    table, counts, _ = sr.reference(pred, gt)
    got = metrics.surface_metrics_from_table(table)
    dice = metrics.dice_per_image(counts)
    assert dice.shape == (2, 2) and all(v.shape == (2, 2) for v in got.values())
    for b in range(2):
        for c in range(2):
            ag, ga, assd, hd = sr.direct_metrics(pred[b, c], gt[b, c])
            assert got["asd_pred_gt"][b, c] == ag and got["asd_gt_pred"][b, c] == ga
            assert got["assd"][b, c] == assd and got["hd"][b, c] == hd
            i, s, g = (pred[b, c] & gt[b, c]).sum(), pred[b, c].sum(), gt[b, c].sum()
            assert dice[b, c] == (2.0 * i + 1.0) / (1.0 + s + g)


def test_empty_sets_are_nan_not_an_exception():
    pred, gt = sr.empty_96x80()
    table, counts, _ = sr.reference(pred, gt)
    got = metrics.surface_metrics_from_table(table)
    for key in ("asd_pred_gt", "asd_gt_pred", "assd", "hd"):
        assert np.isnan(got[key][:, 0]).all() and np.isfinite(got[key][:, 1]).all(), key
    assert np.isnan(table[:, 0, :, 1]).all() and (table[:, 0, :, 2] == -1).all()
    assert table[0, 0, 0, 0] == 0 and table[0, 0, 1, 0] > 0 and table[1, 0, 0, 0] > 0 and table[1, 0, 1, 0] == 0 and (table[2, 0, :, 0] == 0).all()
    dice = metrics.dice_per_image(counts)
    assert dice[2, 0] == 1.0 and dice[0, 0] == 1.0 / (1.0 + gt[0, 0].sum())
    # a table that only carries the counted n (no NaN / -1 marks) is treated the same
    bare = table.copy()
    bare[:, 0, :, 1:] = 0.0
    assert np.isnan(metrics.surface_metrics_from_table(bare)["assd"][:, 0]).all()


def _scipy_batch(prob, threshold=0.75, dataset='G'):
    thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
    return torch.from_numpy(np.stack([_scipy_postprocess(p, thr_cup, thr_disc) for p in prob.cpu().numpy()]))


def test_evaluate_structure_with_oracle_stages(monkeypatch):
    batches, logits = sr.eval_batches(n_images=4, batch=2, S=128)
    logits[1][0] = -6.0                                    # image 1 predicts no cup at all
    calls = []
    monkeypatch.setattr(ops, "surface_distances", lambda p, g: (calls.append(tuple(p.shape)), sr.surface_distances(p, g))[1])
    monkeypatch.setattr(Utils, "postprocessing_batch", _scipy_batch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    class Model(torch.nn.Module):
        def forward(self, x):
            assert not self.training and not torch.is_grad_enabled()
            return sr.standin_model(logits)(x)

    model = Model().train()
    res = ev.evaluate(model, batches)
    assert model.training                                   # the caller's mode is restored
    assert calls == [(2, 2, 128, 128)] * 2                  # one metric call per batch, none per image
    assert set(res) == {"per_image", "mean", "n_images", "n_undefined"}
    assert res["n_images"] == 4 and res["n_undefined"] == {"cup": 1, "disc": 0}
    assert [r["img_name"] for r in res["per_image"]] == ["img_%02d.png" % i for i in range(4)]
    for i, r in enumerate(res["per_image"]):
        assert set(r) == {"img_name"} | set(ev.FIELDS)
        b, k = divmod(i, 2)
        prob = torch.sigmoid(logits[i]).numpy()
        mask = _scipy_postprocess(prob, 0.75, 0.75).astype(bool)
        gt = batches[b]["map"][k].numpy() > 0.5
        for c, name in enumerate(("cup", "disc")):
            _, _, assd, hd = sr.direct_metrics(mask[c], gt[c])
            inter, s, g = (mask[c] & gt[c]).sum(), mask[c].sum(), gt[c].sum()
            assert r[name + "_dice"] == (2.0 * inter + 1.0) / (1.0 + s + g)
            if i == 1 and c == 0:
                assert math.isnan(r["cup_assd"]) and math.isnan(r["cup_hd"])
            else:
                assert mask[c].any(), "the post-processing must not empty these ellipses"
                assert r[name + "_assd"] == assd and r[name + "_hd"] == hd
    for key in ev.FIELDS:
        assert res["mean"][key] == float(np.nanmean([r[key] for r in res["per_image"]]))
    # without post-processing the plain thresholds decide: +-6 logits give back the drawn ellipses
    raw = ev.evaluate(model, batches, postprocess=False)
    assert raw["n_undefined"] == {"cup": 1, "disc": 0}
    pm = (logits[0] > 0).numpy()
    gt0 = batches[0]["map"][0].numpy() > 0.5
    assert raw["per_image"][0]["disc_hd"] == sr.direct_metrics(pm[1], gt0[1])[3]


def test_evaluate_rejects_uint8_handover_batches():
    with pytest.raises(ValueError, match="decoded float batches"):
        ev.evaluate(lambda x: x, [{"image_u8": torch.zeros(1, 8, 8, 3, dtype=torch.uint8)}])


def test_surface_distances_has_no_cpu_fallback(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = torch.zeros(1, 2, 8, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.surface_distances(m, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.assd_2label(m, m)


def test_header_declares_the_surface_symbols():
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    for sym in ("uda_surface_distance_workspace_bytes(", "uda_surface_distance("):
        assert sym in txt
    assert "utils/metrics.py:62-68" in txt and "utils/Utils.py:438-463" in txt
    from uda_clr_amd.kernels import SYMBOLS
    assert {"uda_surface_distance_workspace_bytes", "uda_surface_distance"} <= set(SYMBOLS)
