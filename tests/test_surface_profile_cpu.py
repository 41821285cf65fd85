"""Without a GPU: the closed forms of utils/metrics.py over the profile of ops.surface_profile (percentile distances / hd95, surface
Dice at a tolerance, vertical cup-to-disc ratio) against the figures formed directly from the distances, with the scipy oracle
(tests/surface_profile_ref.py) in the kernel's place; evaluate() with the new arguments; the command line's parser and writers.

Percentile distances are compared within 4 * 2^-52 * ref + n * 2^-52 * (sqrt(d2_hi) - sqrt(d2_lo)) (surface_profile_ref.
percentile_bound: derived, not measured); percentile 100 and percentile 0, tolerance counts and the CDR exactly."""
import csv
import json
import math
import os

import numpy as np
import pytest
import torch

import surface_profile_ref as spr
import surface_ref as sr
from kernel_cases import _scipy_postprocess
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops
from uda_clr_amd.dataloaders import synthetic
from uda_clr_amd.utils import Utils, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCT = (0, 50, 95, 100)
TOL = (1, 1.5, 2, 5, math.sqrt(2.0))
CASES = {"special": sr.special_96x80, "empty": sr.empty_96x80, "33x17": lambda: sr.random_pairs(133, 1, 33, 17)}


@pytest.fixture(scope="module", params=sorted(CASES))
def case(request):
    """masks, the oracle's (table, counts, profile) and the direct figures of one input, computed once"""
    pred, gt = CASES[request.param]()
    table, counts, prof = spr.surface_profile(pred, gt, PCT, TOL)
    return request.param, pred, gt, table, prof, spr.direct(pred, gt, PCT, TOL)


def test_percentile_distances_match_numpy_percentile(case):
    name, pred, gt, table, prof, want = case
    got = metrics.percentile_distance_from_profile(table, prof)
    assert got["hd_p"].shape == want["hd_p"].shape and got["hd_p_directed"].shape == want["hd_p_directed"].shape
    both = np.concatenate([got["hd_p_directed"], got["hd_p"][:, :, None]], 2)             # [B,2,3,Q] in the order of the sets
    ref = np.concatenate([want["hd_p_directed"], want["hd_p"][:, :, None]], 2)
    assert np.array_equal(np.isnan(both), np.isnan(ref))
    ok = ~np.isnan(ref)
    assert ok.any()
    err, bound = np.abs(both - ref)[ok], spr.percentile_bound(table, prof, np.nan_to_num(ref))[ok]
    print("%s: worst error %.3e, worst error / bound %.3f over %d entries" % (name, err.max(), float((err / np.maximum(bound, 1e-300)).max()), int(ok.sum())))
    assert (err <= bound).all()
    # the ends are exact: percentile 100 is the Hausdorff distance of the table, percentile 0 the smallest distance
    hd = metrics.surface_metrics_from_table(table)["hd"]
    assert np.array_equal(got["hd_p"][..., PCT.index(100)], hd, equal_nan=True)
    top = np.concatenate([table[..., 2], table[..., 2].max(-1, keepdims=True)], -1)       # max d2 of each direction and of both
    assert np.array_equal(both[..., PCT.index(100)][ok[..., 0]], np.sqrt(top[ok[..., 0]]))
    assert np.array_equal(both[..., PCT.index(0)][ok[..., 0]], np.sqrt(prof["order"][..., PCT.index(0), 0][ok[..., 0]].astype(np.float64)))
    assert np.array_equal(both[..., PCT.index(0)], ref[..., PCT.index(0)], equal_nan=True)
    if name == "empty":
        assert np.isnan(both[:, 0]).all() and np.isfinite(both[:, 1]).all()


def test_float_and_integer_tolerance_rules_agree_on_the_oracle(case):
    """sqrt(d2) <= tau and d2 <= floor(tau^2) select the same border pixels for the tolerances used here"""
    _, pred, gt, _, _, _ = case
    t2 = spr.tol2_of(TOL)
    assert t2.tolist() == [1, 2, 4, 25, 2]
    seen = 0
    for b in range(pred.shape[0]):
        for c in range(2):
            d = spr.directed_d2(pred[b, c], gt[b, c])
            for arr in d or ():
                for tau, t in zip(TOL, t2):
                    assert np.array_equal(np.sqrt(arr.astype(np.float64)) <= tau, arr <= t)
                    seen += 1
    assert seen


def test_surface_dice_matches_the_count_by_distance(case):
    name, _, _, table, prof, want = case
    got = metrics.surface_dice_from_profile(table, prof)
    assert got.shape == want["nsd"].shape and np.array_equal(got, want["nsd"], equal_nan=True)
    assert (got[~np.isnan(got)] <= 1.0).all() and (np.diff(got[..., [0, 1, 2, 3]], axis=-1)[~np.isnan(got[..., 1:4])] >= 0).all()
    if name == "empty":
        assert np.isnan(got[:, 0]).all() and np.isfinite(got[:, 1]).all() and (prof["within"][:, 0] == -1).all()


def test_vertical_cdr_matches_nonzero_row_extents(case):
    name, pred, gt, _, prof, _ = case
    got = metrics.vertical_cdr_from_profile(prof)
    vp, vg = spr.vcdr_direct(pred, gt)
    assert np.array_equal(got["vcdr_pred"], vp, equal_nan=True) and np.array_equal(got["vcdr_gt"], vg, equal_nan=True)
    assert np.array_equal(got["cdr_error"], np.abs(vp - vg), equal_nan=True)
    if name == "empty":                                   # a cup that is empty gives vCDR 0, and the extents of the other mask stay defined
        assert got["vcdr_pred"][0] == 0.0 and got["vcdr_gt"][0] > 0 and got["vcdr_gt"][1] == 0.0 and got["vcdr_pred"][2] == 0.0 == got["vcdr_gt"][2]
        assert (prof["extent"][0, 0, 1] == -1).all() and (prof["extent"][0, 0, 0] >= 0).all()


def test_vertical_cdr_without_a_disc_is_nan():
    pred, gt = sr.random_pairs(5, 2, 33, 17)
    pred[0, 1] = False                                    # image 0 predicts no disc; image 1 has no true disc
    gt[1, 1] = False
    got = metrics.vertical_cdr_from_profile(spr.profile(pred, gt, (), ()))
    vp, vg = spr.vcdr_direct(pred, gt)
    assert math.isnan(got["vcdr_pred"][0]) and math.isnan(got["vcdr_gt"][1]) and np.isnan(got["cdr_error"]).all()
    assert got["vcdr_gt"][0] == vg[0] and got["vcdr_pred"][1] == vp[1]


def _scipy_batch(prob, threshold=0.75, dataset='G'):
    thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
    return torch.from_numpy(np.stack([_scipy_postprocess(p, thr_cup, thr_disc) for p in prob.cpu().numpy()]))


@pytest.fixture
def host_stages(monkeypatch):
    """the device stages of evaluate() replaced by their oracles; returns the list of profile calls"""
    calls = []

    def profile(p, g, percentiles=(95,), tolerances=()):
        calls.append((tuple(p.shape), tuple(percentiles), tuple(tolerances)))
        return spr.surface_profile(p, g, percentiles, tolerances)
    monkeypatch.setattr(ops, "surface_profile", profile)
    monkeypatch.setattr(ops, "surface_distances", sr.surface_distances)
    monkeypatch.setattr(Utils, "postprocessing_batch", _scipy_batch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    return calls


def test_evaluate_adds_hd95_nsd_and_cdr(host_stages):
    batches, logits = sr.eval_batches(4, 2, 128)
    model = sr.standin_model(logits)
    res = ev.evaluate(model, batches, hd95=True, tolerances=(2,), cdr=True)
    extra = ("cup_hd95", "disc_hd95", "cup_nsd_2", "disc_nsd_2", "vcdr_pred", "vcdr_gt", "cdr_error")
    assert res["extra_fields"] == extra and ev.FIELDS == ("cup_dice", "disc_dice", "cup_assd", "disc_assd", "cup_hd", "disc_hd")
    assert host_stages == [((2, 2, 128, 128), (95,), (2.0,))] * 2          # one call per batch, none per image
    assert set(res) == {"per_image", "mean", "n_images", "n_undefined", "extra_fields"}
    plain = ev.evaluate(model, batches)
    assert set(plain) == {"per_image", "mean", "n_images", "n_undefined"} and set(plain["mean"]) == set(ev.FIELDS)
    assert len(host_stages) == 2                                            # the default call does not go through the profile
    for i, (r, p) in enumerate(zip(res["per_image"], plain["per_image"])):
        assert set(p) == {"img_name"} | set(ev.FIELDS) and set(r) == set(p) | set(extra)
        assert all(r[k] == p[k] for k in p)
        b, k = divmod(i, 2)
        mask = _scipy_postprocess(torch.sigmoid(logits[i]).numpy(), 0.75, 0.75).astype(bool)[None]
        gt = batches[b]["map"][k].numpy()[None] > 0.5
        want = spr.direct(mask, gt, (95,), (2,))
        table, _, prof = spr.surface_profile(mask, gt, (95,), (2,))
        bound = spr.percentile_bound(table, prof, want["hd_p"][:, :, None])[0, :, 2, 0]
        vp, vg = spr.vcdr_direct(mask, gt)
        for c, name in enumerate(("cup", "disc")):
            assert abs(r[name + "_hd95"] - want["hd_p"][0, c, 0]) <= bound[c] and 0 < r[name + "_hd95"] <= r[name + "_hd"]
            assert r[name + "_nsd_2"] == want["nsd"][0, c, 0]
        assert r["vcdr_pred"] == vp[0] and r["vcdr_gt"] == vg[0] and r["cdr_error"] == abs(vp[0] - vg[0]) and 0 < r["vcdr_gt"] < 1
    for key in ev.FIELDS + extra:
        assert res["mean"][key] == float(np.nanmean([r[key] for r in res["per_image"]]))
    # each argument alone adds only its own names; the tolerance is formatted with %g
    only = ev.evaluate(model, batches, tolerances=(1.5, 2))
    assert only["extra_fields"] == ("cup_nsd_1.5", "disc_nsd_1.5", "cup_nsd_2", "disc_nsd_2")
    assert host_stages[-1] == ((2, 2, 128, 128), (), (1.5, 2.0))
    assert ev.evaluate(model, batches, cdr=True)["extra_fields"] == ("vcdr_pred", "vcdr_gt", "cdr_error")


def test_parser_reads_every_option():
    a = ev.build_parser().parse_args(["--data-dir", "d", "--checkpoint", "c.pth"])
    assert (a.dataset, a.split, a.backbone, a.out_stride, a.use_TN, a.threshold) == ("Drishti-GS", "test", "mobilenet", 16, False, 0.75)
    assert not a.no_postprocess and not a.hd95 and a.tolerance == [] and not a.cdr and a.csv is None and a.json is None
    a = ev.build_parser().parse_args("--data-dir d --dataset RIM-ONE_r3 --split train --checkpoint c.pth --backbone drn --out-stride 8 --use_TN "
                                     "--batch-size 3 --threshold 0.5 --no-postprocess --hd95 --tolerance 1 2.5 --cdr --csv a.csv --json a.json".split())
    assert (a.dataset, a.split, a.backbone, a.out_stride, a.use_TN, a.batch_size, a.threshold) == ("RIM-ONE_r3", "train", "drn", 8, True, 3, 0.5)
    assert a.no_postprocess and a.hd95 and a.tolerance == [1.0, 2.5] and a.cdr and (a.csv, a.json) == ("a.csv", "a.json")
    with pytest.raises(SystemExit):
        ev.build_parser().parse_args(["--checkpoint", "c.pth"])


def test_command_line_writes_csv_and_json(host_stages, tmp_path, capsys):
    """main() in-process on a synthetic split with a stand-in model: brightness thresholds of the drawn image"""
    synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=64)

    def model(image):
        grey = (image.mean(1) + 1.0) * 127.5
        return torch.stack([(grey - 165.0), (grey - 110.0)], 1), None
    argv = ["--data-dir", str(tmp_path), "--dataset", "Drishti-GS", "--checkpoint", "unused", "--batch-size", "2", "--no-postprocess",
            "--hd95", "--cdr", "--tolerance", "2", "--csv", str(tmp_path / "out.csv"), "--json", str(tmp_path / "out.json")]
    res = ev.main(argv, model=model)
    fields = ev.FIELDS + res["extra_fields"]
    assert res["n_images"] == 3 and len(host_stages) == 2
    assert "mean over 3 images" in capsys.readouterr().out
    rows = list(csv.reader(open(tmp_path / "out.csv")))
    assert rows[0] == ["img_name"] + list(fields) and len(rows) == 4
    assert sorted(r[0] for r in rows[1:]) == ["img_%03d.png" % i for i in range(3)]
    for row, r in zip(rows[1:], res["per_image"]):
        assert row[0] == r["img_name"]
        for k, text in zip(fields, row[1:]):
            assert float(text) == r[k] or (math.isnan(float(text)) and math.isnan(r[k]))
    back = json.load(open(tmp_path / "out.json"))
    assert back["n_images"] == 3 and back["extra_fields"] == list(res["extra_fields"]) and back["n_undefined"] == res["n_undefined"]
    assert [r["img_name"] for r in back["per_image"]] == [r["img_name"] for r in res["per_image"]]
    for k in fields:
        assert back["mean"][k] == res["mean"][k] or (math.isnan(back["mean"][k]) and math.isnan(res["mean"][k]))
    assert 0.5 < res["mean"]["disc_dice"] <= 1.0            # the stand-in does segment the drawn disc


def test_surface_profile_front_end_checks_before_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = torch.zeros(1, 2, 8, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.surface_profile(m, m)
    with pytest.raises(ValueError, match="percentiles"):
        ops.surface_profile(m, m, percentiles=(150,))
    with pytest.raises(ValueError, match="tolerances"):
        ops.surface_profile(m, m, tolerances=(-1,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.hd95_2label(m, m)


def test_header_declares_the_profile_symbols():
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    for sym in ("uda_surface_profile_workspace_bytes(", "uda_surface_profile("):
        assert sym in txt
