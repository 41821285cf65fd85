"""Without a GPU: the sector table, the closed forms of utils/metrics.py over the integers of ops.disc_morphometry (with the numpy
restatement of tests/morphometry_ref.py in the kernel's place) on hand-computed cases and against the figures formed straight from the
pixels, the NaN / empty rules, and how evaluate() and predict pass the option on.

Equality throughout, except where two different library routines stand behind one figure:
  cup_offset   np.hypot here, math.hypot in the restatement, each within 1 ulp of the true value: |a - b| <= 4 * 2^-52 * value;
  major, minor the package forms the 2x2 covariance from integer numerators (one rounding each) and solves it in closed form, the
               restatement takes np.cov of the centred coordinates (N <= 2^13 pixels here, relative error <= N * 2^-53 < 1e-12 per
               entry) and LAPACK's eigh: |a - b| <= 1e-9 * major, a bound on both axes because an eigenvalue moves by at most the
               norm of the perturbation, which is relative to the LARGER one; orientation within 1e-6 degrees where the two axes
               differ by more than 1 % (the eigenvector's angle moves by perturbation / eigenvalue gap)."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import morphometry_ref as mr
import surface_profile_ref as spr
import surface_ref as sr
from kernel_cases import _scipy_postprocess
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict
from uda_clr_amd.utils import Utils, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _closed(masks, K):
    table = metrics.sector_table(K)
    return metrics.morphometry_from_moments(dict(mr.integers(masks, table), table=table)), table


# ------------------------------------------------------------------------------------------------------------ the sector table
@pytest.mark.parametrize("K", [8, 72, 360])
def test_sector_table(K):
    s = metrics.sector_table(K)
    assert s.dtype == np.int64 and s.shape == (K, 2)
    assert s[0].tolist() == [2 ** 30, 0] and s[K // 8, 0] == s[K // 8, 1] > 0
    assert s[K // 4].tolist() == [0, 2 ** 30] and s[K // 2].tolist() == [-2 ** 30, 0] and s[3 * K // 4].tolist() == [0, -2 ** 30]
    nxt = np.roll(s, -1, axis=0)
    assert (s[:, 0] * nxt[:, 1] - s[:, 1] * nxt[:, 0] > 0).all()                          # strictly counter-clockwise, the wrap included
    q = K // 4
    assert np.array_equal(np.roll(s, -q, axis=0), np.stack([-s[:, 1], s[:, 0]], 1))      # s_{j + K/4} = (-s_j.y, s_j.x) all the way round
    assert np.abs(s).max() == 2 ** 30
    t = 2.0 * np.pi * np.arange(q) / K
    assert np.array_equal(s[:q, 0], np.rint(2.0 ** 30 * np.cos(t))) and np.array_equal(s[:q, 1], np.rint(2.0 ** 30 * np.sin(t)))


@pytest.mark.parametrize("K", [0, 4, 12, 100, 368])
def test_sector_table_refuses(K):
    with pytest.raises(ValueError, match="multiple of 8"):
        metrics.sector_table(K)


# ------------------------------------------------------------------------------------------------------- hand-computed cases
def test_nested_squares_9x9_by_hand():
    f, table = _closed(mr.nested_9x9(), 8)
    ints = mr.integers(mr.nested_9x9(), table)
    assert ints["radial"].tolist() == [[[625, 1250] * 4, [3125, 5000] * 4]]
    assert ints["moments"].tolist() == [[[9, 36, 36, 150, 150, 144], [25, 100, 100, 450, 450, 400]]]
    assert ints["extent"].tolist() == [[[3, 5, 3, 5], [2, 6, 2, 6]]] and ints["overlap"].tolist() == [9]
    assert f["vcdr"][0] == 0.6 and f["hcdr"][0] == 0.6 and f["acdr"][0] == 0.36 and f["rim_area"][0] == 16.0
    assert f["centroid"].tolist() == [[[4.0, 4.0], [4.0, 4.0]]] and f["cup_offset"].tolist() == [[0.0, 0.0]]
    want = [1.0 - (math.sqrt(625) / 25) / (math.sqrt(3125) / 25), 1.0 - (math.sqrt(1250) / 25) / (math.sqrt(5000) / 25)] * 4
    assert f["rim_ratio"][0].tolist() == want and want[1] == 0.5 and abs(want[0] - (1 - 1 / math.sqrt(5))) < 1e-15
    assert f["rdr_min"][0] == 0.5 and f["rdr_min_angle"][0] == 67.5 and f["n_empty_sectors"][0] == 0
    for q in ("rim_up", "rim_left", "rim_down", "rim_right"):                              # every quadrant holds one sector of each kind
        assert f[q][0] == math.fsum([want[1], want[0]]) / 2
    # a square: both eigenvalues (s^2 - 1) / 12, no direction
    assert f["major"][0].tolist() == f["minor"][0].tolist() == [4 * math.sqrt(8 / 12), 4 * math.sqrt(24 / 12)]
    assert f["orientation"][0].tolist() == [0.0, 0.0] and f["eccentricity"][0].tolist() == [0.0, 0.0]


def test_rectangles_and_a_diagonal_by_hand():
    m = np.zeros((3, 2, 48, 64), bool)
    m[0, 1, 10:20, 5:35] = True                             # 10 rows x 30 columns: the major axis lies along x
    m[0, 0, 12:18, 10:20] = True
    m[1, 1, 4:44, 30:38] = True                             # 40 rows x 8 columns: along y
    for i in range(20):                                     # a line rising to the right: row falls as the column grows -> +45 degrees
        m[2, 1, 30 - i, 10 + i] = True
    f, _ = _closed(m, 8)
    near = lambda v: pytest.approx(v, rel=1e-14, abs=0)     # (a + b) / 2 + (a - b) / 2 is a within a few roundings, not exactly
    assert f["major"][0, 1] == near(4 * math.sqrt((900 - 1) / 12)) and f["minor"][0, 1] == near(4 * math.sqrt((100 - 1) / 12))
    assert f["orientation"][0].tolist() == [0.0, 0.0] and f["eccentricity"][0, 1] == near(math.sqrt(1 - 99 / 899))
    assert f["major"][1, 1] == near(4 * math.sqrt((1600 - 1) / 12)) and f["minor"][1, 1] == near(4 * math.sqrt((64 - 1) / 12))
    assert f["orientation"][1, 1] == 90.0 and math.isnan(f["orientation"][1, 0])
    assert f["orientation"][2, 1] == near(45.0) and f["minor"][2, 1] == 0.0 and f["eccentricity"][2, 1] == 1.0
    assert f["hcdr"][0] == 10 / 30 and f["vcdr"][0] == 6 / 10 and f["acdr"][0] == 60 / 300
    assert f["cup_offset"][0].tolist() == [14.5 - 14.5, 14.5 - 19.5]


# ------------------------------------------------------------------------------------------- against the figures from the pixels
CASES = {"9x9 K=8": (mr.nested_9x9, 8), "33x17": (lambda: mr.ellipse_pairs(5, 3, 33, 17), 72), "96x80": (lambda: mr.ellipse_pairs(6, 3, 96, 80), 72),
         "empties": (mr.empties_96x80, 72), "partly outside": (mr.cup_partly_outside_96x80, 72), "off centre": (mr.cup_off_centre_96x80, 72),
         "single pixel": (mr.single_pixel_disc, 8), "borders": (mr.touching_borders_96x80, 72), "96x80 K=360": (lambda: mr.ellipse_pairs(7, 1, 96, 80), 360)}
EXACT = ("vcdr", "hcdr", "acdr", "rim_area", "rim_ratio", "rdr_min", "rdr_min_angle", "n_empty_sectors", "rim_up", "rim_left", "rim_down", "rim_right")


def _check_figures(f, want):
    for k in EXACT:
        assert np.array_equal(f[k], want[k], equal_nan=True), k
    off = np.hypot(f["cup_offset"][:, 0], f["cup_offset"][:, 1])
    assert np.array_equal(np.isnan(off), np.isnan(want["cup_offset"]))
    ok = ~np.isnan(off)
    assert (np.abs(off - want["cup_offset"])[ok] <= 4 * 2.0 ** -52 * want["cup_offset"][ok]).all()
    for b in range(off.shape[0]):
        for k in range(2):
            if np.isnan(want["cov"][b, k]).any():
                assert math.isnan(f["major"][b, k]) and math.isnan(f["minor"][b, k]) and math.isnan(f["orientation"][b, k])
                continue
            major, minor, ang = mr.axes_of(want["cov"][b, k])
            assert abs(f["major"][b, k] - major) <= 1e-9 * major and abs(f["minor"][b, k] - minor) <= 1e-9 * major + 1e-300
            if minor < 0.99 * major:
                d = abs(f["orientation"][b, k] - ang)
                assert min(d, 180.0 - d) <= 1e-6, (b, k, f["orientation"][b, k], ang)


@pytest.mark.parametrize("name", sorted(CASES))
def test_closed_forms_match_the_figures_from_the_pixels(name):
    make, K = CASES[name]
    masks = make()
    f, table = _closed(masks, K)
    _check_figures(f, mr.figures(masks, table))


def test_vertical_cdr_is_that_of_the_surface_profile():
    masks = np.concatenate([mr.ellipse_pairs(6, 3, 96, 80), mr.empties_96x80()])
    f, _ = _closed(masks, 72)
    ext = mr.integers(masks, metrics.sector_table(72))["extent"]
    profile = {"extent": np.stack([ext[:, :, :2], ext[:, :, :2]], 2)}                     # [B, class, slot, 2]: both slots the same mask
    got = metrics.vertical_cdr_from_profile(profile)
    assert np.array_equal(f["vcdr"], got["vcdr_pred"], equal_nan=True) and np.array_equal(f["vcdr"], got["vcdr_gt"], equal_nan=True)
    assert np.isfinite(f["vcdr"][:3]).all() and math.isnan(f["vcdr"][4])


def test_empty_and_nan_rules():
    f, _ = _closed(mr.empties_96x80(), 72)
    # image 0: no cup - ratios 0, the rim is the whole radius wherever the disc has a sector, no cup ellipse
    assert f["vcdr"][0] == f["hcdr"][0] == f["acdr"][0] == 0.0 and (f["rim_ratio"][0] == 1.0).all() and f["rdr_min"][0] == 1.0
    assert f["n_empty_sectors"][0] == 0 and f["rim_up"][0] == f["rim_right"][0] == 1.0 and f["rdr_min_angle"][0] == 2.5
    assert np.isnan(f["centroid"][0, 0]).all() and np.isnan(f["cup_offset"][0]).all()
    assert math.isnan(f["major"][0, 0]) and math.isnan(f["orientation"][0, 0]) and math.isnan(f["eccentricity"][0, 0]) and f["major"][0, 1] > 0
    # image 1: no disc - every ratio NaN, the cup's own ellipse stays; image 2: nothing at all
    for b in (1, 2):
        for k in ("vcdr", "hcdr", "acdr", "rdr_min", "rdr_min_angle", "rim_up", "rim_left", "rim_down", "rim_right"):
            assert math.isnan(f[k][b]), (k, b)
        assert np.isnan(f["rim_ratio"][b]).all() and f["n_empty_sectors"][b] == 72 and f["rim_area"][b] == 0.0
    assert f["major"][1, 0] > 0 and math.isnan(f["major"][1, 1]) and np.isnan(f["major"][2]).all()
    # a cup away from the disc's centroid: its far sectors are empty, the near ones are not, and the thinnest rim is among the near ones
    f, table = _closed(mr.cup_off_centre_96x80(), 72)
    rad = mr.integers(mr.cup_off_centre_96x80(), table)["radial"][0]
    assert (rad[1] >= 0).all() and 0 < (rad[0] < 0).sum() < 72 and f["n_empty_sectors"][0] == (rad[0] < 0).sum()
    assert np.array_equal(np.isnan(f["rim_ratio"][0]), rad[0] < 0) and 0 < f["rdr_min"][0] < 1
    assert rad[0, int(f["rdr_min_angle"][0] // 5)] >= 0
    # one pixel: u = 0 for it, no sector at all
    f, _ = _closed(mr.single_pixel_disc(), 8)
    assert f["vcdr"][0] == f["hcdr"][0] == f["acdr"][0] == 1.0 and f["n_empty_sectors"][0] == 8 and math.isnan(f["rdr_min"][0])
    assert f["major"][0].tolist() == [0.0, 0.0] and f["eccentricity"][0].tolist() == [0.0, 0.0]


# ----------------------------------------------------------------------------------------------------------------- plumbing
def _scipy_batch(prob, threshold=0.75, dataset='G'):
    thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
    return torch.from_numpy(np.stack([_scipy_postprocess(p, thr_cup, thr_disc) for p in prob.cpu().numpy()]))


@pytest.fixture
def host_stages(monkeypatch):
    """the device stages of evaluate() replaced by their restatements; returns the list of morphometry calls (shape, sectors)"""
    calls = []

    def morph(masks, sectors=72):
        calls.append((tuple(masks.shape), masks.dtype, sectors))
        table = metrics.sector_table(sectors)
        return dict(mr.integers(masks.cpu().numpy(), table), table=table)
    monkeypatch.setattr(ops, "disc_morphometry", morph)
    monkeypatch.setattr(ops, "surface_distances", sr.surface_distances)
    monkeypatch.setattr(ops, "surface_profile", spr.surface_profile)
    monkeypatch.setattr(Utils, "postprocessing_batch", _scipy_batch)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    return calls


def test_evaluate_adds_the_morphometry_fields(host_stages):
    batches, logits = sr.eval_batches(4, 2, 128)
    model = sr.standin_model(logits)
    plain = ev.evaluate(model, batches)
    assert host_stages == [] and "extra_fields" not in plain and set(plain["mean"]) == set(ev.FIELDS)
    res = ev.evaluate(model, batches, morphometry=True, sectors=40)
    want_names = ("hcdr_pred", "hcdr_gt", "hcdr_error", "acdr_pred", "acdr_gt", "acdr_error", "rdr_min_pred", "rdr_min_gt", "rdr_min_error",
                  "rim_up_pred", "rim_up_gt", "rim_left_pred", "rim_left_gt", "rim_down_pred", "rim_down_gt", "rim_right_pred", "rim_right_gt",
                  "cup_offset_pred")
    assert res["extra_fields"] == want_names == ev.extra_fields(morphometry=True) == ev.extra_fields(False, (), False, True)
    assert ev.extra_fields(True, (2,), True, True) == ev.extra_fields(True, (2,), True) + want_names and ev.extra_fields() == ()
    assert host_stages == [((4, 2, 128, 128), torch.uint8, 40)] * 2                       # ONE call per batch: prediction and truth stacked
    table = metrics.sector_table(40)
    for i, (r, p) in enumerate(zip(res["per_image"], plain["per_image"])):
        assert set(r) == set(p) | set(want_names) and all(r[k] == p[k] for k in p)
        b, k = divmod(i, 2)
        mask = _scipy_postprocess(torch.sigmoid(logits[i]).numpy(), 0.75, 0.75).astype(bool)[None]
        gt = batches[b]["map"][k].numpy()[None] > 0.5
        fp, fg = mr.figures(mask, table), mr.figures(gt, table)
        for x in ("hcdr", "acdr", "rdr_min"):
            assert r[x + "_pred"] == fp[x][0] and r[x + "_gt"] == fg[x][0] and r[x + "_error"] == abs(fp[x][0] - fg[x][0])
            assert 0 < r[x + "_gt"] < 1
        for q in ("up", "left", "down", "right"):
            assert r["rim_%s_pred" % q] == fp["rim_" + q][0] and r["rim_%s_gt" % q] == fg["rim_" + q][0]
        assert abs(r["cup_offset_pred"] - fp["cup_offset"][0]) <= 4 * 2.0 ** -52 * fp["cup_offset"][0]
    for key in ev.FIELDS + want_names:
        assert res["mean"][key] == float(np.nanmean([r[key] for r in res["per_image"]]))
    both = ev.evaluate(model, batches, cdr=True, morphometry=True)                        # after the existing names, and beside them
    assert both["extra_fields"] == ("vcdr_pred", "vcdr_gt", "cdr_error") + want_names and host_stages[-1][2] == 72


def test_evaluate_parser_and_writers(host_stages, tmp_path):
    a = ev.build_parser().parse_args(["--data-dir", "d", "--checkpoint", "c"])
    assert a.morphometry is False and a.sectors == 72
    a = ev.build_parser().parse_args(["--data-dir", "d", "--checkpoint", "c", "--morphometry", "--sectors", "120"])
    assert a.morphometry is True and a.sectors == 120
    batches, logits = sr.eval_batches(2, 2, 128)
    res = ev.evaluate(sr.standin_model(logits), batches, morphometry=True)
    ev.write_csv(str(tmp_path / "m.csv"), res)
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert rows[0] == ["img_name"] + list(ev.FIELDS) + list(ev.MORPHOMETRY_FIELDS) and len(rows) == 3
    assert float(rows[1][rows[0].index("acdr_pred")]) == res["per_image"][0]["acdr_pred"]
    assert "rdr_min_pred" in ev.format_mean(res)


def test_predict_columns_parser_and_csv(host_stages, tmp_path):
    a = predict.build_parser().parse_args(["--images", "i", "--out", "o"])
    assert a.morphometry is False and a.sectors == 72
    a = predict.build_parser().parse_args(["--images", "i", "--out", "o", "--morphometry", "--sectors", "8"])
    assert a.morphometry is True and a.sectors == 8
    masks = mr.ellipse_pairs(6, 2, 96, 80)
    cols = predict.morphometry_columns(torch.from_numpy(masks), 72)
    assert host_stages == [((2, 2, 96, 80), torch.bool, 72)] and tuple(cols) == predict.MORPHOMETRY_COLUMNS
    assert predict.MORPHOMETRY_COLUMNS == ("hcdr_pred", "acdr_pred", "rdr_min_pred", "rim_up_pred", "rim_left_pred", "rim_down_pred", "rim_right_pred",
                                           "cup_offset_pred", "cup_major", "cup_minor", "cup_orientation", "disc_major", "disc_minor", "disc_orientation")
    want = mr.figures(masks, metrics.sector_table(72))
    for x in ("hcdr", "acdr", "rdr_min", "rim_up", "rim_left", "rim_down", "rim_right"):
        assert np.array_equal(cols[x + "_pred"], want[x])
    major, minor, ang = mr.axes_of(want["cov"][1, 1])
    assert abs(cols["disc_major"][1] - major) <= 1e-9 * major and abs(cols["disc_minor"][1] - minor) <= 1e-9 * major
    # rows with and without the columns: the CSV keeps its two columns without them
    plain = [{"img_name": "a.png", "vcdr_pred": 0.5}]
    predict.write_csv(str(tmp_path / "p.csv"), plain)
    assert list(csv.reader(open(tmp_path / "p.csv"))) == [["img_name", "vcdr_pred"], ["a.png", "0.5"]]
    full = [dict(plain[0], **{k: float(cols[k][0]) for k in predict.MORPHOMETRY_COLUMNS})]
    predict.write_csv(str(tmp_path / "f.csv"), full)
    rows = list(csv.reader(open(tmp_path / "f.csv")))
    assert rows[0] == ["img_name", "vcdr_pred"] + list(predict.MORPHOMETRY_COLUMNS) and [float(v) for v in rows[1][2:]] == [full[0][k] for k in predict.MORPHOMETRY_COLUMNS]


def test_front_end_checks_before_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = torch.zeros(1, 2, 8, 8, dtype=torch.bool)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.disc_morphometry(m)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.disc_morphometry(m, sectors=12)
    with pytest.raises(ValueError, match="sectors"):
        ops.disc_morphometry(m, sectors=np.zeros((12, 2), np.int64))
    with pytest.raises(ValueError, match="2\\^30"):
        ops.disc_morphometry(m, sectors=metrics.sector_table(8) * 2)
    with pytest.raises(ValueError, match=r"\[B, 2, H, W\]"):
        ops.disc_morphometry(torch.zeros(1, 3, 8, 8), 8)


def test_binding_and_symbols_exist():
    """fails before the feature: the entry point, its binding and its declaration"""
    from uda_clr_amd.kernels import SYMBOLS, HipKernels
    assert "uda_disc_morphometry" in SYMBOLS and "uda_disc_morphometry_workspace_bytes" in SYMBOLS
    assert len(SYMBOLS["uda_disc_morphometry"][1]) == 13 and len(SYMBOLS["uda_disc_morphometry_workspace_bytes"][1]) == 4
    assert callable(getattr(HipKernels, "disc_morphometry")) and callable(ops.disc_morphometry)
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    for sym in ("uda_disc_morphometry_workspace_bytes(", "uda_disc_morphometry("):
        assert sym in txt
    lib = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")
    if os.path.exists(lib):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "uda_disc_morphometry")
