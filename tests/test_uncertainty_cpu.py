"""Without a GPU: the integer tables of calibration and selective prediction (the numpy restatement of tests/uncertainty_ref.py in the
kernel's place) on a hand-computed plane and at the bin edges, the closed forms of utils/metrics.py over them against the figures formed
straight from the pixels, pooling, and how evaluate(), predict and the command lines pass the options on.

Ratios of two integers (coverage, kept Dice, error rates, prevalence, bin accuracy) are compared for equality: one IEEE division of the
same integers on both sides.  ECE, MCE, Brier, mean confidence, AUROC and AURC are sums of such terms taken in another order by the direct
evaluation (math.fsum over pixels there, integer sums and one division here): within 4 ulp.  Both sides form the gap of a bin from the
same two exactly representable sums, so no cancellation separates them."""
import csv
import math
import os

import numpy as np
import pytest
import torch

import surface_profile_ref as spr
import surface_ref as sr
import uncertainty_ref as ur
from kernel_cases import _scipy_postprocess
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict
from uda_clr_amd.utils import Utils, metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 4 * np.spacing(abs(b))          # 4 ulp


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _planes(seed, B=2, H=24, W=20):
    rng = np.random.default_rng(seed)
    gt = rng.random((B, 2, H, W)) < 0.4
    prob = np.clip(np.where(gt, 0.7, 0.2) + 0.35 * rng.standard_normal((B, 2, H, W)), 0, 1).astype(np.float32)
    prob[:, :, :3] = 0.0                                                    # a run in one bin
    pred = prob > 0.5
    unc = (0.1 * rng.random((B, 2, H, W)) * (1.0 + 3.0 * (pred != gt))).astype(np.float32)
    return prob, unc, pred, gt


# ------------------------------------------------------------------------------------------------------------- by hand
def test_default_edges_hold_the_trainers_threshold():
    assert ops.DEFAULT_UNC_EDGES == (0.005, 0.01, 0.02, 0.03, 0.04, 0.06, 0.08, 0.12, 0.16) == ur.DEFAULT_EDGES


def test_tables_of_a_3x4_plane_by_hand():
    p = np.array([[0.0, 0.25, 0.5, 1.0], [0.125, 0.375, 0.75, 0.875], [0.0, 0.0, 0.99, 0.5]], np.float32)
    g = np.array([[0, 0, 1, 1], [0, 1, 1, 1], [0, 0, 1, 0]], bool)
    a = p > 0.4
    u = np.array([[0.0, 0.05, 0.2, 0.0], [0.01, 0.3, 0.05, 0.0], [0.0, 0.0, 0.0, 0.2]], np.float32)
    t = ur.tables(np.stack([p, p])[None], np.stack([u, u])[None], np.stack([a, a])[None], np.stack([g, ~g])[None], M=4, edges=(0.05, 0.2))
    q = lambda *v: sum(int(x * 65536) for x in v)
    q2 = lambda *v: sum(int(x * 65536) ** 2 for x in v)
    # bins of width 1/4: [0, 1/4) holds 0, 0.125, 0, 0; [1/4, 1/2) 0.25, 0.375; [1/2, 3/4) 0.5, 0.5; [3/4, 1] 1, 0.75, 0.875, 0.99
    q99 = int(np.rint(np.float32(0.99) * 65536.0))
    assert t["rel"][0, 0].tolist() == [[4, 0, q(0.125), 0, q2(0.125)], [2, 1, q(0.25, 0.375), q(0.375), q2(0.25, 0.375)],
                                       [2, 1, q(0.5, 0.5), q(0.5), q2(0.5, 0.5)],
                                       [4, 4, q(1, 0.75, 0.875) + q99, q(1, 0.75, 0.875) + q99, q2(1, 0.75, 0.875) + q99 ** 2]]
    assert t["rel"][0, 1, :, 1].tolist() == [4, 1, 1, 0] and t["rel"][0, 1, :, 0].tolist() == [4, 2, 2, 4]
    # u < 0.05: 7 pixels; [0.05, 0.2): the two 0.05; >= 0.2: 0.2, 0.3, 0.2.  pred = p > 0.4: 0.5, 1, 0.75, 0.875, 0.99, 0.5
    assert t["risk"][0, 0].tolist() == [[3, 0, 0, 4], [1, 0, 0, 1], [1, 1, 1, 0]]
    assert t["risk"][0, 1].tolist() == [[0, 3, 4, 0], [0, 1, 1, 0], [1, 1, 0, 1]]
    assert not t["invalid"].any() and t["edges"].dtype == np.float32
    c = metrics.calibration_from_table(t["rel"])
    assert c["prevalence"][0].tolist() == [0.5, 0.5] and c["bin_n"][0, 0].tolist() == [4, 2, 2, 4]
    assert c["bin_accuracy"][0, 0].tolist() == [0.0, 0.5, 0.5, 1.0] and c["bin_confidence"][0, 0, 1] == 0.3125
    assert c["ece"][0, 0] == (0.125 + abs(1 - 0.625) + 0.0 + abs(4 - (2.625 + q99 / 65536))) / 12
    s = metrics.selective_from_table(t["risk"], (0.05, 0.2))
    assert s["coverage"][0, 0].tolist() == [7 / 12, 9 / 12] and s["error"][0, 0].tolist() == [0.0, 0.0] and s["error_all"][0, 0] == 2 / 12
    assert s["dice"][0, 0].tolist() == [1.0, 1.0] and s["dice"][0, 1].tolist() == [1 / 8, 1 / 10]
    # wrong pixels (2) sit in the last bin, right ones in bins (7, 2, 1): 2 * 9 wins and 2 ties
    assert s["unc_auroc"][0, 0] == (2 * 18 + 2) / (2 * 2 * 10) and s["aurc"][0, 0] == (1 - 9 / 12) * (0 + 2 / 12) / 2


def test_bin_edges_of_both_tables():
    M = 15
    nxt = lambda v, d: np.nextafter(np.float32(v), np.float32(d))
    ps = [np.float32(0), np.float32(-0.0), np.float32(1), nxt(1, 0), nxt(1, 2), np.float32(1.0000001), np.float32(np.nan), np.float32(-1e-9)]
    for k in range(1, M):
        v = np.float32(k) / np.float32(M)
        ps += [v, nxt(v, 0), nxt(v, 1)]
    p = np.array(ps, np.float32)
    valid = ~(np.isnan(p) | (p < 0) | (p > 1))
    assert (~valid).sum() == 4 and nxt(1, 2) == np.float32(1.0000001)
    pad = lambda a: np.broadcast_to(np.asarray(a)[None, None, None, :], (1, 2, 1, len(a)))
    t = ur.tables(pad(p), None, pad(np.ones(len(p), bool)), None, M=M)
    assert t["invalid"][0, 0].tolist() == [4, 0] and t["rel"][0, 0, :, 0].sum() == valid.sum() and t["risk"] is None
    b, _ = ur.bins_of(p[valid], M)
    assert b[0] == b[1] == 0 and b[2] == b[3] == M - 1                        # 0, -0.0 in the first bin; 1 and the float below it in the last
    for k in range(1, M):                                                     # k / M: the fp32 product decides, and the kernel takes the same
        v = np.float32(k) / np.float32(M)
        assert ur.bins_of(v, M)[0] == int(np.floor(v * np.float32(M))) and ur.bins_of(nxt(v, 0), M)[0] in (k - 1, k)
    assert ur.bins_of(np.float32(1 / 3), 15)[0] == 5 and ur.bins_of(np.float32(0.2), 15)[0] == 3
    e = np.asarray(ur.DEFAULT_EDGES, np.float32)
    us = [np.float32(0), np.float32(-0.0), np.float32(np.inf), np.float32(np.nan), np.float32(-1e-9), np.float32(-np.inf)]
    for x in e:
        us += [x, nxt(x, 0), nxt(x, 1)]
    u = np.array(us, np.float32)
    t = ur.tables(None, pad(u), pad(np.ones(len(u), bool)), pad(np.zeros(len(u), bool)))
    assert t["invalid"][0, 1].tolist() == [0, 3] and t["rel"] is None
    fp = t["risk"][0, 0, :, 1]
    assert fp.sum() == len(u) - 3 and fp[0] == 3 and fp[-1] == 3              # 0, -0.0 and the float below the first edge; +inf and the last edge's two
    assert fp.tolist() == [3] + [3] * (len(e) - 1) + [3]                      # an edge and the float above it go up, the float below stays


# ------------------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("M", [1, 10, 15, 64])
def test_calibration_closed_forms_against_direct_evaluation(M):
    prob, unc, pred, gt = _planes(5)
    prob[0, 0, 5, :4] = [np.nan, 1.5, -0.25, 1.0]
    rel = ur.tables(prob, None, pred, gt, M=M)["rel"]
    c = metrics.calibration_from_table(rel)
    for b in range(2):
        for k in range(2):
            d = ur.direct_calibration(prob[b, k], gt[b, k], M)
            assert _same(c["prevalence"][b, k], d["prevalence"])
            for name in ("ece", "mce", "brier", "confidence"):
                assert _close(c[name][b, k], d[name]), (name, c[name][b, k], d[name])
    assert c["bin_n"].shape == (2, 2, M) and (c["bin_n"].sum(-1) == 24 * 20 - np.array([[3, 0], [0, 0]])).all()
    empty = metrics.calibration_from_table(np.zeros((2, M, 5), np.int64))
    assert all(np.isnan(empty[k]).all() for k in ("ece", "mce", "brier", "confidence", "prevalence", "bin_accuracy"))


@pytest.mark.parametrize("edges", [(), (0.04,), ur.DEFAULT_EDGES])
def test_selective_closed_forms_against_direct_evaluation(edges):
    prob, unc, pred, gt = _planes(6)
    unc[1, 1, 0, :3] = [np.nan, -1.0, np.inf]
    t = ur.tables(None, unc, pred, gt, edges=edges)
    s = metrics.selective_from_table(t["risk"], edges)
    e32 = np.asarray(edges, np.float32)
    for b in range(2):
        for k in range(2):
            d = ur.direct_selective(unc[b, k], pred[b, k], gt[b, k], edges)
            assert _same(s["error_all"][b, k], d["error_all"])
            for j in range(len(edges)):
                assert _same(s["coverage"][b, k, j], d["coverage"][j]) and _same(s["dice"][b, k, j], d["dice"][j])
                assert _same(s["error"][b, k, j], d["error"][j])
            u = unc[b, k].ravel()
            with np.errstate(invalid="ignore"):
                ok = u >= 0
            bins = (e32[None, :] <= u[ok][:, None]).sum(1)
            wrong = (pred[b, k] != gt[b, k]).ravel()[ok]
            assert _close(s["unc_auroc"][b, k], ur.brute_auroc(bins[wrong], bins[~wrong]))
            assert _close(s["aurc"][b, k], ur.direct_aurc(t["risk"][b, k]))
    assert t["invalid"][1, 1].tolist() == [0, 2]
    assert (s["unc_auroc"] > 0.5).all() if edges else (s["unc_auroc"] == 0.5).all()      # errors were drawn more uncertain; one bin: all ties


def test_empty_sets_give_nan():
    risk = np.zeros((3, 3, 4), np.int64)
    risk[0, :, 0] = [5, 2, 1]                                                 # no wrong pixel
    risk[1, :, 1] = [1, 0, 3]                                                 # no right pixel
    s = metrics.selective_from_table(risk, (0.1, 0.2))
    assert np.isnan(s["unc_auroc"]).all() and s["error_all"][:2].tolist() == [0.0, 1.0] and np.isnan(s["error_all"][2])
    assert s["aurc"][:2].tolist() == [0.0, 1.0] and np.isnan(s["aurc"][2]) and np.isnan(s["coverage"][2]).all()
    assert s["error"][1].tolist() == [1.0, 1.0] and s["dice"][2].tolist() == [1.0, 1.0]
    risk = np.zeros((1, 3, 4), np.int64)
    risk[0, 2] = [1, 1, 0, 2]                                                 # nothing below the second edge
    s = metrics.selective_from_table(risk, (0.1, 0.2))
    assert np.isnan(s["error"][0]).all() and s["coverage"][0].tolist() == [0.0, 0.0] and s["aurc"][0] == 0.25
    with pytest.raises(ValueError, match="edges"):
        metrics.selective_from_table(risk, (0.1,))


def test_pooled_tables_are_the_sums_over_images():
    prob, unc, pred, gt = _planes(7, B=3)
    t = ur.tables(prob, unc, pred, gt, M=10)
    cat = lambda a: np.concatenate(list(a), 1)[None]                          # the three images side by side as one
    one = ur.tables(cat(prob), cat(unc), cat(pred), cat(gt), M=10)
    assert np.array_equal(t["rel"].sum(0), one["rel"][0]) and np.array_equal(t["risk"].sum(0), one["risk"][0])
    c, s = metrics.calibration_from_table(t["rel"].sum(0)), metrics.selective_from_table(t["risk"].sum(0), ur.DEFAULT_EDGES)
    assert c["ece"].shape == (2,) and s["coverage"].shape == (2, 9)
    for k in range(2):
        d = ur.direct_calibration(cat(prob)[0, k], cat(gt)[0, k], 10)
        assert _close(c["ece"][k], d["ece"]) and _close(c["brier"][k], d["brier"])
        d = ur.direct_selective(cat(unc)[0, k], cat(pred)[0, k], cat(gt)[0, k], ur.DEFAULT_EDGES)
        assert s["coverage"][k].tolist() == d["coverage"] and s["error_all"][k] == d["error_all"]


# ----------------------------------------------------------------------------------------------------------------- plumbing
def _scipy_batch(prob, threshold=0.75, dataset='G'):
    thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
    return torch.from_numpy(np.stack([_scipy_postprocess(p, thr_cup, thr_disc) for p in prob.cpu().numpy()]))


@pytest.fixture
def host(monkeypatch, tmp_path):
    """the device stages of evaluate() replaced by their restatements; returns the HostOps that keeps the calls"""
    h = ur.HostOps()
    pictures = []
    monkeypatch.setattr(ops, "mc_uncertainty", h.mc_uncertainty)
    monkeypatch.setattr(ops, "selective_tables", h.selective_tables)
    monkeypatch.setattr(ops, "surface_distances", sr.surface_distances)
    monkeypatch.setattr(ops, "surface_profile", spr.surface_profile)
    monkeypatch.setattr(Utils, "postprocessing_batch", _scipy_batch)
    monkeypatch.setattr(Utils, "save_per_img_batch", lambda *a, **k: pictures.append("overlay"))
    monkeypatch.setattr(Utils, "save_mask_batch", lambda *a, **k: pictures.append("mask"))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    h.pictures = pictures
    return h


def _soft_model(logits):
    """the stand-in of surface_ref with its +-6 logits softened to +-1.5 near the top rows, so that the probabilities fill several bins"""
    inner = sr.standin_model(logits)

    def model(image):
        lg = inner(image)[0].clone()
        lg[:, :, :48] *= 0.25
        return lg, None
    return model


def _passes(model, sigma=1.0):
    def passes(image, T):
        lg = model(image)[0]
        g = torch.Generator().manual_seed(T)
        return (lg[None] + sigma * torch.randn((T,) + tuple(lg.shape), generator=g)).contiguous()
    return passes


def test_evaluate_without_the_flags_is_the_evaluate_of_before(host):
    batches, logits = sr.eval_batches(4, 2, 128)
    plain = ev.evaluate(sr.standin_model(logits), batches)
    assert host.unc_calls == [] and host.table_calls == [] and set(plain) == {"per_image", "mean", "n_images", "n_undefined"}
    assert set(plain["mean"]) == set(ev.FIELDS) and all(set(r) == {"img_name"} | set(ev.FIELDS) for r in plain["per_image"])
    assert ev.extra_fields() == () and ev.extra_fields(True, (2,), True, True) == ev.extra_fields(True, (2,), True, True, False, 0)


def test_evaluate_adds_calibration_and_uncertainty(host, tmp_path):
    batches, logits = sr.eval_batches(4, 2, 128)
    model = _soft_model(logits)
    passes = _passes(model)
    plain = ev.evaluate(model, batches)
    cal_names = ("cup_ece", "disc_ece", "cup_brier", "disc_brier")
    unc_names = ("cup_unc_auroc", "disc_unc_auroc", "cup_cov_0.04", "disc_cov_0.04", "cup_dice_0.04", "disc_dice_0.04", "cup_err_0.04", "disc_err_0.04")
    assert ev.extra_fields(calibration=True) == cal_names and ev.extra_fields(mc_passes=4) == unc_names
    assert ev.extra_fields(cdr=True, morphometry=True, calibration=True, mc_passes=2) == ev.extra_fields(cdr=True, morphometry=True) + cal_names + unc_names
    assert ev.extra_fields(mc_passes=2, report_edges=(0.02, 0.04))[2:5] == ("cup_cov_0.02", "disc_cov_0.02", "cup_dice_0.02")

    cal = ev.evaluate(model, batches, calibration=True, bins=10)
    assert cal["extra_fields"] == cal_names and host.unc_calls == [] and len(host.table_calls) == 2       # ONE call per batch, no pass made
    assert all(c["unc"] is None and c["bins"] == 10 and c["prob"].shape == (2, 2, 128, 128) for c in host.table_calls)
    assert "risk_coverage" not in cal and cal["calibration"]["bins"] == 10

    del host.table_calls[:]
    res = ev.evaluate(model, batches, calibration=True, mc_passes=4, mc_logits=passes, save_dir=str(tmp_path))
    assert res["extra_fields"] == cal_names + unc_names
    assert host.unc_calls == [((4, 2, 2, 128, 128), ("std",), 1600.0)] * 2 and len(host.table_calls) == 2     # both tables in one call
    assert sorted(os.listdir(tmp_path / "uncertainty")) == ["img_%02d.png" % i for i in range(4)] and host.pictures.count("mask") == 2
    from PIL import Image
    pooled_rel, pooled_risk = 0, 0
    for b, call in enumerate(host.table_calls):
        assert call["bins"] == 15 and call["edges"] == ops.DEFAULT_UNC_EDGES and call["gt"].dtype == bool
        std = ur.maps64(passes(batches[b]["image"], 4).numpy())["std"].astype(np.float32)
        assert np.array_equal(call["unc"], std) and np.array_equal(call["gt"], batches[b]["map"].numpy() > 0.5)
        t = ur.tables(call["prob"], call["unc"], call["pred"], call["gt"], 15, ops.DEFAULT_UNC_EDGES)
        pooled_rel, pooled_risk = pooled_rel + t["rel"].sum(0), pooled_risk + t["risk"].sum(0)
        for i in range(2):
            r, p = res["per_image"][2 * b + i], plain["per_image"][2 * b + i]
            assert set(r) == set(p) | set(cal_names + unc_names) and all(r[k] == p[k] for k in p)
            png = np.asarray(Image.open(tmp_path / "uncertainty" / ("img_%02d.png" % (2 * b + i))))
            u8 = ur.quantise(std[i], 1600.0)
            assert png.shape == (128, 128, 3) and not png[..., 0].any() and np.array_equal(png[..., 1], u8[1]) and np.array_equal(png[..., 2], u8[0])
            for k, c in enumerate(("cup", "disc")):
                d = ur.direct_calibration(call["prob"][i, k], call["gt"][i, k], 15)
                assert _close(r[c + "_ece"], d["ece"]) and _close(r[c + "_brier"], d["brier"]) and 0 < r[c + "_ece"] < 0.5
                d = ur.direct_selective(call["unc"][i, k], call["pred"][i, k], call["gt"][i, k], (0.04,))
                assert r[c + "_cov_0.04"] == d["coverage"][0] and r[c + "_dice_0.04"] == d["dice"][0] and _same(r[c + "_err_0.04"], d["error"][0])
                assert 0 < r[c + "_cov_0.04"] < 1
                bins = (np.asarray(ops.DEFAULT_UNC_EDGES, np.float32)[None] <= call["unc"][i, k].reshape(-1, 1)).sum(1)
                wrong = (call["pred"][i, k] != call["gt"][i, k]).ravel()
                assert _close(r[c + "_unc_auroc"], ur.brute_auroc(bins[wrong], bins[~wrong]))
    for key in cal_names + unc_names:
        assert res["mean"][key] == float(np.nanmean([r[key] for r in res["per_image"]]))
    assert res["calibration"]["rel"] == pooled_rel.tolist() and res["risk_coverage"]["risk"] == pooled_risk.tolist()
    c, s = metrics.calibration_from_table(pooled_rel), metrics.selective_from_table(pooled_risk, ops.DEFAULT_UNC_EDGES)
    assert res["calibration"]["ece"] == c["ece"].tolist() and res["calibration"]["bin_n"] == c["bin_n"].tolist()
    assert res["risk_coverage"]["coverage"] == s["coverage"].tolist() and res["risk_coverage"]["passes"] == 4
    assert res["risk_coverage"]["unc_auroc"] == s["unc_auroc"].tolist() and res["risk_coverage"]["edges"] == list(ops.DEFAULT_UNC_EDGES)
    ev.write_json(str(tmp_path / "r.json"), res)
    import json
    back = json.load(open(tmp_path / "r.json"))
    assert back["calibration"]["rel"] == pooled_rel.tolist() and back["extra_fields"] == list(cal_names + unc_names)
    ev.write_csv(str(tmp_path / "r.csv"), res)
    rows = list(csv.reader(open(tmp_path / "r.csv")))
    assert rows[0] == ["img_name"] + list(ev.FIELDS + cal_names + unc_names) and len(rows) == 5
    assert all(_same(float(v), res["per_image"][0][k]) for k, v in zip(rows[0][1:], rows[1][1:]))
    assert "cup_cov_0.04" in ev.format_mean(res)


def test_evaluate_refuses_what_it_cannot_do(host):
    batches, logits = sr.eval_batches(2, 2, 128)
    model = sr.standin_model(logits)
    with pytest.raises(ValueError, match="mc_inference_logits"):
        ev.evaluate(model, batches, mc_passes=4)                               # a plain callable has no stochastic passes
    with pytest.raises(ValueError, match="report_edges"):
        ev.evaluate(model, batches, mc_passes=4, mc_logits=_passes(model), report_edges=(0.05,))
    assert host.table_calls == []


def test_command_line_passes_the_flags_on(host, tmp_path, capsys):
    from uda_clr_amd.dataloaders import synthetic
    synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=128)
    argv = ["--data-dir", str(tmp_path), "--dataset", "Drishti-GS", "--checkpoint", "unused", "--batch-size", "2"]

    def model(image):
        grey = (image.mean(1) + 1.0) * 127.5
        return torch.stack([(grey - 165.0), (grey - 110.0)], 1) / 8.0, None
    plain = ev.main(argv, model=model)
    assert host.unc_calls == [] and host.table_calls == [] and "extra_fields" not in plain
    res = ev.main(argv + ["--calibration", "--bins", "12", "--mc-passes", "4", "--csv", str(tmp_path / "c.csv")], model=model, mc_logits=ur.noisy_passes())
    assert "disc_unc_auroc" in capsys.readouterr().out
    assert res["extra_fields"] == ev.CALIBRATION_FIELDS + ev.uncertainty_fields() and res["calibration"]["bins"] == 12
    assert [c[0] for c in host.unc_calls] == [(4, 2, 2, 128, 128), (4, 1, 2, 128, 128)] and all(c[2] is None for c in host.unc_calls)     # no save_dir: no picture
    assert [c["bins"] for c in host.table_calls] == [12, 12] and np.array(res["calibration"]["rel"]).shape == (2, 12, 5)
    assert all(all(_same(r[k], p[k]) for k in p) for r, p in zip(res["per_image"], plain["per_image"]))
    assert list(csv.reader(open(tmp_path / "c.csv")))[0] == ["img_name"] + list(ev.FIELDS + res["extra_fields"])


def test_parsers():
    a = ev.build_parser().parse_args(["--data-dir", "d", "--checkpoint", "c"])
    assert a.calibration is False and a.bins == 15 and a.mc_passes == 0
    a = ev.build_parser().parse_args(["--data-dir", "d", "--checkpoint", "c", "--calibration", "--bins", "20", "--mc-passes", "8"])
    assert a.calibration is True and a.bins == 20 and a.mc_passes == 8
    assert predict.build_parser().parse_args(["--images", "i", "--out", "o"]).mc_passes == 0
    assert predict.build_parser().parse_args(["--images", "i", "--out", "o", "--mc-passes", "8"]).mc_passes == 8


def test_predict_columns_and_csv(host, tmp_path):
    prob, unc, pred, gt = _planes(9)
    pred[1, 0] = False                                                        # an empty cup: nan share
    cols = predict.uncertainty_columns(torch.from_numpy(unc), torch.from_numpy(pred))
    assert tuple(cols) == predict.UNCERTAINTY_COLUMNS == ("cup_unsure", "disc_unsure", "unsure_px")
    call = host.table_calls[0]
    assert call["prob"] is None and call["gt"] is None and call["edges"] == ops.DEFAULT_UNC_EDGES and len(host.table_calls) == 1
    unsure = (unc >= np.float32(0.04)) & pred
    for b in range(2):
        for k, c in enumerate(("cup", "disc")):
            n = int(pred[b, k].sum())
            assert _same(cols[c + "_unsure"][b], int(unsure[b, k].sum()) / n if n else math.nan)
        assert cols["unsure_px"][b] == unsure[b].sum()
    assert math.isnan(cols["cup_unsure"][1]) and 0 < cols["disc_unsure"][0] < 1
    plain = [{"img_name": "a.png", "vcdr_pred": 0.5}]
    predict.write_csv(str(tmp_path / "p.csv"), plain)
    assert list(csv.reader(open(tmp_path / "p.csv"))) == [["img_name", "vcdr_pred"], ["a.png", "0.5"]]
    full = [dict(plain[0], **{k: float(cols[k][0]) for k in predict.UNCERTAINTY_COLUMNS})]
    predict.write_csv(str(tmp_path / "f.csv"), full)
    rows = list(csv.reader(open(tmp_path / "f.csv")))
    assert rows[0] == ["img_name", "vcdr_pred"] + list(predict.UNCERTAINTY_COLUMNS) and [float(v) for v in rows[1][2:]] == [full[0][k] for k in rows[0][2:]]
    both = [dict(full[0], **{k: 1.0 for k in predict.MORPHOMETRY_COLUMNS})]
    predict.write_csv(str(tmp_path / "b.csv"), both)
    assert list(csv.reader(open(tmp_path / "b.csv")))[0] == ["img_name", "vcdr_pred"] + list(predict.MORPHOMETRY_COLUMNS + predict.UNCERTAINTY_COLUMNS)


def test_front_ends_check_before_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m, f = torch.zeros(1, 2, 8, 8, dtype=torch.bool), torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.selective_tables(f, f, m)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mc_uncertainty(torch.zeros(4, 1, 2, 8, 8))
    with pytest.raises(ValueError, match="1..64 bins"):
        ops.selective_tables(f, f, m, bins=65)
    with pytest.raises(ValueError, match="1..64 bins"):
        ops.selective_tables(f, f, m, edges=np.linspace(0.0, 1.0, 64))
    with pytest.raises(ValueError, match="ascending"):
        ops.selective_tables(f, f, m, edges=(0.2, 0.1))
    with pytest.raises(ValueError, match="ascending"):
        ops.selective_tables(f, f, m, edges=(0.1, float("inf")))
    with pytest.raises(ValueError, match="prob .*unc"):
        ops.selective_tables(None, None, m)


def test_binding_and_symbols_exist():
    """fails before the feature: the entry points, their bindings and their declarations"""
    from uda_clr_amd.kernels import SYMBOLS, HipKernels
    assert len(SYMBOLS["uda_mc_uncertainty"][1]) == 10 and len(SYMBOLS["uda_selective_tables"][1]) == 14
    assert callable(getattr(HipKernels, "mc_uncertainty")) and callable(getattr(HipKernels, "selective_tables"))
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    assert callable(getattr(DeepLab, "mc_inference_logits"))
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    assert "uda_mc_uncertainty(" in txt and "uda_selective_tables(" in txt and "uda_mc_stats(" in txt
    lib = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")
    if os.path.exists(lib):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "uda_mc_uncertainty") and hasattr(ctypes.CDLL(lib), "uda_selective_tables")
