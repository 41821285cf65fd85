"""The host half of the domain-gap report (uda_clr_amd/domain_gap.py) without a GPU: the Frechet distance, the shift identity of
``MomentAccumulator.finalize``'s host math, the report's fields, the command line with injected fakes, and the slab constant of
csrc/scatter_plan.h."""
import csv
import json
import os
import re

import numpy as np
import pytest
import torch

from uda_clr_amd import domain_gap as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rng(seed):
    return np.random.default_rng(seed)


def _spd(C, rng, n=None):
    x = rng.standard_normal((n or 4 * C, C)) * rng.uniform(0.5, 2.0, C)
    x -= x.mean(0)
    return x.T @ x / x.shape[0]


# ------------------------------------------------------------------------------------------------------------ frechet_distance
def test_frechet_diagonal_closed_form():
    rng = _rng(0)
    C = 17
    a, b = rng.uniform(0.1, 3.0, C), rng.uniform(0.1, 3.0, C)
    m1, m2 = rng.standard_normal(C), rng.standard_normal(C)
    want = ((m1 - m2) ** 2).sum() + ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    got = dg.frechet_distance(m1, np.diag(a), m2, np.diag(b))
    assert abs(got - want) <= 1e-10 * want


def test_frechet_symmetric_and_zero_on_itself():
    rng = _rng(1)
    C = 12
    c1, c2 = _spd(C, rng), _spd(C, rng)
    m1, m2 = rng.standard_normal(C), rng.standard_normal(C)
    d12, d21 = dg.frechet_distance(m1, c1, m2, c2), dg.frechet_distance(m2, c2, m1, c1)
    assert d12 > 0 and abs(d12 - d21) <= 1e-9 * d12
    self_d = dg.frechet_distance(m1, c1, m1, c1)
    assert 0.0 <= self_d <= 1e-9 * np.trace(c1)


def test_frechet_rank_deficient_is_finite():
    rng = _rng(2)
    C = 20
    c1, c2 = _spd(C, rng, n=7), _spd(C, rng, n=5)            # fewer samples than channels: singular covariances
    assert np.linalg.matrix_rank(c1) < C
    d = dg.frechet_distance(rng.standard_normal(C), c1, rng.standard_normal(C), c2)
    assert np.isfinite(d) and d >= 0.0
    assert dg.frechet_distance(np.zeros(C), c1, np.zeros(C), c1) >= 0.0


def test_frechet_nan_propagates():
    rng = _rng(3)
    C = 5
    c = _spd(C, rng)
    m = rng.standard_normal(C)
    bad_c, bad_m = c.copy(), m.copy()
    bad_c[1, 2] = np.nan
    bad_m[0] = np.nan
    assert np.isnan(dg.frechet_distance(m, bad_c, m, c))
    assert np.isnan(dg.frechet_distance(m, c, m, bad_c))
    assert np.isnan(dg.frechet_distance(bad_m, c, m, c))
    assert np.isnan(dg.frechet_distance(m, c, bad_m, c))


# ------------------------------------------------------------------------------------------------------------ shift identity
def _sums_about(f, w, centre):
    C = f.shape[1]
    sums = np.zeros((4, C + 1))
    scatter = np.zeros((4, C, C))
    for k in range(4):
        sums[k, :C], sums[k, C] = w[:, k] @ f, w[:, k].sum()
        d = f - centre[k]
        scatter[k] = (d * w[:, k:k + 1]).T @ d
    return sums, scatter


def test_shift_identity_any_centre_gives_the_same_moments():
    rng = _rng(4)
    P, C = 400, 9
    f = rng.standard_normal((P, C)) * 0.3 + 3.0             # mean ten times the spread
    w = rng.uniform(0.0, 1.0, (P, 4))
    true_mean = (w.T @ f) / w.sum(0)[:, None]
    results = [dg.moments_from_sums(*_sums_about(f, w, c), c)
               for c in (np.zeros((4, C)), true_mean, true_mean + 50.0)]
    ref = results[1]
    for k in range(4):                                      # about the true mean the shift term vanishes: the plain definition
        d = f - true_mean[k]
        np.testing.assert_allclose(ref["cov"][k], (d * w[:, k:k + 1]).T @ d / w[:, k].sum(), rtol=0, atol=1e-12)
    for r in results:
        np.testing.assert_allclose(r["count"], w.sum(0), rtol=1e-14)
        for k in range(4):
            tr = np.trace(ref["cov"][k])
            assert np.abs(r["mean"][k] - ref["mean"][k]).max() <= 1e-9 * tr
            assert np.abs(r["cov"][k] - ref["cov"][k]).max() <= 1e-9 * tr


def test_empty_class_has_nan_moments():
    rng = _rng(5)
    f, w = rng.standard_normal((30, 4)), rng.uniform(0, 1, (30, 4))
    w[:, 2] = 0.0
    m = dg.moments_from_sums(*_sums_about(f, w, np.zeros((4, 4))), np.zeros((4, 4)))
    assert m["count"][2] == 0 and np.isnan(m["mean"][2]).all() and np.isnan(m["cov"][2]).all()
    assert np.isfinite(m["mean"][[0, 1, 3]]).all() and np.isfinite(m["cov"][[0, 1, 3]]).all()


# ------------------------------------------------------------------------------------------------------------ gap_report
def _moments(seed, C=6, empty=()):
    rng = _rng(seed)
    m = {"count": rng.uniform(10, 100, 4), "mean": rng.standard_normal((4, C)), "cov": np.stack([_spd(C, rng) for _ in range(4)])}
    for k in empty:
        m["count"][k], m["mean"][k], m["cov"][k] = 0.0, np.nan, np.nan
    return m


def test_gap_report_fields_and_intra_loss():
    src, tgt = _moments(6), _moments(7)
    rep = dg.gap_report(src, tgt)
    assert set(rep) == {"classes", "structures", "intra_loss", "n_empty", "channels"}
    assert tuple(rep["classes"]) == ("cup_obj", "disc_obj", "cup_bck", "disc_bck")
    for k, name in enumerate(dg.CLASSES):
        row = rep["classes"][name]
        assert set(row) == {"n_src", "n_tgt", "proto_mse", "proto_cos", "compact_src", "compact_tgt", "frechet"}
        assert row["n_src"] == src["count"][k] and row["n_tgt"] == tgt["count"][k]
        np.testing.assert_allclose(row["proto_mse"], np.mean((src["mean"][k] - tgt["mean"][k]) ** 2), rtol=1e-14)
        np.testing.assert_allclose(row["compact_src"], np.trace(src["cov"][k]) / 6, rtol=1e-14)
        np.testing.assert_allclose(row["compact_tgt"], np.trace(tgt["cov"][k]) / 6, rtol=1e-14)
        assert -1.0 <= row["proto_cos"] <= 1.0 and row["frechet"] >= 0.0
    assert set(rep["structures"]) == {"cup", "disc"}
    for name, o, b in (("cup", 0, 2), ("disc", 1, 3)):
        row = rep["structures"][name]
        assert set(row) == {"separation_src", "separation_tgt", "fisher_src", "fisher_tgt"}
        d = src["mean"][o] - src["mean"][b]
        np.testing.assert_allclose(row["separation_src"], np.mean(d * d), rtol=1e-14)
        np.testing.assert_allclose(row["fisher_src"], d @ d / (np.trace(src["cov"][o]) + np.trace(src["cov"][b])), rtol=1e-14)
    np.testing.assert_allclose(rep["intra_loss"], sum(rep["classes"][n]["proto_mse"] for n in dg.CLASSES), rtol=1e-15)
    assert rep["n_empty"] == 0 and rep["channels"] == 6


def test_gap_report_empty_class_is_nan_and_counted():
    rep = dg.gap_report(_moments(8), _moments(9, empty=(0,)))
    row = rep["classes"]["cup_obj"]
    assert rep["n_empty"] == 1 and row["n_tgt"] == 0
    for k in ("proto_mse", "proto_cos", "compact_tgt", "frechet"):
        assert np.isnan(row[k]), k
    assert np.isfinite(row["compact_src"])
    assert np.isnan(rep["structures"]["cup"]["fisher_tgt"]) and np.isfinite(rep["structures"]["cup"]["fisher_src"])
    assert np.isfinite(rep["structures"]["disc"]["fisher_tgt"])
    assert np.isnan(rep["intra_loss"])
    assert all(np.isfinite(v) for v in rep["classes"]["disc_obj"].values())


def test_json_file_is_standard_json_with_null_for_nan(tmp_path):
    rep = dg.gap_report(_moments(8), _moments(9, empty=(0,)))
    dg.write_json(tmp_path / "r.json", rep)
    with open(tmp_path / "r.json") as f:
        text = f.read()
    assert "NaN" not in text
    back = json.loads(text, parse_constant=lambda c: pytest.fail("non-standard constant %s" % c))
    assert back["classes"]["cup_obj"]["frechet"] is None and back["intra_loss"] is None and back["n_empty"] == 1
    assert back["classes"]["disc_obj"] == rep["classes"]["disc_obj"]


# ------------------------------------------------------------------------------------------------------------ command line
def test_parser_accepts_the_documented_arguments():
    args = dg.build_parser().parse_args(
        ["--data-dir", "d", "--source", "REFUGE", "--target", "Drishti-GS", "--source-split", "train", "--target-split", "test",
         "--checkpoint", "c.pth", "--backbone", "drn", "--out-stride", "8", "--use_TN", "--batch-size", "4",
         "--target-weights", "hard", "--threshold", "0.6", "--json", "r.json", "--csv", "r.csv"])
    assert (args.source, args.target, args.source_split, args.target_split) == ("REFUGE", "Drishti-GS", "train", "test")
    assert (args.backbone, args.out_stride, args.use_TN, args.batch_size) == ("drn", 8, True, 4)
    assert (args.target_weights, args.threshold, args.json, args.csv) == ("hard", 0.6, "r.json", "r.csv")
    with pytest.raises(SystemExit):
        dg.build_parser().parse_args(["--data-dir", "d", "--checkpoint", "c", "--target-weights", "other"])


def test_main_with_injected_fakes_writes_json_and_csv(tmp_path, monkeypatch):
    """no device call: the model is a plain callable, the class weights and MomentAccumulator.update are host stand-ins"""
    C, h = 5, 4
    g = torch.Generator().manual_seed(0)
    seen = []

    def model(image):
        B = image.shape[0]
        feat = image.mean(1, keepdim=True)[:, :, :h, :h] + torch.arange(C, dtype=torch.float32).view(1, C, 1, 1)
        return (None, None, None, None, feat, torch.zeros(B, 2, h, h), None)

    def fake_weights(sample_map, o_before, weights="labels", threshold=0.75):
        seen.append(weights)
        m = sample_map[:, :, :h, :h].permute(0, 2, 3, 1).reshape(-1, 2)
        return torch.cat([m, 1 - m], 1)

    def fake_update(self, feature, wts):
        f = feature.permute(0, 2, 3, 1).reshape(-1, self.C).double()
        w = wts.double()
        if self.sums is None:
            self.sums = torch.zeros(4, self.C + 1, dtype=torch.float64)
            self.scatter = torch.zeros(4, self.C, self.C, dtype=torch.float64)
            self.centre = torch.zeros(4, self.C)
        self.sums[:, :self.C] += w.t() @ f
        self.sums[:, self.C] += w.sum(0)
        self.scatter += torch.einsum("pk,pi,pj->kij", w, f, f)

    monkeypatch.setattr(dg, "class_weights", fake_weights)
    monkeypatch.setattr(dg.MomentAccumulator, "update", fake_update)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)

    def loader(n):
        return [{"image": torch.randn(b, 3, 8, 8, generator=g), "map": (torch.rand(b, 2, 8, 8, generator=g) > 0.5).float()} for b in n]

    jp, cp = tmp_path / "r.json", tmp_path / "r.csv"
    rep = dg.main(["--data-dir", "unused", "--checkpoint", "unused", "--target-weights", "soft", "--json", str(jp), "--csv", str(cp)],
                  model=model, loaders=(loader((2, 1)), loader((3,))))
    assert seen == ["labels", "labels", "soft"]                 # source weights are always the labels
    with open(jp) as f:
        back = json.load(f)
    assert back["intra_loss"] == rep["intra_loss"] and back["target_weights"] == "soft" and set(back["classes"]) == set(dg.CLASSES)
    with open(cp) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["class"] + list(dg.CLASS_FIELDS)
    assert [r[0] for r in rows[1:]] == list(dg.CLASSES) and all(len(r) == len(rows[0]) for r in rows)
    assert float(rows[1][rows[0].index("frechet")]) == rep["classes"]["cup_obj"]["frechet"]


# ------------------------------------------------------------------------------------------------------------ the plan header
def test_ps_slab_parses_and_is_in_range():
    with open(os.path.join(ROOT, "uda_clr_amd", "csrc", "scatter_plan.h")) as f:
        m = re.search(r"^#define\s+PS_SLAB\s+(\d+)\b", f.read(), re.M)
    assert m, "scatter_plan.h must define PS_SLAB as a plain number"
    assert 1 <= int(m.group(1)) <= 65536
