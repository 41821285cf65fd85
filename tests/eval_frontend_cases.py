"""The runs of tests/test_eval_frontend_cpu.py and of tests/golden/make_golden_eval_frontend.py, which records their results: evaluate()
and predict on two batches of two 64 x 64 images with every device stage replaced by its host restatement and counted.

``predict.predict`` refuses to start without a device (it has no host path to fall back to), so its two runs go through what it does per
batch once it has one: ``predict.batches`` -> the normalisation -> ``predict.predict_batch`` under no_grad.  The functions used here keep
their signatures across the package's history, so the same file runs on the commit the fixture was recorded on."""
import csv
import json
import os

import numpy as np
import torch

import morphometry_ref as mr
import surface_profile_ref as spr
import surface_ref as sr
import tta_ref
import uncertainty_ref as ur
from kernel_cases import _scipy_postprocess
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict
from uda_clr_amd.utils import Utils, metrics

S, N_BATCHES, BATCH = 64, 2, 2
COUNTED_OPS = ("surface_distances", "surface_profile", "disc_morphometry", "mc_uncertainty", "selective_tables", "tta_view", "tta_fuse")
COUNTED_UTILS = ("postprocessing_batch", "save_per_img_batch", "save_mask_batch", "save_uncertainty_batch")


def _field(cy, cx, a, b):
    """1 at the centre of the ellipse, 0 on its border, negative outside"""
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    return 1.0 - ((y - cy) / a) ** 2 - ((x - cx) / b) ** 2


def eval_batches(seed=5):
    """[{'image', 'map', 'img_name'}]: image channel 0 / 1 holds a smooth cup / disc field (what the pointwise model reads) quantised to
    the 256 levels of a byte, channel 2 noise; the ground truth is a shifted copy, so that there are errors to rank.  The
    fields are wider than the truth (cup semi-axes 9..11, disc 17..20) by what the threshold 0.75 (field > 0.27, 0.85 of the semi-axes)
    and the radius-7 erosion of the post-processing take off again."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(N_BATCHES):
        image, truth = np.zeros((BATCH, 3, S, S), np.float32), np.zeros((BATCH, 2, S, S), np.float32)
        for i in range(BATCH):
            cy, cx = rng.uniform(31, 33, 2)
            for c, (lo, hi) in enumerate(((9, 11), (17, 20))):
                a, d = rng.uniform(lo, hi, 2)
                f = _field(cy, cx, (a + 8) / 0.85, (d + 8) / 0.85) + 0.08 * rng.standard_normal((S, S))
                image[i, c] = np.clip(f, -1.0, 1.0)
                truth[i, c] = _field(cy + rng.uniform(-2, 2), cx + rng.uniform(-2, 2), a * rng.uniform(0.9, 1.1), d * rng.uniform(0.9, 1.1)) > 0
            image[i, 2] = np.clip(0.3 * rng.standard_normal((S, S)), -1.0, 1.0)
        u8 = np.clip(np.rint((image + 1.0) * 127.5), 0, 255).astype(np.uint8)
        out.append({"image": torch.from_numpy(u8.astype(np.float32) / 127.5 - 1.0), "map": torch.from_numpy(truth),
                    "img_name": ["img_%02d.png" % (b * BATCH + i) for i in range(BATCH)], "u8": u8})
    return out


def model(x):
    """pointwise 3 -> 2: every view of an image gives the logits of the image, permuted"""
    return torch.stack([4.0 * x[:, 0] + 0.5 * x[:, 2], 4.0 * x[:, 1] - 0.5 * x[:, 2]], 1), None


def mc_logits(x, T):
    """T 'passes': the model's logits plus seeded noise, larger near the decision boundary so that the std spreads over the bins"""
    lg = model(x)[0]
    g = torch.Generator().manual_seed(100 * T + int(x.shape[0]))
    noise = torch.randn((T,) + tuple(lg.shape), generator=g)
    return (lg[None] + 1.5 * noise * torch.exp(-lg.abs() / 2.0)[None]).contiguous()


def _scipy_batch(prob, threshold=0.75, dataset='G'):
    thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
    return torch.from_numpy(np.stack([_scipy_postprocess(p, thr_cup, thr_disc) for p in prob.cpu().numpy()]))


def _morph(masks, sectors=72):
    table = metrics.sector_table(sectors)
    return dict(mr.integers(masks.cpu().numpy(), table), table=table)


def install(monkeypatch):
    """the host stages in the device stages' places, every one counted -> {name: calls so far}"""
    host, views = ur.HostOps(), tta_ref.HostTta()
    stages = {"surface_distances": sr.surface_distances, "surface_profile": spr.surface_profile, "disc_morphometry": _morph,
              "mc_uncertainty": host.mc_uncertainty, "selective_tables": host.selective_tables, "tta_view": views.tta_view,
              "tta_fuse": views.tta_fuse, "postprocessing_batch": _scipy_batch, "save_per_img_batch": lambda *a, **k: None,
              "save_mask_batch": lambda *a, **k: None, "save_uncertainty_batch": lambda *a, **k: None}
    counts = dict.fromkeys(COUNTED_OPS + COUNTED_UTILS, 0)

    def counted(name, fn):
        def call(*a, **k):
            counts[name] += 1
            return fn(*a, **k)
        return call
    for name in COUNTED_OPS:
        monkeypatch.setattr(ops, name, counted(name, stages[name]))
    for name in COUNTED_UTILS:
        monkeypatch.setattr(Utils, name, counted(name, stages[name]))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    return counts


def _per_batch(counts, before):
    per = {k: (counts[k] - before[k]) / N_BATCHES for k in counts}
    assert all(v == int(v) for v in per.values()), per
    return {k: int(v) for k, v in per.items() if v}


def run_evaluate(counts, tmp, batches, **options):
    """-> {'json': write_json's file read back, 'csv': write_csv's rows, 'calls': calls per batch}"""
    before = dict(counts)
    res = ev.evaluate(model, batches, **options)
    calls = _per_batch(counts, before)
    ev.write_json(os.path.join(tmp, "r.json"), res)
    ev.write_csv(os.path.join(tmp, "r.csv"), res)
    with open(os.path.join(tmp, "r.json")) as f, open(os.path.join(tmp, "r.csv"), newline="") as g:
        return {"json": json.load(f), "csv": list(csv.reader(g)), "calls": calls}


def run_predict(counts, tmp, batches, **options):
    """-> {'rows': predict's rows, 'csv': predict.write_csv's rows, 'calls': calls per batch}"""
    before = dict(counts)
    images = [(n, a) for b in batches for n, a in zip(b["img_name"], np.ascontiguousarray(b["u8"].transpose(0, 2, 3, 1)))]
    rows = []
    with torch.no_grad():
        for names, u8 in predict.batches(images, BATCH):
            u8 = torch.from_numpy(u8)
            x = (u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()
            rows += predict.predict_batch(model, u8, x, names, os.path.join(tmp, "out"), **options)[0]
    calls = _per_batch(counts, before)
    predict.write_csv(os.path.join(tmp, "p.csv"), rows)
    with open(os.path.join(tmp, "p.csv"), newline="") as g:
        return {"rows": rows, "csv": list(csv.reader(g)), "calls": calls}


EVALUATE_RUNS = {"evaluate_mc": dict(hd95=True, tolerances=(2,), cdr=True, morphometry=True, calibration=True, mc_passes=3, mc_logits=mc_logits),
                 "evaluate_tta": dict(tta="flips", tta_uncertainty=True)}
PREDICT_RUNS = {"predict_mc": dict(dataset="G", morphometry=True, mc_passes=3, mc_logits=mc_logits),
                "predict_tta": dict(dataset="G", tta="flips", tta_uncertainty=True)}


def run_all(monkeypatch, tmp):
    """every run of the fixture, in its order -> {run: result}"""
    counts = install(monkeypatch)
    batches = eval_batches()
    out = {name: run_evaluate(counts, tmp, batches, **o) for name, o in EVALUATE_RUNS.items()}
    out.update({name: run_predict(counts, tmp, batches, **o) for name, o in PREDICT_RUNS.items()})
    return out
