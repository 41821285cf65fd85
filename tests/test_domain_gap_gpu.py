"""-m gpu: the domain-gap report (uda_clr_amd/domain_gap.py) on the device: streaming moments of a stub generator against the float64
moments of the concatenated batches, the three weight sources against ``ops.gen_prototype``, the report's intra_loss against
``ops.proto_align``, and the command line on a real MobileNetV2 DeepLab.

The covariance bound.  The accumulator holds S about a fixed centre a (the first batch's fp32 centroids) and W, and finalize() forms
cov = S / W - d d^T, d = mu - a.  Per entry
    |cov - cov64| <= gamma_n A_ij(a) / W                        the kernel's bound (tests/test_proto_scatter_gpu.py), per batch, added
                   + MEAN_TOL |S64_ij(a)| / W                   W from uda_proto_reduce (fp32 per workgroup, fp64 across)
                   + |d_i| e_j + |d_j| e_i + e_i e_j            the shift with a mean that is off by e = MEAN_TOL max|mu|
with MEAN_TOL = 1e-6, the relative tolerance this file holds the means (and the weight totals) to."""
import os
import re

import numpy as np
import pytest
import torch

import scatter_ref as sr
from uda_clr_amd import domain_gap as dg
from uda_clr_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "uda_clr_amd", "csrc", "scatter_plan.h")) as _f:
    PS_SLAB = int(re.search(r"^#define\s+PS_SLAB\s+(\d+)\b", _f.read(), re.M).group(1))
GAMMA = sr.gamma(PS_SLAB + 4)
MEAN_TOL = 1e-6
C, FH, S = 305, 16, 64          # feature channels, feature side, image side


class StubGenerator(object):
    """a callable with DeepLab's 7 outputs that replays prepared (feature, o_before) pairs, one per call"""
    def __init__(self, pairs):
        self.pairs, self.i = pairs, 0

    def __call__(self, image):
        feat, o = self.pairs[self.i]
        self.i += 1
        assert image.shape[0] == feat.shape[0]
        full = torch.zeros(feat.shape[0], 2, S, S, device=DEV)
        return full, full[:, :1], None, None, feat.to(DEV), o.to(DEV), None


def _batch(B, g, empty_cup=False):
    """a label map [B,2,S,S] (cup inside disc, rectangles), features [B,C,FH,FH] whose class means differ, mean ten times the
    spread, and logits o_before that follow the labels softly"""
    m = torch.zeros(B, 2, S, S)
    for b in range(B):
        y, x = (int(v) for v in torch.randint(8, 24, (2,), generator=g))
        m[b, 1, y:y + 32, x:x + 28] = 1.0
        if not empty_cup:
            m[b, 0, y + 8:y + 20, x + 8:x + 24] = 1.0
    small = m[:, :, ::S // FH, ::S // FH]                                       # F.interpolate(mode='nearest'): src = floor(dst * 4)
    feat = 3.0 + 0.3 * torch.randn(B, C, FH, FH, generator=g) + 0.2 * small[:, :1] - 0.15 * small[:, 1:]
    o = 4.0 * (small - 0.5) + torch.randn(B, 2, FH, FH, generator=g)
    return {"image": torch.zeros(B, 3, S, S), "map": m}, feat, o


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _label_weights(samples):
    m = torch.cat([_rows(s["map"][:, :, ::S // FH, ::S // FH]) for s in samples])
    return torch.cat([m, 1.0 - m], 1)


def _moments(samples, pairs, weights="labels", monkeypatch=None):
    """dg.domain_moments over the stub, and the fp32 centre its accumulator used"""
    seen = {}
    real = dg.MomentAccumulator.finalize

    def finalize(self):
        seen["centre"] = self.centre.cpu()
        return real(self)
    monkeypatch.setattr(dg.MomentAccumulator, "finalize", finalize)
    return dg.domain_moments(StubGenerator(pairs), samples, weights=weights), seen["centre"]


def _check_against_fp64(got, centre, feats, wts):
    """means to MEAN_TOL, covariances within the derived bound of the module docstring; feats / wts: per-batch rows
    -> (that bound per covariance entry [4, C, C], the bound of a mean entry)"""
    allf, allw = torch.cat(feats), torch.cat(wts)
    count, mean, cov = sr.moments64(allf, allw)
    np.testing.assert_allclose(got["count"], count.numpy(), rtol=MEAN_TOL)
    scale = float(mean.abs().max())
    assert np.abs(got["mean"] - mean.numpy()).max() <= MEAN_TOL * scale
    absum = sum(sr.abs_scatter64(f, w, centre) for f, w in zip(feats, wts))
    s64 = sr.scatter64(allf, allw, centre)
    d = (mean - centre.double()).abs()
    e = MEAN_TOL * scale
    shift = e * (d[:, :, None] + d[:, None, :]) + e * e
    bound = (GAMMA * absum + MEAN_TOL * s64.abs()) / count[:, None, None] + shift
    err = np.abs(got["cov"] - cov.numpy())
    worst = float((torch.from_numpy(err) / bound).max())
    print("max |cov - cov64| / bound = %.3e" % worst)
    assert worst <= 1.0
    return bound.numpy(), MEAN_TOL * scale


def test_streaming_equals_fp64_moments_of_the_concatenation(monkeypatch):
    g = torch.Generator().manual_seed(11)
    batches = [_batch(B, g) for B in (3, 3, 1)]                                 # the last batch is smaller
    samples, pairs = [b[0] for b in batches], [(b[1], b[2]) for b in batches]
    got, centre = _moments(samples, pairs, monkeypatch=monkeypatch)
    assert got["mean"].shape == (4, C) and got["cov"].shape == (4, C, C) and got["cov"].dtype == np.float64
    first = sr.moments64(_rows(pairs[0][0]), _label_weights(samples[:1]))[1]
    assert float((centre.double() - first).abs().max()) <= 1e-5 * float(first.abs().max())       # the centre is the first batch's centroids
    _check_against_fp64(got, centre, [_rows(p[0]) for p in pairs], [_label_weights([s]) for s in samples])
    assert np.array_equal(got["cov"], got["cov"].transpose(0, 2, 1))


def test_empty_class_in_the_first_batch_gives_the_same_moments(monkeypatch):
    g = torch.Generator().manual_seed(12)
    batches = [_batch(2, g), _batch(2, g, empty_cup=True), _batch(1, g)]
    results = []
    for order in ((0, 1, 2), (1, 0, 2)):                                        # with and without the cup-less batch first
        samples, pairs = [batches[i][0] for i in order], [(batches[i][1], batches[i][2]) for i in order]
        got, centre = _moments(samples, pairs, monkeypatch=monkeypatch)
        bound, mean_bound = _check_against_fp64(got, centre, [_rows(p[0]) for p in pairs], [_label_weights([s]) for s in samples])
        results.append((got, centre, bound, mean_bound))
    (a, centre_a, bound_a, mean_a), (b, centre_b, bound_b, mean_b) = results
    assert bool((centre_b[0] == 0).all()) and not bool((centre_a[0] == 0).any())                  # cup_obj: zero centre only when empty first
    assert bool((centre_b[1:] != 0).all())
    # the two orders against each other: each is within its own bound of the same fp64 moments, so they differ by at most the sum
    np.testing.assert_allclose(a["count"], b["count"], rtol=2 * MEAN_TOL)
    assert np.abs(a["mean"] - b["mean"]).max() <= mean_a + mean_b
    ratio = float((np.abs(a["cov"] - b["cov"]) / (bound_a + bound_b)).max())
    print("max |cov(cup-less batch first) - cov(other order)| / (sum of the two bounds) = %.3e" % ratio)
    assert ratio <= 1.0


@pytest.mark.parametrize("weights", ["soft", "hard"])
def test_predicted_weights_are_what_gen_prototype_is_given(weights, monkeypatch):
    g = torch.Generator().manual_seed(13)
    sample, feat, o = _batch(3, g)
    got, _ = _moments([sample], [(feat, o)], weights=weights, monkeypatch=monkeypatch)
    prob = torch.sigmoid(o.to(DEV))
    pred = prob if weights == "soft" else (prob > 0.75).float()
    want = ops.gen_prototype(pred, feat.to(DEV)).matrix.double().cpu().numpy()
    assert np.abs(got["mean"] - want).max() <= 1e-5 * np.abs(want).max()
    if weights == "hard":
        assert got["count"][0] == float((pred[:, 0] > 0.5).sum()) and got["count"][0] + got["count"][2] == pred[:, 0].numel()


def test_intra_loss_is_the_trainers(monkeypatch):
    g = torch.Generator().manual_seed(14)
    (s_src, f_src, o_src), (s_tgt, f_tgt, o_tgt) = _batch(3, g), _batch(2, g)
    f_tgt = f_tgt + 0.05 * torch.randn(1, C, 1, 1, generator=g)                # a domain shift
    src, _ = _moments([s_src], [(f_src, o_src)], monkeypatch=monkeypatch)
    tgt, _ = _moments([s_tgt], [(f_tgt, o_tgt)], weights="soft", monkeypatch=monkeypatch)
    report = dg.gap_report(src, tgt)
    cur_src = ops.gen_prototype_from_labels(s_src["map"].to(DEV), f_src.to(DEV))
    cur_tgt = ops.gen_prototype(torch.sigmoid(o_tgt.to(DEV)), f_tgt.to(DEV))
    intra = float(ops.proto_align(cur_src, cur_tgt, None, None, 0.3)[0])
    assert intra > 0 and abs(report["intra_loss"] - intra) <= 1e-5 * intra
    assert report["n_empty"] == 0


def test_command_line_on_a_real_deeplab(tmp_path):
    import json
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    torch.manual_seed(21)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(DEV)
    g = torch.Generator().manual_seed(22)

    def loader(n):
        out = []
        for _ in range(n):
            sample, _, _ = _batch(2, g)
            sample["image"] = torch.randn(2, 3, S, S, generator=g)
            out.append(sample)
        return out
    src, tgt = loader(2), loader(1)
    argv = ["--data-dir", "unused", "--checkpoint", "unused", "--json", str(tmp_path / "r.json"), "--csv", str(tmp_path / "r.csv")]
    report = dg.main(argv + ["--target-weights", "soft"], model=model, loaders=(src, tgt))
    assert report["channels"] == C and model.training                         # left in the mode it was found in
    nan_classes = 0
    for name in dg.CLASSES:
        row = report["classes"][name]
        empty = not (row["n_src"] > 0 and row["n_tgt"] > 0)
        nan_classes += empty
        for k, v in row.items():
            assert np.isfinite(v) or (empty and np.isnan(v)), (name, k, v)
        assert empty or row["frechet"] >= 0.0
    assert report["n_empty"] >= nan_classes and (nan_classes > 0 or np.isfinite(report["intra_loss"]))
    for name, o, b in dg.STRUCTURES:                                         # a structure's field may be NaN only with one of ITS classes empty there
        for dom in ("src", "tgt"):
            empty = not (report["classes"][dg.CLASSES[o]]["n_" + dom] > 0 and report["classes"][dg.CLASSES[b]]["n_" + dom] > 0)
            for field in ("separation_", "fisher_"):
                v = report["structures"][name][field + dom]
                assert np.isfinite(v) or (empty and np.isnan(v)), (name, field + dom, v)
    with open(tmp_path / "r.json") as f:
        assert json.load(f)["channels"] == C
    with open(tmp_path / "r.csv") as f:
        assert len(f.read().strip().splitlines()) == 5
    # a domain against itself: no prototype distance, no Frechet distance
    same = dg.main(argv, model=model, loaders=(src, src))
    for name in dg.CLASSES:
        row = same["classes"][name]
        assert row["n_src"] > 0 and row["proto_mse"] == 0.0
        assert 0.0 <= row["frechet"] < 1e-6 * row["compact_src"] * C, (name, row)
