"""not-gpu: the evaluation front end keeps what it computed, how often it calls each stage, and where every packed table lies.

  recorded results  evaluate() and predict on the runs of tests/eval_frontend_cases.py (host stages in the device stages' places) against
                    tests/golden/eval_frontend.json, recorded by tests/golden/make_golden_eval_frontend.py before the probability stage
                    moved to uda_clr_amd/inference.py: names, order, integers and strings exactly, NaN only where the fixture has NaN, floats
                    within 1e-12 relative - they are float64 closed forms of integer tables, the margin allows for another libm only
  calls per batch   the "ONE call per batch" promises of the docstrings, as numbers
  layouts           the four packed tables: views disjoint and covering, sizes as the literals the bindings used to carry, and the host
                    helper giving back what the device helper laid out"""
import json
import math
import os

import numpy as np
import pytest
import torch

import eval_frontend_cases as cases
from uda_clr_amd import evaluate as ev
from uda_clr_amd import inference, kernels, predict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_frontend.json")

# calls per batch, counted on the commit the fixture was recorded on by the same wrapping (tests/eval_frontend_cases.install)
CALLS = {
    "evaluate_mc": {"postprocessing_batch": 1, "surface_profile": 1, "disc_morphometry": 1, "mc_uncertainty": 1, "selective_tables": 1},
    "evaluate_tta": {"postprocessing_batch": 1, "surface_distances": 1, "tta_view": 4, "tta_fuse": 1, "selective_tables": 1},
    "predict_mc": {"postprocessing_batch": 1, "surface_profile": 1, "disc_morphometry": 1, "mc_uncertainty": 1, "selective_tables": 1,
                   "save_per_img_batch": 1, "save_mask_batch": 1, "save_uncertainty_batch": 1},
    "predict_tta": {"postprocessing_batch": 1, "surface_profile": 1, "tta_view": 4, "tta_fuse": 1, "selective_tables": 1,
                    "save_per_img_batch": 1, "save_mask_batch": 1, "save_uncertainty_batch": 1},
}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    patch = pytest.MonkeyPatch()
    try:
        yield cases.run_all(patch, str(tmp_path_factory.mktemp("eval_frontend")))
    finally:
        patch.undo()


def _same(got, want, where):
    if isinstance(want, dict):
        assert isinstance(got, dict) and list(got) == list(want), where
        for k in want:
            _same(got[k], want[k], "%s[%r]" % (where, k))
    elif isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "%s[%d]" % (where, i))
    elif isinstance(want, float):
        assert isinstance(got, float), where
        if math.isnan(want) or math.isnan(got):
            assert math.isnan(want) and math.isnan(got), (where, got, want)
        else:
            assert got == want or abs(got - want) <= 1e-12 * abs(want), (where, got, want)
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


def _same_csv(got, want, where):
    """header and names exactly; the figures are repr(float)"""
    assert got[0] == want[0] and len(got) == len(want), where
    for r, (g, w) in enumerate(zip(got[1:], want[1:])):
        assert g[0] == w[0] and len(g) == len(w), (where, r)
        _same([float(v) for v in g[1:]], [float(v) for v in w[1:]], "%s row %d" % (where, r))


# ------------------------------------------------------------------------------------------------------------ recorded results
@pytest.mark.parametrize("name", ["evaluate_mc", "evaluate_tta", "predict_mc", "predict_tta"])
def test_results_are_the_recorded_ones(runs, name):
    with open(GOLDEN) as f:
        want = json.load(f)[name]
    got = json.loads(json.dumps(runs[name]))                                  # tuples as lists, as the fixture went through JSON
    assert list(got) == list(want)
    for part in ("json", "rows"):
        if part in want:
            _same(got[part], want[part], "%s.%s" % (name, part))
    _same_csv(got["csv"], want["csv"], name + ".csv")
    assert len(got["csv"]) == 1 + cases.N_BATCHES * cases.BATCH


def test_the_runs_are_not_degenerate(runs):
    """the fixture pins something: every figure of the first run is finite and strictly inside its range, the passes spread the std over
    the bins, and the views of a pointwise model agree"""
    mc, tta = runs["evaluate_mc"]["json"], runs["evaluate_tta"]["json"]
    assert mc["extra_fields"] == list(ev.extra_fields(True, (2.0,), True, True, True, 3)) and mc["risk_coverage"]["passes"] == 3
    assert all(math.isfinite(v) for v in mc["mean"].values()) and 0.5 < mc["mean"]["cup_dice"] < 1 and 0 < mc["mean"]["cup_cov_0.04"] < 1
    assert tta["tta"] == [[g, cases.S, cases.S] for g in range(4)] and tta["risk_coverage"]["views"] == 4 and tta["mean"]["cup_cov_0.04"] == 1.0
    assert all(tta["mean"][k] == mc["mean"][k] for k in ev.FIELDS)            # flips of a pointwise model: the same probabilities
    assert [r["img_name"] for r in runs["predict_mc"]["rows"]] == ["img_%02d.png" % i for i in range(4)]
    assert runs["predict_mc"]["csv"][0] == ["img_name", "vcdr_pred"] + list(predict.MORPHOMETRY_COLUMNS + predict.UNCERTAINTY_COLUMNS)
    assert runs["predict_tta"]["csv"][0] == ["img_name", "vcdr_pred"] + list(predict.UNCERTAINTY_COLUMNS)


# ------------------------------------------------------------------------------------------------------------- calls per batch
@pytest.mark.parametrize("name", sorted(CALLS))
def test_calls_per_batch(runs, name):
    assert runs[name]["calls"] == CALLS[name]


def test_pictures_cost_evaluate_three_calls_and_change_no_figure(runs, tmp_path, monkeypatch):
    """with save_dir the same stage calls plus the three writers, and the quantised std only then"""
    counts = cases.install(monkeypatch)
    asked = []
    fuse = cases.ops.tta_fuse
    monkeypatch.setattr(cases.ops, "tta_fuse", lambda logits, views, size, outputs=("mean",), u8_scale=None:
                        (asked.append(u8_scale), fuse(logits, views, size, outputs, u8_scale))[1])
    got = cases.run_evaluate(counts, str(tmp_path), cases.eval_batches(), save_dir=str(tmp_path / "pictures"), **cases.EVALUATE_RUNS["evaluate_tta"])
    assert got["calls"] == dict(CALLS["evaluate_tta"], save_per_img_batch=1, save_mask_batch=1, save_uncertainty_batch=1)
    assert asked == [inference.UNCERTAINTY_U8_SCALE] * cases.N_BATCHES == [ev.UNCERTAINTY_U8_SCALE] * cases.N_BATCHES
    _same(got["json"], runs["evaluate_tta"]["json"], "with save_dir")
    del asked[:]
    cases.run_evaluate(counts, str(tmp_path), cases.eval_batches(), **cases.EVALUATE_RUNS["evaluate_tta"])
    assert asked == [None] * cases.N_BATCHES


# --------------------------------------------------------------------------------------------------------- the shared stage
class _Net(torch.nn.Module):
    def forward(self, x):
        return x[:, :2], None


def test_eval_mode_puts_back_what_it_found():
    training, resting, plain = _Net().train(), _Net().eval(), (lambda x: x)
    with inference.eval_mode(training, resting, plain, training):
        assert not training.training and not resting.training and not torch.is_grad_enabled()
    assert training.training and not resting.training and torch.is_grad_enabled()
    with pytest.raises(KeyError):
        with inference.eval_mode(training):
            raise KeyError("inside")
    assert training.training
    assert inference.first_output((1, 2)) == 1 and inference.first_output([3]) == 3 and inference.first_output(4) == 4


def test_argument_checks_are_the_shared_ones(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    assert predict.check_tta is inference.check_uncertainty_args and predict.resolve_mc_logits is inference.resolve_mc_logits
    passes = lambda x, T: None
    assert inference.resolve_mc_logits(None, 0, None) is None and inference.resolve_mc_logits(None, 3, passes) is passes
    with pytest.raises(ValueError, match="mc_inference_logits"):
        inference.resolve_mc_logits(lambda x: x, 3, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                # why the predict runs above go batch by batch
        predict.predict(cases.model, [], "unused", mc_passes=3, mc_logits=passes)


# --------------------------------------------------------------------------------------------------------------------- layouts
def _layout_cases():
    for B in (1, 3):
        yield "surface B%d" % B, kernels.surface_layout(B), ["table", "counts"], [B * 12, B * 6]
        for Q in (0, 2):
            for T in (0, 2):
                yield ("profile B%d Q%d T%d" % (B, Q, T), kernels.profile_layout(B, Q, T), ["table", "counts", "order", "within", "extent"],
                       [B * 12, B * 6, B * 12 * Q, B * 4 * T, B * 8])
        K = 8
        yield "morphometry B%d" % B, kernels.morphometry_layout(B, K), ["moments", "extent", "overlap", "radial"], [B * 12, B * 8, B, B * 2 * K]
        for M in (1, 15):
            for prob, unc in ((False, True), (True, False), (True, True)):
                names = ["rel"] * prob + ["risk"] * unc + ["invalid"]
                sizes = [B * 2 * M * 5] * prob + [B * 2 * K * 4] * unc + [B * 4]
                yield "selective B%d M%d %s" % (B, M, "+".join(names)), kernels.selective_layout(B, M, K, prob, unc), names, sizes


@pytest.mark.parametrize("name,layout,names,sizes", list(_layout_cases()), ids=[c[0] for c in _layout_cases()])
def test_layouts(name, layout, names, sizes):
    packed, views = kernels.packed_views(layout, "cpu")
    assert list(views) == names == [field for field, _, _ in layout] and [v.numel() for v in views.values()] == sizes
    assert packed.dtype == torch.int64 and packed.dim() == 1 and packed.numel() == sum(sizes)
    at = packed.data_ptr()
    for v in views.values():                                                  # in order, back to back, from the first word to the last
        assert v.is_contiguous() and v.element_size() == 8 and (v.numel() == 0 or v.data_ptr() == at)
        at += 8 * v.numel()
    assert at == packed.data_ptr() + 8 * packed.numel()
    packed.copy_(torch.arange(packed.numel()))
    host = kernels.unpack_host(layout, packed.numpy().copy())
    assert list(host) == names
    for field, dtype, shape in layout:
        assert tuple(views[field].shape) == tuple(shape) == host[field].shape and views[field].dtype == dtype
        assert host[field].dtype == (np.float64 if field == "table" else np.int64)
        assert np.array_equal(host[field].view(np.int64), views[field].view(torch.int64).numpy())         # bit for bit, the float64 table too
    if "table" in views:
        assert views["table"].dtype == torch.float64 and np.array_equal(host["table"].view(np.int64).ravel(), np.arange(sizes[0]))
