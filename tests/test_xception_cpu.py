"""DeepLab(backbone='xception') without a GPU: the parameter tree against the reference's manifest, and the engine's
Xception orchestration (driven with the tests' torch statement of the kernels, tests/kernel_spec.py) against the
functional oracle of tests/xception_ref.py and against the fixtures the reference itself wrote
(tests/golden/make_golden_xception.py)."""
import json
import os

import numpy as np
import pytest
import torch

import model_cases
import xception_ref
from kernel_spec import SpecKernels
from oracle import deeplab_ref, step_ref
from uda_clr_amd.engine import GeneratorEngine
from uda_clr_amd.networks.deeplabv3 import DeepLab

GOLDEN = model_cases.GOLDEN
NAMES = model_cases.NAMES


def _model(output_stride=16, perturb=True):
    m = model_cases.seeded_model(perturb=perturb, backbone="xception", output_stride=output_stride)
    m._engine_override = GeneratorEngine(SpecKernels(), output_stride, backbone="xception")
    return m


def test_manifest_matches_reference():
    """855 state-dict keys in the reference's order, their shapes, and the seeded-initialisation sums (xception.py:234-245
    after the constructors' own draws), then the ASPP / decoder as for the other backbones."""
    with open(os.path.join(GOLDEN, "manifest_xception.json")) as f:
        man = json.load(f)
    torch.manual_seed(1337)
    m = DeepLab(num_classes=2, backbone="xception", output_stride=16, method="prototype_full")
    sd = m.state_dict()
    assert man["n_state_keys"] == len(sd) == 855
    assert [e["key"] for e in man["entries"]] == list(sd.keys())
    for e in man["entries"]:
        v = sd[e["key"]]
        assert list(v.shape) == e["shape"], e["key"]
        assert abs(float(v.double().sum()) - e["sum"]) <= 1e-9 * max(1.0, abs(e["sum"])), e["key"]
    params = list(m.parameters())
    assert len(params) == man["n_param_tensors"]
    assert sum(p.numel() for p in params) == man["n_params"] == 54701399
    n1 = sum(p.numel() for p in m.get_1x_lr_params())
    n10 = sum(p.numel() for p in m.get_10x_lr_params())
    assert n1 == sum(p.numel() for p in m.backbone.parameters()) == 37867312
    assert n1 + n10 == man["n_params"]


def test_pretrained_loader_fetches_nothing(monkeypatch):
    """The reference's loader keeps no key (model_dict is empty, xception.py:247-281): the drop-in loads nothing and never
    reaches for the network."""
    import torch.utils.model_zoo as model_zoo
    import urllib.request

    def refuse(*a, **k):
        raise AssertionError("pretrained=True must not fetch")
    monkeypatch.setattr(model_zoo, "load_url", refuse)
    monkeypatch.setattr(urllib.request, "urlopen", refuse)
    from uda_clr_amd.networks.backbone.xception import AlignedXception
    torch.manual_seed(0)
    a = AlignedXception(16, torch.nn.BatchNorm2d, pretrained=True)
    torch.manual_seed(0)
    b = AlignedXception(16, torch.nn.BatchNorm2d, pretrained=False)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka


def test_transnorm_raises():
    with pytest.raises(NotImplementedError, match="TransNorm"):
        DeepLab(num_classes=2, backbone="xception", output_stride=16, sync_bn=False)


@pytest.mark.parametrize("size", [64, 96])
def test_eval_forward_matches_oracle(size):
    m = _model().eval()
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        mine = m(x)
        ref = xception_ref.deeplab_forward(deeplab_ref.canonical_state(m.state_dict()), x, training=False)
    for n, a, b in zip(NAMES, mine, ref):
        assert a.shape == b.shape, n
        assert model_cases.rel(a, b) < 2e-4, (n, model_cases.rel(a, b))


@pytest.mark.parametrize("output_stride", [16, 8])
def test_train_forward_backward_matches_oracle(output_stride):
    """Training forward + backward at 64^2 (injected dropout masks) against the fp64 oracle, with the bounds of the
    other backbones' CPU cases: outputs within 3x the fp32 oracle's own fp64 distance, gradients by model_cases.grads_ok."""
    eng = GeneratorEngine(SpecKernels(), output_stride, backbone="xception")
    with xception_ref.as_deeplab_oracle():
        fwd, grads, stats, fwd64 = model_cases.train_parity(torch.device("cpu"), backbone="xception",
                                                            output_stride=output_stride, engine=eng)
    for n, (mine, floor) in fwd64.items():
        assert mine < 3.0 * floor + 2e-4, (n, mine, floor)
    assert all(v[0] < float("inf") for v in grads.values()), [k for k, v in grads.items() if v[0] == float("inf")]
    bad, gmean = model_cases.grads_ok(grads)
    assert not bad, list(bad.items())[:10]
    assert gmean < 1.5, gmean
    assert stats < 1e-3, stats


def test_frozen_batchnorm_training_matches_oracle():
    """freeze_bn() while training: eval-mode BatchNorm (running statistics, no batch terms in the backward), live dropout."""
    eng = GeneratorEngine(SpecKernels(), backbone="xception")
    with xception_ref.as_deeplab_oracle():
        fwd, grads, stats, _ = model_cases.train_parity(torch.device("cpu"), backbone="xception", frozen_bn=True,
                                                        engine=eng, seed=11)
    assert stats == 0.0
    model_cases.frozen_grads_ok(grads)


def golden_errors(dev, tag, engine=None):
    """The Xception model (``engine``: CPU tests' kernel statement) against forward_<tag>.npz, as model_cases.golden_parity
    does for the other backbones."""
    z = np.load(os.path.join(GOLDEN, "forward_%s.npz" % tag))
    B, S, os_ = int(z["B"]), int(z["S"]), int(z["output_stride"])
    m = model_cases.seeded_model(backbone="xception", output_stride=os_)
    if engine is not None:
        m._engine_override = engine
    torch.manual_seed(int(z["input_seed"]))
    x = torch.randn(B, 3, S, S)
    errs = {}
    m.to(dev).eval()
    with torch.no_grad():
        out = m(x.to(dev))
    for n, t in zip(NAMES, out):
        f = t.double().cpu().reshape(-1)
        idx = torch.linspace(0, f.numel() - 1, 97).long()
        ref = torch.from_numpy(z["eval.%s.smp" % n])
        errs["eval." + n + ".smp"] = (f[idx] - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
        errs["eval." + n + ".abs"] = abs(f.abs().sum().item() - float(z["eval.%s.abs" % n])) / float(z["eval.%s.abs" % n])
    from make_golden_inputs import synth_targets
    tmap, tbd = synth_targets(B, S, S, int(z["target_seed"]))
    m.train()
    sd0 = deeplab_ref.canonical_state({k: v.cpu() for k, v in m.state_dict().items()})
    rec = {}
    torch.manual_seed(int(z["dropout_seed"]))
    with torch.no_grad():
        xception_ref.deeplab_forward(sd0, x, training=True, record=rec, output_stride=os_)
    for k, v in rec.items():
        assert int(v.sum()) == int(z["mask.%s.sum" % k]), "dropout stream differs from the reference's draw"
    m.set_dropout_masks(rec)
    out = m(x.to(dev))
    assert all(bool(torch.isfinite(t).all()) for t in out)
    loss = step_ref.seg_loss(out[0], out[1], tmap.to(dev), tbd.to(dev))
    loss.backward()
    errs["train.loss"] = abs(loss.item() - float(z["train.loss"])) / abs(float(z["train.loss"]))
    live = m._flat_state()
    keys = [str(k) for k in z["train.grad_keys"]]
    gn = np.array([live[k].grad.double().norm().item() for k in keys])
    rel_gn = np.abs(gn - z["train.grad_norm"]) / np.maximum(z["train.grad_norm"], 1e-12)
    conv = np.array([live[k].dim() == 4 for k in keys])
    errs["train.grad_norm.conv"] = float(rel_gn[conv].max())
    errs["train.grad_norm.median"] = float(np.median(rel_gn))
    bs = np.array([live[k].double().sum().item() for k in z["train.bn_keys"]])
    # running-stat sums relative to max(|ref|, 1e-2), not 1e-3 as for the other backbones: the outer BN of a separable conv reads a
    # BN output through a 1x1 conv, so its batch mean is W * beta of the inner BN, analytically 0 at the seeded init (reference:
    # |sum| ~ 1e-7 over 1536-2048 channels).  Measured on MI355X: the exit flow's bn3 / bn4 / bn5 running means come out at
    # -0.9 ... -2.0e-5 (1e-8 per channel, ~1e-7 of the unit-variance activations), 2.0e-2 against the 1e-3 floor and 2.0e-3
    # against this one; every other running statistic sits within 1.2e-7 of the fixture, the fp64 oracle within 3.5e-4.
    errs["train.bn_sum"] = float(np.max(np.abs(bs - z["train.bn_sum"]) / np.maximum(np.abs(z["train.bn_sum"]), 1e-2)))
    return errs


GOLDEN_BOUNDS = {"train.grad_norm.conv": 5e-2, "train.grad_norm.median": 2e-2, "train.bn_sum": 5e-3}


def check_golden(errs):
    for k, v in errs.items():
        bound = GOLDEN_BOUNDS.get(k, 1e-3 if k.startswith(("eval.", "train.loss")) else 5e-3)
        assert v < bound, (k, v, bound)


@pytest.mark.parametrize("tag", ["xception_128", "xception_256", "xception_os8_128"])
def test_engine_matches_reference_fixture(tag):
    os_ = 8 if "os8" in tag else 16
    check_golden(golden_errors(torch.device("cpu"), tag, GeneratorEngine(SpecKernels(), os_, backbone="xception")))
