"""DeepLab(backbone='xception') without a GPU: the parameter tree against the reference's manifest, and the engine's
Xception orchestration (driven with the tests' torch statement of the kernels, tests/kernel_spec.py) against the
functional oracle of tests/xception_ref.py and against the fixtures the reference itself wrote
(tests/golden/make_golden_xception.py)."""
import json
import os

import pytest
import torch

import backbone_cases
import model_cases
import xception_ref
from kernel_spec import SpecKernels
from oracle import deeplab_ref
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
    fwd, grads, stats, fwd64 = model_cases.train_parity(torch.device("cpu"), backbone="xception", output_stride=output_stride,
                                                        engine=eng, oracle_forward=xception_ref.deeplab_forward)
    backbone_cases.train_checks(fwd64, grads, stats, stats_bound=1e-3, gmean_bound=1.5)


def test_frozen_batchnorm_training_matches_oracle():
    """freeze_bn() while training: eval-mode BatchNorm (running statistics, no batch terms in the backward), live dropout."""
    eng = GeneratorEngine(SpecKernels(), backbone="xception")
    fwd, grads, stats, _ = model_cases.train_parity(torch.device("cpu"), backbone="xception", frozen_bn=True, engine=eng, seed=11,
                                                    oracle_forward=xception_ref.deeplab_forward)
    assert stats == 0.0
    model_cases.frozen_grads_ok(grads)


def golden_errors(dev, tag, engine=None):
    return backbone_cases.golden_errors(dev, tag, "xception", xception_ref.deeplab_forward, engine)


@pytest.mark.parametrize("tag", ["xception_128", "xception_256", "xception_os8_128"])
def test_engine_matches_reference_fixture(tag):
    os_ = 8 if "os8" in tag else 16
    backbone_cases.check_golden(golden_errors(torch.device("cpu"), tag, GeneratorEngine(SpecKernels(), os_, backbone="xception")))
