"""DeepLab(backbone='drn') without a GPU: the parameter tree against the reference's manifest, the pretrained-weights loader,
and the engine's DRN orchestration (driven with the tests' torch statement of the kernels, tests/kernel_spec.py +
tests/drn_spec.py) against the functional oracle of tests/drn_ref.py and against the fixtures the reference itself wrote
(tests/golden/make_golden_drn.py)."""
import json
import os

import pytest
import torch

import backbone_cases
import drn_ref
import model_cases
from drn_spec import DrnSpecKernels
from oracle import deeplab_ref
from uda_clr_amd.engine import GeneratorEngine
from uda_clr_amd.networks.deeplabv3 import DeepLab

GOLDEN = model_cases.GOLDEN
NAMES = model_cases.NAMES


def _engine():
    return GeneratorEngine(DrnSpecKernels(), 8, backbone="drn")


def _model(perturb=True):
    m = model_cases.seeded_model(perturb=perturb, backbone="drn", output_stride=8)
    m._engine_override = _engine()
    return m


def test_manifest_matches_reference():
    """405 state-dict keys in the reference's order, their shapes, and the seeded-initialisation sums (drn.py:159-169 after the
    constructors' own draws), then the ASPP / decoder as for the other backbones."""
    with open(os.path.join(GOLDEN, "manifest_drn.json")) as f:
        man = json.load(f)
    torch.manual_seed(1337)
    m = DeepLab(num_classes=2, backbone="drn", output_stride=16, method="prototype_full")
    sd = m.state_dict()
    assert man["n_state_keys"] == len(sd) == 405
    assert [e["key"] for e in man["entries"]] == list(sd.keys())
    for e in man["entries"]:
        v = sd[e["key"]]
        assert list(v.shape) == e["shape"], e["key"]
        assert abs(float(v.double().sum()) - e["sum"]) <= 1e-9 * max(1.0, abs(e["sum"])), e["key"]
    params = list(m.parameters())
    assert len(params) == man["n_param_tensors"] == 204
    assert sum(p.numel() for p in params) == man["n_params"] == 40733143
    n1 = sum(p.numel() for p in m.get_1x_lr_params())
    n10 = sum(p.numel() for p in m.get_10x_lr_params())
    assert n1 == sum(p.numel() for p in m.backbone.parameters()) == 35296176
    assert n1 + n10 == man["n_params"]


def test_output_stride_is_forced_to_8():
    """deeplabv3.py:14-15: whatever output_stride is passed, the DRN model is the output-stride-8 one (ASPP rates 12 / 24 / 36)."""
    m = DeepLab(num_classes=2, backbone="drn", output_stride=16, method="prototype_full")
    assert m.output_stride == 8
    assert m.aspp.aspp2.atrous_conv.dilation == (12, 12) and m.aspp.aspp1.atrous_conv.in_channels == 512
    assert m.decoder.conv1.in_channels == 256
    m._engine_override = _engine()
    m.eval()
    with torch.no_grad():
        out = m(torch.randn(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)))
    assert tuple(out[2].shape) == (1, 256, 8, 8) and tuple(out[3].shape) == (1, 304, 16, 16)


def test_pretrained_loader(monkeypatch, tmp_path):
    """Nothing is ever fetched.  Without UDA_CLR_DRN_D_54_PTH pretrained=True leaves the seeded initialisation; with it the
    weights are those of the file, loaded the reference's way (fc.weight / fc.bias dropped, then a strict load, drn.py:380-383)."""
    import torch.utils.model_zoo as model_zoo
    import urllib.request

    def refuse(*a, **k):
        raise AssertionError("pretrained=True must not fetch")
    monkeypatch.setattr(model_zoo, "load_url", refuse)
    monkeypatch.setattr(urllib.request, "urlopen", refuse)
    monkeypatch.delenv("UDA_CLR_DRN_D_54_PTH", raising=False)
    from uda_clr_amd.networks.backbone.drn import drn_d_54
    torch.manual_seed(0)
    a = drn_d_54(torch.nn.BatchNorm2d, pretrained=True)
    torch.manual_seed(0)
    b = drn_d_54(torch.nn.BatchNorm2d, pretrained=False)
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb), ka
    g = torch.Generator().manual_seed(9)
    saved = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v + 3) for k, v in a.state_dict().items()}
    saved["fc.weight"], saved["fc.bias"] = torch.randn(1000, 512, 1, 1, generator=g), torch.randn(1000, generator=g)
    path = str(tmp_path / "drn_d_54.pth")
    torch.save(saved, path)
    monkeypatch.setenv("UDA_CLR_DRN_D_54_PTH", path)
    c = drn_d_54(torch.nn.BatchNorm2d, pretrained=True)
    for k, v in c.state_dict().items():
        assert torch.equal(v, saved[k]), k
    torch.manual_seed(0)
    d = drn_d_54(torch.nn.BatchNorm2d, pretrained=False)           # pretrained=False ignores the variable
    assert torch.equal(d.state_dict()["layer0.0.weight"], b.state_dict()["layer0.0.weight"])
    del saved["layer8.0.weight"]                                   # the load is strict, as the reference's
    torch.save(saved, path)
    with pytest.raises(RuntimeError, match="layer8.0.weight"):
        drn_d_54(torch.nn.BatchNorm2d, pretrained=True)


def test_transnorm_raises():
    with pytest.raises(NotImplementedError, match="TransNorm"):
        DeepLab(num_classes=2, backbone="drn", sync_bn=False)


@pytest.mark.parametrize("size", [64, 96])
def test_eval_forward_matches_oracle(size):
    m = _model().eval()
    x = torch.randn(2, 3, size, size, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        mine = m(x)
        ref = drn_ref.deeplab_forward(deeplab_ref.canonical_state(m.state_dict()), x, training=False)
    for n, a, b in zip(NAMES, mine, ref):
        assert a.shape == b.shape, n
        assert model_cases.rel(a, b) < 2e-4, (n, model_cases.rel(a, b))


def narrow_table(route):
    """drn._DRN_NARROW as the engine routes it ("routed"), with every narrow conv the implicit-GEMM route can serve on that route
    ("implicit-gemm": the stride-1 ones; a stride-2 conv below the wide tiles has the narrow kernels only) and with every listed
    shape on the narrow kernels ("narrow")"""
    from uda_clr_amd.networks.backbone.drn import _DRN_NARROW
    return {k: {"routed": v, "implicit-gemm": v and k[3] == 2, "narrow": True}[route] for k, v in _DRN_NARROW.items()}


@pytest.mark.parametrize("route", ["routed", "implicit-gemm", "narrow"])
def test_train_forward_backward_matches_oracle(route, monkeypatch):
    """Training forward + backward at 64^2 (injected dropout masks) against the fp64 oracle, with the bounds of the other
    backbones' CPU cases: outputs within 3x the fp32 oracle's own fp64 distance, gradients by model_cases.grads_ok with no
    parameter left out (every DRN BatchNorm is followed by a ReLU or by the residual add + ReLU: no gradient is analytically
    zero).  Runs on the routes the engine picks, with every stride-1 head conv on the implicit-GEMM route and with every head
    conv on the narrow kernels (``narrow_table``)."""
    from uda_clr_amd.networks.backbone import drn
    monkeypatch.setattr(drn, "_DRN_NARROW", narrow_table(route))
    fwd, grads, stats, fwd64 = model_cases.train_parity(torch.device("cpu"), backbone="drn", output_stride=8, engine=_engine(),
                                                        oracle_forward=drn_ref.deeplab_forward)
    backbone_cases.train_checks(fwd64, grads, stats, stats_bound=1e-3, gmean_bound=1.5, n_grads=204)


def test_frozen_batchnorm_training_matches_oracle():
    """freeze_bn() while training: eval-mode BatchNorm (running statistics, no batch terms in the backward), live dropout."""
    fwd, grads, stats, _ = model_cases.train_parity(torch.device("cpu"), backbone="drn", output_stride=8, frozen_bn=True,
                                                    engine=_engine(), seed=11, oracle_forward=drn_ref.deeplab_forward)
    assert stats == 0.0
    model_cases.frozen_grads_ok(grads)


def test_mc_fast_path_equals_plain_stochastic_forwards():
    """GeneratorEngine.mc_forward (the DRN backbone's activations reused) vs plain stochastic forwards on identical masks."""
    backbone_cases.mc_fast_path_equals_plain_stochastic_forwards(lambda: _model().train(), torch.device("cpu"), 8)


def golden_errors(dev, tag, engine=None):
    return backbone_cases.golden_errors(dev, tag, "drn", drn_ref.deeplab_forward, engine, n_grad_keys=204, output_stride=8)


@pytest.mark.parametrize("tag", ["drn_128", "drn_256"])
def test_engine_matches_reference_fixture(tag):
    backbone_cases.check_golden(golden_errors(torch.device("cpu"), tag, _engine()))
