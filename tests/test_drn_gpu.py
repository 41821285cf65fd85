"""-m gpu: DeepLab(backbone='drn') on the HIP kernels against the fp64 / fp32 oracle of tests/drn_ref.py and against the
fixtures the reference's own DeepLab(backbone='drn') wrote (tests/golden/make_golden_drn.py).  Bounds are those of
test_xception_gpu.py (= the ResNet-101 cases of test_generator_gpu.py)."""
import pytest
import torch

import backbone_cases
import drn_ref
import model_cases
from test_drn_cpu import golden_errors, narrow_table

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("size", [64, 96])
def test_eval_forward_matches_oracle(size):
    errs = model_cases.eval_parity(DEV, 2, size, backbone="drn", oracle_forward=drn_ref.deeplab_forward)
    assert max(errs.values()) < 1e-3, errs


@pytest.mark.parametrize("route", ["routed", "implicit-gemm", "narrow"])
def test_train_forward_backward_matches_oracle(route, monkeypatch):
    """on the routes the engine picks, with every stride-1 head conv on the implicit-GEMM route and with every one on the narrow kernels"""
    from uda_clr_amd.networks.backbone import drn
    monkeypatch.setattr(drn, "_DRN_NARROW", narrow_table(route))
    fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, backbone="drn", output_stride=8, oracle_forward=drn_ref.deeplab_forward)
    backbone_cases.train_checks(fwd64, grads, stats, n_grads=204)


def test_frozen_batchnorm_training_matches_oracle():
    fwd, grads, stats, _ = model_cases.train_parity(DEV, backbone="drn", output_stride=8, frozen_bn=True, seed=11,
                                                    oracle_forward=drn_ref.deeplab_forward)
    assert stats == 0.0
    model_cases.frozen_grads_ok(grads)


def test_padding_columns_never_leak(monkeypatch):
    """Every fp32 work matrix starts as NaN / Inf / 3e38 (engine.POISON_BUFFERS): same results as on clean buffers."""
    from uda_clr_amd import engine
    monkeypatch.setattr(engine, "POISON_BUFFERS", True)
    fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, S=96, backbone="drn", output_stride=8,
                                                        oracle_forward=drn_ref.deeplab_forward)
    backbone_cases.train_checks(fwd64, grads, stats, n_grads=204)


def test_work_buffers_and_statistics_arena_are_written_inside(monkeypatch):
    """The same poisoned run with every work buffer of the engine between guard rows and the statistics arenas between guard
    doubles (engine_guards.guarded): every guard is bit-intact afterwards, the results meet the same bounds."""
    import engine_guards
    from uda_clr_amd import engine
    monkeypatch.setattr(engine, "POISON_BUFFERS", True)
    with engine_guards.guarded() as guards:
        fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, S=96, backbone="drn", output_stride=8,
                                                            oracle_forward=drn_ref.deeplab_forward)
        torch.cuda.synchronize()
    assert guards.counts()[0] >= 100 and guards.counts()[1] >= 2, guards.counts()
    assert guards.violations() == [], "(buffer, side, first changed guard element)"
    backbone_cases.train_checks(fwd64, grads, stats, n_grads=204)


@pytest.mark.parametrize("tag", ["drn_128", "drn_256"])
def test_matches_reference_fixtures(tag):
    errs = golden_errors(DEV, tag)
    print({k: "%.2e" % v for k, v in errs.items() if k.startswith("train.") and not k.endswith(".abs")})
    backbone_cases.check_golden(errs)


def test_mc_fast_path_equals_plain_stochastic_forwards():
    """GeneratorEngine.mc_forward (the DRN backbone's activations reused) vs plain stochastic forwards on identical masks."""
    backbone_cases.mc_fast_path_equals_plain_stochastic_forwards(
        lambda: model_cases.seeded_model(perturb=True, backbone="drn").to(DEV).train(), DEV, 8)


def test_prototype_full_train_step(tmp_path):
    """One Trainer_prototype_full step with a DRN generator at 128^2, B = 2 + 2: finite losses, every parameter moves."""
    backbone_cases.prototype_full_train_step("drn", DEV, tmp_path)


def test_drn_per_gpu_batch_8_at_512_properties():
    """B = 8 at 512^2: eval batch independence and the training-batch permutation properties; every one of the 204 parameters has
    a finite gradient, none is left out of the bound."""
    backbone_cases.per_gpu_batch_8_at_512_properties("drn", DEV, 8, n_params=204)
