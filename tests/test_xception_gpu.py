"""-m gpu: DeepLab(backbone='xception') on the HIP kernels against the fp64 / fp32 oracle of tests/xception_ref.py and against
the fixtures the reference's own DeepLab(backbone='xception') wrote (tests/golden/make_golden_xception.py).  Bounds are
those of the ResNet-101 cases in test_generator_gpu.py."""
import pytest
import torch

import backbone_cases
import model_cases
import xception_ref
from test_xception_cpu import golden_errors

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("size", [64, 96])
def test_eval_forward_matches_oracle(size):
    errs = model_cases.eval_parity(DEV, 2, size, backbone="xception", oracle_forward=xception_ref.deeplab_forward)
    assert max(errs.values()) < 1e-3, errs


@pytest.mark.parametrize("output_stride", [16, 8])
def test_train_forward_backward_matches_oracle(output_stride):
    fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, backbone="xception", output_stride=output_stride,
                                                        oracle_forward=xception_ref.deeplab_forward)
    backbone_cases.train_checks(fwd64, grads, stats)


def test_padding_columns_never_leak(monkeypatch):
    """Every fp32 work matrix starts as NaN / Inf / 3e38 (engine.POISON_BUFFERS): same results as on clean buffers."""
    from uda_clr_amd import engine
    monkeypatch.setattr(engine, "POISON_BUFFERS", True)
    fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, S=96, backbone="xception", oracle_forward=xception_ref.deeplab_forward)
    backbone_cases.train_checks(fwd64, grads, stats)


def test_work_buffers_and_statistics_arena_are_written_inside(monkeypatch):
    """The same poisoned run with every work buffer of the engine between guard rows and the statistics arenas between guard
    doubles (engine_guards.guarded): every guard is bit-intact afterwards, the results meet the same bounds."""
    import engine_guards
    from uda_clr_amd import engine
    monkeypatch.setattr(engine, "POISON_BUFFERS", True)
    with engine_guards.guarded() as guards:
        fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, S=96, backbone="xception", oracle_forward=xception_ref.deeplab_forward)
        torch.cuda.synchronize()
    assert guards.counts()[0] >= 100 and guards.counts()[1] >= 2, guards.counts()
    assert guards.violations() == [], "(buffer, side, first changed guard element)"
    backbone_cases.train_checks(fwd64, grads, stats)


@pytest.mark.parametrize("tag", ["xception_128", "xception_256", "xception_os8_128"])
def test_matches_reference_fixtures(tag):
    backbone_cases.check_golden(golden_errors(DEV, tag))


def test_mc_fast_path_equals_plain_stochastic_forwards():
    """GeneratorEngine.mc_forward (the Xception backbone's activations reused) vs plain stochastic forwards on identical masks."""
    backbone_cases.mc_fast_path_equals_plain_stochastic_forwards(
        lambda: model_cases.seeded_model(perturb=True, backbone="xception").to(DEV).train(), DEV, 16)


def test_prototype_full_train_step(tmp_path):
    """One Trainer_prototype_full step with an Xception generator at 128^2, B = 2 + 2: finite losses, parameters move."""
    backbone_cases.prototype_full_train_step("xception", DEV, tmp_path)


def test_xception_per_gpu_batch_8_at_512_properties():
    """B = 8 at 512^2: eval batch independence and the training-batch permutation properties; the separable convs' inner BN bias
    gradients (analytically zero) are left out of the permutation bound."""
    backbone_cases.per_gpu_batch_8_at_512_properties("xception", DEV, 16, unmeasurable=(".bn.bias",))
