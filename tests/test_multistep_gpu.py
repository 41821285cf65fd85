"""-m gpu: every step of the product Trainers on the HIP path against the fp64 oracle evaluated at the trainer's own state before
that step (tests/step_cases.py), with everything that carries state from one step to the next switched on: the generator's and
the discriminators' shared weight layouts (relayouts and bf16x3-packed ``w._x3`` rows), the MC fast path and its invalidation by
``note_params_changed``, ``fused_grad_accumulation``, FlatAdam's raw-pointer update, the discriminators' fused SGD, the centroid
EMA state and the BatchNorm running statistics (two training forwards plus the replayed MC passes).

Bounds: the same at every step, set from an MI355X run of this file (measured maxima over all steps and runs in brackets):
scalars 1e-4 [4.0e-5, ResNet-101 seg; prototype terms <= 1.3e-5]; running statistics 2e-3 [3.9e-4]; centroid EMA state 1e-3
[1.6e-4]; MC std map 2e-4 [7.3e-5]; reliability masks: at most 4 flipped pixels [0]; every optimizer update against torch's rule
replayed in fp64 1e-6 [3.2e-7].  Gradients per tensor: ``gen_grads.worst`` / ``dis_grads.worst`` <= 2 in units of
``model_cases.grad_ok``'s bound (grads_ok's tail allowance included) [generator 1.43: backbone.features.16/17.conv.7.bias, the
near-cancelling BatchNorm biases model_cases documents, f32 mode step 4; discriminator 1.04: dis.conv1.weight at step 1]; geometric
mean of the generator's HIP / fp32-oracle ratios <= 4 [2.24, bf16x3 step 4; the other 14 steps 0.05 - 1.84, f32 mode alike].  These
two are looser than the single-step ``grads_ok`` (10x per tensor, mean 1.5): at B = 2 they are fp32 noise that scatters from step
to step in both matrix modes, and 15 step evaluations are 15 draws where the single-step test makes one.  A stale cache or a lost
gradient lands far outside: (i) 414x / mean 32, (ii) 59x, (iii) 22x / mean 33 at step 1.  The file adds ~75 s to the -m gpu run.

Run (a) starts from the unperturbed seeded model: from the perturbed one the few pixels that pass the MC reliability gate
(std < 0.04) carry no cup pseudo label at this size, a retrified centroid is 0 / 0 (in the reference as well) and the step stops
on a NaN loss.  Runs (b) and (c) start from ``model_cases.seeded_model(perturb=True)``.
"""
import pytest
import torch

import model_cases
import step_cases
from uda_clr_amd.optim import FlatAdam

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

PROTO_BOUNDS = {"scalar.seg": 1e-4, "scalar.adv": 1e-4, "scalar.D_same": 1e-4, "scalar.D_diff": 1e-4, "scalar.intra": 1e-4,
                "scalar.inter": 1e-4, "bn_running": 2e-3, "centroids": 1e-3, "std_map": 2e-4, "mask_flips": 4,
                "update.gen": 1e-6, "update.dis": 1e-6, "update.dis2": 1e-6, "gen_grads.worst": 2.0, "gen_grads.gmean": 4.0,
                "dis_grads.worst": 2.0}
BASE_BOUNDS = {"scalar.seg": 1e-4, "bn_running": 2e-3, "update.gen": 1e-6, "gen_grads.worst": 2.0, "gen_grads.gmean": 4.0}


def _gen(perturb, backbone="mobilenet", mfma=None):
    m = model_cases.seeded_model(perturb=perturb, backbone=backbone).to(DEV)
    if mfma is not None:              # the matrix instructions of the wide conv tiles, as test_kernels_gpu.py switches them
        K = m._engine_for(torch.empty(1, device=DEV)).K
        K.mfma = K.MFMA_F32 if mfma == "f32" else K.MFMA_BF16X3
    return m


def _counters_ok(kind, tr, reports):
    assert isinstance(tr.optim_gen, FlatAdam), type(tr.optim_gen)
    for k, rep in enumerate(reports):
        c = rep["counts"]
        assert c.get("note_params_changed", 0) >= 1, (k + 1, c)
        if kind == "proto":
            assert c.get("wshare", 0) >= 1 and c.get("wshare_dis", 0) >= 1 and c.get("wshare_dis2", 0) >= 1, (k + 1, c)
            assert c.get("mc_fast", 0) == 1 and c.get("mc_plain", 0) == 0, (k + 1, c)
            assert c.get("accum_scope", 0) >= 1 and c.get("accum_add", 0) >= 1, (k + 1, c)


def _check(title, kind, tr, reports, bounds):
    print("\n" + step_cases.table(title, reports, bounds))
    _counters_ok(kind, tr, reports)
    bad = step_cases.violations(reports, bounds)
    assert not bad, bad


def test_prototype_trainer_every_step_on_hip(tmp_path):
    """Run (a): Trainer_prototype_full.train_step, MobileNetV2, 64^2, B = 2 + 2, product discriminators, retrify on, 4 steps."""
    reports, tr = step_cases.run("proto", _gen(False), DEV, tmp_path, B=2, S=64, steps=4)
    _check("(a) prototype_full, MobileNetV2 64^2", "proto", tr, reports, PROTO_BOUNDS)


@pytest.mark.parametrize("mfma", ["bf16x3", "f32"])
def test_baseline_trainer_every_step_on_hip(tmp_path, mfma):
    """Run (b): Trainer_baseline, MobileNetV2, 128^2, B = 2, 4 steps, both matrix modes."""
    reports, tr = step_cases.run("baseline", _gen(True, mfma=mfma), DEV, tmp_path, B=2, S=128, steps=4)
    _check("(b) baseline, MobileNetV2 128^2, %s" % mfma, "baseline", tr, reports, BASE_BOUNDS)


def test_baseline_trainer_every_step_on_hip_resnet(tmp_path):
    """Run (c): Trainer_baseline, ResNet-101, 96^2, B = 2, 3 steps (stride-2 and long-K bf16x3 1x1 layouts)."""
    reports, tr = step_cases.run("baseline", _gen(True, backbone="resnet"), DEV, tmp_path, B=2, S=96, steps=3)
    _check("(c) baseline, ResNet-101 96^2", "baseline", tr, reports, BASE_BOUNDS)


# ---- sensitivity: one deliberate fault each (wrong numbers only), reported by the step check above
def test_stale_generator_layouts_fail_the_second_step(tmp_path):
    """(i) One ``_wshare`` dict for the generator across optimizer steps: step 1 passes, step 2 fails by >= 10x its bound
    (measured: 410x the grad_ok bound on the worst tensor, 205x the bound of 2)."""
    reports, tr = step_cases.run("proto", _gen(False), DEV, tmp_path, B=2, S=64, steps=2, faults=("stale_wshare",))
    print("\n" + step_cases.table("(i) stale generator layouts", reports, PROTO_BOUNDS))
    assert not step_cases.violations(reports[:1], PROTO_BOUNDS)
    assert reports[1]["gen_grads.worst"] >= 10 * PROTO_BOUNDS["gen_grads.worst"], reports[1]["gen_grads.worst"]


def test_stale_discriminator_layouts_fail_the_second_step(tmp_path):
    """(ii) The same for the uncertainty discriminator.  At the reference's discriminator rate (2.5e-5) one SGD step moves its
    weights by ~1e-5 relative, below the noise floor: a stale discriminator layout there measured 0.098 of the bound at step 2,
    i.e. invisible.  This check runs the discriminators at lr 0.1, where one step moves them like the generator's Adam step
    (measured: 59x the grad_ok bound on the worst tensor, 29x the bound of 2)."""
    reports, tr = step_cases.run("proto", _gen(False), DEV, tmp_path, B=2, S=64, steps=2, stale_dis=("dis2",), lr_dis=0.1)
    print("\n" + step_cases.table("(ii) stale discriminator layouts", reports, PROTO_BOUNDS))
    assert not step_cases.violations(reports[:1], PROTO_BOUNDS)
    assert reports[1]["dis_grads.worst"] >= 10 * PROTO_BOUNDS["dis_grads.worst"], reports[1]["dis_grads.worst"]


def test_dropped_accumulation_fails_the_first_step(tmp_path):
    """(iii) ``fused_grad_accumulation`` dropping the later node's add: the first step already fails by >= 10x (measured: 22x the
    grad_ok bound on the worst tensor, 11x the bound of 2)."""
    reports, tr = step_cases.run("proto", _gen(False), DEV, tmp_path, B=2, S=64, steps=1, faults=("drop_accum",))
    print("\n" + step_cases.table("(iii) dropped accumulation", reports, PROTO_BOUNDS))
    assert reports[0]["counts"].get("accum_add", 0) >= 1
    assert reports[0]["gen_grads.worst"] >= 10 * PROTO_BOUNDS["gen_grads.worst"], reports[0]["gen_grads.worst"]
