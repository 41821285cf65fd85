"""not-gpu: every step of the product Trainers against the fp64 oracle evaluated at the trainer's own state before that step
(tests/step_cases.py), with the machinery that carries state from one step to the next switched on: shared weight layouts,
the MC fast path and its invalidation by ``note_params_changed``, ``fused_grad_accumulation``, the centroid EMA state and the
BatchNorm running statistics.  The generator runs on ``GeneratorEngine(SpecKernels())`` (the torch statement of the kernels), the
discriminators are the oracle's, the optimizers torch's.  This pins the host-side cache logic on a machine without a GPU.

Every bound holds at every step and was set from the measured values (in brackets, max over the three steps):

  prototype run (64^2, B = 2 + 2): scalars 1e-4 [seg 1.6e-6, adv 3.3e-8, D_same 2.7e-7, D_diff 2.0e-8, intra 6.4e-6,
  inter 2.2e-5]; running statistics 2e-3 [6.1e-4]; centroid EMA state 1e-3 [1.5e-4]; MC std map 2e-4 [4.9e-5]; reliability
  masks: at most 4 flipped pixels [0]; optimizer updates vs torch's rule 1e-6 [3.5e-7].  Gradients: every tensor within
  ``model_cases.grad_ok`` (generator [0.59 of the bound], discriminators [0.50]); geometric mean of the generator's
  engine / fp32-oracle ratios <= 4 [3.10 at step 1, 0.95, 0.71], the multi-step bound of tests/test_multistep_gpu.py.  At B = 2
  that mean is fp32 noise that scatters from step to step (another batch seed: 1.09, 1.21, 2.10), far above grads_ok's single
  draw of 1.5; a stale cache moves it to 585.  The prototype run starts from the unperturbed seeded model at 64^2: from the
  perturbed one, or at 32^2, the few reliable pixels of the MC gate carry no cup pseudo label, a retrified centroid is 0 / 0 (in
  the reference as well) and the step stops on a NaN loss.

  baseline run (32^2, B = 2, perturbed model): seg 1e-4 [6.8e-5]; running statistics 2e-3 [5.0e-4]; updates 1e-6 [5.8e-8];
  gradients: ``model_cases.grads_ok`` unchanged (geometric mean <= 1.5 [0.80]).

Sensitivity: the generator's ``_wshare`` dict kept across optimizer steps passes step 1 and fails step 2 by >= 10x the gradient
bound (measured: 353x on the worst tensor, geometric mean 585).
"""
import pytest
import torch

import model_cases
import step_cases
from kernel_spec import SpecKernels
from uda_clr_amd.engine import GeneratorEngine

CPU = torch.device("cpu")
PROTO_BOUNDS = {"scalar.seg": 1e-4, "scalar.adv": 1e-4, "scalar.D_same": 1e-4, "scalar.D_diff": 1e-4, "scalar.intra": 1e-4,
                "scalar.inter": 1e-4, "bn_running": 2e-3, "centroids": 1e-3, "std_map": 2e-4, "mask_flips": 4,
                "update.gen": 1e-6, "update.dis": 1e-6, "update.dis2": 1e-6, "gen_grads.worst": 1.0, "gen_grads.gmean": 4.0,
                "dis_grads.worst": 1.0}
BASE_BOUNDS = {"scalar.seg": 1e-4, "bn_running": 2e-3, "update.gen": 1e-6, "gen_grads.worst": 1.0, "gen_grads.gmean": 1.5}


def _gen(perturb):
    m = model_cases.seeded_model(perturb=perturb)
    m._engine_override = GeneratorEngine(SpecKernels())
    return m


def _counters_ok(kind, reports):
    for k, rep in enumerate(reports):
        c = rep["counts"]
        assert c.get("note_params_changed", 0) >= 1, (k + 1, c)
        if kind == "proto":
            assert c.get("wshare", 0) >= 1 and c.get("mc_fast", 0) == 1 and c.get("mc_plain", 0) == 0, (k + 1, c)
            assert c.get("accum_scope", 0) >= 1 and c.get("accum_add", 0) >= 1, (k + 1, c)


def test_recording_generator_answers_every_trainer_probe():
    """Every ``hasattr`` probe in train_process/*.py answers the same for the recording generator as for the product DeepLab."""
    names = step_cases.probed_names()
    assert {"mc_dropout_logits", "shared_weight_layouts", "fused_grad_accumulation", "note_params_changed"} <= names, names
    plain = model_cases.seeded_model()
    rec = step_cases.RecordingDeepLab.adopt(model_cases.seeded_model())
    assert {n: hasattr(rec, n) for n in names} == {n: hasattr(plain, n) for n in names}


def test_prototype_trainer_every_step_matches_fp64_at_its_state(tmp_path):
    reports, _ = step_cases.run("proto", _gen(False), CPU, tmp_path, B=2, S=64, steps=3, cpu_oracle_dis=True)
    print(step_cases.table("prototype_full, CPU engine, 64^2", reports, PROTO_BOUNDS))
    _counters_ok("proto", reports)
    assert not step_cases.violations(reports, PROTO_BOUNDS)


def test_baseline_trainer_every_step_matches_fp64_at_its_state(tmp_path):
    reports, _ = step_cases.run("baseline", _gen(True), CPU, tmp_path, B=2, S=32, steps=3)
    print(step_cases.table("baseline, CPU engine, 32^2", reports, BASE_BOUNDS))
    _counters_ok("baseline", reports)
    assert not step_cases.violations(reports, BASE_BOUNDS)


def test_stale_generator_layouts_fail_the_second_step(tmp_path):
    """Sensitivity (i): one ``_wshare`` dict for all steps - the layouts of the parameters before the first optimizer step."""
    reports, _ = step_cases.run("proto", _gen(False), CPU, tmp_path, B=2, S=64, steps=2, faults=("stale_wshare",),
                                cpu_oracle_dis=True)
    print(step_cases.table("prototype_full, stale generator layouts", reports, PROTO_BOUNDS))
    assert not step_cases.violations(reports[:1], PROTO_BOUNDS)
    assert reports[1]["gen_grads.worst"] >= 10.0, reports[1]["gen_grads.worst"]
