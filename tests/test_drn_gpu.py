"""-m gpu: DeepLab(backbone='drn') on the HIP kernels against the fp64 / fp32 oracle of tests/drn_ref.py and against the
fixtures the reference's own DeepLab(backbone='drn') wrote (tests/golden/make_golden_drn.py).  Bounds are those of
test_xception_gpu.py (= the ResNet-101 cases of test_generator_gpu.py)."""
import pytest
import torch

import drn_ref
import model_cases
from test_drn_cpu import check_golden, golden_errors

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("size", [64, 96])
def test_eval_forward_matches_oracle(size):
    with drn_ref.as_deeplab_oracle():
        errs = model_cases.eval_parity(DEV, 2, size, backbone="drn")
    assert max(errs.values()) < 1e-3, errs


def _train_checks(fwd64, grads, stats):
    for n, (e, floor) in fwd64.items():
        assert e < 3.0 * floor + 2e-4, (n, e, floor)
    assert stats < 5e-3, stats
    assert len(grads) == 204                     # no parameter is left out: none of DRN's gradients is analytically zero
    bad, gmean = model_cases.grads_ok(grads)
    print("gradient noise vs the fp32 oracle's: geometric mean %.3f over %d tensors" % (gmean, len(grads)))
    assert not bad, list(bad.items())[:10]
    assert gmean < 4.0, gmean


@pytest.mark.parametrize("narrow", ["", "0", "1"], ids=["routed", "implicit-gemm", "narrow"])
def test_train_forward_backward_matches_oracle(narrow, monkeypatch):
    """on the routes the engine picks, with every head conv on the implicit-GEMM route and with every one on the narrow kernels"""
    from uda_clr_amd import engine
    monkeypatch.setattr(engine, "_DRN_NARROW_ENV", narrow)
    with drn_ref.as_deeplab_oracle():
        fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, backbone="drn", output_stride=8)
    _train_checks(fwd64, grads, stats)


def test_frozen_batchnorm_training_matches_oracle():
    with drn_ref.as_deeplab_oracle():
        fwd, grads, stats, _ = model_cases.train_parity(DEV, backbone="drn", output_stride=8, frozen_bn=True, seed=11)
    assert stats == 0.0
    model_cases.frozen_grads_ok(grads)


def test_padding_columns_never_leak(monkeypatch):
    """Every fp32 work matrix starts as NaN / Inf / 3e38 (engine.POISON_BUFFERS): same results as on clean buffers."""
    from uda_clr_amd import engine
    monkeypatch.setattr(engine, "POISON_BUFFERS", True)
    with drn_ref.as_deeplab_oracle():
        fwd, grads, stats, fwd64 = model_cases.train_parity(DEV, S=96, backbone="drn", output_stride=8)
    _train_checks(fwd64, grads, stats)


@pytest.mark.parametrize("tag", ["drn_128", "drn_256"])
def test_matches_reference_fixtures(tag):
    errs = golden_errors(DEV, tag)
    print({k: "%.2e" % v for k, v in errs.items() if k.startswith("train.") and not k.endswith(".abs")})
    check_golden(errs)


def test_mc_fast_path_equals_plain_stochastic_forwards():
    """GeneratorEngine.mc_forward (the DRN backbone's activations reused) vs plain stochastic forwards on identical masks."""
    from oracle import deeplab_ref
    B, S, passes = 2, 64, 2
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(B, 3, S, S, generator=gen).to(DEV)

    def masks(n):
        mk = deeplab_ref.draw_masks(n, S, S, gen)
        mk["aspp.dropout"] = (torch.rand(n, 256, S // 8, S // 8, generator=gen) >= 0.5).to(torch.uint8)
        return mk
    m0 = masks(B)
    mc_masks = [masks(2 * B) for _ in range(passes)]
    res = []
    for fast in (False, True):
        m = model_cases.seeded_model(perturb=True, backbone="drn").to(DEV).train()
        m.set_dropout_masks(m0)
        m(x)
        if not fast:
            m._recent = []
        preds = m.mc_dropout_logits(x, passes=passes, reps=2, masks=mc_masks)
        res.append((preds, {k: v.clone() for k, v in m.state_dict().items()}))
    (p0, s0), (p1, s1) = res
    assert model_cases.rel(p1, p0) < 1e-4
    for k in s0:
        if k.endswith("num_batches_tracked"):
            assert int(s0[k]) == int(s1[k]) == 1 + passes
        elif k.endswith("running_mean") or k.endswith("running_var"):
            assert model_cases.rel(s1[k], s0[k]) < 1e-4, k


def test_prototype_full_train_step(tmp_path):
    """One Trainer_prototype_full step with a DRN generator at 128^2, B = 2 + 2: finite losses, every parameter moves (target
    prototypes from the soft predictions, as in test_xception_gpu.py; the retrified path runs in tests/bench_drn.py at 512^2)."""
    from make_golden_inputs import synth_loader
    from oracle import step_ref
    from uda_clr_amd.networks.GAN import BoundaryDiscriminator, UncertaintyDiscriminator
    from uda_clr_amd.train_process import Trainer_prototype_full
    m = model_cases.seeded_model(backbone="drn").to(DEV).train()
    torch.manual_seed(3)
    d1, d2 = BoundaryDiscriminator().to(DEV), UncertaintyDiscriminator().to(DEV)
    og, od, od2 = step_ref.make_optimizers(m, d1, d2)
    loaderS, loaderT = synth_loader(1, 2, 128, 500), synth_loader(1, 2, 128, 700)
    tr = Trainer_prototype_full.Trainer(
        cuda=True, model_gen=m, model_dis=d1, model_uncertainty_dis=d2, optimizer_gen=og, optimizer_dis=od,
        optimizer_uncertainty_dis=od2, lr_gen=1e-3, lr_dis=2.5e-5, val_loader=loaderT, domain_loaderS=loaderS,
        domain_loaderT=loaderT, out=str(tmp_path), max_epoch=1, stop_epoch=1, interval_validate=100, batch_size=2, warmup_epoch=-1,
        target_name="RIM-ONE_r3", use_pid=True, retrify_pesudo=False)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    row = tr.train_step(loaderS[0], loaderT[0])
    torch.cuda.synchronize()
    assert all(torch.isfinite(torch.tensor(float(v))) for v in row), row
    moved = [k for k, v in m.named_parameters() if not torch.equal(v.detach(), before[k])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))[:10]


def test_drn_per_gpu_batch_8_at_512_properties():
    """Full-size properties (B = 8, 512^2; the oracle runs the 128^2 / 256^2 fixtures, not this): eval batch independence;
    permuting the training batch (and its dropout masks) permutes the outputs and leaves gradients and running statistics
    unchanged up to summation order; every parameter has a finite gradient, none is left out of the bound."""
    from uda_clr_amd import ops
    B, S = 8, 512
    g = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(B, 3, S, S, generator=g, device=DEV)
    keep = lambda shp, p: (torch.rand(shp, generator=g, device=DEV) >= p).to(torch.uint8)
    sites = {"aspp.dropout": ((256, S // 8, S // 8), 0.5), "decoder.last_conv_boundary.3": ((256, S // 4, S // 4), 0.5),
             "decoder.last_conv_boundary.7": ((256, S // 4, S // 4), 0.1), "decoder.last_conv.2": ((305, S // 4, S // 4), 0.1)}
    masks = {k: keep((B,) + shp, p) for k, (shp, p) in sites.items()}
    m = model_cases.seeded_model(perturb=True, backbone="drn").to(DEV)
    m.eval()
    with torch.no_grad():
        full = m(x)
        part = m(x[2:4].contiguous())
    for n, a, b in zip(model_cases.NAMES, full, part):
        assert model_cases.rel(a[2:4], b) < 1e-5, n
    del full, part
    tmap = (torch.rand(B, 2, S, S, generator=g, device=DEV) > 0.5).float()
    tbd = torch.rand(B, 1, S, S, generator=g, device=DEV)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(DEV)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    runs = []
    for p in (None, perm):
        m.load_state_dict(sd0)
        m.train()
        for q in m.parameters():
            q.grad = None
        sel = (lambda t: t) if p is None else (lambda t: t[p].contiguous())
        m.set_dropout_masks({k: sel(v) for k, v in masks.items()})
        out = m(sel(x))
        ops.seg_loss(out[0], out[1], sel(tmap), sel(tbd)).backward()
        runs.append((out[0].detach(), {k: q.grad.clone() for k, q in m.named_parameters()},
                     {k: v.clone() for k, v in m.state_dict().items() if "running" in k}))
        del out
    (o0, g0, r0), (o1, g1, r1) = runs
    assert all(bool(torch.isfinite(v).all()) for v in g0.values()) and len(g0) == len(list(m.parameters())) == 204
    assert model_cases.rel(o1, o0[perm]) < 2e-4
    for k in r0:
        assert model_cases.rel(r1[k], r0[k]) < 3e-4, k
    errs = sorted((model_cases.l2rel(g1[k], g0[k]), k) for k in g0)
    print("drn B=8 512^2: permutation test, median %.2e worst %s" % (errs[len(errs) // 2][0], errs[-1]))
    assert errs[len(errs) // 2][0] < 5e-3 and errs[-1][0] < 2e-2, (errs[len(errs) // 2], errs[-1])
