"""The cases that the Aligned Xception and the DRN-D-54 tests share (test_{xception,drn}_{cpu,gpu}.py call them with their
backbone's name, output stride and oracle forward): bounds are those of the ResNet-101 cases in test_generator_gpu.py."""
import torch

import model_cases
from oracle import deeplab_ref

GOLDEN_BOUNDS = {"train.grad_norm.conv": 5e-2, "train.grad_norm.median": 2e-2, "train.bn_sum": 5e-3}


def golden_errors(dev, tag, backbone, oracle_forward, engine=None, **fixture_holds):
    """model_cases.golden_parity for this backbone (``engine``: CPU tests' kernel statement)."""
    # running-stat sums relative to max(|ref|, 1e-2), not 1e-3 as for the other backbones: the outer BN of a separable conv reads a
    # BN output through a 1x1 conv, so its batch mean is W * beta of the inner BN, analytically 0 at the seeded init (reference:
    # |sum| ~ 1e-7 over 1536-2048 channels).  Measured on MI355X: the exit flow's bn3 / bn4 / bn5 running means come out at
    # -0.9 ... -2.0e-5 (1e-8 per channel, ~1e-7 of the unit-variance activations), 2.0e-2 against the 1e-3 floor and 2.0e-3
    # against this one; every other running statistic sits within 1.2e-7 of the fixture, the fp64 oracle within 3.5e-4.
    # (DRN's fixtures are held to the Xception ones' floor.)
    return model_cases.golden_parity(dev, tag, backbone=backbone, oracle_forward=oracle_forward, engine=engine, stat_floor=1e-2,
                                     **fixture_holds)


def check_golden(errs):
    for k, v in errs.items():
        bound = GOLDEN_BOUNDS.get(k, 1e-3 if k.startswith(("eval.", "train.loss")) else 5e-3)
        assert v < bound, (k, v, bound)


def train_checks(fwd64, grads, stats, stats_bound=5e-3, gmean_bound=4.0, n_grads=None):
    """Outputs within 3x the fp32 oracle's own fp64 distance, gradients by model_cases.grads_ok; ``n_grads``: no parameter is
    left out (none of DRN's gradients is analytically zero).  The defaults are the GPU cases' bounds."""
    for n, (e, floor) in fwd64.items():
        assert e < 3.0 * floor + 2e-4, (n, e, floor)
    assert stats < stats_bound, stats
    assert n_grads is None or len(grads) == n_grads
    assert all(v[0] < float("inf") for v in grads.values()), [k for k, v in grads.items() if v[0] == float("inf")]
    bad, gmean = model_cases.grads_ok(grads)
    print("gradient noise vs the fp32 oracle's: geometric mean %.3f over %d tensors" % (gmean, len(grads)))
    assert not bad, list(bad.items())[:10]
    assert gmean < gmean_bound, gmean


def mc_fast_path_equals_plain_stochastic_forwards(make_model, dev, output_stride):
    """GeneratorEngine.mc_forward (the backbone's activations reused) vs plain stochastic forwards on identical masks;
    ``make_model()``: a fresh training-mode model on ``dev``."""
    B, S, passes = 2, 64, 2
    gen = torch.Generator().manual_seed(8)
    x = torch.randn(B, 3, S, S, generator=gen).to(dev)

    def masks(n):
        mk = deeplab_ref.draw_masks(n, S, S, gen)
        if output_stride == 8:          # the ASPP output (and its dropout mask) lives at 1/8 resolution
            mk["aspp.dropout"] = (torch.rand(n, 256, S // 8, S // 8, generator=gen) >= 0.5).to(torch.uint8)
        return mk
    m0 = masks(B)
    mc_masks = [masks(2 * B) for _ in range(passes)]
    res = []
    for fast in (False, True):
        m = make_model()
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


def prototype_full_train_step(backbone, dev, tmp_path):
    """One Trainer_prototype_full step at 128^2, B = 2 + 2: finite losses, every parameter moves.  Target prototypes from the
    soft predictions (retrify_pesudo=False): with the retrified pseudo labels an untrained Xception generator's first step at
    this size gave a NaN loss (measured on MI355X, all generator outputs finite) - the uncertainty-masked class means of the
    pseudo labels, not the generator; the retrified path runs in tests/bench_xception.py / bench_drn.py at 512^2."""
    from make_golden_inputs import synth_loader
    from oracle import step_ref
    from uda_clr_amd.networks.GAN import BoundaryDiscriminator, UncertaintyDiscriminator
    from uda_clr_amd.train_process import Trainer_prototype_full
    m = model_cases.seeded_model(backbone=backbone).to(dev).train()
    torch.manual_seed(3)
    d1, d2 = BoundaryDiscriminator().to(dev), UncertaintyDiscriminator().to(dev)
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


def per_gpu_batch_8_at_512_properties(backbone, dev, output_stride, n_params=None, unmeasurable=()):
    """Full-size properties (B = 8, 512^2; the oracle runs the 128^2 / 256^2 fixtures, not this): eval batch independence;
    permuting the training batch (and its dropout masks) permutes the outputs and leaves gradients and running statistics
    unchanged up to summation order; every gradient finite, every parameter gets one (``n_params`` of them).  Gradients whose
    key ends in ``unmeasurable`` are left out of the permutation bound (see below)."""
    from uda_clr_amd import ops
    B, S = 8, 512
    g = torch.Generator(device=dev).manual_seed(4)
    x = torch.randn(B, 3, S, S, generator=g, device=dev)
    keep = lambda shp, p: (torch.rand(shp, generator=g, device=dev) >= p).to(torch.uint8)
    sa = S // output_stride
    sites = {"aspp.dropout": ((256, sa, sa), 0.5), "decoder.last_conv_boundary.3": ((256, S // 4, S // 4), 0.5),
             "decoder.last_conv_boundary.7": ((256, S // 4, S // 4), 0.1), "decoder.last_conv.2": ((305, S // 4, S // 4), 0.1)}
    masks = {k: keep((B,) + shp, p) for k, (shp, p) in sites.items()}
    m = model_cases.seeded_model(perturb=True, backbone=backbone).to(dev)
    m.eval()
    with torch.no_grad():
        full = m(x)
        part = m(x[2:4].contiguous())
    for n, a, b in zip(model_cases.NAMES, full, part):
        assert model_cases.rel(a[2:4], b) < 1e-5, n
    del full, part
    tmap = (torch.rand(B, 2, S, S, generator=g, device=dev) > 0.5).float()
    tbd = torch.rand(B, 1, S, S, generator=g, device=dev)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(dev)
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
    assert all(bool(torch.isfinite(v).all()) for v in g0.values()) and len(g0) == len(list(m.parameters()))
    assert n_params is None or len(g0) == n_params
    assert model_cases.rel(o1, o0[perm]) < 2e-4
    for k in r0:
        assert model_cases.rel(r1[k], r0[k]) < 3e-4, k
    # Xception leaves ".bn.bias" out: the inner BN of a separable conv (``.bn``, xception.py:21) feeds a 1x1 conv into a
    # training-mode BN, which removes any per-channel constant: its bias gradient is analytically zero, rounding noise in every
    # evaluation order (measured: 5e-2 l2rel between the two orders here) - there is nothing for the bound to measure.  DRN leaves
    # none out.
    errs = sorted((model_cases.l2rel(g1[k], g0[k]), k) for k in g0 if not k.endswith(unmeasurable))
    print("%s B=8 512^2: permutation test, median %.2e worst %s" % (backbone, errs[len(errs) // 2][0], errs[-1]))
    assert errs[len(errs) // 2][0] < 5e-3 and errs[-1][0] < 2e-2, (errs[len(errs) // 2], errs[-1])
