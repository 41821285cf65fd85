"""Multi-step trainer parity (TEST INFRASTRUCTURE): every training step of a product Trainer, with the machinery that carries
state from one step to the next switched on, against the fp64 oracle evaluated AT THE TRAINER'S OWN STATE before that step.

A free-running trajectory cannot give a sharp test (tests/tools/trajectory_anchor.py: Adam's first, sign-like step alone is 6 %
from fp64 in the reference's own fp32).  Restarting the oracle from the product's state at every step removes the trajectory
divergence, so step k is held to the same bound as step 1.  A cache that survives an optimizer step (a kernel-side weight layout,
a bf16x3-packed weight, the activations the MC fast path reuses, the gradient stash of ``fused_grad_accumulation``) makes step k
a function of stale state and moves the affected layers by about one Adam update (~1e-2 relative).

  * ``RecordingDeepLab`` - the product DeepLab (a subclass: every method the trainers probe with ``hasattr`` stays present) that
    draws the dropout keep-masks of every training forward and every MC pass from a seeded CPU generator, records them, counts
    how often each cache path ran, and can inject the faults the sensitivity tests need.
  * ``OptimSpy`` - wraps ``step`` of an optimizer AFTER the trainer took it over (a wrapped Adam would not be taken over):
    parameters, gradients and moments before the step, parameters after it; ``update_err`` replays torch's update rule in fp64.
  * ``run`` - drives the trainer step by step; after each step the oracle (``oracle_step``) runs the same step from the snapshot
    in fp64 (all host threads) and in fp32 on ONE host thread (the yardstick of ``model_cases.grads_ok``), and ``compare``
    returns the per-step errors.
"""
from __future__ import annotations

import collections
import contextlib
import glob
import math
import os
import re

import torch

import model_cases
from make_golden_inputs import synth_loader
from oracle import deeplab_ref, gan_ref, step_ref
from uda_clr_amd.networks.deeplabv3 import DeepLab

TRAIN_PROCESS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uda_clr_amd", "train_process")


def probed_names():
    """Every attribute name the trainers probe with ``hasattr(<obj>, "<name>")``."""
    names = set()
    for path in glob.glob(os.path.join(TRAIN_PROCESS, "*.py")):
        names |= set(re.findall(r"hasattr\(\s*[\w.]+\s*,\s*['\"](\w+)['\"]\s*\)", open(path).read()))
    return names


# ------------------------------------------------------------------------------------------------------------------ generator
class RecordingDeepLab(DeepLab):
    """The product generator with seeded, recorded dropout masks and counters; ``adopt`` turns a built DeepLab into one.

    faults (sensitivity tests only): "stale_wshare" - ``shared_weight_layouts`` hands over ONE dict for all steps (layouts of the
    parameters before the first optimizer step); "drop_accum" - the multi-tensor add of ``fused_grad_accumulation`` is skipped
    (the later pass's gradients are lost)."""

    @classmethod
    def adopt(cls, m, seed=123, faults=()):
        m.__class__ = cls
        m._mask_gen = torch.Generator().manual_seed(seed)
        m.mask_log = []                        # keep-masks in call order: ("fwd", {site: mask}) / ("mc", [{site: mask}] * passes)
        m.counts = collections.Counter()
        m.faults = set(faults)
        m._stale = {}
        return m

    def _draw(self, n, h, w):
        return deeplab_ref.draw_masks(n, h, w, self._mask_gen)

    def _dev(self, masks):
        dev = next(self.parameters()).device
        return {k: v.to(dev) for k, v in masks.items()}

    def forward(self, input):
        if self.training and self._next_masks is None:
            masks = self._draw(input.shape[0], input.shape[2], input.shape[3])
            self.mask_log.append(("fwd", masks))
            self.set_dropout_masks(self._dev(masks))
        self.counts["forward"] += 1
        return super().forward(input)

    def mc_dropout_logits(self, x, passes=4, reps=2, masks=None):
        assert masks is None
        masks = [self._draw(reps * x.shape[0], x.shape[2], x.shape[3]) for _ in range(passes)]
        self.mask_log.append(("mc", masks))
        before = self.counts["forward"]
        out = super().mc_dropout_logits(x, passes=passes, reps=reps, masks=[self._dev(m) for m in masks])
        self.counts["mc_plain" if self.counts["forward"] > before else "mc_fast"] += 1
        return out

    def shared_weight_layouts(self):
        self.counts["wshare"] += 1
        if "stale_wshare" not in self.faults:
            return super().shared_weight_layouts()

        @contextlib.contextmanager
        def stale():
            keep, self._wshare = self._wshare, self._stale
            try:
                yield self
            finally:
                self._wshare = keep
        return stale()

    def fused_grad_accumulation(self):
        self.counts["accum_scope"] += 1
        n = sum(1 for p in self.parameters() if p.requires_grad)
        inner = super().fused_grad_accumulation()
        orig, counts, drop = torch._foreach_add_, self.counts, "drop_accum" in self.faults

        def spy(a, b, *args, **kw):
            if len(a) == n:                    # the generator's stash add (the engines' own adds are shorter lists)
                counts["accum_add"] += 1
                if drop:
                    return None
            return orig(a, b, *args, **kw)

        @contextlib.contextmanager
        def scope():
            torch._foreach_add_ = spy
            try:
                with inner:
                    yield self
            finally:
                torch._foreach_add_ = orig
        return scope()

    def note_params_changed(self):
        self.counts["note_params_changed"] += 1
        return super().note_params_changed()


def instrument_discriminator(d, counts, tag, stale=False):
    """Count the trainer's ``shared_weight_layouts`` scopes of a product discriminator; ``stale``: one dict for all steps."""
    if not hasattr(d, "shared_weight_layouts"):
        return d
    orig, persistent = d.shared_weight_layouts, {}

    def shared_weight_layouts():
        counts["wshare_" + tag] += 1
        if not stale:
            return orig()

        @contextlib.contextmanager
        def scope():
            keep, d._wshare = d._wshare, persistent
            try:
                yield d
            finally:
                d._wshare = keep
        return scope()
    d.shared_weight_layouts = shared_weight_layouts
    return d


# ------------------------------------------------------------------------------------------------------------------ optimizers
class OptimSpy:
    """Wraps ``opt.step`` (instance attribute): per step the pre-step parameters, gradients, moments / momentum buffers and step
    count, and the post-step parameters, all on the host."""

    def __init__(self, opt, names):
        self.opt, self.names, self.steps = opt, names, []
        self._orig = opt.step
        opt.step = self._step

    def _params(self):
        return [p for g in self.opt.param_groups for p in g["params"]]

    def _step(self, *a, **k):
        opt = self.opt
        rec = {"pre": {}, "grad": {}, "state": {}, "hyper": {}, "post": {}}
        # FlatAdam keeps one step count for all parameters (the per-parameter "step" tensors are synced only on demand) until it
        # hands over to torch's own per-parameter counts for good (_torch_steps)
        t = opt._step if hasattr(opt, "_step") and not getattr(opt, "_torch_steps", False) else None
        for g in opt.param_groups:
            for p in g["params"]:
                n = self.names[id(p)]
                rec["pre"][n] = p.detach().double().cpu()
                rec["grad"][n] = None if p.grad is None else p.grad.detach().double().cpu()
                st = opt.state.get(p, {})
                rec["state"][n] = {k2: (float(v) if k2 == "step" else v.detach().double().cpu())
                                   for k2, v in st.items() if isinstance(v, torch.Tensor) or k2 == "step"}
                if t is not None:
                    rec["state"][n]["step"] = float(t)
                rec["hyper"][n] = {k2: g[k2] for k2 in ("lr", "betas", "eps", "momentum", "weight_decay", "dampening", "nesterov")
                                   if k2 in g}
        out = self._orig(*a, **k)
        for p in self._params():
            rec["post"][self.names[id(p)]] = p.detach().double().cpu()
        self.steps.append(rec)
        return out

    def update_err(self, rec=None):
        """max over tensors of |post - torch's rule(pre, grad, state)| / max|pre| (fp64 replay of Adam / SGD)."""
        rec = rec if rec is not None else self.steps[-1]
        worst = 0.0
        for n, p in rec["pre"].items():
            g, st, h = rec["grad"][n], rec["state"][n], rec["hyper"][n]
            if g is None:
                want = p
            elif "betas" in h:                              # Adam (torch.optim.adam, amsgrad / weight decay off)
                b1, b2 = h["betas"]
                t = st.get("step", 0.0) + 1
                m = b1 * st.get("exp_avg", torch.zeros_like(p)) + (1 - b1) * g
                v = b2 * st.get("exp_avg_sq", torch.zeros_like(p)) + (1 - b2) * g * g
                denom = v.sqrt() / math.sqrt(1 - b2 ** t) + h["eps"]
                want = p - h["lr"] / (1 - b1 ** t) * m / denom
            else:                                           # SGD with momentum (no dampening, no Nesterov)
                d = g + h.get("weight_decay", 0.0) * p
                buf = st.get("momentum_buffer")
                buf = d if buf is None or h.get("momentum", 0.0) == 0 else h["momentum"] * buf + d
                want = p - h["lr"] * buf
            scale = max(p.abs().max().item(), (want - p).abs().max().item(), 1e-30)       # (a zero-initialised bias: its update)
            worst = max(worst, (rec["post"][n] - want).abs().max().item() / scale)
        return worst


class GradCapture:
    """Optimizer stand-in for the oracle step: zero_grad / step only record the gradients (parameters stay put)."""

    def __init__(self, named):
        self.named, self.grads = list(named), None

    def zero_grad(self):
        for _, p in self.named:
            p.grad = None

    def step(self):
        self.grads = {n: (None if p.grad is None else p.grad.detach().clone()) for n, p in self.named}


# ------------------------------------------------------------------------------------------------------------------ oracle
class _QueuedOracle(deeplab_ref.OracleDeepLab):
    """The oracle generator taking the recorded keep-masks, one set per training forward, in call order."""

    def forward(self, x):
        self.masks = self.queue.pop(0) if self.training else None
        return super().forward(x)


def _mask_queue(log):
    q = []
    for kind, m in log:
        q.extend([m] if kind == "fwd" else m)
    return q


def oracle_step(snap, kind, batch, dtype):
    """One step of the oracle from ``snap`` (the product's state before the step) with the recorded masks.  Returns
    {"row", "gen_grads", "dis_grads", "buffers", "centroids", "maps"} (fp64 / fp32 values, per ``dtype``)."""
    g = _QueuedOracle(snap["gen"], output_stride=snap.get("output_stride", 16)).to(dtype).train()
    g.queue = [{k: v.clone() for k, v in m.items()} for m in _mask_queue(snap["masks"])]
    gnamed = [(k, v) for k, v in g.flat_state().items() if isinstance(v, torch.nn.Parameter)]
    cg = GradCapture(gnamed)
    c = lambda t: t.to(dtype)
    out = {}
    if kind == "baseline":
        img, tmap, tbd = batch
        seg = step_ref.baseline_step(g, cg, c(img), c(tmap), c(tbd))
        out["row"] = {"seg": seg}
    else:
        d1, d2 = gan_ref.BoundaryDiscriminator(), gan_ref.UncertaintyDiscriminator()
        d1.load_state_dict(snap["dis"]); d2.load_state_dict(snap["dis2"])
        d1.to(dtype); d2.to(dtype)
        c1 = GradCapture([("dis." + n, p) for n, p in d1.named_parameters()])
        c2 = GradCapture([("dis2." + n, p) for n, p in d2.named_parameters()])
        st = step_ref.PrototypeFullStep(g, d1, d2, cg, c1, c2, use_pid=True, retrify_pesudo=True)
        st.bank.state = {k: (None if v is None else tuple(c(t) for t in v)) for k, v in snap["centroids"].items()}
        img, tmap, tbd, imgT = batch
        out["row"] = st(c(img), c(tmap), c(tbd), c(imgT))
        out["dis_grads"] = dict(c1.grads, **c2.grads)
        out["centroids"] = st.bank.state
        out["maps"] = st.retrify_maps
    assert not g.queue, "the oracle step used fewer masks than the product step drew"
    out["gen_grads"] = cg.grads
    out["buffers"] = {k: v.detach().clone() for k, v in g.flat_state().items() if model_cases._is_running(k)}
    return out


# ------------------------------------------------------------------------------------------------------------------ driver
ROW_NAMES = {"proto": ("seg", "adv", "D_same", "D_diff", "intra", "inter"), "baseline": ("seg",)}


def _host(t):
    return t.detach().cpu().clone()


def snapshot(tr, kind, gen):
    s = {"gen": {k: _host(v) for k, v in gen.state_dict().items()}, "output_stride": gen.output_stride}
    if kind == "proto":
        s["dis"] = {k: _host(v) for k, v in tr.model_dis.state_dict().items()}
        s["dis2"] = {k: _host(v) for k, v in tr.model_dis2.state_dict().items()}
        s["centroids"] = {"src": None if tr.src_centroids is None else tuple(_host(t).reshape(1, -1, 1, 1) for t in tr.src_centroids),
                          "tgt": None if tr.tgt_centroids is None else tuple(_host(t).reshape(1, -1, 1, 1) for t in tr.tgt_centroids)}
    return s


def make_trainer(kind, gen, dev, tmp, S, B, cpu_oracle_dis=False, stale_dis=(), lr_dis=2.5e-5):
    """The product trainer around ``gen`` (a RecordingDeepLab on ``dev``), spies attached after construction."""
    import oracle_ops
    from uda_clr_amd.networks.GAN import BoundaryDiscriminator, UncertaintyDiscriminator
    from uda_clr_amd.train_process import Trainer_baseline, Trainer_prototype_full
    loader = synth_loader(1, B, S, 40)
    if kind == "baseline":
        og = torch.optim.Adam(gen.parameters(), lr=1e-3, betas=(0.9, 0.99))
        tr = Trainer_baseline.Trainer(cuda=dev.type == "cuda", model_gen=gen, optimizer_gen=og, val_loader=loader,
                                      domain_loaderS=loader, domain_loaderT=loader, out=str(tmp), max_epoch=1, lr_gen=1e-3,
                                      batch_size=B, warmup_epoch=-1)
    else:
        torch.manual_seed(1338)
        if cpu_oracle_dis:
            d1, d2 = gan_ref.BoundaryDiscriminator(), gan_ref.UncertaintyDiscriminator()
        else:
            d1, d2 = BoundaryDiscriminator().to(dev), UncertaintyDiscriminator().to(dev)
        og, od, od2 = step_ref.make_optimizers(gen, d1, d2, lr_dis=lr_dis)
        tr = Trainer_prototype_full.Trainer(
            cuda=dev.type == "cuda", model_gen=gen, model_dis=d1, model_uncertainty_dis=d2, optimizer_gen=og, optimizer_dis=od,
            optimizer_uncertainty_dis=od2, val_loader=loader, domain_loaderS=loader, domain_loaderT=loader, out=str(tmp),
            max_epoch=1, use_global=True, use_pid=True, retrify_pesudo=True, global_pro_weight=0.9, pro_weight=0.1,
            lr_gen=1e-3, lr_dis=lr_dis, batch_size=B, warmup_epoch=-1)
        instrument_discriminator(d1, gen.counts, "dis", stale="dis" in stale_dis)
        instrument_discriminator(d2, gen.counts, "dis2", stale="dis2" in stale_dis)
    if dev.type != "cuda":
        tr.ops = oracle_ops.OracleOps()
    names = {id(v): k for k, v in gen._flat_state().items()}
    tr.spies = {"gen": OptimSpy(tr.optim_gen, names)}
    if kind == "proto":
        tr.spies["dis"] = OptimSpy(tr.optim_dis, {id(p): "dis." + n for n, p in tr.model_dis.named_parameters()})
        tr.spies["dis2"] = OptimSpy(tr.optim_dis2, {id(p): "dis2." + n for n, p in tr.model_dis2.named_parameters()})
    tr.epoch, tr.iteration = 0, 0
    return tr


def batches(kind, B, S, steps, seed=70):
    out = []
    for k in range(steps):
        s = synth_loader(1, B, S, seed + 2 * k)[0]
        t = synth_loader(1, B, S, seed + 2 * k + 1)[0]
        out.append((s, t))
    return out


def product_step(tr, kind, sample_s, sample_t):
    if kind == "baseline":
        tr.domain_loaderS = [sample_s]
        tr.train_epoch()
        return {"seg": tr.running_seg_loss}
    vals = tr.train_step(sample_s, sample_t)
    return dict(zip(ROW_NAMES["proto"], vals))


def _stat_err(a, b):
    """max |a - b| / max |b| with an absolute floor of 1e-3: a running mean whose batch means are zero to rounding (a BN over
    a constant input) is measured against the floor instead of against ~0."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-3)


def _worst(grads):
    """max over tensors of err / (grad_ok bound): 1.0 = the bound of ``model_cases.grads_ok``, including its tail allowance (at most
    two tensors whose fp32-oracle distance is above 5e-3 may sit between 10x and 30x; they are measured against 30x)."""
    fail = [k for k, v in grads.items() if not model_cases.grad_ok(*v)]
    tail = {k for k in fail if grads[k][1] > 5e-3 and model_cases.grad_ok(*grads[k], factor=30.0)}
    tail = tail if len(tail) <= 2 else set()
    return max(v[0] / ((30.0 if k in tail else 10.0) * v[1] + 2e-3) for k, v in grads.items())


def compare(kind, tr, gen, row, o64, o32):
    """Errors of one product step against the fp64 oracle at the same state."""
    live = gen._flat_state()
    rep = {}
    for n in ROW_NAMES[kind]:
        rep["scalar." + n] = abs(row[n] - o64["row"][n]) / max(abs(o64["row"][n]), 1e-12)
    spy = tr.spies["gen"].steps[-1]
    grads = {}
    for k, g64 in o64["gen_grads"].items():
        g = spy["grad"].get(k)
        grads[k] = (float("inf") if g is None else model_cases.l2rel(g, g64), model_cases.l2rel(o32["gen_grads"][k], g64))
    bad, gmean = model_cases.grads_ok(grads)
    rep["gen_grads.bad"], rep["gen_grads.gmean"] = sorted(bad), gmean
    rep["gen_grads.worst"] = _worst(grads)
    rep["bn_running"] = max(_stat_err(live[k], v) for k, v in o64["buffers"].items())
    rep["update.gen"] = tr.spies["gen"].update_err()
    if kind == "proto":
        dg = {}
        for tag in ("dis", "dis2"):
            sp = tr.spies[tag].steps[-1]
            for k, g64 in o64["dis_grads"].items():
                if k.startswith(tag + "."):
                    g = sp["grad"].get(k)
                    dg[k] = (float("inf") if g is None else model_cases.l2rel(g, g64), model_cases.l2rel(o32["dis_grads"][k], g64))
            rep["update." + tag] = tr.spies[tag].update_err()
        rep["dis_grads.bad"] = sorted(k for k, v in dg.items() if not model_cases.grad_ok(*v))
        rep["dis_grads.worst"] = max(v[0] / (10 * v[1] + 2e-3) for v in dg.values())
        cen = [(_host(a).reshape(-1), b.reshape(-1)) for which in ("src", "tgt")
               for a, b in zip(getattr(tr, which + "_centroids"), o64["centroids"][which])]
        rep["centroids"] = max(model_cases.rel(a, b) for a, b in cen)
        std64, m0, m1 = o64["maps"]
        rep["std_map"] = model_cases.rel(tr.target_std_map, std64)
        rep["mask_flips"] = int((_host(tr.mask_0).double() != m0).sum() + (_host(tr.mask_1).double() != m1).sum())
    return rep


def run(kind, gen, dev, tmp, B, S, steps, faults=(), stale_dis=(), cpu_oracle_dis=False, before_step=None, seed=70, lr_dis=2.5e-5):
    """Drive ``steps`` product steps; returns (per-step reports, the trainer).  ``gen``: a DeepLab already on ``dev``."""
    RecordingDeepLab.adopt(gen, faults=faults)
    tr = make_trainer(kind, gen, dev, tmp, S, B, cpu_oracle_dis=cpu_oracle_dis, stale_dis=stale_dis, lr_dis=lr_dis)
    gen.train()
    if kind == "proto":
        tr.model_dis.train(); tr.model_dis2.train()
    reports = []
    for k, (s, t) in enumerate(batches(kind, B, S, steps, seed)):
        if before_step is not None:
            before_step(k, tr)
        snap = snapshot(tr, kind, gen)
        gen.mask_log = []
        counts0 = collections.Counter(gen.counts)
        row = product_step(tr, kind, s, t)
        if dev.type == "cuda":
            torch.cuda.synchronize()
        snap["masks"] = gen.mask_log
        batch = (s["image"], s["map"], s["boundary"]) + ((t["image"],) if kind == "proto" else ())
        o64 = oracle_step(snap, kind, batch, torch.float64)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)            # the fp32 yardstick on ONE host thread, as model_cases.train_parity
        try:
            o32 = oracle_step(snap, kind, batch, torch.float32)
        finally:
            torch.set_num_threads(threads)
        rep = compare(kind, tr, gen, row, o64, o32)
        rep["counts"] = dict(gen.counts - counts0)
        reports.append(rep)
    return reports, tr


def table(title, reports, bounds):
    """Per-step table: error, bound, ratio."""
    lines = ["%s" % title, "%-22s %5s %12s %12s %8s" % ("quantity", "step", "error", "bound", "ratio")]
    for name, bound in bounds.items():
        for k, rep in enumerate(reports):
            if name in rep:
                e = rep[name]
                lines.append("%-22s %5d %12.3e %12.3e %8.3f" % (name, k + 1, e, bound, e / bound if bound else float("nan")))
    lines.append("counters per step: " + "; ".join(str(dict(sorted(r["counts"].items()))) for r in reports))
    return "\n".join(lines)


def violations(reports, bounds):
    """[(step, quantity, error, bound)] of every bounded quantity over its bound.  The gradient criteria are bounded quantities too:
    ``gen_grads.worst`` / ``dis_grads.worst`` (1.0 = ``model_cases.grad_ok``'s bound, grads_ok's tail allowance included) and
    ``gen_grads.gmean`` (``model_cases.grads_ok``: 1.5)."""
    return [(k + 1, name, rep[name], bound) for k, rep in enumerate(reports) for name, bound in bounds.items()
            if name in rep and not rep[name] <= bound]
