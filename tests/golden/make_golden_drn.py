#!/usr/bin/env python
"""Generate the DRN-D-54 fixtures in tests/golden/ from the REFERENCE itself.

Run in the build container only (needs the reference tree, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_drn.py

Reuses the shims and writers of make_golden.py.  Two more shims stand between the reference's drn.py and a running model,
both installed here and neither an edit of the reference:

  * ``torch.utils.model_zoo.load_url`` is replaced by a function that raises BEFORE anything of the reference is imported, and
    ``drn.drn_d_54`` is wrapped so that it is always called with ``pretrained=False`` (its default would download);
  * ``drn.SynchronizedBatchNorm2d`` (a name drn.py:164,262 test against but never import) is bound to ``nn.BatchNorm2d``.

Writes

  manifest_drn.json        state-dict keys / shapes / seeded-init sums of DeepLab(backbone='drn')
  forward_drn_128.npz      B = 2, 128^2  (eval outputs, train outputs, loss, gradient norms, running-stat sums, dropout-mask
  forward_drn_256.npz      B = 2, 256^2   sums; same fields as forward_resnet_128.npz plus ``output_stride`` = 8)

and compares tests/drn_ref.py (the functional oracle of the DRN tests) with the reference on full tensors while doing so: a
mismatch exits non-zero.  ``noise`` (on by default) prints what the reference alone does on these cases: per-tensor gradient
distance fp32 <-> fp64, gradient norms of two fp32 runs (1 thread <-> 8 threads) and outputs fp32 <-> fp64 - the floor the
fixture bounds of the tests sit above.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _refuse(*a, **k):
    raise SystemExit("the reference tried to download pretrained weights: the pretrained=False shim is not in place")


import torch.utils.model_zoo as _model_zoo  # noqa: E402

_model_zoo.load_url = _refuse               # before anything of the reference is imported

import make_golden  # noqa: E402
from make_golden import install_reference, make_manifest, ref_model, synth_targets  # noqa: E402,F401


def install_drn_shims():
    from networks.backbone import drn
    drn.model_zoo.load_url = _refuse
    drn.SynchronizedBatchNorm2d = torch.nn.BatchNorm2d
    d54 = drn.drn_d_54
    drn.drn_d_54 = lambda BatchNorm, pretrained=True: d54(BatchNorm, pretrained=False)


def make_forward(m, B, S, tag):
    """make_golden.make_forward with the DRN oracle in place of oracle.deeplab_ref's forward."""
    import drn_ref
    from oracle import deeplab_ref
    keep = deeplab_ref.deeplab_forward
    deeplab_ref.deeplab_forward = drn_ref.deeplab_forward
    try:
        make_golden.make_forward(m, B, S, tag)
    finally:
        deeplab_ref.deeplab_forward = keep
    path = os.path.join(HERE, "forward_%s.npz" % tag)
    z = dict(np.load(path))
    z["output_stride"] = np.int64(8)
    np.savez_compressed(path, **z)


def noise_report(m, B, S):
    """The reference alone on this case (dropout off, the BCE + MSE loss of the fixtures): fp32 on 1 thread, fp32 on 8 threads
    and the same modules in fp64."""
    import copy
    torch.manual_seed(0)
    x = torch.randn(B, 3, S, S)
    tmap, tbd = synth_targets(B, S, S, 11)

    def run(model, dt, threads):
        keep = torch.get_num_threads()
        torch.set_num_threads(threads)
        try:
            model = copy.deepcopy(model).to(dt).train()
            for mod in model.modules():
                if isinstance(mod, torch.nn.Dropout):
                    mod.eval()
            out = model(x.to(dt))
            loss = torch.nn.BCELoss()(torch.sigmoid(out[0]), tmap.to(dt)) + torch.nn.MSELoss()(torch.sigmoid(out[1]), tbd.to(dt))
            loss.backward()
            return [o.detach().double() for o in out], {k: p.grad.double() for k, p in model.named_parameters()}
        finally:
            torch.set_num_threads(keep)

    o1, g1 = run(m, torch.float32, 1)
    o8, g8 = run(m, torch.float32, 8)
    o64, g64 = run(m, torch.float64, 8)
    d1 = np.array([((g1[k] - g64[k]).norm() / g64[k].norm().clamp_min(1e-30)).item() for k in g64])
    d8 = np.array([((g8[k] - g64[k]).norm() / g64[k].norm().clamp_min(1e-30)).item() for k in g64])
    n1, n8 = np.array([g1[k].norm().item() for k in g64]), np.array([g8[k].norm().item() for k in g64])
    rel = np.abs(n1 - n8) / np.maximum(n8, 1e-12)
    conv = np.array([g64[k].dim() == 4 for k in g64])
    keys = list(g64)
    outd = max(((a - c).abs().max() / c.abs().max()).item() for a, c in zip(o1, o64))
    print("reference noise floor, DRN %d^2, B = %d" % (S, B))
    print("  per-tensor gradient distance fp32 <-> fp64 (l2, relative): median %.2e (1 thread) / %.2e (8 threads), worst %.2e; "
          "%d of %d tensors above 5e-3; %d with a zero gradient"
          % (np.median(d1), np.median(d8), max(d1.max(), d8.max()), int((d1 > 5e-3).sum()), len(d1),
             int(sum(float(g64[k].norm()) == 0.0 for k in g64))))
    print("  gradient norm fp32 (1 thread) <-> fp32 (8 threads): median %.2e / worst conv %.2e / worst any tensor %.2e (%s)"
          % (np.median(rel), rel[conv].max(), rel.max(), keys[int(rel.argmax())]))
    print("  outputs fp32 <-> fp64: %.2e" % outd)


if __name__ == "__main__":
    install_reference()
    install_drn_shims()
    which = sys.argv[1:] or ["manifest", "128", "256", "noise"]
    m = make_manifest("drn", "manifest_drn.json") if "manifest" in which else ref_model(backbone="drn")
    for size in (128, 256):
        if str(size) in which:
            make_forward(m, 2, size, "drn_%d" % size)
            if "noise" in which:
                noise_report(m, 2, size)
    print("drn fixtures written to", HERE)
