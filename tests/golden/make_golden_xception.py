#!/usr/bin/env python
"""Generate the Aligned Xception fixtures in tests/golden/ from the REFERENCE itself.

Run in the build container only (needs the reference tree, which never travels):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_xception.py

Reuses the shims and writers of make_golden.py; the reference's ``AlignedXception._load_pretrained_model`` (a download
whose result it then discards: every key is filtered against an empty dict) is patched to a no-op.  Writes

  manifest_xception.json          state-dict keys / shapes / seeded-init sums of DeepLab(backbone='xception')
  forward_xception_128.npz        OS16, B = 2, 128^2  (eval outputs, train outputs, loss, gradient norms, running-stat
  forward_xception_256.npz        OS16, B = 2, 256^2   sums, dropout-mask sums; same fields as forward_resnet_128.npz
  forward_xception_os8_128.npz    OS8,  B = 2, 128^2   plus ``output_stride``)

and compares tests/xception_ref.py (the functional oracle of the Xception tests) with the reference on full tensors while
doing so: a mismatch exits non-zero.
"""
import functools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
from make_golden import install_reference, make_manifest, ref_model, summarize, synth_targets  # noqa: E402,F401


def _ref_xception(output_stride):
    if output_stride == 16:
        return ref_model(backbone="xception")
    from networks.deeplabv3 import DeepLab
    torch.manual_seed(1337)
    return DeepLab(num_classes=2, backbone="xception", output_stride=output_stride, sync_bn=True, freeze_bn=False,
                   method="prototype_full")


def make_forward(m, B, S, tag, output_stride):
    """make_golden.make_forward with the Xception oracle in place of oracle.deeplab_ref's forward."""
    import xception_ref
    from oracle import deeplab_ref
    keep = deeplab_ref.deeplab_forward
    deeplab_ref.deeplab_forward = functools.partial(xception_ref.deeplab_forward, output_stride=output_stride)
    try:
        make_golden.make_forward(m, B, S, tag)
    finally:
        deeplab_ref.deeplab_forward = keep
    path = os.path.join(HERE, "forward_%s.npz" % tag)
    z = dict(np.load(path))
    z["output_stride"] = np.int64(output_stride)
    np.savez_compressed(path, **z)


if __name__ == "__main__":
    install_reference()
    from networks.backbone import xception
    xception.AlignedXception._load_pretrained_model = lambda self: None
    which = sys.argv[1:] or ["manifest", "128", "256", "os8"]
    m = make_manifest("xception", "manifest_xception.json") if "manifest" in which else _ref_xception(16)
    if "128" in which:
        make_forward(m, 2, 128, "xception_128", 16)
    if "256" in which:
        make_forward(m, 2, 256, "xception_256", 16)
    del m
    if "os8" in which:
        make_forward(_ref_xception(8), 2, 128, "xception_os8_128", 8)
    print("xception fixtures written to", HERE)
