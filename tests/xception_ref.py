"""Functional CPU restatement of the reference generator with the Aligned Xception backbone.

TEST INFRASTRUCTURE.  ``oracle.deeplab_ref.deeplab_forward`` tells its two backbones apart by their keys and would take
Xception for a ResNet, so this file states the Xception network on its own: a flat ``state_dict`` (reference key names)
evaluated with ``torch.nn.functional`` ops, in the dtype of the tensors it is given (fp32 = the reference's arithmetic,
fp64 = the ground truth of the GPU bounds).  BatchNorm / dropout bookkeeping, mask drawing and state canonicalisation are
``oracle.deeplab_ref``'s own (``_Ctx``, ``draw_masks``, ``canonical_state``).

Reference anchors
  networks/backbone/xception.py   :8-14 fixed_padding, :17-31 SeparableConv2d, :34-90 Block (rep[0] is the shared
                                  in-place ReLU, so ``skip`` reads the RECTIFIED input), :93-177 flow geometry,
                                  :179-231 forward
  networks/aspp.py:65-78, networks/decoder.py:45-56, networks/deeplabv3.py:32-41
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle.deeplab_ref import _Ctx, canonical_state, draw_masks  # noqa: F401  (re-exported for the tests)
from uda_clr_amd.networks.backbone.xception import exit_plan, xception_plan


def _sep(c, x, pre, stride, dil):
    sd = c.sd
    C = x.shape[1]
    x = F.pad(x, (dil, dil, dil, dil))                 # fixed_padding of the (already rectified) input
    x = F.conv2d(x, sd[pre + ".conv1.weight"], None, stride, 0, dil, C)
    x = c.bn(x, pre + ".bn")
    return F.conv2d(x, sd[pre + ".pointwise.weight"])


def _block(c, z, pre, stride, has_skip, seps):
    """``z`` is the rectified block input (relu(z) for start_with_relu blocks - the in-place ReLU reaches the skip)."""
    h = z
    for j, (idx, ci, co, s, d) in enumerate(seps):
        if j:
            h = F.relu(h)
        h = c.bn(_sep(c, h, "%s.rep.%d" % (pre, idx), s, d), "%s.rep.%d" % (pre, idx + 1))
    if has_skip:
        skip = c.bn(F.conv2d(z, c.sd[pre + ".skip.weight"], None, stride), pre + ".skipbn")
    else:
        skip = z
    return h + skip


def xception_backbone(c, x, output_stride=16):
    sd = c.sd
    h = F.relu(c.bn(F.conv2d(x, sd["backbone.conv1.weight"], None, 2, 1), "backbone.bn1"))
    h = F.relu(c.bn(F.conv2d(h, sd["backbone.conv2.weight"], None, 1, 1), "backbone.bn2"))
    low = None
    for name, inp, planes, stride, has_skip, seps in xception_plan(output_stride):
        h = F.relu(_block(c, h, "backbone." + name, stride, has_skip, seps))
        if name == "block1":
            low = h
    for sep, bn, ci, co, d in exit_plan(output_stride):
        h = F.relu(c.bn(_sep(c, h, "backbone." + sep, 1, d), "backbone." + bn))
    return h, low


def deeplab_forward(sd, x, training=True, masks=None, record=None, output_stride=16, bn_training=None):
    """(x1, x2, feature, x_bu_feature, x_feature, x1_before, x2_before), as ``oracle.deeplab_ref.deeplab_forward``."""
    c = _Ctx(sd, training, masks, record, bn_training)
    h, low = xception_backbone(c, x, output_stride)
    # --- ASPP (aspp.py:65-78)
    dils = (1, 6, 12, 18) if output_stride == 16 else (1, 12, 24, 36)
    br = []
    for j, d in enumerate(dils, start=1):
        y = F.conv2d(h, sd["aspp.aspp%d.atrous_conv.weight" % j], None, 1, 0 if j == 1 else d, d)
        br.append(F.relu(c.bn(y, "aspp.aspp%d.bn" % j)))
    g = F.adaptive_avg_pool2d(h, 1)
    g = F.relu(c.bn(F.conv2d(g, sd["aspp.global_avg_pool.1.weight"]), "aspp.global_avg_pool.2"))
    g = F.interpolate(g, size=h.shape[2:], mode="bilinear", align_corners=True)
    y = F.relu(c.bn(F.conv2d(torch.cat(br + [g], 1), sd["aspp.conv1.weight"]), "aspp.bn1"))
    feature = c.dropout(y, "aspp.dropout", 0.5)
    # --- decoder (decoder.py:45-56)
    lo = F.relu(c.bn(F.conv2d(low, sd["decoder.conv1.weight"]), "decoder.bn1"))
    up = F.interpolate(feature, size=lo.shape[2:], mode="bilinear", align_corners=True)
    x_bu = torch.cat((up, lo), 1)
    b = F.relu(c.bn(F.conv2d(x_bu, sd["decoder.last_conv_boundary.0.weight"], None, 1, 1), "decoder.last_conv_boundary.1"))
    b = c.dropout(b, "decoder.last_conv_boundary.3", 0.5)
    b = F.relu(c.bn(F.conv2d(b, sd["decoder.last_conv_boundary.4.weight"], None, 1, 1), "decoder.last_conv_boundary.5"))
    b = c.dropout(b, "decoder.last_conv_boundary.7", 0.1)
    x2_before = F.conv2d(b, sd["decoder.last_conv_boundary.8.weight"], sd["decoder.last_conv_boundary.8.bias"])
    x_feature = torch.cat((x_bu, x2_before), 1)
    s = c.dropout(F.relu(c.bn(x_feature, "decoder.last_conv.0")), "decoder.last_conv.2", 0.1)
    x1_before = F.conv2d(s, sd["decoder.last_conv.3.weight"], sd["decoder.last_conv.3.bias"])
    # --- heads (deeplabv3.py:39-40)
    size = x.shape[2:]
    x2 = F.interpolate(x2_before, size=size, mode="bilinear", align_corners=True)
    x1 = F.interpolate(x1_before, size=size, mode="bilinear", align_corners=True)
    return x1, x2, feature, x_bu, x_feature, x1_before, x2_before


@contextlib.contextmanager
def as_deeplab_oracle():
    """Inside: ``oracle.deeplab_ref.deeplab_forward`` is this file's forward, so the whole-model helpers of
    ``model_cases`` (which call it by module attribute) drive the Xception model against its own oracle."""
    from oracle import deeplab_ref
    keep = deeplab_ref.deeplab_forward
    deeplab_ref.deeplab_forward = deeplab_forward
    try:
        yield
    finally:
        deeplab_ref.deeplab_forward = keep
