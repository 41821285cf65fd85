"""Functional CPU restatement of the reference generator with the DRN-D-54 backbone.

TEST INFRASTRUCTURE.  ``oracle.deeplab_ref.deeplab_forward`` tells its backbones apart by their keys and would take DRN for a
ResNet, so this file states the DRN network on its own: a flat ``state_dict`` (reference key names) evaluated with
``torch.nn.functional`` ops, in the dtype of the tensors it is given (fp32 = the reference's arithmetic, fp64 = the ground
truth of the GPU bounds).  BatchNorm / dropout bookkeeping, mask drawing and state canonicalisation are
``oracle.deeplab_ref``'s own (``_Ctx``, ``draw_masks``, ``canonical_state``).

Reference anchors
  networks/backbone/drn.py   :61-99 Bottleneck (its 3x3 conv uses dilation[1] only), :123-155 layer geometry of arch 'D',
                             :172-206 _make_layer / _make_conv_layers, :208-234 forward (low-level feature = layer3 output)
  networks/deeplabv3.py:14-15 (output stride forced to 8), networks/aspp.py:37-38,65-78 (512 input channels, rates of OS 8),
  networks/decoder.py:11-12,45-56, networks/deeplabv3.py:32-41
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle.deeplab_ref import _Ctx, canonical_state, draw_masks  # noqa: F401  (re-exported for the tests)
from uda_clr_amd.networks.backbone.drn import drn_plan


def _conv_layers(c, h, rows):
    for ck, bk, ci, co, k, s, d in rows:
        h = F.conv2d(h, c.sd["backbone." + ck + ".weight"], None, s, 3 if k == 7 else d, d)
        h = F.relu(c.bn(h, "backbone." + bk))
    return h


def _bottleneck(c, z, pre, stride, dil, has_ds):
    sd = c.sd
    h = F.relu(c.bn(F.conv2d(z, sd[pre + ".conv1.weight"]), pre + ".bn1"))
    h = F.relu(c.bn(F.conv2d(h, sd[pre + ".conv2.weight"], None, stride, dil, dil), pre + ".bn2"))
    h = c.bn(F.conv2d(h, sd[pre + ".conv3.weight"]), pre + ".bn3")
    if has_ds:
        z = c.bn(F.conv2d(z, sd[pre + ".downsample.0.weight"], None, stride), pre + ".downsample.1")
    return F.relu(h + z)


def drn_backbone(c, x):
    head, blocks, tail = drn_plan()
    h = _conv_layers(c, x, head)
    low = None
    for pre, inp, planes, stride, dil, has_ds in blocks:
        h = _bottleneck(c, h, "backbone." + pre, stride, dil, has_ds)
        if pre.startswith("layer3."):
            low = h
    return _conv_layers(c, h, tail), low


def deeplab_forward(sd, x, training=True, masks=None, record=None, output_stride=8, bn_training=None):
    """(x1, x2, feature, x_bu_feature, x_feature, x1_before, x2_before), as ``oracle.deeplab_ref.deeplab_forward``.
    ``output_stride`` is accepted for the callers' sake; DRN runs at 8 whatever it says (deeplabv3.py:14-15)."""
    c = _Ctx(sd, training, masks, record, bn_training)
    h, low = drn_backbone(c, x)
    # --- ASPP (aspp.py:65-78)
    br = []
    for j, d in enumerate((1, 12, 24, 36), start=1):
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
    ``model_cases`` (which call it by module attribute) drive the DRN model against its own oracle."""
    from oracle import deeplab_ref
    keep = deeplab_ref.deeplab_forward
    deeplab_ref.deeplab_forward = deeplab_forward
    try:
        yield
    finally:
        deeplab_ref.deeplab_forward = keep
