"""Functional CPU restatement of the reference's DRN-D-54 backbone.

TEST INFRASTRUCTURE.  ``oracle.deeplab_ref.deeplab_forward`` tells its own backbones apart by their keys and would take DRN for a
ResNet, so this file states the DRN backbone - a flat ``state_dict`` (reference key names) evaluated with
``torch.nn.functional`` ops, in the dtype of the tensors it is given (fp32 = the reference's arithmetic, fp64 = the ground
truth of the GPU bounds) - and binds ``deeplab_forward`` over it at output stride 8.  ASPP, decoder, heads and the BatchNorm /
dropout bookkeeping are ``oracle.deeplab_ref``'s own.

Reference anchors
  networks/backbone/drn.py   :61-99 Bottleneck (its 3x3 conv uses dilation[1] only), :123-155 layer geometry of arch 'D',
                             :172-206 _make_layer / _make_conv_layers, :208-234 forward (low-level feature = layer3 output)
  networks/deeplabv3.py:14-15 (output stride forced to 8), networks/aspp.py:37-38 (512 input channels, rates of OS 8)
"""
from __future__ import annotations

import torch.nn.functional as F

from oracle.deeplab_ref import deeplab_forward as _shared_forward
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


def drn_backbone(c, x, output_stride=8):
    head, blocks, tail = drn_plan()
    h = _conv_layers(c, x, head)
    low = None
    for pre, inp, planes, stride, dil, has_ds in blocks:
        h = _bottleneck(c, h, "backbone." + pre, stride, dil, has_ds)
        if pre.startswith("layer3."):
            low = h
    return _conv_layers(c, h, tail), low


def deeplab_forward(sd, x, training=True, masks=None, record=None, output_stride=8, bn_training=None):
    """``oracle.deeplab_ref.deeplab_forward`` (ASPP, decoder and heads) over the DRN backbone.  ``output_stride`` is accepted for
    the callers' sake; DRN runs at 8 whatever it says (deeplabv3.py:14-15)."""
    return _shared_forward(sd, x, training, masks, record, 8, bn_training, backbone=drn_backbone)
