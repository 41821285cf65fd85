"""Functional CPU restatement of the reference's Aligned Xception backbone.

TEST INFRASTRUCTURE.  ``oracle.deeplab_ref.deeplab_forward`` tells its own two backbones apart by their keys and would take
Xception for a ResNet, so this file states the Xception backbone - a flat ``state_dict`` (reference key names) evaluated with
``torch.nn.functional`` ops, in the dtype of the tensors it is given (fp32 = the reference's arithmetic, fp64 = the ground
truth of the GPU bounds) - and binds ``deeplab_forward`` over it.  ASPP, decoder, heads and the BatchNorm / dropout
bookkeeping are ``oracle.deeplab_ref``'s own.

Reference anchors
  networks/backbone/xception.py   :8-14 fixed_padding, :17-31 SeparableConv2d, :34-90 Block (rep[0] is the shared
                                  in-place ReLU, so ``skip`` reads the RECTIFIED input), :93-177 flow geometry,
                                  :179-231 forward
"""
from __future__ import annotations

import torch.nn.functional as F

from oracle.deeplab_ref import deeplab_forward as _shared_forward
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
    """``oracle.deeplab_ref.deeplab_forward`` (ASPP, decoder and heads) over the Xception backbone."""
    return _shared_forward(sd, x, training, masks, record, output_stride, bn_training, backbone=xception_backbone)
