"""Aligned Xception backbone - parameter tree only (compute: uda_clr_amd.engine).

Key names, construction order and initialisation of the reference's ``networks/backbone/xception.py``:
``conv1, bn1, conv2, bn2``, ``block1 .. block20`` (each: ``skip`` / ``skipbn`` when the block changes width or
stride, then ``rep.<i>`` separable convs ``conv1`` (depthwise) / ``bn`` / ``pointwise`` and their outer BatchNorm
``rep.<i+1>``; the Sequential indices are those left after ``rep = rep[1:]`` for ``start_with_relu=False``,
:75-76), and the exit flow ``conv3 .. conv5`` / ``bn3 .. bn5``.  ``xception_plan`` is the geometry the engine
executes.
"""
import math

import torch.nn as nn

from .._tree import Holder, child, conv


def _sep(root, prefix, cin, cout, stride, dil, BatchNorm):
    """SeparableConv2d (xception.py:17-31): depthwise 3x3, its own BN, pointwise 1x1 - constructed in that order."""
    child(root, prefix + ".conv1", conv(cin, cin, 3, stride, 0, dil, cin))
    child(root, prefix + ".bn", BatchNorm(cin))
    child(root, prefix + ".pointwise", conv(cin, cout, 1))


def _block_seps(inplanes, planes, reps, stride, dil, start_with_relu, grow_first, is_last):
    """[(rep index, cin, cout, stride, dilation)] of one Block (xception.py:34-76)."""
    units = []
    filters = inplanes
    if grow_first:
        units.append((inplanes, planes, 1, dil))
        filters = planes
    for _ in range(reps - 1):
        units.append((filters, filters, 1, dil))
    if not grow_first:
        units.append((inplanes, planes, 1, dil))
    if stride != 1:
        units.append((planes, planes, 2, 1))
    if stride == 1 and is_last:
        units.append((planes, planes, 1, 1))
    off = 1 if start_with_relu else 0          # [relu, sep, bn] per unit; rep[1:] drops the leading relu
    return [(3 * k + off, ci, co, s, d) for k, (ci, co, s, d) in enumerate(units)]


def xception_plan(output_stride=16):
    """Per block: (name, inplanes, planes, stride, has_skip, seps) with seps as in ``_block_seps``
    (xception.py:101-176); the exit flow's three separable convs follow as ``exit_plan``."""
    if output_stride == 16:
        e3, mid, ex = 2, 1, (1, 2)
    elif output_stride == 8:
        e3, mid, ex = 1, 2, (2, 4)
    else:
        raise NotImplementedError
    rows = [("block1", 64, 128, 2, 2, 1, False, True, False),
            ("block2", 128, 256, 2, 2, 1, False, True, False),
            ("block3", 256, 728, 2, e3, 1, True, True, True)]
    rows += [("block%d" % i, 728, 728, 3, 1, mid, True, True, False) for i in range(4, 20)]
    rows.append(("block20", 728, 1024, 2, 1, ex[0], True, False, True))
    plan = []
    for name, inp, planes, reps, stride, dil, swr, grow, last in rows:
        plan.append((name, inp, planes, stride, planes != inp or stride != 1,
                     _block_seps(inp, planes, reps, stride, dil, swr, grow, last)))
    return plan


def exit_plan(output_stride=16):
    """[(sep prefix, bn prefix, cin, cout, dilation)] of conv3 .. conv5 (xception.py:170-177)."""
    d = 2 if output_stride == 16 else 4
    return [("conv3", "bn3", 1024, 1536, d), ("conv4", "bn4", 1536, 1536, d), ("conv5", "bn5", 1536, 2048, d)]


class AlignedXception(Holder):
    def __init__(self, output_stride, BatchNorm, pretrained=True):
        super().__init__()
        BatchNorm = BatchNorm or nn.BatchNorm2d
        self.output_stride = output_stride
        plan = xception_plan(output_stride)
        child(self, "conv1", conv(3, 32, 3, 2, 1))
        child(self, "bn1", BatchNorm(32))
        child(self, "conv2", conv(32, 64, 3, 1, 1))
        child(self, "bn2", BatchNorm(64))
        for name, inp, planes, stride, has_skip, seps in plan:
            if has_skip:                     # the reference builds the shortcut before ``rep`` (xception.py:38-42)
                child(self, name + ".skip", conv(inp, planes, 1, stride))
                child(self, name + ".skipbn", BatchNorm(planes))
            for idx, ci, co, s, d in seps:
                _sep(self, "%s.rep.%d" % (name, idx), ci, co, s, d, BatchNorm)
                child(self, "%s.rep.%d" % (name, idx + 1), BatchNorm(co))
        for sep, bn, ci, co, d in exit_plan(output_stride):
            _sep(self, sep, ci, co, 1, d, BatchNorm)
            child(self, bn, BatchNorm(co))
        for m in self.modules():                                   # xception.py:234-245
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()
        if pretrained:
            self._load_pretrained_model()

    def _load_pretrained_model(self):
        """No-op, as the reference's loader is in effect (xception.py:247-281): it downloads an ImageNet state dict and
        keeps only keys ``in model_dict``, which it has just created empty, so no weight is ever loaded and the seeded
        initialisation stands.  The download itself is left out."""
        return None
