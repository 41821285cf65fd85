"""DRN-D-54 backbone - parameter tree only (compute: uda_clr_amd.engine).

Key names, construction order and initialisation of the reference's ``networks/backbone/drn.py:102-206``
(``DRN(Bottleneck, [1, 1, 3, 4, 6, 3, 1, 1], arch='D')``): ``layer0`` (7x7 stride 1, 3 -> 16), ``layer1`` / ``layer2``
(3x3 conv layers, the second at stride 2), ``layer3 .. layer6`` of Bottlenecks (layer3 / layer4 at stride 2,
layer5 / layer6 dilated by 2 / 4), ``layer7`` / ``layer8`` (3x3 conv layers, dilation 2 / 1).  The output sits at
1/8 of the input, the low-level feature is the ``layer3`` output at 1/4.  ``drn_plan`` is the geometry the engine
executes.
"""
import math
import os

import torch
import torch.nn as nn

from .._tree import Holder, child, conv

D54_LAYERS = (1, 1, 3, 4, 6, 3, 1, 1)
CHANNELS = (16, 32, 64, 128, 256, 512, 512, 512)


def drn_plan(layers=D54_LAYERS):
    """(head, blocks, tail) of an arch-'D' DRN with Bottleneck blocks (drn.py:123-155, 172-206):
      head / tail  [(conv key, bn key, cin, cout, ksize, stride, dilation)]   layer0 - layer2 / layer7 - layer8
      blocks       [(prefix, inplanes, planes, stride, dilation, has_downsample)]   layer3 - layer6
    A Bottleneck's 3x3 conv uses ``dilation[1]`` only, so ``new_level`` does not show (drn.py:69-71, 186-187)."""
    def conv_layers(name, inp, ch, n, stride, dil):
        rows = []
        for i in range(n):                     # Sequential of [conv, bn, relu] triples (drn.py:196-206)
            rows.append(("%s.%d" % (name, 3 * i), "%s.%d" % (name, 3 * i + 1), inp, ch, 3, stride if i == 0 else 1, dil))
            inp = ch
        return rows, inp

    head = [("layer0.0", "layer0.1", 3, CHANNELS[0], 7, 1, 1)]
    inp = CHANNELS[0]
    rows, inp = conv_layers("layer1", inp, CHANNELS[0], layers[0], 1, 1)
    head += rows
    rows, inp = conv_layers("layer2", inp, CHANNELS[1], layers[1], 2, 1)
    head += rows
    blocks = []
    for li, stride, dil in ((3, 2, 1), (4, 2, 1), (5, 1, 2), (6, 1, 4)):
        planes = CHANNELS[li - 1]
        for b in range(layers[li - 1]):
            st = stride if b == 0 else 1
            blocks.append(("layer%d.%d" % (li, b), inp, planes, st, dil, b == 0 and (st != 1 or inp != 4 * planes)))
            inp = 4 * planes
    tail, inp = conv_layers("layer7", inp, CHANNELS[6], layers[6], 1, 2)
    rows, inp = conv_layers("layer8", inp, CHANNELS[7], layers[7], 1, 1)
    return head, blocks, tail + rows


class DRN(Holder):
    def __init__(self, layers=D54_LAYERS, BatchNorm=None):
        super().__init__()
        BatchNorm = BatchNorm or nn.BatchNorm2d
        self.layers = tuple(layers)
        self.out_dim = CHANNELS[-1]
        head, blocks, tail = drn_plan(layers)

        def conv_rows(rows):
            for ck, bk, ci, co, k, s, d in rows:
                child(self, ck, conv(ci, co, k, s, 3 if k == 7 else d, d))
                child(self, bk, BatchNorm(co))
        conv_rows(head)
        for pre, inp, planes, stride, dil, has_ds in blocks:
            if has_ds:            # the reference builds the shortcut before the block's own convs (drn.py:175-181)
                ds0, ds1 = conv(inp, 4 * planes, 1, stride), BatchNorm(4 * planes)
            child(self, pre + ".conv1", conv(inp, planes, 1))
            child(self, pre + ".bn1", BatchNorm(planes))
            child(self, pre + ".conv2", conv(planes, planes, 3, stride, dil, dil))
            child(self, pre + ".bn2", BatchNorm(planes))
            child(self, pre + ".conv3", conv(planes, 4 * planes, 1))
            child(self, pre + ".bn3", BatchNorm(4 * planes))
            if has_ds:
                child(self, pre + ".downsample.0", ds0)
                child(self, pre + ".downsample.1", ds1)
        conv_rows(tail)
        for m in self.modules():                                   # drn.py:159-169
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, (nn.BatchNorm2d, BatchNorm)):
                m.weight.data.fill_(1)
                m.bias.data.zero_()


def drn_d_54(BatchNorm, pretrained=True):
    """drn.py:377-384.  The reference downloads the ImageNet DRN-D-54 state dict; nothing is fetched here.  Set
    ``UDA_CLR_DRN_D_54_PTH`` to a local copy of that state dict to load it the reference's way (``fc.weight`` /
    ``fc.bias`` dropped, then a strict load); unset means the seeded initialisation stands."""
    model = DRN(D54_LAYERS, BatchNorm)
    path = os.environ.get("UDA_CLR_DRN_D_54_PTH") if pretrained else None
    if path:
        pre = dict(torch.load(path, map_location="cpu", weights_only=True))
        pre.pop("fc.weight", None)
        pre.pop("fc.bias", None)
        model.load_state_dict(pre)
    return model
