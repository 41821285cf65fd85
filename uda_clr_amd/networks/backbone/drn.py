"""DRN-D-54 backbone: geometry plan, parameter tree and its execution on the engine's kernels.

Key names, construction order and initialisation of the reference's ``networks/backbone/drn.py:102-206``
(``DRN(Bottleneck, [1, 1, 3, 4, 6, 3, 1, 1], arch='D')``): ``layer0`` (7x7 stride 1, 3 -> 16), ``layer1`` / ``layer2``
(3x3 conv layers, the second at stride 2), ``layer3 .. layer6`` of Bottlenecks (layer3 / layer4 at stride 2,
layer5 / layer6 dilated by 2 / 4), ``layer7`` / ``layer8`` (3x3 conv layers, dilation 2 / 1).  The output sits at
1/8 of the input, the low-level feature is the ``layer3`` output at 1/4.  ``drn_plan`` is the geometry.
"""
import os

import torch
import torch.nn as nn

from ...acts import ACT_RELU, Act
from .._tree import Holder, child, conv, normal_bn_init
from ._bottleneck import bottleneck_bn_channels, bottleneck_tree, bottlenecks_backward, bottlenecks_forward, conv3x3, conv3x3_backward

# Which passes of DRN's narrow 3x3 convolutions (16 / 32 / 64 channels: layer1, layer2 and layer3's conv2, drn.py:131-136) run on
# the direct kernels (uda_conv3n_*) instead of the implicit-GEMM route: (pass, Cin, Cout, stride of the LAYER) -> bool, as measured
# in profiles/drn_head_kernels.md.  "dgrad" runs as the stride-1 conv Cout -> Cin of the (zero-stuffed) gradient.  The two entries
# read different weight layouts, so the engine asks here before it asks for the layout.
_DRN_NARROW = {("fwd", 16, 16, 1): True, ("fwd", 16, 32, 2): True, ("fwd", 64, 64, 2): True, ("fwd", 64, 64, 1): False,
               ("wgrad", 16, 16, 1): True, ("wgrad", 16, 32, 2): True, ("wgrad", 64, 64, 2): True, ("wgrad", 64, 64, 1): True,
               ("dgrad", 16, 16, 1): True, ("dgrad", 16, 32, 2): True, ("dgrad", 64, 64, 2): True, ("dgrad", 64, 64, 1): False}


def _narrow(what, cin, cout, stride, dil=1):
    """True when this pass of a 3x3 convolution layer (cin -> cout at ``stride``) runs on the narrow direct kernels."""
    return dil == 1 and _DRN_NARROW.get((what, cin, cout, stride), False)


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
        bottleneck_tree(self, blocks, BatchNorm)
        conv_rows(tail)
        normal_bn_init(self.modules(), (nn.BatchNorm2d, BatchNorm))


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


class DRNExec:
    """The backbone's launch sequence on the kernels of one ``GeneratorEngine`` (``engine``: its helpers and kernel binding)."""
    c_high, c_low = CHANNELS[-1], 4 * CHANNELS[2]

    def __init__(self, engine, output_stride):
        if output_stride != 8:
            raise ValueError("the DRN backbone's output sits at 1/8 of the input (deeplabv3.py:14-15): output_stride must be 8")
        self.E = engine
        self.head, blocks, self.tail = drn_plan()
        self.blocks = [("backbone." + pre,) + tuple(rest) for pre, *rest in blocks]
        self.low_after = [pre for pre, *_ in self.blocks if pre.startswith("backbone.layer3.")][-1]
        # channels that receive BN statistics in one forward
        self.bn_channels = sum(row[3] for row in self.head + self.tail) + bottleneck_bn_channels(self.blocks)

    def forward(self, ctx, x, training):
        """drn.py:208-234.  layer0 - layer2 (the head: 7x7 stem and two narrow 3x3 convs at full / half resolution) and
        layer7 - layer8 are conv + BN + ReLU with the BN pending in the consumer; layer3 - layer6 are the Bottleneck sequence
        shared with ResNet-101.  The low-level feature is the layer3 output."""
        E = self.E
        K, S = E.K, ctx.S
        N, _, H, W = x.shape
        a, head = None, []
        for ck, bk, ci, co, k, s, d in self.head:
            key = "backbone." + ck + ".weight"
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            y = E._buf(x, N * Ho * Wo, co)
            st = E._stats(ctx, co, training)
            if k == 7:
                K.stem7s1_fwd(x, E._w(ctx, key, "hwio"), y, st)
            else:
                conv3x3(E, ctx, a, key, d, s, y, st, _narrow)
            src, H, W = a, Ho, Wo
            a = E._bn_act(ctx, "backbone." + bk, y, N, H, W, st, N * H * W, training, ACT_RELU)
            head.append(dict(key=key, src=src, a=a, stride=s, dil=d))
        a, low = bottlenecks_forward(E, ctx, x, a, training, self.blocks, self.low_after, _narrow)
        tail = []
        for ck, bk, ci, co, k, s, d in self.tail:
            key = "backbone." + ck + ".weight"
            y = E._buf(x, a.P, co)
            st = E._stats(ctx, co, training)
            conv3x3(E, ctx, a, key, d, 1, y, st, _narrow)
            src = a
            a = E._bn_act(ctx, "backbone." + bk, y, N, a.H, a.W, st, a.P, training, ACT_RELU)
            tail.append(dict(key=key, src=src, a=a, stride=1, dil=d))
        out = E._buf(x, a.P, a.C)                # the ASPP's pooling branch reads the activated matrix
        K.bn_apply(a, out, None)
        S["dhead"], S["dtail"] = head, tail
        return Act(out, N, a.H, a.W), low

    def backward(self, ctx, G, d_a, d_low):
        """d_a: gradient w.r.t. the activated [P8, 512] backbone output, d_low: w.r.t. the layer3 output."""
        E = self.E
        K, S, x = E.K, ctx.S, ctx.x
        d_z = d_a
        for r in reversed(S["dtail"]):
            dy = E._bn_backward(ctx, G, r["a"], d_z)
            d_z = conv3x3_backward(E, ctx, G, r["key"], r["src"], dy, r["dil"], 1, E._buf(x, r["src"].P, r["src"].C), _narrow)
            del dy
        d_z = bottlenecks_backward(E, ctx, G, d_z, d_low, self.low_after, _narrow)
        for r in reversed(S["dhead"]):
            dy = E._bn_backward(ctx, G, r["a"], d_z)
            src = r["src"]
            if src is None:                          # layer0 reads the image, which needs no gradient
                dw = torch.empty_like(ctx.params[r["key"]])
                K.stem7s1_wgrad(x, dy, dw)
                G[r["key"]] = dw
            else:
                d_z = conv3x3_backward(E, ctx, G, r["key"], src, dy, r["dil"], r["stride"], E._buf(x, src.P, src.C), _narrow)
            del dy
