"""ResNet-101 backbone: geometry plan, parameter tree and its execution on the engine's kernels.

Key names and construction order of the reference's ``networks/backbone/resnet.py:45-111``
(``conv1, bn1, layer1..layer3`` of Bottlenecks [3, 4, 23], ``layer4`` = multi-grid unit [1, 2, 4]);
``resnet_plan`` is the per-block geometry.
"""
import torch
import torch.nn as nn

from ...acts import ACT_RELU, Act
from .._tree import Holder, child, conv, load_known_keys, normal_bn_init
from ._bottleneck import bottleneck_bn_channels, bottleneck_tree, bottlenecks_backward, bottlenecks_forward


def resnet_plan(output_stride=16, layers=(3, 4, 23)):
    """[(prefix, inplanes, planes, stride, dilation, has_downsample)] (resnet.py:47-70, 72-111)."""
    if output_stride == 16:
        strides, dils = (1, 2, 2, 1), (1, 1, 1, 2)
    elif output_stride == 8:
        strides, dils = (1, 2, 1, 1), (1, 1, 2, 4)
    else:
        raise NotImplementedError
    plan, inp = [], 64
    for li, (planes, n) in enumerate(zip((64, 128, 256), layers), start=1):
        for b in range(n):
            s = strides[li - 1] if b == 0 else 1
            plan.append(("layer%d.%d" % (li, b), inp, planes, s, dils[li - 1], b == 0 and (s != 1 or inp != 4 * planes)))
            inp = 4 * planes
    for b, mg in enumerate((1, 2, 4)):
        s = strides[3] if b == 0 else 1
        plan.append(("layer4.%d" % b, inp, 512, s, mg * dils[3], b == 0 and (s != 1 or inp != 2048)))
        inp = 2048
    return plan


class ResNet(Holder):
    def __init__(self, output_stride, BatchNorm, pretrained=True):
        super().__init__()
        BatchNorm = BatchNorm or nn.BatchNorm2d
        self.output_stride = output_stride
        child(self, "conv1", conv(3, 64, 7, 2, 3))
        child(self, "bn1", BatchNorm(64))
        bottleneck_tree(self, resnet_plan(output_stride), BatchNorm)
        normal_bn_init(self.modules(), (nn.BatchNorm2d, BatchNorm))
        if pretrained:
            self._load_pretrained_model()

    def _load_pretrained_model(self):
        """The reference downloads torchvision's ImageNet ResNet-101 (resnet.py:138-146); there is no
        network here.  Set ``UDA_CLR_RESNET101_PTH`` to that state dict to load it the same
        key-filtered way; unset means seeded random initialisation."""
        load_known_keys(self, "UDA_CLR_RESNET101_PTH")


def ResNet101(output_stride, BatchNorm, pretrained=True):
    return ResNet(output_stride, BatchNorm, pretrained=pretrained)


class ResNetExec:
    """The backbone's launch sequence on the kernels of one ``GeneratorEngine`` (``engine``: its helpers and kernel binding)."""
    c_high, c_low = 2048, 256
    LOW_AFTER = "backbone.layer1.2"

    def __init__(self, engine, output_stride):
        self.E = engine
        self.blocks = [("backbone." + pre,) + tuple(rest) for pre, *rest in resnet_plan(output_stride)]
        self.bn_channels = 64 + bottleneck_bn_channels(self.blocks)      # channels that receive BN statistics in one forward

    def forward(self, ctx, x, training):
        """resnet.py:113-124.  The 3x3 convs of the two stride-2 bottlenecks (layer2.0, layer3.0) and their weight gradients walk
        the strided output grid in the wide-tile kernels' loaders; only their input gradient is a stride-1 conv of the
        zero-stuffed gradient."""
        E = self.E
        K, S, params = E.K, ctx.S, ctx.params
        N, _, Hin, Win = x.shape
        H, W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
        y0 = E._buf(x, N * H * W, 64)
        st = E._stats(ctx, 64, training)
        K.stem7_fwd(x, params["backbone.conv1.weight"], y0, st)
        a0 = E._bn_act(ctx, "backbone.bn1", y0, N, H, W, st, N * H * W, training, ACT_RELU)
        Hp, Wp = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        z = E._buf(x, N * Hp * Wp, 64)
        idx = torch.empty((N * Hp * Wp, 64), dtype=torch.uint8, device=x.device)
        K.maxpool_fwd(a0, z, idx)
        S["stem"] = dict(a0=a0, idx=idx)
        a = Act(z, N, Hp, Wp)
        return bottlenecks_forward(E, ctx, x, a, training, self.blocks, self.LOW_AFTER)

    def backward(self, ctx, G, d_z, d_low):
        """d_z: gradient w.r.t. the [P16, 2048] backbone output, d_low: w.r.t. the layer1 output."""
        E = self.E
        K, S, x = E.K, ctx.S, ctx.x
        N = ctx.N
        d_z = bottlenecks_backward(E, ctx, G, d_z, d_low, self.LOW_AFTER)
        st = S["stem"]
        a0 = st["a0"]
        dU0 = E._buf(x, a0.P, 64)
        K.maxpool_bwd(d_z, st["idx"], N, a0.H, a0.W, dU0)
        dy0 = E._bn_backward(ctx, G, a0, dU0)
        dw0 = torch.empty_like(ctx.params["backbone.conv1.weight"])
        K.stem7_wgrad(x, dy0, dw0)
        G["backbone.conv1.weight"] = dw0
