"""MobileNetV2 backbone: geometry plan, parameter tree and its execution on the engine's kernels.

Mirrors the construction order and key names of the reference's
``networks/backbone/mobilenet.py:70-122`` (stem ``features.0``, 17 inverted-residual blocks
``features.1 .. features.17`` with members ``conv.<idx>``, aliases ``low_level_features`` =
``features[0:4]`` and ``high_level_features`` = ``features[4:]``).
"""
import torch
import torch.nn as nn

from ...acts import ACT_NONE, ACT_RELU6, Act
from .._tree import Holder, child, conv, kaiming_bn_init, load_known_keys

# (t, c, n, s) rows of the MobileNetV2 table (mobilenet.py:77-86)
_MBV2 = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1),
         (6, 160, 3, 2), (6, 320, 1, 1))


def block_plan(output_stride: int = 16):
    """[(inp, oup, stride, dilation, expand)] per inverted-residual block (mobilenet.py:88-111)."""
    plan, inp, cur, rate = [], 32, 2, 1
    for t, c, n, s in _MBV2:
        if cur == output_stride:
            stride, dil = 1, rate
            rate *= s
        else:
            stride, dil = s, 1
            cur *= s
        for i in range(n):
            plan.append((inp, c, stride if i == 0 else 1, dil, t))
            inp = c
    return plan


class MobileNetV2(Holder):
    def __init__(self, output_stride=8, BatchNorm=None, width_mult=1., pretrained=True):
        super().__init__()
        if width_mult != 1.:
            raise NotImplementedError("only width_mult=1 is built")
        BatchNorm = BatchNorm or nn.BatchNorm2d
        self.output_stride = output_stride
        feats = Holder()
        self.add_module("features", feats)
        child(feats, "0.0", conv(3, 32, 3, 2, 1))
        child(feats, "0.1", BatchNorm(32))
        for i, (inp, oup, stride, dil, t) in enumerate(block_plan(output_stride), start=1):
            hid, idx = round(inp * t), 0
            if t != 1:
                child(feats, "%d.conv.0" % i, conv(inp, hid, 1))
                child(feats, "%d.conv.1" % i, BatchNorm(hid))
                idx = 3
            child(feats, "%d.conv.%d" % (i, idx), conv(hid, hid, 3, stride, 0, dil, hid))
            child(feats, "%d.conv.%d" % (i, idx + 1), BatchNorm(hid))
            child(feats, "%d.conv.%d" % (i, idx + 3), conv(hid, oup, 1))
            child(feats, "%d.conv.%d" % (i, idx + 4), BatchNorm(oup))
        kaiming_bn_init(self.modules(), (nn.BatchNorm2d, BatchNorm))
        if pretrained:
            self._load_pretrained_model()
        lo, hi = Holder(), Holder()
        for k in range(len(feats)):
            (lo if k < 4 else hi).add_module(str(k), feats[k])   # Sequential slices keep their keys
        self.add_module("low_level_features", lo)
        self.add_module("high_level_features", hi)

    def _load_pretrained_model(self):
        """The reference reads a hard-coded absolute path (mobilenet.py:124-133).  Set
        ``UDA_CLR_MOBILENET_PTH`` to a MobileNetV2 state dict to load it the same key-filtered way;
        unset means seeded random initialisation."""
        load_known_keys(self, "UDA_CLR_MOBILENET_PTH")


class MobileNetV2Exec:
    """The backbone's launch sequence on the kernels of one ``GeneratorEngine`` (``engine``: its helpers and kernel binding)."""
    c_high, c_low = 320, 24

    def __init__(self, engine, output_stride):
        self.E = engine
        self.blocks = block_plan(output_stride)
        # channels that receive BN statistics in one forward
        self.bn_channels = 32 + sum((inp * t if t != 1 else 0) + inp * t + oup for inp, oup, stride, dil, t in self.blocks)

    def forward(self, ctx, x, training):
        E = self.E
        K, S, params = E.K, ctx.S, ctx.params
        N, _, Hin, Win = x.shape
        # ---- stem (mobilenet.py:8-13)
        H, W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
        y0 = E._buf(x, N * H * W, 32)
        st = E._stats(ctx, 32, training)
        K.stem_fwd(x, params["backbone.features.0.0.weight"], y0, st)
        a = E._bn_act(ctx, "backbone.features.0.1", y0, N, H, W, st, N * H * W, training, ACT_RELU6)
        S["stem"] = a
        # ---- inverted residual blocks (mobilenet.py:25-67)
        recs = []
        low = None
        for i, (inp, oup, stride, dil, t) in enumerate(self.blocks, start=1):
            pre = "backbone.features.%d" % i
            zin, H, W = a, a.H, a.W
            hid = inp * t
            if t != 1:
                ye = E._buf(x, N * H * W, hid)
                st = E._stats(ctx, hid, training)
                K.conv(zin, E._w(ctx, pre + ".conv.0.weight", "ohwi"), 1, 1, ye, stats=st)
                cnt = N * (H + 2 * dil) * (W + 2 * dil)          # quirk Q1
                e = E._bn_act(ctx, pre + ".conv.1", ye, N, H, W, st, cnt, training, ACT_RELU6, q1=True)
                border, kd, kdb, kp, kpb = 1, ".conv.3", ".conv.4", ".conv.6", ".conv.7"
            else:
                e, border, kd, kdb, kp, kpb = zin, 0, ".conv.0", ".conv.1", ".conv.3", ".conv.4"
            Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
            Po = N * Ho * Wo
            yd = E._buf(x, Po, hid)
            st = E._stats(ctx, hid, training)
            K.dwconv_fwd(e, E._w(ctx, pre + kd + ".weight", "dw"), stride, dil, border, yd, st)
            d = E._bn_act(ctx, pre + kdb, yd, N, Ho, Wo, st, Po, training, ACT_RELU6)
            yp = E._buf(x, Po, oup)
            st = E._stats(ctx, oup, training)
            K.conv(d, E._w(ctx, pre + kp + ".weight", "ohwi"), 1, 1, yp, stats=st)
            pb = E._bn_act(ctx, pre + kpb, yp, N, Ho, Wo, st, Po, training, ACT_NONE)
            use_res = stride == 1 and inp == oup
            z = E._buf(x, Po, oup)
            K.bn_apply(pb, z, zin.x if use_res else None)
            a = Act(z, N, Ho, Wo)
            recs.append(dict(pre=pre, t=t, stride=stride, dil=dil, zin=zin, e=e, d=d, pb=pb,
                             use_res=use_res, border=border, keys=(kd, kdb, kp, kpb)))
            if i == 3:
                low = a
        S["blocks"] = recs
        return a, low

    def backward(self, ctx, G, d_a, d_low):
        E = self.E
        K, S, x = E.K, ctx.S, ctx.x
        N = ctx.N
        # ---- backbone, last block first (mobilenet.py:61-67)
        d_z = d_a
        dU_stem = None
        for i in range(len(S["blocks"]), 0, -1):
            r = S["blocks"][i - 1]
            pre, t, stride, dil = r["pre"], r["t"], r["stride"], r["dil"]
            kd, kdb, kp, kpb = r["keys"]
            zin, e, d, pb = r["zin"], r["e"], r["d"], r["pb"]
            No, Ho, Wo = d.N, d.H, d.W
            Hi, Wi = zin.H, zin.W
            dyp = E._buf(x, d.P, pb.C)
            E._bn_backward(ctx, G, pb, d_z, out=dyp)
            E._wgrad(ctx, G, pre + kp + ".weight", d, dyp, 1, 1)
            dUd = E._buf(x, d.P, d.C)
            E._dgrad(ctx, pre + kp + ".weight", dyp, No, Ho, Wo, 1, 1, dUd)
            dyd = E._bn_backward(ctx, G, d, dUd)
            dUe = E._dw_backward(ctx, G, pre + kd + ".weight", e, dyd, stride, dil, r["border"])
            del dUd, dyd, dyp
            if t != 1:
                q1_total = None
                if e.bn.frozen:
                    # quirk Q1 with a frozen depthwise BN behind: the gradient summed over ALL padded positions of the block input
                    # is colsum(dy_dw) * sum of the depthwise taps = scale_dw * dbeta_dw * sum_t w (engine docstring)
                    dbeta = G[pre + kdb + ".bias"]
                    if d.bn.gain is not None:          # frozen TransNorm: dbeta carries the gain, colsum(dy_dw) = scale * sum(g) does not need it twice
                        dbeta = dbeta / d.bn.gain
                    q1_total = (d.scale * dbeta * ctx.params[pre + kd + ".weight"].sum((1, 2, 3))).contiguous()
                dye = E._bn_backward(ctx, G, e, dUe, q1_total=q1_total)
                E._wgrad(ctx, G, pre + ".conv.0.weight", zin, dye, 1, 1)
                d_zin = E._buf(x, zin.P, zin.C)
                addend = d_z if r["use_res"] else (d_low if i == 4 else None)
                E._dgrad(ctx, pre + ".conv.0.weight", dye, N, Hi, Wi, 1, 1, d_zin, addend=addend)
                d_z = d_zin
                del dUe, dye
            else:
                dU_stem = dUe
        # ---- stem (mobilenet.py:8-13); the image itself needs no gradient
        dy0 = E._bn_backward(ctx, G, S["stem"], dU_stem)
        dw0 = torch.empty_like(ctx.params["backbone.features.0.0.weight"])
        K.stem_wgrad(x, dy0, dw0)
        G["backbone.features.0.0.weight"] = dw0
