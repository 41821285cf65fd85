"""Aligned Xception backbone: geometry plan, parameter tree and its execution on the engine's kernels.

Key names, construction order and initialisation of the reference's ``networks/backbone/xception.py``:
``conv1, bn1, conv2, bn2``, ``block1 .. block20`` (each: ``skip`` / ``skipbn`` when the block changes width or
stride, then ``rep.<i>`` separable convs ``conv1`` (depthwise) / ``bn`` / ``pointwise`` and their outer BatchNorm
``rep.<i+1>``; the Sequential indices are those left after ``rep = rep[1:]`` for ``start_with_relu=False``,
:75-76), and the exit flow ``conv3 .. conv5`` / ``bn3 .. bn5``.  ``xception_plan`` is the geometry.
"""
import torch
import torch.nn as nn

from ...acts import ACT_NONE, ACT_RELU, Act
from .._tree import Holder, child, conv, normal_bn_init


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
        normal_bn_init(self.modules(), nn.BatchNorm2d)
        if pretrained:
            self._load_pretrained_model()

    def _load_pretrained_model(self):
        """No-op, as the reference's loader is in effect (xception.py:247-281): it downloads an ImageNet state dict and
        keeps only keys ``in model_dict``, which it has just created empty, so no weight is ever loaded and the seeded
        initialisation stands.  The download itself is left out."""
        return None


class XceptionExec:
    """The backbone's launch sequence on the kernels of one ``GeneratorEngine`` (``engine``: its helpers and kernel binding)."""
    c_high, c_low = 2048, 128

    def __init__(self, engine, output_stride):
        self.E = engine
        self.blocks, self.exit = xception_plan(output_stride), exit_plan(output_stride)
        n = 32 + 64                      # channels that receive BN statistics in one forward
        for name, inp, planes, stride, has_skip, seps in self.blocks:
            n += sum(ci + co for _, ci, co, _, _ in seps) + (planes if has_skip else 0)
        self.bn_channels = n + sum(ci + co for _, _, ci, co, _ in self.exit)

    def _sep_forward(self, ctx, v, pre, bn_key, cout, stride, dil, training, act):
        """SeparableConv2d + its outer BatchNorm (xception.py:26-31, 47-73) on the rectified input ``v``: depthwise 3x3 with
        a zero border (the reference pads AFTER the activation, ``fixed_padding`` = dil on every side), its own BN pending in
        the pointwise conv's prologue, the outer BN pending with ``act`` in the consumer's."""
        E = self.E
        K, N = E.K, ctx.N
        Ho, Wo = (v.H - 1) // stride + 1, (v.W - 1) // stride + 1
        Po, cin = N * Ho * Wo, v.C
        yd = E._buf(v.x, Po, cin)
        st = E._stats(ctx, cin, training)
        K.dwconv_fwd(v, E._w(ctx, pre + ".conv1.weight", "dw"), stride, dil, 0, yd, st)
        d = E._bn_act(ctx, pre + ".bn", yd, N, Ho, Wo, st, Po, training, ACT_NONE)
        yp = E._buf(v.x, Po, cout)
        st = E._stats(ctx, cout, training)
        K.conv(d, E._w(ctx, pre + ".pointwise.weight", "ohwi"), 1, 1, yp, stats=st)
        p = E._bn_act(ctx, bn_key, yp, N, Ho, Wo, st, Po, training, act)
        return dict(pre=pre, v=v, d=d, p=p, stride=stride, dil=dil)

    def forward(self, ctx, x, training):
        """xception.py:179-231.  Every block output is only ever read rectified (the shared in-place ReLU of ``rep[0]``
        rectifies the block input before the identity skip reads it, :44-49,80-90; blocks 1-2 get a rectified input, the
        output of block 20 is rectified before conv3), so each block materialises relu(bn(rep) + skip) once (bn_add_relu)
        and its successor reads that matrix for both its separable convs and its skip."""
        E = self.E
        K, S, params = E.K, ctx.S, ctx.params
        N, _, Hin, Win = x.shape
        H, W = (Hin - 1) // 2 + 1, (Win - 1) // 2 + 1
        y1 = E._buf(x, N * H * W, 32)
        st = E._stats(ctx, 32, training)
        K.stem_fwd(x, params["backbone.conv1.weight"], y1, st)
        a1 = E._bn_act(ctx, "backbone.bn1", y1, N, H, W, st, N * H * W, training, ACT_RELU)
        y2 = E._buf(x, N * H * W, 64)
        st = E._stats(ctx, 64, training)
        K.conv(a1, E._w(ctx, "backbone.conv2.weight", "ohwi"), 3, 1, y2, stats=st)
        a = E._bn_act(ctx, "backbone.bn2", y2, N, H, W, st, N * H * W, training, ACT_RELU)
        S["xstem"] = dict(a1=a1, a2=a)
        recs, low = [], None
        for name, inp, planes, stride, has_skip, seps in self.blocks:
            pre = "backbone." + name
            u = a                                   # the rectified block input (block1: bn2 + ReLU still pending)
            seprecs, v = [], u
            for j, (idx, ci, co, s, d) in enumerate(seps):
                last = j == len(seps) - 1
                r = self._sep_forward(ctx, v, "%s.rep.%d" % (pre, idx), "%s.rep.%d" % (pre, idx + 1), co, s, d, training,
                                      ACT_NONE if last else ACT_RELU)
                seprecs.append(r)
                v = r["p"]
            Ho, Wo = v.H, v.W
            Po = N * Ho * Wo
            us = ad = None
            if has_skip:
                us = u
                if stride != 1:
                    usb = E._buf(x, Po, inp)
                    K.rows_stride(u.x, N, u.H, u.W, stride, usb)
                    us = Act(usb, N, Ho, Wo, u.scale, u.shift, u.act, bn=u.bn)     # the pending transform is per channel
                yk = E._buf(x, Po, planes)
                st = E._stats(ctx, planes, training)
                K.conv(us, E._w(ctx, pre + ".skip.weight", "ohwi"), 1, 1, yk, stats=st)
                ad = E._bn_act(ctx, pre + ".skipbn", yk, N, Ho, Wo, st, Po, training, ACT_NONE)
            zo = E._buf(x, Po, planes)
            K.bn_add_relu(v, ad if has_skip else u, zo)
            a = Act(zo, N, Ho, Wo)
            recs.append(dict(pre=pre, stride=stride, u=u, us=us, ad=ad, seps=seprecs, zo=a))
            if name == "block1":
                low = a                             # low_level_feat = relu(block1 output) (xception.py:193-194)
        exits = []
        for sep, bn, ci, co, d in self.exit:
            r = self._sep_forward(ctx, a, "backbone." + sep, "backbone." + bn, co, 1, d, training, ACT_RELU)
            exits.append(r)
            a = r["p"]
        out = E._buf(x, a.P, a.C)                # the ASPP's pooling branch reads the activated matrix
        K.bn_apply(a, out, None)
        S["xblocks"], S["xexit"] = recs, exits
        return Act(out, N, a.H, a.W), low

    def _sep_backward(self, ctx, G, r, dP):
        """Reverse of ``_sep_forward``: dP is the gradient w.r.t. the activated outer-BN output.  Returns the gradient
        w.r.t. the rectified input ``v`` (a fresh [P, Cin] matrix)."""
        E = self.E
        x, N = ctx.x, ctx.N
        pre, v, d, p, stride, dil = r["pre"], r["v"], r["d"], r["p"], r["stride"], r["dil"]
        dyp = E._buf(x, p.P, p.C)
        E._bn_backward(ctx, G, p, dP, out=dyp)
        E._wgrad(ctx, G, pre + ".pointwise.weight", d, dyp, 1, 1)
        dUd = E._buf(x, d.P, d.C)
        E._dgrad(ctx, pre + ".pointwise.weight", dyp, N, d.H, d.W, 1, 1, dUd)
        del dyp
        dyd = E._bn_backward(ctx, G, d, dUd)
        return E._dw_backward(ctx, G, pre + ".conv1.weight", v, dyd, stride, dil, 0)

    def backward(self, ctx, G, d_a, d_low):
        """d_a: gradient w.r.t. the activated [P16, 2048] backbone output, d_low: w.r.t. relu(block1 output)."""
        E = self.E
        K, S, x = E.K, ctx.S, ctx.x
        N = ctx.N
        dP = d_a
        for r in reversed(S["xexit"]):
            dP = self._sep_backward(ctx, G, r, dP)
        d_z = dP                                    # gradient w.r.t. relu(block20 output)
        for r in reversed(S["xblocks"]):
            pre, stride, u, us, ad, zo = r["pre"], r["stride"], r["u"], r["us"], r["ad"], r["zo"]
            if pre.endswith(".block1"):
                d_z.add_(d_low)
            g = E._buf(x, zo.P, zo.C)            # gradient w.r.t. bn(rep) + skip
            K.relu_gate(d_z, zo.x, g)
            del d_z
            seps = r["seps"]
            dP = g
            for j in range(len(seps) - 1, -1, -1):
                # the last separable conv's outer BN reads g (not in place: the skip's BN backward needs it afterwards)
                dP = self._sep_backward(ctx, G, seps[j], dP)
            d_u = dP                                # gradient w.r.t. the rectified block input, from the separable convs
            if ad is not None:
                dyk = E._bn_backward(ctx, G, ad, g)
                E._wgrad(ctx, G, pre + ".skip.weight", us, dyk, 1, 1)
                if stride == 1:
                    E._dgrad(ctx, pre + ".skip.weight", dyk, N, u.H, u.W, 1, 1, d_u, addend=d_u)
                else:
                    d_us = E._buf(x, us.P, us.C)
                    E._dgrad(ctx, pre + ".skip.weight", dyk, N, us.H, us.W, 1, 1, d_us)
                    full = E._buf(x, u.P, u.C)
                    K.rows_stride(d_us, N, u.H, u.W, stride, full, scatter=True)
                    d_u.add_(full)
                    del d_us, full
                del dyk
            else:
                d_u.add_(g)
            del g
            d_z = d_u
        st = S["xstem"]
        a1, a2 = st["a1"], st["a2"]
        dy2 = E._bn_backward(ctx, G, a2, d_z)
        E._wgrad(ctx, G, "backbone.conv2.weight", a1, dy2, 3, 1)
        dU1 = E._buf(x, a1.P, a1.C)
        E._dgrad(ctx, "backbone.conv2.weight", dy2, N, a1.H, a1.W, 3, 1, dU1)
        del dy2
        dy1 = E._bn_backward(ctx, G, a1, dU1)
        dw1 = torch.empty_like(ctx.params["backbone.conv1.weight"])
        K.stem_wgrad(x, dy1, dw1)
        G["backbone.conv1.weight"] = dw1
