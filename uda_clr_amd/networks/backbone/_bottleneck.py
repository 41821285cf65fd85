"""The Bottleneck sequence (ResNet-101 layer1-4, DRN-D-54 layer3-6) and the 3x3 convolution at stride 1 | 2 of any width,
executed on the engine's kernels.  ``E`` is the ``GeneratorEngine`` whose helpers and kernel binding run the launches;
``narrow`` is the backbone's predicate (pass, cin, cout, stride, dil) -> bool for the narrow direct kernels (DRN's head; None:
never)."""
import torch

from ...acts import ACT_NONE, ACT_RELU, Act
from .._tree import child, conv


def bottleneck_tree(root, blocks, BatchNorm):
    """The parameter holders of the Bottlenecks ``blocks`` (resnet.py:9-21,47-70 = drn.py:61-77,172-194) under ``root``."""
    for pre, inp, planes, stride, dil, has_ds in blocks:
        if has_ds:            # the reference builds the shortcut before the block's own convs
            ds0, ds1 = conv(inp, 4 * planes, 1, stride), BatchNorm(4 * planes)
        child(root, pre + ".conv1", conv(inp, planes, 1))
        child(root, pre + ".bn1", BatchNorm(planes))
        child(root, pre + ".conv2", conv(planes, planes, 3, stride, dil, dil))
        child(root, pre + ".bn2", BatchNorm(planes))
        child(root, pre + ".conv3", conv(planes, 4 * planes, 1))
        child(root, pre + ".bn3", BatchNorm(4 * planes))
        if has_ds:
            child(root, pre + ".downsample.0", ds0)
            child(root, pre + ".downsample.1", ds1)


def bottleneck_bn_channels(blocks):
    """Channels that receive BN statistics in one forward over ``blocks`` (rows of ``resnet_plan`` / ``drn_plan``)."""
    return sum(2 * planes + 4 * planes * (2 if has_ds else 1) for pre, inp, planes, stride, dil, has_ds in blocks)


def conv3x3(E, ctx, src, key, dil, stride, out, st, narrow=None):
    """3x3 conv (pad = dil) of ``src`` at stride 1 | 2 into ``out`` with the statistics epilogue: on the narrow direct kernel where
    the backbone's table says so, else on the launch the library plans (it refuses a stride-2 conv below its wide tiles)."""
    if narrow is not None and narrow("fwd", src.C, out.shape[1], stride, dil):
        E.K.conv3n_fwd(src, E._w(ctx, key, "hwio"), stride, out, stats=st)
    else:
        E.K.conv(src, E._w(ctx, key, "ohwi"), 3, dil, out, stats=st, stride=stride)


def conv3x3_backward(E, ctx, G, key, src, dy, dil, stride, out, narrow=None):
    """Weight gradient of ``conv3x3`` into G and its input gradient (w.r.t. the activated ``src``) into ``out``; the input
    gradient of a stride-2 conv is a stride-1 conv of the zero-stuffed gradient."""
    K, N, H, W = E.K, src.N, src.H, src.W
    cin, cout = src.C, dy.shape[1]
    if narrow is not None and narrow("wgrad", cin, cout, stride, dil):
        dw = torch.empty_like(ctx.params[key])
        K.conv3n_wgrad(src, dy, stride, dw)
        G[key] = dw
    else:
        E._wgrad(ctx, G, key, src, dy, 3, dil, stride)
    if stride != 1:
        full = E._buf(src.x, src.P, cout)
        K.rows_stride(dy, N, H, W, stride, full, scatter=True)
        dy = full
    if narrow is not None and narrow("dgrad", cin, cout, stride, dil):
        K.conv3n_fwd(Act(dy, N, H, W), E._w(ctx, key, "hwio_dgrad"), 1, out)
    else:
        E._dgrad(ctx, key, dy, N, H, W, 3, dil, out)
    return out


def bottlenecks_forward(E, ctx, x, a, training, blocks, low_after, narrow=None):
    """resnet.py:23-43 = drn.py:79-99 over ``blocks``; ``a`` may carry a pending transform (DRN: layer2's BN + ReLU).
    Returns the last block's output and the output of block ``low_after``."""
    K, S = E.K, ctx.S
    N = ctx.N
    recs, low = [], None
    for pre, inp, planes, stride, dil, has_ds in blocks:
        zin, H, W = a, a.H, a.W
        P = N * H * W
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        Po = N * Ho * Wo
        y1 = E._buf(x, P, planes)
        st = E._stats(ctx, planes, training)
        K.conv(zin, E._w(ctx, pre + ".conv1.weight", "ohwi"), 1, 1, y1, stats=st)
        a1 = E._bn_act(ctx, pre + ".bn1", y1, N, H, W, st, P, training, ACT_RELU)
        y2 = E._buf(x, Po, planes)
        st = E._stats(ctx, planes, training)
        conv3x3(E, ctx, a1, pre + ".conv2.weight", dil, stride, y2, st, narrow)
        a2 = E._bn_act(ctx, pre + ".bn2", y2, N, Ho, Wo, st, Po, training, ACT_RELU)
        y3 = E._buf(x, Po, 4 * planes)
        st = E._stats(ctx, 4 * planes, training)
        K.conv(a2, E._w(ctx, pre + ".conv3.weight", "ohwi"), 1, 1, y3, stats=st)
        a3 = E._bn_act(ctx, pre + ".bn3", y3, N, Ho, Wo, st, Po, training, ACT_NONE)
        zs = ad = None
        if has_ds:
            zs = zin
            if stride != 1:
                zsb = E._buf(x, Po, inp)
                K.rows_stride(zin.x, N, H, W, stride, zsb)
                zs = Act(zsb, N, Ho, Wo, zin.scale, zin.shift, zin.act, bn=zin.bn)     # the pending transform is per channel
            yd = E._buf(x, Po, 4 * planes)
            st = E._stats(ctx, 4 * planes, training)
            K.conv(zs, E._w(ctx, pre + ".downsample.0.weight", "ohwi"), 1, 1, yd, stats=st)
            ad = E._bn_act(ctx, pre + ".downsample.1", yd, N, Ho, Wo, st, Po, training, ACT_NONE)
        zo = E._buf(x, Po, 4 * planes)
        K.bn_add_relu(a3, ad if has_ds else zin, zo)
        a = Act(zo, N, Ho, Wo)
        recs.append(dict(pre=pre, stride=stride, dil=dil, zin=zin, a1=a1, a2=a2, a3=a3, zs=zs, ad=ad, zo=a))
        if pre == low_after:
            low = a
    S["rblocks"] = recs
    return a, low


def bottlenecks_backward(E, ctx, G, d_z, d_low, low_after, narrow=None):
    """d_z: gradient w.r.t. the last block's output, d_low: w.r.t. the output of block ``low_after``.  Returns the gradient
    w.r.t. the (activated) input of the first block."""
    K, S, x = E.K, ctx.S, ctx.x
    N = ctx.N
    for r in reversed(S["rblocks"]):
        pre, stride, dil = r["pre"], r["stride"], r["dil"]
        zin, a1, a2, a3, zs, ad, zo = r["zin"], r["a1"], r["a2"], r["a3"], r["zs"], r["ad"], r["zo"]
        H, W, Ho, Wo = zin.H, zin.W, zo.H, zo.W
        if pre == low_after:
            d_z.add_(d_low)
        g = E._buf(x, zo.P, zo.C)
        K.relu_gate(d_z, zo.x, g)
        del d_z
        dy3 = E._buf(x, zo.P, zo.C)
        E._bn_backward(ctx, G, a3, g, out=dy3)
        E._wgrad(ctx, G, pre + ".conv3.weight", a2, dy3, 1, 1)
        dU2 = E._buf(x, a2.P, a2.C)
        E._dgrad(ctx, pre + ".conv3.weight", dy3, N, Ho, Wo, 1, 1, dU2)
        del dy3
        dy2 = E._bn_backward(ctx, G, a2, dU2)
        dU1 = E._buf(x, a1.P, a1.C)
        conv3x3_backward(E, ctx, G, pre + ".conv2.weight", a1, dy2, dil, stride, dU1, narrow)
        del dU2, dy2
        dy1 = E._bn_backward(ctx, G, a1, dU1)
        E._wgrad(ctx, G, pre + ".conv1.weight", zin, dy1, 1, 1)
        d_zin = E._buf(x, zin.P, zin.C)
        if ad is not None:
            dyd = E._bn_backward(ctx, G, ad, g)
            E._wgrad(ctx, G, pre + ".downsample.0.weight", zs, dyd, 1, 1)
            if stride == 1:
                E._dgrad(ctx, pre + ".downsample.0.weight", dyd, N, H, W, 1, 1, d_zin)
            else:
                d_zs = E._buf(x, zs.P, zs.C)
                E._dgrad(ctx, pre + ".downsample.0.weight", dyd, N, Ho, Wo, 1, 1, d_zs)
                K.rows_stride(d_zs, N, H, W, stride, d_zin, scatter=True)
                del d_zs
            E._dgrad(ctx, pre + ".conv1.weight", dy1, N, H, W, 1, 1, d_zin, addend=d_zin)
        else:
            E._dgrad(ctx, pre + ".conv1.weight", dy1, N, H, W, 1, 1, d_zin, addend=g)
        del g, dU1, dy1
        d_z = d_zin
    return d_z
