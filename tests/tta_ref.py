"""torch restatements, on the CPU, of the views of test-time augmentation (include/uda_clr_hip.h, uda_tta_view / uda_tta_fuse), written
from their definitions with torch.flip / transpose / rot90 / F.interpolate(align_corners=True), in float64 and in fp32, the inputs of
the tests and host stand-ins for ops.tta_view / ops.tta_fuse."""
import numpy as np
import torch
import torch.nn.functional as F

import uncertainty_ref as ur

CODES = {"id": 0, "hflip": 1, "vflip": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6, "antitranspose": 7}


def permute(t, g):
    """the view code g applied to the last two axes of t (no resampling)"""
    if g == 0:
        return t
    if g == 1:
        return torch.flip(t, (-1,))
    if g == 2:
        return torch.flip(t, (-2,))
    if g == 3:
        return torch.flip(t, (-2, -1))
    if g == 4:
        return t.transpose(-2, -1)
    if g == 5:
        return torch.rot90(t, 1, (-2, -1))
    if g == 6:
        return torch.rot90(t, -1, (-2, -1))
    if g == 7:
        return torch.flip(t, (-2, -1)).transpose(-2, -1)
    raise ValueError(g)


def unpermute(t, g):
    """the inverse of ``permute``: the transpose is undone first, then the two mirrorings"""
    if g & 4:
        t = t.transpose(-2, -1)
    dims = tuple(d for d, bit in ((-2, 2), (-1, 1)) if g & bit)
    return torch.flip(t, dims) if dims else t


def resize(t, size):
    size = tuple(int(s) for s in size)
    return t if tuple(t.shape[-2:]) == size else F.interpolate(t, size, mode="bilinear", align_corners=True)


def view(image, v, dtype=torch.float32):
    """the input of view v = (g, h, w) of a [B,C,H,W] image, computed in ``dtype``"""
    g, h, w = v
    return permute(resize(image.to(dtype), (h, w)), g).contiguous()


def unview(logits, v, size, dtype=torch.float32):
    """the logits of view v mapped back to the frame ``size`` = (H, W), computed in ``dtype``"""
    return resize(unpermute(logits.to(dtype), v[0]).contiguous(), size)


def view_shape(v):
    g, h, w = v
    return (w, h) if g & 4 else (h, w)


def fuse64(view_logits, views, size):
    """float64 maps {'mean', 'std', 'entropy', 'mi'} of the views' logits mapped back in float64"""
    z = torch.stack([unview(t, v, size, torch.float64) for t, v in zip(view_logits, views)])
    return ur.maps64(z.numpy())


def fuse32_torch(view_logits, views, size):
    """the same in fp32 torch: the yardstick of the kernel's error bound"""
    z = torch.stack([unview(t, v, size, torch.float32) for t, v in zip(view_logits, views)])
    return ur.maps32_torch(z)


def view_logits(views, B, C, seed):
    """random fp32 logits of the views' shapes: smooth x 4 plus noise, so that probabilities spread and the views disagree"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for v in views:
        r, c = view_shape(v)
        base = F.avg_pool2d(2.0 * torch.randn(B, C, r, c, generator=g), 5, 1, 2) * 4.0
        out.append((base + 0.5 * torch.randn(B, C, r, c, generator=g)).contiguous())
    return out


class HostTta(object):
    """ops.tta_view / ops.tta_fuse on the host (fp32 views, float64 maps), with every call kept"""
    def __init__(self):
        self.view_calls, self.fuse_calls = [], []

    def tta_view(self, image, v):
        self.view_calls.append((tuple(image.shape), tuple(v)))
        return view(image.detach().cpu(), v)

    def tta_fuse(self, logits, views, size, outputs=("mean",), u8_scale=None):
        self.fuse_calls.append(([tuple(t.shape) for t in logits], [tuple(v) for v in views], tuple(size), tuple(outputs), u8_scale))
        m = fuse64([t.detach().cpu() for t in logits], views, size)
        out = {k: torch.from_numpy(m[k].astype(np.float32)) for k in outputs}
        if u8_scale is not None:
            out["std_u8"] = torch.from_numpy(ur.quantise(m["std"].astype(np.float32), u8_scale))
        return out
