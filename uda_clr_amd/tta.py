"""Test-time augmentation: predict an image under several views, map every prediction back to the image's frame, average.

A view is (g, h, w) as ``ops.tta_view`` takes it: the image resampled to h x w (align_corners=True; h and w multiples of 16 in 16..1024,
the sizes the generator accepts), mirrored left-right (g & 1) and top-bottom (g & 2), then transposed (g & 4).  The eight codes are the
symmetries of the square: a left eye is the mirror image of a right eye, and the disc's apparent size varies from camera to camera.

    views = parse_views("flips,id@0.75,id@1.25", H, W)
    maps = tta_predict(model, image, views, outputs=("mean", "std"))        # one model forward per distinct view shape

``ops.tta_view`` forms the views' inputs and ``ops.tta_fuse`` reads all V logit tensors once (csrc/tta.hip): 'mean' is the fused
probability, 'std' the unbiased std over the views of sigmoid(x / 2) - the quantity of the MC-dropout maps, so that
``ops.selective_tables`` and the risk-coverage report take it as it stands.  ``evaluate(..., tta=...)`` and ``predict`` use these."""
import math

import torch

from . import ops
from .inference import first_output
from .kernels import check_side

CODES = {"id": 0, "hflip": 1, "vflip": 2, "rot180": 3, "transpose": 4, "rot90": 5, "rot270": 6, "antitranspose": 7}
NAMES = tuple(sorted(CODES, key=CODES.get))
SHORTHANDS = {"flips": ("id", "hflip", "vflip", "rot180"), "d4": NAMES}
MIN_VIEWS, MAX_VIEWS = 2, 32


def scaled_size(n, s):
    """the side a scale ``s`` gives a side of ``n`` pixels: the nearest multiple of 16, at least 16"""
    return 16 * max(1, int(math.floor(n * s / 16.0 + 0.5)))


def _check_views(views):
    """[(g, h, w)] as ints, every one valid, no two equal, 2..32 of them"""
    out = []
    for v in views:
        try:
            g, h, w = (int(a) for a in v)
        except (TypeError, ValueError):
            raise ValueError("tta: a view is (g, h, w), got %r" % (v,)) from None
        if not 0 <= g <= 7:
            raise ValueError("tta: view code %d outside 0..7" % g)
        check_side("tta: view size", h, w)
        if (g, h, w) in out:
            raise ValueError("tta: view %s at %d x %d is given twice" % (NAMES[g], h, w))
        out.append((g, h, w))
    if not MIN_VIEWS <= len(out) <= MAX_VIEWS:
        raise ValueError("tta: %d views outside %d..%d" % (len(out), MIN_VIEWS, MAX_VIEWS))
    return out


def parse_views(spec, H, W):
    """'hflip,rot90@0.75,...' -> [(g, h, w)] for an H x W image.  Tokens, separated by commas: id hflip vflip rot180 transpose rot90
    rot270 antitranspose, and the shorthands flips (= id,hflip,vflip,rot180) and d4 (= all eight); each optionally followed by @s, a
    scale: h = 16 * max(1, floor(H * s / 16 + 0.5)), w likewise.  A view given twice (two scales may round to one size), fewer than 2
    or more than 32 views, an unknown token or a size outside 16..1024 is a ValueError."""
    check_side("tta: image height", int(H))
    check_side("tta: image width", int(W))
    if not isinstance(spec, str) or not spec.strip():
        raise ValueError("tta: a view list is a string such as 'flips,id@0.75', got %r" % (spec,))
    views = []
    for token in spec.split(","):
        name, at, scale = token.strip().partition("@")
        name = name.strip()
        s = 1.0
        if at:
            try:
                s = float(scale)
            except ValueError:
                raise ValueError("tta: scale %r of %r is not a number" % (scale, token.strip())) from None
            if not (s > 0.0 and math.isfinite(s)):
                raise ValueError("tta: scale %r of %r must be positive and finite" % (s, token.strip()))
        if name not in CODES and name not in SHORTHANDS:
            raise ValueError("tta: unknown view %r (known: %s, %s)" % (name, ", ".join(NAMES), ", ".join(SHORTHANDS)))
        h, w = (int(H), int(W)) if not at else (scaled_size(int(H), s), scaled_size(int(W), s))
        views += [(CODES[n], h, w) for n in SHORTHANDS.get(name, (name,))]
    return _check_views(views)


def normalise_views(tta, H, W):
    """a spec string or a list of (g, h, w) -> the checked list of (g, h, w) for an H x W image"""
    return parse_views(tta, H, W) if isinstance(tta, str) else _check_views(list(tta))


def view_shape(view):
    """(rows, columns) of the view's input and logits"""
    g, h, w = view
    return (w, h) if g & 4 else (h, w)


def tta_logits(model, image, views, max_batch=64):
    """The model's logits on every view of ``image`` [B,C,H,W]: ``ops.tta_view`` forms the inputs, views of equal tensor shape go
    through the model together - concatenated along the batch, at most ``max_batch`` images per forward (one view alone where B is
    larger) - and the V logit tensors come back in the order of ``views`` as slices of those forwards' outputs, not copies.
    ``model``'s first (or only) output is the logits."""
    views = _check_views(views)
    B = image.shape[0]
    per = max(1, int(max_batch) // B)
    groups = {}
    for v, view in enumerate(views):
        groups.setdefault(view_shape(view), []).append(v)
    logits = [None] * len(views)
    for members in groups.values():
        for i in range(0, len(members), per):
            part = members[i:i + per]
            inputs = [ops.tta_view(image, views[v]) for v in part]
            out = first_output(model(inputs[0] if len(part) == 1 else torch.cat(inputs))).float().contiguous()
            if out.shape[0] != B * len(part) or tuple(out.shape[2:]) != tuple(inputs[0].shape[2:]):
                raise ValueError("tta: the model gave logits %s for inputs %s" % (tuple(out.shape), (B * len(part),) + tuple(inputs[0].shape[1:])))
            for k, v in enumerate(part):
                logits[v] = out[k * B:(k + 1) * B]
    return logits


def tta_predict(model, image, views, outputs=("mean",), u8_scale=None, max_batch=64):
    """``tta_logits`` and then ``ops.tta_fuse``: {name: [B,C,H,W] device tensor} of the names in ``outputs`` ('mean', 'std', 'entropy',
    'mi'; with ``u8_scale`` also 'std_u8') for the image's own frame.  ``views``: a spec string or a list of (g, h, w)."""
    H, W = image.shape[-2:]
    views = normalise_views(views, H, W)
    return ops.tta_fuse(tta_logits(model, image, views, max_batch), views, (H, W), outputs, u8_scale)
