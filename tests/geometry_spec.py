"""The numpy statement of uda_geometry_u8 (csrc/geometry.hip): the coefficient / bound / index tables of Pillow's 8-bit
BILINEAR resample and of its NEAREST resize, the two integer passes, and the backward chain of index maps
(flip -> quarter turns -> crop origin and pad -> scaled image -> source).  It is the CPU stand-in for the HIP entry, in the role
kernel_spec.py plays for the other kernels; every comparison against it is byte equality.

Record layout (int32 [GEOM_R], dataloaders.custom_transforms.GEOM_*):
    0 scale fired   1, 2 scaled (w, h)   3 pad width   4, 5 crop origin (x1, y1) in the padded image
    6 quarter turns (counter-clockwise, PIL's rotate(90) == np.rot90(a, 1))   7 flip left-right   8 flip top-bottom   9 crop size S
"""
import numpy as np

GEOM_R = 10
PRECISION_BITS = 22          # Pillow: 32 - 8 - 2


def bilinear_tables(n_in, n_out):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter (support 1): per output position the first
    source index, the number of taps and the taps' integer weights (double arithmetic, weights summed in tap order)."""
    scale = float(n_in) / float(n_out)
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    ksize = int(np.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in)
    n = xmax - xmin
    w = np.zeros((n_out, ksize), np.float64)
    ww = np.zeros(n_out, np.float64)
    for t in range(ksize):
        arg = np.abs(((t + xmin) - center + 0.5) * ss)
        wt = np.where((arg < 1.0) & (t < n), 1.0 - arg, 0.0)
        w[:, t] = wt
        ww = ww + wt
    ww = np.where(ww != 0.0, ww, 1.0)
    k = (0.5 + (w / ww[:, None]) * float(1 << PRECISION_BITS)).astype(np.int64)       # no negative weights for this filter
    k[np.arange(ksize)[None, :] >= n[:, None]] = 0
    return xmin.astype(np.int32), n.astype(np.int32), k.astype(np.int32)


def nearest_table(n_in, n_out):
    """Pillow's ImagingScaleAffine index table: xo starts at a / 2 and is ACCUMULATED in double, index = (int)xo."""
    a = float(n_in) / float(n_out)
    steps = np.full(n_out, a, np.float64)
    steps[0] = a * 0.5
    xo = np.cumsum(steps)                  # sequential double additions
    return np.minimum(xo.astype(np.int64), n_in - 1).astype(np.int32)


def _pass(src, xmin, n, k):
    """one 8-bit pass along axis 1 of src [rows, n_in, C]: clip8((2^21 + sum src * k) >> 22)"""
    acc = np.full((src.shape[0], len(xmin), src.shape[2]), 1 << (PRECISION_BITS - 1), np.int64)
    for t in range(k.shape[1]):
        idx = np.minimum(xmin + t, src.shape[1] - 1)
        acc += src[:, idx, :].astype(np.int64) * k[None, :, t, None]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_bilinear(src, w, h):
    """Image.resize((w, h), BILINEAR) of an 8-bit image [H0, W0, C]: horizontal pass, then vertical over its uint8 result;
    an axis whose size does not change is skipped."""
    H0, W0 = src.shape[:2]
    out = src
    if w != W0:
        out = _pass(out, *bilinear_tables(W0, w))
    if h != H0:
        out = _pass(out.transpose(1, 0, 2), *bilinear_tables(H0, h)).transpose(1, 0, 2)
    return np.ascontiguousarray(out)


def resize_nearest(src, w, h):
    """Image.resize((w, h), NEAREST) of an 8-bit plane [H0, W0]"""
    H0, W0 = src.shape
    if (w, h) == (W0, H0):
        return src.copy()
    return np.ascontiguousarray(src[nearest_table(H0, h)][:, nearest_table(W0, w)])


def crop_coords(rec):
    """Backward index chain of one record: for every output pixel (i, j) the row and column in the S x S crop."""
    S, turns, flr, ftb = int(rec[9]), int(rec[6]) & 3, int(rec[7]), int(rec[8])
    i, j = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    if ftb:
        i = S - 1 - i
    if flr:
        j = S - 1 - j
    if turns == 1:              # rot90(a, 1)[i, j] = a[j, S-1-i]
        i, j = j, S - 1 - i
    elif turns == 2:
        i, j = S - 1 - i, S - 1 - j
    elif turns == 3:            # rot90(a, 3)[i, j] = a[S-1-j, i]
        i, j = S - 1 - j, i
    return i, j


def geometry(rec, image, label):
    """What the kernel writes for one sample: image uint8 [S, S, 3], label uint8 [S, S] from the source image [H0, W0, 3] and
    mask [H0, W0] and the int32 record."""
    rec = np.asarray(rec).reshape(-1)
    assert rec.shape[0] == GEOM_R
    H0, W0 = label.shape
    S = int(rec[9])
    w, h = (int(rec[1]), int(rec[2])) if rec[0] else (W0, H0)
    if rec[0]:
        image, label = resize_bilinear(image, w, h), resize_nearest(label, w, h)
    cy, cx = crop_coords(rec)
    sy, sx = cy + int(rec[5]) - int(rec[3]), cx + int(rec[4]) - int(rec[3])
    inside = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    syc, sxc = np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)
    out_i = np.where(inside[..., None], image[syc, sxc], 0).astype(np.uint8)
    out_l = np.where(inside, label[syc, sxc], 255).astype(np.uint8)
    assert out_i.shape == (S, S, 3)
    return out_i, out_l


def geometry_batch(records, index, images, labels):
    """records int32 [B, GEOM_R], index [B] into the lists of source arrays"""
    outs = [geometry(r, images[int(i)], labels[int(i)]) for r, i in zip(np.asarray(records), np.asarray(index).reshape(-1))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
