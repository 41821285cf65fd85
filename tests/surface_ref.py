"""scipy oracle of the surface-distance kernels (csrc/surface.hip) and the masks the tests feed them.

medpy.metric.binary's conventions with scipy alone (medpy is not a dependency): border(M) = M & ~binary_erosion(M, cross),
outside of the image unset; d2_X = squared Euclidean distance to the nearest pixel of border(X), an integer, recovered exactly
from scipy's float64 transform by rint(edt ** 2); a directed entry A -> G is (|border(A)|, sum of sqrt(d2_G) over border(A),
max of d2_G over border(A)).  If either border set is empty both entries are (n, NaN, -1), and the distance map to an empty
border set is -1 everywhere (scipy's transform has no defined value there)."""
import math

import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)


def border(m):
    m = np.asarray(m).astype(bool)
    return m & ~ndimage.binary_erosion(m, CROSS)


def d2_to_border(m):
    b = border(m)
    if not b.any():
        return np.full(b.shape, -1, np.int64)
    return np.rint(ndimage.distance_transform_edt(~b) ** 2).astype(np.int64)


def d2_brute(m):
    """the same map as an integer minimum over all border pixels"""
    b = border(m)
    ys, xs = np.nonzero(b)
    yy, xx = np.mgrid[0:b.shape[0], 0:b.shape[1]]
    return ((yy[..., None] - ys) ** 2 + (xx[..., None] - xs) ** 2).min(-1).astype(np.int64)


def table(a, g):
    """[2 dir: a -> g, g -> a][3: n, s, m] float64 of one (image, class)"""
    ba, bg = border(a), border(g)
    out = np.empty((2, 3), np.float64)
    empty = not ba.any() or not bg.any()
    for k, (src, other) in enumerate(((ba, g), (bg, a))):
        out[k, 0] = int(src.sum())
        if empty:
            out[k, 1:] = np.nan, -1.0
        else:
            d = d2_to_border(other)[src]
            out[k, 1:] = math.fsum(np.sqrt(d.astype(np.float64)).tolist()), float(d.max())
    return out


def reference(pred, gt):
    """pred, gt bool [B,2,H,W] -> table f64 [B,2,2,3], counts i64 [B,2,3], d2 i64 [B,2,2,H,W] (0 = to gt border, 1 = to pred border)"""
    pred, gt = np.asarray(pred) > 0.5, np.asarray(gt) > 0.5
    B, C, H, W = pred.shape
    t = np.empty((B, C, 2, 3), np.float64)
    c = np.empty((B, C, 3), np.int64)
    d = np.empty((B, C, 2, H, W), np.int64)
    for b in range(B):
        for k in range(C):
            t[b, k] = table(pred[b, k], gt[b, k])
            c[b, k] = (pred[b, k] & gt[b, k]).sum(), pred[b, k].sum(), gt[b, k].sum()
            d[b, k, 0], d[b, k, 1] = d2_to_border(gt[b, k]), d2_to_border(pred[b, k])
    return t, c, d


def surface_distances(pred, gt):
    """stand-in for uda_clr_amd.ops.surface_distances on the host"""
    t, c, _ = reference(np.asarray(pred), np.asarray(gt))
    return t, c


def direct_metrics(a, g):
    """asd(a,g), asd(g,a), assd, hd of one (image, class) by the definitions' own mean / max (NaN if a border set is empty)"""
    ba, bg = border(a), border(g)
    if not ba.any() or not bg.any():
        return (float("nan"),) * 4
    dag = np.sqrt(d2_to_border(g)[ba].astype(np.float64))
    dga = np.sqrt(d2_to_border(a)[bg].astype(np.float64))
    ag, ga = math.fsum(dag.tolist()) / dag.size, math.fsum(dga.tolist()) / dga.size
    return ag, ga, (ag + ga) / 2.0, float(max(dag.max(), dga.max()))


# ---------------------------------------------------------------------------------------------------------------- masks
def ellipse(H, W, cy, cx, a, b, theta=0.0):
    """filled ellipse with semi-axes a (along the direction theta from the y axis) and b"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (yy - cy) * math.cos(theta) + (xx - cx) * math.sin(theta)
    v = -(yy - cy) * math.sin(theta) + (xx - cx) * math.cos(theta)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def random_ellipse(rng, H, W, lo=0.12, hi=0.3):
    s = min(H, W)
    return ellipse(H, W, rng.uniform(0.35, 0.65) * H, rng.uniform(0.35, 0.65) * W, rng.uniform(lo, hi) * s, rng.uniform(lo, hi) * s,
                   rng.uniform(0, math.pi))


def random_pairs(seed, B, H, W):
    """pred, gt bool [B,2,H,W]: rotated ellipses, the prediction a perturbed copy of the ground truth"""
    rng = np.random.default_rng(seed)
    s = min(H, W)
    pred, gt = np.zeros((B, 2, H, W), bool), np.zeros((B, 2, H, W), bool)
    for b in range(B):
        for c in range(2):
            cy, cx, a, d, th = rng.uniform(0.4, 0.6) * H, rng.uniform(0.4, 0.6) * W, rng.uniform(0.12, 0.3) * s, rng.uniform(0.12, 0.3) * s, rng.uniform(0, math.pi)
            gt[b, c] = ellipse(H, W, cy, cx, a, d, th)
            pred[b, c] = ellipse(H, W, cy + rng.uniform(-0.05, 0.05) * s, cx + rng.uniform(-0.05, 0.05) * s, a * rng.uniform(0.8, 1.2),
                                 d * rng.uniform(0.8, 1.2), th + rng.uniform(-0.3, 0.3))
    return pred, gt


def special_96x80():
    """pred, gt bool [3,2,96,80]: over the six planes - overlapping ellipses; a mask touching two image edges; a single pixel
    against an ellipse; the full image against a 1-pixel-wide line; two disjoint blobs against one; a checkerboard patch."""
    H, W = 96, 80
    rng = np.random.default_rng(7)
    pred, gt = np.zeros((3, 2, H, W), bool), np.zeros((3, 2, H, W), bool)
    pred[0, 0], gt[0, 0] = ellipse(H, W, 44, 36, 25, 14, 0.5), ellipse(H, W, 50, 42, 22, 18, 1.1)
    pred[0, 1], gt[0, 1] = ellipse(H, W, 4, 6, 30, 22, 0.3), random_ellipse(rng, H, W)          # runs over the top and the left edge
    pred[1, 0, 40, 13] = True
    gt[1, 0] = random_ellipse(rng, H, W)
    pred[1, 1][:] = True
    gt[1, 1][np.arange(10, 70), np.arange(10, 70) // 2 + 20] = True                             # a 1-pixel-wide oblique line
    gt[1, 1][80, 5:75] = True                                                                   # and a horizontal one
    pred[2, 0] = ellipse(H, W, 20, 20, 9, 12) | ellipse(H, W, 70, 58, 14, 8, 0.7)
    gt[2, 0] = ellipse(H, W, 48, 40, 20, 20)
    yy, xx = np.mgrid[0:H, 0:W]
    pred[2, 1] = ((yy + xx) % 2 == 0) & (yy >= 30) & (yy < 61) & (xx >= 11) & (xx < 50)
    gt[2, 1] = random_ellipse(rng, H, W)
    assert pred[0, 1][0].any() and pred[0, 1][:, 0].any() and (border(pred[2, 1]) == pred[2, 1]).all()
    return pred, gt


def empty_96x80():
    """pred, gt bool [3,2,96,80]: class 0 of the three images has an empty prediction, an empty ground truth, both empty"""
    pred, gt = random_pairs(11, 3, 96, 80)
    pred[0, 0] = False
    gt[1, 0] = False
    pred[2, 0] = False
    gt[2, 0] = False
    return pred, gt


# ------------------------------------------------------------------------------------------- inputs of the evaluate() tests
def eval_batches(n_images=4, batch=2, S=128, seed=3):
    """[{'image', 'map', 'img_name'}] with ground-truth ellipses of semi-axes >= 20 px (the radius-7 erosion of the
    post-processing cannot empty them) and, per image, the logits (+-6) of a shifted and rescaled copy."""
    import torch
    rng = np.random.default_rng(seed)
    out, logits = [], {}
    for b0 in range(0, n_images, batch):
        mp = np.zeros((batch, 2, S, S), np.float32)
        lg = np.zeros((batch, 2, S, S), np.float32)
        names = []
        for i in range(batch):
            cy, cx = rng.uniform(0.45, 0.55, 2) * S
            for c, (lo, hi) in enumerate(((20, 26), (32, 40))):
                a, d, th = rng.uniform(lo, hi), rng.uniform(lo, hi), rng.uniform(0, math.pi)
                mp[i, c] = ellipse(S, S, cy, cx, a, d, th)
                p = ellipse(S, S, cy + rng.uniform(-4, 4), cx + rng.uniform(-4, 4), max(a * rng.uniform(0.9, 1.15), 20.0),
                            max(d * rng.uniform(0.9, 1.15), 20.0), th)
                lg[i, c] = np.where(p, 6.0, -6.0)
            names.append("img_%02d.png" % (b0 + i))
        image = torch.from_numpy(rng.standard_normal((batch, 3, S, S)).astype(np.float32))
        image[:, 0, 0, 0] = torch.arange(b0, b0 + batch, dtype=torch.float32)          # the stand-in model's key to its logits
        for i in range(batch):
            logits[b0 + i] = torch.from_numpy(lg[i])
        out.append({"image": image, "map": torch.from_numpy(mp), "img_name": names})
    return out, logits


def standin_model(logits):
    """callable image -> (logits, None): looks the batch's logits up by the index stored in image[:, 0, 0, 0]"""
    import torch

    def model(image):
        idx = [int(round(float(v))) for v in image[:, 0, 0, 0].cpu()]
        return torch.stack([logits[i] for i in idx]).to(image.device), None
    return model
