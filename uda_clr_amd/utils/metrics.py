"""Validation metrics - drop-in for the reference's ``utils/metrics.py`` (same function names and
return conventions).  The thresholding and the three pixel counts per class run in one HIP kernel
(uda_seg_counts); Dice, pixel accuracy and IoU are closed forms of those counts:

    dice = (2I + 1) / (1 + S + G)                                 (metrics.py:71-101, +1 smoothing)
    2x2 confusion (rows = label, cols = prediction): TP = I, FP = S - I, FN = G - I, TN = n - S - G + I
    PA = (TP + TN) / n,  IoU_fg = TP / (TP + FP + FN),  IoU_bg = TN / (TN + FP + FN)   (:149-168)
"""
import math

import numpy as np
import torch

from .. import ops


def dice_from_counts(inter, seg, gt):
    return (2.0 * float(inter) + 1.0) / (1.0 + float(seg) + float(gt))


def dice_coeff_2label(pred, target):
    """(cup dice, disc dice) at sigmoid(pred) > 0.75 over the whole batch (metrics.py:118-132)."""
    c = ops.seg_counts(pred, target, 0.75)
    return dice_from_counts(*c[0].tolist()), dice_from_counts(*c[1].tolist())


def dice_coeff(pred, target):
    """Single-label Dice at threshold 0.5 (metrics.py:104-116) over all channels together."""
    c = ops.seg_counts(pred, target, 0.5).sum(0)
    return dice_from_counts(*c.tolist())


def _pa_miou(inter, seg, gt, n):
    tp, fp, fn = float(inter), float(seg - inter), float(gt - inter)
    tn = float(n) - tp - fp - fn
    pa = (tp + tn) / float(n)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = np.array([tn / (tn + fp + fn) if (tn + fp + fn) else np.nan,
                        tp / (tp + fp + fn) if (tp + fp + fn) else np.nan])
    return pa, float(np.nanmean(iou))


def pixel_acc(pred, target):
    """(PA_cup, PA_disc, IoU_cup, IoU_disc) as metrics.py:149-168."""
    c = ops.seg_counts(pred, target, 0.75)
    n = pred.shape[0] * pred.shape[2] * pred.shape[3]
    pa_c, iou_c = _pa_miou(*c[0].tolist(), n)
    pa_d, iou_d = _pa_miou(*c[1].tolist(), n)
    return pa_c, pa_d, iou_c, iou_d


def DiceLoss(input, target):
    smooth = 1.0
    i, t = input.contiguous().view(-1), target.contiguous().view(-1)
    return 1 - ((2.0 * (i * t).sum() + smooth) / (i.sum() + t.sum() + smooth))


# ---- per-image metrics of an evaluation: closed forms of the table and counts of ops.surface_distances (medpy.metric.binary's
# definitions of asd / assd / hd in pixels; an (image, class) whose prediction or ground truth has no border pixel is NaN, where
# medpy raises, so that one empty mask does not stop a batch)
def surface_metrics_from_table(table):
    """table [B,2,2,3] (class; direction pred -> gt, gt -> pred; n, sum of distances, max squared distance) -> dict of [B,2]
    float64 arrays: asd_pred_gt, asd_gt_pred, assd = their mean, hd = sqrt of the larger max.  Pure numpy."""
    t = np.asarray(table, dtype=np.float64)
    n, s, m = t[..., 0], t[..., 1], t[..., 2]
    undefined = (n == 0).any(-1) | (m < 0).any(-1) | np.isnan(s).any(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        asd = np.where(undefined[..., None], np.nan, s / n)
        hd = np.where(undefined, np.nan, np.sqrt(np.maximum(m.max(-1), 0.0)))
    return {"asd_pred_gt": asd[..., 0], "asd_gt_pred": asd[..., 1], "assd": (asd[..., 0] + asd[..., 1]) / 2.0, "hd": hd}


def dice_per_image(counts):
    """counts [B,2,3] = (|pred & gt|, |pred|, |gt|) per image and class -> Dice [B,2] with the +1 smoothing of metrics.py:71-101."""
    c = np.asarray(counts, dtype=np.float64)
    return (2.0 * c[..., 0] + 1.0) / (1.0 + c[..., 1] + c[..., 2])


def assd_2label(pred_mask, gt_mask):
    """(cup, disc) average symmetric surface distance in pixels per image (arrays of length B) of [B,2,H,W] masks."""
    a = surface_metrics_from_table(ops.surface_distances(pred_mask, gt_mask)[0])["assd"]
    return a[:, 0], a[:, 1]


def hd_2label(pred_mask, gt_mask):
    """(cup, disc) Hausdorff distance in pixels per image (arrays of length B) of [B,2,H,W] masks."""
    h = surface_metrics_from_table(ops.surface_distances(pred_mask, gt_mask)[0])["hd"]
    return h[:, 0], h[:, 1]


# ---- closed forms of the profile of ops.surface_profile: percentiles of the surface distances (hd95 is medpy's
# np.percentile(np.hstack((d_pred_gt, d_gt_pred)), 95)), the surface Dice at a tolerance, the vertical cup-to-disc ratio
def _lerp(a, b, t):
    """numpy's percentile interpolation between a <= b at weight t"""
    d = b - a
    return np.where(t >= 0.5, b - d * (1.0 - t), a + d * t)


def percentile_distance_from_profile(table, profile):
    """table [B,2,2,3], profile of ``ops.surface_profile`` -> {'hd_p' [B,2,Q]: the percentiles of the distances of both directions
    pooled, 'hd_p_directed' [B,2,2,Q]: of pred -> gt and gt -> pred alone}, float64 pixels, NaN where either border set is empty.
    With n distances in a set and quantile q the virtual index is v = (n - 1) * q (the kernel's own single multiply), and the value
    lerp(sqrt(d2_lo), sqrt(d2_hi), v - floor(v)) of the lo-th and hi-th smallest squared distances the kernel selected."""
    n = np.asarray(table, dtype=np.float64)[..., 0]                                  # [B,2,2]
    order = np.asarray(profile["order"])                                                 # [B,2,3,Q,2]
    q = np.asarray(profile["quantiles"], dtype=np.float64)
    n3 = np.concatenate([n, n.sum(-1, keepdims=True)], -1)                               # [B,2,3]: pred -> gt, gt -> pred, pooled
    undefined = (order < 0).any(-1)
    v = np.maximum(n3 - 1.0, 0.0)[..., None] * q
    root = np.sqrt(np.maximum(order, 0).astype(np.float64))
    val = np.where(undefined, np.nan, _lerp(root[..., 0], root[..., 1], v - np.floor(v)))
    return {"hd_p": val[:, :, 2], "hd_p_directed": val[:, :, :2]}


def surface_dice_from_profile(table, profile):
    """Surface Dice (NSD) per tolerance [B,2,T]: the share of the border pixels of both masks that lie within the tolerance of the
    other mask's border, (within_0 + within_1) / (n_0 + n_1); NaN where either border set is empty."""
    n = np.asarray(table, dtype=np.float64)[..., 0].sum(-1)                          # [B,2]
    w = np.asarray(profile["within"])                                                    # [B,2,2,T]
    undefined = (w < 0).any(2) | (n == 0)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(undefined, np.nan, w.sum(2).astype(np.float64) / n[..., None])


def vertical_cdr_from_profile(profile):
    """Vertical cup-to-disc ratio per image from the masks' row extents: diameter = last row - first row + 1 (0 for an empty mask),
    vCDR = cup diameter / disc diameter, NaN where that disc is empty -> {'vcdr_pred', 'vcdr_gt', 'cdr_error' = |pred - gt|}, [B]."""
    e = np.asarray(profile["extent"])                                                    # [B, class, slot, 2]
    diam = np.where(e[..., 0] < 0, 0, e[..., 1] - e[..., 0] + 1).astype(np.float64)      # [B, class, slot]
    with np.errstate(divide="ignore", invalid="ignore"):
        vcdr = np.where(diam[:, 1] > 0, diam[:, 0] / diam[:, 1], np.nan)                 # [B, slot]
    return {"vcdr_pred": vcdr[:, 1], "vcdr_gt": vcdr[:, 0], "cdr_error": np.abs(vcdr[:, 1] - vcdr[:, 0])}


# ---- optic-disc morphometry: closed forms of the integers of ops.disc_morphometry.  Angles are in degrees,
# counter-clockwise from "right" as the image is seen (x = column, y = -row); nothing is named nasal or temporal, because the
# laterality of the eye is not known here.
def sector_table(K):
    """int64 [K,2]: the boundary rays (x, y) of K sectors, sector j spanning [360 j / K, 360 (j + 1) / K) degrees.  For j < K / 4,
    s_j = (rint(2^30 cos t), rint(2^30 sin t)) at t = 2 pi j / K in float64; the other three quadrants are exact 90-degree rotations,
    s_{j + K/4} = (-s_j.y, s_j.x).  K is a multiple of 8 in 8..360 (whole sectors per 90-degree quadrant centred on an axis)."""
    K = int(K)
    if K % 8 or not 8 <= K <= 360:
        raise ValueError("sector_table: K must be a multiple of 8 in 8..360, got %d" % K)
    q = K // 4
    t = 2.0 * np.pi * np.arange(q, dtype=np.float64) / K
    s = np.empty((K, 2), np.int64)
    s[:q, 0], s[:q, 1] = np.rint(2.0 ** 30 * np.cos(t)), np.rint(2.0 ** 30 * np.sin(t))
    for k in range(1, 4):
        s[k * q:(k + 1) * q, 0], s[k * q:(k + 1) * q, 1] = -s[(k - 1) * q:k * q, 1], s[(k - 1) * q:k * q, 0]
    return s


def _row_means(a):
    """[B,n] -> [B]: per row the correctly rounded sum (math.fsum: no order of summation to state) of the entries that are not NaN,
    over their number; NaN where there is none"""
    out = np.full(a.shape[0], np.nan)
    for b, row in enumerate(a):
        vals = [float(v) for v in row if not math.isnan(v)]
        if vals:
            out[b] = math.fsum(vals) / len(vals)
    return out


def morphometry_from_moments(m):
    """m: the dict of ``ops.disc_morphometry`` -> dict of per-image float64 arrays (class 0 = cup, 1 = disc), all computed from the
    exact integers; NaN where a figure has no meaning:
        vcdr, hcdr [B]      cup / disc diameter along rows / columns (last - first + 1); NaN without a disc, 0 for an empty cup
        acdr [B]            n_cup / n_disc; NaN without a disc
        rim_area [B]        n_disc - overlap, pixels of the disc outside the cup
        centroid [B,2,2]    (row, column) per class; NaN for an empty plane
        major, minor [B,2]  4 sqrt(lambda) of the two eigenvalues of the pixel covariance, whose numerators n sum r^2 - (sum r)^2, ...
                            are formed in integers: the full axes of the ellipse with that covariance; NaN for an empty plane
        orientation [B,2]   angle of the major axis in (-90, 90] degrees (0 for a circle); eccentricity [B,2] = sqrt(1 - minor^2 / major^2)
        cup_offset [B,2]    cup centroid - disc centroid as (rows, columns)
        rim_ratio [B,K]     1 - R_cup / R_disc per sector, R = sqrt(radial) / n_disc the furthest pixel of the class in the sector:
                            the rim's share of the disc radius there.  NaN where either sector holds no pixel; with a wholly empty cup,
                            1 wherever the disc's sector holds one
        rdr_min, rdr_min_angle [B]   the thinnest rim and the centre of its sector (the first of equals) in degrees
        n_empty_sectors [B] sectors whose rim_ratio is NaN
        rim_up, rim_left, rim_down, rim_right [B]   mean rim_ratio (NaN entries left out) of the 90-degree quadrants centred on 90, 180,
                            270 and 0 degrees"""
    mom, ext = np.asarray(m["moments"], np.int64), np.asarray(m["extent"], np.int64)
    ovl, rad = np.asarray(m["overlap"], np.int64), np.asarray(m["radial"], np.int64)
    B, K = rad.shape[0], rad.shape[2]
    n, sr, sc, srr, scc, src = (mom[..., i] for i in range(6))                            # [B,2]
    nf = n.astype(np.float64)
    some, disc = n > 0, n[:, 1] > 0
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, lo, hi in (("vcdr", 0, 1), ("hcdr", 2, 3)):
            diam = np.where(ext[..., lo] < 0, 0, ext[..., hi] - ext[..., lo] + 1).astype(np.float64)
            out[name] = np.where(diam[:, 1] > 0, diam[:, 0] / diam[:, 1], np.nan)
        out["acdr"] = np.where(disc, nf[:, 0] / nf[:, 1], np.nan)
        out["rim_area"] = (n[:, 1] - ovl).astype(np.float64)
        cen = np.stack([sr / nf, sc / nf], -1)                                            # 0 / 0 = NaN for an empty plane
        out["centroid"] = cen
        n2 = nf * nf
        vrr, vcc, vrc = (n * srr - sr * sr) / n2, (n * scc - sc * sc) / n2, (n * src - sr * sc) / n2      # integer numerators < 2^61
        half, diff = (vcc + vrr) / 2.0, (vcc - vrr) / 2.0                                 # x = column, y = -row: cov_xy = -vrc
        root = np.sqrt(diff * diff + vrc * vrc)
        l1, l2 = half + root, np.maximum(half - root, 0.0)
        out["major"], out["minor"] = 4.0 * np.sqrt(l1), 4.0 * np.sqrt(l2)
        out["orientation"] = np.where(some, np.degrees(0.5 * np.arctan2(0.0 - 2.0 * vrc, vcc - vrr)), np.nan)      # 0.0 - 0.0 = +0.0: 90, not -90
        out["eccentricity"] = np.where(l1 > 0, np.sqrt(1.0 - l2 / l1), np.where(some, 0.0, np.nan))
        out["cup_offset"] = cen[:, 0] - cen[:, 1]
        R = np.sqrt(np.maximum(rad, 0).astype(np.float64)) / nf[:, 1, None, None]         # [B,2,K]
        ratio = np.where((rad < 0).any(1), np.nan, 1.0 - R[:, 0] / R[:, 1])
        ratio = np.where((~some[:, 0])[:, None] & (rad[:, 1] >= 0), 1.0, ratio)
    out["rim_ratio"] = ratio
    empty = np.isnan(ratio)
    out["n_empty_sectors"] = empty.sum(1).astype(np.float64)
    first = np.where(empty, np.inf, ratio).argmin(1)
    out["rdr_min"] = np.where(empty.all(1), np.nan, np.where(empty, np.inf, ratio).min(1))
    out["rdr_min_angle"] = np.where(empty.all(1), np.nan, (first + 0.5) * (360.0 / K))
    e = K // 8
    turned = np.roll(ratio, e, axis=1)                                                    # entry 0 = sector K - K/8: -45 degrees
    for i, name in enumerate(("rim_right", "rim_up", "rim_left", "rim_down")):
        out[name] = _row_means(turned[:, 2 * e * i:2 * e * (i + 1)])
    return out


def hd95_2label(pred_mask, gt_mask):
    """(cup, disc) 95th-percentile Hausdorff distance in pixels per image (arrays of length B) of [B,2,H,W] masks."""
    table, _, profile = ops.surface_profile(pred_mask, gt_mask, percentiles=(95,))
    h = percentile_distance_from_profile(table, profile)["hd_p"][..., 0]
    return h[:, 0], h[:, 1]


# ---- calibration and selective prediction: closed forms, in float64, of the integer tables of ops.selective_tables
Q_ONE = 65536                # q = rint(p * Q_ONE): the fixed-point probability of the reliability table


def _ratio(num, den):
    """num / den in float64, NaN where den is 0"""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)


def calibration_from_table(rel):
    """int64 [..., M, 5] reliability table (n, n_pos, sum q, sum q over gt-set pixels, sum q^2 per confidence bin; per (image, class),
    or summed over images for pooled figures) -> {
        'ece'         [...]  sum_b |n_pos - sum q / 65536| / sum n: the bins' |accuracy - confidence| weighted by their share
        'mce'         [...]  the largest |accuracy - confidence| of a bin that holds a pixel
        'brier'       [...]  mean (p - y)^2 = (sum q^2 - 2 * 65536 * sum q_pos + 65536^2 * n_pos) / (65536^2 * n), of the rounded p
        'confidence'  [...]  mean p            'prevalence'  [...]  share of gt-set pixels
        'bin_n' int64, 'bin_accuracy', 'bin_confidence'  [..., M]: the reliability diagram; NaN for an empty bin}
    NaN throughout for a table without a pixel."""
    rel = np.asarray(rel, np.int64)
    n, n_pos, q, q_pos, qq = (rel[..., i] for i in range(5))
    N = n.sum(-1)
    gap = np.abs(n_pos.astype(np.float64) - q.astype(np.float64) / Q_ONE)
    acc, conf = _ratio(n_pos, n), _ratio(q, n.astype(np.float64) * Q_ONE)
    with np.errstate(invalid="ignore"):
        mce = np.where(N > 0, np.max(np.where(n > 0, gap / np.maximum(n, 1), -np.inf), -1), np.nan)     # |acc - conf| without its cancellation
    num = qq.sum(-1) - 2 * Q_ONE * q_pos.sum(-1) + Q_ONE * Q_ONE * n_pos.sum(-1)                # an exact integer
    return {"ece": _ratio(gap.sum(-1), N), "mce": mce, "brier": _ratio(num, N.astype(np.float64) * (Q_ONE * Q_ONE)),
            "confidence": _ratio(q.sum(-1), N.astype(np.float64) * Q_ONE), "prevalence": _ratio(n_pos.sum(-1), N),
            "bin_n": n, "bin_accuracy": acc, "bin_confidence": conf}


def selective_from_table(risk, edges):
    """int64 [..., K, 4] risk table ((TP, FP, FN, TN) per uncertainty bin; per (image, class), or summed over images) and its K - 1
    edges -> per edge e_j, keeping the pixels with u < e_j (bins 0..j):
        'coverage' [..., K-1]  kept / all           'dice'   [..., K-1]  (2 TP + 1) / (2 TP + FP + FN + 1) over the kept pixels
        'error'    [..., K-1]  (FP + FN) / kept, NaN where nothing is kept
    and 'error_all' [...] the error rate of all pixels,
        'aurc'      [...] area under the binned risk-coverage curve: the points (coverage, error) of the K prefixes bins 0..j, joined by
                    trapezoids, the stretch from coverage 0 to the first point that keeps a pixel at that point's error
        'unc_auroc' [...] probability that a wrong pixel is more uncertain than a right one, ties counted half (Mann-Whitney), from
                    the two histograms: a pair inside one bin is a tie.  NaN when there is no wrong or no right pixel
        'edges' as given."""
    risk = np.asarray(risk, np.int64)
    edges = np.asarray(edges, np.float64)
    K = risk.shape[-2]
    if edges.shape != (K - 1,):
        raise ValueError("selective_from_table: %d bins need %d edges, got %s" % (K, K - 1, edges.shape))
    cum = np.cumsum(risk, -2)                                                # prefix j = bins 0..j
    tp, fp, fn, tn = (cum[..., i] for i in range(4))
    kept, total = tp + fp + fn + tn, risk.sum((-1, -2))
    wrong_k, right_k = risk[..., 1] + risk[..., 2], risk[..., 0] + risk[..., 3]
    cover, err = _ratio(kept, total[..., None]), _ratio(fp + fn, kept)
    # trapezoids over the K prefixes; a prefix that keeps nothing has zero width and takes the first defined error
    first = np.argmax(kept > 0, -1)
    e = np.where(kept > 0, err, np.take_along_axis(err, first[..., None], -1))
    aurc = cover[..., 0] * e[..., 0] + ((cover[..., 1:] - cover[..., :-1]) * (e[..., 1:] + e[..., :-1]) / 2).sum(-1)
    below = np.cumsum(right_k, -1) - right_k                                # right pixels in lower bins
    two_u = (wrong_k * (2 * below + right_k)).sum(-1)
    W, R = wrong_k.sum(-1), right_k.sum(-1)
    return {"coverage": cover[..., :-1], "dice": _ratio(2 * tp + 1, 2 * tp + fp + fn + 1)[..., :-1], "error": err[..., :-1],
            "error_all": _ratio(W, total), "aurc": np.where(total > 0, aurc, np.nan),
            "unc_auroc": _ratio(two_u, 2.0 * W.astype(np.float64) * R.astype(np.float64)), "edges": edges}
