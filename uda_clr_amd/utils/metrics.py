"""Validation metrics - drop-in for the reference's ``utils/metrics.py`` (same function names and
return conventions).  The thresholding and the three pixel counts per class run in one HIP kernel
(uda_seg_counts); Dice, pixel accuracy and IoU are closed forms of those counts:

    dice = (2I + 1) / (1 + S + G)                                 (metrics.py:71-101, +1 smoothing)
    2x2 confusion (rows = label, cols = prediction): TP = I, FP = S - I, FN = G - I, TN = n - S - G + I
    PA = (TP + TN) / n,  IoU_fg = TP / (TP + FP + FN),  IoU_bg = TN / (TN + FP + FN)   (:149-168)
"""
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


def hd95_2label(pred_mask, gt_mask):
    """(cup, disc) 95th-percentile Hausdorff distance in pixels per image (arrays of length B) of [B,2,H,W] masks."""
    table, _, profile = ops.surface_profile(pred_mask, gt_mask, percentiles=(95,))
    h = percentile_distance_from_profile(table, profile)["hd_p"][..., 0]
    return h[:, 0], h[:, 1]
