"""scipy / numpy oracle of pass 5 of the surface kernels (csrc/surface.hip, uda_surface_profile) on top of tests/surface_ref.py.

Per (image, class): the squared distances of both directions are gathered with surface_ref's `border` and `d2_to_border` and SORTED;
`order`, `within` and `extent` are read off the sorted arrays by the rules of include/uda_clr_hip.h, and the figures the closed forms
of utils/metrics.py are to reproduce are formed directly: np.percentile(np.hstack((d_ag, d_ga)), p) (medpy's hd95 at p = 95), the
count by sqrt(d2) <= tau, the row extents by np.nonzero."""
import numpy as np

import surface_ref as sr


def directed_d2(a, g):
    """sorted int64 squared distances (pred -> gt, gt -> pred) of one (image, class), or None if either border set is empty"""
    ba, bg = sr.border(a), sr.border(g)
    if not ba.any() or not bg.any():
        return None
    return np.sort(sr.d2_to_border(g)[ba]), np.sort(sr.d2_to_border(a)[bg])


def rows_of(m):
    ys = np.nonzero(np.asarray(m))[0]
    return (int(ys.min()), int(ys.max())) if ys.size else (-1, -1)


def tol2_of(tolerances):
    t = np.asarray(list(tolerances), np.float64)
    return np.floor(t * t).astype(np.int64)


def profile(pred, gt, percentiles=(95,), tolerances=()):
    """pred, gt bool [B,2,H,W] -> the dict ops.surface_profile returns as its third value"""
    pred, gt = np.asarray(pred) > 0.5, np.asarray(gt) > 0.5
    B = pred.shape[0]
    q = np.true_divide(np.asarray(list(percentiles), np.float64), 100)
    tol = np.asarray(list(tolerances), np.float64)
    t2 = tol2_of(tolerances)
    order = np.full((B, 2, 3, len(q), 2), -1, np.int64)
    within = np.full((B, 2, 2, len(tol)), -1, np.int64)
    extent = np.empty((B, 2, 2, 2), np.int64)
    for b in range(B):
        for c in range(2):
            extent[b, c, 0], extent[b, c, 1] = rows_of(gt[b, c]), rows_of(pred[b, c])
            d = directed_d2(pred[b, c], gt[b, c])
            if d is None:
                continue
            for s, arr in enumerate((d[0], d[1], np.sort(np.hstack(d)))):
                n = arr.size
                for i, qq in enumerate(q):
                    v = np.float64(n - 1) * qq
                    lo = int(np.floor(v))
                    order[b, c, s, i] = arr[lo], arr[min(lo + 1, n - 1)]
            for k in range(2):
                within[b, c, k] = [(d[k] <= t).sum() for t in t2]
    return {"order": order, "within": within, "extent": extent, "quantiles": q, "tolerances": tol, "tol2": t2}


def surface_profile(pred, gt, percentiles=(95,), tolerances=()):
    """stand-in for uda_clr_amd.ops.surface_profile on the host"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    t, c, _ = sr.reference(pred, gt)
    return t, c, profile(pred, gt, percentiles, tolerances)


def direct(pred, gt, percentiles, tolerances):
    """the figures by their definitions: hd_p [B,2,P] (pooled), hd_p_directed [B,2,2,P], nsd [B,2,T] by the FLOAT rule
    sqrt(d2) <= tau; NaN where a border set is empty"""
    pred, gt = np.asarray(pred) > 0.5, np.asarray(gt) > 0.5
    B, P, T = pred.shape[0], len(percentiles), len(tolerances)
    hd, hdd, nsd = np.full((B, 2, P), np.nan), np.full((B, 2, 2, P), np.nan), np.full((B, 2, T), np.nan)
    for b in range(B):
        for c in range(2):
            d = directed_d2(pred[b, c], gt[b, c])
            if d is None:
                continue
            dag, dga = np.sqrt(d[0].astype(np.float64)), np.sqrt(d[1].astype(np.float64))
            for i, p in enumerate(percentiles):
                hd[b, c, i] = np.percentile(np.hstack((dag, dga)), p)
                hdd[b, c, 0, i], hdd[b, c, 1, i] = np.percentile(dag, p), np.percentile(dga, p)
            for t, tau in enumerate(tolerances):
                nsd[b, c, t] = ((dag <= tau).sum() + (dga <= tau).sum()) / float(dag.size + dga.size)
    return {"hd_p": hd, "hd_p_directed": hdd, "nsd": nsd}


def vcdr_direct(pred, gt):
    """vcdr_pred, vcdr_gt [B] by np.nonzero row extents: cup height / disc height, NaN without a disc"""
    def one(m):
        h = []
        for c in range(2):
            lo, hi = rows_of(m[c])
            h.append(0 if lo < 0 else hi - lo + 1)
        return h[0] / h[1] if h[1] else float("nan")
    pred, gt = np.asarray(pred) > 0.5, np.asarray(gt) > 0.5
    return np.array([one(p) for p in pred]), np.array([one(g) for g in gt])


def percentile_bound(table, prof, ref):
    """4 * 2^-52 * ref + n * 2^-52 * (sqrt(d2_hi) - sqrt(d2_lo)), per set: [B,2,3,Q].  Both sides take correctly rounded square
    roots of the same integers; the lerp variants differ by at most two roundings; a virtual index formed differently moves the
    result by at most its own rounding (n * 2^-52 bounds an ulp of (n - 1) * q) times the gap."""
    eps = 2.0 ** -52
    n = np.asarray(table)[..., 0]
    n3 = np.concatenate([n, n.sum(-1, keepdims=True)], -1)[..., None]
    root = np.sqrt(np.maximum(prof["order"], 0).astype(np.float64))
    return 4 * eps * ref + n3 * eps * (root[..., 1] - root[..., 0])


# ---------------------------------------------------------------------------------------------------------------- masks
def ties_96x80():
    """pred, gt bool [1,2,96,80]: a gt line on row 40 and a pred line on row 50, both 60 pixels wide: the distances tie at d2 = 100"""
    pred, gt = np.zeros((1, 2, 96, 80), bool), np.zeros((1, 2, 96, 80), bool)
    gt[0, :, 40, 10:70] = True
    pred[0, :, 50, 10:70] = True
    return pred, gt


def top_digit_1024():
    """pred, gt bool [1,2,1024,1024]: single pixels in opposite corners (swapped in the disc plane): every d2 is 2 * 1023^2"""
    pred, gt = np.zeros((1, 2, 1024, 1024), bool), np.zeros((1, 2, 1024, 1024), bool)
    gt[0, 0, 0, 0] = pred[0, 0, 1023, 1023] = True
    pred[0, 1, 0, 0] = gt[0, 1, 1023, 1023] = True
    return pred, gt

