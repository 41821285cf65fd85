"""numpy / float64 restatement of uda_mc_uncertainty and uda_selective_tables (include/uda_clr_hip.h), written from their definitions,
the figures of utils.metrics.calibration_from_table / selective_from_table formed straight from the pixels, the inputs of the tests
and host stand-ins for ops.mc_uncertainty / ops.selective_tables."""
import math

import numpy as np
import torch

Q_ONE = 65536
DEFAULT_EDGES = (0.005, 0.01, 0.02, 0.03, 0.04, 0.06, 0.08, 0.12, 0.16)


# ------------------------------------------------------------------------------------------------------------------ the maps
def _entropy64(p):
    p = np.asarray(p, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(p > 0, -p * np.log(np.where(p > 0, p, 1.0)), 0.0)
        q = 1.0 - p
        b = np.where(q > 0, -q * np.log(np.where(q > 0, q, 1.0)), 0.0)
    return a + b


def _sigmoid64(x):
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def maps64(logits):
    """[T, ...] logits -> {'mean', 'std', 'entropy', 'mi'} in float64, from the float64 value of every logit"""
    x = np.asarray(logits, np.float64)
    T = x.shape[0]
    p = _sigmoid64(x)
    mean = p.mean(0)
    h = _sigmoid64(x / 2.0)
    std = np.sqrt(((h - h.mean(0)) ** 2).sum(0) / (T - 1))
    ent = _entropy64(mean)
    return {"mean": mean, "std": std, "entropy": ent, "mi": np.maximum(0.0, ent - _entropy64(p).mean(0))}


def maps32_torch(logits):
    """the same formulas stated in fp32 torch on the CPU: the yardstick of the kernel's error bound"""
    x = torch.as_tensor(logits, dtype=torch.float32)
    p = torch.sigmoid(x)
    mean = p.mean(0)
    std = torch.sigmoid(x / 2.0).std(0)
    H = lambda v: -(torch.xlogy(v, v) + torch.xlogy(1.0 - v, 1.0 - v))
    ent = H(mean)
    return {"mean": mean.numpy(), "std": std.numpy(), "entropy": ent.numpy(), "mi": torch.clamp(ent - H(p).mean(0), min=0.0).numpy()}


def quantise(std32, scale):
    """min(255, (int)floorf(std * scale)) in fp32"""
    v = np.floor(np.asarray(std32, np.float32) * np.float32(scale))
    return np.minimum(v, np.float32(255.0)).astype(np.uint8)


def mc_logits(T, B, H, W, seed):
    """[T,B,2,H,W] fp32: a smooth base x 6 plus per-pass noise on half of the pixels (tests/kernel_cases.py, the mc_stats case), and
    planted +-40, +-90 and 0: in every pass (std 0, entropy 0), and in one pass only among moderate ones"""
    g = torch.Generator().manual_seed(seed)
    base = torch.nn.functional.avg_pool2d(2.0 * torch.randn(B, 2, H, W, generator=g), 9, 1, 4) * 6.0
    x = base.repeat(T, 1, 1, 1) + 0.35 * torch.randn(T * B, 2, H, W, generator=g) * (torch.rand(1, 2, H, W, generator=g) > 0.5).float()
    x = x.reshape(T, B, 2, H, W).contiguous()
    flat = x.view(T, -1)
    for i, v in enumerate((40.0, -40.0, 90.0, -90.0, 0.0)):
        flat[:, 3 + 7 * i] = v                     # every pass
        flat[T - 1, 5 + 7 * i] = v                 # the last pass only
        flat[0, flat.shape[1] - 1 - i] = v         # the first pass only, in the last elements (the scalar path's tail)
    return x


# ------------------------------------------------------------------------------------------------------------------ the tables
def bins_of(p32, M):
    """confidence bin and q of valid p: fp32 multiply, as the kernel"""
    p32 = np.asarray(p32, np.float32)
    b = np.minimum(M - 1, np.floor(p32 * np.float32(M)).astype(np.int64))
    q = np.rint(p32.astype(np.float64) * Q_ONE).astype(np.int64)          # a power of two: exact in either precision
    return b, q


def tables(prob, unc, pred, gt=None, M=15, edges=DEFAULT_EDGES):
    """-> {'rel' int64 [B,2,M,5] or None, 'risk' int64 [B,2,K,4] or None, 'invalid' int64 [B,2,2], 'edges' float32}"""
    pred = np.asarray(pred) != 0
    gt = pred if gt is None else np.asarray(gt) != 0
    B = pred.shape[0]
    e32 = np.asarray(list(edges), np.float32)
    K = e32.size + 1
    rel = None if prob is None else np.zeros((B, 2, M, 5), np.int64)
    risk = None if unc is None else np.zeros((B, 2, K, 4), np.int64)
    invalid = np.zeros((B, 2, 2), np.int64)
    for b in range(B):
        for c in range(2):
            g, a = gt[b, c].ravel(), pred[b, c].ravel()
            if prob is not None:
                p = np.asarray(prob[b, c], np.float32).ravel()
                with np.errstate(invalid="ignore"):
                    ok = (p >= 0) & (p <= 1)
                invalid[b, c, 0] = (~ok).sum()
                bb, q = bins_of(p[ok], M)
                gg = g[ok].astype(np.int64)
                for j, v in enumerate((np.ones_like(q), gg, q, q * gg, q * q)):
                    rel[b, c, :, j] = _isum(bb, v, M)
            if unc is not None:
                u = np.asarray(unc[b, c], np.float32).ravel()
                with np.errstate(invalid="ignore"):
                    ok = u >= 0
                invalid[b, c, 1] = (~ok).sum()
                k = (e32[None, :] <= u[ok][:, None]).sum(1) if K > 1 else np.zeros(int(ok.sum()), np.int64)
                aa, gg = a[ok], g[ok]
                for j, sel in enumerate((aa & gg, aa & ~gg, ~aa & gg, ~aa & ~gg)):
                    risk[b, c, :, j] = np.bincount(k[sel], minlength=K)
    return {"rel": rel, "risk": risk, "invalid": invalid, "edges": e32}


def _isum(index, values, n):
    """exact integer sums per index (np.bincount's weights are float64: not exact for sums of q^2 beyond 2^53, so add integers)"""
    out = np.zeros(n, np.int64)
    np.add.at(out, index, values.astype(np.int64))
    return out


# ------------------------------------------------------------------------------------------ figures straight from the pixels
def direct_calibration(prob, gt, M):
    """ECE, MCE, Brier, mean confidence, prevalence of ONE plane by direct evaluation on p = q / 65536 (NaN and out-of-range p left out)"""
    p = np.asarray(prob, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        ok = (p >= 0) & (p <= 1)
    b, q = bins_of(p[ok], M)
    y = (np.asarray(gt).ravel()[ok] != 0).astype(np.float64)
    pq = q.astype(np.float64) / Q_ONE
    n = pq.size
    if n == 0:
        return dict(ece=math.nan, mce=math.nan, brier=math.nan, confidence=math.nan, prevalence=math.nan)
    gaps = [(abs(math.fsum(y[b == j]) - math.fsum(pq[b == j])), int((b == j).sum())) for j in range(M)]
    return dict(ece=math.fsum(g for g, _ in gaps) / n, mce=max(g / m for g, m in gaps if m), brier=math.fsum(((pq - y) ** 2).tolist()) / n,
                confidence=math.fsum(pq.tolist()) / n, prevalence=math.fsum(y.tolist()) / n)


def direct_selective(unc, pred, gt, edges):
    """per edge (u < edge kept) coverage, Dice, error; the overall error; of ONE plane (NaN and negative u left out)"""
    u = np.asarray(unc, np.float32).ravel()
    with np.errstate(invalid="ignore"):
        ok = u >= 0
    u, a, g = u[ok], np.asarray(pred).ravel()[ok] != 0, np.asarray(gt).ravel()[ok] != 0
    out = dict(coverage=[], dice=[], error=[], error_all=float((a != g).sum()) / u.size if u.size else math.nan)
    for e in np.asarray(list(edges), np.float32):
        k = u < e
        tp, fp, fn = int((a & g & k).sum()), int((a & ~g & k).sum()), int((~a & g & k).sum())
        out["coverage"].append(k.sum() / u.size if u.size else math.nan)
        out["dice"].append((2 * tp + 1) / (2 * tp + fp + fn + 1))
        out["error"].append((fp + fn) / int(k.sum()) if k.any() else math.nan)
    return out


def brute_auroc(bin_of_wrong, bin_of_right):
    """pair count: wrong pixel in a higher bin than the right one = 1, same bin = 1/2"""
    w, r = np.asarray(bin_of_wrong), np.asarray(bin_of_right)
    if w.size == 0 or r.size == 0:
        return math.nan
    wins = (w[:, None] > r[None, :]).sum()
    ties = (w[:, None] == r[None, :]).sum()
    return (2 * int(wins) + int(ties)) / (2 * w.size * r.size)


def direct_aurc(risk_plane):
    """trapezoids over the prefixes of ONE [K,4] table, by a plain loop"""
    total = int(risk_plane.sum())
    if total == 0:
        return math.nan
    pts, kept, wrong = [], 0, 0
    for row in risk_plane:
        kept += int(row.sum())
        wrong += int(row[1] + row[2])
        if kept:
            pts.append((kept / total, wrong / kept))
    area = pts[0][0] * pts[0][1]
    for (c0, e0), (c1, e1) in zip(pts, pts[1:]):
        area += (c1 - c0) * (e1 + e0) / 2
    return area


# ------------------------------------------------------------------------------------------------------------- host stand-ins
class HostOps(object):
    """ops.mc_uncertainty / ops.selective_tables on the host, with every call kept"""
    def __init__(self):
        self.unc_calls, self.table_calls = [], []

    def mc_uncertainty(self, logits, outputs=("mean", "std", "entropy", "mi"), u8_scale=None):
        x = logits.detach().cpu().numpy()
        m = maps64(x)
        out = {k: torch.from_numpy(m[k].astype(np.float32)) for k in outputs}
        if u8_scale is not None:
            out["std_u8"] = torch.from_numpy(quantise(m["std"].astype(np.float32), u8_scale))
        self.unc_calls.append((tuple(logits.shape), tuple(outputs), u8_scale))
        return out

    def selective_tables(self, prob, unc, pred, gt=None, bins=15, edges=DEFAULT_EDGES):
        n = lambda t: None if t is None else t.detach().cpu().numpy()
        mask = lambda t: None if t is None else (n(t) if t.dtype == torch.bool else n(t) > 0.5)
        args = dict(prob=n(prob), unc=n(unc), pred=mask(pred), gt=mask(gt), bins=bins, edges=tuple(edges))
        self.table_calls.append(args)
        return tables(args["prob"], args["unc"], args["pred"], args["gt"], bins, edges)


def noisy_passes(seed=11, sigma=1.5):
    """stand-in mc_logits for a brightness model: (image, T) -> [T,B,2,H,W] = the model's logits plus seeded noise, larger near the
    decision boundary so that the std spreads over the bins"""
    def passes(image, T):
        grey = (image.mean(1) + 1.0) * 127.5
        lg = torch.stack([(grey - 165.0), (grey - 110.0)], 1) / 8.0
        g = torch.Generator().manual_seed(seed + int(image.shape[0]))
        noise = torch.randn((T,) + tuple(lg.shape), generator=g).to(lg.device)
        return (lg[None] + sigma * noise * torch.exp(-lg.abs() / 4.0)[None]).contiguous()
    return passes
