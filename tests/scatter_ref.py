"""float64 restatement of uda_proto_scatter (include/uda_clr_hip.h) and the quantities its error bound is stated in."""
import torch


def scatter64(feat, wts, centre=None):
    """S[k][i][j] = sum_p w_k[p] (f[p,i] - a_k[i]) (f[p,j] - a_k[j]) in float64: feat [P, C], wts [P, 4], centre [4, C] or None"""
    f, w = feat.double().cpu(), wts.double().cpu()
    a = torch.zeros(4, f.shape[1], dtype=torch.float64) if centre is None else centre.double().cpu()
    d = f[None] - a[:, None]                                    # [4, P, C]
    return torch.einsum("pk,kpi,kpj->kij", w, d, d)


def abs_scatter64(feat, wts, centre=None):
    """A[k][i][j] = sum_p |w_k[p]| |f[p,i] - a_k[i]| |f[p,j] - a_k[j]| in float64: what the rounding errors are relative to"""
    f, w = feat.double().cpu(), wts.double().cpu()
    a = torch.zeros(4, f.shape[1], dtype=torch.float64) if centre is None else centre.double().cpu()
    d = (f[None] - a[:, None]).abs()
    return torch.einsum("pk,kpi,kpj->kij", w.abs(), d, d)


def gamma(n):
    """gamma_n = n u / (1 - n u) with u = 2^-24, the unit roundoff of fp32"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def moments64(feat, wts):
    """weighted count [4], mean [4, C] and biased covariance [4, C, C] of the rows, in float64 about the true mean"""
    f, w = feat.double().cpu(), wts.double().cpu()
    count = w.sum(0)
    mean = (w.t() @ f) / count[:, None]
    d = f[None] - mean[:, None]
    cov = torch.einsum("pk,kpi,kpj->kij", w, d, d) / count[:, None, None]
    return count, mean, cov
