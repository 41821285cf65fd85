"""-m gpu: uda_proto_scatter (csrc/proto_scatter.hip) against its float64 restatement (tests/scatter_ref.py).

Accuracy.  Every entry is held to a bound derived from the arithmetic the header states, nothing fitted:
    |S - S64| <= gamma_n * A_ij,   A_ij = sum_p |w_k[p]| |f_pi - a_i| |f_pj - a_j| (fp64),   n = PS_SLAB + 4,
    gamma_n = n u / (1 - n u),  u = 2^-24:
two centring roundings, one weight multiply, a chain of at most PS_SLAB fused multiply-adds (one fp32 accumulator never sums more
pixels than that), one for the fp64 combine.  The features have a mean ten times their spread, so with a given centre A_ij is about a
hundred times smaller than the uncentred sum: an implementation that forms the moments about 0 and shifts would miss the bound.

Shapes.  Every C of {1, 3, 5, 31, 32, 33, 64, 65, 305} (below / at / above the 32-wide MFMA tile and the 64-wide channel block, the
flagship width) at two P; every P of {1, 7, 63, 65, PS_SLAB-1, PS_SLAB, PS_SLAB+1, 2 PS_SLAB+3} (below / at / above the 32-pixel chunk
and the slab) at C in {5, 33, 305}, each with both row strides; and one P beyond (partial sets) x PS_SLAB at C = 5, the smallest at
which a workgroup flushes a second slab into its partial.  Weights and centre rotate through soft / 0-1 / one class all-zero and
null / given.  Every case runs under kernel_cases.footprint(): only ``scatter`` and the stated workspace bytes may change."""
import functools
import os
import re

import pytest
import torch

import kernel_cases as kc
import scatter_ref as sr
from uda_clr_amd.acts import round4

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "uda_clr_amd", "csrc", "scatter_plan.h")) as _f:
    PS_SLAB = int(re.search(r"^#define\s+PS_SLAB\s+(\d+)\b", _f.read(), re.M).group(1))
GAMMA = sr.gamma(PS_SLAB + 4)

ALL_C = (1, 3, 5, 31, 32, 33, 64, 65, 305)
ALL_P = (1, 7, 63, 65, PS_SLAB - 1, PS_SLAB, PS_SLAB + 1, 2 * PS_SLAB + 3)
WKINDS = ("soft", "binary", "zero_class")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _data(P, C, wkind, given_centre):
    """host inputs and the float64 reference of one case, built once and never changed: (values [P,C], wts, centre, S64, A)"""
    g = kc.gen(1000 * C + P)
    vals = torch.randn(P, C, generator=g) * 0.3 + 3.0 + 0.2 * torch.randn(C, generator=g)      # mean ten times the spread
    wts = torch.rand(P, 4, generator=g)                                                         # soft, and no w_{k+2} = 1 - w_k
    if wkind == "binary":
        wts = (wts > 0.5).float()
    if wkind == "zero_class":
        wts[:, 2] = 0.0
    centre = (3.0 + 0.1 * torch.randn(4, C, generator=g)) if given_centre else None
    return vals, wts, centre, sr.scatter64(vals, wts, centre), sr.abs_scatter64(vals, wts, centre)


def _matrix(vals, extra):
    """[P, C] view of a [P, round4(C) + extra] buffer (kernel_cases.to_dev poisons the padding lanes of the device copy by row)"""
    P, C = vals.shape
    buf = kc._poison(torch.empty(P, round4(C) + extra))
    buf[:, :C] = vals
    return buf[:, :C]


def _run(vals, wts, centre, extra=4, pad=None, calls=1):
    """uda_proto_scatter through the binding into a zeroed output, under the footprint registry -> scatter on the host.
    pad: a value written ON THE DEVICE into lanes C .. ld - 1 of every row of the feature matrix, in place of the by-row poison"""
    K = kc.hip()
    P, C = vals.shape
    with kc.footprint():
        m = _matrix(vals, extra)
        if m.stride(0) == C:                                                                  # no padding lanes
            assert pad is None
            f = kc.ro_dev(m, DEV, "feat")
        else:
            f = kc.to_dev(m, DEV, "feat")
            if pad is not None:
                ld = f.stride(0)
                lanes = f.as_strided((P, ld - C), (ld, 1), f.storage_offset() + C)
                lanes.fill_(pad)
                assert bool(torch.isnan(lanes).all() if pad != pad else (lanes == pad).all())
            kc.read_only(f)                                                                   # the snapshot is taken with the padding in place
        w = kc.ro_dev(wts, DEV, "wts")
        a = kc.ro_dev(centre, DEV, "centre")
        out = kc.out_dev((4, C, C), torch.float64, DEV, fill=0, name="scatter")
        for _ in range(calls):
            K.proto_scatter(f, w, out, a)
        torch.cuda.synchronize()
        bad = kc.footprint_violations()
    assert bad == [], "uda_proto_scatter wrote outside scatter and its workspace: (buffer, first position)"
    return out.cpu()


def _check(P, C, extra, wkind, given_centre):
    vals, wts, centre, want, absum = _data(P, C, wkind, given_centre)
    got = _run(vals, wts, centre, extra)
    assert bool(torch.isfinite(got).all())
    excess = ((got - want).abs() - GAMMA * absum).max().item()
    worst = ((got - want).abs() / absum.clamp_min(1e-300)).max().item()
    print("P %d C %d ld +%d %s centre %s: max |S - S64| / A = %.3e (bound %.3e)" % (P, C, extra, wkind, given_centre, worst, GAMMA))
    assert excess <= 0.0, "an entry misses gamma_n * A_ij by %.3e (worst ratio %.3e, bound %.3e)" % (excess, worst, GAMMA)
    assert torch.equal(got, got.transpose(1, 2)), "the two triangles differ"
    if wkind == "zero_class":
        assert not bool(got[2].any()), "a class without weight is not exactly 0"
    return got


def _variant(i):
    return WKINDS[i % 3], bool((i // 3 + i) % 2)


@pytest.mark.parametrize("P", [65, PS_SLAB + 1])
@pytest.mark.parametrize("C", ALL_C)
def test_every_width_against_fp64(C, P):
    wkind, given = _variant(ALL_C.index(C) + (P > 65))
    _check(P, C, 4 if C % 2 else 0, wkind, given)


@pytest.mark.parametrize("extra", [0, 4], ids=["ld=round4", "ld=round4+4"])
@pytest.mark.parametrize("P", ALL_P)
@pytest.mark.parametrize("C", [5, 33, 305])
def test_every_pixel_count_against_fp64(C, P, extra):
    wkind, given = _variant(ALL_P.index(P) + (5, 33, 305).index(C))
    _check(P, C, extra, wkind, given)


@pytest.mark.parametrize("given", [False, True], ids=["null centre", "given centre"])
@pytest.mark.parametrize("wkind", WKINDS)
def test_weight_sets_and_centres(wkind, given):
    _check(PS_SLAB + 1, 33, 4, wkind, given)


def test_second_slab_into_one_partial():
    """more pixels than (partial sets) x PS_SLAB: a workgroup's range holds two slabs, the second is ADDED into its fp64 partial"""
    C = 5
    nsets = kc.hip().lib.uda_proto_scatter_workspace_bytes(C) // (4 * 64 * 64 * 8)          # one 64-wide channel block at C <= 64
    assert nsets >= 1
    _check((nsets + 1) * PS_SLAB + 5, C, 4, "soft", True)


def test_same_bits_twice_and_exactly_twice_when_called_twice():
    vals, wts, centre, _, _ = _data(2 * PS_SLAB + 3, 33, "soft", True)
    one = _run(vals, wts, centre)
    assert torch.equal(one, _run(vals, wts, centre)), "two runs of the same inputs differ"
    two = _run(vals, wts, centre, calls=2)
    assert torch.equal(two, 2.0 * one), "adding the same call twice is not exactly twice the first result"
    assert torch.equal(two, two.transpose(1, 2))


@pytest.mark.parametrize("extra", [0, 4], ids=["ld=round4", "ld=round4+4"])
@pytest.mark.parametrize("C", [5, 33, 305])
def test_nan_padding_lanes_change_no_bit(C, extra):
    """lanes C .. ld - 1 of every row of the DEVICE matrix hold 0.0 in one run and NaN in the other: the same bits come out"""
    vals, wts, centre, _, _ = _data(65, C, "soft", True)
    clean = _run(vals, wts, centre, extra=extra, pad=0.0)
    assert bool(torch.isfinite(clean).all()) and bool(clean.any())
    assert torch.equal(_run(vals, wts, centre, extra=extra, pad=float("nan")), clean)


def test_ops_class_scatter_front_end():
    from uda_clr_amd import ops
    g = kc.gen(7)
    B, C, h, w = 2, 33, 5, 7
    feat = (torch.randn(B, C, h, w, generator=g) * 0.3 + 3.0)
    wts = torch.rand(B * h * w, 4, generator=g)
    centre = 3.0 + 0.1 * torch.randn(4, C, generator=g)
    rows = feat.permute(0, 2, 3, 1).reshape(-1, C)
    want, absum = sr.scatter64(rows, wts, centre), sr.abs_scatter64(rows, wts, centre)
    got = ops.class_scatter(feat.to(DEV), wts.to(DEV), centre.to(DEV))
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == (4, C, C)
    assert bool(((got.cpu() - want).abs() <= GAMMA * absum).all())
    again = ops.class_scatter(feat.to(DEV), wts.to(DEV), centre.to(DEV), out=got)
    assert again is got and torch.equal(got.cpu(), 2.0 * ops.class_scatter(feat.to(DEV), wts.to(DEV), centre.to(DEV)).cpu())
    with pytest.raises(Exception):
        ops.class_scatter(feat, wts, centre)                                                  # a CPU tensor raises: no fallback


def test_bad_arguments_return_an_error_and_write_nothing():
    K = kc.hip()
    lib = K.lib
    P, C = 9, 5
    vals, wts, centre, _, _ = _data(P, C, "soft", True)
    need = lib.uda_proto_scatter_workspace_bytes(C)
    assert need > 0 and lib.uda_proto_scatter_workspace_bytes(C) == need
    with kc.footprint():
        f = kc.ro_dev(_matrix(vals, 4), DEV, "feat")
        w = kc.ro_dev(wts, DEV, "wts")
        a = kc.ro_dev(centre, DEV, "centre")
        out = kc.out_dev((4, C, C), torch.float64, DEV, fill=float("nan"), name="poisoned scatter")
        ws = kc.ro_dev(torch.full((need,), 0x5A, dtype=torch.uint8), DEV, "workspace")
        ok = dict(feat=f.data_ptr(), ldf=f.stride(0), P=P, C=C, wts=w.data_ptr(), centre=a.data_ptr(), scatter=out.data_ptr(),
                  ws=ws.data_ptr(), nbytes=need)
        bad = {"C = 0": dict(C=0), "C = 1025": dict(C=1025), "ldf too small": dict(ldf=round4(C) - 4), "ldf not a multiple of 4": dict(ldf=round4(C) + 2),
               "P = 0": dict(P=0), "null feat": dict(feat=None), "null wts": dict(wts=None), "null scatter": dict(scatter=None),
               "null workspace": dict(ws=None), "workspace too small": dict(nbytes=need - 1)}
        for name, change in bad.items():
            q = dict(ok, **change)
            rc = lib.uda_proto_scatter(q["feat"], q["ldf"], q["P"], q["C"], q["wts"], q["centre"], q["scatter"], q["ws"], q["nbytes"], _stream())
            assert rc != 0, name
            assert lib.uda_last_error(), name
        torch.cuda.synchronize()
        changed = kc.footprint_violations()
        still_nan = bool(torch.isnan(out).all())
    assert still_nan and changed == [], changed
