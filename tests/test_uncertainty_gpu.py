"""-m gpu: uda_mc_uncertainty and uda_selective_tables (csrc/uncertainty.hip) against the restatements of tests/uncertainty_ref.py,
DeepLab.mc_inference_logits, and evaluate / predict with MC passes end to end.

The maps.  Bound per map = 4 x the max abs error, against float64, of the SAME formulas stated in fp32 torch on the CPU
(uncertainty_ref.maps32_torch) on the same logits; the factor covers another expf and another order of summation.  That yardstick was
measured once, on the CPU, on the inputs of these tests (mc_logits(T, B, H, W, seed = 100 + T)) - max abs error of the fp32 torch
statement; the kernel's own figures are in profiles/uncertainty_kernels.md:

      T  shape          mean     std      entropy  mi
      2  [1,2,33,17]    6.5e-08  7.2e-08  1.8e-07  1.0e-07
      8  [1,2,33,17]    1.6e-07  2.3e-08  3.2e-07  2.7e-07
     32  [1,2,33,17]    3.1e-07  1.4e-08  8.0e-07  9.2e-07
      2  [2,2,96,80]    1.0e-07  8.8e-08  3.7e-07  1.4e-07
      8  [2,2,96,80]    2.1e-07  3.9e-08  9.8e-07  5.7e-07
     32  [2,2,96,80]    3.1e-07  1.9e-08  9.8e-07  7.5e-07

The test forms the same figures again from the same statement (_case) and bounds each map by 4 x its own.  torch.std sums in double on
the CPU, so its error is that of the fp32 sigmoids alone and shrinks with T; the kernel sums its deviations in double for that reason.
std_u8 has no tolerance: it must equal the fp32 quantisation
of the std map the same call stored.

The tables.  Every integer equal to the restatement's, no tolerance: the kernel is fed given maps, so no threshold can fall differently."""
import csv
import math

import numpy as np
import pytest
import torch

import uncertainty_ref as ur
from kernel_cases import footprint, footprint_violations, out_dev, ro_dev
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict
from uda_clr_amd.dataloaders import synthetic
from uda_clr_amd.utils import metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAPS = ("mean", "std", "entropy", "mi")
SHAPES = {"33x17": (1, 33, 17), "96x80": (2, 96, 80)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


_CASES = {}


def _case(T, shape):
    """logits, their float64 maps and the fp32 torch statement's max abs error per map: computed once per (T, shape)"""
    if (T, shape) not in _CASES:
        B, H, W = SHAPES[shape]
        x = ur.mc_logits(T, B, H, W, 100 + T)
        want = ur.maps64(x.numpy())
        t32 = ur.maps32_torch(x)
        yard = {k: float(np.abs(t32[k].astype(np.float64) - want[k]).max()) for k in MAPS}
        _CASES[(T, shape)] = (x, want, yard)
    return _CASES[(T, shape)]


# ------------------------------------------------------------------------------------------------------------------ the maps
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("T", [2, 8, 32])
def test_maps_against_float64(T, shape):
    x, want, yard = _case(T, shape)
    assert (x[0].numel() % 4 != 0) == (shape == "33x17")                      # 1122 elements per pass: rows 1, 3, ... are not 16-byte aligned
    got = ops.kernels().mc_uncertainty(x.to(DEV), MAPS, u8_scale=1600.0)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in got.items()}
    line = []
    for k in MAPS:
        assert host[k].shape == want[k].shape and host[k].dtype == np.float32
        err = float(np.abs(host[k].astype(np.float64) - want[k]).max())
        line.append("%s %.2e (yardstick %.2e)" % (k, err, yard[k]))
    print("T=%d %s: " % (T, shape) + ", ".join(line))
    for k in MAPS:
        err = float(np.abs(host[k].astype(np.float64) - want[k]).max())
        assert yard[k] > 0 and err <= 4 * yard[k], (k, err, yard[k])
    assert host["std_u8"].dtype == np.uint8 and np.array_equal(host["std_u8"], ur.quantise(host["std"], 1600.0))
    assert (host["mi"] >= 0).all() and (host["mi"] <= host["entropy"]).all() and host["entropy"].max() <= math.log(2.0) * (1 + 1e-6)
    flat = {k: v.reshape(-1) for k, v in host.items()}
    for i, v in enumerate((40.0, -40.0, 90.0, -90.0, 0.0)):                  # planted in every pass: no spread, and no entropy at |x| >= 40
        j = 3 + 7 * i
        assert flat["std"][j] == 0.0 and flat["std_u8"][j] == 0 and flat["mi"][j] <= 2e-7
        assert abs(flat["mean"][j] - (0.5 if v == 0 else float(v > 0))) <= 1e-15
        assert abs(flat["entropy"][j] - (math.log(2.0) if v == 0 else 0.0)) <= (2e-7 if v == 0 else 1e-14)


def test_quantisation_saturates_and_follows_the_stored_std():
    x, _, _ = _case(8, "33x17")
    for scale in (1600.0, 255.0 / 0.04, 1e6, 3.0):
        got = ops.kernels().mc_uncertainty(x.to(DEV), ("std",), u8_scale=scale)
        std, u8 = got["std"].cpu().numpy(), got["std_u8"].cpu().numpy()
        assert np.array_equal(u8, ur.quantise(std, scale))
    assert u8.max() <= 1 and ops.kernels().mc_uncertainty(x.to(DEV), (), u8_scale=1e6)["std_u8"].max().item() == 255


@pytest.mark.parametrize("shape", list(SHAPES))
def test_outputs_not_asked_for_are_not_computed_into_the_others(shape):
    """every subset of the outputs gives the bits of the full call; a null output is a pointer the kernel never touches"""
    K, xd = ops.kernels(), _case(8, shape)[0].to(DEV)
    full = K.mc_uncertainty(xd, MAPS, u8_scale=1600.0)
    for names, scale in ((("std",), None), (("mean", "std"), None), (("entropy",), None), (("mi", "mean"), 1600.0), ((), 1600.0)):
        part = K.mc_uncertainty(xd, names, u8_scale=scale)
        assert set(part) == set(names) | ({"std_u8"} if scale else set())
        for k, v in part.items():
            assert torch.equal(v, full[k]), (names, k)
    with pytest.raises(ValueError, match="outputs"):
        K.mc_uncertainty(xd, ())
    with pytest.raises(ValueError, match="outputs"):
        K.mc_uncertainty(xd, ("variance",))


@pytest.mark.parametrize("T", [2, 8, 32])
def test_chunked_evaluation_is_bit_identical(T):
    """chunks of 1000 (16-byte path), 122 and odd sizes (element-wise path) of the 96x80 case against the whole"""
    x, _, _ = _case(T, "96x80")
    K = ops.kernels()
    flat = x.reshape(T, -1).to(DEV)
    n = flat.shape[1]
    whole = K.mc_uncertainty(flat, MAPS, u8_scale=1600.0)
    start = 0
    for size in (1000, 122, 4097, 3, 1, n):
        stop = min(start + size, n)
        part = K.mc_uncertainty(flat[:, start:stop].contiguous(), MAPS, u8_scale=1600.0)
        for k, v in part.items():
            assert torch.equal(v, whole[k][start:stop]), (k, start, stop)
        start = stop
        if start == n:
            break
    assert start == n


@pytest.mark.parametrize("T", [1, 33, 0])
def test_pass_counts_outside_2_to_32_are_errors_that_write_nothing(T):
    K = ops.kernels()
    x = torch.zeros(40, 64, device=DEV)
    outs = [torch.full((64,), -7.0, device=DEV) for _ in range(4)]
    u8 = torch.full((64,), 0xA5, dtype=torch.uint8, device=DEV)
    rc = K.lib.uda_mc_uncertainty(x.data_ptr(), T, 64, *[o.data_ptr() for o in outs], u8.data_ptr(), 1600.0, _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_mc_uncertainty" in K.lib.uda_last_error()
    assert all(bool((o == -7.0).all()) for o in outs) and bool((u8 == 0xA5).all())
    rc = K.lib.uda_mc_uncertainty(x.data_ptr(), 8, 64, None, None, None, None, None, 0.0, _stream())
    assert rc != 0 and b"no output" in K.lib.uda_last_error()
    rc = K.lib.uda_mc_uncertainty(x.data_ptr(), 8, 64, None, None, None, None, u8.data_ptr(), 0.0, _stream())
    assert rc != 0 and b"u8_scale" in K.lib.uda_last_error() and bool((u8 == 0xA5).all())
    if T == 1:
        with pytest.raises(Exception, match="outside 2..32"):
            ops.mc_uncertainty(x[:1].reshape(1, 1, 2, 8, 4))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_mc_uncertainty_write_footprint(shape):
    x, want, yard = _case(8, shape)
    K, n = ops.kernels(), x[0].numel()
    with footprint():
        xd = ro_dev(x.reshape(8, n), DEV, "logits")
        outs = [out_dev((n,), torch.float32, DEV, name=k) for k in MAPS]
        u8 = out_dev((n,), torch.uint8, DEV, name="std_u8")
        rc = K.lib.uda_mc_uncertainty(xd.data_ptr(), 8, n, *[o.data_ptr() for o in outs], u8.data_ptr(), 1600.0, _stream())
        torch.cuda.synchronize()
        assert rc == 0, K.lib.uda_last_error()
    assert footprint_violations() == [], "uda_mc_uncertainty wrote outside its outputs: (buffer, first position)"
    for k, o in zip(MAPS, outs):
        assert float(np.abs(o.cpu().numpy().astype(np.float64) - want[k].reshape(-1)).max()) <= 4 * yard[k], k
    # a subset: the other three buffers keep their fill
    with footprint():
        xd = ro_dev(x.reshape(8, n), DEV, "logits")
        keep = [out_dev((n,), torch.float32, DEV, name=k) for k in ("mean", "entropy", "mi")]
        std = out_dev((n,), torch.float32, DEV, name="std")
        before = [k.clone() for k in keep]
        rc = K.lib.uda_mc_uncertainty(xd.data_ptr(), 8, n, None, std.data_ptr(), None, None, None, 0.0, _stream())
        torch.cuda.synchronize()
        assert rc == 0, K.lib.uda_last_error()
    assert footprint_violations() == [] and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(keep, before))
    assert torch.equal(std, outs[1])


# ------------------------------------------------------------------------------------------------------------------ the tables
def _maps(seed, B, H, W, planted=True):
    """prob, unc fp32 and pred, gt bool [B,2,H,W]: smooth blobs, background runs of p = 0, errors more uncertain, the edge values planted"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    gt = np.zeros((B, 2, H, W), bool)
    prob = np.zeros((B, 2, H, W), np.float32)
    for b in range(B):
        for c in range(2):
            cy, cx, r = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, (0.18 + 0.12 * c) * min(H, W)
            d = np.hypot(yy - cy, xx - cx)
            gt[b, c] = d < r
            soft = 1.0 / (1.0 + np.exp((d - r * rng.uniform(0.85, 1.15)) / 2.0)) + 0.08 * rng.standard_normal((H, W))
            prob[b, c] = np.where(d > 1.6 * r, 0.0, np.clip(soft, 0, 1))
    pred = prob > 0.5
    unc = (0.05 * rng.random((B, 2, H, W)) ** 2 * (1.0 + 4.0 * (pred != gt)) * (prob > 0)).astype(np.float32)
    if planted:
        e = np.asarray(ur.DEFAULT_EDGES, np.float32)
        nxt = lambda v, d: np.nextafter(np.float32(v), np.float32(d))
        us = [0.0, -0.0, np.inf, np.nan, -1e-9, -np.inf] + [f(v) for v in e for f in (lambda v: v, lambda v: nxt(v, 0), lambda v: nxt(v, 1))]
        ps = [0.0, -0.0, 1.0, nxt(1, 0), 1.0000001, np.nan, -1e-9, 2.0]
        for M in (15, 64):
            for k in range(1, M):
                v = np.float32(k) / np.float32(M)
                ps += [v, nxt(v, 0), nxt(v, 1)]
        unc.reshape(B, 2, -1)[:, :, 5:5 + len(us)] = np.asarray(us, np.float32)
        prob.reshape(B, 2, -1)[:, :, 40:40 + len(ps)] = np.asarray(ps, np.float32)
    return prob, unc, pred, gt


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.astype(np.uint8) if a.dtype == bool else a).to(DEV)


def _run(prob, unc, pred, gt, M=15, edges=ur.DEFAULT_EDGES):
    rel, risk, invalid = ops.kernels().selective_tables(_dev(prob), _dev(unc), _dev(pred), _dev(gt), M, edges)
    torch.cuda.synchronize()
    return {"rel": None if rel is None else rel.cpu().numpy(), "risk": None if risk is None else risk.cpu().numpy(), "invalid": invalid.cpu().numpy()}


def _check(prob, unc, pred, gt, M=15, edges=ur.DEFAULT_EDGES):
    got, want = _run(prob, unc, pred, gt, M, edges), ur.tables(prob, unc, pred, gt, M, edges)
    for name in ("rel", "risk", "invalid"):
        if want[name] is None:
            assert got[name] is None, name
            continue
        assert got[name].dtype == np.int64 and got[name].shape == want[name].shape, name
        bad = got[name] != want[name]
        assert not bad.any(), "%s differs in %d of %d entries, first at %s: %d for %d" % (
            name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[name][bad][0], want[name][bad][0])
    return got


@pytest.mark.parametrize("H,W", [(33, 17), (96, 80)], ids=["33x17", "96x80"])
def test_tables_with_the_edge_values_planted(H, W):
    """33 x 17: the element-wise walk; 96 x 80: the 16-byte walk"""
    prob, unc, pred, gt = _maps(H, 3, H, W)
    got = _check(prob, unc, pred, gt)
    assert (got["invalid"] == [4, 3]).all() and got["rel"][..., 0].sum() == 3 * 2 * (H * W - 4)
    _check(prob, unc, pred, gt, M=64)
    _check(prob, unc, pred, gt, M=1, edges=())
    _check(prob, unc, pred, gt, M=7, edges=np.linspace(0.0, 0.2, 63))


def test_tables_512():
    got = _check(*_maps(512, 2, 512, 512))
    assert (got["rel"][:, :, 0, 0] > 50000).all() and (got["risk"][..., 1:3].sum((-1, -2)) > 0).all()      # background run; errors present


def test_one_bin_1024_has_the_largest_sums():
    """every p = 1.0, every u = 0: one confidence bin and one uncertainty bin take all 2^20 pixels of a plane"""
    one = np.ones((1, 2, 1024, 1024), np.float32)
    pred = np.ones((1, 2, 1024, 1024), bool)
    gt = pred.copy()
    gt[0, 1, :512] = False
    got = _check(one, np.zeros_like(one), pred, gt)
    assert got["rel"][0, 0, 14].tolist() == [2 ** 20, 2 ** 20, 2 ** 36, 2 ** 36, 2 ** 52] and got["rel"][0, :, :14].sum() == 0
    assert got["risk"][0, 1, 0].tolist() == [2 ** 19, 2 ** 19, 0, 0] and got["rel"][0, 1, 14, 3] == 2 ** 35


def test_empty_masks_and_absent_inputs():
    prob, unc, pred, gt = _maps(9, 2, 96, 80)
    none = np.zeros_like(pred)
    got = _check(prob, unc, none, none)
    assert (got["risk"][..., :3] == 0).all() and (got["rel"][..., 1] == 0).all() and (got["rel"][..., 3] == 0).all()
    got = _check(prob, unc, pred, None)                                        # gt = pred: nothing is wrong
    assert (got["risk"][..., 1:3] == 0).all() and (got["risk"][..., 0].sum(-1) > 0).all()
    got = _check(None, unc, pred, gt)
    assert got["rel"] is None and (got["invalid"][..., 0] == 0).all() and (got["invalid"][..., 1] == 3).all()
    got = _check(prob, None, pred, gt)
    assert got["risk"] is None and (got["invalid"][..., 1] == 0).all() and (got["invalid"][..., 0] == 4).all()
    _check(prob[:, :, :33, :17], unc[:, :, :33, :17], pred[:, :, :33, :17], None)


def test_deterministic_and_independent_of_the_batch():
    prob, unc, pred, gt = _maps(21, 4, 96, 80)
    K = ops.kernels()
    p, u, a, g = _dev(prob), _dev(unc), _dev(pred), _dev(gt)
    first = K.selective_tables(p, u, a, g, 15, ur.DEFAULT_EDGES, want_packed=True)[-1]
    assert torch.equal(first, K.selective_tables(p, u, a, g, 15, ur.DEFAULT_EDGES, want_packed=True)[-1])
    whole = K.selective_tables(p, u, a, g, 15, ur.DEFAULT_EDGES)
    flip = lambda t: torch.flip(t, [0]).contiguous()
    back = K.selective_tables(flip(p), flip(u), flip(a), flip(g), 15, ur.DEFAULT_EDGES)
    for i in range(4):
        alone = K.selective_tables(*(t[i:i + 1].contiguous() for t in (p, u, a, g)), 15, ur.DEFAULT_EDGES)
        pair = K.selective_tables(*(t[[i, (i + 2) % 4]].contiguous() for t in (p, u, a, g)), 15, ur.DEFAULT_EDGES)
        for w, o, r, q in zip(whole, alone, back, pair):
            assert torch.equal(w[i], o[0]) and torch.equal(w[i], r[3 - i]) and torch.equal(w[i], q[0]), i


def test_front_end_takes_the_mask_types_of_disc_morphometry():
    prob, unc, pred, gt = _maps(6, 2, 96, 80, planted=False)
    want = ur.tables(prob, unc, pred, gt)
    pt, ut = torch.from_numpy(prob), torch.from_numpy(unc)
    u8 = torch.from_numpy(pred.astype(np.uint8) * 255)
    for m in (u8, u8.to(DEV), torch.from_numpy(pred), torch.from_numpy(pred).to(DEV), torch.from_numpy(pred.astype(np.float32)).to(DEV),
              torch.from_numpy(pred.astype(np.float64) * 0.9)):
        got = ops.selective_tables(pt, ut.to(DEV), m, torch.from_numpy(gt))
        assert set(got) == {"rel", "risk", "invalid", "edges"} and got["edges"].dtype == np.float32
        for name in ("rel", "risk", "invalid"):
            assert isinstance(got[name], np.ndarray) and got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), name
    got = ops.selective_tables(None, ut, u8, None, edges=(0.04,))
    assert got["rel"] is None and np.array_equal(got["risk"], ur.tables(None, unc, pred, None, edges=(0.04,))["risk"])
    maps = ops.mc_uncertainty(ur.mc_logits(4, 2, 96, 80, 1))                   # a host tensor is moved; [B,2,H,W] maps come back
    assert set(maps) == set(MAPS) and all(v.shape == (2, 2, 96, 80) and v.is_cuda for v in maps.values())


@pytest.mark.parametrize("case", ["M=65", "M=0", "K=65", "unsorted edges", "equal edges", "NaN edge", "H=1025", "no table", "rel without prob",
                                  "risk without unc"])
def test_bad_arguments_return_an_error_and_write_nothing(case):
    """(the entry takes no workspace: there is no short one to refuse)"""
    import ctypes as C
    K = ops.kernels()
    B, H, W, M = 1, 64, 48, 15
    prob = torch.full((B, 2, 1025, W), 0.5, device=DEV)
    unc = torch.full((B, 2, 1025, W), 0.01, device=DEV)
    masks = torch.ones(B, 2, 1025, W, dtype=torch.uint8, device=DEV)
    outs = [torch.full(shape, -77, dtype=torch.int64, device=DEV) for shape in ((B, 2, 65, 5), (B, 2, 65, 4), (B, 2, 2))]
    edges = list(ur.DEFAULT_EDGES)
    args = dict(prob=prob.data_ptr(), unc=unc.data_ptr(), gt=masks.data_ptr(), H=H, M=M, K=10, rel=outs[0].data_ptr(), risk=outs[1].data_ptr())
    if case == "M=65":
        args["M"] = 65
    elif case == "M=0":
        args["M"] = 0
    elif case == "K=65":
        edges, args["K"] = list(np.linspace(0.0, 1.0, 64)), 65
    elif case == "unsorted edges":
        edges[3], edges[4] = edges[4], edges[3]
    elif case == "equal edges":
        edges[4] = edges[3]
    elif case == "NaN edge":
        edges[-1] = float("nan")
    elif case == "H=1025":
        args["H"] = 1025
    elif case == "no table":
        args["rel"] = args["risk"] = None
    elif case == "rel without prob":
        args["prob"] = None
    else:
        args["unc"] = None
    rc = K.lib.uda_selective_tables(args["prob"], args["unc"], masks.data_ptr(), args["gt"], B, args["H"], W, args["M"],
                                    (C.c_float * len(edges))(*edges), args["K"], args["rel"], args["risk"], outs[2].data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_selective_tables" in K.lib.uda_last_error()
    assert all(bool((o == -77).all()) for o in outs) and bool((masks == 1).all()) and bool((prob == 0.5).all()) and bool((unc == 0.01).all())
    with pytest.raises(ValueError, match="1..64 bins"):
        K.selective_tables(prob[:, :, :H].contiguous(), None, masks[:, :, :H].contiguous(), None, 65, ())


@pytest.mark.parametrize("H,W", [(33, 17), (96, 80)], ids=["bytes", "words"])
def test_selective_tables_write_footprint(H, W):
    import ctypes as C
    prob, unc, pred, gt = _maps(3, 2, H, W)
    want = ur.tables(prob, unc, pred, gt)
    K, B, edges = ops.kernels(), 2, list(ur.DEFAULT_EDGES)
    with footprint():
        ins = [ro_dev(torch.from_numpy(a), DEV, name) for a, name in ((prob, "prob"), (unc, "unc"), (pred.astype(np.uint8), "pred"), (gt.astype(np.uint8), "gt"))]
        outs = [out_dev(shape, torch.int64, DEV, name=name) for name, shape in (("rel", (B, 2, 15, 5)), ("risk", (B, 2, 10, 4)), ("invalid", (B, 2, 2)))]
        rc = K.lib.uda_selective_tables(*[t.data_ptr() for t in ins], B, H, W, 15, (C.c_float * 9)(*edges), 10, *[o.data_ptr() for o in outs], _stream())
        torch.cuda.synchronize()
        assert rc == 0, K.lib.uda_last_error()
    assert footprint_violations() == [], "uda_selective_tables wrote outside its outputs: (buffer, first position)"
    for name, o in zip(("rel", "risk", "invalid"), outs):
        assert np.array_equal(o.cpu().numpy(), want[name]), name
    with footprint():                                                          # the risk table alone: rel is a pointer never touched
        ins = [ro_dev(torch.from_numpy(a), DEV, name) for a, name in ((unc, "unc"), (pred.astype(np.uint8), "pred"))]
        risk, invalid = out_dev((B, 2, 10, 4), torch.int64, DEV, name="risk"), out_dev((B, 2, 2), torch.int64, DEV, name="invalid")
        rc = K.lib.uda_selective_tables(None, ins[0].data_ptr(), ins[1].data_ptr(), None, B, H, W, 0, (C.c_float * 9)(*edges), 10, None,
                                        risk.data_ptr(), invalid.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert rc == 0, K.lib.uda_last_error()
    assert footprint_violations() == [] and np.array_equal(risk.cpu().numpy(), ur.tables(None, unc, pred, None)["risk"])


# ------------------------------------------------------------------------------------------------------ mc_inference_logits
@pytest.mark.parametrize("sync_bn", [True, False], ids=["batchnorm", "transnorm"])
def test_mc_inference_logits_leaves_the_model_as_found(sync_bn):
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    torch.manual_seed(3)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16, sync_bn=sync_bn).to(DEV)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(4)).to(DEV)
    g = torch.Generator().manual_seed(5)
    for name, buf in model.named_buffers():                                    # running statistics that are not the initial ones
        if "running_mean" in name:
            buf.add_(0.05 * torch.randn(buf.shape, generator=g).to(DEV))
        elif "running_var" in name:
            buf.mul_(1.0 + 0.2 * torch.rand(buf.shape, generator=g).to(DEV))
    model.eval()
    with torch.no_grad():
        before = model(x)[0].clone()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    flags = [m.training for m in model.modules()]
    model.set_dropout_seed(77)
    offset = model._engine.rng_offset
    a = model.mc_inference_logits(x, 4)
    assert a.shape == (4, 2, 2, 64, 64) and a.dtype == torch.float32 and not a.requires_grad and bool(torch.isfinite(a).all())
    assert all(not torch.equal(a[i], a[j]) for i in range(4) for j in range(i))           # dropout is live: the passes differ
    assert [m.training for m in model.modules()] == flags
    now = model.state_dict()
    assert set(now) == set(state) and all(torch.equal(now[k], state[k]) for k in state)    # num_batches_tracked included
    with torch.no_grad():
        assert torch.equal(model(x)[0], before)
    model.set_dropout_seed(77)
    assert torch.equal(model.mc_inference_logits(x, 4), a)
    model.set_dropout_seed(78)
    assert not torch.equal(model.mc_inference_logits(x, 4), a)
    model.train()                                                              # found in training mode: left in training mode
    flags = [m.training for m in model.modules()]
    model.mc_inference_logits(x, 2)
    now = model.state_dict()
    assert [m.training for m in model.modules()] == flags and all(torch.equal(now[k], state[k]) for k in state)
    maps = ops.mc_uncertainty(a)
    assert all(v.shape == (2, 2, 64, 64) for v in maps.values()) and float(maps["std"].max()) > 0
    # what it is defined as: freeze_bn() under train(), then mc_dropout_logits(x, passes, reps=1), from the same place of the dropout stream
    model.freeze_bn()
    model.set_dropout_seed(77)
    model._engine.rng_offset = offset
    assert torch.equal(model.mc_dropout_logits(x, 4, reps=1).view_as(a), a)


# ------------------------------------------------------------------------------------------------ evaluate and predict on the device
def _brightness_model(image):
    """stand-in generator for the drawn images of dataloaders.synthetic: disc and cup by brightness, soft enough to fill the bins"""
    grey = (image.mean(1) + 1.0) * 127.5
    return torch.stack([(grey - 165.0), (grey - 110.0)], 1) / 8.0, None


@pytest.fixture
def recorded(monkeypatch):
    """ops.mc_uncertainty and ops.selective_tables as they are, with the maps of every call kept"""
    calls = {"unc": [], "tables": []}
    real_u, real_t = ops.mc_uncertainty, ops.selective_tables

    def unc(logits, outputs=MAPS, u8_scale=None):
        out = real_u(logits, outputs, u8_scale)
        calls["unc"].append((logits.detach().cpu().numpy(), {k: v.cpu().numpy() for k, v in out.items()}, u8_scale))
        return out

    def tables(prob, unc_map, pred, gt=None, bins=15, edges=ops.DEFAULT_UNC_EDGES):
        n = lambda t: None if t is None else t.detach().cpu().numpy()
        calls["tables"].append(dict(prob=n(prob), unc=n(unc_map), pred=n(pred) != 0, gt=None if gt is None else n(gt) != 0, bins=bins, edges=tuple(edges)))
        return real_t(prob, unc_map, pred, gt, bins, edges)
    monkeypatch.setattr(ops, "mc_uncertainty", unc)
    monkeypatch.setattr(ops, "selective_tables", tables)
    return calls


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _close(a, b):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= 4 * np.spacing(abs(b))          # 4 ulp


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def test_evaluate_with_calibration_and_mc_passes_on_synthetic_data(tmp_path, recorded, capsys):
    synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=128)
    argv = ["--data-dir", str(tmp_path), "--dataset", "Drishti-GS", "--checkpoint", "unused", "--batch-size", "2"]
    passes = ur.noisy_passes()
    plain = ev.main(argv, model=_brightness_model)
    assert recorded == {"unc": [], "tables": []} and set(plain) == {"per_image", "mean", "n_images", "n_undefined"}
    assert all(set(r) == {"img_name"} | set(ev.FIELDS) for r in plain["per_image"])      # without the flags: no call, the result of before
    out = tmp_path / "pictures"
    res = ev.main(argv + ["--calibration", "--mc-passes", "4", "--save-dir", str(out), "--csv", str(tmp_path / "u.csv"), "--json", str(tmp_path / "u.json")],
                  model=_brightness_model, mc_logits=passes)
    assert "cup_cov_0.04" in capsys.readouterr().out
    names = ev.CALIBRATION_FIELDS + ev.uncertainty_fields()
    assert res["extra_fields"] == names and [c[0].shape for c in recorded["unc"]] == [(4, 2, 2, 128, 128), (4, 1, 2, 128, 128)]
    assert len(recorded["tables"]) == 2 and all(c[2] == 1600.0 and set(c[1]) == {"std", "std_u8"} for c in recorded["unc"])
    i, pooled_rel, pooled_risk = 0, 0, 0
    for (logits, maps, _), call in zip(recorded["unc"], recorded["tables"]):
        assert np.array_equal(maps["std_u8"], ur.quantise(maps["std"], 1600.0))
        assert np.array_equal(call["unc"], maps["std"]) and call["bins"] == 15 and call["edges"] == ops.DEFAULT_UNC_EDGES
        t = ur.tables(call["prob"], call["unc"], call["pred"], call["gt"], 15, call["edges"])
        pooled_rel, pooled_risk = pooled_rel + t["rel"].sum(0), pooled_risk + t["risk"].sum(0)
        for j in range(call["pred"].shape[0]):
            r, p = res["per_image"][i], plain["per_image"][i]
            assert all(_same(r[k], p[k]) for k in p)
            stem = r["img_name"].split(".")[0]
            png = _png(out / "uncertainty" / (stem + ".png"))
            assert png.shape == (128, 128, 3) and not png[..., 0].any()
            assert np.array_equal(png[..., 1], maps["std_u8"][j, 1]) and np.array_equal(png[..., 2], maps["std_u8"][j, 0])
            for k, c in enumerate(("cup", "disc")):
                d = ur.direct_calibration(call["prob"][j, k], call["gt"][j, k], 15)
                assert _close(r[c + "_ece"], d["ece"]) and _close(r[c + "_brier"], d["brier"])
                d = ur.direct_selective(call["unc"][j, k], call["pred"][j, k], call["gt"][j, k], (0.04,))
                assert _same(r[c + "_cov_0.04"], d["coverage"][0]) and _same(r[c + "_dice_0.04"], d["dice"][0]) and _same(r[c + "_err_0.04"], d["error"][0])
                bins = (np.asarray(call["edges"], np.float32)[None] <= call["unc"][j, k].reshape(-1, 1)).sum(1)
                wrong = (call["pred"][j, k] != call["gt"][j, k]).ravel()
                assert _close(r[c + "_unc_auroc"], ur.brute_auroc(bins[wrong], bins[~wrong]))
            assert 0 < r["disc_cov_0.04"] < 1                                    # the stand-in's noise does spread over the threshold
            i += 1
    assert i == 3 and res["calibration"]["rel"] == pooled_rel.tolist() and res["risk_coverage"]["risk"] == pooled_risk.tolist()
    s = metrics.selective_from_table(pooled_risk, ops.DEFAULT_UNC_EDGES)
    assert res["risk_coverage"]["aurc"] == s["aurc"].tolist() and all(_close(a, ur.direct_aurc(pooled_risk[k])) for k, a in enumerate(s["aurc"]))
    rows = list(csv.reader(open(tmp_path / "u.csv")))
    assert rows[0] == ["img_name"] + list(ev.FIELDS + names) and len(rows) == 4
    for row, r in zip(rows[1:], res["per_image"]):
        assert all(_same(float(v), r[k]) for k, v in zip(rows[0][1:], row[1:]))
    import json
    back = json.load(open(tmp_path / "u.json"))
    assert back["calibration"]["rel"] == pooled_rel.tolist() and back["risk_coverage"]["risk"] == pooled_risk.tolist()


def test_predict_with_mc_passes_on_synthetic_data(tmp_path, recorded):
    split = synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=128)
    images = split + "/ROIs/image"
    plain = predict.main(["--images", images, "--out", str(tmp_path / "a"), "--csv", str(tmp_path / "a.csv"), "--batch-size", "2"], model=_brightness_model)
    assert recorded == {"unc": [], "tables": []} and all(set(r) == {"img_name", "vcdr_pred"} for r in plain)
    assert list(csv.reader(open(tmp_path / "a.csv")))[0] == ["img_name", "vcdr_pred"] and not (tmp_path / "a" / "uncertainty").exists()
    rows = predict.main(["--images", images, "--out", str(tmp_path / "b"), "--csv", str(tmp_path / "b.csv"), "--batch-size", "2", "--mc-passes", "4"],
                        model=_brightness_model, mc_logits=ur.noisy_passes())
    assert [c[0].shape for c in recorded["unc"]] == [(4, 2, 2, 128, 128), (4, 1, 2, 128, 128)] and len(recorded["tables"]) == 2
    i = 0
    for (logits, maps, scale), call in zip(recorded["unc"], recorded["tables"]):
        assert scale == 1600.0 and call["prob"] is None and call["gt"] is None and np.array_equal(call["unc"], maps["std"])
        unsure = (call["unc"] >= np.float32(0.04)) & call["pred"]
        for j in range(call["pred"].shape[0]):
            r, p = rows[i], plain[i]
            assert r["img_name"] == p["img_name"] and _same(r["vcdr_pred"], p["vcdr_pred"]) and set(r) == set(p) | set(predict.UNCERTAINTY_COLUMNS)
            for k, c in enumerate(("cup", "disc")):
                n = int(call["pred"][j, k].sum())
                assert _same(r[c + "_unsure"], int(unsure[j, k].sum()) / n if n else math.nan)
            assert r["unsure_px"] == unsure[j].sum() and 0 < r["disc_unsure"] < 1
            png = _png(tmp_path / "b" / "uncertainty" / (r["img_name"].split(".")[0] + ".png"))
            assert not png[..., 0].any() and np.array_equal(png[..., 1], maps["std_u8"][j, 1]) and np.array_equal(png[..., 2], maps["std_u8"][j, 0])
            i += 1
    back = list(csv.reader(open(tmp_path / "b.csv")))
    assert back[0] == ["img_name", "vcdr_pred"] + list(predict.UNCERTAINTY_COLUMNS) and len(back) == 4
    for row, r in zip(back[1:], rows):
        assert row[0] == r["img_name"] and all(_same(float(v), r[k]) for k, v in zip(back[0][1:], row[1:]))
