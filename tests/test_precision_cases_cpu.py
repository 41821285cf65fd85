"""not-gpu: the bf16x3 pack cases and the one-product probes (kernel_cases.X3_PACK_CASES / PROBE_CASES) can pass and can fail.

  * The statement of the split (SpecKernels.x3_split) is exact on the pack cases' value table: a1 + a2 + a3 == x in float64
    wherever x is a multiple of 2^-133 (bf16's smallest subnormal), and within 2^-134 below that - the split of such a value
    cannot be exact, bf16 has no bit for it.
  * With SpecKernels standing in for HipKernels every pack case and every probe passes on the CPU (the probes' float64 gather
    agrees with the statement's fp32 conv within the fp32 bound 2 U24).
  * X3Emu emulates the bf16x3 kernels: both operands split with x3_split, the chosen piece products formed in fp32 (exact) and
    summed in fp32 in the kernels' order.  With all six terms it passes every probe of a bf16x3 route; each planted fault fails
    exactly the probes listed with it.

Why this file exists: every one of these faults PASSES the existing dense cases.  On "conv3x3 256->256 relu mask" (2e-5) and
"wgrad3x3 256->256 P=4608 mask (x3 128 tiles)" (3e-5) the emulation measures, with the cases' own metric max|a - b| / max|b|
(test_every_fault_passes_the_existing_dense_cases asserts it):

    variant                               conv        wgrad       the probes that must fail, in U24 = 2^-24 |x w| (bound 8)
    six terms (intact)                    1.2e-06     8.2e-07     1.4 - 1.8  (passes; an MI355X measures 2.2 - 2.7)
    a1 b3 dropped                         3.0e-06     2.5e-06     110 - 129
    a2 b2 dropped                         2.8e-06     3.3e-06     228 - 251
    three terms only                      4.4e-06     4.4e-06     380 - 465
    a3 zero in a row's last 16-block      1.5e-06     1.6e-06     125 - 129
    a3 taken from lane k ^ 1              3.5e-06     3.0e-06     > 3500
    wgrad: third piece of dy dropped      -           2.5e-06     115 - 126
    tail route alone without a1 b3        (no tail route)         121 - 129

(The emulation forms each piece product with an fp32 conv and adds six of them, so its intact figure sits above the 5.8e-9 of a
float64-accumulating emulation; the point is the column's spread: every fault stays at least four times below 2e-5 / 3e-5.)"""
import pytest
import torch
import torch.nn.functional as F

import kernel_cases as kc
from kernel_spec import SpecKernels, _nchw, _rows, transform

CPU = torch.device("cpu")
_BY_NAME = dict(kc.CASES)
PACKS = [c[0] for c in kc.X3_PACK_CASES]
PROBES = [c[0] for c in kc.PROBE_CASES]
X3_PROBES = [n for n, fn in kc.PROBE_CASES if kc._is_x3(kc._declared(fn.route, 1))]
BIG_PACK = [n for n in PACKS if "grid-stride" in n]


def _run(name, impl, monkeypatch):
    monkeypatch.setattr(kc, "_HIP", impl)
    err, tol = _BY_NAME[name](CPU)
    assert kc.footprint_violations() == []
    return err, tol


# ---- the statement
def test_the_split_is_exact_on_the_value_table():
    x = kc.x3_value_table()
    assert x.numel() > 1100 and x.numel() % 2 == 1
    bits = x.view(torch.int32)
    expo = (bits >> 23) & 0xFF
    assert set(range(1, 254)) <= set(expo.tolist()) and 0 in expo.tolist()                       # every exponent, subnormals
    assert bool((bits == 0).any()) and bool((bits == -2 ** 31).any())                            # +-0
    assert x.abs().max().view(torch.int32).item() == 0x7F7F7FFF
    a1, a2, a3 = SpecKernels().x3_split(x)
    s = a1.double() + a2.double() + a3.double()
    on_grid = (x.double() * 2.0 ** 133) == torch.round(x.double() * 2.0 ** 133)
    assert int(on_grid.sum()) > 900 and int((~on_grid).sum()) > 50
    assert bool((s[on_grid] == x.double()[on_grid]).all())
    assert bool(((s - x.double()).abs()[~on_grid] <= 2.0 ** -134).all())
    assert bool((x[expo >= 17].double() == s[expo >= 17]).all())                                 # |x| >= 2^-110: always exact
    r2 = x.double() - a1.double() - a2.double()
    assert bool(((r2 < 0) & (x > 0)).any()) and bool(((x.double() - a1.double() < 0) & (x > 0)).any())      # negative residuals
    # the piece bounds the probes' tolerance rests on (bf16 keeps 8 significant bits, round to nearest): |a2| <= 2^-8 |a|, |a3| <= 2^-16 |a|
    big = expo >= 40
    assert bool((a2.double().abs()[big] <= 2.0 ** -8 * x.double().abs()[big]).all())
    assert bool((a3.double().abs()[big] <= 2.0 ** -16 * x.double().abs()[big]).all())


def test_the_packed_layout_is_the_stated_one():
    """element (row, k, piece q) at ((row * nb + k // 16) * 3 + q) * 16 + k % 16; zero pieces behind K; 64 unwritten bytes"""
    S = SpecKernels()
    x = torch.arange(1, 3 * 40 + 1, dtype=torch.float32).reshape(3, 40) * 1.0009765625
    out = torch.full((3 * 3 * 96 + 64,), 0xA5, dtype=torch.uint8)
    assert S.x3_pack(kc.Act(x, 1, 1, 3), 3, 40, out=out) is out
    assert bool((out[-64:] == 0xA5).all())
    flat = out[:-64].view(torch.bfloat16)
    pieces = S.x3_split(x)
    for row, k, q in ((0, 0, 0), (2, 39, 2), (1, 16, 1), (1, 15, 2), (2, 31, 0)):
        assert flat[((row * 3 + k // 16) * 3 + q) * 16 + k % 16] == pieces[q][row, k]
    assert bool((flat.reshape(3, 3, 3, 16)[:, 2, :, 8:].view(torch.int16) == 0).all())


@pytest.mark.parametrize("name", PACKS)
def test_spec_kernels_pass_the_pack_case_on_the_cpu(name, monkeypatch):
    err, tol = _run(name, kc.SPEC, monkeypatch)
    assert err == 0.0 and tol == 0.0


class PackLosesThePieceOfTheLastLane(SpecKernels):
    """a pack whose third piece is zero in lane 15 of every block"""
    def x3_split(self, x):
        a1, a2, a3 = super().x3_split(x)
        a3 = a3.clone()
        a3.reshape(-1)[15::16] = 0
        return a1, a2, a3


@pytest.mark.parametrize("name", [n for n in PACKS if n not in BIG_PACK])
def test_a_pack_that_loses_one_lane_of_the_third_piece_fails_the_pack_case(name, monkeypatch):
    assert type(kc.SPEC) is SpecKernels                      # (the cases compare with the statement, not with the stand-in)
    err, _ = _run(name, PackLosesThePieceOfTheLastLane(), monkeypatch)
    assert err > 0, name


# ---- the emulated kernel
SIX = ((3, 1), (2, 2), (1, 3), (2, 1), (1, 2), (1, 1))       # (activation piece, piece of the weight / of dy), the kernels' add order


def _without(*drop):
    return tuple(t for t in SIX if t not in drop)


class X3Emu(SpecKernels):
    """conv / conv_wgrad as the bf16x3 kernels compute them: x3_split of both operands, the piece products of ``terms`` as fp32
    matrix products (every product of two bf16 pieces is exact in fp32), summed in fp32 in the order of ``terms``.  A call whose
    declared route (kernel_cases.DETAIL["route"], set by the probes) is not a bf16x3 one runs the fp32 statement, as the library
    does.  Where every weight row (every column of dy) holds at most one nonzero the matrix product is formed as the elementwise
    product it degenerates to - the other addends are exact zeros, the result is the same bit for bit
    (test_the_sparse_form_of_the_emulation_equals_its_matrix_form)."""
    mfma = 1

    def __init__(self, terms=SIX, tail_terms=None, wgrad_terms=None, a3_last_block_zero=False, a3_lane_swap=False, sparse=True):
        self.terms, self.tail_terms, self.wgrad_terms = terms, tail_terms or terms, wgrad_terms or terms
        self.a3_last_block_zero, self.a3_lane_swap, self.sparse = a3_last_block_zero, a3_lane_swap, sparse

    def _act_pieces(self, src):
        """the packed activation operand as the (possibly faulty) pack leaves it: three fp32 [P, C] matrices"""
        u = transform(src).contiguous()
        a = [p.float() for p in self.x3_split(u)]
        Cc = u.shape[1]
        if self.a3_last_block_zero:
            a[2][:, (Cc - 1) // 16 * 16:] = 0
        if self.a3_lane_swap:
            a[2] = a[2][:, (torch.arange(Cc) ^ 1).clamp(max=Cc - 1)]
        return a

    def _x3_route(self):
        r = kc.DETAIL.get("route")
        return r is None or kc._is_x3(r)

    def conv(self, src, w, ksize, dil, out, bias=None, addend=None, stats=None, origin=0, stride=1):
        if not self._x3_route():
            return super().conv(src, w, ksize, dil, out, bias, addend, stats, origin, stride)
        terms = self.tail_terms if "x3+tail" in (kc.DETAIL.get("route") or "") else self.terms
        Cin, Cout, T = src.C, out.shape[1], ksize * ksize
        A = [self._pad_taps(_nchw(a, src.N, src.H, src.W), ksize, dil, origin) for a in self._act_pieces(src)]
        w3 = self._taps_channels(w, T, Cin).contiguous()                                         # [Cout, T, Cin]
        B = [p.float() for p in self.x3_split(w3)]
        d = dil if ksize == 3 else 1
        nz = w3 != 0
        y = None
        if self.sparse and int(nz.reshape(Cout, -1).sum(1).max()) <= 1:
            t_o, c_o = nz.reshape(Cout, -1).float().argmax(1) // Cin, nz.reshape(Cout, -1).float().argmax(1) % Cin
            Ho, Wo = (src.H - 1) // stride + 1, (src.W - 1) // stride + 1
            cols = {}
            for t in set(t_o.tolist()):
                kh, kw = divmod(t, ksize)
                sel = (t_o == t).nonzero().reshape(-1)
                cols[t] = (sel, [a[:, c_o[sel], kh * d:kh * d + (Ho - 1) * stride + 1:stride, kw * d:kw * d + (Wo - 1) * stride + 1:stride] for a in A])
            for i, j in terms:
                part = torch.zeros(src.N, Cout, Ho, Wo)
                for t, (sel, views) in cols.items():
                    part[:, sel] = views[i - 1] * B[j - 1][sel, t, c_o[sel]].reshape(1, -1, 1, 1)
                y = part if y is None else y + part
        else:
            for i, j in terms:
                part = F.conv2d(A[i - 1], B[j - 1].reshape(Cout, ksize, ksize, Cin).permute(0, 3, 1, 2), None, stride, 0, d)
                y = part if y is None else y + part
        y = _rows(y)
        if bias is not None:
            y = y + bias
        if stats is not None:
            stats[0, 0] += y.double().sum(0)
            stats[0, 1] += (y.double() ** 2).sum(0)
        if addend is not None:
            y = y + addend
        out.copy_(y)

    def conv_wgrad(self, src, dy, ksize, dil, dw, origin=0, stride=1):
        if not self._x3_route():
            return super().conv_wgrad(src, dy, ksize, dil, dw, origin, stride)
        Cout, Cin = dy.shape[1], src.C
        Ho, Wo = (src.H - 1) // stride + 1, (src.W - 1) // stride + 1
        A = [self._pad_taps(_nchw(a, src.N, src.H, src.W), ksize, dil, origin) for a in self._act_pieces(src)]
        dyc = dy.contiguous()
        D = [p.float() for p in self.x3_split(dyc)]
        d = dil if ksize == 3 else 1
        nz = dyc != 0
        res = None
        if self.sparse and int(nz.sum(0).max()) <= 1:
            pi = nz.float().argmax(0)
            n_, oh, ow = pi // (Ho * Wo), pi // Wo % Ho, pi % Wo
            o = torch.arange(Cout)
            for i, j in self.wgrad_terms:
                part = torch.empty(Cout, Cin, ksize, ksize)
                for t in range(ksize * ksize):
                    kh, kw = divmod(t, ksize)
                    part[:, :, kh, kw] = A[i - 1][n_, :, oh * stride + kh * d, ow * stride + kw * d] * D[j - 1][pi, o].unsqueeze(1)
                res = part if res is None else res + part
        else:
            for i, j in self.wgrad_terms:
                part = torch.nn.grad.conv2d_weight(A[i - 1], dw.shape, _nchw(D[j - 1], src.N, Ho, Wo), stride, 0, d)
                res = part if res is None else res + part
        dw.copy_(res)


def test_the_sparse_form_of_the_emulation_equals_its_matrix_form(monkeypatch):
    """the two forms agree wherever the output is a product (the matrix form may write -0.0 where the sparse form writes 0.0)"""
    for name in ("conv probe 3x3 40->256 2x16x16 (ragged 16-block: Cin % 16 = 8)", "conv probe 1x1 96->24 (low)"):
        fn = _BY_NAME[name]
        errs = []
        for sparse in (True, False):
            monkeypatch.setattr(kc, "_HIP", X3Emu(sparse=sparse))
            kc.DETAIL.clear()
            errs.append(fn(CPU)[0])
        assert errs[0] == errs[1] and 0 < errs[0] <= 8 * kc.U24, (name, errs)


FAULTS = {
    "a1 b3 dropped": (dict(terms=_without((1, 3))), lambda n: True),
    "a2 b2 dropped": (dict(terms=_without((2, 2))), lambda n: True),
    "three terms only": (dict(terms=((2, 1), (1, 2), (1, 1))), lambda n: True),
    "the activations' third piece zero in the last 16-block of a row": (dict(a3_last_block_zero=True), lambda n: True),
    "the activations' third piece taken from lane k ^ 1": (dict(a3_lane_swap=True), lambda n: True),
    "the weight gradient's third piece of dy dropped": (dict(wgrad_terms=_without((1, 3))), lambda n: n.startswith("wgrad")),
    "the tail-split route alone without a1 b3": (dict(tail_terms=_without((1, 3))), lambda n: "x3+tail" in kc._declared(_BY_NAME[n].route, 1)),
}


def test_the_probe_list_covers_the_routes():
    assert len(PROBES) == len(set(PROBES)) == 28 and len(X3_PROBES) == 20
    routes = {" ".join(kc._declared(_BY_NAME[n].route, 1).split()[:3]) for n in X3_PROBES}
    assert routes >= {"x3 128x128 k3", "x3 128x128 k1", "x3 128x256 k1", "x3 256x128 k3", "x3 256x256 k3", "x3 256x64 k3",
                      "x3+tail 128x128 k3", "x3+tail 128x128 k1", "x3+tail 256x128 k3", "x3+tail 128x256 k3", "x3+tail 256x256 k3",
                      "wgrad-x3 128x256 S=24", "wgrad-x3 256x256 S=64", "wgrad-x3 128x128 S=32"}, routes
    assert {kc._declared(_BY_NAME[n].route, 0).split()[0] for n in PROBES} == {"ws", "low", "narrow", "few", "stream", "heads", "cout1", "wgrad-ws"}
    assert sum(1 for n in X3_PROBES if FAULTS["the tail-split route alone without a1 b3"][1](n)) == 7
    assert kc.X3_PACK_BIG_P * 128 * 2 > 65536 * 256                    # uda_x3_pack: tot = P * nb * 2 against its grid cap


@pytest.mark.parametrize("name", PROBES)
def test_probe_passes_on_the_statement_and_fails_on_exactly_its_faults(name, monkeypatch):
    err, tol = _run(name, kc.SPEC, monkeypatch)
    assert err <= 2 * kc.U24 and tol == 2 * kc.U24                                    # float64 gather against the fp32 statement
    assert kc.DETAIL["worst"] is not None and float(kc.DETAIL["units"]) <= 2
    if name not in X3_PROBES:
        return
    err, tol = _run(name, X3Emu(), monkeypatch)
    assert tol == 8 * kc.U24 and 0 < err <= tol, (err / kc.U24, kc.DETAIL)
    for fault, (kw, mine) in FAULTS.items():
        err, tol = _run(name, X3Emu(**kw), monkeypatch)
        assert (not err <= tol) == bool(mine(name)), (fault, err / kc.U24, kc.DETAIL)
        if mine(name):
            assert err > 4 * tol, (fault, err / kc.U24)                              # an order of magnitude, not a near miss


# ---- the existing dense cases do not see any of this
DENSE = {"conv": ("conv3x3 256->256 relu mask", 2e-5), "wgrad": ("wgrad3x3 256->256 P=4608 mask (x3 128 tiles)", 3e-5)}


class _EmuWithRoutes(X3Emu):
    """the dense cases ask for the planned route before the call; the emulation plans nothing (the check is switched off below)"""
    conv_route = wgrad_route = lambda self, *a, **kw: None


def test_every_fault_passes_the_existing_dense_cases(monkeypatch):
    """the dense cases' metric for the intact emulation and for every fault: all far below the cases' tolerances"""
    seen = {}
    monkeypatch.setattr(kc, "_check_route", lambda *a: None)          # (the emulation plans nothing)
    for kind, (name, tol) in DENSE.items():
        for fault, (kw, _) in [("intact", ({}, None))] + list(FAULTS.items()):
            if (kind == "conv" and "wgrad_terms" in kw) or "tail_terms" in kw:          # (not a tail route; dy's pieces: wgrad only)
                continue
            kc.DETAIL.clear()
            err, t = _run(name, _EmuWithRoutes(**kw), monkeypatch)
            assert t == tol and err < tol / 4, (name, fault, err)
            seen[(kind, fault)] = err
    print({k: "%.1e" % v for k, v in seen.items()})
    assert seen[("conv", "three terms only")] > 2 * seen[("conv", "intact")]          # (the faults are there: the metric moves, a little)
