"""Per-kernel parity cases: HIP kernel (through the C ABI) vs. the fp32 torch statement in
tests/kernel_spec.py, on seeded inputs.  ``CASES`` is a list of (name, fn); fn(dev) returns the
worst relative error (max |a-b| / max |b|) over the outputs of that case and the tolerance.
Used by tests/test_kernels_gpu.py (asserting) and tests/gpu_report.py (printing everything)."""
from __future__ import annotations

import functools
import math
import os
import re

import torch

from kernel_spec import SpecKernels
from uda_clr_amd.acts import ACT_NONE, ACT_RELU, ACT_RELU6, Act, BNRec, round4
from uda_clr_amd.kernels import UdaSrc

SPEC = SpecKernels()
_HIP = None
DETAIL = {}          # last case's per-output errors (for the report)


def hip():
    global _HIP
    if _HIP is None:
        from uda_clr_amd.kernels import HipKernels
        _HIP = HipKernels()
    return _HIP


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _poison(buf):
    """Fill a float matrix with what an uninitialised buffer may hold: NaN, +-Inf and huge finite values by row (the fused
    clamps swallow a NaN, so NaN alone would not show a padding lane that takes part in a sum; Inf * 0 does)."""
    vals = torch.tensor([float("nan"), float("inf"), -float("inf"), 3.0e38], dtype=buf.dtype, device=buf.device)
    buf.copy_(vals[torch.arange(buf.shape[0], device=buf.device) % 4].unsqueeze(1).expand_as(buf))
    return buf


def padded(P, C, g, dev=None, scale=1.0, dtype=torch.float32):
    """[P, C] view of a [P, round4(C)+4] buffer whose padding holds NaN / Inf / huge values (must never leak)."""
    buf = _poison(torch.empty((P, round4(C) + 4), dtype=dtype))
    buf[:, :C] = torch.randn(P, C, generator=g) * scale
    if dev is not None:
        buf = buf.to(dev)
    return buf[:, :C]


# ------------------------------------------------------------------------------------- launches past their grid caps
# Many launches take grid = min(ceil(work / items), CAP) workgroups and walk the remainder with a grid-stride (or persistent-tile)
# loop.  A "capped" case is shaped so that work > CAP * items, the last pass is partly filled and the work is no multiple of 256: the
# loop body runs a second time, on other indices than the first.  The caps are read from their plain-number #defines in csrc, the
# conditions are held without a GPU by tests/test_capped_cases_cpu.py, and a wrong value is reported with the pass it belongs to.
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uda_clr_amd", "csrc")
CAP_FILES = ("launch_caps.h", "dw_plan.h", "upconv_plan.h", "drn_head.hip")


@functools.lru_cache(maxsize=None)
def cap_value(name):
    """a workgroup cap of the library, from its ``#define NAME number`` in csrc"""
    for f in CAP_FILES:
        with open(os.path.join(CSRC, f)) as fh:
            m = re.search(r"^#define %s (\d+)\b" % re.escape(name), fh.read(), re.M)
        if m:
            return int(m.group(1))
    raise KeyError("no #define %s <number> in %s" % (name, ", ".join(CAP_FILES)))


class Capped:
    """One launch of a capped case.  launch: the kernel; cap: the name of its #define; work: its work items; items: work items
    per workgroup; index(row, column) -> the work item that writes that element of the compared output (a [P, C] matrix, or any
    other tensor flattened to [numel, 1]); None for an output that is a sum over all work items.  whole: why the work is a multiple of
    256 at every shape of this kind (else a capped case's work must not be one)."""
    def __init__(self, launch, cap, work, items=256, index=None, whole=None):
        self.launch, self.cap, self.work, self.items, self.index, self.whole = launch, cap, int(work), items, index, whole

    def grid(self):
        return min(-(-self.work // self.items), cap_value(self.cap))

    def passes(self):
        return -(-self.work // (self.grid() * self.items))


def by_group(C):
    """one thread per pixel row and group of 4 channels, channel groups fastest: e = row * (C / 4) + column / 4"""
    return lambda r, c: r * (C // 4) + c // 4


def by_element(C):
    return lambda r, c: r * C + c


def rel_at(got, want, tol, cap=None):
    """rel(got, want); beyond tol on a capped launch: an AssertionError that names the first wrong output's work item and the pass
    of the grid-stride loop it belongs to (item // (grid * items per workgroup))"""
    err = rel(got, want)
    if cap is None or cap.index is None or err <= tol:
        return err
    a, b = got.detach().double().cpu(), want.detach().double().cpu()
    if a.dim() != 2:
        a, b = a.reshape(-1, 1), b.reshape(-1, 1)
    bad = ~((a - b).abs() <= tol * max(b.abs().max().item(), 1e-30))          # (a NaN is wrong)
    r, c = (int(v) for v in bad.nonzero()[0])
    e = cap.index(r, c)
    raise AssertionError("%s: rel err %.3e > %.1e; the first wrong output (row %d, column %d) is work item %d of %d = pass %d of the "
                         "grid-stride loop (grid %d = %s, %d items per workgroup, %d of %d outputs wrong)"
                         % (cap.launch, err, tol, r, c, e, cap.work, e // (cap.grid() * cap.items), cap.grid(), cap.cap, cap.items,
                            int(bad.sum()), bad.numel()))


# ------------------------------------------------------------------------------------- write footprints
# Every device buffer a case hands to a kernel is a registered frame: the tensor the kernel sees, inside an allocation that the
# test owns on both sides of it.  After the case, footprint_violations() compares the bits of every frame with a snapshot and
# reports what changed outside the windows the kernels may write:
#   strided [P, C] matrices (to_dev): GUARD_ROWS poisoned rows before and after the P rows; the window is rows [0, P) x columns
#       [0, C) - the lanes [C, ld) of a row are "never written" (Padding lanes);
#   contiguous outputs (out_dev) and workspaces (HipKernels._ws, patched while a case runs): GUARD_BYTES of 0xA5 on both sides;
#   read-only operands (ro_dev, act_to): no window, every bit must survive.
# Known limit: a spill that writes the identical bit pattern back is invisible - with the by-row poison, a NaN written onto a NaN
# row.  The four fills alternate by row, so any spill that touches two consecutive rows is visible.
#
# GUARD_ROWS: the furthest a ragged last tile can reach behind row P - 1 (or before row 0) if its row guard were missing.
#   dense convs (conv_plan.h): tiles of 64 / 128 / 256 pixel rows, the last one starts at a row < P: at most 255 rows behind;
#   stem (dw_plan.h STEM_PIX_PER_WG): 256 pixels per workgroup: 255 rows;
#   flat / channel-blocked depthwise (dw_plan.h): lanes x DW_ITER_FWD pixels per workgroup, 256 / (C / 4) lanes: 512 pixels at
#       C = 4, 128 at the narrowest width any case uses (C = 64): 127 rows;
#   spatial TH x TW tiles - depthwise 8 x 16 / 8 x 8 (DW_TILED_VARIANTS), upconv 16 x 16 (UPT_TH x UPT_TW), the narrow dense 3x3
#       family 8 x 32 (N3_TW) and the 7x7 stride-1 stem 16 x 64 (H7_TH x H7_TW), resample one pixel per wave: the last tile of the
#       last image ends at linear row (tiles_y * TH - 1) * W + tiles_x * TW - 1 of that image.  The largest over-hang in the suite
#       is the stem's 1 x 33 x 80 shape (test_drn_kernels_gpu.py): tile rows 32..47 and columns 64..127 reach row 47 * 80 + 127 =
#       3887 of P = 2640 rows, 1247 behind; the depthwise shapes stay below 336 (the 8 x 8 tiles of the 1 x 97 x 95 stride-2 case: 49 x 48
#       outputs, tile rows 48..55 reach row 55 * 48 + 47 = 2687 of P = 2352, 335 behind; the 3 x 3-tile seam shapes 195 and 111),
#       upconv's tile kernel below 15 * 16 + 16.
#   1280 is the next multiple of 256 above all of them.
GUARD_ROWS = 1280          # multiple of 4: row 0 of the window keeps the poison phase and the 16-byte alignment of the allocation
GUARD_BYTES = 4096
_FRAMES = []


class _Frame:
    """bits: the whole allocation as a flat integer view; wins: [(offset, rows, pitch, width)] in elements of ``bits``;
    origin / pitch / unit describe how a flat position is reported: (row, column) of a matrix, or a byte offset"""
    __slots__ = ("name", "keep", "bits", "snap", "wins", "origin", "pitch", "unit")

    def __init__(self, name, keep, bits, wins, origin, pitch, unit):
        self.name, self.keep, self.bits, self.wins, self.origin, self.pitch, self.unit = name, keep, bits, wins, origin, pitch, unit
        self.snap = bits.clone()

    def where(self, i):
        rel = i - self.origin
        if self.pitch:
            return (rel // self.pitch, rel % self.pitch)       # (row, column); row -1 / row P: the guard rows
        return rel * self.unit                                  # byte offset from the first byte of the tensor


_BITS = {4: torch.int32, 8: torch.int64, 1: torch.uint8, 2: torch.int16}


def _flat_bits(t):
    """a contiguous tensor's memory as a flat integer tensor of the same element size (bits are compared, not float values)"""
    return t.view(-1).view(_BITS[t.element_size()])


def _register(name, keep, bits, wins, origin, pitch, unit):
    f = _Frame(name or "buffer %d" % len(_FRAMES), keep, bits, wins, origin, pitch, unit)
    _FRAMES.append(f)
    return f


def _frame_of(t):
    p = t.untyped_storage().data_ptr()
    for f in _FRAMES:
        if f.keep.untyped_storage().data_ptr() == p:
            return f
    raise KeyError("tensor is not part of a registered frame")


def _window(f, v):
    """the window of frame f that the view v covers (a [P, C] row-strided view, or any contiguous view)"""
    isz = f.bits.element_size()
    scale = v.element_size() // isz
    off = v.storage_offset() * v.element_size() // isz
    if v.dim() == 2 and not v.is_contiguous():
        assert v.stride(1) == 1
        return (off, v.shape[0], v.stride(0) * scale, v.shape[1] * scale)
    assert v.is_contiguous()
    return (off, 1, v.numel() * scale, v.numel() * scale)


def footprint_begin():
    del _FRAMES[:]


def to_dev(t, dev, name=None):
    """Move a [P, C] view keeping its row stride (so padding / alignment are preserved).  A strided view becomes rows
    [GUARD_ROWS, GUARD_ROWS + P) of a registered frame of GUARD_ROWS + P + GUARD_ROWS rows with the same row stride; padding
    lanes and guard rows hold the by-row poison, so a read out of range still leaks NaN / Inf into the compared values."""
    if t is None:
        return None
    if t.dim() == 2 and t.stride(0) != t.shape[1]:
        P, ld, G = t.shape[0], t.stride(0), GUARD_ROWS
        base = torch.empty(P + 2 * G, ld, dtype=t.dtype, device=dev)
        if t.dtype.is_floating_point:
            _poison(base)
        elif t.dtype == torch.uint8:
            base.copy_((torch.arange(base.numel(), device=dev) % 251).to(torch.uint8).view_as(base))      # keep-mask padding: arbitrary bytes
        v = base[G:G + P, :t.shape[1]]
        v.copy_(t)
        assert v.data_ptr() % 16 == 0 or ld * t.element_size() % 16
        _register(name or "matrix %d [%d, %d]" % (len(_FRAMES), P, t.shape[1]), base, _flat_bits(base), [(G * ld, P, ld, t.shape[1])], G * ld, ld, t.element_size())
        return v
    return t.to(dev)


def out_dev(shape, dtype, dev, fill=None, name=None, cols=None):
    """A contiguous output (weight gradient, NCHW head, coefficient vector, statistics accumulator, byte mask): a 16-byte aligned
    slice of a registered flat buffer with GUARD_BYTES of 0xA5 on both sides.  fill = None leaves the 0xA5 bytes in the tensor
    (torch.empty), a number fills it.  cols: of a 2-D tensor only columns [0, cols) of each row are a kernel's to write."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = torch.empty(0, dtype=dtype).element_size()
    for d in shape:
        n *= d
    buf = torch.full((2 * GUARD_BYTES + (n + 15) // 16 * 16,), 0xA5, dtype=torch.uint8, device=dev)
    t = buf[GUARD_BYTES:GUARD_BYTES + n].view(dtype).view(shape)
    assert t.data_ptr() % 16 == 0
    if fill is not None:
        t.fill_(fill)
    win = (GUARD_BYTES, 1, n, n)
    if cols is not None:
        win = (GUARD_BYTES, shape[0], shape[1] * t.element_size(), cols * t.element_size())
    _register(name or "output %d %s" % (len(_FRAMES), list(shape)), buf, buf, [win], GUARD_BYTES, 0, 1)
    return t


def out_like(t, dev, name=None):
    """a contiguous operand that a kernel updates in place: out_dev holding t's values"""
    return out_dev(t.shape, t.dtype, dev, name=name).copy_(t)


def ro_dev(t, dev, name=None):
    """an operand no kernel may write (weights, coefficient vectors, gradients read by a pass): checked whole"""
    if t is None:
        return None
    if t.dim() == 2 and t.stride(0) != t.shape[1]:
        return read_only(to_dev(t, dev, name))
    x = t.to(dev) if t.device != torch.device(dev) else t.clone()
    _register(name or "operand %d %s" % (len(_FRAMES), list(x.shape)), x, _flat_bits(x), [], 0, 0, x.element_size())
    return x


def read_only(t):
    """from here on no bit of the frame behind t may change (its snapshot is taken now)"""
    if t is not None:
        f = _frame_of(t)
        f.wins = []
        f.snap.copy_(f.bits)
    return t


def only_writes(*views):
    """Window cases: snapshot every frame now; until the next call of this function only the given views may change (all other
    columns of their matrices, the guard rows, every other frame and the neighbouring slices of a shared arena may not)."""
    for f in _FRAMES:
        f.wins = []
        f.snap.copy_(f.bits)
    for v in views:
        if v is not None:
            f = _frame_of(v)
            f.wins.append(_window(f, v))


def guarded_ws(like, nbytes):
    """stands in for HipKernels._ws while a case runs: exactly the queried bytes (16 where nothing is asked for, as the original),
    16-byte aligned, inside a registered buffer with GUARD_BYTES of 0xA5 on both sides"""
    n = int(nbytes) if int(nbytes) > 0 else 16
    buf = torch.full((2 * GUARD_BYTES + (n + 15) // 16 * 16,), 0xA5, dtype=torch.uint8, device=like.device)
    _register("workspace %d (%d bytes)" % (len(_FRAMES), n), buf, buf, [(GUARD_BYTES, 1, n, n)], GUARD_BYTES, 0, 1)
    return buf[GUARD_BYTES:GUARD_BYTES + n]


def footprint_violations():
    """[(frame name, position)] of every registered frame with a changed bit outside its windows: position is (row, column) of
    the first one in a strided matrix (row -1 / row P and beyond: guard rows; column >= C: padding lanes), else the byte offset
    from the tensor's first byte (negative: before it; >= its size: behind it)."""
    out = []
    for f in _FRAMES:
        d = f.bits != f.snap
        for off, rows, pitch, width in f.wins:
            d[off:off + rows * pitch].view(rows, pitch)[:, :width] = False
        if bool(d.any()):
            out.append((f.name, f.where(int(d.nonzero()[0]))))
    return out


class footprint:
    """``with footprint():`` - an empty registry, and HipKernels._ws handing out guarded workspaces inside"""
    def __enter__(self):
        from uda_clr_amd.kernels import HipKernels
        footprint_begin()
        self.cls, self.keep = HipKernels, HipKernels.__dict__["_ws"]
        HipKernels._ws = staticmethod(guarded_ws)
        return self

    def __exit__(self, *exc):
        self.cls._ws = self.keep
        return False


def footprinted(fn):
    """a case that begins with a cleared registry and runs under ``footprint``; the frames stay for footprint_violations()"""
    @functools.wraps(fn)
    def run(dev):
        with footprint():
            return fn(dev)
    return run


def act_to(a: Act, dev) -> Act:
    bn = None
    if a.bn is not None:
        bn = BNRec(a.bn.key, ro_dev(a.bn.mean, dev), ro_dev(a.bn.invstd, dev), a.bn.count, a.bn.q1_border)
    return Act(ro_dev(a.x, dev), a.N, a.H, a.W, ro_dev(a.scale, dev), ro_dev(a.shift, dev), a.act, ro_dev(a.mask, dev), a.mask_scale, bn)


def make_src(N, H, W, C, g, lazy=True, act=ACT_RELU, mask=False, bn=False, q1=False):
    P = N * H * W
    x = padded(P, C, g)
    scale = shift = None
    if lazy:
        scale = 0.5 + torch.rand(C, generator=g)
        shift = 0.3 * torch.randn(C, generator=g)
    m, ms = None, 1.0
    if mask:
        mb = torch.zeros(P, round4(C), dtype=torch.uint8)
        mb[:, :C] = (torch.rand(P, C, generator=g) > 0.3).to(torch.uint8)
        m, ms = mb[:, :C], 1.0 / 0.7
    rec = None
    if bn:
        rec = BNRec("t", 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g), float(P * (1.3 if q1 else 1.0)), q1)
    return Act(x, N, H, W, scale, shift, act if lazy else ACT_NONE, m, ms, rec)


# ------------------------------------------------------------------------------------- cases
# Dense cases (conv / dgrad / wgrad) declare with ``route=`` the launch the library must plan for their call (HipKernels.conv_route /
# wgrad_route: family, tile, template variant, splits).  The labels are the test ids and stay as they were written; where a label's
# parenthesised remark about tiles or kernels and the route differ, the route is what runs - it is asserted.  The same holds for the
# depthwise, stem and upconv cases (HipKernels.dw_route / stem_route / upconv_route).
def _declared(route, mfma):
    """a dense case's declared route: one text, or (f32, bf16x3) where the two MFMA modes differ"""
    return route if isinstance(route, str) else route[mfma]


def _check_route(got, route, mfma):
    assert got == _declared(route, mfma), "planned route %r, the case declares %r (mfma mode %d)" % (got, _declared(route, mfma), mfma)


def plan_route(K, q):
    """The route of a dense case's call from its recorded shape (``run.plan_query``) alone, without a GPU: stand-in addresses,
    the row strides of ``padded`` unless the query overrides them (ldx / ldy / ld_add: column windows of a wider matrix)."""
    s = UdaSrc()
    s.x, s.ldx, s.N, s.H, s.W, s.C = 0x10000, q.get("ldx") or round4(q["C"]) + 4, q["N"], q["H"], q["W"], q["C"]
    if q["lazy"]:
        s.scale, s.shift, s.act = 0x20000, 0x30000, ACT_RELU
    if q["mask"]:
        s.mask, s.ldm = 0x40000, round4(q["C"])
    ld = q.get("ldy") or round4(q["Cout"]) + 4
    ld_add = q.get("ld_add") or ld
    if q["kind"] == "wgrad":
        return K.route(K.wgrad_args(s, q["Cout"], q["k"], q["dil"], q["origin"], q["stride"], 0x50000, ld, 0x60000))
    return K.route(K.conv_args(s, q["Cout"], q["k"], q["dil"], q["origin"], q["stride"], 0x50000, 0x70000 if q["bias"] else None,
                               0x80000 if q["addend"] else None, ld_add if q["addend"] else 0, 0x90000, ld, 0xa0000 if q["stats"] else None))


def _query(kind, N, H, W, C, Cout, k, dil, lazy=False, mask=False, bias=False, addend=False, stats=False, origin=0, stride=1,
           ldx=None, ldy=None, ld_add=None):
    return dict(kind=kind, N=N, H=H, W=W, C=C, Cout=Cout, k=k, dil=dil, lazy=lazy, mask=mask, bias=bias, addend=addend, stats=stats,
                origin=origin, stride=stride, ldx=ldx, ldy=ldy, ld_add=ld_add)


def case_conv(N, H, W, Cin, Cout, k, dil, lazy=True, mask=False, bias=False, addend=False, stats=True, seed=0, origin=0, stride=1, *, route):
    """route: what HipKernels.conv_route must say about this call (asserted in the run, and without a GPU by test_conv_plan_cpu.py)"""
    def run(dev):
        g = gen(seed)
        src = make_src(N, H, W, Cin, g, lazy, ACT_RELU6 if Cin % 8 else ACT_RELU, mask)
        w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
        b = torch.randn(Cout, generator=g) if bias else None
        P = N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        kw = {"stride": stride} if stride != 1 else {}
        ad = padded(P, Cout, g) if addend else None
        out_r = padded(P, Cout, g)
        st_r = torch.zeros(16, 2, Cout, dtype=torch.float64) if stats else None
        SPEC.conv(src, SPEC.relayout_ohwi(w), k, dil, out_r, b, ad, st_r, origin=origin, **kw)
        K = hip()
        out_h = to_dev(padded(P, Cout, g), dev)
        st_h = out_dev((16, 2, Cout), torch.float64, dev, fill=0) if stats else None
        wl = ro_dev(K.relayout_ohwi(w.to(dev)), dev)
        errs = [rel(wl, SPEC.relayout_ohwi(w))]
        args = (act_to(src, dev), wl, k, dil, out_h, ro_dev(b, dev), ro_dev(ad, dev), st_h)
        _check_route(K.conv_route(*args, origin=origin, **kw), route, K.mfma)
        K.conv(*args, origin=origin, **kw)
        errs.append(rel(out_h, out_r))
        if stats:
            errs.append(rel(st_h.sum(0), st_r.sum(0)))
        return max(errs), 2e-5
    run.plan_query, run.route = _query("conv", N, H, W, Cin, Cout, k, dil, lazy, mask, bias, addend, stats, origin, stride), route
    return run


def case_dgrad(N, H, W, Cin, Cout, k, dil, accumulate=False, seed=1, *, route):
    """input-gradient of a conv = conv of dy with the dgrad weight layout"""
    def run(dev):
        g = gen(seed)
        P = N * H * W
        dy = padded(P, Cout, g)
        w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
        ad = padded(P, Cin, g) if accumulate else None
        ref = torch.nn.grad.conv2d_input((N, Cin, H, W), w, dy.reshape(N, H, W, Cout).permute(0, 3, 1, 2), 1,
                                         dil * (k // 2), dil).permute(0, 2, 3, 1).reshape(P, Cin)
        if ad is not None:
            ref = ref + ad
        K = hip()
        wd = ro_dev(K.relayout_dgrad(w.to(dev)), dev)
        e0 = rel(wd, SPEC.relayout_dgrad(w))
        out = to_dev(padded(P, Cin, g), dev)
        adh = to_dev(ad, dev)
        if accumulate:      # in-place accumulate, as the engine uses it
            out.copy_(adh)
            adh = out
        args = (Act(ro_dev(dy, dev), N, H, W), wd, k, dil, out)
        _check_route(K.conv_route(*args, addend=adh), route, K.mfma)
        K.conv(*args, addend=adh)
        return max(e0, rel(out, ref)), 2e-5
    run.plan_query, run.route = _query("conv", N, H, W, Cout, Cin, k, dil, addend=accumulate), route
    return run


def case_wgrad(N, H, W, Cin, Cout, k, dil, lazy=True, mask=False, seed=2, origin=0, stride=1, *, route):
    def run(dev):
        g = gen(seed)
        src = make_src(N, H, W, Cin, g, lazy, ACT_RELU, mask)
        dy = padded(N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1), Cout, g)
        ref = torch.empty(Cout, Cin, k, k)
        kw = {"stride": stride} if stride != 1 else {}
        SPEC.conv_wgrad(src, dy, k, dil, ref, origin=origin, **kw)
        out = out_dev((Cout, Cin, k, k), torch.float32, dev)
        K = hip()
        args = (act_to(src, dev), ro_dev(dy, dev), k, dil, out)
        _check_route(K.wgrad_route(*args, origin=origin, **kw), route, K.mfma)
        K.conv_wgrad(*args, origin=origin, **kw)
        return rel(out, ref), 3e-5
    run.plan_query, run.route = _query("wgrad", N, H, W, Cin, Cout, k, dil, lazy, mask, origin=origin, stride=stride), route
    return run


def _entry(route):
    return " ".join(route.split()[:2])          # "<family> <tile>" of a dense route, "<op> <kernel>" of a depthwise / stem one


def case_dw(N, H, W, C, stride, dil, border, seed=3, capped=False, seams=False, *, route):
    """route: the "<op> <kernel>" HipKernels.dw_route must begin with for the forward, input-gradient and weight-gradient call
    (asserted before each call, and without a GPU by test_dw_plan_cpu.py).  capped: the flat input gradient runs past its cap;
    seams: the tiled forward / weight gradient have real neighbours on every side of a tile (test_capped_cases_cpu.py holds both)."""
    cap = Capped("dwconv_dgrad_kernel", "DW_DGRAD_MAX_WG", N * H * W * (C // 4), 256, by_group(C),
                 whole="C / 4 = 256 channel groups: one pixel per workgroup" if C == 1024 else None) if capped else None

    def run(dev):
        g = gen(seed)
        src = make_src(N, H, W, C, g, True, ACT_RELU6)
        w = torch.randn(C, 1, 3, 3, generator=g) / 3.0
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        Po = N * Ho * Wo
        K = hip()
        w9 = SPEC.relayout_dw(w)
        w9h = ro_dev(K.relayout_dw(w.to(dev)), dev)
        errs = [rel(w9h, w9)]
        y_r, st_r = padded(Po, C, g), torch.zeros(16, 2, C, dtype=torch.float64)
        SPEC.dwconv_fwd(src, w9, stride, dil, border, y_r, st_r)
        y_h, st_h = to_dev(padded(Po, C, g), dev), out_dev((16, 2, C), torch.float64, dev, fill=0)
        sh = act_to(src, dev)
        for op, want in zip(("fwd", "dgrad", "wgrad"), route):
            got = _entry(K.dw_route(op, N, H, W, C, stride, dil))
            assert got == want, "planned route %r, the case declares %r" % (got, want)
        K.dwconv_fwd(sh, w9h, stride, dil, border, y_h, st_h)
        errs += [rel(y_h, y_r), rel(st_h.sum(0), st_r.sum(0))]
        dy = padded(Po, C, g)
        dx_r = padded(N * H * W, C, g)
        SPEC.dwconv_dgrad(dy, w9, stride, dil, N, H, W, dx_r)
        dx_h = to_dev(padded(N * H * W, C, g), dev)
        K.dwconv_dgrad(ro_dev(dy, dev), w9h, stride, dil, N, H, W, dx_h)
        errs.append(rel_at(dx_h, dx_r, 3e-5, cap))
        dw_r = torch.empty(C, 1, 3, 3)
        SPEC.dwconv_wgrad(src, dy, stride, dil, border, dw_r)
        dw_h = out_dev((C, 1, 3, 3), torch.float32, dev)
        K.dwconv_wgrad(sh, ro_dev(dy, dev), stride, dil, border, dw_h)
        errs.append(rel(dw_h, dw_r))
        return max(errs), 3e-5
    run.dw_query, run.route = dict(N=N, H=H, W=W, C=C, stride=stride, dil=dil), route
    run.capped, run.seams = [cap] if capped else [], seams
    return run


def _stem_dy(Po, g, dy_offset):
    """the stem's output gradient, [Po, 32]: padded(), or with dy_offset = 1 columns 1..32 of a poisoned [Po, 33] matrix"""
    if not dy_offset:
        return padded(Po, 32, g)
    return _poison(torch.empty(Po, 33))[:, 1:33].copy_(torch.randn(Po, 32, generator=g))


def case_stem(N, H, W, seed=4, dy_offset=0, *, route):
    """route: the "<op> <kernel>" HipKernels.stem_route must begin with for the forward and the weight-gradient call.
    dy_offset = 1: dy is columns 1..32 of a [Po, 33] matrix - neither 16-byte aligned nor with a row stride that is a multiple of 4."""
    def run(dev):
        g = gen(seed)
        x = torch.randn(N, 3, H, W, generator=g)
        w = torch.randn(32, 3, 3, 3, generator=g) / 5.0
        Po = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        y_r, st_r = padded(Po, 32, g), torch.zeros(16, 2, 32, dtype=torch.float64)
        SPEC.stem_fwd(x, w, y_r, st_r)
        K = hip()
        y_h, st_h = to_dev(padded(Po, 32, g), dev), out_dev((16, 2, 32), torch.float64, dev, fill=0)
        xh = ro_dev(x, dev)
        assert _entry(K.stem_route("fwd", xh)) == route[0], (K.stem_route("fwd", xh), route)
        K.stem_fwd(xh, ro_dev(w, dev), y_h, st_h)
        dy = _stem_dy(Po, g, dy_offset)
        dw_r, dw_h = torch.empty(32, 3, 3, 3), out_dev((32, 3, 3, 3), torch.float32, dev)
        SPEC.stem_wgrad(x, dy, dw_r)
        dyh = _poison(torch.empty(Po, 33, device=dev))[:, 1:33].copy_(dy) if dy_offset else ro_dev(dy, dev)
        assert (dyh.stride(0), dyh.data_ptr() % 16 == 0) == (q["lddy"], q["aligned"]), "stem_query does not describe the dy of this call"
        assert _entry(K.stem_route("wgrad", xh, dyh)) == route[1], (K.stem_route("wgrad", xh, dyh), route)
        K.stem_wgrad(xh, dyh, dw_h)
        return max(rel(y_h, y_r), rel(st_h.sum(0), st_r.sum(0)), rel(dw_h, dw_r)), 3e-5
    # what the weight gradient's route depends on besides the image: dy's row stride and 16-byte alignment, read off a one-row dy
    d1 = _stem_dy(1, gen(seed), dy_offset)
    q = dict(N=N, H=H, W=W, lddy=d1.stride(0), aligned=d1.storage_offset() % 4 == 0)
    run.stem_query, run.route = q, route
    return run


def case_transnorm(C, n0=300, n1=500, seed=9):
    """uda_tn_gain / uda_tn_eval_coeffs against their torch statement (batchnorm.py:474-520)."""
    def run(dev):
        g = gen(seed)
        K = hip()
        xs = [2.0 * torch.randn(n0, C, generator=g) + 0.5, 0.7 * torch.randn(n1, C, generator=g) - 0.2]
        st = torch.zeros(2, 16, 2, C, dtype=torch.float64)
        for h in (0, 1):
            SPEC.colstats(xs[h], st[h])
        st = st[:, torch.randperm(16, generator=g)]                  # any slot may hold the sums
        gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
        cr = torch.randn(2, 2, C, generator=g)                        # [scale | shift][half][C], pre-filled as after bn_finalize
        ch = out_like(cr, dev)
        gr, gh = torch.empty(C), out_dev((C,), torch.float32, dev)
        SPEC.tn_gain(st[0], st[1], float(n0), float(n1), 1e-5, cr[0, 0], cr[1, 0], cr[0, 1], cr[1, 1], gr)
        sth = st.to(dev)
        K.tn_gain(sth[0], sth[1], float(n0), float(n1), 1e-5, ch[0, 0], ch[1, 0], ch[0, 1], ch[1, 1], gh)
        errs = [rel(gh, gr), rel(ch, cr)]
        rms, rmt = torch.randn(C, generator=g), torch.randn(C, generator=g)
        rvs, rvt = 0.5 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g)
        er, eh = torch.empty(2, C), out_dev((2, C), torch.float32, dev)
        SPEC.tn_eval_coeffs(gamma, beta, rms, rvs, rmt, rvt, 1e-5, er[0], er[1])
        K.tn_eval_coeffs(gamma.to(dev), beta.to(dev), rms.to(dev), rvs.to(dev), rmt.to(dev), rvt.to(dev), 1e-5, eh[0], eh[1])
        errs.append(rel(eh, er))
        return max(errs), 2e-6
    return run


def case_bn(P, C, q1=False, mask=False, training=True, seed=5, frozen=False):
    def run(dev):
        g = gen(seed)
        K = hip()
        errs = []
        x = padded(P, C, g, scale=2.0)
        st_r = torch.zeros(16, 2, C, dtype=torch.float64)
        SPEC.colstats(x, st_r)
        st_h = out_dev((16, 2, C), torch.float64, dev, fill=0)
        K.colstats(ro_dev(x, dev), st_h)
        errs.append(rel(st_h.sum(0), st_r.sum(0)))
        gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
        rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
        cr = torch.empty(4, C)
        ch = out_dev((4, C), torch.float32, dev)
        rmh, rvh = out_like(rm, dev), out_like(rv, dev)
        cnt = float(P * (1.25 if q1 else 1.0))
        if training:
            SPEC.bn_finalize(st_r, cnt, gamma, beta, rm, rv, 0.1, 1e-5, cr[0], cr[1], cr[2], cr[3])
            K.bn_finalize(st_h, cnt, ro_dev(gamma, dev), ro_dev(beta, dev), rmh, rvh, 0.1, 1e-5, ch[0], ch[1], ch[2], ch[3])
            errs += [rel(ch, cr), rel(rmh, rm), rel(rvh, rv)]
        else:
            SPEC.bn_eval_coeffs(gamma, beta, rm, rv, 1e-5, cr[0], cr[1])
            K.bn_eval_coeffs(ro_dev(gamma, dev), ro_dev(beta, dev), ro_dev(rm, dev), ro_dev(rv, dev), 1e-5, ch[0], ch[1])
            cr[2:], ch[2:] = 0.0, 0.0
            errs.append(rel(ch[:2], cr[:2]))
        # keep pre-activations away from the ReLU/ReLU6 kinks: there the gate legitimately depends
        # on fma-vs-(mul,add) rounding, which is not what this case tests
        a0 = x * cr[0] + cr[1]
        x[(a0.abs() < 1e-4) | ((a0 - 6).abs() < 1e-4)] += 0.01
        if C % 4 == 0:
            m = None
            if mask:
                m = (torch.rand(P, C, generator=g) > 0.5).to(torch.uint8)
            src = Act(x, 1, 1, P, cr[0].clone(), cr[1].clone(), ACT_RELU, m, 2.0 if mask else 1.0)
            res = padded(P, C, g)
            o_r = padded(P, C, g)
            SPEC.bn_apply(src, o_r, res)
            o_h = to_dev(padded(P, C, g), dev)
            K.bn_apply(act_to(src, dev), o_h, ro_dev(res, dev))
            errs.append(rel(o_h, o_r))
        if training or frozen:
            q1t = None
            if frozen:       # eval-mode BN inside a training pass (freeze_bn): xhat against the running statistics, count = inf,
                cr[2], cr[3] = rm, torch.rsqrt(rv + 1e-5)      # and the quirk-Q1 total handed in
                cnt = float("inf")
                q1t = torch.randn(C, generator=g) if q1 else None
            mb = None
            if mask:
                mbuf = torch.zeros(P, round4(C), dtype=torch.uint8)
                mbuf[:, :C] = (torch.rand(P, C, generator=g) > 0.5).to(torch.uint8)
                mb = mbuf[:, :C]
            y = Act(x, 1, 1, P, cr[0].clone(), cr[1].clone(), ACT_RELU6 if q1 else ACT_RELU, mb, 2.0 if mask else 1.0,
                    BNRec("t", cr[2].clone(), cr[3].clone(), cnt, q1))
            dU = padded(P, C, g)
            s_r = torch.zeros(16, 3, C, dtype=torch.float64)
            SPEC.bnbwd_reduce(dU, y, s_r)
            yh = act_to(y, dev)
            dUh = ro_dev(dU, dev)
            s_h = out_dev((16, 3, C), torch.float64, dev, fill=0)
            K.bnbwd_reduce(dUh, yh, s_h)
            errs.append(rel(s_h.sum(0), s_r.sum(0)))
            gr, gh = torch.empty(4, C), out_dev((4, C), torch.float32, dev)
            SPEC.bnbwd_finalize(s_r, y, gr[0], gr[1], gr[2], gr[3], q1_total=q1t)
            K.bnbwd_finalize(s_h, yh, gh[0], gh[1], gh[2], gh[3], q1_total=None if q1t is None else q1t.to(dev))
            errs.append(rel(gh[2:], gr[2:]))
            errs.append(float((gh[:2].cpu() - gr[:2]).abs().max()) if frozen else rel(gh[:2], gr[:2]))     # frozen: c1 = c2 = 0 exactly
            ad = padded(P, C, g)
            o_r = padded(P, C, g)
            SPEC.bnbwd_apply(dU, y, gr[0], gr[1], o_r, ad)
            adh = to_dev(ad, dev)
            K.bnbwd_apply(dUh, yh, gh[0], gh[1], adh, adh)      # in place over the addend
            errs.append(rel(adh, o_r))
        DETAIL.clear()
        DETAIL.update({"errs": ["%.1e" % e for e in errs]})
        return max(errs), 3e-5
    return run


def case_bnbwd_lowrank(P, C, k, mask, seed=9):
    """uda_bnbwd_reduce_lowrank / uda_bnbwd_apply_lowrank: the BN-backward passes on an upstream gradient given as the outer product
    d [P, k] @ w [k, C] (the input gradient of the decoder's 1x1 heads, k = 2 / 1) against (a) the torch statement and (b) the
    ordinary passes fed the materialised matrix."""
    def run(dev):
        g = gen(seed)
        K = hip()
        x = padded(P, C, g)
        sc, sh = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
        a0 = x * sc + sh
        x[a0.abs() < 1e-4] += 0.01
        mean, istd = 0.1 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
        mb = None
        if mask:
            mbuf = torch.zeros(P, round4(C), dtype=torch.uint8)
            mbuf[:, :C] = (torch.rand(P, C, generator=g) > 0.1).to(torch.uint8)
            mb = mbuf[:, :C]
        y = Act(x, 1, 1, P, sc, sh, ACT_RELU, mb, 1.0 / 0.9 if mask else 1.0, BNRec("t", mean, istd, float(P), False))
        wide = padded(P, 8, g)                                  # d is a column window of a wider matrix, as in the engine
        d = wide[:, 4:4 + k]
        w = torch.randn(k, C, generator=g) / C ** 0.5
        s_r = torch.zeros(16, 3, C, dtype=torch.float64)
        SPEC.bnbwd_reduce(None, y, s_r, lowrank=(d, w))
        yh, dh, wh = act_to(y, dev), ro_dev(wide, dev)[:, 4:4 + k], ro_dev(w, dev)
        s_h = out_dev((16, 3, C), torch.float64, dev, fill=0)
        K.bnbwd_reduce(None, yh, s_h, lowrank=(dh, wh))
        s_m = out_dev((16, 3, C), torch.float64, dev, fill=0)
        dU = to_dev(padded(P, C, g), dev)
        dU.copy_(dh @ wh)
        K.bnbwd_reduce(dU, yh, s_m)
        errs = [rel(s_h.sum(0), s_r.sum(0)), rel(s_h.sum(0), s_m.sum(0))]
        gr = torch.empty(4, C)
        SPEC.bnbwd_finalize(s_r, y, gr[0], gr[1], gr[2], gr[3])
        gh = gr.to(dev)
        ad = padded(P, C, g)
        o_r = padded(P, C, g)
        SPEC.bnbwd_apply(None, y, gr[0], gr[1], o_r, ad, lowrank=(d, w))
        adh = to_dev(ad, dev)
        o_m = to_dev(padded(P, C, g), dev)
        K.bnbwd_apply(dU, yh, gh[0], gh[1], o_m, adh)
        K.bnbwd_apply(None, yh, gh[0], gh[1], adh, adh, lowrank=(dh, wh))      # in place over the addend, as the engine does
        errs += [rel(adh, o_r), rel(adh, o_m)]
        return max(errs), 3e-5
    return run


def case_mc_seg_head(N, h, w, H, W, Cf, Cl, reps, mask, seed=10):
    """uda_mc_seg_head (the 305 -> 2 head of a no-grad stochastic pass on the virtual x_feature = cat(up(feature), low rows shared by
    the repeated batch, boundary)) and the store-less statistics pass uda_upsample_fwd_stats(out = NULL), against the torch statement
    that materialises the matrix."""
    def run(dev):
        g = gen(seed)
        K = hip()
        P, Cc = N * H * W, Cf + Cl + 1
        feat = padded(N * h * w, Cf, g)
        low = padded(P // reps, Cl, g)
        bnd = padded(P, 1, g)
        sc, sh = 0.5 + torch.rand(Cc, generator=g), 0.3 * torch.randn(Cc, generator=g)
        mk = None
        if mask:
            mbuf = torch.randint(0, 256, (P, round4(Cc)), generator=g, dtype=torch.uint8)     # padding bytes arbitrary
            mbuf[:, :Cc] = (torch.rand(P, Cc, generator=g) > 0.1).to(torch.uint8)
            mk = mbuf[:, :Cc]
        w4 = torch.randn(2, Cc, 1, 1, generator=g) / Cc ** 0.5
        bias = torch.randn(2, generator=g)
        o_r, o_h = padded(P, 2, g), to_dev(padded(P, 2, g), dev)
        SPEC.mc_seg_head(feat, N, h, w, low, bnd, H, W, sc, sh, ACT_RELU, mk, 1.0 / 0.9, SPEC.relayout_ohwi(w4), bias, o_r)
        K.mc_seg_head(ro_dev(feat, dev), N, h, w, ro_dev(low, dev), ro_dev(bnd, dev), H, W, ro_dev(sc, dev), ro_dev(sh, dev), ACT_RELU,
                      None if mk is None else ro_dev(mbuf, dev)[:, :Cc], 1.0 / 0.9, ro_dev(K.relayout_ohwi(w4.to(dev)), dev), ro_dev(bias, dev), o_h)
        st_r = torch.zeros(16, 2, Cc, dtype=torch.float64)
        st_h = out_dev((16, 2, Cc), torch.float64, dev, fill=0)
        SPEC.upsample_stats(feat, N, h, w, H, W, st_r)
        K.upsample_stats(ro_dev(feat, dev), N, h, w, H, W, st_h)
        return max(rel(o_h, o_r), rel(st_h.sum(0), st_r.sum(0))), 2e-5
    return run


def case_upsample_stats(N, h, w, H, W, C, Cs, seed=8, capped=False):
    """uda_upsample_fwd_stats: the upsampled tensor AND its per-channel (sum, sum of squares) in channels [0, C) of a wider
    accumulator; uda_colstats_window: the remaining channels of the wide buffer (a strided column window) into the same accumulator
    (round 3: the BatchNorm(305) statistics of decoder.py:23 without a pass over the whole 305-channel buffer)."""
    def run(dev):
        g = gen(seed)
        K = hip()
        x = padded(N * h * w, C, g)
        wide_r, wide_h = padded(N * H * W, Cs, g), to_dev(padded(N * H * W, Cs, g), dev)
        wide_r[:, C:] = torch.randn(N * H * W, Cs - C, generator=g)
        wide_h[:, C:] = wide_r[:, C:].to(dev)
        st_r = torch.zeros(16, 2, Cs, dtype=torch.float64)
        st_h = out_dev((16, 2, Cs), torch.float64, dev, fill=0)
        SPEC.upsample_fwd(x, N, h, w, wide_r[:, :C], H, W, stats=st_r)
        K.upsample_fwd(ro_dev(x, dev), N, h, w, wide_h[:, :C], H, W, stats=st_h)
        SPEC.colstats_window(wide_r[:, C:], st_r, C)
        K.colstats_window(wide_h[:, C:], st_h, C)
        full = torch.zeros(16, 2, Cs, dtype=torch.float64)
        SPEC.colstats(wide_r, full)                       # the one-pass statement over the whole buffer
        return max(rel_at(wide_h[:, :C], wide_r[:, :C], 2e-5, cap), rel(wide_h, wide_r), rel(st_h.sum(0), st_r.sum(0)),
                   rel(st_h.sum(0), full.sum(0))), 2e-5
    cap = Capped("upsample_fwd_kernel<true, true>", "UPSAMPLE_STATS_MAX_WG", N * H * W * (C // 4), 256, by_group(C)) if capped else None
    run.capped = [cap] if capped else []
    return run


def case_resample(N, h, w, H, W, C, seed=6, capped=False):
    caps = [Capped("upsample_fwd_kernel", "RESAMPLE_MAX_WG", N * H * W * (C // 4), 256, by_group(C)),
            Capped("upsample_bwd_kernel", "RESAMPLE_MAX_WG", N * h * w * (C // 4), 256, by_group(C))] if capped else [None, None]

    def run(dev):
        g = gen(seed)
        K = hip()
        x = padded(N * h * w, C, g)
        o_r, o_h = padded(N * H * W, C, g), to_dev(padded(N * H * W, C, g), dev)
        SPEC.upsample_fwd(x, N, h, w, o_r, H, W)
        K.upsample_fwd(ro_dev(x, dev), N, h, w, o_h, H, W)
        ref_t = torch.nn.functional.interpolate(x.reshape(N, h, w, C).permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                                                align_corners=True).permute(0, 2, 3, 1).reshape(N * H * W, C)
        errs = [rel_at(o_h, o_r, 2e-5, caps[0]), rel(o_h, ref_t)]
        d = padded(N * H * W, C, g)
        dx_r, dx_h = padded(N * h * w, C, g), to_dev(padded(N * h * w, C, g), dev)
        SPEC.upsample_bwd(d, N, H, W, dx_r, h, w)
        K.upsample_bwd(ro_dev(d, dev), N, H, W, dx_h, h, w)
        errs.append(rel_at(dx_h, dx_r, 2e-5, caps[1]))
        return max(errs), 2e-5
    run.capped = caps if capped else []
    return run


def case_head(N, h, w, H, W, C, seed=7, capped=False):
    # one thread per pixel; the forward's output is NCHW: flat element ((n * C + c) * H + oh) * W + ow belongs to pixel (n, oh, ow)
    caps = [Capped("head_upsample_fwd_kernel", "RESAMPLE_MAX_WG", N * H * W, 256, lambda r, c: r // (C * H * W) * H * W + r % (H * W)),
            Capped("head_upsample_bwd_kernel", "RESAMPLE_MAX_WG", N * h * w, 256, lambda r, c: r)] if capped else [None, None]

    def run(dev):
        g = gen(seed)
        K = hip()
        x = padded(N * h * w, C, g)
        o_r, o_h = torch.empty(N, C, H, W), out_dev((N, C, H, W), torch.float32, dev)
        SPEC.head_upsample_fwd(x, N, h, w, o_r)
        K.head_upsample_fwd(ro_dev(x, dev), N, h, w, o_h)
        ref_t = torch.nn.functional.interpolate(x.reshape(N, h, w, C).permute(0, 3, 1, 2), size=(H, W), mode="bilinear",
                                                align_corners=True)
        errs = [rel_at(o_h, o_r, 2e-5, caps[0]), rel(o_h, ref_t)]
        d = torch.randn(N, C, H, W, generator=g)
        base = padded(N * h * w, C, g)
        dx_r = base.clone()
        SPEC.head_upsample_bwd(d, dx_r, N, h, w, True)
        dx_h = to_dev(base, dev)
        K.head_upsample_bwd(ro_dev(d, dev), dx_h, N, h, w, True)
        errs.append(rel_at(dx_h, dx_r, 2e-5, caps[1]))
        dx_h2 = to_dev(base, dev)
        K.head_upsample_bwd(ro_dev(d, dev), dx_h2, N, h, w, False)
        errs.append(rel_at(dx_h2, dx_r - base, 2e-5, caps[1]))
        return max(errs), 2e-5
    run.capped = caps if capped else []
    return run


def case_gap(N, HW, C, seed=8, capped=False):
    cap = Capped("broadcast_rows_kernel", "RESAMPLE_MAX_WG", N * HW * (C // 4), 256, by_group(C)) if capped else None

    def run(dev):
        g = gen(seed)
        K = hip()
        x = padded(N * HW, C, g)
        o_r, o_h = torch.empty(N, C), out_dev((N, C), torch.float32, dev)
        SPEC.gap_fwd(x, N, o_r, 1.0 / HW)
        K.gap_fwd(ro_dev(x, dev), N, o_h, 1.0 / HW)
        errs = [rel(o_h, o_r)]
        ad = padded(N * HW, C, g)
        b_r, b_h = padded(N * HW, C, g), to_dev(padded(N * HW, C, g), dev)
        SPEC.broadcast_rows(o_r, N, b_r, 0.25, ad)
        K.broadcast_rows(ro_dev(o_r, dev), N, b_h, 0.25, ro_dev(ad, dev))
        errs.append(rel_at(b_h, b_r, 2e-5, cap))
        return max(errs), 2e-5
    run.capped = [cap] if capped else []
    return run


def case_dropout(P, C, p, seed=9, capped=False):
    """capped: P * ceil(C / 8) work items exceed the cap.  The kernel's counter is the ELEMENT index e = row * ceil(C / 8) + group
    (uda_dropout_mask), whatever the grid: the rows a second pass serves must not repeat those of the first, must keep the rate, and
    the rows [0, 4096) must equal the mask of the same (seed, offset) and C drawn on 4096 rows, which fit one pass."""
    G8 = (C + 7) // 8
    cap = Capped("dropout_mask_kernel", "RESAMPLE_MAX_WG", P * G8, 256, by_element(G8)) if capped else None

    def run(dev):
        K = hip()
        m = out_dev((P, round4(C)), torch.uint8, dev, fill=0)[:, :C]      # uda_dropout_mask writes round4(C) bytes per row (its documented shape)
        K.dropout_mask(m, p, 1234, 7)
        m2 = out_dev((P, round4(C)), torch.uint8, dev, fill=0)[:, :C]      # uda_dropout_mask writes round4(C) bytes per row (its documented shape)
        K.dropout_mask(m2, p, 1234, 7)
        m3 = out_dev((P, round4(C)), torch.uint8, dev, fill=0)[:, :C]      # uda_dropout_mask writes round4(C) bytes per row (its documented shape)
        K.dropout_mask(m3, p, 1234, 8)
        assert torch.equal(m, m2), "same (seed, offset) must reproduce the mask"
        assert not torch.equal(m, m3), "different offsets must give different masks"
        assert int(m.max()) <= 1
        keep = m.float().mean().item()
        col = m.float().mean(0)
        # binomial tolerance (5 sigma) on the overall rate, loose bound per column
        sig = ((1 - p) * p / (P * C)) ** 0.5
        err = abs(keep - (1 - p)) / (5 * sig)
        assert (col - (1 - p)).abs().max().item() < 8 * ((1 - p) * p / P) ** 0.5
        if capped:
            assert cap.grid() * 256 % G8 == 0
            step = cap.grid() * 256 // G8                    # rows one pass of the grid serves
            n2 = P - step                                    # rows [step, P): the second pass
            assert 0 < n2 < step
            a, b = m[:n2].cpu(), m[step:].cpu()
            same_rows = int((a == b).all(1).sum())
            # a counter taken from the thread index repeats every row; independent rows agree per byte with probability q
            q = (1 - p) ** 2 + p ** 2
            agree = (a == b).float().mean().item()
            assert same_rows == 0, "%d of %d second-pass rows copy the row one grid stride (%d rows) before them" % (same_rows, n2, step)
            assert abs(agree - q) < 5 * (q * (1 - q) / (n2 * C)) ** 0.5, "rows p and p + %d agree in %.4f of their bytes, %.4f expected" % (step, agree, q)
            keep2 = b.float().mean().item()
            err = max(err, abs(keep2 - (1 - p)) / (5 * ((1 - p) * p / (n2 * C)) ** 0.5))      # the second pass alone, its own 5 sigma
            ms = out_dev((4096, round4(C)), torch.uint8, dev, fill=0)[:, :C]
            K.dropout_mask(ms, p, 1234, 7)
            assert torch.equal(m[:4096], ms), "the mask of a shape past the cap differs from the one-pass mask of the same (seed, offset) on the rows both have"
        return err, 1.0
    run.capped = [cap] if capped else []
    return run


CASES = [
    # 1x1 convs of the backbone (narrow N configs, small K, Q1-style sizes)
    ("conv1x1 16->96 relu6", case_conv(2, 24, 20, 16, 96, 1, 1, route="low 64x128 xf1")),
    ("conv1x1 96->24 none-lazy", case_conv(2, 17, 13, 96, 24, 1, 1, lazy=False, route="low 64x64 xf0")),
    ("conv1x1 144->32", case_conv(1, 16, 16, 144, 32, 1, 1, route="low 64x64 xf1")),
    ("conv1x1 32->192 (128-wide tiles)", case_conv(2, 12, 12, 32, 192, 1, 1, route="narrow 128x96 xf1")),
    ("conv1x1 960->320", case_conv(2, 8, 8, 960, 320, 1, 1, stats=True, route="ws 64x128 k1 xf1")),
    ("conv1x1 1280->256 relu", case_conv(2, 8, 8, 1280, 256, 1, 1, route=("ws 64x128 k1 xf1", "x3 128x128 k1"))),
    ("conv1x1 305->2 bias mask (C%4!=0)", case_conv(2, 16, 16, 305, 2, 1, 1, mask=True, bias=True, stats=False, route="heads 128x2")),
    ("conv1x1 256->1 bias mask", case_conv(2, 16, 16, 256, 1, 1, 1, mask=True, bias=True, stats=False, route="heads 128x1")),
    ("conv1x1 100->2 addend, ragged P (heads kernel, raw operand)", case_conv(2, 17, 13, 100, 2, 1, 1, lazy=False, addend=True, stats=False, route="heads 128x2")),
    ("conv1x1 68->1 lazy, P < 128 (heads kernel)", case_conv(1, 9, 7, 68, 1, 1, 1, bias=True, stats=False, route="heads 128x1")),
    ("conv1x1 320->256 P=N (gap branch)", case_conv(4, 1, 1, 320, 256, 1, 1, lazy=False, route="ws 64x128 k1 xf0")),
    ("conv1x1 24->48 addend", case_conv(2, 16, 16, 24, 48, 1, 1, addend=True, stats=False, route="low 64x64 xf1")),
    # 3x3 convs
    ("conv3x3 304->256 p1 mask", case_conv(2, 16, 16, 304, 256, 3, 1, lazy=False, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("conv3x3 256->256 relu mask", case_conv(2, 16, 12, 256, 256, 3, 1, mask=True, route=("ws 64x128 k3 xf2", "x3 128x128 k3"))),
    ("conv3x3 320->256 dil6", case_conv(2, 8, 8, 320, 256, 3, 6, lazy=False, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("conv3x3 320->256 dil12 (mostly padding)", case_conv(2, 8, 8, 320, 256, 3, 12, lazy=False, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("conv3x3 64->40 dil2 odd sizes", case_conv(1, 11, 9, 64, 40, 3, 2, route="low 64x64 pipe")),
    ("conv3x3 256->48 (long K, narrow tile)", case_conv(2, 16, 16, 256, 48, 3, 1, lazy=False, route=("low 64x64 pipe", "x3 256x64 k3"))),
    ("conv3x3 128->64 relu mask stats (long K, narrow tile)", case_conv(2, 12, 12, 128, 64, 3, 1, mask=True, route=("low 64x64 pipe", "x3 256x64 k3"))),
    ("dgrad3x3 48<-256 addend (the decoder's low-level input gradient)", case_dgrad(2, 16, 16, 48, 256, 3, 1, accumulate=True, route=("low 64x64 pipe", "x3 256x64 k3"))),
    # dgrad through the same kernel
    ("dgrad1x1 96<-16", case_dgrad(2, 12, 12, 96, 16, 1, 1, route="low 64x128 xf0")),
    ("dgrad1x1 305<-2", case_dgrad(2, 16, 16, 305, 2, 1, 1, route="narrow 128x160 xf0")),
    ("dgrad1x1 256<-1", case_dgrad(2, 16, 16, 256, 1, 1, 1, route="narrow 128x128 xf0")),
    ("dgrad3x3 304<-256 accumulate", case_dgrad(2, 12, 12, 304, 256, 3, 1, accumulate=True, route=("ws 64x128 k3 xf0", "x3+tail 128x128 k3 full 0 tail 9x8"))),
    ("dgrad3x3 320<-256 dil6 accumulate", case_dgrad(2, 8, 8, 320, 256, 3, 6, accumulate=True, route=("ws 64x128 k3 xf0", "x3+tail 128x128 k3 full 0 tail 3x8"))),
    # wgrad
    ("wgrad1x1 16->96", case_wgrad(2, 24, 20, 16, 96, 1, 1, route="wgrad 128x32 S=3 red8")),
    ("wgrad1x1 96->24", case_wgrad(2, 17, 13, 96, 24, 1, 1, route="wgrad 32x128 S=1 red8")),
    ("wgrad1x1 32->16 (64x64 tiles)", case_wgrad(2, 16, 16, 32, 16, 1, 1, route="wgrad 64x64 S=2 red8")),
    ("wgrad1x1 960->320", case_wgrad(2, 8, 8, 960, 320, 1, 1, route="wgrad-ws 128x128 xf1 S=1 red8")),
    ("wgrad1x1 305->2 mask", case_wgrad(2, 16, 16, 305, 2, 1, 1, mask=True, route="wgrad 32x128 S=2 red8")),
    ("wgrad1x1 256->1 mask", case_wgrad(2, 16, 16, 256, 1, 1, 1, mask=True, route="wgrad 32x128 S=2 red8")),
    ("wgrad1x1 320->256 P=4", case_wgrad(4, 1, 1, 320, 256, 1, 1, lazy=False, route="wgrad-ws 128x128 xf0 S=1 red8")),
    ("wgrad3x3 304->256", case_wgrad(2, 16, 16, 304, 256, 3, 1, lazy=False, route="wgrad-ws 128x128 xf0 S=4 red8")),
    ("wgrad3x3 256->256 mask", case_wgrad(2, 16, 12, 256, 256, 3, 1, mask=True, route="wgrad-ws 128x128 xf2 S=3 red8")),
    ("wgrad3x3 320->256 dil6", case_wgrad(2, 8, 8, 320, 256, 3, 6, lazy=False, route="wgrad-ws 128x128 xf0 S=1 red8")),
    ("wgrad3x3 64->40 dil2", case_wgrad(1, 11, 9, 64, 40, 3, 2, route="wgrad-ws 128x128 xf1 S=1 red8")),
    # depthwise
    ("dw 32 s1 d1 border0", case_dw(2, 16, 16, 32, 1, 1, 0, route=("fwd tiled-8x16", "dgrad flat", "wgrad tiled-8x16"))),
    ("dw 96 s2 d1 border1", case_dw(2, 16, 16, 96, 2, 1, 1, route=("fwd tiled-8x8", "dgrad flat", "wgrad tiled-8x8"))),
    ("dw 144 s1 d1 border1 odd", case_dw(1, 13, 11, 144, 1, 1, 1, route=("fwd tiled-8x16", "dgrad flat", "wgrad tiled-8x16"))),
    ("dw 960 s1 d2 border1", case_dw(2, 8, 8, 960, 1, 2, 1, route=("fwd tiled-8x16", "dgrad flat", "wgrad tiled-8x16"))),
    ("dw 576 s1 d1 border1", case_dw(2, 8, 8, 576, 1, 1, 1, route=("fwd tiled-8x16", "dgrad flat", "wgrad tiled-8x16"))),
    # the flat forward / weight-gradient kernels with the quirk-Q1 border: MobileNetV2's dilation-4 blocks at output stride 8
    ("dw 960 s1 d4 border1 (flat: one pixel lane, 16 idle threads)", case_dw(2, 8, 8, 960, 1, 4, 1, route=("fwd flat", "dgrad flat", "wgrad flat"))),
    ("dw 64 s1 d4 border1 odd (flat: 16 pixel lanes, extents below the dilated window)",
     case_dw(1, 9, 7, 64, 1, 4, 1, route=("fwd flat", "dgrad flat", "wgrad flat"))),
    ("stem 2x3x32x32", case_stem(2, 32, 32, route=("fwd pixels", "wgrad pixels"))),
    ("stem 1x3x48x80", case_stem(1, 48, 80, route=("fwd pixels", "wgrad pixels"))),
    ("stem 2x3x20x512 (row-staged kernels: Wo = 256)", case_stem(2, 20, 512, route=("fwd rows", "wgrad rows"))),
    ("stem 1x3x7x1024 (row-staged kernels: two segments per row)", case_stem(1, 7, 1024, route=("fwd rows", "wgrad rows"))),
    ("stem 2x3x20x512 dy off 16-byte alignment (row-staged forward, per-pixel weight gradient)",
     case_stem(2, 20, 512, dy_offset=1, route=("fwd rows", "wgrad pixels"))),
    # batch norm pieces
    ("bn C=32 P=3000", case_bn(3000, 32)),
    ("bn C=96 q1", case_bn(1500, 96, q1=True)),
    ("bn C=256 mask", case_bn(700, 256, mask=True)),
    ("bn C=305 mask (C%4!=0)", case_bn(600, 305, mask=True)),
    ("bn frozen (eval-mode backward) C=96 q1 total", case_bn(1500, 96, q1=True, training=False, frozen=True)),
    ("bn frozen (eval-mode backward) C=256 mask", case_bn(700, 256, mask=True, training=False, frozen=True)),
    ("transnorm gain / eval coefficients C=305", case_transnorm(305)),
    ("transnorm gain / eval coefficients C=1280 (> one pass of the workgroup)", case_transnorm(1280, 40, 24)),
    ("bn C=1024 (concat)", case_bn(300, 1024)),
    ("bn eval C=144", case_bn(500, 144, training=False)),
    ("bn C=256 P=4", case_bn(4, 256)),
    # resampling
    ("upsample 4x4->16x16 C=256", case_resample(2, 4, 4, 16, 16, 256)),
    ("upsample 8x6->32x24 C=64", case_resample(1, 8, 6, 32, 24, 64)),
    ("upsample + stats 8x8->32x32 C=256 into 305 (+ 49-channel window)", case_upsample_stats(2, 8, 8, 32, 32, 256, 305)),
    ("mc seg head 4 x (8x8 -> 32x32) 256 + 48 + 1, batch repeated twice, mask", case_mc_seg_head(4, 8, 8, 32, 32, 256, 48, 2, True)),
    ("mc seg head 3 x (5x7 -> 20x28) 64 + 8 + 1, no repeat, no mask", case_mc_seg_head(3, 5, 7, 20, 28, 64, 8, 1, False)),
    ("mc seg head 2 x (5x9 -> 17x33) exact ratio 1/4 (last source row / column reached exactly)", case_mc_seg_head(2, 5, 9, 17, 33, 64, 8, 1, False)),
    ("mc seg head 2 x (6x6 -> 6x6) ratio 1, (3x4 -> 13x7) mixed", case_mc_seg_head(2, 6, 6, 6, 6, 64, 8, 1, True)),
    ("mc seg head 2 x (3x4 -> 13x7) 64 + 8 + 1", case_mc_seg_head(2, 3, 4, 13, 7, 64, 8, 1, False)),
    ("bn backward, low-rank dU: C=305 k=2 mask (seg head)", case_bnbwd_lowrank(3000, 305, 2, True)),
    ("bn backward, low-rank dU: C=256 k=1 mask (boundary head)", case_bnbwd_lowrank(2500, 256, 1, True)),
    ("bn backward, low-rank dU: C=40 k=2 raw", case_bnbwd_lowrank(777, 40, 2, False)),
    ("upsample + stats 5x7->20x28 C=64 into 72 (+ 8-channel window)", case_upsample_stats(3, 5, 7, 20, 28, 64, 72)),
    ("head 16x16->64x64 C=2", case_head(2, 16, 16, 64, 64, 2)),
    ("head 12x10->48x40 C=1", case_head(1, 12, 10, 48, 40, 1)),
    ("gap C=320", case_gap(3, 64, 320)),
    ("gap C=256 HW=16", case_gap(4, 16, 256)),
    ("dropout p=.5", case_dropout(4096, 256, 0.5)),
    ("dropout p=.1 C=305", case_dropout(4096, 305, 0.1)),
]


# ------------------------------------------------------------------------------------- losses / prototypes
def case_seg_loss(B, S, seed=10):
    def run(dev):
        g = gen(seed)
        K = hip()
        o = 3 * torch.randn(B, 2, S, S, generator=g)
        o[0, 0, 0, :8] = torch.tensor([40., -40., 110., -110., 17., -17., 90., -90.])    # saturating logits (log clamp)
        b = 2 * torch.randn(B, 1, S, S, generator=g)
        tm = (torch.rand(B, 2, S, S, generator=g) > 0.5).float()
        tb = torch.rand(B, 1, S, S, generator=g)
        l_r = SPEC.seg_loss_fwd(o, tm, b, tb)
        l_h = K.seg_loss_fwd(o.to(dev), tm.to(dev), b.to(dev), tb.to(dev))
        gs = torch.tensor([0.37])
        do_r, db_r = SPEC.seg_loss_bwd(o, tm, b, tb, gs)
        do_h, db_h = K.seg_loss_bwd(o.to(dev), tm.to(dev), b.to(dev), tb.to(dev), gs.to(dev))
        return max(rel(l_h, l_r), rel(do_h, do_r), rel(db_h, db_r)), 2e-5
    return run


UNDECIDED = 1e-5       # a thresholded output is decided where the float64 statement is further than this from the threshold


def case_seg_counts(B, S, seed=11, C=2, W=None, edge=False):
    """Exact counts.  The input holds no undecided element: a logit whose float64 sigmoid lies within UNDECIDED of the threshold
    is moved away by 1e-2 (asserted).  Every channel with room gets two logits just outside that band (4e-5 in probability on
    either side of the threshold, three hundred times the fp32 sigmoid's error), so that a shifted threshold shows at every
    shape.  edge: one target plane of zeros, one of ones, and fractional / tiny / negative-zero targets for the ``!= 0``."""
    W = S if W is None else W
    thr = 0.75

    def run(dev):
        g = gen(seed)
        lg = 2 * torch.randn(B, C, S, W, generator=g) + 1.0
        tg = (torch.rand(B, C, S, W, generator=g) > 0.6).float()
        flat = lg.permute(1, 0, 2, 3).reshape(C, -1)             # (copies: written back below)
        t0 = math.log(thr / (1 - thr))
        if flat.shape[1] >= 2:
            flat[:, 0], flat[:, 1] = t0 + 2e-4, t0 - 2e-4
        else:
            flat[0::2, 0], flat[1::2, 0] = t0 + 2e-4, t0 - 2e-4
        lg = flat.reshape(C, B, S, W).permute(1, 0, 2, 3).contiguous()
        if edge:
            kind = torch.randint(0, 8, tg.shape, generator=g)
            for k, v in ((0, 0.5), (1, 1e-30), (2, -0.0), (3, -1.0)):
                tg[kind == k] = v
            tg[0, 0] = 0.0
            tg[B - 1, C - 1] = 1.0
        near = (torch.sigmoid(lg.double()) - thr).abs() <= UNDECIDED
        lg[near] += 1e-2
        assert not bool(((torch.sigmoid(lg.double()) - thr).abs() <= UNDECIDED).any()), "undecided logit in the test input"
        c_r = SPEC.seg_counts(lg.double(), tg.double(), thr)
        assert torch.equal(c_r, SPEC.seg_counts(lg, tg, thr))           # (decided in float64 = decided in fp32)
        c_h = hip().seg_counts(ro_dev(lg, dev), ro_dev(tg, dev), thr)
        return float((c_h.cpu() - c_r).abs().max()), 0.0
    return run


def retrify_errors(B, h, w, lg, std_map, mean_map, w_h, m0_h, m1_h):
    """Mode 2 has two thresholded factors, sigmoid(logit) > 0.75 and bilinear(std) < 0.04.  A pixel is decided where the float64
    statement keeps all four of them (two channels each) further than UNDECIDED from the threshold.  Input condition, asserted
    here on the CPU: at most 0.5 % of the pixels are undecided.  -> [mask mismatches on decided pixels, weight error on decided
    pixels against the float64 statement]; undecided pixels are left out, the device results are taken as they are."""
    F = torch.nn.functional
    p = torch.sigmoid(lg.double()).reshape(B, h, w, 2)
    sd = F.interpolate(std_map.double(), size=(h, w), mode="bilinear", align_corners=True).permute(0, 2, 3, 1)
    und = (((p - 0.75).abs() <= UNDECIDED) | ((sd - 0.04).abs() <= UNDECIDED)).any(-1).reshape(-1)
    assert float(und.double().mean()) <= 0.005, "%d of %d pixels undecided in the test input" % (int(und.sum()), und.numel())
    dec = ~und
    w64, m0_64, m1_64 = SPEC.proto_weights(2, B, h, w, logits=lg.double(), std_map=std_map.double(), mean_map=mean_map.double())
    wrong = int((m0_h.cpu().double() != m0_64)[dec].sum() + (m1_h.cpu().double() != m1_64)[dec].sum())
    return [float(wrong), rel(w_h.cpu()[dec], w64[dec])]


def case_proto(B, h, C, mode, seed=12):
    def run(dev):
        g = gen(seed)
        K = hip()
        P = B * h * h
        feat = padded(P, C, g)
        H = 4 * h
        errs = []
        if mode == 0:
            mp = (torch.rand(B, 2, H, H, generator=g) > 0.6).float()
            w_r, _, _ = SPEC.proto_weights(0, B, h, h, map_=mp)
            w_h, _, _ = K.proto_weights(0, B, h, h, map_=mp.to(dev))
        elif mode == 1:
            lg = padded(P, 2, g, scale=2.0)
            w_r, _, _ = SPEC.proto_weights(1, B, h, h, logits=lg)
            w_h, _, _ = K.proto_weights(1, B, h, h, logits=to_dev(lg, dev))
        else:
            T = 8
            base = torch.nn.functional.avg_pool2d(2.0 * torch.randn(B, 2, H, H, generator=g), 9, 1, 4) * 6.0
            preds = base.repeat(T, 1, 1, 1) + 0.35 * torch.randn(T * B, 2, H, H, generator=g) * \
                (torch.rand(1, 2, H, H, generator=g) > 0.5).float()
            sd_r, mn_r = SPEC.mc_stats(preds, T)
            sd_h, mn_h = K.mc_stats(preds.to(dev), T)
            errs += [rel(sd_h, sd_r), rel(mn_h, mn_r)]
            lgn = torch.nn.functional.interpolate(base, size=(h, h), mode="bilinear", align_corners=True)
            lg = padded(P, 2, g)
            lg.copy_(lgn.permute(0, 2, 3, 1).reshape(P, 2))
            w_r, m0_r, m1_r = SPEC.proto_weights(2, B, h, h, logits=lg, std_map=sd_r, mean_map=mn_r)
            # the HIP weights kernel reads the reference std / mean maps: one input, one float64 statement of it
            w_h, m0_h, m1_h = K.proto_weights(2, B, h, h, logits=to_dev(lg, dev), std_map=ro_dev(sd_r, dev), mean_map=ro_dev(mn_r, dev))
            errs += retrify_errors(B, h, h, lg, sd_r, mn_r, w_h, m0_h, m1_h)
            assert 0.05 < float(m0_r.mean()) / 2 < 0.999, "degenerate mask in the test input"
        if mode != 2:
            errs.append(rel(w_h, w_r))
        s_r = torch.zeros(4, C + 1, dtype=torch.float64)
        SPEC.proto_reduce(feat, w_r, s_r)
        s_h = out_dev((4, C + 1), torch.float64, dev, fill=0)
        fh, wh = ro_dev(feat, dev), ro_dev(w_r, dev)
        K.proto_reduce(fh, wh, s_h)
        errs += [rel(s_h, s_r), rel(K.proto_finalize(s_h), SPEC.proto_finalize(s_r))]
        dC = torch.randn(4, C, generator=g)
        base = padded(P, C, g)
        df_r = base.clone()
        dw_r = SPEC.proto_bwd(feat, w_r, s_r, dC, df_r, True, True)
        df_h = to_dev(base, dev)
        dw_h = K.proto_bwd(fh, wh, s_h, dC.to(dev), df_h, True, True)
        errs += [rel(df_h, df_r), rel(dw_h, dw_r)]
        DETAIL.clear()
        DETAIL.update({"errs": ["%.1e" % e for e in errs]})
        return max(errs), 3e-5
    return run


def case_adam(n, seed=13):
    def run(dev):
        g = gen(seed)
        p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g)
        m, v = 0.1 * torch.randn(n, generator=g), torch.rand(n, generator=g) * 0.01
        ph, mh, vh = out_like(p, dev), out_like(m, dev), out_like(v, dev)
        for step in (1, 2, 7):
            SPEC.adam_step(p, gr, m, v, 1e-3, 0.9, 0.99, 1e-8, step)
            hip().adam_step(ph, ro_dev(gr, dev), mh, vh, 1e-3, 0.9, 0.99, 1e-8, step)
        ref = torch.nn.Parameter(torch.randn(n, generator=gen(seed)))
        return max(rel(ph, p), rel(mh, m), rel(vh, v)), 1e-5
    return run


def case_feat4(P, C, seed=14):
    def run(dev):
        g = gen(seed)
        K = hip()
        feat = padded(P, C, g)
        coef = torch.randn(4, C + 1, generator=g)
        o_r = SPEC.feat_dot4(feat, coef)
        o_h = K.feat_dot4(ro_dev(feat, dev), ro_dev(coef, dev))
        w = torch.randn(P, 4, generator=g)
        base = padded(P, C, g)
        d_r = base.clone()
        SPEC.feat_rank4(w, coef, d_r, True)
        d_h = to_dev(base, dev)
        K.feat_rank4(ro_dev(w, dev), ro_dev(coef, dev), d_h, True)
        return max(rel(o_h, o_r), rel(d_h, d_r)), 2e-5
    return run


CASES += [
    ("feat dot4/rank4 C=305", case_feat4(3000, 305)),
    # wide warp-specialised tiles (BN = 256 needs >= 512 workgroups: P >= 65536)
    ("conv3x3 16->256 P=65536 (BN=256 tiles) relu mask", case_conv(4, 128, 128, 16, 256, 3, 1, mask=True, route="narrow 128x128")),
    ("conv1x1 64->200 P=65536 (BN=256 tiles) bias addend", case_conv(4, 128, 128, 64, 200, 1, 1, bias=True, addend=True, route="narrow 128x128 xf1")),
    ("dgrad3x3 304<-32 P=65536 accumulate", case_dgrad(4, 128, 128, 304, 32, 3, 1, accumulate=True, route=("ws 128x320 k3 xf0", "x3 256x128 k3"))),
    ("wgrad3x3 16->256 P=65536 mask", case_wgrad(4, 128, 128, 16, 256, 3, 1, mask=True, route="wgrad-ws 128x128 xf2 S=256 red8")),
    ("seg loss 2x64", case_seg_loss(2, 64)),
    ("seg counts 3x96", case_seg_counts(3, 96)),
    ("proto hard C=305 h=32", case_proto(2, 32, 305, 0)),
    ("proto soft C=305 h=16", case_proto(2, 16, 305, 1)),
    ("proto retrify C=305 h=32", case_proto(1, 32, 305, 2)),
    ("proto hard C=64 h=8", case_proto(3, 8, 64, 0)),
    ("adam 100003", case_adam(100003)),
]


def case_discriminative(B, h, C, seed=15):
    """ops.discriminative_loss (HIP) against oracle/losses_ref.py (parity unpinned: our reading of Appendix B)."""
    def run(dev):
        from oracle import losses_ref
        from uda_clr_amd import ops
        g = gen(seed)
        feat = torch.randn(B, C, h, h, generator=g)
        cents = tuple(torch.randn(1, C, 1, 1, generator=g) for _ in range(4))
        lab = (torch.rand(B, 2, h, h, generator=g) > 0.5).float()
        f_r = feat.clone().requires_grad_(True)
        l_r = losses_ref.discriminative_loss(f_r, cents, lab)
        l_r.backward()
        f_h = feat.to(dev).requires_grad_(True)
        l_h = ops.discriminative_loss(f_h, tuple(c.to(dev) for c in cents), lab.to(dev))
        l_h.backward()
        return max(rel(l_h, l_r), rel(f_h.grad, f_r.grad)), 5e-5
    return run


CASES += [("discriminative loss (unpinned) C=305", case_discriminative(2, 16, 305))]


# ------------------------------------------------------------------ ResNet-101 pieces
def case_stem7(N, H, W, seed=16):
    def run(dev):
        g = gen(seed)
        x = torch.randn(N, 3, H, W, generator=g)
        w = torch.randn(64, 3, 7, 7, generator=g) / 12.0
        Po = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        y_r, st_r = padded(Po, 64, g), torch.zeros(16, 2, 64, dtype=torch.float64)
        SPEC.stem7_fwd(x, w, y_r, st_r)
        K = hip()
        y_h, st_h = to_dev(padded(Po, 64, g), dev), out_dev((16, 2, 64), torch.float64, dev, fill=0)
        K.stem7_fwd(ro_dev(x, dev), ro_dev(w, dev), y_h, st_h)
        dy = padded(Po, 64, g)
        dw_r, dw_h = torch.empty(64, 3, 7, 7), out_dev((64, 3, 7, 7), torch.float32, dev)
        SPEC.stem7_wgrad(x, dy, dw_r)
        K.stem7_wgrad(ro_dev(x, dev), ro_dev(dy, dev), dw_h)
        return max(rel(y_h, y_r), rel(st_h.sum(0), st_r.sum(0)), rel(dw_h, dw_r)), 3e-5
    return run


def case_maxpool(N, H, W, C, seed=17):
    def run(dev):
        g = gen(seed)
        K = hip()
        src = make_src(N, H, W, C, g, lazy=True, act=ACT_RELU)
        Po = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        z_r, i_r = padded(Po, C, g), torch.zeros(Po, round4(C), dtype=torch.uint8)[:, :C]
        SPEC.maxpool_fwd(src, z_r, i_r)
        z_h, i_h = to_dev(padded(Po, C, g), dev), out_dev((Po, round4(C)), torch.uint8, dev, fill=0, cols=C)[:, :C]
        K.maxpool_fwd(act_to(src, dev), z_h, i_h)
        dz = padded(Po, C, g)
        du_r, du_h = padded(N * H * W, C, g), to_dev(padded(N * H * W, C, g), dev)
        SPEC.maxpool_bwd(dz, i_r, N, H, W, du_r)
        K.maxpool_bwd(ro_dev(dz, dev), i_h, N, H, W, du_h)
        return max(rel(z_h, z_r), float((i_h.cpu() != i_r).sum()), rel(du_h, du_r)), 1e-6
    return run


def case_rows_stride(N, H, W, C, s, seed=18):
    def run(dev):
        g = gen(seed)
        K = hip()
        Po = N * ((H - 1) // s + 1) * ((W - 1) // s + 1)
        big, small = padded(N * H * W, C, g), padded(Po, C, g)
        o_r, o_h = padded(Po, C, g), to_dev(padded(Po, C, g), dev)
        SPEC.rows_stride(big, N, H, W, s, o_r)
        K.rows_stride(ro_dev(big, dev), N, H, W, s, o_h)
        f_r, f_h = padded(N * H * W, C, g), to_dev(padded(N * H * W, C, g), dev)
        SPEC.rows_stride(small, N, H, W, s, f_r, scatter=True)
        K.rows_stride(ro_dev(small, dev), N, H, W, s, f_h, scatter=True)
        return max(rel(o_h, o_r), rel(f_h, f_r)), 0.0
    return run


def case_bottleneck_tail(N, H, W, C, seed=19):
    def run(dev):
        g = gen(seed)
        K = hip()
        a = make_src(N, H, W, C, g, lazy=True, act=ACT_NONE)
        errs = []
        for lazy_b in (False, True):
            b = make_src(N, H, W, C, g, lazy=lazy_b, act=ACT_NONE)
            z_r, z_h = padded(a.P, C, g), to_dev(padded(a.P, C, g), dev)
            SPEC.bn_add_relu(a, b, z_r)
            K.bn_add_relu(act_to(a, dev), act_to(b, dev), z_h)
            errs.append(rel(z_h, z_r))
        dz = padded(a.P, C, g)
        g_r, g_h = padded(a.P, C, g), to_dev(padded(a.P, C, g), dev)
        SPEC.relu_gate(dz, z_r, g_r)
        K.relu_gate(ro_dev(dz, dev), ro_dev(z_r, dev), g_h)
        errs.append(rel(g_h, g_r))
        return max(errs), 1e-6
    return run


CASES += [
    ("stem7 2x3x32x32", case_stem7(2, 32, 32)),
    ("stem7 1x3x48x80", case_stem7(1, 48, 80)),
    ("maxpool 2x16x16 C=64", case_maxpool(2, 16, 16, 64)),
    ("maxpool 1x24x40 C=64", case_maxpool(1, 24, 40, 64)),
    ("rows stride 2 C=256", case_rows_stride(2, 16, 16, 256, 2)),
    ("rows stride 2 C=128 8x12", case_rows_stride(1, 8, 12, 128, 2)),
    ("bottleneck tail C=256", case_bottleneck_tail(2, 16, 16, 256)),
    ("bottleneck tail C=2048", case_bottleneck_tail(2, 4, 4, 2048)),
    ("conv1x1 2048->512 (ResNet layer4)", case_conv(2, 8, 8, 2048, 512, 1, 1, route=("ws 64x128 k1 xf1", "x3 128x128 k1"))),
    ("conv3x3 512->512 dil4 (ResNet layer4)", case_conv(2, 8, 8, 512, 512, 3, 4, route=("ws 64x128 k3 xf1", "x3 128x128 k3"))),
    ("conv3x3 2048->256 dil6 (ResNet ASPP)", case_conv(2, 8, 8, 2048, 256, 3, 6, lazy=False, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("dgrad1x1 1024<-256", case_dgrad(2, 8, 8, 1024, 256, 1, 1, accumulate=True, route=("ws 64x128 k1 xf0", "x3 128x128 k1"))),
    ("wgrad1x1 1024->2048", case_wgrad(2, 8, 8, 1024, 2048, 1, 1, route="wgrad-ws 128x128 xf1 S=1 red8")),
    ("wgrad3x3 2048->256 dil6", case_wgrad(2, 8, 8, 2048, 256, 3, 6, lazy=False, route="wgrad-ws 128x128 xf0 S=1 red8")),
]

# 256-pixel workgroup tiles of the wide-tile kernel (taken when >= 512 of them exist: P >= 131072 at Cout = 256)
CASES += [
    ("conv3x3 32->256 P=131580 (256x256 tiles, ragged) relu mask", case_conv(2, 255, 258, 32, 256, 3, 1, mask=True, route=("ws 128x128 k3 xf2", "x3 128x256 k3"))),
    ("conv1x1 200->256 P=131072 (256x256 tiles) bias addend", case_conv(2, 256, 256, 200, 256, 1, 1, bias=True, addend=True, route="ws 256x256 k1 xf1")),
    ("conv3x3 24->250 P=131072 dil2 (256x256 tiles) raw", case_conv(2, 256, 256, 24, 250, 3, 2, lazy=False, route="narrow 128x128 pipe")),
]


# 2x2 taps (the space-to-depth form of the discriminators' 4x4 stride-2 convs, GAN.py:90-101)
CASES += [
    ("conv2x2 o0 8->64 (narrow) raw", case_conv(2, 18, 18, 8, 64, 2, 1, lazy=False, origin=0, route="low 64x64")),
    ("conv2x2 o0 256->128 (wide)", case_conv(2, 19, 17, 256, 128, 2, 1, lazy=False, origin=0, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("conv2x2 o1 128->256 (wide, dgrad form) addend", case_conv(2, 19, 17, 128, 256, 2, 1, lazy=False, addend=True, origin=1, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("conv2x2 o0 2048->1", case_conv(2, 9, 9, 2048, 1, 2, 1, lazy=False, origin=0, route="low 64x64 pipe")),
    ("wgrad2x2 o0 8->64", case_wgrad(2, 18, 18, 8, 64, 2, 1, lazy=False, origin=0, route="wgrad 64x64 S=2 red8")),
    ("wgrad2x2 o0 256->128", case_wgrad(2, 19, 17, 256, 128, 2, 1, lazy=False, origin=0, route="wgrad-ws 128x128 xf0 S=5 red8")),
    ("wgrad2x2 o0 2048->1", case_wgrad(2, 9, 9, 2048, 1, 2, 1, lazy=False, origin=0, route="wgrad 32x128 S=1 red8")),
]


def case_s2d(N, H, W, C, nchw, vh=None, vw=None, seed=20, capped=False):
    vh_, vw_ = vh or H, vw or W
    Hz, Wz = (vh_ + 5) // 2, (vw_ + 5) // 2
    v4 = not nchw and C % 4 == 0        # (padded() rows are 16-byte aligned with a row stride that is a multiple of 4)
    caps = [None, None]
    if capped and v4:                   # 4 channels per thread: z is [Pz, 4C] in groups of 4, the source side [P, C] in groups of 4
        caps = [Capped("s2d_fwd4_kernel", "S2D_MAX_WG", N * Hz * Wz * C, 256, by_group(4 * C)),
                Capped("s2d_bwd4_kernel", "S2D_MAX_WG", N * H * W * (C // 4), 256, by_group(C))]
    elif capped:                        # one element per thread; an NCHW destination is compared flat, in the kernel's own order
        caps = [Capped("s2d_fwd_kernel", "S2D_MAX_WG", N * Hz * Wz * 4 * C, 256, by_element(4 * C)),
                Capped("s2d_bwd_kernel", "S2D_MAX_WG", N * H * W * C, 256, by_element(1 if nchw else C))]

    def run(dev):
        g = gen(seed)
        K = hip()
        src = torch.randn(N, C, H, W, generator=g) if nchw else padded(N * H * W, C, g)
        z_r, z_h = padded(N * Hz * Wz, 4 * C, g), to_dev(padded(N * Hz * Wz, 4 * C, g), dev)
        SPEC.s2d_fwd(src, nchw, N, H, W, C, vh_, vw_, 0.2, z_r)
        K.s2d_fwd(ro_dev(src, dev), nchw, N, H, W, C, vh_, vw_, 0.2, z_h)
        errs = [rel_at(z_h, z_r, 0.0, caps[0])]
        dz = torch.randn(N * Hz * Wz, 4 * C, generator=g)
        zs = torch.randn(N * Hz * Wz, 4 * C, generator=g)
        for sign in (None, zs):
            if nchw:
                d_r, d_h = torch.empty(N, C, H, W), out_dev((N, C, H, W), torch.float32, dev)
            else:
                d_r, d_h = padded(N * H * W, C, g), to_dev(padded(N * H * W, C, g), dev)
            SPEC.s2d_bwd(dz, sign, 0.2, N, H, W, C, vh_, vw_, d_r, nchw)
            K.s2d_bwd(ro_dev(dz, dev), ro_dev(sign, dev), 0.2, N, H, W, C, vh_, vw_, d_h, nchw)
            errs.append(rel_at(d_h, d_r, 0.0, caps[1]))
        return max(errs), 0.0
    run.capped = caps if capped else []
    return run


CASES += [
    ("s2d nchw C=1 32x32", case_s2d(2, 32, 32, 1, True)),
    ("s2d nchw C=2 30x34", case_s2d(2, 30, 34, 2, True)),
    ("s2d rows C=64 grid 18x18 valid 17x17", case_s2d(2, 18, 18, 64, False, 17, 17)),
    ("s2d rows C=6 grid 11x9 valid 9x8 (scalar path)", case_s2d(1, 11, 9, 6, False, 9, 8)),
]


def case_s2d_packed(N, H, W, C, vh=None, vw=None, seed=22):
    """bf16x3 mode: the packed space-to-depth operands written in ONE pass (uda_x3_pack_s2d_fwd / _bwd, round 3) are bit-identical
    to the two-pass forms they replace (uda_s2d_fwd / uda_s2d_bwd + uda_x3_pack: the split is exact), and the gate read from the
    sign of the forward's source rows equals the gate read from the sign of z = lrelu(source)."""
    def run(dev):
        g = gen(seed)
        K = hip()
        vh_, vw_ = vh or H, vw or W
        Hz, Wz = (vh_ + 5) // 2, (vw_ + 5) // 2
        src = to_dev(padded(N * H * W, C, g), dev)
        src[::7] = 0.0                                   # exact zeros: lrelu(0) = 0 is "not positive" for both kinds of gate
        z = to_dev(padded(N * Hz * Wz, 4 * C, g), dev)
        K.s2d_fwd(src, False, N, H, W, C, vh_, vw_, 0.2, z)
        za = Act(z, N, Hz, Wz)
        want = K.x3_pack(K._src(za), za.P, za.C, dev)
        got = K.s2d_pack_fwd(src, N, H, W, C, vh_, vw_, 0.2)
        body = lambda t, rows, ch: t[:rows * ((ch + 15) // 16) * 96]          # (uda_x3_packed_bytes adds 64 bytes that nobody writes)
        bad = int((body(got._x3, za.P, za.C) != body(want, za.P, za.C)).sum())
        dz = to_dev(padded(N * Hz * Wz, 4 * C, g), dev)
        d_z, d_g = to_dev(padded(N * H * W, C, g), dev), to_dev(padded(N * H * W, C, g), dev)
        K.s2d_bwd(dz, z, 0.2, N, H, W, C, vh_, vw_, d_z, False)
        K.s2d_bwd(dz, None, 0.2, N, H, W, C, vh_, vw_, d_g, False, gate=src)
        bad += int((d_z != d_g).sum())
        da = Act(d_g, N, H, W)
        want_b = K.x3_pack(K._src(da), da.P, da.C, dev)
        got_b = K.s2d_pack_bwd(dz, src, 0.2, N, H, W, C, vh_, vw_)
        bad += int((body(got_b._x3, da.P, da.C) != body(want_b, da.P, da.C)).sum())
        got_n = K.s2d_pack_bwd(dz, None, 0.2, N, H, W, C, vh_, vw_)          # no gate (slope irrelevant)
        K.s2d_bwd(dz, None, 1.0, N, H, W, C, vh_, vw_, d_z, False)
        dn = Act(d_z, N, H, W)
        bad += int((body(got_n._x3, dn.P, dn.C) != body(K.x3_pack(K._src(dn), dn.P, dn.C, dev), dn.P, dn.C)).sum())
        return float(bad), 0.0
    return run


CASES += [
    ("s2d packed C=64 grid 18x18 valid 17x17", case_s2d_packed(2, 18, 18, 64, 17, 17)),
    ("s2d packed C=128 grid 35x35 valid 33x33", case_s2d_packed(3, 35, 35, 128, 33, 33)),
    ("s2d packed C=8 grid 11x9 valid 9x8 (half-filled 16-blocks)", case_s2d_packed(1, 11, 9, 8, 9, 8)),
    ("s2d packed C=72 grid 10x12 (4C = 288, ragged tiles)", case_s2d_packed(2, 10, 12, 72)),
]


def _k_row(chan, taps):
    """floats of one row of a relayouted weight (uda_k_row / uda_relayout_s2d): channels padded to 4, from 32 on tap-chunked in 32s"""
    Kc = round4(chan)
    return Kc if taps == 1 else (taps * Kc if Kc < 32 else -(-Kc // 32) * taps * 32)


def case_relayout_s2d(O, C, seed=21, capped=False):
    """capped: both operands run past the cap.  The dgrad operand's 4C rows of a multiple of 128 floats are always a multiple of 256
    work items; the forward operand (O rows) is shaped not to be."""
    caps = [Capped("relayout_s2d_kernel (forward operand)", "RELAYOUT_S2D_MAX_WG", O * _k_row(4 * C, 4), 256, by_element(1)),
            Capped("relayout_s2d_kernel (dgrad operand)", "RELAYOUT_S2D_MAX_WG", 4 * C * _k_row(O, 4), 256, by_element(1),
                   whole="4C rows of a multiple of 128 floats")] if capped else [None, None]

    def run(dev):
        w = torch.randn(O, C, 4, 4, generator=gen(seed))
        K = hip()
        return max(rel_at(K.relayout_s2d(w.to(dev), False), SPEC.relayout_s2d(w, False), 0.0, caps[0]),
                   rel_at(K.relayout_s2d(w.to(dev), True), SPEC.relayout_s2d(w, True), 0.0, caps[1])), 0.0
    run.capped = caps if capped else []
    return run


def case_relayout(O, I, k, seed=23, capped=False):
    """uda_relayout_ohwi / uda_relayout_dgrad on their own (the dense cases compare them at widths of one pass)"""
    caps = [Capped("relayout_ohwi_kernel", "RELAYOUT_MAX_WG", O * _k_row(I, k * k), 256, by_element(1)),
            Capped("relayout_dgrad_kernel", "RELAYOUT_MAX_WG", I * _k_row(O, k * k), 256, by_element(1))] if capped else [None, None]

    def run(dev):
        w = torch.randn(O, I, k, k, generator=gen(seed))
        K = hip()
        wh = ro_dev(w, dev)
        return max(rel_at(K.relayout_ohwi(wh), SPEC.relayout_ohwi(w), 0.0, caps[0]),
                   rel_at(K.relayout_dgrad(wh), SPEC.relayout_dgrad(w), 0.0, caps[1])), 0.0
    run.capped = caps if capped else []
    return run


CASES += [("relayout s2d 64<-2", case_relayout_s2d(64, 2)), ("relayout s2d 128<-64", case_relayout_s2d(128, 64)),
          ("relayout s2d 1<-512", case_relayout_s2d(1, 512))]

# 256 x 256 weight-gradient tiles (Cout >= 192, J >= 256, >= 4096 pixel chunks = 131072 pixels)
CASES += [
    ("wgrad3x3 32->256 P=131072 (256x256 tiles)", case_wgrad(2, 256, 256, 32, 256, 3, 1, lazy=False, route=("wgrad-ws 256x256 xf0 S=256 red8", "wgrad-x3 256x256 S=256 red8"))),
    ("wgrad3x3 40->200 P=131325 mask (256x256 tiles, ragged)", case_wgrad(1, 255, 515, 40, 200, 3, 2, mask=True, route="wgrad-ws 256x256 xf2 S=242 red8")),
    ("wgrad1x1 300->320 P=131072 lazy (256x256 tiles)", case_wgrad(2, 256, 256, 300, 320, 1, 1, route="wgrad-ws 256x256 xf1 S=128 red8")),
    ("wgrad2x2 o0 64->256 P=131841 (256x256 tiles)", case_wgrad(1, 363, 363, 64, 256, 2, 1, lazy=False, route=("wgrad-ws 256x256 xf0 S=243 red8", "wgrad-x3 256x256 S=243 red8"))),
]

# weight gradients the bf16x3 mode routes to its own kernel (Cin % 16 == 0, Cout >= 96, k >= 2, P >= 4096; transposed LDS reads)
CASES += [
    ("wgrad3x3 256->256 P=4608 mask (x3 128 tiles)", case_wgrad(2, 48, 48, 256, 256, 3, 1, mask=True, route=("wgrad-ws 128x128 xf2 S=24 red8", "wgrad-x3 128x256 S=24 red8"))),
    ("wgrad3x3 304->256 P=8192 (x3 128 tiles)", case_wgrad(2, 64, 64, 304, 256, 3, 1, lazy=False, route=("wgrad-ws 128x128 xf0 S=22 red8", "wgrad-x3 256x256 S=22 red8"))),
    ("wgrad3x3 320->256 dil12 P=4608 (x3)", case_wgrad(2, 48, 48, 320, 256, 3, 12, route=("wgrad-ws 128x128 xf1 S=21 red8", "wgrad-x3 128x256 S=21 red8"))),
    ("wgrad3x3 48->100 P=4700 ragged (x3)", case_wgrad(2, 50, 47, 48, 100, 3, 1, route=("wgrad-ws 128x128 xf1 S=30 red8", "wgrad-x3 128x256 S=30 red8"))),
    ("wgrad2x2 o0 256->128 P=8978 (x3)", case_wgrad(2, 67, 67, 256, 128, 2, 1, lazy=False, origin=0, route=("wgrad-ws 128x128 xf0 S=57 red8", "wgrad-x3 128x256 S=57 red8"))),
    ("wgrad2x2 o0 64->200 P=70225 (x3 256 tiles, ragged)", case_wgrad(1, 265, 265, 64, 200, 2, 1, lazy=False, origin=0, route=("wgrad-ws 128x128 xf0 S=244 red8", "wgrad-x3 256x256 S=244 red8"))),
    ("wgrad1x1 256->2304 P=4608 (x3, tap GEMM of the re-associated decoder conv)", case_wgrad(2, 48, 48, 256, 2304, 1, 1, lazy=False, route=("wgrad-ws 128x128 xf0 S=24 red8", "wgrad-x3 128x256 S=24 red8"))),
    ("wgrad2x2 o0 1024->512 P=9248 (x3 256 tiles on few pixels)", case_wgrad(2, 68, 68, 1024, 512, 2, 1, lazy=False, origin=0, route=("wgrad-ws 128x128 xf0 S=8 red8", "wgrad-x3 256x256 S=8 red8"))),
]
# bf16x3: the last, partly filled round of tiles split over K (no statistics epilogue; fp32 partial tiles + x3_tail_reduce_kernel)
CASES += [
    ("conv3x3 64->128 P=37965 bias addend, no stats (x3 tail split, ragged rows)", case_conv(1, 195, 195 - 0, 64, 128, 3, 1, bias=True, addend=True, stats=False, route=("ws 128x128 k3 xf1", "x3 256x128 k3"))),
    ("conv2x2 o1 256->250 P=38000 raw, no stats (x3 tail split, ragged columns)", case_conv(1, 200, 190, 256, 250, 2, 1, lazy=False, stats=False, origin=1, route=("ws 128x128 k3 xf0", "x3 128x128 k3"))),
    ("conv1x1 256->2304 P=4864 no stats (x3 tail split, wide 1x1)", case_conv(1, 38, 128, 256, 2304, 1, 1, lazy=False, stats=False, route=("ws 128x192 k1 xf0", "x3 128x128 k1"))),
    ("dgrad3x3 304<-256 P=37888 accumulate (x3 tail split)", case_dgrad(2, 148, 128, 304, 256, 3, 1, accumulate=True, route=("ws 128x128 k3 xf0", "x3 256x128 k3"))),
]
# bf16x3 routes added with the 256 x 64 tile and the wide 1x1 route
CASES += [
    ("conv1x1 256->2304 stats (x3 wide 1x1)", case_conv(2, 40, 36, 256, 2304, 1, 1, lazy=False, route=("ws 128x256 k1 xf0", "x3 128x256 k1"))),
    ("conv1x1 144->1030 relu6 ragged (x3 wide 1x1)", case_conv(1, 37, 29, 144, 1030, 1, 1, route="narrow 128x96 xf1")),
    ("conv3x3 256->48 P=2442 ragged (x3 256 x 64 tile)", case_conv(2, 33, 37, 256, 48, 3, 1, lazy=False, route=("low 64x64 pipe", "x3 256x64 k3"))),
    ("conv3x3 160->60 dil2 mask stats (x3 256 x 64 tile)", case_conv(1, 45, 41, 160, 60, 3, 2, mask=True, route=("low 64x64 pipe", "x3 256x64 k3"))),
    ("conv2x2 o1 256->56 addend (x3 256 x 64 tile)", case_conv(2, 30, 30, 256, 56, 2, 1, lazy=False, addend=True, origin=1, route="low 64x64 pipe")),
]
# narrow 1x1 convs: 64-pixel tiles when 128-pixel tiles would leave half of the CUs without a workgroup (the 32x32-map layers at
# B = 16: P = 16384), and the 128-pixel tiles of the same routes on more pixels (round 3)
CASES += [
    ("conv1x1 384->64 P=16384 relu6 stats (64-pixel tiles)", case_conv(16, 32, 32, 384, 64, 1, 1, route="low 64x64 pipe xf1")),
    ("conv1x1 576->96 P=16384 addend no stats (64-pixel tiles, 128 columns)", case_conv(16, 32, 32, 576, 96, 1, 1, addend=True, stats=False, route="low 64x128 pipe xf1")),
    ("conv1x1 192->30 P=5655 ragged mask bias (64-pixel tiles)", case_conv(3, 65, 29, 192, 30, 1, 1, mask=True, bias=True, route="low 64x64 pipe")),
    ("dgrad1x1 64<-384 P=16384 accumulate (64-pixel tiles)", case_dgrad(16, 32, 32, 64, 384, 1, 1, accumulate=True, route="low 64x64 pipe xf0")),
    ("conv1x1 384->64 P=32000 ragged stats (128-pixel tiles)", case_conv(2, 125, 128, 384, 64, 1, 1, route="narrow 128x64 pipe xf1")),
    ("conv1x1 96->24 P=40000 raw addend (128-pixel tiles)", case_conv(1, 200, 200, 96, 24, 1, 1, lazy=False, addend=True, route="narrow 128x32 xf0")),
    ("conv1x1 64->96 P=28900 relu6 mask (128-pixel tiles)", case_conv(1, 170, 170, 64, 96, 1, 1, mask=True, route="narrow 128x96")),
]
# bf16x3 on long-K 1x1 convs towards >= 256 outputs (ResNet-101's bottleneck convs on the 32x32 maps, round 3)
CASES += [
    ("conv1x1 1024->256 P=8192 raw stats (x3 long-K 1x1)", case_conv(8, 32, 32, 1024, 256, 1, 1, lazy=False, route=("ws 64x128 k1 xf0", "x3 128x128 k1"))),
    ("conv1x1 2048->512 P=2312 relu ragged (x3 long-K 1x1)", case_conv(2, 34, 34, 2048, 512, 1, 1, route=("ws 64x128 k1 xf1", "x3 128x128 k1"))),
    ("dgrad1x1 1024<-256 P=8192 accumulate (x3 wide 1x1)", case_dgrad(8, 32, 32, 1024, 256, 1, 1, accumulate=True, route=("ws 128x256 k1 xf0", "x3 128x256 k1"))),
    ("wgrad1x1 1024->256 P=8192 raw (x3 long-K 1x1)", case_wgrad(8, 32, 32, 1024, 256, 1, 1, lazy=False, route=("wgrad-ws 128x128 xf0 S=64 red8", "wgrad-x3 256x256 S=64 red8"))),
    ("wgrad1x1 2048->512 P=4624 relu (x3 long-K 1x1)", case_wgrad(4, 34, 34, 2048, 512, 1, 1, route=("wgrad-ws 128x128 xf1 S=15 red8", "wgrad-x3 128x256 S=15 red8"))),
]
# short-K 1x1 convs over >= 32768 pixels: the barrier-free one-wave-per-32-pixels kernel (conv1x1_stream_kernel)
CASES += [
    ("conv1x1 16->96 P=33800 relu6 stats (stream kernel, ragged last tile)", case_conv(2, 130, 130, 16, 96, 1, 1, route="stream 8x3")),
    ("conv1x1 16->90 P=33800 raw addend no stats (stream kernel, ragged columns)", case_conv(2, 130, 130, 16, 90, 1, 1, lazy=False, addend=True, stats=False, route="stream 8x3")),
    ("conv1x1 24->144 P=40000 raw addend (stream kernel, two column groups)", case_conv(1, 200, 200, 24, 144, 1, 1, lazy=False, addend=True, route="stream 12x5")),
    ("conv1x1 24->48 P=36100 relu stats (stream kernel)", case_conv(1, 190, 190, 24, 48, 1, 1, route="stream 12x2")),
    ("conv1x1 32->192 P=36300 relu stats addend (stream kernel, two column groups)", case_conv(3, 110, 110, 32, 192, 1, 1, addend=True, route="narrow 128x96 xf1")),
    ("conv1x1 32->130 P=32768 raw (stream kernel, second group ragged)", case_conv(2, 128, 128, 32, 130, 1, 1, lazy=False, route="narrow 128x160 xf0")),
    ("conv1x1 32->192 P=262144 relu6 stats (stream kernel, two column groups)", case_conv(4, 256, 256, 32, 192, 1, 1, route="stream 16x3")),
    ("conv1x1 16->32 P=33800 raw addend (stream kernel, one block)", case_conv(2, 130, 130, 16, 32, 1, 1, lazy=False, addend=True, stats=False, route="stream 8x1")),
    ("conv1x1 24->96 P=40000 raw addend (stream kernel, three blocks)", case_conv(1, 200, 200, 24, 96, 1, 1, lazy=False, addend=True, stats=False, route="stream 12x3")),
]
# stride 2 on the wide tiles: the loaders walk the strided output grid (ResNet-101 layer2.0 / layer3.0 conv2, resnet.py:66, and their
# weight gradients; the 1x1 form is the shortcut conv, resnet.py:93)
CASES += [
    ("conv3x3 s2 128->128 65x67 relu stats (strided grid, odd sizes)", case_conv(2, 65, 67, 128, 128, 3, 1, stride=2, route=("ws 64x128 k3 xf1", "x3 128x128 k3"))),
    ("conv3x3 s2 256->256 P=8192 raw addend no stats (tail split)", case_conv(8, 64, 64, 256, 256, 3, 1, lazy=False, addend=True, stats=False, stride=2, route=("ws 64x128 k3 xf0", "x3+tail 128x256 k3 full 0 tail 64x4"))),
    ("conv3x3 s2 dil2 160->200 mask ragged", case_conv(3, 41, 38, 160, 200, 3, 2, mask=True, stride=2, route=("ws 64x128 k3 xf2", "x3 128x128 k3"))),
    ("conv1x1 s2 256->512 33x40 relu bias", case_conv(2, 33, 40, 256, 512, 1, 1, bias=True, stride=2, route="ws 64x128 k1 xf1")),
    ("conv1x1 s2 512->1024 raw (x3 wide 1x1)", case_conv(2, 64, 64, 512, 1024, 1, 1, lazy=False, stride=2, route=("ws 64x128 k1 xf0", "x3 128x128 k1"))),
    ("wgrad3x3 s2 128->128 65x67 relu", case_wgrad(2, 65, 67, 128, 128, 3, 1, stride=2, route="wgrad-ws 128x128 xf1 S=15 red8")),
    ("wgrad3x3 s2 256->256 P=16384 raw (x3)", case_wgrad(4, 128, 128, 256, 256, 3, 1, lazy=False, stride=2, route=("wgrad-ws 128x128 xf0 S=27 red8", "wgrad-x3 256x256 S=27 red8"))),
    ("wgrad3x3 s2 128->128 41 images of 20x20 (rows shorter than a chunk)", case_wgrad(41, 20, 20, 128, 128, 3, 1, stride=2, route=("wgrad-ws 128x128 xf1 S=26 red8", "wgrad-x3 128x256 S=26 red8"))),
    ("wgrad1x1 s2 256->512 33x40 mask", case_wgrad(2, 33, 40, 256, 512, 1, 1, mask=True, stride=2, route="wgrad-ws 128x128 xf2 S=5 red8")),
]


# Routes that no case above takes (tests/test_conv_plan_cpu.py holds every entry of uda_conv_route_list() against the declared
# routes): the bf16x3 K-split of the last round of tiles on each tile shape - alone, after full rounds, with ragged rows and
# columns, on a long-K 1x1 conv and as an accumulating input gradient - and the remaining tiles of the other families
CASES += [
    ("conv3x3 256->256 P=1152 bias addend, no stats", case_conv(2, 24, 24, 256, 256, 3, 1, bias=True, addend=True, stats=False, route=("ws 64x128 k3 xf1", "x3+tail 128x128 k3 full 0 tail 18x8"))),
    ("conv2x2 o1 384->250 P=1147 raw, no stats, ragged rows and columns", case_conv(1, 37, 31, 384, 250, 2, 1, lazy=False, stats=False, origin=1, route=("ws 64x128 k3 xf0", "x3+tail 128x128 k3 full 0 tail 18x8"))),
    ("conv1x1 1536->300 P=1147 relu, no stats", case_conv(1, 37, 31, 1536, 300, 1, 1, stats=False, route=("ws 64x128 k1 xf1", "x3+tail 128x128 k1 full 0 tail 27x8"))),
    ("dgrad3x3 304<-256 P=1152 accumulate", case_dgrad(2, 24, 24, 304, 256, 3, 1, accumulate=True, route=("ws 64x128 k3 xf0", "x3+tail 128x128 k3 full 0 tail 27x8"))),
    ("conv3x3 256->256 P=16637 raw, no stats", case_conv(1, 131, 127, 256, 256, 3, 1, lazy=False, stats=False, route=("ws 128x256 k3 xf0", "x3+tail 128x128 k3 full 256 tail 4x8"))),
    ("conv2x2 o1 384->300 P=3811 raw addend, no stats", case_conv(1, 37, 103, 384, 300, 2, 1, lazy=False, addend=True, stats=False, origin=1, route=("ws 64x128 k3 xf0", "x3+tail 256x128 k3 full 0 tail 45x5"))),
    ("conv2x2 o1 384->500 P=37201 raw, no stats", case_conv(1, 193, 193, 384, 500, 2, 1, lazy=False, stats=False, origin=1, route=("ws 128x128 k3 xf0", "x3+tail 256x256 k3 full 256 tail 36x7"))),
    ("conv2x2 o0 64->160 P=49729 relu stats", case_conv(1, 223, 223, 64, 160, 2, 1, route=("ws 128x192 k3 xf1", "x3 256x256 k3"))),
    ("conv2x2 o0 256->1 bias raw, no stats", case_conv(2, 9, 7, 256, 1, 2, 1, lazy=False, bias=True, stats=False, route="cout1 4x1")),
    ("conv1x1 196->160 P=12285 relu6 stats", case_conv(3, 65, 63, 196, 160, 1, 1, route="few 64x192 pipe xf1")),
    ("conv1x1 200->300 P=12285 relu mask addend", case_conv(3, 65, 63, 200, 300, 1, 1, mask=True, addend=True, route="few 64x320 pipe")),
    ("wgrad1x1 128->1024 P=4096 raw", case_wgrad(1, 64, 64, 128, 1024, 1, 1, lazy=False, route=("wgrad-ws 128x128 xf0 S=32 red8", "wgrad-x3 128x128 S=32 red8"))),
]


# ---------------------------------------------------------------- input pipeline tail: bit-exact against scipy
def _fundus_like(B, H, W, g):
    """uint8 image + grey-coded mask (255 background, 128 disc rim, 0 cup) with ellipses that touch the border in one sample."""
    import numpy as np
    rs = np.random.RandomState(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
    img = rs.randint(0, 256, (B, H, W, 3)).astype(np.uint8)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    lab = np.full((B, H, W), 255, np.uint8)
    for b in range(B):
        cy, cx = (0.15 if b == 0 else rs.uniform(0.35, 0.65)) * H, rs.uniform(0.35, 0.65) * W
        a, c = rs.uniform(0.2, 0.35) * H, rs.uniform(0.2, 0.35) * W
        r = np.sqrt(((yy - cy) / a) ** 2 + ((xx - cx) / c) ** 2)
        lab[b][r <= 1.0] = 128
        lab[b][r <= rs.uniform(0.4, 0.7)] = 0
        lab[b][rs.rand(H, W) < 0.002] = rs.choice([0, 60, 128, 200, 201, 255])      # isolated pixels, threshold values 50/51/200/201
        lab[b][0, :7] = 50
        lab[b][-1, -9:] = 51
    return img, lab


def case_normalize_tf(B, H, W, seed=41):
    """uda_normalize_tf against the reference's own per-sample arithmetic (custom_transforms.py:414-466: numpy + scipy.ndimage)."""
    def run(dev):
        import numpy as np
        from scipy import ndimage
        g = gen(seed)
        img, lab = _fundus_like(B, H, W, g)
        K = hip()
        image, mp, bd = K.normalize_tf(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev))
        worst = 0.0
        for b in range(B):
            ri = img[b].astype(np.float32)
            ri /= 127.5
            ri -= 1.0
            cup, disc = (lab[b] <= 50).astype(np.float64), (lab[b] <= 200).astype(np.float64)
            ring = np.zeros((H, W), bool)
            for m in (cup, disc):
                d = ndimage.binary_dilation(m, iterations=5).astype(m.dtype)
                e = ndimage.binary_erosion(m, iterations=5).astype(m.dtype)
                s = d + e
                s[s == 2] = 0
                ring |= s > 0
            rb = ndimage.gaussian_filter(ring.astype(np.uint8) * 255, sigma=3) / 255.0
            exact = (torch.equal(image[b].cpu(), torch.from_numpy(ri.transpose(2, 0, 1).copy())) and
                     torch.equal(mp[b].cpu(), torch.from_numpy(np.stack([cup, disc])).float()) and
                     torch.equal(bd[b, 0].cpu(), torch.from_numpy(rb).float()))
            worst = max(worst, 0.0 if exact else 1.0)
        return worst, 0.5          # bit-exact or fail
    return run


def case_elastic(B, H, W, seed=43):
    """uda_field_smooth + uda_elastic_warp against scipy (custom_transforms.py:95-147) on numpy's own uniform draw: the float64
    displacement field and the warped bytes are both bit-identical."""
    def run(dev):
        import numpy as np
        from scipy import ndimage
        g = gen(seed)
        img, lab = _fundus_like(B, H, W, g)
        rs = np.random.RandomState(7)
        alpha, sigma = 2.0 * W, 0.08 * W
        noise = np.stack([[rs.rand(H, W) * 2 - 1 for _ in range(B)] for _ in range(2)])
        K = hip()
        fld = K.field_smooth(torch.from_numpy(noise).to(dev), sigma, alpha)
        ref_f = np.stack([[ndimage.gaussian_filter(noise[q, b], sigma, mode="constant", cval=0) * alpha
                           for b in range(B)] for q in range(2)])
        bad = int((fld.cpu().numpy() != ref_f).sum())
        apply = torch.tensor([1] * (B - 1) + [0], dtype=torch.uint8)
        io, lo = K.elastic_warp(torch.from_numpy(img).to(dev), torch.from_numpy(lab).to(dev), fld[0], fld[1], apply.to(dev))
        gx, gy = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        for b in range(B):
            if not apply[b]:
                bad += int((io[b].cpu().numpy() != img[b]).sum() + (lo[b].cpu().numpy() != lab[b]).sum())
                continue
            idx = np.reshape(gx + ref_f[0, b], (-1, 1)), np.reshape(gy + ref_f[1, b], (-1, 1))
            ri = np.stack([ndimage.map_coordinates(img[b][:, :, c], idx, order=1).reshape(H, W) for c in range(3)], -1)
            rl = ndimage.map_coordinates(lab[b], idx, order=1, mode="nearest").reshape(H, W)
            bad += int((io[b].cpu().numpy() != ri).sum() + (lo[b].cpu().numpy() != rl).sum())
        return float(bad), 0.5       # bit-exact or fail
    return run


CASES += [
    ("normalize_tf 3 x 96 x 80 vs scipy (bit-exact)", case_normalize_tf(3, 96, 80)),
    ("normalize_tf 2 x 512 x 512 vs scipy (bit-exact)", case_normalize_tf(2, 512, 512)),
    ("elastic field + warp 3 x 96 x 80 vs scipy (bit-exact)", case_elastic(3, 96, 80)),
    ("elastic field + warp 2 x 256 x 256 vs scipy (bit-exact)", case_elastic(2, 256, 256)),
]


# ---------------------------------------------------------------- upsample-then-conv3x3 by low-resolution tap GEMMs + interpolation
def upconv_routes(K, q):
    """("fwd <kernel>", "bwd <kernel>") the library plans for an upconv case's two calls, from its recorded arguments
    (``run.upconv_query``) alone - no GPU needed"""
    fwd = K.upconv_route("fwd", q["N"], q["h"], q["w"], q["H"], q["W"], q["C"], q["dil"], q["ldg"], q["ld_add"], q["addend_rows"], stats=True)
    return _entry(fwd), _entry(K.upconv_route("bwd", q["N"], q["h"], q["w"], q["H"], q["W"], q["C"], q["dil"], q["ldg"]))


def _strip_index(H, W, C):
    """upconv_fwd_strip_kernel's work item of output (row, column): strips of 4 pixels, the four vertically adjacent strips of a
    4-row band consecutive, channel groups fastest"""
    def index(r, c):
        n, oh, ow = r // (H * W), r // W % H, r % W
        sp = ((n * (H // 4) + oh // 4) * (W // 4) + ow // 4) * 4 + oh % 4
        return sp * (C // 4) + c // 4
    return index


def case_upconv(N, h, w, H, W, C, dil=1, addend_rows=None, seed=47, fwd_only=False, capped=False, remap=False, *, route=None):
    """route: the "fwd <kernel>" / "bwd <kernel>" HipKernels.upconv_route must begin with for the two calls (asserted on the real
    tensors before them, and without a GPU by test_upconv_plan_cpu.py, which also wants one of every case in CASES; None - the
    shape fuzzer - asserts nothing).  As with the dense cases, where a label's remark and the route differ the route is what runs.
    fwd_only: the backward (planned and declared all the same) is not run - its CPU statement takes 12 s at the shapes that take
    the strip kernels past their cap.  capped: the strip forward runs past its cap; remap: the forward's grid is one on which
    uda_xcd_remap is not the identity (test_capped_cases_cpu.py holds both)."""
    cap = Capped("upconv_fwd_strip_kernel", "UPCONV_STRIP_MAX_WG", N * H * (W // 4) * (C // 4), 256, _strip_index(H, W, C),
                 whole="H % 4 == 0 on the strip kernels and C / 4 = 64 channel groups" if C == 256 else None) if capped else None

    def run(dev):
        g = gen(seed)
        K = hip()
        gl = torch.randn(N * h * w, 9 * C, generator=g)
        ad = None if addend_rows is None else padded(addend_rows, C, g)
        o_r = padded(N * H * W, C, g)
        st_r = torch.zeros(16, 2, C, dtype=torch.float64)
        SPEC.upconv_fwd(gl, N, h, w, o_r, H, W, ad, dil, st_r)
        o_h = to_dev(padded(N * H * W, C, g), dev)
        st_h = out_dev((16, 2, C), torch.float64, dev, fill=0)
        gl_h, ad_h = ro_dev(gl, dev), ro_dev(ad, dev)
        q = run.upconv_query              # g and dg are contiguous [N*h*w, 9*C]
        assert gl_h.stride(0) == q["ldg"] and (ad is None or (ad_h.stride(0), ad_h.shape[0]) == (q["ld_add"], q["addend_rows"])), \
            "upconv_query does not describe the tensors of this call"
        got = upconv_routes(K, q)
        assert route is None or got == tuple(route), "planned routes %r, the case declares %r" % (got, route)
        K.upconv_fwd(gl_h, N, h, w, o_h, H, W, ad_h, dil, st_h)
        errs = [rel_at(o_h, o_r, 2e-5, cap), rel(st_h.sum(0), st_r.sum(0))]
        if fwd_only:
            return max(errs), 2e-5
        dy = padded(N * H * W, C, g)
        dg_r = torch.empty(N * h * w, 9 * C)
        SPEC.upconv_bwd(dy, N, H, W, dg_r, h, w, dil)
        dg_h = out_dev((N * h * w, 9 * C), torch.float32, dev)
        K.upconv_bwd(ro_dev(dy, dev), N, H, W, dg_h, h, w, dil)
        errs.append(rel(dg_h, dg_r))
        return max(errs), 2e-5
    run.upconv_query = dict(N=N, h=h, w=w, H=H, W=W, C=C, dil=dil, ldg=9 * C, ld_add=None if addend_rows is None else round4(C) + 4,
                            addend_rows=addend_rows or 0)
    run.route = route
    run.capped, run.remap = [cap] if capped else [], remap
    return run


def case_upconv_identity(N, h, w, H, W, Cf, Cl, Cout, seed=48):
    """The identity the engine relies on: conv3x3(cat(up(f), low)) == upconv(f W_taps^T) + conv3x3_low(low), against
    F.interpolate + F.conv2d on the same tensors (HIP kernels for every piece)."""
    def run(dev):
        import torch.nn.functional as F
        g = gen(seed)
        K = hip()
        f = torch.randn(N, Cf, h, w, generator=g)
        low = torch.randn(N, Cl, H, W, generator=g)
        wt = torch.randn(Cout, Cf + Cl, 3, 3, generator=g) / ((Cf + Cl) * 9) ** 0.5
        ref = F.conv2d(torch.cat([F.interpolate(f, size=(H, W), mode="bilinear", align_corners=True), low], 1), wt, None, 1, 1)
        ref = ref.permute(0, 2, 3, 1).reshape(N * H * W, Cout)
        f2 = to_dev(f.permute(0, 2, 3, 1).reshape(N * h * w, Cf).contiguous(), dev)
        l2 = to_dev(low.permute(0, 2, 3, 1).reshape(N * H * W, Cl).contiguous(), dev)
        w_taps = wt[:, :Cf].permute(2, 3, 0, 1).reshape(9 * Cout, Cf, 1, 1).contiguous()
        gl = out_dev((N * h * w, 9 * Cout), torch.float32, dev)
        K.conv(Act(f2, N, h, w), K.relayout_ohwi(w_taps.to(dev)), 1, 1, gl)
        y0 = out_dev((N * H * W, Cout), torch.float32, dev)
        K.conv(Act(l2, N, H, W), K.relayout_ohwi(wt[:, Cf:].contiguous().to(dev)), 3, 1, y0)
        y = out_dev((N * H * W, Cout), torch.float32, dev)
        K.upconv_fwd(gl, N, h, w, y, H, W, y0)
        return rel(y, ref), 2e-5
    return run


CASES += [
    ("upconv fwd/bwd 2 x (8x8 -> 32x32) x 64", case_upconv(2, 8, 8, 32, 32, 64, route=("fwd tile", "bwd thread"))),
    ("upconv fwd/bwd 1 x (5x7 -> 12x20) x 8, addend", case_upconv(1, 5, 7, 12, 20, 8, addend_rows=240, route=("fwd strip3", "bwd thread"))),
    ("upconv fwd/bwd 4 x (4x4 -> 16x16) x 16, addend shared by 2 reps", case_upconv(4, 4, 4, 16, 16, 16, addend_rows=512, route=("fwd strip3", "bwd thread"))),
    ("upconv fwd/bwd 1 x (16x16 -> 32x32) x 12 dil 2 (pixel kernel + colstats)", case_upconv(1, 16, 16, 32, 32, 12, dil=2, route=("fwd pixel", "bwd thread"))),
    ("upconv fwd/bwd 2 x (16x16 -> 32x32) x 32 (x2: 4-column strips)", case_upconv(2, 16, 16, 32, 32, 32, route=("fwd strip4", "bwd thread"))),
    ("upconv fwd/bwd 1 x (5x7 -> 13x18) x 8 (W % 4 != 0: pixel kernel), addend", case_upconv(1, 5, 7, 13, 18, 8, addend_rows=234, route=("fwd pixel", "bwd thread"))),
    ("upconv fwd/bwd 2 x (1x1 -> 4x4) x 4 (degenerate source)", case_upconv(2, 1, 1, 4, 4, 4, route=("fwd strip3", "bwd thread"))),
    ("upconv fwd/bwd 1 x (43x43 -> 128x128) x 8 (scale exactly 1/3: 4-column strips)", case_upconv(1, 43, 43, 128, 128, 8, route=("fwd strip4", "bwd thread"))),
    ("upconv fwd/bwd 1 x (85x85 -> 128x128) x 8 (scale 0.661: 4-column strips)", case_upconv(1, 85, 85, 128, 128, 8, route=("fwd pixel", "bwd thread"))),
    ("upconv fwd/bwd 1 x (86x86 -> 128x128) x 8 (scale 0.669: pixel kernel)", case_upconv(1, 86, 86, 128, 128, 8, route=("fwd pixel", "bwd thread"))),
    ("upconv fwd/bwd 3 x (32x32 -> 128x128) x 256 (the decoder's shape)", case_upconv(3, 32, 32, 128, 128, 256, addend_rows=16384, route=("fwd tile", "bwd wave"))),
    ("upconv fwd/bwd 2 x (4x4 -> 16x16) x 256 (tile kernel, one tile; wave-per-pixel bwd)", case_upconv(2, 4, 4, 16, 16, 256, addend_rows=256, route=("fwd tile", "bwd wave"))),
    ("upconv fwd/bwd 1 x (5x9 -> 17x33) x 256 (exact ratio 1/4, odd sizes: strip / pixel fwd, wave bwd)", case_upconv(1, 5, 9, 17, 33, 256, route=("fwd pixel", "bwd wave"))),
    ("upconv fwd/bwd 1 x (9x5 -> 32x16) x 256 (tile kernel, ratio 0.258 / 0.267), addend", case_upconv(1, 9, 5, 32, 16, 256, addend_rows=512, route=("fwd tile", "bwd wave"))),
    ("upconv fwd/bwd 2 x (16x16 -> 48x64) x 256 (tile kernel at x3 / x4.2)", case_upconv(2, 16, 16, 48, 64, 256, route=("fwd tile", "bwd wave"))),
    ("upconv fwd/bwd 1 x (83x83 -> 128x128) x 8 (3*sw = 1.937: the last width on 4-column strips, 84 is on the pixel kernel)",
     case_upconv(1, 83, 83, 128, 128, 8, route=("fwd strip4", "bwd thread"))),
    ("upconv fwd/bwd 1 x (10x5 -> 16x16) x 32 (tile geometry, footprint 10 x 5 over the LDS bound: 3-column strips)",
     case_upconv(1, 10, 5, 16, 16, 32, route=("fwd strip3", "bwd thread"))),
    ("upconv fwd/bwd 1 x (2x2 -> 16x16) x 256 (x15: 36 tap rows exceed the wave kernel's weight table, thread bwd)",
     case_upconv(1, 2, 2, 16, 16, 256, route=("fwd tile", "bwd thread"))),
    ("upconv fwd/bwd 1 x (8x8 -> 16x16) x 256 (x2, the output-stride-8 geometry: 4-column strips, wave bwd)",
     case_upconv(1, 8, 8, 16, 16, 256, route=("fwd strip4", "bwd wave"))),
    ("upconv identity vs interpolate+conv2d 2 x (8x8 -> 32x32), 64+16 -> 32", case_upconv_identity(2, 8, 8, 32, 32, 64, 16, 32)),
]


# ---------------------------------------------------------------- evaluation post-processing vs scipy
def _scipy_postprocess(prob, thr_cup, thr_disc):
    """utils/Utils.py:427-463 with skimage's two calls replaced by their scipy.ndimage equivalents: binary_erosion(diamond(7))
    = ndimage.binary_erosion(structure=L1 ball, border_value=1) (skimage erodes with the outside set), measure.label =
    ndimage.label with the full 3x3 structure (both number components in raster order of their first pixel).  The chain itself
    is stated once, in tests/postproc_shapes.py (stages), which also keeps the masks after the erosion and after the keep."""
    import postproc_shapes
    return postproc_shapes.stages(prob, thr_cup, thr_disc)["filled"]


def case_postprocess(B, H, W, seed=61):
    def run(dev):
        import numpy as np
        g = gen(seed)
        K = hip()
        rs = np.random.RandomState(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        prob = np.zeros((B, 2, H, W), np.float32)
        for b in range(B):
            for c in range(2):
                p = 0.08 * rs.rand(H, W)
                for _ in range(rs.randint(1, 4)):               # a few blobs (one of them touching the border in sample 0), with holes
                    cy = (0.05 if (b == 0 and c == 1) else rs.uniform(0.25, 0.75)) * H
                    cx, a, d = rs.uniform(0.25, 0.75) * W, rs.uniform(0.12, 0.3) * H, rs.uniform(0.12, 0.3) * W
                    r = np.sqrt(((yy - cy) / a) ** 2 + ((xx - cx) / d) ** 2)
                    p = np.maximum(p, np.clip(1.25 - r, 0, 1))
                    hole = np.sqrt((yy - cy - 0.3 * a) ** 2 + (xx - cx) ** 2) < rs.uniform(2, 9)
                    p[hole] = 0.02
                p += 0.5 * (rs.rand(H, W) < 0.03)                 # salt: isolated pixels the median removes
                p[rs.rand(H, W) < 0.03] = 0.0                     # pepper inside the blobs
                prob[b, c] = np.clip(p, 0, 1)
        out = K.postprocess(torch.from_numpy(prob).to(dev), 0.75, 0.75).cpu().numpy()
        bad = sum(int((out[b] != _scipy_postprocess(prob[b], 0.75, 0.75)).sum()) for b in range(B))
        outd = K.postprocess(torch.from_numpy(prob[:1]).to(dev), 0.1, 0.5).cpu().numpy()
        bad += int((outd[0] != _scipy_postprocess(prob[0], 0.1, 0.5)).sum())
        empty = K.postprocess(torch.zeros(1, 2, H, W, device=dev), 0.75, 0.75)
        bad += int(empty.sum())
        return float(bad), 0.5                  # bit-exact or fail
    return run


CASES += [
    ("postprocess 3 x 2 x 128 x 128 vs scipy (bit-exact)", case_postprocess(3, 128, 128)),
    ("postprocess 2 x 2 x 200 x 136 vs scipy (ragged tiles)", case_postprocess(2, 200, 136, seed=62)),
    ("postprocess 1 x 2 x 512 x 512 vs scipy", case_postprocess(1, 512, 512, seed=63)),
]


# ---------------------------------------------------------------- fused alignment / adversarial glue
def case_proto_align(C, prev, seed=71):
    """uda_proto_align_fwd / bwd (EMA of the eight centroids + intra / inter and the gradient through the current term)."""
    def run(dev):
        g = gen(seed)
        K = hip()
        cs, ct = torch.randn(4, C, generator=g), torch.randn(4, C, generator=g)
        ps, pt = (torch.randn(4, C, generator=g), torch.randn(4, C, generator=g)) if prev else (None, None)
        d = lambda t: None if t is None else t.to(dev)
        ns_r, nt_r, l_r = SPEC.proto_align_fwd(cs, ct, ps, pt, 0.9)
        ns_h, nt_h, l_h = K.proto_align_fwd(cs.to(dev), ct.to(dev), d(ps), d(pt), 0.9)
        gi = torch.tensor([0.37])
        w = 0.9 if prev else 1.0
        a_r, b_r = SPEC.proto_align_bwd(ns_r, nt_r, gi, w, w)
        a_h, b_h = K.proto_align_bwd(ns_h, nt_h, gi.to(dev), w, w)
        exact = torch.equal(ns_h.cpu(), ns_r) and torch.equal(nt_h.cpu(), nt_r)      # the EMA itself: the reference's expression, bit for bit
        return max(rel(l_h, l_r), rel(a_h, a_r), rel(b_h, b_r), 0.0 if exact else 1.0), 2e-6
    return run


def case_adv_loss(n1, n2, label, scale, seed=72):
    def run(dev):
        g = gen(seed)
        K = hip()
        d1, d2 = 3 * torch.randn(n1, generator=g), 3 * torch.randn(n2, generator=g)
        d1[:4] = torch.tensor([40., -40., 100., -100.])
        l_r = SPEC.adv_loss_fwd(d1, d2, label, scale)
        l_h = K.adv_loss_fwd(d1.to(dev), d2.to(dev), label, scale)
        gi = torch.tensor([1.7])
        a_r, b_r = SPEC.adv_loss_bwd(d1, d2, label, scale, gi)
        a_h, b_h = K.adv_loss_bwd(d1.to(dev), d2.to(dev), label, scale, gi.to(dev))
        return max(rel(l_h, l_r), rel(a_h, a_r), rel(b_h, b_r)), 2e-6
    return run


def case_adv_s2d(N, C, H, W, op, seed=73, capped=False):
    """First discriminator layer fed by logits: z = s2d(sigmoid | uncertainty map) and its adjoint incl. the map's derivative."""
    caps = [Capped("s2d_fwd_kernel (uda_adv_s2d_fwd)", "S2D_MAX_WG", N * ((H + 5) // 2) * ((W + 5) // 2) * 4 * C, 256, by_element(4 * C)),
            Capped("s2d_bwd_kernel (uda_adv_s2d_bwd)", "S2D_MAX_WG", N * C * H * W, 256, by_element(1))] if capped else [None, None]

    def run(dev):
        g = gen(seed)
        K = hip()
        x = 3 * torch.randn(N, C, H, W, generator=g)
        x[0, 0, 0, :4] = torch.tensor([30., -30., 90., -90.])          # saturated sigmoids: log(s + 1e-7) at s = 0 and s = 1
        Hz, Wz = (H + 5) // 2, (W + 5) // 2
        z_r, z_h = torch.empty(N * Hz * Wz, 4 * C), out_dev((N * Hz * Wz, 4 * C), torch.float32, dev)
        SPEC.adv_s2d_fwd(x, op, z_r)
        K.adv_s2d_fwd(ro_dev(x, dev), op, z_h)
        dz = torch.randn(N * Hz * Wz, 4 * C, generator=g)
        d_r, d_h = torch.empty_like(x), out_dev((N, C, H, W), torch.float32, dev)
        SPEC.adv_s2d_bwd(dz, x, op, d_r)
        K.adv_s2d_bwd(ro_dev(dz, dev), ro_dev(x, dev), op, d_h)
        return max(rel_at(z_h, z_r, 5e-6, caps[0]), rel_at(d_h, d_r, 5e-6, caps[1])), 5e-6
    run.capped = caps if capped else []
    return run


CASES += [
    ("proto_align C=305 first use", case_proto_align(305, False)),
    ("proto_align C=305 EMA", case_proto_align(305, True)),
    ("proto_align C=7 EMA", case_proto_align(7, True)),
    ("adv_loss 2x17x17 label 1 scale 0.01", case_adv_loss(578, 578, 1.0, 0.01)),
    ("adv_loss label 0 scale 1 ragged", case_adv_loss(300, 77, 0.0, 1.0)),
    ("adv_s2d sigmoid C=1 64x64", case_adv_s2d(2, 1, 64, 64, 1)),
    ("adv_s2d entropy C=2 50x46", case_adv_s2d(2, 2, 50, 46, 2)),
]


# ---------------------------------------------------------------- column windows of wide buffers, as engine.py's call sites use them
# Each case builds one wide matrix whose columns outside the window hold live finite data, runs the producers in the engine's order and
# after every call holds the window against the statement and every other bit - the other columns, the padding lanes, the guard rows,
# the neighbouring slices of the shared fp64 arena, every operand - against its state before the call (only_writes).
def _no_spill(what):
    got = footprint_violations()
    assert got == [], "%s wrote outside its window: (buffer, first position) %s" % (what, got)


def _arena(sizes, dev):
    """consecutive [16, nq, C] slices of one fp64 arena (engine.py _Arena.take), on the CPU and on the device"""
    n = sum(16 * nq * C for nq, C in sizes)
    ar, ah = torch.zeros(n, dtype=torch.float64), out_dev((n,), torch.float64, dev, fill=0, name="statistics arena")
    out, off = [], 0
    for nq, C in sizes:
        m = 16 * nq * C
        out.append((ar[off:off + m].view(16, nq, C), ah[off:off + m].view(16, nq, C)))
        off += m
    return out


ASPP_BRANCHES = ((1, 1), (3, 6), (3, 12), (3, 18))


def case_window_aspp(N, H, W, seed=80, *, routes):
    """engine.py forward, ASPP: 1x1 and three dilated 3x3 convs 320 -> 256 with statistics into windows 0..3 of cat [P, 1280],
    broadcast_rows into [1024, 1280)"""
    def run(dev):
        g = gen(seed)
        K = hip()
        P = N * H * W
        src = make_src(N, H, W, 320, g, lazy=False)
        cat_r = padded(P, 1280, g)
        cat_h = to_dev(cat_r, dev, name="cat")
        st = _arena([(2, 256)] * 5, dev)
        sh = act_to(src, dev)
        errs = []
        for j, (k, dil) in enumerate(ASPP_BRANCHES):
            sl = slice(256 * j, 256 * (j + 1))
            w = torch.randn(256, 320, k, k, generator=g) / (320 * k * k) ** 0.5
            SPEC.conv(src, SPEC.relayout_ohwi(w), k, dil, cat_r[:, sl], None, None, st[j][0])
            wl = ro_dev(K.relayout_ohwi(w.to(dev)), dev, name="weight %d" % j)
            _check_route(K.conv_route(sh, wl, k, dil, cat_h[:, sl], stats=st[j][1]), routes[j], K.mfma)
            only_writes(cat_h[:, sl], st[j][1])
            K.conv(sh, wl, k, dil, cat_h[:, sl], stats=st[j][1])
            _no_spill("conv %dx%d dil %d into window %d" % (k, k, dil, j))
            errs += [rel(cat_h[:, sl], cat_r[:, sl]), rel(st[j][1].sum(0), st[j][0].sum(0))]
        yg = padded(N, 256, g)
        SPEC.broadcast_rows(yg, N, cat_r[:, 1024:1280], 1.0)
        ygh = ro_dev(yg, dev, name="yg")
        only_writes(cat_h[:, 1024:1280])
        K.broadcast_rows(ygh, N, cat_h[:, 1024:1280], 1.0)
        _no_spill("broadcast_rows into window 4")
        errs.append(rel(cat_h, cat_r))
        return max(errs), 2e-5
    run.plan_queries = [(_query("conv", N, H, W, 320, 256, k, dil, stats=True, ldy=1284), routes[j]) for j, (k, dil) in enumerate(ASPP_BRANCHES)]
    return run


def case_window_decoder_fwd(N, h, w, H, W, seed=81, *, route):
    """engine.py forward, decoder: xf [P, 305] (ld 308) assembled by upsample_fwd with statistics -> [0, 256), bn_apply ->
    [256, 304), the 256 -> 1 boundary head (bias, keep-mask) -> [304, 305); then colstats_window over [256, 305)"""
    def run(dev):
        g = gen(seed)
        K = hip()
        P = N * H * W
        xf_r = _poison(torch.empty(P, 308))[:, :305]
        xf_r.copy_(torch.randn(P, 305, generator=g))
        xf_h = to_dev(xf_r, dev, name="xf")
        (_, _), (s_r, s_h), (_, _) = st = _arena([(2, 48), (2, 305), (2, 256)], dev)
        feat = padded(N * h * w, 256, g)
        SPEC.upsample_fwd(feat, N, h, w, xf_r[:, 0:256], H, W, stats=s_r)
        fh = ro_dev(feat, dev, name="feature")
        only_writes(xf_h[:, 0:256], s_h)
        K.upsample_fwd(fh, N, h, w, xf_h[:, 0:256], H, W, stats=s_h)
        _no_spill("upsample_fwd into [0, 256)")
        errs = [rel(xf_h[:, 0:256], xf_r[:, 0:256]), rel(s_h.sum(0), s_r.sum(0))]
        lo = make_src(N, H, W, 48, g, True, ACT_RELU)
        SPEC.bn_apply(lo, xf_r[:, 256:304], None)
        loh = act_to(lo, dev)
        only_writes(xf_h[:, 256:304])
        K.bn_apply(loh, xf_h[:, 256:304], None)
        _no_spill("bn_apply into [256, 304)")
        errs.append(rel(xf_h[:, 256:304], xf_r[:, 256:304]))
        b2 = make_src(N, H, W, 256, g, True, ACT_RELU, mask=True)
        wt, b = torch.randn(1, 256, 1, 1, generator=g) / 16.0, torch.randn(1, generator=g)
        SPEC.conv(b2, SPEC.relayout_ohwi(wt), 1, 1, xf_r[:, 304:305], b)
        b2h, wl, bh = act_to(b2, dev), ro_dev(K.relayout_ohwi(wt.to(dev)), dev, name="head weight"), ro_dev(b, dev, name="head bias")
        _check_route(K.conv_route(b2h, wl, 1, 1, xf_h[:, 304:305], bias=bh), route, K.mfma)
        only_writes(xf_h[:, 304:305])
        K.conv(b2h, wl, 1, 1, xf_h[:, 304:305], bias=bh)
        _no_spill("conv1x1 256 -> 1 into [304, 305)")
        errs.append(rel(xf_h[:, 304:305], xf_r[:, 304:305]))
        SPEC.colstats_window(xf_r[:, 256:305], s_r, 256)
        only_writes(s_h)
        K.colstats_window(xf_h[:, 256:305], s_h, 256)
        _no_spill("colstats_window over [256, 305)")
        full = torch.zeros(16, 2, 305, dtype=torch.float64)
        SPEC.colstats(xf_r, full)
        errs += [rel(s_h.sum(0), s_r.sum(0)), rel(s_h.sum(0), full.sum(0)), rel(xf_h, xf_r)]
        assert all(float(a.abs().sum()) == 0.0 for a in (st[0][1], st[2][1]))
        return max(errs), 2e-5
    run.plan_queries = [(_query("conv", N, H, W, 256, 1, 1, 1, lazy=True, mask=True, bias=True, ldy=308), route)]
    return run


def case_window_decoder_bwd(N, H, W, seed=82, *, route):
    """engine.py backward, decoder: d_xf [P, 305] (ld 308, lanes 305..307 zeroed): bnbwd_apply (low-rank dU of the 305 -> 2 head) in
    place over [:, :305], head_upsample_bwd accumulating into [304, 305), the 3x3 input gradient 48 <- 256 accumulating in place
    into [256, 304).  The boundary head's NCHW gradient is four times d_xf's grid on each side; the zero lanes must still be zero bits."""
    def run(dev):
        g = gen(seed)
        K = hip()
        P = N * H * W
        base = torch.zeros(P, 308)
        base[:, :305] = torch.randn(P, 305, generator=g)
        d_r = base.clone()[:, :305]
        d_h = to_dev(base[:, :305], dev, name="d_xf")
        frame = _frame_of(d_h)
        lanes = d_h.as_strided((P, 3), (308, 1), d_h.storage_offset() + 305)
        lanes.zero_()                                                    # (to_dev poisons the lanes: the engine zeroes them)
        x = padded(P, 305, g)
        sc, shf = 0.5 + torch.rand(305, generator=g), 0.3 * torch.randn(305, generator=g)
        x[(x * sc + shf).abs() < 1e-4] += 0.01
        y = Act(x, N, H, W, sc, shf, ACT_RELU, None, 1.0, BNRec("t", 0.1 * torch.randn(305, generator=g), 0.5 + torch.rand(305, generator=g), float(P), False))
        d2, w2 = padded(P, 2, g), torch.randn(2, 305, generator=g) / 305 ** 0.5
        s_r = torch.zeros(16, 3, 305, dtype=torch.float64)
        SPEC.bnbwd_reduce(None, y, s_r, lowrank=(d2, w2))
        gr = torch.empty(4, 305)
        SPEC.bnbwd_finalize(s_r, y, gr[0], gr[1], gr[2], gr[3])
        SPEC.bnbwd_apply(None, y, gr[0], gr[1], d_r, d_r.clone(), lowrank=(d2, w2))
        yh, d2h, w2h, gh = act_to(y, dev), ro_dev(d2, dev, name="d_x1b"), ro_dev(w2, dev, name="w_head"), ro_dev(gr, dev, name="c1 c2")
        only_writes(d_h)
        K.bnbwd_apply(None, yh, gh[0], gh[1], d_h, d_h, lowrank=(d2h, w2h))
        _no_spill("bnbwd_apply in place over [:, :305]")
        errs = [rel(d_h, d_r)]
        gx2 = torch.randn(N, 1, 4 * H, 4 * W, generator=g)
        SPEC.head_upsample_bwd(gx2, d_r[:, 304:305], N, H, W, True)
        gx2h = ro_dev(gx2, dev, name="gx2")
        only_writes(d_h[:, 304:305])
        K.head_upsample_bwd(gx2h, d_h[:, 304:305], N, H, W, True)
        _no_spill("head_upsample_bwd into [304, 305)")
        errs.append(rel(d_h[:, 304:305], d_r[:, 304:305]))
        dy = padded(P, 256, g)
        wt = torch.randn(256, 48, 3, 3, generator=g) / (48 * 9) ** 0.5
        ref = torch.nn.grad.conv2d_input((N, 48, H, W), wt, dy.reshape(N, H, W, 256).permute(0, 3, 1, 2), 1, 1, 1)
        d_r[:, 256:304] += ref.permute(0, 2, 3, 1).reshape(P, 48)
        wd, dyh = ro_dev(K.relayout_dgrad(wt.to(dev)), dev, name="low_dgrad weight"), Act(ro_dev(dy, dev, name="dy1"), N, H, W)
        win = d_h[:, 256:304]
        _check_route(K.conv_route(dyh, wd, 3, 1, win, addend=win), route, K.mfma)
        only_writes(win)
        K.conv(dyh, wd, 3, 1, win, addend=win)
        _no_spill("dgrad3x3 48 <- 256 in place into [256, 304)")
        errs.append(rel(d_h, d_r))
        assert frame is _frame_of(lanes) and int((lanes.view(torch.int32) != 0).sum()) == 0, "lanes 305..307 are no longer zero bits"
        return max(errs), 2e-5
    run.plan_queries = [(_query("conv", N, H, W, 256, 48, 3, 1, addend=True, ldy=308, ld_add=308), route)]
    return run


def case_window_coef(first, seed=83):
    """bn_finalize into the channel window [first, first + 256) of coef [4][1280] (engine.py: coef[q][..., sl]), and tn_gain over the
    same window of the per-half coefficients [4][2][1280]"""
    def run(dev):
        g = gen(seed)
        K = hip()
        sl = slice(first, first + 256)
        xs = [2.0 * torch.randn(40, 256, generator=g) + 0.5, 0.7 * torch.randn(24, 256, generator=g) - 0.2]
        (_, _), (s0r, s0h), (s1r, s1h), (_, _) = st = _arena([(2, 64), (2, 256), (2, 256), (2, 64)], dev)
        SPEC.colstats(xs[0], s0r)
        SPEC.colstats(xs[1], s1r)
        s0h.copy_(s0r)
        s1h.copy_(s1r)
        gamma, beta = 0.5 + torch.rand(256, generator=g), torch.randn(256, generator=g)
        rm, rv = torch.randn(256, generator=g), 0.5 + torch.rand(256, generator=g)
        cr = torch.randn(4, 1280, generator=g)
        ch = out_like(cr, dev, name="coef")
        rmh, rvh, gah, beh = out_like(rm, dev, name="running mean"), out_like(rv, dev, name="running var"), ro_dev(gamma, dev), ro_dev(beta, dev)
        SPEC.bn_finalize(s0r, 40.0, gamma, beta, rm, rv, 0.1, 1e-5, cr[0][sl], cr[1][sl], cr[2][sl], cr[3][sl])
        only_writes(rmh, rvh, *(ch[q][sl] for q in range(4)))
        K.bn_finalize(s0h, 40.0, gah, beh, rmh, rvh, 0.1, 1e-5, ch[0][sl], ch[1][sl], ch[2][sl], ch[3][sl])
        _no_spill("bn_finalize into coef[q][%d:%d]" % (first, first + 256))
        errs = [rel(ch, cr), rel(rmh, rm), rel(rvh, rv)]
        tr = torch.randn(4, 2, 1280, generator=g)
        th = out_like(tr, dev, name="coef per half")
        gr, gh = torch.empty(256), out_dev((256,), torch.float32, dev, name="gain")
        SPEC.tn_gain(s0r, s1r, 40.0, 24.0, 1e-5, tr[0][0][sl], tr[1][0][sl], tr[0][1][sl], tr[1][1][sl], gr)
        only_writes(gh, th[0][0][sl], th[1][0][sl], th[0][1][sl], th[1][1][sl])
        K.tn_gain(s0h, s1h, 40.0, 24.0, 1e-5, th[0][0][sl], th[1][0][sl], th[0][1][sl], th[1][1][sl], gh)
        _no_spill("tn_gain over coef[q][h][%d:%d]" % (first, first + 256))
        errs += [rel(th, tr), rel(gh, gr)]
        return max(errs), 2e-6
    return run


# the routes of "conv1x1 320->256 P=N", "conv3x3 320->256 dil6" and "dgrad3x3 48<-256 addend" above: the wide row strides change none
ASPP_ROUTES = ("ws 64x128 k1 xf0",) + (("ws 64x128 k3 xf0", "x3 128x128 k3"),) * 3
DEC_BWD_ROUTE = ("low 64x64 pipe", "x3 256x64 k3")
WINDOW_CASES = [
    ("aspp windows of cat [128, 1280]: 2 x 8x8", case_window_aspp(2, 8, 8, routes=ASPP_ROUTES)),
    ("aspp windows of cat [126, 1280]: 2 x 9x7 (ragged tiles)", case_window_aspp(2, 9, 7, routes=ASPP_ROUTES)),
    ("decoder forward windows of xf [512, 308]: 2 x (4x4 -> 16x16)", case_window_decoder_fwd(2, 4, 4, 16, 16, route="heads 128x1")),
    ("decoder forward windows of xf [286, 308]: 2 x (5x7 -> 13x11)", case_window_decoder_fwd(2, 5, 7, 13, 11, route="heads 128x1")),
    ("decoder backward windows of d_xf [512, 308]: 2 x 16x16", case_window_decoder_bwd(2, 16, 16, route=DEC_BWD_ROUTE)),
    ("decoder backward windows of d_xf [286, 308]: 2 x 13x11", case_window_decoder_bwd(2, 13, 11, route=DEC_BWD_ROUTE)),
    ("coefficient window [0, 256) of [4][1280]", case_window_coef(0)),
    ("coefficient window [512, 768) of [4][1280]", case_window_coef(512)),
    ("coefficient window [1024, 1280) of [4][1280]", case_window_coef(1024)),
]
WINDOW_CASES = [(name, footprinted(fn)) for name, fn in WINDOW_CASES]


# ---------------------------------------------------------------- losses_proto.hip at its edges
# The training-step glue at the shapes where its kernels change behaviour: every LDS split of the prototype reduce (C = 1 .. 1024,
# PP = 256 .. 1 pixel lanes), a workgroup filled exactly and by one pixel more, the grid-stride step of the backward kernel
# (P > 32768), h != w and non-integral H / h in the weights, inputs below one workgroup and one wave in the block sums.  The
# reference is the float64 evaluation of the statement: SpecKernels' torch expressions on double copies of the fp32 inputs
# (proto_reduce / proto_bwd / feat_* are float64 there already).  Tolerances are those of the families' first cases.
def _f64(*ts):
    return tuple(None if t is None else t.double() for t in ts)


def _factor(P):
    """B, h, w with B * h * w = P and h != w where P allows it (the weights need a pixel grid)"""
    for B in (3, 2, 5, 1):
        if P % B == 0:
            n = P // B
            h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
            return B, h, n // h
    raise AssertionError(P)


def proto_edge_weights(P, g):
    """reference weights [P, 4] of the three modes on a B x h x w grid of P pixels (inputs of the reduce, not compared)"""
    B, h, w = _factor(P)
    H, W = 2 * h + 1, w + 3
    mp = (torch.rand(B, 2, H, W, generator=g) > 0.6).float()
    lg = 2.0 * torch.randn(P, 2, generator=g) + 1.1              # sigmoid > 0.75 on about half of the pixels
    sd, mn = 0.06 * torch.rand(B, 2, H, W, generator=g), torch.rand(B, 2, H, W, generator=g)
    return [SPEC.proto_weights(0, B, h, w, map_=mp)[0], SPEC.proto_weights(1, B, h, w, logits=lg)[0],
            SPEC.proto_weights(2, B, h, w, logits=lg, std_map=sd, mean_map=mn)[0]]


def case_proto_edge(P, C, seed=90):
    """uda_proto_reduce / finalize / bwd at one (P, C), with the reference weights of all three modes: sums with the count column,
    centroids, d_feat accumulated into live data and written over NaN, d_w."""
    def run(dev):
        g = gen(seed)
        K = hip()
        feat = padded(P, C, g)
        feat += 0.25                                             # centroids away from 0: every class has a scale of its own
        fh = ro_dev(feat, dev)
        errs = []
        for mode, w_r in enumerate(proto_edge_weights(P, g)):
            s_r = torch.zeros(4, C + 1, dtype=torch.float64)
            SPEC.proto_reduce(feat, w_r, s_r)
            assert float(s_r[:, C].min()) >= 1.0, "a class without weight in the test input (mode %d)" % mode
            s_h = out_dev((4, C + 1), torch.float64, dev, fill=0, name="sums mode %d" % mode)
            wh = ro_dev(w_r, dev)
            K.proto_reduce(fh, wh, s_h)
            errs += [rel(s_h[:, :C], s_r[:, :C]), rel(s_h[:, C], s_r[:, C]), rel(K.proto_finalize(s_h), SPEC.proto_finalize(s_r))]
            dC = torch.randn(4, C, generator=g)
            base = padded(P, C, g)
            df_r = base.clone()
            dw_r = SPEC.proto_bwd(feat, w_r, s_r, dC, df_r, True, True)
            df_h = to_dev(base, dev)
            dw_h = K.proto_bwd(fh, wh, ro_dev(s_r, dev), ro_dev(dC, dev), df_h, True, True)
            errs += [rel(df_h, df_r), rel(dw_h, dw_r)]
            over = padded(P, C, g)
            over.fill_(float("nan"))                             # overwriting: nothing of the old content may survive
            df_r = torch.empty(P, C)
            SPEC.proto_bwd(feat, w_r, s_r, dC, df_r, False, False)
            df_h = to_dev(over, dev)
            K.proto_bwd(fh, wh, ro_dev(s_r, dev), ro_dev(dC, dev), df_h, False, False)
            errs.append(rel(df_h, df_r))
        DETAIL.clear()
        DETAIL.update({"errs": ["%.1e" % e for e in errs]})
        return max(errs), 3e-5
    return run


def case_proto_weights(mode, B, H, W, h, w, seed=91):
    """uda_proto_weights on an (H, W) -> (h, w) geometry.  Mode 0: F.interpolate(mode="nearest"), exact.  Mode 1: [P, 2] logits
    in a matrix of row stride 12.  Mode 2: align_corners bilinear of i.i.d. std / mean maps, compared on decided pixels."""
    def run(dev):
        g = gen(seed)
        K = hip()
        P = B * h * w
        if mode == 0:
            mp = (torch.rand(B, 2, H, W, generator=g) > 0.5).float()
            w_r, _, _ = SPEC.proto_weights(0, B, h, w, map_=mp)
            w_h, _, _ = K.proto_weights(0, B, h, w, map_=ro_dev(mp, dev))
            return float((w_h.cpu() - w_r).abs().max()), 0.0
        lg = padded(P, 6, g, scale=2.0)[:, :2]
        if mode == 1:
            w_r, _, _ = SPEC.proto_weights(1, B, h, w, logits=lg.double())
            w_h, _, _ = K.proto_weights(1, B, h, w, logits=ro_dev(lg, dev))
            return rel(w_h, w_r), 3e-5
        sd, mn = 0.08 * torch.rand(B, 2, H, W, generator=g), torch.rand(B, 2, H, W, generator=g)
        w_h, m0_h, m1_h = K.proto_weights(2, B, h, w, logits=ro_dev(lg, dev), std_map=ro_dev(sd, dev), mean_map=ro_dev(mn, dev))
        errs = retrify_errors(B, h, w, lg, sd, mn, w_h, m0_h, m1_h)
        m0 = SPEC.proto_weights(2, B, h, w, logits=lg, std_map=sd, mean_map=mn)[1]
        assert 0.05 < float(m0.mean()) / 2 < 0.999, "degenerate mask in the test input"
        return max(errs), 3e-5
    return run


SEG_SATURATED = ((40., 0.), (-40., 1.), (110., 0.), (-110., 1.),      # wrong and certain: the -100 clamp of the log, the 1e-12 floor
                 (17., 1.), (-17., 0.), (90., 1.), (-90., 0.),        # right and certain: the clamped log meets the factor 0
                 (40., 1.), (-40., 0.), (110., 1.), (-110., 0.))
# (|logit| = 17 and 90 come with the target on their side only: there fp32 rounds the sigmoid to exactly 1 resp. 0 while float64
# does not, so with the opposite target the fp32 statement itself says 100 where float64 says 17 resp. 90)


def case_seg_loss_edge(B, S, seed=92):
    """uda_seg_loss_fwd / bwd below one workgroup (1 x 2 x 5 x 5) and on a ragged size, saturated logits with targets of exactly
    0 and 1, against the float64 statement."""
    def run(dev):
        g = gen(seed)
        K = hip()
        o = 3 * torch.randn(B, 2, S, S, generator=g)
        b = 2 * torch.randn(B, 1, S, S, generator=g)
        tm = (torch.rand(B, 2, S, S, generator=g) > 0.5).float()
        tb = torch.rand(B, 1, S, S, generator=g)
        sat = torch.tensor(SEG_SATURATED)
        o.view(-1)[:len(sat)], tm.view(-1)[:len(sat)] = sat[:, 0], sat[:, 1]
        b.view(-1)[:4], tb.view(-1)[:4] = torch.tensor([60., -60., 60., -60.]), torch.tensor([0., 1., 1., 0.])
        gs = torch.tensor([0.37])
        l_r = SPEC.seg_loss_fwd(*_f64(o, tm, b, tb))
        do_r, db_r = SPEC.seg_loss_bwd(*_f64(o, tm, b, tb, gs))
        args = [ro_dev(t, dev) for t in (o, tm, b, tb)]
        l_h = K.seg_loss_fwd(*args)
        do_h, db_h = K.seg_loss_bwd(*args, ro_dev(gs, dev))
        return max(rel(l_h, l_r), rel(do_h, do_r), rel(db_h, db_r)), 2e-5
    return run


def case_mc_stats_edge(B, H, W, seed=93):
    """uda_mc_stats on n = B * 2 * H * W (no multiple of the 1024 elements of a workgroup's step): a third of the pixels with
    eight identical passes (std exactly 0), logits of +-100 both constant and alternating over the passes."""
    def run(dev):
        T = 8
        g = gen(seed)
        base = 3.0 * torch.randn(1, B, 2, H, W, generator=g)
        same = torch.rand(1, B, 2, H, W, generator=g) < 1.0 / 3
        p = base + 1.5 * torch.randn(T, B, 2, H, W, generator=g) * (~same).float()
        sign = torch.tensor([1., -1.] * (T // 2)).view(T, 1)
        pf = p.view(T, -1)
        pf[:, 0:2], pf[:, 2:4] = torch.tensor([100., -100.]), 100. * sign
        same.view(-1)[0:2], same.view(-1)[2:4] = True, False
        preds = p.reshape(T * B, 2, H, W)
        assert preds.shape[0] * 2 * H * W // T % 1024 != 0
        sd_r, mn_r = SPEC.mc_stats(preds.double(), T)
        sd_h, mn_h = hip().mc_stats(ro_dev(preds, dev), T)
        flat = sd_h.cpu()[same[0]]
        exact = bool((flat == 0).all())                          # (NaN and the tiny std of a mean that misses h by an ulp both fail this)
        return max(rel(sd_h, sd_r), rel(mn_h, mn_r), 0.0 if exact else float("inf")), 3e-5
    return run


def case_adv_loss_edge(n1, n2, label, scale, seed=94):
    """uda_adv_loss_fwd / bwd with one element per map and with one below / one above a workgroup, against float64"""
    def run(dev):
        g = gen(seed)
        K = hip()
        d1, d2 = 3 * torch.randn(n1, generator=g), 3 * torch.randn(n2, generator=g)
        sat = torch.tensor([40., -40., 100., -100.])
        d1[-4:], d2[:4] = sat[:n1], sat[:n2]
        gi = torch.tensor([1.7])
        l_r = SPEC.adv_loss_fwd(d1.double(), d2.double(), label, scale)
        a_r, b_r = SPEC.adv_loss_bwd(d1.double(), d2.double(), label, scale, gi.double())
        dh = ro_dev(d1, dev), ro_dev(d2, dev)
        l_h = K.adv_loss_fwd(*dh, label, scale)
        a_h, b_h = K.adv_loss_bwd(*dh, label, scale, ro_dev(gi, dev))
        return max(rel(l_h, l_r), rel(a_h, a_r), rel(b_h, b_r)), 2e-6
    return run


def case_proto_align_edge(C, seed=95):
    """uda_proto_align_fwd / bwd at one channel, at a full workgroup and one more, and at four strides: the EMA bit for bit (the
    fp32 expression is the statement), the losses and gradients against float64 on that EMA."""
    def run(dev):
        g = gen(seed)
        K = hip()
        cs, ct, ps, pt = (torch.randn(4, C, generator=g) for _ in range(4))
        ns_r, nt_r, _ = SPEC.proto_align_fwd(cs, ct, ps, pt, 0.9)
        _, _, l_r = SPEC.proto_align_fwd(ns_r.double(), nt_r.double(), None, None, 0.9)
        gi = torch.tensor([0.37])
        a_r, b_r = SPEC.proto_align_bwd(ns_r.double(), nt_r.double(), gi.double(), 0.9, 0.9)
        ns_h, nt_h, l_h = K.proto_align_fwd(*(ro_dev(t, dev) for t in (cs, ct, ps, pt)), 0.9)
        a_h, b_h = K.proto_align_bwd(ns_h, nt_h, ro_dev(gi, dev), 0.9, 0.9)
        exact = torch.equal(ns_h.cpu(), ns_r) and torch.equal(nt_h.cpu(), nt_r)
        return max(rel(l_h, l_r), rel(a_h, a_r), rel(b_h, b_r), 0.0 if exact else 1.0), 2e-6
    return run


def case_adam_edge(n, seed=96):
    """uda_adam_step below and just above one workgroup, steps 1, 2 and 100000 (both bias corrections round to 1), against float64.
    The last max(1, n // 4) elements (n > 1) have g = m = v = 0: their update must be exactly 0, not 0 / 0."""
    def run(dev):
        g = gen(seed)
        p, gr = 0.05 * torch.randn(n, generator=g), torch.randn(n, generator=g)
        m, v = 0.1 * torch.randn(n, generator=g), torch.rand(n, generator=g) * 0.01
        z = slice(n - max(1, n // 4), n) if n > 1 else slice(0, 0)
        gr[z] = m[z] = v[z] = 0.0
        p0 = p.clone()
        ph, mh, vh, gh = out_like(p, dev), out_like(m, dev), out_like(v, dev), ro_dev(gr, dev)
        p, gr, m, v = _f64(p, gr, m, v)
        for step in (1, 2, 100000):
            SPEC.adam_step(p, gr, m, v, 1e-3, 0.9, 0.99, 1e-8, step)
            hip().adam_step(ph, gh, mh, vh, 1e-3, 0.9, 0.99, 1e-8, step)
        still = torch.equal(ph.cpu()[z], p0[z]) and not bool(mh.cpu()[z].any()) and not bool(vh.cpu()[z].any())
        return max(rel(ph, p), rel(mh, m), rel(vh, v), 0.0 if still else float("inf")), 1e-5
    return run


TAIL_P = 32768 + 37         # proto_bwd_kernel: 8192 workgroups x 4 waves, one pixel per wave and step; 37 pixels take a second step
LOSS_PROTO_EDGE_CASES = [("proto edge P=%d C=%d (PP=%d)" % (P, C, 256 // ((C + 3) // 4)), case_proto_edge(P, C))
                         for P, C in ((300, 1), (300, 4), (300, 7), (1000, 60), (1000, 61), (96, 305), (97, 305), (40, 1024))]
LOSS_PROTO_EDGE_CASES += [
    ("proto edge P=%d C=12 (PP=85, grid-stride tail)" % TAIL_P, case_proto_edge(TAIL_P, 12)),
    ("feat dot4/rank4 P=%d C=12 (grid-stride tail)" % TAIL_P, case_feat4(TAIL_P, 12)),
    ("proto weights hard 50x37 -> 13x9", case_proto_weights(0, 2, 50, 37, 13, 9)),
    ("proto weights hard 7x5 -> 7x5", case_proto_weights(0, 2, 7, 5, 7, 5)),
    ("proto weights hard 3x5 -> 8x8 (upsampling)", case_proto_weights(0, 2, 3, 5, 8, 8)),
    ("proto weights hard 9x9 -> 1x1", case_proto_weights(0, 2, 9, 9, 1, 1)),
    ("proto weights soft 13x9 ldl=12", case_proto_weights(1, 3, 0, 0, 13, 9)),
    ("proto weights retrify 50x37 -> 13x9", case_proto_weights(2, 3, 50, 37, 13, 9)),
    ("proto weights retrify 20x20 -> 1x6", case_proto_weights(2, 3, 20, 20, 1, 6)),
    ("proto weights retrify 20x20 -> 6x1", case_proto_weights(2, 3, 20, 20, 6, 1)),
    ("seg loss 1x5 (below one workgroup)", case_seg_loss_edge(1, 5)),
    ("seg loss 3x33", case_seg_loss_edge(3, 33)),
    ("seg counts C=1 3x97x53", case_seg_counts(3, 97, C=1, W=53, edge=True, seed=97)),
    ("seg counts C=2 3x97x53", case_seg_counts(3, 97, C=2, W=53, edge=True, seed=98)),
    ("seg counts C=64 3x1x1", case_seg_counts(3, 1, C=64, edge=True, seed=99)),
    ("seg counts C=64 1x1x1", case_seg_counts(1, 1, C=64, edge=True, seed=100)),
    ("mc stats 3x2x37x29", case_mc_stats_edge(3, 37, 29)),
    ("adv_loss 1 + 1", case_adv_loss_edge(1, 1, 1.0, 0.01)),
    ("adv_loss 255 + 257", case_adv_loss_edge(255, 257, 0.0, 1.0)),
] + [("proto_align C=%d EMA (float64)" % C, case_proto_align_edge(C)) for C in (1, 256, 257, 1000)] \
  + [("adam n=%d steps 1, 2, 100000" % n, case_adam_edge(n)) for n in (1, 3, 255, 257)]
CASES += LOSS_PROTO_EDGE_CASES
# the two older cases that this section's rules rewrote: exact counts, device masks and weights taken as they are
LOSS_PROTO_CHANGED = ("seg counts 3x96", "proto retrify C=305 h=32")


# ------------------------------------------------------------------------------------- bf16x3: the split, and one product per output
# The dense cases above compare whole outputs with max|a - b| / max|b| at 2e-5 / 3e-5; a bf16x3 kernel that loses a third-order
# piece product stays four times below that (tests/test_precision_cases_cpu.py plants such kernels and records the figures).
# This section takes the accumulation out of the measurement:
#   * pack cases: uda_x3_pack (raw, BN + activation, + keep-mask; activation rows and weight rows) against the statement
#     SpecKernels.x3_pack, bit for bit, on a table of bit patterns;
#   * probes: every output of a dense call is ONE product x * w, all other addends exact zeros, compared per element with the
#     float64 product.  Bounds, in units of U24 = 2^-24 |x w| (derived, not fitted):
#       fp32 routes    the accumulator holds round(x w) plus exact zeros: <= 1; the probes allow 2;
#       bf16x3 routes  six exact piece products added into an fp32 accumulator (a3b1, a2b2, a1b3, a2b1, a1b2, a1b1): at most five
#                      inexact additions of <= (1 + 2^-7) each, plus the three dropped products: bf16 keeps 8 significant bits, so
#                      with pieces rounded to nearest |a2| <= 2^-8 |a|, |a3| <= 2^-16 |a| and a2b3 + a3b2 + a3b3 <= 2 (+ 2^-8):
#                      <= 7.1; the probes allow 8.  A lost a1b3 / a2b2 product measures 117 / 225, a two-piece split 373.
U24 = 2.0 ** -24
X3_PACK_GRID_CAP = 65536 * 256          # uda_x3_pack: at most 65536 workgroups of 256 octets per step of its grid-stride loop


def _i32(bits):
    b = torch.as_tensor(bits, dtype=torch.int64)
    return ((b & 0x7FFFFFFF) - (b & 0x80000000)).to(torch.int32)


@functools.lru_cache(maxsize=None)
def x3_value_table():
    """fp32 values by bit pattern, all inside the split's domain (|x| <= 0x7F7F7FFF): every exponent from the smallest normal to
    2^126 with full random mantissas and both signs (four values each), +-0, subnormals (the build keeps them), round-up carries,
    ties to even in the first and in the second piece, values whose first / second residual is negative, and the largest
    magnitudes whose bf16 rounding is finite.  An odd number of entries, so rows of 16-multiples do not repeat lane by lane."""
    g = gen(31)
    e = torch.arange(1, 254, dtype=torch.int64)
    rows = [(s << 31) | (e << 23) | torch.randint(0, 1 << 23, (253,), generator=g) for s in (0, 1, 0, 1)]
    sub = torch.randint(1, 1 << 23, (64,), generator=g) | (torch.randint(0, 2, (64,), generator=g) << 31)
    special = [0x00000000, 0x80000000,
               0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00400000, 0x00008000, 0x00018000, 0x0000FFFF, 0x00010000, 0x80010001,
               0x3F7FFFFF, 0x3FFFFFFF, 0xBF7FFFFF, 0x3F7FFF80, 0x407FFFFF, 0x7EFFFFFF, 0x00FFFFFF,          # carries
               0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F800080, 0x3F800180, 0x3F808080,          # ties
               0x3F807FFF, 0xBF807FFF, 0x3F80FFFF, 0x3F8000FF, 0x3F80807F, 0x40490FDB,                      # negative residuals
               0x7F7F7FFF, 0xFF7F7FFF, 0x7F7F0000, 0x7F123456, 0x7F7E7FFF, 0xFF7F7F80]                      # the top of the domain
    t = _i32(torch.cat(rows + [sub, torch.tensor(special, dtype=torch.int64)])).view(torch.float32)
    if t.numel() % 2 == 0:
        t = torch.cat([t, _i32([0x3EAAAAAB]).view(torch.float32)])
    assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(t.to(torch.bfloat16).float()).all())
    return t[torch.randperm(t.numel(), generator=g)]


def _x3_out(rows, K, dev):
    """a guarded buffer of uda_x3_packed_bytes(rows, K) bytes whose window is the body: the 64 trailing bytes are nobody's to write"""
    body = rows * ((K + 15) // 16) * 96
    return out_dev((1, body + 64), torch.uint8, dev, cols=body)[0], body


def _x3_pack(K, a, dev, out):
    return K.x3_pack(K._src(a) if hasattr(K, "_src") else a, a.P, a.C, dev, out=out)


def case_x3_pack_raw(P, C, seed=0, on_device=False):
    """XF 0, [P, C] activation rows with poisoned padding lanes: packed bytes == statement, bit for bit.  on_device: the operand is
    built and the statement evaluated with torch on the test's device (the grid-stride shape: half a gigabyte of operand)."""
    def run(dev):
        K = hip()
        tab = x3_value_table()
        n = tab.numel()
        if on_device:
            blk = tab[(torch.arange(509 * C) + seed) % n].reshape(509, C).to(dev)
            x = _poison(torch.empty(P, round4(C) + 4, device=dev))[:, :C]
            x.copy_(blk.repeat(-(-P // 509), 1)[:P])
            a = Act(x, 1, 1, P)
            ah = Act(ro_dev(x, dev), 1, 1, P)
        else:
            x = padded(P, C, gen(seed))
            x.copy_(tab[(torch.arange(P * C) + seed) % n].reshape(P, C))
            a = Act(x, 1, 1, P)
            ah = act_to(a, dev)
        want = SPEC.x3_pack(a, P, C)
        out, body = _x3_out(P, C, dev)
        _x3_pack(K, ah, dev, out)
        bad = out[:body] != want[:body].to(out.device)
        DETAIL.clear()
        if bool(bad.any()):
            i = int(bad.nonzero()[0]) // 2
            DETAIL.update(first_bad=dict(row=i // (48 * ((C + 15) // 16)), block=i // 48 % ((C + 15) // 16), piece=i // 16 % 3, lane=i % 16))
        return float(bad.sum()), 0.0
    return run


def case_x3_pack_rows(O, I, k, seed=0):
    """weight rows: the relayouted [O, I, k, k] weight through x3_pack_rows"""
    def run(dev):
        K = hip()
        tab = x3_value_table()
        w = tab[(torch.arange(O * I * k * k) * 7 + seed) % tab.numel()].reshape(O, I, k, k).contiguous()
        wl = ro_dev(K.relayout_ohwi(w.to(dev)), dev)
        want = SPEC.x3_pack_rows(SPEC.relayout_ohwi(w))
        out, body = _x3_out(wl.shape[0], wl.numel() // wl.shape[0], dev)
        K.x3_pack_rows(wl, out=out)
        return float((out[:body].cpu() != want[:body]).sum()), 0.0
    return run


def _quantised(x, bits):
    """x rounded to ``bits`` significant bits"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def case_x3_pack_xf(P, C, act, mask, seed=0):
    """XF 1 / XF 2: the three pieces sum (float64) to ONE fp32 value v; v lies within one fp32 ulp of x * scale + shift evaluated
    in float64 and clamped (times mask_scale 2 where kept, exactly 0 where dropped); pieces == the statement's split of v, bit for
    bit; the lanes [C, 16 nb) are zero pieces.  x carries 12 and scale 11 significant bits, so x * scale is exact in fp32 and an
    fma and a mul + add round the same sum once (no cancellation against a rounded product); shift and hence v have full
    mantissas.  Pre-activations within 1e-3 of a kink are moved away (asserted)."""
    def run(dev):
        g = gen(seed)
        K = hip()
        x = padded(P, C, g)
        x.copy_(_quantised(2.0 * torch.randn(P, C, generator=g), 12))
        scale, shift = _quantised(0.5 + torch.rand(C, generator=g), 11), 0.3 * torch.randn(C, generator=g)
        pre = lambda: x.double() * scale.double() + shift.double()
        for _ in range(4):
            near = (pre().abs() < 1e-3) | ((pre() - 6).abs() < 1e-3)
            x[near] = _quantised(x[near] + 0.25, 12)
        assert not bool(((pre().abs() < 1e-3) | ((pre() - 6).abs() < 1e-3)).any()), "pre-activation on a kink in the test input"
        m = None
        if mask:
            mb = torch.zeros(P, round4(C), dtype=torch.uint8)
            mb[:, :C] = (torch.rand(P, C, generator=g) > 0.3).to(torch.uint8)
            m = mb[:, :C]
        a = Act(x, 1, 1, P, scale, shift, act, m, 2.0 if mask else 1.0)
        out, body = _x3_out(P, C, dev)
        _x3_pack(K, act_to(a, dev), dev, out)
        nb = (C + 15) // 16
        pc = out[:body].cpu().view(torch.bfloat16).reshape(P, nb, 3, 16).permute(2, 0, 1, 3).reshape(3, P, nb * 16)
        bad = int((pc[:, :, C:].contiguous().view(torch.int16) != 0).sum())                          # lanes behind C: zero pieces
        v = pc[:, :, :C].double().sum(0)
        v32 = v.float()
        bad += int((v32.double() != v).sum()) + int((~torch.isfinite(v)).sum())            # one fp32 value
        ref = torch.clamp(pre(), 0.0, 6.0 if act == ACT_RELU6 else float("inf"))
        if mask:
            ref = ref * (m.double() * 2.0)
            bad += int((v[m == 0] != 0).sum())
        r32 = ref.float().abs()
        ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
        bad += int((((v - ref).abs() > ulp) | ((ref == 0) & (v != 0))).sum())
        want = torch.stack(SPEC.x3_split(v32))
        bad += int((want.view(torch.int16) != pc[:, :, :C].contiguous().view(torch.int16)).sum())
        return float(bad), 0.0
    return run


X3_PACK_BIG_P = X3_PACK_GRID_CAP // (2 * 128) + 3          # C = 2048: 256 octets per row; three rows are left for the second step
assert X3_PACK_BIG_P * 128 * 2 > X3_PACK_GRID_CAP
X3_PACK_CASES = [("x3 pack raw P=%d C=%d" % (P, C), case_x3_pack_raw(P, C, seed=P + C)) for C in (16, 40, 52, 304, 2048) for P in (1, 255, 257)]
X3_PACK_CASES += [
    ("x3 pack raw P=%d C=2048 (grid-stride loop takes a second step)" % X3_PACK_BIG_P, case_x3_pack_raw(X3_PACK_BIG_P, 2048, seed=5, on_device=True)),
    ("x3 pack weight rows 3x3 72->40", case_x3_pack_rows(40, 72, 3)),
    ("x3 pack weight rows 2x2 48->33", case_x3_pack_rows(33, 48, 2)),
    ("x3 pack relu P=257 C=40", case_x3_pack_xf(257, 40, ACT_RELU, False, seed=1)),
    ("x3 pack relu6 P=255 C=304", case_x3_pack_xf(255, 304, ACT_RELU6, False, seed=2)),
    ("x3 pack relu mask P=257 C=52", case_x3_pack_xf(257, 52, ACT_RELU, True, seed=3)),
    ("x3 pack relu6 mask P=255 C=2048", case_x3_pack_xf(255, 2048, ACT_RELU6, True, seed=4)),
]
CASES += X3_PACK_CASES


def _full_mantissa(shape, g, e_lo, e_hi, signed=True):
    """fp32 values +-2^e (1 + m 2^-23): e uniform in [e_lo, e_hi), all 23 mantissa bits random"""
    e = torch.randint(e_lo, e_hi, shape, generator=g)
    m = torch.randint(0, 1 << 23, shape, generator=g)
    v = torch.ldexp(1.0 + m.double() / (1 << 23), e)
    if signed:
        v = v * (2.0 * torch.randint(0, 2, shape, generator=g) - 1.0)
    return v.float()


def _tap_offset(t, k, dil, origin):
    """(dh, dw) of tap t, as SpecKernels._pad_taps lays the taps out"""
    kh, kw = divmod(t, k)
    if k == 3:
        return (kh - 1) * dil, (kw - 1) * dil
    if k == 2:
        return kh - origin, kw - origin
    return 0, 0


def _probe_operand(N, H, W, C, g, mask):
    """raw full-mantissa rows in [2^-3, 2^3), both signs; mask: a keep-mask with mask_scale 2 (an exact multiply)"""
    x = padded(N * H * W, C, g)
    x.copy_(_full_mantissa((N * H * W, C), g, -3, 3))
    m = None
    if mask:
        mb = torch.zeros(N * H * W, round4(C), dtype=torch.uint8)
        mb[:, :C] = (torch.rand(N * H * W, C, generator=g) > 0.3).to(torch.uint8)
        m = mb[:, :C]
    a = Act(x, N, H, W, None, None, ACT_NONE, m, 2.0 if mask else 1.0)
    u = x.double() if m is None else x.double() * (m.double() * 2.0)
    return a, u.reshape(N, H, W, C)


def probe_positions(Cin, T, Cout, rounds=None):
    """[rounds][Cout] flat K positions t * Cin + c of the one nonzero weight of each output channel.  rounds = None: position
    (o + r * Cout) mod Ktot in round r of ceil(Ktot / Cout) - every position is hit.  rounds = n: n // T rounds per tap, each a run
    of min(Cout, Cin) consecutive channels, the runs spread from channel 0 to the last channel."""
    Ktot = Cin * T
    o = torch.arange(Cout)
    if rounds is None:
        pos = torch.stack([(o + r * Cout) % Ktot for r in range(-(-Ktot // Cout))])
    else:
        rpt, n = rounds // T, min(Cout, Cin)
        assert rpt >= 2
        pos = torch.stack([t * Cin + (j * (Cin - n) + (rpt - 1) // 2) // (rpt - 1) + o % n for t in range(T) for j in range(rpt)])
    hit = torch.unique(pos)
    c = hit % Cin
    assert set((hit // Cin).tolist()) == set(range(T)), "a tap is never probed"
    assert set((c % 16).tolist()) == set(k % 16 for k in range(Cin)), "a lane k mod 16 is never probed"
    assert 0 in (c // 16).tolist() and (Cin - 1) // 16 in (c // 16).tolist(), "the first / last 16-block of a row is never probed"
    return pos, Ktot - hit.numel()


_PROBE_INPUTS = {}


def _probe_inputs(key, build):
    """the CPU side of a probe (operands and float64 expectations of every round), built once and kept while the same probe runs
    again (the other matrix mode, the stand-ins of tests/test_precision_cases_cpu.py); the next probe replaces it"""
    if key not in _PROBE_INPUTS:
        _PROBE_INPUTS.clear()
        _PROBE_INPUTS[key] = build()
    return _PROBE_INPUTS[key]


def _is_x3(route):
    return route.startswith(("x3", "wgrad-x3"))


def _worst(got, want):
    """(worst |got - want| / |want| over want != 0, its flat index); inf where got is not finite or not exactly 0 at want == 0"""
    zero = want == 0
    if not bool(torch.isfinite(got).all()) or bool((got[zero] != 0).any()):
        bad = (~torch.isfinite(got)) | (zero & (got != 0))
        return float("inf"), int(bad.reshape(-1).nonzero()[0])
    e = torch.where(zero, torch.zeros_like(want), (got - want).abs() / want.abs().clamp_min(1e-300))
    i = int(e.argmax())
    return float(e.reshape(-1)[i]), i


def case_conv_probe(N, H, W, Cin, Cout, k, dil, mask=False, addend=False, stats=False, origin=0, stride=1, rounds=None, dgrad=False,
                    seed=40, *, route):
    """Every output of the conv is one product: in round r output channel o has one nonzero weight, at flat K position
    probe_positions()[r][o] (tap t, channel c), full-mantissa in [0.5, 2); the operand is raw and full-mantissa.  Expected, in
    float64: x[stride * p + offset(t), c] * w, and exactly 0.0 where the tap leaves the image.  Fresh tensors in every round (the
    packed forms ride on the tensor objects).  addend: an addend of exact zeros (in place, as the accumulating input gradient runs);
    stats: a statistics accumulator, which the planner takes as "no K-split" - its sums are held to the dense cases' 2e-5;
    dgrad: the weight goes through relayout_dgrad (rows = this conv's outputs, taps flipped).
    -> (worst |y - x w| / |x w|, 2 U24 on an fp32 route, 8 U24 on a bf16x3 route)."""
    T = k * k
    pos, left_out = probe_positions(Cin, T, Cout, rounds)

    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    P = N * Ho * Wo

    def build():
        g = gen(seed)
        data = []
        for r in range(pos.shape[0]):
            a, u4 = _probe_operand(N, H, W, Cin, g, mask)
            wv = _full_mantissa((Cout,), g, -1, 1)
            t_o, c_o = pos[r] // Cin, pos[r] % Cin
            w4 = torch.zeros(Cout, Cin, k, k)
            w4[torch.arange(Cout), c_o, t_o // k, t_o % k] = wv
            want = torch.zeros(P, Cout, dtype=torch.float64)
            for t in set(t_o.tolist()):
                dh, dw = _tap_offset(t, k, dil, origin)
                pad = max(abs(dh), abs(dw))
                up = torch.nn.functional.pad(u4, (0, 0, pad, pad, pad, pad))
                tv = up[:, pad + dh:pad + dh + (Ho - 1) * stride + 1:stride, pad + dw:pad + dw + (Wo - 1) * stride + 1:stride]
                cols = (t_o == t).nonzero().reshape(-1)
                want[:, cols] = tv.reshape(P, Cin)[:, c_o[cols]] * wv[cols].double()
            data.append((a, w4, want))
        return data

    def run(dev):
        K = hip()
        declared = _declared(route, getattr(K, "mfma", 0))
        kw = {"stride": stride} if stride != 1 else {}
        worst, where = 0.0, None
        for r, (a, w4, want) in enumerate(_probe_inputs(run, build)):
            a = Act(a.x, a.N, a.H, a.W, None, None, ACT_NONE, a.mask, a.mask_scale)        # a fresh descriptor: no packed form rides on it
            t_o, c_o = pos[r] // Cin, pos[r] % Cin
            g = gen(seed + 1 + r)
            if dgrad:
                wl = K.relayout_dgrad(w4.permute(1, 0, 2, 3).flip(2, 3).contiguous().to(dev))
            else:
                wl = K.relayout_ohwi(w4.to(dev))
            wl = ro_dev(wl, dev)
            out = to_dev(padded(P, Cout, g), dev)
            ad = None
            if addend:
                out.zero_()
                ad = out
            st = out_dev((16, 2, Cout), torch.float64, dev, fill=0) if stats else None
            args = (act_to(a, dev), wl, k, dil, out, None, ad, st)
            if hasattr(K, "conv_route"):
                _check_route(K.conv_route(*args, origin=origin, **kw), route, K.mfma)
            DETAIL.clear()
            DETAIL["route"] = declared
            K.conv(*args, origin=origin, **kw)
            e, i = _worst(out.double().cpu(), want)
            if stats and e < float("inf"):
                s = st.sum(0).cpu()
                if max(rel(s[0], want.sum(0)), rel(s[1], (want ** 2).sum(0))) > 2e-5:
                    e = float("inf")
            if where is None or e > worst:
                p, o = divmod(i, Cout)
                worst, where = e, dict(round=r, row=p, column=o, k=int(pos[r][o]), tap=int(t_o[o]), channel=int(c_o[o]),
                                       expected=float(want[p, o]), got=float(out[p, o]))
        DETAIL.update(worst=where, units="%.2f" % (worst / U24), rounds=int(pos.shape[0]), k_positions_left_out=left_out)
        return worst, (8 if _is_x3(declared) else 2) * U24
    run.plan_query, run.route = _query("conv", N, H, W, Cin, Cout, k, dil, mask=mask, addend=addend, stats=stats, origin=origin, stride=stride), route
    run.k_positions_left_out = left_out
    return run


def case_dgrad_probe(N, H, W, Cin, Cout, k, dil, rounds=None, seed=41, *, route):
    """the accumulating input gradient of a conv Cin -> Cout: a conv of dy [P, Cout] towards Cin columns, added in place onto zeros"""
    return case_conv_probe(N, H, W, Cout, Cin, k, dil, addend=True, rounds=rounds, dgrad=True, seed=seed, route=route)


def wgrad_probe_pixels(N, Ho, Wo, route):
    """The pixels of dy's grid that a weight-gradient probe puts its nonzeros on: the first and the last 16 pixels of every
    pixel-range split of the planned route (S splits of ceil(chunks / S) chunks; a chunk is 16 pixels on the bf16x3 kernel, 32 on
    the wide fp32 one, 64 on the narrow one) - that is all 16 residues of the pixel index mod 16 - and the corners and edge
    midpoints of the first and the last image (first / last row and column)."""
    P = N * Ho * Wo
    chunk = 16 if route.startswith("wgrad-x3") else (32 if route.startswith("wgrad-ws") else 64)
    S = int(route.split("S=")[1].split()[0])
    nchunks = -(-P // chunk)
    cps = -(-nchunks // S)
    assert -(-nchunks // cps) == S
    px = []
    for s in range(S):
        p0, p1 = s * cps * chunk, min((s + 1) * cps * chunk, P)
        px += list(range(p0, min(p0 + 16, p1))) + list(range(max(p1 - 16, p0), p1))
    for n in (0, N - 1):
        for h, w in ((0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (0, Wo // 2), (Ho - 1, Wo // 2), (Ho // 2, 0), (Ho // 2, Wo - 1)):
            px.append((n * Ho + h) * Wo + w)
    px = list(dict.fromkeys(px))
    assert set(p % 16 for p in px) == set(range(min(16, P)))
    return torch.tensor(px)


def case_wgrad_probe(N, H, W, Cin, Cout, k, dil, mask=False, origin=0, stride=1, seed=42, *, route):
    """Every weight gradient is one product: dy has one nonzero per column o, at pixel pi(o, r) = wgrad_probe_pixels()[(r * Cout + o)
    mod n], in as many rounds as it takes to use every listed pixel.  Expected, in float64: dw[o, c, t] = dy[pi, o] *
    x[stride * pi + offset(t), c], exactly 0.0 where the offset leaves the image.  -> (worst relative error, 2 / 8 U24)."""
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Po = N * Ho * Wo
    o = torch.arange(Cout)

    def build(declared):
        g = gen(seed)
        px = wgrad_probe_pixels(N, Ho, Wo, declared)
        data = []
        for r in range(-(-px.numel() // Cout)):
            a, u4 = _probe_operand(N, H, W, Cin, g, mask)
            pi = px[(r * Cout + o) % px.numel()]
            val = _full_mantissa((Cout,), g, -3, 3)
            dy = padded(Po, Cout, g)
            dy.zero_()
            dy[pi, o] = val
            n_, oh, ow = pi // (Ho * Wo), pi // Wo % Ho, pi % Wo
            want = torch.zeros(Cout, Cin, k, k, dtype=torch.float64)
            for t in range(k * k):
                dh, dw_ = _tap_offset(t, k, dil, origin)
                ih, iw = oh * stride + dh, ow * stride + dw_
                ok = (ih >= 0) & (ih < H) & (iw >= 0) & (iw < W)
                rows = u4[n_, ih.clamp(0, H - 1), iw.clamp(0, W - 1)] * ok.double().unsqueeze(1)
                want[:, :, t // k, t % k] = rows * val.double().unsqueeze(1)
            data.append((a, dy, pi, want))
        return px, data

    def run(dev):
        K = hip()
        declared = _declared(route, getattr(K, "mfma", 0))
        kw = {"stride": stride} if stride != 1 else {}
        px, data = _probe_inputs((run, declared), lambda: build(declared))
        worst, where = 0.0, None
        R = len(data)
        for r, (a, dy, pi, want) in enumerate(data):
            a = Act(a.x, a.N, a.H, a.W, None, None, ACT_NONE, a.mask, a.mask_scale)
            out = out_dev((Cout, Cin, k, k), torch.float32, dev)
            args = (act_to(a, dev), ro_dev(dy, dev), k, dil, out)
            if hasattr(K, "wgrad_route"):
                _check_route(K.wgrad_route(*args, origin=origin, **kw), route, K.mfma)
            DETAIL.clear()
            DETAIL["route"] = declared
            K.conv_wgrad(*args, origin=origin, **kw)
            e, i = _worst(out.double().cpu(), want)
            if where is None or e > worst:
                oc, rest = divmod(i, Cin * k * k)
                c, t = divmod(rest, k * k)
                worst, where = e, dict(round=r, column=oc, channel=c, tap=t, pixel=int(pi[oc]), expected=float(want.reshape(-1)[i]),
                                       got=float(out.reshape(-1)[i]))
        DETAIL.update(worst=where, units="%.2f" % (worst / U24), rounds=R, pixels=int(px.numel()))
        return worst, (8 if _is_x3(declared) else 2) * U24
    run.plan_query, run.route = _query("wgrad", N, H, W, Cin, Cout, k, dil, mask=mask, origin=origin, stride=stride), route
    return run


# Routes and shapes (the smallest shape the planner sends each way; without statistics a short conv splits its only round of tiles
# over K, so the plain x3 128x128 routes are probed with a statistics accumulator).  K positions left out: only where said.
# The plan sends no 3x3 conv to the fp32 wide tiles in bf16x3 mode ("ws ... k3" runs in the other mode of the x3 shapes).
# Measured on an MI355X, worst per-product error in units of U24 (every probe within its derived bound, none needed explaining):
#   f32 mode, and every fp32 family in either mode (ws, low, narrow, few, stream, heads, cout1, wgrad-ws): 0.98 - 1.00
#   bf16x3 mode: x3 128x128 k3 2.45 (stride 2: 2.57, ragged 16-block: 2.45), x3 128x128 k1 2.56, x3 128x256 k1 2.59, x3 256x128 k3 2.71,
#     x3 256x256 k3 2.51, x3 256x64 k3 2.48; x3+tail 128x128 k3 2.38 (2x2 origin 1: 2.40, accumulating input gradient: 2.58),
#     x3+tail 128x128 k1 2.38, x3+tail 256x128 k3 2.64, x3+tail 128x256 k3 2.46, x3+tail 256x256 k3 2.73;
#     wgrad-x3 128x256 2.45 (2x2: 2.21, stride 2: 2.38), wgrad-x3 256x256 2.47, wgrad-x3 128x128 2.28
#   pack cases: bit-exact, fp32 subnormals included (the device keeps them, as the statement does).
PROBE_CASES = [
    ("conv probe 3x3 304->256 2x16x16 stats mask", case_conv_probe(2, 16, 16, 304, 256, 3, 1, mask=True, stats=True, route=("ws 64x128 k3 xf2", "x3 128x128 k3"))),
    ("conv probe 1x1 2048->512 P=2312 stats", case_conv_probe(2, 34, 34, 2048, 512, 1, 1, stats=True, route=("ws 64x128 k1 xf0", "x3 128x128 k1"))),
    ("conv probe 1x1 256->2304 P=2880", case_conv_probe(2, 40, 36, 256, 2304, 1, 1, route=("ws 128x256 k1 xf0", "x3 128x256 k1"))),
    ("conv probe 3x3 64->128 P=38025", case_conv_probe(1, 195, 195, 64, 128, 3, 1, route=("ws 128x128 k3 xf0", "x3 256x128 k3"))),
    ("conv probe 2x2 o0 64->160 P=49729", case_conv_probe(1, 223, 223, 64, 160, 2, 1, route=("ws 128x192 k3 xf0", "x3 256x256 k3"))),
    ("conv probe 3x3 256->48 P=2442 (18 of 48 rounds: channels 0..47 and 208..255 of every tap)",
     case_conv_probe(2, 33, 37, 256, 48, 3, 1, rounds=18, route=("low 64x64 pipe", "x3 256x64 k3"))),
    ("conv probe 3x3 256->256 P=1152 mask (tail split)", case_conv_probe(2, 24, 24, 256, 256, 3, 1, mask=True, route=("ws 64x128 k3 xf2", "x3+tail 128x128 k3 full 0 tail 18x8"))),
    ("conv probe 1x1 1536->300 P=1147 (tail split)", case_conv_probe(1, 37, 31, 1536, 300, 1, 1, route=("ws 64x128 k1 xf0", "x3+tail 128x128 k1 full 0 tail 27x8"))),
    ("conv probe 2x2 o1 384->300 P=3811 zero addend (tail split)", case_conv_probe(1, 37, 103, 384, 300, 2, 1, addend=True, origin=1, route=("ws 64x128 k3 xf0", "x3+tail 256x128 k3 full 0 tail 45x5"))),
    ("conv probe 3x3 176->512 P=2809 (tail split)", case_conv_probe(1, 53, 53, 176, 512, 3, 1, route=("ws 64x128 k3 xf0", "x3+tail 128x256 k3 full 0 tail 44x5"))),
    ("conv probe 3x3 176->512 P=38809 (tail split after a full round)", case_conv_probe(1, 197, 197, 176, 512, 3, 1, route=("ws 128x128 k3 xf0", "x3+tail 256x256 k3 full 256 tail 48x5"))),
    ("conv probe 3x3 s2 128->128 65x67", case_conv_probe(2, 65, 67, 128, 128, 3, 1, stride=2, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("conv probe 2x2 o1 384->250 P=1147 (tail split)", case_conv_probe(1, 37, 31, 384, 250, 2, 1, origin=1, route=("ws 64x128 k3 xf0", "x3+tail 128x128 k3 full 0 tail 18x8"))),
    ("conv probe 3x3 40->256 2x16x16 (ragged 16-block: Cin % 16 = 8)", case_conv_probe(2, 16, 16, 40, 256, 3, 1, route=("ws 64x128 k3 xf0", "x3 128x128 k3"))),
    ("dgrad probe 3x3 304<-256 P=1152 accumulate (tail split)", case_dgrad_probe(2, 24, 24, 304, 256, 3, 1, route=("ws 64x128 k3 xf0", "x3+tail 128x128 k3 full 0 tail 27x8"))),
    # the other forward families, fp32 in both modes
    ("conv probe 1x1 96->24 (low)", case_conv_probe(2, 17, 13, 96, 24, 1, 1, route="low 64x64 xf0")),
    ("conv probe 1x1 32->192 (narrow)", case_conv_probe(2, 12, 12, 32, 192, 1, 1, route="narrow 128x96 xf0")),
    ("conv probe 1x1 196->160 P=12285 (few)", case_conv_probe(3, 65, 63, 196, 160, 1, 1, route="few 64x192 pipe xf0")),
    ("conv probe 1x1 16->96 P=33800 (stream)", case_conv_probe(2, 130, 130, 16, 96, 1, 1, route="stream 8x3")),
    ("conv probe 1x1 100->2 (heads)", case_conv_probe(2, 17, 13, 100, 2, 1, 1, route="heads 128x2")),
    ("conv probe 2x2 o0 256->1 (cout1; 64 of 1024 positions: 16 channels 17 apart of every tap)", case_conv_probe(2, 9, 7, 256, 1, 2, 1, rounds=64, route="cout1 4x1")),
    ("conv probe 1x1 320->256 P=4 (ws 1x1)", case_conv_probe(4, 1, 1, 320, 256, 1, 1, route="ws 64x128 k1 xf0")),
    # weight gradients
    ("wgrad probe 3x3 256->256 P=4608 mask", case_wgrad_probe(2, 48, 48, 256, 256, 3, 1, mask=True, route=("wgrad-ws 128x128 xf2 S=24 red8", "wgrad-x3 128x256 S=24 red8"))),
    ("wgrad probe 3x3 64->192 P=8192", case_wgrad_probe(2, 64, 64, 64, 192, 3, 1, route=("wgrad-ws 128x128 xf0 S=64 red8", "wgrad-x3 256x256 S=64 red8"))),
    ("wgrad probe 1x1 128->1024 P=4096", case_wgrad_probe(1, 64, 64, 128, 1024, 1, 1, route=("wgrad-ws 128x128 xf0 S=32 red8", "wgrad-x3 128x128 S=32 red8"))),
    ("wgrad probe 2x2 o1 64->128 P=4608", case_wgrad_probe(2, 48, 48, 64, 128, 2, 1, origin=1, route=("wgrad-ws 128x128 xf0 S=36 red8", "wgrad-x3 128x256 S=36 red8"))),
    ("wgrad probe 3x3 s2 64->128 41 images of 20x20", case_wgrad_probe(41, 20, 20, 64, 128, 3, 1, stride=2, route=("wgrad-ws 128x128 xf0 S=26 red8", "wgrad-x3 128x256 S=26 red8"))),
    ("wgrad probe 1x1 960->320 P=128 (wgrad-ws)", case_wgrad_probe(2, 8, 8, 960, 320, 1, 1, route="wgrad-ws 128x128 xf0 S=1 red8")),
]
CASES += PROBE_CASES


# ---------------------------------------------------------------- past the grid caps: second passes, tile seams, XCD remap
# The shapes above fit one pass of every capped grid-stride loop, one LDS tile across and grids on which uda_xcd_remap is the
# identity or has r = 0.  These are the smallest shapes of their kind at which
#   - a grid-stride loop runs a second, partly filled pass (``capped=True``: work > CAP * items, work % 256 != 0; the caps are read
#     from csrc, tests/test_capped_cases_cpu.py holds the conditions and fails when a cap moves),
#   - the LDS-tiled depthwise kernels have 3 x 3 tiles x 2 images, ragged both ways (``seams=True``): a halo with real neighbours
#     on all sides, the quirk-Q1 border value owed at the IMAGE edge only, tilesX > 1 in the tile decode, more than 16 workgroups in
#     x so that blockIdx.x % UDA_STAT_SLOTS wraps,
#   - uda_xcd_remap runs with q >= 1 and r != 0 (``remap=True``: grid >= 8, grid % 8 != 0),
#   - the weight gradient's plan has more than 256 slabs and ends in wgrad_reduce_kernel<64> (declared by the route).
# Left out on purpose: upconv_fwd_kernel (pixel), upconv_bwd_kernel and upconv_bwd_wave_kernel (UPCONV_FLAT_MAX_WG = 65536) and
# x3_pack_kernel and its siblings (65536): crossing any of them takes 16.7 M work items, operands of 0.5 - 2.4 GB; they stay with the
# whole-network tests.  fda.hip, uncertainty.hip and morphometry.hip size their grids differently and have their own suites.
# The persistent tile loops of drn_head.hip are in tests/test_drn_kernels_gpu.py.
# The weight-gradient cases keep the fp32 statement: over their 90 000 - 262 144 pixels it is within 2.1e-6 of its own float64
# evaluation (measured per case: 5.1e-7, 4.0e-7, 2.0e-6, 5.8e-7), a fifteenth of the constructor's 3e-5.
# CPU statement times (16 threads): no case above 5 s; the largest is the strip4 forward at 5 x (43 -> 128) x 256 with 1.7 s.
_TILED = ("fwd tiled-8x16", "dgrad flat", "wgrad tiled-8x16")
_TILED_S2 = ("fwd tiled-8x8", "dgrad flat", "wgrad tiled-8x8")
CAPPED_CASES = [
    ("dw 1024 s2 d1 border1 97x95 (dgrad past its cap on the stride-2 branch; 6x7 tiles x 32 channel slices)",
     case_dw(1, 97, 95, 1024, 2, 1, 1, capped=True, route=_TILED_S2)),
    ("dw 1024 s1 d2 border0 96x96 (dgrad past its cap on the general branch)", case_dw(1, 96, 96, 1024, 1, 2, 0, capped=True, route=_TILED)),
]
for _b in (0, 1):
    CAPPED_CASES += [
        ("dw seams 96 s1 d1 border%d 2x19x37 (3x3 tiles)" % _b, case_dw(2, 19, 37, 96, 1, 1, _b, seams=True, route=_TILED)),
        ("dw seams 40 s1 d2 border%d 2x19x37 (3x3 tiles)" % _b, case_dw(2, 19, 37, 40, 1, 2, _b, seams=True, route=_TILED)),
        ("dw seams 96 s2 d1 border%d 2x37x43 (3x3 tiles)" % _b, case_dw(2, 37, 43, 96, 2, 1, _b, seams=True, route=_TILED_S2)),
        ("dw seams 40 s2 d2 border%d 2x37x43 (3x3 tiles)" % _b, case_dw(2, 37, 43, 40, 2, 2, _b, seams=True, route=_TILED_S2)),
    ]
CAPPED_CASES += [
    ("upconv fwd/bwd 5 x (43x43 -> 128x128) x 256, forward only (strip4 past its cap, addend shared per image)",
     case_upconv(5, 43, 43, 128, 128, 256, addend_rows=16384, fwd_only=True, capped=True, route=("fwd strip4", "bwd wave"))),
    ("upconv fwd/bwd 7 x (25x25 -> 100x100) x 256, forward only (strip3 past its cap, addend shared per image)",
     case_upconv(7, 25, 25, 100, 100, 256, addend_rows=10000, fwd_only=True, capped=True, route=("fwd strip3", "bwd wave"))),
    ("upconv fwd/bwd 1 x (13x4 -> 52x16) x 64 (strip3 on 13 workgroups: XCD remap)", case_upconv(1, 13, 4, 52, 16, 64, remap=True, route=("fwd strip3", "bwd thread"))),
    ("upconv fwd/bwd 1 x (26x8 -> 52x16) x 64 (strip4 on 13 workgroups: XCD remap)", case_upconv(1, 26, 8, 52, 16, 64, remap=True, route=("fwd strip4", "bwd thread"))),
    ("upconv fwd/bwd 1 x (12x12 -> 48x48) x 32 (tile kernel on 9 workgroups: XCD remap)", case_upconv(1, 12, 12, 48, 48, 32, remap=True, route=("fwd tile", "bwd thread"))),
    ("upconv fwd/bwd 3 x (12x12 -> 48x48) x 32, addend (tile kernel on 27 workgroups: XCD remap)",
     case_upconv(3, 12, 12, 48, 48, 32, addend_rows=2304, remap=True, route=("fwd tile", "bwd thread"))),
    ("wgrad1x1 24->48 P=90000 (282 slabs, red64, 64x64 tiles)", case_wgrad(1, 300, 300, 24, 48, 1, 1, route="wgrad 64x64 S=282 red64")),
    ("wgrad1x1 16->96 P=90000 mask (282 slabs, red64, 128x32 tiles)", case_wgrad(1, 300, 300, 16, 96, 1, 1, mask=True, route="wgrad 128x32 S=282 red64")),
    ("wgrad3x3 16->16 P=135000 (422 slabs, red64, 32x128 tiles)", case_wgrad(1, 375, 360, 16, 16, 3, 1, route="wgrad 32x128 S=422 red64")),
    ("wgrad1x1 24->48 P=262144 (the slab cap: 1024 slabs, red64)", case_wgrad(4, 256, 256, 24, 48, 1, 1, route="wgrad 64x64 S=1024 red64")),
    ("upsample 257x259->301x299 C=256 (forward and backward past their cap)", case_resample(1, 257, 259, 301, 299, 256, capped=True)),
    ("upsample + stats 65x65->257x257 C=64 into 72 (past the statistics kernel's cap)", case_upsample_stats(1, 65, 65, 257, 257, 64, 72, capped=True)),
    ("head 2049x2051->2051x2053 C=1 (forward and backward past their cap)", case_head(1, 2049, 2051, 2051, 2053, 1, capped=True)),
    ("gap C=256 3 x 25001 (broadcast_rows past its cap)", case_gap(3, 25001, 256, capped=True)),
    ("dropout p=.5 140001 x 256 (past its cap)", case_dropout(140001, 256, 0.5, capped=True)),
    ("s2d rows C=64 513x513 (4 channels per thread, forward and backward past their cap)", case_s2d(1, 513, 513, 64, False, capped=True)),
    ("s2d nchw C=1 2049x2051 (scalar path, forward and backward past their cap)", case_s2d(1, 2049, 2051, 1, True, capped=True)),
    ("adv_s2d sigmoid C=1 2049x2051 (past the cap)", case_adv_s2d(1, 1, 2049, 2051, 1, capped=True)),
    ("adv_s2d entropy C=2 1449x1451 (past the cap)", case_adv_s2d(1, 2, 1449, 1451, 2, capped=True)),
    ("relayout s2d 497<-264 (both operands past the cap)", case_relayout_s2d(497, 264, capped=True)),
    ("relayout ohwi / dgrad 455x260x3x3 (past the cap)", case_relayout(455, 260, 3, capped=True)),
]
CASES += CAPPED_CASES


# every case begins with a cleared footprint registry and runs with guarded workspaces (footprint_violations() after it)
CASES = [(name, footprinted(fn)) for name, fn in CASES]
