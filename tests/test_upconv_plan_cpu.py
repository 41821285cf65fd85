"""not-gpu: the launch plan of the decoder's interpolation pass (uda_upconv_fwd / uda_upconv_bwd, csrc/upconv_plan.h).  The routing
rule is written out here in numpy.float32 and held against the library's planner (uda_upconv_route) over a sweep of geometries and
on both sides of every 32-bit extent; the routes the GPU kernel cases declare against the planner; and the planner's repertoire
(uda_upconv_route_list) against the declared routes, so that no upconv kernel the library can choose goes without a case that runs
it.  Plan queries only: nothing here allocates or runs an operand."""
import ctypes
import functools
import os

import numpy as np
import pytest

from kernel_cases import CASES, upconv_routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")

F = np.float32
LIM32 = 1 << 31
_UP = [(n, fn) for n, fn in CASES if n.startswith("upconv fwd/bwd")]
PAIRS = [(43, 128), (83, 128), (84, 128), (85, 128), (86, 128), (32, 128), (5, 17), (9, 33), (9, 32), (5, 16), (16, 48), (16, 64)]   # the cases' (w, W)


@pytest.fixture(scope="module")
def K():
    from uda_clr_amd.kernels import HipKernels
    return HipKernels()


# ---- the rule
@functools.lru_cache(maxsize=None)
def _scale(n_in, n_out):
    return F(n_in - 1) / F(n_out - 1) if n_out > 1 else F(0)


def _foot(o_min, o_max, scale, n_in, n_out):
    """rows (columns) of g a tile whose tap positions span [o_min, o_max] blends"""
    lo, hi = int(scale * F(max(o_min, 0))), int(scale * F(min(o_max, n_out - 1)))
    lo, hi = min(lo, n_in - 1), min(hi, n_in - 1)
    return hi + (1 if hi < n_in - 1 else 0) - lo + 1


@functools.lru_cache(maxsize=None)
def _side(n_in, n_out):
    """of one image side: 3 * scale < 0.98, 3 * scale < 1.96, the tile kernel's largest footprint, the wave kernel's table fits"""
    s = _scale(n_in, n_out)
    r = max([_foot(t * 16 - 1, t * 16 + 16, s, n_in, n_out) for t in range(n_out // 16)] + [1])
    return F(3) * s < F(0.98), F(3) * s < F(1.96), r, bool(s > 0 and F(2) / s + F(6) <= F(32))


def _grid(threads, cap):
    return min(-(-threads // 256), cap)


def rule(op, N, h, w, H, W, C, dil, ldg, ld_add=None, addend_rows=0, stats=False):
    """the route text uda_upconv_route must give"""
    if min(N, h, w, H, W) <= 0 or dil < 1 or C <= 0 or C % 4 or ldg % 4 or ldg < 9 * C:
        return "none"
    G = C // 4
    if op == "bwd":
        wave = C == 256 and dil == 1 and _side(h, H)[3] and _side(w, W)[3] and N * h * w < LIM32
        return "bwd wave grid %d" % _grid(N * h * w * 64, 65536) if wave else "bwd thread grid %d" % _grid(N * h * w * G, 65536)
    if ld_add is not None and (ld_add % 4 or ld_add < C or addend_rows <= 0 or (N * H * W) % addend_rows):
        return "none"
    nc3, nc4, RC, _ = _side(w, W)
    strips = N * H * (W // 4) * G
    fits32 = N * H * W < LIM32 and strips < LIM32 - 65536 * 256 and N * h * w * ldg * 4 < LIM32 and \
        (ld_add is None or addend_rows * ld_add < 4 * LIM32)
    if not (H % 4 == 0 and W % 4 == 0 and dil == 1 and nc4 and 256 % G == 0 and fits32):
        return "fwd pixel grid %d" % _grid(N * H * W * G, 65536) + (" stats colstats" if stats else "")
    tail = " stats fused" if stats else ""
    R = _side(h, H)[2]
    if nc3 and H % 16 == 0 and W % 16 == 0 and C % 32 == 0 and R * RC * 1152 <= 57344 and N * (H // 16) * (W // 16) * (C // 32) < LIM32:
        return "fwd tile grid %d R %d RC %d lds %d" % (N * (H // 16) * (W // 16) * (C // 32), R, RC, R * RC * 1152) + tail
    return "fwd strip%d grid %d" % (3 if nc3 else 4, _grid(strips, 4096)) + tail


_BUF = ctypes.create_string_buffer(96)


def planned(K, op, N, h, w, H, W, C, dil, ldg, ld_add=None, addend_rows=0, stats=False):
    K.lib.uda_upconv_route(0 if op == "fwd" else 1, N, h, w, H, W, C, dil, ldg, int(ld_add is not None), ld_add or 0, addend_rows, int(stats),
                           _BUF, len(_BUF))
    return _BUF.value.decode()


# ---- rule against planner
@pytest.mark.parametrize("dil", [1, 2])
def test_route_follows_the_rule_over_the_sweep(K, dil):
    sides_h = [(h, H) for h in range(1, 21) for H in (4, 12, 13, 16, 17, 32, 48, 128)] + PAIRS
    sides_w = [(w, W) for w in range(1, 21) for W in (4, 12, 13, 16, 17, 32, 48, 128)] + PAIRS
    wrong, seen = {}, set()
    for C in (4, 8, 12, 32, 36, 64, 256):
        for h, H in sides_h:
            for w, W in sides_w:
                for op in ("fwd", "bwd"):
                    want = rule(op, 2, h, w, H, W, C, dil, 9 * C, stats=op == "fwd")
                    got = planned(K, op, 2, h, w, H, W, C, dil, 9 * C, stats=op == "fwd")
                    seen.add(" ".join(want.split()[:2]))
                    if got != want:
                        wrong[(op, h, w, H, W, C)] = (got, want)
    assert not wrong, (len(wrong), dict(list(wrong.items())[:8]))
    if dil == 1:
        assert seen == set(K.lib.uda_upconv_route_list().decode().split("\n")), seen
    else:
        assert seen == {"fwd pixel", "bwd thread"}, seen


def test_without_statistics_and_with_an_addend_the_kernel_is_the_same(K):
    for h, w, H, W, C in ((8, 8, 32, 32, 64), (16, 16, 32, 32, 32), (5, 7, 13, 18, 8), (4, 4, 16, 16, 16)):
        base = planned(K, "fwd", 2, h, w, H, W, C, 1, 9 * C)
        assert base == rule("fwd", 2, h, w, H, W, C, 1, 9 * C) and "stats" not in base
        assert planned(K, "fwd", 2, h, w, H, W, C, 1, 9 * C + 8, C + 4, H * W, True).startswith(base + " stats ")


def test_refused_arguments_have_no_route(K):
    ok = dict(N=2, h=4, w=4, H=16, W=16, C=16, dil=1, ldg=144)
    assert planned(K, "fwd", **ok) == "fwd strip3 grid 2"
    for bad in (dict(N=0), dict(h=0), dict(W=0), dict(dil=0), dict(C=0), dict(C=6), dict(ldg=140), dict(ldg=146),
                dict(ld_add=12, addend_rows=512), dict(ld_add=18, addend_rows=512), dict(ld_add=16, addend_rows=0), dict(ld_add=16, addend_rows=96)):
        q = dict(ok, **bad)
        assert planned(K, "fwd", **q) == rule("fwd", **q) == "none", bad
    assert planned(K, "bwd", **dict(ok, ld_add=12, addend_rows=7)) == "bwd thread grid 1"        # the adjoint has no addend to refuse
    K.lib.uda_upconv_route(2, 2, 4, 4, 16, 16, 16, 1, 144, 0, 0, 0, 0, _BUF, len(_BUF))
    assert _BUF.value == b"none"
    assert K.lib.uda_upconv_route(0, 2, 4, 4, 16, 16, 16, 1, 144, 0, 0, 0, 0, None, 0) == -1
    with pytest.raises(KeyError):
        K.upconv_route("dgrad", 2, 4, 4, 16, 16, 16)


# ---- the 32-bit extents of the strip, tile and wave kernels: (what, arguments just below, just above, entry below, entry above)
EXTENTS = [
    ("output pixels N*H*W < 2^31", dict(N=131071, h=1, w=1, H=128, W=128, C=4, ldg=36), dict(N=131072), "fwd strip3", "fwd pixel"),
    ("strips N*H*(W/4)*(C/4) < 2^31 - 65536*256", dict(N=520191, h=1, w=1, H=64, W=64, C=16, ldg=144), dict(N=520192), "fwd strip3", "fwd pixel"),
    ("bytes of g N*h*w*ldg*4 < 2^31: 228 images, the doubled MC batch of 114 per GPU", dict(N=227, h=32, w=32, H=128, W=128, C=256, ldg=2304,
                                                                                         ld_add=256, addend_rows=16384), dict(N=228), "fwd tile", "fwd pixel"),
    ("the same on the strip kernel (x2)", dict(N=58254, h=2, w=2, H=4, W=4, C=256, ldg=2304), dict(N=58255), "fwd strip4", "fwd pixel"),
    ("addend elements addend_rows*ld_add < 2^33", dict(N=1, h=1, w=1, H=4, W=4, C=4, ldg=36, ld_add=(1 << 29) - 4, addend_rows=16),
     dict(ld_add=1 << 29), "fwd strip3", "fwd pixel"),
    ("low-resolution pixels N*h*w < 2^31 (wave kernel)", dict(N=536870911, h=2, w=2, H=4, W=4, C=256, ldg=2304), dict(N=536870912),
     "bwd wave", "bwd thread"),
]


@pytest.mark.parametrize("what,below,step,e_below,e_above", EXTENTS, ids=[e[0] for e in EXTENTS])
def test_each_32_bit_extent_from_both_sides(K, what, below, step, e_below, e_above):
    op = e_below.split()[0]
    for q, entry in ((below, e_below), (dict(below, **step), e_above)):
        got = planned(K, op, dil=1, stats=op == "fwd", **q)
        assert got == rule(op, dil=1, stats=op == "fwd", **q) and got.startswith(entry + " grid "), (what, q, got)
        if op == "fwd":
            assert got.endswith(" stats colstats" if entry == "fwd pixel" else " stats fused"), (what, q, got)


def test_the_tile_grid_cannot_reach_its_extent(K):
    """nwg = N*(H/16)*(W/16)*(C/32) < 2^31 is implied: C/4 divides 256, so nwg <= N*H*W/8 < 2^28.  The widest tile launch the other
    extents admit is planned as a tile and its grid is exact."""
    q = dict(N=58254, h=1, w=1, H=16, W=16, C=1024, dil=1, ldg=9216)          # N*h*w*ldg*4 = 2^31 - 8192
    got = planned(K, "fwd", stats=True, **q)
    assert got == rule("fwd", stats=True, **q) == "fwd tile grid %d R 1 RC 1 lds 1152 stats fused" % (58254 * 32)
    assert planned(K, "fwd", stats=True, **dict(q, N=58255)) == "fwd pixel grid 65536 stats colstats"


# ---- cases against planner
def test_upconv_cases_declare_what_the_library_plans(K):
    assert len(_UP) >= 19
    for name, fn in _UP:
        assert getattr(fn, "route", None), "no declared route: " + name
        assert upconv_routes(K, fn.upconv_query) == tuple(fn.route), name


def test_every_upconv_route_is_declared_by_a_case(K):
    entries = K.lib.uda_upconv_route_list().decode().split("\n")
    assert len(entries) == 6 and len(set(entries)) == 6 and all(len(e.split()) == 2 for e in entries), entries
    declared = {r for _, fn in _UP for r in fn.route}
    unrun = [e for e in entries if e not in declared]
    assert not unrun, "no kernel case runs %s" % unrun
    assert not declared - set(entries), "declared by a case, missing from uda_upconv_route_list: %s" % (declared - set(entries))
