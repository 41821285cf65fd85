"""not-gpu: the launch plans of the depthwise 3x3 convolution and the 3 -> 32 stem.  The routing rule is written out here and held
against the library's planner (uda_dwconv_route) over every channel count; the workspace query against its formula; and the
planner's whole repertoire (uda_dwconv_route_list, the four stem routes) against the routes the GPU kernel cases declare, so that
no depthwise or stem kernel the library can choose goes without a case that runs it."""
import os

import pytest

import dw_shapes as XS
from kernel_cases import CASES, _entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")

OPS = ("fwd", "dgrad", "wgrad")
CHANNELS = list(range(4, 2053, 4)) + [2056, 2, 6, 0]
_DW = [(n, fn) for n, fn in CASES if hasattr(fn, "dw_query")]
_STEM = [(n, fn) for n, fn in CASES if hasattr(fn, "stem_query")]


@pytest.fixture(scope="module")
def K():
    from uda_clr_amd.kernels import HipKernels
    return HipKernels()


def _auto(op, C, stride, dil):
    """what the library chooses by shape"""
    if C % 4 or C < 4:
        return "none"
    if C > 1024 or (dil > 2 and C >= 1024):                    # channel-blocked: up to 2048 channels
        return op + " cb" if C <= 2048 else "none"
    if op == "dgrad" or dil > 2:
        return op + " flat"
    return op + (" tiled-8x16" if stride == 1 else " tiled-8x8")


def _pinned(op, family, C, stride, dil):
    """what a pinned family serves"""
    if C % 4 or C < 4:
        return "none"
    if family == "cb":
        return op + " cb" if C <= 2048 else "none"
    if op == "dgrad":                                          # flat: no upper bound on C; there is no tiled input gradient
        return "dgrad flat" if family == "flat" else "none"
    if C > 1024:
        return "none"
    if family == "flat":
        return op + " flat"
    if dil > 2:
        return "none"
    return op + (" tiled-8x16" if stride == 1 else " tiled-8x8")


def test_auto_route_follows_the_rule_at_every_width(K):
    wrong = {}
    for op in OPS:
        for C in CHANNELS:
            for stride in (1, 2):
                for dil in (1, 2, 4):
                    got = _entry(K.dw_route(op, 2, 9, 7, C, stride, dil))
                    if got != _auto(op, C, stride, dil):
                        wrong[(op, C, stride, dil)] = (got, _auto(op, C, stride, dil))
    assert not wrong, dict(list(wrong.items())[:8])
    assert _entry(K.dw_route("dgrad", 2, 9, 7, 2056, 1, 1)) == "none" and _entry(K.dw_route("dgrad", 2, 9, 7, 2056, 1, 1, "flat")) == "dgrad flat"


@pytest.mark.parametrize("family", ["flat", "tiled", "cb"])
def test_pinned_family_serves_what_it_can_and_nothing_else(K, family):
    wrong = {}
    for op in OPS:
        for C in CHANNELS:
            for stride in (1, 2):
                for dil in (1, 2, 4):
                    got = _entry(K.dw_route(op, 2, 9, 7, C, stride, dil, family))
                    if got != _pinned(op, family, C, stride, dil):
                        wrong[(op, C, stride, dil)] = (got, _pinned(op, family, C, stride, dil))
    assert not wrong, dict(list(wrong.items())[:8])


def test_bad_geometry_and_unknown_names_have_no_route(K):
    assert K.dw_route("fwd", 2, 9, 7, 64, 3, 1) == "none" and K.dw_route("fwd", 2, 9, 7, 64, 1, 0) == "none"
    assert K.dw_route("wgrad", 0, 9, 7, 64, 1, 1) == "none"
    buf = __import__("ctypes").create_string_buffer(32)
    K.lib.uda_dwconv_route(3, 2, 9, 7, 64, 1, 1, 0, buf, len(buf))
    assert buf.value == b"none"
    K.lib.uda_dwconv_route(0, 2, 9, 7, 64, 1, 1, 4, buf, len(buf))
    assert buf.value == b"none"
    with pytest.raises(ValueError):
        K.dw_route("fwd", 2, 9, 7, 64, 1, 1, "blocked")


@pytest.mark.parametrize("Pout,C", [(1, 4), (300, 64), (1 << 20, 960), (4096, 1024), (4096, 1028), (100, 2048)])
def test_workspace_bytes_keep_their_values(K, Pout, C):
    want = 16 * 9 * C * 8                                       # fp64 slot replicas: tiled and channel-blocked
    if C <= 1024:                                               # flat: one partial row per workgroup of 256 // (C // 4) lanes x 32 pixels
        want = max(want, -(-Pout // ((256 // (C // 4)) * 32)) * 9 * C * 4 + 9 * C * 8)
    assert K.lib.uda_dwconv_workspace_bytes(Pout, C) == want


def test_workspace_bytes_of_fewer_than_four_channels(K):
    for C in (0, 2, 3):
        assert K.lib.uda_dwconv_workspace_bytes(300, C) == 0


def test_depthwise_cases_declare_what_the_library_plans(K):
    assert len(_DW) >= 7
    for name, fn in _DW:
        q = fn.dw_query
        got = tuple(_entry(K.dw_route(op, q["N"], q["H"], q["W"], q["C"], q["stride"], q["dil"])) for op in OPS)
        assert got == tuple(fn.route), name


def test_xception_shapes_declare_what_the_library_plans(K):
    assert len(XS.ROUTED) == len(XS.SHAPES)
    for shape in XS.SHAPES:
        N, H, W, C, stride, dil, lazy = shape
        for family in ("", "cb"):
            got = tuple(_entry(K.dw_route(op, N, H, W, C, stride, dil, family)) for op in OPS)
            assert got == XS.declared(family, shape), (shape, family)


def test_every_depthwise_route_is_declared_by_a_case(K):
    entries = K.lib.uda_dwconv_route_list().decode().split("\n")
    assert len(entries) == 10 and len(set(entries)) == 10 and all(len(e.split()) == 2 for e in entries), entries
    declared = {r for _, fn in _DW for r in fn.route}
    declared |= {r for shape in XS.SHAPES for family in ("", "cb") for r in XS.declared(family, shape)}      # what the Xception kernel test asserts
    unrun = [e for e in entries if e not in declared]
    assert not unrun, "no kernel case runs %s" % unrun
    assert not declared - set(entries), "declared by a case, missing from uda_dwconv_route_list: %s" % (declared - set(entries))


def test_stem_cases_declare_what_the_library_plans_and_cover_the_four_routes(K):
    import ctypes
    declared = set()
    for name, fn in _STEM:
        q = fn.stem_query
        buf = ctypes.create_string_buffer(64)
        got = []
        for op, lddy, al in ((0, 0, 0), (2, q["lddy"], int(q["aligned"]))):
            K.lib.uda_stem_route(op, q["N"], q["H"], q["W"], lddy, al, buf, len(buf))
            got.append(_entry(buf.value.decode()))
        assert tuple(got) == tuple(fn.route), name
        declared |= set(fn.route)
    assert declared == {"fwd rows", "fwd pixels", "wgrad rows", "wgrad pixels"}
    buf = ctypes.create_string_buffer(64)
    K.lib.uda_stem_route(1, 2, 32, 32, 36, 1, buf, len(buf))          # the stem has no input gradient
    assert buf.value == b"none"
