"""not-gpu: the kernel cases that are there to take a launch past its workgroup cap, across a tile seam or through the XCD remap
(kernel_cases.CAPPED_CASES, the *_CAPPED lists of test_drn_kernels_gpu.py) do so.  A grid-stride launch takes
grid = min(ceil(work / items), CAP) workgroups; its case must have work > CAP * items (a second pass), work % (CAP * items) != 0 (the
last pass partly filled) and work % 256 != 0.  CAP is read from its plain-number #define in uda_clr_amd/csrc (kernel_cases.cap_value),
the grid from the library's route query where there is one (uda_dwconv_route, uda_upconv_route), else from the same formula.  A
cap that is raised turns a two-pass case into a one-pass one: this module then fails and names the case.  Plan queries and
arithmetic only: nothing here allocates or runs an operand.

Left out on purpose: upconv_fwd_kernel (pixel), upconv_bwd_kernel, upconv_bwd_wave_kernel (UPCONV_FLAT_MAX_WG) and x3_pack_kernel
with its siblings, caps of 65536: crossing one takes 16.7 M work items, operands of 0.5 - 2.4 GB; they stay with the whole-network
tests.  fda.hip, uncertainty.hip and morphometry.hip size their grids differently and have their own suites.  Three launches are a
multiple of 256 work items at every shape of their kind and say why (Capped.whole): 256 channel groups (C = 1024 on the flat
depthwise input gradient, C = 256 on the strip kernels, whose rows come in fours) and the dgrad operand of relayout_s2d."""
import math
import os
import re

import pytest

import kernel_cases as kc
from kernel_cases import CAPPED_CASES, CASES, cap_value, plan_route, upconv_routes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")

CAPS = ("RESAMPLE_MAX_WG", "UPSAMPLE_STATS_MAX_WG", "S2D_MAX_WG", "RELAYOUT_S2D_MAX_WG", "RELAYOUT_MAX_WG", "WGRAD_REDUCE_MAX_WG",
        "DW_DGRAD_MAX_WG", "UPCONV_STRIP_MAX_WG", "UPCONV_FLAT_MAX_WG", "H7W_MAX_WG", "N3_MAX_WG_SMALL", "N3_MAX_WG_LARGE")
STAT_SLOTS = 16            # UDA_STAT_SLOTS


@pytest.fixture(scope="module")
def K():
    from uda_clr_amd.kernels import HipKernels
    return HipKernels()


def _grid(route):
    """the numbers behind "grid" in a route text: "dgrad flat grid 8192" -> (8192,), "fwd tiled-8x16 grid 18x3 lds 23040" -> (18, 3)"""
    m = re.search(r" grid (\d+)(?:x(\d+))?", route)
    assert m, route
    return tuple(int(v) for v in m.groups() if v is not None)


def _two_passes(name, cap, grid):
    """the conditions of a capped launch, against the grid the library plans (or its formula)"""
    limit = cap_value(cap.cap) * cap.items
    what = "%s: %s (%s = %d)" % (name, cap.launch, cap.cap, cap_value(cap.cap))
    assert grid == cap_value(cap.cap), "%s: grid %d is not the cap" % (what, grid)
    assert cap.work > limit, "%s: %d work items fit one pass of %d" % (what, cap.work, limit)
    assert cap.work % limit != 0, "%s: %d work items fill the last pass" % (what, cap.work)
    assert cap.passes() == -(-cap.work // limit) >= 2, what
    assert cap.work % 256 != 0 or cap.whole, "%s: %d work items are a multiple of 256" % (what, cap.work)


def test_every_cap_is_a_plain_number_in_csrc():
    for name in CAPS:
        assert cap_value(name) >= 256 and cap_value(name) % 256 == 0, name
    with pytest.raises(KeyError):
        cap_value("NO_SUCH_CAP")


def test_the_capped_cases_are_kernel_cases():
    names = [n for n, _ in CASES]
    assert len(set(names)) == len(names)
    assert all(n in names for n, _ in CAPPED_CASES)
    used = {c.cap for _, fn in CAPPED_CASES for c in getattr(fn, "capped", [])}
    assert used == {"RESAMPLE_MAX_WG", "UPSAMPLE_STATS_MAX_WG", "S2D_MAX_WG", "RELAYOUT_S2D_MAX_WG", "RELAYOUT_MAX_WG", "DW_DGRAD_MAX_WG",
                    "UPCONV_STRIP_MAX_WG"}, used
    launches = {c.launch.split()[0] for _, fn in CAPPED_CASES for c in getattr(fn, "capped", [])}
    assert launches >= {"dwconv_dgrad_kernel", "upconv_fwd_strip_kernel", "upsample_fwd_kernel", "upsample_fwd_kernel<true,", "upsample_bwd_kernel",
                        "head_upsample_fwd_kernel", "head_upsample_bwd_kernel", "broadcast_rows_kernel", "dropout_mask_kernel", "s2d_fwd_kernel",
                        "s2d_fwd4_kernel", "s2d_bwd_kernel", "s2d_bwd4_kernel", "relayout_s2d_kernel", "relayout_ohwi_kernel",
                        "relayout_dgrad_kernel"}, launches


def test_row_lengths_of_the_relayouted_weights(K):
    """kernel_cases._k_row, from which the relayout cases count their work items, against the shapes the bindings allocate"""
    from uda_clr_amd.kernels import conv_weight_shape
    for rows, k, chan in ((455, 3, 260), (260, 3, 455), (497, 2, 1056), (1056, 2, 497), (64, 2, 8), (7, 1, 305), (3, 3, 20)):
        assert rows * kc._k_row(chan, k * k) == math.prod(conv_weight_shape(rows, k, chan)), (rows, k, chan)


def test_depthwise_cases_past_the_cap(K):
    got = [(n, fn) for n, fn in CAPPED_CASES if hasattr(fn, "dw_query") and fn.capped]
    assert len(got) == 2 and {(fn.dw_query["stride"], fn.dw_query["dil"]) for _, fn in got} == {(2, 1), (1, 2)}      # the stride-2 branch and the general loop
    for name, fn in got:
        q = fn.dw_query
        (cap,) = fn.capped
        assert cap.work == q["N"] * q["H"] * q["W"] * (q["C"] // 4) and (cap.whole is None or q["C"] // 4 % 256 == 0)
        route = K.dw_route("dgrad", q["N"], q["H"], q["W"], q["C"], q["stride"], q["dil"])
        assert route.startswith("dgrad flat grid "), (name, route)
        _two_passes(name, cap, _grid(route)[0])


def test_depthwise_seam_cases_have_neighbours_on_every_side(K):
    got = [(n, fn) for n, fn in CAPPED_CASES if getattr(fn, "seams", False)]
    assert len(got) == 8 and {fn.route[0] for _, fn in got} == {"fwd tiled-8x16", "fwd tiled-8x8"}
    for name, fn in got:
        q = fn.dw_query
        Ho, Wo = (q["H"] - 1) // q["stride"] + 1, (q["W"] - 1) // q["stride"] + 1
        for op in ("fwd", "wgrad"):
            route = K.dw_route(op, q["N"], q["H"], q["W"], q["C"], q["stride"], q["dil"])
            TH, TW = (int(v) for v in re.match(r"\w+ tiled-(\d+)x(\d+) ", route).groups())
            gx, gy = _grid(route)
            tilesX, tilesY = -(-Wo // TW), -(-Ho // TH)
            assert gx == tilesX * tilesY * q["N"] and gy == -(-q["C"] // 32), (name, route)
            assert tilesX >= 3 and tilesY >= 3 and q["N"] >= 2, (name, route)            # a tile with neighbours on all four sides, in a second image
            assert Wo % TW and Ho % TH, (name, "not ragged")
            assert gx > STAT_SLOTS, (name, "blockIdx.x % UDA_STAT_SLOTS does not wrap")
    assert {(fn.dw_query["stride"], fn.dw_query["dil"]) for _, fn in got} == {(1, 1), (1, 2), (2, 1), (2, 2)}


def test_upconv_cases_past_the_cap_and_through_the_remap(K):
    capped = [(n, fn) for n, fn in CAPPED_CASES if hasattr(fn, "upconv_query") and fn.capped]
    assert {fn.route[0] for _, fn in capped} == {"fwd strip3", "fwd strip4"}
    for name, fn in capped:
        q = fn.upconv_query
        (cap,) = fn.capped
        assert cap.work == q["N"] * q["H"] * (q["W"] // 4) * (q["C"] // 4) and (cap.whole is None or (q["C"] // 4 * 4) % 256 == 0)
        route = K.upconv_route("fwd", q["N"], q["h"], q["w"], q["H"], q["W"], q["C"], q["dil"], q["ldg"], q["ld_add"], q["addend_rows"], stats=True)
        assert route.endswith("stats fused") and upconv_routes(K, q) == tuple(fn.route), (name, route)
        _two_passes(name, cap, _grid(route)[0])
        assert 0 < q["addend_rows"] < q["N"] * q["H"] * q["W"]          # the addend is shared: its row wraps inside the launch
    remap = [(n, fn) for n, fn in CAPPED_CASES if getattr(fn, "remap", False)]
    assert sorted(fn.route[0] for _, fn in remap) == ["fwd strip3", "fwd strip4", "fwd tile", "fwd tile"]
    for name, fn in remap:
        q = fn.upconv_query
        route = K.upconv_route("fwd", q["N"], q["h"], q["w"], q["H"], q["W"], q["C"], q["dil"], q["ldg"], q["ld_add"], q["addend_rows"], stats=True)
        grid = _grid(route)[0]
        assert grid >= 8 and grid % 8 != 0, "%s: on a grid of %d uda_xcd_remap is the identity or has no remainder" % (name, grid)


def test_weight_gradient_cases_end_in_the_64_lane_reduction(K):
    got = [(n, fn) for n, fn in CAPPED_CASES if hasattr(fn, "plan_query")]
    assert len(got) == 4
    tiles = set()
    for name, fn in got:
        for mode in (K.MFMA_F32, K.MFMA_BF16X3):
            K.mfma = mode
            route = plan_route(K, fn.plan_query)
            assert route == fn.route and route.endswith(" red64"), (name, route)
            assert int(re.search(r" S=(\d+) ", route).group(1)) > 256, (name, route)
            tiles.add(route.split()[1])
    assert tiles == {"64x64", "128x32", "32x128"}
    assert max(int(re.search(r" S=(\d+) ", fn.route).group(1)) for _, fn in got) == 1024          # one case at the slab cap


def test_launches_without_a_route_query_run_past_their_cap():
    seen = 0
    for name, fn in CAPPED_CASES:
        if hasattr(fn, "dw_query") or hasattr(fn, "upconv_query"):
            continue
        for cap in getattr(fn, "capped", []):
            _two_passes(name, cap, cap.grid())
            seen += 1
    assert seen == 19


def test_drn_shapes_past_the_persistent_tile_caps():
    """stem7s1_wgrad_kernel and conv3n_wgrad_kernel walk their tiles with min(tiles, cap) workgroups, one partial row of the workspace
    each: more tiles than the cap, and not a whole number of rounds"""
    import test_drn_kernels_gpu as drn
    assert len(drn.STEM_CAPPED) >= 1 and len(drn.CONV_CAPPED) >= 3
    for N, H, W in drn.STEM_CAPPED:
        tiles, cap = N * -(-H // 8) * -(-W // 64), cap_value("H7W_MAX_WG")          # H7W_TH x H7_TW
        assert cap < tiles < 2 * cap, ("stem7s1_wgrad", (N, H, W), tiles, cap)
    caps = set()
    for N, H, W, Cin, Cout, stride, lazy in drn.CONV_CAPPED:
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        th = 8 if stride == 1 and Cout < 64 else 4
        name = "N3_MAX_WG_SMALL" if Cin * Cout <= 512 else "N3_MAX_WG_LARGE"
        tiles, cap = N * -(-Ho // th) * -(-Wo // 32), cap_value(name)
        assert cap < tiles < 2 * cap, ("conv3n_wgrad", (N, H, W, Cin, Cout, stride), tiles, name, cap)
        caps.add((name, stride))
    assert caps >= {("N3_MAX_WG_SMALL", 1), ("N3_MAX_WG_SMALL", 2), ("N3_MAX_WG_LARGE", 1)}
