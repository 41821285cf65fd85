"""not-gpu: the launch plans of the dense convolution.  Every dense kernel case declares the route (kernel family, tile, template
variant, splits) its call must take; here the declared routes are held against the library's planner (uda_conv_route /
uda_conv_wgrad_route on the case's shape, in both MFMA modes), and the planner's whole repertoire (uda_conv_route_list)
against the cases, so that no kernel the library can choose goes without a case that runs it."""
import os

import pytest

from kernel_cases import CASES, WINDOW_CASES, _declared, plan_route

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="library not built (run __graft_entry__.build())")

_DENSE = [c for c in CASES if c[0].startswith(("conv", "dgrad", "wgrad"))]


def _entry(route):
    return " ".join(route.split()[:2])          # "<family> <tile>"


@pytest.fixture(scope="module")
def K():
    from uda_clr_amd.kernels import HipKernels
    return HipKernels()


def test_every_dense_case_records_its_shape_and_route():
    assert len(_DENSE) >= 119
    for name, fn in _DENSE:
        assert hasattr(fn, "plan_query") and fn.route, name


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_declared_routes_are_what_the_library_plans(K, mode):
    K.mfma = K.MFMA_BF16X3 if mode == "bf16x3" else K.MFMA_F32
    wrong = {}
    for name, fn in _DENSE:
        got = plan_route(K, fn.plan_query)
        if got != _declared(fn.route, K.mfma):
            wrong[name] = (got, _declared(fn.route, K.mfma))
    assert not wrong, wrong


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_declared_routes_of_the_window_cases_are_what_the_library_plans(K, mode):
    """the dense calls of the window cases (tests/test_footprint_gpu.py): column windows of wide matrices, ldy / ld_add far above Cout"""
    K.mfma = K.MFMA_BF16X3 if mode == "bf16x3" else K.MFMA_F32
    queries = [(name, q, route) for name, fn in WINDOW_CASES for q, route in getattr(fn, "plan_queries", [])]
    assert len(queries) == 12 and all(q["ldy"] > q["Cout"] + 200 for _, q, _ in queries)
    wrong = {(name, q["k"], q["dil"]): (plan_route(K, q), _declared(route, K.mfma)) for name, q, route in queries
             if plan_route(K, q) != _declared(route, K.mfma)}
    assert not wrong, wrong


def test_every_route_the_library_can_choose_is_declared_by_a_case(K):
    entries = K.lib.uda_conv_route_list().decode().split("\n")
    assert len(entries) == len(set(entries)) and all(len(e.split()) == 2 for e in entries), entries
    declared = {_entry(_declared(fn.route, m)) for _, fn in _DENSE for m in (0, 1)}
    unrun = [e for e in entries if e not in declared]
    assert not unrun, "no kernel case runs %s" % unrun
    assert not declared - set(entries), "declared by a case, missing from uda_conv_route_list: %s" % (declared - set(entries))


def test_refused_arguments_have_no_route(K):
    from kernel_cases import _query
    K.mfma = K.MFMA_F32
    assert plan_route(K, _query("conv", 2, 16, 16, 64, 32, 3, 1, stride=2)) == "none"          # stride 2 on a narrow tile
    assert plan_route(K, _query("wgrad", 2, 16, 16, 64, 32, 3, 1, stride=2)) == "none"
