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


def _stride2_convs():
    """{(network, layer, Cin, Cout, dilation, input side)}: every 3x3 conv at stride 2 of the ResNet-101 and DRN-D-54 plans, with the
    side of its input for a 64 x 64 image"""
    from uda_clr_amd.networks.backbone.drn import drn_plan
    from uda_clr_amd.networks.backbone.resnet import resnet_plan
    found = set()

    def bottlenecks(net, blocks, side):
        for pre, inp, planes, stride, dil, has_ds in blocks:          # conv2 planes -> planes carries the block's stride
            if stride == 2:
                found.add((net, pre, planes, planes, dil, side))
            side = (side - 1) // stride + 1
        return side

    def conv_layers(net, rows, side):
        for ck, bk, ci, co, k, stride, dil in rows:
            if k == 3 and stride == 2:
                found.add((net, ck, ci, co, dil, side))
            side = (side - 1) // stride + 1
        return side

    for output_stride in (8, 16):
        bottlenecks("resnet", resnet_plan(output_stride), 16)         # behind conv1 and the max-pool: 1/4
    head, blocks, tail = drn_plan()
    conv_layers("drn", tail, bottlenecks("drn", blocks, conv_layers("drn", head, 64)))
    return found


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
def test_every_stride2_conv3x3_of_the_networks_has_a_kernel(K, mode):
    """The engines run a 3x3 conv on DRN's narrow direct kernels where its table says so and hand everything else to the library's
    planner, whatever the stride (networks/backbone/_bottleneck.py).  So every stride-2 3x3 conv of the plans is either in that
    table for the forward and the weight gradient, or planned by uda_conv_route and uda_conv_wgrad_route; geometry of a
    2 x 3 x 64 x 64 input."""
    from kernel_cases import _query
    from uda_clr_amd.networks.backbone.drn import _narrow
    K.mfma = K.MFMA_BF16X3 if mode == "bf16x3" else K.MFMA_F32
    convs = _stride2_convs()
    assert {c[:4] for c in convs} == {("drn", "layer2.0", 16, 32), ("drn", "layer3.0", 64, 64), ("drn", "layer4.0", 128, 128),
                                      ("resnet", "layer2.0", 128, 128), ("resnet", "layer3.0", 256, 256)}
    for net, layer, ci, co, dil, side in sorted(convs):
        narrow = [net == "drn" and _narrow(what, ci, co, 2, dil) for what in ("fwd", "wgrad")]
        planned = [plan_route(K, _query(kind, 2, side, side, ci, co, 3, dil, lazy=True, stats=kind == "conv", stride=2))
                   for kind in ("conv", "wgrad")]
        assert all(narrow) or "none" not in planned, (net, layer, narrow, planned)


def test_refused_arguments_have_no_route(K):
    from kernel_cases import _query
    K.mfma = K.MFMA_F32
    assert plan_route(K, _query("conv", 2, 16, 16, 64, 32, 3, 1, stride=2)) == "none"          # stride 2 on a narrow tile
    assert plan_route(K, _query("wgrad", 2, 16, 16, 64, 32, 3, 1, stride=2)) == "none"
