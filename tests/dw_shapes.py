"""The depthwise shapes of tests/test_xception_kernels_gpu.py and the kernel each must be served by: shared by that GPU test, which
asserts the routes before its calls, and by tests/test_dw_plan_cpu.py, which holds them against the planner without a GPU."""

# (N, H, W, C, stride, dilation, BN + ReLU prologue)
SHAPES = [(3, 9, 13, 4, 1, 1, True), (1, 7, 5, 64, 2, 1, True), (3, 6, 10, 64, 1, 4, False),
          (1, 12, 9, 728, 1, 1, True), (3, 11, 8, 728, 2, 1, True), (1, 10, 14, 728, 1, 2, False),
          (1, 9, 9, 1024, 1, 2, True), (3, 8, 11, 1024, 1, 4, True), (1, 5, 12, 1024, 2, 1, False),
          (1, 13, 10, 1536, 1, 2, True), (3, 7, 9, 1536, 1, 4, True), (1, 8, 6, 1536, 2, 1, False),
          (1, 9, 12, 2048, 1, 4, True), (3, 5, 7, 2048, 1, 1, False), (1, 6, 6, 2048, 2, 2, True)]

# the kernel the launch plan must choose for each of SHAPES: (forward and weight gradient, input gradient).  Channel-blocked above
# 1024 channels and at 1024 with dilation 4; else the input gradient is flat, the others tiled (8x16 at stride 1, 8x8 at stride 2)
# up to dilation 2 and flat beyond.
ROUTED = [("tiled-8x16", "flat"), ("tiled-8x8", "flat"), ("flat", "flat"),
          ("tiled-8x16", "flat"), ("tiled-8x8", "flat"), ("tiled-8x16", "flat"),
          ("tiled-8x16", "flat"), ("cb", "cb"), ("tiled-8x8", "flat"),
          ("cb", "cb"), ("cb", "cb"), ("cb", "cb"),
          ("cb", "cb"), ("cb", "cb"), ("cb", "cb")]


def declared(family, shape):
    """the "<op> <kernel>" of the forward, input-gradient and weight-gradient call on `shape`, routed ("") or pinned ("cb")"""
    fw, dg = ("cb", "cb") if family == "cb" else ROUTED[SHAPES.index(tuple(shape))]
    return "fwd " + fw, "dgrad " + dg, "wgrad " + fw
