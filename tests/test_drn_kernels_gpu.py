"""-m gpu: the DRN head kernels (uda_clr_amd/csrc/drn_head.hip) against fp64 torch on small odd shapes: the 7x7 stride-1 stem
(3 -> 16, NCHW in) and the narrow dense 3x3 family (16 / 32 / 64 channels on either side, stride 1 | 2) at the channel pairs
the model uses and at the family's extremes.  Inputs and outputs are [P, C] views with ld > C whose padding columns hold
NaN / Inf (kernel_cases.padded): nothing may leak.  The kernels are fp32 VALU code: UDA_CLR_MFMA does not reach them, so there
is one matrix mode to test."""
import pytest
import torch
import torch.nn.functional as F

from kernel_cases import act_to, footprint, footprint_violations, gen, hip, make_src, out_dev, padded, ro_dev, to_dev
from uda_clr_amd.acts import ACT_NONE, ACT_RELU, Act

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _footprint():
    """every test starts with an empty footprint registry and runs with guarded workspaces (kernel_cases.footprint)"""
    with footprint():
        yield

# fp32 sums of at most 9 * 64 products (y, dx) and of N * Ho * Wo <= 3,000 products (dw, statistics; fp32 within a workgroup's
# tile, fp64 across tiles): the bound test_xception_kernels_gpu.py uses for sums of this length
BOUND = 2e-5


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _nchw(rows, N, H, W):
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


# (N, H, W): one tile, several 16 x 64 tiles with ragged edges, three images
STEM_SHAPES = [(1, 9, 13), (1, 19, 71), (3, 21, 37), (1, 33, 80)]


@pytest.mark.parametrize("N,H,W", STEM_SHAPES, ids=["n%d_%dx%d" % s for s in STEM_SHAPES])
def test_stem7s1_matches_fp64(N, H, W):
    assert N * H * W <= 3000
    g = gen(40 + H)
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(16, 3, 7, 7, generator=g) / 7.0
    P = N * H * W
    y = F.conv2d(x.double(), w.double(), None, 1, 3)
    dy = padded(P, 16, g)
    dwr = torch.nn.grad.conv2d_weight(x.double(), w.shape, _nchw(dy.double(), N, H, W), 1, 3)
    yr = _rows(y)

    K = hip()
    yh = to_dev(padded(P, 16, g), DEV)
    st = out_dev((16, 2, 16), torch.float64, DEV, fill=0)
    K.stem7s1_fwd(ro_dev(x, DEV), ro_dev(K.relayout_hwio(w.to(DEV)), DEV), yh, st)
    yh2 = to_dev(padded(P, 16, g), DEV)
    K.stem7s1_fwd(ro_dev(x, DEV), ro_dev(K.relayout_hwio(w.to(DEV)), DEV), yh2, None)           # without the statistics epilogue
    dwh = out_dev((16, 3, 7, 7), torch.float32, DEV)
    K.stem7s1_wgrad(ro_dev(x, DEV), ro_dev(dy, DEV), dwh)
    torch.cuda.synchronize()
    errs = {"y": _rel(yh, yr), "y_nostats": _rel(yh2, yr), "sum": _rel(st.sum(0)[0], yr.sum(0)),
            "sumsq": _rel(st.sum(0)[1], (yr * yr).sum(0)), "dw": _rel(dwh, dwr)}
    print(errs)
    assert max(errs.values()) < BOUND, errs
    assert footprint_violations() == [], "a kernel wrote outside its outputs: (buffer, first position)"


# (N, H, W, Cin, Cout, stride, BN + ReLU prologue): the model's pairs (16 -> 16; 16 -> 32 stride 2; 64 -> 64 stride 2, and
# 32 -> 16 / 64 -> 64 at stride 1, the input-gradient forms), then the family's extremes; stride 2 on odd and even extents
CONV_SHAPES = [(1, 13, 37, 16, 16, 1, True), (3, 9, 35, 16, 16, 1, False),
               (1, 21, 67, 16, 32, 2, True), (3, 18, 40, 16, 32, 2, False), (1, 8, 6, 16, 32, 2, True),
               (1, 19, 69, 64, 64, 2, True), (3, 12, 34, 64, 64, 2, False),
               (1, 11, 35, 32, 16, 1, False), (1, 10, 33, 64, 64, 1, True),
               (1, 9, 34, 16, 64, 1, True), (3, 7, 11, 64, 16, 2, True), (1, 17, 36, 64, 16, 1, False),
               (1, 15, 33, 32, 32, 2, True), (1, 14, 66, 16, 64, 2, False), (3, 5, 9, 32, 64, 1, True)]


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,lazy", CONV_SHAPES,
                         ids=["n%d_%dx%d_%dto%d_s%d_%s" % (s[:6] + ("bn" if s[6] else "raw",)) for s in CONV_SHAPES])
def test_conv3n_matches_fp64(N, H, W, Cin, Cout, stride, lazy):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Po = N * Ho * Wo
    assert Po <= 3000
    g = gen(300 + Cin + 3 * Cout + stride + H)
    src = make_src(N, H, W, Cin, g, lazy, ACT_RELU)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (3.0 * Cin ** 0.5)
    # fp64 statement: zero border AFTER the producer's BN + ReLU
    u = src.x.double()
    if lazy:
        u = torch.relu(u * src.scale.double() + src.shift.double())
    u = _nchw(u, N, H, W)
    wd = w.double()
    y = F.conv2d(u, wd, None, stride, 1)
    dy = padded(Po, Cout, g)
    gy = _nchw(dy.double(), N, Ho, Wo)
    dx = torch.nn.grad.conv2d_input((N, Cin, H, W), wd, gy, stride, 1)
    dwr = torch.nn.grad.conv2d_weight(u, wd.shape, gy, stride, 1)
    yr = _rows(y)

    K = hip()
    sh = act_to(src, DEV)
    yh = to_dev(padded(Po, Cout, g), DEV)
    st = out_dev((16, 2, Cout), torch.float64, DEV, fill=0)
    K.conv3n_fwd(sh, ro_dev(K.relayout_hwio(w.to(DEV)), DEV), stride, yh, st)
    dwh = out_dev((Cout, Cin, 3, 3), torch.float32, DEV)
    K.conv3n_wgrad(sh, ro_dev(dy, DEV), stride, dwh)
    # input gradient the way the engine forms it: the stride-1 kernel on the (zero-stuffed) gradient with flipped, transposed weights
    dyf = ro_dev(dy, DEV)
    if stride != 1:
        dyf = to_dev(padded(N * H * W, Cout, g), DEV)
        K.rows_stride(ro_dev(dy, DEV), N, H, W, stride, dyf, scatter=True)
    dxh = to_dev(padded(N * H * W, Cin, g), DEV)
    K.conv3n_fwd(Act(dyf, N, H, W), K.relayout_hwio(w.to(DEV), True), 1, dxh, None)
    torch.cuda.synchronize()
    errs = {"y": _rel(yh, yr), "sum": _rel(st.sum(0)[0], yr.sum(0)), "sumsq": _rel(st.sum(0)[1], (yr * yr).sum(0)),
            "dx": _rel(dxh, _rows(dx)), "dw": _rel(dwh, dwr)}
    print(errs)
    assert max(errs.values()) < BOUND, errs
    assert footprint_violations() == [], "a kernel wrote outside its outputs: (buffer, first position)"


# ---- the weight gradients past their workgroup caps.  stem7s1_wgrad_kernel (8 x 64 tiles) and conv3n_wgrad_kernel (8 x 32 tiles at
# stride 1 below 64 output channels, else 4 x 32) launch min(tiles, cap) workgroups that walk their tiles with a stride of the grid
# and write ONE partial row of the workspace each; the shapes above have at most 4 tiles.  Here a workgroup takes a second tile and
# the last round is partly filled (tests/test_capped_cases_cpu.py holds that against H7W_MAX_WG / N3_MAX_WG_* of drn_head.hip).
# BOUND stays: a workgroup sums at most two tiles of 512 (stem, 8 x 32: 256; 4 x 32: 128) products in fp32, fewer than the 3,000
# the bound was worked out for; the partial rows are added in fp64.  Weight gradients only: the forward kernels launch one
# workgroup per tile.
STEM_CAPPED = [(2, 264, 520)]                                   # 2 * 33 * 9 = 594 tiles on 512 workgroups
CONV_CAPPED = [(3, 100, 100, 64, 64, 1, True),                  # 3 * 25 * 4 = 300 tiles of 4 x 32 on 256 workgroups
               (4, 200, 360, 16, 16, 1, False),                 # 4 * 25 * 12 = 1200 tiles of 8 x 32 on 1024
               (2, 263, 1001, 16, 32, 2, True)]                 # stride 2, 132 x 501 outputs: 2 * 33 * 16 = 1056 tiles of 4 x 32 on 1024


@pytest.mark.parametrize("N,H,W", STEM_CAPPED, ids=["n%d_%dx%d" % s for s in STEM_CAPPED])
def test_stem7s1_wgrad_past_its_workgroup_cap_matches_fp64(N, H, W):
    g = gen(40 + H)
    x = torch.randn(N, 3, H, W, generator=g)
    dy = padded(N * H * W, 16, g)
    dwr = torch.nn.grad.conv2d_weight(x.double(), (16, 3, 7, 7), _nchw(dy.double(), N, H, W), 1, 3)
    dwh = out_dev((16, 3, 7, 7), torch.float32, DEV)
    hip().stem7s1_wgrad(ro_dev(x, DEV), ro_dev(dy, DEV), dwh)
    torch.cuda.synchronize()
    err = _rel(dwh, dwr)
    print({"dw": err})
    assert err < BOUND
    assert footprint_violations() == [], "a kernel wrote outside its outputs: (buffer, first position)"


@pytest.mark.parametrize("N,H,W,Cin,Cout,stride,lazy", CONV_CAPPED,
                         ids=["n%d_%dx%d_%dto%d_s%d_%s" % (s[:6] + ("bn" if s[6] else "raw",)) for s in CONV_CAPPED])
def test_conv3n_wgrad_past_its_workgroup_cap_matches_fp64(N, H, W, Cin, Cout, stride, lazy):
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    g = gen(300 + Cin + 3 * Cout + stride + H)
    src = make_src(N, H, W, Cin, g, lazy, ACT_RELU)
    u = src.x.double()
    if lazy:
        u = torch.relu(u * src.scale.double() + src.shift.double())
    dy = padded(N * Ho * Wo, Cout, g)
    dwr = torch.nn.grad.conv2d_weight(_nchw(u, N, H, W), (Cout, Cin, 3, 3), _nchw(dy.double(), N, Ho, Wo), stride, 1)
    dwh = out_dev((Cout, Cin, 3, 3), torch.float32, DEV)
    hip().conv3n_wgrad(act_to(src, DEV), ro_dev(dy, DEV), stride, dwh)
    torch.cuda.synchronize()
    err = _rel(dwh, dwr)
    print({"dw": err})
    assert err < BOUND
    assert footprint_violations() == [], "a kernel wrote outside its outputs: (buffer, first position)"


def test_statistics_are_added_into():
    """the statistics epilogue ADDS into its fp64 accumulator (several launches of one BatchNorm share it)"""
    N, H, W = 1, 9, 40
    g = gen(5)
    src = act_to(make_src(N, H, W, 16, g, True, ACT_RELU), DEV)
    K = hip()
    w = K.relayout_hwio(torch.randn(16, 16, 3, 3, generator=g).to(DEV))
    y = to_dev(padded(N * H * W, 16, g), DEV)
    st = out_dev((16, 2, 16), torch.float64, DEV, fill=0)
    K.conv3n_fwd(src, w, 1, y, st)
    once = st.sum(0).clone()
    K.conv3n_fwd(src, w, 1, y, st)
    torch.cuda.synchronize()
    assert _rel(st.sum(0), 2 * once) < 1e-12
    assert footprint_violations() == [], "a kernel wrote outside its outputs: (buffer, first position)"


def test_entries_reject_what_no_kernel_serves():
    """a width outside 16 / 32 / 64, a dropout mask on the operand: an error naming the limit, not a launch"""
    K = hip()
    g = gen(3)
    src = act_to(make_src(1, 4, 4, 24, g, False, ACT_NONE), DEV)
    out = to_dev(padded(16, 16, g), DEV)
    with pytest.raises(RuntimeError, match="16, 32 or 64"):
        K.conv3n_fwd(src, torch.zeros(3, 3, 24, 16, device=DEV), 1, out)
    src = act_to(make_src(1, 4, 4, 16, g, False, ACT_NONE), DEV)
    out = to_dev(padded(16, 128, g), DEV)
    with pytest.raises(RuntimeError, match="16, 32 or 64"):
        K.conv3n_fwd(src, torch.zeros(3, 3, 16, 128, device=DEV), 1, out)
    with pytest.raises(RuntimeError, match="16, 32 or 64"):
        K.conv3n_wgrad(src, to_dev(padded(16, 128, g), DEV), 1, out_dev((128, 16, 3, 3), torch.float32, DEV))
    masked = act_to(make_src(1, 4, 4, 16, g, True, ACT_RELU, mask=True), DEV)
    with pytest.raises(RuntimeError, match="mask"):
        K.conv3n_fwd(masked, torch.zeros(3, 3, 16, 16, device=DEV), 1, to_dev(padded(16, 16, g), DEV))
    # the implicit-GEMM entry keeps refusing a narrow stride-2 conv (the engine routes those to the narrow family)
    w = K.relayout_ohwi(torch.zeros(32, 16, 3, 3, device=DEV))
    with pytest.raises(RuntimeError, match="stride 2"):
        K.conv(src, w, 3, 1, to_dev(padded(4, 32, g), DEV), stride=2)
    torch.cuda.synchronize()
    assert footprint_violations() == [], "a refused call wrote something: (buffer, first position)"
