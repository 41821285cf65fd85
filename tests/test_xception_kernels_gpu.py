"""-m gpu: the depthwise entry points at the Xception widths against fp64 torch.  Every case runs twice: with the kernel
family the library's launch plan chooses (C > 1024 and dilation 4 at 1024 channels on the channel-blocked kernels, narrower
widths on the tiled / flat ones) and pinned to the channel-blocked family, which may serve every width.  Each variant asserts
through dw_route which kernel serves its three calls.
Inputs are [P, C] views with ld > C whose padding columns hold NaN / Inf (kernel_cases.padded): nothing may leak."""
import pytest
import torch
import torch.nn.functional as F

from dw_shapes import SHAPES, declared
from kernel_cases import act_to, footprint, footprint_violations, gen, hip, make_src, out_dev, padded, ro_dev, to_dev
from uda_clr_amd.acts import ACT_NONE, ACT_RELU

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _footprint():
    """every test starts with an empty footprint registry and runs with guarded workspaces (kernel_cases.footprint)"""
    with footprint():
        yield


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    if not torch.isfinite(a).all():
        return float("inf")
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _nchw(rows, N, H, W):
    return rows.reshape(N, H, W, -1).permute(0, 3, 1, 2)


def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("family", ["", "cb"], ids=["routed", "channel-blocked"])
@pytest.mark.parametrize("N,H,W,C,stride,dil,lazy", SHAPES, ids=["n%d_%dx%d_c%d_s%d_d%d_%s" % (s[:6] + ("bn" if s[6] else "raw",))
                                                                 for s in SHAPES])
def test_depthwise_matches_fp64(family, N, H, W, C, stride, dil, lazy):
    g = gen(100 + C + 7 * dil + stride)
    src = make_src(N, H, W, C, g, lazy, ACT_RELU)
    w = torch.randn(C, 1, 3, 3, generator=g) / 3.0
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Po = N * Ho * Wo
    # fp64 statement: zero border AFTER the producer's BN + ReLU (xception.py:8-14,26-31)
    u = src.x.double()
    if lazy:
        u = torch.relu(u * src.scale.double() + src.shift.double())
    u = _nchw(u, N, H, W)
    wd = w.double()
    y = F.conv2d(F.pad(u, (dil,) * 4), wd, None, stride, 0, dil, C)
    dy = padded(Po, C, g)
    gy = _nchw(dy.double(), N, Ho, Wo)
    dx = torch.nn.grad.conv2d_input((N, C, H + 2 * dil, W + 2 * dil), wd, gy, stride, 0, dil, C)[:, :, dil:dil + H, dil:dil + W]
    dwr = torch.nn.grad.conv2d_weight(F.pad(u, (dil,) * 4), wd.shape, gy, stride, 0, dil, C)
    yr = _rows(y)

    K = hip()
    for op, want in zip(("fwd", "dgrad", "wgrad"), declared(family, (N, H, W, C, stride, dil, lazy))):
        route = K.dw_route(op, N, H, W, C, stride, dil, family)
        assert " ".join(route.split()[:2]) == want, route
    w9 = K.relayout_dw(w.to(DEV))
    sh = act_to(src, DEV)
    yh = to_dev(padded(Po, C, g), DEV)
    st = out_dev((16, 2, C), torch.float64, DEV, fill=0)
    K.dwconv_fwd(sh, w9, stride, dil, 0, yh, st, family=family)
    dxh = to_dev(padded(N * H * W, C, g), DEV)
    K.dwconv_dgrad(ro_dev(dy, DEV), w9, stride, dil, N, H, W, dxh, family=family)
    dwh = out_dev((C, 1, 3, 3), torch.float32, DEV)
    K.dwconv_wgrad(sh, ro_dev(dy, DEV), stride, dil, 0, dwh, family=family)
    torch.cuda.synchronize()
    errs = {"y": _rel(yh, yr), "sum": _rel(st.sum(0)[0], yr.sum(0)), "sumsq": _rel(st.sum(0)[1], (yr * yr).sum(0)),
            "dx": _rel(dxh, _rows(dx)), "dw": _rel(dwh, dwr)}
    # fp32 sums of 9 products (y, dx) and of up to 9 * 300 products (dw, statistics): measured <= 1e-6 relative
    assert max(errs.values()) < 2e-5, errs
    assert footprint_violations() == [], "a kernel wrote outside its outputs: (buffer, first position)"


def test_stride1_input_gradient_is_the_flipped_forward():
    """The engine computes a stride-1 depthwise input gradient as the forward conv of dy with the taps reversed (no
    prologue, zero border): on the channel-blocked kernels that equals their own input-gradient kernel."""
    N, H, W, C, dil = 2, 9, 11, 1536, 4
    g = gen(7)
    dy = padded(N * H * W, C, g)
    w = torch.randn(C, 1, 3, 3, generator=g)
    K = hip()
    w9 = K.relayout_dw(w.to(DEV))
    a = to_dev(padded(N * H * W, C, g), DEV)
    b = to_dev(padded(N * H * W, C, g), DEV)
    from uda_clr_amd.acts import Act
    K.dwconv_fwd(Act(ro_dev(dy, DEV), N, H, W), w9.flip(0).contiguous(), 1, dil, 0, a, None)
    K.dwconv_dgrad(ro_dev(dy, DEV), w9, 1, dil, N, H, W, b)
    torch.cuda.synchronize()
    assert _rel(a, b) < 1e-6
    assert footprint_violations() == [], "a kernel wrote outside its outputs: (buffer, first position)"


def test_routed_entries_reject_what_no_kernel_serves():
    K = hip()
    g = gen(3)
    src = act_to(make_src(1, 4, 4, 2052, g, False, ACT_NONE), DEV)
    w9 = torch.zeros(9, 2052, device=DEV)
    out = to_dev(padded(16, 2052, g), DEV)
    with pytest.raises(RuntimeError, match="2048"):
        K.dwconv_fwd(src, w9, 1, 1, 0, out)
    torch.cuda.synchronize()
    assert footprint_violations() == [], "a refused call wrote something: (buffer, first position)"
