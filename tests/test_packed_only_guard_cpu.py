"""not-gpu: a matrix that exists only as its packed bf16x3 operand (HipKernels._packed_only: the fp32 view is uninitialised) is
refused wherever it would be read as fp32 rows.  The checks are host code in front of every launch, so they run here on host
tensors, against the built library's own size function and with nothing launched:
  * conv() / conv_wgrad() in the fp32 matrix mode,
  * conv() / conv_wgrad() that would slice the operand into image groups (the slices lose the attached packed form),
  * _packed() after the attachment was removed (it would pack the uninitialised fp32 view)."""
import pytest
import torch

from uda_clr_amd.acts import Act
from uda_clr_amd.kernels import HipKernels

N, H, W, C = 4, 8, 8, 16


def _marked(K, rows=N * H * W, Cc=C):
    m, xs = K._packed_only(rows, Cc, "cpu")
    assert K._x3_only(m) and m._x3 is xs and tuple(m.shape) == (rows, Cc)
    return m


def test_f32_mode_refuses_a_packed_only_operand():
    K = HipKernels("f32")
    m = _marked(K)
    out = torch.empty(N * H * W, 32)
    with pytest.raises(RuntimeError, match="packed-only .* fp32 matrix mode"):
        K.conv(Act(m, N, H, W), torch.empty(32, 1, C), 1, 1, out)
    with pytest.raises(RuntimeError, match="packed-only .* fp32 matrix mode"):
        K.conv_wgrad(Act(torch.empty(N * H * W, 32), N, H, W), m, 1, 1, torch.empty(C, 32, 1, 1))
    with pytest.raises(RuntimeError, match="packed-only .* fp32 matrix mode"):
        K.conv_wgrad(Act(m, N, H, W), torch.empty(N * H * W, 32), 1, 1, torch.empty(32, C, 1, 1))


def test_image_groups_refuse_a_packed_only_operand():
    K = HipKernels("bf16x3")
    K.ELEM_LIMIT = 32 * (64 + 256)           # this instance: at most 64 rows of 32 floats per launch -> one image of 64 rows per group
    assert K._image_groups(N, H * W, 32, C) == [(0, 1), (1, 2), (2, 3), (3, 4)] and K._image_groups(N, H * W, 32) is not None
    m = _marked(K)
    with pytest.raises(RuntimeError, match="packed-only .* sliced into 4 image groups"):
        K.conv(Act(m, N, H, W), torch.empty(32, 1, C), 1, 1, torch.empty(N * H * W, 32))
    with pytest.raises(RuntimeError, match="packed-only .* sliced into"):
        K.conv_wgrad(Act(torch.empty(N * H * W, 32), N, H, W), m, 1, 1, torch.empty(C, 32, 1, 1))
    # an ordinary matrix takes the group path as before: the first slice reaches the device check of the first launch
    from uda_clr_amd.kernels import UdaError
    with pytest.raises(UdaError, match="device tensors"):
        K.conv(Act(torch.empty(N * H * W, C), N, H, W), torch.empty(32, 1, C), 1, 1, torch.empty(N * H * W, 32))


def test_packed_refuses_to_repack_the_fp32_view():
    K = HipKernels("bf16x3")
    m = _marked(K)
    a = Act(m, N, H, W)
    assert K._packed(a, None, "cpu") is m._x3           # attached: handed over, nothing packed
    stripped = _marked(K)
    del stripped._x3
    with pytest.raises(RuntimeError, match="packed-only .* lost its packed form"):
        K._packed(Act(stripped, N, H, W), None, "cpu")
    short = _marked(K)
    short._x3 = short._x3[:-16]
    with pytest.raises(RuntimeError, match="stale attachment"):
        K._packed(Act(short, N, H, W), None, "cpu")
