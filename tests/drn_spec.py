"""Plain-PyTorch fp32 statement of the DRN head kernels (TEST INFRASTRUCTURE): ``kernel_spec.SpecKernels`` plus the entries
of uda_clr_amd/csrc/drn_head.hip (``stem7s1_*``, ``conv3n_*``, ``relayout_hwio``), so that the engine's DRN orchestration runs
on CPU and the ``-m gpu`` kernel tests have their per-kernel statement."""
from __future__ import annotations

import torch
import torch.nn.functional as F

from kernel_spec import SpecKernels, _nchw, _rows, transform
from uda_clr_amd.acts import Act

NARROW = (16, 32, 64)          # channel counts the narrow 3x3 kernels are built for (either side)


class DrnSpecKernels(SpecKernels):
    @staticmethod
    def relayout_hwio(w, dgrad=False):
        """[O, I, kh, kw] -> [kh, kw, I, O]; dgrad: [kh, kw, O, I] with flipped taps."""
        if dgrad:
            return w.flip(2, 3).permute(2, 3, 0, 1).contiguous()
        return w.permute(2, 3, 1, 0).contiguous()

    @staticmethod
    def _add_stats(stats, y):
        if stats is not None:
            stats[0, 0] += y.double().sum(0)
            stats[0, 1] += (y.double() ** 2).sum(0)

    # ------------------------------------------------------------------ layer0: 7x7 stride 1 pad 3, 3 -> 16, NCHW in
    def stem7s1_fwd(self, x, w_hwio, out, stats=None):
        assert tuple(w_hwio.shape) == (7, 7, 3, 16)
        y = _rows(F.conv2d(x, w_hwio.permute(3, 2, 0, 1), None, 1, 3))
        self._add_stats(stats, y)
        out.copy_(y)

    def stem7s1_wgrad(self, x, dy, dw):
        N, _, H, W = x.shape
        dw.copy_(torch.nn.grad.conv2d_weight(x, dw.shape, _nchw(dy, N, H, W), 1, 3))

    # ------------------------------------------------------------------ narrow dense 3x3, pad 1, stride 1 | 2
    def conv3n_fwd(self, src: Act, w_hwio, stride, out, stats=None):
        """out[(n, oh, ow), co] = sum u(n, s*oh + kh - 1, s*ow + kw - 1, ci) * w_hwio[kh, kw, ci, co], u = 0 outside the image."""
        assert src.C in NARROW and out.shape[1] in NARROW and stride in (1, 2) and src.mask is None
        u = _nchw(transform(src), src.N, src.H, src.W)
        y = _rows(F.conv2d(u, w_hwio.permute(3, 2, 0, 1), None, stride, 1))
        self._add_stats(stats, y)
        out.copy_(y)

    def conv3n_wgrad(self, src: Act, dy, stride, dw):
        assert src.C in NARROW and dy.shape[1] in NARROW and stride in (1, 2) and src.mask is None
        u = _nchw(transform(src), src.N, src.H, src.W)
        g = _nchw(dy, src.N, (src.H - 1) // stride + 1, (src.W - 1) // stride + 1)
        dw.copy_(torch.nn.grad.conv2d_weight(u, dw.shape, g, stride, 1))
