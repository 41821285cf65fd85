"""ctypes bindings of libuda_clr_hip.so (include/uda_clr_hip.h) at the torch-tensor level.

PyTorch is only the owner of device memory and of the current HIP stream here: every method
checks layouts on the host, passes raw pointers + sizes through the C ABI and launches on
``torch.cuda.current_stream()``.  There is no fallback: a missing library or a non-GPU tensor
raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional

import torch

from .abi import CONSTANTS, STRUCTS, SYMBOLS
from .acts import conv_weight_shape, Act, round4

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libuda_clr_hip.so")
_lib = None

# constants, argument blocks and every symbol (name -> (restype, argtypes)) as include/uda_clr_hip.h declares them
STAT_SLOTS = CONSTANTS["UDA_STAT_SLOTS"]
FDA_MAX_BAND = CONSTANTS["UDA_FDA_MAX_BAND"]
UdaSrc, UdaConvArgs, UdaWgradArgs = STRUCTS["uda_src_t"], STRUCTS["uda_conv_args_t"], STRUCTS["uda_wgrad_args_t"]


def load_library(path: Optional[str] = None):
    """dlopen the C-ABI library and bind every declared symbol (raises if one is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or _LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError("libuda_clr_hip.so not found at %s - build it with "
                           "`python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % path)
    lib = C.CDLL(path)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError -> symbol missing
        fn.restype, fn.argtypes = res, args
    if lib.uda_version() < 3:            # version 1 has no `family` argument in uda_dwconv_*: it would read the stream there;
        #                                  version 2 refuses uda_upconv_fwd with stats where the kernel does not accumulate them
        raise RuntimeError("%s is ABI version %d, these bindings need 3 - rebuild it" % (path, lib.uda_version()))
    _lib = lib
    return lib


class UdaError(RuntimeError):
    pass


_DW_FAMILY = {"": CONSTANTS["UDA_DW_AUTO"], **{f: CONSTANTS["UDA_DW_" + f.upper()] for f in ("flat", "tiled", "cb")}}
_DW_OP = {op: CONSTANTS["UDA_DW_" + op.upper()] for op in ("fwd", "dgrad", "wgrad")}
_UP_OP = {"fwd": 0, "bwd": 1}                              # uda_upconv_route's op


def _family(family: str) -> int:
    """Depthwise kernel family of a binding call: "" (the library's launch plan chooses by shape) or "flat" / "tiled" / "cb"
    (that family, or an error where it cannot serve the shape)."""
    if family not in _DW_FAMILY:
        raise ValueError("depthwise kernel family %r" % (family,))
    return _DW_FAMILY[family]


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _mat(t: torch.Tensor, name="tensor"):
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError("%s must be a [P, C] row-major view" % name)
    return t.data_ptr(), t.stride(0)


def check_side(what, *sides):
    """every side a multiple of 16 in 16..1024: the sizes the generator and the resampling kernels take"""
    if any(n % 16 or not 16 <= n <= 1024 for n in sides):
        raise ValueError("%s %s: each side must be a multiple of 16 in 16..1024" % (what, " x ".join("%d" % n for n in sides)))


# ---------------------------------------------------------------------- packed tables of the evaluation kernels
# A kernel that fills several small tables gets them as views of ONE buffer of 8-byte words, so that one copy brings all of them to the
# host.  A layout is the ordered list of (name, dtype, shape) of those views; ``packed_views`` carves the device buffer for the binding
# and ``unpack_host`` carves its host copy for ``ops``, both from the same list.
_I64, _F64 = torch.int64, torch.float64


def surface_layout(B):
    return [("table", _F64, (B, 2, 2, 3)), ("counts", _I64, (B, 2, 3))]


def profile_layout(B, Q, T):
    return surface_layout(B) + [("order", _I64, (B, 2, 3, Q, 2)), ("within", _I64, (B, 2, 2, T)), ("extent", _I64, (B, 2, 2, 2))]


def morphometry_layout(B, K):
    return [("moments", _I64, (B, 2, 6)), ("extent", _I64, (B, 2, 4)), ("overlap", _I64, (B,)), ("radial", _I64, (B, 2, K))]


def selective_layout(B, M, K, prob=True, unc=True):
    """``rel`` only with probabilities, ``risk`` only with uncertainties"""
    return [("rel", _I64, (B, 2, M, 5))] * bool(prob) + [("risk", _I64, (B, 2, K, 4))] * bool(unc) + [("invalid", _I64, (B, 2, 2))]


def packed_views(layout, device):
    """-> (int64 buffer on ``device``, {name: its view of the layout's dtype and shape})"""
    sizes = [math.prod(shape) for _, _, shape in layout]
    packed = torch.empty(sum(sizes), dtype=_I64, device=device)
    return packed, {name: part.view(dtype).view(shape) for (name, dtype, shape), part in zip(layout, torch.split(packed, sizes))}


def unpack_host(layout, host):
    """the host copy of a packed buffer (numpy int64) -> {name: numpy view}"""
    import numpy as np
    parts = np.split(host, np.cumsum([math.prod(shape) for _, _, shape in layout])[:-1])
    return {name: part.view(str(dtype).split(".")[1]).reshape(shape) for (name, dtype, shape), part in zip(layout, parts)}


class HipKernels:
    name = "hip"

    MFMA_F32, MFMA_BF16X3 = CONSTANTS["UDA_MFMA_F32"], CONSTANTS["UDA_MFMA_BF16X3"]

    def __init__(self, mfma=None):
        self.lib = load_library()
        # matrix instructions of the wide (MFMA-bound) conv tiles (UDA_CLR_MFMA, include/uda_clr_hip.h UDA_MFMA_*):
        #   "bf16x3" (default) = fp32 emulated on the bf16 pipe by exact 3-way operand splitting - fp32-level results (per-call
        #             error against float64 equal to the fp32 kernel's, tests/bench_x3.py), 1.5-1.7x the fp32-MFMA kernel's rate;
        #   "f32"    = v_mfma_f32_32x32x2_f32, the exact fp32 fma chain.
        mode = (mfma or os.environ.get("UDA_CLR_MFMA", "bf16x3")).lower()
        if mode not in ("f32", "bf16x3"):
            raise ValueError("UDA_CLR_MFMA must be 'f32' or 'bf16x3', got %r" % mode)
        self.mfma = self.MFMA_BF16X3 if mode == "bf16x3" else self.MFMA_F32

    # ------------------------------------------------------------------ plumbing
    @staticmethod
    def _stream():
        return torch.cuda.current_stream().cuda_stream

    def _ck(self, rc):
        if rc != 0:
            raise UdaError(self.lib.uda_last_error().decode())

    @staticmethod
    def _dev(t):
        if not t.is_cuda:
            raise UdaError("HIP kernels need device tensors (got %s); there is no CPU fallback" % t.device)
        if t.dtype not in (torch.float32, torch.float64, torch.uint8):
            raise UdaError("unsupported dtype %s" % t.dtype)

    def _src(self, a: Act) -> UdaSrc:
        a.check()
        self._dev(a.x)
        s = UdaSrc()
        s.x, s.ldx = a.x.data_ptr(), a.x.stride(0)
        s.N, s.H, s.W, s.C = a.N, a.H, a.W, a.C
        s.scale, s.shift = _ptr(a.scale), _ptr(a.shift)
        if a.scale is not None:
            assert a.scale.is_contiguous() and a.shift.is_contiguous() and a.scale.numel() == a.C
        s.act = a.act
        if a.mask is not None:
            s.mask, s.ldm = a.mask.data_ptr(), a.mask.stride(0)
        else:
            s.mask, s.ldm = None, 0
        s.mask_scale = a.mask_scale
        return s

    @staticmethod
    def _ck_stats(stats, Cc):
        """a statistics accumulator of Cc channels: double [STAT_SLOTS][2][Cc], or None"""
        if stats is not None:
            assert stats.dtype == torch.float64 and stats.is_contiguous() and tuple(stats.shape) == (STAT_SLOTS, 2, Cc)

    @staticmethod
    def _ws(like, nbytes):
        return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)

    def _ck_masks(self, who, *masks):
        """contiguous uint8 [B,2,H,W] device masks, all of one shape -> (B, H, W)"""
        for t in masks:
            self._dev(t)
            if t.dtype != torch.uint8 or not t.is_contiguous() or t.dim() != 4 or t.shape[1] != 2:
                raise ValueError("%s: contiguous uint8 [B, 2, H, W] masks (got %s %s)" % (who, t.dtype, tuple(t.shape)))
            if t.shape != masks[0].shape:
                raise ValueError("%s: shapes differ: %s and %s" % (who, tuple(masks[0].shape), tuple(t.shape)))
        B, _, H, W = masks[0].shape
        return B, H, W

    @staticmethod
    def _named_maps(who, outputs, u8_scale, shape, device):
        """the maps of ``mc_uncertainty`` / ``tta_fuse``: {name: f32 tensor of ``shape``} for the names in ``outputs``, with ``u8_scale``
        also the uint8 'std_u8'; ``.get(name)`` is None for a map that was not asked for"""
        names = ("mean", "std", "entropy", "mi")
        outputs = tuple(outputs)
        if any(o not in names for o in outputs) or not (outputs or u8_scale is not None):
            raise ValueError("%s: outputs among %r (got %r)" % (who, names, outputs))
        out = {o: torch.empty(shape, dtype=torch.float32, device=device) for o in names if o in outputs}
        if u8_scale is not None:
            out["std_u8"] = torch.empty(shape, dtype=torch.uint8, device=device)
        return out

    @staticmethod
    def _u8_f32(outputs, B, S, device):
        """the outputs of ``photo_reduce`` / ``roi_cut``: {'u8': uint8 [B,S,S,3], 'f32': f32 [B,3,S,S]} for the names in ``outputs``"""
        if not outputs or set(outputs) - {"u8", "f32"}:
            raise ValueError("outputs: 'u8', 'f32' or both, got %r" % (outputs,))
        out = {}
        if "u8" in outputs:
            out["u8"] = torch.empty(B, S, S, 3, dtype=torch.uint8, device=device)
        if "f32" in outputs:
            out["f32"] = torch.empty(B, 3, S, S, dtype=torch.float32, device=device)
        return out

    def _propagate(self, name, n_flags, x, thresholds, sweeps):
        """The entry ``name`` (uda_postprocess, uda_display_masks) on f32 [B,2,H,W] ``x`` -> uint8 [B,2,H,W].  Runs the tile-wise
        propagations for ``sweeps`` launches and repeats with twice as many, up to six attempts, while the device reports unfinished
        tiles in one of its ``n_flags`` flags; then raises."""
        B, _, H, W = x.shape
        out = torch.empty(B, 2, H, W, dtype=torch.uint8, device=x.device)
        flags = torch.zeros(n_flags, dtype=torch.int32, device=x.device)
        ws = self._ws(x, getattr(self.lib, name + "_workspace_bytes")(B, H, W))
        n = int(sweeps) if sweeps else 2 * ((H + 31) // 32 + (W + 31) // 32) + 4
        for _ in range(6):
            self._ck(getattr(self.lib, name)(x.data_ptr(), B, H, W, *thresholds, n, out.data_ptr(), flags.data_ptr(), ws.data_ptr(),
                                             ws.numel(), self._stream()))
            if int(flags.sum()) == 0:            # host sync: evaluation path only
                return out
            n *= 2
        raise UdaError("%s: label propagation did not converge after %d sweeps" % (name, n // 2))   # the last attempt's

    # ------------------------------------------------------------------ weight layouts
    def relayout_ohwi(self, w):
        O, I, k, _ = w.shape
        out = torch.empty(conv_weight_shape(O, k, I), dtype=torch.float32, device=w.device)
        self._ck(self.lib.uda_relayout_ohwi(w.contiguous().data_ptr(), O, I, k, out.data_ptr(), self._stream()))
        return out

    def relayout_dgrad(self, w):
        O, I, k, _ = w.shape
        out = torch.empty(conv_weight_shape(I, k, O), dtype=torch.float32, device=w.device)
        self._ck(self.lib.uda_relayout_dgrad(w.contiguous().data_ptr(), O, I, k, out.data_ptr(), self._stream()))
        return out

    def relayout_dw(self, w):
        Cc = w.shape[0]
        out = torch.empty(9, Cc, dtype=torch.float32, device=w.device)
        self._ck(self.lib.uda_relayout_dw(w.contiguous().data_ptr(), Cc, out.data_ptr(), self._stream()))
        return out

    # ------------------------------------------------------------------ dense conv
    # The conv / weight-gradient kernels address their operands with 32-bit offsets: rows * row stride of one operand must stay
    # below 2^29 elements (fp32) resp. 2^27 sixteen-byte units of the packed bf16x3 operand.  Larger batches are run as groups
    # of whole images (a convolution never crosses an image; statistics are ADDED into, weight gradients summed).
    ELEM_LIMIT = 1 << 29

    def _image_groups(self, N, rows_per_image, widest_ld, x3_channels=0):
        """None when one launch can take the whole operand, else [(n0, n1)] image ranges that can."""
        lim_rows = self.ELEM_LIMIT // max(int(widest_ld), 1) - 256
        if x3_channels:
            lim_rows = min(lim_rows, (self.ELEM_LIMIT // 4) // (((x3_channels + 15) // 16) * 6) - 256)
        if N * rows_per_image <= lim_rows:
            return None
        g = lim_rows // rows_per_image
        if g < 1:
            raise UdaError("one image (%d pixels x %d floats per row) exceeds the 32-bit offsets of the conv kernels" % (rows_per_image, widest_ld))
        return [(n0, min(N, n0 + g)) for n0 in range(0, N, g)]

    @staticmethod
    def _act_rows(a: Act, n0, n1):
        ppi = a.P // a.N
        r = slice(n0 * ppi, n1 * ppi)
        return Act(a.x[r], n1 - n0, a.H, a.W, a.scale, a.shift, a.act, None if a.mask is None else a.mask[r], a.mask_scale, a.bn, a.meta)

    @staticmethod
    def _x3_only(t):
        """True for a matrix that exists only as its packed bf16x3 operand (``_packed_only``): its fp32 values are uninitialised"""
        return getattr(t, "_x3_only", False)

    def _refuse_x3_only(self, who, why, *operands):
        """A packed-only operand can be read by the bf16x3 kernels alone, whole: anything else would read its uninitialised fp32
        view (a slice of it, ``_act_rows``, also loses the attached packed form)."""
        for t in operands:
            if self._x3_only(t):
                raise RuntimeError("%s: a packed-only [%d, %d] operand %s; its fp32 values were never written"
                                   % (who, t.shape[0], t.shape[1], why))

    def conv(self, src: Act, w, ksize, dil, out, bias=None, addend=None, stats=None, origin=0, stride=1):
        """stride 2 (wide tiles only: the C side raises otherwise): ``out`` / ``addend`` / ``stats`` live on the strided grid"""
        if self.mfma == self.MFMA_F32:
            self._refuse_x3_only("conv", "reaches the fp32 matrix mode", src.x)
        groups = self._image_groups(src.N, src.P // src.N, max(src.x.stride(0), out.stride(0), 0 if addend is None else addend.stride(0),
                                                               0 if src.mask is None else src.mask.stride(0) // 4),
                                    src.C if self.mfma != self.MFMA_F32 else 0)
        Po = src.N * ((src.H - 1) // stride + 1) * ((src.W - 1) // stride + 1)
        if groups is not None:
            self._refuse_x3_only("conv", "would be sliced into %d image groups" % len(groups), src.x)
            ppo = Po // src.N
            for n0, n1 in groups:
                r = slice(n0 * ppo, n1 * ppo)
                self.conv(self._act_rows(src, n0, n1), w, ksize, dil, out[r], bias, None if addend is None else addend[r], stats, origin, stride)
            return
        a = self._conv_args_of(src, w, ksize, dil, out, bias, addend, stats, origin, stride)
        if self.mfma != self.MFMA_F32 and self.lib.uda_conv_uses_x3(C.byref(a)):
            # bf16x3: both operands as their three bf16 pieces.  The packed forms are kept on the descriptor / the relayouted
            # weight, so an activation read by several convolutions (the ASPP input) and a weight used by several passes of one
            # step are split once.
            xs = self._packed(src, a.src, out.device)
            xw = getattr(w, "_x3", None)
            if xw is None:
                xw = self.x3_pack_rows(w)
                w._x3 = xw
            a.x3_src, a.x3_w = xs.data_ptr(), xw.data_ptr()
            nws = int(self.lib.uda_conv_fwd_workspace_bytes(C.byref(a)))
            if nws:         # fp32 partial tiles of the K-split last round of tiles
                ws = self._ws(out, nws)
                a.workspace, a.workspace_bytes = ws.data_ptr(), nws
            return self._conv_x3(a)
        self._refuse_x3_only("conv", "reaches a route that reads fp32 rows", src.x)
        self._ck(self.lib.uda_conv_fwd(C.byref(a), self._stream()))

    def conv_args(self, usrc: UdaSrc, Cout, ksize, dil=1, origin=0, stride=1, w=None, bias=None, addend=None, ld_add=0, y=None, ldy=0,
                  stats=None) -> UdaConvArgs:
        """The argument block of uda_conv_fwd from raw addresses (None: absent).  The only place that fills one."""
        a = UdaConvArgs()
        a.src, a.origin = usrc, origin
        a.w, a.Cout, a.ksize, a.dil, a.stride = w, Cout, ksize, dil, stride
        a.bias, a.addend, a.ld_add = bias, addend, ld_add
        a.y, a.ldy, a.stats = y, ldy, stats
        a.mfma = self.mfma
        return a

    def _conv_args_of(self, src: Act, w, ksize, dil, out, bias, addend, stats, origin, stride) -> UdaConvArgs:
        Cout = out.shape[1]
        assert w.is_contiguous() and tuple(w.shape) == conv_weight_shape(Cout, ksize, src.C), \
            "weight layout %s does not match conv %dx%d %d->%d" % (tuple(w.shape), ksize, ksize, src.C, Cout)
        assert out.shape[0] == src.N * ((src.H - 1) // stride + 1) * ((src.W - 1) // stride + 1) and stride in (1, 2)
        if bias is not None:
            assert bias.is_contiguous() and bias.numel() == Cout
        if addend is not None:
            assert addend.shape == out.shape
        self._ck_stats(stats, Cout)
        return self.conv_args(self._src(src), Cout, ksize, dil, origin, stride, w.data_ptr(), _ptr(bias),
                              *((None, 0) if addend is None else _mat(addend, "addend")), *_mat(out, "out"), _ptr(stats))

    def route(self, a) -> str:
        """The launch the library plans for an argument block of ``conv`` / ``conv_wgrad`` (uda_conv_route, uda_conv_wgrad_route);
        a conv that can split its last round of tiles is described with the workspace ``conv`` would bring."""
        buf = C.create_string_buffer(96)
        if isinstance(a, UdaWgradArgs):
            self.lib.uda_conv_wgrad_route(C.byref(a), buf, len(buf))
        else:
            nws = int(self.lib.uda_conv_fwd_workspace_bytes(C.byref(a)))
            if nws and not a.workspace:
                a.workspace, a.workspace_bytes = 16, nws      # the plan tests the address, it reads nothing
            self.lib.uda_conv_route(C.byref(a), buf, len(buf))
        return buf.value.decode()

    def conv_route(self, src: Act, w, ksize, dil, out, bias=None, addend=None, stats=None, origin=0, stride=1) -> str:
        """``route`` of the ``conv`` call with these arguments (as one launch)"""
        return self.route(self._conv_args_of(src, w, ksize, dil, out, bias, addend, stats, origin, stride))

    def _conv_x3(self, a):
        """the bf16x3 GEMM launch alone (bench.py times this)"""
        self._ck(self.lib.uda_conv_fwd(C.byref(a), self._stream()))

    def x3_pack(self, usrc: UdaSrc, rows, K, device, out=None):
        """``out``: a caller's uint8 buffer of uda_x3_packed_bytes(rows, K) bytes (the kernel tests hand in a guarded one)"""
        nbytes = int(self.lib.uda_x3_packed_bytes(rows, K))
        if out is None:
            out = torch.empty(nbytes, dtype=torch.uint8, device=device)
        assert out.dtype == torch.uint8 and out.is_contiguous() and out.numel() == nbytes and out.data_ptr() % 16 == 0
        self._ck(self.lib.uda_x3_pack(C.byref(usrc), out.data_ptr(), self._stream()))
        return out

    def _packed(self, src: Act, usrc: UdaSrc, device):
        """The packed form of a conv operand, split once per step: it rides on the descriptor (a pending transform belongs to the
        descriptor) and, for a raw operand (a gradient matrix, a discriminator's space-to-depth image), on the tensor object, so
        the forward conv, the input-gradient conv and the weight gradient that read the same matrix share one packing pass.
        The engines never write into a matrix after it has been read as a conv operand (gradients are complete before the
        producer's backward reads them)."""
        xs = getattr(src, "_x3", None)
        raw = not src.lazy
        if xs is None and raw:
            xs = getattr(src.x, "_x3", None)
        if xs is not None and xs.numel() != int(self.lib.uda_x3_packed_bytes(src.P, src.C)):
            raise RuntimeError("bf16x3 packed operand of %d bytes attached to a [%d, %d] matrix (expected %d): stale attachment"
                               % (xs.numel(), src.P, src.C, int(self.lib.uda_x3_packed_bytes(src.P, src.C))))
        if xs is None:
            self._refuse_x3_only("bf16x3 packing", "has lost its packed form and would be re-packed from its fp32 view", src.x)
            xs = self.x3_pack(usrc, src.P, src.C, device)
            if raw:
                try:
                    src.x._x3 = xs
                except AttributeError:
                    pass
        src._x3 = xs
        return xs

    def x3_pack_rows(self, w, out=None):
        """a relayouted weight [rows, taps, K'] (contiguous rows) as packed rows"""
        rows, klen = w.shape[0], w.numel() // w.shape[0]
        s = UdaSrc()
        s.x, s.ldx, s.N, s.H, s.W, s.C = w.data_ptr(), klen, 1, 1, rows, klen
        s.scale = s.shift = s.mask = None
        s.act, s.ldm, s.mask_scale = 0, 0, 1.0
        return self.x3_pack(s, rows, klen, w.device, out)

    def conv_wgrad(self, src: Act, dy, ksize, dil, dw, origin=0, stride=1):
        """stride 2 (wide tiles only): ``dy`` lives on the strided output grid of the forward conv"""
        if self.mfma == self.MFMA_F32:
            self._refuse_x3_only("conv_wgrad", "reaches the fp32 matrix mode", src.x, dy)
        groups = self._image_groups(src.N, src.P // src.N, max(src.x.stride(0), dy.stride(0), 0 if src.mask is None else src.mask.stride(0) // 4))
        Ho, Wo = (src.H - 1) // stride + 1, (src.W - 1) // stride + 1
        Po = src.N * Ho * Wo
        if groups is not None:
            self._refuse_x3_only("conv_wgrad", "would be sliced into %d image groups" % len(groups), src.x, dy)
            ppo = Po // src.N
            tmp = torch.empty_like(dw)
            for i, (n0, n1) in enumerate(groups):
                self.conv_wgrad(self._act_rows(src, n0, n1), dy[n0 * ppo:n1 * ppo], ksize, dil, dw if i == 0 else tmp, origin, stride)
                if i:
                    dw.add_(tmp)
            return
        a = self._wgrad_args_of(src, dy, ksize, dil, dw, origin, stride)
        ws = self._ws(dy, self.lib.uda_conv_wgrad_workspace_bytes(Po, a.Cout, src.C, ksize))
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        if self.mfma != self.MFMA_F32 and self.lib.uda_conv_wgrad_uses_x3(C.byref(a)):
            # bf16x3: the source's packed form usually exists already (the forward conv packed the same descriptor); dy is packed
            # once for its input-gradient conv and this weight gradient (the packed form rides on the tensor object)
            xs = self._packed(src, a.src, dy.device)
            dsrc = Act(dy, src.N, Ho, Wo)
            xd = self._packed(dsrc, self._src(dsrc), dy.device)
            a.x3_src, a.x3_dy = xs.data_ptr(), xd.data_ptr()
        else:
            self._refuse_x3_only("conv_wgrad", "reaches a route that reads fp32 rows", src.x, dy)
        self._ck(self.lib.uda_conv_wgrad(C.byref(a), self._stream()))

    def wgrad_args(self, usrc: UdaSrc, Cout, ksize, dil=1, origin=0, stride=1, dy=None, lddy=0, dw=None) -> UdaWgradArgs:
        """The argument block of uda_conv_wgrad from raw addresses, without workspace and packed operands.  The only place that fills one."""
        a = UdaWgradArgs()
        a.src, a.origin = usrc, origin
        a.dy, a.lddy, a.dw = dy, lddy, dw
        a.Cout, a.ksize, a.dil, a.stride = Cout, ksize, dil, stride
        a.mfma = self.mfma
        return a

    def _wgrad_args_of(self, src: Act, dy, ksize, dil, dw, origin, stride) -> UdaWgradArgs:
        Cout = dy.shape[1]
        assert dy.shape[0] == src.N * ((src.H - 1) // stride + 1) * ((src.W - 1) // stride + 1) and stride in (1, 2)
        assert dw.is_contiguous() and tuple(dw.shape) == (Cout, src.C, ksize, ksize)
        return self.wgrad_args(self._src(src), Cout, ksize, dil, origin, stride, *_mat(dy, "dy"), dw.data_ptr())

    def wgrad_route(self, src: Act, dy, ksize, dil, dw, origin=0, stride=1) -> str:
        """``route`` of the ``conv_wgrad`` call with these arguments (as one launch)"""
        return self.route(self._wgrad_args_of(src, dy, ksize, dil, dw, origin, stride))

    # ------------------------------------------------------------------ depthwise
    def dwconv_fwd(self, src: Act, w9c, stride, dil, border_mode, out, stats=None, family=""):
        """``family``: "" lets the library's launch plan choose by shape (the engine always does), "flat" / "tiled" / "cb" pin a
        kernel family (kernel tests and measurements); ``dw_route`` tells which kernel a call takes."""
        s = self._src(src)
        Ho, Wo = (src.H - 1) // stride + 1, (src.W - 1) // stride + 1
        assert out.shape == (src.N * Ho * Wo, src.C) and w9c.is_contiguous() and tuple(w9c.shape) == (9, src.C)
        y, ldy = _mat(out, "out")
        self._ck_stats(stats, src.C)
        self._ck(self.lib.uda_dwconv_fwd(C.byref(s), w9c.data_ptr(), stride, dil, border_mode, y, ldy, _ptr(stats), _family(family),
                                         self._stream()))

    def dwconv_dgrad(self, dy, w9c, stride, dil, N, H, W, out, family=""):
        Cc = dy.shape[1]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        assert dy.shape[0] == N * Ho * Wo and out.shape == (N * H * W, Cc)
        g, ldg = _mat(dy, "dy")
        o, ldo = _mat(out, "out")
        self._ck(self.lib.uda_dwconv_dgrad(g, ldg, w9c.data_ptr(), Cc, stride, dil, N, H, W, o, ldo, _family(family), self._stream()))

    def dwconv_wgrad(self, src: Act, dy, stride, dil, border_mode, dw, family=""):
        s = self._src(src)
        Ho, Wo = (src.H - 1) // stride + 1, (src.W - 1) // stride + 1
        assert dy.shape == (src.N * Ho * Wo, src.C) and dw.is_contiguous() and dw.numel() == 9 * src.C
        g, ldg = _mat(dy, "dy")
        ws = self._ws(dy, self.lib.uda_dwconv_workspace_bytes(dy.shape[0], src.C))
        self._ck(self.lib.uda_dwconv_wgrad(C.byref(s), g, ldg, stride, dil, border_mode, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                           _family(family), self._stream()))

    def dw_route(self, op, N, H, W, Cc, stride, dil, family="") -> str:
        """The launch the library plans for ``dwconv_fwd`` / ``dwconv_dgrad`` / ``dwconv_wgrad`` (op "fwd" / "dgrad" / "wgrad") on
        an N x H x W x Cc input grid: "<op> <kernel> ...", "none" for a shape the entry refuses (uda_dwconv_route)."""
        buf = C.create_string_buffer(96)
        self.lib.uda_dwconv_route(_DW_OP[op], N, H, W, Cc, stride, dil, _family(family), buf, len(buf))
        return buf.value.decode()

    # ------------------------------------------------------------------ stem
    def stem_fwd(self, x, w, out, stats=None):
        self._dev(x)
        N, c3, H, W = x.shape
        assert c3 == 3 and x.is_contiguous() and w.is_contiguous() and tuple(w.shape) == (32, 3, 3, 3)
        Po = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        assert out.shape == (Po, 32)
        y, ldy = _mat(out, "out")
        self._ck_stats(stats, 32)
        self._ck(self.lib.uda_stem_fwd(x.data_ptr(), N, H, W, w.data_ptr(), y, ldy, _ptr(stats), self._stream()))

    def stem_wgrad(self, x, dy, dw):
        N, _, H, W = x.shape
        Po = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        assert dy.shape == (Po, 32) and dw.is_contiguous() and dw.numel() == 864
        g, ldg = _mat(dy, "dy")
        ws = self._ws(dy, self.lib.uda_stem_workspace_bytes(Po))
        self._ck(self.lib.uda_stem_wgrad(x.data_ptr(), N, H, W, g, ldg, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                         self._stream()))

    def stem_route(self, op, x, dy=None) -> str:
        """The kernel ``stem_fwd`` (op "fwd") / ``stem_wgrad`` (op "wgrad", with its ``dy``) runs on the image batch ``x``:
        "fwd rows", "fwd pixels", "wgrad rows" or "wgrad pixels", then the grid (uda_stem_route)."""
        N, _, H, W = x.shape
        g, ldg = (0, 0) if dy is None else _mat(dy, "dy")
        buf = C.create_string_buffer(96)
        self.lib.uda_stem_route(_DW_OP[op], N, H, W, ldg, int(g % 16 == 0), buf, len(buf))
        return buf.value.decode()

    # ------------------------------------------------------------------ ResNet-101 pieces
    def stem7_fwd(self, x, w, out, stats=None):
        self._dev(x)
        N, c3, H, W = x.shape
        assert c3 == 3 and x.is_contiguous() and w.is_contiguous() and tuple(w.shape) == (64, 3, 7, 7)
        Po = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        assert out.shape == (Po, 64)
        y, ldy = _mat(out, "out")
        self._ck_stats(stats, 64)
        self._ck(self.lib.uda_stem7_fwd(x.data_ptr(), N, H, W, w.data_ptr(), y, ldy, _ptr(stats), self._stream()))

    def stem7_wgrad(self, x, dy, dw):
        N, _, H, W = x.shape
        Po = N * ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
        assert dy.shape == (Po, 64) and dw.is_contiguous() and dw.numel() == 64 * 147
        g, ldg = _mat(dy, "dy")
        ws = self._ws(dy, self.lib.uda_stem7_workspace_bytes(Po))
        self._ck(self.lib.uda_stem7_wgrad(x.data_ptr(), N, H, W, g, ldg, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                          self._stream()))

    # ------------------------------------------------------------------ DRN-D-54 head
    @staticmethod
    def relayout_hwio(w, dgrad=False):
        """[O, I, kh, kw] -> [kh, kw, I, O], the operand of stem7s1_fwd / conv3n_fwd (output channels fastest: one tap's
        weights of one input channel are consecutive).  dgrad=True: [kh, kw, O, I] with flipped taps, the operand that makes
        the stride-1 conv3n_fwd the input gradient."""
        if dgrad:
            return w.flip(2, 3).permute(2, 3, 0, 1).contiguous()
        return w.permute(2, 3, 1, 0).contiguous()

    def stem7s1_fwd(self, x, w_hwio, out, stats=None):
        self._dev(x)
        N, c3, H, W = x.shape
        assert c3 == 3 and x.is_contiguous() and w_hwio.is_contiguous() and tuple(w_hwio.shape) == (7, 7, 3, 16)
        assert out.shape == (N * H * W, 16)
        y, ldy = _mat(out, "out")
        self._ck_stats(stats, 16)
        self._ck(self.lib.uda_stem7s1_fwd(x.data_ptr(), N, H, W, w_hwio.data_ptr(), y, ldy, _ptr(stats), self._stream()))

    def stem7s1_wgrad(self, x, dy, dw):
        N, _, H, W = x.shape
        assert dy.shape == (N * H * W, 16) and dw.is_contiguous() and tuple(dw.shape) == (16, 3, 7, 7)
        g, ldg = _mat(dy, "dy")
        ws = self._ws(dy, self.lib.uda_stem7s1_workspace_bytes(N * H * W))
        self._ck(self.lib.uda_stem7s1_wgrad(x.data_ptr(), N, H, W, g, ldg, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                            self._stream()))

    def conv3n_fwd(self, src: Act, w_hwio, stride, out, stats=None):
        """narrow dense 3x3 (16 / 32 / 64 channels on either side, stride 1 | 2; anything else raises from the C side)"""
        s = self._src(src)
        Cout = out.shape[1]
        Ho, Wo = (src.H - 1) // stride + 1, (src.W - 1) // stride + 1
        assert out.shape[0] == src.N * Ho * Wo and w_hwio.is_contiguous() and tuple(w_hwio.shape) == (3, 3, src.C, Cout)
        y, ldy = _mat(out, "out")
        self._ck_stats(stats, Cout)
        self._ck(self.lib.uda_conv3n_fwd(C.byref(s), w_hwio.data_ptr(), Cout, stride, y, ldy, _ptr(stats), self._stream()))

    def conv3n_wgrad(self, src: Act, dy, stride, dw):
        s = self._src(src)
        Cout = dy.shape[1]
        Ho, Wo = (src.H - 1) // stride + 1, (src.W - 1) // stride + 1
        assert dy.shape[0] == src.N * Ho * Wo and dw.is_contiguous() and tuple(dw.shape) == (Cout, src.C, 3, 3)
        g, ldg = _mat(dy, "dy")
        ws = self._ws(dy, self.lib.uda_conv3n_workspace_bytes(src.C, Cout))
        self._ck(self.lib.uda_conv3n_wgrad(C.byref(s), g, ldg, Cout, stride, dw.data_ptr(), ws.data_ptr(), ws.numel(),
                                           self._stream()))

    def maxpool_fwd(self, src: Act, out, idx):
        s = self._src(src)
        Po = src.N * ((src.H - 1) // 2 + 1) * ((src.W - 1) // 2 + 1)
        assert out.shape == (Po, src.C) and idx.shape == (Po, src.C) and idx.dtype == torch.uint8
        o, ldo = _mat(out, "out")
        i, ldi = _mat(idx, "idx")
        self._ck(self.lib.uda_maxpool_fwd(C.byref(s), o, ldo, i, ldi, self._stream()))

    def maxpool_bwd(self, dz, idx, N, H, W, out):
        Cc = dz.shape[1]
        assert out.shape == (N * H * W, Cc) and idx.shape == dz.shape
        g, ldg = _mat(dz, "dz")
        i, ldi = _mat(idx, "idx")
        o, ldo = _mat(out, "out")
        self._ck(self.lib.uda_maxpool_bwd(g, ldg, i, ldi, N, H, W, Cc, o, ldo, self._stream()))

    def rows_stride(self, src, N, H, W, stride, out, scatter=False):
        """scatter=False: out[(n,oh,ow)] = src[(n,oh*s,ow*s)] (src is the H x W side); scatter=True: the
        transpose, out is the H x W side and receives zeros between the samples."""
        Cc = src.shape[1]
        Po = N * ((H - 1) // stride + 1) * ((W - 1) // stride + 1)
        big, small = (out, src) if scatter else (src, out)
        assert big.shape == (N * H * W, Cc) and small.shape == (Po, Cc)
        a, lda = _mat(src, "src")
        o, ldo = _mat(out, "out")
        self._ck(self.lib.uda_rows_stride(a, lda, N, H, W, Cc, stride, int(scatter), o, ldo, self._stream()))

    def bn_add_relu(self, a: Act, b: Act, out):
        sa, sb = self._src(a), self._src(b)
        assert out.shape == a.x.shape == b.x.shape
        o, ldo = _mat(out, "out")
        self._ck(self.lib.uda_bn_add_relu(C.byref(sa), C.byref(sb), o, ldo, self._stream()))

    def relu_gate(self, dz, z, out):
        assert dz.shape == z.shape == out.shape
        g, ldg = _mat(dz, "dz")
        v, ldv = _mat(z, "z")
        o, ldo = _mat(out, "out")
        self._ck(self.lib.uda_relu_gate(g, ldg, v, ldv, dz.shape[0], dz.shape[1], o, ldo, self._stream()))

    # ------------------------------------------------------------------ patch-discriminator geometry
    def relayout_s2d(self, w, dgrad):
        O, Cc = w.shape[0], w.shape[1]
        assert tuple(w.shape[2:]) == (4, 4)
        out = torch.empty(conv_weight_shape(4 * Cc, 2, O) if dgrad else conv_weight_shape(O, 2, 4 * Cc), dtype=torch.float32,
                          device=w.device)
        self._ck(self.lib.uda_relayout_s2d(w.detach().contiguous().data_ptr(), O, Cc, int(bool(dgrad)), out.data_ptr(), self._stream()))
        return out

    def s2d_fwd(self, src, nchw, N, Hs, Ws, Cc, vh, vw, slope, z):
        """src: NCHW tensor (nchw=True) or [N*Hs*Ws, C] rows; z: [N*Hz*Wz, 4C] rows with Hz = (vh+5)//2."""
        self._dev(src)
        Hz, Wz = (vh + 5) // 2, (vw + 5) // 2
        assert z.shape == (N * Hz * Wz, 4 * Cc)
        if nchw:
            assert src.is_contiguous() and tuple(src.shape) == (N, Cc, Hs, Ws)
            sp, lds_ = src.data_ptr(), 0
        else:
            assert src.shape == (N * Hs * Ws, Cc)
            sp, lds_ = _mat(src, "src")
        zp, ldz = _mat(z, "z")
        self._ck(self.lib.uda_s2d_fwd(sp, lds_, int(nchw), N, Hs, Ws, Cc, vh, vw, float(slope), zp, ldz, Hz, Wz, self._stream()))

    # ---- bf16x3: space-to-depth operands in packed form only (no fp32 image); the engine asks the routing predicates first
    @staticmethod
    def _raw_src(N, H, W, Cc) -> UdaSrc:
        """descriptor of a raw [N*H*W, Cc] operand by shape alone, for the routing predicates"""
        s = UdaSrc()
        s.N, s.H, s.W, s.C, s.ldx = N, H, W, Cc, round4(Cc)
        return s

    def conv_route_x3(self, N, H, W, Cin, Cout, ksize):
        """True when ``conv`` of a RAW [N*H*W, Cin] operand to Cout outputs runs on the bf16x3 kernel in one launch."""
        if self.mfma != self.MFMA_BF16X3 or self._image_groups(N, H * W, max(round4(Cin), round4(Cout)), Cin) is not None:
            return False
        return bool(self.lib.uda_conv_uses_x3(C.byref(self.conv_args(self._raw_src(N, H, W, Cin), Cout, ksize))))

    def wgrad_route_x3(self, N, H, W, Cin, Cout, ksize):
        """True when ``conv_wgrad`` of a raw [N*H*W, Cin] source against a [N*H*W, Cout] gradient runs on the bf16x3 kernel."""
        if self.mfma != self.MFMA_BF16X3 or self._image_groups(N, H * W, max(round4(Cin), round4(Cout))) is not None:
            return False
        return bool(self.lib.uda_conv_wgrad_uses_x3(C.byref(self.wgrad_args(self._raw_src(N, H, W, Cin), Cout, ksize))))

    def _packed_only(self, rows, Cc, device):
        """A [rows, Cc] fp32 matrix that exists ONLY in packed bf16x3 form: the returned tensor is an (uninitialised, never
        read) fp32 view over the head of the packed buffer, which rides on it as ``_x3`` like any cached packed operand -
        the x3 conv / weight-gradient kernels read nothing else.  It is marked (``_x3_only``): ``conv``, ``conv_wgrad`` and
        ``_packed`` raise where it would be read as fp32 rows (``_refuse_x3_only``).  Returns (matrix, packed bytes)."""
        xs = torch.empty(int(self.lib.uda_x3_packed_bytes(rows, Cc)), dtype=torch.uint8, device=device)
        m = xs[:rows * Cc * 4].view(torch.float32).view(rows, Cc)
        m._x3 = xs
        m._x3_only = True
        return m, xs

    def packed_out(self, rows, Cc, device, fp32=None):
        """The destination(s) of a producer that writes its [rows, Cc] result as a packed bf16x3 operand (``bnbwd_apply`` /
        ``upconv_bwd`` with ``out_x3``): -> (matrix, packed bytes).  Without ``fp32`` the matrix is packed-only
        (``_packed_only``); with it (a [rows, Cc] fp32 matrix the producer writes too) the packed form is attached to that."""
        if fp32 is None:
            return self._packed_only(rows, Cc, device)
        assert tuple(fp32.shape) == (rows, Cc)
        xs = torch.empty(int(self.lib.uda_x3_packed_bytes(rows, Cc)), dtype=torch.uint8, device=device)
        fp32._x3 = xs
        return fp32, xs

    def _x3_dst(self, out, out_x3, rows, Cc):
        """(fp32 address or None, row stride, packed address) of a producer's destinations; a packed-only ``out`` has no fp32 side"""
        assert out_x3.dtype == torch.uint8 and out_x3.is_contiguous() and out_x3.data_ptr() % 16 == 0
        assert out_x3.numel() == int(self.lib.uda_x3_packed_bytes(rows, Cc))
        if out is None or self._x3_only(out):
            return None, 0, out_x3.data_ptr()
        return _mat(out, "out") + (out_x3.data_ptr(),)

    def s2d_pack_fwd(self, src, N, Hs, Ws, Cc, vh, vw, slope):
        """uda_s2d_fwd + uda_x3_pack in one pass: src rows [N*Hs*Ws, Cc] -> the packed z image (a packed-only matrix
        [N*Hz*Wz, 4*Cc], see ``_packed_only``)."""
        self._dev(src)
        Hz, Wz = (vh + 5) // 2, (vw + 5) // 2
        assert src.shape == (N * Hs * Ws, Cc) and Cc % 8 == 0
        sp, lds_ = _mat(src, "src")
        z, xs = self._packed_only(N * Hz * Wz, 4 * Cc, src.device)
        self._ck(self.lib.uda_x3_pack_s2d_fwd(sp, lds_, N, Hs, Ws, Cc, vh, vw, float(slope), Hz, Wz, xs.data_ptr(), self._stream()))
        return z

    def s2d_pack_bwd(self, dz, gate, slope, N, Hs, Ws, Cc, vh, vw):
        """uda_s2d_bwd_gate + uda_x3_pack in one pass: the packed-only gradient matrix [N*Hs*Ws, Cc]."""
        Hz, Wz = (vh + 5) // 2, (vw + 5) // 2
        assert dz.shape == (N * Hz * Wz, 4 * Cc) and Cc % 8 == 0 and (gate is None or gate.shape == (N * Hs * Ws, Cc))
        gp, ldz = _mat(dz, "dz")
        tp, ldt = (None, 0) if gate is None else _mat(gate, "gate")
        d, xs = self._packed_only(N * Hs * Ws, Cc, dz.device)
        self._ck(self.lib.uda_x3_pack_s2d_bwd(gp, ldz, Hz, Wz, tp, ldt, float(slope), N, Hs, Ws, Cc, vh, vw, xs.data_ptr(), self._stream()))
        return d

    def s2d_bwd(self, dz, z_sign, slope, N, Hs, Ws, Cc, vh, vw, dst, nchw, gate=None):
        """``gate``: rows [N*Hs*Ws, Cc] of the forward's source whose sign is the LeakyReLU gate (instead of z_sign)."""
        Hz, Wz = (vh + 5) // 2, (vw + 5) // 2
        assert dz.shape == (N * Hz * Wz, 4 * Cc) and (z_sign is None or (z_sign.shape == dz.shape and z_sign.stride(0) == dz.stride(0)))
        gp, ldz = _mat(dz, "dz")
        if gate is not None:
            assert z_sign is None and not nchw and gate.shape == (N * Hs * Ws, Cc) and dst.shape == (N * Hs * Ws, Cc)
            tp, ldt = _mat(gate, "gate")
            dp, ldd = _mat(dst, "dst")
            self._ck(self.lib.uda_s2d_bwd_gate(gp, ldz, Hz, Wz, tp, ldt, float(slope), N, Hs, Ws, Cc, vh, vw, dp, ldd, self._stream()))
            return
        if nchw:
            assert dst.is_contiguous() and tuple(dst.shape) == (N, Cc, Hs, Ws)
            dp, ldd = dst.data_ptr(), 0
        else:
            assert dst.shape == (N * Hs * Ws, Cc)
            dp, ldd = _mat(dst, "dst")
        self._ck(self.lib.uda_s2d_bwd(gp, _ptr(z_sign), ldz, Hz, Wz, float(slope), N, Hs, Ws, Cc, vh, vw, dp, ldd, int(nchw),
                                      self._stream()))

    def adv_s2d_fwd(self, logits, pre_op, z):
        """z = s2d(pre(logits)), logits NCHW [N,C,H,W]; pre_op 1 = sigmoid, 2 = -sigmoid * log(sigmoid + 1e-7)."""
        self._dev(logits)
        N, Cc, H, W = logits.shape
        Hz, Wz = (H + 5) // 2, (W + 5) // 2
        assert logits.is_contiguous() and logits.dtype == torch.float32 and z.shape == (N * Hz * Wz, 4 * Cc)
        zp, ldz = _mat(z, "z")
        self._ck(self.lib.uda_adv_s2d_fwd(logits.data_ptr(), N, Cc, H, W, int(pre_op), zp, ldz, Hz, Wz, self._stream()))

    def adv_s2d_bwd(self, dz, logits, pre_op, d_logits):
        N, Cc, H, W = logits.shape
        Hz, Wz = (H + 5) // 2, (W + 5) // 2
        assert dz.shape == (N * Hz * Wz, 4 * Cc) and logits.is_contiguous() and d_logits.is_contiguous()
        assert tuple(d_logits.shape) == tuple(logits.shape)
        gp, ldz = _mat(dz, "dz")
        self._ck(self.lib.uda_adv_s2d_bwd(gp, ldz, Hz, Wz, logits.data_ptr(), N, Cc, H, W, int(pre_op), d_logits.data_ptr(),
                                          self._stream()))

    # ------------------------------------------------------------------ batch norm
    def bn_finalize(self, stats, count, gamma, beta, rmean, rvar, momentum, eps, scale, shift, mean, invstd):
        Cc = gamma.numel()
        for t in (gamma, beta, rmean, rvar, scale, shift, mean, invstd):
            assert t.is_contiguous() and t.numel() == Cc
        assert stats.dtype == torch.float64 and stats.is_contiguous() and tuple(stats.shape) == (STAT_SLOTS, 2, Cc)
        self._ck(self.lib.uda_bn_finalize(stats.data_ptr(), Cc, float(count), gamma.data_ptr(), beta.data_ptr(),
                                          rmean.data_ptr(), rvar.data_ptr(), momentum, eps, scale.data_ptr(),
                                          shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), self._stream()))

    def bn_running_replay(self, mean, invstd, count, k, momentum, eps, rmean, rvar):
        Cc = mean.numel()
        for t in (mean, invstd, rmean, rvar):
            assert t.is_contiguous() and t.numel() == Cc
        self._ck(self.lib.uda_bn_running_replay(mean.data_ptr(), invstd.data_ptr(), Cc, float(count), int(k), momentum, eps,
                                                rmean.data_ptr(), rvar.data_ptr(), self._stream()))

    def bn_eval_coeffs(self, gamma, beta, rmean, rvar, eps, scale, shift):
        Cc = gamma.numel()
        for t in (gamma, beta, rmean, rvar, scale, shift):
            assert t.is_contiguous() and t.numel() == Cc
        self._ck(self.lib.uda_bn_eval_coeffs(gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), Cc,
                                             eps, scale.data_ptr(), shift.data_ptr(), self._stream()))

    def tn_gain(self, stats0, stats1, count0, count1, eps, scale0, shift0, scale1, shift1, gain):
        Cc = gain.numel()
        for t in (scale0, shift0, scale1, shift1, gain):
            assert t.is_contiguous() and t.numel() == Cc
        for st in (stats0, stats1):
            assert st.dtype == torch.float64 and st.is_contiguous() and tuple(st.shape) == (STAT_SLOTS, 2, Cc)
        self._ck(self.lib.uda_tn_gain(stats0.data_ptr(), stats1.data_ptr(), Cc, float(count0), float(count1), eps,
                                      scale0.data_ptr(), shift0.data_ptr(), scale1.data_ptr(), shift1.data_ptr(),
                                      gain.data_ptr(), self._stream()))

    def tn_eval_coeffs(self, gamma, beta, rmean_s, rvar_s, rmean_t, rvar_t, eps, scale, shift):
        Cc = gamma.numel()
        for t in (gamma, beta, rmean_s, rvar_s, rmean_t, rvar_t, scale, shift):
            assert t.is_contiguous() and t.numel() == Cc
        self._ck(self.lib.uda_tn_eval_coeffs(gamma.data_ptr(), beta.data_ptr(), rmean_s.data_ptr(), rvar_s.data_ptr(),
                                             rmean_t.data_ptr(), rvar_t.data_ptr(), Cc, eps, scale.data_ptr(),
                                             shift.data_ptr(), self._stream()))

    def bn_apply(self, src: Act, out, residual=None):
        s = self._src(src)
        assert out.shape == src.x.shape and src.C % 4 == 0
        o, ldo = _mat(out, "out")
        r, ldr = (None, 0) if residual is None else _mat(residual, "residual")
        self._ck(self.lib.uda_bn_apply(C.byref(s), r, ldr, o, ldo, self._stream()))

    def colstats(self, x, stats):
        self._dev(x)
        p, ld = _mat(x, "x")
        slots, nq, Cc = stats.shape
        assert slots == STAT_SLOTS and Cc == x.shape[1] and stats.dtype == torch.float64 and stats.is_contiguous()
        self._ck(self.lib.uda_colstats(p, ld, x.shape[0], Cc, nq, stats.data_ptr(), self._stream()))

    def colstats_window(self, x, stats, c_off):
        """(sum, sum of squares) of x's channels ADDED into channels [c_off, c_off + C) of the wider accumulator ``stats``."""
        self._dev(x)
        p, ld = _mat(x, "x")
        slots, nq, Cs = stats.shape
        Cc = x.shape[1]
        assert slots == STAT_SLOTS and c_off >= 0 and c_off + Cc <= Cs and stats.dtype == torch.float64 and stats.is_contiguous()
        self._ck(self.lib.uda_colstats_window(p, ld, x.shape[0], Cc, nq, stats.data_ptr() + 8 * c_off, Cs, self._stream()))

    def colsum(self, x, out):
        st = torch.zeros(STAT_SLOTS, 1, x.shape[1], dtype=torch.float64, device=x.device)
        self.colstats(x, st)
        out.copy_(st.sum(0)[0])

    @staticmethod
    def _lowrank(lowrank, y):
        """(d [P, k] rows, w [k, C] contiguous) of dU = d @ w, k = 1 or 2"""
        d, w = lowrank
        k = d.shape[1]
        assert k in (1, 2) and d.shape[0] == y.P and tuple(w.shape) == (k, y.C) and w.is_contiguous() and d.stride(1) == 1
        assert d.dtype == w.dtype == torch.float32
        return d.data_ptr(), d.stride(0), k, w.data_ptr()

    def bnbwd_reduce(self, dU, y: Act, sums, lowrank=None):
        s = self._src(y)
        assert sums.dtype == torch.float64 and tuple(sums.shape) == (STAT_SLOTS, 3, y.C) and sums.is_contiguous()
        if lowrank is not None:
            dp, ldd, k, wp = self._lowrank(lowrank, y)
            self._ck(self.lib.uda_bnbwd_reduce_lowrank(dp, ldd, k, wp, C.byref(s), y.bn.mean.data_ptr(), y.bn.invstd.data_ptr(),
                                                       sums.data_ptr(), self._stream()))
            return
        assert dU.shape == y.x.shape
        d, ldu = _mat(dU, "dU")
        self._ck(self.lib.uda_bnbwd_reduce(d, ldu, C.byref(s), y.bn.mean.data_ptr(), y.bn.invstd.data_ptr(),
                                           sums.data_ptr(), self._stream()))

    def bnbwd_finalize(self, sums, y: Act, c1, c2, dgamma, dbeta, q1_total=None):
        if q1_total is not None:
            assert q1_total.is_contiguous() and q1_total.numel() == y.C and q1_total.dtype == torch.float32
        self._ck(self.lib.uda_bnbwd_finalize(sums.data_ptr(), y.C, float(y.bn.count), int(y.bn.q1_border), y.act,
                                             y.shift.data_ptr(), y.bn.mean.data_ptr(), y.bn.invstd.data_ptr(), _ptr(q1_total),
                                             c1.data_ptr(), c2.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(),
                                             self._stream()))

    def bnbwd_apply(self, dU, y: Act, c1, c2, out, addend=None, lowrank=None, out_x3=None):
        """``out_x3`` (uint8, uda_x3_packed_bytes(P, C) bytes): the result also - with a packed-only or absent ``out``: only - as
        the packed bf16x3 operand ``x3_pack`` would make of ``out``, written in the same pass (``packed_out``)"""
        s = self._src(y)
        ad, lda = (None, 0) if addend is None else _mat(addend, "addend")
        if out_x3 is not None:
            assert out is None or y.x.shape == out.shape
            o, ldo, ox = self._x3_dst(out, out_x3, y.P, y.C)
            if lowrank is not None:
                dp, ldd, k, wp = self._lowrank(lowrank, y)
                self._ck(self.lib.uda_bnbwd_apply_lowrank_x3(dp, ldd, k, wp, C.byref(s), y.bn.mean.data_ptr(), y.bn.invstd.data_ptr(),
                                                             c1.data_ptr(), c2.data_ptr(), ad, lda, o, ldo, ox, self._stream()))
                return
            assert dU.shape == y.x.shape
            d, ldu = _mat(dU, "dU")
            self._ck(self.lib.uda_bnbwd_apply_x3(d, ldu, C.byref(s), y.bn.mean.data_ptr(), y.bn.invstd.data_ptr(),
                                                 c1.data_ptr(), c2.data_ptr(), ad, lda, o, ldo, ox, self._stream()))
            return
        assert y.x.shape == out.shape
        o, ldo = _mat(out, "out")
        if lowrank is not None:
            dp, ldd, k, wp = self._lowrank(lowrank, y)
            self._ck(self.lib.uda_bnbwd_apply_lowrank(dp, ldd, k, wp, C.byref(s), y.bn.mean.data_ptr(), y.bn.invstd.data_ptr(),
                                                      c1.data_ptr(), c2.data_ptr(), ad, lda, o, ldo, self._stream()))
            return
        assert dU.shape == y.x.shape
        d, ldu = _mat(dU, "dU")
        self._ck(self.lib.uda_bnbwd_apply(d, ldu, C.byref(s), y.bn.mean.data_ptr(), y.bn.invstd.data_ptr(),
                                          c1.data_ptr(), c2.data_ptr(), ad, lda, o, ldo, self._stream()))

    # ------------------------------------------------------------------ resampling / pooling
    def upsample_fwd(self, x, N, h, w, out, H, W, stats=None):
        """``stats`` (fp64 [SLOTS, 2, Cs >= C]): also ADD the output's per-channel (sum, sum of squares) into its channels [0, C)."""
        self._dev(x)
        p, ld = _mat(x, "x")
        o, ldo = _mat(out, "out")
        assert x.shape[0] == N * h * w and out.shape == (N * H * W, x.shape[1])
        if stats is not None:
            assert stats.dtype == torch.float64 and stats.is_contiguous() and stats.shape[:2] == (STAT_SLOTS, 2) and stats.shape[2] >= x.shape[1]
            self._ck(self.lib.uda_upsample_fwd_stats(p, ld, N, h, w, x.shape[1], o, ldo, H, W, stats.data_ptr(), stats.shape[2], self._stream()))
            return
        self._ck(self.lib.uda_upsample_fwd(p, ld, N, h, w, x.shape[1], o, ldo, H, W, self._stream()))

    def upsample_stats(self, x, N, h, w, H, W, stats):
        """per-channel (sum, sum of squares) of the bilinearly upsampled tensor ADDED into channels [0, C) of ``stats``; the
        tensor itself is not written"""
        self._dev(x)
        p, ld = _mat(x, "x")
        assert x.shape[0] == N * h * w and stats.dtype == torch.float64 and stats.is_contiguous()
        assert stats.shape[:2] == (STAT_SLOTS, 2) and stats.shape[2] >= x.shape[1]
        self._ck(self.lib.uda_upsample_fwd_stats(p, ld, N, h, w, x.shape[1], None, 0, H, W, stats.data_ptr(), stats.shape[2], self._stream()))

    def mc_seg_head(self, feature, N, h, w, low, bnd, H, W, scale, shift, act, mask, mask_scale, wgt, bias, out):
        """decoder.last_conv on the virtual x_feature = cat(up(feature), low rows (shared by the repeated batch), boundary):
        ``uda_mc_seg_head``.  feature [N*h*w, Cf], low [P_low, Cl] with P_low | N*H*W, bnd [N*H*W, 1], wgt = relayout_ohwi of the
        [2, C, 1, 1] weight, out [N*H*W, 2]."""
        self._dev(feature)
        fp, ldf = _mat(feature, "feature")
        lp, ldl = _mat(low, "low")
        P = N * H * W
        Cf, Cl = feature.shape[1], low.shape[1]
        Cc = Cf + Cl + 1
        assert feature.shape[0] == N * h * w and P % low.shape[0] == 0 and bnd.shape == (P, 1) and out.shape == (P, 2)
        assert bnd.stride(1) == 1 and out.stride(1) == 1 and wgt.is_contiguous() and wgt.shape[0] == 2 and wgt.numel() // 2 >= Cc
        assert scale.is_contiguous() and shift.is_contiguous() and scale.numel() == Cc and bias.numel() == 2
        mp, ldm = (None, 0)
        if mask is not None:
            assert mask.dtype == torch.uint8 and mask.shape == (P, Cc) and mask.stride(1) == 1
            mp, ldm = mask.data_ptr(), mask.stride(0)
        self._ck(self.lib.uda_mc_seg_head(fp, ldf, N, h, w, Cf, lp, ldl, Cl, low.shape[0], bnd.data_ptr(), bnd.stride(0), H, W,
                                          scale.data_ptr(), shift.data_ptr(), int(act), mp, ldm, float(mask_scale), wgt.data_ptr(),
                                          wgt.numel() // 2, bias.data_ptr(), out.data_ptr(), out.stride(0), self._stream()))

    def upsample_bwd(self, dout, N, H, W, dx, h, w):
        p, ld = _mat(dout, "dout")
        o, ldo = _mat(dx, "dx")
        assert dout.shape[0] == N * H * W and dx.shape == (N * h * w, dout.shape[1])
        self._ck(self.lib.uda_upsample_bwd(p, ld, N, H, W, dout.shape[1], o, ldo, h, w, self._stream()))

    def upconv_fwd(self, g, N, h, w, out, H, W, addend=None, dil=1, stats=None):
        """out[p] = addend[p % addend.rows] + sum over the 9 taps of the bilinear (align_corners) read of g's tap plane at the tap
        position; g: [N*h*w, 9*C] (tap-major columns), out: [N*H*W, C]; stats ([SLOTS, 2, C] fp64, added into): column sums
        and sums of squares of out (by the kernel or by a colstats launch after it, as the library's launch plan says)."""
        self._dev(g)
        Cc = out.shape[1]
        assert g.shape == (N * h * w, 9 * Cc) and out.shape[0] == N * H * W
        gp, ldg = _mat(g, "g")
        o, ldo = _mat(out, "out")
        ad, lda, rows = (None, 0, 1) if addend is None else (_mat(addend, "addend") + (addend.shape[0],))
        if addend is not None:
            assert addend.shape[1] == Cc and (N * H * W) % addend.shape[0] == 0
        self._ck_stats(stats, Cc)
        self._ck(self.lib.uda_upconv_fwd(gp, ldg, N, h, w, Cc, dil, ad, lda, rows, o, ldo, H, W, _ptr(stats), self._stream()))

    def upconv_bwd(self, dy, N, H, W, dg, h, w, dil=1, dg_x3=None):
        """``dg_x3`` (uint8, uda_x3_packed_bytes(N*h*w, 9*C) bytes): dg also - with a packed-only or absent ``dg``: only - as the
        packed bf16x3 operand ``x3_pack`` would make of it, written in the same pass (``packed_out``)"""
        self._dev(dy)
        Cc = dy.shape[1]
        assert dy.shape[0] == N * H * W and (dg is None or dg.shape == (N * h * w, 9 * Cc))
        d, ldy = _mat(dy, "dy")
        if dg_x3 is not None:
            gp, ldg, gx = self._x3_dst(dg, dg_x3, N * h * w, 9 * Cc)
            self._ck(self.lib.uda_upconv_bwd_x3(d, ldy, N, H, W, Cc, dil, gp, ldg, gx, h, w, self._stream()))
            return
        gp, ldg = _mat(dg, "dg")
        self._ck(self.lib.uda_upconv_bwd(d, ldy, N, H, W, Cc, dil, gp, ldg, h, w, self._stream()))

    def upconv_route(self, op, N, h, w, H, W, Cc, dil=1, ldg=None, ld_add=None, addend_rows=0, stats=False) -> str:
        """The launch the library plans for ``upconv_fwd`` (op "fwd") / ``upconv_bwd`` (op "bwd"): "<op> <kernel> grid ...", for a
        forward with statistics ending in "stats fused" or "stats colstats"; "none" for arguments the entry refuses
        (uda_upconv_route).  ldg: row stride of g / dg (default 9 * Cc); ld_add: row stride of the addend, None without one."""
        buf = C.create_string_buffer(96)
        self.lib.uda_upconv_route(_UP_OP[op], N, h, w, H, W, Cc, dil, 9 * Cc if ldg is None else ldg, int(ld_add is not None),
                                  ld_add or 0, addend_rows, int(stats), buf, len(buf))
        return buf.value.decode()

    def head_upsample_fwd(self, x, N, h, w, out):
        self._dev(x)
        p, ld = _mat(x, "x")
        Cc = x.shape[1]
        assert out.is_contiguous() and out.shape[0] == N and out.shape[1] == Cc and x.shape[0] == N * h * w
        self._ck(self.lib.uda_head_upsample_fwd(p, ld, N, h, w, Cc, out.data_ptr(), out.shape[2], out.shape[3],
                                                self._stream()))

    def head_upsample_bwd(self, dout, dx, N, h, w, accumulate=False):
        self._dev(dout)
        p, ld = _mat(dx, "dx")
        assert dout.is_contiguous() and dout.shape[0] == N and dout.shape[1] == dx.shape[1] and dx.shape[0] == N * h * w
        self._ck(self.lib.uda_head_upsample_bwd(dout.data_ptr(), N, dout.shape[1], dout.shape[2], dout.shape[3], p, ld,
                                                h, w, int(accumulate), self._stream()))

    def gap_fwd(self, x, N, out, scale):
        self._dev(x)
        p, ld = _mat(x, "x")
        o, ldo = _mat(out, "out")
        assert x.shape[0] % N == 0 and out.shape == (N, x.shape[1])
        self._ck(self.lib.uda_gap_fwd(p, ld, N, x.shape[0] // N, x.shape[1], scale, o, ldo, self._stream()))

    def broadcast_rows(self, g, N, out, scale, addend=None):
        self._dev(g)
        p, ld = _mat(g, "g")
        o, ldo = _mat(out, "out")
        assert g.shape == (N, out.shape[1]) and out.shape[0] % N == 0
        ad, lda = (None, 0) if addend is None else _mat(addend, "addend")
        self._ck(self.lib.uda_broadcast_rows(p, ld, N, out.shape[0] // N, out.shape[1], scale, ad, lda, o, ldo,
                                             self._stream()))

    def dropout_mask(self, mask, p, seed, offset):
        self._dev(mask)
        assert mask.dtype == torch.uint8 and mask.stride(1) == 1
        self._ck(self.lib.uda_dropout_mask(mask.data_ptr(), mask.stride(0), mask.shape[0], mask.shape[1], p,
                                           int(seed), int(offset), self._stream()))

    # ------------------------------------------------------------------ losses / metrics
    def seg_loss_fwd(self, o, tmap, b, tbd):
        """-> device float[3] = (BCE(sigmoid(o), map) + MSE(sigmoid(b), boundary), bce, mse)"""
        for t in (o, tmap, b, tbd):
            self._dev(t)
            assert t.is_contiguous()
        assert o.shape == tmap.shape and b.shape == tbd.shape
        loss = torch.empty(3, dtype=torch.float32, device=o.device)
        ws = torch.empty(2, dtype=torch.float64, device=o.device)
        self._ck(self.lib.uda_seg_loss_fwd(o.data_ptr(), tmap.data_ptr(), o.numel(), b.data_ptr(), tbd.data_ptr(),
                                           b.numel(), loss.data_ptr(), ws.data_ptr(), self._stream()))
        return loss

    def seg_loss_bwd(self, o, tmap, b, tbd, gscale):
        d_o, d_b = torch.empty_like(o), torch.empty_like(b)
        assert gscale.numel() == 1 and gscale.dtype == torch.float32
        self._ck(self.lib.uda_seg_loss_bwd(o.data_ptr(), tmap.data_ptr(), o.numel(), b.data_ptr(), tbd.data_ptr(),
                                           b.numel(), gscale.data_ptr(), d_o.data_ptr(), d_b.data_ptr(), self._stream()))
        return d_o, d_b

    def seg_counts(self, logits, target, thr):
        """-> int64 [C, 3] = (intersection, predicted, ground truth) for sigmoid(logits) > thr"""
        self._dev(logits)
        assert logits.is_contiguous() and target.is_contiguous() and logits.shape == target.shape
        B, Cc, H, W = logits.shape
        counts = torch.empty(Cc, 3, dtype=torch.int64, device=logits.device)
        self._ck(self.lib.uda_seg_counts(logits.data_ptr(), target.data_ptr(), B, Cc, H * W, thr, counts.data_ptr(),
                                         self._stream()))
        return counts

    # ------------------------------------------------------------------ prototypes
    def mc_stats(self, preds, T):
        self._dev(preds)
        assert preds.is_contiguous() and preds.shape[0] % T == 0
        shape = (preds.shape[0] // T,) + tuple(preds.shape[1:])
        std = torch.empty(shape, dtype=torch.float32, device=preds.device)
        mean = torch.empty_like(std)
        self._ck(self.lib.uda_mc_stats(preds.data_ptr(), T, std.numel(), std.data_ptr(), mean.data_ptr(), self._stream()))
        return std, mean

    def proto_weights(self, mode, B, h, w, map_=None, logits=None, std_map=None, mean_map=None):
        dev = (map_ if map_ is not None else logits).device
        P = B * h * w
        wts = torch.empty(P, 4, dtype=torch.float32, device=dev)
        H = W = 0
        m0 = m1 = None
        if mode == 0:
            assert map_.is_contiguous() and map_.shape[:2] == (B, 2)
            H, W = map_.shape[2], map_.shape[3]
        if mode in (1, 2):
            assert logits.shape == (P, 2) and logits.stride(1) == 1
        if mode == 2:
            assert std_map.is_contiguous() and mean_map.is_contiguous() and std_map.shape == mean_map.shape
            H, W = std_map.shape[2], std_map.shape[3]
            m0 = torch.empty(P, dtype=torch.float32, device=dev)
            m1 = torch.empty(P, dtype=torch.float32, device=dev)
        self._ck(self.lib.uda_proto_weights(mode, B, h, w, H, W, _ptr(map_), _ptr(logits),
                                            0 if logits is None else logits.stride(0), _ptr(std_map), _ptr(mean_map),
                                            wts.data_ptr(), _ptr(m0), _ptr(m1), self._stream()))
        return wts, m0, m1

    def proto_reduce(self, feat, wts, sums):
        self._dev(feat)
        f, ldf = _mat(feat, "feat")
        P, Cc = feat.shape
        assert wts.shape == (P, 4) and wts.is_contiguous() and sums.dtype == torch.float64 and tuple(sums.shape) == (4, Cc + 1)
        ws = self._ws(feat, self.lib.uda_proto_workspace_bytes(P, Cc))
        self._ck(self.lib.uda_proto_reduce(f, ldf, P, Cc, wts.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                           self._stream()))

    def proto_finalize(self, sums):
        Cc = sums.shape[1] - 1
        cent = torch.empty(4, Cc, dtype=torch.float32, device=sums.device)
        self._ck(self.lib.uda_proto_finalize(sums.data_ptr(), Cc, cent.data_ptr(), self._stream()))
        return cent

    def proto_scatter(self, feat, wts, scatter, centre=None):
        """scatter (double [4, C, C]) += sum_p w_k[p] (f[p] - centre_k)(f[p] - centre_k)^T; centre float [4, C] or None (zeros)"""
        self._dev(feat)
        f, ldf = _mat(feat, "feat")
        P, Cc = feat.shape
        assert wts.shape == (P, 4) and wts.is_contiguous() and wts.dtype == torch.float32
        assert scatter.dtype == torch.float64 and scatter.is_contiguous() and tuple(scatter.shape) == (4, Cc, Cc)
        if centre is not None:
            assert centre.dtype == torch.float32 and centre.is_contiguous() and tuple(centre.shape) == (4, Cc)
        ws = self._ws(feat, self.lib.uda_proto_scatter_workspace_bytes(Cc))
        self._ck(self.lib.uda_proto_scatter(f, ldf, P, Cc, wts.data_ptr(), _ptr(centre), scatter.data_ptr(), ws.data_ptr(), ws.numel(),
                                            self._stream()))

    def proto_bwd(self, feat, wts, sums, dC, d_feat=None, accumulate=False, want_dw=False):
        f, ldf = _mat(feat, "feat")
        P, Cc = feat.shape
        assert dC.is_contiguous() and tuple(dC.shape) == (4, Cc) and dC.dtype == torch.float32
        coef = torch.empty(4, Cc + 1, dtype=torch.float32, device=feat.device)
        d_w = torch.empty(P, 4, dtype=torch.float32, device=feat.device) if want_dw else None
        dptr, ldd = (None, 0) if d_feat is None else _mat(d_feat, "d_feat")
        self._ck(self.lib.uda_proto_bwd(f, ldf, P, Cc, wts.data_ptr(), sums.data_ptr(), dC.data_ptr(), coef.data_ptr(),
                                        dptr, ldd, int(accumulate), _ptr(d_w), self._stream()))
        return d_w

    def proto_align_fwd(self, cur_src, cur_tgt, prev_src, prev_tgt, decay):
        """-> (new_src [4,C], new_tgt [4,C], losses float[2] = (intra, inter)); prev_* None on first use."""
        self._dev(cur_src)
        Cc = cur_src.shape[1]
        for t in (cur_src, cur_tgt, prev_src, prev_tgt):
            assert t is None or (t.is_contiguous() and tuple(t.shape) == (4, Cc) and t.dtype == torch.float32)
        new_src, new_tgt = torch.empty_like(cur_src), torch.empty_like(cur_tgt)
        losses = torch.empty(2, dtype=torch.float32, device=cur_src.device)
        self._ck(self.lib.uda_proto_align_fwd(cur_src.data_ptr(), cur_tgt.data_ptr(), _ptr(prev_src), _ptr(prev_tgt),
                                              float(1 - decay), float(decay), Cc, new_src.data_ptr(), new_tgt.data_ptr(),
                                              losses.data_ptr(), self._stream()))
        return new_src, new_tgt, losses

    def proto_align_bwd(self, new_src, new_tgt, g, w_src, w_tgt):
        Cc = new_src.shape[1]
        assert g.numel() == 1 and g.dtype == torch.float32 and new_src.is_contiguous() and new_tgt.is_contiguous()
        d_src, d_tgt = torch.empty_like(new_src), torch.empty_like(new_tgt)
        self._ck(self.lib.uda_proto_align_bwd(new_src.data_ptr(), new_tgt.data_ptr(), g.data_ptr(), float(w_src), float(w_tgt), Cc,
                                              d_src.data_ptr(), d_tgt.data_ptr(), self._stream()))
        return d_src, d_tgt

    def adv_loss_fwd(self, d1, d2, label, scale):
        self._dev(d1)
        assert d1.is_contiguous() and d2.is_contiguous() and d1.dtype == d2.dtype == torch.float32
        loss = torch.empty(1, dtype=torch.float32, device=d1.device)
        self._ck(self.lib.uda_adv_loss_fwd(d1.data_ptr(), d1.numel(), d2.data_ptr(), d2.numel(), float(label), float(scale),
                                           loss.data_ptr(), self._stream()))
        return loss

    def adv_loss_bwd(self, d1, d2, label, scale, g):
        assert g.numel() == 1 and g.dtype == torch.float32
        g1, g2 = torch.empty_like(d1), torch.empty_like(d2)
        self._ck(self.lib.uda_adv_loss_bwd(d1.data_ptr(), d1.numel(), d2.data_ptr(), d2.numel(), float(label), float(scale),
                                           g.data_ptr(), g1.data_ptr(), g2.data_ptr(), self._stream()))
        return g1, g2

    def feat_dot4(self, feat, coef):
        """[P,4]: feat @ coef[:, :C].T + coef[:, C]"""
        f, ldf = _mat(feat, "feat")
        P, Cc = feat.shape
        assert coef.is_contiguous() and tuple(coef.shape) == (4, Cc + 1) and coef.dtype == torch.float32
        out = torch.empty(P, 4, dtype=torch.float32, device=feat.device)
        self._ck(self.lib.uda_feat_dot4(f, ldf, P, Cc, coef.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def feat_rank4(self, wts, coef, d_feat, accumulate=False):
        """d_feat (+)= wts @ coef[:, :C]"""
        d, ldd = _mat(d_feat, "d_feat")
        P, Cc = d_feat.shape
        assert wts.is_contiguous() and tuple(wts.shape) == (P, 4) and tuple(coef.shape) == (4, Cc + 1) and coef.is_contiguous()
        self._ck(self.lib.uda_feat_rank4(wts.data_ptr(), coef.data_ptr(), P, Cc, d, ldd, int(accumulate), self._stream()))

    # ------------------------------------------------------------------ optimiser
    # ------------------------------------------------------------------ input pipeline tail
    @staticmethod
    def gaussian_weights(sigma, radius):
        """The taps of scipy.ndimage.gaussian_filter1d, computed the way scipy computes them (numpy, float64), centre first."""
        import numpy as np
        x = np.arange(-radius, radius + 1)
        phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
        phi = phi / phi.sum()
        return phi[radius:].copy()

    def normalize_tf(self, image_u8, label_u8, sigma=3.0):
        """uint8 [B,H,W,3] + uint8 grey mask [B,H,W] -> (image f32 [B,3,H,W], map f32 [B,2,H,W], boundary f32 [B,1,H,W])."""
        for t in (image_u8, label_u8):
            self._dev(t)
            assert t.dtype == torch.uint8 and t.is_contiguous()
        B, H, W, ch = image_u8.shape
        assert ch == 3 and tuple(label_u8.shape) == (B, H, W)
        radius = int(4.0 * sigma + 0.5)
        wts = self.gaussian_weights(sigma, radius)
        dev = image_u8.device
        image = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
        mp = torch.empty(B, 2, H, W, dtype=torch.float32, device=dev)
        bd = torch.empty(B, 1, H, W, dtype=torch.float32, device=dev)
        ws = self._ws(image_u8, self.lib.uda_normalize_tf_workspace_bytes(B, H, W))
        self._ck(self.lib.uda_normalize_tf(image_u8.data_ptr(), label_u8.data_ptr(), B, H, W,
                                           wts.ctypes.data_as(C.POINTER(C.c_double)), radius, image.data_ptr(), mp.data_ptr(),
                                           bd.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return image, mp, bd

    def field_smooth(self, noise, sigma, alpha):
        """alpha * scipy.ndimage.gaussian_filter(noise, sigma, mode='constant') per [H,W] plane of a float64 [..., H, W] tensor,
        bit-identical to scipy (same taps, same summation order, no fused multiply-add)."""
        self._dev(noise)
        assert noise.dtype == torch.float64 and noise.is_contiguous()
        H, W = noise.shape[-2:]
        radius = int(4.0 * sigma + 0.5)
        wts = torch.from_numpy(self.gaussian_weights(sigma, radius)).to(noise.device)
        tmp, out = torch.empty_like(noise), torch.empty_like(noise)
        self._ck(self.lib.uda_field_smooth(noise.data_ptr(), noise.numel() // (H * W), H, W, wts.data_ptr(), radius, float(alpha),
                                           tmp.data_ptr(), out.data_ptr(), self._stream()))
        return out

    def elastic_warp(self, image_u8, label_u8, dx, dy, apply=None):
        for t in (image_u8, label_u8, dx, dy):
            self._dev(t)
            assert t.is_contiguous()
        B, H, W, ch = image_u8.shape
        assert ch == 3 and tuple(label_u8.shape) == (B, H, W) == tuple(dx.shape) == tuple(dy.shape)
        assert image_u8.dtype == label_u8.dtype == torch.uint8 and dx.dtype == dy.dtype == torch.float64
        if apply is not None:
            assert apply.dtype == torch.uint8 and apply.numel() == B and apply.is_cuda
        io, lo = torch.empty_like(image_u8), torch.empty_like(label_u8)
        self._ck(self.lib.uda_elastic_warp(image_u8.data_ptr(), label_u8.data_ptr(), dx.data_ptr(), dy.data_ptr(), _ptr(apply),
                                           B, H, W, io.data_ptr(), lo.data_ptr(), self._stream()))
        return io, lo

    def photometric_u8(self, image_u8, sp_pos, sp_count, sp_value, lut, erase_box):
        """salt-and-pepper scatter, gamma table and box erasing on a uint8 [B,H,W,3] batch, in place."""
        self._dev(image_u8)
        B, H, W, ch = image_u8.shape
        assert ch == 3 and image_u8.dtype == torch.uint8 and image_u8.is_contiguous()
        assert sp_pos.dtype == sp_count.dtype == sp_value.dtype == erase_box.dtype == torch.int32 and lut.dtype == torch.uint8
        assert sp_pos.dim() == 3 and sp_pos.shape[0] == B and sp_pos.shape[2] == 2 and sp_count.numel() == B == sp_value.numel()
        assert tuple(lut.shape) == (B, 256) and tuple(erase_box.shape) == (B, 5)
        for t in (sp_pos, sp_count, sp_value, lut, erase_box):
            assert t.is_cuda and t.is_contiguous()
        self._ck(self.lib.uda_photometric_u8(image_u8.data_ptr(), B, H, W, sp_pos.data_ptr(), sp_count.data_ptr(),
                                             sp_value.data_ptr(), sp_pos.shape[1], lut.data_ptr(), erase_box.data_ptr(),
                                             self._stream()))
        return image_u8

    def geometry_u8(self, image_pool, label_pool, offsets, sizes, src_index, records, S):
        """scale-crop, rotate and flip of a batch from the device-resident source pools and the recorded draws:
        -> (uint8 [B,S,S,3], uint8 [B,S,S])."""
        for t in (image_pool, label_pool):
            self._dev(t)
            assert t.dtype == torch.uint8 and t.is_contiguous()
        for t in (offsets, sizes, src_index, records):
            assert t.is_cuda and t.is_contiguous()
        n = offsets.numel()
        B = src_index.numel()
        assert offsets.dtype == src_index.dtype == torch.int64 and sizes.dtype == records.dtype == torch.int32
        assert tuple(sizes.shape) == (n, 2) and tuple(records.shape) == (B, 10)
        assert label_pool.numel() * 3 == image_pool.numel()
        io = torch.empty(B, S, S, 3, dtype=torch.uint8, device=image_pool.device)
        lo = torch.empty(B, S, S, dtype=torch.uint8, device=image_pool.device)
        ws = self._ws(image_pool, self.lib.uda_geometry_u8_workspace_bytes(B, S))
        self._ck(self.lib.uda_geometry_u8(image_pool.data_ptr(), label_pool.data_ptr(), offsets.data_ptr(), sizes.data_ptr(), n,
                                          src_index.data_ptr(), records.data_ptr(), B, S, io.data_ptr(), lo.data_ptr(),
                                          ws.data_ptr(), ws.numel(), self._stream()))
        return io, lo

    # ------------------------------------------------------------------ Fourier style transfer (csrc/fda.hip)
    def _ck_fda(self, who, band, *batches):
        """contiguous uint8 [N,H,W,3] device batches of one size and a band the library takes -> (H, W, band)"""
        for t in batches:
            self._dev(t)
            if t.dtype != torch.uint8 or not t.is_contiguous() or t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1:
                raise ValueError("%s: contiguous uint8 [N, H, W, 3] batches (got %s %s)" % (who, t.dtype, tuple(t.shape)))
        H, W = batches[0].shape[1:3]
        if any(tuple(t.shape[1:3]) != (H, W) for t in batches):
            raise ValueError("%s: source and target sizes differ: %s" % (who, [tuple(t.shape) for t in batches]))
        band = int(band)
        if not 0 <= band <= FDA_MAX_BAND or 2 * band + 2 > min(H, W):
            raise ValueError("%s: band %d outside 0..%d or 2 band + 2 > min(H, W) of batches %s"
                             % (who, band, FDA_MAX_BAND, [tuple(t.shape) for t in batches]))
        return H, W, band

    def fda_spectrum(self, image_u8, band, out=None):
        """uint8 [N,H,W,3] -> float64 [N,3,2 band + 1,band + 1,2]: (re, im) of the DFT coefficients F[n,c,u,v], u = -band..band, v = 0..band
        (include/uda_clr_hip.h, uda_fda_spectrum)."""
        H, W, band = self._ck_fda("fda_spectrum", band, image_u8)
        N = image_u8.shape[0]
        shape = (N, 3, 2 * band + 1, band + 1, 2)
        if out is None:
            out = torch.empty(shape, dtype=torch.float64, device=image_u8.device)
        elif out.dtype != torch.float64 or tuple(out.shape) != shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("fda_spectrum: out must be contiguous float64 %s on the device (got %s %s)" % (shape, out.dtype, tuple(out.shape)))
        ws = self._ws(image_u8, self.lib.uda_fda_workspace_bytes(N, 0, H, W, band))
        self._ck(self.lib.uda_fda_spectrum(image_u8.data_ptr(), N, H, W, band, out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    def fda_transfer(self, src_u8, tgt_u8, pair, band, apply=None, out=None):
        """source uint8 [B,H,W,3] with the low-frequency amplitudes (band) of target uint8 [Bt,H,W,3] image pair[b] (int32 [B], device),
        where apply[b] (uint8 [B], device; None = all) is set -> uint8 [B,H,W,3] (include/uda_clr_hip.h, uda_fda_transfer)."""
        H, W, band = self._ck_fda("fda_transfer", band, src_u8, tgt_u8)
        B, Bt = src_u8.shape[0], tgt_u8.shape[0]
        if not pair.is_cuda or pair.dtype != torch.int32 or not pair.is_contiguous() or tuple(pair.shape) != (B,):
            raise ValueError("fda_transfer: pair must be contiguous int32 [%d] on the device (got %s %s)" % (B, pair.dtype, tuple(pair.shape)))
        if apply is not None and (not apply.is_cuda or apply.dtype != torch.uint8 or not apply.is_contiguous() or tuple(apply.shape) != (B,)):
            raise ValueError("fda_transfer: apply must be contiguous uint8 [%d] on the device (got %s %s)" % (B, apply.dtype, tuple(apply.shape)))
        if out is None:
            out = torch.empty_like(src_u8)
        elif out.dtype != torch.uint8 or out.shape != src_u8.shape or not out.is_contiguous() or not out.is_cuda:
            raise ValueError("fda_transfer: out must be contiguous uint8 %s on the device (got %s %s)" % (tuple(src_u8.shape), out.dtype, tuple(out.shape)))
        ws = self._ws(src_u8, self.lib.uda_fda_workspace_bytes(B, Bt, H, W, band))
        self._ck(self.lib.uda_fda_transfer(src_u8.data_ptr(), B, H, W, tgt_u8.data_ptr(), Bt, H, W, pair.data_ptr(), _ptr(apply), band,
                                           out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()))
        return out

    # ------------------------------------------------------------------ whole photographs (csrc/wholephoto.hip)
    @staticmethod
    def _ck_photos(pool, offsets, sizes, src_index, S):
        """the pool tables of uda_photo_reduce_u8 / uda_roi_cut_u8 -> (n_sources, B)"""
        if not pool.is_cuda or pool.dtype != torch.uint8 or not pool.is_contiguous() or pool.dim() != 1 or pool.numel() % 3:
            raise ValueError("a photograph pool is a flat contiguous uint8 device tensor of [H,W,3] images (got %s %s)" % (pool.dtype, tuple(pool.shape)))
        for t in (offsets, sizes, src_index):
            if not t.is_cuda or not t.is_contiguous():
                raise UdaError("HIP kernels need contiguous device tensors; there is no CPU fallback")
        n, B = offsets.numel(), src_index.numel()
        if offsets.dtype != torch.int64 or src_index.dtype != torch.int64 or sizes.dtype != torch.int32 or tuple(sizes.shape) != (n, 2):
            raise ValueError("offsets int64 [n], sizes int32 [n, 2], src_index int64 [B]")
        check_side("size", S)
        if not 1 <= B <= 8192:
            raise ValueError("batch of %d photographs outside 1..8192" % B)
        return n, B

    def photo_reduce(self, pool, offsets, sizes, src_index, S, outputs=("f32",)):
        """the coarse S x S canvas of every selected photograph (uda_photo_reduce_u8) -> {'u8': uint8 [B,S,S,3], 'f32': f32 [B,3,S,S]}
        for the names in ``outputs``, and 'factor': int32 [B]"""
        n, B = self._ck_photos(pool, offsets, sizes, src_index, S)
        out = self._u8_f32(outputs, B, S, pool.device)
        factor = torch.empty(B, dtype=torch.int32, device=pool.device)
        self._ck(self.lib.uda_photo_reduce_u8(pool.data_ptr(), pool.numel() // 3, offsets.data_ptr(), sizes.data_ptr(), n, src_index.data_ptr(),
                                              B, S, _ptr(out.get("u8")), _ptr(out.get("f32")), factor.data_ptr(), self._stream()))
        return dict(factor=factor, **out)

    def roi_cut(self, pool, offsets, sizes, src_index, boxes, S, outputs=("u8", "f32")):
        """Pillow's crop(box).resize((S, S), BILINEAR) of every selected photograph (uda_roi_cut_u8); boxes int32 [B,3] = (x0, y0, R) on
        the device -> {'u8': uint8 [B,S,S,3], 'f32': f32 [B,3,S,S]} for the names in ``outputs``"""
        n, B = self._ck_photos(pool, offsets, sizes, src_index, S)
        out = self._u8_f32(outputs, B, S, pool.device)
        if not boxes.is_cuda or boxes.dtype != torch.int32 or not boxes.is_contiguous() or tuple(boxes.shape) != (B, 3):
            raise ValueError("boxes: contiguous int32 [%d, 3] on the device (got %s %s)" % (B, boxes.dtype, tuple(boxes.shape)))
        self._ck(self.lib.uda_roi_cut_u8(pool.data_ptr(), pool.numel() // 3, offsets.data_ptr(), sizes.data_ptr(), n, src_index.data_ptr(),
                                         boxes.data_ptr(), B, S, _ptr(out.get("u8")), _ptr(out.get("f32")), self._stream()))
        return out

    def roi_paste(self, masks_u8, boxes, sizes, out_offsets, out_bytes):
        """uint8 [B,2,S,S] masks, boxes int32 [B,3], sizes int32 [B,2] = (H, W), out_offsets int64 [B], all on the device -> one flat
        uint8 [out_bytes] buffer holding every photograph's [H,W] grey mask (0 cup, 128 disc only, 255 background; uda_roi_paste_u8).
        The buffer is not pre-filled: the offsets must tile it, as ``ops.roi_paste`` lays them out."""
        B, S, W = self._ck_masks("roi_paste", masks_u8)
        if S != W:
            raise ValueError("roi_paste: square [B, 2, S, S] masks (got %s)" % (tuple(masks_u8.shape),))
        for t, dt, shape in ((boxes, torch.int32, (B, 3)), (sizes, torch.int32, (B, 2)), (out_offsets, torch.int64, (B,))):
            if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != shape:
                raise ValueError("roi_paste: contiguous %s %s on the device (got %s %s)" % (dt, list(shape), t.dtype, tuple(t.shape)))
        check_side("size", S)
        out = torch.empty(int(out_bytes), dtype=torch.uint8, device=masks_u8.device)
        self._ck(self.lib.uda_roi_paste_u8(masks_u8.data_ptr(), boxes.data_ptr(), sizes.data_ptr(), out_offsets.data_ptr(), B, S, out.data_ptr(),
                                           out.numel(), self._stream()))
        return out

    def postprocess(self, pred, thr_cup, thr_disc, sweeps=None):
        """pred f32 [B,2,H,W] probabilities -> uint8 [B,2,H,W] masks after the reference's evaluation post-processing.
        Runs the tile-wise propagations for ``sweeps`` launches and repeats with twice as many, up to six attempts, while the
        device reports unfinished tiles; then raises.  A launch carries a label from one 32 x 32 tile into the next, so the
        default, 2 * (tile rows + tile columns) + 4, is enough when the path inside a component to its first pixel (and inside
        the background to the image border) crosses each line between two tile rows or tile columns at most twice: any convex
        blob, a ring.  A spiral wall of three turns on 256 x 256 needs 50 launches against 36 and takes the second attempt."""
        self._dev(pred)
        assert pred.dtype == torch.float32 and pred.is_contiguous() and pred.dim() == 4 and pred.shape[1] == 2
        return self._propagate("uda_postprocess", 2, pred, (float(thr_cup), float(thr_disc)), sweeps)

    def display_masks(self, prob, threshold=0.75, sweeps=None):
        """prob f32 [B,2,H,W] probabilities (left unchanged) -> uint8 [B,2,H,W] display masks of the reference's ``save_per_img``
        (include/uda_clr_hip.h, uda_display_masks).  Sweeps, doubling and the six attempts as ``postprocess``; the device reports
        three propagations here (components, first flood, second flood)."""
        self._dev(prob)
        if prob.dtype != torch.float32 or not prob.is_contiguous() or prob.dim() != 4 or prob.shape[1] != 2:
            raise ValueError("display_masks: contiguous float32 [B, 2, H, W] probabilities (got %s %s)" % (prob.dtype, tuple(prob.shape)))
        return self._propagate("uda_display_masks", 3, prob, (float(threshold),), sweeps)

    def overlay_u8(self, image_u8, masks_u8, out=None):
        """image uint8 [B,H,W,3], masks uint8 [B,2,H,W] (nonzero = set) -> uint8 [B,H,W,3]: channel 1's outline in (0, 255, 0),
        channel 0's in (0, 0, 255) over it, the image elsewhere (include/uda_clr_hip.h, uda_overlay_u8).  ``out`` may not alias
        the image."""
        for t in (image_u8, masks_u8):
            self._dev(t)
            if t.dtype != torch.uint8 or not t.is_contiguous() or t.dim() != 4:
                raise ValueError("overlay_u8: contiguous uint8 tensors (got %s %s)" % (t.dtype, tuple(t.shape)))
        B, H, W, ch = image_u8.shape
        if ch != 3 or tuple(masks_u8.shape) != (B, 2, H, W):
            raise ValueError("overlay_u8: image [B, H, W, 3] and masks [B, 2, H, W] (got %s and %s)" % (tuple(image_u8.shape), tuple(masks_u8.shape)))
        if out is None:
            out = torch.empty_like(image_u8)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or out.shape != image_u8.shape or not out.is_cuda:
            raise ValueError("overlay_u8: out must be a contiguous uint8 device tensor of the image's shape")
        self._ck(self.lib.uda_overlay_u8(image_u8.data_ptr(), masks_u8.data_ptr(), B, H, W, out.data_ptr(), self._stream()))
        return out

    def image_u8(self, x, out=None):
        """f32 [B,3,H,W] in [-1, 1] -> uint8 [B,H,W,3] = clip(rint((x + 1) * 127.5), 0, 255) (uda_image_u8)."""
        self._dev(x)
        if x.dtype != torch.float32 or not x.is_contiguous() or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError("image_u8: contiguous float32 [B, 3, H, W] (got %s %s)" % (x.dtype, tuple(x.shape)))
        B, _, H, W = x.shape
        if out is None:
            out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=x.device)
        elif out.dtype != torch.uint8 or not out.is_contiguous() or tuple(out.shape) != (B, H, W, 3) or not out.is_cuda:
            raise ValueError("image_u8: out must be a contiguous uint8 [B, H, W, 3] device tensor")
        self._ck(self.lib.uda_image_u8(x.data_ptr(), B, H, W, out.data_ptr(), self._stream()))
        return out

    def surface_distance(self, pred_u8, gt_u8, want_d2=False, want_packed=False):
        """uint8 [B,2,H,W] masks (nonzero = set) -> (table f64 [B,2,2,3], counts i64 [B,2,3][, d2 i32 [B,2,2,H,W]]) on the
        device: per image and class the directed entries (n, sum of distances, max squared distance) pred -> gt and gt -> pred
        between the masks' borders, and the Dice counts (include/uda_clr_hip.h, uda_surface_distance).  Table and counts are views of
        one buffer of 8-byte words (``surface_layout``), handed back as the last value with ``want_packed`` (one copy moves both)."""
        B, H, W = self._ck_masks("surface_distance", pred_u8, gt_u8)
        packed, v = packed_views(surface_layout(B), pred_u8.device)
        d2 = torch.empty(B, 2, 2, H, W, dtype=torch.int32, device=pred_u8.device) if want_d2 else None
        ws = self._ws(pred_u8, self.lib.uda_surface_distance_workspace_bytes(B, H, W))
        self._ck(self.lib.uda_surface_distance(pred_u8.data_ptr(), gt_u8.data_ptr(), B, H, W, v["table"].data_ptr(), v["counts"].data_ptr(),
                                               _ptr(d2), ws.data_ptr(), ws.numel(), self._stream()))
        return (v["table"], v["counts"]) + ((d2,) if want_d2 else ()) + ((packed,) if want_packed else ())

    def surface_profile(self, pred_u8, gt_u8, quantiles, tol2, want_packed=False):
        """uint8 [B,2,H,W] masks -> (table f64 [B,2,2,3], counts i64 [B,2,3], order i64 [B,2,3,Q,2], within i64 [B,2,2,T],
        extent i64 [B,2,2,2]) on the device (include/uda_clr_hip.h, uda_surface_profile): table and counts as
        ``surface_distance``; per set (pred -> gt, gt -> pred, both pooled) and quantile the two squared distances a percentile
        interpolates between; per direction the border pixels within each squared tolerance; per mask its first and last row.
        The five are views of one buffer of 8-byte words, handed back as a sixth value with ``want_packed`` (one copy moves all)."""
        B, H, W = self._ck_masks("surface_profile", pred_u8, gt_u8)
        q = [float(v) for v in quantiles]
        t2 = [int(v) for v in tol2]
        if any(not 0.0 <= v <= 1.0 for v in q):                   # also true for NaN
            raise ValueError("surface_profile: quantiles must lie in [0, 1], got %r" % (q,))
        if any(v < 0 or v > 2 ** 31 - 1 for v in t2):
            raise ValueError("surface_profile: squared tolerances must lie in 0..2^31-1, got %r" % (t2,))
        Q, T = len(q), len(t2)
        packed, v = packed_views(profile_layout(B, Q, T), pred_u8.device)
        cq, ct = (C.c_double * max(Q, 1))(*q), (C.c_int32 * max(T, 1))(*t2)
        ws = self._ws(pred_u8, self.lib.uda_surface_profile_workspace_bytes(B, H, W))
        self._ck(self.lib.uda_surface_profile(pred_u8.data_ptr(), gt_u8.data_ptr(), B, H, W, C.addressof(cq), Q, C.addressof(ct), T,
                                              *[t.data_ptr() for t in v.values()], None, ws.data_ptr(), ws.numel(), self._stream()))
        return tuple(v.values()) + ((packed,) if want_packed else ())

    def disc_morphometry(self, masks_u8, sectors, want_packed=False):
        """uint8 [B,2,H,W] masks (0 cup, 1 disc; nonzero = set), sectors int64 [K,2] on the device (``utils.metrics.sector_table``)
        -> (moments i64 [B,2,6], extent i64 [B,2,4], overlap i64 [B], radial i64 [B,2,K]) on the device (include/uda_clr_hip.h,
        uda_disc_morphometry): per class n, sum r, sum c, sum r^2, sum c^2, sum r*c; first and last row and column; the pixels set
        in both planes; per sector about the disc centroid the largest squared distance scaled by n_disc^2, -1 for an empty sector.
        The four are views of one int64 buffer, handed back as a fifth value with ``want_packed`` (one copy moves all)."""
        B, H, W = self._ck_masks("disc_morphometry", masks_u8)
        if not sectors.is_cuda:
            raise UdaError("HIP kernels need device tensors (got %s); there is no CPU fallback" % sectors.device)
        if sectors.dtype != torch.int64 or not sectors.is_contiguous() or sectors.dim() != 2 or sectors.shape[1] != 2:
            raise ValueError("disc_morphometry: contiguous int64 [K, 2] sector table (got %s %s)" % (sectors.dtype, tuple(sectors.shape)))
        K = sectors.shape[0]
        if K % 8 or not 8 <= K <= 360:
            raise ValueError("disc_morphometry: the number of sectors must be a multiple of 8 in 8..360, got %d" % K)
        packed, v = packed_views(morphometry_layout(B, K), masks_u8.device)
        ws = self._ws(masks_u8, self.lib.uda_disc_morphometry_workspace_bytes(B, H, W, K))
        self._ck(self.lib.uda_disc_morphometry(masks_u8.data_ptr(), B, H, W, sectors.data_ptr(), K, *[t.data_ptr() for t in v.values()],
                                               ws.data_ptr(), ws.numel(), self._stream()))
        return tuple(v.values()) + ((packed,) if want_packed else ())

    def mc_uncertainty(self, logits, outputs=("mean", "std", "entropy", "mi"), u8_scale=None):
        """f32 [T, ...] logits of T stochastic passes (2 <= T <= 32) -> {name: map of shape logits.shape[1:]} on the device, one read of
        the logits (include/uda_clr_hip.h, uda_mc_uncertainty): 'mean' of sigmoid(x), 'std' = unbiased std of sigmoid(x / 2) (the
        trainer's quantity), 'entropy' of the mean, 'mi' = entropy minus the mean entropy of the passes; with ``u8_scale`` also
        'std_u8' = min(255, floor(std * u8_scale)) as uint8.  Only the maps named are computed and written."""
        self._dev(logits)
        if logits.dtype != torch.float32 or not logits.is_contiguous() or logits.dim() < 2:
            raise ValueError("mc_uncertainty: contiguous float32 [T, ...] logits (got %s %s)" % (logits.dtype, tuple(logits.shape)))
        out = self._named_maps("mc_uncertainty", outputs, u8_scale, tuple(logits.shape[1:]), logits.device)
        self._ck(self.lib.uda_mc_uncertainty(logits.data_ptr(), logits.shape[0], logits[0].numel(), _ptr(out.get("mean")), _ptr(out.get("std")),
                                             _ptr(out.get("entropy")), _ptr(out.get("mi")), _ptr(out.get("std_u8")),
                                             0.0 if u8_scale is None else float(u8_scale), self._stream()))
        return out

    def selective_tables(self, prob, unc, pred_u8, gt_u8=None, bins=15, edges=(), want_packed=False):
        """prob, unc f32 [B,2,H,W] (either None), pred, gt uint8 [B,2,H,W] (nonzero = set; gt None = pred), ``bins`` confidence bins,
        ``edges`` K - 1 ascending host floats -> (rel i64 [B,2,bins,5] or None, risk i64 [B,2,K,4] or None, invalid i64 [B,2,2]) on the
        device (include/uda_clr_hip.h, uda_selective_tables).  The three are views of one int64 buffer, handed back as a fourth value
        with ``want_packed`` (one copy moves all)."""
        B, H, W = self._ck_masks("selective_tables", pred_u8, *(() if gt_u8 is None else (gt_u8,)))
        for t in (prob, unc):
            if t is not None:
                self._dev(t)
                if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != pred_u8.shape:
                    raise ValueError("selective_tables: contiguous float32 maps of the masks' shape (got %s %s)" % (t.dtype, tuple(t.shape)))
        if prob is None and unc is None:
            raise ValueError("selective_tables: prob (reliability table), unc (risk table) or both")
        edges = [float(e) for e in edges]
        M, K = int(bins), len(edges) + 1
        if not 1 <= M <= 64 or not K <= 64:
            raise ValueError("selective_tables: 1..64 bins (got %d confidence, %d uncertainty)" % (M, K))
        packed, v = packed_views(selective_layout(B, M, K, prob is not None, unc is not None), pred_u8.device)
        self._ck(self.lib.uda_selective_tables(_ptr(prob), _ptr(unc), pred_u8.data_ptr(), _ptr(gt_u8), B, H, W, M,
                                               (C.c_float * max(len(edges), 1))(*edges), K, _ptr(v.get("rel")), _ptr(v.get("risk")),
                                               v["invalid"].data_ptr(), self._stream()))
        return (v.get("rel"), v.get("risk"), v["invalid"]) + ((packed,) if want_packed else ())

    @staticmethod
    def _ck_tta_view(who, v, view):
        """a view (g, h, w) as include/uda_clr_hip.h defines it -> (g, h, w) as ints"""
        try:
            g, h, w = (int(a) for a in view)
        except (TypeError, ValueError):
            raise ValueError("%s: view %d must be (g, h, w), got %r" % (who, v, view)) from None
        if not 0 <= g <= 7:
            raise ValueError("%s: view %d: code %d outside 0..7" % (who, v, g))
        check_side("%s: view %d: size" % (who, v), h, w)
        return g, h, w

    @staticmethod
    def _ck_tta_frame(who, B, Cc, H, W):
        if not 1 <= B <= 8192:
            raise ValueError("%s: batch %d outside 1..8192" % (who, B))
        if not 1 <= Cc <= 4:
            raise ValueError("%s: %d channels outside 1..4" % (who, Cc))
        check_side("%s: frame" % who, H, W)

    def tta_view(self, image, view):
        """f32 [B,C,H,W] image, view (g, h, w) -> the view's input f32 [B,C,h,w] ([B,C,w,h] for a transposed code g & 4) on the device
        (include/uda_clr_hip.h, uda_tta_view): resampled to (h, w) with align_corners=True, mirrored, transposed; a view of the
        image's own size is a permutation of its values."""
        self._dev(image)
        if image.dtype != torch.float32 or not image.is_contiguous() or image.dim() != 4:
            raise ValueError("tta_view: contiguous float32 [B, C, H, W] image (got %s %s)" % (image.dtype, tuple(image.shape)))
        g, h, w = self._ck_tta_view("tta_view", 0, view)
        B, Cc, H, W = image.shape
        self._ck_tta_frame("tta_view", B, Cc, H, W)
        out = torch.empty((B, Cc, w, h) if g & 4 else (B, Cc, h, w), dtype=torch.float32, device=image.device)
        self._ck(self.lib.uda_tta_view(image.data_ptr(), B, Cc, H, W, g, h, w, out.data_ptr(), self._stream()))
        return out

    def tta_fuse(self, view_logits, views, size, outputs=("mean",), u8_scale=None):
        """V f32 [B,C,h_v',w_v'] logit tensors of the views (g, h, w) of an H x W frame, ``size`` = (H, W) -> {name: [B,C,H,W] map} on
        the device, one read of the logits (include/uda_clr_hip.h, uda_tta_fuse): every view mapped back to the frame, then the maps
        of ``mc_uncertainty`` over the views: 'mean', 'std', 'entropy', 'mi' and with ``u8_scale`` 'std_u8'."""
        view_logits, views = list(view_logits), list(views)
        V = len(views)
        if not 2 <= V <= 32:
            raise ValueError("tta_fuse: %d views outside 2..32" % V)
        if len(view_logits) != V:
            raise ValueError("tta_fuse: %d logit tensors for %d views" % (len(view_logits), V))
        try:
            H, W = (int(a) for a in size)
        except (TypeError, ValueError):
            raise ValueError("tta_fuse: size must be (H, W), got %r" % (size,)) from None
        views = [self._ck_tta_view("tta_fuse", v, view) for v, view in enumerate(views)]
        if view_logits[0] is None or view_logits[0].dim() != 4:
            raise ValueError("tta_fuse: view 0: contiguous float32 [B, C, h, w] logits (got %r)" %
                             (None if view_logits[0] is None else tuple(view_logits[0].shape),))
        B, Cc = view_logits[0].shape[:2]
        self._ck_tta_frame("tta_fuse", B, Cc, H, W)
        for v, (t, (g, h, w)) in enumerate(zip(view_logits, views)):
            if t is None:
                raise ValueError("tta_fuse: view %d: no logits (None)" % v)
            self._dev(t)
            want = (B, Cc, w, h) if g & 4 else (B, Cc, h, w)
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != want or t.data_ptr() % 16:
                raise ValueError("tta_fuse: view %d (g %d, %d x %d): contiguous 16-byte aligned float32 logits of shape %s (got %s %s)"
                                 % (v, g, h, w, want, t.dtype, tuple(t.shape)))
        out = self._named_maps("tta_fuse", outputs, u8_scale, (B, Cc, H, W), view_logits[0].device)
        ints = lambda k: (C.c_int * V)(*[view[k] for view in views])
        self._ck(self.lib.uda_tta_fuse((C.c_void_p * V)(*[t.data_ptr() for t in view_logits]), ints(0), ints(1), ints(2), V, B, Cc, H, W,
                                       _ptr(out.get("mean")), _ptr(out.get("std")), _ptr(out.get("entropy")), _ptr(out.get("mi")),
                                       _ptr(out.get("std_u8")), 0.0 if u8_scale is None else float(u8_scale), self._stream()))
        return out

    def adam_step(self, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
        for t in (params, grads, exp_avg, exp_avg_sq):
            self._dev(t)
            assert t.is_contiguous() and t.dtype == torch.float32 and t.numel() == params.numel()
        self._ck(self.lib.uda_adam_step(params.data_ptr(), grads.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                        params.numel(), lr, beta1, beta2, eps, int(step), self._stream()))
