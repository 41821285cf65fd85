"""not-gpu: the view grammar of uda_clr_amd.tta, the argument errors of evaluate / predict, the grouping of tta_logits (with a stub model
and tests/tta_ref.py standing in for ops.tta_view), the restatements of tests/tta_ref.py themselves, and the declarations of the two
C entries."""
import os
import re

import numpy as np
import pytest
import torch

import tta_ref
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict, tta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 48, 80


# ------------------------------------------------------------------------------------------------------------------ the grammar
def test_names_and_shorthands():
    assert tta.parse_views("id,hflip,vflip,rot180,transpose,rot90,rot270,antitranspose", H, W) == [(g, H, W) for g in range(8)]
    assert tta.parse_views("d4", H, W) == [(g, H, W) for g in range(8)]
    assert tta.parse_views("flips", H, W) == [(g, H, W) for g in range(4)]
    assert tta.parse_views(" rot90 , id ", H, W) == [(5, H, W), (0, H, W)]                       # the order given is the order kept
    assert tta.parse_views("flips,id@0.75,id@1.25", 512, 512) == [(g, 512, 512) for g in range(4)] + [(0, 384, 384), (0, 640, 640)]
    assert tta.parse_views("flips@0.5,rot90", 64, 96) == [(g, 32, 48) for g in range(4)] + [(5, 64, 96)]
    assert tta.CODES == tta_ref.CODES and tta.NAMES[5] == "rot90"


@pytest.mark.parametrize("n,s,want", [(48, 0.75, 32), (80, 0.75, 64), (48, 1.25, 64), (80, 1.25, 96), (48, 1.0, 48), (48, 0.1, 16), (48, 0.5, 32),
                                      (80, 0.5, 48), (512, 0.99, 512), (512, 1.016, 528), (512, 1.015, 512)])
def test_size_rounding(n, s, want):
    """16 * max(1, floor(n * s / 16 + 0.5)): 48 * 0.5 / 16 = 1.5 rounds up, 48 * 0.75 / 16 = 2.25 down"""
    assert tta.scaled_size(n, s) == want
    assert tta.parse_views("id,hflip@%r" % s, n, n)[1] == (1, want, want)


def test_scaled_sizes_of_the_small_frame():
    assert tta.parse_views("id,id@0.75,transpose@1.25", H, W) == [(0, 48, 80), (0, 32, 64), (4, 64, 96)]


@pytest.mark.parametrize("spec,match", [("id,id", "twice"), ("id,hflip,id@1.0", "twice"), ("id@0.99,id@1.01", "twice"), ("flips,hflip", "twice"),
                                        ("id", "1 views outside 2..32"), ("d4,d4@0.5,d4@0.75,d4@1.25,id@1.5", "33 views outside 2..32"),
                                        ("id,mirror", "unknown view 'mirror'"), ("id,hflip@big", "scale 'big'"), ("id,hflip@-1", "scale -1.0"),
                                        ("id,hflip@0", "scale 0.0"), ("id,hflip@40", "1024"), ("", "view list"), ("id,,hflip", "unknown view ''")])
def test_grammar_errors(spec, match):
    with pytest.raises(ValueError, match=re.escape(match)):
        tta.parse_views(spec, H, W)


def test_view_lists_and_frames_are_checked():
    assert tta.normalise_views([(0, 48, 80), [4, 32, 64]], H, W) == [(0, 48, 80), (4, 32, 64)]
    assert tta.normalise_views("flips", H, W) == [(g, H, W) for g in range(4)]
    for views, match in (([(0, 48, 80)], "1 views"), ([(0, 48, 80), (8, 48, 80)], "code 8"), ([(0, 48, 80), (1, 40, 80)], "40"),
                         ([(0, 48, 80), (1, 48, 1040)], "1040"), ([(0, 48, 80), (0, 48, 80)], "twice"), ([(0, 48, 80), (1, 48)], "(g, h, w)"),
                         ([(g % 8, 16 * (1 + g // 8), 16) for g in range(33)], "33 views")):
        with pytest.raises(ValueError, match=re.escape(match)):
            tta.normalise_views(views, H, W)
    with pytest.raises(ValueError, match="image height 50"):
        tta.parse_views("flips", 50, 80)
    assert len(tta.normalise_views([(g % 8, 16 * (1 + g // 8), 16) for g in range(32)], H, W)) == 32


# ------------------------------------------------------------------------------------------------------------ argument errors
def test_evaluate_and_predict_argument_errors():
    model = lambda x: x[:, :2]
    with pytest.raises(ValueError, match="tta_uncertainty=True and mc_passes=4"):
        ev.evaluate(model, [], tta="flips", tta_uncertainty=True, mc_passes=4, mc_logits=lambda x, t: None)
    with pytest.raises(ValueError, match="tta_uncertainty=True needs tta"):
        ev.evaluate(model, [], tta_uncertainty=True)
    with pytest.raises(ValueError, match="code 9"):
        ev.evaluate(model, [], tta=[(0, 64, 64), (9, 64, 64)])
    with pytest.raises(ValueError, match="tta_uncertainty=True and mc_passes=4"):
        predict.predict(model, [], "unused", tta="flips", tta_uncertainty=True, mc_passes=4)
    with pytest.raises(ValueError, match="tta_uncertainty=True needs tta"):
        predict.predict(model, [], "unused", tta_uncertainty=True)
    names = ev.extra_fields(calibration=True, tta_uncertainty=True)
    assert names == ev.extra_fields(calibration=True, mc_passes=8) == ev.CALIBRATION_FIELDS + ev.uncertainty_fields()
    assert ev.extra_fields() == ()
    for parser in (ev.build_parser(), predict.build_parser()):
        base = ["--data-dir", "d", "--checkpoint", "c"] if parser.prog.endswith("evaluate") else ["--images", "d", "--out", "o"]
        a = parser.parse_args(base)
        assert a.tta is None and a.tta_uncertainty is False
        a = parser.parse_args(base + ["--tta", "flips,id@0.75", "--tta-uncertainty"])
        assert a.tta == "flips,id@0.75" and a.tta_uncertainty is True


def test_ops_refuse_what_the_entries_refuse():
    """every ValueError is raised on the host before a device is touched, and names the offending value"""
    from uda_clr_amd.kernels import HipKernels
    for view, match in (((8, 48, 80), "code 8"), ((0, 40, 80), "40 x 80"), ((0, 48, 2048), "48 x 2048"), ((0, 48), "(g, h, w)")):
        with pytest.raises(ValueError, match=re.escape(match)):
            HipKernels._ck_tta_view("tta_view", 0, view)
    for args, match in (((0, 2, 48, 80), "batch 0"), ((8193, 2, 48, 80), "batch 8193"), ((2, 5, 48, 80), "5 channels"), ((2, 0, 48, 80), "0 channels"),
                        ((2, 2, 40, 80), "40 x 80"), ((2, 2, 48, 1040), "48 x 1040")):
        with pytest.raises(ValueError, match=re.escape(match)):
            HipKernels._ck_tta_frame("tta_fuse", *args)
    with pytest.raises(ValueError, match="u8_scale"):
        ops.tta_fuse([None, None], [(0, 48, 80), (1, 48, 80)], (48, 80), u8_scale=0.0)
    with pytest.raises(ValueError, match="u8_scale"):
        ops.tta_fuse([None, None], [(0, 48, 80), (1, 48, 80)], (48, 80), u8_scale=float("inf"))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        ops.tta_view(torch.zeros(3, 48, 80), (0, 48, 80))


# -------------------------------------------------------------------------------------------------------- grouping of tta_logits
class _Stub(object):
    """a pointwise 3 -> 2 model that records the shape of every call"""
    def __init__(self):
        self.shapes = []

    def __call__(self, x):
        self.shapes.append(tuple(x.shape))
        return torch.stack([x[:, 0] - 0.5 * x[:, 2], x[:, 1] + 0.25 * x[:, 0]], 1), None


def test_tta_logits_groups_views_by_tensor_shape(monkeypatch):
    host = tta_ref.HostTta()
    monkeypatch.setattr(ops, "tta_view", host.tta_view)
    image = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(0))
    views = tta.parse_views("d4,id@0.75,rot90@0.75,hflip@0.75", H, W)
    model = _Stub()
    logits = tta.tta_logits(model, image, views)
    # four shapes in the order of their first view: [48][80] (id hflip vflip rot180), [80][48] (the transposed four), [32][64], [64][32]
    assert model.shapes == [(8, 3, 48, 80), (8, 3, 80, 48), (4, 3, 32, 64), (2, 3, 64, 32)]
    assert [tuple(t.shape) for t in logits] == [(2, 2) + tta_ref.view_shape(v) for v in views]
    assert [c[1] for c in host.view_calls] == [views[i] for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 9)]
    for t, v in zip(logits, views):
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        assert torch.equal(t, model(tta_ref.view(image, v))[0])                                  # each view's own logits, in the order of views
    assert logits[1].data_ptr() == logits[0].data_ptr() + logits[0].numel() * 4               # slices of one output, not copies
    # the cap: 2 images per view, at most 5 images per forward -> 2 views per forward; a cap below B still runs one view at a time
    model = _Stub()
    tta.tta_logits(model, image, views, max_batch=5)
    assert model.shapes == [(4, 3, 48, 80)] * 2 + [(4, 3, 80, 48)] * 2 + [(4, 3, 32, 64), (2, 3, 64, 32)]
    model = _Stub()
    tta.tta_logits(model, image, views[:3], max_batch=1)
    assert model.shapes == [(2, 3, 48, 80)] * 3


def test_tta_predict_hands_the_views_to_the_fuse(monkeypatch):
    host = tta_ref.HostTta()
    monkeypatch.setattr(ops, "tta_view", host.tta_view)
    monkeypatch.setattr(ops, "tta_fuse", host.tta_fuse)
    image = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(1))
    out = tta.tta_predict(_Stub(), image, "d4", outputs=("mean", "std"), u8_scale=1600.0)
    shapes, views, size, outputs, scale = host.fuse_calls[0]
    assert views == [(g, H, W) for g in range(8)] and size == (H, W) and outputs == ("mean", "std") and scale == 1600.0
    assert shapes == [(2, 2, H, W)] * 4 + [(2, 2, W, H)] * 4
    plain = _Stub()(image)[0]
    assert float(out["std"].abs().max()) < 1e-15 and not out["std_u8"].any()                   # a pointwise model: every view agrees (float64 stand-in)
    assert float((out["mean"] - torch.sigmoid(plain)).abs().max()) < 1e-6


# ------------------------------------------------------------------------------------------------------------ the restatements
@pytest.mark.parametrize("g", range(8))
def test_every_code_is_the_formula_and_its_inverse_undoes_it(g):
    R = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(g), dtype=torch.float64)
    U = tta_ref.permute(R, g)
    assert tuple(U.shape[-2:]) == tta_ref.view_shape((g, H, W))
    i, j = np.meshgrid(np.arange(U.shape[-2]), np.arange(U.shape[-1]), indexing="ij")
    fi, fj = (j, i) if g & 4 else (i, j)                                                       # U[i][j] = F[j][i]
    ri = H - 1 - fi if g & 2 else fi
    rj = W - 1 - fj if g & 1 else fj
    assert np.array_equal(U.numpy(), R.numpy()[:, :, ri, rj])
    assert torch.equal(tta_ref.unpermute(U, g), R)
    for size in ((H, W), (32, 64), (64, 96)):                                                   # with a resample: the inverse of the permutation still
        v = (g, size[0], size[1])
        mid = tta_ref.resize(R, size)
        assert torch.equal(tta_ref.unpermute(tta_ref.view(R, v, torch.float64), g), mid)
        back = tta_ref.unview(tta_ref.view(R, v, torch.float64), v, (H, W), torch.float64)
        assert torch.equal(back, tta_ref.resize(mid, (H, W)))
    assert torch.equal(tta_ref.unview(tta_ref.view(R, (g, H, W), torch.float64), (g, H, W), (H, W), torch.float64), R)


def test_the_fused_maps_of_a_pointwise_model_are_those_of_the_plain_image():
    image = torch.randn(2, 3, H, W, generator=torch.Generator().manual_seed(3))
    model, views = _Stub(), [(g, H, W) for g in range(8)]
    maps = tta_ref.fuse64([model(tta_ref.view(image, v))[0] for v in views], views, (H, W))
    plain = model(image)[0].double().numpy()
    assert np.abs(maps["std"]).max() < 1e-15 and np.abs(maps["mean"] - 1.0 / (1.0 + np.exp(-plain))).max() < 1e-15


# --------------------------------------------------------------------------------------------------------------- declarations
def test_symbols_are_declared_with_the_headers_argument_counts():
    from uda_clr_amd.kernels import SYMBOLS, HipKernels
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("uda_tta_view", "uda_tta_fuse"):
        m = re.search(r"\bint %s\s*\((.*?)\)\s*;" % name, txt, flags=re.S)
        assert m, name
        assert len(SYMBOLS[name][1]) == len(m.group(1).split(",")), name
    assert len(SYMBOLS["uda_tta_view"][1]) == 10 and len(SYMBOLS["uda_tta_fuse"][1]) == 16
    assert callable(getattr(HipKernels, "tta_view")) and callable(getattr(HipKernels, "tta_fuse"))
    assert callable(ops.tta_view) and callable(ops.tta_fuse)
    src = open(os.path.join(ROOT, "uda_clr_amd", "csrc", "tta.hip")).read()
    shared = open(os.path.join(ROOT, "uda_clr_amd", "csrc", "tta_fuse.h")).read()
    assert '#include "tta_fuse.h"' in src and '#include "unc_element.h"' in shared and "unc_element<T>" in shared     # the same code, not a copy
    assert '#include "unc_element.h"' in open(os.path.join(ROOT, "uda_clr_amd", "csrc", "uncertainty.hip")).read()
    assert "unc_element.h" in open(os.path.join(ROOT, "uda_clr_amd", "csrc", "Makefile")).read()
    lib = os.path.join(ROOT, "uda_clr_amd", "lib", "libuda_clr_hip.so")
    if os.path.exists(lib):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "uda_tta_view") and hasattr(ctypes.CDLL(lib), "uda_tta_fuse")
