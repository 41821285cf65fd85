"""-m gpu: uda_tta_view and uda_tta_fuse (csrc/tta.hip) against the restatements of tests/tta_ref.py and against uda_mc_uncertainty,
uda_clr_amd.tta on the device, and evaluate / predict with test-time augmentation end to end.

The small frame is 48 x 80 with B = 2, C = 2 (3 for an image): not square, so that swapped axes, a swapped h / w or a transposed tensor
read as if it were not show; 48 and 80 are no multiples of the kernels' 32 x 32 tile.  The scaled sizes are (32, 64) and (64, 96).

Exact parts have no tolerance: a view of the frame's own size is a permutation, and the fuse of such views must give the bits of
uda_mc_uncertainty on the inverse-permuted stack.  Scaled parts: bound = 4 x the max abs error, against float64, of the same statement
in fp32 torch on the CPU on the same input (the factor covers another association of the lerp and another expf); each test forms that
yardstick again and prints it beside the kernel's error.

The round trip (a pointwise model under d4): every view's logit at a pixel is the plain image's logit, so the std is exactly 0 and the
mean has the bits of the same statistics on 8 copies of the plain logits.  "sigmoid of the model on the plain image" is read as the
library's sigmoid (unc_element.h, which uda_tta_fuse must use unchanged): torch.sigmoid forms exp(-x) in one step where unc_element
squares exp(-|x| / 2), so the two differ in the last bit on a share of the pixels whatever the views do; against float64 the mean is
held to 4 x the error of torch's fp32 sigmoid."""
import csv
import ctypes as C
import math

import numpy as np
import pytest
import torch

import tta_ref
import uncertainty_ref as ur
from kernel_cases import footprint, footprint_violations, out_dev, ro_dev
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict, tta
from uda_clr_amd.dataloaders import synthetic

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MAPS = ("mean", "std", "entropy", "mi")
B, H, W = 2, 48, 80
SCALED = ((32, 64), (64, 96))
D4 = [(g, H, W) for g in range(8)]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _image(Cc):
    return torch.randn(B, Cc, H, W, generator=torch.Generator().manual_seed(20 + Cc))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _raw_view(K, image, out, v):
    g, h, w = v
    return K.lib.uda_tta_view(image.data_ptr(), image.shape[0], image.shape[1], image.shape[2], image.shape[3], g, h, w, out.data_ptr(), _stream())


def _raw_fuse(K, logits, views, Bn, Cc, size, outs, u8, scale=1600.0, V=None, ptrs=None):
    V = len(views) if V is None else V
    n = max(len(views), 1)
    ptrs = [t.data_ptr() for t in logits] if ptrs is None else ptrs
    ints = lambda k: (C.c_int * n)(*[v[k] for v in views])
    return K.lib.uda_tta_fuse((C.c_void_p * n)(*ptrs), ints(0), ints(1), ints(2), V, Bn, Cc, size[0], size[1],
                              *[None if o is None else o.data_ptr() for o in outs], None if u8 is None else u8.data_ptr(), scale, _stream())


# ---------------------------------------------------------------------------------------------------------- the view kernel
@pytest.mark.parametrize("Cc", [3, 2])
def test_views_of_the_frames_size_are_permutations(Cc):
    K, image = ops.kernels(), _image(Cc)
    for g in range(8):
        want = tta_ref.permute(image, g).contiguous()
        with footprint():
            x = ro_dev(image, DEV, "image")
            out = out_dev(tuple(want.shape), torch.float32, DEV, name="view %d" % g)
            rc = _raw_view(K, x, out, (g, H, W))
            torch.cuda.synchronize()
            assert rc == 0, K.lib.uda_last_error()
        assert footprint_violations() == [], "uda_tta_view wrote outside its output: (buffer, first position)"
        assert torch.equal(_bits(out.cpu()), _bits(want)), g
        assert torch.equal(ops.tta_view(image, (g, H, W)).cpu(), want)


_RESIZED = {}


def _resized(size):
    """the 3-channel image resampled to ``size`` in float64 and in fp32 torch: computed once per size"""
    if size not in _RESIZED:
        image = _image(3)
        _RESIZED[size] = (tta_ref.resize(image.double(), size), tta_ref.resize(image, size))
    return _RESIZED[size]


@pytest.mark.parametrize("size", SCALED + ((96, 160), (16, 16)), ids=lambda s: "%dx%d" % s)
def test_scaled_views_against_float64(size):
    K, x = ops.kernels(), _image(3).to(DEV)
    r64, r32 = _resized(size)
    yard = float((r32.double() - r64).abs().max())
    worst = 0.0
    for g in range(8):
        got = K.tta_view(x, (g,) + size).cpu()
        want = tta_ref.permute(r64, g)
        assert got.shape == want.shape and got.is_contiguous()
        worst = max(worst, float((got.double() - want).abs().max()))
    print("view %dx%d -> %dx%d: max abs error %.2e (yardstick %.2e, fp32 torch against float64)" % (H, W, size[0], size[1], worst, yard))
    assert yard > 0 and worst <= 4 * yard, (worst, yard)


# ------------------------------------------------------------------------------------------------------ the fuse, exact part
def _d4_case():
    """8 passes of logits in the frame (planted +-40, +-90, 0 in every pass at the same places, as the uncertainty tests) and the same
    passes stored as the eight views see them: pass g permuted by code g, the transposed ones [80][48]"""
    x = ur.mc_logits(8, B, H, W, 108)
    return x, [tta_ref.permute(x[g], g).contiguous() for g in range(8)]


def test_fuse_of_permuted_passes_equals_mc_uncertainty():
    K = ops.kernels()
    x, stored = _d4_case()
    assert [tuple(t.shape[-2:]) for t in stored] == [(H, W)] * 4 + [(W, H)] * 4
    want = K.mc_uncertainty(x.to(DEV), MAPS, u8_scale=1600.0)
    with footprint():
        logits = [ro_dev(t, DEV, "view %d" % g) for g, t in enumerate(stored)]
        outs = [out_dev((B, 2, H, W), torch.float32, DEV, name=k) for k in MAPS]
        u8 = out_dev((B, 2, H, W), torch.uint8, DEV, name="std_u8")
        rc = _raw_fuse(K, logits, D4, B, 2, (H, W), outs, u8)
        torch.cuda.synchronize()
        assert rc == 0, K.lib.uda_last_error()
    assert footprint_violations() == [], "uda_tta_fuse wrote outside its outputs: (buffer, first position)"
    for k, o in zip(MAPS, outs):
        assert torch.equal(_bits(o), _bits(want[k])), k
    assert torch.equal(u8, want["std_u8"])
    flat = {k: o.reshape(-1).cpu() for k, o in zip(MAPS, outs)}
    for i, v in enumerate((40.0, -40.0, 90.0, -90.0, 0.0)):
        j = 3 + 7 * i
        assert flat["std"][j] == 0.0 and abs(float(flat["mean"][j]) - (0.5 if v == 0 else float(v > 0))) <= 1e-15
    # any order of the views is the same order of the passes
    order = [5, 0, 7, 2, 4, 1, 6, 3]
    got = ops.tta_fuse([stored[g] for g in order], [D4[g] for g in order], (H, W), MAPS, u8_scale=1600.0)
    want = K.mc_uncertainty(x[order].contiguous().to(DEV), MAPS, u8_scale=1600.0)
    assert set(got) == set(want) and all(torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)) for k in want)


def _pointwise(x):
    """a fixed 3 -> 2 channel linear map, done in torch where x lives"""
    return torch.stack([1.5 * x[:, 0] - 2.0 * x[:, 1] + 0.25 * x[:, 2] + 0.5, -0.75 * x[:, 0] + 3.0 * x[:, 2] - 1.0], 1), None


def test_round_trip_of_a_pointwise_model_under_d4():
    image = (2.0 * _image(3)).to(DEV)
    got = tta.tta_predict(_pointwise, image, "d4", outputs=("mean", "std"), u8_scale=1600.0)
    plain = _pointwise(image)[0].contiguous()
    assert float(got["std"].abs().max()) == 0.0 and not bool(got["std_u8"].any())           # every view brought the same logit to every pixel
    same = ops.mc_uncertainty(plain[None].expand(8, -1, -1, -1, -1).contiguous(), ("mean",))["mean"]
    assert torch.equal(_bits(got["mean"]), _bits(same))                                       # the library's sigmoid of the plain image
    p64 = torch.sigmoid(plain.double().cpu())
    yard = float((torch.sigmoid(plain.cpu()).double() - p64).abs().max())
    err = float((got["mean"].cpu().double() - p64).abs().max())
    differ = int((got["mean"] != torch.sigmoid(plain)).sum())
    print("round trip: mean against float64 sigmoid %.2e (yardstick %.2e); %d of %d elements differ from torch.sigmoid on the device in the last bits"
          % (err, yard, differ, plain.numel()))
    assert err <= 4 * yard
    # a code whose forward and inverse do not match moves a value: a model that is not pointwise must then show a spread
    ramp = lambda x: (_pointwise(x)[0] + torch.linspace(-3, 3, x.shape[-1], device=x.device), None)
    assert float(tta.tta_predict(ramp, image, "d4", outputs=("std",))["std"].max()) > 0.01


# ----------------------------------------------------------------------------------------------------- the fuse, scaled part
def _mixed_views(V):
    if V == 2:
        return [(5, 32, 64), (0, 64, 96)]
    if V == 5:
        return [(0, H, W), (6, 32, 64), (3, 64, 96), (7, 64, 96), (1, 32, 64)]
    sizes = ((H, W),) + SCALED
    return [(i % 8,) + sizes[(i // 8) % 3] for i in range(24)] + [(i % 8,) + SCALED[i % 2] for i in range(24, V)]


_FUSED = {}


def _fused_case(key, views):
    """logits of the views, their float64 maps and the fp32 torch statement's max abs error per map: computed once per case"""
    if key not in _FUSED:
        logits = tta_ref.view_logits(views, B, 2, 300 + len(views))
        want = tta_ref.fuse64(logits, views, (H, W))
        t32 = tta_ref.fuse32_torch(logits, views, (H, W))
        _FUSED[key] = (logits, want, {k: float(np.abs(t32[k].astype(np.float64) - want[k]).max()) for k in MAPS})
    return _FUSED[key]


def _check_fused(name, views, got, want, yard):
    host = {k: v.cpu().numpy() for k, v in got.items()}
    line = []
    for k in MAPS:
        assert host[k].shape == want[k].shape == (B, 2, H, W) and host[k].dtype == np.float32
        line.append("%s %.2e (yardstick %.2e)" % (k, float(np.abs(host[k].astype(np.float64) - want[k]).max()), yard[k]))
    print("%s: " % name + ", ".join(line))
    for k in MAPS:
        err = float(np.abs(host[k].astype(np.float64) - want[k]).max())
        assert yard[k] > 0 and err <= 4 * yard[k], (k, err, yard[k])
    assert host["std_u8"].dtype == np.uint8 and np.array_equal(host["std_u8"], ur.quantise(host["std"], 1600.0))


@pytest.mark.parametrize("V", [2, 5, 32])
def test_scaled_fuse_against_float64(V):
    views = _mixed_views(V)
    assert len(views) == V and {v[1:] for v in views} >= set(SCALED)
    logits, want, yard = _fused_case(V, views)
    got = ops.tta_fuse(logits, views, (H, W), MAPS, u8_scale=1600.0)
    torch.cuda.synchronize()
    _check_fused("V=%d" % V, views, got, want, yard)


def test_transposed_views_too_large_for_the_lds_rectangle():
    """(96, 160) is twice the frame: a tile's taps span 66 stored rows, beyond the 48 of the LDS rectangle, so the transposed views take
    their taps from memory; (64, 96) beside them takes the LDS path"""
    views = [(4, 96, 160), (7, 96, 160), (5, 64, 96), (6, 96, 160), (2, 96, 160)]
    logits, want, yard = _fused_case("large", views)
    got = ops.tta_fuse(logits, views, (H, W), MAPS, u8_scale=1600.0)
    torch.cuda.synchronize()
    _check_fused("large views", views, got, want, yard)


# -------------------------------------------------------------------------------------------------------------- other properties
def test_subsets_of_the_outputs_and_an_image_alone_give_the_same_bits():
    views = _mixed_views(5)
    logits = [t.to(DEV) for t in _fused_case(5, views)[0]]
    full = ops.tta_fuse(logits, views, (H, W), MAPS, u8_scale=1600.0)
    for names, scale in ((("std",), None), (("mean", "std"), None), (("entropy",), None), (("mi", "mean"), 1600.0), ((), 1600.0), (("mean",), None)):
        part = ops.tta_fuse(logits, views, (H, W), names, u8_scale=scale)
        assert set(part) == set(names) | ({"std_u8"} if scale else set())
        for k, v in part.items():
            assert torch.equal(v.view(torch.uint8), full[k].view(torch.uint8)), (names, k)
    alone = ops.tta_fuse([t[1:2].contiguous() for t in logits], views, (H, W), MAPS, u8_scale=1600.0)
    for k, v in alone.items():
        assert v.shape[0] == 1 and torch.equal(v.view(torch.uint8), full[k][1:2].contiguous().view(torch.uint8)), k
    image = _image(3).to(DEV)
    for v in ((5, 32, 64), (2, H, W), (7, 64, 96)):
        assert torch.equal(ops.tta_view(image[1:2].contiguous(), v), ops.tta_view(image, v)[1:2])
    with pytest.raises(ValueError, match="outputs"):
        ops.tta_fuse(logits, views, (H, W), ())
    with pytest.raises(ValueError, match="outputs"):
        ops.tta_fuse(logits, views, (H, W), ("variance",))


def _bad(name):
    views = [(g, H, W) for g in (0, 1)]
    case = dict(views=views, V=None, null=None, match=b"uda_tta_fuse", size=(H, W), Bn=B, Cc=2)
    if name == "V=1":
        case.update(views=views[:1], match=b"1 views outside 2..32")
    elif name == "V=33":
        case.update(views=[(g % 8, H, W) for g in range(33)], match=b"33 views outside 2..32")
    elif name == "g=8":
        case.update(views=[(0, H, W), (8, H, W)], match=b"code 8")
    elif name == "h=40":
        case.update(views=[(0, H, W), (1, 40, W)], match=b"40 x 80")
    elif name == "null view":
        case.update(null=1, match=b"view 1: null logits")
    elif name == "H=40":
        case.update(size=(40, W), match=b"H 40")
    elif name == "B=0":
        case.update(Bn=0, match=b"batch 0")
    elif name == "C=5":
        case.update(Cc=5, match=b"5 channels")
    return case


@pytest.mark.parametrize("name", ["V=1", "V=33", "g=8", "h=40", "null view", "H=40", "B=0", "C=5"])
def test_bad_arguments_are_errors_that_write_nothing(name):
    K, case = ops.kernels(), _bad(name)
    views = case["views"]
    store = torch.zeros(B, 2, H, W, device=DEV)
    ptrs = [store.data_ptr()] * len(views)
    if case["null"] is not None:
        ptrs[case["null"]] = None
    outs = [torch.full((B, 2, H, W), -7.0, device=DEV) for _ in MAPS]
    u8 = torch.full((B, 2, H, W), 0xA5, dtype=torch.uint8, device=DEV)
    rc = _raw_fuse(K, None, views, case["Bn"], case["Cc"], case["size"], outs, u8, ptrs=ptrs)
    torch.cuda.synchronize()
    assert rc != 0 and case["match"] in K.lib.uda_last_error(), K.lib.uda_last_error()
    assert all(bool((o == -7.0).all()) for o in outs) and bool((u8 == 0xA5).all())
    out = torch.full((B, 2, W, H), -7.0, device=DEV)
    bad_view = {"g=8": (8, H, W), "h=40": (1, 40, W)}.get(name)
    if bad_view is not None:
        rc = _raw_view(K, store, out, bad_view)
        torch.cuda.synchronize()
        assert rc != 0 and b"uda_tta_view" in K.lib.uda_last_error() and bool((out == -7.0).all())
        with pytest.raises(ValueError, match="code 8" if name == "g=8" else "40 x 80"):
            ops.tta_view(store, bad_view)
    if name in ("V=1", "V=33", "g=8", "h=40"):
        with pytest.raises(ValueError, match={"V=1": "1 views", "V=33": "33 views", "g=8": "code 8", "h=40": "40 x 80"}[name]):
            ops.tta_fuse([store] * len(views), views, (H, W))
    if name == "null view":
        with pytest.raises(ValueError, match="view 1: no logits"):
            ops.tta_fuse([store, None], views, (H, W))
        rc = K.lib.uda_tta_fuse(None, None, None, None, 2, B, 2, H, W, *[o.data_ptr() for o in outs], u8.data_ptr(), 1600.0, _stream())
        assert rc != 0 and b"null argument" in K.lib.uda_last_error()
        rc = _raw_fuse(K, None, views, B, 2, (H, W), [None] * 4, None, ptrs=[store.data_ptr()] * 2)
        assert rc != 0 and b"no output" in K.lib.uda_last_error()
        rc = K.lib.uda_tta_view(None, B, 2, H, W, 0, H, W, out.data_ptr(), _stream())
        assert rc != 0 and b"null argument" in K.lib.uda_last_error() and bool((out == -7.0).all())
        with pytest.raises(ValueError, match=r"shape \(2, 2, 80, 48\)"):
            ops.tta_fuse([store, store], [(0, H, W), (4, H, W)], (H, W))                      # a transposed view stored as if it were not


# ------------------------------------------------------------------------------------------------------------------ end to end
def _brightness_model(image):
    """stand-in generator for the drawn images of dataloaders.synthetic: disc and cup by brightness (pointwise: every view agrees)"""
    grey = (image.mean(1) + 1.0) * 127.5
    return torch.stack([(grey - 165.0), (grey - 110.0)], 1) / 8.0, None


def _leaning_model(image):
    """the same with a tilt along the columns: not symmetric under the mirrorings, so the views disagree near the borders"""
    tilt = torch.linspace(-1.5, 1.5, image.shape[-1], device=image.device)
    return _brightness_model(image)[0] + tilt, None


def _same(a, b):
    return a == b or (isinstance(a, float) and isinstance(b, float) and math.isnan(a) and math.isnan(b))


def test_evaluate_with_tta_on_the_generator(tmp_path, capsys):
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=64)
    torch.manual_seed(3)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16, sync_bn=True).to(DEV)
    argv = ["--data-dir", str(tmp_path), "--dataset", "Drishti-GS", "--checkpoint", "unused", "--batch-size", "2"]
    res = ev.main(argv + ["--tta", "flips,id@0.75,id@1.25", "--tta-uncertainty", "--calibration", "--csv", str(tmp_path / "t.csv"),
                          "--save-dir", str(tmp_path / "pictures")], model=model)
    assert "cup_cov_0.04" in capsys.readouterr().out
    names = ev.CALIBRATION_FIELDS + ev.uncertainty_fields()
    assert res["extra_fields"] == names and res["n_images"] == 3
    assert res["tta"] == [[g, 64, 64] for g in range(4)] + [[0, 48, 48], [0, 80, 80]]
    print("tta on the generator: " + "  ".join("%s %.4f" % (k, res["mean"][k]) for k in names))
    for r in res["per_image"]:
        assert set(r) == {"img_name"} | set(ev.FIELDS) | set(names)
        for k in ev.CALIBRATION_FIELDS + ("cup_cov_0.04", "disc_cov_0.04", "cup_dice_0.04", "disc_dice_0.04"):
            assert math.isfinite(r[k]) and 0.0 <= r[k] <= 1.0, (k, r[k])
        stem = r["img_name"].split(".")[0]
        for folder in ("overlay", "mask", "uncertainty"):
            assert (tmp_path / "pictures" / folder / (stem + ".png")).exists()
    assert all(math.isfinite(res["mean"][k]) for k in ev.CALIBRATION_FIELDS + ("cup_cov_0.04", "disc_cov_0.04"))
    assert res["risk_coverage"]["views"] == 6 and "passes" not in res["risk_coverage"] and np.asarray(res["risk_coverage"]["risk"]).sum() == 3 * 2 * 64 * 64
    assert np.asarray(res["calibration"]["rel"])[..., 0].sum() == 3 * 2 * 64 * 64
    rows = list(csv.reader(open(tmp_path / "t.csv")))
    assert rows[0] == ["img_name"] + list(ev.FIELDS + names) and len(rows) == 4


def test_evaluate_with_a_pointwise_model_under_d4_gives_the_result_without_tta(tmp_path):
    synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=64)
    argv = ["--data-dir", str(tmp_path), "--dataset", "Drishti-GS", "--checkpoint", "unused", "--batch-size", "2", "--hd95", "--cdr"]
    plain = ev.main(argv, model=_brightness_model)
    res = ev.main(argv + ["--tta", "d4"], model=_brightness_model)
    assert res.pop("tta") == [[g, 64, 64] for g in range(8)] and "tta" not in plain
    assert set(res) == set(plain) and res["n_images"] == 3 and res["n_undefined"] == plain["n_undefined"] and res["extra_fields"] == plain["extra_fields"]
    for r, p in zip(res["per_image"], plain["per_image"]):
        assert set(r) == set(p) and all(_same(r[k], p[k]) for k in p), (r, p)
    assert all(_same(res["mean"][k], plain["mean"][k]) for k in plain["mean"])


def test_predict_with_tta_writes_pictures_and_columns(tmp_path):
    from PIL import Image
    split = synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=64)
    images = split + "/ROIs/image"
    plain = predict.main(["--images", images, "--out", str(tmp_path / "a"), "--batch-size", "2"], model=_leaning_model)
    rows = predict.main(["--images", images, "--out", str(tmp_path / "b"), "--csv", str(tmp_path / "b.csv"), "--batch-size", "2", "--tta", "flips",
                         "--tta-uncertainty"], model=_leaning_model)
    assert len(rows) == 3 and [r["img_name"] for r in rows] == [p["img_name"] for p in plain]
    spread = 0
    for r in rows:
        assert set(r) == {"img_name", "vcdr_pred"} | set(predict.UNCERTAINTY_COLUMNS)
        stem = r["img_name"].split(".")[0]
        for folder in ("overlay", "original_image", "mask", "uncertainty"):
            assert (tmp_path / "b" / folder / (stem + ".png")).exists(), folder
        png = np.asarray(Image.open(tmp_path / "b" / "uncertainty" / (stem + ".png")))
        assert png.shape == (64, 64, 3) and not png[..., 0].any()
        spread += int(png[..., 1:].max())
        assert r["unsure_px"] >= 0
    assert spread > 0                                                                         # the tilted model's views do disagree
    back = list(csv.reader(open(tmp_path / "b.csv")))
    assert back[0] == ["img_name", "vcdr_pred"] + list(predict.UNCERTAINTY_COLUMNS) and len(back) == 4
    with pytest.raises(ValueError, match="tta_uncertainty=True needs tta"):
        predict.main(["--images", images, "--out", str(tmp_path / "c"), "--tta-uncertainty"], model=_leaning_model)
