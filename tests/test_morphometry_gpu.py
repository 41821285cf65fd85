"""-m gpu: uda_disc_morphometry (csrc/morphometry.hip) against the numpy restatement of tests/morphometry_ref.py - every entry of
moments, extent, overlap and radial, all integers, for equality; determinism, batch independence, mask types, the argument checks and
the write footprint; evaluate(morphometry=True) and predict --morphometry on the device against the figures from the pixels.

There is no tolerance on any integer.  The floats of the last two tests are compared as tests/test_morphometry_cpu.py states."""
import csv
import math

import numpy as np
import pytest
import torch

import morphometry_ref as mr
from kernel_cases import footprint, footprint_violations, out_dev, ro_dev
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict
from uda_clr_amd.dataloaders import synthetic
from uda_clr_amd.kernels import HipKernels
from uda_clr_amd.utils import metrics

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("moments", "extent", "overlap", "radial")


def _u8(m):
    return torch.from_numpy(np.asarray(m).astype(np.uint8)).to(DEV)


def _table(K):
    return torch.from_numpy(metrics.sector_table(K)).to(DEV)


def _run(masks, K):
    out = ops.kernels().disc_morphometry(_u8(masks), _table(K))
    torch.cuda.synchronize()
    return dict(zip(NAMES, (t.cpu().numpy() for t in out)))


def _check(masks, K):
    got, want = _run(masks, K), mr.integers(masks, metrics.sector_table(K))
    for name in NAMES:
        assert got[name].dtype == np.int64 and got[name].shape == want[name].shape, name
        bad = got[name] != want[name]
        assert not bad.any(), "%s differs in %d of %d entries, first at %s: %d for %d" % (
            name, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[name][bad][0], want[name][bad][0])
    return got


def _n_empty(got):
    return metrics.morphometry_from_moments(got)["n_empty_sectors"]


def test_nested_squares_9x9_on_the_boundary_rays():
    got = _check(mr.nested_9x9(), 8)
    assert got["radial"].tolist() == [[[625, 1250] * 4, [3125, 5000] * 4]] and got["overlap"].tolist() == [9]
    assert got["extent"].tolist() == [[[3, 5, 3, 5], [2, 6, 2, 6]]]


@pytest.mark.parametrize("H,W", [(33, 17), (96, 80)], ids=["33x17", "96x80"])
def test_ellipse_pairs(H, W):
    """W = 17: the byte-wise walk (and shapes so small that sectors stay empty: the -1 entries are compared like every other);
    W = 80: the 16-byte walk, cup semi-axes >= 14 px, so no sector is empty"""
    got = _check(mr.ellipse_pairs(100 + H, 3, H, W), 72)
    if W == 80:
        assert (_n_empty(got) == 0).all()


def test_ellipse_pairs_512():
    got = _check(mr.ellipse_pairs(612, 2, 512, 512), 72)
    assert (_n_empty(got) == 0).all() and (got["radial"] > 0).all()


def test_empty_cup_empty_disc_and_both():
    got = _check(mr.empties_96x80(), 72)
    assert (got["moments"][0, 0] == 0).all() and (got["extent"][0, 0] == -1).all() and (got["radial"][0, 0] == -1).all() and (got["radial"][0, 1] >= 0).all()
    assert (got["moments"][1, 1] == 0).all() and (got["radial"][1] == -1).all() and got["moments"][1, 0, 0] > 0 and (got["extent"][1, 0] >= 0).all()
    assert (got["moments"][2] == 0).all() and (got["extent"][2] == -1).all() and (got["radial"][2] == -1).all() and got["overlap"].tolist()[1:] == [0, 0]


def test_cup_partly_outside_the_disc():
    m = mr.cup_partly_outside_96x80()
    got = _check(m, 72)
    assert 0 < got["overlap"][0] < got["moments"][0, 0, 0] and (got["radial"][0, 0] > got["radial"][0, 1]).any()


def test_cup_away_from_the_disc_centroid_leaves_sectors_empty():
    got = _check(mr.cup_off_centre_96x80(), 72)
    assert 0 < (got["radial"][0, 0] == -1).sum() < 72 and (got["radial"][0, 1] >= 0).all()


def test_single_pixel_disc_has_no_sector():
    got = _check(mr.single_pixel_disc(), 8)
    assert (got["radial"] == -1).all() and got["moments"][0, 1].tolist() == [1, 20, 5, 400, 25, 100] and got["extent"][0, 1].tolist() == [20, 20, 5, 5]


def test_masks_touching_all_four_borders():
    got = _check(mr.touching_borders_96x80(), 72)
    assert got["extent"][0, 0].tolist() == got["extent"][0, 1].tolist() == got["extent"][1, 1].tolist() == [0, 95, 0, 79]


def test_360_sectors():
    _check(mr.ellipse_pairs(7, 1, 96, 80), 360)


def test_full_plane_1024_has_the_largest_magnitudes():
    got = _check(mr.full_minus_corner_1024(), 72)
    n = 1024 * 1024 - 1
    assert got["moments"][0, 1, 0] == n and got["radial"].max() > 2 ** 58 and got["moments"][0, 1, 3] > 2 ** 38
    assert (_n_empty(got) > 0).all()                       # the cup sits in one corner


def test_deterministic_and_independent_of_the_batch():
    masks = np.concatenate([mr.ellipse_pairs(6, 3, 96, 80), mr.empties_96x80(), mr.cup_off_centre_96x80()])
    K, m, t = ops.kernels(), _u8(masks), _table(72)
    a, b = K.disc_morphometry(m, t, want_packed=True)[-1], K.disc_morphometry(m, t, want_packed=True)[-1]
    assert torch.equal(a, b)
    whole = K.disc_morphometry(m, t)
    back = K.disc_morphometry(torch.flip(m, [0]).contiguous(), t)
    for i in range(masks.shape[0]):
        alone = K.disc_morphometry(m[i:i + 1].contiguous(), t)
        for w, o, r in zip(whole, alone, back):
            assert torch.equal(w[i], o[0]) and torch.equal(w[i], r[masks.shape[0] - 1 - i]), i


def test_front_end_takes_uint8_bool_float_and_host_masks():
    masks = mr.ellipse_pairs(6, 2, 96, 80)
    want = mr.integers(masks, metrics.sector_table(72))
    u8 = torch.from_numpy(masks.astype(np.uint8) * 255)
    for m in (u8, u8.to(DEV), torch.from_numpy(masks), torch.from_numpy(masks).to(DEV), torch.from_numpy(masks.astype(np.float32)).to(DEV),
              torch.from_numpy(masks.astype(np.float64) * 0.9)):
        got = ops.disc_morphometry(m)
        assert set(got) == set(NAMES) | {"table"} and np.array_equal(got["table"], metrics.sector_table(72))
        for name in NAMES:
            assert isinstance(got[name], np.ndarray) and got[name].dtype == np.int64 and np.array_equal(got[name], want[name]), name
    got = ops.disc_morphometry(u8, sectors=metrics.sector_table(8))
    assert np.array_equal(got["radial"], mr.integers(masks, metrics.sector_table(8))["radial"])


@pytest.mark.parametrize("case", ["K=12", "K=368", "H=1025", "short workspace"])
def test_bad_arguments_return_an_error_and_write_nothing(case):
    K = ops.kernels()
    B, H, W, S = 1, 64, 48, 16
    masks = torch.ones(B, 2, 1025, W, dtype=torch.uint8, device=DEV)          # large enough for the rejected H as well
    table = torch.from_numpy(np.concatenate([metrics.sector_table(360), metrics.sector_table(8)])).to(DEV)
    outs = [torch.full(shape, -77, dtype=torch.int64, device=DEV) for shape in ((B, 2, 6), (B, 2, 4), (B,), (B, 2, 368))]
    need = K.lib.uda_disc_morphometry_workspace_bytes(B, H, W, S)
    assert need >= B * 8 * 4 and K.lib.uda_disc_morphometry_workspace_bytes(B, 1024, 1024, 360) == need      # per image, not per pixel
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    h, nbytes = H, need
    if case == "K=12":
        S = 12
    elif case == "K=368":
        S = 368
    elif case == "H=1025":
        h = 1025
    else:
        nbytes = need - 1
    rc = K.lib.uda_disc_morphometry(masks.data_ptr(), B, h, W, table.data_ptr(), S, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                    outs[3].data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_disc_morphometry" in K.lib.uda_last_error()
    assert all(bool((o == -77).all()) for o in outs) and bool((ws == 0xA5).all()) and bool((masks == 1).all())
    with pytest.raises(ValueError, match="multiple of 8"):
        K.disc_morphometry(masks[:, :, :H].contiguous(), table[:12].contiguous())


@pytest.mark.parametrize("H,W", [(33, 17), (96, 80)], ids=["bytes", "words"])
def test_write_footprint(H, W):
    """only the four outputs and the queried workspace bytes change; the masks and the table keep every bit"""
    masks, S = mr.ellipse_pairs(3, 2, H, W), 72
    want = mr.integers(masks, metrics.sector_table(S))
    B = masks.shape[0]
    K = ops.kernels()
    with footprint():
        m = ro_dev(torch.from_numpy(masks.astype(np.uint8)), DEV, "masks")
        t = ro_dev(torch.from_numpy(metrics.sector_table(S)), DEV, "sectors")
        outs = [out_dev(shape, torch.int64, DEV, name=name) for name, shape in zip(NAMES, ((B, 2, 6), (B, 2, 4), (B,), (B, 2, S)))]
        ws = HipKernels._ws(m, K.lib.uda_disc_morphometry_workspace_bytes(B, H, W, S))
        assert m.data_ptr() % 16 == 0
        rc = K.lib.uda_disc_morphometry(m.data_ptr(), B, H, W, t.data_ptr(), S, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                        outs[3].data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0, K.lib.uda_last_error()
    assert footprint_violations() == [], "uda_disc_morphometry wrote outside its outputs: (buffer, first position)"
    for name, o in zip(NAMES, outs):
        assert np.array_equal(o.cpu().numpy(), want[name]), name


# ------------------------------------------------------------------------------------------------ evaluate and predict on the device
def _brightness_model(image):
    """stand-in generator for the drawn images of dataloaders.synthetic: disc and cup by brightness"""
    grey = (image.mean(1) + 1.0) * 127.5
    return torch.stack([(grey - 165.0), (grey - 110.0)], 1), None


@pytest.fixture
def recorded(monkeypatch):
    """ops.disc_morphometry as it is, with the masks and the sectors of every call kept"""
    calls, real = [], ops.disc_morphometry

    def morph(masks, sectors=72):
        calls.append((masks.detach().cpu().numpy() != 0, sectors))
        return real(masks, sectors)
    monkeypatch.setattr(ops, "disc_morphometry", morph)
    return calls


def _same(a, b):
    return a == b or (math.isnan(a) and math.isnan(b))


def _close(a, b, bound):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= bound


def test_evaluate_with_morphometry_on_synthetic_data(tmp_path, recorded, capsys):
    synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=128)
    argv = ["--data-dir", str(tmp_path), "--dataset", "Drishti-GS", "--checkpoint", "unused", "--batch-size", "2"]
    plain = ev.main(argv, model=_brightness_model)
    assert recorded == [] and set(plain) == {"per_image", "mean", "n_images", "n_undefined"} and set(plain["mean"]) == set(ev.FIELDS)
    assert all(set(r) == {"img_name"} | set(ev.FIELDS) for r in plain["per_image"])      # without the flag: no call, the result of before
    res = ev.main(argv + ["--morphometry", "--sectors", "40", "--csv", str(tmp_path / "m.csv")], model=_brightness_model)
    assert "rdr_min_pred" in capsys.readouterr().out
    assert res["extra_fields"] == ev.MORPHOMETRY_FIELDS and [c[0].shape for c in recorded] == [(4, 2, 128, 128), (2, 2, 128, 128)]
    assert all(c[1] == 40 for c in recorded)
    table = metrics.sector_table(40)
    masks = np.concatenate([recorded[0][0][:2], recorded[1][0][:1]]), np.concatenate([recorded[0][0][2:], recorded[1][0][1:]])
    fp, fg = mr.figures(masks[0], table), mr.figures(masks[1], table)
    assert (fg["acdr"] > 0).all() and np.isfinite(fp["acdr"]).all()                        # the stand-in does find every disc
    for i, (r, p) in enumerate(zip(res["per_image"], plain["per_image"])):
        assert all(_same(r[k], p[k]) for k in p)
        for x in ("hcdr", "acdr", "rdr_min"):
            assert _same(r[x + "_pred"], fp[x][i]) and _same(r[x + "_gt"], fg[x][i]) and _same(r[x + "_error"], abs(fp[x][i] - fg[x][i])), x
        for q in ("up", "left", "down", "right"):
            assert _same(r["rim_%s_pred" % q], fp["rim_" + q][i]) and _same(r["rim_%s_gt" % q], fg["rim_" + q][i]), q
        assert _close(r["cup_offset_pred"], fp["cup_offset"][i], 4 * 2.0 ** -52 * fp["cup_offset"][i])
    rows = list(csv.reader(open(tmp_path / "m.csv")))
    assert rows[0] == ["img_name"] + list(ev.FIELDS + ev.MORPHOMETRY_FIELDS) and len(rows) == 4
    for row, r in zip(rows[1:], res["per_image"]):
        assert all(_same(float(v), r[k]) for k, v in zip(rows[0][1:], row[1:]))


def test_predict_with_morphometry_on_synthetic_data(tmp_path, recorded):
    split = synthetic.write_dataset(str(tmp_path), "Drishti-GS", "test", n=3, size=128)
    images = split + "/ROIs/image"
    plain = predict.main(["--images", images, "--out", str(tmp_path / "a"), "--csv", str(tmp_path / "a.csv"), "--batch-size", "2"], model=_brightness_model)
    assert recorded == [] and all(set(r) == {"img_name", "vcdr_pred"} for r in plain)
    assert list(csv.reader(open(tmp_path / "a.csv")))[0] == ["img_name", "vcdr_pred"]
    rows = predict.main(["--images", images, "--out", str(tmp_path / "b"), "--csv", str(tmp_path / "b.csv"), "--batch-size", "2", "--morphometry"],
                        model=_brightness_model)
    assert [c[0].shape for c in recorded] == [(2, 2, 128, 128), (1, 2, 128, 128)] and all(c[1] == 72 for c in recorded)
    masks = np.concatenate([c[0] for c in recorded])
    want = mr.figures(masks, metrics.sector_table(72))
    assert np.isfinite(want["acdr"]).all()                                                 # the stand-in does find every disc
    for i, (r, p) in enumerate(zip(rows, plain)):
        assert r["img_name"] == p["img_name"] and _same(r["vcdr_pred"], p["vcdr_pred"]) and _same(r["vcdr_pred"], want["vcdr"][i])
        for x in ("hcdr", "acdr", "rdr_min", "rim_up", "rim_left", "rim_down", "rim_right"):
            assert _same(r[x + "_pred"], want[x][i]), x
        assert _close(r["cup_offset_pred"], want["cup_offset"][i], 4 * 2.0 ** -52 * want["cup_offset"][i])
        for k, c in enumerate(("cup", "disc")):
            if np.isnan(want["cov"][i, k]).any():          # (a cup that the post-processing emptied)
                assert math.isnan(r[c + "_major"]) and math.isnan(r[c + "_minor"]) and math.isnan(r[c + "_orientation"])
                continue
            major, minor, ang = mr.axes_of(want["cov"][i, k])
            assert abs(r[c + "_major"] - major) <= 1e-9 * major and abs(r[c + "_minor"] - minor) <= 1e-9 * major
            if minor < 0.99 * major:
                d = abs(r[c + "_orientation"] - ang)
                assert min(d, 180.0 - d) <= 1e-6
    back = list(csv.reader(open(tmp_path / "b.csv")))
    assert back[0] == ["img_name", "vcdr_pred"] + list(predict.MORPHOMETRY_COLUMNS) and len(back) == 4
    for row, r in zip(back[1:], rows):
        assert row[0] == r["img_name"] and all(_same(float(v), r[k]) for k, v in zip(back[0][1:], row[1:]))
