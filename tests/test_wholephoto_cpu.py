"""not-gpu: the numpy restatement of the whole-photograph entries (tests/wholephoto_ref.py) against what it restates - Pillow for the
cut, float64 interpolation for the paste rule - and the host-side pieces of uda_clr_amd/wholephoto.py and predict.py.  Nothing here
runs a kernel; tests/test_wholephoto_gpu.py compares the kernels with the restatement byte for byte."""
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import wholephoto_ref as wr
from uda_clr_amd import ops, predict, wholephoto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = wr.S_TEST


# ------------------------------------------------------------------------------------------------ cut
@pytest.mark.parametrize("case", wr.CUT_CASES, ids=[c[0] for c in wr.CUT_CASES])
def test_restated_cut_equals_pillow_byte_for_byte(case):
    _, i, (x0, y0, R) = case
    photo = wr.random_photos(12, wr.CUT_SHAPES)[i]
    want = np.asarray(Image.fromarray(photo).crop((x0, y0, x0 + R, y0 + R)).resize((S, S), Image.BILINEAR))
    got = wr.cut(photo, (x0, y0, R), S)
    assert got.dtype == np.uint8 and got.shape == (S, S, 3) and np.array_equal(got, want)


@pytest.mark.parametrize("R,size", [(800, 512), (1280, 512), (640, 512), (512, 512), (120, 48), (97, 48), (31, 48)])
def test_restated_cut_equals_pillow_at_the_working_sizes(R, size):
    """the default 800 -> 512, both bounds' neighbourhood, and the shapes of the second GPU case; a window over two sides"""
    photo = wr.random_photos(R, [(R + 37, R + 11)])[0]
    x0, y0 = -R // 3, 29
    want = np.asarray(Image.fromarray(photo).crop((x0, y0, x0 + R, y0 + R)).resize((size, size), Image.BILINEAR))
    assert np.array_equal(wr.cut(photo, (x0, y0, R), size), want)


# ------------------------------------------------------------------------------------------------ paste
def _float64_upsample(plane, R):
    return torch.nn.functional.interpolate(torch.from_numpy((plane != 0).astype(np.float64))[None, None], size=(R, R), mode="bilinear",
                                           align_corners=False)[0, 0].numpy()


@pytest.mark.parametrize("R", [16, 10, 25, 40, 8, 33])
def test_paste_rule_equals_float64_interpolation_outside_exact_ties(R):
    ties = 0
    for name, m in wr.mask_cases(13):
        for k in (0, 1):
            v = wr.upsample_votes(m[k], R)
            tie = 2 * v == 4 * R * R
            mine, theirs = 2 * v > 4 * R * R, _float64_upsample(m[k], R) > 0.5
            assert np.array_equal(mine[~tie], theirs[~tie]), (name, k)
            assert not mine[tie].any()                                         # a tie is not set
            assert (v >= 0).all() and (v <= 4 * R * R).all()
            ties += int(tie.sum())
    if R == 16:                                                                # the identity: no interpolation, no tie
        assert ties == 0
        for _, m in wr.mask_cases(13):
            assert np.array_equal(2 * wr.upsample_votes(m[0], 16) > 4 * 256, m[0] != 0)


def test_paste_ties_exist_and_are_counted():
    """R = 8 from S = 16 samples the midpoint between mask pixels 2 j and 2 j + 1, weight 1/2 each: where a region ends between such a
    pair the vote is exactly half, and the pixel is not set"""
    m = np.zeros((16, 16), np.uint8)
    m[:, :7] = 1
    v = wr.upsample_votes(m, 8)
    tie = 2 * v == 4 * 64
    assert int(tie.sum()) == 8 and tie[:, 3].all() and (2 * v > 4 * 64)[:, :3].all() and not (2 * v > 4 * 64)[:, 3:].any()
    assert (wr.paste(np.stack([m, m]), (0, 0, 8), 8, 8)[:, 3] == 255).all()


def test_paste_coding_and_outside():
    masks = dict(wr.mask_cases(13))
    g = wr.paste(masks["cup where the disc is not"], (5, 3, 16), 30, 44)
    win = g[3:19, 5:21]
    m = masks["cup where the disc is not"]
    assert np.array_equal(win == 0, m[0] != 0) and np.array_equal(win == 128, (m[1] != 0) & (m[0] == 0))      # cup without disc -> 0
    assert (g[:3] == 255).all() and (g[19:] == 255).all() and (g[:, :5] == 255).all() and (g[:, 21:] == 255).all()
    assert (wr.paste(masks["all ones"], (100, 100, 16), 30, 44) == 255).all()
    assert (wr.paste(masks["all ones"], (-14, -14, 40), 12, 12) == 0).all()


# ------------------------------------------------------------------------------------------------ reduce
def test_reduce_with_factor_1_is_the_identity_plus_zero_fill():
    for H, W in [(1, 1), (16, 16), (9, 16), (16, 5)]:
        photo = wr.random_photos(H * 31 + W, [(H, W)])[0]
        canvas, f = wr.reduce_photo(photo, S)
        assert f == 1 and np.array_equal(canvas[:H, :W], photo) and not canvas[H:].any() and not canvas[:, W:].any()


def test_reduce_partial_edge_blocks_and_rounding():
    photo = wr.random_photos(3, [(33, 64)])[0]
    canvas, f = wr.reduce_photo(photo, S)
    assert f == 4 and not canvas[9:].any()
    assert np.array_equal(canvas[8, 3], (photo[32:33, 12:16].astype(np.int64).sum((0, 1)) + 2) // 4)          # one row of the last block row
    assert np.array_equal(canvas[2, 5], (photo[8:12, 20:24].astype(np.int64).sum((0, 1)) + 8) // 16)
    assert [wr.factor_of(*hw, S) for hw in wr.REDUCE_SHAPES] == [1, 1, 2, 4, 4, 9]
    assert wr.factor_of(2048, 2048, 512) == 4 and wr.factor_of(2124, 2056, 512) == 5 and wr.factor_of(8192, 1, 16) == 512


def test_normalise_is_the_reciprocal_product():
    v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, 2)
    x = wr.normalise(v)
    assert x.dtype == np.float32 and x.shape == (3, 1, 256) and x[0, 0, 0] == -1.0 and x[0, 0, 255] == 1.0
    assert np.array_equal(x[1, 0], (np.arange(256, dtype=np.float32) * (np.float32(1) / np.float32(127.5))).astype(np.float32) - np.float32(1))


# ------------------------------------------------------------------------------------------------ locate / boxes
def test_boxes_shift_or_centre_as_specified():
    sizes = [(100, 200), (100, 200), (100, 200), (30, 200), (30, 31), (48, 48)]
    centres = [(50, 100), (3, 190), (99, 0), (10, 100), (2, 30), (0, 47)]
    got = wholephoto.boxes(np.array(centres), np.array(sizes), 48)
    assert got.dtype == np.int32 and got.tolist() == [[76, 26, 48], [152, 0, 48], [0, 52, 48], [76, -9, 48], [-8, -9, 48], [0, 0, 48]]
    assert np.array_equal(got, wr.boxes(centres, sizes, 48))
    odd = wholephoto.boxes(np.array([(50, 100)]), np.array([(100, 200)]), 25)
    assert odd.tolist() == [[88, 38, 25]] and np.array_equal(odd, wr.boxes([(50, 100)], [(100, 200)], 25))


def test_centre_formula():
    assert wr.centre([4, 10, 22], 5, 100, 200) == (5 * (20 + 4) // 8, 5 * (44 + 4) // 8, 1) == (15, 30, 1)
    assert wr.centre([0, 0, 0], 5, 101, 200) == (50, 100, 0)
    assert wr.centre([1, 0, 0], 1, 9, 9) == (0, 0, 1) and wr.centre([1, 0, 0], 4, 9, 9) == (2, 2, 1)        # pixel centre 0.5 * f


def test_photo_pool_and_host_checks():
    photos = wr.random_photos(1, [(5, 7), (1, 1), (3, 2)])
    pool = ops.PhotoPool(photos, "cpu")
    assert len(pool) == 3 and pool.sizes_host.tolist() == [[5, 7], [1, 1], [3, 2]] and pool.offsets.tolist() == [0, 35, 36]
    assert pool.pool.dtype == torch.uint8 and pool.pool.numel() == 3 * 42 and pool.sizes.dtype == torch.int32 and pool.offsets.dtype == torch.int64
    assert np.array_equal(pool.pool[35 * 3:36 * 3].numpy(), photos[1].reshape(-1))
    with pytest.raises(ValueError, match="PhotoPool"):
        ops.PhotoPool([np.zeros((4, 4), np.uint8)], "cpu")
    with pytest.raises(ValueError, match="at least one"):
        ops.PhotoPool([], "cpu")
    for bad in ([[0, 0, 7]], [[0, 0, 41]]):
        with pytest.raises(ValueError, match="8..2.5"):
            ops._check_boxes(torch.tensor(bad, dtype=torch.int32), 1, 16, "roi_cut")
    assert ops._check_boxes(torch.tensor([[0, 0, 40], [-5, 3, 8]]), 2, 16, "roi_cut").dtype == torch.int32
    with pytest.raises(ValueError, match=r"\[2, 3\]"):
        ops._check_boxes(torch.zeros(3, 3, dtype=torch.int32), 2, 16, "roi_cut")


# ------------------------------------------------------------------------------------------------ header, parser
def test_header_declares_the_three_entries_and_symbols_list_them():
    from uda_clr_amd.kernels import SYMBOLS
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    for name, nargs in (("uda_photo_reduce_u8", 12), ("uda_roi_cut_u8", 12), ("uda_roi_paste_u8", 9)):
        assert re.search(r"\bint %s\(" % name, txt) and name in SYMBOLS and len(SYMBOLS[name][1]) == nargs
    assert "fundus_dataloader.py:41" in txt and "Image.BILINEAR" in txt
    src = open(os.path.join(ROOT, "uda_clr_amd", "csrc", "geometry.hip")).read() + open(os.path.join(ROOT, "uda_clr_amd", "csrc", "wholephoto.hip")).read()
    assert src.count('#include "pil_resample.h"') == 2 and "precompute" not in src.replace("precompute_coeffs", "")       # one copy of the coefficient code


def test_parser_has_the_four_options():
    ap = predict.build_parser()
    a = ap.parse_args(["--images", "i", "--out", "o"])
    assert (a.whole_photo, a.roi_size, a.locator_checkpoint, a.centres) == (False, 800, None, None)
    a = ap.parse_args(["--images", "i", "--out", "o", "--whole-photo", "--roi-size", "640", "--locator-checkpoint", "l.pth", "--centres", "c.csv"])
    assert (a.whole_photo, a.roi_size, a.locator_checkpoint, a.centres) == (True, 640, "l.pth", "c.csv")


def test_without_whole_photo_an_odd_sized_image_is_still_refused(tmp_path):
    Image.fromarray(np.zeros((70, 150, 3), np.uint8)).save(tmp_path / "odd.png")
    with pytest.raises(ValueError, match="odd.png"):
        predict.main(["--images", str(tmp_path), "--out", str(tmp_path / "out"), "--checkpoint", "unused"])
    with pytest.raises(ValueError, match="odd.png"):
        predict.read_images(str(tmp_path), ["odd.png"])
    assert predict.read_images(str(tmp_path), ["odd.png"], any_size=True)[0][1].shape == (70, 150, 3)


def test_centres_csv_and_the_row_columns(tmp_path):
    (tmp_path / "c.csv").write_text("img_name,cx,cy\na.png,10,20\nb.png,31.6,2\n")
    assert predict.read_centres(str(tmp_path / "c.csv")) == {"a.png": (10, 20), "b.png": (32, 2)}
    rows = [{"img_name": "a.png", "vcdr_pred": 0.5, "roi_x0": 1, "roi_y0": 2, "roi_size": 48, "located": 1, "disc_cx": 3.5, "disc_cy": float("nan")}]
    predict.write_csv(str(tmp_path / "r.csv"), rows)
    assert (tmp_path / "r.csv").read_text().splitlines()[0] == "img_name,vcdr_pred," + ",".join(predict.WHOLE_PHOTO_COLUMNS)
    assert set(wholephoto.PIXEL_COLUMNS) <= set(predict.MORPHOMETRY_COLUMNS)
    with pytest.raises(ValueError, match="roi_size"):
        wholephoto.predict_photos(None, [], str(tmp_path), roi_size=1300, size=512)
    with pytest.raises(ValueError, match="no centre"):
        wholephoto.predict_photos(None, [("x.png", np.zeros((4, 4, 3), np.uint8))], str(tmp_path), roi_size=48, size=32, centres={})


# ------------------------------------------------------------------------------------------------ the restated pipeline end to end
@pytest.mark.parametrize("k", range(len(wr.DRAWN)))
def test_restated_pipeline_finds_the_drawn_disc(k):
    """what tests/test_wholephoto_gpu.py asks of predict --whole-photo holds for the restatement it compares with"""
    shape, centre, radius = wr.DRAWN[k]
    out = wr.restated_pipeline(wr.draw_photo(shape, centre, radius))
    f = wr.factor_of(shape[0], shape[1], wr.E2E_SIZE)
    x0, y0, R = (int(v) for v in out["box"])
    assert out["located"] == 1 and R == wr.E2E_ROI and 0 <= x0 <= shape[1] - R and 0 <= y0 <= shape[0] - R
    assert x0 <= centre[1] - radius and centre[1] + radius < x0 + R and y0 <= centre[0] - radius and centre[0] + radius < y0 + R
    assert abs(out["disc_cx"] - (centre[1] + 0.5)) <= f and abs(out["disc_cy"] - (centre[0] + 0.5)) <= f
    g = out["photo_mask"]
    assert g.shape == shape and set(np.unique(g).tolist()) == {0, 128, 255} and (g[:y0] == 255).all() and (g[:, :x0] == 255).all()
    again = wr.restated_pipeline(wr.draw_photo(shape, centre, radius), centre_xy=(out["centre"][1], out["centre"][0]))
    assert np.array_equal(again["box"], out["box"]) and np.array_equal(again["photo_mask"], g)


def test_restated_pipeline_on_a_black_photograph():
    out = wr.restated_pipeline(np.zeros((50, 90, 3), np.uint8))
    assert out["located"] == 0 and out["box"].tolist() == [21, 1, 48] and (out["photo_mask"] == 255).all() and np.isnan(out["disc_cx"])
