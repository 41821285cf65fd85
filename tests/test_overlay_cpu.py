"""not-gpu: the numpy / scipy statement of the prediction pictures (tests/overlay_ref.py) against independent marching squares, against
a restatement of the reference's painting lines (utils/Utils.py:564-580), the two claims the kernel chain of uda_display_masks rests
on, the grey-level facts of the byte image, and the declarations of the new entries."""
import inspect
import os
import re

import numpy as np
import pytest

import overlay_ref as ovr
import postproc_shapes as shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTOUR_SHAPES = ((9, 13), (33, 17), (2, 2), (2, 9))


def _random_masks():
    rng = np.random.default_rng(11)
    for H, W in CONTOUR_SHAPES:
        for density in (0.2, 0.5, 0.8):
            for _ in range(4):
                yield (rng.random((H, W)) < density).astype(np.uint8)


def _as_set(points):
    return set(map(tuple, np.asarray(points, np.float64).reshape(-1, 2).tolist()))


def test_vertices_are_contourpy_s_marching_squares_vertices():
    contourpy = pytest.importorskip("contourpy")
    n = 0
    for m in _random_masks():
        gen = contourpy.contour_generator(z=m.astype(np.float64), name="serial", line_type=contourpy.LineType.Separate)
        lines = gen.lines(0.5)                                        # [(x, y)] = (column, row)
        theirs = _as_set(np.concatenate([l[:, ::-1] for l in lines])) if lines else set()
        assert _as_set(ovr.vertices(m)) == theirs, m
        n += len(theirs)
    assert n > 500                                                    # the comparison was not one of empty sets


def test_vertices_are_skimage_s_find_contours_vertices():
    measure = pytest.importorskip("skimage.measure")
    for m in _random_masks():
        contours = measure.find_contours(m, 0.5)
        theirs = _as_set(np.concatenate(contours)) if contours else set()
        assert _as_set(ovr.vertices(m)) == theirs, m


def _paint_as_the_reference(patch_image, contours, colour):
    """the seven assignments of utils/Utils.py:565-571 (and :574-580) per contour, numpy's own indexing: -1 wraps, H or W raises"""
    for contour in contours:
        for dy, dx in ovr.OFFSETS:
            patch_image[(contour[:, 0] + float(dy)).astype(int), (contour[:, 1] + float(dx)).astype(int), :] = colour


def _reference_picture(image, masks):
    out = image.copy()
    _paint_as_the_reference(out, [ovr.vertices(masks[1])], ovr.GREEN)         # its contours_cup = prob_map[1]: this project's channel 1
    _paint_as_the_reference(out, [ovr.vertices(masks[0])], ovr.BLUE)          # its contours_disc = prob_map[0]: channel 0, painted over
    return out


def test_paint_equals_the_reference_s_lines_on_masks_clear_of_the_border_ring():
    rng = np.random.default_rng(5)
    for H, W in ((9, 13), (33, 17), (40, 40), (3, 3), (4, 7)):
        for _ in range(4):
            masks = np.zeros((2, H, W), np.uint8)
            masks[:, 1:-1, 1:-1] = rng.random((2, H - 2, W - 2)) < 0.4
            image = ovr.random_image(1, H, W, seed=H * W)[0]
            keep = image.copy()
            for c in range(2):
                assert ovr.paint(image.copy(), masks[c], ovr.BLUE).shape == (0, 2)           # nothing dropped
            assert np.array_equal(ovr.overlay(image, masks), _reference_picture(image, masks))
            assert np.array_equal(image, keep)
    for name, m in ovr.hand_masks():
        if m.shape[1] > 2 and m.shape[2] > 2 and not (m[:, 0].any() or m[:, -1].any() or m[:, :, 0].any() or m[:, :, -1].any()):
            image = ovr.random_image(1, m.shape[1], m.shape[2], seed=3)[0]
            assert np.array_equal(ovr.overlay(image, m), _reference_picture(image, m)), name


def test_dropped_targets_are_exactly_those_at_minus_one_h_or_w():
    rng = np.random.default_rng(6)
    cases = [(rng.random((H, W)) < 0.5).astype(np.uint8) for H, W in ((9, 13), (2, 2), (2, 9), (1, 6), (6, 1), (33, 17)) for _ in range(3)]
    cases += [m[c] for _, m in ovr.hand_masks() for c in range(2)]
    n_dropped = 0
    for m in cases:
        H, W = m.shape
        t = ovr.targets(ovr.vertices(m)).reshape(-1, 2)
        bad = (t[:, 0] == -1) | (t[:, 0] == H) | (t[:, 1] == -1) | (t[:, 1] == W)
        assert t[:, 0].min(initial=0) >= -1 and t[:, 0].max(initial=0) <= H and t[:, 1].min(initial=0) >= -1 and t[:, 1].max(initial=0) <= W
        image = np.full((H, W, 3), 7, np.uint8)
        dropped = ovr.paint(image, m, ovr.GREEN)
        assert _as_set(dropped) == _as_set(t[bad]) and len(dropped) == int(bad.sum())
        # every kept target is painted, nothing else is
        want = np.zeros((H, W), bool)
        want[t[~bad, 0], t[~bad, 1]] = True
        assert np.array_equal((image == np.array(ovr.GREEN, np.uint8)).all(-1), want)
        assert (image[~want] == 7).all()
        n_dropped += len(dropped)
    assert n_dropped > 0
    # a vertex at y = 0.5 with dy = -1 lands on row 0 (truncation towards zero), not on row -1
    assert ovr.targets(np.array([[0.5, 3.0]]))[0, 4].tolist() == [0, 3]


@pytest.fixture(scope="module")
def library_stages():
    return [(name, ovr.display_stages(prob)) for name, prob in ovr.library()]          # postproc_shapes.library() + "tip bay"


def test_the_second_largest_component_step_changes_no_pixel(library_stages):
    for name, st in library_stages:
        assert np.array_equal(st["second_keep"], st["dilated"]), name
        for c in range(2):                                   # and the reason: at most one 8-connected component goes in and comes out
            assert shapes.ndimage.label(st["filled"][c], structure=shapes.FULL)[1] <= 1, name
            assert shapes.ndimage.label(st["dilated"][c], structure=shapes.FULL)[1] <= 1, name


def test_the_second_fill_is_not_a_no_op(library_stages):
    """no shape of postproc_shapes.library() needs it - the diagonal ring's hole is 4-separated from the outside, so the first fill
    takes it - hence overlay_ref.tip_bay: a bay the dilation closes"""
    changed = {name: int((st["display"] != st["second_keep"]).sum()) for name, st in library_stages}
    print("pixels the second fill adds:", {k: v for k, v in changed.items() if v})
    assert changed["tip bay"] > 0
    st = dict(library_stages)["tip bay"]
    assert np.array_equal(st["filled"], shapes.stages(ovr.tip_bay(), 0.75, 0.75)["keep"])          # the first fill added nothing there


def test_display_masks_leave_the_probabilities_alone_and_ignore_the_ring():
    prob = shapes.ones(40, 48)
    keep = prob.copy()
    d = ovr.display_masks(prob)
    assert np.array_equal(prob, keep)
    inner = prob.copy()
    inner[:, 0, :] = inner[:, -1, :] = inner[:, :, 0] = inner[:, :, -1] = 0.0
    assert np.array_equal(d, ovr.display_masks(inner)) and d.any()


def test_rounding_returns_all_256_grey_levels_and_truncation_loses_63():
    x = ovr.normalized_levels()                                               # Normalize_tf's own output, fp32
    assert x.dtype == np.float32
    untransformed = (x + np.float32(1)) * np.float32(127.5)                   # the reference's untransform (utils/Utils.py:587-590), fp32
    assert untransformed.dtype == np.float32
    truncated = untransformed.astype(np.uint8)
    wrong = truncated != np.arange(256)
    assert int(wrong.sum()) == 63                                             # 63 of the 256 levels do not come back ...
    assert np.array_equal(truncated[wrong], np.arange(256)[wrong] - 1)        # ... but as the level below
    back = ovr.image_u8(np.broadcast_to(x[None, None, None, :], (1, 3, 1, 256)))
    assert np.array_equal(back[0, 0, :, 0], np.arange(256)) and np.array_equal(back[0, 0, :, 2], np.arange(256))
    # clipping, and the one exact tie of the range: 127.5 rounds to the even 128
    edge = np.array([-1.5, -1.0, 1.0, 1.5, 0.0], np.float32).reshape(1, 1, 1, 5).repeat(3, 1)
    assert ovr.image_u8(edge)[0, 0, :, 0].tolist() == [0, 0, 255, 255, 128]


def test_grey_mask_coding():
    pred = np.zeros((2, 2, 3), np.uint8)
    pred[1, 0, :] = 1
    pred[0, 0, 0] = 1
    assert ovr.grey_mask(pred).tolist() == [[0, 128, 128], [255, 255, 255]]


def test_the_new_entries_are_declared():
    from uda_clr_amd import evaluate as ev
    from uda_clr_amd.kernels import SYMBOLS, HipKernels
    from uda_clr_amd.utils import Utils
    txt = open(os.path.join(ROOT, "include", "uda_clr_hip.h")).read()
    assert "utils/Utils.py:515-585" in txt
    for name in ("uda_display_masks_workspace_bytes", "uda_display_masks", "uda_overlay_u8", "uda_image_u8"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
        assert name in SYMBOLS
    for name in ("display_masks", "overlay_u8", "image_u8"):
        assert callable(getattr(HipKernels, name))
    sig = inspect.signature(ev.evaluate)
    assert sig.parameters["save_dir"].default is None and list(sig.parameters)[-1] == "save_dir"
    assert ev.build_parser().parse_args(["--data-dir", "d", "--checkpoint", "c", "--save-dir", "out"]).save_dir == "out"
    assert list(inspect.signature(Utils.save_per_img).parameters) == ["patch_image", "data_save_path", "img_name", "prob_map", "mask_path", "ext"]
    from uda_clr_amd import ops, predict
    assert inspect.signature(ops.display_masks).parameters["threshold"].default == 0.75
    assert callable(ops.overlay) and callable(predict.main) and callable(Utils.save_per_img_batch)
