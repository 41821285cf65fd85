"""Prediction on whole fundus photographs: locate the disc, cut the ROI, predict, paste the masks back.

The training sets ship pre-cut, disc-centred ROIs (``ROIs/image``, dataloaders/fundus_dataloader.py:41) and the reference has no code
for the step that made them; a photograph as the camera gives it (2124 x 2056, 2896 x 1944, 1634 x 1634, the disc anywhere) is what
``predict_photos`` takes.  Per batch of photographs, one upload:

    ops.photo_reduce    the photograph reduced by an integer factor onto a size x size canvas               (uda_photo_reduce_u8)
    locate              a generator on the canvas -> the disc's centroid, in photograph pixels, in integers
    boxes               a roi_size window around it, shifted into the photograph
    ops.roi_cut         the window resampled to size x size, byte for byte as Pillow's crop().resize(BILINEAR) (uda_roi_cut_u8)
    predict.predict_batch   the pipeline of ``predict`` on that ROI, unchanged
    ops.roi_paste       the masks back into a photograph-sized grey mask                                   (uda_roi_paste_u8)

Every definition here is this project's; only the ROI resample is Pillow's, so that the generator sees what a Pillow-made ROI would give
it.  The 800-pixel window is the convention of the public ROI releases of these data sets, not a number from the reference (its scripts
only say "images ROIs"): it is a parameter.
"""
import os

import numpy as np
import torch

from . import inference, ops, predict
from .kernels import check_side
from .utils import Utils

# morphometry columns of ``predict`` that are lengths in ROI pixels: multiplied by roi_size / size to read in photograph pixels
PIXEL_COLUMNS = ("cup_offset_pred", "cup_major", "cup_minor", "disc_major", "disc_minor")


def locate(canvas_f32, factor, sizes, locator, threshold=0.75, dataset="Drishti-GS"):
    """The disc's centre per photograph from the coarse canvas: ``locator`` (a generator) forward -> sigmoid ->
    ``Utils.postprocessing_batch`` -> the moments (n, sum r, sum c) of the disc plane (``ops.disc_morphometry``); the centroid of the
    pixel centres, scaled by the factor f, in integers:
        cy = f * (2 sum r + n) // (2 n)        cx = f * (2 sum c + n) // (2 n)
    ``canvas_f32`` [B,3,S,S] and ``factor`` [B] as ``ops.photo_reduce`` gives them, ``sizes`` host [B,2] = (H, W).
    -> (centres int64 [B,2] = (cy, cx), located int64 [B]) on the host; an empty disc plane gives located 0 and the photograph's
    centre (H // 2, W // 2)."""
    pred = Utils.postprocessing_batch(inference.probabilities(locator, canvas_f32)[0], threshold, dataset)
    mom = ops.disc_morphometry(pred, 8)["moments"][:, 1, :3]
    f = np.asarray(factor.cpu() if torch.is_tensor(factor) else factor).astype(np.int64).reshape(-1)
    sizes = np.asarray(sizes, np.int64).reshape(-1, 2)
    centres, located = np.empty((len(f), 2), np.int64), np.zeros(len(f), np.int64)
    for b in range(len(f)):
        n, sr, sc = (int(v) for v in mom[b])
        if n == 0:
            centres[b] = (sizes[b, 0] // 2, sizes[b, 1] // 2)
        else:
            centres[b] = (int(f[b]) * (2 * sr + n) // (2 * n), int(f[b]) * (2 * sc + n) // (2 * n))
            located[b] = 1
    return centres, located


def _box_axis(c, length, roi_size):
    if length >= roi_size:
        return min(max(c - roi_size // 2, 0), length - roi_size)        # shifted into the photograph
    return -((roi_size - length) // 2)                                  # the photograph centred in the window


def boxes(centres, sizes, roi_size):
    """centres [B,2] = (cy, cx) and sizes [B,2] = (H, W) -> int32 [B,3] = (x0, y0, R): x0 = cx - R // 2, y0 = cy - R // 2; per axis the
    window is shifted into the photograph when the photograph is at least R long, otherwise the photograph is centred in the window
    (first position -((R - length) // 2))."""
    R = int(roi_size)
    return np.array([[_box_axis(int(cx), int(W), R), _box_axis(int(cy), int(H), R), R]
                     for (cy, cx), (H, W) in zip(np.asarray(centres), np.asarray(sizes))], np.int32).reshape(-1, 3)


def predict_photos(model, photos, out_dir, roi_size=800, size=512, locator=None, centres=None, dataset="Drishti-GS", threshold=0.75,
                   batch_size=8, morphometry=False, sectors=72, mc_passes=0, mc_logits=None, tta=None, tta_uncertainty=False):
    """``photos`` [(name, uint8 [H,W,3])] of any sizes -> the rows of ``predict.predict`` on each photograph's ROI, in order, and
    its folders at ROI scale (overlay/, original_image/, mask/, uncertainty/), plus <out_dir>/photo_mask/<stem>.png: the grey mask at
    the photograph's size (0 cup, 128 disc only, 255 elsewhere).
        roi_size  R, side of the window in photograph pixels, 8 <= R <= 2.5 * size        size  the generator's input side
        locator   the generator of the coarse stage (default: ``model``)
        centres   {name: (cx, cy)} in photograph pixels: the coarse stage is skipped (located = 1)
        tta, tta_uncertainty   as ``predict.predict``: the views are those of the cut ROI; the coarse stage stays single-view
    Every row also carries roi_x0, roi_y0, roi_size, located (1: the coarse stage found a disc; 0: the window sits on the photograph's
    centre) and disc_cx, disc_cy: the centroid of the final disc mask in photograph pixels, x0 + (mean column + 0.5) * R / size (nan
    without a disc); the morphometry columns that are lengths in pixels (PIXEL_COLUMNS) are multiplied by R / size."""
    R, S = int(roi_size), int(size)
    check_side("size", S)
    if R < 8 or 2 * R > 5 * S:
        raise ValueError("roi_size must lie in 8..2.5 * size = %d, got %d" % (5 * S // 2, R))
    if centres is not None:
        missing = [n for n, _ in photos if n not in centres]
        if missing:
            raise ValueError("no centre given for %s" % ", ".join(missing[:5]))
    if not torch.cuda.is_available():
        raise RuntimeError("uda_clr_amd computes only on the MI355X HIP kernels (there is no CPU fallback)")
    mc_passes = int(mc_passes)
    inference.check_uncertainty_args(tta, tta_uncertainty, mc_passes)
    mc_logits = inference.resolve_mc_logits(model, mc_passes, mc_logits)
    locator = model if locator is None else locator
    dev = torch.device("cuda")
    rows = []
    with inference.eval_mode(model, locator):
        for i in range(0, len(photos), int(batch_size)):
            part = photos[i:i + int(batch_size)]
            names = [n for n, _ in part]
            pool = ops.PhotoPool([a for _, a in part], dev)                          # the one upload
            if centres is None:
                red = ops.photo_reduce(pool, size=S, outputs=("f32",))
                cen, located = locate(red["f32"], red["factor"], pool.sizes_host, locator, threshold, dataset)
            else:
                cen = np.array([(centres[n][1], centres[n][0]) for n in names], np.int64)
                located = np.ones(len(names), np.int64)
            bx = boxes(cen, pool.sizes_host, R)
            roi = ops.roi_cut(pool, torch.from_numpy(bx), size=S, outputs=("u8", "f32"))
            part_rows, pred = predict.predict_batch(model, roi["u8"], roi["f32"], names, out_dir, dataset, threshold, morphometry, sectors,
                                                    mc_passes, mc_logits, tta, tta_uncertainty)
            masks = ops.roi_paste(pool, pred, torch.from_numpy(bx))
            host = torch.cat([m.reshape(-1) for m in masks]).cpu().numpy()         # the one copy of the photograph-sized masks
            mom = ops.disc_morphometry(pred, 8)["moments"][:, 1, :3]
            at = 0
            for b, (name, row) in enumerate(zip(names, part_rows)):
                H, W = (int(v) for v in pool.sizes_host[b])
                Utils._save_png(host[at:at + H * W].reshape(H, W), os.path.join(out_dir, "photo_mask"), name)
                at += H * W
                n, sr, sc = (int(v) for v in mom[b])
                row.update({"roi_x0": int(bx[b, 0]), "roi_y0": int(bx[b, 1]), "roi_size": R, "located": int(located[b]),
                            "disc_cx": bx[b, 0] + (sc / n + 0.5) * R / S if n else float("nan"),
                            "disc_cy": bx[b, 1] + (sr / n + 0.5) * R / S if n else float("nan")})
                for k in PIXEL_COLUMNS:
                    if k in row:
                        row[k] = row[k] * R / S
            rows += part_rows
    return rows
