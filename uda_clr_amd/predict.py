"""Run a trained generator on a folder of fundus images that have no ground-truth masks.

Every image file of ``--images`` is read with PIL, normalised as ``Normalize_tf`` normalises the image (v / 127.5 - 1) and batched
with the images of its own size; per batch forward -> sigmoid -> ``postprocessing_batch`` -> pictures, all on the device:

    <out>/overlay/<stem>.png          outlines of the display masks over the image (utils/Utils.py:515-585; disc green, cup blue)
    <out>/original_image/<stem>.png   the image as it was fed
    <out>/mask/<stem>.png             the evaluation mask, BEAL grey coding: 0 = cup, 128 = disc only, 255 = background
    --csv FILE                        img_name, vcdr_pred: the predicted vertical cup-to-disc ratio (cup rows / disc rows, nan without a disc)

An image whose height or width is not a multiple of 16 is refused by name: the generator takes no other size and no padding is invented.
With ``--whole-photo`` the files are whole fundus photographs of any size instead (``uda_clr_amd.wholephoto``): per photograph the disc is
located on a coarse canvas, a ``--roi-size`` window around it is cut and resampled to 512 x 512 as Pillow would, the steps above run on
that ROI, and <out>/photo_mask/<stem>.png is the mask at the photograph's size; the CSV also carries roi_x0, roi_y0, roi_size, located,
disc_cx, disc_cy.  ``--locator-checkpoint`` names a second generator for the coarse stage, ``--centres`` a CSV (img_name, cx, cy) that
replaces it.

    python -m uda_clr_amd.predict --images DIR --checkpoint FILE --out DIR [--backbone mobilenet] [--out-stride 16] [--use_TN]
                                  [--dataset Drishti-GS] [--threshold 0.75] [--batch-size 8] [--csv FILE] [--morphometry [--sectors 72]]
                                  [--mc-passes 8] [--tta flips,id@0.75,id@1.25 [--tta-uncertainty]]
                                  [--whole-photo [--roi-size 800] [--locator-checkpoint FILE] [--centres CSV]]

With ``--morphometry`` the CSV also carries, per image, hcdr_pred and acdr_pred (horizontal and area cup-to-disc ratio), rdr_min_pred and
rim_{up,left,down,right}_pred (thinnest and per-quadrant rim-to-disc ratio), cup_offset_pred (pixels) and {cup,disc}_{major,minor,
orientation} (ellipse axes in pixels, degrees counter-clockwise from "right"); without it the CSV is img_name, vcdr_pred.

With ``--mc-passes T`` (2..32) every batch also runs T MC-dropout passes (``DeepLab.mc_inference_logits``: running statistics, live
dropout) and ``ops.mc_uncertainty``: <out>/uncertainty/<stem>.png is RGB (0, disc, cup) of min(255, floor(std * 1600)) of the std over
the passes of sigmoid(x / 2) - the quantity the trainer trusts a pseudo-label below 0.04 of, grey 64 here - and the CSV carries
cup_unsure, disc_unsure (the share of the predicted structure's pixels with std >= 0.04, nan for an empty structure) and unsure_px
(those pixels counted, cup plane plus disc plane).

With ``--tta SPEC`` every batch is predicted under the views of SPEC (``uda_clr_amd.tta``: mirrorings, quarter turns, scales) and the mean
over the views, mapped back to the image's frame, is what the masks, pictures and figures come from; ``--tta-uncertainty`` writes the
uncertainty pictures and the three columns above from the std over the views instead of dropout passes.  With ``--whole-photo`` the views
are those of the cut ROI: the coarse stage that locates the disc stays single-view.
"""
import argparse
import csv
import os
import sys

import numpy as np
import torch

from . import inference, ops
from .engine import check_input_size
from .evaluate import load_generator
from .inference import check_uncertainty_args as check_tta, resolve_mc_logits  # noqa: F401  (their names before they moved)
from .utils import Utils, metrics

EXTENSIONS = (".png", ".jpg", ".jpeg", ".bmp", ".tif", ".tiff")


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m uda_clr_amd.predict", description="Masks, contour pictures and the vertical CDR of a folder of fundus images.")
    ap.add_argument("--images", required=True, metavar="DIR", help="folder of image files (no masks needed)")
    ap.add_argument("--checkpoint", default=None, help="file with a 'model_state_dict'")
    ap.add_argument("--out", required=True, metavar="DIR")
    ap.add_argument("--backbone", default="mobilenet")
    ap.add_argument("--out-stride", type=int, default=16)
    ap.add_argument("--use_TN", action="store_true", help="TransNorm in place of BatchNorm, as the trainers' switch")
    ap.add_argument("--dataset", default="Drishti-GS", help="as utils.Utils.postprocessing: names starting with 'D' threshold cup > 0.1, disc > 0.5")
    ap.add_argument("--threshold", type=float, default=0.75)
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--csv", default=None, metavar="FILE", help="one row per image: img_name, vcdr_pred")
    ap.add_argument("--morphometry", action="store_true", help="the CSV also gets horizontal and area CDR, rim profile figures, cup offset, ellipse axes")
    ap.add_argument("--sectors", type=int, default=72, metavar="K", help="sectors of the rim profile: a multiple of 8 in 8..360")
    ap.add_argument("--mc-passes", type=int, default=0, metavar="T",
                    help="MC-dropout passes (2..32): writes uncertainty/ pictures, the CSV also gets cup_unsure, disc_unsure, unsure_px")
    ap.add_argument("--tta", default=None, metavar="SPEC",
                    help="test-time augmentation: views id hflip vflip rot180 transpose rot90 rot270 antitranspose, flips, d4, each optionally @scale, "
                         "e.g. flips,id@0.75,id@1.25; masks and pictures come from the mean over the views")
    ap.add_argument("--tta-uncertainty", action="store_true",
                    help="with --tta: uncertainty/ pictures and cup_unsure, disc_unsure, unsure_px from the std over the views")
    ap.add_argument("--whole-photo", action="store_true",
                    help="the files are whole photographs of any size: locate the disc, cut a --roi-size window, predict on it, paste the mask back")
    ap.add_argument("--roi-size", type=int, default=800, metavar="R",
                    help="side of the window cut around the disc, in photograph pixels (8..1280; 800 is the convention of the public ROI releases)")
    ap.add_argument("--locator-checkpoint", default=None, metavar="FILE", help="a second generator for the coarse stage (default: the same one)")
    ap.add_argument("--centres", default=None, metavar="CSV", help="img_name, cx, cy in photograph pixels: skips the coarse stage")
    return ap


def list_images(folder):
    names = sorted(n for n in os.listdir(folder) if n.lower().endswith(EXTENSIONS))
    if not names:
        raise SystemExit("no image files under %s" % folder)
    return names


def read_images(folder, names, any_size=False):
    """-> [(name, uint8 [H,W,3])], every size checked before anything runs (``any_size``: whole photographs, no check)"""
    from PIL import Image
    out = []
    for name in names:
        with Image.open(os.path.join(folder, name)) as im:
            a = np.ascontiguousarray(np.asarray(im.convert("RGB"), dtype=np.uint8))
        if not any_size:
            try:
                check_input_size(a.shape[0], a.shape[1])
            except ValueError as e:
                raise ValueError("%s: %s" % (name, e)) from None
        out.append((name, a))
    return out


def batches(images, batch_size):
    """images of one size together, in the order of their first image, at most ``batch_size`` each: [(names, uint8 [B,H,W,3])]"""
    groups = {}
    for name, a in images:
        groups.setdefault(a.shape, []).append((name, a))
    out = []
    for group in groups.values():
        for i in range(0, len(group), batch_size):
            part = group[i:i + batch_size]
            out.append(([n for n, _ in part], np.stack([a for _, a in part])))
    return out


MORPHOMETRY_COLUMNS = ("hcdr_pred", "acdr_pred", "rdr_min_pred", "rim_up_pred", "rim_left_pred", "rim_down_pred", "rim_right_pred",
                       "cup_offset_pred") + tuple("%s_%s" % (c, x) for c in ("cup", "disc") for x in ("major", "minor", "orientation"))


def morphometry_columns(pred, sectors=72):
    """{name: [B] float64} of MORPHOMETRY_COLUMNS for [B,2,H,W] predicted masks: one ``ops.disc_morphometry`` call and its closed forms"""
    f = metrics.morphometry_from_moments(ops.disc_morphometry(pred, sectors))
    cols = {x + "_pred": f[x] for x in ("hcdr", "acdr", "rdr_min", "rim_up", "rim_left", "rim_down", "rim_right")}
    cols["cup_offset_pred"] = np.hypot(f["cup_offset"][:, 0], f["cup_offset"][:, 1])
    for k, c in enumerate(("cup", "disc")):
        for x in ("major", "minor", "orientation"):
            cols["%s_%s" % (c, x)] = f[x][:, k]
    return cols


UNCERTAINTY_COLUMNS = ("cup_unsure", "disc_unsure", "unsure_px")
UNSURE_STD = 0.04               # the trainer's trust threshold on the std of sigmoid(x / 2) (reference utils/Utils.py:197-200)


def uncertainty_columns(unc, pred):
    """{name: [B] float64} of UNCERTAINTY_COLUMNS for the [B,2,H,W] std map and predicted masks: one ``ops.selective_tables`` call with
    the prediction as its own ground truth, so that the TP column counts the predicted structure's pixels per uncertainty bin"""
    edges = ops.DEFAULT_UNC_EDGES
    tp = ops.selective_tables(None, unc, pred, None, edges=edges)["risk"][..., 0]
    first = [float(np.float32(e)) for e in edges].index(float(np.float32(UNSURE_STD))) + 1         # the first bin with std >= 0.04
    unsure, n = tp[..., first:].sum(-1), tp.sum(-1)
    share = metrics._ratio(unsure, n)
    return {"cup_unsure": share[:, 0], "disc_unsure": share[:, 1], "unsure_px": unsure.sum(-1).astype(np.float64)}


def predict_batch(model, u8, x, names, out_dir, dataset="Drishti-GS", threshold=0.75, morphometry=False, sectors=72, mc_passes=0, mc_logits=None,
                  tta=None, tta_uncertainty=False):
    """The per-batch body that ``predict`` and ``wholephoto.predict_photos`` share: ``u8`` uint8 [B,H,W,3] and ``x`` f32 [B,3,H,W] (its
    normalised form) on the device -> (rows, pred): forward -> sigmoid -> ``postprocessing_batch``, the three folders written, one
    row per image as ``predict`` documents them, and the uint8 [B,2,H,W] evaluation masks on the device.  With ``tta`` (a view list,
    ``uda_clr_amd.tta``) the probabilities are the mean over the views, and with ``tta_uncertainty`` the std over the views fills the
    uncertainty picture and columns."""
    prob, unc = inference.probabilities(model, x, tta, tta_uncertainty, mc_passes, mc_logits, std_u8=True)
    pred = Utils.postprocessing_batch(prob, threshold, dataset)
    Utils.save_per_img_batch(u8, out_dir, names, prob)
    Utils.save_mask_batch(pred, out_dir, names)
    # the prediction as both masks: slot 1 of 'extent' is the prediction's first and last row per class
    profile = ops.surface_profile(pred, pred, percentiles=(), tolerances=())[2]
    vcdr = metrics.vertical_cdr_from_profile(profile)["vcdr_pred"]
    rows = [{"img_name": n, "vcdr_pred": float(v)} for n, v in zip(names, vcdr)]
    if morphometry:
        cols = morphometry_columns(pred, sectors)
        for i in range(len(names)):
            rows[i].update({k: float(cols[k][i]) for k in MORPHOMETRY_COLUMNS})
    if unc is not None:
        Utils.save_uncertainty_batch(unc["std_u8"], out_dir, names)
        cols = uncertainty_columns(unc["std"], pred)
        for i in range(len(names)):
            rows[i].update({k: float(cols[k][i]) for k in UNCERTAINTY_COLUMNS})
    return rows, pred


def predict(model, images, out_dir, dataset="Drishti-GS", threshold=0.75, batch_size=8, morphometry=False, sectors=72, mc_passes=0,
            mc_logits=None, tta=None, tta_uncertainty=False):
    """``images`` as ``read_images`` returns them -> [{'img_name', 'vcdr_pred'}] in batch order; writes the three folders.
    ``morphometry``: every row also carries MORPHOMETRY_COLUMNS (horizontal and area cup-to-disc ratio, the thinnest rim-to-disc ratio
    of ``sectors`` sectors and its quadrant means, the cup's decentration in pixels, full axes in pixels and orientation in degrees of
    the ellipse with each structure's covariance), from one ``ops.disc_morphometry`` call per batch.
    ``mc_passes`` T in 2..32: per batch T stochastic passes (``mc_logits(x, T)`` -> [T,B,2,H,W] logits; default
    ``model.mc_inference_logits``), ``ops.mc_uncertainty`` and one ``ops.selective_tables`` call; writes uncertainty/<stem>.png and
    every row also carries UNCERTAINTY_COLUMNS.  0 (the default) makes no pass and no call.
    ``tta`` a view list (a string such as 'flips,id@0.75' or a list of (g, h, w), ``uda_clr_amd.tta``): the masks and pictures come from
    the mean over the views; ``tta_uncertainty`` (needs ``tta``, excludes ``mc_passes``): uncertainty/<stem>.png and UNCERTAINTY_COLUMNS
    from the std over the views."""
    check_tta(tta, tta_uncertainty, mc_passes)
    if not torch.cuda.is_available():
        raise RuntimeError("uda_clr_amd computes only on the MI355X HIP kernels (there is no CPU fallback)")
    mc_passes = int(mc_passes)
    mc_logits = resolve_mc_logits(model, mc_passes, mc_logits)
    dev = torch.device("cuda")
    rows = []
    with inference.eval_mode(model):
        for names, u8 in batches(images, batch_size):
            u8 = torch.from_numpy(u8).to(dev)
            x = (u8.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()              # Normalize_tf's image, ToTensor's layout
            rows += predict_batch(model, u8, x, names, out_dir, dataset, threshold, morphometry, sectors, mc_passes, mc_logits,
                                  tta, tta_uncertainty)[0]
    return rows


WHOLE_PHOTO_COLUMNS = ("roi_x0", "roi_y0", "roi_size", "located", "disc_cx", "disc_cy")


def write_csv(path, rows):
    """img_name, vcdr_pred, and MORPHOMETRY_COLUMNS, UNCERTAINTY_COLUMNS and WHOLE_PHOTO_COLUMNS where the rows carry them"""
    more = MORPHOMETRY_COLUMNS if rows and MORPHOMETRY_COLUMNS[0] in rows[0] else ()
    more += UNCERTAINTY_COLUMNS if rows and UNCERTAINTY_COLUMNS[0] in rows[0] else ()
    more += WHOLE_PHOTO_COLUMNS if rows and WHOLE_PHOTO_COLUMNS[0] in rows[0] else ()
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("img_name", "vcdr_pred") + more)
        for r in rows:
            w.writerow([r["img_name"], repr(r["vcdr_pred"])] + [repr(r[k]) for k in more])


def read_centres(path):
    """--centres: a CSV with the columns img_name, cx, cy (photograph pixels) -> {img_name: (cx, cy)}"""
    with open(path, newline="") as f:
        return {r["img_name"]: (int(round(float(r["cx"]))), int(round(float(r["cy"])))) for r in csv.DictReader(f)}


def main(argv=None, model=None, mc_logits=None, locator=None, size=512):
    """The command line.  ``model``: a callable to run instead of the checkpoint's DeepLab, ``mc_logits``: its stochastic passes,
    ``locator``: a callable for the coarse stage of --whole-photo instead of --locator-checkpoint's DeepLab, ``size``: the input side
    that --whole-photo resamples canvas and ROI to, for a generator that takes another one than the data sets' 512 (tests)."""
    args = build_parser().parse_args(argv)
    images = read_images(args.images, list_images(args.images), any_size=args.whole_photo)
    if model is None:
        if not args.checkpoint:
            raise SystemExit("--checkpoint is required")
        model = load_generator(args.checkpoint, args.backbone, args.out_stride, args.use_TN,
                               torch.device("cuda") if torch.cuda.is_available() else None)
    options = dict(dataset=args.dataset, threshold=args.threshold, batch_size=args.batch_size, morphometry=args.morphometry, sectors=args.sectors,
                   mc_passes=args.mc_passes, mc_logits=mc_logits, tta=args.tta, tta_uncertainty=args.tta_uncertainty)
    if args.whole_photo:
        from . import wholephoto
        if locator is None and args.locator_checkpoint:
            locator = load_generator(args.locator_checkpoint, args.backbone, args.out_stride, args.use_TN,
                                     torch.device("cuda") if torch.cuda.is_available() else None)
        rows = wholephoto.predict_photos(model, images, args.out, roi_size=args.roi_size, size=size, locator=locator,
                                         centres=read_centres(args.centres) if args.centres else None, **options)
    else:
        rows = predict(model, images, args.out, **options)
    print("%d images -> %s" % (len(rows), args.out))
    if args.csv:
        write_csv(args.csv, rows)
    return rows


if __name__ == "__main__":
    main(sys.argv[1:])
