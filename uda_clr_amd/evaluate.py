"""Per-image evaluation in the form of the paper's tables: for every test image, after the evaluation post-processing
(utils/Utils.py:438-463), Dice, average symmetric surface distance and Hausdorff distance of cup and disc.

The forward, ``postprocessing_batch`` and ``ops.surface_distances`` run per batch on the device; the metrics are closed forms
(utils/metrics.py) of the small table that one copy per batch brings to the host.  No per-image device call is made.

On request (``hd95``, ``tolerances``, ``cdr``) the batch goes through ``ops.surface_profile`` instead - the same table and counts plus
the order statistics, tolerance counts and row extents that the 95th-percentile Hausdorff distance, the surface Dice at a tolerance
and the vertical cup-to-disc ratio are closed forms of - still one copy per batch.  ``morphometry`` adds one ``ops.disc_morphometry``
call per batch over the predicted and the true masks together: horizontal and area cup-to-disc ratio, the rim-to-disc profile's
thinnest point and quadrant means, the cup's decentration.

``calibration`` and ``mc_passes`` add one ``ops.selective_tables`` call per batch: the reliability table of the deterministic
probabilities against the labels (ECE, Brier score, reliability diagram) and, from T MC-dropout passes of the same batch
(``DeepLab.mc_inference_logits`` -> ``ops.mc_uncertainty``), the errors of the scored masks per bin of the std of sigmoid(x / 2) - the
quantity the trainer thresholds at 0.04 (reference utils/Utils.py:165-166, :197-200): what share of the pixels that mask keeps, how
clean the kept labels are, and how well the uncertainty ranks the errors (AUROC, risk-coverage curve).

``tta`` scores the mean over several views of the image - mirrorings, quarter turns, a few scales - instead of one forward
(``uda_clr_amd.tta``: ``ops.tta_view``, one forward per distinct view shape, ``ops.tta_fuse``); ``tta_uncertainty`` reads the std over
those views where ``mc_passes`` reads the std over dropout passes.

With ``save_dir`` every image also leaves three PNG files there: ``overlay/`` (the reference's contour picture, utils/Utils.py:515-585),
``original_image/`` and ``mask/`` (the evaluation masks the metrics were computed on, BEAL grey coding).

    python -m uda_clr_amd.evaluate --data-dir DIR --dataset Drishti-GS --checkpoint FILE [--hd95] [--tolerance 2 ...] [--cdr]
                                   [--morphometry [--sectors 72]] [--calibration [--bins 15]] [--mc-passes 8]
                                   [--tta flips,id@0.75,id@1.25 [--tta-uncertainty]]
                                   [--csv per_image.csv] [--json result.json] [--save-dir DIR]
"""
import argparse
import csv
import json
import sys

import numpy as np
import torch

from . import inference, ops
from .inference import UNCERTAINTY_U8_SCALE  # noqa: F401  (``predict`` and the tests take it from here)
from .utils import Utils, metrics

FIELDS = ("cup_dice", "disc_dice", "cup_assd", "disc_assd", "cup_hd", "disc_hd")


def _names(sample, B, seen):
    names = sample.get("img_name") if hasattr(sample, "get") else None
    if names is None:
        return ["%d" % (seen + i) for i in range(B)]
    return [str(n) for n in ([names] if isinstance(names, str) else list(names))]


MORPHOMETRY_FIELDS = tuple("%s_%s" % (x, s) for x in ("hcdr", "acdr", "rdr_min") for s in ("pred", "gt", "error")) + tuple(
    "rim_%s_%s" % (q, s) for q in ("up", "left", "down", "right") for s in ("pred", "gt")) + ("cup_offset_pred",)


CALIBRATION_FIELDS = ("cup_ece", "disc_ece", "cup_brier", "disc_brier")


def uncertainty_fields(report_edges=(0.04,)):
    """names of the per-image figures of ``mc_passes``: the AUROC, then coverage, kept Dice and kept error rate per reported edge"""
    names = ["cup_unc_auroc", "disc_unc_auroc"]
    for e in report_edges:
        names += ["%s_%s_%g" % (c, x, e) for x in ("cov", "dice", "err") for c in ("cup", "disc")]
    return tuple(names)


def extra_fields(hd95=False, tolerances=(), cdr=False, morphometry=False, calibration=False, mc_passes=0, report_edges=(0.04,),
                 tta_uncertainty=False):
    """names of the per-image figures that ``evaluate`` adds for these arguments, in the order of its tables (``tta_uncertainty`` adds
    the names of ``mc_passes``: the same figures from the std over the views)"""
    names = ["cup_hd95", "disc_hd95"] if hd95 else []
    for tau in tolerances:
        names += ["cup_nsd_%g" % tau, "disc_nsd_%g" % tau]
    return (tuple(names + (["vcdr_pred", "vcdr_gt", "cdr_error"] if cdr else [])) + (MORPHOMETRY_FIELDS if morphometry else ()) +
            (CALIBRATION_FIELDS if calibration else ()) + (uncertainty_fields(report_edges) if mc_passes or tta_uncertainty else ()))


def morphometry_columns(pred, gt, sectors=72):
    """{name: [B] float64} of MORPHOMETRY_FIELDS for [B,2,H,W] prediction and ground-truth masks: ONE ``ops.disc_morphometry`` call over
    both, stacked along the batch, and the closed forms of ``metrics.morphometry_from_moments``"""
    B = pred.shape[0]
    f = metrics.morphometry_from_moments(ops.disc_morphometry(torch.cat([ops._mask_u8(pred), ops._mask_u8(gt)]), sectors))
    cols = {}
    for x in ("hcdr", "acdr", "rdr_min"):
        cols[x + "_pred"], cols[x + "_gt"] = f[x][:B], f[x][B:]
        cols[x + "_error"] = np.abs(f[x][:B] - f[x][B:])
    for q in ("up", "left", "down", "right"):
        cols["rim_%s_pred" % q], cols["rim_%s_gt" % q] = f["rim_" + q][:B], f["rim_" + q][B:]
    cols["cup_offset_pred"] = np.hypot(f["cup_offset"][:B, 0], f["cup_offset"][:B, 1])
    return cols


def _edge_index(unc_edges, report_edges):
    """positions of ``report_edges`` in ``unc_edges``, both compared as the float32 values the kernel bins with"""
    have = [float(np.float32(e)) for e in unc_edges]
    try:
        return [have.index(float(np.float32(e))) for e in report_edges]
    except ValueError:
        raise ValueError("report_edges %r must be among unc_edges %r" % (tuple(report_edges), tuple(unc_edges))) from None


def calibration_columns(rel):
    """{name: [B] float64} of CALIBRATION_FIELDS from a [B,2,M,5] reliability table"""
    c = metrics.calibration_from_table(rel)
    return {"cup_ece": c["ece"][:, 0], "disc_ece": c["ece"][:, 1], "cup_brier": c["brier"][:, 0], "disc_brier": c["brier"][:, 1]}


def uncertainty_columns(risk, unc_edges, report_edges=(0.04,)):
    """{name: [B] float64} of ``uncertainty_fields(report_edges)`` from a [B,2,K,4] risk table"""
    s = metrics.selective_from_table(risk, unc_edges)
    cols = {"cup_unc_auroc": s["unc_auroc"][:, 0], "disc_unc_auroc": s["unc_auroc"][:, 1]}
    for e, j in zip(report_edges, _edge_index(unc_edges, report_edges)):
        for x, key in (("cov", "coverage"), ("dice", "dice"), ("err", "error")):
            cols["cup_%s_%g" % (x, e)], cols["disc_%s_%g" % (x, e)] = s[key][:, 0, j], s[key][:, 1, j]
    return cols


def _lists(d):
    """a dict of numpy arrays as nested lists (what ``write_json`` can dump)"""
    return {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()}


def evaluate(model, loader, dataset='G', threshold=0.75, postprocess=True, hd95=False, tolerances=(), cdr=False, morphometry=False,
             sectors=72, calibration=False, bins=15, mc_passes=0, unc_edges=ops.DEFAULT_UNC_EDGES, report_edges=(0.04,), mc_logits=None,
             tta=None, tta_uncertainty=False, save_dir=None):
    """Score ``model`` on every image of ``loader``.

    model       callable whose first output (or only output) is the [B,2,H,W] logits (cup, disc), e.g. ``DeepLab``
    loader      iterable of decoded float batches {'image' [B,3,H,W], 'map' [B,2,H,W], 'img_name'} (UDA_CLR_DEVICE_INPUT unset or 0)
    dataset     as ``utils.Utils.postprocessing``: names starting with 'D' threshold cup > 0.1 and disc > 0.5, others ``threshold``
    postprocess False: the plain thresholds only, without median / erosion / largest component / hole filling

    -> {'per_image': [{'img_name', 'cup_dice', 'disc_dice', 'cup_assd', 'disc_assd', 'cup_hd', 'disc_hd'}, ...],
        'mean': nanmean of each field, 'n_images', 'n_undefined': {'cup', 'disc'}}; distances in pixels.  An (image, class) whose
    predicted or true mask is empty has NaN distances and is counted in ``n_undefined``.

    hd95        True: also 'cup_hd95', 'disc_hd95', the 95th percentile of the distances of both directions pooled (medpy's hd95)
    tolerances  pixel distances tau: also 'cup_nsd_<tau>', 'disc_nsd_<tau>' (tau as %g), the share of both borders' pixels within tau
                of the other border (d2 <= floor(tau^2))
    cdr         True: also 'vcdr_pred', 'vcdr_gt' (cup height / disc height in rows, NaN without a disc) and 'cdr_error' = |pred - gt|
    morphometry True: also, from ONE ``ops.disc_morphometry`` call per batch over the prediction and ground-truth masks together
                (``sectors`` sectors around the disc centroid), 'hcdr', 'acdr' (horizontal and area cup-to-disc ratio) and 'rdr_min'
                (the thinnest rim-to-disc ratio) as '<x>_pred', '<x>_gt', '<x>_error' = |pred - gt|; 'rim_{up,left,down,right}_pred' /
                '_gt' (mean rim-to-disc ratio per 90-degree quadrant); 'cup_offset_pred' (distance of the predicted cup's centroid from
                the predicted disc's, pixels).  False (the default) makes no further call.
    calibration True: also, from ONE ``ops.selective_tables`` call per batch on ``prob`` against ``target > 0.5`` with ``bins``
                confidence bins, '{cup,disc}_ece' and '{cup,disc}_brier' per image, and res['calibration']: the table summed over the
                images ('rel' [2][bins][5]) with its pooled figures and reliability diagram (``metrics.calibration_from_table``)
    mc_passes   T in 2..32: also T stochastic passes per batch (``mc_logits(image, T)`` -> [T,B,2,H,W] logits; default
                ``model.mc_inference_logits``: running statistics, live dropout), ``ops.mc_uncertainty`` for the std over the passes of
                sigmoid(x / 2), and in the SAME ``ops.selective_tables`` call the risk table of ``pred`` (the masks scored above) against
                the labels per bin of that std (``unc_edges``).  Per image '{cup,disc}_unc_auroc' (do the errors sit where the std is
                large?) and per edge e of ``report_edges`` (each one of ``unc_edges``; e as %g) '{cup,disc}_cov_<e>' (share of pixels with
                std < e), '{cup,disc}_dice_<e>' and '{cup,disc}_err_<e>' (Dice and error rate over those pixels); res['risk_coverage']:
                the table summed over the images ('risk' [2][K][4]) with its pooled figures (``metrics.selective_from_table``).
                0 (the default) makes no pass and no call.
    With any of the six set, per-image dicts and 'mean' carry the added names and the result lists them as 'extra_fields'.

    save_dir    a folder: per image also <save_dir>/overlay/<stem>.png (outlines of the display masks of ``prob``: disc green, cup blue,
                ``Utils.save_per_img_batch``), original_image/<stem>.png and mask/<stem>.png (``pred``, the masks the figures above
                were computed on: 0 = cup, 128 = disc only, 255 = background).  The returned result is the same with and without it.
                With ``mc_passes`` also uncertainty/<stem>.png, RGB (0, disc, cup) of min(255, floor(std * 1600)): the trainer's
                threshold 0.04 is grey 64.  None (the default) makes no further call.

    tta         a view list - a string such as 'flips,id@0.75,id@1.25' (``tta.parse_views``) or a list of (g, h, w): ``prob`` is the
                mean over the views of the probabilities mapped back to the image's frame (``tta.tta_predict``: ``ops.tta_view``, one
                forward per distinct view shape, ``ops.tta_fuse``), and everything downstream - post-processing, metrics, calibration,
                pictures - uses it.  The result records the checked list as res['tta'] (that of the first batch).  None (the default):
                one forward of the image, as before.
    tta_uncertainty  True (needs ``tta``, excludes ``mc_passes``): the unbiased std over the views of sigmoid(x / 2) takes the place
                of the MC-dropout std: the same ``ops.selective_tables`` call, the same '{cup,disc}_unc_auroc', '_cov_<e>', '_dice_<e>',
                '_err_<e>' names, res['risk_coverage'] with 'views' in the place of 'passes', uncertainty/<stem>.png from its
                'std_u8'."""
    tolerances = tuple(float(t) for t in tolerances)
    profiled = extra_fields(hd95, tolerances, cdr)
    mc_passes = int(mc_passes)
    tta_uncertainty = bool(tta_uncertainty)
    inference.check_uncertainty_args(tta, tta_uncertainty, mc_passes)
    if tta is not None:
        from . import tta as tta_views
        if not isinstance(tta, str):
            tta = tta_views.normalise_views(tta, None, None)
    used_views = None
    with_unc = bool(mc_passes) or tta_uncertainty
    extra = extra_fields(hd95, tolerances, cdr, morphometry, calibration, mc_passes, report_edges, tta_uncertainty)
    if with_unc:
        _edge_index(unc_edges, report_edges)
    mc_logits = inference.resolve_mc_logits(model, mc_passes, mc_logits)
    pooled_rel = pooled_risk = None
    dev = torch.device("cuda") if torch.cuda.is_available() else None
    per_image = []
    with inference.eval_mode(model):
        for sample in loader:
            if 'image' not in sample or 'map' not in sample:
                raise ValueError("evaluate() takes decoded float batches {'image', 'map'} (UDA_CLR_DEVICE_INPUT unset or 0)")
            image, target = sample['image'], sample['map']
            if dev is not None:
                image, target = image.to(dev), target.to(dev)
            views = None if tta is None else tta_views.normalise_views(tta, image.shape[-2], image.shape[-1])
            used_views = views if used_views is None else used_views
            prob, unc = inference.probabilities(model, image, views, tta_uncertainty, mc_passes, mc_logits, std_u8=save_dir is not None)
            if postprocess:
                pred = Utils.postprocessing_batch(prob, threshold, dataset)
            else:
                thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
                pred = torch.stack([prob[:, 0] > thr_cup, prob[:, 1] > thr_disc], 1)
            if profiled:                                                         # the batch's one copy to the host, either way
                table, counts, profile = ops.surface_profile(pred, target > 0.5, percentiles=(95,) if hd95 else (), tolerances=tolerances)
            else:
                table, counts = ops.surface_distances(pred, target > 0.5)
            dice = metrics.dice_per_image(counts)
            sm = metrics.surface_metrics_from_table(table)
            more = {}
            if hd95:
                h = metrics.percentile_distance_from_profile(table, profile)["hd_p"][..., 0]
                more["cup_hd95"], more["disc_hd95"] = h[:, 0], h[:, 1]
            if tolerances:
                nsd = metrics.surface_dice_from_profile(table, profile)
                for t, tau in enumerate(tolerances):
                    more["cup_nsd_%g" % tau], more["disc_nsd_%g" % tau] = nsd[:, 0, t], nsd[:, 1, t]
            if cdr:
                more.update(metrics.vertical_cdr_from_profile(profile))
            if morphometry:
                more.update(morphometry_columns(pred, target > 0.5, sectors))
            if calibration or with_unc:                                          # both tables in one call, one copy
                tables = ops.selective_tables(prob if calibration else None, unc["std"] if with_unc else None, pred, target > 0.5,
                                              bins=bins, edges=unc_edges)
                if calibration:
                    more.update(calibration_columns(tables["rel"]))
                    pooled_rel = tables["rel"].sum(0) + (0 if pooled_rel is None else pooled_rel)
                if with_unc:
                    more.update(uncertainty_columns(tables["risk"], unc_edges, report_edges))
                    pooled_risk = tables["risk"].sum(0) + (0 if pooled_risk is None else pooled_risk)
            names = _names(sample, dice.shape[0], len(per_image))
            if save_dir is not None:
                Utils.save_per_img_batch(image, save_dir, names, prob)
                Utils.save_mask_batch(pred, save_dir, names)
                if with_unc:
                    Utils.save_uncertainty_batch(unc["std_u8"], save_dir, names)
            for i, name in enumerate(names):
                per_image.append({"img_name": name,
                                  "cup_dice": float(dice[i, 0]), "disc_dice": float(dice[i, 1]),
                                  "cup_assd": float(sm["assd"][i, 0]), "disc_assd": float(sm["assd"][i, 1]),
                                  "cup_hd": float(sm["hd"][i, 0]), "disc_hd": float(sm["hd"][i, 1])})
                per_image[-1].update({k: float(more[k][i]) for k in extra})
    cols = {k: np.array([r[k] for r in per_image], np.float64) for k in FIELDS + extra}
    mean = {k: (float(np.nanmean(v)) if np.isfinite(v).any() else float("nan")) for k, v in cols.items()}
    res = {"per_image": per_image, "mean": mean, "n_images": len(per_image),
           "n_undefined": {"cup": int(np.isnan(cols["cup_assd"]).sum()), "disc": int(np.isnan(cols["disc_assd"]).sum())}}
    if extra:
        res["extra_fields"] = extra
    if calibration and pooled_rel is not None:
        res["calibration"] = dict(_lists(metrics.calibration_from_table(pooled_rel)), rel=pooled_rel.tolist(), bins=int(bins))
    if pooled_risk is not None:
        res["risk_coverage"] = dict(_lists(metrics.selective_from_table(pooled_risk, unc_edges)), risk=pooled_risk.tolist(),
                                    **({"passes": mc_passes} if mc_passes else {"views": len(used_views)}))
    if tta is not None:
        res["tta"] = [list(v) for v in used_views] if used_views is not None else []
    return res


# ------------------------------------------------------------------------------------------------------------ command line
class _Compose(object):
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, sample):
        for t in self.transforms:
            sample = t(sample)
        return sample


def build_parser():
    ap = argparse.ArgumentParser(prog="python -m uda_clr_amd.evaluate", description="Per-image evaluation of a DeepLab checkpoint on a fundus test split.")
    ap.add_argument("--data-dir", required=True, help="root that holds <dataset>/<split>/ROIs/{image,mask}")
    ap.add_argument("--dataset", default="Drishti-GS")
    ap.add_argument("--split", default="test")
    ap.add_argument("--checkpoint", required=True, help="file with a 'model_state_dict'")
    ap.add_argument("--backbone", default="mobilenet")
    ap.add_argument("--out-stride", type=int, default=16)
    ap.add_argument("--use_TN", action="store_true", help="TransNorm in place of BatchNorm, as the trainers' switch")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--threshold", type=float, default=0.75)
    ap.add_argument("--no-postprocess", action="store_true", help="the plain thresholds only")
    ap.add_argument("--hd95", action="store_true")
    ap.add_argument("--tolerance", type=float, nargs="+", default=[], metavar="TAU", help="surface Dice at these pixel tolerances")
    ap.add_argument("--cdr", action="store_true", help="vertical cup-to-disc ratio and its error")
    ap.add_argument("--morphometry", action="store_true", help="horizontal and area CDR, thinnest rim, rim per quadrant, cup offset")
    ap.add_argument("--sectors", type=int, default=72, metavar="K", help="sectors of the rim profile: a multiple of 8 in 8..360")
    ap.add_argument("--calibration", action="store_true", help="ECE and Brier score per image, pooled reliability diagram")
    ap.add_argument("--bins", type=int, default=15, metavar="N", help="confidence bins of the reliability diagram, 1..64")
    ap.add_argument("--mc-passes", type=int, default=0, metavar="T",
                    help="MC-dropout passes (2..32): uncertainty AUROC, coverage / Dice / error of the pixels with std < 0.04, risk-coverage table")
    ap.add_argument("--tta", default=None, metavar="SPEC",
                    help="test-time augmentation: views id hflip vflip rot180 transpose rot90 rot270 antitranspose, flips, d4, each optionally @scale, "
                         "e.g. flips,id@0.75,id@1.25; the mean over the views is what is scored")
    ap.add_argument("--tta-uncertainty", action="store_true", help="with --tta: the std over the views fills the columns and pictures of --mc-passes")
    ap.add_argument("--csv", default=None, metavar="PATH", help="one row per image")
    ap.add_argument("--json", default=None, metavar="PATH", help="the whole result")
    ap.add_argument("--save-dir", default=None, metavar="DIR", help="write overlay/, original_image/ and mask/ PNG files per image")
    return ap


def write_csv(path, res):
    """img_name and the fields of ``res`` (the six of FIELDS, then its 'extra_fields'), one row per image; NaN is written as nan"""
    fields = FIELDS + tuple(res.get("extra_fields", ()))
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("img_name",) + fields)
        for r in res["per_image"]:
            w.writerow([r["img_name"]] + [repr(float(r[k])) for k in fields])


def write_json(path, res):
    """the whole result; NaN as the JSON extension ``NaN`` that ``json.load`` reads back"""
    with open(path, "w") as f:
        json.dump(dict(res, extra_fields=list(res.get("extra_fields", ()))), f, indent=1)
        f.write("\n")


def format_mean(res):
    fields = FIELDS + tuple(res.get("extra_fields", ()))
    return "mean over %d images: " % res["n_images"] + "  ".join("%s %.4f" % (k, res["mean"][k]) for k in fields)


def load_generator(checkpoint, backbone="mobilenet", out_stride=16, use_TN=False, device=None):
    """A DeepLab with the checkpoint's 'model_state_dict' loaded by the trainers' key filter (train_use_fix_initial.py:231-238):
    keys the model does not have are dropped, keys the file does not have keep their initial value."""
    from .networks.deeplabv3 import DeepLab
    model = DeepLab(num_classes=2, backbone=backbone, output_stride=out_stride, sync_bn=not use_TN)
    pretrained = torch.load(checkpoint, map_location="cpu", weights_only=True)["model_state_dict"]
    model_dict = model.state_dict()
    model_dict.update({k: v for k, v in pretrained.items() if k in model_dict})
    model.load_state_dict(model_dict)
    return model.to(device) if device is not None else model


def main(argv=None, model=None, mc_logits=None):
    """The command line.  ``model``: a callable to score instead of the checkpoint's DeepLab, ``mc_logits``: its stochastic passes (tests)."""
    args = build_parser().parse_args(argv)
    from torch.utils.data import DataLoader
    from .dataloaders import custom_transforms as tr
    from .dataloaders.fundus_dataloader import FundusSegmentation
    data = FundusSegmentation(base_dir=args.data_dir, dataset=args.dataset, split=args.split,
                              transform=_Compose([tr.Normalize_tf(), tr.ToTensor()]))
    if len(data) == 0:
        raise SystemExit("no images under %s/%s/%s/ROIs/image" % (args.data_dir, args.dataset, args.split))
    loader = DataLoader(data, batch_size=args.batch_size, shuffle=False, num_workers=0)
    if model is None:
        model = load_generator(args.checkpoint, args.backbone, args.out_stride, args.use_TN,
                               torch.device("cuda") if torch.cuda.is_available() else None)
    res = evaluate(model, loader, dataset=args.dataset, threshold=args.threshold, postprocess=not args.no_postprocess,
                   hd95=args.hd95, tolerances=tuple(args.tolerance), cdr=args.cdr, save_dir=args.save_dir,
                   morphometry=args.morphometry, sectors=args.sectors, calibration=args.calibration, bins=args.bins,
                   mc_passes=args.mc_passes, mc_logits=mc_logits, tta=args.tta, tta_uncertainty=args.tta_uncertainty)
    print(format_mean(res))
    if args.csv:
        write_csv(args.csv, res)
    if args.json:
        write_json(args.json, res)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
