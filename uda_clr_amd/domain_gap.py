"""Category-level domain-gap report: per class (cup / disc, object / background) the mean and covariance of the generator's feature
over a whole dataset, for the source and the target domain, and what the method's regularisers are about, read off them:

  * how far apart the two domains' class distributions are - the prototype distance the trainer's ``intra_loss`` sums
    (Trainer_prototype_full.py:428-444) and the Frechet distance between the two Gaussians;
  * how compact each class is - tr(cov) / C, the class mean of the D(f, c_k) the discriminative loss minimises;
  * how well object and background separate - the terms of ``inter_loss`` and a Fisher-type ratio.

The first moments are ``uda_proto_reduce`` (the trainer's prototype sums), the second moments ``uda_proto_scatter`` (``ops.class_scatter``,
DESIGN.md 3p): both add into fp64 accumulators that stay on the device over the whole loader, and ONE copy brings them to the host.

    python -m uda_clr_amd.domain_gap --data-dir DIR --source REFUGE --target Drishti-GS --checkpoint FILE
                                     [--target-weights labels|soft|hard] [--json report.json] [--csv per_class.csv]
"""
import argparse
import csv
import json
import sys

import numpy as np
import torch

from . import inference, ops

CLASSES = ("cup_obj", "disc_obj", "cup_bck", "disc_bck")          # the order of uda_proto_weights
STRUCTURES = (("cup", 0, 2), ("disc", 1, 3))                      # name, object class, background class
CLASS_FIELDS = ("n_src", "n_tgt", "proto_mse", "proto_cos", "compact_src", "compact_tgt", "frechet")
WEIGHTS = ("labels", "soft", "hard")


def moments_from_sums(sums, scatter, centre):
    """The host half of ``MomentAccumulator.finalize``, in float64: sums [4, C+1] (weighted channel sums, then the weight total),
    scatter [4, C, C] about ``centre`` [4, C] -> {'count' [4], 'mean' [4, C], 'cov' [4, C, C]}.

    The shift identity: with mu = sums / W and d = mu - a,
        sum_p w (f - mu)(f - mu)^T = sum_p w (f - a)(f - a)^T - W d d^T,
    so cov = S / W - d d^T for ANY centre a; a centre near the mean only keeps the subtraction from cancelling.  A class without
    weight has NaN mean and covariance."""
    sums, scatter, centre = (np.asarray(t, np.float64) for t in (sums, scatter, centre))
    C = sums.shape[1] - 1
    count = sums[:, C].copy()
    mean = np.full((4, C), np.nan)
    cov = np.full((4, C, C), np.nan)
    for k in range(4):
        if count[k] > 0:
            mean[k] = sums[k, :C] / count[k]
            d = mean[k] - centre[k]
            cov[k] = scatter[k] / count[k] - np.outer(d, d)
    return {"count": count, "mean": mean, "cov": cov}


class MomentAccumulator(object):
    """Streaming weighted mean and covariance of the four classes' features, on the device.

    ``update(feature, wts)`` adds one batch: the weighted channel sums and weight totals through ``uda_proto_reduce`` into an fp64
    [4, C+1] tensor, the scatter about a FIXED centre through ``ops.class_scatter`` into an fp64 [4, C, C] tensor.  The centre is
    the first batch's class centroids (zeros for a class that is empty there): near the mean, so that the fp32 products are of
    deviations, and fixed, so that batches add.  ``finalize()`` makes one copy to the host and shifts to the true mean in fp64.

    The covariance is the BIASED, weighted maximum-likelihood one: cov_k = sum_p w_k[p] (f_p - mu_k)(f_p - mu_k)^T / sum_p w_k[p],
    without Bessel's correction (for soft weights there is no agreed one)."""

    def __init__(self, C):
        self.C = int(C)
        self.sums = self.scatter = self.centre = None

    def update(self, feature, wts):
        """feature [B, C, h, w] on the device, wts [B*h*w, 4] as ``uda_proto_weights`` writes them"""
        K = ops.kernels()
        rows = ops.rows_view(feature.detach())
        if rows.shape[1] != self.C:
            raise ValueError("MomentAccumulator(%d) got a feature of %d channels" % (self.C, rows.shape[1]))
        first = self.sums is None
        if first:
            self.sums = torch.zeros(4, self.C + 1, dtype=torch.float64, device=rows.device)
            self.scatter = torch.zeros(4, self.C, self.C, dtype=torch.float64, device=rows.device)
        K.proto_reduce(rows, wts, self.sums)
        if first:
            count = self.sums[:, self.C:]
            self.centre = torch.where(count > 0, self.sums[:, :self.C] / count.clamp_min(1e-300), torch.zeros_like(count)).float().contiguous()
        ops.class_scatter(rows, wts, self.centre, out=self.scatter)       # the rows, not the feature: one packing copy at most

    def finalize(self):
        """-> {'count' [4], 'mean' [4, C], 'cov' [4, C, C]} as float64 numpy arrays (``moments_from_sums``)"""
        if self.sums is None:
            raise ValueError("MomentAccumulator.finalize() before any update()")
        n1, n2 = self.sums.numel(), self.scatter.numel()
        host = torch.cat([self.sums.view(-1), self.scatter.view(-1), self.centre.double().view(-1)]).cpu().numpy()
        return moments_from_sums(host[:n1].reshape(4, self.C + 1), host[n1:n1 + n2].reshape(4, self.C, self.C),
                                 host[n1 + n2:].reshape(4, self.C))


def class_weights(sample_map, o_before, weights="labels", threshold=0.75):
    """[P, 4] class weights at the feature's resolution, all through ``uda_proto_weights`` mode 0:
        labels  the label map [B,2,H,W], nearest-resized inside the kernel (``ops.gen_prototype_from_labels``)
        soft    sigmoid(o_before), the trainer's target weights (Trainer_prototype_full.py:375-377)
        hard    sigmoid(o_before) > threshold"""
    B, _, h, w = o_before.shape
    if weights == "labels":
        src = sample_map.to(o_before.device)
    elif weights == "soft":
        src = torch.sigmoid(o_before)
    elif weights == "hard":
        src = (torch.sigmoid(o_before) > threshold).float()
    else:
        raise ValueError("weights must be one of %r, got %r" % (WEIGHTS, weights))
    return ops.kernels().proto_weights(0, B, h, w, map_=src.detach().contiguous().float())[0]


def domain_moments(model, loader, weights="labels", threshold=0.75):
    """Class moments of ``model``'s feature over every batch of ``loader``.

    model    the generator: a callable returning the 7-tuple of ``DeepLab`` - output 4 is the feature the trainer calls
             ``xs_feature`` / ``xt_feature`` (305 channels), output 5 the logits ``o_before`` at the feature's resolution
    loader   iterable of decoded float batches {'image' [B,3,H,W], 'map' [B,2,H,W]} ('map' is needed for ``weights='labels'`` only)
    -> ``MomentAccumulator.finalize()``'s dict"""
    if weights not in WEIGHTS:
        raise ValueError("weights must be one of %r, got %r" % (WEIGHTS, weights))
    dev = torch.device("cuda") if torch.cuda.is_available() else None
    acc = None
    with inference.eval_mode(model):
        for sample in loader:
            if 'image' not in sample or (weights == "labels" and 'map' not in sample):
                raise ValueError("domain_moments() takes decoded float batches {'image', 'map'} (UDA_CLR_DEVICE_INPUT unset or 0)")
            image = sample['image'] if dev is None else sample['image'].to(dev)
            out = model(image)
            feature, o_before = out[4], out[5]
            if acc is None:
                acc = MomentAccumulator(feature.shape[1])
            acc.update(feature, class_weights(sample.get('map'), o_before, weights, threshold))
    if acc is None:
        raise ValueError("domain_moments(): the loader gave no batch")
    return acc.finalize()


def _psd_sqrt(m):
    """symmetric square root of a symmetric positive semi-definite matrix through eigh, eigenvalues clamped at 0"""
    w, v = np.linalg.eigh((m + m.T) * 0.5)
    return (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T


def frechet_distance(mu1, cov1, mu2, cov2):
    """Squared Frechet (2-Wasserstein) distance between N(mu1, cov1) and N(mu2, cov2), float64 on the host:
        d^2 = |mu1 - mu2|^2 + tr(cov1 + cov2 - 2 (cov1^{1/2} cov2 cov1^{1/2})^{1/2})
    Both square roots come from ``eigh`` with the eigenvalues clamped at 0 (no general matrix square root, no scipy).  The inner
    matrix is M^T M for M = cov2^{1/2} cov1^{1/2}, so the trace of its root is the sum of M's singular values; taking them from M
    instead of the eigenvalues of M^T M keeps the null directions of a rank-deficient covariance (fewer pixels than channels) at
    eps * |M| instead of sqrt(eps) * |M|, which is what lets a distribution against itself come out at 0.  The result is clamped
    at 0; NaN in gives NaN out."""
    mu1, cov1, mu2, cov2 = (np.asarray(t, np.float64) for t in (mu1, cov1, mu2, cov2))
    if not (np.isfinite(mu1).all() and np.isfinite(mu2).all() and np.isfinite(cov1).all() and np.isfinite(cov2).all()):
        return float("nan")
    cross = np.linalg.svd(_psd_sqrt(cov2) @ _psd_sqrt(cov1), compute_uv=False).sum()
    d = mu1 - mu2
    return float(max(d @ d + np.trace(cov1) + np.trace(cov2) - 2.0 * cross, 0.0))


def gap_report(src, tgt):
    """``src`` / ``tgt``: the moment dicts of the two domains (``domain_moments``) ->
      {'classes': {name: {n_src, n_tgt, proto_mse, proto_cos, compact_src, compact_tgt, frechet}} for cup_obj, disc_obj, cup_bck, disc_bck,
       'structures': {cup | disc: {separation_src, separation_tgt, fisher_src, fisher_tgt}},
       'intra_loss': sum of the four proto_mse, 'n_empty': 0..8, the (class, domain) pairs without weight, 'channels': C}
    proto_mse = mean_c (mu_s - mu_t)^2, the summands of the trainer's intra_loss; compact = tr(cov) / C, the class mean of
    Appendix B's D(f, c_k); separation = mean_c (mu_obj - mu_bck)^2, the terms of inter_loss; fisher = |mu_obj - mu_bck|^2 /
    (tr cov_obj + tr cov_bck).  A class that is empty in a domain has NaN in every field that needs it."""
    C = src["mean"].shape[1]
    if tgt["mean"].shape[1] != C:
        raise ValueError("gap_report: %d source channels, %d target channels" % (C, tgt["mean"].shape[1]))
    classes = {}
    n_empty = 0
    for k, name in enumerate(CLASSES):
        ms, mt = src["mean"][k], tgt["mean"][k]
        d = ms - mt
        norm = np.sqrt(ms @ ms) * np.sqrt(mt @ mt)
        classes[name] = {"n_src": float(src["count"][k]), "n_tgt": float(tgt["count"][k]),
                         "proto_mse": float(np.mean(d * d)),
                         "proto_cos": float(ms @ mt / norm) if norm > 0 else float("nan"),
                         "compact_src": float(np.trace(src["cov"][k]) / C), "compact_tgt": float(np.trace(tgt["cov"][k]) / C),
                         "frechet": frechet_distance(ms, src["cov"][k], mt, tgt["cov"][k])}
        n_empty += int(not src["count"][k] > 0) + int(not tgt["count"][k] > 0)
    structures = {}
    for name, o, b in STRUCTURES:
        row = {}
        for dom, m in (("src", src), ("tgt", tgt)):
            d = m["mean"][o] - m["mean"][b]
            within = np.trace(m["cov"][o]) + np.trace(m["cov"][b])
            row["separation_" + dom] = float(np.mean(d * d))
            row["fisher_" + dom] = float(d @ d / within) if within != 0 else float("nan")
        structures[name] = row
    return {"classes": classes, "structures": structures, "intra_loss": float(sum(classes[n]["proto_mse"] for n in CLASSES)),
            "n_empty": n_empty, "channels": int(C)}


# ------------------------------------------------------------------------------------------------------------ command line
def build_parser():
    ap = argparse.ArgumentParser(prog="python -m uda_clr_amd.domain_gap",
                                 description="Per-class feature moments of a DeepLab checkpoint on a source and a target split, and the gap between them.")
    ap.add_argument("--data-dir", required=True, help="root that holds <dataset>/<split>/ROIs/{image,mask}")
    ap.add_argument("--source", default="REFUGE", help="source dataset (labels give its class weights)")
    ap.add_argument("--target", default="Drishti-GS")
    ap.add_argument("--source-split", default="train")
    ap.add_argument("--target-split", default="test")
    ap.add_argument("--checkpoint", required=True, help="file with a 'model_state_dict'")
    ap.add_argument("--backbone", default="mobilenet")
    ap.add_argument("--out-stride", type=int, default=16)
    ap.add_argument("--use_TN", action="store_true", help="TransNorm in place of BatchNorm, as the trainers' switch")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--target-weights", choices=WEIGHTS, default="labels",
                    help="target class weights: its labels, sigmoid of the prediction (the trainer's), or the prediction above --threshold")
    ap.add_argument("--threshold", type=float, default=0.75)
    ap.add_argument("--json", default=None, metavar="PATH", help="the whole report")
    ap.add_argument("--csv", default=None, metavar="PATH", help="one row per class")
    return ap


def write_csv(path, report):
    """class and CLASS_FIELDS, one row per class; NaN is written as nan"""
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(("class",) + CLASS_FIELDS)
        for name in CLASSES:
            w.writerow([name] + [repr(float(report["classes"][name][k])) for k in CLASS_FIELDS])


def _strict(x):
    """NaN -> None, through dicts"""
    if isinstance(x, dict):
        return {k: _strict(v) for k, v in x.items()}
    return None if isinstance(x, float) and x != x else x


def write_json(path, report):
    """the whole report as standard JSON: a NaN field (an empty class) is written as ``null``"""
    with open(path, "w") as f:
        json.dump(_strict(report), f, indent=1, allow_nan=False)
        f.write("\n")


def format_report(report):
    lines = ["%-9s %10s %10s %11s %9s %11s %11s %11s" % (("class",) + CLASS_FIELDS)]
    for name in CLASSES:
        r = report["classes"][name]
        lines.append("%-9s %10.0f %10.0f %11.4e %9.4f %11.4e %11.4e %11.4e" % ((name,) + tuple(r[k] for k in CLASS_FIELDS)))
    for name, _, _ in STRUCTURES:
        r = report["structures"][name]
        lines.append("%-4s separation src %.4e tgt %.4e   fisher src %.4f tgt %.4f" % (name, r["separation_src"], r["separation_tgt"],
                                                                                       r["fisher_src"], r["fisher_tgt"]))
    lines.append("intra_loss %.6e   empty classes %d" % (report["intra_loss"], report["n_empty"]))
    return "\n".join(lines)


def _loader(data_dir, dataset, split, batch_size):
    from torch.utils.data import DataLoader
    from .dataloaders import custom_transforms as tr
    from .dataloaders.fundus_dataloader import FundusSegmentation
    from .evaluate import _Compose
    data = FundusSegmentation(base_dir=data_dir, dataset=dataset, split=split, transform=_Compose([tr.Normalize_tf(), tr.ToTensor()]))
    if len(data) == 0:
        raise SystemExit("no images under %s/%s/%s/ROIs/image" % (data_dir, dataset, split))
    return DataLoader(data, batch_size=batch_size, shuffle=False, num_workers=0)


def main(argv=None, model=None, loaders=None):
    """The command line.  ``model``: a generator to use instead of the checkpoint's DeepLab; ``loaders``: (source, target) batch
    iterables to use instead of the two splits on disk (tests)."""
    args = build_parser().parse_args(argv)
    if loaders is None:
        loaders = (_loader(args.data_dir, args.source, args.source_split, args.batch_size),
                   _loader(args.data_dir, args.target, args.target_split, args.batch_size))
    if model is None:
        from .evaluate import load_generator
        model = load_generator(args.checkpoint, args.backbone, args.out_stride, args.use_TN,
                               torch.device("cuda") if torch.cuda.is_available() else None)
    src = domain_moments(model, loaders[0], "labels", args.threshold)
    tgt = domain_moments(model, loaders[1], args.target_weights, args.threshold)
    report = gap_report(src, tgt)
    report["source"], report["target"], report["target_weights"] = args.source, args.target, args.target_weights
    print(format_report(report))
    if args.csv:
        write_csv(args.csv, report)
    if args.json:
        write_json(args.json, report)
    return report


if __name__ == "__main__":
    main(sys.argv[1:])
