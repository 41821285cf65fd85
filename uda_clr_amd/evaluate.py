"""Per-image evaluation in the form of the paper's tables: for every test image, after the evaluation post-processing
(utils/Utils.py:438-463), Dice, average symmetric surface distance and Hausdorff distance of cup and disc.

The forward, ``postprocessing_batch`` and ``ops.surface_distances`` run per batch on the device; the metrics are closed forms
(utils/metrics.py) of the small table that one copy per batch brings to the host.  No per-image device call is made.
"""
import numpy as np
import torch

from . import ops
from .utils import Utils, metrics

FIELDS = ("cup_dice", "disc_dice", "cup_assd", "disc_assd", "cup_hd", "disc_hd")


def _names(sample, B, seen):
    names = sample.get("img_name") if hasattr(sample, "get") else None
    if names is None:
        return ["%d" % (seen + i) for i in range(B)]
    return [str(n) for n in ([names] if isinstance(names, str) else list(names))]


def evaluate(model, loader, dataset='G', threshold=0.75, postprocess=True):
    """Score ``model`` on every image of ``loader``.

    model       callable whose first output (or only output) is the [B,2,H,W] logits (cup, disc), e.g. ``DeepLab``
    loader      iterable of decoded float batches {'image' [B,3,H,W], 'map' [B,2,H,W], 'img_name'} (UDA_CLR_DEVICE_INPUT unset or 0)
    dataset     as ``utils.Utils.postprocessing``: names starting with 'D' threshold cup > 0.1 and disc > 0.5, others ``threshold``
    postprocess False: the plain thresholds only, without median / erosion / largest component / hole filling

    -> {'per_image': [{'img_name', 'cup_dice', 'disc_dice', 'cup_assd', 'disc_assd', 'cup_hd', 'disc_hd'}, ...],
        'mean': nanmean of each field, 'n_images', 'n_undefined': {'cup', 'disc'}}; distances in pixels.  An (image, class) whose
    predicted or true mask is empty has NaN distances and is counted in ``n_undefined``."""
    dev = torch.device("cuda") if torch.cuda.is_available() else None
    was_training = getattr(model, "training", False)
    if hasattr(model, "eval"):
        model.eval()
    per_image = []
    try:
        with torch.no_grad():
            for sample in loader:
                if 'image' not in sample or 'map' not in sample:
                    raise ValueError("evaluate() takes decoded float batches {'image', 'map'} (UDA_CLR_DEVICE_INPUT unset or 0)")
                image, target = sample['image'], sample['map']
                if dev is not None:
                    image, target = image.to(dev), target.to(dev)
                out = model(image)
                logits = out[0] if isinstance(out, (tuple, list)) else out
                prob = torch.sigmoid(logits.float())
                if postprocess:
                    pred = Utils.postprocessing_batch(prob, threshold, dataset)
                else:
                    thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
                    pred = torch.stack([prob[:, 0] > thr_cup, prob[:, 1] > thr_disc], 1)
                table, counts = ops.surface_distances(pred, target > 0.5)           # the batch's one copy to the host
                dice = metrics.dice_per_image(counts)
                sm = metrics.surface_metrics_from_table(table)
                for i, name in enumerate(_names(sample, dice.shape[0], len(per_image))):
                    per_image.append({"img_name": name,
                                      "cup_dice": float(dice[i, 0]), "disc_dice": float(dice[i, 1]),
                                      "cup_assd": float(sm["assd"][i, 0]), "disc_assd": float(sm["assd"][i, 1]),
                                      "cup_hd": float(sm["hd"][i, 0]), "disc_hd": float(sm["hd"][i, 1])})
    finally:
        if was_training and hasattr(model, "train"):
            model.train()
    cols = {k: np.array([r[k] for r in per_image], np.float64) for k in FIELDS}
    mean = {k: (float(np.nanmean(v)) if np.isfinite(v).any() else float("nan")) for k, v in cols.items()}
    return {"per_image": per_image, "mean": mean, "n_images": len(per_image),
            "n_undefined": {"cup": int(np.isnan(cols["cup_assd"]).sum()), "disc": int(np.isnan(cols["disc_assd"]).sum())}}
