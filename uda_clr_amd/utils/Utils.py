"""Prototype helpers and ramp functions - drop-in for the hot-path part of the reference's
``utils/Utils.py`` (same names and signatures, no cv2 / skimage / albumentations at import).

  gen_prototype(pred, feature)                                   Utils.py:108-131
  gen_prototype_retrify(oT_before, xt_feature, preds, features, T, stride)   Utils.py:159-225
  sigmoid_rampup / linear_rampup / cosine_rampdown               Utils.py:312-334

  postprocessing(prediction, threshold=0.75, dataset='G')         Utils.py:438-463 (+ get_largest_fillhole :427-436)

  save_per_img(patch_image, data_save_path, img_name, prob_map, mask_path=None, ext="bmp")   Utils.py:515-585
  save_per_img_batch(images, out_dir, names, prob) / save_mask_batch(pred, out_dir, names)   the same per batch; BEAL grey masks

The pictures are computed on the device (``ops.display_masks``, ``ops.overlay``) and written with PIL.
The JET-coloured probability / entropy maps (draw_ent, draw_mask, draw_boundary, Utils.py:349-424) depend on OpenCV's colour
table and are not built, nor are joint_val_image / save_val_img (Utils.py:466-511).
"""
import math
import os

import numpy as np

from ..ops import gen_prototype, gen_prototype_from_labels, gen_prototype_retrify  # noqa: F401
from .metrics import *  # noqa: F401,F403  (the reference re-exports its metrics the same way)


def sigmoid_rampup(current, rampup_length):
    """exp(-5 (1 - t)^2) ramp of https://arxiv.org/abs/1610.02242"""
    if rampup_length == 0:
        return 1.0
    current = float(np.clip(current, 0.0, rampup_length))
    phase = 1.0 - current / rampup_length
    return float(math.exp(-5.0 * phase * phase))


def linear_rampup(current, rampup_length):
    assert current >= 0 and rampup_length >= 0
    return 1.0 if current >= rampup_length else current / rampup_length


def cosine_rampdown(current, rampdown_length):
    assert 0 <= current <= rampdown_length
    return float(0.5 * (math.cos(math.pi * current / rampdown_length) + 1))


def adaptation_factor(m):
    return 1.0 / (1.0 + math.exp(-0.8 * (m + 1))) - 0.3


def postprocessing(prediction, threshold=0.75, dataset='G'):
    """Evaluation post-processing of ONE image's [2, H, W] (cup, disc) probability map, as utils/Utils.py:438-463: threshold
    (dataset names starting with 'D': disc > 0.5, cup > 0.1; otherwise both > ``threshold``), five 7x7 median filters, erosion
    by the radius-7 diamond, largest connected component, holes filled.  Runs on the device (``uda_postprocess``); a CPU
    tensor is moved there.  Returns a numpy array like the reference's: [2, H, W], float for the 'D' branch (it writes the
    masks into a copy of the probabilities), uint8 otherwise.  ``postprocessing_batch`` does a whole [B, 2, H, W] batch."""
    import torch
    from ..ops import kernels
    pred = torch.as_tensor(prediction)
    if pred.dim() != 3 or pred.shape[0] != 2:
        raise ValueError("expected a [2, H, W] prediction")
    out = postprocessing_batch(pred[None], threshold, dataset)[0].cpu().numpy()
    return out.astype(np.float32) if dataset[0] == 'D' else out


def postprocessing_batch(predictions, threshold=0.75, dataset='G'):
    """[B, 2, H, W] probabilities -> uint8 [B, 2, H, W] post-processed masks, on the device."""
    import torch
    from ..ops import kernels
    pred = predictions
    if not pred.is_cuda:
        if not torch.cuda.is_available():
            raise RuntimeError("uda_clr_amd post-processing computes only on the MI355X HIP kernels (there is no CPU fallback)")
        pred = pred.cuda()
    thr_cup, thr_disc = (0.1, 0.5) if dataset[0] == 'D' else (threshold, threshold)
    return kernels().postprocess(pred.contiguous().float(), thr_cup, thr_disc)


def _stem(img_name):
    return str(img_name).split('.')[0]                       # as the reference: everything before the first dot


def _save_png(array, folder, img_name):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, _stem(img_name) + '.png')
    Image.fromarray(array).save(path)
    return path


def save_per_img_batch(images, out_dir, names, prob, originals=True):
    """The reference's contour pictures of a whole batch: ``<out_dir>/overlay/<stem>.png`` and, with ``originals``,
    ``<out_dir>/original_image/<stem>.png`` per image.
        images  float [B,3,H,W] in [-1, 1] or uint8 [B,H,W,3]
        prob    [B,2,H,W] (cup, disc) probabilities (display masks by ``ops.display_masks``, always > 0.75 as in the reference) or uint8 / bool masks
    Image bytes, display masks and painting run on the device; one copy brings the batch to the host, 3 B per pixel for the
    overlays and 3 more when the originals are written.  Neither argument is modified.  Returns the overlay paths."""
    import torch
    from .. import ops
    names = [str(n) for n in names]
    if len(names) != images.shape[0]:
        raise ValueError("save_per_img_batch: %d names for %d images" % (len(names), images.shape[0]))
    (images,) = ops._to_device(images)
    if images.dtype != torch.uint8:
        images = ops.kernels().image_u8(images.contiguous().float())
    over = ops.overlay(images, prob)
    host = (torch.stack([over, images.contiguous()]) if originals else over[None]).cpu().numpy()     # the one copy (it synchronises)
    paths = []
    for i, name in enumerate(names):
        if originals:
            _save_png(host[1, i], os.path.join(out_dir, 'original_image'), name)
        paths.append(_save_png(host[0, i], os.path.join(out_dir, 'overlay'), name))
    return paths


def save_mask_batch(pred, out_dir, names):
    """``<out_dir>/mask/<stem>.png`` per image in the BEAL grey coding: 0 = cup, 128 = disc only, 255 = background, from
    [B,2,H,W] (cup, disc) masks (nonzero = set).  One copy of 1 B per pixel.  Returns the paths."""
    import torch
    pred = pred != 0
    grey = torch.where(pred[:, 0], 0, torch.where(pred[:, 1], 128, 255)).to(torch.uint8).cpu().numpy()
    return [_save_png(grey[i], os.path.join(out_dir, 'mask'), name) for i, name in enumerate(names)]


def save_uncertainty_batch(std_u8, out_dir, names):
    """``<out_dir>/uncertainty/<stem>.png`` per image: RGB (0, disc, cup) of the uint8 [B,2,H,W] (cup, disc) quantised MC-dropout std
    (``ops.mc_uncertainty(..., u8_scale=...)['std_u8']``).  One copy of 3 B per pixel.  Returns the paths."""
    import torch
    rgb = torch.stack([torch.zeros_like(std_u8[:, 0]), std_u8[:, 1], std_u8[:, 0]], -1).cpu().numpy()
    return [_save_png(rgb[i], os.path.join(out_dir, 'uncertainty'), name) for i, name in enumerate(names)]


def save_per_img(patch_image, data_save_path, img_name, prob_map, mask_path=None, ext="bmp"):
    """``<data_save_path>/original_image/<stem>.png`` and ``<data_save_path>/overlay/<stem>.png`` of ONE image, as
    utils/Utils.py:515-585: ``patch_image`` [H, W, 3] in 0..255 (cast to uint8 by truncation, as there), ``prob_map`` [2, H, W]
    (cup, disc).  Channel 1's outline is green, channel 0's blue over it.  ``mask_path`` and ``ext`` are accepted and unused, as in
    the reference.  Unlike the reference neither ``prob_map`` (its border ring) nor ``patch_image`` is written to, and outline
    pixels that would fall outside the image are dropped instead of wrapping round or raising."""
    import torch
    image = np.ascontiguousarray(np.asarray(patch_image).astype(np.uint8))
    if image.ndim != 3 or image.shape[2] != 3:
        raise ValueError("expected an [H, W, 3] image")
    prob = prob_map.detach().float() if torch.is_tensor(prob_map) else torch.from_numpy(np.array(prob_map, dtype=np.float32))
    if prob.dim() != 3 or prob.shape[0] != 2:
        raise ValueError("expected a [2, H, W] probability map")
    save_per_img_batch(torch.from_numpy(image)[None], data_save_path, [img_name], prob[None])
