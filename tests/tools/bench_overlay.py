#!/usr/bin/env python
"""Measurements for the prediction pictures (profiles/overlay_kernels.md), one process, device events, every shape warmed,
at B = 16 and 512 x 512:

  (a) forward        the MobileNetV2 DeepLab eval forward under no_grad
  (b) display_masks  ops.display_masks on the probabilities of synthetic ellipses (host synchronisation of the retry check included)
  (c) overlay        ops.overlay of uint8 images and the display masks of (b); and uda_overlay_u8 alone with its achieved GB/s
                     against the algorithmic bytes, 3 (image) + 2 (masks) + 3 (out) per pixel
  (d) image_u8       uda_image_u8 alone (12 B read + 3 B written per pixel)
                     The two kernels take tens of microseconds, so "alone" is a window of --inner back-to-back calls divided by
                     their number (a window around one call would measure the launch); the batch's 32 MiB stay in the last-level cache
                     between calls, which the GB/s figure therefore includes.
  (e) scipy          the statement of tests/overlay_ref.py (display masks, then painting) per image on one host core

No time here is a pass criterion; the file records what was measured.

    python tests/tools/bench_overlay.py [--batch 16] [--size 512] [--reps 20] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import overlay_ref as ovr  # noqa: E402
from bench_surface import inputs, timed  # noqa: E402
from uda_clr_amd import ops  # noqa: E402


def timed_window(fn, reps, inner):
    """median and spread (ms PER CALL) of device-event windows around ``inner`` back-to-back calls of fn"""
    def window():
        for _ in range(inner):
            fn()
    w = timed(window, reps)
    return {"median_ms": w["median_ms"] / inner, "min_ms": w["min_ms"] / inner, "max_ms": w["max_ms"] / inner, "reps": reps, "calls_per_window": inner}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=200, help="calls per window of the kernel-only figures")
    ap.add_argument("--scipy-images", type=int, default=4, help="images of the batch the host statement is timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlay.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    prob, _ = inputs(B, S, dev)
    K = ops.kernels()
    x = torch.rand(B, 3, S, S, device=dev) * 2 - 1
    image = K.image_u8(x)
    masks = ops.display_masks(prob)
    out = {"batch": B, "size": S, "device": torch.cuda.get_device_name(0)}
    out["display_masks"] = timed(lambda: ops.display_masks(prob), args.reps)
    from uda_clr_amd.utils import Utils
    out["postprocess"] = timed(lambda: Utils.postprocessing_batch(prob), args.reps)      # the evaluation chain the display chain extends
    out["overlay"] = timed(lambda: ops.overlay(image, masks), args.reps)
    dst = torch.empty_like(image)
    out["overlay_kernel_only"] = timed_window(lambda: K.overlay_u8(image, masks, out=dst), args.reps, args.inner)
    px = B * S * S
    out["overlay_kernel_only"]["algorithmic_bytes"] = 8 * px
    out["overlay_kernel_only"]["GBps"] = 8 * px / (out["overlay_kernel_only"]["median_ms"] * 1e-3) / 1e9
    out["image_u8_kernel_only"] = timed_window(lambda: K.image_u8(x, out=dst), args.reps, args.inner)
    out["image_u8_kernel_only"]["GBps"] = 15 * px / (out["image_u8_kernel_only"]["median_ms"] * 1e-3) / 1e9
    # the timed size computes the right thing (two images against the host statement)
    ph, ih = prob[:2].cpu().numpy(), image[:2].cpu().numpy()
    mh = ovr.display_masks(ph)
    assert np.array_equal(masks[:2].cpu().numpy(), mh)
    assert np.array_equal(ops.overlay(image[:2], masks[:2]).cpu().numpy(), ovr.overlay_batch(ih, mh))
    out["outline_pixels_per_image_mean"] = float((ops.overlay(image, masks) != image).any(-1).float().sum() / B)
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    torch.manual_seed(0)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(dev).eval()
    with torch.no_grad():
        out["forward"] = timed(lambda: model(x), args.reps)
    n = min(args.scipy_images, B)
    ph, ih = prob[:n].cpu().numpy(), image[:n].cpu().numpy()
    per_mask, per_paint = [], []
    for b in range(n):
        t0 = time.perf_counter()
        m = ovr.display_masks(ph[b])
        t1 = time.perf_counter()
        ovr.overlay(ih[b], m)
        per_mask.append((t1 - t0) * 1e3)
        per_paint.append((time.perf_counter() - t1) * 1e3)
    out["scipy_display_masks_per_image"] = {"median_ms": statistics.median(per_mask), "min_ms": min(per_mask), "max_ms": max(per_mask), "images": n}
    out["scipy_overlay_per_image"] = {"median_ms": statistics.median(per_paint), "min_ms": min(per_paint), "max_ms": max(per_paint), "images": n}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
