#!/usr/bin/env python
"""Measurements for the per-image evaluation (profiles/surface_kernels.md), one process, device events, every shape warmed,
at B = 16 and 512 x 512:

  (a) forward      the MobileNetV2 DeepLab eval forward under no_grad
  (b) postprocess  utils.Utils.postprocessing_batch on the probabilities of synthetic ellipses
  (c) surface      ops.surface_distances on the post-processed masks of (b) against the ellipses' ground truth, copy to the
                   host included
  (d) scipy        the oracle of tests/surface_ref.py per image on one host core (median over the images of the batch)

The requirement is (c) <= (a): the metric must never be what bounds an evaluation.

    python tests/tools/bench_surface.py [--batch 16] [--size 512] [--reps 20] [--out FILE]
    python tests/tools/bench_surface.py --only surface     # (c) alone, e.g. under `rocprofv3 --kernel-trace --stats` for the kernel split
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

import surface_ref as sr  # noqa: E402
from uda_clr_amd import ops  # noqa: E402
from uda_clr_amd.utils import Utils  # noqa: E402


def timed(fn, reps, warmup=3):
    """median and spread (ms) of device-event windows around single calls of fn"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def inputs(B, S, dev):
    """ground-truth ellipses and the probabilities of perturbed copies (cup: semi-axes 0.12-0.2 S, disc: 0.25-0.35 S)"""
    rng = np.random.default_rng(17)
    gt, prob = np.zeros((B, 2, S, S), np.float32), np.zeros((B, 2, S, S), np.float32)
    for b in range(B):
        cy, cx = rng.uniform(0.45, 0.55, 2) * S
        for c, (lo, hi) in enumerate(((0.12, 0.2), (0.25, 0.35))):
            a, d, th = rng.uniform(lo, hi) * S, rng.uniform(lo, hi) * S, rng.uniform(0, np.pi)
            gt[b, c] = sr.ellipse(S, S, cy, cx, a, d, th)
            p = sr.ellipse(S, S, cy + rng.uniform(-0.02, 0.02) * S, cx + rng.uniform(-0.02, 0.02) * S, a * rng.uniform(0.9, 1.1),
                           d * rng.uniform(0.9, 1.1), th + rng.uniform(-0.2, 0.2))
            prob[b, c] = np.where(p, 0.95, 0.03)
    return torch.from_numpy(prob).to(dev), torch.from_numpy(gt).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["surface"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    prob, gt = inputs(B, S, dev)
    masks = Utils.postprocessing_batch(prob)
    gt_b = gt > 0.5
    out = {"batch": B, "size": S, "device": torch.cuda.get_device_name(0)}
    out["surface"] = timed(lambda: ops.surface_distances(masks, gt_b), args.reps)
    K = ops.kernels()
    m8, g8 = masks.contiguous(), gt_b.to(torch.uint8).contiguous()
    out["surface_kernels_only"] = timed(lambda: K.surface_distance(m8, g8), args.reps)          # without mask conversion and copy
    table, counts = ops.surface_distances(masks, gt_b)
    rt, rc, _ = sr.reference(masks[:2].cpu().numpy(), gt_b[:2].cpu().numpy())                   # the timed size computes the right thing
    assert np.array_equal(table[:2, ..., 0], rt[..., 0]) and np.array_equal(table[:2, ..., 2], rt[..., 2]) and np.array_equal(counts[:2], rc)
    assert np.allclose(table[:2, ..., 1], rt[..., 1], rtol=1e-12, atol=0)
    out["border_pixels_per_plane_mean"] = float(table[..., 0].mean())
    if args.only is None:
        from uda_clr_amd.networks.deeplabv3 import DeepLab
        torch.manual_seed(0)
        model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(dev).eval()
        image = torch.randn(B, 3, S, S, device=dev)
        with torch.no_grad():
            out["forward"] = timed(lambda: model(image), args.reps)
        out["postprocess"] = timed(lambda: Utils.postprocessing_batch(prob), args.reps)
        mh, gh = masks.cpu().numpy() > 0, gt_b.cpu().numpy()
        per = []
        for b in range(B):
            t0 = time.perf_counter()
            for c in range(2):
                sr.table(mh[b, c], gh[b, c])
            per.append((time.perf_counter() - t0) * 1e3)
        out["scipy_per_image"] = {"median_ms": statistics.median(per), "min_ms": min(per), "max_ms": max(per), "images": B}
        out["surface_le_forward"] = out["surface"]["median_ms"] <= out["forward"]["median_ms"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
