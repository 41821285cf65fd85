#!/usr/bin/env python
"""What hd95, one surface-Dice tolerance and the CDR add to the evaluation's metric call (profiles/surface_kernels.md): in one
process, device events, warmed, the median of repeated single calls, at B = 16 and 512 x 512, on the post-processed masks of
tests/tools/bench_surface.py:

  surface   ops.surface_distances(masks, gt)                                   - (c) of bench_surface.py, copy to the host included
  profile   ops.surface_profile(masks, gt, percentiles=(95,), tolerances=(2,)) - the same plus pass 5 and its larger copy

The requirement either is held to is that of bench_surface.py: no longer than the eval forward (a) it sits beside; run that tool
for (a).  The two are timed in turns (surface, profile, surface, ...) so that a drift of the clock falls on both alike.

    python tests/tools/bench_surface_profile.py [--batch 16] [--size 512] [--reps 20] [--out FILE]
    python tests/tools/bench_surface_profile.py --only profile     # under `rocprofv3 --kernel-trace --stats` for pass 5's own time
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import surface_profile_ref as spr  # noqa: E402
from bench_surface import inputs  # noqa: E402
from uda_clr_amd import ops  # noqa: E402
from uda_clr_amd.utils import Utils  # noqa: E402


def timed_in_turns(fns, reps, warmup=3):
    """{name: median / min / max ms} of device-event windows around single calls, the functions taking turns"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": reps} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["profile"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_surface_profile.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    B, S = args.batch, args.size
    prob, gt = inputs(B, S, dev)
    masks = Utils.postprocessing_batch(prob)
    gt_b = gt > 0.5
    K = ops.kernels()
    m8, g8 = masks.contiguous(), gt_b.to(torch.uint8).contiguous()
    fns = {"profile": lambda: ops.surface_profile(masks, gt_b, percentiles=(95,), tolerances=(2,)),
           "profile_kernels_only": lambda: K.surface_profile(m8, g8, [0.95], [4])}
    if args.only is None:
        fns.update({"surface": lambda: ops.surface_distances(masks, gt_b), "surface_kernels_only": lambda: K.surface_distance(m8, g8)})
    out = {"batch": B, "size": S, "device": torch.cuda.get_device_name(0)}
    out.update(timed_in_turns(fns, args.reps))
    table, counts, prof = ops.surface_profile(masks, gt_b, percentiles=(95,), tolerances=(2,))
    want = spr.profile(masks[:2].cpu().numpy(), gt_b[:2].cpu().numpy(), (95,), (2,))                  # the timed size computes the right thing
    assert all(np.array_equal(prof[k][:2], want[k]) for k in ("order", "within", "extent"))
    out["border_pixels_per_plane_mean"] = float(table[..., 0].mean())
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
