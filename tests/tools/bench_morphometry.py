#!/usr/bin/env python
"""What the optic-disc morphometry adds to an evaluation (profiles/morphometry_kernels.md): in one process, device events, warmed,
the median of repeated single calls, at B = 16 and 512 x 512, on the post-processed masks of tests/tools/bench_surface.py:

  morphometry               ops.disc_morphometry(masks)                                      - mask conversion and the copy to the host included
  morphometry_kernels_only  HipKernels.disc_morphometry(uint8 masks, table on the device)    - the three launches
  morphometry_pair          ops.disc_morphometry(prediction and ground truth stacked, 2 B)   - what evaluate(morphometry=True) calls
  closed_forms              utils.metrics.morphometry_from_moments on the host (wall clock)
  profile                   ops.surface_profile(masks, gt, percentiles=(95,), tolerances=(2,)) - the yardstick, in the same run
  forward                   the MobileNetV2 DeepLab eval forward under no_grad

No time is fixed in advance; the yardstick is `profile`, which runs an exact distance transform where this call reads the masks twice.
The functions are timed in turns so that a drift of the clock falls on all alike.

    python tests/tools/bench_morphometry.py [--batch 16] [--size 512] [--sectors 72] [--reps 20] [--out FILE]
    python tests/tools/bench_morphometry.py --only morphometry     # under `rocprofv3 --kernel-trace --stats` for the kernels' own times
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
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import morphometry_ref as mr  # noqa: E402
from bench_surface import inputs  # noqa: E402
from bench_surface_profile import timed_in_turns  # noqa: E402
from uda_clr_amd import ops  # noqa: E402
from uda_clr_amd.utils import Utils, metrics  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--sectors", type=int, default=72)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only", choices=["morphometry"], default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_morphometry.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    B, S, Ks = args.batch, args.size, args.sectors
    prob, gt = inputs(B, S, dev)
    masks = Utils.postprocessing_batch(prob)
    gt_b = gt > 0.5
    K = ops.kernels()
    m8 = masks.contiguous()
    pair = torch.cat([m8, gt_b.to(torch.uint8)]).contiguous()
    table = metrics.sector_table(Ks)
    table_dev = torch.from_numpy(table).to(dev)
    fns = {"morphometry": lambda: ops.disc_morphometry(masks, Ks),
           "morphometry_kernels_only": lambda: K.disc_morphometry(m8, table_dev)}
    if args.only is None:
        from uda_clr_amd.networks.deeplabv3 import DeepLab
        torch.manual_seed(0)
        model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(dev).eval()
        image = torch.randn(B, 3, S, S, device=dev)

        def forward():
            with torch.no_grad():
                model(image)
        fns.update({"morphometry_pair": lambda: ops.disc_morphometry(pair, Ks),
                    "profile": lambda: ops.surface_profile(masks, gt_b, percentiles=(95,), tolerances=(2,)),
                    "forward": forward})
    out = {"batch": B, "size": S, "sectors": Ks, "device": torch.cuda.get_device_name(0)}
    out.update(timed_in_turns(fns, args.reps))
    got = ops.disc_morphometry(masks, Ks)
    want = mr.integers(masks[:2].cpu().numpy(), table)                                     # the timed size computes the right thing
    assert all(np.array_equal(got[k][:2], want[k]) for k in ("moments", "extent", "overlap", "radial"))
    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        f = metrics.morphometry_from_moments(got)
        wall.append((time.perf_counter() - t0) * 1e3)
    out["closed_forms"] = {"median_ms": statistics.median(wall), "min_ms": min(wall), "max_ms": max(wall), "reps": args.reps}
    out["set_pixels_per_image_mean"] = float(got["moments"][..., 0].sum(1).mean())
    out["mask_bytes"] = int(m8.numel())
    out["n_empty_sectors_max"] = float(f["n_empty_sectors"].max())
    if args.only is None:
        out["morphometry_below_profile"] = out["morphometry"]["median_ms"] < out["profile"]["median_ms"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
