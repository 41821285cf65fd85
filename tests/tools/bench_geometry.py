#!/usr/bin/env python
"""Measurements for UDA_CLR_DEVICE_INPUT=3 (profiles/geometry_kernels.md):

  worker   median ms per sample of the training chain (train_use_fix_initial.py:150-161) in ONE process on this host, at level 2
           (workers do the PIL geometry) and at level 3 (workers only draw), 800 x 800 sources, the same seeds, split by whether
           the scale branch fired;
  kernel   device-event time per call of the C entry uda_geometry_u8 (its tables pre-kernel + the gather / resample kernel, on
           preallocated buffers; windows of about 0.4 s each) at B = 32, S = 512 from 800 x 800 sources: every
           sample scaled by 0.5, every sample scaled by 1.5, none scaled; next to the algorithmic bytes (the source window of
           image and mask, 4 B per source pixel, plus 4 B per output pixel) and the resulting GB/s.  The first two samples of each
           case are compared with the numpy statement (tests/geometry_spec.py) at the timed size.

    python tests/tools/bench_geometry.py [worker] [kernel] [--samples 200] [--out FILE]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def worker(samples):
    from PIL import Image
    import geometry_cases as gc
    from make_golden_inputs import fundus_u8
    from uda_clr_amd.dataloaders import custom_transforms as tr
    img, lab = fundus_u8(1, 800, 800, 605)
    src = {"image": Image.fromarray(img[0]), "label": Image.fromarray(lab[0]), "img_name": "s", "src_index": 0}
    random.seed(1)
    chain = gc.train_chain(512)
    times = {2: {0: [], 1: []}, 3: {0: [], 1: []}}
    for i in range(samples):
        fired = None
        for lvl in (3, 2):
            random.seed(1000 + i); np.random.seed(1000 + i)
            with gc.level(lvl):
                t0 = time.perf_counter()
                s = chain({k: v for k, v in src.items() if lvl >= 3 or k != "src_index"})
                dt = (time.perf_counter() - t0) * 1e3
            if lvl == 3:
                fired = int(s["geom"][tr.GEOM_SCALED])
            times[lvl][fired].append(dt)
    out = {"samples": samples}
    for lvl in (2, 3):
        for fired in (0, 1):
            out["level%d_scale%d_median_ms" % (lvl, fired)] = statistics.median(times[lvl][fired])
        out["level%d_median_ms" % lvl] = statistics.median(times[lvl][0] + times[lvl][1])
    out["n_scale_fired"] = len(times[3][1])
    out["ratio_level2_over_level3"] = out["level2_median_ms"] / out["level3_median_ms"]
    return out


def kernel(windows=7, target_ms=400.0):
    import torch
    import geometry_spec as gs
    from uda_clr_amd import ops
    assert torch.cuda.is_available(), "the kernel measurement needs the GPU"
    dev = torch.device("cuda:0")
    B, S, H0, n_src = 32, 512, 800, 32
    rs = np.random.RandomState(3)
    imgs = [rs.randint(0, 256, (H0, H0, 3)).astype(np.uint8) for _ in range(n_src)]
    labs = [rs.randint(0, 256, (H0, H0)).astype(np.uint8) for _ in range(n_src)]
    pool = ops.SourcePool(imgs, labs, dev)
    K = ops.kernels()
    out = {}
    for name, wh in (("scale_0.5", (int(0.5 * H0),) * 2), ("scale_1.5", (int(1.4999 * H0),) * 2), ("unscaled", None)):
        recs, src_px = [], 0
        for b in range(B):
            w = wh[0] if wh else H0
            pad = (S - w) // 2 + 5 if w < S else 0
            hi = w + 2 * pad - S
            recs.append([int(bool(wh)), w if wh else 0, w if wh else 0, pad, rs.randint(0, hi + 1), rs.randint(0, hi + 1), rs.randint(4),
                         rs.randint(2), rs.randint(2), S])
            side = min(S, w) * (H0 / float(w))                  # source pixels under the window, per axis
            src_px += side * side
        recs = np.array(recs, np.int32)
        idx = np.arange(B, dtype=np.int64) % n_src
        r_dev, i_dev = torch.from_numpy(recs).to(dev), torch.from_numpy(idx).to(dev)
        iu, lu = K.geometry_u8(pool.image_pool, pool.label_pool, pool.offsets, pool.sizes, i_dev, r_dev, S)
        torch.cuda.synchronize()
        wi, wl = gs.geometry_batch(recs[:2], idx[:2], imgs, labs)
        assert np.array_equal(iu[:2].cpu().numpy(), wi) and np.array_equal(lu[:2].cpu().numpy(), wl), name
        # the timed call is the C entry alone (tables pre-kernel + main kernel) on preallocated outputs and workspace
        ws = torch.empty(int(K.lib.uda_geometry_u8_workspace_bytes(B, S)), dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        args = (pool.image_pool.data_ptr(), pool.label_pool.data_ptr(), pool.offsets.data_ptr(), pool.sizes.data_ptr(), n_src,
                i_dev.data_ptr(), r_dev.data_ptr(), B, S, iu.data_ptr(), lu.data_ptr(), ws.data_ptr(), ws.numel(), stream)
        run = lambda: K.lib.uda_geometry_u8(*args)
        assert run() == 0

        def window(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                run()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n                      # ms per call

        window(50)                                              # warm-up
        calls = max(200, int(target_ms / max(window(200), 1e-4)))          # each timed window lasts about target_ms
        per_call = [window(calls) for _ in range(windows)]
        assert np.array_equal(iu[:2].cpu().numpy(), wi), name
        nbytes = 4.0 * src_px + 4.0 * B * S * S
        med = statistics.median(per_call)
        out[name] = {"median_us": med * 1e3, "min_us": min(per_call) * 1e3, "max_us": max(per_call) * 1e3,
                     "algorithmic_MB": nbytes / 1e6, "GBps": nbytes / (med * 1e-3) / 1e9, "calls_per_window": calls, "windows": windows}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="*", default=["worker", "kernel"])
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if "worker" in a.what:
        res["worker"] = worker(a.samples)
    if "kernel" in a.what:
        res["kernel"] = kernel()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
