"""Time of the class-scatter kernel of the domain-gap report on the device, in one process, with device events:

    python tests/tools/bench_domain_gap.py [--batch 16] [--size 512] [--windows 7] [--reps 40] [--json PATH]

  * uda_proto_scatter on the features of one batch, [B, 305, size/4, size/4] (B = 16 at 512 x 512: P = 262144 pixels), with the
    share of the 155 TFLOP/s fp32-matrix rate it reaches, counting 4 * P * C^2 FLOP: one triangle of four classes;
  * uda_proto_reduce on the same features (the first moments that ``MomentAccumulator.update`` takes beside it);
  * the torch formulation of the same scatter, ((w_k * (F - a_k)).T @ (F - a_k) four times, fp32), checked against the kernel first;
  * the eval forward of a MobileNetV2 DeepLab on the same batch, which the call rides beside in ``domain_moments``.

Every figure is the median over ``--windows`` windows of ``--reps`` back-to-back calls between two device events, after a warm-up;
min and max over the windows say how far a difference can be trusted."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from uda_clr_amd import ops  # noqa: E402

F32_MATRIX_TFLOPS = 155.0
C = 305


def window(fn, reps):
    """microseconds per call of ``reps`` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps


def compare(fns, windows, reps):
    """{name: (median, min, max) us} of several callables, their windows alternating"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            times[k].append(window(fn, reps))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in times.items()}


def torch_scatter(rows, wts, centre):
    out = []
    for k in range(4):
        d = rows - centre[k]
        out.append((d * wts[:, k:k + 1]).t() @ d)
    return torch.stack(out)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_domain_gap needs the MI355X: there is nothing to time without it")
    dev = torch.device("cuda:0")
    K = ops.kernels()
    B, S = args.batch, args.size
    h = S // 4
    P = B * h * h
    g = torch.Generator(device=dev).manual_seed(0)
    rows = torch.empty(P, 308, device=dev)[:, :C]                            # the NHWC rows view of a [B, 305, h, h] feature
    rows.copy_(torch.randn(P, C, generator=g, device=dev) * 0.3 + 3.0)
    prob = torch.rand(B, 2, h, h, generator=g, device=dev)
    wts = K.proto_weights(0, B, h, h, map_=prob)[0]
    sums = torch.zeros(4, C + 1, dtype=torch.float64, device=dev)
    K.proto_reduce(rows, wts, sums)
    centre = K.proto_finalize(sums)
    scatter = torch.zeros(4, C, C, dtype=torch.float64, device=dev)
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "size": S, "pixels": P, "channels": C, "windows": args.windows, "reps": args.reps}

    K.proto_scatter(rows, wts, scatter, centre)
    ref = torch_scatter(rows, wts, centre)
    out["max |kernel - torch| / max |torch|"] = float((scatter - ref.double()).abs().max() / ref.abs().max())

    t = compare({"uda_proto_scatter": lambda: K.proto_scatter(rows, wts, scatter, centre),
                 "uda_proto_reduce": lambda: K.proto_reduce(rows, wts, sums),
                 "torch (w (F - a)).T @ (F - a) x 4": lambda: torch_scatter(rows, wts, centre)}, args.windows, args.reps)
    flop = 4.0 * P * C * C
    out["kernels"] = {k: {"us": v[0], "us_min": v[1], "us_max": v[2]} for k, v in t.items()}
    us = t["uda_proto_scatter"][0]
    out["scatter_flop"] = flop
    out["scatter_tflops"] = flop / us * 1e-6
    out["scatter_share_of_155TF"] = flop / us * 1e-6 / F32_MATRIX_TFLOPS

    from uda_clr_amd.networks.deeplabv3 import DeepLab
    torch.manual_seed(0)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(dev).eval()
    x = torch.randn(B, 3, S, S, generator=g, device=dev)

    def eval_forward():
        with torch.no_grad():
            return model(x)
    f = compare({"one eval forward": eval_forward}, 3, 2)["one eval forward"]
    out["forward"] = {"ms": f[0] / 1000.0, "ms_min": f[1] / 1000.0, "ms_max": f[2] / 1000.0}
    out["scatter_over_forward"] = us / f[0]
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            fh.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
