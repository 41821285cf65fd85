"""Times of the evaluation-side uncertainty kernels on the device, in one process, with device events:

    python tests/tools/bench_uncertainty.py [--batch 16] [--passes 8] [--size 512] [--windows 7] [--reps 20] [--json PATH]

  * uda_mc_uncertainty with std and mean only against uda_mc_stats on the same logits (the existing kernel of the same traffic:
    (T + 2) * n * 4 bytes), alternating, and uda_mc_uncertainty with all five outputs ((T + 4) * n * 4 + n bytes);
  * uda_selective_tables (both tables) against the torch composition of the same tables on the device (floor / bucketize + bincount),
    checked for equality first, on a fundus-like batch (background runs of p = 0) and on a batch of white noise (a new bin at
    nearly every pixel: the worst case of the run-length design);
  * both beside the T stochastic forwards of a MobileNetV2 DeepLab (DeepLab.mc_inference_logits) on the same batch.

Every figure is the median over ``--windows`` windows of ``--reps`` back-to-back calls between two device events, after a warm-up of
every shape; min and max over the windows say how far a difference can be trusted.  Bytes are the algorithm's, from the shapes."""
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

EDGES = ops.DEFAULT_UNC_EDGES


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


def fundus_like(T, B, S, dev, g):
    """[T,B,2,S,S] logits: -8 background, +8 inside a disc, a soft edge, per-pass noise; and ground truth of a shifted disc"""
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    base, gt = torch.empty(B, 2, S, S), torch.empty(B, 2, S, S, dtype=torch.bool)
    for b in range(B):
        cy, cx = (0.4 + 0.2 * torch.rand(2, generator=g)) * S
        for c, r in enumerate((0.12 * S, 0.22 * S)):
            d = torch.hypot(yy - cy, xx - cx)
            base[b, c] = torch.clamp((r - d) * 0.5, -8.0, 8.0)
            gt[b, c] = torch.hypot(yy - cy - 3.0, xx - cx + 2.0) < r
    noise = torch.randn(T, B, 2, S, S, generator=g) * torch.exp(-base.abs() / 3.0)
    return (base[None] + noise).to(dev).contiguous(), gt.to(dev)


def torch_tables(prob, unc, pred, gt, M, edges_dev):
    """the same int64 tables by floor / bucketize + bincount (float64 weights: exact below 2^53)"""
    B = prob.shape[0]
    plane = torch.arange(B * 2, device=prob.device).view(B, 2, 1, 1)
    ok = (prob >= 0) & (prob <= 1)
    b = torch.clamp(torch.floor(prob * float(M)), max=M - 1).long()
    q = torch.round(prob * 65536.0).double()
    g = gt.double()
    idx = (plane * M + b)[ok]
    cols = [torch.bincount(idx, weights=w[ok] if w is not None else None, minlength=B * 2 * M) for w in (None, g, q, q * g, q * q)]
    rel = torch.stack([c.long() if c.dtype != torch.int64 else c for c in cols], -1).view(B, 2, M, 5)
    K = edges_dev.numel() + 1
    oku = unc >= 0
    k = torch.bucketize(unc, edges_dev, right=True)
    code = torch.where(pred, torch.where(gt, 0, 1), torch.where(gt, 2, 3))
    risk = torch.bincount(((plane * K + k) * 4 + code)[oku], minlength=B * 2 * K * 4).view(B, 2, K, 4)
    return rel, risk


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_uncertainty needs the MI355X: there is nothing to time without it")
    dev = torch.device("cuda:0")
    K = ops.kernels()
    B, T, S = args.batch, args.passes, args.size
    g = torch.Generator().manual_seed(0)
    logits, gt = fundus_like(T, B, S, dev, g)
    n = logits[0].numel()
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "passes": T, "size": S, "windows": args.windows, "reps": args.reps}

    # ---- the streaming kernel
    flat = logits.view(T * B, 2, S, S)
    t = compare({"mc_stats": lambda: K.mc_stats(flat, T),
                 "mc_uncertainty std+mean": lambda: K.mc_uncertainty(logits, ("mean", "std")),
                 "mc_uncertainty all five": lambda: K.mc_uncertainty(logits, ("mean", "std", "entropy", "mi"), u8_scale=1600.0)},
                args.windows, args.reps)
    sd, mn = K.mc_stats(flat, T)
    new = K.mc_uncertainty(logits, ("mean", "std"))
    out["max |std - mc_stats std|"] = float((new["std"] - sd.view_as(new["std"])).abs().max())
    out["max |mean - mc_stats mean|"] = float((new["mean"] - mn.view_as(new["mean"])).abs().max())
    nbytes = {"mc_stats": (T + 2) * n * 4, "mc_uncertainty std+mean": (T + 2) * n * 4, "mc_uncertainty all five": (T + 4) * n * 4 + n}
    out["streaming"] = {k: {"us": v[0], "us_min": v[1], "us_max": v[2], "bytes": nbytes[k], "TB_per_s": nbytes[k] / v[0] * 1e-6} for k, v in t.items()}

    # ---- the histogram kernel
    full = K.mc_uncertainty(logits, ("mean", "std"))
    edges_dev = torch.tensor(EDGES, dtype=torch.float32, device=dev)
    cases = {"fundus-like": (full["mean"], full["std"], (full["mean"] > 0.5), gt),
             "white noise": (torch.rand(B, 2, S, S, generator=g).to(dev), (0.2 * torch.rand(B, 2, S, S, generator=g)).to(dev),
                             (torch.rand(B, 2, S, S, generator=g) > 0.5).to(dev), (torch.rand(B, 2, S, S, generator=g) > 0.5).to(dev))}
    out["tables"] = {}
    for name, (prob, unc, pred, truth) in cases.items():
        p8, g8 = pred.to(torch.uint8).contiguous(), truth.to(torch.uint8).contiguous()
        rel, risk, _ = K.selective_tables(prob, unc, p8, g8, 15, EDGES)
        rel_t, risk_t = torch_tables(prob, unc, pred, truth, 15, edges_dev)
        same = bool(torch.equal(rel, rel_t) and torch.equal(risk, risk_t))
        t = compare({"uda_selective_tables": lambda: K.selective_tables(prob, unc, p8, g8, 15, EDGES),
                     "torch bucketize + bincount": lambda: torch_tables(prob, unc, pred, truth, 15, edges_dev)}, args.windows, max(args.reps // 4, 2))
        tb = 2 * n * 4 + 2 * n
        out["tables"][name] = {"equal_to_torch": same, "bytes": tb,
                               **{k: {"us": v[0], "us_min": v[1], "us_max": v[2], "TB_per_s": tb / v[0] * 1e-6} for k, v in t.items()}}

    # ---- beside the T forwards
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    torch.manual_seed(0)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(dev).eval()
    x = torch.randn(B, 3, S, S, generator=g).to(dev)

    def eval_forward():
        with torch.no_grad():
            return model(x)
    t = compare({"T forwards (mc_inference_logits)": lambda: model.mc_inference_logits(x, T), "one eval forward": eval_forward}, 3, 2)
    out["forwards"] = {k: {"ms": v[0] / 1000.0, "ms_min": v[1] / 1000.0, "ms_max": v[2] / 1000.0} for k, v in t.items()}
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
