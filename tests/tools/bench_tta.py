"""Times of the test-time-augmentation kernels on the device, in one process, with device events:

    python tests/tools/bench_tta.py [--batch 16] [--size 512] [--specs d4 flips,id@0.75,id@1.25] [--windows 7] [--reps 20] [--json PATH]

  * per view list: uda_tta_fuse (mean and std; all five outputs) against uda_mc_uncertainty on the same count of logit tensors of the
    frame's size, alternating - the kernel of the parent is the yardstick: both read V tensors once and write the same maps;
  * for d4: the four mirrored views alone against the four transposed views alone (the same bytes: what the LDS rectangle costs);
  * uda_tta_view per view, summed;
  * the whole tta_predict beside the forwards it wraps (tta_logits alone) on a MobileNetV2 DeepLab.

Every figure is the median over ``--windows`` windows of ``--reps`` back-to-back calls between two device events, after a warm-up of
every shape; min and max over the windows say how far a difference can be trusted.  Bytes are the algorithm's, from the shapes: every
view's logits once plus the outputs."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))

from bench_uncertainty import compare  # noqa: E402
from uda_clr_amd import ops, tta  # noqa: E402


def _rows(t, nbytes):
    return {k: {"us": v[0], "us_min": v[1], "us_max": v[2], "bytes": nbytes[k], "TB_per_s": nbytes[k] / v[0] * 1e-6} for k, v in t.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--specs", nargs="+", default=["d4", "flips,id@0.75,id@1.25"])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-model", action="store_true", help="kernels only: skip tta_predict on the DeepLab")
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_tta needs the MI355X: there is nothing to time without it")
    dev = torch.device("cuda:0")
    K = ops.kernels()
    B, S = args.batch, args.size
    g = torch.Generator().manual_seed(0)
    n = B * 2 * S * S
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "size": S, "windows": args.windows, "reps": args.reps, "specs": {}}
    image = torch.randn(B, 3, S, S, generator=g).to(dev)
    model = None
    if not args.no_model:
        from uda_clr_amd.networks.deeplabv3 import DeepLab
        torch.manual_seed(0)
        model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(dev).eval()

    for spec in args.specs:
        views = tta.parse_views(spec, S, S)
        V = len(views)
        logits = [(4.0 * torch.randn((B, 2) + tta.view_shape(v), generator=g)).to(dev) for v in views]
        stack = (4.0 * torch.randn(V, B, 2, S, S, generator=g)).to(dev)
        read = sum(t.numel() for t in logits) * 4
        all5 = ("mean", "std", "entropy", "mi")
        fns = {"tta_fuse mean+std": lambda: K.tta_fuse(logits, views, (S, S), ("mean", "std")),
               "mc_uncertainty mean+std": lambda: K.mc_uncertainty(stack, ("mean", "std")),
               "tta_fuse all five": lambda: K.tta_fuse(logits, views, (S, S), all5, u8_scale=1600.0),
               "mc_uncertainty all five": lambda: K.mc_uncertainty(stack, all5, u8_scale=1600.0)}
        nbytes = {"tta_fuse mean+std": read + 2 * n * 4, "mc_uncertainty mean+std": (V + 2) * n * 4,
                  "tta_fuse all five": read + 4 * n * 4 + n, "mc_uncertainty all five": (V + 4) * n * 4 + n}
        row = {"views": [list(v) for v in views], "fuse": _rows(compare(fns, args.windows, args.reps), nbytes)}
        halves = {"mirrored": [i for i, v in enumerate(views) if not v[0] & 4 and v[1:] == (S, S)],
                  "transposed": [i for i, v in enumerate(views) if v[0] & 4 and v[1:] == (S, S)]}
        if len(halves["mirrored"]) >= 2 and len(halves["mirrored"]) == len(halves["transposed"]):
            def half(idx):
                return lambda: K.tta_fuse([logits[i] for i in idx], [views[i] for i in idx], (S, S), ("mean", "std"))
            hb = (len(halves["mirrored"]) + 2) * n * 4
            row["halves"] = _rows(compare({k + " half": half(idx) for k, idx in halves.items()}, args.windows, args.reps),
                                  {k + " half": hb for k in halves})
        vt = compare({"%s %dx%d" % (tta.NAMES[v[0]], v[1], v[2]): (lambda v=v: K.tta_view(image, v)) for v in views}, args.windows, args.reps)
        row["view"] = {k: {"us": t[0], "us_min": t[1], "us_max": t[2]} for k, t in vt.items()}
        row["view_total_us"] = sum(t[0] for t in vt.values())
        if model is not None:
            def forwards():
                with torch.no_grad():
                    return tta.tta_logits(model, image, views)

            def whole():
                with torch.no_grad():
                    return tta.tta_predict(model, image, views, outputs=("mean", "std"))

            def one():
                with torch.no_grad():
                    return model(image)
            t = compare({"tta_predict": whole, "tta_logits (views + forwards)": forwards, "one eval forward": one}, 3, 2)
            row["predict"] = {k: {"ms": v[0] / 1000.0, "ms_min": v[1] / 1000.0, "ms_max": v[2] / 1000.0} for k, v in t.items()}
        out["specs"][spec] = row
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
