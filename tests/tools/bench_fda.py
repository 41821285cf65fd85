"""Times of the Fourier style transfer on the device, in one process, with device events:

    python tests/tools/bench_fda.py [--batch 16] [--targets 16] [--size 512] [--bands 5 46] [--windows 7] [--reps 20] [--json PATH]

  * ops.fda_transfer (csrc/fda.hip) beside the same transfer written with torch.fft.fft2 / ifft2 on float64 copies of both batches on
    the same device, alternating - the torch formulation is the yardstick;
  * ops.fda_spectrum of the source and target images together: the share of the row and column passes;
  * the bytes-over-bandwidth floor: both uint8 batches read once for the spectra, the source read again and the output written.

Every figure is the median over ``--windows`` windows of ``--reps`` back-to-back calls between two device events, after a warm-up of
every shape; min and max over the windows say how far a difference can be trusted.  The two formulations' bytes are compared as well
(they may differ where a value lies within the two float64 paths' disagreement of a tie; the count is reported)."""
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
from uda_clr_amd import ops  # noqa: E402

HBM_TB_PER_S = 8.0            # MI355X peak


def torch_fda(src, tgt, band, pair):
    """the literal statement with torch.fft on float64 copies: uint8 [B,H,W,3] x uint8 [Bt,H,W,3] -> uint8 [B,H,W,3]"""
    H, W = src.shape[1:3]
    s = src.permute(0, 3, 1, 2).double()
    t = tgt[pair].permute(0, 3, 1, 2).double()
    fs = torch.fft.fftshift(torch.fft.fft2(s), dim=(-2, -1))
    ft = torch.fft.fftshift(torch.fft.fft2(t), dim=(-2, -1))
    amp, pha = fs.abs(), fs.angle()
    ys, xs = slice(H // 2 - band, H // 2 + band + 1), slice(W // 2 - band, W // 2 + band + 1)
    pha[..., ys, xs] = torch.where(amp[..., ys, xs] <= 1e-6 * H * W, torch.zeros_like(pha[..., ys, xs]), pha[..., ys, xs])
    amp[..., ys, xs] = ft.abs()[..., ys, xs]
    out = torch.fft.ifft2(torch.fft.ifftshift(torch.polar(amp, pha), dim=(-2, -1))).real
    return out.round().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def fundus_like(n, S, g):
    """uint8 [n,S,S,3]: a bright disc on a vignetted background with noise, per image its own colour cast"""
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    out = torch.empty(n, S, S, 3)
    for i in range(n):
        cy, cx = (0.4 + 0.2 * torch.rand(2, generator=g)) * S
        d = torch.hypot(yy - cy, xx - cx) / S
        cast = 0.5 + 0.5 * torch.rand(3, generator=g)
        base = 0.75 * torch.exp(-d * d * 6.0) + 0.25 * (d < 0.2).float()
        out[i] = base[..., None] * cast + 0.05 * torch.randn(S, S, 3, generator=g)
    return (out.clamp_(0, 1) * 255).round().to(torch.uint8)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--targets", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--bands", type=int, nargs="+", default=[5, 46])
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_fda needs the MI355X: there is nothing to time without it")
    dev = torch.device("cuda:0")
    B, Bt, S = args.batch, args.targets, args.size
    g = torch.Generator().manual_seed(0)
    src, tgt = fundus_like(B, S, g).to(dev), fundus_like(Bt, S, g).to(dev)
    both = torch.cat([src, tgt])
    pair = (torch.arange(B, dtype=torch.int32) % Bt).to(dev)
    nbytes = (B + Bt) * S * S * 3 + 2 * B * S * S * 3
    out = {"device": torch.cuda.get_device_name(0), "batch": B, "targets": Bt, "size": S, "windows": args.windows, "reps": args.reps,
           "bytes": nbytes, "floor_us_at_%g_TB_per_s" % HBM_TB_PER_S: nbytes / HBM_TB_PER_S * 1e-6, "bands": {}}
    for band in args.bands:
        hip, ref = ops.fda_transfer(src, tgt, band=band, pair=pair), torch_fda(src, tgt, band, pair.long())
        differ = int((hip != ref).sum())
        worst = int((hip.int() - ref.int()).abs().max())
        t = compare({"fda_transfer": lambda: ops.fda_transfer(src, tgt, band=band, pair=pair),
                     "torch.fft float64": lambda: torch_fda(src, tgt, band, pair.long()),
                     "fda_spectrum of both batches": lambda: ops.fda_spectrum(both, band)}, args.windows, args.reps)
        row = {k: {"us": v[0], "us_min": v[1], "us_max": v[2]} for k, v in t.items()}
        row["fda_transfer"]["TB_per_s"] = nbytes / t["fda_transfer"][0] * 1e-6
        row["torch_over_hip"] = t["torch.fft float64"][0] / t["fda_transfer"][0]
        row["bytes_differing_from_torch"], row["largest_difference"] = differ, worst
        out["bands"][str(band)] = row
    line = json.dumps(out)
    print(line)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(line + "\n")
    return out


if __name__ == "__main__":
    main()
