#!/usr/bin/env python
"""What the whole-photograph stage costs (profiles/wholephoto_kernels.md): in one process, device events, warmed, the median of
repeated single calls, at B = 16 synthetic 2048 x 2048 photographs, ROI 800 -> 512:

  reduce    HipKernels.photo_reduce, both outputs      floor: reads 3 H W, writes 15 S^2 per photograph
  cut       HipKernels.roi_cut, both outputs           floor: reads 3 (R + 5)^2, writes 15 S^2
  paste     HipKernels.roi_paste                       floor: reads 2 S^2, writes H W
  stage     ops.photo_reduce -> boxes (host) -> ops.roi_cut -> ops.roi_paste: everything of predict_photos that is not a forward or
            the existing pipeline, the small copies to and from the host included
  forward   the MobileNetV2 DeepLab eval forward under no_grad at [B,3,S,S] (predict_photos runs it twice)
  upload    ops.PhotoPool of the batch (host wall clock, the copy of 3 H W bytes per photograph included)
  host_*    the same outputs on the host with Pillow and numpy (wall clock, per batch): block means by reshape, crop().resize(),
            v / 127.5 - 1, the restated paste rule

The achieved GB/s are the floors' bytes over the median time.  No time is fixed in advance.  The device outputs of the first
photograph are compared with the host's, byte for byte, at the timed size.

    python tests/tools/bench_wholephoto.py [--batch 16] [--side 2048] [--roi 800] [--size 512] [--reps 20] [--out FILE]
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

import wholephoto_ref as wr  # noqa: E402
from bench_surface_profile import timed_in_turns  # noqa: E402
from uda_clr_amd import ops, wholephoto  # noqa: E402


def photographs(B, side, seed=0):
    """B synthetic photographs [side, side, 3]: smooth noise, a bright disc and a brighter cup somewhere; -> (images, centres (cy, cx))"""
    rng = np.random.RandomState(seed)
    base = rng.randint(0, 64, (side, side, 3)).astype(np.uint8)
    r, c = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    out, centres = [], []
    for b in range(B):
        cy, cx = (int(v) for v in rng.randint(side // 4, 3 * side // 4, 2))
        img = np.roll(base, b * 37, 1).copy()
        d2 = (r - cy) ** 2 + (c - cx) ** 2
        img[d2 <= (side // 12) ** 2] += 100
        img[d2 <= (side // 30) ** 2] += 80
        out.append(img)
        centres.append((cy, cx))
    return out, np.array(centres, np.int64)


def host_reduce(img, S):
    """wr.reduce_photo for a side that the factor divides, by reshape"""
    H, W = img.shape[:2]
    f = wr.factor_of(H, W, S)
    assert H % f == 0 and W % f == 0
    m = (img.reshape(H // f, f, W // f, f, 3).astype(np.uint32).sum((1, 3)) + f * f // 2) // (f * f)
    canvas = np.zeros((S, S, 3), np.uint8)
    canvas[:H // f, :W // f] = m
    return canvas


def host_normalise(u8):
    return np.ascontiguousarray(np.moveaxis(u8.astype(np.float32) / np.float32(127.5) - np.float32(1.0), -1, 0))


def host_cut(img, box, S):
    from PIL import Image
    x0, y0, R = (int(v) for v in box)
    return np.asarray(Image.fromarray(img).crop((x0, y0, x0 + R, y0 + R)).resize((S, S), Image.BILINEAR))


def wall(fn, reps):
    fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--side", type=int, default=2048)
    ap.add_argument("--roi", type=int, default=800)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_wholephoto.py measures on the MI355X; no device found")
    dev = torch.device("cuda:0")
    B, side, R, S = args.batch, args.side, args.roi, args.size
    images, centres = photographs(B, side)
    pool = ops.PhotoPool(images, dev)
    bx_host = wholephoto.boxes(centres, pool.sizes_host, R)
    bx = torch.from_numpy(bx_host).to(dev)
    idx = torch.arange(B, dtype=torch.int64, device=dev)
    masks_host = np.stack([wr.mask_cases(b, S)[0][1] for b in range(B)])
    masks = torch.from_numpy(masks_host).to(dev)
    sizes_dev = pool.sizes
    starts = torch.arange(B, dtype=torch.int64, device=dev) * side * side
    K = ops.kernels()

    def stage():
        ops.photo_reduce(pool, size=S, outputs=("f32",))["factor"].cpu()
        b = torch.from_numpy(wholephoto.boxes(centres, pool.sizes_host, R))
        ops.roi_cut(pool, b, size=S)
        ops.roi_paste(pool, masks, b)

    from uda_clr_amd.networks.deeplabv3 import DeepLab
    torch.manual_seed(0)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(dev).eval()
    image = torch.randn(B, 3, S, S, device=dev)

    def forward():
        with torch.no_grad():
            model(image)

    fns = {"reduce": lambda: K.photo_reduce(pool.pool, pool.offsets, pool.sizes, idx, S, ("u8", "f32")),
           "cut": lambda: K.roi_cut(pool.pool, pool.offsets, pool.sizes, idx, bx, S, ("u8", "f32")),
           "paste": lambda: K.roi_paste(masks, bx, sizes_dev, starts, B * side * side),
           "stage": stage, "forward": forward}
    out = {"batch": B, "side": side, "roi": R, "size": S, "device": torch.cuda.get_device_name(0)}
    out.update(timed_in_turns(fns, args.reps))
    floors = {"reduce": B * (3 * side * side + 15 * S * S), "cut": B * (3 * (R + 5) ** 2 + 15 * S * S), "paste": B * (2 * S * S + side * side)}
    for k, nbytes in floors.items():
        out[k]["floor_bytes"] = nbytes
        out[k]["achieved_GBps"] = nbytes / (out[k]["median_ms"] * 1e-3) / 1e9

    # the timed size computes the right thing (first photograph, against the host's outputs)
    red = ops.photo_reduce(pool, index=[0], size=S, outputs=("u8", "f32"))
    roi = ops.roi_cut(pool, bx_host[:1], index=[0], size=S)
    pasted = ops.roi_paste(pool, masks[:1], bx_host[:1], index=[0])[0]
    assert np.array_equal(red["u8"][0].cpu().numpy(), host_reduce(images[0], S)) and int(red["factor"][0]) == wr.factor_of(side, side, S)
    assert np.array_equal(roi["u8"][0].cpu().numpy(), host_cut(images[0], bx_host[0], S))
    assert np.array_equal(roi["f32"][0].cpu().numpy().view(np.int32), wr.normalise(host_cut(images[0], bx_host[0], S)).view(np.int32))
    assert np.array_equal(pasted.cpu().numpy(), wr.paste(masks_host[0], bx_host[0], side, side))

    out["upload"] = wall(lambda: (ops.PhotoPool(images, dev), torch.cuda.synchronize()), args.host_reps)
    out["host_reduce"] = wall(lambda: [host_normalise(host_reduce(i, S)) for i in images], args.host_reps)
    out["host_cut"] = wall(lambda: [host_normalise(host_cut(i, b, S)) for i, b in zip(images, bx_host)], args.host_reps)
    out["host_paste"] = wall(lambda: [wr.paste(m, b, side, side) for m, b in zip(masks_host, bx_host)], args.host_reps)
    out["host_stage_ms"] = out["host_reduce"]["median_ms"] + out["host_cut"]["median_ms"] + out["host_paste"]["median_ms"]
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
