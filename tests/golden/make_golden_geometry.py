#!/usr/bin/env python
"""Generate tests/golden/geometry.npz + geometry.json from the REFERENCE's own dataloaders/custom_transforms.py
(:152-182 RandomCrop, :208-223 RandomFlip, :315-355 RandomRotate / RandomScaleCrop).

Run in the build container only (it imports the reference the way make_golden.py's `input` mode does; nothing of it is copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_geometry.py

Per case: random.seed(py_seed); RandomRotate() (draws its degree); RandomScaleCrop(S) -> RandomRotate -> RandomFlip on one seeded
source (tests/make_golden_inputs.fundus_u8(1, H0, W0, src_seed)[0]).  Stored: the seeds, the source shape, the degree, every draw
the transforms took from `random` (observed through a recording proxy), the outcome derived from them, and the output image and
mask - in full at S = 48 (geometry.npz), as SHA-256 at S = 512 from 800 x 800.  The seed search keeps a case when it covers a
branch no earlier case covers and asserts at the end that every branch is covered."""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

S_SMALL = 48
SOURCES = [(72, 80, 601), (64, 64, 602), (40, 40, 603), (48, 48, 604)]        # (H0, W0, src_seed)
REQUIRED = (["unscaled", "up_up", "down_down", "up_down", "pad_w", "pad_h", "small_unscaled", "exact_no_draw"]
            + ["deg%d" % d for d in (90, 180, 270, 360)] + ["flip%d%d" % (a, b) for a in (0, 1) for b in (0, 1)]
            + ["src72x80", "src64x64", "src40x40"])


class Recorder(object):
    """stands in for the `random` module inside the reference's file: same stream, every draw logged"""
    def __init__(self):
        self.log = []

    def random(self):
        v = random.random()
        self.log.append(["random", v])
        return v

    def uniform(self, a, b):
        v = random.uniform(a, b)
        self.log.append(["uniform", v])
        return v

    def randint(self, a, b):
        v = random.randint(a, b)
        self.log.append(["randint", v])
        return v


def run_case(rt, img, lab, S, py_seed):
    from PIL import Image
    rec = Recorder()
    rt.random = rec
    try:
        random.seed(py_seed)
        rot = rt.RandomRotate()
        s = {"image": Image.fromarray(img), "label": Image.fromarray(lab), "img_name": "s"}
        for t in (rt.RandomScaleCrop(S), rot, rt.RandomFlip()):
            s = t(s)
    finally:
        rt.random = random
    return rot.degree, rec.log, np.array(s["image"]), np.array(s["label"])


def outcome(log, degree, H0, W0, S):
    """what the draws mean, read off the log in the order the transforms take them"""
    it = iter(log)
    assert next(it)[0] == "randint"                                    # RandomRotate(): the degree
    o = {"scaled": int(next(it)[1] > 0.5), "w": W0, "h": H0, "pad": 0, "x1": 0, "y1": 0}
    if o["scaled"]:
        o["w"], o["h"] = int(next(it)[1] * W0), int(next(it)[1] * H0)
    w, h = o["w"], o["h"]
    if w < S or h < S:
        o["pad"] = int(max((S - w) // 2 + 5, (S - h) // 2 + 5))
        w, h = w + 2 * o["pad"], h + 2 * o["pad"]
    o["crop_drawn"] = int((w, h) != (S, S))
    if o["crop_drawn"]:
        o["x1"], o["y1"] = int(next(it)[1]), int(next(it)[1])
    o["rotated"] = int(next(it)[1] > 0.5)
    o["turns"] = (degree // 90) % 4 if o["rotated"] else 0
    o["flip_lr"], o["flip_tb"] = int(next(it)[1] < 0.5), int(next(it)[1] < 0.5)
    assert next(it, None) is None, "draws left over"
    return o


def tags(o, degree, H0, W0, S):
    t = {"src%dx%d" % (H0, W0), "flip%d%d" % (o["flip_lr"], o["flip_tb"])}
    if o["rotated"]:
        t.add("deg%d" % degree)
    if o["scaled"]:
        up = (o["w"] > W0, o["h"] > H0)
        down = (o["w"] < W0, o["h"] < H0)
        if all(up):
            t.add("up_up")
        if all(down):
            t.add("down_down")
        if (up[0] and down[1]) or (up[1] and down[0]):
            t.add("up_down")
        if o["w"] < S:
            t.add("pad_w")
        if o["h"] < S:
            t.add("pad_h")
    else:
        t.add("unscaled")
        if H0 < S and W0 < S:
            t.add("small_unscaled")
        if (H0, W0) == (S, S):
            t.add("exact_no_draw")
            assert not o["crop_drawn"]
    return t


def digest(a):
    import hashlib
    a = np.ascontiguousarray(a)
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


def main():
    import make_golden
    from make_golden_inputs import fundus_u8
    make_golden.install_reference()
    from dataloaders import custom_transforms as rt
    cases, arrays, covered = [], {}, set()
    for H0, W0, src_seed in SOURCES:
        img, lab = fundus_u8(1, H0, W0, src_seed)
        for py_seed in range(400):
            degree, log, oi, ol = run_case(rt, img[0], lab[0], S_SMALL, py_seed)
            o = outcome(log, degree, H0, W0, S_SMALL)
            new = (tags(o, degree, H0, W0, S_SMALL) & set(REQUIRED)) - covered
            if not new:
                continue
            covered |= new
            name = "c%02d" % len(cases)
            cases.append(dict(name=name, S=S_SMALL, py_seed=py_seed, src_seed=src_seed, H0=H0, W0=W0, degree=degree, draws=log,
                              outcome=o, covers=sorted(new)))
            arrays[name + ".image"], arrays[name + ".label"] = oi, ol
    missing = [t for t in REQUIRED if t not in covered]
    assert not missing, "the seed search left branches uncovered: %s" % missing
    # the real shape: S = 512 from 800 x 800, one case with the scale branch fired and one without, digests only
    img, lab = fundus_u8(1, 800, 800, 605)
    big, want = [], {0, 1}
    for py_seed in range(100):
        degree, log, oi, ol = run_case(rt, img[0], lab[0], 512, py_seed)
        o = outcome(log, degree, 800, 800, 512)
        if o["scaled"] in want:
            want.discard(o["scaled"])
            big.append(dict(name="big%d" % o["scaled"], S=512, py_seed=py_seed, src_seed=605, H0=800, W0=800, degree=degree, draws=log,
                            outcome=o, sha256={"image": digest(oi), "label": digest(ol)}))
    assert not want
    with open(os.path.join(HERE, "geometry.json"), "w") as f:
        json.dump({"cases": cases, "digest_cases": big, "required": REQUIRED}, f, indent=1, sort_keys=True)
    np.savez_compressed(os.path.join(HERE, "geometry.npz"), **arrays)
    print("geometry: %d full cases, %d digest cases, branches %s" % (len(cases), len(big), sorted(covered)))


if __name__ == "__main__":
    main()
