"""Shared by tests/test_geometry_cpu.py and tests/test_geometry_gpu.py: the fixture of tests/golden/make_golden_geometry.py
(outputs of the reference's RandomScaleCrop -> RandomRotate -> RandomFlip), its sources rebuilt from their seeds, the repo's
chain run at a given UDA_CLR_DEVICE_INPUT level, and numpy stand-ins for the device ops of TrainerBase._decode."""
import contextlib
import functools
import hashlib
import json
import os
import random

import numpy as np
import torch
from PIL import Image

import geometry_spec as gs
from make_golden_inputs import fundus_u8
from uda_clr_amd.dataloaders import custom_transforms as tr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(GOLDEN, "geometry.json")) as f:
        meta = json.load(f)
    return meta, dict(np.load(os.path.join(GOLDEN, "geometry.npz")))


@functools.lru_cache(maxsize=None)
def source(H0, W0, seed):
    img, lab = fundus_u8(1, H0, W0, seed)
    img, lab = img[0], lab[0]
    img.setflags(write=False)
    lab.setflags(write=False)
    return img, lab


def case_source(case):
    return source(case["H0"], case["W0"], case["src_seed"])


def digest(a):
    a = np.ascontiguousarray(a)
    return "%s%s:%s" % (a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest())


@contextlib.contextmanager
def level(n):
    old = tr.DEVICE_TAIL
    tr.DEVICE_TAIL = n
    try:
        yield
    finally:
        tr.DEVICE_TAIL = old


def run_geometry(case, lvl):
    """The repo's three geometric transforms from the case's seed, as the fixture's generator ran the reference's.  Level 0:
    (image, mask) arrays.  Level 3: the int32 record Normalize_tf emits.  Also the generators' states afterwards."""
    img, lab = case_source(case)
    with level(lvl):
        random.seed(case["py_seed"])
        np.random.seed(case["py_seed"])
        rot = tr.RandomRotate()
        assert rot.degree == case["degree"]
        s = {"image": Image.fromarray(img), "label": Image.fromarray(lab), "img_name": "s"}
        if lvl >= 3:
            s["src_index"] = 0
        for t in (tr.RandomScaleCrop(case["S"]), rot, tr.RandomFlip()):
            s = t(s)
        state = (random.getstate(), np.random.get_state())
        if lvl >= 3:
            return tr.Normalize_tf()(s)["geom"], state
        return (np.array(s["image"]), np.array(s["label"])), state


def same_state(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def record_from_outcome(o, S):
    return np.array([o["scaled"], o["w"] if o["scaled"] else 0, o["h"] if o["scaled"] else 0, o["pad"], o["x1"], o["y1"], o["turns"],
                     o["flip_lr"], o["flip_tb"], S], np.int32)


def make_record(rs, H0, W0, S, scaled=None, wh=None):
    """A seeded record drawn the way the transforms draw: sizes in [0.5, 1.5) of the source, the reference's pad rule, a crop
    origin inside the padded image, any quarter turn and flips."""
    scaled = bool(rs.randint(2)) if scaled is None else scaled
    w, h = W0, H0
    if scaled:
        w, h = wh if wh is not None else (int(rs.uniform(0.5, 1.5) * W0), int(rs.uniform(0.5, 1.5) * H0))
    pad = int(max((S - w) // 2 + 5, (S - h) // 2 + 5)) if (w < S or h < S) else 0
    pw, ph = w + 2 * pad, h + 2 * pad
    x1, y1 = int(rs.randint(0, pw - S + 1)), int(rs.randint(0, ph - S + 1))
    return np.array([int(scaled), w if scaled else 0, h if scaled else 0, pad, x1, y1, rs.randint(4), rs.randint(2), rs.randint(2), S], np.int32)


# ---------------------------------------------------------------------------- numpy stand-ins for HipOps (CPU tests of _decode)
class NumpyOps(object):
    """What TrainerBase._decode calls, on the numpy statements: geometry_spec for uda_geometry_u8, the recorded photometric
    outcomes applied with numpy, the CPU Normalize_tf for uda_normalize_tf.  The elastic transform must not have fired."""
    calls = None

    def __init__(self):
        self.calls = []

    def SourcePool(self, images, labels, device):
        self.calls.append("upload")
        return [np.asarray(i) for i in images], [np.asarray(l) for l in labels]

    def geometry_u8(self, pool, src_index, records):
        self.calls.append("geometry")
        iu, lu = gs.geometry_batch(records.numpy().reshape(-1, gs.GEOM_R), src_index.numpy().reshape(-1), pool[0], pool[1])
        return torch.from_numpy(iu), torch.from_numpy(lu)

    def elastic_deform(self, iu, lu, apply=None, noise=None):
        self.calls.append("elastic")
        assert not bool(apply.any()), "the numpy stand-in has no elastic transform"
        return iu, lu

    def photometric_u8(self, iu, pos, n, val, lut, erase):
        self.calls.append("photometric")
        out = []
        for b in range(iu.shape[0]):
            img = iu[b].numpy().copy()
            p = pos[b].numpy()[:int(n.reshape(-1)[b])]
            img[p[:, 0], p[:, 1], :] = int(val.reshape(-1)[b])
            img = lut[b].numpy()[img]
            top, left, h, w, v = [int(x) for x in erase[b]]
            if h > 0:
                img[top:top + h, left:left + w, :] = v
            out.append(img)
        return torch.from_numpy(np.stack(out))

    def normalize_tf(self, iu, lu):
        self.calls.append("normalize_tf")
        with level(0):
            outs = [tr.ToTensor()(tr.Normalize_tf()({"image": i.numpy(), "label": l.numpy(), "img_name": ""})) for i, l in zip(iu, lu)]
        return tuple(torch.stack([o[k] for o in outs]) for k in ("image", "map", "boundary"))


class Compose(object):
    def __init__(self, ts):
        self.ts = ts

    def __call__(self, s):
        for t in self.ts:
            s = t(s)
        return s


def train_chain(S):
    """train_use_fix_initial.py:150-161; RandomRotate draws its degree here"""
    return Compose([tr.RandomScaleCrop(S), tr.RandomRotate(), tr.RandomFlip(), tr.elastic_transform(), tr.add_salt_pepper_noise(),
                    tr.adjust_light(), tr.eraser(), tr.Normalize_tf(), tr.ToTensor()])


def paired_samples(ds, per_index, first_seed=0):
    """For every dataset index the first ``per_index`` seeds at which the elastic transform does not fire (its noise has no
    reproducible stream): the level-3 sample (records) and the level-0 sample (the CPU chain's tensors) from the same seed, with
    the generators' states after each."""
    out = []
    for idx in range(len(ds)):
        found, seed = 0, first_seed + 1000 * idx
        while found < per_index:
            seed += 1
            random.seed(seed); np.random.seed(seed)
            with level(3):
                got = ds[idx]
            st3 = (random.getstate(), np.random.get_state())
            if int(got["aug_elastic"][0]):
                continue
            random.seed(seed); np.random.seed(seed)
            with level(0):
                want = ds[idx]
            st0 = (random.getstate(), np.random.get_state())
            assert same_state(st3, st0), (idx, seed)
            out.append((got, want))
            found += 1
    return out


def collate(samples):
    return torch.utils.data.default_collate(samples)
