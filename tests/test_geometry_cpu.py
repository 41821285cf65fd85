"""not-gpu: UDA_CLR_DEVICE_INPUT=3, the device-side scale-crop / rotate / flip, on its numpy statement (tests/geometry_spec.py).

The fixture (tests/golden/geometry.*) holds what the REFERENCE's RandomScaleCrop(S) -> RandomRotate() -> RandomFlip() produce
from seeded sources; every comparison here is byte equality - the arithmetic is integer, there is no tolerance to choose."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

import geometry_cases as gc
import geometry_spec as gs
from uda_clr_amd.dataloaders import custom_transforms as tr
from uda_clr_amd.dataloaders import fundus_dataloader as DL
from uda_clr_amd.dataloaders.synthetic import write_dataset
from uda_clr_amd.train_process._common import TrainerBase

META, ARRAYS = gc.fixture()
CASES = META["cases"]


def test_fixture_covers_every_branch():
    covered = {t for c in CASES for t in c["covers"]}
    assert covered == set(META["required"]) and len(META["required"]) == 19
    assert {c["outcome"]["scaled"] for c in META["digest_cases"]} == {0, 1}
    assert {(c["H0"], c["W0"]) for c in CASES} >= {(72, 80), (64, 64), (40, 40), (48, 48)}


@pytest.mark.parametrize("case", CASES + META["digest_cases"], ids=lambda c: c["name"])
def test_level0_transforms_reproduce_the_reference_from_the_same_seeds(case):
    """pins the ORDER of the draws of the repo's geometric transforms against the reference's"""
    (img, lab), _ = gc.run_geometry(case, 0)
    if "sha256" in case:
        assert gc.digest(img) == case["sha256"]["image"] and gc.digest(lab) == case["sha256"]["label"]
    else:
        assert np.array_equal(img, ARRAYS[case["name"] + ".image"]) and np.array_equal(lab, ARRAYS[case["name"] + ".label"])


@pytest.mark.parametrize("case", CASES + META["digest_cases"], ids=lambda c: c["name"])
def test_level3_records_through_the_spec_reproduce_the_reference(case):
    rec, st3 = gc.run_geometry(case, 3)
    _, st0 = gc.run_geometry(case, 0)
    assert gc.same_state(st3, st0), "level 3 must consume `random` and `np.random` exactly as level 0"
    assert rec.dtype == np.int32 and rec.shape == (tr.GEOM_R,) and gs.GEOM_R == tr.GEOM_R
    assert np.array_equal(rec, gc.record_from_outcome(case["outcome"], case["S"])), (rec, case["outcome"])
    img, lab = gs.geometry(rec, *gc.case_source(case))
    if "sha256" in case:
        assert gc.digest(img) == case["sha256"]["image"] and gc.digest(lab) == case["sha256"]["label"]
    else:
        assert np.array_equal(img, ARRAYS[case["name"] + ".image"]) and np.array_equal(lab, ARRAYS[case["name"] + ".label"])


RESIZES = [(800, 800, int(0.5 * 800), int(1.4999 * 800)), (800, 800, int(1.4999 * 800), int(0.5 * 800)), (800, 800, 1100, 900),
           (800, 800, 800, 613), (640, 480, int(0.5 * 480), int(0.5 * 640)), (640, 480, int(1.4999 * 480), int(1.4999 * 640)),
           (640, 480, 333, 901), (513, 517, int(0.5 * 517), 700), (513, 517, int(1.4999 * 517), 257), (513, 517, 600, 513),
           (72, 80, 40, 107), (40, 40, 59, 20), (64, 64, 48, 48), (48, 48, 71, 24)]


@pytest.mark.parametrize("H0,W0,w,h", RESIZES)
def test_spec_resize_equals_the_installed_pillow(H0, W0, w, h):
    img, lab = gc.source(H0, W0, 610)
    assert np.array_equal(gs.resize_bilinear(img, w, h), np.array(Image.fromarray(img).resize((w, h), Image.BILINEAR)))
    assert np.array_equal(gs.resize_nearest(lab, w, h), np.array(Image.fromarray(lab).resize((w, h), Image.NEAREST)))


def test_quarter_turns_and_flips_of_the_spec_are_pils():
    img, lab = gc.source(48, 48, 604)
    for turns in range(4):
        for flr in (0, 1):
            for ftb in (0, 1):
                rec = np.array([0, 0, 0, 0, 0, 0, turns, flr, ftb, 48], np.int32)
                a = Image.fromarray(img).rotate(90 * turns if turns else 360, Image.BILINEAR)
                m = Image.fromarray(lab).rotate(90 * turns if turns else 360, Image.NEAREST, expand=255)
                if flr:
                    a, m = a.transpose(Image.FLIP_LEFT_RIGHT), m.transpose(Image.FLIP_LEFT_RIGHT)
                if ftb:
                    a, m = a.transpose(Image.FLIP_TOP_BOTTOM), m.transpose(Image.FLIP_TOP_BOTTOM)
                gi, gl = gs.geometry(rec, img, lab)
                assert np.array_equal(gi, np.array(a)) and np.array_equal(gl, np.array(m)), (turns, flr, ftb)


def test_level3_sample_holds_no_pixels_and_stays_under_64_kib():
    chain = gc.train_chain(512)
    val = gc.Compose([tr.RandomCrop(512), tr.Normalize_tf(), tr.ToTensor()])
    src = {"image": Image.new("RGB", (800, 800)), "label": Image.new("L", (800, 800)), "img_name": "s", "src_index": 7}
    seen = set()
    with gc.level(3):
        for seed in range(12):
            random.seed(seed); np.random.seed(seed)
            for c in (chain, val):
                s = c(dict(src))
                assert "image_u8" not in s and "label_u8" not in s and "image" not in s and "label" not in s
                assert int(s["src_index"][0]) == 7 and s["geom"].dtype == torch.int32 and tuple(s["geom"].shape) == (tr.GEOM_R,)
                nbytes = sum(v.numpy().nbytes for v in s.values() if isinstance(v, torch.Tensor))
                assert nbytes < 64 * 1024, nbytes
                assert int(s["geom"][tr.GEOM_SIZE]) == 512
                if c is chain:
                    seen.add(int(s["aug_sp_n"][0]) > 0)          # with and without the largest record, the noisy positions
    assert seen == {True, False}
    # other levels get no index from the dataset, level 3 does
    for lvl, has in ((0, False), (2, False), (3, True)):
        with gc.level(lvl):
            ds = DL.FundusSegmentation.__new__(DL.FundusSegmentation)
            ds.image_pool, ds.label_pool, ds.img_name_pool, ds.transform = [src["image"]], [src["label"]], ["s"], None
            assert ("src_index" in ds[0]) == has


def test_level3_chain_must_keep_the_scripts_order():
    src = {"image": Image.new("RGB", (64, 64)), "label": Image.new("L", (64, 64)), "img_name": "s", "src_index": 0}
    with gc.level(3):
        with pytest.raises(ValueError):
            tr.RandomFlip()(dict(src))
        with pytest.raises(ValueError):
            tr.RandomCrop(48)(tr.RandomFlip()(tr.RandomCrop(48)(dict(src))))
        with pytest.raises(ValueError):
            tr.Normalize_tf()(tr.RandomCrop(48)({k: v for k, v in src.items() if k != "src_index"}))


class _T(TrainerBase):
    def __init__(self):
        self.ops = gc.NumpyOps()

    def _to(self, t):
        return t

    def _device(self):
        return torch.device("cpu")


def test_full_level3_chain_on_the_numpy_statements_equals_the_level0_chain(tmp_path):
    """geometry -> (elastic not fired) -> photometric records -> Normalize_tf through TrainerBase._decode, for the training chain
    and the validation chain, with sources of one dataset; the pool is uploaded once per dataset and found through a loader."""
    from torch.utils.data import DataLoader
    write_dataset(str(tmp_path), "refuge", "train", 4, size=128, seed=4)
    random.seed(11)
    ds = DL.FundusSegmentation(base_dir=str(tmp_path), dataset="refuge", split="train", transform=gc.train_chain(96))
    pairs = gc.paired_samples(ds, 2)
    batch = gc.collate([g for g, _ in pairs])
    assert set(batch["geom"][:, tr.GEOM_SCALED].tolist()) == {0, 1} and batch["src_index"].shape == (8, 1)
    t = _T()
    loader = DataLoader(ds, batch_size=4)
    dec = t._decode(batch, loader)
    for k in ("image", "map", "boundary"):
        assert torch.equal(dec[k], torch.stack([w[k] for _, w in pairs])), k
    assert t.ops.calls == ["upload", "geometry", "elastic", "photometric", "normalize_tf"]
    t._decode(batch, ds)
    assert t.ops.calls.count("upload") == 1, "one upload per dataset object"
    # the validation chain: RandomCrop only
    ds.transform = gc.Compose([tr.RandomCrop(96), tr.Normalize_tf(), tr.ToTensor()])
    got, want = [], []
    for idx in range(4):
        for lvl, dst in ((3, got), (0, want)):
            random.seed(50 + idx)
            with gc.level(lvl):
                dst.append(ds[idx])
    dec = t._decode(gc.collate(got), ds)
    for k in ("image", "map", "boundary"):
        assert torch.equal(dec[k], torch.stack([w[k] for w in want])), k


def test_decode_without_a_dataset_raises():
    batch = {"src_index": torch.zeros(2, 1, dtype=torch.int64), "geom": torch.zeros(2, tr.GEOM_R, dtype=torch.int32)}
    with pytest.raises(ValueError, match="dataset"):
        _T()._decode(batch)
    with pytest.raises(ValueError, match="image_pool"):
        _T()._decode(batch, [batch])


def test_entry_point_is_declared_with_its_citation_and_bound():
    from uda_clr_amd import ops
    from uda_clr_amd.kernels import SYMBOLS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "include", "uda_clr_hip.h")).read()
    assert "uda_geometry_u8(" in txt and "custom_transforms.py:152-182,208-223,315-355" in txt
    assert "uda_geometry_u8" in SYMBOLS and "uda_geometry_u8_workspace_bytes" in SYMBOLS
    assert callable(ops.geometry_u8)
