"""-m gpu: uda_geometry_u8 (csrc/geometry.hip), the device-side scale-crop / rotate / flip of UDA_CLR_DEVICE_INPUT=3.

Against the fixture recorded from the reference (tests/golden/geometry.*), against its numpy statement (tests/geometry_spec.py)
and inside the Trainer.  Every comparison is byte equality: the arithmetic is integer."""
import random

import numpy as np
import pytest
import torch

import geometry_cases as gc
import geometry_spec as gs
import model_cases
from uda_clr_amd import ops
from uda_clr_amd.dataloaders import custom_transforms as tr
from uda_clr_amd.dataloaders import fundus_dataloader as DL
from uda_clr_amd.dataloaders.synthetic import write_dataset
from uda_clr_amd.train_process import Trainer_baseline
from uda_clr_amd.train_process._common import HipOps, TrainerBase

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
META, ARRAYS = gc.fixture()
CASES = META["cases"]


def _run(cases_or_sources, records, index):
    """the kernel on a batch: sources [(image, mask)], records int32 [B, R], index [B] into the sources"""
    pool = ops.SourcePool([s[0] for s in cases_or_sources], [s[1] for s in cases_or_sources], DEV)
    iu, lu = ops.geometry_u8(pool, torch.from_numpy(np.asarray(index, np.int64)), torch.from_numpy(np.stack(records)))
    torch.cuda.synchronize()
    return iu.cpu().numpy(), lu.cpu().numpy()


def _batches():
    """ragged batches over all fixture cases: B = 1, then one mixing scaled, unscaled and padded samples, then the rest"""
    first = [c for c in CASES if c["outcome"]["scaled"]][:1]
    rest = [c for c in CASES if c is not first[0]]
    mixed = ([c for c in rest if c["outcome"]["scaled"] and not c["outcome"]["pad"]][:2] + [c for c in rest if not c["outcome"]["scaled"]][:2]
             + [c for c in rest if c["outcome"]["pad"]][:3])
    mixed = [c for i, c in enumerate(mixed) if c not in mixed[:i]]
    assert any(c["outcome"]["scaled"] for c in mixed) and any(not c["outcome"]["scaled"] for c in mixed) and any(c["outcome"]["pad"] for c in mixed)
    tail = [c for c in rest if c not in mixed]
    out = [first, mixed] + ([tail] if tail else [])
    assert sorted(c["name"] for b in out for c in b) == sorted(c["name"] for c in CASES)
    return out


@pytest.mark.parametrize("batch", _batches(), ids=lambda b: "B%d" % len(b))
def test_kernel_reproduces_every_fixture_case(batch):
    shapes = sorted({(c["H0"], c["W0"], c["src_seed"]) for c in CASES})            # one pool of all sources: sizes differ inside a batch
    sources = [gc.source(*s) for s in shapes]
    index = [shapes.index((c["H0"], c["W0"], c["src_seed"])) for c in batch]
    records = [gc.record_from_outcome(c["outcome"], c["S"]) for c in batch]
    iu, lu = _run(sources, records, index)
    for b, c in enumerate(batch):
        assert np.array_equal(iu[b], ARRAYS[c["name"] + ".image"]), c["name"]
        assert np.array_equal(lu[b], ARRAYS[c["name"] + ".label"]), c["name"]


def test_kernel_reproduces_the_two_512_cases_from_800x800():
    cases = META["digest_cases"]
    iu, lu = _run([gc.case_source(cases[0])], [gc.record_from_outcome(c["outcome"], c["S"]) for c in cases], [0, 0])
    for b, c in enumerate(cases):
        assert iu[b].shape == (512, 512, 3)
        assert gc.digest(iu[b]) == c["sha256"]["image"] and gc.digest(lu[b]) == c["sha256"]["label"], c["name"]


def _further_records():
    """16 seeded records at S = 48 over four source shapes, the first four chosen: the crop window is the whole scaled image
    (touches all four borders; xmin clamps at 0 and xmax at `in` under the 64 -> 48 and 80 -> 48 downscale), a scaled size of
    exactly S on one axis, an axis left unscaled while the other scales, and the widest downscale."""
    S, rs = 48, np.random.RandomState(77)
    shapes = [(72, 80, 601), (64, 64, 602), (40, 40, 603), (48, 48, 604)]
    chosen = [(1, (48, 48)), (0, (48, 70)), (1, (64, 90)), (0, (40, 36))]
    recs, index = [], []
    for i in range(16):
        si, wh = chosen[i] if i < len(chosen) else (int(rs.randint(4)), None)
        H0, W0, _ = shapes[si]
        recs.append(gc.make_record(rs, H0, W0, S, scaled=True if wh else None, wh=wh))
        index.append(si)
    assert tuple(recs[0][[1, 2, 3, 4, 5]]) == (48, 48, 0, 0, 0)
    return shapes, recs, index


def test_kernel_equals_the_numpy_statement_on_further_records():
    shapes, recs, index = _further_records()
    sources = [gc.source(*s) for s in shapes]
    want_i, want_l = gs.geometry_batch(np.stack(recs), index, [s[0] for s in sources], [s[1] for s in sources])
    iu, lu = _run(sources, recs, index)
    for b in range(len(recs)):
        assert np.array_equal(iu[b], want_i[b]) and np.array_equal(lu[b], want_l[b]), (b, recs[b])


class _T(TrainerBase):
    def __init__(self):
        self.ops = HipOps()

    def _to(self, t):
        return t.to(DEV)

    def _device(self):
        return DEV


def test_level3_decode_on_the_device_equals_the_cpu_chain(tmp_path):
    """UDA_CLR_DEVICE_INPUT=3 through TrainerBase._decode on the HIP kernels: from the recorded draws (elastic not fired) the
    decoded batch equals the level-0 chain's tensors exactly, for the same seeds."""
    write_dataset(str(tmp_path), "refuge", "train", 4, size=128, seed=4)
    random.seed(11)
    ds = DL.FundusSegmentation(base_dir=str(tmp_path), dataset="refuge", split="train", transform=gc.train_chain(96))
    pairs = gc.paired_samples(ds, 2)
    batch = gc.collate([g for g, _ in pairs])
    assert set(batch["geom"][:, tr.GEOM_SCALED].tolist()) == {0, 1}
    dec = _T()._decode(batch, ds)
    for k in ("image", "map", "boundary"):
        assert torch.equal(dec[k].cpu(), torch.stack([w[k] for _, w in pairs])), k


class _Batches(list):
    """a sequence of ready-made batches that names its dataset, like a DataLoader"""
    dataset = None


def _rows(path):
    with open(path) as f:
        return [l.split(",") for l in f.read().strip().split("\n")[1:]]


def test_trainer_epoch_over_a_level3_loader_equals_the_epoch_at_level0(tmp_path):
    write_dataset(str(tmp_path / "data"), "refuge", "train", 4, size=128, seed=5)
    random.seed(12)
    ds = DL.FundusSegmentation(base_dir=str(tmp_path / "data"), dataset="refuge", split="train", transform=gc.train_chain(64))
    pairs = gc.paired_samples(ds, 2)
    l3, l0 = _Batches(), _Batches()
    for i in (0, 4):
        l3.append(gc.collate([g for g, _ in pairs[i:i + 4]]))
        l0.append(gc.collate([w for _, w in pairs[i:i + 4]]))
    l3.dataset = ds
    rows = []
    for tag, loader in (("l3", l3), ("l0", l0)):
        m = model_cases.seeded_model().to(DEV)
        m._engine_for(torch.empty(1, device=DEV)).seed = 1337            # same dropout streams in both runs
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.99))
        t = Trainer_baseline.Trainer(cuda=True, model_gen=m, optimizer_gen=opt, lr_gen=1e-3, lr_decrease_rate=0.1,
                                     val_loader=loader, domain_loaderS=loader, domain_loaderT=loader, out=str(tmp_path / tag),
                                     max_epoch=1, stop_epoch=1, interval_validate=1, batch_size=4, warmup_epoch=-1)
        t.epoch = 0
        t.iteration = 0
        t.train()
        t.validate()
        rows.append(_rows(tmp_path / tag / "log.csv"))
    a, b = rows
    assert len(a) == len(b) >= 3
    for ra, rb in zip(a, b):
        assert ra[2:8] == rb[2:8], (ra, rb)          # loss columns and the validation tuple, digit for digit
