"""-m gpu: the three entries of csrc/wholephoto.hip (uda_photo_reduce_u8, uda_roi_cut_u8, uda_roi_paste_u8) against the numpy
restatement of tests/wholephoto_ref.py, and ``predict --whole-photo`` end to end against the restated pipeline.

Every comparison is byte (bit) equality; there is no tolerance anywhere.  The shapes are the smallest at which the kernels can go
wrong: S = 16 (one 16-wide tile, one column chunk), photographs that are no multiple of anything, partial edge blocks, rows whose
first byte is at every alignment, windows over each side of the photograph."""
import csv
import os

import numpy as np
import pytest
import torch

import wholephoto_ref as wr
from kernel_cases import footprint, footprint_violations, out_dev, ro_dev
from uda_clr_amd import ops, predict

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
S = wr.S_TEST


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _norm_torch(u8_bhwc):
    """the expression of predict.predict, on the device"""
    return (u8_bhwc.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous()


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def _first_bad(got, want):
    bad = np.argwhere(got != want)
    return "%d of %d differ, first at %s: %s for %s" % (len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.fixture(scope="module")
def reduce_case():
    photos = wr.random_photos(11, wr.REDUCE_SHAPES)
    photos[3][:, :, 0] = 255                                   # the largest sums
    return photos, ops.PhotoPool(photos, DEV), wr.reduce_batch(photos, range(len(photos)), S)


@pytest.fixture(scope="module")
def cut_case():
    photos = wr.random_photos(12, wr.CUT_SHAPES)
    index = np.array([c[1] for c in wr.CUT_CASES], np.int64)
    boxes = np.array([c[2] for c in wr.CUT_CASES], np.int32)
    return photos, ops.PhotoPool(photos, DEV), index, boxes, wr.cut_batch(photos, index, boxes, S)


@pytest.fixture(scope="module")
def paste_case():
    """every window with every mask pair, in one batch"""
    masks, index, boxes = [], [], []
    for _, i, box in wr.PASTE_WINDOWS:
        for _, m in wr.mask_cases(13):
            masks.append(m)
            index.append(i)
            boxes.append(box)
    masks, boxes = np.stack(masks), np.array(boxes, np.int32)
    sizes = np.array([wr.PASTE_SHAPES[i] for i in index], np.int32)
    want = [wr.paste(m, b, int(hw[0]), int(hw[1])) for m, b, hw in zip(masks, boxes, sizes)]
    return masks, boxes, sizes, want


# ------------------------------------------------------------------------------------------------ reduce
def test_reduce_both_outputs_and_factor(reduce_case):
    photos, pool, (want, factor) = reduce_case
    assert factor.tolist() == [1, 1, 2, 4, 4, 9]
    got = ops.photo_reduce(pool, size=S, outputs=("u8", "f32"))
    u8 = got["u8"].cpu().numpy()
    assert u8.dtype == np.uint8 and u8.shape == want.shape and np.array_equal(u8, want), _first_bad(u8, want)
    assert got["factor"].dtype == torch.int32 and got["factor"].cpu().tolist() == factor.tolist()
    assert _same_bits(got["f32"], _norm_torch(got["u8"])), "the f32 canvas is not torch's u8.float() / 127.5 - 1 of the u8 canvas"
    assert np.array_equal(got["f32"].cpu().numpy().view(np.int32), wr.normalise(want).view(np.int32))
    for i in (0, 1):                                           # f = 1: the identity plus zero fill
        H, W = wr.REDUCE_SHAPES[i]
        assert np.array_equal(u8[i, :H, :W], photos[i]) and not u8[i, H:].any() and not u8[i, :, W:].any()
    for name in ("u8", "f32"):                                 # either output alone
        one = ops.photo_reduce(pool, size=S, outputs=(name,))
        assert set(one) == {name, "factor"} and torch.equal(one[name], got[name]) and torch.equal(one["factor"], got["factor"])


def test_reduce_index_outside_the_pool_gives_zeros_and_factor_0(reduce_case):
    photos, pool, (want, factor) = reduce_case
    index = torch.tensor([2, -1, len(photos), 3], dtype=torch.int64, device=DEV)       # on the device: not range-checked by the front-end
    got = ops.photo_reduce(pool, index=index, size=S, outputs=("u8", "f32"))
    u8 = got["u8"].cpu().numpy()
    assert got["factor"].cpu().tolist() == [2, 0, 0, 4]
    assert np.array_equal(u8[0], want[2]) and np.array_equal(u8[3], want[3]) and not u8[1:3].any()
    assert bool((got["f32"][1:3] == -1.0).all())
    with pytest.raises(ValueError, match="outside the pool"):
        ops.photo_reduce(pool, index=[0, len(photos)], size=S)


def test_reduce_alone_equals_inside_a_batch(reduce_case):
    photos, pool, _ = reduce_case
    index = [5, 0, 3, 3, 2]
    whole = ops.photo_reduce(pool, index=index, size=S, outputs=("u8", "f32"))
    again = ops.photo_reduce(pool, index=index, size=S, outputs=("u8", "f32"))
    for k in ("u8", "f32", "factor"):
        assert torch.equal(whole[k], again[k])
    for pos, i in enumerate(index):
        alone = ops.photo_reduce(pool, index=[i], size=S, outputs=("u8", "f32"))
        for k in ("u8", "f32", "factor"):
            assert torch.equal(alone[k][0], whole[k][pos]), (k, pos)


def test_reduce_larger_canvas_with_two_column_chunks():
    """S = 80: two column chunks (64 + 16), f = 3, rows whose bytes start at every alignment"""
    photos = wr.random_photos(14, [(200, 239), (80, 77)])
    want, factor = wr.reduce_batch(photos, [0, 1], 80)
    got = ops.photo_reduce(ops.PhotoPool(photos, DEV), size=80, outputs=("u8", "f32"))
    u8 = got["u8"].cpu().numpy()
    assert got["factor"].cpu().tolist() == factor.tolist() == [3, 1] and np.array_equal(u8, want), _first_bad(u8, want)
    assert _same_bits(got["f32"], _norm_torch(got["u8"]))


def _reduce_raw(K, pool, idx, B, s, u8, f32, factor):
    return K.lib.uda_photo_reduce_u8(pool.pool.data_ptr(), pool.pool.numel() // 3, pool.offsets.data_ptr(), pool.sizes.data_ptr(), len(pool),
                                     idx.data_ptr(), B, s, None if u8 is None else u8.data_ptr(), None if f32 is None else f32.data_ptr(),
                                     None if factor is None else factor.data_ptr(), _stream())


def test_reduce_write_footprint_and_inputs_unchanged(reduce_case):
    photos, _, (want, factor) = reduce_case
    K, B = ops.kernels(), len(photos)
    with footprint():
        pool = ops.PhotoPool(photos, "cpu")
        pool.pool, pool.offsets, pool.sizes = ro_dev(pool.pool, DEV, "pool"), ro_dev(pool.offsets, DEV, "offsets"), ro_dev(pool.sizes, DEV, "sizes")
        idx = ro_dev(torch.arange(B, dtype=torch.int64), DEV, "index")
        u8, f32, fac = out_dev((B, S, S, 3), torch.uint8, DEV, name="canvas_u8"), out_dev((B, 3, S, S), torch.float32, DEV, name="canvas_f32"), \
            out_dev((B,), torch.int32, DEV, name="factor")
        assert _reduce_raw(K, pool, idx, B, S, u8, f32, fac) == 0, K.lib.uda_last_error()
        torch.cuda.synchronize()
    assert footprint_violations() == [], "uda_photo_reduce_u8 wrote outside its outputs: (buffer, first position)"
    assert np.array_equal(u8.cpu().numpy(), want) and fac.cpu().tolist() == factor.tolist() and _same_bits(f32, _norm_torch(u8))


@pytest.mark.parametrize("case", ["null pool", "null factor", "no output", "S=24", "S=8", "B=0"])
def test_reduce_bad_arguments_return_an_error_and_write_nothing(reduce_case, case):
    photos, pool, _ = reduce_case
    K, B = ops.kernels(), len(photos)
    idx = torch.arange(B, dtype=torch.int64, device=DEV)
    u8, f32 = torch.full((B, 24, 24, 3), 0xA5, dtype=torch.uint8, device=DEV), torch.full((B, 3, 24, 24), -77.0, device=DEV)
    fac = torch.full((B,), -77, dtype=torch.int32, device=DEV)
    s = {"S=24": 24, "S=8": 8}.get(case, S)
    if case == "null pool":
        rc = K.lib.uda_photo_reduce_u8(None, pool.pool.numel() // 3, pool.offsets.data_ptr(), pool.sizes.data_ptr(), len(pool), idx.data_ptr(), B, s,
                                       u8.data_ptr(), f32.data_ptr(), fac.data_ptr(), _stream())
    elif case == "null factor":
        rc = _reduce_raw(K, pool, idx, B, s, u8, f32, None)
    elif case == "no output":
        rc = _reduce_raw(K, pool, idx, B, s, None, None, fac)
    else:
        rc = _reduce_raw(K, pool, idx, 0 if case == "B=0" else B, s, u8, f32, fac)
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_photo_reduce_u8" in K.lib.uda_last_error()
    assert bool((u8 == 0xA5).all()) and bool((f32 == -77.0).all()) and bool((fac == -77).all())


# ------------------------------------------------------------------------------------------------ cut
def test_cut_every_case_u8_and_f32(cut_case):
    photos, pool, index, boxes, want = cut_case
    got = ops.roi_cut(pool, torch.from_numpy(boxes), index=torch.from_numpy(index), size=S)
    u8 = got["u8"].cpu().numpy()
    for k, (name, _, _) in enumerate(wr.CUT_CASES):
        assert np.array_equal(u8[k], want[k]), "%s: %s" % (name, _first_bad(u8[k], want[k]))
    assert _same_bits(got["f32"], _norm_torch(got["u8"])), "the f32 ROI is not torch's u8.float() / 127.5 - 1 of the u8 ROI"
    names = [c[0] for c in wr.CUT_CASES]
    k = names.index("R=16 pure copy")
    assert np.array_equal(u8[k], photos[0][7:23, 5:21])
    for name in ("wholly outside", "wholly outside to the left"):
        assert not u8[names.index(name)].any()
    for name in ("u8", "f32"):                                 # a null output is accepted
        one = ops.roi_cut(pool, torch.from_numpy(boxes), index=torch.from_numpy(index), size=S, outputs=(name,))
        assert set(one) == {name} and torch.equal(one[name], got[name])


def test_cut_two_tiles_per_axis_at_the_bound():
    """S = 48: tiles of 32 and 16 per axis; R = 120 = 2.5 S, the widest patch a tile stages; R = 48 and R = 31 beside it"""
    photos = wr.random_photos(15, [(131, 157)])
    boxes = np.array([[20, 5, 120], [-30, 40, 120], [60, 50, 48], [100, 90, 31], [3, 2, 97]], np.int32)
    want = wr.cut_batch(photos, [0] * len(boxes), boxes, 48)
    got = ops.roi_cut(ops.PhotoPool(photos, DEV), torch.from_numpy(boxes), index=[0] * len(boxes), size=48)
    u8 = got["u8"].cpu().numpy()
    for k in range(len(boxes)):
        assert np.array_equal(u8[k], want[k]), "box %s: %s" % (boxes[k].tolist(), _first_bad(u8[k], want[k]))
    assert _same_bits(got["f32"], _norm_torch(got["u8"]))


def test_cut_alone_equals_inside_a_batch(cut_case):
    photos, pool, index, boxes, want = cut_case
    pick = [8, 1, 13, 4, 1]
    idx, bx = torch.from_numpy(index[pick]), torch.from_numpy(boxes[pick])
    whole, again = ops.roi_cut(pool, bx, index=idx, size=S), ops.roi_cut(pool, bx, index=idx, size=S)
    assert torch.equal(whole["u8"], again["u8"]) and torch.equal(whole["f32"], again["f32"])
    for pos, k in enumerate(pick):
        alone = ops.roi_cut(pool, bx[pos:pos + 1], index=idx[pos:pos + 1], size=S)
        assert torch.equal(alone["u8"][0], whole["u8"][pos]) and torch.equal(alone["f32"][0], whole["f32"][pos]), pos
        assert np.array_equal(alone["u8"][0].cpu().numpy(), want[k])


def _cut_raw(K, pool, idx, boxes, B, s, u8, f32):
    return K.lib.uda_roi_cut_u8(pool.pool.data_ptr(), pool.pool.numel() // 3, pool.offsets.data_ptr(), pool.sizes.data_ptr(), len(pool),
                                idx.data_ptr(), None if boxes is None else boxes.data_ptr(), B, s, None if u8 is None else u8.data_ptr(),
                                None if f32 is None else f32.data_ptr(), _stream())


def test_cut_write_footprint_and_inputs_unchanged(cut_case):
    photos, _, index, boxes, want = cut_case
    K, B = ops.kernels(), len(index)
    with footprint():
        pool = ops.PhotoPool(photos, "cpu")
        pool.pool, pool.offsets, pool.sizes = ro_dev(pool.pool, DEV, "pool"), ro_dev(pool.offsets, DEV, "offsets"), ro_dev(pool.sizes, DEV, "sizes")
        idx, bx = ro_dev(torch.from_numpy(index), DEV, "index"), ro_dev(torch.from_numpy(boxes), DEV, "boxes")
        u8, f32 = out_dev((B, S, S, 3), torch.uint8, DEV, name="roi_u8"), out_dev((B, 3, S, S), torch.float32, DEV, name="roi_f32")
        assert _cut_raw(K, pool, idx, bx, B, S, u8, f32) == 0, K.lib.uda_last_error()
        torch.cuda.synchronize()
    assert footprint_violations() == [], "uda_roi_cut_u8 wrote outside its outputs: (buffer, first position)"
    assert np.array_equal(u8.cpu().numpy(), want) and _same_bits(f32, _norm_torch(u8))


@pytest.mark.parametrize("case", ["null boxes", "no output", "S=24", "B=0", "R=7", "R=41"])
def test_cut_bad_arguments_return_an_error_and_write_nothing(cut_case, case):
    photos, pool, index, boxes, _ = cut_case
    K, B = ops.kernels(), 3
    idx, bx = torch.from_numpy(index[:B]).to(DEV), torch.from_numpy(boxes[:B]).to(DEV)
    u8, f32 = torch.full((B, 24, 24, 3), 0xA5, dtype=torch.uint8, device=DEV), torch.full((B, 3, 24, 24), -77.0, device=DEV)
    if case in ("R=7", "R=41"):                                # the boxes are data: the front-end refuses them on the host, before any launch;
        bad = boxes[:B].copy()                                 # on the device the kernel keeps such a box in bounds (an all-zero ROI)
        bad[1, 2] = int(case[2:])
        with pytest.raises(ValueError, match="8..2.5"):
            ops.roi_cut(pool, torch.from_numpy(bad), index=idx, size=S)
        got = ops.roi_cut(pool, torch.from_numpy(bad).to(DEV), index=idx, size=S, outputs=("u8",))["u8"].cpu().numpy()
        good = ops.roi_cut(pool, bx, index=idx, size=S, outputs=("u8",))["u8"].cpu().numpy()
        assert not got[1].any() and np.array_equal(got[0], good[0]) and np.array_equal(got[2], good[2])
        return
    if case == "null boxes":
        rc = _cut_raw(K, pool, idx, None, B, S, u8, f32)
    elif case == "no output":
        rc = _cut_raw(K, pool, idx, bx, B, S, None, None)
    else:
        rc = _cut_raw(K, pool, idx, bx, 0 if case == "B=0" else B, 24 if case == "S=24" else S, u8, f32)
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_roi_cut_u8" in K.lib.uda_last_error()
    assert bool((u8 == 0xA5).all()) and bool((f32 == -77.0).all())


# ------------------------------------------------------------------------------------------------ paste
def test_paste_every_window_with_every_mask(paste_case):
    masks, boxes, sizes, want = paste_case
    m = torch.from_numpy(masks).to(DEV)
    keep = m.clone()
    got = ops.roi_paste(sizes, m, torch.from_numpy(boxes))
    assert torch.equal(m, keep)
    k = 0
    for wname, _, _ in wr.PASTE_WINDOWS:
        for mname, _ in wr.mask_cases(13):
            g = got[k].cpu().numpy()
            assert g.dtype == np.uint8 and g.shape == want[k].shape and np.array_equal(g, want[k]), "%s, %s: %s" % (wname, mname, _first_bad(g, want[k]))
            if wname.startswith("wholly outside") or mname == "all zeros":
                assert (g == 255).all()
            k += 1
    assert set(np.unique(np.concatenate([w.reshape(-1) for w in want])).tolist()) == {0, 128, 255}


def test_paste_takes_a_pool_bool_and_float_masks(paste_case):
    masks, boxes, sizes, want = paste_case
    photos = [np.zeros((H, W, 3), np.uint8) for H, W in wr.PASTE_SHAPES]
    pool = ops.PhotoPool(photos, DEV)
    pick = [0, 16, 27, 31, 40]
    index = [0 if tuple(sizes[k]) == wr.PASTE_SHAPES[0] else 1 for k in pick]
    for m in (torch.from_numpy(masks[pick] != 0), torch.from_numpy((masks[pick] != 0).astype(np.float32) * 0.9).to(DEV)):
        got = ops.roi_paste(pool, m, torch.from_numpy(boxes[pick]), index=index)
        for pos, k in enumerate(pick):
            assert np.array_equal(got[pos].cpu().numpy(), want[k]), pos


def test_paste_alone_equals_inside_a_batch(paste_case):
    masks, boxes, sizes, want = paste_case
    pick = [22, 3, 41, 15, 3]
    m, bx = torch.from_numpy(masks[pick]).to(DEV), torch.from_numpy(boxes[pick])
    whole, again = ops.roi_paste(sizes[pick], m, bx), ops.roi_paste(sizes[pick], m, bx)
    for pos, k in enumerate(pick):
        alone = ops.roi_paste(sizes[pick][pos:pos + 1], m[pos:pos + 1], bx[pos:pos + 1])
        assert torch.equal(alone[0], whole[pos]) and torch.equal(again[pos], whole[pos]), pos
        assert np.array_equal(whole[pos].cpu().numpy(), want[k])


def _paste_raw(K, m, bx, sz, off, B, s, out):
    return K.lib.uda_roi_paste_u8(None if m is None else m.data_ptr(), bx.data_ptr(), sz.data_ptr(), off.data_ptr(), B, s,
                                  None if out is None else out.data_ptr(), 0 if out is None else out.numel(), _stream())


def _paste_operands(masks, boxes, sizes, put):
    px = sizes[:, 0].astype(np.int64) * sizes[:, 1]
    starts = np.concatenate([[0], np.cumsum(px)]).astype(np.int64)
    return (put(torch.from_numpy(masks), "masks"), put(torch.from_numpy(boxes), "boxes"), put(torch.from_numpy(sizes), "sizes"),
            put(torch.from_numpy(starts[:-1].copy()), "out_offsets"), starts)


def test_paste_write_footprint_and_inputs_unchanged(paste_case):
    masks, boxes, sizes, want = paste_case
    K, B = ops.kernels(), len(want)
    with footprint():
        m, bx, sz, off, starts = _paste_operands(masks, boxes, sizes, lambda t, name: ro_dev(t, DEV, name))
        out = out_dev((int(starts[-1]),), torch.uint8, DEV, name="out")
        assert _paste_raw(K, m, bx, sz, off, B, S, out) == 0, K.lib.uda_last_error()
        torch.cuda.synchronize()
    assert footprint_violations() == [], "uda_roi_paste_u8 wrote outside its output: (buffer, first position)"
    assert np.array_equal(out.cpu().numpy(), np.concatenate([w.reshape(-1) for w in want]))


@pytest.mark.parametrize("case", ["null masks", "null out", "S=24", "B=0", "R=7", "R=41"])
def test_paste_bad_arguments_return_an_error_and_write_nothing(paste_case, case):
    masks, boxes, sizes, want = paste_case
    K, B = ops.kernels(), 4
    if case in ("R=7", "R=41"):                                # as for the cut: refused on the host; on the device an all-255 mask
        bad = boxes[:B].copy()
        bad[2, 2] = int(case[2:])
        with pytest.raises(ValueError, match="8..2.5"):
            ops.roi_paste(sizes[:B], torch.from_numpy(masks[:B]), torch.from_numpy(bad))
        got = ops.roi_paste(sizes[:B], torch.from_numpy(masks[:B]).to(DEV), torch.from_numpy(bad).to(DEV))
        assert bool((got[2] == 255).all()) and all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in (0, 1, 3))
        return
    m, bx, sz, off, starts = _paste_operands(masks[:B], boxes[:B], sizes[:B], lambda t, name: t.to(DEV))
    out = torch.full((int(starts[-1]),), 0xA5, dtype=torch.uint8, device=DEV)
    if case == "null masks":
        rc = _paste_raw(K, None, bx, sz, off, B, S, out)
    elif case == "null out":
        rc = _paste_raw(K, m, bx, sz, off, B, S, None)
    else:
        rc = _paste_raw(K, m, bx, sz, off, 0 if case == "B=0" else B, 24 if case == "S=24" else S, out)
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_roi_paste_u8" in K.lib.uda_last_error()
    assert bool((out == 0xA5).all())


# ------------------------------------------------------------------------------------------------ predict --whole-photo end to end
class _Counting:
    """the stand-in generator of tests/wholephoto_ref.py, counting its calls"""
    def __init__(self):
        self.calls = 0

    def __call__(self, image):
        self.calls += 1
        return wr.brightness_stub(image)


@pytest.fixture(scope="module")
def drawn(tmp_path_factory):
    """three drawn photographs and a black one as PNG files, and the restated pipeline of each"""
    from PIL import Image
    folder = tmp_path_factory.mktemp("photos")
    photos = [wr.draw_photo(*d) for d in wr.DRAWN] + [np.zeros((50, 90, 3), np.uint8)]
    names = ["a%d.png" % i for i in range(len(photos))]
    for n, p in zip(names, photos):
        Image.fromarray(p).save(str(folder / n))
    return str(folder), names, photos, [wr.restated_pipeline(p) for p in photos]


def _png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im)


def test_whole_photo_end_to_end_equals_the_restated_pipeline(drawn, tmp_path):
    folder, names, photos, want = drawn
    stub = _Counting()
    out = tmp_path / "out"
    rows = predict.main(["--images", folder, "--out", str(out), "--whole-photo", "--roi-size", str(wr.E2E_ROI), "--batch-size", "3",
                         "--csv", str(tmp_path / "rows.csv"), "--morphometry"], model=stub, size=wr.E2E_SIZE)
    assert stub.calls == 4 and [r["img_name"] for r in rows] == names             # two batches, two stages each
    for i, (row, w, photo) in enumerate(zip(rows, want, photos)):
        stem = names[i].split(".")[0]
        assert (row["roi_x0"], row["roi_y0"], row["roi_size"]) == tuple(int(v) for v in w["box"]) and row["located"] == w["located"], i
        g = _png(str(out / "photo_mask" / (stem + ".png")))
        assert g.shape == photo.shape[:2] and g.dtype == np.uint8 and np.array_equal(g, w["photo_mask"]), i
        roi_mask = _png(str(out / "mask" / (stem + ".png")))
        assert np.array_equal(roi_mask, np.where(w["masks"][0] != 0, 0, np.where(w["masks"][1] != 0, 128, 255)))
        assert np.array_equal(_png(str(out / "original_image" / (stem + ".png"))), wr.cut(photo, w["box"], wr.E2E_SIZE))
        assert os.path.exists(str(out / "overlay" / (stem + ".png")))
        for k in ("disc_cx", "disc_cy"):
            assert row[k] == w[k] or (np.isnan(row[k]) and np.isnan(w[k])), (i, k)
    for row, (shape, centre, radius) in zip(rows[:3], wr.DRAWN):
        f = wr.factor_of(shape[0], shape[1], wr.E2E_SIZE)
        x0, y0, R = row["roi_x0"], row["roi_y0"], row["roi_size"]
        assert row["located"] == 1
        assert x0 <= centre[1] - radius and centre[1] + radius < x0 + R and y0 <= centre[0] - radius and centre[0] + radius < y0 + R      # the whole disc
        assert abs(row["disc_cx"] - (centre[1] + 0.5)) <= f and abs(row["disc_cy"] - (centre[0] + 0.5)) <= f
        assert row["disc_major"] > 0 and 0 < row["vcdr_pred"] < 1
    black = rows[3]                                                                # 50 x 90: centred window, shifted into the 90 columns
    assert black["located"] == 0 and (black["roi_x0"], black["roi_y0"]) == (45 - 24, 25 - 24) and np.isnan(black["disc_cx"])
    assert (_png(str(out / "photo_mask" / "a3.png")) == 255).all()
    head = list(csv.reader(open(str(tmp_path / "rows.csv"))))[0]
    assert head == ["img_name", "vcdr_pred"] + list(predict.MORPHOMETRY_COLUMNS) + list(predict.WHOLE_PHOTO_COLUMNS)


def test_whole_photo_pixel_columns_are_in_photograph_pixels(drawn, tmp_path):
    """the ROI-scale figures of predict on the very ROI files the whole-photo run wrote, times R / size"""
    folder, names, photos, want = drawn
    whole = predict.main(["--images", folder, "--out", str(tmp_path / "w"), "--whole-photo", "--roi-size", str(wr.E2E_ROI), "--morphometry"],
                         model=wr.brightness_stub, size=wr.E2E_SIZE)
    plain = predict.main(["--images", str(tmp_path / "w" / "original_image"), "--out", str(tmp_path / "p"), "--morphometry"], model=wr.brightness_stub)
    for w, p in zip(whole[:3], plain[:3]):
        for k in predict.MORPHOMETRY_COLUMNS:
            scaled = k in ("cup_offset_pred", "cup_major", "cup_minor", "disc_major", "disc_minor")
            assert w[k] == (p[k] * wr.E2E_ROI / wr.E2E_SIZE if scaled else p[k]) or (np.isnan(w[k]) and np.isnan(p[k])), k
        assert w["vcdr_pred"] == p["vcdr_pred"]


def test_centres_reproduce_the_boxes_without_the_locator(drawn, tmp_path):
    folder, names, photos, want = drawn
    with open(str(tmp_path / "c.csv"), "w") as f:
        f.write("img_name,cx,cy\n" + "".join("%s,%d,%d\n" % (n, w["centre"][1], w["centre"][0]) for n, w in zip(names, want)))
    stub = _Counting()

    def never(image):
        raise AssertionError("the locator was called")
    rows = predict.main(["--images", folder, "--out", str(tmp_path / "out"), "--whole-photo", "--roi-size", str(wr.E2E_ROI), "--centres",
                         str(tmp_path / "c.csv")], model=stub, locator=never, size=wr.E2E_SIZE)
    assert stub.calls == 1                                                         # one batch, the ROI stage only
    for i, (row, w) in enumerate(zip(rows, want)):
        assert (row["roi_x0"], row["roi_y0"], row["roi_size"]) == tuple(int(v) for v in w["box"]) and row["located"] == 1, i
        if i < 3:
            assert np.array_equal(_png(str(tmp_path / "out" / "photo_mask" / ("a%d.png" % i))), w["photo_mask"])


def test_odd_sizes_are_refused_without_whole_photo(drawn, tmp_path):
    folder = drawn[0]
    with pytest.raises(ValueError, match="a2.png|a3.png"):
        predict.main(["--images", folder, "--out", str(tmp_path / "out")], model=wr.brightness_stub)


def test_real_generator_goes_through_both_stages(drawn, tmp_path):
    """a seeded-init DeepLab at size 64: every file is written and every row is complete (no accuracy claim)"""
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    folder, names, photos, _ = drawn
    torch.manual_seed(3)
    model = DeepLab(num_classes=2, backbone="mobilenet", output_stride=16).to(DEV)
    rows = predict.main(["--images", folder, "--out", str(tmp_path / "out"), "--whole-photo", "--roi-size", "96", "--batch-size", "4"], model=model, size=64)
    assert [r["img_name"] for r in rows] == names and model.training       # the mode it came in is restored
    for n, photo, row in zip(names, photos, rows):
        stem = n.split(".")[0]
        assert set(predict.WHOLE_PHOTO_COLUMNS) <= set(row) and row["roi_size"] == 96 and row["located"] in (0, 1)
        assert _png(str(tmp_path / "out" / "photo_mask" / (stem + ".png"))).shape == photo.shape[:2]
        assert _png(str(tmp_path / "out" / "mask" / (stem + ".png"))).shape == (64, 64)
        assert _png(str(tmp_path / "out" / "original_image" / (stem + ".png"))).shape == (64, 64, 3)
        assert os.path.exists(str(tmp_path / "out" / "overlay" / (stem + ".png")))
        assert set(np.unique(_png(str(tmp_path / "out" / "photo_mask" / (stem + ".png")))).tolist()) <= {0, 128, 255}
