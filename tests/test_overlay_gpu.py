"""-m gpu: the prediction pictures on the device (uda_display_masks, uda_overlay_u8, uda_image_u8 and what sits on them) against the
numpy / scipy statement of tests/overlay_ref.py.  Byte equality throughout: there is no tolerance in this file."""
import csv
import os

import numpy as np
import pytest
import torch

import overlay_ref as ovr
import postproc_shapes as shapes
import surface_ref as sr
from uda_clr_amd import evaluate as ev
from uda_clr_amd import ops, predict
from uda_clr_amd.utils import Utils

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
LIBRARY = ovr.library()                          # postproc_shapes.library() and overlay_ref.tip_bay()
_ORACLE = {}


def _oracle(name):
    """display masks of a library shape by scipy, computed once and handed out read-only"""
    if name not in _ORACLE:
        m = ovr.display_masks(dict(LIBRARY)[name])
        m.setflags(write=False)
        _ORACLE[name] = m
    return _ORACLE[name]


def _dev(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)          # a copy: the shared oracles are read-only


# ------------------------------------------------------------------------------------------------------------- display masks
@pytest.mark.parametrize("name", [n for n, _ in LIBRARY])
def test_display_masks_equal_the_oracle(name):
    prob = dict(LIBRARY)[name]
    p = _dev(prob[None])
    got = ops.display_masks(p)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + prob.shape
    assert np.array_equal(got[0].cpu().numpy(), _oracle(name))
    assert np.array_equal(p[0].cpu().numpy(), prob)                      # the border ring is applied where the threshold reads


@pytest.mark.parametrize("where", ["top", "bottom", "left", "right", "corner"])
def test_display_masks_of_blobs_against_the_borders(where):
    for name in ("tie later_larger", "nested blob_in_ring", "blob 33x17", "tip bay"):
        prob = ovr.shifted(dict(LIBRARY)[name], where)
        assert (prob[:, 0] > 0.5).any() or (prob[:, -1] > 0.5).any() or (prob[:, :, 0] > 0.5).any() or (prob[:, :, -1] > 0.5).any()
        got = ops.display_masks(_dev(prob[None]))[0].cpu().numpy()
        assert np.array_equal(got, ovr.display_masks(prob)), name


def test_an_image_s_display_masks_do_not_depend_on_its_neighbours():
    names = ["tie equal", "tie third_first", "tie later_larger", "nested blob_in_ring", "nested open_ring"]          # all 128 x 128
    for order in ([0, 1, 2, 3, 4], [3, 0, 4, 2, 1, 3]):
        batch = np.stack([dict(LIBRARY)[names[i]] for i in order])
        got = ops.display_masks(_dev(batch)).cpu().numpy()
        for k, i in enumerate(order):
            assert np.array_equal(got[k], _oracle(names[i])), (order, k)


def test_threshold_argument_and_the_fixed_default():
    prob = np.where(shapes.tie("equal") > 0.5, np.float32(0.6), shapes.OUT).astype(np.float32)       # between 0.5 and 0.75
    assert not ops.display_masks(_dev(prob[None])).any()
    got = ops.display_masks(_dev(prob[None]), threshold=0.5)[0].cpu().numpy()
    assert got.any() and np.array_equal(got, ovr.display_masks(prob, 0.5))


@pytest.fixture
def attempts(monkeypatch):
    """the `sweeps` argument of every uda_display_masks call HipKernels.display_masks makes"""
    lib = ops.kernels().lib
    real, seen = lib.uda_display_masks, []

    def spy(*args):
        seen.append(args[5])
        return real(*args)
    monkeypatch.setattr(lib, "uda_display_masks", spy)
    return seen


def test_one_sweep_on_the_spiral_is_reported_and_retried(attempts):
    """By tests/postproc_shapes.py's model of the tile-wise propagation the 256 spiral needs 50 launches for the components, 35 for the
    first flood and 36 for the flood of the dilated mask (the 192 spiral 29, 17 and 16).  So the entry with sweeps = 1 reports all
    three unfinished; the binding at its default of 36 finds the components unfinished, retries with 72 and returns the oracle's
    mask; from sweeps = 1 its six attempts end at 32 launches: enough for the 192 spiral, and on the 256 one it gives up without a
    mask, exactly as HipKernels.postprocess does (tests/test_postproc_gpu.py)."""
    from uda_clr_amd.kernels import UdaError
    name = "spiral 256/20/18"
    K = ops.kernels()
    p = _dev(dict(LIBRARY)[name][None])
    B, _, H, W = p.shape
    out = torch.empty(B, 2, H, W, dtype=torch.uint8, device=DEV)
    flags = torch.full((3,), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(K.lib.uda_display_masks_workspace_bytes(B, H, W), dtype=torch.uint8, device=DEV)
    rc = K.lib.uda_display_masks(p.data_ptr(), B, H, W, 0.75, 1, out.data_ptr(), flags.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    f = flags.cpu().numpy()
    print("not_converged after one sweep:", f.tolist())
    assert (f > 0).all()
    del attempts[:]
    got = K.display_masks(p)                                               # default sweeps: 36 < 50
    assert attempts == [shapes.default_sweeps(256, 256), 2 * shapes.default_sweeps(256, 256)]
    assert np.array_equal(got[0].cpu().numpy(), _oracle(name))
    small = "spiral 192/20/18"
    del attempts[:]
    got = K.display_masks(_dev(dict(LIBRARY)[small][None]), sweeps=1)
    assert attempts == [1, 2, 4, 8, 16, 32] and np.array_equal(got[0].cpu().numpy(), _oracle(small))
    del attempts[:]
    with pytest.raises(UdaError, match="uda_display_masks: label propagation did not converge after 32 sweeps"):
        K.display_masks(p, sweeps=1)
    assert attempts == [1, 2, 4, 8, 16, 32]


@pytest.mark.parametrize("case", ["H=0", "null prob", "short workspace", "sweeps=0"])
def test_display_masks_bad_arguments_write_nothing(case):
    K = ops.kernels()
    B, H, W = 1, 40, 24
    p = torch.rand(B, 2, H, W, device=DEV)
    out = torch.full((B, 2, H, W), 0x5A, dtype=torch.uint8, device=DEV)
    flags = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    need = K.lib.uda_display_masks_workspace_bytes(B, H, W)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device=DEV)
    h, ptr, nbytes, sweeps = {"H=0": (0, p.data_ptr(), need, 4), "null prob": (H, None, need, 4), "short workspace": (H, p.data_ptr(), need - 1, 4),
                              "sweeps=0": (H, p.data_ptr(), need, 0)}[case]
    rc = K.lib.uda_display_masks(ptr, B, h, W, 0.75, sweeps, out.data_ptr(), flags.data_ptr(), ws.data_ptr(), nbytes,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc != 0 and b"uda_display_masks" in K.lib.uda_last_error()
    assert bool((out == 0x5A).all()) and bool((flags == -7).all()) and bool((ws == 0xA5).all())


# ------------------------------------------------------------------------------------------------------------------- overlay
def _check_overlay(masks, seed=0):
    """masks uint8 [B,2,H,W] on the host: the device picture over random image bytes equals the statement's"""
    B, _, H, W = masks.shape
    image = ovr.random_image(B, H, W, seed)
    got = ops.overlay(_dev(image), _dev(masks))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W, 3)
    want = ovr.overlay_batch(image, masks)
    g = got.cpu().numpy()
    assert np.array_equal(g, want), "first differing (b, row, column, channel): %s" % (np.argwhere(g != want)[:4].tolist(),)
    return g


@pytest.mark.parametrize("name", [n for n, _ in LIBRARY])
def test_overlay_of_the_display_masks(name):
    _check_overlay(_oracle(name)[None], seed=len(name))


@pytest.mark.parametrize("name,masks", ovr.hand_masks(), ids=[n for n, _ in ovr.hand_masks()])
def test_overlay_of_hand_made_masks(name, masks):
    g = _check_overlay(masks[None], seed=1)
    if name == "overlapping outlines":
        assert g[0, 10, 15].tolist() == list(ovr.BLUE) and g[0, 29, 15].tolist() == list(ovr.GREEN)     # shared top edge: blue wins
    if name == "checkerboard":
        assert (g[0] == np.array(ovr.BLUE, np.uint8)).all()                                              # every pair differs
    if name == "full planes":
        assert np.array_equal(g[0], ovr.random_image(1, 12, 7, 1)[0])                                    # no pair differs: a plain copy


def test_overlay_is_the_same_alone_and_inside_a_batch_and_from_run_to_run():
    group = [m for n, m in ovr.hand_masks() if n.startswith("corner pixel") or n == "single pixel"]      # all 9 x 11
    batch = np.stack(group)
    image = ovr.random_image(len(group), 9, 11, 4)
    whole = ops.overlay(_dev(image), _dev(batch))
    assert torch.equal(whole, ops.overlay(_dev(image), _dev(batch)))
    for i in (0, 2, 4):
        assert torch.equal(whole[i], ops.overlay(_dev(image[i:i + 1]), _dev(batch[i:i + 1]))[0])
    rev = ops.overlay(_dev(image[::-1]), _dev(batch[::-1]))
    assert torch.equal(whole, rev.flip(0))


def test_overlay_takes_float_images_and_probabilities():
    name = "nested blob_in_ring"
    prob = dict(LIBRARY)[name]
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(2)) * 2 - 1
    got = ops.overlay(x.to(DEV), _dev(prob[None]))
    want = ovr.overlay(ovr.image_u8(x.numpy())[0], _oracle(name))
    assert np.array_equal(got[0].cpu().numpy(), want)
    assert torch.equal(got, ops.overlay(x, torch.from_numpy(_oracle(name).copy())[None].bool()))         # CPU tensors, bool masks


def test_overlay_refuses_aliasing_and_bad_shapes():
    K = ops.kernels()
    image = _dev(ovr.random_image(1, 16, 16, 0))
    masks = torch.zeros(1, 2, 16, 16, dtype=torch.uint8, device=DEV)
    keep = image.clone()
    with pytest.raises(Exception, match="alias"):
        K.overlay_u8(image, masks, out=image)
    assert torch.equal(image, keep)
    with pytest.raises(ValueError):
        K.overlay_u8(image, masks[:, :, :8].contiguous())
    with pytest.raises(ValueError):
        ops.overlay(image.int(), masks)


# ------------------------------------------------------------------------------------------------------------------ footprint
def test_every_entry_writes_its_output_window_only():
    """out inside a larger sentinel-filled buffer, masks that touch all four borders (so outline targets fall outside the image on
    every side): every byte outside the window keeps its sentinel, every operand is unchanged"""
    K = ops.kernels()
    B, H, W = 2, 33, 45
    guard = 4096
    masks = np.zeros((B, 2, H, W), np.uint8)
    masks[0, 0], masks[0, 1] = 1, (np.indices((H, W)).sum(0) % 2)
    masks[1, 0, :, ::2] = 1
    masks[1, 1, ::4, :] = 1
    for c in range(2):
        for b in range(B):
            m = masks[b, c]
            assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    image = ovr.random_image(B, H, W, 9)
    d_image, d_masks = _dev(image), _dev(masks)
    n = B * H * W * 3
    buf = torch.full((guard + n + guard,), 0xC3, dtype=torch.uint8, device=DEV)
    out = buf[guard:guard + n].view(B, H, W, 3)
    K.overlay_u8(d_image, d_masks, out=out)
    assert bool((buf[:guard] == 0xC3).all()) and bool((buf[guard + n:] == 0xC3).all())
    assert np.array_equal(out.cpu().numpy(), ovr.overlay_batch(image, masks))
    assert np.array_equal(d_image.cpu().numpy(), image) and np.array_equal(d_masks.cpu().numpy(), masks)

    x = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(3)) * 2.4 - 1.2
    d_x = x.to(DEV)
    buf.fill_(0xC3)
    K.image_u8(d_x, out=out)
    assert bool((buf[:guard] == 0xC3).all()) and bool((buf[guard + n:] == 0xC3).all())
    assert np.array_equal(out.cpu().numpy(), ovr.image_u8(x.numpy())) and torch.equal(d_x.cpu(), x)

    prob = np.stack([shapes.ones(H, W), shapes.blob_33x17().repeat(3, 2)[:, :H, :W]])                      # set pixels on all borders
    d_prob = _dev(prob)
    m = B * 2 * H * W
    mbuf = torch.full((guard + m + guard,), 0xC3, dtype=torch.uint8, device=DEV)
    mout = mbuf[guard:guard + m].view(B, 2, H, W)
    flags = torch.zeros(3, dtype=torch.int32, device=DEV)
    ws = torch.empty(K.lib.uda_display_masks_workspace_bytes(B, H, W), dtype=torch.uint8, device=DEV)
    rc = K.lib.uda_display_masks(d_prob.data_ptr(), B, H, W, 0.75, shapes.default_sweeps(H, W), mout.data_ptr(), flags.data_ptr(),
                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0 and int(flags.sum()) == 0
    assert bool((mbuf[:guard] == 0xC3).all()) and bool((mbuf[guard + m:] == 0xC3).all())
    assert np.array_equal(mout.cpu().numpy(), ovr.display_masks(prob)) and np.array_equal(d_prob.cpu().numpy(), prob)


# ---------------------------------------------------------------------------------------------------------------- image bytes
def test_image_u8_returns_all_256_levels():
    K = ops.kernels()
    x = torch.from_numpy(np.broadcast_to(ovr.normalized_levels()[None, None, None, :], (1, 3, 2, 256)).copy())
    got = K.image_u8(x.to(DEV)).cpu().numpy()
    assert got.shape == (1, 2, 256, 3) and (got == np.arange(256, dtype=np.uint8)[None, None, :, None]).all()
    y = torch.rand(2, 3, 19, 23, generator=torch.Generator().manual_seed(8)) * 2.4 - 1.2                  # with values to clip
    y[0, 0, 0, :5] = torch.tensor([-1.5, -1.0, 1.0, 1.5, 0.0])
    assert np.array_equal(K.image_u8(y.to(DEV)).cpu().numpy(), ovr.image_u8(y.numpy()))


# ---------------------------------------------------------------------------------------------------------------------- files
def _read(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im).copy()


def test_save_per_img_writes_the_two_files(tmp_path):
    name = "nested blob_in_ring"
    prob = dict(LIBRARY)[name].copy()
    keep = prob.copy()
    patch = ovr.random_image(1, 128, 128, 6)[0].astype(np.float64) + 0.75              # HWC in 0..255, truncated to bytes as the reference does
    patch_keep = patch.copy()
    Utils.save_per_img(patch, str(tmp_path), "V0007.crop.bmp", prob, mask_path=None, ext="bmp")
    assert np.array_equal(prob, keep) and np.array_equal(patch, patch_keep)
    assert sorted(os.listdir(tmp_path)) == ["original_image", "overlay"]
    original = _read(tmp_path / "original_image" / "V0007.png")
    assert np.array_equal(original, patch.astype(np.uint8))
    over = _read(tmp_path / "overlay" / "V0007.png")
    device = ops.overlay(_dev(original[None]), _dev(prob[None]))[0].cpu().numpy()
    assert np.array_equal(over, device) and np.array_equal(over, ovr.overlay(original, _oracle(name)))
    assert (over != original).any()


def test_evaluate_with_save_dir_returns_the_same_and_writes_three_files_per_image(tmp_path):
    batches, logits = sr.eval_batches(n_images=4, batch=2, S=128)
    model = sr.standin_model(logits)
    plain = ev.evaluate(model, batches, cdr=True)
    saved = ev.evaluate(model, batches, cdr=True, save_dir=str(tmp_path))
    assert repr(saved) == repr(plain)                                                  # NaN-proof equality of the whole result
    for i in range(4):
        b, k = divmod(i, 2)
        stem = "img_%02d" % i
        prob = torch.sigmoid(logits[i]).numpy()
        image = ovr.image_u8(batches[b]["image"][k:k + 1].numpy())[0]
        assert np.array_equal(_read(tmp_path / "original_image" / (stem + ".png")), image)
        assert np.array_equal(_read(tmp_path / "overlay" / (stem + ".png")), ovr.overlay(image, ovr.display_masks(prob)))
        pred = shapes.stages(prob, 0.75, 0.75)["filled"]                               # the evaluation masks, not the display masks
        assert np.array_equal(_read(tmp_path / "mask" / (stem + ".png")), ovr.grey_mask(pred))
    assert sorted(os.listdir(tmp_path)) == ["mask", "original_image", "overlay"]
    assert all(len(os.listdir(tmp_path / d)) == 4 for d in ("mask", "original_image", "overlay"))


def test_predict_main_on_a_folder(tmp_path):
    from PIL import Image
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    images = ovr.random_image(2, 64, 64, 12)
    for i in range(2):
        Image.fromarray(images[i]).save(src / ("eye_%d.png" % i))
    cup, disc = shapes.disc(64, 64, 30, 32, 12), shapes.disc(64, 64, 32, 32, 22)
    lg = torch.from_numpy(np.where(np.stack([cup, disc]), 6.0, -6.0).astype(np.float32))

    def model(x):                                                                      # stub: the same logits for every image
        assert x.dtype == torch.float32 and tuple(x.shape[1:]) == (3, 64, 64) and float(x.min()) >= -1.0 and float(x.max()) <= 1.0
        return lg.to(x.device)[None].expand(x.shape[0], -1, -1, -1).contiguous(), None
    rows = predict.main(["--images", str(src), "--out", str(out), "--csv", str(tmp_path / "cdr.csv"), "--batch-size", "2"], model=model)
    prob = torch.sigmoid(lg).numpy()
    pred = shapes.stages(prob, 0.75, 0.75)["filled"]
    ext = [np.nonzero(pred[c].any(1))[0] for c in range(2)]
    vcdr = (ext[0][-1] - ext[0][0] + 1) / (ext[1][-1] - ext[1][0] + 1)
    assert [r["img_name"] for r in rows] == ["eye_0.png", "eye_1.png"] and all(r["vcdr_pred"] == vcdr for r in rows)
    with open(tmp_path / "cdr.csv") as f:
        table = list(csv.reader(f))
    assert table[0] == ["img_name", "vcdr_pred"] and [t[0] for t in table[1:]] == ["eye_0.png", "eye_1.png"] and float(table[1][1]) == vcdr
    for i in range(2):
        stem = "eye_%d.png" % i
        assert np.array_equal(_read(out / "original_image" / stem), images[i])
        assert np.array_equal(_read(out / "overlay" / stem), ovr.overlay(images[i], ovr.display_masks(prob)))
        assert np.array_equal(_read(out / "mask" / stem), ovr.grey_mask(pred))
    Image.fromarray(ovr.random_image(1, 50, 64, 1)[0]).save(src / "odd_size.png")
    with pytest.raises(ValueError, match=r"odd_size\.png: input height/width must be multiples of 16, got 50x64"):
        predict.main(["--images", str(src), "--out", str(tmp_path / "out2")], model=model)
    assert not (tmp_path / "out2").exists()                                            # refused before anything ran
