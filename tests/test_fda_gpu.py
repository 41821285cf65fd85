"""-m gpu: uda_fda_spectrum and uda_fda_transfer (csrc/fda.hip) on the device against tests/fda_ref.py, the literal fft2 / fftshift /
swap window / ifft2 statement in numpy float64.

The shapes are the smallest at which the kernels can go wrong: 40 x 56 (B = 2, Bt = 3, band 3: not square, no multiple of 32 or 64; 56 % 4
== 0, so the rows go through the 4-byte loads), 33 x 47 (band 2: odd sizes, the centre H // 2, byte loads, the last lanes of a wave
without a pixel), 16 x 16 (band 7 = the largest the size allows, fewer pixels than lanes), 64 x 64 (band 5: one pass over v, as at 512 with
beta 0.01) and 136 x 136 (band 64: the cap, eleven passes of the chunked loop over v, more than one pixel per lane).  pair = [2, 0]
everywhere.

Spectrum: |dF| <= 1e-12 * sum|s| per channel (a float64 sum of N <= 2^15 terms of at most 255 errs by at most about N 2^-53 sum|s| = 2e-12
sum|s| at 136 x 136 in the worst case and far less in practice; the measured error is printed beside the bound).
Transfer: the bytes equal the oracle's.  tests/test_fda_cpu.py asserts of every fixture used here that no unrounded value lies within
1e-8 of a tie and no windowed source amplitude lies near the zero-magnitude threshold, so a correct float64 implementation has no
excuse."""
import numpy as np
import pytest
import torch

import fda_ref as fr
from kernel_cases import footprint, footprint_violations, out_dev, ro_dev
from uda_clr_amd import ops
from uda_clr_amd.kernels import FDA_MAX_BAND

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)             # (a copy: the shared fixtures are read-only)


def _transfer(fx, **kw):
    args = dict(band=fx["band"], pair=fx["pair"], apply=fx["apply"])
    args.update(kw)
    return ops.fda_transfer(_dev(fx["src"]), _dev(fx["tgt"]), **args).cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. spectrum
@pytest.mark.parametrize("name", list(fr.SHAPES))
def test_spectrum_against_numpy_fft2(name):
    fx = fr.fixture(name)
    img, b = fx["tgt"], fx["band"]                                     # three images
    N, H, W, _ = img.shape
    got = ops.fda_spectrum(_dev(img), b)
    assert got.dtype == torch.complex128 and tuple(got.shape) == (N, 3, 2 * b + 1, b + 1)
    got = got.cpu().numpy()
    full = np.fft.fft2(img.astype(np.float64), axes=(1, 2)).transpose(0, 3, 1, 2)             # [N, 3, H, W]
    want = full[:, :, np.arange(-b, b + 1) % H][:, :, :, :b + 1]
    err = np.abs(got - want).max(axis=(2, 3))
    bound = 1e-12 * img.astype(np.float64).sum(axis=(1, 2))
    print("%s: spectrum error %.3e, bound 1e-12 sum|s| = %.3e" % (name, err.max(), bound.min()))
    assert (err <= bound).all(), (err, bound)


# ------------------------------------------------------------------------------------------------------------ 2.-5. transfer
@pytest.mark.parametrize("name", fr.FIXTURES)
def test_transfer_bytes_equal_the_oracles(name):
    """the five shapes with pair = [2, 0]; 'apply' = [1, 0]: sample 1 is its source; 'constant': source channels all 0 and all 200 (the
    zero-magnitude rule); 'clip': a bright target on a dark source and the reverse, pixels clamped at both ends"""
    fx, want, raw = fr.reference(name)
    got = _transfer(fx)
    diff = got != want
    print("%s: %d of %d bytes differ from the oracle%s" % (name, int(diff.sum()), diff.size,
                                                           "" if not diff.any() else ", first at %s: %d, oracle %.9f" %
                                                           (tuple(np.argwhere(diff)[0]), got[diff][0], raw[diff][0])))
    assert not diff.any()
    if name == "apply":
        assert np.array_equal(got[1], fx["src"][1]) and not np.array_equal(got[0], fx["src"][0])
    if name == "clip":
        assert (raw[0] > 255.5).any() and (raw[1] < -0.5).any() and got[0].max() == 255 and got[1].min() == 0
    if name == "constant":
        assert len(np.unique(got[0, :, :, 0])) > 1                   # the constant channels took the target's low frequencies


@pytest.mark.parametrize("name", list(fr.SHAPES))
def test_a_target_equal_to_the_source_gives_identical_bytes(name):
    fx = fr.fixture(name)
    got = ops.fda_transfer(_dev(fx["src"]), _dev(fx["src"]), band=fx["band"]).cpu().numpy()
    assert np.array_equal(got, fx["src"])


def test_defaults_band_from_beta_and_pairs_in_turn():
    fx, _, _ = fr.reference("64x64 b5")
    src = np.concatenate([fx["src"], fx["src"][:1], fx["src"][1:]])               # B = 4 > Bt = 3: pair = [0, 1, 2, 0]
    got = ops.fda_transfer(_dev(src), _dev(fx["tgt"]), beta=0.08).cpu().numpy()   # floor(0.08 * 64) = 5
    want, _ = fr.oracle(src, fx["tgt"], 5, [0, 1, 2, 0])
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------ 6. footprint
@pytest.mark.parametrize("name", ["33x47 b2", "136x136 b64"])
def test_both_entries_write_only_their_outputs(name):
    fx, want, _ = fr.reference(name)
    K = ops.kernels()
    B, H, W, _ = fx["src"].shape
    b = fx["band"]
    with footprint():
        src, tgt = ro_dev(_dev(fx["src"]), DEV, name="source"), ro_dev(_dev(fx["tgt"]), DEV, name="target")
        pair = ro_dev(torch.tensor(fx["pair"], dtype=torch.int32), DEV, name="pair")
        apply = ro_dev(torch.tensor([1, 1], dtype=torch.uint8), DEV, name="apply")
        spec = out_dev((B, 3, 2 * b + 1, b + 1, 2), torch.float64, DEV, name="spectrum")
        out = out_dev((B, H, W, 3), torch.uint8, DEV, name="out")
        K.fda_spectrum(src, b, out=spec)
        K.fda_transfer(src, tgt, pair, b, apply=apply, out=out)
        torch.cuda.synchronize()
        assert footprint_violations() == []
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(torch.view_as_complex(spec), ops.fda_spectrum(src, b))


# ------------------------------------------------------------------------------------------------------------ 7. reproducibility
@pytest.mark.parametrize("name", ["40x56 b3", "136x136 b64"])
def test_two_calls_give_equal_bytes(name):
    fx = fr.fixture(name)
    src, tgt = _dev(fx["src"]), _dev(fx["tgt"])
    a = ops.fda_transfer(src, tgt, band=fx["band"], pair=fx["pair"])
    s1 = ops.fda_spectrum(tgt, fx["band"])
    b = ops.fda_transfer(src, tgt, band=fx["band"], pair=fx["pair"])
    s2 = ops.fda_spectrum(tgt, fx["band"])
    assert torch.equal(a, b) and torch.equal(torch.view_as_real(s1).view(torch.int64), torch.view_as_real(s2).view(torch.int64))


# ------------------------------------------------------------------------------------------------------------ 8. argument errors
def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("what, H, W, Ht, Wt, band, match", [
    ("band above the cap", 136, 136, 136, 136, FDA_MAX_BAND + 1, "band 65"),
    ("band too wide for the size", 16, 40, 16, 40, 8, "2 band \\+ 2"),
    ("negative band", 16, 16, 16, 16, -1, "band -1"),
    ("sizes differ", 40, 56, 56, 40, 3, "differ"),
])
def test_raw_abi_argument_errors_write_nothing(what, H, W, Ht, Wt, band, match):
    import re
    K = ops.kernels()
    B, Bt = 2, 3
    src = torch.zeros(B, H, W, 3, dtype=torch.uint8, device=DEV)
    tgt = torch.zeros(Bt, Ht, Wt, 3, dtype=torch.uint8, device=DEV)
    pair = torch.zeros(B, dtype=torch.int32, device=DEV)
    out = torch.full((B, H, W, 3), 0x5A, dtype=torch.uint8, device=DEV)
    spec = torch.full((B, 3, 2 * abs(band) + 1, abs(band) + 1, 2), -7.0, dtype=torch.float64, device=DEV)
    ws = torch.full((1 << 22,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = K.lib.uda_fda_transfer(src.data_ptr(), B, H, W, tgt.data_ptr(), Bt, Ht, Wt, pair.data_ptr(), None, band, out.data_ptr(), ws.data_ptr(),
                                ws.numel(), _stream())
    assert rc != 0 and re.search(match, K.lib.uda_last_error().decode()), K.lib.uda_last_error()
    if (H, W) == (Ht, Wt):
        rc = K.lib.uda_fda_spectrum(src.data_ptr(), B, H, W, band, spec.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        assert rc != 0 and re.search(match, K.lib.uda_last_error().decode()), K.lib.uda_last_error()
        if not 0 <= band <= FDA_MAX_BAND:
            assert K.lib.uda_fda_workspace_bytes(B, Bt, H, W, band) == 0
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((spec == -7.0).all()) and bool((ws == 0x5A).all())


def test_raw_abi_refuses_empty_batches_and_a_small_workspace():
    K = ops.kernels()
    src = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    pair = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.full((2, 16, 16, 3), 0x5A, dtype=torch.uint8, device=DEV)
    need = K.lib.uda_fda_workspace_bytes(2, 2, 16, 16, 3)
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device=DEV)
    call = lambda B, Bt, n: K.lib.uda_fda_transfer(src.data_ptr(), B, 16, 16, src.data_ptr(), Bt, 16, 16, pair.data_ptr(), None, 3, out.data_ptr(),
                                                  ws.data_ptr(), n, _stream())
    assert need > 0
    for B, Bt, n in ((0, 2, need), (2, 0, need), (2, 2, need - 1)):
        assert call(B, Bt, n) != 0 and K.lib.uda_last_error().decode().startswith("uda_fda_transfer")
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all()) and bool((ws == 0x5A).all())
    assert call(2, 2, need) == 0


def test_python_layer_raises_value_errors_with_the_shapes():
    K = ops.kernels()
    src = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV)
    tgt = torch.zeros(3, 16, 16, 3, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match=r"pair .*\[0, 3\)"):
        ops.fda_transfer(src, tgt, band=2, pair=[0, 3])
    with pytest.raises(ValueError, match=r"pair .*\[0, 3\)"):
        ops.fda_transfer(src, tgt, band=2, pair=[-1, 0])
    with pytest.raises(ValueError, match="differ.*16, 24"):
        ops.fda_transfer(src, torch.zeros(3, 16, 24, 3, dtype=torch.uint8, device=DEV), band=2)
    with pytest.raises(ValueError, match="band 8"):
        ops.fda_transfer(src, tgt, band=8)
    with pytest.raises(ValueError, match="uint8"):
        K.fda_spectrum(src.float(), 2)
    with pytest.raises(ValueError, match="contiguous"):
        K.fda_spectrum(src.transpose(1, 2), 2)
    with pytest.raises(ValueError, match="int32"):
        K.fda_transfer(src, tgt, torch.zeros(2, dtype=torch.int64, device=DEV), 2)
    # device-side pair values are not read back: the kernel clamps them into [0, Bt)
    fx, _, _ = fr.reference("16x16 b7")
    got = K.fda_transfer(_dev(fx["src"]), _dev(fx["tgt"]), torch.tensor([7, -3], dtype=torch.int32, device=DEV), 7).cpu().numpy()
    assert np.array_equal(got, fr.oracle(fx["src"], fx["tgt"], 7, [2, 0])[0])


# ------------------------------------------------------------------------------------------------------------ 9. trainer
def _trainer(tmp_path):
    from uda_clr_amd.train_process import Trainer_prototype_full
    m, d1, d2 = (torch.nn.Conv2d(3, 2, 1).to(DEV) for _ in range(3))
    og, od, od2 = (torch.optim.SGD(x.parameters(), lr=0.1) for x in (m, d1, d2))
    return Trainer_prototype_full.Trainer(False, m, d1, d2, og, od, od2, [], [], [], str(tmp_path), 1)


def _level1(seed, B, S=64):
    g = torch.Generator().manual_seed(seed)
    lab = torch.full((B, S, S), 255, dtype=torch.uint8)
    lab[:, 12:52, 10:50] = 128
    lab[:, 24:40, 22:38] = 0
    return {"image_u8": torch.from_numpy(fr.images(seed, B, S, S)), "label_u8": lab.roll(int(torch.randint(0, 5, (1,), generator=g)), 1)}


def test_decode_pair_styles_the_source_before_its_tail(tmp_path, monkeypatch):
    monkeypatch.delenv("UDA_CLR_FDA", raising=False)
    tr = _trainer(tmp_path)
    assert (tr.fda_beta, tr.fda_p) == (0.0, 1.0)
    S, T = _level1(31, 2), _level1(32, 3)
    offS, offT = tr._decode_pair(S, T)
    plainS, plainT = tr._decode(S), tr._decode(T)
    for k in ("image", "map", "boundary"):
        assert torch.equal(offS[k].view(torch.int32), plainS[k].view(torch.int32)) and torch.equal(offT[k].view(torch.int32), plainT[k].view(torch.int32)), k
    tr.fda_beta = 0.08                                               # band 5 at 64 x 64
    onS, onT = tr._decode_pair(S, T)
    styled = ops.fda_transfer(S["image_u8"].to(DEV), T["image_u8"].to(DEV), beta=0.08)
    assert np.array_equal(styled.cpu().numpy(), fr.oracle(S["image_u8"].numpy(), T["image_u8"].numpy(), 5)[0])
    image, mp, bd = ops.normalize_tf(styled, S["label_u8"].to(DEV))
    assert torch.equal(onS["image"].view(torch.int32), image.view(torch.int32)) and not torch.equal(onS["image"], plainS["image"])
    assert torch.equal(onS["map"], plainS["map"]) and torch.equal(onS["boundary"], plainS["boundary"])
    assert torch.equal(onS["map"], mp) and torch.equal(onS["boundary"], bd)
    for k in ("image", "map", "boundary"):
        assert torch.equal(onT[k].view(torch.int32), plainT[k].view(torch.int32)), k


def test_the_trainer_reads_the_setting_at_construction(tmp_path, monkeypatch):
    monkeypatch.setenv("UDA_CLR_FDA", "0.09,0.25")
    tr = _trainer(tmp_path)
    assert (tr.fda_beta, tr.fda_p) == (0.09, 0.25)
