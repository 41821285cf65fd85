"""not-gpu: the yardstick of the Fourier style transfer (tests/fda_ref.py) against an independent restatement and against what the
transfer must do by definition; the conditions under which the GPU tests may ask for byte equality, for every fixture they use; and
the trainers' host logic (TrainerBase._decode_pair, the UDA_CLR_FDA setting) with stand-in ops whose fda_transfer is the yardstick."""
import numpy as np
import pytest
import torch

import fda_ref as fr
from uda_clr_amd import ops
from uda_clr_amd.train_process import Trainer_baseline
from uda_clr_amd.train_process._common import HipOps, TrainerBase


# ------------------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("name", fr.FIXTURES)
def test_oracle_equals_the_partial_dft_restatement(name):
    """fft2 / fftshift / swap / ifft2 and the explicit sum over the window agree to 1e-9 grey levels (measured: below 2e-12)"""
    fx, u8, raw = fr.reference(name)
    got = fr.partial_dft(fx["src"], fx["tgt"], fx["band"], fx["pair"])
    if fx["apply"] is not None:
        keep = np.asarray(fx["apply"]) == 0
        got[keep] = fx["src"][keep]
    err = float(np.abs(got - raw).max())
    print("%s: restatement differs by %.2e grey levels" % (name, err))
    assert err <= 1e-9


@pytest.mark.parametrize("name", list(fr.SHAPES))
def test_a_target_equal_to_the_source_gives_the_source_back(name):
    fx = fr.fixture(name)
    u8, raw = fr.oracle(fx["src"], fx["src"], fx["band"])
    assert np.array_equal(u8, fx["src"]) and np.abs(raw - fx["src"]).max() < 1e-9


@pytest.mark.parametrize("name", list(fr.SHAPES))
def test_band_zero_moves_each_channel_mean_to_the_targets(name):
    """band 0 swaps |F[0,0]| = the channel sum: the unrounded output's mean is the target's mean (the bytes' mean to rounding)"""
    fx = fr.fixture(name)
    u8, raw = fr.oracle(fx["src"], fx["tgt"], 0, fx["pair"])
    want = fx["tgt"][fx["pair"]].astype(np.float64).mean(axis=(1, 2))
    assert np.abs(raw.mean(axis=(1, 2)) - want).max() < 1e-9
    inside = (raw > 0) & (raw < 255)
    if inside.all():                                    # without clipping each byte is within half a grey level of its value
        assert np.abs(u8.astype(np.float64).mean(axis=(1, 2)) - want).max() <= 0.5
    assert np.abs(np.clip(raw, 0, 255) - u8).max() <= 0.5


@pytest.mark.parametrize("name", fr.FIXTURES)
def test_fixtures_leave_no_room_for_a_rounding_dispute(name):
    """byte equality on the GPU is a fair demand: no unrounded value within 1e-8 of a tie (a thousand times the float64 disagreement of
    the two statements here), and no windowed source amplitude between 1e-9 H W and 1e-3 H W (the zero-magnitude rule's threshold is
    1e-6 H W: nothing comes near it from either side)"""
    fx, u8, raw = fr.reference(name)
    tie = fr.tie_distance(raw)
    amp = fr.windowed_amplitudes(fx["src"], fx["band"])
    between = (amp >= 1e-9) & (amp <= 1e-3)
    print("%s: closest tie %.2e, smallest amplitude above the rule %.2e H W, %d at zero" % (name, tie, amp[amp > 1e-3].min(), int((amp < 1e-9).sum())))
    assert tie > 1e-8
    assert not between.any(), amp[between]
    if name == "constant":
        assert (amp < 1e-9).sum() >= 4 * (2 * fx["band"] + 1) ** 2 - 4          # the constant channels: everything but (at most) F[0,0]
    if name == "clip":
        assert (raw[0] > 255.5).any() and (raw[1] < -0.5).any()               # at least one pixel clamped at each end
        assert u8[0].max() == 255 and u8[1].min() == 0


def test_ops_defaults_and_host_side_checks_need_no_device():
    assert ops.fda_band(0.01, 512, 512) == 5 and ops.fda_band(0.09, 512, 512) == 46 and ops.fda_band(0.01, 64, 512) == 0
    src, tgt = torch.zeros(2, 16, 16, 3, dtype=torch.uint8), torch.zeros(3, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"pair .*\[0, 3\)"):
        ops.fda_transfer(src, tgt, band=2, pair=[0, 3])
    with pytest.raises(ValueError, match="pair"):
        ops.fda_transfer(src, tgt, band=2, pair=[0])
    assert "fda_transfer" in vars(HipOps()) and HipOps().fda_transfer is ops.fda_transfer


# ------------------------------------------------------------------------------------------------------------ the trainers
class _Ops(object):
    """what _decode_head / _decode_tail call, as plain torch on the CPU; fda_transfer is the yardstick"""
    def __init__(self):
        self.calls = []

    def fda_transfer(self, src, tgt, beta=0.01, band=None, pair=None, apply=None):
        self.calls.append(("fda", beta, None if apply is None else apply.tolist()))
        b = ops.fda_band(beta, src.shape[1], src.shape[2]) if band is None else band
        return torch.from_numpy(fr.oracle(src.numpy(), tgt.numpy(), b, pair, None if apply is None else apply.numpy())[0])

    def elastic_deform(self, iu, lu, apply=None, noise=None):
        self.calls.append(("elastic",))
        return iu.flip(1), lu.flip(1)

    def photometric_u8(self, iu, pos, n, val, lut, erase):
        self.calls.append(("photometric",))
        return torch.stack([lut[b][iu[b].long()] for b in range(iu.shape[0])])

    def normalize_tf(self, iu, lu):
        self.calls.append(("normalize_tf",))
        return iu.permute(0, 3, 1, 2).float() / 127.5 - 1.0, torch.stack([(lu <= 50).float(), (lu <= 200).float()], 1), (lu[:, None] == 128).float()


class _T(TrainerBase):
    def __init__(self):
        self.ops = _Ops()

    def _to(self, t):
        return t

    def _device(self):
        return torch.device("cpu")


def _sample(seed, B, S=32, level=1):
    g = torch.Generator().manual_seed(seed)
    s = {"image_u8": torch.from_numpy(fr.images(seed, B, S, S)), "label_u8": torch.randint(0, 256, (B, S, S), generator=g).to(torch.uint8),
         "img_name": ["s%d" % i for i in range(B)]}
    if level == 2:
        s.update(aug_elastic=torch.ones(B, 1, dtype=torch.uint8), aug_sp_pos=torch.zeros(B, 1, 2, dtype=torch.int32),
                 aug_sp_n=torch.zeros(B, dtype=torch.int32), aug_sp_val=torch.zeros(B, dtype=torch.int32),
                 aug_lut=torch.stack([torch.randperm(256, generator=g) for _ in range(B)]).to(torch.uint8), aug_erase=torch.zeros(B, 5, dtype=torch.int32))
    return s


def _same(a, b):
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


@pytest.mark.parametrize("level", [1, 2])
def test_decode_pair_with_fda_off_is_the_two_decode_calls(level):
    t = _T()
    S, T = _sample(1, 2, level=level), _sample(2, 3, level=level)
    for off in (None, 0.0):
        if off is not None:
            t.fda_beta, t.fda_p = off, 1.0
        dS, dT = t._decode_pair(S, T)
        _same(dS, t._decode(S))
        _same(dT, t._decode(T))
    assert not any(c[0] == "fda" for c in t.ops.calls)
    decoded = {k: v for k, v in t._decode(S).items() if k in ("image", "map", "boundary", "img_name")}      # what level 0 hands over
    assert t._decode(decoded) is decoded                      # a decoded sample still passes through
    assert t._decode_head(decoded) is None


def test_decode_pair_with_fda_on_transfers_between_the_heads_and_the_tails():
    t = _T()
    t.fda_beta, t.fda_p = 0.07, 1.0                           # band 2 at 32 x 32
    S, T = _sample(3, 2, level=2), _sample(4, 3, level=2)
    dS, dT = t._decode_pair(S, T)
    assert [c[0] for c in t.ops.calls] == ["fda", "elastic", "photometric", "normalize_tf", "elastic", "photometric", "normalize_tf"]
    assert t.ops.calls[0] == ("fda", 0.07, None)
    styled = torch.from_numpy(fr.oracle(S["image_u8"].numpy(), T["image_u8"].numpy(), 2)[0])
    assert not torch.equal(styled, S["image_u8"])
    _same(dS, t._decode_tail(S, styled, S["label_u8"]))
    plain = t._decode(S)
    assert torch.equal(dS["map"], plain["map"]) and torch.equal(dS["boundary"], plain["boundary"]) and not torch.equal(dS["image"], plain["image"])
    _same(dT, t._decode(T))                                   # the target is what it was


def test_fda_probability_is_drawn_per_sample_on_the_host():
    t = _T()
    t.fda_beta, t.fda_p = 0.07, 0.5
    S, T = _sample(5, 8), _sample(6, 8)
    torch.manual_seed(0)
    want = (torch.rand(8) < 0.5).to(torch.uint8)
    torch.manual_seed(0)
    dS, _ = t._decode_pair(S, T)
    assert t.ops.calls[0] == ("fda", 0.07, want.tolist()) and 0 < int(want.sum()) < 8
    plain = t._decode(S)["image"]
    for b in range(8):
        assert torch.equal(dS["image"][b], plain[b]) == (want[b] == 0)
    t.fda_p = 0.0
    assert torch.equal(t._decode_pair(S, T)[0]["image"], plain)


def test_level0_batches_raise_and_name_the_setting():
    t = _T()
    t.fda_beta, t.fda_p = 0.07, 1.0
    S, T = _sample(7, 2), _sample(8, 2)
    level0 = lambda s: {k: v for k, v in t._decode(s).items() if k not in ("image_u8", "label_u8")}
    for a, b, which in ((level0(S), T, "source"), (S, level0(T), "target")):
        with pytest.raises(ValueError, match="UDA_CLR_FDA.*UDA_CLR_DEVICE_INPUT.*%s" % which):
            t._decode_pair(a, b)


def test_the_setting_is_read_once_into_attributes(monkeypatch):
    t = _T()
    monkeypatch.delenv("UDA_CLR_FDA", raising=False)
    t._read_fda()
    assert (t.fda_beta, t.fda_p) == (0.0, 1.0)
    for text, want in (("0.01", (0.01, 1.0)), ("0.09,0.5", (0.09, 0.5)), ("0", (0.0, 1.0)), (" 0.02 , 1 ", (0.02, 1.0))):
        monkeypatch.setenv("UDA_CLR_FDA", text)
        t._read_fda()
        assert (t.fda_beta, t.fda_p) == want
    for text in ("x", "0.01,2", "0.6", "-0.1", "0.01,0.5,3"):
        monkeypatch.setenv("UDA_CLR_FDA", text)
        with pytest.raises(ValueError, match="UDA_CLR_FDA"):
            t._read_fda()


def test_trainer_baseline_raises_at_construction_when_the_setting_is_on(monkeypatch, tmp_path):
    m = torch.nn.Linear(1, 1)
    args = dict(cuda=False, model_gen=m, optimizer_gen=torch.optim.Adam(m.parameters()), val_loader=[], domain_loaderS=[], domain_loaderT=[],
                out=str(tmp_path / "run"), max_epoch=1)
    monkeypatch.setenv("UDA_CLR_FDA", "0.01")
    with pytest.raises(ValueError, match="UDA_CLR_FDA=0.01.*no target batch"):
        Trainer_baseline.Trainer(**args)
    assert not (tmp_path / "run").exists()
    monkeypatch.setenv("UDA_CLR_FDA", "0")
    assert Trainer_baseline.Trainer(**args).fda_beta == 0.0
