"""-m gpu: uda_postprocess (csrc/postproc.hip) and HipKernels.postprocess on the adversarial masks of tests/postproc_shapes.py,
against the scipy chain, bit for bit (np.array_equal; there is no tolerance anywhere).

tests/test_postproc_cpu.py proves with scipy and a numpy model of the tile launches what these masks are: a spiral that needs 50
launches (the default at 256 x 256 is 36, six doublings from 1 end at 32), a ring that is one component only by diagonal contacts
around a hole that is a hole only by the 4-neighbourhood, two components of equal area, planes smaller than the windows.  So:
  * labels by the 4-neighbourhood or a flood by the 8-neighbourhood changes thousands of pixels of 'diagonal ring';
  * "last maximum" instead of "first" keeps the other disc of 'tie equal' and 'tie third_first';
  * returning after the first attempt whatever the flags say returns a part of the spiral only."""
import numpy as np
import pytest
import torch

import postproc_shapes as ps
from kernel_cases import _scipy_postprocess
from uda_clr_amd import ops
from uda_clr_amd.kernels import UdaError

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
THR = 0.75
LIBRARY = ps.library()
_ORACLE = {}


def _oracle(name, prob):
    """the oracle's stages of one [2,H,W] plane pair, computed once per session and never written to"""
    if name not in _ORACLE:
        st = ps.stages(prob, THR, THR)
        assert np.array_equal(st["filled"], _scipy_postprocess(prob, THR, THR))
        for a in st.values():
            a.setflags(write=False)
        _ORACLE[name] = st
    return _ORACLE[name]


def _named(name):
    prob = dict(LIBRARY)[name]
    return prob, _oracle(name, prob)


def _device(prob, **kw):
    out = ops.kernels().postprocess(torch.from_numpy(np.ascontiguousarray(prob)).to(DEV), THR, THR, **kw)
    assert out.dtype == torch.uint8 and tuple(out.shape) == tuple(prob.shape)
    return out.cpu().numpy()


def _explain(got, st):
    """per channel: how many pixels differ from the oracle, and which of the oracle's stages the device output still equals"""
    lines = []
    for c in range(2):
        same = [k for k in ("eroded", "keep", "filled") if np.array_equal(got[c], st[k][c])]
        lines.append("channel %d: %d pixels differ from the oracle (%d set, oracle %d); equal to the oracle's stage(s): %s" % (
            c, int((got[c] != st["filled"][c]).sum()), int((got[c] > 0).sum()), int(st["filled"][c].sum()), ", ".join(same) or "none"))
    return "\n".join(lines)


def _assert_oracle(got, st, what):
    assert np.array_equal(got, st["filled"]), what + "\n" + _explain(got, st)


@pytest.mark.parametrize("name", [n for n, _ in LIBRARY])
def test_shape_matches_the_oracle(name):
    prob, st = _named(name)
    _assert_oracle(_device(prob[None])[0], st, name)


def _mixed_batch():
    names = ("spiral 256/20/18", "zeros 256", "diagonal ring in 256", "ones 256")
    probs = (dict(LIBRARY)[names[0]], ps.zeros(256, 256), ps.diagonal_ring(pad_to=256), ps.ones(256, 256))
    return names, probs


def test_batch_of_planes_that_finish_at_different_times_equals_the_singles():
    """B = 4: the 50-launch spiral next to planes that finish in one to four launches; one pair of convergence flags for all"""
    names, probs = _mixed_batch()
    batch = _device(np.stack(probs))
    for b, (name, prob) in enumerate(zip(names, probs)):
        st = _oracle(name, prob)
        _assert_oracle(batch[b], st, "%s in the batch" % name)
        _assert_oracle(_device(prob[None])[0], st, "%s alone" % name)


# ------------------------------------------------------------------------------------------------------------- raw C ABI
GUARD = 4096


def _raw(prob, sweeps, short=0):
    """uda_postprocess on [B,2,H,W] with output and workspace pre-filled with 0xA5 and GUARD more bytes of it behind each; the
    workspace is exactly uda_postprocess_workspace_bytes (minus `short`) long as far as the library knows"""
    K = ops.kernels()
    B, _, H, W = prob.shape
    pred = torch.from_numpy(np.ascontiguousarray(prob)).to(DEV)
    n = B * 2 * H * W
    need = K.lib.uda_postprocess_workspace_bytes(B, H, W)
    assert need >= n * 14 + 2 * B * 4                     # three int planes, two byte planes, one int per plane
    out = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = torch.full((need + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    flags = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    rc = K.lib.uda_postprocess(pred.data_ptr(), B, H, W, THR, THR, sweeps, out.data_ptr(), flags.data_ptr(), ws.data_ptr(),
                               need - short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    err = K.lib.uda_last_error() if rc != 0 else b""
    return rc, err, out[:n].cpu().numpy().reshape(B, 2, H, W), flags.cpu().numpy(), out[n:].cpu().numpy(), ws[:need].cpu().numpy(), ws[need:].cpu().numpy()


def test_raw_entry_point_reports_unfinished_tiles_after_one_sweep():
    """sweeps = 1: after the first launch no label has left its own tile (the halo is read from the launch's input), the spiral's
    first label has 50 tiles to go, so the reporting launch still changes tiles - derived, not measured"""
    prob, _ = _named("spiral 256/20/18")
    rc, _, out, flags, out_guard, _, ws_guard = _raw(prob[None], 1)
    assert rc == 0
    print("sweeps=1: not_converged = %s" % flags.tolist())
    assert flags[0] > 0 and flags[1] >= 0
    assert np.isin(out, (0, 1)).all() and (out_guard == 0xA5).all() and (ws_guard == 0xA5).all()


def test_raw_entry_point_converges_with_64_sweeps_inside_its_buffers():
    prob, st = _named("spiral 256/20/18")
    rc, _, out, flags, out_guard, _, ws_guard = _raw(prob[None], 64)
    assert rc == 0 and flags.tolist() == [0, 0]
    _assert_oracle(out[0], st, "sweeps=64")
    assert (out_guard == 0xA5).all() and (ws_guard == 0xA5).all()


def test_raw_entry_point_ragged_plane_stays_inside_its_buffers():
    """33 x 17 and B = 2: partial tiles in both directions, plane sizes that are no multiple of 4 bytes"""
    prob, st = _named("blob 33x17")
    rc, _, out, flags, out_guard, _, ws_guard = _raw(np.stack([prob, prob[::-1]]), 4)
    assert rc == 0 and flags.tolist() == [0, 0]
    _assert_oracle(out[0], st, "33x17, image 0")
    assert np.array_equal(out[1], st["filled"][::-1])
    assert (out_guard == 0xA5).all() and (ws_guard == 0xA5).all()


@pytest.mark.parametrize("case", ["short workspace", "sweeps=0"])
def test_raw_entry_point_rejects_bad_arguments_and_writes_nothing(case):
    prob, _ = _named("spiral 256/20/18")
    rc, err, out, flags, out_guard, ws, ws_guard = _raw(prob[None], 0 if case == "sweeps=0" else 8, short=1 if case == "short workspace" else 0)
    assert rc != 0 and b"uda_postprocess" in err
    assert (out == 0xA5).all() and (ws == 0xA5).all() and flags.tolist() == [-7, -7]
    assert (out_guard == 0xA5).all() and (ws_guard == 0xA5).all()


# ------------------------------------------------------------------------------------------------------------ the retry loop
@pytest.fixture
def attempts(monkeypatch):
    """the `sweeps` argument of every uda_postprocess call HipKernels.postprocess makes"""
    lib = ops.kernels().lib
    real, seen = lib.uda_postprocess, []

    def spy(*args):
        seen.append(args[6])
        return real(*args)
    monkeypatch.setattr(lib, "uda_postprocess", spy)
    return seen


def test_default_sweeps_retry_once_on_the_spiral(attempts):
    """50 launches needed, 36 by default (tests/test_postproc_cpu.py): the answer cannot come from the first attempt"""
    prob, st = _named("spiral 256/20/18")
    _assert_oracle(_device(prob[None])[0], st, "default sweeps")
    assert attempts == [ps.default_sweeps(256, 256), 2 * ps.default_sweeps(256, 256)]


def test_sweeps_argument_is_used_and_doubled_until_converged(attempts):
    """the 192 spiral needs 29 launches: 1, 2, 4, 8 and 16 fail, 32 succeeds"""
    prob, st = _named("spiral 192/20/18")
    _assert_oracle(_device(prob[None], sweeps=1)[0], st, "sweeps=1")
    assert attempts == [1, 2, 4, 8, 16, 32]


def test_gives_up_after_six_attempts_without_returning_a_mask(attempts):
    prob, _ = _named("spiral 256/20/18")
    got = None
    with pytest.raises(UdaError, match="did not converge after 32 sweeps"):
        got = _device(prob[None], sweeps=1)
    assert got is None and attempts == [1, 2, 4, 8, 16, 32]


def test_easy_shapes_take_one_attempt(attempts):
    prob, st = _named("diagonal ring")
    _assert_oracle(_device(prob[None])[0], st, "diagonal ring")
    assert attempts == [ps.default_sweeps(136, 136)]


# ------------------------------------------------------------------------------------------------------------- drop-in path
def test_utils_postprocessing_batch_on_the_diagonal_ring():
    from uda_clr_amd.utils import Utils
    prob, st = _named("diagonal ring")
    out = Utils.postprocessing_batch(torch.from_numpy(prob[None]))               # a host tensor: moved to the device
    assert out.is_cuda and out.dtype == torch.uint8
    _assert_oracle(out[0].cpu().numpy(), st, "postprocessing_batch")
    one = Utils.postprocessing(torch.from_numpy(prob), threshold=THR, dataset='G')
    assert isinstance(one, np.ndarray) and one.dtype == np.uint8
    _assert_oracle(one, st, "postprocessing")
