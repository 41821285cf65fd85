"""The write-footprint harness of tests/kernel_cases.py can fail: small fake "kernels" (plain torch on CPU tensors) that write
exactly their window report nothing, and each that puts one element elsewhere is reported with the buffer's name and the
position.  Then the bn / resample / gap cases run on the CPU with SpecKernels standing in for HipKernels (same calls): a correct
implementation passes the harness."""
import pytest
import torch

import kernel_cases as kc
from kernel_cases import (GUARD_BYTES, GUARD_ROWS, footprint, footprint_violations, gen, only_writes, out_dev, padded, read_only,
                          ro_dev, to_dev)
from uda_clr_amd.acts import round4

CPU = torch.device("cpu")
P, C = 6, 5                    # round4(C) = 8, ld = 12: lanes 5..7 are padding lanes, 8..11 the four extra floats of padded()
LD = round4(C) + 4


def _rows(v, first, n):
    """rows [first, first + n) x all ld columns of the allocation behind the [P, C] view v (first may be negative)"""
    return v.as_strided((n, v.stride(0)), (v.stride(0), 1), v.storage_offset() + first * v.stride(0))


def _bytes(t, first, n):
    """n bytes of the allocation behind the contiguous tensor t, from byte ``first`` of t (may be negative)"""
    b = t.view(-1).view(torch.uint8)
    return b.as_strided((n,), (1,), b.storage_offset() + first)


def _buffers():
    g = gen(0)
    out = to_dev(padded(P, C, g), CPU, name="out")
    st = out_dev((16, 2, C), torch.float64, CPU, fill=0, name="stats")
    dw = out_dev((4, 3), torch.float32, CPU, name="dw")
    w = ro_dev(torch.randn(7, generator=g), CPU, name="weight")
    x = ro_dev(padded(P, C, g), CPU, name="x")
    from uda_clr_amd.kernels import HipKernels
    ws = HipKernels._ws(w, 40)              # (patched by ``footprint``: the guarded workspace)
    return out, st, dw, w, x, ws


def _exact(out, st, dw, w, x, ws):
    out.fill_(1.0)
    st.fill_(2.0)
    dw.fill_(3.0)
    ws.fill_(7)


FAULTS = {
    "lane C": (lambda out, st, dw, w, x, ws: _rows(out, 2, 1)[0, C:C + 1].fill_(1.0), "out", (2, C)),
    "column round4(C) + 1": (lambda out, st, dw, w, x, ws: _rows(out, 2, 1)[0, round4(C) + 1:round4(C) + 2].fill_(1.0), "out", (2, round4(C) + 1)),
    "row P": (lambda out, st, dw, w, x, ws: _rows(out, P, 1)[0, :1].fill_(1.0), "out", (P, 0)),
    "row -1": (lambda out, st, dw, w, x, ws: _rows(out, -1, 1)[0, 3:4].fill_(1.0), "out", (-1, 3)),
    "last guard row": (lambda out, st, dw, w, x, ws: _rows(out, P + GUARD_ROWS - 1, 1)[0, LD - 1:].fill_(1.0), "out", (P + GUARD_ROWS - 1, LD - 1)),
    "channel C of the last statistics slot": (lambda out, st, dw, w, x, ws: _bytes(st, 16 * 2 * C * 8, 8).view(torch.float64).fill_(1.0),
                                              "stats", 16 * 2 * C * 8),
    "one byte behind a flat output": (lambda out, st, dw, w, x, ws: _bytes(dw, 48, 1).fill_(0), "dw", 48),
    "one byte before a flat output": (lambda out, st, dw, w, x, ws: _bytes(dw, -1, 1).fill_(0), "dw", -1),
    "last guard byte of a flat output": (lambda out, st, dw, w, x, ws: _bytes(dw, 48 + GUARD_BYTES - 1, 1).fill_(0), "dw", 48 + GUARD_BYTES - 1),
    "one element of a read-only vector": (lambda out, st, dw, w, x, ws: w[3:4].add_(1.0), "weight", 3 * 4),
    "one element of a read-only matrix": (lambda out, st, dw, w, x, ws: x[1, 2:3].add_(1.0), "x", (1, 2)),
    "one byte past nbytes of a workspace": (lambda out, st, dw, w, x, ws: _bytes(ws, 40, 1).fill_(0), "workspace", 40),
    "one byte before a workspace": (lambda out, st, dw, w, x, ws: _bytes(ws, -1, 1).fill_(0), "workspace", -1),
}


def test_a_kernel_that_writes_exactly_its_windows_reports_nothing():
    with footprint():
        bufs = _buffers()
        assert bufs[0].data_ptr() % 16 == 0 and bufs[0].stride(0) == LD and bufs[1].data_ptr() % 16 == 0 and bufs[5].data_ptr() % 16 == 0
        assert bufs[5].numel() == 40
        _exact(*bufs)
    assert footprint_violations() == []


@pytest.mark.parametrize("fault", list(FAULTS), ids=list(FAULTS))
def test_one_stray_element_is_reported_with_buffer_and_position(fault):
    write, name, where = FAULTS[fault]
    with footprint():
        bufs = _buffers()
        _exact(*bufs)
        write(*bufs)
    got = footprint_violations()
    assert len(got) == 1 and got[0][0].startswith(name) and got[0][1] == where, got


def test_the_patch_of_the_workspace_allocator_ends_with_the_case():
    from uda_clr_amd.kernels import HipKernels
    before = HipKernels.__dict__["_ws"]
    with footprint():
        assert HipKernels.__dict__["_ws"] is not before
    assert HipKernels.__dict__["_ws"] is before
    wrapped = kc.footprinted(lambda dev: len(kc._FRAMES))
    to_dev(padded(P, C, gen(1)), CPU)
    assert wrapped(CPU) == 0                 # a case begins with a cleared registry


def test_known_limit_identical_bits_are_invisible_two_consecutive_rows_are_not():
    """the by-row poison is NaN, +Inf, -Inf, 3e38: a NaN with the poison's bits onto a NaN guard row changes nothing; the same
    value onto that row and the next one is seen on the second"""
    with footprint():
        out = to_dev(padded(P, C, gen(2)), CPU, name="out")
        assert (P + GUARD_ROWS) % 4 == 2 and GUARD_ROWS % 4 == 0
        guard = _rows(out, P + 2, 2)                                     # rows P + 2 (NaN) and P + 3 (+Inf)
        assert torch.isnan(guard[0]).all() and torch.isinf(guard[1]).all()
        guard[0].copy_(guard[0].clone())
        assert footprint_violations() == []
        guard[1].copy_(guard[0].clone())
    assert footprint_violations() == [("out", (P + 3, 0))]


def test_window_bookkeeping_of_the_window_cases():
    """only_writes: one column window of a wide matrix and one slice of a shared fp64 arena may change; the neighbouring column,
    the neighbouring accumulator and a coefficient window's neighbour may not"""
    with footprint():
        g = gen(3)
        wide = to_dev(padded(P, 24, g), CPU, name="cat")
        arena = out_dev((3 * 16 * 2 * 8,), torch.float64, CPU, fill=0, name="arena")
        coef = out_dev((4, 24), torch.float32, CPU, fill=0, name="coef")
        slots = [arena[i * 256:(i + 1) * 256].view(16, 2, 8) for i in range(3)]
        sl = slice(8, 16)
        wins = (wide[:, sl], slots[1]) + tuple(coef[q][sl] for q in range(4))
        only_writes(*wins)
        for v in wins:
            v.fill_(5.0)
        assert footprint_violations() == []
        only_writes(*wins)
        wide[2, 16] = 1.1                   # (1.1: no zero byte, so the first changed byte is the element's first)
        slots[2][0, 0, 0] = 1.1
        coef[1][7] = 1.1
        assert footprint_violations() == [("cat", (2, 16)), ("arena", 2 * 256 * 8), ("coef", (24 + 7) * 4)]
        only_writes(*wins)
        slots[0][15, 1, 7] = 1.1            # the last double before the window
        assert footprint_violations() == [("arena", 255 * 8)]
        read_only(wide)
        wide[0, 8] = 2.0
    assert ("cat", (0, 8)) in footprint_violations()


# ---- a correct implementation passes: the cases whose calls SpecKernels offers unchanged, on the CPU
_SPEC_CASES = [c for c in kc.CASES if c[0].startswith(("bn C=", "bn eval", "bn frozen", "upsample 4x4", "upsample 8x6", "upsample + stats 5x7",
                                                       "head 12x10", "gap C=256", "bn backward, low-rank dU: C=40"))]
_SPEC_CASES += [c for c in kc.WINDOW_CASES if c[0].startswith("coefficient window")]


@pytest.mark.parametrize("name,fn", _SPEC_CASES, ids=[c[0] for c in _SPEC_CASES])
def test_spec_kernels_pass_the_harness_on_the_cpu(name, fn, monkeypatch):
    assert len(_SPEC_CASES) >= 10
    monkeypatch.setattr(kc, "_HIP", kc.SPEC)
    err, tol = fn(CPU)
    assert err <= tol                       # (the spec against itself)
    assert len(kc._FRAMES) > 0 and footprint_violations() == []


# ---- the guards around the engine's work buffers and statistics arenas (tests/engine_guards.py)
def test_guarded_engine_run_with_spec_kernels_keeps_every_guard_and_a_stray_write_is_reported(monkeypatch):
    import engine_guards
    import model_cases
    from uda_clr_amd import engine
    monkeypatch.setattr(engine, "POISON_BUFFERS", True)
    keep = engine.GeneratorEngine.__dict__["_empty"], engine._Arena
    with engine_guards.guarded() as guards:
        fwd, grads, stats, _ = model_cases.train_parity(CPU, S=64, engine=engine.GeneratorEngine(kc.SPEC))
    assert (engine.GeneratorEngine.__dict__["_empty"], engine._Arena) == keep
    assert guards.counts()[0] >= 100 and guards.counts()[1] >= 2, guards.counts()
    assert guards.violations() == []
    assert max(fwd.values()) < 1e-3 and stats < 1e-3
    # one float into row P of a work matrix, one double behind an arena
    name, base, _ = next(h for h in guards.held if h[1].dim() == 2 and h[1].dtype == torch.float32)
    base[base.shape[0] - GUARD_ROWS, 0] = 1.5
    aname, big, g2 = next(h for h in guards.held if h[0].startswith("statistics arena"))
    g2[1][0][0] = 1.5
    assert sorted(guards.violations()) == sorted([(name, "behind", 0), (aname, "behind", 0)])


# ---- the one entry that writes the lanes [C, round4(C)) by design (uda_dropout_mask: 4-byte words): engine.py never hands it a
# window with live bytes beside it
def test_the_engine_draws_every_dropout_mask_into_a_matrix_of_its_own():
    import model_cases
    from uda_clr_amd.engine import GeneratorEngine

    seen = []

    class Recording(type(kc.SPEC)):
        def dropout_mask(self, mask, p, seed, offset):
            seen.append((mask.storage_offset(), mask.stride(0), mask.shape, mask.untyped_storage().nbytes()))
            return super().dropout_mask(mask, p, seed, offset)

    m = model_cases.seeded_model(perturb=True).train()
    m._engine_override = GeneratorEngine(Recording())
    x = torch.randn(2, 3, 64, 64, generator=gen(0))
    m(x)                                        # training forward, masks drawn by the engine: aspp + three decoder dropouts
    assert len(seen) == 4, seen
    for off, ld, (P_, C_), nbytes in seen:
        assert off == 0 and ld == round4(C_) and nbytes == P_ * round4(C_), (off, ld, P_, C_, nbytes)
