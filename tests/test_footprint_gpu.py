"""-m gpu: the column-window cases of tests/kernel_cases.py (WINDOW_CASES) in both MFMA modes.  Each case runs the producers of one
wide buffer in engine.py's order and asserts after every call that the window equals the statement and that nothing else changed:
the other columns, the padding lanes, the guard rows, the neighbouring accumulators of the shared fp64 arena and every operand."""
import pytest
import torch

import kernel_cases
from kernel_cases import WINDOW_CASES, footprint_violations

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("name,fn", WINDOW_CASES, ids=[c[0] for c in WINDOW_CASES])
def test_window_producers_write_their_window_only(name, fn, mode):
    K = kernel_cases.hip()
    keep = K.mfma
    K.mfma = K.MFMA_BF16X3 if mode == "bf16x3" else K.MFMA_F32
    try:
        err, tol = fn(torch.device("cuda:0"))          # (the case asserts the footprint after every call)
        torch.cuda.synchronize()
    finally:
        K.mfma = keep
    assert err <= tol, "%s (%s): rel err %.3e > %.1e" % (name, mode, err, tol)
    assert footprint_violations() == [], "%s (%s) wrote outside its window: (buffer, first position)" % (name, mode)


def test_the_harness_sees_stray_writes_on_the_device():
    """the bookkeeping itself on device memory (tests/test_footprint_cpu.py proves it on the CPU): plain torch writes into a padding
    lane, the first guard row, the byte behind a flat output and a read-only operand, all inside memory the test owns"""
    from kernel_cases import footprint, gen, out_dev, padded, ro_dev, to_dev
    dev = torch.device("cuda:0")
    with footprint():
        out = to_dev(padded(6, 5, gen(0)), dev, name="out")
        st = out_dev((16, 2, 5), torch.float64, dev, fill=0, name="stats")
        w = ro_dev(torch.randn(7, generator=gen(1)), dev, name="weight")
        out.fill_(1.0)
        st.fill_(2.0)
        assert footprint_violations() == []
        out.as_strided((1, 1), (12, 1), out.storage_offset() + 5).fill_(1.0)                 # row 0, lane C
        out.as_strided((1, 1), (12, 1), out.storage_offset() + 6 * 12 + 3).fill_(1.0)        # row P, column 3
        st.view(-1).as_strided((1,), (1,), st.storage_offset() + 160).fill_(1.0)             # channel C of the last slot
        w[2:3].add_(1.0)
        torch.cuda.synchronize()
    assert footprint_violations() == [("out", (0, 5)), ("stats", 160 * 8), ("weight", 8)]
