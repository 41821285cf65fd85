"""No GPU: the masks of tests/postproc_shapes.py have the properties tests/test_postproc_gpu.py relies on, by the scipy oracle
and the numpy model of the tile launches alone.  If a builder stops giving its property, change the builder, not the assertion."""
import numpy as np
import pytest
from scipy import ndimage

import postproc_shapes as ps

THR = 0.75


def _stages(prob):
    return ps.stages(prob, THR, THR)


def _count(mask, structure):
    return ndimage.label(mask, structure=structure)[1]


def _first_pixel(mask):
    return int(np.flatnonzero(np.asarray(mask).ravel())[0])


def _areas_by_first_pixel(eroded):
    """[(area, raster index of the first pixel)] of the 8-connected components, in raster order of their first pixel"""
    lab, n = ndimage.label(eroded, structure=ps.FULL)
    return [(int((lab == i).sum()), _first_pixel(lab == i)) for i in range(1, n + 1)]


def test_builders_give_two_different_channels_of_two_values():
    for name, prob in ps.library():
        assert prob.dtype == np.float32 and prob.ndim == 3 and prob.shape[0] == 2, name
        assert set(np.unique(prob).tolist()) <= {float(ps.IN), float(ps.OUT)}, name
        assert ps.OUT < THR < ps.IN
        if not (name.startswith("ones") or name.startswith("zeros")):
            assert not np.array_equal(prob[0], prob[1]), name


def test_model_fixed_point_is_scipys_labelling_and_fill():
    """the launch model run to its fixed point IS connected-component labelling by the first pixel's index, and the border flood"""
    for prob in (ps.diagonal_ring(), ps.nested("blob_in_ring"), ps.tie("third_first")):
        st = _stages(prob)
        for c in range(2):
            e, k, f = st["eroded"][c], st["keep"][c], st["filled"][c]
            lab = ps.propagate(ps.label_init(e), True, ps.launches_needed(ps.label_init(e), True))
            ref, n = ndimage.label(e, structure=ps.FULL)
            want = np.zeros(e.shape, np.int64)
            for i in range(1, n + 1):
                want[ref == i] = _first_pixel(ref == i) + 1
            assert np.array_equal(lab, want)
            fl = ps.propagate(ps.flood_init(k), False, ps.launches_needed(ps.flood_init(k), False))
            assert np.array_equal((k > 0) | (fl == 2), f > 0)


def test_model_moves_a_label_one_tile_per_launch():
    """a 1-pixel line along a row of 4 tiles: launch j fills tile j - 1 with the first pixel's label (the halo is the snapshot, so
    tile j sees it one launch later): 4 launches change something, and after one launch the label has not left its tile"""
    m = np.zeros((8, 4 * ps.TILE), np.uint8)
    m[3, :] = 1
    lab = ps.label_init(m)
    assert ps.launches_needed(lab, True) == 4 and ps.launches_needed(lab, False) == 4
    one = ps.propagate(lab, True, 1)
    first = int(lab[3, 0])
    assert (one[3, :ps.TILE] == first).all() and (one[3, ps.TILE:2 * ps.TILE] == lab[3, ps.TILE - 1]).all()
    assert (ps.propagate(lab, True, 4)[3] == first).all()


def test_spiral_256_needs_the_retry_path_and_more_than_six_doublings_from_one():
    st = _stages(ps.spiral(256, 20, 18))
    for c in range(2):
        e, k = st["eroded"][c], st["keep"][c]
        assert _count(e, ps.FULL) == 1 and e.sum() > 10000 and np.array_equal(e, k)
        need = ps.launches_needed(ps.label_init(e), True)
        flood = ps.launches_needed(ps.flood_init(k), False)
        print("spiral 256 channel %d: %d pixels, labels need %d launches, flood %d, default %d" % (c, int(e.sum()), need, flood,
                                                                                                   ps.default_sweeps(256, 256)))
        assert need > ps.default_sweeps(256, 256) and need > 32          # 1, 2, 4, 8, 16, 32: six attempts from sweeps = 1 all fail
        assert need <= 2 * ps.default_sweeps(256, 256) and flood <= 2 * ps.default_sweeps(256, 256)   # the second default attempt ends it
    assert np.array_equal(st["eroded"][1], st["eroded"][0].T)


def test_spiral_192_converges_within_the_doublings_from_one_but_not_at_once():
    st = _stages(ps.spiral(192, 20, 18))
    for c in range(2):
        e, k = st["eroded"][c], st["keep"][c]
        assert _count(e, ps.FULL) == 1
        need = max(ps.launches_needed(ps.label_init(e), True), ps.launches_needed(ps.flood_init(k), False))
        print("spiral 192 channel %d: needs %d launches, default %d" % (c, need, ps.default_sweeps(192, 192)))
        assert 16 < need <= 32                                             # fails at 1 .. 16, passes at 32
        assert need > ps.default_sweeps(192, 192)


def test_diagonal_ring_separates_the_two_connectivities():
    st = _stages(ps.diagonal_ring())
    for c in range(2):
        e, k, f = st["eroded"][c], st["keep"][c], st["filled"][c]
        assert _count(e, ps.FULL) == 1 and _count(e, ps.CROSS) > 1
        assert _count(1 - k, ps.CROSS) == 2 and _count(1 - k, ps.FULL) == 1
        assert int(f.sum()) > int(k.sum()) + 2000 and int(k.sum()) == 2800
        # labels by the 4-neighbourhood would keep one of the pieces only; a flood by the 8-neighbourhood would fill nothing
        lab4, _ = ndimage.label(e, structure=ps.CROSS)
        assert np.bincount(lab4.ravel())[1:].max() < int(k.sum()) // 2
    assert np.array_equal(st["filled"][1][:-2, 2:], st["filled"][0][2:, :-2]) and not np.array_equal(st["filled"][1], st["filled"][0])
    pad = _stages(ps.diagonal_ring(pad_to=256))
    assert np.array_equal(pad["filled"][:, :136, :136], st["filled"]) and int(pad["filled"].sum()) == int(st["filled"].sum())


def test_tie_keeps_the_first_of_two_equal_components():
    for order in ("equal", "third_first"):
        st = _stages(ps.tie(order))
        for c in range(2):
            comps = _areas_by_first_pixel(st["eroded"][c])
            big = max(a for a, _ in comps)
            firsts = [p for a, p in comps if a == big]
            assert len(firsts) == 2, comps
            if order == "third_first":
                assert len(comps) == 3 and comps[0][0] < big                # the component numbered 1 is not the answer
            assert _first_pixel(st["keep"][c]) == min(firsts) and int(st["keep"][c].sum()) == big
            assert np.array_equal(st["keep"][c], st["filled"][c])


def test_tie_keeps_the_later_component_when_it_is_larger():
    st = _stages(ps.tie("later_larger"))
    for c in range(2):
        comps = _areas_by_first_pixel(st["eroded"][c])
        assert len(comps) == 2 and comps[1][0] > comps[0][0]
        assert _first_pixel(st["keep"][c]) == comps[1][1] and int(st["keep"][c].sum()) == comps[1][0]


def test_nested_shapes():
    st = _stages(ps.nested("blob_in_ring"))
    for c in range(2):
        e, k, f = st["eroded"][c], st["keep"][c], st["filled"][c]
        assert _count(e, ps.FULL) == 2 and int(k.sum()) < int(e.sum())      # the blob survives the erosion and is dropped
        assert _count(f, ps.CROSS) == 1 and _count(1 - f, ps.FULL) == 1     # one solid piece, no hole left
        assert ((e > 0) <= (f > 0)).all() and int(f.sum()) > 3 * int(k.sum())
    st = _stages(ps.nested("open_ring"))
    for c in range(2):
        k, f = st["keep"][c], st["filled"][c]
        assert int(k.sum()) > 1000 and np.array_equal(k, f)                  # the corridor survives: the fill gains no pixel
        assert _count(1 - k, ps.CROSS) == 1
    st = _stages(ps.nested("four_borders"))
    for c in range(2):
        e, k, f = st["eroded"][c], st["keep"][c], st["filled"][c]
        assert _count(e, ps.FULL) == 1
        assert k[0].any() and k[-1].any() and k[:, 0].any() and k[:, -1].any()
        assert _count(1 - k, ps.CROSS) >= 6 and _count(1 - k, ps.CROSS) - _count(1 - f, ps.CROSS) == 1     # only the inner pocket is a hole
        up = (lambda r: r) if c == 0 else (lambda r: 95 - r)
        assert not k[up(50), 62] and f[up(50), 62] and int(f.sum()) > int(k.sum()) + 500
        for r, x in ((0, 52), (46, 0), (95, 72), (36, 119), (95, 0)):                                       # the border pockets stay
            assert not f[up(r), x], (r, x)


@pytest.mark.parametrize("H,W", ps.SMALL_ONES)
def test_planes_smaller_than_the_windows_come_out_empty(H, W):
    st = _stages(ps.ones(H, W))
    assert not st["eroded"].any() and not st["filled"].any()


@pytest.mark.parametrize("H,W", ps.LARGE_ONES)
def test_full_planes_lose_their_corners_only(H, W):
    f = _stages(ps.ones(H, W))["filled"]
    for c in range(2):
        assert 0.5 * H * W < int(f[c].sum()) < H * W and _count(f[c], ps.CROSS) == 1
        assert not f[c][0, 0] and not f[c][-1, -1] and not f[c][0, -1] and not f[c][-1, 0] and f[c][H // 2, 8:-8].all()


def test_empty_and_single_blob_planes():
    assert not _stages(ps.zeros(64, 48))["filled"].any()
    st = _stages(ps.blob_33x17())
    for c in range(2):
        assert st["filled"][c].shape == (33, 17) and _count(st["eroded"][c], ps.FULL) == 1 and int(st["filled"][c].sum()) >= 40
    assert not np.array_equal(st["filled"][0], st["filled"][1])


def test_kernel_cases_oracle_is_the_last_stage():
    from kernel_cases import _scipy_postprocess
    prob = ps.nested("blob_in_ring")
    assert np.array_equal(_scipy_postprocess(prob, THR, THR), _stages(prob)["filled"])
    assert np.array_equal(_scipy_postprocess(prob, 0.1, 0.5), ps.stages(prob, 0.1, 0.5)["filled"])
