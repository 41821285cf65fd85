"""scipy oracle of the evaluation post-processing (csrc/postproc.hip), stage by stage, the masks the tests feed it, and a numpy
model of the tile-wise propagation that says how many launches a mask needs.

The chain per channel (utils/Utils.py:427-463 of the reference, skimage's two calls replaced by their scipy.ndimage equivalents):
threshold -> 5 x medfilt2d(7) -> binary_erosion(diamond(7), outside set) -> largest 8-connected component (first maximum of the
areas, components numbered in raster order of their first pixel) -> binary_fill_holes (4-connected background).

Every builder returns float32 [2, H, W] probabilities, IN = 0.9 inside the shape and OUT = 0.05 outside, so any threshold between
them (the tests use 0.75) reproduces the mask.  The two channels hold different shapes (or one shape mirrored, transposed or
moved), so a channel mix-up shows; only the all-set and all-unset planes are the same in both."""
import numpy as np
import scipy.signal
from scipy import ndimage

IN, OUT = np.float32(0.9), np.float32(0.05)
TILE = 32                                    # PP_T of csrc/postproc.hip
FULL = np.ones((3, 3), bool)                 # 8-neighbourhood
CROSS = ndimage.generate_binary_structure(2, 1)
_yy, _xx = np.mgrid[-7:8, -7:8]
DIAMOND = (np.abs(_yy) + np.abs(_xx)) <= 7


# --------------------------------------------------------------------------------------------------------------- the oracle
def stages(prob, thr_cup, thr_disc):
    """prob [2,H,W] -> {'eroded', 'keep', 'filled'}: uint8 [2,H,W] after the erosion, after the largest component, after the fill"""
    prob = np.asarray(prob)
    out = {k: np.zeros(prob.shape, np.uint8) for k in ("eroded", "keep", "filled")}
    for c, thr in ((0, thr_cup), (1, thr_disc)):
        m = (prob[c] > thr).astype(np.uint8)
        for _ in range(5):
            m = scipy.signal.medfilt2d(m, 7)
        m = ndimage.binary_erosion(m, structure=DIAMOND, border_value=1).astype(np.uint8)
        out["eroded"][c] = m
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        if n:
            areas = np.bincount(lab.ravel())[1:]
            m[lab != int(np.argmax(areas)) + 1] = 0
        out["keep"][c] = m
        out["filled"][c] = ndimage.binary_fill_holes(m.astype(int)).astype(np.uint8)
    return out


def default_sweeps(H, W):
    """the launch count HipKernels.postprocess starts with"""
    return 2 * ((H + TILE - 1) // TILE + (W + TILE - 1) // TILE) + 4


# ------------------------------------------------------------------------------------------- model of pp_propagate_kernel
def label_init(eroded):
    """what pp_label_init_kernel writes: raster index + 1 on set pixels, 0 elsewhere"""
    m = np.asarray(eroded) > 0
    return np.where(m, np.arange(m.size, dtype=np.int64).reshape(m.shape) + 1, 0)


def flood_init(keep):
    """what pp_keep_kernel writes for the border flood: 0 = kept, 1 = background on the image border, 2 = other background"""
    k = np.asarray(keep) > 0
    edge = np.ones(k.shape, bool)
    edge[1:-1, 1:-1] = False
    return np.where(k, 0, np.where(edge, 1, 2)).astype(np.int64)


def _launch(lab, conn8):
    """one launch: every TILE x TILE tile goes to the fixed point of "minimum positive label over the neighbourhood", neighbours
    inside the tile live, neighbours outside it from the snapshot `lab`.  The fixed point does not depend on the update order:
    each 4-/8-connected piece of the tile's positive pixels ends at the minimum over its own labels and the positive snapshot
    labels of the halo pixels that touch it."""
    H, W = lab.shape
    big = np.iinfo(np.int64).max
    snap = np.zeros((H + 2, W + 2), np.int64)
    snap[1:-1, 1:-1] = lab
    out = lab.copy()
    offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and (conn8 or not (dy and dx))]
    for h0 in range(0, H, TILE):
        for w0 in range(0, W, TILE):
            th, tw = min(TILE, H - h0), min(TILE, W - w0)
            t = lab[h0:h0 + th, w0:w0 + tw]
            if not t.any():
                continue
            halo = snap[h0:h0 + th + 2, w0:w0 + tw + 2].copy()
            halo[1:-1, 1:-1] = 0
            halo[halo == 0] = big
            m0 = np.where(t > 0, t, big)
            for dy, dx in offs:
                m0 = np.minimum(m0, halo[1 + dy:1 + dy + th, 1 + dx:1 + dx + tw])
            comp, n = ndimage.label(t > 0, structure=FULL if conn8 else CROSS)
            mins = ndimage.minimum(m0, comp, index=np.arange(1, n + 1))
            out[h0:h0 + th, w0:w0 + tw] = np.where(t > 0, np.asarray(mins, np.int64)[np.maximum(comp, 1) - 1], 0)
    return out


def launches_needed(labels, conn8):
    """number of launches that still change a label; the next one changes nothing.  uda_postprocess(sweeps = n) reports
    not_converged = 0 for this propagation exactly when n >= this number."""
    lab = np.asarray(labels, np.int64)
    n = 0
    while True:
        nxt = _launch(lab, conn8)
        if np.array_equal(nxt, lab):
            return n
        lab, n = nxt, n + 1


def propagate(labels, conn8, launches):
    """the labels after `launches` launches (for tests of the model itself)"""
    lab = np.asarray(labels, np.int64)
    for _ in range(launches):
        lab = _launch(lab, conn8)
    return lab


# ----------------------------------------------------------------------------------------------------------------- builders
def _prob(*masks):
    return np.stack([np.where(m, IN, OUT) for m in masks]).astype(np.float32)


def disc(H, W, cy, cx, r):
    yy, xx = np.mgrid[0:H, 0:W]
    return (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r


def spiral_mask(S, t, c):
    """rectangular spiral wall of thickness t around a corridor of width c on S x S.  Turn k is a ring inset by 8 + k * (t + c)
    whose left side stops t + c below its top side (the corridor's mouth); a bar of thickness t joins that end to the top side
    of turn k + 1.  The wall's first pixel in raster order is its outer end, so the minimum label travels its whole length."""
    m = np.zeros((S, S), bool)
    p = t + c
    a, b = 8, S - 8
    while b - a >= 2 * t + c:
        m[a:a + t, a:b] = True                  # top
        m[a:b, b - t:b] = True                  # right
        m[b - t:b, a:b] = True                  # bottom
        m[a + p:b, a:a + t] = True              # left, open at the top
        if (b - p) - (a + p) >= 2 * t + c:
            m[a + p:a + p + t, a:a + p] = True  # bar to the next turn
        a, b = a + p, b - p
    return m


def spiral(S, t, c):
    m = spiral_mask(S, t, c)
    return _prob(m, m.T)


def diagonal_ring_mask():
    """four 40 x 40 squares on 136 x 136, neighbours sharing a 2 x 2 corner: after the erosion one 8-connected component made of
    4-connected pieces, around a hole that is 4-separated from the outside but 8-connected to it"""
    m = np.zeros((136, 136), bool)
    for r0, c0 in ((10, 48), (48, 86), (86, 48), (48, 10)):
        m[r0:r0 + 40, c0:c0 + 40] = True
    return m


def diagonal_ring(pad_to=None):
    """the ring is its own mirror image and its own transpose, so channel 1 holds it moved by (-2, +2): other tile offsets, the same
    counts.  pad_to embeds both channels in the top-left corner of a larger square plane."""
    m = diagonal_ring_mask()
    m2 = np.zeros_like(m)
    m2[:-2, 2:] = m[2:, :-2]
    if pad_to:
        big = np.zeros((2, pad_to, pad_to), bool)
        big[0, :136, :136], big[1, :136, :136] = m, m2
        m, m2 = big
    return _prob(m, m2)


TIE_ORDERS = ("equal", "third_first", "later_larger")


def tie(order="equal"):
    """two discs of radius 20 at (40, 30) and (80, 90) on 128 x 128: equal areas after the erosion, the earlier one is kept.
    'third_first' puts a smaller disc ahead of both in raster order (the first component is not the answer);
    'later_larger' gives the later disc radius 21 ("largest" and "first" disagree).  Channel 1 is the left-right mirror image."""
    assert order in TIE_ORDERS
    H = W = 128
    m = disc(H, W, 40, 30, 20) | disc(H, W, 80, 90, 21 if order == "later_larger" else 20)
    if order == "third_first":
        m |= disc(H, W, 18, 100, 14)
    return _prob(m, m[:, ::-1])


NESTED_KINDS = ("blob_in_ring", "open_ring", "four_borders")


def nested(kind="blob_in_ring"):
    """'blob_in_ring'  a ring of thickness 20 with a disc of radius 14 in its hole: the disc is a smaller component, removed
                       before the fill, so the whole interior is filled.  Channel 1: a square ring with an off-centre blob.
    'open_ring'     the same rings, their holes open to the outside through an 18 px corridor: the fill adds nothing.
    'four_borders'  the whole 96 x 120 plane except pockets on each border, one in a corner and one inside: the shape touches
                    all four borders, the border pockets stay, the inner one is filled.  Channel 1 is upside down."""
    assert kind in NESTED_KINDS
    if kind == "four_borders":
        m = np.ones((96, 120), bool)
        m[0:14, 40:64] = False                  # top (the erosion widens every pocket by 7: they stay 8 px apart)
        m[34:58, 0:14] = False                  # left
        m[82:96, 60:84] = False                 # bottom
        m[24:48, 106:120] = False               # right
        m[80:96, 0:16] = False                  # bottom-left corner
        m[40:60, 50:74] = False                 # inside
        return _prob(m, m[::-1])
    H = W = 128
    ring = disc(H, W, 64, 64, 54) & ~disc(H, W, 64, 64, 34)
    sq = np.zeros((H, W), bool)
    sq[12:116, 10:118] = True
    sq[32:96, 30:98] = False
    if kind == "blob_in_ring":
        return _prob(ring | disc(H, W, 64, 64, 14), sq | disc(H, W, 52, 76, 13))
    ring[55:73, 64:] = False                    # corridor to the right
    sq[:64, 52:70] = False                      # corridor to the top
    return _prob(ring, sq)


SMALL_ONES = ((15, 15), (5, 9), (1, 40))        # smaller than the diamond or the median window
LARGE_ONES = ((31, 33), (16, 200))              # one tile minus / plus one pixel; half a tile high and seven wide


def ones(H, W):
    return _prob(np.ones((H, W), bool), np.ones((H, W), bool))


def zeros(H, W):
    return _prob(np.zeros((H, W), bool), np.zeros((H, W), bool))


def blob_33x17():
    """33 x 17, one tile and one pixel high and narrower than one: a blob across the whole width (the erosion counts the outside
    as set, so it survives); channel 1 holds a different blob reaching the bottom border"""
    a, b = np.zeros((33, 17), bool), np.zeros((33, 17), bool)
    a[3:30, :] = True
    b[9:33, 0:16] = True
    return _prob(a, b)


def library():
    """[(name, prob [2,H,W])]: every shape the device is compared on"""
    out = [("spiral 256/20/18", spiral(256, 20, 18)), ("spiral 192/20/18", spiral(192, 20, 18)), ("diagonal ring", diagonal_ring())]
    out += [("tie " + o, tie(o)) for o in TIE_ORDERS]
    out += [("nested " + k, nested(k)) for k in NESTED_KINDS]
    out += [("ones %dx%d" % hw, ones(*hw)) for hw in LARGE_ONES + SMALL_ONES]
    out += [("zeros 64x48", zeros(64, 48)), ("blob 33x17", blob_33x17())]
    return out
