"""numpy / scipy statement of the prediction pictures (csrc/overlay.hip, uda_display_masks in csrc/postproc.hip): the display mask,
the contour vertices, the painting and the byte image of the reference's ``save_per_img`` (utils/Utils.py:515-585), and the masks the
tests feed them.  Channel 0 = cup, 1 = disc.

Display mask of one [H, W] probability plane: outermost ring read as 0 -> > threshold -> the evaluation chain of
tests/postproc_shapes.py (5 x medfilt2d(7), erosion by DIAMOND with the outside set, largest 8-connected component, fill) ->
binary_dilation(DIAMOND), outside unset -> largest component and fill once more.

Outline: the vertices of skimage.measure.find_contours(M, 0.5) on a {0,1} mask are the midpoints of all 4-adjacent in-image pixel
pairs with different values; each vertex (y, x) paints the seven pixels (int(y + dy), int(x + dx)) for (dy, dx) in OFFSETS, int()
truncating towards zero.  The one departure from the reference: a target whose row or column lies outside the image before any
wrapping (index -1, H or W) is dropped, where the reference wraps -1 to the far border and raises IndexError at H or W."""
import numpy as np
from scipy import ndimage

import postproc_shapes as shapes

OFFSETS = ((0, 0), (1, 0), (1, 1), (0, 1), (-1, 0), (-1, -1), (0, -1))       # utils/Utils.py:565-571, in its order
GREEN, BLUE = (0, 255, 0), (0, 0, 255)                                    # channel 1 first, then channel 0 over it


# --------------------------------------------------------------------------------------------------------------- display mask
def ring_zeroed(plane):
    """a copy of the plane with its outermost rows and columns set to 0 (the input is left alone)"""
    p = np.array(plane, copy=True)
    p[0, :] = p[-1, :] = 0
    p[:, 0] = p[:, -1] = 0
    return p


def largest_component(m):
    """first maximum of the areas, components numbered in raster order of their first pixel (what skimage's label + regionprops give)"""
    m = np.asarray(m).astype(np.uint8).copy()
    lab, n = ndimage.label(m, structure=shapes.FULL)
    if n:
        areas = np.bincount(lab.ravel())[1:]
        m[lab != int(np.argmax(areas)) + 1] = 0
    return m


def fill(m):
    return ndimage.binary_fill_holes(np.asarray(m).astype(int)).astype(np.uint8)


def display_stages(prob, threshold=0.75):
    """prob [2,H,W] -> {'filled', 'dilated', 'second_keep', 'display'}: uint8 [2,H,W] after step 5, 6, the component half of 7, and 7"""
    prob = np.asarray(prob, np.float32)
    zeroed = np.stack([ring_zeroed(prob[0]), ring_zeroed(prob[1])])
    out = {"filled": shapes.stages(zeroed, threshold, threshold)["filled"]}
    out["dilated"] = np.stack([ndimage.binary_dilation(m, structure=shapes.DIAMOND, border_value=0) for m in out["filled"]]).astype(np.uint8)
    out["second_keep"] = np.stack([largest_component(m) for m in out["dilated"]])
    out["display"] = np.stack([fill(m) for m in out["second_keep"]])
    return out


def display_masks(prob, threshold=0.75):
    """prob [B,2,H,W] or [2,H,W] -> uint8 display masks of the same shape"""
    prob = np.asarray(prob)
    if prob.ndim == 3:
        return display_stages(prob, threshold)["display"]
    return np.stack([display_stages(p, threshold)["display"] for p in prob])


# -------------------------------------------------------------------------------------------------------------------- outline
def vertices(mask):
    """float64 [n, 2] (row, column): midpoints of the 4-adjacent pixel pairs of ``mask`` that differ, down pairs then right pairs"""
    m = np.asarray(mask) != 0
    r, c = np.nonzero(m[:-1, :] != m[1:, :])
    down = np.stack([r + 0.5, c.astype(np.float64)], 1)
    r, c = np.nonzero(m[:, :-1] != m[:, 1:])
    right = np.stack([r.astype(np.float64), c + 0.5], 1)
    return np.concatenate([down, right]).reshape(-1, 2)


def targets(verts):
    """int64 [n, 7, 2]: the pixels each vertex paints before any range check, int() as numpy's astype(int) (towards zero)"""
    v = np.asarray(verts, np.float64).reshape(-1, 1, 2)
    return (v + np.asarray(OFFSETS, np.float64)[None]).astype(int)


def paint(image, mask, colour):
    """``image`` uint8 [H,W,3] painted IN PLACE with the outline of ``mask``; returns the dropped targets, int64 [k, 2]"""
    H, W = image.shape[:2]
    t = targets(vertices(mask)).reshape(-1, 2)
    ok = (t[:, 0] >= 0) & (t[:, 0] < H) & (t[:, 1] >= 0) & (t[:, 1] < W)
    image[t[ok, 0], t[ok, 1], :] = colour
    return t[~ok]


def overlay(image, masks):
    """image uint8 [H,W,3], masks [2,H,W] -> a new uint8 [H,W,3]: channel 1 in GREEN, then channel 0 in BLUE over it"""
    out = np.array(image, dtype=np.uint8, copy=True)
    paint(out, masks[1], GREEN)
    paint(out, masks[0], BLUE)
    return out


def overlay_batch(images, masks):
    return np.stack([overlay(i, m) for i, m in zip(images, masks)])


# ------------------------------------------------------------------------------------------------------------------ image bytes
def image_u8(x):
    """float [B,3,H,W] in [-1, 1] -> uint8 [B,H,W,3] = clip(rint((x + 1) * 127.5), 0, 255), every step rounded to fp32"""
    x = np.asarray(x, np.float32)
    v = np.rint((x + np.float32(1.0)) * np.float32(127.5))
    return np.clip(v, 0, 255).astype(np.uint8).transpose(0, 2, 3, 1)


def normalized_levels():
    """what Normalize_tf makes of the 256 grey levels (v / 127.5 - 1 in fp32, custom_transforms.py:432-466)"""
    return np.arange(256, dtype=np.float32) / np.float32(127.5) - np.float32(1.0)


def grey_mask(pred):
    """BEAL grey coding of evaluation masks [..., 2, H, W]: 0 = cup, 128 = disc only, 255 = background"""
    pred = np.asarray(pred) != 0
    cup, disc = pred[..., 0, :, :], pred[..., 1, :, :]
    return np.where(cup, 0, np.where(disc, 128, 255)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------- test masks
def tip_bay():
    """96 x 96: a 76 x 76 square with a diamond-shaped hole of radius 12 whose tip points at the top side through a 9 px wall.  The
    erosion removes the wall where it is thinnest, so the hole becomes a bay with a mouth a few pixels wide and the first fill leaves
    it alone; the dilation closes the mouth (diamonds from both sides of the tip overlap) and shrinks the bay back to a hole, which
    only the SECOND fill fills.  None of tests/postproc_shapes.py's shapes does that: the diagonal ring's hole is 4-separated from
    the outside already and the first fill takes it.  Channel 1 is the transpose (the tip points at the left side)."""
    yy, xx = np.mgrid[0:96, 0:96]
    m = np.zeros((96, 96), bool)
    m[10:86, 10:86] = True
    m &= ~((np.abs(yy - 31) + np.abs(xx - 48)) <= 12)
    return shapes._prob(m, m.T)


def library():
    """tests/postproc_shapes.py's shapes and the one above: every shape the display masks are compared on"""
    return shapes.library() + [("tip bay", tip_bay())]


def shifted(prob, where):
    """the two planes of a library shape moved so that its set pixels touch 'top', 'bottom', 'left', 'right' or the 'corner'
    (top-left); what moves out is lost, what moves in is OUT"""
    prob = np.asarray(prob)
    out = np.full_like(prob, shapes.OUT)
    for c in range(2):
        rows, cols = np.nonzero(prob[c] > 0.5)
        if rows.size == 0:
            continue
        H, W = prob[c].shape
        dy = {"top": -rows.min(), "bottom": H - 1 - rows.max(), "corner": -rows.min()}.get(where, 0)
        dx = {"left": -cols.min(), "right": W - 1 - cols.max(), "corner": -cols.min()}.get(where, 0)
        src = prob[c]
        out[c, max(dy, 0):H + min(dy, 0), max(dx, 0):W + min(dx, 0)] = src[max(-dy, 0):H + min(-dy, 0), max(-dx, 0):W + min(-dx, 0)]
    return out


def random_image(B, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def hand_masks():
    """[(name, masks uint8 [2,H,W])]: the hand-made masks of the overlay tests"""
    out = []

    def two(H, W):
        return np.zeros((2, H, W), np.uint8)
    m = two(9, 11)
    m[0, 4, 5] = 1
    out.append(("single pixel", m))
    for name, (r, c) in (("top-left", (0, 0)), ("top-right", (0, 10)), ("bottom-left", (8, 0)), ("bottom-right", (8, 10))):
        m = two(9, 11)
        m[0, r, c] = 1
        m[1, 8 - r, 10 - c] = 1
        out.append(("corner pixel " + name, m))
    out.append(("full planes", np.ones((2, 12, 7), np.uint8)))
    m = two(12, 7)
    m[1] = 1
    out.append(("full disc, empty cup", m))
    for H, W in ((1, 40), (40, 1), (1, 1), (2, 2)):
        m = two(H, W)
        m[0].reshape(-1)[::3] = 1
        m[1].reshape(-1)[1::5] = 255                      # nonzero means set
        out.append(("%dx%d" % (H, W), m))
    m = two(40, 40)
    m[0, 10:25, 10:25] = 1
    m[1, 10:30, 8:25] = 1                                 # shares the top edge and the right edge with channel 0: blue wins there
    out.append(("overlapping outlines", m))
    yy, xx = np.mgrid[0:37, 0:45]
    out.append(("checkerboard", np.stack([(yy + xx) % 2, (yy + xx + 1) % 2]).astype(np.uint8)))
    for H, W in ((33, 17), (48, 80), (70, 130)):          # outlines across the 32 x 32 tile edges, along them and through their corners
        m = two(H, W)
        m[0, 3:H - 2, 5:W - 3] = 1
        m[0, 31:33, :] ^= 1                               # a band on the first tile edge, out to both borders
        if W > 33:
            m[0, :, 31:33] ^= 1
        m[1] = shapes.disc(H, W, H / 2.0, W / 2.0, min(H, W) / 2.0 + 3)      # touches all four borders
        m[1, 32:, 32:] ^= (np.indices((H - 32, W - 32)).sum(0) % 7 == 0).astype(np.uint8) if H > 32 and W > 32 else 0
        out.append(("tile edges %dx%d" % (H, W), m))
    return out
