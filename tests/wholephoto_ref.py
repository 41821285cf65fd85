"""The numpy int64 restatement of the three entries of csrc/wholephoto.hip (include/uda_clr_hip.h: uda_photo_reduce_u8,
uda_roi_cut_u8, uda_roi_paste_u8) and of the closed forms of uda_clr_amd/wholephoto.py (``locate``'s centre, ``boxes``).  It is the
CPU stand-in for the HIP entries, in the role geometry_spec.py plays for uda_geometry_u8; every comparison against it is byte
equality.  The cut is geometry_spec.resize_bilinear on the zero-padded crop."""
import numpy as np

import geometry_spec as gs


def normalise(u8_hwc):
    """uint8 [..., H, W, 3] -> f32 [..., 3, H, W] = v * fl(1 / 127.5) - 1, each step rounded to fp32 (what torch's
    ``u8.float() / 127.5 - 1.0`` gives on the device: a division by a host scalar is a product with its rounded reciprocal)"""
    inv = np.float32(1.0) / np.float32(127.5)
    x = np.moveaxis(np.asarray(u8_hwc), -1, -3).astype(np.float32)
    return (x * inv).astype(np.float32) - np.float32(1.0)


def factor_of(H, W, S):
    return max(1, -(-max(H, W) // S))


def reduce_photo(img, S):
    """-> (canvas uint8 [S,S,3], f): block means by the integer factor f, (sum + cnt // 2) // cnt, partial edge blocks, zero fill"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    f = factor_of(H, W, S)
    h, w = -(-H // f), -(-W // f)
    canvas = np.zeros((S, S, 3), np.uint8)
    a = img.astype(np.int64)
    for r in range(h):
        for c in range(w):
            blk = a[r * f:min(H, (r + 1) * f), c * f:min(W, (c + 1) * f)]
            cnt = blk.shape[0] * blk.shape[1]
            canvas[r, c] = (blk.sum((0, 1)) + cnt // 2) // cnt
    return canvas, f


def reduce_batch(images, index, S):
    """-> canvas uint8 [B,S,S,3], factor int32 [B]; an index outside the list: zeros and factor 0"""
    out, fac = [], []
    for i in np.asarray(index).reshape(-1):
        if 0 <= int(i) < len(images):
            c, f = reduce_photo(images[int(i)], S)
        else:
            c, f = np.zeros((S, S, 3), np.uint8), 0
        out.append(c)
        fac.append(f)
    return np.stack(out), np.array(fac, np.int32)


def padded_crop(img, x0, y0, R):
    """the R x R window with top-left (x0, y0), 0 outside the photograph (what PIL's crop gives)"""
    img = np.asarray(img)
    H, W = img.shape[:2]
    out = np.zeros((R, R, 3), np.uint8)
    ya, yb, xa, xb = max(0, y0), min(H, y0 + R), max(0, x0), min(W, x0 + R)
    if yb > ya and xb > xa:
        out[ya - y0:yb - y0, xa - x0:xb - x0] = img[ya:yb, xa:xb]
    return out


def cut(img, box, S):
    """uint8 [S,S,3]: Pillow's crop(box).resize((S, S), BILINEAR)"""
    x0, y0, R = (int(v) for v in box)
    return gs.resize_bilinear(padded_crop(img, x0, y0, R), S, S)


def cut_batch(images, index, boxes, S):
    return np.stack([cut(images[int(i)], b, S) for i, b in zip(np.asarray(index).reshape(-1), np.asarray(boxes))])


def paste_axis(R, S):
    """per window position 0..R-1: (i0, i1, fa) with D = 2 R"""
    D = 2 * R
    a = np.clip((2 * np.arange(R, dtype=np.int64) + 1) * S - R, 0, (S - 1) * D)
    i0 = a // D
    return i0, np.minimum(i0 + 1, S - 1), a - i0 * D


def upsample_votes(plane, R):
    """int64 [R,R]: v = sum over the 2 x 2 neighbours of m * wy * wx for a 0/1 plane [S,S]; D^2 = 4 R^2 is the full weight"""
    m = (np.asarray(plane) != 0).astype(np.int64)
    S = m.shape[0]
    D = 2 * R
    i0, i1, f = paste_axis(R, S)
    wy0, wy1, wx0, wx1 = (D - f)[:, None], f[:, None], (D - f)[None, :], f[None, :]
    return (m[i0][:, i0] * wy0 * wx0 + m[i0][:, i1] * wy0 * wx1 + m[i1][:, i0] * wy1 * wx0 + m[i1][:, i1] * wy1 * wx1)


def paste(masks, box, H, W):
    """uint8 [H,W] grey mask (0 cup, 128 disc only, 255 elsewhere) of one [2,S,S] mask pair and its window"""
    x0, y0, R = (int(v) for v in box)
    D2 = 4 * R * R
    cup, disc = (2 * upsample_votes(masks[k], R) > D2 for k in (0, 1))
    win = np.where(cup, 0, np.where(disc, 128, 255)).astype(np.uint8)
    out = np.full((H, W), 255, np.uint8)
    ya, yb, xa, xb = max(0, y0), min(H, y0 + R), max(0, x0), min(W, x0 + R)
    if yb > ya and xb > xa:
        out[ya:yb, xa:xb] = win[ya - y0:yb - y0, xa - x0:xb - x0]
    return out


def centre(moments_disc, f, H, W):
    """(cy, cx, located) in photograph pixels from the disc plane's (n, sum r, sum c) on the canvas and the factor"""
    n, sr, sc = (int(v) for v in moments_disc[:3])
    if n == 0:
        return H // 2, W // 2, 0
    return f * (2 * sr + n) // (2 * n), f * (2 * sc + n) // (2 * n), 1


def box_axis(c, L, R):
    """first window position along one axis: centred on c, shifted into the photograph when it is at least R long, else the
    photograph centred in the window"""
    if L >= R:
        return min(max(c - R // 2, 0), L - R)
    return -((R - L) // 2)


def boxes(centres, sizes, R):
    """centres [B,2] = (cy, cx), sizes [B,2] = (H, W) -> int32 [B,3] = (x0, y0, R)"""
    return np.array([[box_axis(int(cx), int(W), R), box_axis(int(cy), int(H), R), R] for (cy, cx), (H, W) in zip(centres, sizes)], np.int32)


# ------------------------------------------------------------------------------------------------ the shapes and cases of the tests
S_TEST = 16
REDUCE_SHAPES = [(1, 1), (16, 16), (17, 23), (33, 64), (50, 7), (130, 9)]       # f = 1, 1, 2, 4, 4, 9
CUT_SHAPES = [(40, 52), (9, 9)]
PASTE_SHAPES = [(30, 44), (12, 12)]

# (what it is about, photograph, (x0, y0, R)) at S = 16
CUT_CASES = [
    ("R=16 pure copy", 0, (5, 7, 16)),
    ("R=40 the 2.5 bound", 0, (3, 0, 40)),
    ("R=25", 0, (10, 8, 25)),
    ("R=10 upsampling", 0, (20, 15, 10)),
    ("R=8 upsampling", 0, (30, 20, 8)),
    ("over the left side", 0, (-6, 10, 25)),
    ("over the top", 0, (10, -9, 25)),
    ("over the right side", 0, (40, 5, 25)),
    ("over the bottom", 0, (12, 30, 25)),
    ("over the top-left corner, copy", 0, (-5, -7, 16)),
    ("over the bottom-right corner, upsampling", 0, (45, 33, 10)),
    ("wholly outside", 0, (100, 100, 16)),
    ("wholly outside to the left", 0, (-50, 3, 25)),
    ("larger than the photograph", 1, (-8, -10, 25)),
    ("larger than the photograph, copy", 1, (-3, -3, 16)),
    ("the whole 9 x 9 photograph", 1, (0, 0, 9)),
    ("larger than the photograph at the bound", 1, (-15, -16, 40)),
]

PASTE_WINDOWS = [
    ("inside R=16", 0, (5, 3, 16)),
    ("inside R=10", 0, (20, 10, 10)),
    ("inside R=25", 0, (10, 2, 25)),
    ("over the top-left corner R=25", 0, (-7, -5, 25)),
    ("over the bottom-right corner R=25", 0, (30, 20, 25)),
    ("over every side R=40", 0, (-5, -5, 40)),
    ("over every side of 12 x 12, R=16", 1, (-2, -2, 16)),
    ("over two sides of 12 x 12, R=10", 1, (3, 4, 10)),
    ("12 x 12 inside R=40", 1, (-14, -14, 40)),
    ("wholly outside", 0, (100, 100, 16)),
    ("wholly outside to the left", 1, (-50, 0, 25)),
]


def random_photos(seed, shapes):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for H, W in shapes]


def mask_cases(seed, S=S_TEST):
    """[(name, uint8 [2,S,S])]: an ellipse pair, random bits, cup set where the disc is not, all ones, all zeros"""
    rng = np.random.RandomState(seed)
    r, c = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    disc = ((r - 0.45 * S) / (0.36 * S)) ** 2 + ((c - 0.55 * S) / (0.30 * S)) ** 2 <= 1.0
    cup = ((r - 0.50 * S) / (0.20 * S)) ** 2 + ((c - 0.50 * S) / (0.14 * S)) ** 2 <= 1.0
    away = np.roll(cup, S // 3, 1)
    u8 = lambda a, b: np.stack([a, b]).astype(np.uint8)
    return [("ellipse pair", u8(cup, disc)), ("random bits", rng.randint(0, 2, (2, S, S)).astype(np.uint8) * 255),
            ("cup where the disc is not", u8(away | cup, disc & ~away)), ("all ones", np.ones((2, S, S), np.uint8)),
            ("all zeros", np.zeros((2, S, S), np.uint8))]


# ------------------------------------------------------------------------------------------------ the pipeline end to end
# (photograph size, drawn disc centre (row, column), disc radius): grey photographs with a bright disc (140) and a brighter cup (220) on 40
DRAWN = [((96, 128), (50, 76), 16), ((64, 64), (30, 34), 14), ((70, 150), (50, 40), 18)]
E2E_SIZE, E2E_ROI = 32, 48


def draw_photo(shape, centre, radius):
    H, W = shape
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    g = np.full((H, W), 40, np.uint8)
    g[(r - centre[0]) ** 2 + (c - centre[1]) ** 2 <= radius ** 2] = 140
    g[(r - centre[0] - 2) ** 2 + (c - centre[1] + 3) ** 2 <= (radius * 0.4) ** 2] = 220
    return np.ascontiguousarray(np.repeat(g[:, :, None], 3, 2))


def brightness_stub(image):
    """Stand-in generator: [B,3,H,W] in [-1, 1] -> (logits [B,2,H,W], None) by brightness, on whatever device the image is.  The
    evaluation post-processing erodes every mask by a 7-pixel diamond at any scale (utils/Utils.py:427-463), which empties a disc of
    a few canvas pixels, so the stand-in answers 6 pixels wider than what it sees (a 13 x 13 maximum).  The thresholds sit between
    integer grey levels (disc > 110.5; cup > 0.1 after the sigmoid, grey > 163.1), so host and device agree on every pixel."""
    import torch
    grey = torch.nn.functional.max_pool2d((image.mean(1, keepdim=True) + 1.0) * 127.5, 13, 1, 6)[:, 0]
    return torch.stack([grey - 165.3, grey - 110.5], 1), None


def restated_masks(u8_hwc, dataset="Drishti-GS", threshold=0.75):
    """stub -> sigmoid -> the scipy statement of the post-processing (tests/postproc_shapes.py) of one uint8 [S,S,3] image -> [2,S,S]"""
    import torch
    import postproc_shapes
    logits = brightness_stub(torch.from_numpy(normalise(u8_hwc))[None])[0]
    prob = torch.sigmoid(logits.float())[0].numpy()
    thr = (0.1, 0.5) if dataset[0] == "D" else (threshold, threshold)
    return postproc_shapes.stages(prob, *thr)["filled"]


def disc_moments(masks):
    r, c = np.nonzero(masks[1])
    return [len(r), int(r.sum()), int(c.sum())]


def restated_pipeline(photo, size=E2E_SIZE, roi_size=E2E_ROI, centre_xy=None):
    """-> {'box', 'located', 'masks' [2,S,S], 'photo_mask' [H,W], 'disc_cx', 'disc_cy'} of one photograph, every stage restated"""
    H, W = photo.shape[:2]
    if centre_xy is None:
        canvas, f = reduce_photo(photo, size)
        cy, cx, located = centre(disc_moments(restated_masks(canvas)), f, H, W)
    else:
        (cx, cy), located = centre_xy, 1
    box = boxes([(cy, cx)], [(H, W)], roi_size)[0]
    masks = restated_masks(cut(photo, box, size))
    n, sr, sc = disc_moments(masks)
    return {"box": box, "located": located, "masks": masks, "photo_mask": paste(masks, box, H, W), "centre": (cy, cx),
            "disc_cx": box[0] + (sc / n + 0.5) * roi_size / size if n else float("nan"),
            "disc_cy": box[1] + (sr / n + 0.5) * roi_size / size if n else float("nan")}
