"""The numpy restatement of uda_disc_morphometry (include/uda_clr_hip.h) and of the figures formed from it, and the shapes the
morphometry tests use.  Nothing here imports the package: the sector table is an ARGUMENT (the tests hand the package's table to
both sides), everything else is restated from the definitions over the pixels of each mask.

    integers(masks, table)  -> moments, extent, overlap, radial: Python-int / int64 arithmetic, exact
    figures(masks, table)   -> the per-image floats, each from the pixels by the shortest route to its definition
"""
import math

import numpy as np


# ------------------------------------------------------------------------------------------------------------ the integers
def sector_of(ux, uy, table):
    """int64 arrays ux, uy (x right, y up) -> the sector of every vector: the one j with cross(s_j, u) >= 0 and cross(s_j+1, u) < 0;
    -1 for u = 0.  Asserts that every other vector lies in exactly one sector."""
    K = table.shape[0]
    ux, uy = np.asarray(ux, np.int64), np.asarray(uy, np.int64)
    ge = [int(table[j, 0]) * uy - int(table[j, 1]) * ux >= 0 for j in range(K)]          # |s| <= 2^30, |u| < 2^30: below 2^61
    sector = np.full(ux.shape, -1, np.int64)
    hits = np.zeros(ux.shape, np.int64)
    nonzero = (ux != 0) | (uy != 0)
    for j in range(K):
        inside = ge[j] & ~ge[(j + 1) % K] & nonzero
        sector[inside] = j
        hits += inside
    assert (hits[nonzero] == 1).all() and (hits[~nonzero] == 0).all()
    return sector


def integers(masks, table):
    """masks [B,2,H,W] (0 cup, 1 disc; nonzero = set), table int64 [K,2] -> {'moments' [B,2,6], 'extent' [B,2,4], 'overlap' [B],
    'radial' [B,2,K]} int64"""
    m = np.asarray(masks) != 0
    table = np.asarray(table, np.int64)
    B, K = m.shape[0], table.shape[0]
    moments, extent = np.zeros((B, 2, 6), np.int64), np.full((B, 2, 4), -1, np.int64)
    overlap, radial = np.zeros(B, np.int64), np.full((B, 2, K), -1, np.int64)
    for b in range(B):
        pix = []
        for k in range(2):
            r, c = np.nonzero(m[b, k])
            r, c = r.astype(np.int64), c.astype(np.int64)
            pix.append((r, c))
            if r.size:
                moments[b, k] = (r.size, r.sum(), c.sum(), (r * r).sum(), (c * c).sum(), (r * c).sum())
                extent[b, k] = (r.min(), r.max(), c.min(), c.max())
        overlap[b] = int((m[b, 0] & m[b, 1]).sum())
        n, Sr, Sc = (int(v) for v in moments[b, 1, :3])
        if n == 0:
            continue
        for k in range(2):
            r, c = pix[k]
            ux, uy = n * c - Sc, -(n * r - Sr)
            sector, d2 = sector_of(ux, uy, table), ux * ux + uy * uy
            for j in np.unique(sector[sector >= 0]):
                radial[b, k, j] = d2[sector == j].max()
    return {"moments": moments, "extent": extent, "overlap": overlap, "radial": radial}


# -------------------------------------------------------------------------------------------------------------- the figures
def _ratio(a, b):
    return float(a) / float(b) if b else math.nan


def figures(masks, table):
    """per image, straight from the pixels: {'vcdr', 'hcdr', 'acdr', 'rim_area', 'cup_offset' (length), 'rim_ratio' [B,K], 'rdr_min',
    'rdr_min_angle', 'n_empty_sectors', 'rim_up', 'rim_left', 'rim_down', 'rim_right', 'cov' [B,2,2,2] in (x, y) = (column, -row)}"""
    m = np.asarray(masks) != 0
    table = np.asarray(table, np.int64)
    B, K = m.shape[0], table.shape[0]
    ints = integers(m, table)
    names = ("vcdr", "hcdr", "acdr", "rim_area", "cup_offset", "rdr_min", "rdr_min_angle", "n_empty_sectors", "rim_up", "rim_left", "rim_down", "rim_right")
    out = {k: np.full(B, np.nan) for k in names}
    out["rim_ratio"], out["cov"] = np.full((B, K), np.nan), np.full((B, 2, 2, 2), np.nan)
    for b in range(B):
        cup, disc = m[b, 0], m[b, 1]
        rows = [int(x.any(1).sum() and np.ptp(np.nonzero(x.any(1))[0]) + 1) for x in (cup, disc)]
        cols = [int(x.any(0).sum() and np.ptp(np.nonzero(x.any(0))[0]) + 1) for x in (cup, disc)]
        out["vcdr"][b], out["hcdr"][b] = _ratio(rows[0], rows[1]), _ratio(cols[0], cols[1])
        out["acdr"][b] = _ratio(cup.sum(), disc.sum())
        out["rim_area"][b] = float((disc & ~cup).sum())
        cen = []
        for k, x in enumerate((cup, disc)):
            r, c = np.nonzero(x)
            n = r.size
            cen.append((_ratio(int(r.sum()), n), _ratio(int(c.sum()), n)))
            if n:
                out["cov"][b, k] = np.cov(np.stack([c, -r]).astype(np.float64), bias=True).reshape(2, 2)
        out["cup_offset"][b] = math.hypot(cen[0][0] - cen[1][0], cen[0][1] - cen[1][1])
        n_disc, rad = int(disc.sum()), ints["radial"][b]
        ratio = []
        for j in range(K):
            if rad[1, j] < 0 or (rad[0, j] < 0 and cup.any()):
                ratio.append(math.nan)
            elif not cup.any():
                ratio.append(1.0)
            else:
                ratio.append(1.0 - (math.sqrt(int(rad[0, j])) / n_disc) / (math.sqrt(int(rad[1, j])) / n_disc))
        out["rim_ratio"][b] = ratio
        have = [j for j in range(K) if not math.isnan(ratio[j])]
        out["n_empty_sectors"][b] = K - len(have)
        if have:
            jmin = min(have, key=lambda j: (ratio[j], j))
            out["rdr_min"][b], out["rdr_min_angle"][b] = ratio[jmin], (jmin + 0.5) * (360.0 / K)
        for name, centre in (("rim_right", 0), ("rim_up", K // 4), ("rim_left", K // 2), ("rim_down", 3 * K // 4)):
            quad = [ratio[(centre + d) % K] for d in range(-(K // 8), K // 8) if not math.isnan(ratio[(centre + d) % K])]
            out[name][b] = math.fsum(quad) / len(quad) if quad else math.nan          # the correctly rounded sum: no order to agree on
    return out


def axes_of(cov):
    """(major, minor, orientation in degrees) of the ellipse with the 2x2 covariance ``cov`` in (x, y), by symmetric eigendecomposition"""
    lam, vec = np.linalg.eigh(cov)
    v = vec[:, 1]
    ang = math.degrees(math.atan2(v[1], v[0]))
    ang = ang - 180.0 if ang > 90.0 else ang + 180.0 if ang <= -90.0 else ang
    return 4.0 * math.sqrt(max(lam[1], 0.0)), 4.0 * math.sqrt(max(lam[0], 0.0)), ang


# --------------------------------------------------------------------------------------------------------------- the shapes
def ellipse(H, W, cy, cx, a, b, theta=0.0):
    """filled ellipse with semi-axes a (along the direction theta from the row axis) and b"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (yy - cy) * math.cos(theta) + (xx - cx) * math.sin(theta)
    v = -(yy - cy) * math.sin(theta) + (xx - cx) * math.cos(theta)
    return (u / a) ** 2 + (v / b) ** 2 <= 1.0


def nested_9x9():
    """[1,2,9,9]: a 5 x 5 disc with a 3 x 3 cup, both centred on (4, 4).  At K = 8 the pixels on the axes and the diagonals lie exactly
    on boundary rays and the centre pixel has u = 0; radial is [3125, 5000] * 4 for the disc and [625, 1250] * 4 for the cup."""
    m = np.zeros((1, 2, 9, 9), bool)
    m[0, 0, 3:6, 3:6] = True
    m[0, 1, 2:7, 2:7] = True
    return m


def ellipse_pairs(seed, B, H, W, cup=(0.18, 0.26), disc=(0.32, 0.42)):
    """[B,2,H,W]: a rotated disc ellipse and a rotated cup ellipse whose centre is shifted by up to 3 % of the short side; semi-axes
    as shares of the short side.  The defaults keep the cup inside the disc and around the disc's centroid."""
    rng = np.random.default_rng(seed)
    s = min(H, W)
    m = np.zeros((B, 2, H, W), bool)
    for b in range(B):
        cy, cx = rng.uniform(0.47, 0.53) * H, rng.uniform(0.47, 0.53) * W
        m[b, 1] = ellipse(H, W, cy, cx, rng.uniform(*disc) * s, rng.uniform(*disc) * s, rng.uniform(0, math.pi))
        m[b, 0] = ellipse(H, W, cy + rng.uniform(-0.03, 0.03) * s, cx + rng.uniform(-0.03, 0.03) * s, rng.uniform(*cup) * s,
                          rng.uniform(*cup) * s, rng.uniform(0, math.pi))
    return m


def empties_96x80():
    """[3,2,96,80]: image 0 has no cup, image 1 no disc, image 2 neither"""
    m = ellipse_pairs(21, 3, 96, 80)
    m[0, 0] = False
    m[1, 1] = False
    m[2] = False
    return m


def cup_partly_outside_96x80():
    """[1,2,96,80]: the cup runs over the disc's left edge"""
    m = np.zeros((1, 2, 96, 80), bool)
    m[0, 1] = ellipse(96, 80, 48, 44, 30, 26, 0.4)
    m[0, 0] = ellipse(96, 80, 46, 24, 16, 15, 1.0)
    assert (m[0, 0] & ~m[0, 1]).any() and (m[0, 0] & m[0, 1]).any()
    return m


def cup_off_centre_96x80():
    """[1,2,96,80]: the cup lies inside the disc but does not hold the disc's centroid: the cup sectors facing away are empty"""
    m = np.zeros((1, 2, 96, 80), bool)
    m[0, 1] = ellipse(96, 80, 48, 40, 36, 32)
    m[0, 0] = ellipse(96, 80, 30, 52, 8, 7, 0.3)
    assert not m[0, 0, 48, 40] and not (m[0, 0] & ~m[0, 1]).any()
    return m


def single_pixel_disc():
    """[1,2,33,17]: the disc is one pixel (u = 0 for it) and the cup is that pixel too"""
    m = np.zeros((1, 2, 33, 17), bool)
    m[0, :, 20, 5] = True
    return m


def touching_borders_96x80():
    """[2,2,96,80]: image 0's disc is the full plane and its cup touches all four borders as a cross; image 1's disc touches the four
    borders as an ellipse cut by them"""
    m = np.zeros((2, 2, 96, 80), bool)
    m[0, 1] = True
    m[0, 0, 40:56, :] = True
    m[0, 0, :, 30:50] = True
    m[1, 1] = ellipse(96, 80, 47.5, 39.5, 60, 50)
    m[1, 0] = ellipse(96, 80, 50, 38, 20, 18, 0.8)
    for x in (m[0, 0], m[0, 1], m[1, 1]):
        assert x[0].any() and x[-1].any() and x[:, 0].any() and x[:, -1].any()
    return m


def full_minus_corner_1024():
    """[1,2,1024,1024]: the disc is the full plane without its last pixel (so the centroid is not on the pixel grid and n does not
    divide the sums: the largest |u|), the cup a 40 x 40 block at the far corner from the missing pixel"""
    m = np.zeros((1, 2, 1024, 1024), bool)
    m[0, 1] = True
    m[0, 1, 1023, 1023] = False
    m[0, 0, :40, :40] = True
    return m
