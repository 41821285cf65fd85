"""The yardstick of the Fourier style transfer (uda_clr_amd.ops.fda_transfer, include/uda_clr_hip.h uda_fda_*): numpy float64, written
from the literal statement of Fourier Domain Adaptation (Yang & Soatto, CVPR 2020) - fft2 per channel, fftshift, copy the target's
amplitude window [c - b, c + b]^2 with c = (H // 2, W // 2), ifftshift, ifft2 of amplitude * e^{i phase}, real part, clip(rint()).
The zero-magnitude rule: inside the window a source coefficient with |F_s| <= 1e-6 H W has phase 0 (numpy.angle(0) = 0 says so for
an exact zero; a float64 sum over a constant channel leaves about 1e-12 of an arbitrary phase instead).

Also here: an independent restatement as a partial DFT over the window (``partial_dft``), and the seeded fixtures that the CPU and the
GPU tests share.  The CPU tests assert of every fixture that no unrounded value lies within 1e-8 of a half-integer and that every
windowed |F_s| is below 1e-9 H W or above 1e-3 H W: only then is byte equality a fair demand of an implementation whose float64 sums
run in another order (the two statements here differ by about 1e-11 grey levels)."""
import numpy as np

TINY = 1e-6           # times H W: the zero-magnitude rule


def oracle(src, tgt, band, pair=None, apply=None):
    """src uint8 [B,H,W,3], tgt uint8 [Bt,H,W,3] -> (uint8 [B,H,W,3], the unrounded float64 values)"""
    src, tgt = np.asarray(src), np.asarray(tgt)
    B, H, W, _ = src.shape
    assert tgt.shape[1:] == src.shape[1:] and 2 * band + 2 <= min(H, W)
    pair = np.arange(B) % tgt.shape[0] if pair is None else np.asarray(pair)
    ch, cw = H // 2, W // 2
    win = (slice(ch - band, ch + band + 1), slice(cw - band, cw + band + 1))
    raw = src.astype(np.float64)
    for i in range(B):
        if apply is not None and not apply[i]:
            continue
        for c in range(3):
            fs = np.fft.fftshift(np.fft.fft2(src[i, :, :, c].astype(np.float64)))
            ft = np.fft.fftshift(np.fft.fft2(tgt[pair[i], :, :, c].astype(np.float64)))
            amp, pha = np.abs(fs), np.angle(fs)
            pha[win] = np.where(amp[win] <= TINY * H * W, 0.0, pha[win])
            amp[win] = np.abs(ft)[win]
            raw[i, :, :, c] = np.real(np.fft.ifft2(np.fft.ifftshift(amp * np.exp(1j * pha))))
    return np.clip(np.rint(raw), 0, 255).astype(np.uint8), raw


def partial_dft(src, tgt, band, pair=None):
    """The same values without an FFT: out = src + (1 / HW) sum over the window of (|F_t| P - F_s) e^{+2 pi i (u y / H + v x / W)} with the
    (2 band + 1)^2 coefficients formed by explicit sums.  Unrounded float64 [B,H,W,3]."""
    src, tgt = np.asarray(src), np.asarray(tgt)
    B, H, W, _ = src.shape
    pair = np.arange(B) % tgt.shape[0] if pair is None else np.asarray(pair)
    u = np.arange(-band, band + 1)
    ey = np.exp(-2j * np.pi * ((u[:, None] * np.arange(H)[None, :]) % H) / H)          # [u, y]
    ex = np.exp(-2j * np.pi * ((u[:, None] * np.arange(W)[None, :]) % W) / W)          # [v, x]
    out = src.astype(np.float64)
    for i in range(B):
        for c in range(3):
            fs = ey @ src[i, :, :, c].astype(np.float64) @ ex.T
            ft = ey @ tgt[pair[i], :, :, c].astype(np.float64) @ ex.T
            mag = np.abs(fs)
            small = mag <= TINY * H * W
            phase = np.where(small, 1.0, fs / np.where(small, 1.0, mag))
            d = np.abs(ft) * phase - fs
            out[i, :, :, c] += np.real(ey.conj().T @ d @ ex.conj()) / (H * W)
    return out


def windowed_amplitudes(src, band):
    """|F_s| / (H W) over the window, every image and channel: [B, 3, 2 band + 1, 2 band + 1]"""
    src = np.asarray(src)
    B, H, W, _ = src.shape
    f = np.fft.fftshift(np.fft.fft2(src.astype(np.float64), axes=(1, 2)), axes=(1, 2))
    ch, cw = H // 2, W // 2
    return np.abs(f[:, ch - band:ch + band + 1, cw - band:cw + band + 1, :]).transpose(0, 3, 1, 2) / (H * W)


def tie_distance(raw):
    """the smallest distance of an unrounded value to a half-integer"""
    return float(np.abs(np.abs(raw - np.floor(raw) - 0.5)).min())


def images(seed, n, H, W, lo=0, hi=255):
    """structured random photographs, uint8 [n,H,W,3] within [lo, hi]: per channel a few Gaussian blobs on a linear ramp, plus noise"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.empty((n, H, W, 3), np.uint8)
    for i in range(n):
        for c in range(3):
            f = rs.uniform(-1, 1) * yy / H + rs.uniform(-1, 1) * xx / W
            for _ in range(4):
                cy, cx, s = rs.uniform(0, H), rs.uniform(0, W), rs.uniform(0.08, 0.4) * min(H, W)
                f += rs.uniform(-1.5, 1.5) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
            f += rs.uniform(-1, 1, (H, W))
            f = (f - f.min()) / (f.max() - f.min())
            out[i, :, :, c] = np.rint(lo + (hi - lo) * f).astype(np.uint8)
    return out


# name -> (H, W, band, B, Bt, source seed, target seed); pair = [2, 0] in the GPU tests
SHAPES = {
    "40x56 b3": (40, 56, 3, 2, 3, 101, 201),          # not square, no multiple of 32 or 64
    "33x47 b2": (33, 47, 2, 2, 3, 102, 202),          # odd sizes, the centre H // 2
    "16x16 b7": (16, 16, 7, 2, 3, 103, 203),          # the largest band the size allows: 2 b + 2 = 16
    "64x64 b5": (64, 64, 5, 2, 3, 104, 204),
    "136x136 b64": (136, 136, 64, 2, 3, 117, 217),    # the cap, and the chunked loop over v
}
PAIR = [2, 0]


def fixture(name):
    """-> dict(src, tgt, band, pair, apply) of one named case: the shapes above, 'constant' (source channels all 0 and all 200) and
    'clip' (a bright target on a dark source and the reverse), both at 40 x 56"""
    if name in SHAPES:
        H, W, band, B, Bt, ss, st = SHAPES[name]
        return dict(src=images(ss, B, H, W), tgt=images(st, Bt, H, W), band=band, pair=PAIR, apply=None)
    if name == "apply":
        return dict(fixture("40x56 b3"), apply=[1, 0])
    if name == "constant":
        src = images(111, 2, 40, 56)
        src[0, :, :, 0], src[0, :, :, 1] = 0, 200
        src[1, :, :, 2], src[1, :, :, 0] = 0, 200
        return dict(src=src, tgt=images(211, 3, 40, 56), band=3, pair=PAIR, apply=None)
    if name == "clip":
        src = np.concatenate([images(112, 1, 40, 56, 0, 50), images(113, 1, 40, 56, 205, 255)])
        tgt = np.concatenate([images(212, 1, 40, 56, 0, 40), images(213, 1, 40, 56, 60, 200), images(214, 1, 40, 56, 215, 255)])
        return dict(src=src, tgt=tgt, band=3, pair=PAIR, apply=None)          # sample 0: dark source, bright target 2; sample 1 the reverse
    raise KeyError(name)


FIXTURES = list(SHAPES) + ["apply", "constant", "clip"]
_CACHE = {}


def reference(name):
    """(fixture, oracle bytes, oracle unrounded values) of a named case, computed once per process and not to be modified"""
    if name not in _CACHE:
        fx = fixture(name)
        u8, raw = oracle(fx["src"], fx["tgt"], fx["band"], fx["pair"], fx["apply"])
        for a in (fx["src"], fx["tgt"], u8, raw):
            a.setflags(write=False)
        _CACHE[name] = (fx, u8, raw)
    return _CACHE[name]
