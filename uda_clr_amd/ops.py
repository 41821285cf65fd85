"""Differentiable front-ends of the loss / prototype / metric kernels (torch.autograd.Function
wrappers around uda_clr_amd.kernels.HipKernels).  HIP only: CPU tensors raise.

Reference call sites these replace:
  seg_loss               Trainer_prototype_full.py:292-294, Trainer_baseline.py:206-208
  prototypes             utils/Utils.py:108-131 (gen_prototype), :159-225 (gen_prototype_retrify)
  seg_counts / dice ...  utils/metrics.py:118-168
"""
from __future__ import annotations

import torch

from . import kernels as hip
from .acts import nchw_view, round4
from .parallel import all_reduce_sum_

_K = None


def kernels():
    global _K
    if _K is None:
        from .kernels import HipKernels
        _K = HipKernels()
    return _K


def rows_view(t: torch.Tensor) -> torch.Tensor:
    """Logical [B, C, H, W] -> [P, C] NHWC rows with a 16-byte aligned, multiple-of-4 row stride.
    Zero-copy for the channels-last views the generator returns; one packing copy otherwise."""
    B, C, H, W = t.shape
    ld = t.stride(3) if W > 1 else (t.stride(2) // max(W, 1) if H > 1 else round4(C))
    ok = (t.stride(1) == 1 or C == 1) and ld % 4 == 0 and ld >= round4(C) and t.stride(2) == W * ld and \
        t.stride(0) == H * W * ld and (t.data_ptr() % 16 == 0) and t.dtype == torch.float32
    if ok:
        return t.as_strided((B * H * W, C), (ld, 1), t.storage_offset())
    buf = torch.empty(B * H * W, round4(C), dtype=torch.float32, device=t.device)
    v = buf[:, :C]
    v.copy_(t.permute(0, 2, 3, 1).reshape(B * H * W, C))
    return v


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, o, b, tmap, tbd):
        o, b, tmap, tbd = (t.contiguous().float() for t in (o, b, tmap, tbd))
        loss3 = kernels().seg_loss_fwd(o, tmap, b, tbd)
        ctx.save_for_backward(o, b, tmap, tbd)
        return loss3[0]

    @staticmethod
    def backward(ctx, g):
        o, b, tmap, tbd = ctx.saved_tensors
        d_o, d_b = kernels().seg_loss_bwd(o, tmap, b, tbd, g.reshape(1).contiguous().float())
        return d_o, d_b, None, None


def seg_loss(oS, boundaryS, target_map, target_boundary):
    """BCELoss(sigmoid(oS), map) + MSELoss(sigmoid(boundaryS), boundary): one fused pass, and one
    fused pass for both gradients."""
    return _SegLossFn.apply(oS, boundaryS, target_map, target_boundary)


class _ProtoFn(torch.autograd.Function):
    """centroids[4, C] = (sum_p w_k[p] f[p,:]) / (sum_p w_k[p]); sums are all-reduced over the data
    parallel ranks before the division so every rank holds the global centroids."""

    @staticmethod
    def forward(ctx, feat, wts, pred):
        K = kernels()
        rows = rows_view(feat)
        P, C = rows.shape
        sums = torch.zeros(4, C + 1, dtype=torch.float64, device=feat.device)
        K.proto_reduce(rows, wts, sums)
        all_reduce_sum_(sums)
        ctx.save_for_backward(rows, wts, sums)
        ctx.geom = tuple(feat.shape)
        ctx.want_dw = pred is not None and pred.requires_grad
        return K.proto_finalize(sums)

    @staticmethod
    def backward(ctx, dC):
        rows, wts, sums = ctx.saved_tensors
        B, C, H, W = ctx.geom
        d_feat = None
        d_rows = None
        if ctx.needs_input_grad[0]:
            d_rows = torch.empty(rows.shape[0], round4(C), dtype=torch.float32, device=rows.device)[:, :C]
            d_feat = nchw_view(d_rows, B, H, W)
        d_w = kernels().proto_bwd(rows, wts, sums, dC.contiguous().float(), d_rows, False, ctx.want_dw)
        d_pred = None
        if ctx.want_dw:      # w = (p0, p1, 1-p0, 1-p1)
            d_pred = torch.stack([d_w[:, 0] - d_w[:, 2], d_w[:, 1] - d_w[:, 3]], 1).reshape(B, H, W, 2).permute(0, 3, 1, 2)
        return d_feat, None, d_pred


class Centroids(tuple):
    """(cup_obj, disc_obj, cup_bck, disc_bck) as [1,C,1,1] views, like the reference's four return values, plus ``.matrix``,
    the [4, C] tensor they are rows of (what the fused alignment kernel takes)."""
    matrix = None
    centroids = None       # gen_prototype_retrify's 7-tuple: its first four entries as a Centroids of their own


def _split(cent):
    C = cent.shape[1]
    out = Centroids(cent[k].reshape(1, C, 1, 1) for k in range(4))
    out.matrix = cent
    return out


def _matrix(cents):
    m = getattr(cents, "matrix", None)
    return m if m is not None else torch.cat([t.reshape(1, -1) for t in cents], 0)


class _AlignFn(torch.autograd.Function):
    """EMA of both domains' centroids + intra / inter losses in one launch (uda_proto_align_fwd); backward: one launch for both
    current-centroid gradients (the EMA keeps gradient only through the current term, quirk Q4)."""

    @staticmethod
    def forward(ctx, cur_src, cur_tgt, prev_src, prev_tgt, decay):
        K = kernels()
        new_src, new_tgt, losses = K.proto_align_fwd(cur_src.contiguous().float(), cur_tgt.contiguous().float(),
                                                     prev_src, prev_tgt, decay)
        ctx.save_for_backward(new_src, new_tgt)
        ctx.w = (1.0 if prev_src is None else decay, 1.0 if prev_tgt is None else decay)
        ctx.mark_non_differentiable(new_src, new_tgt)
        ctx.set_materialize_grads(False)        # an unused output arrives as None, not as a zero tensor: no device read needed below
        return losses[0], losses[1], new_src, new_tgt

    @staticmethod
    def backward(ctx, g_intra, g_inter, _a, _b):
        new_src, new_tgt = ctx.saved_tensors
        if g_inter is not None:
            raise NotImplementedError("inter_loss is logged only (Trainer_prototype_full.py:443-449, :465); no gradient is built for it")
        if g_intra is None:
            return None, None, None, None, None
        d_src, d_tgt = kernels().proto_align_bwd(new_src, new_tgt, g_intra.reshape(1).contiguous().float(), ctx.w[0], ctx.w[1])
        return d_src, d_tgt, None, None, None


def proto_align(cur_src, cur_tgt, prev_src, prev_tgt, decay):
    """Trainer_prototype_full.py:335-355, 378-398, 428-444 fused: returns (intra_loss, inter_loss, src, tgt) where src / tgt
    are the DETACHED EMA centroids to store for the next iteration (``Centroids``); ``prev_*`` is that stored state or None."""
    ps = None if prev_src is None else _matrix(prev_src).detach().contiguous()
    pt = None if prev_tgt is None else _matrix(prev_tgt).detach().contiguous()
    intra, inter, new_src, new_tgt = _AlignFn.apply(_matrix(cur_src), _matrix(cur_tgt), ps, pt, float(decay))
    return intra, inter, _split(new_src), _split(new_tgt)


class _AdvLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, d1, d2, label, scale):
        d1, d2 = d1.contiguous().float(), d2.contiguous().float()
        ctx.save_for_backward(d1, d2)
        ctx.args = (label, scale)
        return kernels().adv_loss_fwd(d1, d2, label, scale)[0]

    @staticmethod
    def backward(ctx, g):
        d1, d2 = ctx.saved_tensors
        g1, g2 = kernels().adv_loss_bwd(d1, d2, ctx.args[0], ctx.args[1], g.reshape(1).contiguous().float())
        return g1, g2, None, None


def adv_loss(d_out1, d_out2, label, scale=1.0):
    """scale * (BCEWithLogits(d_out1, label) + BCEWithLogits(d_out2, label)) on the two patch-discriminator outputs
    (Trainer_prototype_full.py:456-458, 479-513): one launch forward, one for both gradients."""
    return _AdvLossFn.apply(d_out1, d_out2, float(label), float(scale))


def gen_prototype(pred, feature):
    """utils/Utils.py:108-131.  pred [B,2,h,w] (ch0 cup, ch1 disc; hard labels or probabilities),
    feature [B,C,h,w] -> (cup_obj, disc_obj, cup_bck, disc_bck) centroids [1,C,1,1]."""
    B, _, h, w = pred.shape
    wts, _, _ = kernels().proto_weights(0, B, h, w, map_=pred.detach().contiguous().float())
    return _split(_ProtoFn.apply(feature, wts, pred))


def gen_prototype_from_labels(target_map, feature):
    """Fused form of Trainer_prototype_full.py:330-334: nearest-resize of the full-resolution label
    map to the feature size happens inside the weights kernel."""
    B, _, h, w = feature.shape
    wts, _, _ = kernels().proto_weights(0, B, h, w, map_=target_map.detach().contiguous().float())
    return _split(_ProtoFn.apply(feature, wts, None))


def gen_prototype_retrify(oT_before, xt_feature, preds, features, T, stride):
    """utils/Utils.py:159-225.  ``features`` is accepted for signature parity and ignored (its mean
    is dead in the reference, quirk Q5).  Gradient reaches only ``xt_feature`` (quirk Q6)."""
    K = kernels()
    B, C, h, w = xt_feature.shape
    assert preds.shape[0] == T * stride and stride == B
    std_map, mean_map = K.mc_stats(preds.detach().contiguous().float(), T)
    wts, m0, m1 = K.proto_weights(2, B, h, w, logits=rows_view(oT_before.detach()), std_map=std_map, mean_map=mean_map)
    cents = _split(_ProtoFn.apply(xt_feature, wts, None))
    out = Centroids(tuple(cents) + (std_map, m0.reshape(B, 1, h, w), m1.reshape(B, 1, h, w)))     # the reference's 7 return values
    out.matrix, out.centroids = None, cents
    return out


def class_scatter(feature, wts, centre=None, out=None):
    """Centred, weighted second moments of the four classes (uda_proto_scatter): feature [B,C,h,w] (or its [P,C] rows,
    as ``rows_view`` gives them), wts [P, 4] as uda_proto_weights writes them, centre [4,C] float or None (zeros) -> float64 [4,C,C] on the device,
    S_k = sum_p w_k[p] (f_p - centre_k)(f_p - centre_k)^T.  Added into ``out`` when given.  No autograd."""
    if not feature.is_cuda:
        raise hip.UdaError("class_scatter needs device tensors (got %s); there is no CPU fallback" % feature.device)
    rows = feature.detach() if feature.dim() == 2 else rows_view(feature.detach())
    C = rows.shape[1]
    if out is None:
        out = torch.zeros(4, C, C, dtype=torch.float64, device=feature.device)
    if centre is not None:
        centre = centre.detach().reshape(4, C).contiguous().float()
    kernels().proto_scatter(rows, wts.detach().contiguous().float(), out, centre)
    return out


class _DiscriminativeFn(torch.autograd.Function):
    """Prototype-guided discriminative loss on the source features (no shipped
    source - parity unpinned).  D(f,c) = mean_c (f-c)^2, so D(f,c_obj) - D(f,c_bck) is AFFINE in f:
        diff_k[p] = -(2/C) f[p,:].(c_obj - c_bck) + (|c_obj|^2 - |c_bck|^2)/C
    one pass over the 305-channel feature (uda_feat_dot4) gives both classes' differences, and the
    gradient is a per-pixel scalar times the constant vector (c_bck - c_obj) (uda_feat_rank4)."""

    @staticmethod
    def forward(ctx, feature, cents, labels, margin):
        K = kernels()
        rows = rows_view(feature)
        P, C = rows.shape
        B, _, H, W = feature.shape
        c = cents.detach().float()                      # [4, C]: cup_obj, disc_obj, cup_bck, disc_bck
        coef = torch.zeros(4, C + 1, dtype=torch.float32, device=rows.device)
        for k in (0, 1):
            coef[k, :C] = (-2.0 / C) * (c[k] - c[k + 2])
            coef[k, C] = (c[k].pow(2).sum() - c[k + 2].pow(2).sum()) / C
        diff = K.feat_dot4(rows, coef)[:, :2]                                  # [P, 2]
        m = labels.detach().permute(0, 2, 3, 1).reshape(P, 2).float()
        pos, neg = diff + margin, margin - diff
        loss = ((m * torch.relu(pos)).sum(0) + ((1 - m) * torch.relu(neg)).sum(0)).sum() / P
        ctx.save_for_backward(coef, m, diff)
        ctx.geom, ctx.margin = (B, C, H, W), margin
        return loss

    @staticmethod
    def backward(ctx, g):
        coef, m, diff = ctx.saved_tensors
        B, C, H, W = ctx.geom
        P = m.shape[0]
        s = (m * (diff + ctx.margin > 0).float() - (1 - m) * (ctx.margin - diff > 0).float()) * (g / P)
        wts = torch.zeros(P, 4, dtype=torch.float32, device=m.device)
        wts[:, :2] = s
        d_rows = torch.empty(P, round4(C), dtype=torch.float32, device=m.device)[:, :C]
        kernels().feat_rank4(wts, coef, d_rows, False)
        return nchw_view(d_rows, B, H, W), None, None, None


def discriminative_loss(feature, centroids, labels, margin=0.01):
    """centroids: the 4-tuple (cup_obj, disc_obj, cup_bck, disc_bck) of [1,C,1,1] prototypes (detached)."""
    cents = torch.cat([t.reshape(1, -1) for t in centroids], 0)
    return _DiscriminativeFn.apply(feature, cents, labels, margin)


def normalize_tf(image_u8, label_u8):
    """Device-side ``Normalize_tf`` + ``ToTensor`` (dataloaders/custom_transforms.py:432-466,504-507) of a uint8 batch:
    image_u8 [B,H,W,3], label_u8 [B,H,W] (grey-coded mask) -> image [B,3,H,W] in [-1,1], map [B,2,H,W], boundary [B,1,H,W].
    Bit-identical to the scipy.ndimage calls the reference makes per sample on the CPU (tests/test_input_gpu.py)."""
    return kernels().normalize_tf(image_u8.contiguous(), label_u8.contiguous())


def elastic_deform(image_u8, label_u8, apply=None, noise=None, generator=None):
    """Device-side ``elastic_transform`` (custom_transforms.py:95-147) of a uint8 batch: per sample with ``apply[b]`` set
    (default: drawn with p = 0.5) a displacement field alpha * gaussian_filter(U(-1,1), sigma), alpha = 2 * W, sigma = 0.08 * W,
    bilinear resampling of the image (0 outside) and of the label (nearest edge).  Everything from the uniform noise on is the
    reference's float64 arithmetic in the reference's order: with ``noise`` ([2,B,H,W] float64 in [-1,1), the two fields numpy's
    ``RandomState.rand`` gave the reference) the output bytes equal the reference's (tests/test_input_golden_gpu.py).  Without it
    the noise comes from torch's device generator - the reference seeds its RandomState from OS entropy, so there is no
    stream to reproduce; the distribution is the same."""
    K = kernels()
    B, H, W, _ = image_u8.shape
    dev = image_u8.device
    if apply is None:
        apply = (torch.rand(B, generator=generator) > 0.5).to(torch.uint8).to(dev)
    if noise is None:
        noise = torch.rand(2, B, H, W, device=dev, dtype=torch.float64) * 2.0 - 1.0
    field = K.field_smooth(noise.to(torch.float64).contiguous(), 0.08 * W, 2.0 * W)
    return K.elastic_warp(image_u8.contiguous(), label_u8.contiguous(), field[0], field[1], apply)


def photometric_u8(image_u8, sp_pos, sp_count, sp_value, lut, erase_box):
    """add_salt_pepper_noise -> adjust_light -> eraser (custom_transforms.py:150-250) on a uint8 batch, in place, with the
    outcomes the dataloader workers drew (see dataloaders.custom_transforms.DEVICE_TAIL)."""
    return kernels().photometric_u8(image_u8, sp_pos.contiguous(), sp_count.contiguous().view(-1), sp_value.contiguous().view(-1),
                                    lut.contiguous(), erase_box.contiguous())


def fda_band(beta, H, W):
    """the band of Fourier Domain Adaptation at window ratio ``beta``: b = floor(beta * min(H, W)) (Yang & Soatto's ``np.floor(np.amin((h, w)) * L)``)"""
    import math
    return int(math.floor(float(beta) * min(int(H), int(W))))


def fda_spectrum(image_u8, band):
    """uint8 [N,H,W,3] on the device -> complex128 [N,3,2b+1,b+1]: F[n,c,u,v] = sum_y sum_x s[y,x] e^{-2 pi i (u y / H + v x / W)} for u = -b..b
    (index u + b) and v = 0..b, the half of the window [-b, b]^2 that ``fda_transfer`` computes (the rest is its conjugate mirror).
    float64 throughout; against numpy.fft.fft2 within 1e-12 * sum|s| (tests/test_fda_gpu.py)."""
    return torch.view_as_complex(kernels().fda_spectrum(image_u8.contiguous(), band))


def fda_transfer(src_u8, tgt_u8, beta=0.01, band=None, pair=None, apply=None):
    """Fourier Domain Adaptation (Yang & Soatto, CVPR 2020) of a uint8 source batch [B,H,W,3] towards a uint8 target batch [Bt,H,W,3], on
    the device: source image i takes the amplitude spectrum of target image pair[i] on the (2b+1)^2 lowest frequencies and keeps its own
    phase.  Per channel, with F = fft2,

        out = clip(rint(src + (1 / HW) sum_{(u,v) in [-b,b]^2} (|F_t[u,v]| P[u,v] - F_s[u,v]) e^{+2 pi i (u y / H + v x / W)}), 0, 255)

    P = F_s / |F_s|, and P = (1, 0) where |F_s[u,v]| <= 1e-6 H W (the zero-magnitude rule: what numpy.angle(0) = 0 gives the literal
    fft2 / fftshift / swap window / ifftshift / ifft2 statement, defined for a constant channel too).  float64 from the bytes to the
    rounding; rint rounds ties to even, as numpy's.  ``band`` defaults to floor(beta * min(H, W)), ``pair`` to arange(B) % Bt; ``apply``
    ([B], nonzero = transfer; None = all) leaves the other samples byte for byte.  Host-side ``pair`` values are checked here; values
    already on the device are clamped into [0, Bt) by the kernel.  Labels are not involved.  Equal inputs give equal bytes.
    The formula is pinned against the literal statement (tests/fda_ref.py) by tests/test_fda_cpu.py (restatement, identity, band-0 mean)
    and byte for byte by tests/test_fda_gpu.py (rounding, zero-magnitude rule, clipping, pairing, apply)."""
    if src_u8.dim() != 4 or tgt_u8.dim() != 4:
        raise ValueError("fda_transfer: uint8 [B, H, W, 3] batches (got %s and %s)" % (tuple(src_u8.shape), tuple(tgt_u8.shape)))
    B, H, W = src_u8.shape[:3]
    Bt = tgt_u8.shape[0]
    dev = src_u8.device
    if band is None:
        band = fda_band(beta, H, W)
    if pair is None:
        pair = torch.arange(B, dtype=torch.int32) % max(Bt, 1)
    pair = torch.as_tensor(pair)
    if not pair.is_cuda:
        if pair.numel() != B or (B and (int(pair.min()) < 0 or int(pair.max()) >= Bt)):
            raise ValueError("fda_transfer: pair must hold %d target indices in [0, %d) (got %s)" % (B, Bt, pair.tolist()))
    pair = pair.to(dev).to(torch.int32).reshape(-1).contiguous()
    if apply is not None:
        apply = (torch.as_tensor(apply) != 0).to(torch.uint8).to(dev).reshape(-1).contiguous()
    return kernels().fda_transfer(src_u8.contiguous(), tgt_u8.to(dev).contiguous(), pair, band, apply)


class SourcePool(object):
    """A decoded dataset resident on the device for ``geometry_u8``: every image in one flat uint8 buffer, every mask in
    another, an int64 table of first pixels and an int32 (H0, W0) table, so sources of different sizes share a batch.
    4 B per source pixel (about 1 GB for 400 images of 800 x 800)."""
    def __init__(self, images, labels, device):
        import numpy as np
        imgs = [np.ascontiguousarray(np.asarray(i, dtype=np.uint8)) for i in images]
        labs = [np.ascontiguousarray(np.asarray(l, dtype=np.uint8)) for l in labels]
        if not imgs or len(imgs) != len(labs):
            raise ValueError("SourcePool needs as many masks as images, and at least one")
        for i, l in zip(imgs, labs):
            if i.ndim != 3 or i.shape[2] != 3 or l.shape != i.shape[:2]:
                raise ValueError("SourcePool: sources are [H,W,3] images with [H,W] masks (got %s and %s)" % (i.shape, l.shape))
        self.sizes_host = np.array([l.shape for l in labs], np.int32)
        px = self.sizes_host[:, 0].astype(np.int64) * self.sizes_host[:, 1]
        self.image_pool = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(device)
        self.label_pool = torch.from_numpy(np.concatenate([l.reshape(-1) for l in labs])).to(device)
        self.offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)).to(device)
        self.sizes = torch.from_numpy(self.sizes_host).to(device)

    def __len__(self):
        return int(self.sizes_host.shape[0])


def geometry_u8(pool, src_index, records, size=None):
    """Device-side ``RandomScaleCrop`` / ``RandomCrop`` -> ``RandomRotate`` -> ``RandomFlip`` (custom_transforms.py:152-182,
    208-223,315-355) of a batch: ``pool`` a SourcePool, ``src_index`` [B] the samples' dataset indices, ``records`` int32
    [B,10] the draws the workers recorded (dataloaders.custom_transforms.GEOM_*).  -> uint8 [B,S,S,3], uint8 [B,S,S], byte for
    byte what PIL gives.  Records that are still on the host (what the Trainer hands over) are checked here; the kernel only keeps a
    bad one in bounds.  Records already on the device are not checked: pass ``size`` with them to avoid reading it back."""
    from .dataloaders import custom_transforms as tr
    records = records.reshape(-1, tr.GEOM_R)
    src_index = src_index.reshape(-1)
    if not records.is_cuda:
        r, idx = records.numpy(), src_index.numpy()
        if idx.min() < 0 or idx.max() >= len(pool):
            raise ValueError("geometry_u8: source index outside the pool of %d" % len(pool))
        if (r[:, tr.GEOM_SIZE] != r[0, tr.GEOM_SIZE]).any() or r[0, tr.GEOM_SIZE] <= 0:
            raise ValueError("geometry_u8: one positive crop size per batch")
        hw = pool.sizes_host[idx]
        sc = r[:, tr.GEOM_SCALED] != 0
        if (sc & ((r[:, tr.GEOM_W] * 5 < hw[:, 1] * 2) | (r[:, tr.GEOM_H] * 5 < hw[:, 0] * 2))).any():
            raise ValueError("geometry_u8: a scaled size below 0.4 of its source")
        S = int(r[0, tr.GEOM_SIZE])
    elif size is not None:
        S = int(size)                                   # device records: the caller names the crop size, nothing is read back
    else:
        S = int(records[0, tr.GEOM_SIZE].item())        # device records without `size`: one host synchronisation, and no range checks
    dev = pool.image_pool.device
    return kernels().geometry_u8(pool.image_pool, pool.label_pool, pool.offsets, pool.sizes,
                                 src_index.to(dev).to(torch.int64).contiguous(), records.to(dev).to(torch.int32).contiguous(), S)


class PhotoPool(object):
    """Fundus photographs of any sizes resident on the device for ``photo_reduce`` / ``roi_cut`` / ``roi_paste``: every [H,W,3]
    uint8 image in one flat buffer, an int64 table of first pixels and an int32 (H, W) table (``SourcePool`` without the masks).
    3 B per pixel: one upload per batch of photographs."""
    MAX_SIDE = 8192

    def __init__(self, images, device):
        import numpy as np
        imgs = [np.ascontiguousarray(np.asarray(i, dtype=np.uint8)) for i in images]
        if not imgs:
            raise ValueError("PhotoPool needs at least one photograph")
        for i in imgs:
            if i.ndim != 3 or i.shape[2] != 3 or not (1 <= i.shape[0] <= self.MAX_SIDE and 1 <= i.shape[1] <= self.MAX_SIDE):
                raise ValueError("PhotoPool: photographs are [H,W,3] with 1 <= H, W <= %d (got %s)" % (self.MAX_SIDE, i.shape))
        self.sizes_host = np.array([i.shape[:2] for i in imgs], np.int32)
        px = self.sizes_host[:, 0].astype(np.int64) * self.sizes_host[:, 1]
        self.pool = torch.from_numpy(np.concatenate([i.reshape(-1) for i in imgs])).to(device)
        self.offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)).to(device)
        self.sizes = torch.from_numpy(self.sizes_host).to(device)

    def __len__(self):
        return int(self.sizes_host.shape[0])


def _photo_index(pool, index, who, allow_outside=False):
    """``index`` (None = every photograph in order) as int64 on the pool's device; a host-resident index is range-checked"""
    dev = pool.pool.device
    if index is None:
        return torch.arange(len(pool), dtype=torch.int64, device=dev)
    index = torch.as_tensor(index).reshape(-1)
    if not index.is_cuda and not allow_outside and index.numel() and (int(index.min()) < 0 or int(index.max()) >= len(pool)):
        raise ValueError("%s: photograph index outside the pool of %d" % (who, len(pool)))
    return index.to(dev).to(torch.int64).contiguous()


def _check_boxes(boxes, B, size, who):
    """boxes [B,3] = (x0, y0, R) as contiguous int32; host-resident ones are range-checked (the kernels only keep a bad one in bounds)"""
    boxes = torch.as_tensor(boxes)
    if boxes.dim() != 2 or tuple(boxes.shape) != (B, 3):
        raise ValueError("%s: boxes are [%d, 3] = (x0, y0, R), got %s" % (who, B, tuple(boxes.shape)))
    if not boxes.is_cuda:
        r = boxes[:, 2]
        if int(r.min()) < 8 or 2 * int(r.max()) > 5 * size:
            raise ValueError("%s: window side R must lie in 8..2.5 * size = %d (got %d..%d)" % (who, 5 * size // 2, int(r.min()), int(r.max())))
        if int(boxes[:, :2].abs().max()) > 2 ** 20:
            raise ValueError("%s: window origin beyond +-2^20" % who)
    return boxes.to(torch.int32).contiguous()


def photo_reduce(pool, index=None, size=512, outputs=("f32",)):
    """The coarse canvas of whole photographs (uda_photo_reduce_u8): every photograph of ``pool`` (a PhotoPool) selected by ``index``
    is reduced by the integer factor f = max(1, ceil(max(H, W) / size)) - block means, rounded half up in integers, edge blocks partial
    - into the top-left of a size x size canvas, 0 elsewhere.  -> {'u8': uint8 [B,size,size,3], 'f32': f32 [B,3,size,size] (the bytes
    normalised as ``predict`` normalises an image, so -1 where the canvas is 0)} for the names in ``outputs``, and 'factor': int32 [B],
    all on the device.  An index outside the pool (possible only for a device-resident index) gives a zero canvas and factor 0."""
    return kernels().photo_reduce(pool.pool, pool.offsets, pool.sizes, _photo_index(pool, index, "photo_reduce"), int(size), tuple(outputs))


def roi_cut(pool, boxes, index=None, size=512, outputs=("u8", "f32")):
    """The ROI of whole photographs (uda_roi_cut_u8): for photograph ``index[b]`` of ``pool`` and ``boxes[b]`` = (x0, y0, R), byte for byte
    Pillow's ``im.crop((x0, y0, x0 + R, y0 + R)).resize((size, size), Image.BILINEAR)``; the window may hang over the photograph and
    reads as 0 there; 8 <= R <= 2.5 * size.  -> {'u8': uint8 [B,size,size,3], 'f32': f32 [B,3,size,size] normalised as ``predict``
    normalises an image} for the names in ``outputs``, on the device.  Host-resident boxes are range-checked here."""
    idx = _photo_index(pool, index, "roi_cut")
    boxes = _check_boxes(boxes, idx.numel(), int(size), "roi_cut")
    return kernels().roi_cut(pool.pool, pool.offsets, pool.sizes, idx, boxes.to(pool.pool.device), int(size), tuple(outputs))


def roi_paste(pool_or_sizes, masks, boxes, index=None):
    """ROI masks back into photograph-sized grey masks (uda_roi_paste_u8): ``masks`` [B,2,S,S] (cup, disc; uint8, bool or float, set
    means > 0.5) for the windows ``boxes`` [B,3] = (x0, y0, R) of photographs whose sizes are ``pool_or_sizes``: a PhotoPool (with
    ``index`` selecting B of its photographs, None = all) or a host [B,2] array of (H, W).  -> a list of B uint8 [H,W] views into one flat
    device buffer, BEAL coding (0 cup, 128 disc only, 255 background and everything outside the window): each plane is the bilinear
    upsample (half-pixel centres, edge clamp) of the 0/1 mask thresholded at > 1/2 in exact integers, a tie not set."""
    import numpy as np
    if isinstance(pool_or_sizes, PhotoPool):
        hw = pool_or_sizes.sizes_host
        if index is not None:
            idx = np.asarray(torch.as_tensor(index).cpu()).reshape(-1)
            if idx.size and (idx.min() < 0 or idx.max() >= len(pool_or_sizes)):
                raise ValueError("roi_paste: photograph index outside the pool of %d" % len(pool_or_sizes))
            hw = hw[idx]
    else:
        hw = np.asarray(pool_or_sizes, np.int64).reshape(-1, 2)
    if hw.min() < 1 or hw.max() > PhotoPool.MAX_SIDE:
        raise ValueError("roi_paste: photograph sizes outside 1..%d" % PhotoPool.MAX_SIDE)
    (masks,) = _to_device(masks)
    masks = _mask_u8(masks)
    B = masks.shape[0]
    if hw.shape[0] != B:
        raise ValueError("roi_paste: %d masks for %d photographs" % (B, hw.shape[0]))
    boxes = _check_boxes(boxes, B, int(masks.shape[2]), "roi_paste").to(masks.device)
    px = hw[:, 0].astype(np.int64) * hw[:, 1]
    starts = np.concatenate([[0], np.cumsum(px)]).astype(np.int64)
    flat = kernels().roi_paste(masks, boxes, torch.from_numpy(np.ascontiguousarray(hw, dtype=np.int32)).to(masks.device),
                               torch.from_numpy(starts[:-1].copy()).to(masks.device), int(starts[-1]))
    return [flat[int(starts[b]):int(starts[b + 1])].view(int(hw[b, 0]), int(hw[b, 1])) for b in range(B)]


def photometric_augment(images, generator=None):
    """Device-side photometric augmentation of a [-1,1] image batch in the spirit of utils/Utils.py:33-43
    (brightness/contrast + saturation jitter with p=0.8, grayscale with p=0.2, 5x5 Gaussian blur with
    p=0.5; geometry and labels unchanged).  The reference does this per image on the CPU with
    albumentations/cv2; the exact random streams are not reproducible, so this is 'same family, same
    probabilities' (parity unpinned)."""
    B = images.shape[0]
    dev = images.device
    r = lambda *s: torch.rand(*s, generator=generator, device="cpu").to(dev)
    x = (images + 1.0) * 0.5
    on = (r(B, 1, 1, 1) < 0.8).float()
    alpha = 1.0 + on * (r(B, 1, 1, 1) * 0.4 - 0.2)               # contrast  in [0.8, 1.2]
    beta = on * (r(B, 1, 1, 1) * 0.4 - 0.2)                        # brightness in [-0.2, 0.2]
    x = (x * alpha + beta * x.mean((1, 2, 3), keepdim=True)).clamp(0, 1)
    gray = x.mean(1, keepdim=True)
    sat = 1.0 + on * (r(B, 1, 1, 1) * 0.6 - 0.3)
    x = (gray + (x - gray) * sat).clamp(0, 1)
    tg = (r(B, 1, 1, 1) < 0.2).float()
    x = tg * gray.expand_as(x) + (1 - tg) * x
    k = torch.tensor([1., 4., 6., 4., 1.], device=dev)
    k = (k[:, None] * k[None, :] / 256.0).expand(3, 1, 5, 5)
    blur = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect"), k, groups=3)
    bl = (r(B, 1, 1, 1) < 0.5).float()
    x = bl * blur + (1 - bl) * x
    return x * 2.0 - 1.0


def consistency_threshold(epoch, rampup=200):
    import math
    phase = 1.0 - min(max(float(epoch), 0.0), rampup) / rampup
    return (0.85 + 0.25 * math.exp(-5.0 * phase * phase)) * math.log(2.0)


def consistency_loss(oT_aug, oT, mask_0, mask_1, epoch, aug_weight=1.0):
    """aug_weight * sum(mask * BCE(sigmoid(oT_aug), [sigmoid(oT) > tau(epoch)])) / sum(mask), mask = nearest-
    upsampled cat(mask_0, mask_1) (parity unpinned).  Elementwise torch ops on
    two 512x512x2 maps per image - not worth a kernel of their own yet."""
    F = torch.nn.functional
    y = (torch.sigmoid(oT.detach()) > consistency_threshold(epoch)).to(oT.dtype)
    mask = F.interpolate(torch.cat((mask_0, mask_1), 1), size=oT.shape[2:], mode="nearest")
    bce = F.binary_cross_entropy(torch.sigmoid(oT_aug), y, reduction="none")
    return aug_weight * (mask * bce).sum() / mask.sum().clamp_min(1e-12)


def seg_counts(pred, target, thr=0.75):
    """int64 [C,3] on the host: (intersection, predicted, ground truth) for sigmoid(pred) > thr."""
    return kernels().seg_counts(pred.detach().contiguous().float(), target.detach().contiguous().float(), thr).cpu()


def _mask_u8(m):
    """[B,2,H,W] uint8 / bool / float mask -> uint8 0/1 (set means > 0.5, which for uint8 and bool is nonzero)."""
    if m.dim() != 4 or m.shape[1] != 2:
        raise ValueError("expected a [B, 2, H, W] mask, got %s" % (tuple(m.shape),))
    return (m if m.dtype == torch.bool else m > 0.5).to(torch.uint8).contiguous()


def _to_device(*tensors):
    """the tensors on one device: that of the first device tensor among them, else cuda (CPU tensors are moved there)"""
    if not any(t.is_cuda for t in tensors) and not torch.cuda.is_available():
        raise RuntimeError("uda_clr_amd computes only on the MI355X HIP kernels (there is no CPU fallback)")
    dev = next((t.device for t in tensors if t.is_cuda), torch.device("cuda"))
    return [t.detach().to(dev) for t in tensors]


def display_masks(prob, threshold=0.75):
    """[B,2,H,W] (cup, disc) probabilities -> uint8 [B,2,H,W] display masks on the device, the chain of the reference's
    ``save_per_img`` (utils/Utils.py:523-553): the outermost pixel ring read as 0, ``> threshold`` for both channels whatever the
    dataset, five 7x7 medians, diamond(7) erosion, largest component, fill, diamond(7) dilation, fill.  ``prob`` is not modified
    (the reference zeroes the ring in the caller's array).  Runs on the device (uda_display_masks); a CPU tensor is moved there."""
    if prob.dim() != 4 or prob.shape[1] != 2:
        raise ValueError("expected [B, 2, H, W] probabilities, got %s" % (tuple(prob.shape),))
    (prob,) = _to_device(prob)
    return kernels().display_masks(prob.contiguous().float(), threshold)


def overlay(image, prob_or_masks):
    """The reference's contour picture (utils/Utils.py:556-580) of a batch on the device -> uint8 [B,H,W,3]: the outline of channel
    1 (disc) in (0, 255, 0), that of channel 0 (cup) in (0, 0, 255) over it, three pixels wide, the image elsewhere.
        image          float [B,3,H,W] in [-1, 1] (bytes = clip(rint((x + 1) * 127.5), 0, 255)) or uint8 [B,H,W,3]
        prob_or_masks  [B,2,H,W]: floating point = probabilities, run through ``display_masks``; uint8 or bool = masks, used as is
    Outline pixels that would fall outside the image are dropped.  Neither argument is modified."""
    if prob_or_masks.dim() != 4 or prob_or_masks.shape[1] != 2:
        raise ValueError("expected [B, 2, H, W] probabilities or masks, got %s" % (tuple(prob_or_masks.shape),))
    image, second = _to_device(image, prob_or_masks)
    K = kernels()
    if image.dtype == torch.uint8:
        if image.dim() != 4 or image.shape[3] != 3:
            raise ValueError("a uint8 image is [B, H, W, 3], got %s" % (tuple(image.shape),))
        image = image.contiguous()
    elif image.is_floating_point():
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError("a float image is [B, 3, H, W], got %s" % (tuple(image.shape),))
        image = K.image_u8(image.contiguous().float())
    else:
        raise ValueError("overlay: image must be float [B, 3, H, W] or uint8 [B, H, W, 3], got %s" % image.dtype)
    if second.is_floating_point():
        masks = K.display_masks(second.contiguous().float())
    elif second.dtype in (torch.uint8, torch.bool):
        masks = second.to(torch.uint8).contiguous()
    else:
        raise ValueError("overlay: probabilities (floating point) or masks (uint8 / bool), got %s" % second.dtype)
    return K.overlay_u8(image, masks)


def surface_distances(pred_mask, gt_mask):
    """Per image and class (cup, disc) the surface-distance table and the Dice counts of a [B,2,H,W] mask pair (uint8, bool or
    float; set means > 0.5), on the host after one synchronising copy:
        table  float64 [B,2,2,3]: direction 0 = pred -> gt, 1 = gt -> pred; (n border pixels, sum of their distances to the other
               border, max squared distance); (n, NaN, -1) where either border set is empty
        counts int64 [B,2,3]: |pred & gt|, |pred|, |gt|
    as numpy arrays (``utils.metrics.surface_metrics_from_table`` / ``dice_per_image`` turn them into ASD, ASSD, HD and Dice).
    Runs on the device (uda_surface_distance); CPU tensors are moved there."""
    pred_mask, gt_mask = _to_device(pred_mask, gt_mask)
    packed = kernels().surface_distance(_mask_u8(pred_mask), _mask_u8(gt_mask), want_packed=True)[-1]
    t = hip.unpack_host(hip.surface_layout(pred_mask.shape[0]), packed.cpu().numpy())                  # the one copy (it synchronises)
    return t["table"], t["counts"]


def surface_profile(pred_mask, gt_mask, percentiles=(95,), tolerances=()):
    """``surface_distances`` plus what a percentile of the surface distances (hd95), the surface Dice at a tolerance and the vertical
    cup-to-disc ratio are closed forms of, on the host after ONE synchronising copy.  Masks as ``surface_distances``.
        percentiles  in [0, 100]; the kernel takes quantiles = np.true_divide(percentiles, 100)
        tolerances   tau >= 0 in pixels; a border pixel is within tau when its squared distance d2 <= floor(tau * tau) (float64):
                     d2 is an integer, so that is d2 <= tau^2
    -> table, counts as ``surface_distances``, and profile = {
        'order'   int64 [B,2,3,Q,2]: set 0 = pred -> gt, 1 = gt -> pred, 2 = both pooled; the lo-th and hi-th smallest squared distance
                  around the virtual index (n - 1) * q; -1 where either border set is empty
        'within'  int64 [B,2,2,T]: per direction the border pixels within each tolerance; -1 where either border set is empty
        'extent'  int64 [B,2,2,2]: per mask (0 ground truth, 1 prediction) the first and last row with a set pixel; -1 if empty
        'quantiles' float64 [Q], 'tolerances' float64 [T], 'tol2' int64 [T]: what was used}
    (``utils.metrics.percentile_distance_from_profile`` / ``surface_dice_from_profile`` / ``vertical_cdr_from_profile``).
    Runs on the device (uda_surface_profile); CPU tensors are moved there."""
    import numpy as np
    quantiles = np.true_divide(np.asarray(list(percentiles), np.float64), 100)
    tol = np.asarray(list(tolerances), np.float64)
    if not np.all((quantiles >= 0) & (quantiles <= 1)):
        raise ValueError("surface_profile: percentiles must lie in [0, 100], got %r" % (tuple(percentiles),))
    if not np.all((tol >= 0) & (tol * tol < 2.0 ** 31)):
        raise ValueError("surface_profile: tolerances must be non-negative pixel distances, got %r" % (tuple(tolerances),))
    tol2 = np.floor(tol * tol).astype(np.int64)
    pred_mask, gt_mask = _to_device(pred_mask, gt_mask)
    packed = kernels().surface_profile(_mask_u8(pred_mask), _mask_u8(gt_mask), quantiles.tolist(), tol2.tolist(), want_packed=True)[-1]
    t = hip.unpack_host(hip.profile_layout(pred_mask.shape[0], len(quantiles), len(tol)), packed.cpu().numpy())   # the one copy (it synchronises)
    return t.pop("table"), t.pop("counts"), dict(t, quantiles=quantiles, tolerances=tol, tol2=tol2)


def disc_morphometry(masks, sectors=72):
    """The integers of the optic-disc morphometry of a [B,2,H,W] (cup, disc) mask batch (uint8, bool or float; set means > 0.5), on the
    host after ONE synchronising copy:
        sectors   K (a multiple of 8 in 8..360; the table is ``utils.metrics.sector_table(K)``), or an int64 [K,2] table of boundary
                  rays (x right, y up, strictly counter-clockwise, |x|, |y| <= 2^30)
    -> {'moments' int64 [B,2,6]: per class n, sum r, sum c, sum r^2, sum c^2, sum r*c over the set pixels (row r, column c)
        'extent'  int64 [B,2,4]: first row, last row, first column, last column with a set pixel; -1 for an empty plane
        'overlap' int64 [B]: pixels set in both planes
        'radial'  int64 [B,2,K]: per sector about the DISC centroid the largest ux^2 + uy^2 of u = (n c - sum c, -(n r - sum r)) with
                  the disc's n and sums (sqrt / n is a distance in pixels); -1 for a sector without a pixel, and without a disc
        'table'   int64 [K,2]: the sector table that was used}
    as numpy arrays (``utils.metrics.morphometry_from_moments`` turns them into the CDR family, the rim profile, the cup's decentration
    and the ellipse summaries).  Runs on the device (uda_disc_morphometry); a CPU tensor is moved there."""
    import numpy as np
    from .utils.metrics import sector_table
    table = sector_table(sectors) if isinstance(sectors, (int, np.integer)) else np.ascontiguousarray(np.asarray(sectors), dtype=np.int64)
    if table.ndim != 2 or table.shape[1] != 2 or table.shape[0] % 8 or not 8 <= table.shape[0] <= 360:
        raise ValueError("disc_morphometry: sectors is K or an int64 [K, 2] table, K a multiple of 8 in 8..360 (got shape %s)" % (table.shape,))
    if np.abs(table).max() > 2 ** 30:
        raise ValueError("disc_morphometry: sector table entries must lie within +-2^30")
    if masks.dim() != 4 or masks.shape[1] != 2:
        raise ValueError("expected a [B, 2, H, W] mask, got %s" % (tuple(masks.shape),))
    (masks,) = _to_device(masks)
    packed = kernels().disc_morphometry(_mask_u8(masks), torch.from_numpy(table).to(masks.device), want_packed=True)[-1]
    t = hip.unpack_host(hip.morphometry_layout(masks.shape[0], table.shape[0]), packed.cpu().numpy())   # the one copy (it synchronises)
    return dict(t, table=table)


# uncertainty bins of the selective-prediction table: 0.04 is the trainer's trust threshold on the std of sigmoid(x / 2)
# (reference utils/Utils.py:197-200)
DEFAULT_UNC_EDGES = (0.005, 0.01, 0.02, 0.03, 0.04, 0.06, 0.08, 0.12, 0.16)


def mc_uncertainty(logits, outputs=("mean", "std", "entropy", "mi"), u8_scale=None):
    """[T,B,2,H,W] logits of T stochastic passes (2 <= T <= 32) -> {name: [B,2,H,W] device tensor} for the names in ``outputs``, one
    read of the logits (uda_mc_uncertainty):
        'mean'     mean over the passes of sigmoid(x)
        'std'      unbiased std over the passes of sigmoid(x / 2): the quantity ``gen_prototype_retrify`` thresholds at 0.04
        'entropy'  binary entropy of 'mean' in nats
        'mi'       'entropy' minus the mean entropy of the passes (>= 0): the part of the entropy that the passes disagree about
    and with ``u8_scale`` also 'std_u8' = min(255, floor(std * u8_scale)) as uint8, from the stored fp32 std.  A CPU tensor is moved
    to the device."""
    if logits.dim() < 2:
        raise ValueError("expected [T, ...] logits, got %s" % (tuple(logits.shape),))
    (logits,) = _to_device(logits)
    return kernels().mc_uncertainty(logits.contiguous().float(), outputs, u8_scale)


def selective_tables(prob, unc, pred, gt=None, bins=15, edges=DEFAULT_UNC_EDGES):
    """The integer tables that calibration and selective-prediction figures are closed forms of, per image and class of a [B,2,H,W]
    batch, on the host after ONE synchronising copy (uda_selective_tables):
        prob   probabilities, or None (no reliability table)          unc    uncertainties >= 0, or None (no risk table)
        pred   masks (uint8, bool or float; set means > 0.5)          gt     masks, or None: taken as ``pred``
        bins   M confidence bins, 1..64                               edges  K - 1 ascending finite values, K <= 64
    -> {'rel'     int64 [B,2,M,5]: per bin min(M - 1, floor(p * M)) (fp32): n, n with gt set, sum q, sum q over gt-set pixels, sum q^2,
                  q = rint(p * 65536); None without ``prob``
        'risk'    int64 [B,2,K,4]: per bin #{j: edges[j] <= u}: TP, FP, FN, TN of pred against gt; None without ``unc``
        'invalid' int64 [B,2,2]: pixels with p NaN or outside [0, 1], pixels with u NaN or negative - left out of that table only
        'edges'   float32 [K - 1]: the edges as the kernel compared them}
    as numpy arrays (``utils.metrics.calibration_from_table`` / ``selective_from_table``).  CPU tensors are moved to the device."""
    import numpy as np
    e32 = np.asarray(list(edges), np.float32)
    if not 1 <= int(bins) <= 64 or e32.size > 63:
        raise ValueError("selective_tables: 1..64 bins (got %d confidence, %d uncertainty)" % (bins, e32.size + 1))
    if not np.all(np.isfinite(e32)) or not np.all(e32[1:] > e32[:-1]):
        raise ValueError("selective_tables: edges must be finite and strictly ascending as float32, got %r" % (tuple(edges),))
    if prob is None and unc is None:
        raise ValueError("selective_tables: prob (reliability table), unc (risk table) or both")
    given = [t for t in (prob, unc, pred, gt) if t is not None]
    moved = iter(_to_device(*given))
    prob, unc, pred, gt = (None if t is None else next(moved) for t in (prob, unc, pred, gt))
    f32 = lambda t: None if t is None else t.contiguous().float()
    packed = kernels().selective_tables(f32(prob), f32(unc), _mask_u8(pred), None if gt is None else _mask_u8(gt), int(bins), e32.tolist(),
                                        want_packed=True)[-1]
    layout = hip.selective_layout(pred.shape[0], int(bins), e32.size + 1, prob is not None, unc is not None)
    t = hip.unpack_host(layout, packed.cpu().numpy())                                                    # the one copy (it synchronises)
    return {"rel": t.get("rel"), "risk": t.get("risk"), "invalid": t["invalid"], "edges": e32}


def tta_view(image, view):
    """The input of one test-time-augmentation view of a [B,C,H,W] image (1 <= C <= 4; H, W multiples of 16 in 16..1024), on the
    device (uda_tta_view).  ``view`` = (g, h, w), h and w multiples of 16 in 16..1024:
        R = F.interpolate(image, (h, w), mode='bilinear', align_corners=True)          (the image itself where (h, w) == (H, W))
        g & 1  mirrored left-right, g & 2 mirrored top-bottom, then g & 4 transposed:  0 identity, 1 hflip, 2 vflip, 3 rot180,
        4 transpose, 5 torch.rot90(R, 1, (-2, -1)), 6 torch.rot90(R, -1, (-2, -1)), 7 anti-transpose
    -> float32 [B,C,h,w], or [B,C,w,h] for g & 4.  A CPU tensor is moved to the device."""
    if image.dim() != 4:
        raise ValueError("tta_view: expected a [B, C, H, W] image, got %s" % (tuple(image.shape),))
    (image,) = _to_device(image)
    return kernels().tta_view(image.contiguous().float(), view)


def tta_fuse(view_logits, views, size, outputs=("mean",), u8_scale=None):
    """The logits of V views (2 <= V <= 32) of one [B,C,H,W] batch, mapped back to the image's frame and reduced over the views, in one
    read of the logits (uda_tta_fuse):
        view_logits  V tensors, the model's logits on ``tta_view(image, views[v])``: [B,C,h,w], or [B,C,w,h] for a transposed view
        views        V triples (g, h, w) as ``tta_view`` takes them          size  (H, W) of the frame
    Per view the transpose is undone, then the mirrorings, then (h, w) is resampled to (H, W) with align_corners=True (a view of the
    frame's size is read as it is stored).  -> {name: [B,C,H,W] device tensor} for the names in ``outputs``, the maps of
    ``mc_uncertainty`` with the views in the place of the passes: 'mean' (the fused probability), 'std' (of sigmoid(x / 2) over the
    views), 'entropy', 'mi', and with ``u8_scale`` 'std_u8'.  CPU tensors are moved to the device."""
    import math
    view_logits = list(view_logits)
    if u8_scale is not None and not (0.0 < float(u8_scale) < math.inf):
        raise ValueError("tta_fuse: u8_scale must be a positive finite number, got %r" % (u8_scale,))
    given = [t for t in view_logits if t is not None]
    moved = iter(_to_device(*given)) if given else iter(())
    view_logits = [None if t is None else next(moved).contiguous().float() for t in view_logits]
    return kernels().tta_fuse(view_logits, views, size, outputs, u8_scale)
