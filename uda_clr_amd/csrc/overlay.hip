// Prediction pictures on the device: the contour overlay of utils/Utils.py:556-580 (save_per_img) and the byte image it is
// painted on.
//
//   uda_overlay_u8   For {0,1} masks at level 0.5 the vertices of skimage.measure.find_contours are the midpoints of all
//       4-adjacent pixel pairs with different values, both pixels inside the image: (r + 0.5, c) between (r, c) and (r + 1, c),
//       (r, c + 0.5) between (r, c) and (r, c + 1).  Per vertex (y, x) the reference paints the seven pixels (int(y + dy), int(x + dx)),
//       (dy, dx) in (0,0) (1,0) (1,1) (0,1) (-1,0) (-1,-1) (0,-1), int() truncating towards zero.  Restated as a gather:
//       a vertex between (r0, c0) and its lower (or right) neighbour reaches (r0 + a, c0 + b) for (a, b) in the same seven
//       offsets - the half pixel is truncated away, and at r0 = 0 (c0 = 0) the truncation towards zero sends the two "-1" targets
//       to row (column) 0, onto targets the vertex already has.  So output pixel (r, c) is painted by channel k exactly when
//       one of the pairs anchored at (r - a, c - b) differs in mask k.  A target outside the image has no output pixel: it is
//       dropped, where the reference raises (index H or W) or wraps (index -1) - the one deliberate departure.
//       Channel 0 (cup) paints (0, 0, 255) over channel 1 (disc), (0, 255, 0), as the reference's two loops do.
//       One thread per output pixel, the masks staged in LDS with a 2-pixel halo; no scatter, no atomics, every output byte is
//       written exactly once from values that depend on the image's own planes only.
//   uda_image_u8     NCHW float in [-1, 1] -> NHWC uint8 = clip(rint((x + 1) * 127.5), 0, 255) in fp32, add and multiply rounded
//       separately (no fma), ties to even as numpy's rint.
//
// Byte work on evaluation-sized planes, not on the training path.
#include "common.h"

#define OV_T 32
#define OV_HALO 2
#define OV_S (OV_T + 2 * OV_HALO)
#define OV_OUTSIDE 2        // staged value of a position outside the image: x ^ y == 1 only for two in-image pixels that differ

__global__ __launch_bounds__(256) void overlay_u8_kernel(const uint8_t* __restrict__ image, const uint8_t* __restrict__ masks, int H,
                                                         int W, uint8_t* __restrict__ out) {
    __shared__ uint8_t t[2][OV_S][OV_S + 4];
    const int b = blockIdx.z, h0 = blockIdx.y * OV_T, w0 = blockIdx.x * OV_T;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* M = masks + (int64_t)b * 2 * HW;
    for (int e = threadIdx.x; e < 2 * OV_S * OV_S; e += 256) {
        const int k = e / (OV_S * OV_S), q = e % (OV_S * OV_S);
        const int r = q / OV_S, c = q % OV_S;
        const int h = h0 + r - OV_HALO, w = w0 + c - OV_HALO;
        t[k][r][c] = (h >= 0 && h < H && w >= 0 && w < W) ? (M[k * HW + (int64_t)h * W + w] ? 1 : 0) : OV_OUTSIDE;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < OV_T * OV_T; e += 256) {
        const int r = e / OV_T, c = e % OV_T;
        const int h = h0 + r, w = w0 + c;
        if (h >= H || w >= W) continue;
        bool hit[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            // anchors (r - a, c - b) for the seven offsets (a, b): rows r-1 .. r+1, columns c-1 .. c+1 without the two
            // anti-diagonal corners; each anchor's down pair and right pair
            bool any = false;
#pragma unroll
            for (int a = -1; a <= 1; ++a)
#pragma unroll
                for (int bb = -1; bb <= 1; ++bb) {
                    if (a * bb < 0) continue;                        // (1,-1) and (-1,1) are not among the offsets
                    const int y = r - a + OV_HALO, x = c - bb + OV_HALO;
                    const int v = t[k][y][x];
                    any = any || ((v ^ t[k][y + 1][x]) == 1) || ((v ^ t[k][y][x + 1]) == 1);
                }
            hit[k] = any;
        }
        const int64_t o = (((int64_t)b * H + h) * W + w) * 3;
        uint8_t p0, p1, p2;
        if (hit[0]) { p0 = 0; p1 = 0; p2 = 255; }
        else if (hit[1]) { p0 = 0; p1 = 255; p2 = 0; }
        else { p0 = image[o]; p1 = image[o + 1]; p2 = image[o + 2]; }
        out[o] = p0;
        out[o + 1] = p1;
        out[o + 2] = p2;
    }
}

__global__ __launch_bounds__(256) void image_u8_kernel(const float* __restrict__ x, int64_t HW, uint8_t* __restrict__ out) {
    const int b = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float v = rintf(__fmul_rn(__fadd_rn(x[((int64_t)b * 3 + ch) * HW + p], 1.0f), 127.5f));
        out[((int64_t)b * HW + p) * 3 + ch] = (uint8_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);      // NaN -> 0
    }
}

static bool ov_overlap(const void* a, const void* b, int64_t n) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + (uintptr_t)n && y < x + (uintptr_t)n;
}

extern "C" int uda_overlay_u8(const uint8_t* image, const uint8_t* masks, int B, int H, int W, uint8_t* out, void* stream) {
    UDA_REQUIRE(image && masks && out && B > 0 && H > 0 && W > 0, "uda_overlay_u8: bad args");
    UDA_REQUIRE((int64_t)H * W < ((int64_t)1 << 30) && B <= 65535, "uda_overlay_u8: plane or batch too large");
    UDA_REQUIRE(!ov_overlap(image, out, (int64_t)B * H * W * 3), "uda_overlay_u8: out may not alias image");
    const dim3 tiles(uda_cdiv(W, OV_T), uda_cdiv(H, OV_T), B);
    UDA_REQUIRE(tiles.y <= 65535, "uda_overlay_u8: plane too high");
    hipLaunchKernelGGL(overlay_u8_kernel, tiles, dim3(256), 0, (hipStream_t)stream, image, masks, H, W, out);
    UDA_LAUNCH_CHECK("overlay_u8");
    return 0;
}

extern "C" int uda_image_u8(const float* x, int B, int H, int W, uint8_t* out, void* stream) {
    UDA_REQUIRE(x && out && B > 0 && H > 0 && W > 0, "uda_image_u8: bad args");
    UDA_REQUIRE((int64_t)H * W < ((int64_t)1 << 30) && B <= 65535, "uda_image_u8: plane or batch too large");
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(image_u8_kernel, dim3(uda_cdiv(HW, 256), B), dim3(256), 0, (hipStream_t)stream, x, HW, out);
    UDA_LAUNCH_CHECK("image_u8");
    return 0;
}
