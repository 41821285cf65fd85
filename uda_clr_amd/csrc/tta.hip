// Test-time augmentation at evaluation (include/uda_clr_hip.h): the image is predicted under V views - the eight
// mirrorings / quarter turns of the square's symmetry group (D4) at a few sizes - and the V logit tensors are mapped back to the
// image's frame and reduced per element by the statistics of uda_mc_uncertainty (unc_element.h: the same code, the same bits).
//
// A view (g, h, w): R = bilinear(image -> (h, w)), align_corners=True (bilinear.h);  F[i][j] = R[g & 2 ? h-1-i : i][g & 1 ? w-1-j : j];
// U = F, or for g & 4 its transpose U[i][j] = F[j][i] ([w][h]).  The inverse undoes the transpose, then the mirrorings, then
// resamples (h, w) -> (H, W).  A view of the frame's own size moves values only: no arithmetic touches them in either direction.
//
//   uda_tta_view   one workgroup per 32 x 32 tile of U, a thread per 4 neighbours of a row: 16-byte stores, and 16-byte loads where
//       the view is a permutation.  A transposed view is formed in F's orientation (reads along the image's rows), handed over
//       through a 32 x 33 LDS tile and stored along U's rows: neither side walks a column.
//   uda_tta_fuse   one workgroup per 32 x 32 tile of the frame and (image, channel) plane, a thread per 4 neighbours of a row with
//       the V values of each in registers (V is a template argument, as T in unc_kernel).  Views that are not transposed are read
//       where they lie: a row of the frame is a row of the view, forwards or backwards.  Of a transposed view the workgroup first
//       copies the rectangle of stored logits its tile needs into LDS - whole row segments of the stored tensor, 128 bytes each for
//       a view of the frame's size - with a pitch of 49 floats (odd: the 32 lanes of a half wave, 8 along x by 4 along y, read 32
//       different banks), and takes its taps there.  A view of the frame's size needs 32 x 32 words: one 16-byte load per thread.
//       Two rectangles are used in turn, so that one barrier per transposed view is enough.  The rectangle of a view up to 1.4
//       times the frame's size fits the 48 x 48 words; a larger one is read from memory tap by tap (right, and slow: a lane per
//       stored row).  The device code is in tta_fuse.h, instantiated by tta_fuse_a/b/c.hip; the entry is here.
#include "tta_fuse.h"

// ------------------------------------------------------------------------------------------------------------ uda_tta_view
// F[i][j .. j + 3] of one plane: the mirrorings act on the index of the (h, w) grid, the taps are the image's
__device__ __forceinline__ void tta_view_row4(const float* __restrict__ img, int H, int W, int g, int h, int w, float sh, float sw, int i, int j,
                                              float (&v)[4]) {
    const int a = tta_flip(i, h, g & 2);
    if (h == H && w == W) {
        tta_ld4(img + (int64_t)a * W, j, W, g & 1, v);
    } else {
        int a0, a1;
        float lh0, lh1;
        bil_src(a, sh, H, a0, a1, lh0, lh1);
        const float* r0 = img + (int64_t)a0 * W;
        const float* r1 = img + (int64_t)a1 * W;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int b0, b1;
            float lw0, lw1;
            bil_src(tta_flip(j + k, w, g & 1), sw, W, b0, b1, lw0, lw1);
            v[k] = tta_lerp(lh0, lh1, lw0, lw1, r0[b0], r0[b1], r1[b0], r1[b1]);
        }
    }
}

// grid (cols of U / 32, rows of U / 32, B C), 256 threads = 32 rows x 8 groups of 4 columns
__global__ __launch_bounds__(256) void tta_view_kernel(const float* __restrict__ img, int H, int W, int g, int h, int w, float sh, float sw,
                                                       float* __restrict__ out) {
    __shared__ float tile[TTA_TILE * (TTA_TILE + 1)];
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const float* src = img + (int64_t)blockIdx.z * H * W;
    float* dst = out + (int64_t)blockIdx.z * h * w;
    float v[4];
    if (!(g & 4)) {                                        // U = F, [h][w]
        const int i = blockIdx.y * TTA_TILE + ty, j = blockIdx.x * TTA_TILE + 4 * tx;
        if (i < h && j < w) {
            tta_view_row4(src, H, W, g, h, w, sh, sw, i, j, v);
            uda_st4(dst + (int64_t)i * w + j, make_float4(v[0], v[1], v[2], v[3]));
        }
        return;
    }
    // U[i][j] = F[j][i], [w][h]: this workgroup's tile is rows i0.. of U = columns i0.. of F, columns j0.. of U = rows j0.. of F
    const int i0 = blockIdx.y * TTA_TILE, j0 = blockIdx.x * TTA_TILE;
    if (j0 + ty < h && i0 + 4 * tx < w) {
        tta_view_row4(src, H, W, g, h, w, sh, sw, j0 + ty, i0 + 4 * tx, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[ty * (TTA_TILE + 1) + 4 * tx + k] = v[k];
    }
    __syncthreads();
    const int i = i0 + ty, j = j0 + 4 * tx;
    if (i < w && j < h) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = tile[(4 * tx + k) * (TTA_TILE + 1) + ty];
        uda_st4(dst + (int64_t)i * h + j, make_float4(v[0], v[1], v[2], v[3]));
    }
}

static int tta_check_size(const char* who, const char* what, int n) {
    UDA_REQUIRE(n >= 16 && n <= TTA_SMAX && n % 16 == 0, "%s: %s %d is not a multiple of 16 in 16..%d", who, what, n, TTA_SMAX);
    return 0;
}

static int tta_check_frame(const char* who, int B, int C, int H, int W) {
    UDA_REQUIRE(B >= 1 && B <= 8192, "%s: batch %d outside 1..8192", who, B);
    UDA_REQUIRE(C >= 1 && C <= 4, "%s: %d channels outside 1..4", who, C);
    if (tta_check_size(who, "H", H) || tta_check_size(who, "W", W)) return 1;
    return 0;
}

static int tta_check_view(const char* who, int v, int g, int h, int w) {
    UDA_REQUIRE(g >= 0 && g <= 7, "%s: view %d: code %d outside 0..7", who, v, g);
    UDA_REQUIRE(h >= 16 && h <= TTA_SMAX && h % 16 == 0 && w >= 16 && w <= TTA_SMAX && w % 16 == 0,
                "%s: view %d: size %d x %d, each side must be a multiple of 16 in 16..%d", who, v, h, w, TTA_SMAX);
    return 0;
}

extern "C" int uda_tta_view(const float* image, int B, int C, int H, int W, int g, int h, int w, float* out, void* stream) {
    const char* who = "uda_tta_view";
    UDA_REQUIRE(image && out, "%s: null argument", who);
    UDA_REQUIRE(uda_aligned16(image) && uda_aligned16(out), "%s: image and out must be 16-byte aligned", who);
    if (int rc = tta_check_frame(who, B, C, H, W)) return rc;
    if (int rc = tta_check_view(who, 0, g, h, w)) return rc;
    const int rows = (g & 4) ? w : h, cols = (g & 4) ? h : w;
    hipLaunchKernelGGL(tta_view_kernel, dim3(uda_cdiv(cols, TTA_TILE), uda_cdiv(rows, TTA_TILE), B * C), dim3(256), 0, (hipStream_t)stream, image, H, W,
                       g, h, w, bil_scale(H, h), bil_scale(W, w), out);
    UDA_LAUNCH_CHECK(who);
    return 0;
}

// ------------------------------------------------------------------------------------------------------------ uda_tta_fuse
extern "C" int uda_tta_fuse(const float* const* logits, const int* g, const int* h, const int* w, int V, int B, int C, int H, int W,
                            float* mean_prob, float* std_half, float* entropy, float* mutual_info, uint8_t* std_u8, float u8_scale,
                            void* stream) {
    const char* who = "uda_tta_fuse";
    UDA_REQUIRE(logits && g && h && w, "%s: null argument", who);
    UDA_REQUIRE(V >= 2 && V <= UNC_TMAX, "%s: %d views outside 2..%d", who, V, UNC_TMAX);
    if (int rc = tta_check_frame(who, B, C, H, W)) return rc;
    UDA_REQUIRE(mean_prob || std_half || entropy || mutual_info || std_u8, "%s: no output asked for", who);
    UDA_REQUIRE(!std_u8 || (u8_scale > 0.f && u8_scale < INFINITY), "%s: u8_scale %g is not a positive finite number", who, (double)u8_scale);
    UDA_REQUIRE((!mean_prob || uda_aligned16(mean_prob)) && (!std_half || uda_aligned16(std_half)) && (!entropy || uda_aligned16(entropy)) &&
                    (!mutual_info || uda_aligned16(mutual_info)) && (reinterpret_cast<uintptr_t>(std_u8) & 3u) == 0,
                "%s: the float outputs must be 16-byte aligned, std_u8 4-byte aligned", who);
    TtaViews vw;
    for (int v = 0; v < UNC_TMAX; ++v) {
        vw.p[v] = nullptr;
        vw.sh[v] = vw.sw[v] = 0.f;
        vw.g[v] = vw.h[v] = vw.w[v] = 0;
    }
    for (int v = 0; v < V; ++v) {
        UDA_REQUIRE(logits[v], "%s: view %d: null logits", who, v);
        UDA_REQUIRE(uda_aligned16(logits[v]), "%s: view %d: logits must be 16-byte aligned", who, v);
        if (int rc = tta_check_view(who, v, g[v], h[v], w[v])) return rc;
        vw.p[v] = logits[v];
        vw.g[v] = (short)g[v], vw.h[v] = (short)h[v], vw.w[v] = (short)w[v];
        vw.sh[v] = bil_scale(h[v], H), vw.sw[v] = bil_scale(w[v], W);
    }
    UncOut o = {mean_prob, std_half, entropy, mutual_info, std_u8, u8_scale, (entropy || mutual_info) ? 1 : 0};
    const dim3 grid(uda_cdiv(W, TTA_TILE), uda_cdiv(H, TTA_TILE), B * C);
    if (V <= TTA_FUSE_A_LAST)
        tta_fuse_launch_a(V, grid, (hipStream_t)stream, vw, H, W, o);
    else if (V <= TTA_FUSE_B_LAST)
        tta_fuse_launch_b(V, grid, (hipStream_t)stream, vw, H, W, o);
    else
        tta_fuse_launch_c(V, grid, (hipStream_t)stream, vw, H, W, o);
    UDA_LAUNCH_CHECK(who);
    return 0;
}
