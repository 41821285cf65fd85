// The device code of uda_tta_fuse (tta.hip has the account): shared by tta.hip, which has the entry, and tta_fuse_a/b/c.hip, which
// instantiate the kernel for 2..18, 19..26 and 27..32 views - three translation units of about equal work, so that the 31
// instantiations compile side by side and not one after the other.
#pragma once
#include "common.h"
#include "bilinear.h"
#include "unc_element.h"

#define TTA_TILE 32
#define TTA_STAGE 48             // rows and columns of stored logits that the LDS rectangle holds at most
#define TTA_PITCH 49
#define TTA_SMAX 1024            // largest side of the frame and of a view

__device__ __forceinline__ int tta_flip(int i, int n, int on) { return on ? n - 1 - i : i; }

// resample.hip's lerp, every product and sum rounded on its own: the tap-by-tap path and the LDS path give the same bits
__device__ __forceinline__ float tta_lerp(float lh0, float lh1, float lw0, float lw1, float a00, float a01, float a10, float a11) {
#pragma clang fp contract(off)
    return lh0 * (lw0 * a00 + lw1 * a01) + lh1 * (lw0 * a10 + lw1 * a11);
}

__device__ __forceinline__ void tta_ld4(const float* row, int j, int n, int reversed, float (&v)[4]) {
    const float4 q = uda_ld4(row + (reversed ? n - 4 - j : j));
    v[0] = reversed ? q.w : q.x, v[1] = reversed ? q.z : q.y, v[2] = reversed ? q.y : q.z, v[3] = reversed ? q.x : q.w;
}


// ------------------------------------------------------------------------------------------------------------ uda_tta_fuse
struct TtaViews {                // by value: 704 bytes of kernel arguments
    const float* p[UNC_TMAX];
    float sh[UNC_TMAX], sw[UNC_TMAX];
    short g[UNC_TMAX], h[UNC_TMAX], w[UNC_TMAX];
};

// z[k] = the view's logit in the frame at (y, x + k), k = 0..3, of one plane L of the stored tensor.  (y0, x0): the workgroup's tile;
// (y, x) lies in it and in the frame for every thread (the caller clamps), and every thread of the workgroup comes here: the LDS
// path has a barrier.  g, h, w, sh, sw are the same for the whole workgroup.  stage: two LDS rectangles, used in turn (half says which
// is next): a thread that writes one has passed the barrier of the view before, which every thread reaches only after it has taken
// its taps from this rectangle two views ago - one barrier per transposed view, and the next view's loads need not wait for it.
__device__ __forceinline__ void tta_gather4(const float* __restrict__ L, int g, int h, int w, float sh, float sw, int H, int W, int y, int x,
                                            int y0, int x0, float* stage, int& half, float (&z)[4]) {
    const bool same = h == H && w == W;
    if (!(g & 4)) {                                        // stored [h][w]: the mirrorings act on the taps' indices
        if (same) {
            tta_ld4(L + (int64_t)tta_flip(y, h, g & 2) * w, x, w, g & 1, z);
        } else {
            int a0, a1;
            float lh0, lh1;
            bil_src(y, sh, h, a0, a1, lh0, lh1);
            const float* r0 = L + (int64_t)tta_flip(a0, h, g & 2) * w;
            const float* r1 = L + (int64_t)tta_flip(a1, h, g & 2) * w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int b0, b1;
                float lw0, lw1;
                bil_src(x + k, sw, w, b0, b1, lw0, lw1);
                const int c0 = tta_flip(b0, w, g & 1), c1 = tta_flip(b1, w, g & 1);
                z[k] = tta_lerp(lh0, lh1, lw0, lw1, r0[c0], r0[c1], r1[c0], r1[c1]);
            }
        }
        return;
    }
    // stored [w][h]: tap (a, b) of the (h, w) grid is L[p][q], p = flip(b), q = flip(a).  The taps of the tile: a in [alo, ahi], b in
    // [blo, bhi] (bil_src's indices do not decrease with the output index), i.e. the rectangle p in plo.., q in qlo.. of L
    const int y1 = min(y0 + TTA_TILE - 1, H - 1), x1 = min(x0 + TTA_TILE - 1, W - 1);
    int alo = y0, ahi = y1, blo = x0, bhi = x1;
    if (!same) {
        int t;
        float f0, f1;
        bil_src(y0, sh, h, alo, t, f0, f1);
        bil_src(y1, sh, h, t, ahi, f0, f1);
        bil_src(x0, sw, w, blo, t, f0, f1);
        bil_src(x1, sw, w, t, bhi, f0, f1);
    }
    const int qlo = (g & 2) ? h - 1 - ahi : alo, nq = ahi - alo + 1;
    const int plo = (g & 1) ? w - 1 - bhi : blo, np = bhi - blo + 1;
    const bool staged = np <= TTA_STAGE && nq <= TTA_STAGE;
    if (staged) {
        stage += half * (TTA_STAGE * TTA_PITCH);
        half ^= 1;
        if (same) {                                        // at most 32 x 32 words, qlo and nq multiples of 4 (H % 16 == 0): one 16-byte load a thread
            const int p = threadIdx.x >> 3, q = (threadIdx.x & 7) * 4;
            if (p < np && q < nq) {
                const float4 v = uda_ld4(L + (int64_t)(plo + p) * h + qlo + q);
                float* s = stage + p * TTA_PITCH + q;
                s[0] = v.x, s[1] = v.y, s[2] = v.z, s[3] = v.w;
            }
        } else {
            for (int e = threadIdx.x; e < np * nq; e += 256) {
                const int p = e / nq, q = e - p * nq;
                stage[p * TTA_PITCH + q] = L[(int64_t)(plo + p) * h + qlo + q];
            }
        }
        __syncthreads();
    }
    auto tap = [&](int a, int b) -> float {
        const int p = tta_flip(b, w, g & 1), q = tta_flip(a, h, g & 2);
        return staged ? stage[(p - plo) * TTA_PITCH + (q - qlo)] : L[(int64_t)p * h + q];
    };
    if (same) {
#pragma unroll
        for (int k = 0; k < 4; ++k) z[k] = tap(y, x + k);
    } else {
        int a0, a1;
        float lh0, lh1;
        bil_src(y, sh, h, a0, a1, lh0, lh1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int b0, b1;
            float lw0, lw1;
            bil_src(x + k, sw, w, b0, b1, lw0, lw1);
            z[k] = tta_lerp(lh0, lh1, lw0, lw1, tap(a0, b0), tap(a0, b1), tap(a1, b0), tap(a1, b1));
        }
    }
}

// views V0 .. T - 1 into z, one after the other.  A recursion and not a loop: every view's index is a constant whatever the optimiser
// makes of a body with barriers, so z stays in registers
template <int T, int V0>
__device__ __forceinline__ void tta_gather_views(const TtaViews& vw, int64_t plane, int H, int W, int y, int x, int y0, int x0, float* stage,
                                                 int& half, float (&z)[T][4]) {
    if constexpr (V0 < T) {
        const int h = vw.h[V0], w = vw.w[V0];
        tta_gather4(vw.p[V0] + plane * h * w, vw.g[V0], h, w, vw.sh[V0], vw.sw[V0], H, W, y, x, y0, x0, stage, half, z[V0]);
        tta_gather_views<T, V0 + 1>(vw, plane, H, W, y, x, y0, x0, stage, half, z);
    }
}

// grid (W / 32, H / 32, B C) rounded up, 256 threads = 32 rows x 8 groups of 4 columns
template <int T>
__global__ __launch_bounds__(256) void tta_fuse_kernel(TtaViews vw, int H, int W, UncOut o) {
    __shared__ float stage[2 * TTA_STAGE * TTA_PITCH];
    const int tx = threadIdx.x & 7, ty = threadIdx.x >> 3;
    const int x0 = blockIdx.x * TTA_TILE, y0 = blockIdx.y * TTA_TILE;
    const int x = x0 + 4 * tx, y = y0 + ty;
    const bool active = x < W && y < H;                    // W % 16 == 0: a thread's 4 columns are inside together
    const int xc = min(x, W - 4), yc = min(y, H - 1);      // a thread outside still helps to fill the LDS rectangle; its taps stay inside
    const int64_t plane = blockIdx.z;
    float z[T][4];
    int half = 0;
    tta_gather_views<T, 0>(vw, plane, H, W, yc, xc, y0, x0, stage, half, z);
    if (!active) return;                                  // behind the last barrier
    float r[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float c[T], rj[4];
#pragma unroll
        for (int t = 0; t < T; ++t) c[t] = z[t][j];
        unc_element<T>(c, o.full, rj);
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k][j] = rj[k];
    }
    const int64_t at = (plane * H + y) * W + x;
    float* const outs[4] = {o.mean, o.std_half, o.entropy, o.mi};
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (outs[k]) uda_st4(outs[k] + at, make_float4(r[k][0], r[k][1], r[k][2], r[k][3]));
    if (o.u8)
        *reinterpret_cast<unsigned*>(o.u8 + at) = unc_u8(r[1][0], o.u8_scale) | unc_u8(r[1][1], o.u8_scale) << 8 | unc_u8(r[1][2], o.u8_scale) << 16 |
                                                  unc_u8(r[1][3], o.u8_scale) << 24;
}

template <int T, int LAST>
static void tta_dispatch(int V, dim3 grid, hipStream_t st, const TtaViews& vw, int H, int W, const UncOut& o) {
    if (V == T)
        hipLaunchKernelGGL((tta_fuse_kernel<T>), grid, dim3(256), 0, st, vw, H, W, o);
    else if constexpr (T < LAST)
        tta_dispatch<T + 1, LAST>(V, grid, st, vw, H, W, o);
}

// the launchers of the three pieces: each takes the view counts FIRST..LAST and does nothing for another
#define TTA_FUSE_A_LAST 18
#define TTA_FUSE_B_LAST 26
void tta_fuse_launch_a(int V, dim3 grid, hipStream_t st, const TtaViews& vw, int H, int W, const UncOut& o);
void tta_fuse_launch_b(int V, dim3 grid, hipStream_t st, const TtaViews& vw, int H, int W, const UncOut& o);
void tta_fuse_launch_c(int V, dim3 grid, hipStream_t st, const TtaViews& vw, int H, int W, const UncOut& o);
#define TTA_FUSE_PIECE(name, FIRST, LAST)                                                                         \
    void name(int V, dim3 grid, hipStream_t st, const TtaViews& vw, int H, int W, const UncOut& o) {             \
        tta_dispatch<FIRST, LAST>(V, grid, st, vw, H, W, o);                                                      \
    }
