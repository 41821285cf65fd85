// Launch plan of the decoder's interpolation pass and its adjoint (host only): upconv_plan.
// The kernels and what their thresholds were measured against: upconv.hip, DESIGN.md 3a / 3f.
#pragma once
#include "bilinear.h"

// As conv_plan.h and dw_plan.h: a plan is a pure function of the call's arguments - it dereferences no pointer and reads no
// environment - and is the ONLY place where an upconv kernel is chosen: uda_upconv_fwd / uda_upconv_bwd launch what it says,
// uda_upconv_route reads it.
enum UpOp { UP_FWD, UP_BWD };
enum UpKernel {
    UPK_NONE,       // refused arguments (UpconvPlan::error says why)
    UPK_TILE,       // upconv_fwd_tile_kernel: a 16 x 16 output tile x 32 channels per workgroup, its footprint of g in LDS
    UPK_STRIP3,     // upconv_fwd_strip_kernel<3>: four output pixels of a row per thread, 3 low-resolution columns per tap
    UPK_STRIP4,     // upconv_fwd_strip_kernel<4>: the same with 4 columns
    UPK_PIXEL,      // upconv_fwd_kernel: one output pixel per thread, any geometry, 64-bit indices, no statistics
    UPK_WAVE,       // upconv_bwd_wave_kernel: one wave per low-resolution pixel, C = 256
    UPK_THREAD      // upconv_bwd_kernel: one thread per low-resolution pixel and channel group, any geometry
};

#define UPT_TH 16            // the tile kernel's output tile ...
#define UPT_TW 16
#define UPT_CS 32            // ... and channels per workgroup (8 granules of 4)

struct UpconvPlan {
    int kernel;             // UpKernel
    const char* error;      // non-null: the entry refuses these arguments
    unsigned grid;          // workgroups of 256 threads
    int R, RC;              // tile: rows / columns of the low-resolution footprint of an output tile ...
    size_t lds;             // ... and its bytes of dynamic LDS
    bool fused_stats;       // forward, statistics wanted: the kernel accumulates them itself (otherwise uda_colstats over y follows)
    float sh, sw;           // the interpolation's source steps (align_corners)
};

// rows (columns) of the low-resolution footprint of a tile whose tap positions span [o_min, o_max] (clipped to the image)
static inline int upconv_foot(int o_min, int o_max, float scale, int n_in, int n_out) {
    const float lo = scale * (float)(o_min < 0 ? 0 : o_min), hi = scale * (float)(o_max > n_out - 1 ? n_out - 1 : o_max);
    int i_lo = (int)lo, i_hi = (int)hi;
    if (i_lo > n_in - 1) i_lo = n_in - 1;
    if (i_hi > n_in - 1) i_hi = n_in - 1;
    i_hi += i_hi < n_in - 1 ? 1 : 0;
    return i_hi - i_lo + 1;
}

// workgroups of 256 threads for `threads` of them, at most `cap` (all kernels but the tile kernel walk the rest with a grid stride)
#define UPCONV_FLAT_MAX_WG 65536     // pixel forward, thread / wave backward: one item per thread (wave), grid-stride beyond
#define UPCONV_STRIP_MAX_WG 4096     // strip forward: bounded, the statistics epilogue issues 2*C atomics per workgroup
static inline unsigned upconv_grid(int64_t threads, int64_t cap) {
    const int64_t g = (threads + 255) / 256;
    return (unsigned)(g > cap ? cap : g);
}

// g / dg: [N*h*w, ldg >= 9*C]; y / dy: [N*H*W, >= C].  has_addend, ld_add, addend_rows and want_stats describe a forward call and
// are not read for the adjoint.
static UpconvPlan upconv_plan(int op, int N, int h, int w, int H, int W, int C, int dil, int64_t ldg, bool has_addend, int64_t ld_add,
                              int64_t addend_rows, bool want_stats) {
    UpconvPlan p = {};
    if (op != UP_FWD && op != UP_BWD) { p.error = "no such operation"; return p; }
    if (N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || dil < 1) { p.error = "bad geometry"; return p; }
    if (C <= 0 || C % 4 != 0 || ldg % 4 != 0 || ldg < 9 * (int64_t)C) { p.error = "g must be [N*h*w, >= 9*C], C and its row stride multiples of 4"; return p; }
    if (op == UP_FWD && has_addend && (ld_add % 4 != 0 || ld_add < C || addend_rows <= 0 || ((int64_t)N * H * W) % addend_rows != 0)) {
        p.error = "addend must be [addend_rows, >= C] with addend_rows dividing N*H*W";
        return p;
    }
    const int G = C / 4;
    const int64_t lim32 = (int64_t)1 << 31;
    p.sh = bil_scale(h, H); p.sw = bil_scale(w, W);
    if (op == UP_BWD) {
        // one wave per low-resolution pixel when its 64 lanes are exactly the channel granules, the tap ranges fit the 32-entry weight
        // tables and the pixel index fits the kernel's 32-bit readfirstlane
        const int64_t npix = (int64_t)N * h * w;
        if (C == 256 && dil == 1 && p.sh > 0.f && p.sw > 0.f && 2.f / p.sh + 6.f <= 32.f && 2.f / p.sw + 6.f <= 32.f && npix < lim32) {
            p.kernel = UPK_WAVE;
            p.grid = upconv_grid(npix * 64, UPCONV_FLAT_MAX_WG);
        } else {
            p.kernel = UPK_THREAD;
            p.grid = upconv_grid(npix * G, UPCONV_FLAT_MAX_WG);
        }
        return p;
    }
    // Strips: the four tap positions of a strip span 3*sw low-resolution columns, floor(frac + 3*sw) + 1 <= NC - 1 with NC <= 4 (margins
    // of 2 %: the column indices come from fp32 products scale * x, whose rounding must not push a strip over its last cached column);
    // the statistics epilogue wants every thread on one channel group (C/4 divides 256); the kernels index in 32 bits - output
    // pixels, strips (+ one grid stride of 65536 x 256), the bytes of g behind one buffer descriptor, the addend's elements
    const float sw3 = 3.f * p.sw;
    const int64_t strips = (int64_t)N * H * (W / 4) * G;
    const bool strip = H % 4 == 0 && W % 4 == 0 && dil == 1 && sw3 < 1.96f && 256 % G == 0 &&
                       (int64_t)N * H * W < lim32 && strips < lim32 - 65536 * 256 && (int64_t)N * h * w * ldg * 4 < lim32 &&
                       (!has_addend || addend_rows * ld_add < lim32 * 4);
    if (!strip) {
        p.kernel = UPK_PIXEL;
        p.grid = upconv_grid((int64_t)N * H * W * G, UPCONV_FLAT_MAX_WG);
        return p;
    }
    p.fused_stats = want_stats;
    // the LDS-tiled kernel where the tiling fits: x4-like upsampling (3 columns per strip) of a map whose sides are multiples of 16,
    // the largest tile footprint within 56 KiB
    if (sw3 < 0.98f && H % UPT_TH == 0 && W % UPT_TW == 0 && C % UPT_CS == 0) {
        int R = 1, RC = 1;
        for (int ty = 0; ty < H / UPT_TH; ++ty) { const int r = upconv_foot(ty * UPT_TH - 1, ty * UPT_TH + UPT_TH, p.sh, h, H); if (r > R) R = r; }
        for (int tx = 0; tx < W / UPT_TW; ++tx) { const int r = upconv_foot(tx * UPT_TW - 1, tx * UPT_TW + UPT_TW, p.sw, w, W); if (r > RC) RC = r; }
        const size_t lds = (size_t)R * RC * 72 * 16;            // [R][RC][9 taps][8 granules] float4
        const int64_t nwg = (int64_t)N * (H / UPT_TH) * (W / UPT_TW) * (C / UPT_CS);      // (< 2^28 here: C <= 1024, N*H*W < 2^31)
        if (lds <= 64 * 1024 - 8192 && nwg < lim32) {
            p.kernel = UPK_TILE;
            p.grid = (unsigned)nwg; p.R = R; p.RC = RC; p.lds = lds;
            return p;
        }
    }
    p.kernel = sw3 < 0.98f ? UPK_STRIP3 : UPK_STRIP4;
    p.grid = upconv_grid(strips, UPCONV_STRIP_MAX_WG);
    return p;
}
