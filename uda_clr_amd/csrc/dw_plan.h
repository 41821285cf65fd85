// Launch plans of the depthwise 3x3 convolution and of the 3 -> 32 stem (host only): dw_plan / stem_plan.
// The measured thresholds have their records in profiles/xception_dw_kernels.md and DESIGN.md 3g / 3i.
#pragma once
#include <limits.h>
#include "common.h"

// As conv_plan.h: a plan is a pure function of the call's arguments - it dereferences no pointer and reads no environment - and is
// the ONLY place where a depthwise / stem kernel, a tile or a template variant is chosen: uda_dwconv_* / uda_stem_* launch what it
// says, uda_dwconv_workspace_bytes, uda_dwconv_route and uda_stem_route read it.
enum DwOp { DW_FWD, DW_DGRAD, DW_WGRAD };
enum DwFamily {
    DWF_AUTO,       // only as a request: the shape rule below chooses (UDA_DW_AUTO ... UDA_DW_CB of the C ABI)
    DWF_FLAT,       // dwconv_fwd_kernel / dwconv_dgrad_kernel / dwconv_wgrad_kernel: all C/4 channel groups of a pixel in one workgroup
    DWF_TILED,      // dwconv_fwd_tiled_kernel / dwconv_wgrad_tiled_kernel<S, TH, TW>: 32 channels x a 2-D halo tile in LDS, dilation <= 2
    DWF_CB          // dwconv_cb_*_kernel: a channel block of up to 256 channels x a strip of pixels
};

#define DW_ITER_FWD 8          // pixels per lane: flat forward ...
#define DW_ITER_RED 32         // ... and weight gradient
#define DWT_CB 32              // channels of a tiled workgroup
#define DWB_ITER_FWD 8         // pixels per lane: channel-blocked forward and input gradient ...
#define DWB_ITER_RED 32        // ... and weight gradient
#define DW_CMAX 1024           // flat / tiled forward and weight gradient: LDS sized for it
#define DWB_CMAX 2048
#define DW_DGRAD_MAX_WG 8192   // flat input gradient: one thread per pixel and channel group, grid-stride beyond this many workgroups
// the <stride, tile rows, tile columns> instantiations of the tiled kernels
#define DW_TILED_VARIANTS(X) X(1, 8, 16) X(2, 8, 8)

struct DwPlan {
    int family;             // DwFamily; the requested one when error is set
    const char* error;      // non-null: no kernel of this family serves these arguments
    int S, TH, TW;          // tiled: template arguments ...
    int tilesX, tilesY;     // ... and tiles per image
    int lg;                 // cb: log2 of float4 groups per block
    int lanes;              // flat / cb: pixel lanes of a workgroup
    int Ho, Wo;             // output grid
    int64_t Pout;           // output pixels
    unsigned gx, gy;        // grid
    size_t lds;             // dynamic LDS bytes
    // weight gradient: the workspace is [sum_slots][9][C] doubles, then [part_rows][9][C] floats (flat: the uda_wgp_* layout)
    int sum_slots, part_rows;
    uint64_t ws_bytes;
};

// Shape rule (measured on MI355X at Xception's 512^2, B = 16 shapes, profiles/xception_dw_kernels.md): the channel-blocked kernels
// take the widths the other families reject (C > 1024) and the dilation-4 convs of 1024 channels (fwd 343 -> 235 us, wgrad 346 ->
// 258 us against the flat kernel).  At 728 / 1024 channels with dilation <= 2 the LDS-tiled kernels stay (fwd 25 / 31 us against
// 44 / 52 us).  Every MobileNetV2 launch (C <= 960) keeps its kernel; ResNet-101 has no depthwise conv.
static inline bool dw_use_cb(int C, int dil) { return C > 1024 || (dil > 2 && C >= 1024); }

// widest C a family serves (the flat input gradient keeps nothing per channel in LDS and has no bound)
static inline int dw_cmax(int op, int family) {
    if (family == DWF_CB) return DWB_CMAX;
    return op == DW_DGRAD ? INT_MAX : DW_CMAX;
}

static inline int dwb_lg_groups(int C) {          // log2(CG), CG = the power of two >= C/4, at most 64
    int lg = 0;
    while ((1 << lg) < C / 4 && lg < 6) ++lg;
    return lg;
}

// pixel lanes of a flat (all C/4 groups side by side) or channel-blocked workgroup
static inline int dw_lanes(int family, int C) { return family == DWF_CB ? 256 >> dwb_lg_groups(C) : 256 / (C / 4); }

// what the weight gradient of a family keeps in its workspace over Pout output pixels (C >= 4)
static inline void dw_wgrad_ws(int family, int64_t Pout, int C, int& sum_slots, int& part_rows) {
    sum_slots = family == DWF_FLAT ? 1 : UDA_STAT_SLOTS;
    part_rows = family == DWF_FLAT ? uda_cdiv(Pout, (int64_t)dw_lanes(DWF_FLAT, C) * DW_ITER_RED) : 0;
}
static inline uint64_t dw_wgrad_ws_bytes(int family, int64_t Pout, int C) {
    int slots, rows;
    dw_wgrad_ws(family, Pout, C, slots, rows);
    return (uint64_t)slots * 9 * C * sizeof(double) + (uint64_t)rows * 9 * C * sizeof(float);
}

// N, H, W: the conv's INPUT grid (forward / weight gradient: src; input gradient: dx)
static DwPlan dw_plan(int op, int N, int H, int W, int C, int stride, int dil, int want) {
    DwPlan p = {};
    p.family = want;
    if (op < DW_FWD || op > DW_WGRAD || want < DWF_AUTO || want > DWF_CB) { p.error = "no such operation or kernel family"; return p; }
    if ((stride != 1 && stride != 2) || dil < 1) { p.error = "stride must be 1 or 2, dilation >= 1"; return p; }
    if (N <= 0 || H <= 0 || W <= 0) { p.error = "bad geometry"; return p; }
    if (C % 4 != 0 || C < 4) { p.error = "C must be a multiple of 4, at least 4"; return p; }
    if (want == DWF_AUTO) p.family = dw_use_cb(C, dil) ? DWF_CB : ((op == DW_DGRAD || dil > 2) ? DWF_FLAT : DWF_TILED);
    p.Ho = (H - 1) / stride + 1; p.Wo = (W - 1) / stride + 1;
    p.Pout = (int64_t)N * p.Ho * p.Wo;
    const int64_t P = op == DW_DGRAD ? (int64_t)N * H * W : p.Pout;      // pixels the launch walks
    if (C > dw_cmax(op, p.family)) {
        p.error = p.family == DWF_CB ? "C must be at most 2048 on the channel-blocked kernels"
                                     : "C must be at most 1024 on the flat and tiled kernels (2048 on the channel-blocked ones)";
        return p;
    }
    if (p.family == DWF_CB) {
        p.lg = dwb_lg_groups(C);
        p.lanes = dw_lanes(DWF_CB, C);
        p.gx = uda_cdiv(P, (int64_t)p.lanes * (op == DW_WGRAD ? DWB_ITER_RED : DWB_ITER_FWD));
        p.gy = uda_cdiv(C / 4, 1 << p.lg);
    } else if (op == DW_DGRAD) {
        if (p.family == DWF_TILED) { p.error = "the input gradient has no tiled kernel"; return p; }
        const int g = uda_cdiv(P * (C / 4), 256);        // one thread per pixel and channel group, grid-stride beyond the cap
        p.gx = g > DW_DGRAD_MAX_WG ? DW_DGRAD_MAX_WG : g;
        p.gy = 1;
    } else {
        if (p.family == DWF_TILED) {
            if (dil > 2) { p.error = "the tiled kernels serve dilation 1 and 2"; return p; }
            p.S = stride; p.TH = 8; p.TW = stride == 1 ? 16 : 8;
            const int IH = (p.TH - 1) * p.S + 2 * dil + 1, IW = (p.TW - 1) * p.S + 2 * dil + 1;
            const size_t tile = (size_t)IH * IW * DWT_CB * sizeof(float), red = (size_t)32 * (op == DW_FWD ? 2 : 9) * DWT_CB * sizeof(float);
            p.lds = tile > red ? tile : red;        // the halo tile, reused for the workgroup's reduction
            p.tilesX = uda_cdiv(p.Wo, p.TW); p.tilesY = uda_cdiv(p.Ho, p.TH);
            p.gx = (unsigned)(p.tilesX * p.tilesY * N);
            p.gy = uda_cdiv(C, DWT_CB);
        } else {
            p.lanes = dw_lanes(DWF_FLAT, C);        // (C <= 1024: at least one pixel per workgroup)
            p.gx = uda_cdiv(P, (int64_t)p.lanes * (op == DW_FWD ? DW_ITER_FWD : DW_ITER_RED));
            p.gy = 1;
        }
    }
    if (op == DW_WGRAD) {
        dw_wgrad_ws(p.family, p.Pout, C, p.sum_slots, p.part_rows);
        p.ws_bytes = dw_wgrad_ws_bytes(p.family, p.Pout, C);
    }
    return p;
}

// ---- stem 3 -> 32, stride 2: the row-staged kernels take output rows that are a multiple of 256 pixels wide (the 512 x 512 training
// images); their weight gradient reads dy with 16-byte loads
enum StemKernel { STEM_PIXELS, STEM_ROWS };
#define STEM_PIX_PER_WG 256   // 32 pixels per pass x 8 passes; one 256-pixel row segment of the row-staged kernels

struct StemPlan {
    int kernel;             // StemKernel
    const char* error;
    int Ho, Wo;
    int64_t Pout;
    int grid;               // workgroups = partial rows of the weight gradient (rows: N * Ho * (Wo / 256))
};

static StemPlan stem_plan(int op, int N, int H, int W, int64_t lddy, int dy_aligned16) {
    StemPlan p = {};
    if (op != DW_FWD && op != DW_WGRAD) { p.error = "no such operation"; return p; }
    if (N <= 0 || H <= 1 || W <= 1 || (op == DW_WGRAD && lddy < 32)) { p.error = "bad args"; return p; }
    p.Ho = (H - 1) / 2 + 1; p.Wo = (W - 1) / 2 + 1;
    p.Pout = (int64_t)N * p.Ho * p.Wo;
    p.grid = uda_cdiv(p.Pout, STEM_PIX_PER_WG);
    const bool rows = p.Wo % 256 == 0 && (op == DW_FWD || (dy_aligned16 && lddy % 4 == 0));
    p.kernel = rows ? STEM_ROWS : STEM_PIXELS;
    return p;
}
