// Kernel-argument blocks shared by igemm_conv.hip (single-role kernels, narrow tiles) and
// igemm_ws.hip (warp-specialised kernels, wide tiles).
#pragma once
#include "common.h"

struct ConvKArgs {
    uda_src_t src;
    const float* w;
    int Cout, ksize, dil, Kc, Ktot;
    int cen;       // tap (kh, kw) reads pixel offset ((kh - cen) * dil, (kw - cen) * dil): 1 for 3x3, 0|1 for 2x2
    const float* bias;
    const float* addend;
    int64_t ld_add;
    float* y;
    int64_t ldy;
    double* stats; // [UDA_STAT_SLOTS][2][Cout] or null (fp64 atomics)
    int nMt, nNt;
    int debug;     // diagnostics only (UDA_WS_DEBUG): bit0 skip MFMAs, bit1 skip loader work
    int x3;        // UDA_MFMA_BF16X3: wide tiles on the bf16 pipe by exact 3-way splitting (igemm_x3.hip)
    int stride, Ho, Wo;   // output grid: pixel (n, oh, ow) reads the taps around input pixel (n, oh * stride, ow * stride); wide-tile kernels only
};

struct WgradKArgs {
    uda_src_t src;
    const float* dy;
    int64_t lddy;
    int Cout, ksize, dil, Kc, Jtot;
    int cen;
    float* slab;      // [S][Cout][Jtot]
    int nCot, nJt, chunks_per_split, nchunks;
    int x3;
    int stride, Ho, Wo;   // grid of dy (see ConvKArgs); wide-tile kernels only
};

#define IG_BK 32
#define IG_LD 36
#define WG_BKP 32
#define WGN_BKP 64        // pixels per K-chunk of the narrow (HBM-bound) weight-gradient kernel: one barrier pair per 64 pixels
#define X3_BK 16          // K depth of a bf16x3 chunk
#define X3_ROW 56         // bf16 per staged row: 3 pieces x 16 + 8 pad = 112 B: a row's 96 B arrive as they lie in the packed operand
