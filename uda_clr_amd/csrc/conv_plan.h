// Launch plans of the dense convolution and its weight gradient (host only): conv_plan / wgrad_plan.
// Every measured threshold below has its A/B record in DESIGN.md 3d / 3f.
#pragma once
#include <stdlib.h>
#include "igemm_args.h"

// A plan is a pure function of the call's arguments - it dereferences no pointer - and is the ONLY place where a kernel family, a
// tile or a template variant is chosen: uda_conv_fwd / uda_conv_wgrad launch what it says, the uses_x3 / workspace_bytes queries and
// uda_conv_route / uda_conv_wgrad_route read it.
enum ConvFamily {
    CF_NONE,        // no kernel serves these arguments (ConvPlan::error says why)
    CF_STREAM,      // conv1x1_stream_kernel<bm, bn>: short-K 1x1 over many pixels (bm = channels per lane, bn = column blocks)
    CF_COUT1,       // conv_cout1_kernel: one output on a raw operand
    CF_HEADS,       // conv_heads_kernel<bn>: one or two outputs of a 1x1 conv on a lazy operand
    CF_FEW,         // igemm_conv_kernel, 64-pixel tiles of 192 / 320 columns: few pixels, wide output, long K
    CF_LOW,         // igemm_conv_kernel, 64-pixel tiles of 64 / 128 columns: few pixels
    CF_NARROW,      // igemm_conv_kernel, 128-pixel tiles: narrow outputs or short K
    CF_WS,          // igemm_conv_ws_kernel: warp-specialised wide tiles, fp32 MFMA
    CF_X3,          // igemm_conv_x3_kernel: wide tiles on the bf16 pipe
    CF_X3_TAIL,     // the same with the last, partly filled round of tiles split over K (TAIL launch + x3_tail_reduce_kernel)
    CF_WGRAD,       // igemm_wgrad_kernel: narrow weight-gradient tiles
    CF_WGRAD_WS,    // igemm_wgrad_ws_kernel
    CF_WGRAD_X3,    // igemm_wgrad_x3_kernel
    CF_COUNT
};

struct ConvPlan {
    int family;             // ConvFamily
    const char* error;      // non-null: uda_conv_fwd refuses these arguments
    int bm, bn;             // tile: pixels x columns
    int ks;                 // KS template argument of the wide-tile kernels (1: 1x1, 3: any multi-tap)
    int pipe, xf;           // igemm_conv_kernel: two LDS images; loader form of igemm_conv_kernel (-1 general, 0, 1) / igemm_conv_ws_kernel (0, 1, 2)
    int stride, Ho, Wo;     // output grid
    int64_t P;              // output pixels
    int Kc, Ktot;           // channels rounded to 4; floats per weight row
    int grid;               // workgroups of the (main) launch; 0 for CF_STREAM, which fills the device it runs on
    size_t lds;             // dynamic LDS bytes per workgroup
    // bf16x3: tiles in full rounds, tiles of the last round, workgroups per tail tile (1: no split); the workspace the split wants
    // (whether or not the call brings it) - without it the plan is the best one that does not split
    int64_t full, tail;
    int ksplit;
    uint64_t ws_bytes;
};

struct WgradPlan {
    int family;             // CF_WGRAD, CF_WGRAD_WS or CF_WGRAD_X3
    const char* error;
    int bm, bn, xf;         // tile: outputs x weight-row positions; loader form of igemm_wgrad_ws_kernel
    int nCot, nJt, S, cps, nchunks;     // tiles, splits of the pixel range actually launched, chunks per split, chunks
    int red_q;              // wgrad_reduce_kernel<red_q> sums the S slabs
    int stride, Ho, Wo;
    int64_t P;              // pixels of dy
    int Kc, Jtot;
    size_t lds;             // dynamic LDS bytes (0: the narrow kernel's image is static)
    uint64_t ws_bytes;      // slabs of the fp32 plan (uda_conv_wgrad_workspace_bytes): the bf16x3 plan never uses more
};

constexpr size_t igc_tile_bytes(int bm, int bn) { return (size_t)(bm + bn) * IG_LD * sizeof(float); }      // one image of igemm_conv_kernel
constexpr size_t ws_lds_bytes(int bm, int bn) { return 2 * igc_tile_bytes(bm, bn); }
constexpr size_t x3_lds_bytes(int bm, int bn) { return (size_t)2 * (bm + bn) * X3_ROW * 2; }
constexpr size_t wg_ws_lds_bytes(bool big) { return (size_t)2 * WG_BKP * (big ? 512 : 256) * sizeof(float); }
constexpr size_t wg_x3_lds_bytes(int bm, int bn) { return (size_t)2 * 3 * 16 * ((bm * 2 + 64) + (bn * 2 + 64)); }

int launch_conv_ws(ConvKArgs& k, const ConvPlan& p, hipStream_t st);
int launch_conv_x3(const ConvKArgs& k, const ConvPlan& p, const void* x3_src, const void* x3_w, void* ws, hipStream_t st);
int launch_wgrad_ws(WgradKArgs& k, const WgradPlan& p, hipStream_t st);
int launch_wgrad_x3(const WgradKArgs& k, const WgradPlan& p, const void* x3_src, const void* x3_dy, hipStream_t st);

// floats per weight row of a conv with C input channels and ksize x ksize taps
static inline int uda_k_row(int C, int ksize) {
    const int Kc = ((C + 3) / 4) * 4;
    if (ksize == 1 || Kc < IG_BK) return ksize * ksize * Kc;      // fewer than 32 channels: tap-major, unpadded
    return ((Kc + IG_BK - 1) / IG_BK) * ksize * ksize * IG_BK;
}

// The short-K streaming form applies: 1x1, stride 1, K = Cin in {16, 24, 32}, no keep-mask, no bias, >= 32768 pixels, aligned rows.
// Sets the kernel's <channels per lane, column blocks per group>.
static bool plan_stream(const uda_conv_args_t* a, int64_t P, int& kh, int& nb) {
    if (a->ksize != 1 || (a->stride > 1) || a->src.mask || a->bias || P < 32768) return false;
    if (!uda_aligned16(a->src.x) || a->src.ldx % 4 || (a->src.C != 16 && a->src.C != 24 && a->src.C != 32)) return false;
    if (P * a->ldy >= ((int64_t)1 << 29) || (a->addend && P * a->ld_add >= ((int64_t)1 << 29))) return false;
    const int C = a->src.C, Cout = a->Cout;
    kh = C / 2;
    if (C == 16 && Cout <= 96) nb = Cout <= 32 ? 1 : 3;
    else if (C == 24 && Cout <= 160) nb = Cout <= 64 ? 2 : (Cout <= 96 ? 3 : 5);
    else if (C == 32 && Cout > 96 && Cout <= 192 && P >= 262144) nb = 3;      // (at 65536 pixels, and towards few columns, the tiled kernel is as fast or faster)
    else return false;
    return true;
}

// bf16x3 eligibility: the tap-chunked K order (>= 32 channels per tap), and enough MFMA work per packed element to pay for the packing
// pass (2 * Cout * taps FLOPs per activation element).  Measured (tests/bench_x3.py, profiles/r02_bf16x3_vs_f32_conv_microbench.txt):
// 3x3 / 2x2 convs with >= 128 outputs run 1.5-2.0x faster incl. the pass; a 3x3 conv towards 48 channels over K = 2304 1.9x on
// the 256 x 64 tile; 1x1 convs only when very wide (the 256 -> 2304 tap GEMM of the re-associated decoder conv: 1.6-1.8x), or with a
// long K towards >= 256 outputs (ResNet-101's bottleneck convs 1024 -> 256 and 2048 -> 512 on the 32x32 maps: their operands are
// block inputs / gradients that the weight gradient packs anyway); MobileNetV2's 1x1 convs gain nothing, the packing pass eats it.
static bool conv_x3_eligible(int Kc, int ksize, int Cout) {
    if (ksize == 1) return Kc >= 128 && (Cout >= 1024 || (Kc >= 1024 && Cout >= 256));
    return Kc >= IG_BK && Cout * ksize * ksize >= 432;
}

// Tail of a bf16x3 tile choice: the last, partly filled round of tiles is computed by ksplit workgroups per tile over consecutive K
// ranges (x3_tail_reduce_kernel sums the partial tiles).  Only where it clearly pays: a long K (the fp32 partial tiles are extra
// traffic - one write and one read per split - and on the short-K layers the split bought 2-3 %) and at least three splits
// (measured: discriminator L3 / L4 forward 10 % / 16 %).
struct X3Tail {
    int64_t tiles, full, tail;
    int ksplit;
};

static X3Tail x3_tail_plan(int64_t P, int Cout, int nchunks, int BM, int BN, bool allow) {
    X3Tail t;
    t.tiles = uda_cdiv(P, BM) * uda_cdiv(Cout, BN);
    t.full = (t.tiles / 256) * 256;
    t.tail = t.tiles - t.full;
    t.ksplit = 1;
    if (allow && t.tail > 0 && t.tail <= 85 && nchunks >= 96) {
        int s = (int)(256 / t.tail);
        if (s > 8) s = 8;
        if (s > nchunks / 8) s = nchunks / 8;       // at least 8 chunks per workgroup
        if (s >= 3) t.ksplit = s;
    }
    return t;
}

// bf16x3 tile choice: the cheapest of 256 x 256, 128 x 256, 256 x 128, 128 x 128 under  rounds x tile area / tile efficiency, a round
// being one tile per CU - padding waste (Cout = 304 fits three 128-wide tiles better than two 256-wide ones) and the partly
// filled last round both count; a split last round costs 1 / ksplit of a round plus the reduce.  Efficiencies fitted to the
// discriminator layers (the tiles stage 32 / 48 / 48 / 64 B per MFMA clock and CU, two 128 x 128 workgroups can share a CU).
static const int X3_TILE_BM[4] = {256, 128, 256, 128}, X3_TILE_BN[4] = {256, 256, 128, 128};

static X3Tail x3_pick_tile(int64_t P, int Cout, int nchunks, bool allow_tail, int& bm, int& bn) {
    const double eff[4] = {1.0, 0.97, 0.92, 0.84};
    int best = 0;
    double bestc = 1e300;
    for (int t = 0; t < 4; ++t) {
        const X3Tail tp = x3_tail_plan(P, Cout, nchunks, X3_TILE_BM[t], X3_TILE_BN[t], allow_tail);
        double rounds = (double)(tp.full / 256);
        if (tp.tail > 0) rounds += tp.ksplit > 1 ? 1.0 / tp.ksplit + 0.12 : 1.0;
        const double c = rounds * X3_TILE_BM[t] * X3_TILE_BN[t] / eff[t];
        if (c < bestc) { bestc = c; best = t; }
    }
#ifdef UDA_DIAG          // diagnostic builds only (make DIAG=1): force a tile, for fitting the efficiencies above
    static const int force = getenv("UDA_X3_TILE") ? atoi(getenv("UDA_X3_TILE")) : -1;
    if (force >= 0 && force < 4) best = force;
#endif
    bm = X3_TILE_BM[best]; bn = X3_TILE_BN[best];
    return x3_tail_plan(P, Cout, nchunks, bm, bn, allow_tail);
}

static void plan_x3(ConvPlan& p, const uda_conv_args_t* a) {
    const int nch = uda_cdiv(p.Ktot, X3_BK);
    X3Tail t;
    if (a->ksize >= 2 && a->Cout <= 64) {       // input gradient towards a narrow tensor (decoder low-level branch): one tile shape, never split
        p.bm = 256; p.bn = 64; p.ks = 3;
        t = x3_tail_plan(p.P, a->Cout, nch, 256, 64, false);
    } else {
        // the split needs a conv without statistics epilogue and a workspace: plan with it first (its size is what
        // uda_conv_fwd_workspace_bytes answers), and without it when the call does not bring one
        t = x3_pick_tile(p.P, a->Cout, nch, a->stats == nullptr, p.bm, p.bn);
        if (t.ksplit > 1) p.ws_bytes = (uint64_t)t.tail * t.ksplit * p.bm * p.bn * sizeof(float);
        if (!(p.ws_bytes > 0 && a->workspace && a->workspace_bytes >= p.ws_bytes && uda_aligned16(a->workspace)))
            t = x3_pick_tile(p.P, a->Cout, nch, false, p.bm, p.bn);
    }
    p.family = t.ksplit > 1 ? CF_X3_TAIL : CF_X3;
    p.full = t.full; p.tail = t.tail; p.ksplit = t.ksplit;
    p.grid = (int)(t.ksplit > 1 ? t.full : t.tiles);
    p.lds = x3_lds_bytes(p.bm, p.bn);
}

static void plan_ws(ConvPlan& p, const uda_conv_args_t* a) {
    // Tile width BN = 64*TN chosen by a wave-quantisation model: workgroups run one per CU, a K-chunk
    // costs ~TN MFMA-units, so time ~ ceil(#tiles / 256 CUs) * TN.  E.g. Cout = 304 at P = 262144 ->
    // TN = 5 (one 320-wide tile, 5 % padding); Cout = 320 at P = 16384 -> TN = 3 (256 workgroups).
    const int64_t nMt = uda_cdiv(p.P, 128);
    int best = 2;
    int64_t best_cost = -1;
    for (int tn = 2; tn <= 5; ++tn) {
        const int64_t tiles = nMt * uda_cdiv(a->Cout, 64 * tn);
        const int64_t cost = ((tiles + 255) / 256) * tn * 16 + (tn == 2 ? 3 : 0);   // BN=128 stages A twice as often
        if (best_cost < 0 || cost < best_cost) {
            best_cost = cost;
            best = tn;
        }
    }
    p.family = CF_WS;
    p.bm = 128; p.bn = 64 * best;
    // few pixels (ResNet's 32x32-map layers at B = 8: 64 tiles of 128 rows for 256 CUs): 64-row tiles, twice the workgroups;
    // two 128x128 workgroups per CU beat one 256x128 (measured)
    if (nMt * uda_cdiv(a->Cout, 64 * best) <= 192 && nMt * uda_cdiv(a->Cout, 128) <= 256) { p.bm = 64; p.bn = 128; }
    // 256-pixel tiles (a third less operand staging per MFMA) once they still fill the chip twice over
    else if (best == 4 && uda_cdiv(p.P, 256) * uda_cdiv(a->Cout, 256) >= 512) p.bm = 256;
    p.xf = a->src.mask ? 2 : ((a->src.scale || a->src.act != ACT_NONE) ? 1 : 0);
    p.grid = uda_cdiv(p.P, p.bm) * uda_cdiv(a->Cout, p.bn);
    p.lds = ws_lds_bytes(p.bm, p.bn);
}

static void plan_tile(ConvPlan& p, const uda_conv_args_t* a, int family, int bm, int bn) {
    p.family = family; p.bm = bm; p.bn = bn;
    // long K: the pipelined form (two tile images, loads two chunks ahead); short K keeps the lean one (more workgroups per CU)
    p.pipe = p.Ktot >= 192;
    // 1x1 without a keep-mask: the lean loader (XF 0: also no transform and no activation - gradient matrices; XF 1: the rest)
    p.xf = (a->ksize == 1 && !a->src.mask) ? ((!a->src.scale && a->src.act == ACT_NONE) ? 0 : 1) : -1;
    p.grid = uda_cdiv(p.P, bm) * uda_cdiv(a->Cout, bn);
    p.lds = igc_tile_bytes(bm, bn) * (p.pipe ? 2 : 1);
}

// a: ksize in 1..3 (the only field the planner relies on being valid)
static ConvPlan conv_plan(const uda_conv_args_t* a) {
    ConvPlan p = {};
    const int Cout = a->Cout, ks = a->ksize;
    p.stride = a->stride <= 1 ? 1 : a->stride;
    // stride 2 (resnet.py:66 conv2 of the first bottleneck of layer2 / layer3, :93 their 1x1 shortcut): output pixel (n, oh, ow) is
    // centred on input pixel (n, 2 oh, 2 ow); P counts OUTPUT rows
    p.Ho = (a->src.H - 1) / p.stride + 1; p.Wo = (a->src.W - 1) / p.stride + 1;
    p.P = (int64_t)a->src.N * p.Ho * p.Wo;
    p.Kc = ((a->src.C + 3) / 4) * 4;
    p.Ktot = uda_k_row(a->src.C, ks);
    p.ks = ks >= 2 ? 3 : 1;
    p.xf = -1; p.ksplit = 1;
    const int64_t P = p.P;
    const int Kc = p.Kc, Ktot = p.Ktot;
    const char* const strided = "uda_conv_fwd: stride 2 is built on the wide-tile kernels only (Cout > 96, K > 192)";
    if (plan_stream(a, P, p.bm, p.bn)) { p.family = CF_STREAM; return p; }
    // only the wide-tile kernels walk a strided output grid
    if (Cout == 1 && !a->src.scale && !a->src.mask && a->src.act == ACT_NONE && !a->stats && Ktot >= 1024) {
        p.family = CF_COUT1; p.bm = 4; p.bn = 1; p.grid = uda_cdiv(P, 4);
        if (p.stride != 1) p.error = strided;
        return p;
    }
    if (Cout <= 2 && ks == 1 && !a->stats && Kc >= 64 && Kc <= 2048) {
        p.family = CF_HEADS; p.bm = 128; p.bn = Cout; p.grid = uda_cdiv(P, 128); p.lds = (size_t)(2 + Cout) * Kc * sizeof(float);
        if (p.stride != 1) p.error = strided;
        return p;
    }
    const bool short_k = Ktot <= 192 || (ks >= 2 && Kc < IG_BK);     // (the wide-tile kernels only walk the tap-chunked K order)
    // wide (MFMA-bound) tiles; towards narrow outputs only the bf16x3 mode has one, 64 columns wide (long-K multi-tap convs)
    const bool x3_mode = a->mfma == UDA_MFMA_BF16X3;
    const bool wide = Cout <= 96 ? (x3_mode && ks >= 2 && Cout >= 40 && Cout <= 64 && Kc >= 128 && Ktot >= 1024) : !short_k;
    if (x3_mode && wide && conv_x3_eligible(Kc, ks, Cout)) {
        plan_x3(p, a);
        if (p.stride != 1 && Cout <= 96) p.error = strided;
        return p;
    }
    if (p.stride != 1) {
        if (wide && Cout > 96) plan_ws(p, a);
        else p.error = strided;
        return p;
    }
    // few pixels, wide output, long K (the project convs of the 32x32-map layers: 960 -> 160, 576 -> 160, 960 -> 320 at P = 16384): the
    // 128 x 128 wide tiles pad 160 columns to 256 and give one workgroup per CU; 64-pixel tiles of 192 or 320 columns give the same 256
    // workgroups with 17 % / no padding.  (MobileNetV2's shapes; ResNet-101's wider / longer 1x1 convs stay on the wide-tile kernels: measured)
    if (P > 64 && uda_cdiv(P, 128) <= 192 && Cout > 128 && Cout <= 320 && Ktot > 192 && Ktot <= 1024 && ks == 1) {
        const int c192 = uda_cdiv(Cout, 192) * 192, c320 = uda_cdiv(Cout, 320) * 320;
        const int64_t t192 = uda_cdiv(P, 64) * (c192 / 192), t320 = uda_cdiv(P, 64) * (c320 / 320);
        if (c192 <= c320 && t192 >= 192 && t192 <= 512) { plan_tile(p, a, CF_FEW, 64, 192); return p; }
        if (t320 >= 192 && t320 <= 512) { plan_tile(p, a, CF_FEW, 64, 320); return p; }
    }
    // few pixels (the 32x32-map layers at B = 16: 128 tiles of 128 pixels for 256 CUs): 64-pixel tiles, twice the workgroups
    const bool low = P > 64 && uda_cdiv(P, 128) * uda_cdiv(Cout, Cout <= 64 ? 64 : 128) <= 192;
    if (low && Cout <= 64) plan_tile(p, a, CF_LOW, 64, 64);
    else if (low && Cout <= 128 && (short_k || Cout <= 96)) plan_tile(p, a, CF_LOW, 64, 128);
    else if (Cout <= 96) plan_tile(p, a, CF_NARROW, 128, Cout <= 32 ? 32 : (Cout <= 64 ? 64 : 96));
    else if (short_k) {
        // short K (the backbone's expand convs): output-bound; pick the tile width that wastes the fewest columns
        // (Cout = 144 -> one 160-wide tile instead of two 128-wide ones, 576 -> six 96-wide tiles, ...)
        const int w96 = uda_cdiv(Cout, 96) * 96, w128 = uda_cdiv(Cout, 128) * 128, w160 = uda_cdiv(Cout, 160) * 160;
        plan_tile(p, a, CF_NARROW, 128, (w160 <= w128 && w160 <= w96) ? 160 : (w128 <= w96 ? 128 : 96));
    }
    else plan_ws(p, a);
    return p;
}

static bool conv_plannable(const uda_conv_args_t* a) { return a && a->ksize >= 1 && a->ksize <= 3; }

// fp32 tiles and splits of the weight gradient of a [P, Cout] gradient against Cin channels x ksize^2 taps
static WgradPlan wgrad_plan(int64_t P, int Cout, int Cin, int ksize) {
    WgradPlan p = {};
    p.P = P;
    p.Kc = ((Cin + 3) / 4) * 4;
    const int J = p.Jtot = ksize * ksize * p.Kc;
    const int cm = Cout <= 32 ? 32 : (Cout <= 64 ? 64 : 128);
    const int cn = J <= 32 ? 32 : (J <= 64 ? 64 : 128);
    const bool big = Cout >= 192 && J >= 256 && uda_cdiv(P, WG_BKP) >= 4096;      // (measured: a loss below ~100k pixels)
    if (big) { p.bm = 256; p.bn = 256; }
    else if (cm == 128 && cn == 32) { p.bm = 128; p.bn = 32; }
    else if (cm == 32 && cn == 128) { p.bm = 32; p.bn = 128; }
    else if (cm <= 64 && cn <= 64) { p.bm = 64; p.bn = 64; }
    else { p.bm = 128; p.bn = 128; }
    const bool wide = p.bm == 256 || (p.bm == 128 && p.bn == 128);
    p.family = wide ? CF_WGRAD_WS : CF_WGRAD;
    p.lds = wide ? wg_ws_lds_bytes(big) : 0;
    p.nCot = uda_cdiv(Cout, p.bm);
    p.nJt = uda_cdiv(J, p.bn);
    p.nchunks = uda_cdiv(P, wide ? WG_BKP : WGN_BKP);
    int S = (p.bm == 256 ? 512 : 1024) / (p.nCot * p.nJt);      // 256 x 256 tiles: one workgroup per CU, two rounds
    if (S > p.nchunks / 4) S = p.nchunks / 4;
    if (S < 1) S = 1;
    // up to 256 slabs; up to 1024 for a tiny weight (one or two tiles over a million pixels: the backbone's first blocks, the decoder's
    // 24 -> 48 conv): with 256 workgroups each walks thousands of pixels at one chunk's load latency per chunk, and its slabs are small
    const int scap = (int64_t)Cout * J <= 8192 ? 1024 : 256;
    if (S > scap) S = scap;
    p.cps = uda_cdiv(p.nchunks, S);
    p.S = uda_cdiv(p.nchunks, p.cps);
    p.ws_bytes = (uint64_t)p.S * Cout * J * sizeof(float);
    return p;
}

// Eligibility of the bf16x3 weight gradient: 16-wide channel blocks must not straddle taps (Kc % 16 == 0), enough work to pay for the
// packing of dy (the source's packed form usually exists already from the forward conv).
static bool wgrad_x3_eligible(int Cin, int Cout, int ksize, int64_t P) {
    if (ksize == 1) return Cin % 16 == 0 && P >= 4096 && ((Cin >= 128 && Cout >= 1024) || (Cin >= 1024 && Cout >= 256));
    return Cin % 16 == 0 && Cin >= 32 && Cout >= 96 && P >= 4096;
}

// a: ksize in 1..3
static WgradPlan wgrad_plan(const uda_wgrad_args_t* a) {
    // stride 2: dy lives on the output grid, its pixel (n, oh, ow) pairs with source pixel (n, 2 oh, 2 ow); P = pixels of dy
    const int sd = a->stride <= 1 ? 1 : a->stride;
    const int Ho = (a->src.H - 1) / sd + 1, Wo = (a->src.W - 1) / sd + 1;
    WgradPlan p = wgrad_plan((int64_t)a->src.N * Ho * Wo, a->Cout, a->src.C, a->ksize);
    p.stride = sd; p.Ho = Ho; p.Wo = Wo;
    p.xf = a->src.mask ? 2 : ((a->src.scale || a->src.act != ACT_NONE) ? 1 : 0);
    if (p.family == CF_WGRAD && sd != 1) p.error = "uda_conv_wgrad: stride 2 is built on the wide-tile kernels only (Cout > 64, K > 64)";
    if (p.family == CF_WGRAD_WS && a->mfma == UDA_MFMA_BF16X3 && wgrad_x3_eligible(a->src.C, a->Cout, a->ksize, p.P)) {
        // tiles (Cout x J): 256 x 256 for wide outputs; 128 x 256 otherwise (128 x 128 tiles would stage 64 B per MFMA clock and CU and
        // are load-bound); 128 x 128 only for short J
        const bool big = a->Cout >= 192 && p.Jtot >= 256 && p.P >= 8192;
        const bool wideJ = !big && p.Jtot >= 256;
        p.family = CF_WGRAD_X3;
        p.bm = big ? 256 : 128; p.bn = (big || wideJ) ? 256 : 128;
        p.lds = wg_x3_lds_bytes(p.bm, p.bn);
        p.nCot = uda_cdiv(a->Cout, p.bm); p.nJt = uda_cdiv(p.Jtot, p.bn);
        p.nchunks = uda_cdiv(p.P, X3_BK);
        int S = (big ? 512 : (wideJ ? 768 : 1024)) / (p.nCot * p.nJt);
        if (S > p.nchunks / 8) S = p.nchunks / 8;
        if (S > p.S) S = p.S;               // the slab (ws_bytes) holds the fp32 plan's splits
        if (S < 1) S = 1;
        p.cps = uda_cdiv(p.nchunks, S);
        p.S = uda_cdiv(p.nchunks, p.cps);
    }
    p.red_q = p.S > 256 ? 64 : 8;
    return p;
}
