// DRN-D-54 head for gfx950 (networks/backbone/drn.py of the reference): the convolutions no other backbone has.
//   stem7s1_fwd / stem7s1_wgrad   layer0: conv 7x7 stride 1 pad 3, 3 -> 16, NCHW image in, NHWC out (drn.py:124-129)
//   conv3n_fwd / conv3n_wgrad     narrow dense 3x3 (pad 1, dilation 1), 16 | 32 | 64 channels on either side, stride 1 | 2:
//                                 layer1 16 -> 16, layer2 16 -> 32 stride 2 (drn.py:131-134, 196-206) and layer3.0.conv2
//                                 64 -> 64 stride 2 (drn.py:69-71); with flipped, transposed weights the stride-1 form is
//                                 also the input gradient
// 64-byte ... 256-byte pixel rows at full and half image resolution: too narrow for the 32-wide MFMA tiles of igemm_*.hip
// (a 16-channel output fills half a tile).  These kernels are direct convolutions on the VALU: one thread owns ALL output
// channels of its pixel(s) in registers, the input comes from an LDS halo tile (BN + ReLU prologue applied while staging,
// zero border written after it) and the weights - identical for every lane - are read from the constant address space, so
// they arrive through the scalar cache as SGPR operands of v_fmac and cost no LDS or vector-memory traffic.
#include "common.h"

typedef const __attribute__((address_space(4))) float cfloat;      // uniform-index loads from here are scalar loads

__device__ __forceinline__ cfloat* as_const(const float* p) { return (cfloat*)(uintptr_t)p; }

// sum over the 64 lanes of a wave, result in every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// per-channel (sum, sum of squares) of one workgroup of 256 threads: s1 / s2 hold this thread's NC partials.
// fp32 inside the workgroup, fp64 atomics into replica (blockIdx.x mod UDA_STAT_SLOTS) of [SLOTS][2][NC].
template <int NC>
__device__ __forceinline__ void block_stats(const float* s1, const float* s2, float* red /* [4][2 * NC] */, double* stats) {
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float t1 = wave_sum(s1[c]), t2 = wave_sum(s2[c]);
        if (ln == 0) {
            red[wv * 2 * NC + c] = t1;
            red[wv * 2 * NC + NC + c] = t2;
        }
    }
    __syncthreads();
    if (tid < 2 * NC) {
        const float t = red[tid] + red[2 * NC + tid] + red[4 * NC + tid] + red[6 * NC + tid];
        atomicAdd(&stats[(int64_t)(blockIdx.x % UDA_STAT_SLOTS) * 2 * NC + tid], (double)t);
    }
}

// ------------------------------------------------------------------------------------------ 7x7 stride 1, 3 -> 16
struct Stem7s1Args {
    const float* x;   // [N][3][H][W]
    int N, H, W, tiles_h, tiles_w;
    const float* w;   // forward: [7][7][3][16] (tap-major, output channels fastest)
    float* y;
    int64_t ldy;
    double* stats;    // [UDA_STAT_SLOTS][2][16] or null
    const float* dy;
    int64_t lddy;
    float* part;      // wgrad: [gridDim.x][2352], column = co * 147 + ci * 49 + kh * 7 + kw (OIHW)
    int ntiles;
};

#define H7_TH 16
#define H7_TW 64
#define H7_PITCH 72      // >= H7_TW + 6, multiple of 4: a thread's 10 columns are two 16-byte reads and one 8-byte read

// thread = four outputs adjacent along W x all 16 output channels (64 accumulators); per input row the 10 columns under the
// quad feed 7 taps x 4 pixels x 16 channels.
__global__ __launch_bounds__(256) void stem7s1_fwd_kernel(Stem7s1Args a) {
    __shared__ __attribute__((aligned(16))) float xs[3 * (H7_TH + 6) * H7_PITCH];
    __shared__ float red[4 * 32];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x;
    const int tx = tile % a.tiles_w, ty = (tile / a.tiles_w) % a.tiles_h, n = tile / (a.tiles_w * a.tiles_h);
    const int oh0 = ty * H7_TH, ow0 = tx * H7_TW;
    const int64_t plane = (int64_t)a.H * a.W;
    for (int e = tid; e < 3 * (H7_TH + 6) * (H7_TW + 6); e += 256) {
        const int c = e % (H7_TW + 6), r = (e / (H7_TW + 6)) % (H7_TH + 6), ci = e / ((H7_TW + 6) * (H7_TH + 6));
        const int ih = oh0 - 3 + r, iw = ow0 - 3 + c;
        float v = 0.f;
        if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) v = a.x[((int64_t)n * 3 + ci) * plane + (int64_t)ih * a.W + iw];
        xs[(ci * (H7_TH + 6) + r) * H7_PITCH + c] = v;
    }
    __syncthreads();
    cfloat* wc = as_const(a.w);
    const int r = tid >> 4, cq = tid & 15;
    float acc[4][16];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < 16; ++c) acc[j][c] = 0.f;
#pragma unroll 1
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll 1
        for (int kh = 0; kh < 7; ++kh) {
            const float* row = &xs[(ci * (H7_TH + 6) + r + kh) * H7_PITCH + 4 * cq];
            const float4 x0 = uda_ld4(row), x1 = uda_ld4(row + 4);
            const float2 x2 = *reinterpret_cast<const float2*>(row + 8);
            const float xv[10] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w, x2.x, x2.y};
#pragma unroll
            for (int kw = 0; kw < 7; ++kw) {
                cfloat* wp = wc + ((kh * 7 + kw) * 3 + ci) * 16;
#pragma unroll
                for (int c = 0; c < 16; ++c) {
                    const float wv = wp[c];
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j][c] += wv * xv[j + kw];
                }
            }
        }
    const int oh = oh0 + r;
    float s1[16], s2[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) s1[c] = s2[c] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ow = ow0 + 4 * cq + j;
        if (oh < a.H && ow < a.W) {
            float* dst = a.y + (((int64_t)n * a.H + oh) * a.W + ow) * a.ldy;
#pragma unroll
            for (int c = 0; c < 16; c += 4) uda_st4(dst + c, make_float4(acc[j][c], acc[j][c + 1], acc[j][c + 2], acc[j][c + 3]));
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                s1[c] += acc[j][c];
                s2[c] += acc[j][c] * acc[j][c];
            }
        }
    }
    if (a.stats != nullptr) block_stats<16>(s1, s2, red, a.stats);
}

#define H7W_TH 8
#define H7W_PITCH 73      // odd: the (ci, kh) rows a wave reads in one instruction fall into different banks

// dw[co][ci][kh][kw] partials.  thread = (row (ci, kh) of 7 taps, 4 output channels), 84 such threads form one replica and
// the three replicas of a workgroup take the tile's rows in turn; walking along W the 7-wide window slides through
// registers, so a pixel costs one new LDS value and one 16-byte read of dy for 28 FMAs.
__global__ __launch_bounds__(256) void stem7s1_wgrad_kernel(Stem7s1Args a) {
    __shared__ float xs[3 * (H7W_TH + 6) * H7W_PITCH];
    __shared__ __attribute__((aligned(16))) float gs[H7W_TH * H7_TW * 16];      // 32 KiB; reused for the replica sum
    const int tid = threadIdx.x;
    const int rep = tid / 84, role = tid % 84, rk = role >> 2, cog = role & 3;      // rk = ci * 7 + kh; threads 252 .. 255 only stage
    const bool worker = tid < 252;
    const int64_t plane = (int64_t)a.H * a.W;
    float acc[7][4];
#pragma unroll
    for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int tx = tile % a.tiles_w, ty = (tile / a.tiles_w) % a.tiles_h, n = tile / (a.tiles_w * a.tiles_h);
        const int oh0 = ty * H7W_TH, ow0 = tx * H7_TW;
        __syncthreads();
        for (int e = tid; e < 3 * (H7W_TH + 6) * (H7_TW + 6); e += 256) {
            const int c = e % (H7_TW + 6), r = (e / (H7_TW + 6)) % (H7W_TH + 6), ci = e / ((H7_TW + 6) * (H7W_TH + 6));
            const int ih = oh0 - 3 + r, iw = ow0 - 3 + c;
            float v = 0.f;
            if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) v = a.x[((int64_t)n * 3 + ci) * plane + (int64_t)ih * a.W + iw];
            xs[(ci * (H7W_TH + 6) + r) * H7W_PITCH + c] = v;
        }
        for (int e = tid; e < H7W_TH * H7_TW * 4; e += 256) {
            const int q = e & 3, pix = e >> 2, c = pix % H7_TW, r = pix / H7_TW;
            const int oh = oh0 + r, ow = ow0 + c;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (oh < a.H && ow < a.W) g = uda_ld4(a.dy + (((int64_t)n * a.H + oh) * a.W + ow) * a.lddy + 4 * q);
            uda_st4(&gs[pix * 16 + 4 * q], g);
        }
        __syncthreads();
        if (worker) {
#pragma unroll 1
            for (int r = rep; r < H7W_TH; r += 3) {
                const float* xr = &xs[((rk / 7) * (H7W_TH + 6) + r + rk % 7) * H7W_PITCH];
                float win[7];
#pragma unroll
                for (int k = 0; k < 6; ++k) win[k + 1] = xr[k];
#pragma unroll 8
                for (int c = 0; c < H7_TW; ++c) {
#pragma unroll
                    for (int k = 0; k < 6; ++k) win[k] = win[k + 1];
                    win[6] = xr[c + 6];
                    const float4 g = uda_ld4(&gs[(r * H7_TW + c) * 16 + 4 * cog]);
#pragma unroll
                    for (int k = 0; k < 7; ++k) {
                        acc[k][0] += g.x * win[k]; acc[k][1] += g.y * win[k]; acc[k][2] += g.z * win[k]; acc[k][3] += g.w * win[k];
                    }
                }
            }
        }
    }
    // sum of the three replicas through LDS, then this workgroup's row of partials
    __syncthreads();
    float* red = gs;      // [3][84][28]
    if (worker) {
#pragma unroll
        for (int k = 0; k < 7; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[(rep * 84 + role) * 28 + k * 4 + j] = acc[k][j];
    }
    __syncthreads();
    for (int e = tid; e < 84 * 28; e += 256) {
        const int ro = e / 28, k = (e % 28) >> 2, j = e & 3;
        const int rk2 = ro >> 2, co = (ro & 3) * 4 + j;
        a.part[(int64_t)blockIdx.x * 2352 + co * 147 + rk2 * 7 + k] = red[e] + red[84 * 28 + e] + red[2 * 84 * 28 + e];
    }
}

#define H7W_MAX_WG 512

extern "C" uint64_t uda_stem7s1_workspace_bytes(int64_t P) {
    (void)P;
    return uda_wgp_bytes(H7W_MAX_WG, 2352);
}

extern "C" int uda_stem7s1_fwd(const float* x, int N, int H, int W, const float* w_hwio, float* y, int64_t ldy, double* stats,
                               void* stream) {
    UDA_REQUIRE(x && w_hwio && y && uda_aligned16(y) && uda_aligned16(w_hwio) && ldy % 4 == 0 && ldy >= 16 && N > 0 && H > 0 && W > 0,
                "uda_stem7s1_fwd: bad args (16 output channels: ldy >= 16 and a multiple of 4, y 16-byte aligned)");
    Stem7s1Args a = {};
    a.x = x; a.N = N; a.H = H; a.W = W;
    a.tiles_h = uda_cdiv(H, H7_TH); a.tiles_w = uda_cdiv(W, H7_TW);
    a.w = w_hwio; a.y = y; a.ldy = ldy; a.stats = stats;
    const int64_t nt = (int64_t)N * a.tiles_h * a.tiles_w;
    UDA_REQUIRE(nt < ((int64_t)1 << 31), "uda_stem7s1_fwd: too many tiles");
    a.ntiles = (int)nt;
    hipLaunchKernelGGL(stem7s1_fwd_kernel, dim3(a.ntiles), dim3(256), 0, (hipStream_t)stream, a);
    UDA_LAUNCH_CHECK("stem7s1_fwd");
    return 0;
}

extern "C" int uda_stem7s1_wgrad(const float* x, int N, int H, int W, const float* dy, int64_t lddy, float* dw,
                                 float* workspace, uint64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    UDA_REQUIRE(x && dy && dw && uda_aligned16(dy) && lddy % 4 == 0 && lddy >= 16 && N > 0 && H > 0 && W > 0,
                "uda_stem7s1_wgrad: bad args (16 output channels: lddy >= 16 and a multiple of 4, dy 16-byte aligned)");
    UDA_REQUIRE(workspace && uda_aligned16(workspace) && workspace_bytes >= uda_stem7s1_workspace_bytes((int64_t)N * H * W),
                "uda_stem7s1_wgrad: workspace too small");
    Stem7s1Args a = {};
    a.x = x; a.N = N; a.H = H; a.W = W;
    a.tiles_h = uda_cdiv(H, H7W_TH); a.tiles_w = uda_cdiv(W, H7_TW);
    a.dy = dy; a.lddy = lddy;
    const int64_t nt = (int64_t)N * a.tiles_h * a.tiles_w;
    UDA_REQUIRE(nt < ((int64_t)1 << 31), "uda_stem7s1_wgrad: too many tiles");
    a.ntiles = (int)nt;
    const int nwg = a.ntiles < H7W_MAX_WG ? a.ntiles : H7W_MAX_WG, nel = 2352;
    a.part = uda_wgp_part(workspace, nel);
    uda_wgp_zero(workspace, nel, st);
    hipLaunchKernelGGL(stem7s1_wgrad_kernel, dim3(nwg), dim3(256), 0, st, a);
    UDA_LAUNCH_CHECK("stem7s1_wgrad");
    return uda_wgp_finish(workspace, nwg, nel, dw, "stem7s1_wgrad_store", st);
}

// ------------------------------------------------------------------------------------------ narrow dense 3x3
struct Conv3nArgs {
    uda_src_t src;
    int Ho, Wo, tiles_h, tiles_w, ntiles;
    const float* w;   // forward: [3][3][Cin][Cout]
    float* y;
    int64_t ldy;
    double* stats;
    const float* dy;
    int64_t lddy;
    float* part;      // wgrad: [gridDim.x][Cout * Cin * 9] (OIHW columns)
};

// the transformed operand tile: rows [ih0, ih0 + IH) x columns [iw0, iw0 + IW) x channels [c0, c0 + CK) of image n into
// xs[(r * IW + c) * PP + k]; positions outside the image hold 0 (the border is applied AFTER the BN + ReLU prologue)
template <int IH, int IW, int CK, int PP, bool VEC>
__device__ __forceinline__ void stage_tile(const uda_src_t& s, int n, int ih0, int iw0, int c0, float* xs) {
    constexpr int Q = CK / 4;
    for (int e = threadIdx.x; e < IH * IW * Q; e += 256) {
        const int q = e % Q, pix = e / Q, c = pix % IW, r = pix / IW;
        const int ih = ih0 + r, iw = iw0 + c, ch = c0 + 4 * q;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ih >= 0 && ih < s.H && iw >= 0 && iw < s.W) {
            v = uda_ld4(s.x + (((int64_t)n * s.H + ih) * s.W + iw) * s.ldx + ch);
            if (s.scale != nullptr) {
                const float4 sc = uda_ld4(s.scale + ch), sh = uda_ld4(s.shift + ch);
                v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
            }
            v.x = uda_act(v.x, s.act); v.y = uda_act(v.y, s.act); v.z = uda_act(v.z, s.act); v.w = uda_act(v.w, s.act);
        }
        float* d = &xs[pix * PP + 4 * q];
        if (VEC) uda_st4(d, v);
        else { d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w; }
    }
}

#define N3_TW 32

// thread = one output pixel x ALL COUT channels.  The input is staged CK channels at a time (16 at stride 1, 8 at stride 2:
// the stride-2 halo tile covers four times the pixels); per 16-byte LDS read a thread issues 4 * COUT FMAs whose second
// operand is an SGPR.
template <int CIN, int COUT, int S>
__global__ __launch_bounds__(256) void conv3n_fwd_kernel(Conv3nArgs a) {
    constexpr int CK = S == 1 ? 16 : 8, PP = CK + 4, TH = 8;
    constexpr int IH = (TH - 1) * S + 3, IW = (N3_TW - 1) * S + 3;
    __shared__ __attribute__((aligned(16))) float xs[IH * IW * PP];
    __shared__ float red[4 * 2 * COUT];
    const int tid = threadIdx.x, r = tid >> 5, c = tid & 31;
    const int tile = blockIdx.x;
    const int tx = tile % a.tiles_w, ty = (tile / a.tiles_w) % a.tiles_h, n = tile / (a.tiles_w * a.tiles_h);
    const int oh0 = ty * TH, ow0 = tx * N3_TW;
    cfloat* wc = as_const(a.w);
    float acc[COUT];
#pragma unroll
    for (int co = 0; co < COUT; ++co) acc[co] = 0.f;
#pragma unroll 1
    for (int c0 = 0; c0 < CIN; c0 += CK) {
        if (c0) __syncthreads();
        stage_tile<IH, IW, CK, PP, true>(a.src, n, oh0 * S - 1, ow0 * S - 1, c0, xs);
        __syncthreads();
#pragma unroll 1
        for (int t = 0; t < 9; ++t) {
            const int kh = t / 3, kw = t % 3;
            const float* px = &xs[((r * S + kh) * IW + c * S + kw) * PP];
            cfloat* wt = wc + (t * CIN + c0) * COUT;
#pragma unroll
            for (int q = 0; q < CK / 4; ++q) {
                const float4 xv = uda_ld4(px + 4 * q);
                const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    cfloat* wp = wt + (4 * q + j) * COUT;
#pragma unroll
                    for (int co = 0; co < COUT; ++co) acc[co] += wp[co] * xe[j];
                }
            }
        }
    }
    const int oh = oh0 + r, ow = ow0 + c;
    const bool valid = oh < a.Ho && ow < a.Wo;
    if (valid) {
        float* dst = a.y + (((int64_t)n * a.Ho + oh) * a.Wo + ow) * a.ldy;
#pragma unroll
        for (int co = 0; co < COUT; co += 4) uda_st4(dst + co, make_float4(acc[co], acc[co + 1], acc[co + 2], acc[co + 3]));
    }
    if (a.stats != nullptr) {
        float s2[COUT];
#pragma unroll
        for (int co = 0; co < COUT; ++co) {
            acc[co] = valid ? acc[co] : 0.f;
            s2[co] = acc[co] * acc[co];
        }
        block_stats<COUT>(acc, s2, red, a.stats);
    }
}

// dw[co][ci][kh][kw] partials.  blockIdx.y = 16-channel slice of the input; thread = (input channel ci of the slice, 4 output
// channels) with all nine taps in registers (36 accumulators); CK * COUT / 4 such threads form a replica, the replicas of a
// workgroup take the tile's rows in turn.  Walking along W the 3 x 3 window slides through registers: a pixel costs
// 3 * S new LDS values and one 16-byte read of dy for 36 FMAs.
template <int CIN, int COUT, int S>
__global__ __launch_bounds__(256) void conv3n_wgrad_kernel(Conv3nArgs a) {
    constexpr int CK = 16, PP = CK + 1, TH = (S == 1 && COUT < 64) ? 8 : 4;      // (keeps the dy tile within 32 KiB)
    constexpr int IH = (TH - 1) * S + 3, IW = (N3_TW - 1) * S + 3;
    constexpr int NTO = CK * COUT / 4, REP = 256 / NTO;
    constexpr int GS = TH * N3_TW * COUT, RED = 256 * 36;
    __shared__ float xs[IH * IW * PP];
    __shared__ __attribute__((aligned(16))) float gs[GS > RED ? GS : RED];
    const int tid = threadIdx.x, ci = tid % CK, cog = (tid / CK) % (COUT / 4), rep = tid / NTO;
    const int c0 = blockIdx.y * CK;
    float acc[9][4];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = 0.f;
    for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const int tx = tile % a.tiles_w, ty = (tile / a.tiles_w) % a.tiles_h, n = tile / (a.tiles_w * a.tiles_h);
        const int oh0 = ty * TH, ow0 = tx * N3_TW;
        __syncthreads();
        stage_tile<IH, IW, CK, PP, false>(a.src, n, oh0 * S - 1, ow0 * S - 1, c0, xs);
        for (int e = tid; e < TH * N3_TW * (COUT / 4); e += 256) {
            const int q = e % (COUT / 4), pix = e / (COUT / 4), c = pix % N3_TW, r = pix / N3_TW;
            const int oh = oh0 + r, ow = ow0 + c;
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if (oh < a.Ho && ow < a.Wo) g = uda_ld4(a.dy + (((int64_t)n * a.Ho + oh) * a.Wo + ow) * a.lddy + 4 * q);
            uda_st4(&gs[pix * COUT + 4 * q], g);
        }
        __syncthreads();
#pragma unroll 1
        for (int r = rep; r < TH; r += REP) {
            const float* xr = &xs[(r * S * IW) * PP + ci];
            float u[3][3];
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                u[kh][1] = 0.f;
                u[kh][2] = xr[(kh * IW) * PP];                        // column 0 of the tile; slides to kw = 0 below
                if (S == 1) { u[kh][1] = u[kh][2]; u[kh][2] = xr[(kh * IW + 1) * PP]; }
            }
#pragma unroll 8
            for (int c = 0; c < N3_TW; ++c) {
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    if (S == 1) {
                        u[kh][0] = u[kh][1]; u[kh][1] = u[kh][2];
                        u[kh][2] = xr[(kh * IW + c + 2) * PP];
                    } else {
                        u[kh][0] = u[kh][2];
                        u[kh][1] = xr[(kh * IW + 2 * c + 1) * PP];
                        u[kh][2] = xr[(kh * IW + 2 * c + 2) * PP];
                    }
                }
                const float4 g = uda_ld4(&gs[(r * N3_TW + c) * COUT + 4 * cog]);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const float v = u[kh][kw];
                        acc[kh * 3 + kw][0] += g.x * v; acc[kh * 3 + kw][1] += g.y * v;
                        acc[kh * 3 + kw][2] += g.z * v; acc[kh * 3 + kw][3] += g.w * v;
                    }
            }
        }
    }
    // sum of the replicas through LDS, then this workgroup's columns of its row of partials
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) gs[tid * 36 + t * 4 + j] = acc[t][j];
    __syncthreads();
    for (int e = tid; e < NTO * 36; e += 256) {
        float v = 0.f;
#pragma unroll
        for (int p = 0; p < REP; ++p) v += gs[p * NTO * 36 + e];
        const int role = e / 36, t = (e % 36) >> 2, j = e & 3;
        const int ci2 = role % CK, co = (role / CK) * 4 + j;
        a.part[(int64_t)blockIdx.x * (COUT * CIN * 9) + ((int64_t)co * CIN + c0 + ci2) * 9 + t] = v;
    }
}

#define N3_MAX_WG_SMALL 1024      // Cin * Cout <= 512: partial rows of 4608 floats at most
#define N3_MAX_WG_LARGE 256
static inline int n3_max_wg(int Cin, int Cout) { return Cin * Cout <= 512 ? N3_MAX_WG_SMALL : N3_MAX_WG_LARGE; }

static int n3_check(const uda_src_t* s, int Cout, int stride, const char* who) {
    UDA_REQUIRE(s && s->x && uda_aligned16(s->x) && s->N > 0 && s->H > 0 && s->W > 0, "%s: bad src", who);
    UDA_REQUIRE((s->C == 16 || s->C == 32 || s->C == 64) && (Cout == 16 || Cout == 32 || Cout == 64) && (stride == 1 || stride == 2),
                "%s: the narrow 3x3 kernels are built for 16, 32 or 64 channels on either side and stride 1 or 2 (got %d -> %d, stride %d)",
                who, s->C, Cout, stride);
    UDA_REQUIRE(s->ldx % 4 == 0 && s->ldx >= s->C, "%s: src.ldx=%lld must be a multiple of 4 and >= C=%d", who, (long long)s->ldx, s->C);
    UDA_REQUIRE((s->scale == nullptr) == (s->shift == nullptr), "%s: scale/shift must come together", who);
    UDA_REQUIRE(s->scale == nullptr || (uda_aligned16(s->scale) && uda_aligned16(s->shift)), "%s: scale/shift must be 16-byte aligned", who);
    UDA_REQUIRE(s->mask == nullptr, "%s: a dropout mask on the operand is not built (no DRN head layer has one)", who);
    UDA_REQUIRE(s->act >= ACT_NONE && s->act <= ACT_RELU6, "%s: bad activation code", who);
    return 0;
}

#define N3_DISPATCH(KERNEL, CIN, COUT, S, ...)                                          \
    do {                                                                                \
        if (CIN == 16 && COUT == 16 && S == 1) KERNEL(16, 16, 1, __VA_ARGS__);          \
        else if (CIN == 16 && COUT == 16 && S == 2) KERNEL(16, 16, 2, __VA_ARGS__);     \
        else if (CIN == 16 && COUT == 32 && S == 1) KERNEL(16, 32, 1, __VA_ARGS__);     \
        else if (CIN == 16 && COUT == 32 && S == 2) KERNEL(16, 32, 2, __VA_ARGS__);     \
        else if (CIN == 16 && COUT == 64 && S == 1) KERNEL(16, 64, 1, __VA_ARGS__);     \
        else if (CIN == 16 && COUT == 64 && S == 2) KERNEL(16, 64, 2, __VA_ARGS__);     \
        else if (CIN == 32 && COUT == 16 && S == 1) KERNEL(32, 16, 1, __VA_ARGS__);     \
        else if (CIN == 32 && COUT == 16 && S == 2) KERNEL(32, 16, 2, __VA_ARGS__);     \
        else if (CIN == 32 && COUT == 32 && S == 1) KERNEL(32, 32, 1, __VA_ARGS__);     \
        else if (CIN == 32 && COUT == 32 && S == 2) KERNEL(32, 32, 2, __VA_ARGS__);     \
        else if (CIN == 32 && COUT == 64 && S == 1) KERNEL(32, 64, 1, __VA_ARGS__);     \
        else if (CIN == 32 && COUT == 64 && S == 2) KERNEL(32, 64, 2, __VA_ARGS__);     \
        else if (CIN == 64 && COUT == 16 && S == 1) KERNEL(64, 16, 1, __VA_ARGS__);     \
        else if (CIN == 64 && COUT == 16 && S == 2) KERNEL(64, 16, 2, __VA_ARGS__);     \
        else if (CIN == 64 && COUT == 32 && S == 1) KERNEL(64, 32, 1, __VA_ARGS__);     \
        else if (CIN == 64 && COUT == 32 && S == 2) KERNEL(64, 32, 2, __VA_ARGS__);     \
        else if (CIN == 64 && COUT == 64 && S == 1) KERNEL(64, 64, 1, __VA_ARGS__);     \
        else KERNEL(64, 64, 2, __VA_ARGS__);                                            \
    } while (0)

#define N3_LAUNCH_FWD(CI, CO, S, grid, st, a) hipLaunchKernelGGL((conv3n_fwd_kernel<CI, CO, S>), grid, dim3(256), 0, st, a)
#define N3_LAUNCH_WGRAD(CI, CO, S, grid, st, a) hipLaunchKernelGGL((conv3n_wgrad_kernel<CI, CO, S>), grid, dim3(256), 0, st, a)

extern "C" int uda_conv3n_fwd(const uda_src_t* src, const float* w_hwio, int Cout, int stride, float* y, int64_t ldy,
                              double* stats, void* stream) {
    if (int e = n3_check(src, Cout, stride, "uda_conv3n_fwd")) return e;
    UDA_REQUIRE(w_hwio && uda_aligned16(w_hwio) && y && uda_aligned16(y) && ldy % 4 == 0 && ldy >= Cout,
                "uda_conv3n_fwd: y must be 16-byte aligned with ldy >= Cout and a multiple of 4");
    Conv3nArgs a = {};
    a.src = *src;
    a.Ho = (src->H - 1) / stride + 1; a.Wo = (src->W - 1) / stride + 1;
    a.tiles_h = uda_cdiv(a.Ho, 8); a.tiles_w = uda_cdiv(a.Wo, N3_TW);
    const int64_t nt = (int64_t)src->N * a.tiles_h * a.tiles_w;
    UDA_REQUIRE(nt < ((int64_t)1 << 31), "uda_conv3n_fwd: too many tiles");
    a.ntiles = (int)nt;
    a.w = w_hwio; a.y = y; a.ldy = ldy; a.stats = stats;
    const int Cin = src->C;
    N3_DISPATCH(N3_LAUNCH_FWD, Cin, Cout, stride, dim3(a.ntiles), (hipStream_t)stream, a);
    UDA_LAUNCH_CHECK("conv3n_fwd");
    return 0;
}

extern "C" uint64_t uda_conv3n_workspace_bytes(int Cin, int Cout) {
    return uda_wgp_bytes(n3_max_wg(Cin, Cout), (int64_t)Cin * Cout * 9);
}

extern "C" int uda_conv3n_wgrad(const uda_src_t* src, const float* dy, int64_t lddy, int Cout, int stride, float* dw,
                                float* workspace, uint64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (int e = n3_check(src, Cout, stride, "uda_conv3n_wgrad")) return e;
    UDA_REQUIRE(dy && uda_aligned16(dy) && lddy % 4 == 0 && lddy >= Cout && dw,
                "uda_conv3n_wgrad: dy must be 16-byte aligned with lddy >= Cout and a multiple of 4");
    const int Cin = src->C;
    UDA_REQUIRE(workspace && uda_aligned16(workspace) && workspace_bytes >= uda_conv3n_workspace_bytes(Cin, Cout),
                "uda_conv3n_wgrad: workspace too small");
    Conv3nArgs a = {};
    a.src = *src;
    a.Ho = (src->H - 1) / stride + 1; a.Wo = (src->W - 1) / stride + 1;
    a.tiles_h = uda_cdiv(a.Ho, (stride == 1 && Cout < 64) ? 8 : 4); a.tiles_w = uda_cdiv(a.Wo, N3_TW);
    const int64_t nt = (int64_t)src->N * a.tiles_h * a.tiles_w;
    UDA_REQUIRE(nt < ((int64_t)1 << 31), "uda_conv3n_wgrad: too many tiles");
    a.ntiles = (int)nt;
    a.dy = dy; a.lddy = lddy;
    const int nel = Cin * Cout * 9, cap = n3_max_wg(Cin, Cout);
    const int nwg = a.ntiles < cap ? a.ntiles : cap;
    a.part = uda_wgp_part(workspace, nel);
    uda_wgp_zero(workspace, nel, st);
    N3_DISPATCH(N3_LAUNCH_WGRAD, Cin, Cout, stride, dim3(nwg, Cin / 16), st, a);
    UDA_LAUNCH_CHECK("conv3n_wgrad");
    return uda_wgp_finish(workspace, nwg, nel, dw, "conv3n_wgrad_store", st);
}
