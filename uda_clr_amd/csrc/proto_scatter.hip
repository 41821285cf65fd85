// Class feature scatter matrices for the domain-gap report (uda_clr_amd/domain_gap.py):
//     S_k[i][j] += sum_p w_k[p] (f[p,i] - a_k[i]) (f[p,j] - a_k[j]),   k < 4,  i, j < C
// on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: bitwise an fmaf chain over the pixels), fp32 per slab of PS_SLAB pixels, fp64
// across slabs and splits in a fixed order, no atomics.  The tile / slab / workspace arithmetic is scatter_plan.h.
#include "common.h"
#include "scatter_plan.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

// first linear index of block row bi among the pairs (bi, bj >= bi) of nb blocks
__host__ __device__ static inline int ps_pair_base(int bi, int nb) { return bi * nb - bi * (bi - 1) / 2; }

struct PsArgs {
    const float* f;
    int64_t ldf, P;
    int C;
    const float* wts;
    const float* centre;
    double* part;
    int nb, npair;
    int64_t span;          // pixels per split: a multiple of PS_SLAB
};

// One workgroup's block pair (bi, bj) over the pixels [p0, p1).  DIAG (bi == bj): the B side reads the A side's 64 channels, the
// second 64 columns of the LDS rows are not staged, and the lower-left 32 x 32 tile is not computed.
template <bool DIAG>
__device__ __forceinline__ void ps_block_pair(const PsArgs& a, float* tile, float* wl, int bi, int bj, int64_t p0, int64_t p1, double* part) {
    const int tid = threadIdx.x, k = tid >> 6, lane = tid & 63, r = lane & 31, kh = lane >> 5;
    const int C = a.C;

    // this lane's centre values: rows bi * 64 + 32 t + r of class k on the A side, columns bj * 64 + 32 u + r on the B side
    float ca[2], cb[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int ci = bi * PS_MT + 32 * t + r, cj = bj * PS_MT + 32 * t + r;
        ca[t] = a.centre && ci < C ? a.centre[(int64_t)k * C + ci] : 0.f;
        cb[t] = a.centre && cj < C ? a.centre[(int64_t)k * C + cj] : 0.f;
    }

    // staging: thread -> float4 column c4 of the 2 x 64 channels (16 per block) and pixel rows prow + 8 q of the chunk.
    // Every load is unconditional and in range - an unused column reads column 0, a pixel behind the range reads pixel p1 - 1 - and
    // what must not reach a result is replaced by zeros when the registers are staged, so nothing waits on a load before that.
    const int c4 = tid & 31, prow = tid >> 5;
    const int ch0 = (c4 < 16 ? bi * PS_MT : bj * PS_MT - PS_MT) + c4 * 4;
    const bool col_used = (c4 < 16 || !DIAG) && ch0 < C;          // ch0 % 4 == 0: ch0 < C is ch0 < round4(C), the last lane read
    const bool keep_y = ch0 + 1 < C, keep_z = ch0 + 2 < C, keep_w = ch0 + 3 < C;     // lanes C .. round4(C)-1 may hold anything
    const float* fcol = a.f + (col_used ? ch0 : 0);
    float4 pf[PS_KP / 8], pw;
    auto fetch = [&](int64_t pc) {
#pragma unroll
        for (int q = 0; q < PS_KP / 8; ++q) pf[q] = uda_ld4(fcol + min(pc + prow + 8 * q, p1 - 1) * a.ldf);
        pw = uda_ld4(a.wts + min(pc + (tid & (PS_KP - 1)), p1 - 1) * 4);
    };
    auto stage = [&](int64_t pc, int image) {
#pragma unroll
        for (int q = 0; q < PS_KP / 8; ++q) {
            const bool ok = col_used && pc + prow + 8 * q < p1;
            const float4 v = pf[q];
            uda_st4(&tile[image * (PS_KP * PS_LD) + (prow + 8 * q) * PS_LD + c4 * 4],
                    make_float4(ok ? v.x : 0.f, ok && keep_y ? v.y : 0.f, ok && keep_z ? v.z : 0.f, ok && keep_w ? v.w : 0.f));
        }
        if (tid < PS_KP) uda_st4(&wl[image * (PS_KP * 4) + tid * 4], pc + tid < p1 ? pw : make_float4(0.f, 0.f, 0.f, 0.f));
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][u][e] = 0.f;

    double* mine = part + (int64_t)k * (PS_MT * PS_MT);
    bool first = true;
    // acc -> this wave's fp64 partial tile (written by the first slab, added into by the later ones), then cleared
    auto flush = [&]() {
        double* dst = mine;
        asm volatile("" : "+v"(dst));                            // opaque: the 48 tile addresses are formed here, not kept in registers across the main loop
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (DIAG && t == 1 && u == 0) continue;
                double old[16];                                  // a later slab: all 16 loads in flight together, then the adds
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    // C/D layout: col = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
                    const int row = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * kh, col = 32 * u + r;
                    old[e] = first ? 0.0 : dst[row * PS_MT + col];
                }
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = 32 * t + (e & 3) + 8 * (e >> 2) + 4 * kh, col = 32 * u + r;
                    dst[row * PS_MT + col] = old[e] + (double)acc[t][u][e];
                    acc[t][u][e] = 0.f;
                }
            }
        first = false;
    };

    constexpr int boff = DIAG ? 0 : PS_MT;
    int in_slab = 0, cur = 0;
    fetch(p0);
    stage(p0, 0);
    __syncthreads();
    // chunk c is read from LDS image c & 1 while chunk c + 1 is loaded (before the math) and staged into the other image (after
    // it): the loads have the whole math to arrive, and one barrier per chunk separates an image's readers from its next writers
    for (int64_t pc = p0; pc < p1; pc += PS_KP) {
        const bool more = pc + PS_KP < p1;
        if (more) fetch(pc + PS_KP);
        const float* img = tile + cur * (PS_KP * PS_LD);
        const float* wimg = wl + cur * (PS_KP * 4);
#pragma unroll
        for (int s = 0; s < PS_KP / 2; ++s) {
            const float* row = &img[(2 * s + kh) * PS_LD];
            const float w = wimg[(2 * s + kh) * 4 + k];
            float av[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                av[t] = w * (row[32 * t + r] - ca[t]);
                bv[t] = row[boff + 32 * t + r] - cb[t];
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (DIAG && t == 1 && u == 0) continue;
                    acc[t][u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], bv[u], acc[t][u], 0, 0, 0);
                }
        }
        if (more) stage(pc + PS_KP, cur ^ 1);
        in_slab += PS_KP;
        if (in_slab == PS_SLAB) {
            flush();
            in_slab = 0;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (in_slab || first) flush();
}

// two workgroups per CU (2 waves per SIMD, <= 256 registers): one's staging and barriers hide behind the other's MFMAs
__global__ __launch_bounds__(256, 2) void proto_scatter_kernel(PsArgs a) {
    __shared__ float tile[2 * PS_KP * PS_LD];       // two images of a chunk: one read, one staged
    __shared__ float wl[2 * PS_KP * 4];
    // the pairs of one split are neighbours in the logical order: they read the same pixels through the same L2
    const int logical = uda_xcd_remap(blockIdx.x, gridDim.x);
    const int split = logical / a.npair, pair = logical % a.npair;
    int bi = 0;
    while (pair >= ps_pair_base(bi + 1, a.nb)) ++bi;
    const int bj = bi + (pair - ps_pair_base(bi, a.nb));
    const int64_t p0 = (int64_t)split * a.span, p1 = min(a.P, p0 + a.span);
    double* part = a.part + ((int64_t)split * a.npair + pair) * 4 * (PS_MT * PS_MT);
    if (bi == bj) ps_block_pair<true>(a, tile, wl, bi, bj, p0, p1, part);
    else ps_block_pair<false>(a, tile, wl, bi, bj, p0, p1, part);
}

// scatter[k][i][j] and [k][j][i] += sum over the nsplit partial sets, in split order, of the one partial computed for i <= j
__global__ __launch_bounds__(256) void proto_scatter_combine_kernel(const double* __restrict__ part, int nsplit, int npair, int nb, int C,
                                                                    double* __restrict__ scatter) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)4 * C * C) return;
    const int j = (int)(e % C), i = (int)((e / C) % C), k = (int)(e / ((int64_t)C * C));
    if (i > j) return;
    const int bi = i / PS_MT, bj = j / PS_MT, pair = ps_pair_base(bi, nb) + (bj - bi);
    const double* src = part + ((int64_t)pair * 4 + k) * (PS_MT * PS_MT) + (i % PS_MT) * PS_MT + (j % PS_MT);
    double t = 0.0;
    for (int s = 0; s < nsplit; ++s) t += src[(int64_t)s * npair * 4 * (PS_MT * PS_MT)];
    scatter[((int64_t)k * C + i) * C + j] += t;
    if (i != j) scatter[((int64_t)k * C + j) * C + i] += t;
}

extern "C" uint64_t uda_proto_scatter_workspace_bytes(int C) { return C >= 1 && C <= PS_MAX_C ? ps_workspace_bytes(C) : 0; }

extern "C" int uda_proto_scatter(const float* feat, int64_t ldf, int64_t P, int C, const float* wts, const float* centre,
                                 double* scatter, void* workspace, uint64_t workspace_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    UDA_REQUIRE(C >= 1 && C <= PS_MAX_C && P >= 1, "uda_proto_scatter: needs 1 <= C <= %d and P >= 1", PS_MAX_C);
    UDA_REQUIRE(feat && uda_aligned16(feat) && ldf % 4 == 0 && ldf >= ((C + 3) / 4) * 4 && wts && uda_aligned16(wts) && scatter,
                "uda_proto_scatter: bad args");
    UDA_REQUIRE(workspace && uda_aligned16(workspace) && workspace_bytes >= ps_workspace_bytes(C), "uda_proto_scatter: workspace too small");
    const int nb = ps_nblk(C), npair = ps_npair(C);
    const int64_t per = (P + ps_nsplit(C) - 1) / ps_nsplit(C);
    const int64_t span = (per + PS_SLAB - 1) / PS_SLAB * PS_SLAB;
    const int nsplit = (int)((P + span - 1) / span);               // <= ps_nsplit(C), and every split has a pixel
    PsArgs a{feat, ldf, P, C, wts, centre, (double*)workspace, nb, npair, span};
    hipLaunchKernelGGL(proto_scatter_kernel, dim3(nsplit * npair), dim3(256), 0, st, a);
    UDA_LAUNCH_CHECK("proto_scatter");
    hipLaunchKernelGGL(proto_scatter_combine_kernel, dim3(uda_cdiv((int64_t)4 * C * C, 256)), dim3(256), 0, st, (const double*)workspace,
                       nsplit, npair, nb, C, scatter);
    UDA_LAUNCH_CHECK("proto_scatter_combine");
    return 0;
}
