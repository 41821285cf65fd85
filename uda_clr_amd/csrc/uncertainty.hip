// MC-dropout uncertainty maps and the integer tables of calibration and selective prediction, for the evaluation of a checkpoint on a
// labelled target split (include/uda_clr_hip.h).  The trainer trusts a pseudo-label only where the unbiased std over
// T = 8 stochastic passes of sigmoid(x / 2) is below 0.04 (reference utils/Utils.py:159-199); these two entries let that rule be
// scored against labels.
//
//   uda_mc_uncertainty   streams logits [T][n] once and writes up to five maps.  One thread holds the T values of 4 neighbouring
//       elements (1 on the scalar path) in registers: they are loaded as T independent 16-byte loads, each is replaced by its
//       sigmoid(x / 2) while the running sums of sigmoid(x), sigmoid(-x) and H(sigmoid(x)) are formed, and a second pass over the
//       registers gives the sum of squared deviations (in double) - the two-pass variance of torch.std, no cancellation.  T is a template
//       argument (2..32) so that every index is a constant; the outputs wanted are run-time (uniform branches).
//       Per pass one expf: s = exp(-|x| / 2), e = s * s = exp(-|x|);  sigmoid(|x| / 2) = 1 / (1 + s), sigmoid(|x|) = 1 / (1 + e), the
//       values at -|x| are s and e times those.  H(sigmoid(x)) = log1p(e) + |x| e / (1 + e) has only positive terms.  The entropy of
//       the mean is -(p log p + q log q) with q = mean of sigmoid(-x) summed on its own, so that a mean within an ulp of 1 keeps the
//       relative accuracy of its small side.
//   uda_selective_tables  one launch, grid (G, 2 B): a workgroup walks a contiguous slice of one (image, class) plane.  A thread
//       keeps the sums of the bin it is in (confidence bin, uncertainty bin) in registers and hands them to the workgroup's LDS
//       table only when the bin changes - fundus background is one long run of p = 0 - and at the end, where a wave whose lanes all
//       sit in one bin adds its lanes by shuffles first.  Then one global integer add per non-zero LDS entry.  Integers only:
//       the same bits in any order, for an image alone or inside any batch.
#include "common.h"
#include "unc_element.h"         // UncOut, unc_element<T>, unc_u8: shared with tta.hip

#define SEL_BINS 64             // most confidence bins, most uncertainty bins
#define SEL_MAX 1024             // largest supported H and W

// ------------------------------------------------------------------------------------------------ uda_mc_uncertainty
// the per-element statistics (unc_element<T>) and the quantisation (unc_u8) are in unc_element.h
// V = 4: n % 4 == 0 and every pointer aligned for 16-byte words (4-byte words of std_u8); V = 1: anything
template <int T, int V>
__global__ __launch_bounds__(256) void unc_kernel(const float* __restrict__ x, int64_t n, UncOut o) {
    const int64_t items = n / V, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += stride) {
        float xv[T][V];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            if (V == 4) {
                const float4 q = uda_ld4(x + (int64_t)t * n + 4 * i);
                xv[t][0] = q.x, xv[t][1 % V] = q.y, xv[t][2 % V] = q.z, xv[t][3 % V] = q.w;
            } else {
                xv[t][0] = x[(int64_t)t * n + i];
            }
        }
        float r[4][V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float c[T], rj[4];
#pragma unroll
            for (int t = 0; t < T; ++t) c[t] = xv[t][j];
            unc_element<T>(c, o.full, rj);
#pragma unroll
            for (int k = 0; k < 4; ++k) r[k][j] = rj[k];
        }
        float* const outs[4] = {o.mean, o.std_half, o.entropy, o.mi};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!outs[k]) continue;
            if (V == 4)
                uda_st4(outs[k] + 4 * i, make_float4(r[k][0], r[k][1 % V], r[k][2 % V], r[k][3 % V]));
            else
                outs[k][i] = r[k][0];
        }
        if (o.u8) {
            if (V == 4)
                *reinterpret_cast<unsigned*>(o.u8 + 4 * i) = unc_u8(r[1][0], o.u8_scale) | unc_u8(r[1][1 % V], o.u8_scale) << 8 |
                                                            unc_u8(r[1][2 % V], o.u8_scale) << 16 | unc_u8(r[1][3 % V], o.u8_scale) << 24;
            else
                o.u8[i] = (uint8_t)unc_u8(r[1][0], o.u8_scale);
        }
    }
}

template <int T>
static void unc_launch(bool vec, int grid, hipStream_t st, const float* x, int64_t n, const UncOut& o) {
    if (vec)
        hipLaunchKernelGGL((unc_kernel<T, 4>), dim3(grid), dim3(256), 0, st, x, n, o);
    else
        hipLaunchKernelGGL((unc_kernel<T, 1>), dim3(grid), dim3(256), 0, st, x, n, o);
}

template <int T>
static void unc_dispatch(int passes, bool vec, int grid, hipStream_t st, const float* x, int64_t n, const UncOut& o) {
    if (passes == T)
        unc_launch<T>(vec, grid, st, x, n, o);
    else if constexpr (T < UNC_TMAX)
        unc_dispatch<T + 1>(passes, vec, grid, st, x, n, o);
}

extern "C" int uda_mc_uncertainty(const float* logits, int T, int64_t n, float* mean_prob, float* std_half, float* entropy, float* mutual_info,
                                  uint8_t* std_u8, float u8_scale, void* stream) {
    const char* who = "uda_mc_uncertainty";
    UDA_REQUIRE(logits, "%s: null logits", who);
    UDA_REQUIRE(T >= 2 && T <= UNC_TMAX, "%s: %d passes outside 2..%d", who, T, UNC_TMAX);
    UDA_REQUIRE(n > 0 && n <= ((int64_t)1 << 56) / T, "%s: %lld elements per pass", who, (long long)n);
    UDA_REQUIRE(mean_prob || std_half || entropy || mutual_info || std_u8, "%s: no output asked for", who);
    UDA_REQUIRE(!std_u8 || (u8_scale > 0.f && u8_scale < INFINITY), "%s: u8_scale %g is not a positive finite number", who, (double)u8_scale);
    UncOut o = {mean_prob, std_half, entropy, mutual_info, std_u8, u8_scale, (entropy || mutual_info) ? 1 : 0};
    const bool vec = n % 4 == 0 && uda_aligned16(logits) && (!mean_prob || uda_aligned16(mean_prob)) && (!std_half || uda_aligned16(std_half)) &&
                     (!entropy || uda_aligned16(entropy)) && (!mutual_info || uda_aligned16(mutual_info)) &&
                     (reinterpret_cast<uintptr_t>(std_u8) & 3u) == 0;
    const int64_t items = vec ? n / 4 : n;
    const int grid = (int)(items + 255 > (int64_t)2048 * 256 ? 2048 : (items + 255) / 256);
    unc_dispatch<2>(T, vec, grid, (hipStream_t)stream, logits, n, o);
    UDA_LAUNCH_CHECK(who);
    return 0;
}

// ------------------------------------------------------------------------------------------------ uda_selective_tables
struct SelEdges {
    float e[SEL_BINS - 1];
};

struct SelState {
    int b;                                   // confidence bin of the run, -1 before the first valid pixel
    unsigned n, n_pos, q, q_pos;             // a thread sees <= 4096 pixels: sums of q <= 2^28
    unsigned long long qq;
    int k;                                   // uncertainty bin of the run, -1 before the first
    float lo, hi;                            // edges[k - 1] <= u < edges[k] keeps the run
    unsigned c[4];                           // TP, FP, FN, TN
    unsigned bad_p, bad_u;
};

__device__ __forceinline__ void sel_flush_rel(SelState& s, unsigned long long* s_rel) {
    if (s.b >= 0 && s.n) {
        unsigned long long* row = s_rel + s.b * 5;
        atomicAdd(&row[0], (unsigned long long)s.n);
        if (s.n_pos) atomicAdd(&row[1], (unsigned long long)s.n_pos);
        if (s.q) atomicAdd(&row[2], (unsigned long long)s.q);
        if (s.q_pos) atomicAdd(&row[3], (unsigned long long)s.q_pos);
        if (s.qq) atomicAdd(&row[4], s.qq);
    }
    s.n = s.n_pos = s.q = s.q_pos = 0;
    s.qq = 0;
}

__device__ __forceinline__ void sel_flush_risk(SelState& s, unsigned* s_risk) {
    if (s.k >= 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (s.c[i]) atomicAdd(&s_risk[s.k * 4 + i], s.c[i]);
    }
    s.c[0] = s.c[1] = s.c[2] = s.c[3] = 0;
}

__device__ __forceinline__ void sel_pixel(SelState& s, bool want_rel, bool want_risk, float p, float u, bool pr, bool g, int M, float Mf, int K,
                                          const float* s_edge, unsigned long long* s_rel, unsigned* s_risk) {
    if (want_rel) {
        if (!(p >= 0.f && p <= 1.f)) {
            ++s.bad_p;
        } else {
            const int b = min(M - 1, (int)floorf(__fmul_rn(p, Mf)));
            const unsigned q = (unsigned)(int)rintf(p * 65536.0f);
            if (b != s.b) {
                sel_flush_rel(s, s_rel);
                s.b = b;
            }
            ++s.n;
            s.n_pos += g ? 1u : 0u;
            s.q += q;
            s.q_pos += g ? q : 0u;
            s.qq += (unsigned long long)q * q;
        }
    }
    if (want_risk) {
        if (!(u >= 0.f)) {
            ++s.bad_u;
        } else {
            if (!(u >= s.lo && u < s.hi)) {
                sel_flush_risk(s, s_risk);
                int k = 0;
                for (int j = 0; j < K - 1; ++j) k += s_edge[j] <= u ? 1 : 0;
                s.k = k;
                s.lo = k > 0 ? s_edge[k - 1] : -INFINITY;
                s.hi = k < K - 1 ? s_edge[k] : INFINITY;
            }
            s.c[0] += (pr && g) ? 1u : 0u;
            s.c[1] += (pr && !g) ? 1u : 0u;
            s.c[2] += (!pr && g) ? 1u : 0u;
            s.c[3] += (!pr && !g) ? 1u : 0u;
        }
    }
}

template <class V>
__device__ __forceinline__ V sel_wave_sum(V v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// grid (G, 2 B), 256 threads.  VEC: H * W % 4 == 0 and every base aligned for 16-byte words of floats and 4-byte words of masks.
template <bool VEC>
__global__ __launch_bounds__(256) void sel_tables_kernel(const float* __restrict__ prob, const float* __restrict__ unc, const uint8_t* __restrict__ pred,
                                                         const uint8_t* __restrict__ gt, int HW, int M, int K, SelEdges edges,
                                                         unsigned long long* __restrict__ rel, unsigned long long* __restrict__ risk,
                                                         unsigned long long* __restrict__ invalid) {
    __shared__ unsigned long long s_rel[SEL_BINS * 5];
    __shared__ unsigned s_risk[SEL_BINS * 4];
    __shared__ unsigned s_bad[2];
    __shared__ float s_edge[SEL_BINS];
    const int tid = threadIdx.x, plane = blockIdx.y;
    const bool want_rel = rel != nullptr, want_risk = risk != nullptr;
    for (int e = tid; e < SEL_BINS * 5; e += 256) s_rel[e] = 0;
    s_risk[tid] = 0;
    if (tid < 2) s_bad[tid] = 0;
    if (tid < SEL_BINS) s_edge[tid] = tid < K - 1 ? edges.e[tid] : INFINITY;
    __syncthreads();

    const int64_t base = (int64_t)plane * HW;
    const float* P = want_rel ? prob + base : nullptr;
    const float* U = want_risk ? unc + base : nullptr;
    const uint8_t* A = pred + base;
    const uint8_t* G = gt ? gt + base : A;
    const float Mf = (float)M;
    SelState s;
    s.b = s.k = -1;
    s.n = s.n_pos = s.q = s.q_pos = 0;
    s.qq = 0;
    s.lo = INFINITY, s.hi = -INFINITY;                     // no u is inside: the first valid pixel looks its bin up
    s.c[0] = s.c[1] = s.c[2] = s.c[3] = 0;
    s.bad_p = s.bad_u = 0;

    if (VEC) {
        const int words = HW >> 2, per = (words + (int)gridDim.x - 1) / (int)gridDim.x;
        const int w0 = blockIdx.x * per, w1 = min(w0 + per, words);
        for (int w = w0 + tid; w < w1; w += 256) {
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 p4 = want_rel ? uda_ld4(P + 4 * w) : z, u4 = want_risk ? uda_ld4(U + 4 * w) : z;
            const unsigned a4 = reinterpret_cast<const unsigned*>(A)[w], g4 = reinterpret_cast<const unsigned*>(G)[w];
            const float p[4] = {p4.x, p4.y, p4.z, p4.w}, u[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                sel_pixel(s, want_rel, want_risk, p[j], u[j], ((a4 >> (8 * j)) & 0xffu) != 0, ((g4 >> (8 * j)) & 0xffu) != 0, M, Mf, K, s_edge, s_rel,
                          s_risk);
        }
    } else {
        const int per = (HW + (int)gridDim.x - 1) / (int)gridDim.x;
        const int p0 = blockIdx.x * per, p1 = min(p0 + per, HW);
        for (int i = p0 + tid; i < p1; i += 256)
            sel_pixel(s, want_rel, want_risk, want_rel ? P[i] : 0.f, want_risk ? U[i] : 0.f, A[i] != 0, G[i] != 0, M, Mf, K, s_edge, s_rel, s_risk);
    }

    // what the threads still hold: a wave whose 64 lanes sit in one bin adds them by shuffles, and one lane hands the sums over
    if (want_rel) {
        const int b0 = __builtin_amdgcn_readfirstlane(s.b);
        if (__all(s.b == b0)) {
            const unsigned long long n = sel_wave_sum((unsigned long long)s.n), np = sel_wave_sum((unsigned long long)s.n_pos),
                                     q = sel_wave_sum((unsigned long long)s.q), qp = sel_wave_sum((unsigned long long)s.q_pos), qq = sel_wave_sum(s.qq);
            if ((tid & 63) == 0 && b0 >= 0 && n) {
                unsigned long long* row = s_rel + b0 * 5;
                atomicAdd(&row[0], n);
                if (np) atomicAdd(&row[1], np);
                if (q) atomicAdd(&row[2], q);
                if (qp) atomicAdd(&row[3], qp);
                if (qq) atomicAdd(&row[4], qq);
            }
        } else {
            sel_flush_rel(s, s_rel);
        }
        const unsigned bad = sel_wave_sum(s.bad_p);
        if ((tid & 63) == 0 && bad) atomicAdd(&s_bad[0], bad);
    }
    if (want_risk) {
        const int k0 = __builtin_amdgcn_readfirstlane(s.k);
        if (__all(s.k == k0)) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned c = sel_wave_sum(s.c[i]);
                if ((tid & 63) == 0 && k0 >= 0 && c) atomicAdd(&s_risk[k0 * 4 + i], c);
            }
        } else {
            sel_flush_risk(s, s_risk);
        }
        const unsigned bad = sel_wave_sum(s.bad_u);
        if ((tid & 63) == 0 && bad) atomicAdd(&s_bad[1], bad);
    }
    __syncthreads();
    if (want_rel)
        for (int e = tid; e < M * 5; e += 256)
            if (s_rel[e]) atomicAdd(&rel[(int64_t)plane * M * 5 + e], s_rel[e]);
    if (want_risk && tid < K * 4 && s_risk[tid]) atomicAdd(&risk[(int64_t)plane * K * 4 + tid], (unsigned long long)s_risk[tid]);
    if (tid < 2 && s_bad[tid]) atomicAdd(&invalid[(int64_t)plane * 2 + tid], (unsigned long long)s_bad[tid]);
}

extern "C" int uda_selective_tables(const float* prob, const float* unc, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, int M,
                                    const float* edges, int K, int64_t* rel, int64_t* risk, int64_t* invalid, void* stream) {
    const char* who = "uda_selective_tables";
    UDA_REQUIRE(pred && invalid, "%s: null argument", who);
    UDA_REQUIRE(rel || risk, "%s: no table asked for", who);
    UDA_REQUIRE(!rel || prob, "%s: the reliability table needs prob", who);
    UDA_REQUIRE(!risk || unc, "%s: the risk table needs unc", who);
    UDA_REQUIRE(B >= 1 && B <= 8192, "%s: batch %d outside 1..8192", who, B);
    UDA_REQUIRE(H >= 1 && H <= SEL_MAX && W >= 1 && W <= SEL_MAX, "%s: %d x %d outside 1..%d per side", who, H, W, SEL_MAX);
    UDA_REQUIRE(!rel || (M >= 1 && M <= SEL_BINS), "%s: %d confidence bins outside 1..%d", who, M, SEL_BINS);
    SelEdges e;
    for (int j = 0; j < SEL_BINS - 1; ++j) e.e[j] = INFINITY;
    if (risk) {
        UDA_REQUIRE(K >= 1 && K <= SEL_BINS, "%s: %d uncertainty bins outside 1..%d", who, K, SEL_BINS);
        UDA_REQUIRE(K == 1 || edges, "%s: null edges", who);
        for (int j = 0; j < K - 1; ++j) {
            UDA_REQUIRE(edges[j] - edges[j] == 0.f, "%s: edge %d is not finite", who, j);
            UDA_REQUIRE(j == 0 || edges[j - 1] < edges[j], "%s: edges must ascend strictly (edge %d)", who, j);
            e.e[j] = edges[j];
        }
    }
    if (!rel) M = 1;                                       // not read by the kernel then; kept inside the LDS tables all the same
    if (!risk) K = 1;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    if (rel) (void)hipMemsetAsync(rel, 0, (size_t)B * 2 * M * 5 * sizeof(int64_t), st);
    if (risk) (void)hipMemsetAsync(risk, 0, (size_t)B * 2 * K * 4 * sizeof(int64_t), st);
    (void)hipMemsetAsync(invalid, 0, (size_t)B * 4 * sizeof(int64_t), st);
    const bool vec = HW % 4 == 0 && (!rel || uda_aligned16(prob)) && (!risk || uda_aligned16(unc)) && (reinterpret_cast<uintptr_t>(pred) & 3u) == 0 &&
                     (reinterpret_cast<uintptr_t>(gt) & 3u) == 0;
    int G = uda_cdiv(HW, 256 * 32);                        // about 32 pixels per thread: 32 workgroups per 512 x 512 plane
    G = G < 1 ? 1 : G > 128 ? 128 : G;
    if (vec)
        hipLaunchKernelGGL((sel_tables_kernel<true>), dim3(G, 2 * B), dim3(256), 0, st, prob, unc, pred, gt, HW, M, K, e, (unsigned long long*)rel,
                           (unsigned long long*)risk, (unsigned long long*)invalid);
    else
        hipLaunchKernelGGL((sel_tables_kernel<false>), dim3(G, 2 * B), dim3(256), 0, st, prob, unc, pred, gt, HW, M, K, e, (unsigned long long*)rel,
                           (unsigned long long*)risk, (unsigned long long*)invalid);
    UDA_LAUNCH_CHECK(who);
    return 0;
}
