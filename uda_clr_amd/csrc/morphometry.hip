// Optic-disc morphometry of a (cup, disc) mask pair per image on the device: the integers that the cup-to-disc ratios (vertical,
// horizontal, area), the rim-to-disc profile around the disc, the cup's decentration and an ellipse summary of each structure are
// closed forms of (uda_clr_amd/utils/metrics.py, morphometry_from_moments).  The reference has none of these figures; the
// definitions are this project's (include/uda_clr_hip.h).
//
//   Everything is an integer: sums and maxima give the same bits in any order, so the outputs are bit-identical from run to run
//   and an image's rows do not depend on the batch it sits in.  No floating-point atomics; the only floating-point instruction is
//   the atan2f that GUESSES a pixel's sector, which the integer cross tests then decide.
//
//   Three launches in stream order, MORPH_G workgroups per image in the two that read the masks:
//     0. init     moments = 0, overlap = 0, radial = -1, the extent words of the workspace = 0;
//     1. moments  per class n, sum r, sum c, sum r^2, sum c^2, sum r*c, the pixels set in both planes, and the extents as maxima
//                 of (H - r, r + 1, W - c, c + 1) so that 0 means "no pixel": per thread in registers, per wave by shuffles, per
//                 workgroup by LDS atomics, then one global integer atomic per non-zero word;
//     2. radial   reads the disc's (n, sum r, sum c) that launch 1 left, u = (n * c - sum c, -(n * r - sum r)) per set pixel, its
//                 sector, and the largest |u|^2 per (class, sector) in an LDS table of [2][K] int64 (<= 5.6 KiB), then one global
//                 atomicMax per entry that holds a pixel.  Workgroup 0 of every image also decodes the extents.
//   The masks are read in 16-byte words where W is a multiple of 16 and the base is aligned (a word then lies inside one row),
//   byte by byte otherwise.  Both planes of an image are walked together: the overlap needs both bytes of a pixel.
#include "common.h"

#define MORPH_MAX 1024           // largest supported H and W (that of uda_surface_distance)
#define MORPH_KMAX 360           // most sectors
#define MORPH_G 16               // workgroups per image: 512 x 512 = 16384 words per plane, 4 per thread
#define MORPH_SUMS 13            // 2 x 6 moments and the overlap

static inline size_t morph_align(size_t n) { return (n + 255) & ~(size_t)255; }

// f(r, c, cup set, disc set) for every pixel of this workgroup's slice of image planes `cup` and `disc` with either set
template <class F>
__device__ __forceinline__ void morph_walk(const uint8_t* __restrict__ cup, const uint8_t* __restrict__ disc, int H, int W, F f) {
    const int HW = H * W;                                  // <= 2^20
    if ((W & 15) == 0 && uda_aligned16_dev(cup)) {         // disc = cup + H * W is aligned with it
        const uint4* A = (const uint4*)cup;
        const uint4* D = (const uint4*)disc;
        const int words = HW >> 4, per = (words + (int)gridDim.x - 1) / (int)gridDim.x;
        const int w0 = blockIdx.x * per, w1 = min(w0 + per, words);
        for (int w = w0 + threadIdx.x; w < w1; w += 256) {
            const uint4 qa = A[w], qd = D[w];
            const unsigned wa[4] = {qa.x, qa.y, qa.z, qa.w}, wd[4] = {qd.x, qd.y, qd.z, qd.w};
            const int p = w << 4, r = p / W, c0 = p - r * W;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!(wa[k] | wd[k])) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool a = ((wa[k] >> (8 * j)) & 0xffu) != 0, d = ((wd[k] >> (8 * j)) & 0xffu) != 0;
                    if (a || d) f(r, c0 + k * 4 + j, a, d);
                }
            }
        }
    } else {
        const int per = (HW + (int)gridDim.x - 1) / (int)gridDim.x;
        const int p0 = blockIdx.x * per, p1 = min(p0 + per, HW);
        for (int p = p0 + threadIdx.x; p < p1; p += 256) {
            const bool a = cup[p] != 0, d = disc[p] != 0;
            if (a || d) {
                const int r = p / W;
                f(r, p - r * W, a, d);
            }
        }
    }
}

// ---- 0. initial values.  One thread per word of the longest array.
__global__ __launch_bounds__(256) void morph_init_kernel(int B, int K, long long* __restrict__ moments, long long* __restrict__ overlap,
                                                         long long* __restrict__ radial, unsigned* __restrict__ ext) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < (int64_t)B * 12) moments[e] = 0;
    if (e < B) overlap[e] = 0;
    if (e < (int64_t)B * 2 * K) radial[e] = -1;
    if (e < (int64_t)B * 8) ext[e] = 0;
}

// ---- 1. moments, overlap, extents.  grid (MORPH_G, B).
__global__ __launch_bounds__(256) void morph_moments_kernel(const uint8_t* __restrict__ masks, int H, int W, unsigned long long* __restrict__ moments,
                                                            unsigned long long* __restrict__ overlap, unsigned* __restrict__ ext) {
    __shared__ unsigned long long s_sum[MORPH_SUMS];
    __shared__ unsigned s_ext[8];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* cup = masks + (int64_t)b * 2 * HW;
    if (tid < MORPH_SUMS) s_sum[tid] = 0;
    if (tid < 8) s_ext[tid] = 0;
    __syncthreads();

    unsigned long long v[MORPH_SUMS];                      // [class][n, r, c, rr, cc, rc], overlap
    unsigned x[8];                                         // [class][H - r, r + 1, W - c, c + 1], 0 = no pixel
#pragma unroll
    for (int i = 0; i < MORPH_SUMS; ++i) v[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = 0;
    morph_walk(cup, cup + HW, H, W, [&](int r, int c, bool a, bool d) {
        const unsigned rr = r * r, cc = c * c, rc = r * c;  // < 2^20
        const unsigned e[4] = {(unsigned)(H - r), (unsigned)(r + 1), (unsigned)(W - c), (unsigned)(c + 1)};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const unsigned m = (k ? d : a) ? 1u : 0u;
            v[k * 6 + 0] += m;
            v[k * 6 + 1] += m * (unsigned)r;
            v[k * 6 + 2] += m * (unsigned)c;
            v[k * 6 + 3] += m * rr;
            v[k * 6 + 4] += m * cc;
            v[k * 6 + 5] += m * rc;
#pragma unroll
            for (int i = 0; i < 4; ++i) x[k * 4 + i] = max(x[k * 4 + i], m * e[i]);
        }
        v[12] += (a && d) ? 1u : 0u;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int i = 0; i < MORPH_SUMS; ++i) v[i] += __shfl_down(v[i], o);
#pragma unroll
        for (int i = 0; i < 8; ++i) x[i] = max(x[i], __shfl_down(x[i], o));
    }
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < MORPH_SUMS; ++i)
            if (v[i]) atomicAdd(&s_sum[i], v[i]);
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (x[i]) atomicMax(&s_ext[i], x[i]);
    }
    __syncthreads();
    if (tid < 12 && s_sum[tid]) atomicAdd(&moments[(int64_t)b * 12 + tid], s_sum[tid]);
    if (tid == 12 && s_sum[12]) atomicAdd(&overlap[b], s_sum[12]);
    if (tid >= 64 && tid < 72 && s_ext[tid - 64]) atomicMax(&ext[(int64_t)b * 8 + tid - 64], s_ext[tid - 64]);
}

// ---- 2. the largest |u|^2 per (class, sector), and the extents' decoding.  grid (MORPH_G, B).
__device__ __forceinline__ long long morph_cross(long long ax, long long ay, long long ux, long long uy) { return ax * uy - ay * ux; }

__global__ __launch_bounds__(256) void morph_radial_kernel(const uint8_t* __restrict__ masks, int H, int W, const long long* __restrict__ sectors, int K,
                                                           const long long* __restrict__ moments, const unsigned* __restrict__ ext,
                                                           long long* __restrict__ extent, long long* __restrict__ radial) {
    __shared__ long long s_x[MORPH_KMAX], s_y[MORPH_KMAX], s_max[2 * MORPH_KMAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t HW = (int64_t)H * W;
    const uint8_t* cup = masks + (int64_t)b * 2 * HW;
    if (blockIdx.x == 0 && tid < 8) {                      // [class][first row, last row, first column, last column]
        const unsigned e = ext[(int64_t)b * 8 + tid];
        const int i = tid & 3;
        extent[(int64_t)b * 8 + tid] = e == 0 ? -1ll : i == 0 ? (long long)H - e : i == 2 ? (long long)W - e : (long long)e - 1;
    }
    const long long n = moments[(int64_t)b * 12 + 6], Sr = moments[(int64_t)b * 12 + 7], Sc = moments[(int64_t)b * 12 + 8];
    if (n == 0) return;                                    // the same for every thread; radial keeps its -1
    for (int j = tid; j < K; j += 256) {
        s_x[j] = sectors[2 * j];
        s_y[j] = sectors[2 * j + 1];
    }
    for (int e = tid; e < 2 * K; e += 256) s_max[e] = -1;
    __syncthreads();
    const float per_rad = (float)K * 0.15915494309189535f;  // K / (2 pi)
    morph_walk(cup, cup + HW, H, W, [&](int r, int c, bool a, bool d) {
        const long long ux = n * c - Sc, uy = -(n * r - Sr);
        if (ux == 0 && uy == 0) return;                    // the centroid itself is in no sector
        int j = (int)floorf(atan2f((float)uy, (float)ux) * per_rad) % K;      // a guess within a sector or two of the answer
        if (j < 0) j += K;
        for (int it = 0; it < K; ++it) {                   // decided by integers: cross(s_j, u) >= 0 and cross(s_j+1, u) < 0
            const int jn = j + 1 == K ? 0 : j + 1;
            if (morph_cross(s_x[j], s_y[j], ux, uy) < 0)
                j = j == 0 ? K - 1 : j - 1;
            else if (morph_cross(s_x[jn], s_y[jn], ux, uy) >= 0)
                j = jn;
            else
                break;
        }
        const long long d2 = ux * ux + uy * uy;
        if (a) atomicMax(&s_max[j], d2);
        if (d) atomicMax(&s_max[K + j], d2);
    });
    __syncthreads();
    for (int e = tid; e < 2 * K; e += 256)
        if (s_max[e] >= 0) atomicMax(&radial[(int64_t)b * 2 * K + e], s_max[e]);
}

extern "C" size_t uda_disc_morphometry_workspace_bytes(int B, int H, int W, int K) {
    if (B <= 0 || H <= 0 || W <= 0 || K <= 0) return 0;
    return morph_align((size_t)B * 8 * sizeof(unsigned));
}

extern "C" int uda_disc_morphometry(const uint8_t* masks, int B, int H, int W, const int64_t* sectors, int K, int64_t* moments, int64_t* extent,
                                    int64_t* overlap, int64_t* radial, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "uda_disc_morphometry";
    UDA_REQUIRE(masks && sectors && moments && extent && overlap && radial && workspace, "%s: null argument", who);
    UDA_REQUIRE(B >= 1 && B <= 8192, "%s: batch %d outside 1..8192", who, B);
    UDA_REQUIRE(H >= 1 && H <= MORPH_MAX && W >= 1 && W <= MORPH_MAX, "%s: %d x %d outside 1..%d per side", who, H, W, MORPH_MAX);
    UDA_REQUIRE(K >= 8 && K <= MORPH_KMAX && K % 8 == 0, "%s: %d sectors: a multiple of 8 in 8..%d", who, K, MORPH_KMAX);
    UDA_REQUIRE(workspace_bytes >= uda_disc_morphometry_workspace_bytes(B, H, W, K), "%s: workspace too small (%zu < %zu B)", who, workspace_bytes,
                uda_disc_morphometry_workspace_bytes(B, H, W, K));
    hipStream_t st = (hipStream_t)stream;
    unsigned* ext = (unsigned*)workspace;
    const int64_t longest = (int64_t)B * 2 * K;            // 2 * K >= 16 > 12: radial is the longest array
    hipLaunchKernelGGL(morph_init_kernel, dim3(uda_cdiv(longest, 256)), dim3(256), 0, st, B, K, (long long*)moments, (long long*)overlap,
                       (long long*)radial, ext);
    hipLaunchKernelGGL(morph_moments_kernel, dim3(MORPH_G, B), dim3(256), 0, st, masks, H, W, (unsigned long long*)moments,
                       (unsigned long long*)overlap, ext);
    hipLaunchKernelGGL(morph_radial_kernel, dim3(MORPH_G, B), dim3(256), 0, st, masks, H, W, (const long long*)sectors, K,
                       (const long long*)moments, (const unsigned*)ext, (long long*)extent, (long long*)radial);
    UDA_LAUNCH_CHECK(who);
    return 0;
}
