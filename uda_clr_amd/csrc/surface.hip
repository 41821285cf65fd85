// Exact surface distances between a predicted and a ground-truth mask on the device: the table behind the per-image
// average (symmetric) surface distance and Hausdorff distance of the evaluation (uda_clr_amd/evaluate.py).
//
//   The reference's utils/metrics.py:62-68 keeps `_upscan`, the 1-D scan of a squared distance transform, but ships none of
//   its callers; the masks scored are those of utils/Utils.py:438-463 (postprocessing).  The conventions are
//   medpy.metric.binary's (include/uda_clr_hip.h): border(M) = M & ~erode4(M) with the outside of the image unset, distances
//   in pixels from every border pixel of one mask to the nearest border pixel of the other.
//
//   Per (image, class) there are two border sets (slot 0: ground truth, slot 1: prediction) and one squared distance map to
//   each.  Four passes, all integer until the last:
//     1. border   bytes of both border sets; the three Dice counts by integer atomics (order cannot change an integer sum);
//     2. row      g[y,x] = distance to the nearest border pixel of row y (uint16, SURF_NONE when the row has none): one wave
//                 per row, every lane scans a run of <= 16 pixels, the runs are joined by a wave-wide prefix max / suffix min;
//     3. column   d2[y,x] = min_y' (y - y')^2 + g[y',x]^2, the separable form of the exact Euclidean transform, by brute
//                 force over the rows that have border pixels at all.  g^2 of a 16-column strip sits in LDS (H * 64 B, 64 KiB
//                 at H = 1024: two workgroups per CU; 32 KiB at 512: five); a thread keeps 8 consecutive output rows in
//                 registers so one LDS read feeds 8 candidates.  Everything fits int32: (y-y')^2 + g^2 <= 2 * 1023^2.
//                 A plane without border pixels gets d2 = -1 everywhere.
//     4. gather   over the border pixels of one set: n, max d2 (integer) and sum sqrt((double)d2).  The sum has a FIXED order:
//                 SURF_G workgroups per (image, class, direction), each over its own slice of the plane, thread-strided inside
//                 and folded by a fixed tree, write partials into fixed slots; surf_combine_kernel adds the slots in index
//                 order.  No floating-point atomics: the table is bit-identical from run to run, and the slices depend on
//                 H * W only, so an image's rows do not depend on the batch it sits in.
//   uda_surface_profile runs a fifth pass after these, over the border bytes and d2 maps the workspace already holds:
//     5. profile  per (image, class), integers only: order statistics of the squared distances (directed and pooled) by a
//                 three-level radix select over 7-bit digits (d2 < 2^21), the number of border pixels within each squared
//                 tolerance, and the row extent of both masks.  One workgroup per (image, class), LDS integer atomics only.
#include "common.h"

#define SURF_MAX 1024            // largest supported H and W
#define SURF_NONE 0xFFFFu        // row pass: no border pixel in this row
#define SURF_INF (1 << 30)       // column pass: g^2 of SURF_NONE; + (y-y')^2 < 2^21 cannot overflow
#define SURF_SW 16               // columns per strip of the column pass
#define SURF_RT 8                // output rows per thread of the column pass
#define SURF_ROWS (256 / SURF_SW * SURF_RT)      // output rows per workgroup of the column pass (128)
#define SURF_G 32                // gather workgroups (= partial slots) per (image, class, direction)

struct SurfPartial {
    double s;
    long long n;
    long long m;
};

// ---- 1. border sets and Dice counts.  plane = b * 2 + class; border slot 0 = ground truth, 1 = prediction.
__global__ __launch_bounds__(256) void surf_border_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt, int H, int W,
                                                          uint8_t* __restrict__ border, unsigned long long* __restrict__ counts) {
    __shared__ int red[3][4];
    const int plane = blockIdx.y;
    const int64_t HW = (int64_t)H * W, p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint8_t* P = pred + plane * HW;
    const uint8_t* G = gt + plane * HW;
    int a = 0, g = 0;
    if (p < HW) {
        const int y = (int)(p / W), x = (int)(p % W);
        a = P[p] != 0;
        g = G[p] != 0;
        const bool up = y > 0, dn = y < H - 1, lf = x > 0, rt = x < W - 1;
        const int ia = a && up && dn && lf && rt && P[p - W] && P[p + W] && P[p - 1] && P[p + 1];      // survives the 4-connected erosion
        const int ig = g && up && dn && lf && rt && G[p - W] && G[p + W] && G[p - 1] && G[p + 1];
        border[(plane * 2 + 0) * HW + p] = (uint8_t)(g && !ig);
        border[(plane * 2 + 1) * HW + p] = (uint8_t)(a && !ia);
    }
    const int v[3] = {a & g, a, g};
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = __popcll(__ballot(v[k]));
        if (lane == 0) red[k][wave] = c;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (c) atomicAdd(&counts[plane * 3 + threadIdx.x], (unsigned long long)c);
    }
}

// ---- 2. nearest border pixel within the row.  One wave per row, 4 rows per workgroup; row = blockIdx.x * 4 + wave over all
// rows of all border planes.
__global__ __launch_bounds__(256) void surf_row_kernel(const uint8_t* __restrict__ border, int64_t rows, int W, uint16_t* __restrict__ g) {
    __shared__ uint8_t sb[4][SURF_MAX];
    __shared__ uint16_t sd[4][SURF_MAX];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    const bool live = row < rows;
    const uint8_t* Bd = border + (live ? row : 0) * W;
    if (live)
        for (int x = lane; x < W; x += 64) sb[wave][x] = Bd[x];
    __syncthreads();
    if (!live) return;                                     // no workgroup barrier below this line
    const int ch = (W + 63) >> 6;                          // run length per lane, <= 16
    const int x0 = lane * ch, x1 = min(x0 + ch, W);       // x0 may be >= W: an empty run
    const int FAR = 4 * SURF_MAX;
    int last = -FAR, first = FAR;
    for (int x = x0; x < x1; ++x)
        if (sb[wave][x]) {
            last = x;
            if (first == FAR) first = x;
        }
    int pre = last, suf = first;                           // inclusive prefix max of `last`, inclusive suffix min of `first`
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int a = __shfl_up(pre, o), b = __shfl_down(suf, o);
        if (lane >= o) pre = max(pre, a);
        if (lane + o < 64) suf = min(suf, b);
    }
    int left = __shfl_up(pre, 1), right = __shfl_down(suf, 1);
    if (lane == 0) left = -FAR;
    if (lane == 63) right = FAR;
    for (int x = x0; x < x1; ++x) {                        // distance to the nearest border pixel at or left of x
        if (sb[wave][x]) left = x;
        sd[wave][x] = (uint16_t)min(x - left, (int)SURF_NONE);
    }
    for (int x = x1 - 1; x >= x0; --x) {                   // ... and at or right of x
        if (sb[wave][x]) right = x;
        const int d = min((int)sd[wave][x], right - x);
        sd[wave][x] = d >= SURF_MAX ? (uint16_t)SURF_NONE : (uint16_t)d;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the runs of the other lanes of this wave, through LDS
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    uint16_t* Gd = g + row * W;
    for (int x = lane; x < W; x += 64) Gd[x] = sd[wave][x];
}

// ---- 3. column pass.  grid (strips, row blocks, border planes); dynamic LDS: H * SURF_SW ints.
__global__ __launch_bounds__(256) void surf_column_kernel(const uint16_t* __restrict__ g, int H, int W, int* __restrict__ d2) {
    extern __shared__ int g2[];                            // [H][SURF_SW]
    __shared__ int ylo, yhi;
    const int plane = blockIdx.z, xs = blockIdx.x * SURF_SW;
    const int64_t HW = (int64_t)H * W;
    const uint16_t* Gp = g + plane * HW;
    if (threadIdx.x == 0) {
        ylo = H;
        yhi = -1;
    }
    __syncthreads();
    int lo = H, hi = -1;
    for (int e = threadIdx.x; e < H * SURF_SW; e += 256) {
        const int y = e / SURF_SW, x = xs + e % SURF_SW;
        const unsigned v = x < W ? Gp[(int64_t)y * W + x] : SURF_NONE;
        g2[e] = v == SURF_NONE ? SURF_INF : (int)(v * v);
        if (v != SURF_NONE) {                              // SURF_NONE holds for a whole row, so any column of the strip tells
            lo = min(lo, y);
            hi = max(hi, y);
        }
    }
    if (hi >= 0) {
        atomicMin(&ylo, lo);
        atomicMax(&yhi, hi);
    }
    __syncthreads();
    const int cx = threadIdx.x % SURF_SW, x = xs + cx;
    const int y0 = blockIdx.y * SURF_ROWS + (threadIdx.x / SURF_SW) * SURF_RT;
    int best[SURF_RT];
#pragma unroll
    for (int j = 0; j < SURF_RT; ++j) best[j] = SURF_INF;
    const int a = ylo, b = yhi;
    for (int yp = a; yp <= b; ++yp) {
        const int v = g2[yp * SURF_SW + cx];
        const int d = y0 - yp;
#pragma unroll
        for (int j = 0; j < SURF_RT; ++j) best[j] = min(best[j], __mul24(d + j, d + j) + v);
    }
    if (x >= W) return;
    int* D = d2 + plane * HW;
#pragma unroll
    for (int j = 0; j < SURF_RT; ++j)
        if (y0 + j < H) D[(int64_t)(y0 + j) * W + x] = best[j] >= SURF_INF ? -1 : best[j];
}

// ---- 4. gather.  grid (SURF_G, B * 2 * 2); blockIdx.y = (plane * 2 + dir), dir 0 = pred -> gt, 1 = gt -> pred.
// Direction dir walks border slot 1 - dir and reads the distance map to border slot dir.
__global__ __launch_bounds__(256) void surf_gather_kernel(const uint8_t* __restrict__ border, const int* __restrict__ d2, int64_t HW,
                                                          SurfPartial* __restrict__ partial) {
    __shared__ double ss[256];
    __shared__ int sn[256], sm[256];
    const int pd = blockIdx.y, plane = pd >> 1, dir = pd & 1;
    const uint8_t* Bd = border + (int64_t)(plane * 2 + (1 - dir)) * HW;
    const int* D = d2 + (int64_t)(plane * 2 + dir) * HW;
    const int64_t slice = (HW + SURF_G - 1) / SURF_G, p0 = blockIdx.x * slice;
    const int64_t p1 = p0 + slice < HW ? p0 + slice : HW;
    double s = 0.0;
    int n = 0, m = -1;
    for (int64_t p = p0 + threadIdx.x; p < p1; p += 256)
        if (Bd[p]) {
            const int v = D[p];
            ++n;
            m = max(m, v);
            s += sqrt((double)v);                          // v = -1 (other set empty) gives NaN; the combine overrides that case
        }
    ss[threadIdx.x] = s;
    sn[threadIdx.x] = n;
    sm[threadIdx.x] = m;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                    // fixed tree: the same additions in the same order on every run
        if (threadIdx.x < o) {
            ss[threadIdx.x] += ss[threadIdx.x + o];
            sn[threadIdx.x] += sn[threadIdx.x + o];
            sm[threadIdx.x] = max(sm[threadIdx.x], sm[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        SurfPartial r;
        r.s = ss[0];
        r.n = sn[0];
        r.m = sm[0];
        partial[(int64_t)pd * SURF_G + blockIdx.x] = r;
    }
}

// one thread per (image, class): the SURF_G slots of both directions in index order, then the empty-set rule
__global__ __launch_bounds__(64) void surf_combine_kernel(const SurfPartial* __restrict__ partial, int planes, double* __restrict__ table) {
    const int plane = blockIdx.x * 64 + threadIdx.x;
    if (plane >= planes) return;
    double s[2];
    long long n[2], m[2];
    for (int dir = 0; dir < 2; ++dir) {
        const SurfPartial* P = partial + (int64_t)(plane * 2 + dir) * SURF_G;
        s[dir] = 0.0;
        n[dir] = 0;
        m[dir] = -1;
        for (int k = 0; k < SURF_G; ++k) {
            s[dir] += P[k].s;
            n[dir] += P[k].n;
            m[dir] = P[k].m > m[dir] ? P[k].m : m[dir];
        }
    }
    const bool undefined = n[0] == 0 || n[1] == 0;
    for (int dir = 0; dir < 2; ++dir) {
        double* T = table + (int64_t)(plane * 2 + dir) * 3;
        T[0] = (double)n[dir];
        T[1] = undefined ? __longlong_as_double(0x7ff8000000000000ll) : s[dir];
        T[2] = undefined ? -1.0 : (double)m[dir];
    }
}

// ---- 5. profile.  One workgroup per (image, class); everything an integer.
//   Ranks.  Set 0 = pred -> gt, 1 = gt -> pred, 2 = both pooled.  For a set of n values and quantile q: v = (double)(n - 1) * q (one
//   IEEE multiply), lo = floor(v), hi = min(lo + 1, n - 1); rank r = (set * Q + qi) * 2 + (0: lo, 1: hi), 6 * Q ranks in all.
//   Select.  d2 < 2^21 = three 7-bit digits.  Level 1 histograms the top digit per direction (the pooled histogram is the sum of the
//   two); one thread per rank walks the 128 bins to the bin that holds the rank and keeps (digits so far, rank inside the bin).
//   Levels 2 and 3 re-read the border pixels and histogram the next digit per RANK, of the values whose upper digits equal that
//   rank's; after level 3 the digits are the value.  A rank below n always lands in a bin, so every walk ends inside the 128 bins.
//   LDS: max(2, 6 * Q) histograms of 128 ints (3 KiB at Q = 1, 24 KiB at Q = 8).  Integer LDS atomics only; no global atomics and
//   nothing shared between workgroups, so the result cannot depend on the batch or on the run.
#define SURF_PQ 8                // most quantiles, and most tolerances
#define SURF_BINS 128            // radix of the select: 7 bits per level, 3 levels

struct SurfProfileArgs {
    double q[SURF_PQ];
    int tol2[SURF_PQ];
    int Q, T;
};

// f(p, d2[p]) for every set byte p of one border plane.  16 border bytes per load where the plane allows it (base address and
// H * W multiples of 16), bytes otherwise; d2 is read at border pixels only.
template <class F>
__device__ __forceinline__ void surf_walk(const uint8_t* __restrict__ Bd, const int* __restrict__ D, int HW, F f) {
    if ((HW & 15) == 0 && ((uintptr_t)Bd & 15) == 0) {
        const uint4* V = (const uint4*)Bd;
        for (int c = threadIdx.x; c < (HW >> 4); c += 256) {
            const uint4 q = V[c];
            const unsigned w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!w[k]) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((w[k] >> (8 * j)) & 0xffu) {
                        const int p = c * 16 + k * 4 + j;
                        f(p, D[p]);
                    }
            }
        }
    } else {
        for (int p = threadIdx.x; p < HW; p += 256)
            if (Bd[p]) f(p, D[p]);
    }
}

__global__ __launch_bounds__(256) void surf_profile_kernel(const uint8_t* __restrict__ border, const int* __restrict__ d2, int H, int W,
                                                           SurfProfileArgs a, long long* __restrict__ order, long long* __restrict__ within,
                                                           long long* __restrict__ extent) {
    extern __shared__ int hist[];                          // [max(2, R)][SURF_BINS]
    __shared__ int s_n[2], s_within[2][SURF_PQ], s_pmin[2], s_pmax[2];        // s_n, s_within by direction; s_pmin, s_pmax by border slot
    __shared__ int r_prefix[6 * SURF_PQ], r_rem[6 * SURF_PQ];
    __shared__ double s_q[SURF_PQ];                        // a.q behind a run-time index without a private copy of the argument block
    const int plane = blockIdx.x, tid = threadIdx.x;
    const int HW = H * W;                                  // <= 2^20
    const int Q = a.Q, T = a.T, R = 6 * Q;
    const uint8_t* Bp = border + (int64_t)plane * 2 * HW;
    const int* Dp = d2 + (int64_t)plane * 2 * HW;

    for (int e = tid; e < 2 * SURF_BINS; e += 256) hist[e] = 0;
    if (tid < 2) {
        s_n[tid] = 0;
        s_pmin[tid] = HW;
        s_pmax[tid] = -1;
    }
    if (tid < 2 * SURF_PQ) s_within[tid / SURF_PQ][tid % SURF_PQ] = 0;
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < SURF_PQ; ++i) s_q[i] = a.q[i];
    }
    __syncthreads();

    // level 1: direction dir walks border slot 1 - dir and reads the distance map to border slot dir
    for (int dir = 0; dir < 2; ++dir) {
        int n = 0, pmin = HW, pmax = -1, cnt[SURF_PQ];
#pragma unroll
        for (int t = 0; t < SURF_PQ; ++t) cnt[t] = 0;
        surf_walk(Bp + (int64_t)(1 - dir) * HW, Dp + (int64_t)dir * HW, HW, [&](int p, int v) {
            ++n;
            pmin = min(pmin, p);
            pmax = max(pmax, p);
            if (v >= 0) {                                  // v = -1: the other set is empty, the plane undefined; no bin for it
                atomicAdd(&hist[dir * SURF_BINS + ((v >> 14) & (SURF_BINS - 1))], 1);
#pragma unroll
                for (int t = 0; t < SURF_PQ; ++t) cnt[t] += (t < T && v <= a.tol2[t]) ? 1 : 0;
            }
        });
        if (n) {
            atomicAdd(&s_n[dir], n);
            atomicMin(&s_pmin[1 - dir], pmin);
            atomicMax(&s_pmax[1 - dir], pmax);
#pragma unroll
            for (int t = 0; t < SURF_PQ; ++t)
                if (cnt[t]) atomicAdd(&s_within[dir][t], cnt[t]);
        }
    }
    __syncthreads();

    const int n0 = s_n[0], n1 = s_n[1];
    if (tid < 4) {                                         // extent: slot = tid / 2 was walked by direction 1 - slot
        const int slot = tid >> 1, k = tid & 1;
        const int ns = s_n[1 - slot], p = k ? s_pmax[slot] : s_pmin[slot];
        extent[((int64_t)plane * 2 + slot) * 2 + k] = ns ? p / W : -1;
    }
    const bool undefined = n0 == 0 || n1 == 0;             // the same for every thread
    for (int e = tid; e < 2 * T; e += 256) within[(int64_t)plane * 2 * T + e] = undefined ? -1 : s_within[e / T][e % T];
    if (undefined) {
        for (int e = tid; e < R; e += 256) order[(int64_t)plane * R + e] = -1;
        return;
    }
    if (R == 0) return;

    if (tid < R) {
        const int set = tid / (2 * Q), qi = (tid >> 1) % Q;
        const int n = set == 0 ? n0 : set == 1 ? n1 : n0 + n1;
        const double v = (double)(n - 1) * s_q[qi];
        const int lo = (int)floor(v);
        int k = (tid & 1) ? min(lo + 1, n - 1) : lo, b = 0;
        for (; b < SURF_BINS - 1; ++b) {
            const int c = (set != 1 ? hist[b] : 0) + (set != 0 ? hist[SURF_BINS + b] : 0);
            if (k < c) break;
            k -= c;
        }
        r_prefix[tid] = b;
        r_rem[tid] = k;
    }
    __syncthreads();

    for (int shift = 7; shift >= 0; shift -= 7) {          // levels 2 and 3
        for (int e = tid; e < R * SURF_BINS; e += 256) hist[e] = 0;
        __syncthreads();
        for (int dir = 0; dir < 2; ++dir)
            surf_walk(Bp + (int64_t)(1 - dir) * HW, Dp + (int64_t)dir * HW, HW, [&](int p, int v) {
                const int up = v >> (shift + 7), bin = (v >> shift) & (SURF_BINS - 1);
                for (int i = 0; i < 2 * Q; ++i) {          // the ranks of this direction's own set, then those of the pooled set
                    const int r0 = dir * 2 * Q + i, r1 = 4 * Q + i;
                    if (r_prefix[r0] == up) atomicAdd(&hist[r0 * SURF_BINS + bin], 1);
                    if (r_prefix[r1] == up) atomicAdd(&hist[r1 * SURF_BINS + bin], 1);
                }
            });
        __syncthreads();
        if (tid < R) {
            int k = r_rem[tid], b = 0;
            for (; b < SURF_BINS - 1; ++b) {
                const int c = hist[tid * SURF_BINS + b];
                if (k < c) break;
                k -= c;
            }
            r_prefix[tid] = (r_prefix[tid] << 7) | b;
            r_rem[tid] = k;
        }
        __syncthreads();
    }
    if (tid < R) order[(int64_t)plane * R + tid] = r_prefix[tid];
}

// workspace: partial slots | d2 (when the caller keeps none) | g | border, each over B * 2 * 2 planes
static inline size_t surf_align(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t uda_surface_distance_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    const size_t planes = (size_t)4 * B, HW = (size_t)H * W;
    return surf_align(planes * SURF_G * sizeof(SurfPartial)) + surf_align(planes * HW * sizeof(int)) +
           surf_align(planes * HW * sizeof(uint16_t)) + surf_align(planes * HW) + 256;
}

// the argument checks both entry points share; `who` names the entry point in the error text
static int surf_check(const char* who, const void* pred, const void* gt, int B, int H, int W, const void* table, const void* counts,
                      const void* workspace, size_t workspace_bytes) {
    UDA_REQUIRE(pred && gt && table && counts && workspace, "%s: null argument", who);
    UDA_REQUIRE(B >= 1 && B <= 8192, "%s: batch %d outside 1..8192", who, B);
    UDA_REQUIRE(H >= 1 && H <= SURF_MAX && W >= 1 && W <= SURF_MAX, "%s: %d x %d outside 1..%d per side", who, H, W, SURF_MAX);
    UDA_REQUIRE(workspace_bytes >= uda_surface_distance_workspace_bytes(B, H, W), "%s: workspace too small (%zu < %zu B)", who,
                workspace_bytes, uda_surface_distance_workspace_bytes(B, H, W));
    return 0;
}

// passes 1-4 on checked arguments; leaves the border bytes and the d2 maps of all 4 * B planes behind
static int surf_passes(const char* who, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, double* table, int64_t* counts, int32_t* d2,
                       void* workspace, hipStream_t st, const uint8_t** border_out, const int** d2_out) {
    const int planes = 2 * B, bplanes = 4 * B;
    const int64_t HW = (int64_t)H * W;
    char* w = (char*)workspace;
    SurfPartial* partial = (SurfPartial*)w;
    w += surf_align((size_t)bplanes * SURF_G * sizeof(SurfPartial));
    int* dmap = d2 ? d2 : (int*)w;
    w += surf_align((size_t)bplanes * HW * sizeof(int));
    uint16_t* g = (uint16_t*)w;
    w += surf_align((size_t)bplanes * HW * sizeof(uint16_t));
    uint8_t* border = (uint8_t*)w;
    if (hipMemsetAsync(counts, 0, (size_t)planes * 3 * sizeof(int64_t), st) != hipSuccess) return uda_set_error("%s: memset failed", who);
    hipLaunchKernelGGL(surf_border_kernel, dim3(uda_cdiv(HW, 256), planes), dim3(256), 0, st, pred, gt, H, W, border,
                       (unsigned long long*)counts);
    const int64_t rows = (int64_t)bplanes * H;
    hipLaunchKernelGGL(surf_row_kernel, dim3(uda_cdiv(rows, 4)), dim3(256), 0, st, border, rows, W, g);
    hipLaunchKernelGGL(surf_column_kernel, dim3(uda_cdiv(W, SURF_SW), uda_cdiv(H, SURF_ROWS), bplanes), dim3(256),
                       (size_t)H * SURF_SW * sizeof(int), st, g, H, W, dmap);
    hipLaunchKernelGGL(surf_gather_kernel, dim3(SURF_G, bplanes), dim3(256), 0, st, border, dmap, HW, partial);
    hipLaunchKernelGGL(surf_combine_kernel, dim3(uda_cdiv(planes, 64)), dim3(64), 0, st, partial, planes, table);
    *border_out = border;
    *d2_out = dmap;
    return 0;
}

extern "C" int uda_surface_distance(const uint8_t* pred, const uint8_t* gt, int B, int H, int W, double* table, int64_t* counts,
                                    int32_t* d2, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = surf_check("uda_surface_distance", pred, gt, B, H, W, table, counts, workspace, workspace_bytes)) return rc;
    const uint8_t* border;
    const int* dmap;
    if (int rc = surf_passes("uda_surface_distance", pred, gt, B, H, W, table, counts, d2, workspace, (hipStream_t)stream, &border, &dmap)) return rc;
    UDA_LAUNCH_CHECK("uda_surface_distance");
    return 0;
}

extern "C" size_t uda_surface_profile_workspace_bytes(int B, int H, int W) { return uda_surface_distance_workspace_bytes(B, H, W); }

extern "C" int uda_surface_profile(const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const double* quantiles, int Q,
                                   const int32_t* tol2, int T, double* table, int64_t* counts, int64_t* order, int64_t* within,
                                   int64_t* extent, int32_t* d2, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = surf_check("uda_surface_profile", pred, gt, B, H, W, table, counts, workspace, workspace_bytes)) return rc;
    UDA_REQUIRE(extent, "uda_surface_profile: null argument");
    UDA_REQUIRE(Q >= 0 && Q <= SURF_PQ && (Q == 0 || (quantiles && order)), "uda_surface_profile: %d quantiles outside 0..%d, or no array for them", Q, SURF_PQ);
    UDA_REQUIRE(T >= 0 && T <= SURF_PQ && (T == 0 || (tol2 && within)), "uda_surface_profile: %d tolerances outside 0..%d, or no array for them", T, SURF_PQ);
    SurfProfileArgs a = {};
    a.Q = Q;
    a.T = T;
    for (int i = 0; i < Q; ++i) {
        UDA_REQUIRE(quantiles[i] >= 0.0 && quantiles[i] <= 1.0, "uda_surface_profile: quantile %d (%g) outside [0, 1]", i, quantiles[i]);   // false for NaN
        a.q[i] = quantiles[i];
    }
    for (int i = 0; i < T; ++i) {
        UDA_REQUIRE(tol2[i] >= 0, "uda_surface_profile: squared tolerance %d (%d) is negative", i, tol2[i]);
        a.tol2[i] = tol2[i];
    }
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* border;
    const int* dmap;
    if (int rc = surf_passes("uda_surface_profile", pred, gt, B, H, W, table, counts, d2, workspace, st, &border, &dmap)) return rc;
    const int R = 6 * Q;
    hipLaunchKernelGGL(surf_profile_kernel, dim3(2 * B), dim3(256), (size_t)(R > 2 ? R : 2) * SURF_BINS * sizeof(int), st, border, dmap, H, W, a,
                       (long long*)order, (long long*)within, (long long*)extent);
    UDA_LAUNCH_CHECK("uda_surface_profile");
    return 0;
}
