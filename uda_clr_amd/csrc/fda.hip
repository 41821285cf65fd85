// Fourier Domain Adaptation of a uint8 source batch (include/uda_clr_hip.h; Yang & Soatto, CVPR 2020): a source image
// takes the amplitudes of a target image on the (2b+1)^2 lowest frequencies Omega = [-b, b]^2 and keeps its own phase.  Only Omega
// changes, so no FFT is needed:
//
//     out = src + (1 / HW) sum_{(u,v) in Omega} D[u,v] e^{+2 pi i (u y / H + v x / W)},   D = |F_t| F_s / |F_s| - F_s
//
// with F[u,v] = sum_y sum_x s[y,x] e^{-2 pi i (u y / H + v x / W)} per channel.  F_s is Hermitian and |F_t| is even, so D[-u,-v] =
// conj(D[u,v]): the half plane v >= 0 is computed and the sum is Re(G[y,0]) + 2 sum_{v=1..b} Re(G[y,v] e^{2 pi i v x / W}) with
// G[y,v] = sum_u D[u,v] e^{2 pi i u y / H}.  (2b + 2 <= min(H, W) keeps the Nyquist row and column out of Omega.)
//
//   fda_twiddle_kernel  e^{2 pi i k / n} for k in [0, n), n = W and n = H, by sincospi of the fraction reduced to (-1/2, 1/2] turns.
//   fda_rows_kernel     R[n,c,y,v] = sum_x s[n,y,x,c] e^{-2 pi i v x / W}: one wave per image row, the W twiddles in LDS, the phase of
//       (x, v) is the table entry (v x) mod W, stepped by x from one v to the next.  The row is read with 4-byte loads (4 pixels = 3
//       words per lane) where W % 4 == 0.  FDA_VC frequencies at a time: 3 x FDA_VC complex accumulators per lane; a wider band reads
//       the row again (from L1 / L2).  The 64 lanes are summed by halving (fda_wave_sums): 36 values in 38 exchanges, each sum stored by the lane it ends in.
//   fda_cols_kernel     F[n,c,u,v] = sum_y R[n,c,y,v] e^{-2 pi i u y / H}: one workgroup per (n, c, u), y strided over its threads,
//       fda_wave_sums per wave, the four waves through LDS in wave order.
//   fda_delta_kernel    D[b,c,u,v] from F of source b and of target pair[b] (clamped to [0, Bt)), with the zero-magnitude rule.
//   fda_g_kernel        G[b,c,y,v] = sum_u D[b,c,u,v] e^{+2 pi i u y / H}, u ascending, one thread per value.
//   fda_synth_kernel    one workgroup per image row: the row's 3 (b+1) values of G and the W twiddles in LDS, a thread per 4 pixels.
//
// Everything from the bytes to the rounding is float64.  Every sum has one order that depends on the shapes only (no atomics): equal
// inputs give equal bytes.
#include "common.h"

#define FDA_VC 6                 // frequencies v per pass over a row or column: band 5 (beta 0.01 at 512) in one
#define FDA_MAX_SIDE 2048        // W twiddles of 16 bytes in LDS: 32 KiB, beside them 3 (b + 1) values of G
#define FDA_MAX_BATCH 8192

typedef double2 fda_c;           // (re, im)

// Sums over the 64 lanes of a[0 .. N) at once, by halving: at distance M a lane keeps one half of its values and hands the other half
// to its partner, so the six steps move N/2 + N/4 + ... values instead of 6 N.  Afterwards a[0] of the lane that the function gives
// an index e >= 0 is the wave's sum of element e; a lane with -1 holds padding.  The order of every sum is fixed by N alone.
template <int NMAX, int N, int M>
__device__ __forceinline__ int fda_wave_sums(double (&a)[NMAX], int lane) {
    constexpr int HALF = (N + 1) / 2;
    const bool up = (lane & M) != 0;                                // keeps elements [HALF, N)
#pragma unroll
    for (int j = 0; j < HALF; ++j) {
        const double lo = a[j], hi = j + HALF < N ? a[j + HALF] : 0.0;
        const double send = up ? lo : hi, keep = up ? hi : lo;
        a[j] = keep + __shfl_xor(send, M, 64);
    }
    int e = 0;
    if constexpr (M > 1) e = fda_wave_sums<NMAX, HALF, M / 2>(a, lane);
    if (e < 0) return -1;
    e += up ? HALF : 0;
    return e < N ? e : -1;
}

// tw[k] = e^{2 pi i k / n}
__global__ __launch_bounds__(256) void fda_twiddle_kernel(fda_c* __restrict__ twW, int W, fda_c* __restrict__ twH, int H) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < W) {
        const int kk = 2 * k <= W ? k : k - W;
        double s, c;
        sincospi(2.0 * (double)kk / (double)W, &s, &c);
        twW[k] = make_double2(c, s);
    }
    if (k < H) {
        const int kk = 2 * k <= H ? k : k - H;
        double s, c;
        sincospi(2.0 * (double)kk / (double)H, &s, &c);
        twH[k] = make_double2(c, s);
    }
}

// one pixel's three bytes into the accumulators of frequencies v0 .. v0 + nv - 1: acc[(c FDA_VC + j) 2 + (0 re, 1 im)]
__device__ __forceinline__ void fda_row_pixel(const fda_c* __restrict__ tw, int W, int x, int v0, int nv, double s0, double s1, double s2,
                                              double (&acc)[6 * FDA_VC]) {
    int idx = (v0 * x) % W;
#pragma unroll
    for (int j = 0; j < FDA_VC; ++j) {
        if (j >= nv) break;
        const fda_c t = tw[idx];
        acc[2 * j] += s0 * t.x, acc[2 * j + 1] -= s0 * t.y;
        acc[2 * (FDA_VC + j)] += s1 * t.x, acc[2 * (FDA_VC + j) + 1] -= s1 * t.y;
        acc[2 * (2 * FDA_VC + j)] += s2 * t.x, acc[2 * (2 * FDA_VC + j) + 1] -= s2 * t.y;
        idx += x;
        if (idx >= W) idx -= W;
    }
}

// images [0, Na) are a's, [Na, Na + Nb) are b's; R is [Na + Nb][3][H][band + 1].  Dynamic LDS: W twiddles.
template <bool VEC>
__global__ __launch_bounds__(256) void fda_rows_kernel(const uint8_t* __restrict__ a, int Na, const uint8_t* __restrict__ b, int Nb, int H, int W,
                                                       int band, const fda_c* __restrict__ twW, fda_c* __restrict__ R) {
    extern __shared__ __align__(16) unsigned char fda_smem[];
    fda_c* tw = reinterpret_cast<fda_c*>(fda_smem);
    for (int k = threadIdx.x; k < W; k += 256) tw[k] = twW[k];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t rows = (int64_t)(Na + Nb) * H;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < rows; r += (int64_t)gridDim.x * 4) {
        const int n = (int)(r / H), y = (int)(r % H);
        const uint8_t* row = n < Na ? a + ((int64_t)n * H + y) * W * 3 : b + ((int64_t)(n - Na) * H + y) * W * 3;
        for (int v0 = 0; v0 <= band; v0 += FDA_VC) {
            const int nv = min(FDA_VC, band + 1 - v0);
            double acc[6 * FDA_VC];
#pragma unroll
            for (int k = 0; k < 6 * FDA_VC; ++k) acc[k] = 0.0;
            if (VEC) {
                const uint32_t* row4 = reinterpret_cast<const uint32_t*>(row);
                for (int x = 4 * lane; x < W; x += 256) {
                    const uint32_t w0 = row4[3 * (x >> 2)], w1 = row4[3 * (x >> 2) + 1], w2 = row4[3 * (x >> 2) + 2];
                    fda_row_pixel(tw, W, x, v0, nv, (double)(w0 & 255u), (double)((w0 >> 8) & 255u), (double)((w0 >> 16) & 255u), acc);
                    fda_row_pixel(tw, W, x + 1, v0, nv, (double)(w0 >> 24), (double)(w1 & 255u), (double)((w1 >> 8) & 255u), acc);
                    fda_row_pixel(tw, W, x + 2, v0, nv, (double)((w1 >> 16) & 255u), (double)(w1 >> 24), (double)(w2 & 255u), acc);
                    fda_row_pixel(tw, W, x + 3, v0, nv, (double)((w2 >> 8) & 255u), (double)((w2 >> 16) & 255u), (double)(w2 >> 24), acc);
                }
            } else {
                for (int x = lane; x < W; x += 64)
                    fda_row_pixel(tw, W, x, v0, nv, (double)row[3 * x], (double)row[3 * x + 1], (double)row[3 * x + 2], acc);
            }
            const int e = fda_wave_sums<6 * FDA_VC, 6 * FDA_VC, 32>(acc, lane);
            const int c = e / (2 * FDA_VC), j = (e >> 1) % FDA_VC;
            if (e >= 0 && j < nv)
                reinterpret_cast<double*>(R + (((int64_t)n * 3 + c) * H + y) * (band + 1) + v0 + j)[e & 1] = acc[0];
        }
    }
}

// grid: planes * (2 band + 1) workgroups, workgroup = (plane, u).  F is [planes][2 band + 1][band + 1].
__global__ __launch_bounds__(256) void fda_cols_kernel(const fda_c* __restrict__ R, int H, int band, const fda_c* __restrict__ twH,
                                                       fda_c* __restrict__ F) {
    __shared__ double part[4][2 * FDA_VC];                          // per wave: (re, im) of FDA_VC frequencies
    const int nu = 2 * band + 1;
    const int64_t plane = blockIdx.x / nu;
    const int ui = blockIdx.x % nu;
    const int um = ui < band ? ui - band + H : ui - band;          // u mod H
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int v0 = 0; v0 <= band; v0 += FDA_VC) {
        const int nv = min(FDA_VC, band + 1 - v0);
        double acc[2 * FDA_VC];
#pragma unroll
        for (int k = 0; k < 2 * FDA_VC; ++k) acc[k] = 0.0;
        for (int y = threadIdx.x; y < H; y += 256) {
            const fda_c t = twH[(um * y) % H];                      // conjugated below: e^{-2 pi i u y / H}
            const fda_c* p = R + (plane * H + y) * (band + 1) + v0;
#pragma unroll
            for (int j = 0; j < FDA_VC; ++j) {
                if (j >= nv) break;
                const fda_c r = p[j];
                acc[2 * j] += r.x * t.x + r.y * t.y;
                acc[2 * j + 1] += r.y * t.x - r.x * t.y;
            }
        }
        const int e = fda_wave_sums<2 * FDA_VC, 2 * FDA_VC, 32>(acc, lane);
        if (e >= 0) part[wave][e] = acc[0];
        __syncthreads();
        if ((int)threadIdx.x < 2 * nv) {
            const int k = threadIdx.x;
            reinterpret_cast<double*>(F + (plane * nu + ui) * (band + 1) + v0)[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
        }
        __syncthreads();
    }
}

// F: the spectra of the B sources, then of the Bt targets; D [B][3][2 band + 1][band + 1]
__global__ __launch_bounds__(256) void fda_delta_kernel(const fda_c* __restrict__ F, int B, int Bt, const int* __restrict__ pair, int per_image,
                                                        double tiny, fda_c* __restrict__ D) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * per_image) return;
    const int bb = (int)(i / per_image), rest = (int)(i % per_image);
    const int p = min(max(pair[bb], 0), Bt - 1);
    const fda_c fs = F[i], ft = F[((int64_t)B + p) * per_image + rest];
    const double ms = sqrt(fs.x * fs.x + fs.y * fs.y), mt = sqrt(ft.x * ft.x + ft.y * ft.y);
    double px = 1.0, py = 0.0;
    if (ms > tiny) px = fs.x / ms, py = fs.y / ms;
    D[i] = make_double2(mt * px - fs.x, mt * py - fs.y);
}

// G [planes][H][band + 1], planes = 3 B
__global__ __launch_bounds__(256) void fda_g_kernel(const fda_c* __restrict__ D, int64_t total, int H, int band, const fda_c* __restrict__ twH,
                                                    fda_c* __restrict__ G) {
    const int nv = band + 1;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int v = (int)(i % nv), y = (int)((i / nv) % H);
        const int64_t plane = i / ((int64_t)nv * H);
        const fda_c* d = D + plane * (2 * band + 1) * nv + v;
        int idx = (int)(((int64_t)(H - band) * y) % H);             // u = -band
        double re = 0.0, im = 0.0;
        for (int ui = 0; ui <= 2 * band; ++ui) {
            const fda_c t = twH[idx], q = d[(int64_t)ui * nv];
            re += q.x * t.x - q.y * t.y;
            im += q.x * t.y + q.y * t.x;
            idx += y;
            if (idx >= H) idx -= H;
        }
        G[i] = make_double2(re, im);
    }
}

// the three channels of pixel x: s + inv * (Re G[y,0] + 2 sum_{v >= 1} Re(G[y,v] tw[(v x) mod W])), rounded half to even, clamped
__device__ __forceinline__ void fda_synth_pixel(const fda_c* __restrict__ tw, const fda_c* __restrict__ g, int W, int band, int x, double inv,
                                                uint32_t (&s)[3]) {
    const int nv = band + 1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    int idx = 0;
    for (int v = 1; v <= band; ++v) {
        idx += x;
        if (idx >= W) idx -= W;
        const fda_c t = tw[idx], g0 = g[v], g1 = g[nv + v], g2 = g[2 * nv + v];
        a0 += g0.x * t.x - g0.y * t.y;
        a1 += g1.x * t.x - g1.y * t.y;
        a2 += g2.x * t.x - g2.y * t.y;
    }
    const double r0 = rint((double)s[0] + inv * (g[0].x + 2.0 * a0));
    const double r1 = rint((double)s[1] + inv * (g[nv].x + 2.0 * a1));
    const double r2 = rint((double)s[2] + inv * (g[2 * nv].x + 2.0 * a2));
    s[0] = (uint32_t)fmin(fmax(r0, 0.0), 255.0);
    s[1] = (uint32_t)fmin(fmax(r1, 0.0), 255.0);
    s[2] = (uint32_t)fmin(fmax(r2, 0.0), 255.0);
}

// Dynamic LDS: W twiddles, then the row's 3 (band + 1) values of G.
template <bool VEC>
__global__ __launch_bounds__(128) void fda_synth_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ apply, int B, int H, int W, int band,
                                                        const fda_c* __restrict__ twW, const fda_c* __restrict__ G, uint8_t* __restrict__ out) {
    extern __shared__ __align__(16) unsigned char fda_smem[];
    fda_c* tw = reinterpret_cast<fda_c*>(fda_smem);
    fda_c* g = tw + W;
    const int nv = band + 1;
    for (int k = threadIdx.x; k < W; k += 128) tw[k] = twW[k];
    const double inv = 1.0 / ((double)H * (double)W);
    const int64_t rows = (int64_t)B * H;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const int bb = (int)(r / H), y = (int)(r % H);
        const uint8_t* in = src + r * W * 3;
        uint8_t* o = out + r * W * 3;
        if (apply && !apply[bb]) {                                   // the same for the whole workgroup
            if (VEC)
                for (int k = threadIdx.x; k < 3 * (W >> 2); k += 128) reinterpret_cast<uint32_t*>(o)[k] = reinterpret_cast<const uint32_t*>(in)[k];
            else
                for (int k = threadIdx.x; k < 3 * W; k += 128) o[k] = in[k];
            continue;
        }
        __syncthreads();                                            // the table is complete; the previous row's readers of g are done
        for (int k = threadIdx.x; k < 3 * nv; k += 128) g[k] = G[(((int64_t)bb * 3 + k / nv) * H + y) * nv + k % nv];
        __syncthreads();
        if (VEC) {
            for (int x = 4 * threadIdx.x; x < W; x += 512) {
                const uint32_t* p = reinterpret_cast<const uint32_t*>(in) + 3 * (x >> 2);
                const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
                uint32_t s0[3] = {w0 & 255u, (w0 >> 8) & 255u, (w0 >> 16) & 255u};
                uint32_t s1[3] = {w0 >> 24, w1 & 255u, (w1 >> 8) & 255u};
                uint32_t s2[3] = {(w1 >> 16) & 255u, w1 >> 24, w2 & 255u};
                uint32_t s3[3] = {(w2 >> 8) & 255u, (w2 >> 16) & 255u, w2 >> 24};
                fda_synth_pixel(tw, g, W, band, x, inv, s0);
                fda_synth_pixel(tw, g, W, band, x + 1, inv, s1);
                fda_synth_pixel(tw, g, W, band, x + 2, inv, s2);
                fda_synth_pixel(tw, g, W, band, x + 3, inv, s3);
                uint32_t* q = reinterpret_cast<uint32_t*>(o) + 3 * (x >> 2);
                q[0] = s0[0] | (s0[1] << 8) | (s0[2] << 16) | (s1[0] << 24);
                q[1] = s1[1] | (s1[2] << 8) | (s2[0] << 16) | (s2[1] << 24);
                q[2] = s2[2] | (s3[0] << 8) | (s3[1] << 16) | (s3[2] << 24);
            }
        } else {
            for (int x = threadIdx.x; x < W; x += 128) {
                uint32_t s[3] = {in[3 * x], in[3 * x + 1], in[3 * x + 2]};
                fda_synth_pixel(tw, g, W, band, x, inv, s);
                o[3 * x] = (uint8_t)s[0], o[3 * x + 1] = (uint8_t)s[1], o[3 * x + 2] = (uint8_t)s[2];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
static int fda_check(const char* who, int N, int Nt, int H, int W, int band) {
    UDA_REQUIRE(N >= 1 && N <= FDA_MAX_BATCH && Nt >= 0 && Nt <= FDA_MAX_BATCH, "%s: batch %d (and %d) outside 1..%d", who, N, Nt, FDA_MAX_BATCH);
    UDA_REQUIRE(band >= 0 && band <= UDA_FDA_MAX_BAND, "%s: band %d outside 0..%d", who, band, UDA_FDA_MAX_BAND);
    UDA_REQUIRE(H >= 2 && W >= 2 && H <= FDA_MAX_SIDE && W <= FDA_MAX_SIDE, "%s: size %d x %d, each side must be in 2..%d", who, H, W, FDA_MAX_SIDE);
    UDA_REQUIRE(2 * band + 2 <= (H < W ? H : W), "%s: band %d needs 2 band + 2 <= min(H, W), the size is %d x %d", who, band, H, W);
    return 0;
}

// the workspace's parts, each a multiple of 16 bytes: twiddles of W and of H, R, F (sources, then targets), D, G
struct FdaWs {
    size_t twW, twH, R, F, D, G, end;
};
static FdaWs fda_layout(int B, int Bt, int H, int W, int band) {
    const size_t c = sizeof(fda_c), nv = (size_t)band + 1, nu = 2 * (size_t)band + 1, n = (size_t)B + (size_t)Bt;
    FdaWs l;
    l.twW = 0;
    l.twH = l.twW + c * (size_t)W;
    l.R = l.twH + c * (size_t)H;
    l.F = l.R + c * n * 3 * (size_t)H * nv;
    l.D = l.F + (Bt ? c * n * 3 * nu * nv : 0);                     // uda_fda_spectrum writes F to its output
    l.G = l.D + (Bt ? c * (size_t)B * 3 * nu * nv : 0);
    l.end = l.G + (Bt ? c * (size_t)B * 3 * (size_t)H * nv : 0);
    return l;
}

extern "C" size_t uda_fda_workspace_bytes(int B, int Bt, int H, int W, int band) {
    if (B < 1 || B > FDA_MAX_BATCH || Bt < 0 || Bt > FDA_MAX_BATCH || H < 2 || W < 2 || H > FDA_MAX_SIDE || W > FDA_MAX_SIDE || band < 0 ||
        band > UDA_FDA_MAX_BAND)
        return 0;
    return fda_layout(B, Bt, H, W, band).end;
}

// twiddles, row pass and column pass of Na + Nb images into F
static int fda_spectra(const char* who, const uint8_t* a, int Na, const uint8_t* b, int Nb, int H, int W, int band, char* ws, const FdaWs& l, fda_c* F,
                       hipStream_t st) {
    fda_c* twW = reinterpret_cast<fda_c*>(ws + l.twW);
    fda_c* twH = reinterpret_cast<fda_c*>(ws + l.twH);
    fda_c* R = reinterpret_cast<fda_c*>(ws + l.R);
    hipLaunchKernelGGL(fda_twiddle_kernel, dim3(uda_cdiv(H > W ? H : W, 256)), dim3(256), 0, st, twW, W, twH, H);
    UDA_LAUNCH_CHECK(who);
    const int64_t rows = (int64_t)(Na + Nb) * H;
    const int grid = (int)(uda_cdiv(rows, 4) < 2048 ? uda_cdiv(rows, 4) : 2048);
    const size_t lds = sizeof(fda_c) * (size_t)W;
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(a) & 3u) == 0 && (reinterpret_cast<uintptr_t>(b) & 3u) == 0;
    if (vec)
        hipLaunchKernelGGL(fda_rows_kernel<true>, dim3(grid), dim3(256), lds, st, a, Na, b, Nb, H, W, band, twW, R);
    else
        hipLaunchKernelGGL(fda_rows_kernel<false>, dim3(grid), dim3(256), lds, st, a, Na, b, Nb, H, W, band, twW, R);
    UDA_LAUNCH_CHECK(who);
    hipLaunchKernelGGL(fda_cols_kernel, dim3((unsigned)((Na + Nb) * 3 * (2 * band + 1))), dim3(256), 0, st, R, H, band, twH, F);
    UDA_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int uda_fda_spectrum(const uint8_t* image_hwc, int N, int H, int W, int band, double* spectrum, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const char* who = "uda_fda_spectrum";
    UDA_REQUIRE(image_hwc && spectrum && workspace, "%s: null argument", who);
    if (int rc = fda_check(who, N, 0, H, W, band)) return rc;
    UDA_REQUIRE(uda_aligned16(spectrum) && uda_aligned16(workspace), "%s: spectrum and workspace must be 16-byte aligned", who);
    const FdaWs l = fda_layout(N, 0, H, W, band);
    UDA_REQUIRE(workspace_bytes >= l.end, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, l.end);
    return fda_spectra(who, image_hwc, N, nullptr, 0, H, W, band, static_cast<char*>(workspace), l, reinterpret_cast<fda_c*>(spectrum),
                       (hipStream_t)stream);
}

extern "C" int uda_fda_transfer(const uint8_t* src_hwc, int B, int H, int W, const uint8_t* tgt_hwc, int Bt, int Ht, int Wt, const int* pair,
                                const uint8_t* apply, int band, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream) {
    const char* who = "uda_fda_transfer";
    UDA_REQUIRE(src_hwc && tgt_hwc && pair && out && workspace, "%s: null argument", who);
    UDA_REQUIRE(Bt >= 1, "%s: %d target images", who, Bt);
    if (int rc = fda_check(who, B, Bt, H, W, band)) return rc;
    UDA_REQUIRE(H == Ht && W == Wt, "%s: source %d x %d and target %d x %d differ in size", who, H, W, Ht, Wt);
    UDA_REQUIRE(uda_aligned16(workspace), "%s: workspace must be 16-byte aligned", who);
    const FdaWs l = fda_layout(B, Bt, H, W, band);
    UDA_REQUIRE(workspace_bytes >= l.end, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, l.end);
    hipStream_t st = (hipStream_t)stream;
    char* ws = static_cast<char*>(workspace);
    fda_c* F = reinterpret_cast<fda_c*>(ws + l.F);
    fda_c* D = reinterpret_cast<fda_c*>(ws + l.D);
    fda_c* G = reinterpret_cast<fda_c*>(ws + l.G);
    if (int rc = fda_spectra(who, src_hwc, B, tgt_hwc, Bt, H, W, band, ws, l, F, st)) return rc;
    const int nv = band + 1, per_image = 3 * (2 * band + 1) * nv;
    hipLaunchKernelGGL(fda_delta_kernel, dim3(uda_cdiv((int64_t)B * per_image, 256)), dim3(256), 0, st, F, B, Bt, pair, per_image,
                       1e-6 * (double)H * (double)W, D);
    UDA_LAUNCH_CHECK(who);
    const int64_t total = (int64_t)B * 3 * H * nv;
    hipLaunchKernelGGL(fda_g_kernel, dim3((unsigned)(uda_cdiv(total, 256) < 8192 ? uda_cdiv(total, 256) : 8192)), dim3(256), 0, st, D, total, H, band,
                       reinterpret_cast<const fda_c*>(ws + l.twH), G);
    UDA_LAUNCH_CHECK(who);
    const int64_t rows = (int64_t)B * H;
    const int grid = (int)(rows < 8192 ? rows : 8192);
    const size_t lds = sizeof(fda_c) * ((size_t)W + 3 * (size_t)nv);
    const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(src_hwc) & 3u) == 0 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0;
    const fda_c* twW = reinterpret_cast<const fda_c*>(ws + l.twW);
    if (vec)
        hipLaunchKernelGGL(fda_synth_kernel<true>, dim3(grid), dim3(128), lds, st, src_hwc, apply, B, H, W, band, twW, G, out);
    else
        hipLaunchKernelGGL(fda_synth_kernel<false>, dim3(grid), dim3(128), lds, st, src_hwc, apply, B, H, W, band, twW, G, out);
    UDA_LAUNCH_CHECK(who);
    return 0;
}
