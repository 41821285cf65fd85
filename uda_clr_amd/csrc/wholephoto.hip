// Whole-photograph prediction (uda_clr_amd/wholephoto.py): the byte traffic between a fundus photograph of any size
// and the fixed-size ROI the generator takes.  The reference ships ROIs that were cut beforehand and has none of this; every
// definition is this project's (include/uda_clr_hip.h), except the ROI resample, which is Pillow's.
//
//   uda_photo_reduce_u8  the coarse canvas: block means by an integer factor f = ceil(max(H, W) / S), rounded half up in integers.
//                        A workgroup owns 64 canvas columns of one canvas row; it stages the f source rows' segments through LDS in
//                        16-byte words (as many rows per pass as 8 KiB hold; for the very large f of a tiny canvas, fewer columns
//                        per pass) and thread (column, channel) sums its bytes from LDS.
//   uda_roi_cut_u8       crop((x0, y0, x0 + R, y0 + R)).resize((S, S), BILINEAR) of Pillow, byte for byte: the crop reads as 0 outside
//                        the photograph, the coefficient tables are those of geometry.hip (pil_resample.h) for R -> S on both axes.  A
//                        workgroup owns a 32 x 32 output tile: it forms the tile's 2 x 32 table entries, stages the source patch its
//                        taps span (at most 88 x 88 pixels, only the part inside the photograph) in 16-byte words, runs the horizontal
//                        pass from that patch into LDS as uint8 and the vertical pass from there.
//   uda_roi_paste_u8     each photograph's grey mask as one byte stream: a thread forms 16 bytes and stores them as one 16-byte word
//                        (the bytes in front of the first aligned word and behind the last one singly).  A word outside the window
//                        is 255 without further work; inside, each plane's bilinear upsample is decided in integers.
//
// 16-byte loads never leave the pool: a word that is not wholly inside [pool, pool + 3 * pool_pixels) is read byte by byte, only the
// bytes inside.  Integer arithmetic only, apart from the final uint8 -> float of the normalised outputs; no atomics.
#include "pil_resample.h"

// no fused multiply-add: the coefficient tables see Pillow's doubles, the normalised outputs torch's two rounded steps
#pragma clang fp contract(off)

#define WP_MAX_SIDE 8192
#define WP_MAX_B 8192
#define WP_MAX_S 1024
#define WP_MAX_ORIGIN (1 << 20)     // |x0|, |y0| beyond this: the window is wholly outside any photograph anyway

struct WpPhoto {
    const uint8_t* base;            // null: no such photograph
    int H, W;
};

__device__ __forceinline__ WpPhoto wp_photo(const uint8_t* pool, int64_t pool_pixels, const int64_t* offsets, const int* sizes, int n_sources,
                                            int64_t si) {
    WpPhoto p = {nullptr, 0, 0};
    if (si < 0 || si >= n_sources) return p;
    const int H = sizes[si * 2], W = sizes[si * 2 + 1];
    const int64_t off = offsets[si];
    if (H < 1 || W < 1 || H > WP_MAX_SIDE || W > WP_MAX_SIDE || off < 0 || off + (int64_t)H * W > pool_pixels) return p;
    p.base = pool + off * 3;
    p.H = H;
    p.W = W;
    return p;
}

// v * fl(1 / 127.5) - 1, product and difference each rounded to fp32: the bits of torch's `u8.float() / 127.5 - 1.0` on the device,
// which divides by a host scalar as a product with its rounded reciprocal
// (written as two statements under contract(off): the product must not be fused into the subtraction)
__device__ __forceinline__ float wp_norm(int v) {
    const float p = (float)v * (1.0f / 127.5f);
    return p - 1.0f;
}

// the 16 bytes at the 16-byte aligned address a; a byte outside [lo, hi) is not touched and reads as 0
__device__ __forceinline__ uint4 wp_load16(uintptr_t a, uintptr_t lo, uintptr_t hi) {
    if (a >= lo && a + 16 <= hi) return *reinterpret_cast<const uint4*>(a);
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int i = 0; i < 16; ++i)
        if (a + i >= lo && a + i < hi) w[i >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t*>(a + i)) << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// ------------------------------------------------------------------------------------------------ reduce.  grid (S / 64, S, B)
#define RED_CW 64                   // canvas columns per workgroup
#define RED_LDS (8 * 1024)          // staging bytes: the f <= 6 rows of a 512 canvas in one pass, and 8 workgroups per CU

__global__ __launch_bounds__(256) void photo_reduce_kernel(const uint8_t* __restrict__ pool, int64_t pool_pixels, const int64_t* __restrict__ offsets,
                                                           const int* __restrict__ sizes, int n_sources, const int64_t* __restrict__ src_index, int S,
                                                           uint8_t* __restrict__ canvas_u8, float* __restrict__ canvas_f32, int* __restrict__ factor) {
    __shared__ uint4 stage[RED_LDS / 16];
    __shared__ uint32_t outw[RED_CW * 3 / 4];
    const int b = blockIdx.z, r = blockIdx.y, c0 = blockIdx.x * RED_CW, tid = threadIdx.x;
    const int ncols = min(RED_CW, S - c0);                       // a multiple of 16
    const WpPhoto ph = wp_photo(pool, pool_pixels, offsets, sizes, n_sources, src_index[b]);
    int f = 0, h = 0, w = 0;
    if (ph.base) {
        f = max(1, (max(ph.H, ph.W) + S - 1) / S);
        h = (ph.H + f - 1) / f;
        w = (ph.W + f - 1) / f;
    }
    if (blockIdx.x == 0 && r == 0 && tid == 0) factor[b] = f;
    const int col = c0 + tid / 3, ch = tid % 3;                  // threads 0..191: one (column, channel) each
    const uint8_t* sb = reinterpret_cast<const uint8_t*>(stage);
    unsigned acc = 0;                                            // <= 512 * 512 * 255
    if (ph.base && r < h && c0 < w) {                            // the same for every thread of the workgroup, as are all loop bounds below
        const int H = ph.H, W = ph.W;
        const int c_end = min(c0 + ncols, w), y0 = r * f, y1 = min(H, y0 + f);
        const int cols_per = max(1, min(RED_CW, (RED_LDS - 32) / (3 * f)));
        const uintptr_t lo = (uintptr_t)pool, hi = lo + (uintptr_t)pool_pixels * 3;
        for (int cp = c0; cp < c_end; cp += cols_per) {
            const int ce = min(cp + cols_per, c_end);
            const int xs = cp * f, xe = min(W, ce * f), pb = (xe - xs) * 3;
            const int pitch = (pb + 30) & ~15;                   // a row's bytes behind its address's low four bits, in whole words
            const int wpr = pitch >> 4, rows_per = max(1, RED_LDS / pitch);
            for (int ys = y0; ys < y1; ys += rows_per) {
                const int nr = min(rows_per, y1 - ys);
                __syncthreads();
                for (int e = tid; e < nr * wpr; e += 256) {
                    const int j = e / wpr, q = e - j * wpr;
                    const uintptr_t a = (uintptr_t)(ph.base + ((int64_t)(ys + j) * W + xs) * 3);
                    if (q * 16 < (int)(a & 15) + pb) stage[j * wpr + q] = wp_load16((a & ~(uintptr_t)15) + (uintptr_t)q * 16, lo, hi);
                }
                __syncthreads();
                if (tid < RED_CW * 3 && col >= cp && col < ce) {
                    const int xa = col * f - xs, xb = min(W, (col + 1) * f) - xs;
                    for (int j = 0; j < nr; ++j) {
                        const uintptr_t a = (uintptr_t)(ph.base + ((int64_t)(ys + j) * W + xs) * 3);
                        const uint8_t* p = sb + j * pitch + (int)(a & 15) + ch;
                        for (int x = xa; x < xb; ++x) acc += p[x * 3];
                    }
                }
            }
        }
    }
    int v = 0;
    if (tid < RED_CW * 3 && ph.base && r < h && col < w && col < c0 + ncols) {
        const int cnt = (min(ph.H, (r + 1) * f) - r * f) * (min(ph.W, (col + 1) * f) - col * f);
        v = (int)((acc + (unsigned)cnt / 2u) / (unsigned)cnt);
    }
    __syncthreads();
    uint8_t* ob = reinterpret_cast<uint8_t*>(outw);
    if (tid < RED_CW * 3) ob[tid] = (uint8_t)v;
    __syncthreads();
    if (canvas_u8) {                                             // the row segment starts a multiple of 48 bytes behind the base
        uint8_t* o = canvas_u8 + (((int64_t)b * S + r) * S + c0) * 3;
        if (((uintptr_t)canvas_u8 & 3) == 0) {
            if (tid < ncols * 3 / 4) reinterpret_cast<uint32_t*>(o)[tid] = outw[tid];
        } else if (tid < ncols * 3) {
            o[tid] = ob[tid];
        }
    }
    if (canvas_f32 && tid < RED_CW * 3) {
        const int c2 = tid / RED_CW, cc = tid % RED_CW;
        if (cc < ncols) canvas_f32[(((int64_t)b * 3 + c2) * S + r) * S + c0 + cc] = wp_norm(ob[cc * 3 + c2]);
    }
}

// ------------------------------------------------------------------------------------------------ cut.  grid (S / 32, S / 32, B)
#define CUT_T 32                    // tile side
#define CUT_SPAN 88                 // source positions a tile's taps can span per axis: 31 * 2.5 + 1 + taps = 84 at R / S = 2.5, with room
#define CUT_PITCH ((CUT_SPAN * 3 + 30) & ~15)

__device__ __forceinline__ bool wp_box_ok(int x0, int y0, int R, int S) {
    return R >= 8 && 2 * (int64_t)R <= 5 * (int64_t)S && x0 >= -WP_MAX_ORIGIN && x0 <= WP_MAX_ORIGIN && y0 >= -WP_MAX_ORIGIN && y0 <= WP_MAX_ORIGIN;
}

__global__ __launch_bounds__(256) void roi_cut_kernel(const uint8_t* __restrict__ pool, int64_t pool_pixels, const int64_t* __restrict__ offsets,
                                                      const int* __restrict__ sizes, int n_sources, const int64_t* __restrict__ src_index,
                                                      const int* __restrict__ boxes, int S, uint8_t* __restrict__ roi_u8, float* __restrict__ roi_f32) {
    __shared__ uint4 patch[CUT_SPAN * CUT_PITCH / 16];           // the source patch, rows CUT_PITCH bytes apart
    __shared__ uint32_t hpass[CUT_SPAN][CUT_T + 1];              // horizontal pass, one packed RGB pixel per word
    __shared__ GeoEntry tx[CUT_T], ty[CUT_T];
    uint32_t (*res)[CUT_T] = reinterpret_cast<uint32_t (*)[CUT_T]>(patch);       // the tile's pixels, packed: over the patch, dead after the horizontal pass
    const int b = blockIdx.z, oy0 = blockIdx.y * CUT_T, ox0 = blockIdx.x * CUT_T, tid = threadIdx.x;
    const int th = min(CUT_T, S - oy0), tw = min(CUT_T, S - ox0);       // 16 or 32
    const int x0 = boxes[b * 3], y0 = boxes[b * 3 + 1], R = boxes[b * 3 + 2];
    const WpPhoto ph = wp_photo(pool, pool_pixels, offsets, sizes, n_sources, src_index[b]);
    const bool ok = ph.base != nullptr && wp_box_ok(x0, y0, R, S);       // the same for every thread of the workgroup
    if (ok) {
        if (tid < 2 * CUT_T) {
            const int axis = tid / CUT_T, i = tid % CUT_T;
            if (i < (axis ? th : tw)) {
                GeoEntry e;
                geo_bilinear_entry((axis ? oy0 : ox0) + i, R, S, e);
                e.nn = 0;
                (axis ? ty : tx)[i] = e;
            }
        }
        __syncthreads();
        int clo = R, chi = 0, rlo = R, rhi = 0;                  // positions of the zero-padded R x R crop that the taps need
        for (int i = 0; i < tw; ++i) {
            clo = min(clo, tx[i].x0);
            chi = max(chi, tx[i].x0 + tx[i].n);
        }
        for (int i = 0; i < th; ++i) {
            rlo = min(rlo, ty[i].x0);
            rhi = max(rhi, ty[i].x0 + ty[i].n);
        }
        chi = min(min(chi, R), clo + CUT_SPAN);
        rhi = min(min(rhi, R), rlo + CUT_SPAN);
        // the part of it inside the photograph, in photograph coordinates
        const int H = ph.H, W = ph.W;
        const int X0 = max(0, x0 + clo), Y0 = max(0, y0 + rlo);
        const int X1 = max(X0, min(W, x0 + chi)), Y1 = max(Y0, min(H, y0 + rhi));
        const int pb = (X1 - X0) * 3, wpr = CUT_PITCH / 16;
        const uintptr_t lo = (uintptr_t)pool, hi = lo + (uintptr_t)pool_pixels * 3;
        if (pb > 0) {
            for (int e = tid; e < (Y1 - Y0) * wpr; e += 256) {
                const int j = e / wpr, q = e - j * wpr;
                const uintptr_t a = (uintptr_t)(ph.base + ((int64_t)(Y0 + j) * W + X0) * 3);
                if (q * 16 < (int)(a & 15) + pb) patch[j * wpr + q] = wp_load16((a & ~(uintptr_t)15) + (uintptr_t)q * 16, lo, hi);
            }
        }
        __syncthreads();
        const uint8_t* pbytes = reinterpret_cast<const uint8_t*>(patch);
        const int nrows = rhi - rlo;
        for (int e = tid; e < nrows * CUT_T; e += 256) {
            const int r = e / CUT_T, c = e % CUT_T;
            if (c >= tw) continue;
            const GeoEntry ex = tx[c];
            const int Y = y0 + rlo + r;
            int a0 = 1 << (GEO_PREC - 1), a1 = a0, a2 = a0;
            if (Y >= Y0 && Y < Y1) {
                const uintptr_t a = (uintptr_t)(ph.base + ((int64_t)Y * W + X0) * 3);
                const uint8_t* row = pbytes + (Y - Y0) * CUT_PITCH + (int)(a & 15);
#pragma unroll
                for (int t = 0; t < GEO_TAPS; ++t) {
                    const int k = ex.k[t];
                    const int X = x0 + ex.x0 + t;
                    if (k == 0 || X < X0 || X >= X1) continue;   // outside the photograph the crop is 0
                    const uint8_t* p = row + (X - X0) * 3;
                    a0 += (int)p[0] * k; a1 += (int)p[1] * k; a2 += (int)p[2] * k;
                }
            }
            hpass[r][c] = (uint32_t)geo_clip8(a0) | ((uint32_t)geo_clip8(a1) << 8) | ((uint32_t)geo_clip8(a2) << 16);
        }
        __syncthreads();
        for (int e = tid; e < CUT_T * CUT_T; e += 256) {
            const int oy = e / CUT_T, ox = e % CUT_T;
            if (oy >= th || ox >= tw) continue;
            const GeoEntry ey = ty[oy];
            int a0 = 1 << (GEO_PREC - 1), a1 = a0, a2 = a0;
#pragma unroll
            for (int t = 0; t < GEO_TAPS; ++t) {
                const int k = ey.k[t];
                if (k == 0) continue;
                const int r = min(max(ey.x0 + t - rlo, 0), CUT_SPAN - 1);
                const uint32_t v = hpass[r][ox];
                a0 += (int)(v & 255u) * k; a1 += (int)((v >> 8) & 255u) * k; a2 += (int)((v >> 16) & 255u) * k;
            }
            res[oy][ox] = (uint32_t)geo_clip8(a0) | ((uint32_t)geo_clip8(a1) << 8) | ((uint32_t)geo_clip8(a2) << 16);
        }
    } else {
        for (int e = tid; e < CUT_T * CUT_T; e += 256) res[e / CUT_T][e % CUT_T] = 0u;
    }
    __syncthreads();
    if (roi_u8) {                                                // a tile row starts a multiple of 48 bytes behind the base
        uint8_t* o = roi_u8 + (((int64_t)b * S + oy0) * S + ox0) * 3;
        if (((uintptr_t)roi_u8 & 3) == 0) {
            const int dw = tw * 3 / 4;
            for (int e = tid; e < th * dw; e += 256) {
                const int row = e / dw, d = e - row * dw;
                uint32_t word = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int k = d * 4 + i;
                    word |= ((res[row][k / 3] >> (8 * (k % 3))) & 255u) << (8 * i);
                }
                *reinterpret_cast<uint32_t*>(o + (int64_t)row * S * 3 + d * 4) = word;
            }
        } else {
            for (int e = tid; e < th * tw * 3; e += 256) {
                const int row = e / (tw * 3), k = e - row * tw * 3;
                o[(int64_t)row * S * 3 + k] = (uint8_t)((res[row][k / 3] >> (8 * (k % 3))) & 255u);
            }
        }
    }
    if (roi_f32) {
        for (int e = tid; e < 3 * th * tw; e += 256) {
            const int c2 = e / (th * tw), rem = e - c2 * th * tw, row = rem / tw, cc = rem - row * tw;
            roi_f32[(((int64_t)b * 3 + c2) * S + oy0 + row) * S + ox0 + cc] = wp_norm((int)((res[row][cc] >> (8 * c2)) & 255u));
        }
    }
}

// ------------------------------------------------------------------------------------------------ paste.  grid (PASTE_G, B)
#define PASTE_G 256

// per axis: position i of R over S samples, half-pixel centres, edge clamp, in units of 1 / D, D = 2 R
__device__ __forceinline__ void paste_axis(int i, int R, int S, int& i0, int& i1, int& f) {
    const int D = 2 * R;
    const int a = min(max((2 * i + 1) * S - R, 0), (S - 1) * D);
    i0 = a / D;
    f = a - i0 * D;
    i1 = min(i0 + 1, S - 1);
}

// the grey level of a window pixel in the row (i0, i1, fy) at column j: each plane set iff 2 v > D^2, v = sum of m * wy * wx over the
// 2 x 2 neighbours
__device__ __forceinline__ unsigned paste_px(const uint8_t* __restrict__ cup, const uint8_t* __restrict__ disc, int S, int R, int i0, int i1, int fy,
                                             int j) {
    int j0, j1, fx;
    paste_axis(j, R, S, j0, j1, fx);
    const int D = 2 * R, D2 = D * D;                              // <= 5120^2 < 2^25
    const int w00 = (D - fy) * (D - fx), w01 = (D - fy) * fx, w10 = fy * (D - fx), w11 = fy * fx;
    const int p00 = i0 * S + j0, p01 = i0 * S + j1, p10 = i1 * S + j0, p11 = i1 * S + j1;
    const int vc = (cup[p00] ? w00 : 0) + (cup[p01] ? w01 : 0) + (cup[p10] ? w10 : 0) + (cup[p11] ? w11 : 0);
    if (2 * vc > D2) return 0u;
    const int vd = (disc[p00] ? w00 : 0) + (disc[p01] ? w01 : 0) + (disc[p10] ? w10 : 0) + (disc[p11] ? w11 : 0);
    return 2 * vd > D2 ? 128u : 255u;
}

__global__ __launch_bounds__(256) void roi_paste_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ boxes, const int* __restrict__ sizes,
                                                        const int64_t* __restrict__ out_offsets, int S, uint8_t* __restrict__ out, int64_t out_bytes) {
    const int b = blockIdx.y;
    const int H = sizes[b * 2], W = sizes[b * 2 + 1];
    const int64_t off = out_offsets[b];
    if (H < 1 || W < 1 || H > WP_MAX_SIDE || W > WP_MAX_SIDE || off < 0 || off + (int64_t)H * W > out_bytes) return;      // nothing is this mask's
    const int x0 = boxes[b * 3], y0 = boxes[b * 3 + 1], R = boxes[b * 3 + 2];
    const bool ok = wp_box_ok(x0, y0, R, S);
    const uint8_t* cup = masks + (int64_t)b * 2 * S * S;
    const uint8_t* disc = cup + (int64_t)S * S;
    uint8_t* o = out + off;
    const int n = H * W;                                         // <= 2^26
    const int sh = (int)((uintptr_t)o & 15);
    const int nwords = (sh + n + 15) >> 4;
    for (int q = blockIdx.x * 256 + threadIdx.x; q < nwords; q += PASTE_G * 256) {
        const int p0 = q * 16 - sh, pa = max(p0, 0), pe = min(p0 + 16, n);
        int y = pa / W, x = pa - y * W;
        uint32_t word[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
        const bool one_row = x + (pe - pa) <= W;
        const bool outside = !ok || (one_row && (y < y0 || y >= y0 + R || x + (pe - pa) <= x0 || x >= x0 + R));
        if (!outside) {
            int row = -1, i0 = 0, i1 = 0, fy = 0;                // the window row these belong to
            for (int p = pa; p < pe; ++p) {
                unsigned g = 255u;
                if (y >= y0 && y < y0 + R && x >= x0 && x < x0 + R) {
                    if (row != y - y0) {
                        row = y - y0;
                        paste_axis(row, R, S, i0, i1, fy);
                    }
                    g = paste_px(cup, disc, S, R, i0, i1, fy, x - x0);
                }
                const int i = p - p0;
                word[i >> 2] = (word[i >> 2] & ~(255u << (8 * (i & 3)))) | (g << (8 * (i & 3)));
                if (++x == W) {
                    x = 0;
                    ++y;
                }
            }
        }
        if (pe - pa == 16) {
            *reinterpret_cast<uint4*>(o + p0) = make_uint4(word[0], word[1], word[2], word[3]);
        } else {
            for (int p = pa; p < pe; ++p) {
                const int i = p - p0;
                o[p] = (uint8_t)((word[i >> 2] >> (8 * (i & 3))) & 255u);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ entries
static int wp_check_batch(const char* who, int B, int S) {
    UDA_REQUIRE(B >= 1 && B <= WP_MAX_B, "%s: batch %d outside 1..%d", who, B, WP_MAX_B);
    UDA_REQUIRE(S >= 16 && S <= WP_MAX_S && S % 16 == 0, "%s: size %d: a multiple of 16 in 16..%d", who, S, WP_MAX_S);
    return 0;
}

extern "C" int uda_photo_reduce_u8(const uint8_t* pool, int64_t pool_pixels, const int64_t* offsets, const int* sizes, int n_sources,
                                   const int64_t* src_index, int B, int S, uint8_t* canvas_u8, float* canvas_f32, int* factor, void* stream) {
    const char* who = "uda_photo_reduce_u8";
    UDA_REQUIRE(pool && offsets && sizes && src_index && factor, "%s: null argument", who);
    UDA_REQUIRE(canvas_u8 || canvas_f32, "%s: neither canvas_u8 nor canvas_f32 given", who);
    UDA_REQUIRE(pool_pixels > 0 && n_sources > 0, "%s: need pool_pixels, n_sources > 0 (got %lld, %d)", who, (long long)pool_pixels, n_sources);
    if (wp_check_batch(who, B, S)) return -1;
    hipLaunchKernelGGL(photo_reduce_kernel, dim3(uda_cdiv(S, RED_CW), S, B), dim3(256), 0, (hipStream_t)stream, pool, pool_pixels, offsets, sizes,
                       n_sources, src_index, S, canvas_u8, canvas_f32, factor);
    UDA_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int uda_roi_cut_u8(const uint8_t* pool, int64_t pool_pixels, const int64_t* offsets, const int* sizes, int n_sources,
                              const int64_t* src_index, const int* boxes, int B, int S, uint8_t* roi_u8, float* roi_f32, void* stream) {
    const char* who = "uda_roi_cut_u8";
    UDA_REQUIRE(pool && offsets && sizes && src_index && boxes, "%s: null argument", who);
    UDA_REQUIRE(roi_u8 || roi_f32, "%s: neither roi_u8 nor roi_f32 given", who);
    UDA_REQUIRE(pool_pixels > 0 && n_sources > 0, "%s: need pool_pixels, n_sources > 0 (got %lld, %d)", who, (long long)pool_pixels, n_sources);
    if (wp_check_batch(who, B, S)) return -1;
    hipLaunchKernelGGL(roi_cut_kernel, dim3(uda_cdiv(S, CUT_T), uda_cdiv(S, CUT_T), B), dim3(256), 0, (hipStream_t)stream, pool, pool_pixels, offsets,
                       sizes, n_sources, src_index, boxes, S, roi_u8, roi_f32);
    UDA_LAUNCH_CHECK(who);
    return 0;
}

extern "C" int uda_roi_paste_u8(const uint8_t* masks, const int* boxes, const int* sizes, const int64_t* out_offsets, int B, int S, uint8_t* out,
                                int64_t out_bytes, void* stream) {
    const char* who = "uda_roi_paste_u8";
    UDA_REQUIRE(masks && boxes && sizes && out_offsets && out, "%s: null argument", who);
    UDA_REQUIRE(out_bytes > 0, "%s: need out_bytes > 0 (got %lld)", who, (long long)out_bytes);
    if (wp_check_batch(who, B, S)) return -1;
    hipLaunchKernelGGL(roi_paste_kernel, dim3(PASTE_G, B), dim3(256), 0, (hipStream_t)stream, masks, boxes, sizes, out_offsets, S, out, out_bytes);
    UDA_LAUNCH_CHECK(who);
    return 0;
}
