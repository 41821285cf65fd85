// Device-side head of the input pipeline (UDA_CLR_DEVICE_INPUT=3): the PIL geometry the reference's dataloader workers do per
// sample, dataloaders/custom_transforms.py:152-182 (RandomCrop), :208-223 (RandomFlip), :315-355 (RandomRotate,
// RandomScaleCrop), done per BATCH from a device-resident copy of the decoded dataset and the workers' recorded draws.
//
//   uda_geometry_u8   per output pixel the chain of index maps runs backwards: undo flip top-bottom, undo flip left-right, undo
//                     the quarter turns (PIL's rotate(90) on a square is np.rot90(a, 1)), add the crop origin and subtract the
//                     pad; outside the scaled image the fill (0 image / 255 mask), inside it the resized pixel.
//
// Only the BILINEAR resize is arithmetic, and Pillow's 8-bit resample is integer arithmetic over double-precision coefficient
// tables (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc):
//     scale = in / out, fs = max(scale, 1), support = fs, center = (xx + 0.5) * scale,
//     xmin = max(0, (int)(center - support + 0.5)), xmax = min(in, (int)(center + support + 0.5)),
//     w[x] = 1 - |(x + xmin - center + 0.5) * (1 / fs)| (0 from magnitude 1 on), summed in tap order, each divided by the sum,
//     k[x] = (int)(0.5 + w[x] * 2^22);   pixel = clip8((2^21 + sum src * k) >> 22),
// horizontal pass first, vertical pass over its uint8 result; an axis whose size does not change is skipped (the identity
// weights {2^22} used for it here give the same byte).  The NEAREST mask resize (Geometry.c: ImagingScaleAffine) indexes with
// (int)xo where xo starts at in / out / 2 and is ACCUMULATED in double per output.  geometry_tables_kernel builds both per
// sample and axis for the S positions of the crop window; geometry_kernel does integer work only.
//
// A workgroup owns a 32x32 output tile = a 32x32 rectangle of the crop (the maps above are permutations of the square).  For a
// scaled sample it runs the horizontal pass for the source rows its vertical taps need (<= ~70 rows at scale 0.5; the tile's 2 x 32 table entries are staged in LDS too) into LDS as
// uint8 and the vertical pass from LDS; an unscaled sample is a plain gather.  Byte-load bound: at most the source window (4x
// the crop at scale 0.5) plus 4 B per output pixel.
#include "pil_resample.h"        // GeoEntry, geo_bilinear_entry, geo_clip8: the coefficient code shared with wholephoto.hip

#define GEO_R 10              // record length, dataloaders.custom_transforms.GEOM_*
#define GEO_T 32              // tile side
#define GEO_ROWS 88           // source rows a tile's vertical taps can span: 31 * 2.5 + 1 + taps = 84 at in / out = 2.5, with room

// grid (B, 2): axis 0 = columns (x), axis 1 = rows (y)
__global__ __launch_bounds__(256) void geometry_tables_kernel(const int* __restrict__ sizes, int n_sources,
                                                              const int64_t* __restrict__ src_index, const int* __restrict__ records,
                                                              int S, GeoEntry* __restrict__ tables) {
    const int b = blockIdx.x, axis = blockIdx.y;
    const int* rec = records + (int64_t)b * GEO_R;
    const int64_t si = src_index[b];
    if (si < 0 || si >= n_sources || !rec[0]) return;          // unscaled samples gather without tables
    const int n_in = sizes[si * 2 + (axis == 0 ? 1 : 0)];       // sizes hold (H0, W0)
    const int n_out = rec[axis == 0 ? 1 : 2];
    const int first = rec[axis == 0 ? 4 : 5] - rec[3];          // crop origin minus pad: window position 0 in the scaled image
    GeoEntry* T = tables + ((int64_t)b * 2 + axis) * S;
    if (n_out <= 0) {
        for (int c = threadIdx.x; c < S; c += 256) { T[c].x0 = -1; T[c].n = 0; T[c].nn = 0; }
        return;
    }
    for (int c = threadIdx.x; c < S; c += 256) {
        GeoEntry e;
        const int xx = first + c;
        if (xx < 0 || xx >= n_out) {
#pragma unroll
            for (int t = 0; t < GEO_TAPS; ++t) e.k[t] = 0;
            e.x0 = -1;
            e.n = 0;
        } else {
            geo_bilinear_entry(xx, n_in, n_out, e);
        }
        T[c].x0 = e.x0;
        T[c].n = e.n;
#pragma unroll
        for (int t = 0; t < GEO_TAPS; ++t) T[c].k[t] = e.k[t];
    }
    // NEAREST: the accumulation is sequential in double; one thread walks the outputs up to the window's end
    if (threadIdx.x == 0) {
        const double a = (double)n_in / (double)n_out;
        double xo = a * 0.5;
        const int last = min(first + S, n_out);
        for (int xx = 0; xx < last; ++xx) {
            if (xx >= first) {
                int i = (int)xo;
                T[xx - first].nn = i < n_in ? i : n_in - 1;
            }
            xo += a;
        }
        for (int c = 0; c < S; ++c)
            if (first + c < 0 || first + c >= n_out) T[c].nn = 0;
    }
}

// output (oy, ox) -> crop (cy, cx): undo flip top-bottom, flip left-right, then the counter-clockwise quarter turns
__device__ __forceinline__ void geo_crop_of(int oy, int ox, int S, int turns, int flr, int ftb, int& cy, int& cx) {
    if (ftb) oy = S - 1 - oy;
    if (flr) ox = S - 1 - ox;
    switch (turns & 3) {
        case 1: cy = ox; cx = S - 1 - oy; break;               // rot90(a, 1)[i][j] = a[j][S-1-i]
        case 2: cy = S - 1 - oy; cx = S - 1 - ox; break;
        case 3: cy = S - 1 - ox; cx = oy; break;               // rot90(a, 3)[i][j] = a[S-1-j][i]
        default: cy = oy; cx = ox; break;
    }
}

__global__ __launch_bounds__(256) void geometry_kernel(const uint8_t* __restrict__ image_pool, const uint8_t* __restrict__ label_pool,
                                                       const int64_t* __restrict__ offsets, const int* __restrict__ sizes, int n_sources,
                                                       const int64_t* __restrict__ src_index, const int* __restrict__ records, int S,
                                                       const GeoEntry* __restrict__ tables, uint8_t* __restrict__ image_out,
                                                       uint8_t* __restrict__ label_out) {
    __shared__ uint32_t hpass[GEO_ROWS][GEO_T + 1];             // horizontal pass, one packed RGB pixel per word (+1: a quarter turn reads down a column)
    __shared__ GeoEntry tx[GEO_T], ty[GEO_T];                   // the tile's table entries, read from global memory once
    const int b = blockIdx.z, oy0 = blockIdx.y * GEO_T, ox0 = blockIdx.x * GEO_T;
    const int oy1 = min(oy0 + GEO_T, S) - 1, ox1 = min(ox0 + GEO_T, S) - 1;
    const int* rec = records + (int64_t)b * GEO_R;
    const int scaled = rec[0], pad = rec[3], x1 = rec[4], y1 = rec[5], turns = rec[6], flr = rec[7], ftb = rec[8];
    const int64_t si = src_index[b];
    const bool have = si >= 0 && si < n_sources;
    const int H0 = have ? sizes[si * 2] : 0, W0 = have ? sizes[si * 2 + 1] : 0;
    const uint8_t* I = image_pool + (have ? offsets[si] * 3 : 0);
    const uint8_t* L = label_pool + (have ? offsets[si] : 0);
    uint8_t* IO = image_out + (int64_t)b * S * S * 3;
    uint8_t* LO = label_out + (int64_t)b * S * S;
    const int tid = threadIdx.x;

    if (!have || !scaled) {                                     // gather only
        for (int e = tid; e < GEO_T * GEO_T; e += 256) {
            const int oy = oy0 + e / GEO_T, ox = ox0 + e % GEO_T;
            if (oy > oy1 || ox > ox1) continue;
            int cy, cx;
            geo_crop_of(oy, ox, S, turns, flr, ftb, cy, cx);
            const int sy = cy + y1 - pad, sx = cx + x1 - pad;
            const int64_t o = (int64_t)oy * S + ox;
            if (sy >= 0 && sy < H0 && sx >= 0 && sx < W0) {
                const uint8_t* p = I + ((int64_t)sy * W0 + sx) * 3;
                IO[o * 3] = p[0]; IO[o * 3 + 1] = p[1]; IO[o * 3 + 2] = p[2];
                LO[o] = L[(int64_t)sy * W0 + sx];
            } else {
                IO[o * 3] = 0; IO[o * 3 + 1] = 0; IO[o * 3 + 2] = 0;
                LO[o] = 255;
            }
        }
        return;
    }

    // the tile's rectangle of the crop
    int ay, ax, by, bx;
    geo_crop_of(oy0, ox0, S, turns, flr, ftb, ay, ax);
    geo_crop_of(oy1, ox1, S, turns, flr, ftb, by, bx);
    const int cy0 = min(ay, by), cy1 = max(ay, by), cx0 = min(ax, bx), cx1 = max(ax, bx);     // each spans at most GEO_T
    const int tw = cx1 - cx0 + 1, th = cy1 - cy0 + 1;
    if (tid < 2 * GEO_T) {
        const int axis = tid / GEO_T, i = tid % GEO_T;
        if (i < (axis == 0 ? tw : th)) {
            const GeoEntry* T = tables + ((int64_t)b * 2 + axis) * S + (axis == 0 ? cx0 : cy0);
            (axis == 0 ? tx : ty)[i] = T[i];
        }
    }
    __syncthreads();
    // source rows the vertical taps of rows cy0..cy1 need (bounds grow with the row)
    int rlo = H0, rhi = 0;
    for (int i = 0; i < th; ++i) {
        const int y0 = ty[i].x0;
        if (y0 < 0) continue;
        rlo = min(rlo, y0);
        rhi = max(rhi, y0 + ty[i].n);
    }
    rhi = min(min(rhi, H0), rlo + GEO_ROWS);
    const int nrows = rhi - rlo;                                // <= 0: the tile lies in the pad
    for (int e = tid; e < nrows * GEO_T; e += 256) {
        const int r = e / GEO_T, c = e % GEO_T;
        if (c >= tw) continue;
        const GeoEntry ex = tx[c];
        if (ex.x0 < 0) continue;                                // never read
        const uint8_t* row = I + (int64_t)(rlo + r) * W0 * 3;
        int a0 = 1 << (GEO_PREC - 1), a1 = a0, a2 = a0;
#pragma unroll
        for (int t = 0; t < GEO_TAPS; ++t) {
            const int k = ex.k[t];
            if (k == 0) continue;
            const uint8_t* p = row + (int64_t)min(ex.x0 + t, W0 - 1) * 3;
            a0 += (int)p[0] * k; a1 += (int)p[1] * k; a2 += (int)p[2] * k;
        }
        hpass[r][c] = (uint32_t)geo_clip8(a0) | ((uint32_t)geo_clip8(a1) << 8) | ((uint32_t)geo_clip8(a2) << 16);
    }
    __syncthreads();
    for (int e = tid; e < GEO_T * GEO_T; e += 256) {
        const int oy = oy0 + e / GEO_T, ox = ox0 + e % GEO_T;
        if (oy > oy1 || ox > ox1) continue;
        int cy, cx;
        geo_crop_of(oy, ox, S, turns, flr, ftb, cy, cx);
        const GeoEntry ey = ty[cy - cy0];
        const int xs = tx[cx - cx0].x0, xn = tx[cx - cx0].nn;
        const int64_t o = (int64_t)oy * S + ox;
        if (ey.x0 < 0 || xs < 0) {
            IO[o * 3] = 0; IO[o * 3 + 1] = 0; IO[o * 3 + 2] = 0;
            LO[o] = 255;
            continue;
        }
        int a0 = 1 << (GEO_PREC - 1), a1 = a0, a2 = a0;
#pragma unroll
        for (int t = 0; t < GEO_TAPS; ++t) {
            const int k = ey.k[t];
            if (k == 0) continue;
            const int r = min(max(ey.x0 + t - rlo, 0), GEO_ROWS - 1);
            const uint32_t v = hpass[r][cx - cx0];
            a0 += (int)(v & 255u) * k; a1 += (int)((v >> 8) & 255u) * k; a2 += (int)((v >> 16) & 255u) * k;
        }
        IO[o * 3] = (uint8_t)geo_clip8(a0); IO[o * 3 + 1] = (uint8_t)geo_clip8(a1); IO[o * 3 + 2] = (uint8_t)geo_clip8(a2);
        LO[o] = L[(int64_t)ey.nn * W0 + xn];
    }
}

extern "C" size_t uda_geometry_u8_workspace_bytes(int B, int S) { return (size_t)B * 2 * S * sizeof(GeoEntry) + 32; }

extern "C" int uda_geometry_u8(const uint8_t* image_pool, const uint8_t* label_pool, const int64_t* offsets, const int* sizes,
                               int n_sources, const int64_t* src_index, const int* records, int B, int S, uint8_t* image_out,
                               uint8_t* label_out, void* workspace, size_t workspace_bytes, void* stream) {
    UDA_REQUIRE(image_pool && label_pool && offsets && sizes && src_index && records && image_out && label_out && workspace,
                "uda_geometry_u8: null argument");
    UDA_REQUIRE(B > 0 && S > 0 && n_sources > 0, "uda_geometry_u8: need B, S, n_sources > 0 (got B=%d, S=%d, n_sources=%d)", B, S, n_sources);
    UDA_REQUIRE(B <= 65535, "uda_geometry_u8: B = %d exceeds the grid's 65535 samples", B);
    UDA_REQUIRE(workspace_bytes >= uda_geometry_u8_workspace_bytes(B, S), "uda_geometry_u8: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    GeoEntry* tables = (GeoEntry*)(((uintptr_t)workspace + 31) & ~(uintptr_t)31);
    hipLaunchKernelGGL(geometry_tables_kernel, dim3(B, 2), dim3(256), 0, st, sizes, n_sources, src_index, records, S, tables);
    UDA_LAUNCH_CHECK("geometry_tables");
    hipLaunchKernelGGL(geometry_kernel, dim3(uda_cdiv(S, GEO_T), uda_cdiv(S, GEO_T), B), dim3(256), 0, st, image_pool, label_pool,
                       offsets, sizes, n_sources, src_index, records, S, tables, image_out, label_out);
    UDA_LAUNCH_CHECK("geometry");
    return 0;
}
