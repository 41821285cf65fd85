// Pillow's 8-bit BILINEAR resample as integer arithmetic over double-precision coefficient tables (Resample.c: precompute_coeffs,
// normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc), shared by geometry.hip (the scale-crop of the input
// pipeline) and wholephoto.hip (the ROI cut):
//     scale = in / out, fs = max(scale, 1), support = fs, center = (xx + 0.5) * scale,
//     xmin = max(0, (int)(center - support + 0.5)), xmax = min(in, (int)(center + support + 0.5)),
//     w[x] = 1 - |(x + xmin - center + 0.5) * (1 / fs)| (0 from magnitude 1 on), summed in tap order, each divided by the sum,
//     k[x] = (int)(0.5 + w[x] * 2^22);   pixel = clip8((2^21 + sum src * k) >> 22).
// An axis whose size does not change is skipped by Pillow; the identity weights {2^22} used for it here give the same byte.
#pragma once
#include "common.h"

// the tables must see the doubles Pillow's C loops see (no fused multiply-add there)
#pragma clang fp contract(off)

#define GEO_TAPS 5            // in / out <= 2.5: at most 5 taps per axis
#define GEO_PREC 22

struct GeoEntry {             // one output position along one axis
    int x0;                   // first source index of the taps; -1: outside the scaled image (fill)
    int n;                    // number of taps
    int k[GEO_TAPS];          // integer weights, 0 past the last tap
    int nn;                   // source index of the NEAREST resize (geometry.hip only)
};

// x0, n and k of output position xx of n_out (0 <= xx < n_out) resampled from n_in; nn is left alone
__device__ __forceinline__ void geo_bilinear_entry(int xx, int n_in, int n_out, GeoEntry& e) {
#pragma unroll
    for (int t = 0; t < GEO_TAPS; ++t) e.k[t] = 0;
    if (n_in == n_out) {
        e.x0 = xx;
        e.n = 1;
        e.k[0] = 1 << GEO_PREC;
        return;
    }
    const double scale = (double)n_in / (double)n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 1.0 * fs, ss = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    int n = xmax - xmin;
    if (n > GEO_TAPS) n = GEO_TAPS;                     // cannot happen for in / out <= 2.5; keeps a bad record in bounds
    if (n < 0) n = 0;
    double w[GEO_TAPS], ww = 0.0;
#pragma unroll
    for (int t = 0; t < GEO_TAPS; ++t) {
        double a = ((double)(t + xmin) - center + 0.5) * ss;
        if (a < 0.0) a = -a;
        w[t] = (t < n && a < 1.0) ? 1.0 - a : 0.0;
        if (t < n) ww += w[t];
    }
#pragma unroll
    for (int t = 0; t < GEO_TAPS; ++t) {
        const double q = ww != 0.0 ? w[t] / ww : w[t];
        e.k[t] = t < n ? (int)(0.5 + q * (double)(1 << GEO_PREC)) : 0;
    }
    e.x0 = xmin;
    e.n = n;
}

__device__ __forceinline__ int geo_clip8(int acc) {
    const int v = acc >> GEO_PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
