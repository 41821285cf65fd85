// The per-element statistics of uda_mc_uncertainty, shared by uncertainty.hip (T passes on one grid) and tta.hip (V views mapped
// back to the image's frame): both files compile this very code, so that equal inputs give equal bits.
#pragma once
#include "common.h"

#define UNC_TMAX 32

struct UncOut {
    float* mean;
    float* std_half;
    float* entropy;
    float* mi;
    uint8_t* u8;
    float u8_scale;
    int full;                    // entropy or mi wanted
};

__device__ __forceinline__ float unc_plogp(float v) { return v > 0.f ? __fmul_rn(-v, logf(v)) : 0.f; }        // 0 log 0 = 0

// c[T]: the logits of one element, replaced by their sigmoid(x / 2).  -> r = (mean_prob, std_half, entropy, mutual_info)
template <int T>
__device__ __forceinline__ void unc_element(float (&c)[T], int full, float (&r)[4]) {
#pragma clang fp contract(off)   // the 16-byte and the element-wise kernel give the same bits: no product is fused with a sum in one only
    float sp = 0.f, sq = 0.f, sh = 0.f;
    double hm = 0.0;                 // the deviations and their squares are summed in double, as torch.std on the CPU sums them: what
                                     // is left of the error is that of the T fp32 sigmoids
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const float x = c[t], a = fabsf(x);
        const float s = expf(-0.5f * a), e = __fmul_rn(s, s);
        const float hb = 1.f / (1.f + s), pb = 1.f / (1.f + e);          // the sigmoids at +|x| / 2 and +|x|, both >= 1/2
        const float hs = __fmul_rn(s, hb), ps = __fmul_rn(e, pb);        // ... at -|x| / 2 and -|x|
        const bool pos = x >= 0.f;
        c[t] = pos ? hb : hs;
        hm += (double)c[t];
        sp += pos ? pb : ps;
        if (full) {
            sq += pos ? ps : pb;
            sh += log1pf(e) + (e > 0.f ? __fmul_rn(a, ps) : 0.f);
        }
    }
    hm = hm / (double)T;
    double ss = 0.0;
#pragma unroll
    for (int t = 0; t < T; ++t) {
        const double d = (double)c[t] - hm;
        ss = fma(d, d, ss);
    }
    r[0] = sp / (float)T;
    r[1] = (float)sqrt(ss / (double)(T - 1));
    r[2] = r[3] = 0.f;
    if (full) {
        r[2] = unc_plogp(r[0]) + unc_plogp(sq / (float)T);
        r[3] = fmaxf(0.f, r[2] - sh / (float)T);
    }
}

__device__ __forceinline__ unsigned unc_u8(float std_half, float scale) {
    const float v = floorf(__fmul_rn(std_half, scale));
    return v >= 255.f ? 255u : v > 0.f ? (unsigned)(int)v : 0u;
}
