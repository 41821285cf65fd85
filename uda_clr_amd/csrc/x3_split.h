// The bf16x3 operand split and the packed operand layout, for every kernel that writes a packed operand: the packing pass
// (igemm_x3.hip) and the producers that write their result in packed form (bn_elementwise.hip, upconv.hip).
#pragma once
#include "common.h"

typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

// Packed operand ("x3 layout"): per row (pixel, or weight row) and per 16-wide K block the three bf16 pieces, 96 contiguous bytes:
//     element (row, k, piece q) at ((row * nb + k / 16) * 3 + q) * 16 + k % 16,   nb = K blocks per row.
// Activations: k = channel (nb = ceil(C / 16)).  Weights: k = position in the tap-chunked K order of the fp32 layout.
// k >= K inside the last block holds zero pieces.

// (v0, v1) -> the three bf16 pieces of each, packed (v0 in the low half).
// Domain: |v| <= 0x7F7F7FFF, the largest fp32 whose bf16 rounding is finite; above it the first piece is infinite and the split means
// nothing.  The pieces sum to v exactly wherever v is a multiple of 2^-133, bf16's smallest subnormal (every |v| >= 2^-110); below
// that the third piece is rounded to that grid (error <= 2^-134).  tests/kernel_spec.py x3_split states the same, bit for bit.
__device__ __forceinline__ void x3_split2(float v0, float v1, uint32_t& p1, uint32_t& p2, uint32_t& p3) {
    bf16x2 a = {(__bf16)v0, (__bf16)v1};                       // v_cvt_pk_bf16_f32 (round to nearest even)
    p1 = __builtin_bit_cast(uint32_t, a);
    const float r0 = v0 - __builtin_bit_cast(float, p1 << 16), r1 = v1 - __builtin_bit_cast(float, p1 & 0xffff0000u);   // exact
    bf16x2 b = {(__bf16)r0, (__bf16)r1};
    p2 = __builtin_bit_cast(uint32_t, b);
    const float s0 = r0 - __builtin_bit_cast(float, p2 << 16), s1 = r1 - __builtin_bit_cast(float, p2 & 0xffff0000u);   // exact
    bf16x2 c = {(__bf16)s0, (__bf16)s1};                       // s has <= 8 significant bits left: exact
    p3 = __builtin_bit_cast(uint32_t, c);
}

// A producer's store: the four values v of columns [k0, k0 + 4) (k0 % 4 == 0) of packed row `row`, 8 bytes into each piece.  Of the
// four only the first nvalid are columns of the matrix; the others are written as zeros (the padding of a ragged last block).
__device__ __forceinline__ void x3_store4(uint32_t* out, int64_t row, int nb, int k0, const float v[4], int nvalid) {
    uint32_t lo[3], hi[3];
    x3_split2(nvalid > 0 ? v[0] : 0.f, nvalid > 1 ? v[1] : 0.f, lo[0], lo[1], lo[2]);
    x3_split2(nvalid > 2 ? v[2] : 0.f, nvalid > 3 ? v[3] : 0.f, hi[0], hi[1], hi[2]);
    uint2* d = reinterpret_cast<uint2*>(out + ((row * nb + (k0 >> 4)) * 3) * 8 + ((k0 & 15) >> 1));
#pragma unroll
    for (int q = 0; q < 3; ++q) d[q * 4] = make_uint2(lo[q], hi[q]);
}

// Zero pieces for the columns [k0, 16 * nb) of packed row `row` (k0 % 4 == 0): what is left of a ragged last block behind the
// matrix's last four columns.
__device__ __forceinline__ void x3_store_pad(uint32_t* out, int64_t row, int nb, int k0) {
    for (int k = k0; k < nb * 16; k += 4) {
        uint2* d = reinterpret_cast<uint2*>(out + ((row * nb + (k >> 4)) * 3) * 8 + ((k & 15) >> 1));
#pragma unroll
        for (int q = 0; q < 3; ++q) d[q * 4] = make_uint2(0u, 0u);
    }
}

__host__ __device__ static inline int x3_blocks(int K) { return (K + 15) / 16; }      // nb of a row of K values
