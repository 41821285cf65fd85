// Tile and slab plan of proto_scatter_kernel (proto_scatter.hip), as plain numbers so that tests/test_domain_gap_cpu.py and
// tests/test_proto_scatter_gpu.py can read them.
//
// The C channels are cut into NB = ceil(C / PS_MT) blocks of PS_MT = 64; only the NPAIR = NB (NB + 1) / 2 block pairs bi <= bj are
// computed.  One workgroup of 4 waves owns one block pair over one range of pixels: wave k holds class k's 64 x 64 tile as 2 x 2
// accumulators of v_mfma_f32_32x32x2_f32 (the lower-left one of a diagonal pair is never computed).  The RAW features of PS_KP
// pixels x (64 + 64) channels are staged in LDS once per chunk and read by all four waves, which subtract their class's centre and
// apply their class's weight on the way to the operand registers.  LDS rows are PS_LD floats apart: PS_LD = 32 (mod 64 banks), so
// the two pixel rows one operand read touches (lanes 0-31 / 32-63) fall on disjoint banks.  There are two LDS images of a chunk
// (2 x PS_KP x PS_LD floats and 2 x PS_KP x 4 weights, 41 KiB): chunk c + 1 is loaded into registers before the math on chunk c and
// staged into the other image after it, with one barrier per chunk; two workgroups share a CU.
//
// The pixels are cut into slabs of PS_SLAB: one fp32 accumulator sums at most PS_SLAB pixels, then it is added into the workgroup's
// own fp64 partial tile in the workspace and cleared.  A pixel range ("split") is a whole number of slabs; there are at most
// ps_nsplit(C) of them - as many as put PS_TARGET_WG workgroups (2 per CU of 256) on the device, never more than PS_MAX_SPLIT - so
// the workspace, ps_nsplit(C) partial sets of NPAIR x 4 x 64 x 64 doubles, depends on C alone.  A second kernel adds the partial
// sets of the splits that ran, in split order, into both triangles of the output.
#pragma once

#define PS_SLAB 4096             /* pixels one fp32 accumulator sums before the fp64 combine */
#define PS_KP 32                 /* pixels per staged chunk (16 k-steps of the 32x32x2 MFMA) */
#define PS_MT 64                 /* channel block: 2 MFMA tiles of 32 */
#define PS_LD 160                /* LDS row stride in floats: 2 * PS_MT channels + 32 */
#define PS_MAX_C 1024
#define PS_TARGET_WG 512
#define PS_MAX_SPLIT 128

constexpr int ps_nblk(int C) { return (C + PS_MT - 1) / PS_MT; }
constexpr int ps_npair(int C) { return ps_nblk(C) * (ps_nblk(C) + 1) / 2; }
constexpr int ps_nsplit(int C) {
    const int n = (PS_TARGET_WG + ps_npair(C) - 1) / ps_npair(C);
    return n > PS_MAX_SPLIT ? PS_MAX_SPLIT : n;
}
constexpr unsigned long long ps_workspace_bytes(int C) {
    return (unsigned long long)ps_nsplit(C) * ps_npair(C) * 4 * PS_MT * PS_MT * sizeof(double);
}
static_assert(PS_SLAB % PS_KP == 0 && PS_KP % 2 == 0, "a slab is a whole number of chunks, a chunk a whole number of k-steps");
static_assert(PS_LD >= 2 * PS_MT && PS_LD % 64 == 32 && PS_LD % 4 == 0, "LDS rows: both channel blocks, odd multiple of 32 banks, float4 stores");
static_assert(ps_nsplit(1) >= 1 && ps_nsplit(PS_MAX_C) >= 1, "at least one split at every width");
