/* libuda_clr_hip.so - C ABI of the MI355X (gfx950) kernels behind the UDA_CLR per-step hot path.
 *
 * The reference (fengweie/UDA_CLR) is pure Python/PyTorch: it has no FFI of its own.  Each entry
 * point below replaces the ATen operator(s) that the cited reference line executes; the
 * reference-side binding a maintainer would add is the ctypes stub in INTEGRATION.md
 * (uda_clr_amd/kernels.py is that stub, grown into a class).
 *
 * Conventions
 *   - plain C: raw device pointers, sizes, a hipStream_t passed as void*; no C++/torch types.
 *   - every function returns 0 on success, a negative code on failure and never throws;
 *     uda_last_error() returns a thread-local message for the last failure.
 *   - kernels never allocate: outputs and workspaces are caller-owned (PyTorch caching allocator);
 *     workspace sizes come from the *_workspace_bytes queries.
 *   - launches are asynchronous on `stream`; functions are re-entrant (no global mutable state).
 *   - activations are NHWC fp32 matrices [P = N*H*W, ld] (channels fastest, ld % 4 == 0, base
 *     16-byte aligned, at least round4(C) readable floats per row).  uda_src_t adds the pending
 *     per-channel transform the consumer applies on load:
 *         u[p,c] = act(x[p,c]*scale[c] + shift[c]) * (mask[p,c] * mask_scale)
 *   - write footprint: an output matrix is written in rows [0, P) x columns [0, C) only (never the lanes [C, ld) of a row, so a
 *     column window of a wider matrix is a valid output), a contiguous output within its stated shape, a workspace within the
 *     queried bytes, an input never.  The one entry that writes lanes [C, round4(C)) says so (uda_dropout_mask).
 */
#ifndef UDA_CLR_HIP_H
#define UDA_CLR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-channel statistics are accumulated with fp64 atomics into UDA_STAT_SLOTS replicas
 * (slot = workgroup index mod UDA_STAT_SLOTS, spreads contention); consumers sum the replicas. */
#define UDA_STAT_SLOTS 16

#define UDA_ACT_NONE 0
#define UDA_ACT_RELU 1
#define UDA_ACT_RELU6 2

typedef struct uda_src {
    const float* x;       /* [P, ldx] */
    int64_t ldx;
    int32_t N, H, W, C;
    const float* scale;   /* [C] or NULL (identity) */
    const float* shift;   /* [C] or NULL */
    int32_t act;          /* UDA_ACT_* */
    int32_t _pad;
    const uint8_t* mask;  /* [P, ldm] keep-mask (1 = keep) or NULL */
    int64_t ldm;
    float mask_scale;     /* 1/(1-p) */
    float _pad2;
} uda_src_t;

const char* uda_last_error(void);
int uda_version(void);

/* ---- weight re-layouts (tiny; once per step).  torch layout OIHW in. */
/* K order of one weight row: k = 1: [round4(I)];  k > 1 ("tap-chunked"): [nCC][k*k][32] with nCC = ceil(round4(I)/32),
 * i.e. element (tap t, channel c) at ((c/32)*k*k + t)*32 + c%32, zero padded: all taps of one 32-channel slice are
 * consecutive K-chunks of the implicit GEMM, so a workgroup re-reads its pixel strip while it is L2-resident;
 * with round4(I) < 32 the row stays tap-major and unpadded, [k*k][round4(I)].
 * out[O][row as above]                              - operand of uda_conv_fwd              */
int uda_relayout_ohwi(const float* w, int O, int I, int k, float* out, void* stream);
/* out[I][row over O as above], taps flipped        - operand of uda_conv_fwd used as dgrad */
int uda_relayout_dgrad(const float* w, int O, int I, int k, float* out, void* stream);
/* depthwise [C][1][3][3] -> [9][C] */
int uda_relayout_dw(const float* w, int C, float* out, void* stream);

/* ---- dense convolution (stride 1; stride 2 on the wide tiles) as MFMA implicit GEMM (1x1, 3x3 with any dilation, and 2x2).
 * Replaces F.conv2d at mobilenet.py:43,49,57, aspp.py:50-53,56,59, decoder.py:20,32,33,37,41 and,
 * with uda_relayout_dgrad weights, their input-gradient.
 *   y[p,co] = bias[co] + addend[p,co] + sum_{t,ci} u(p+off_t, ci) * w[co][t][ci]
 * stats (optional, double[UDA_STAT_SLOTS][2][Cout], ADDED into): sum and sum of squares of y
 * before addend. */
/* UDA_MFMA_F32: v_mfma_f32_32x32x2_f32, the exact fp32 fma chain.  UDA_MFMA_BF16X3: fp32 emulated on the bf16 matrix pipe:
 * every operand is split exactly into three bf16 pieces (a = a1 + a2 + a3) and the six piece products down to 2^-24 relative
 * are accumulated in fp32 (v_mfma_f32_32x32x16_bf16) - same fp32-level error as the fma chain (measured per call against
 * float64 by tests/noise_report.py), 2.67x its matrix-pipe rate.  Inputs, outputs, accumulators and statistics stay fp32/fp64. */
#define UDA_MFMA_F32 0
#define UDA_MFMA_BF16X3 1
typedef struct uda_conv_args {
    uda_src_t src;
    const float* w;        /* [Cout][row], the layout uda_relayout_ohwi writes */
    int32_t Cout, ksize, dil;
    int32_t origin;        /* ksize 2 only: tap (kh,kw) reads pixel (h + kh - origin, w + kw - origin); 0 = the
                              space-to-depth form of the 4x4 stride-2 convs of GAN.py:90-101, 1 = its input gradient.
                              ksize 3 is centred (pad = dil), ksize 1 has one tap. */
    const float* bias;     /* [Cout] or NULL */
    const float* addend;   /* [P, ld_add] or NULL (may alias y) */
    int64_t ld_add;
    float* y;              /* [P, ldy] */
    int64_t ldy;
    double* stats;         /* [UDA_STAT_SLOTS][2][Cout] or NULL */
    int32_t mfma;          /* UDA_MFMA_*: which matrix instructions the wide (MFMA-bound) tiles use; narrow kernels ignore it */
    int32_t stride;        /* 0 | 1: stride 1.  2 (resnet.py:66,93; wide-tile kernels only: Cout > 96, K > 192, else an error):
                              y, addend, stats live on the grid ((H-1)/2+1) x ((W-1)/2+1), row (n,oh,ow) is centred on src pixel (n,2oh,2ow) */
    const void* x3_src;    /* UDA_MFMA_BF16X3, when uda_conv_uses_x3(a): src packed by uda_x3_pack (transform already applied) ... */
    const void* x3_w;      /* ... and the weight rows w ([Cout] rows of the relayouted row length) packed by uda_x3_pack */
    void* workspace;       /* optional, 16-byte aligned: uda_conv_fwd_workspace_bytes(a) bytes let the bf16x3 kernel split the last, */
    uint64_t workspace_bytes; /* partly filled round of tiles over K (fp32 partial tiles, summed in a fixed order); NULL / too small: not split */
} uda_conv_args_t;
/* 1 when uda_conv_fwd will run these arguments on the bf16x3 wide-tile kernel and therefore needs x3_src / x3_w */
int uda_conv_uses_x3(const uda_conv_args_t* a);
/* bytes of workspace these arguments can make use of (0: none; the conv runs the same without it) */
uint64_t uda_conv_fwd_workspace_bytes(const uda_conv_args_t* a);
int uda_conv_fwd(const uda_conv_args_t* a, void* stream);
/* The launch uda_conv_fwd plans for these arguments, as a short stable text "<family> <tile> ..." with the template variants and
 * splits: "stream 8x3", "narrow 128x96 pipe xf1", "ws 256x256 k3 xf2", "x3+tail 128x256 k3 full 256 tail 40x6", "heads 128x2";
 * "none" for arguments it refuses.  The plan is a function of the arguments alone (no pointer is dereferenced, no environment
 * read), and the only place where a kernel is chosen.  Returns the text's length as snprintf does, -1 without a buffer. */
int uda_conv_route(const uda_conv_args_t* a, char* buf, int len);
/* every "<family> <tile>" uda_conv_route / uda_conv_wgrad_route can begin with, one per line */
const char* uda_conv_route_list(void);
/* Operand packing for UDA_MFMA_BF16X3: every fp32 value as its three bf16 pieces, out[rows][ceil(C/16)][3][16] (96 contiguous
 * bytes per row and 16-wide block), rows = N*H*W of src, values = the TRANSFORMED ones act(x*scale+shift)*mask*mask_scale, so a
 * tensor is split once however many taps, workgroups or convolutions read it.  Weight rows: src with N = H = 1, W = rows,
 * C = row length, no transform.  uda_x3_packed_bytes(rows, C): size of out. */
uint64_t uda_x3_packed_bytes(int64_t rows, int K);
int uda_x3_pack(const uda_src_t* src, void* out, void* stream);

/* weight gradient of the same convolution: dw[co][ci][kh][kw] = sum_p dy[p,co]*u(p+off_t,ci) */
typedef struct uda_wgrad_args {
    uda_src_t src;
    const float* dy;       /* [P, lddy] */
    int64_t lddy;
    int32_t Cout, ksize, dil;
    int32_t origin;        /* as in uda_conv_args_t */
    float* dw;             /* OIHW, contiguous */
    float* workspace;
    uint64_t workspace_bytes;
    int32_t mfma;          /* UDA_MFMA_*, as in uda_conv_args_t */
    int32_t stride;        /* as in uda_conv_args_t: 2 = dy lives on the strided output grid (wide-tile kernels only) */
    const void* x3_src;    /* UDA_MFMA_BF16X3, when uda_conv_wgrad_uses_x3(a): src packed by uda_x3_pack (the forward conv's packed form) ... */
    const void* x3_dy;     /* ... and dy ([P] rows of Cout values) packed by uda_x3_pack */
} uda_wgrad_args_t;
uint64_t uda_conv_wgrad_workspace_bytes(int64_t P, int Cout, int Cin, int ksize);
int uda_conv_wgrad_uses_x3(const uda_wgrad_args_t* a);
int uda_conv_wgrad(const uda_wgrad_args_t* a, void* stream);
/* as uda_conv_route: "wgrad 64x64 S=12 red8", "wgrad-ws 256x256 xf1 S=2 red8", "wgrad-x3 128x256 S=12 red8" (S: splits of the
 * pixel range, red: the wgrad_reduce_kernel variant that sums them) */
int uda_conv_wgrad_route(const uda_wgrad_args_t* a, char* buf, int len);

/* ---- depthwise 3x3 (mobilenet.py:39,53; Aligned Xception, networks/backbone/xception.py:17-31): stride 1|2, dilation >= 1
 * (1|2|4 in the networks), "pad 0 on a padded input"; C a multiple of 4.
 * border_mode 0: out-of-image taps read 0 (xception.py:8-14, fixed_padding after the activation); 1: they read act(shift[c]) (quirk Q1).
 * Three kernel families serve it: UDA_DW_FLAT (all C/4 channel groups of a pixel in one workgroup; C <= 1024, the input gradient
 * any C), UDA_DW_TILED (32 channels x a halo tile in LDS; forward and weight gradient, dilation <= 2, C <= 1024) and UDA_DW_CB
 * (channel-blocked strips, C <= 2048).  `family` = UDA_DW_AUTO lets the library's launch plan choose by shape: channel-blocked
 * for C > 1024 and for dilation > 2 at C >= 1024, else tiled where it exists (forward / weight gradient at dilation <= 2), else
 * flat.  Any other value pins that family (kernel tests and measurements); a family that cannot serve the shape is an error.
 * The plan is a function of the arguments alone (no pointer is dereferenced, no environment read) and the only place where a
 * kernel, its grid or a template variant is chosen.  Workspace of the weight gradient: uda_dwconv_workspace_bytes, enough for
 * whichever family serves C. */
#define UDA_DW_AUTO 0
#define UDA_DW_FLAT 1
#define UDA_DW_TILED 2
#define UDA_DW_CB 3
#define UDA_DW_FWD 0
#define UDA_DW_DGRAD 1
#define UDA_DW_WGRAD 2
uint64_t uda_dwconv_workspace_bytes(int64_t Pout, int C);
int uda_dwconv_fwd(const uda_src_t* src, const float* w9c, int stride, int dil, int border_mode,
                   float* y, int64_t ldy, double* stats /* [SLOTS][2][C] or NULL */, int family, void* stream);
int uda_dwconv_dgrad(const float* dy, int64_t lddy, const float* w9c, int C, int stride, int dil,
                     int N, int H, int W, float* dx, int64_t lddx, int family, void* stream);
int uda_dwconv_wgrad(const uda_src_t* src, const float* dy, int64_t lddy, int stride, int dil,
                     int border_mode, float* dw /* [C][9] */, float* workspace,
                     uint64_t workspace_bytes, int family, void* stream);
/* The launch planned for op (UDA_DW_FWD / _DGRAD / _WGRAD) on an N x H x W x C input grid, as uda_conv_route: a short stable
 * text "<op> <kernel> ..." followed by the grid, the pixel lanes of a workgroup and lg (log2 of the float4 groups of a channel
 * block): "fwd tiled-8x16 grid 12x30 lds 19584", "dgrad flat grid 8192", "wgrad cb grid 3x6 lanes 4 lg 6"; "none" for arguments
 * the entry refuses.  Returns the text's length as snprintf does, -1 without a buffer. */
int uda_dwconv_route(int op, int N, int H, int W, int C, int stride, int dil, int family, char* buf, int len);
/* every "<op> <kernel>" uda_dwconv_route can begin with, one per line */
const char* uda_dwconv_route_list(void);

/* ---- stem conv 3x3 stride 2 pad 1, 3 -> 32, NCHW image in, NHWC out (mobilenet.py:10).  Output rows that are a multiple of 256
 * pixels wide run on row-staged kernels (the weight gradient only with dy 16-byte aligned and lddy % 4 == 0), anything else on
 * the per-pixel kernels: the stem's launch plan, what uda_stem_route reports. */
uint64_t uda_stem_workspace_bytes(int64_t Pout);
int uda_stem_fwd(const float* x, int N, int H, int W, const float* w, float* y, int64_t ldy,
                 double* stats /* [SLOTS][2][32] or NULL */, void* stream);
int uda_stem_wgrad(const float* x, int N, int H, int W, const float* dy, int64_t lddy, float* dw,
                   float* workspace, uint64_t workspace_bytes, void* stream);
/* op UDA_DW_FWD or UDA_DW_WGRAD (lddy, dy_aligned16: the weight gradient's dy): "fwd rows", "fwd pixels", "wgrad rows" or
 * "wgrad pixels", then the grid; "none" for refused arguments.  Same contract as uda_dwconv_route. */
int uda_stem_route(int op, int N, int H, int W, int64_t lddy, int dy_aligned16, char* buf, int len);

/* ---- ResNet-101 variant (BASELINE.json configs[4]; networks/backbone/resnet.py)
 * conv1 7x7 stride 2 pad 3, 3 -> 64, NCHW image in, NHWC out (resnet.py:59,114); W % 8 == 0 */
uint64_t uda_stem7_workspace_bytes(int64_t Pout);
int uda_stem7_fwd(const float* x, int N, int H, int W, const float* w, float* y, int64_t ldy,
                  double* stats /* [SLOTS][2][64] or NULL */, void* stream);
int uda_stem7_wgrad(const float* x, int N, int H, int W, const float* dy, int64_t lddy, float* dw,
                    float* workspace, uint64_t workspace_bytes, void* stream);
/* MaxPool2d(3, 2, 1) of the pending transform of src (resnet.py:63,117).  idx[p,c] = winning tap
 * kh*3+kw (first maximum in scan order, as ATen); the backward gathers dz through idx. */
int uda_maxpool_fwd(const uda_src_t* src, float* out, int64_t ldo, uint8_t* idx, int64_t ldi, void* stream);
int uda_maxpool_bwd(const float* dz, int64_t lddz, const uint8_t* idx, int64_t ldi, int N, int H, int W,
                    int C, float* du, int64_t ldu, void* stream);
/* every stride-th pixel of an [N,H,W,C] matrix (scatter = 0) or the transpose, zero insertion
 * (scatter = 1, dst is the H x W side): the stride-2 convs of resnet.py:13,76-79 around the stride-1 kernels */
int uda_rows_stride(const float* src, int64_t ld_src, int N, int H, int W, int C, int stride, int scatter,
                    float* dst, int64_t ld_dst, void* stream);
/* Bottleneck tail (resnet.py:37-41): out = relu(transform(a) + transform(b)) */
int uda_bn_add_relu(const uda_src_t* a, const uda_src_t* b, float* out, int64_t ldo, void* stream);
/* its backward gate: out = dz where z > 0 else 0 */
int uda_relu_gate(const float* dz, int64_t lddz, const float* z, int64_t ldz, int64_t P, int C, float* out,
                  int64_t ldo, void* stream);

/* ---- DRN-D-54 head (networks/backbone/drn.py): the layers no other backbone has
 * layer0: conv 7x7 stride 1 pad 3, 3 -> 16, NCHW image in, NHWC out (drn.py:124-129, 214).  w_hwio: the weight as
 * [7][7][3][16] (taps, input channel, output channels fastest; 16-byte aligned).  The weight gradient comes out OIHW. */
uint64_t uda_stem7s1_workspace_bytes(int64_t P);
int uda_stem7s1_fwd(const float* x, int N, int H, int W, const float* w_hwio, float* y, int64_t ldy,
                    double* stats /* [SLOTS][2][16] or NULL */, void* stream);
int uda_stem7s1_wgrad(const float* x, int N, int H, int W, const float* dy, int64_t lddy, float* dw,
                      float* workspace, uint64_t workspace_bytes, void* stream);
/* narrow dense 3x3 convolution, pad 1, dilation 1: C and Cout each 16, 32 or 64, stride 1 or 2 (anything else is an error) -
 * layer1 16 -> 16, layer2 16 -> 32 stride 2 (drn.py:131-134, 196-206, 216-217), layer3.0.conv2 64 -> 64 stride 2 (drn.py:69-71, 86).
 *   y[(n,oh,ow), co] = sum_{kh,kw,ci} u(n, s*oh + kh - 1, s*ow + kw - 1, ci) * w_hwio[kh][kw][ci][co]
 * u = the pending transform of src (no dropout mask), 0 outside the image; y and stats live on the grid
 * ((H-1)/s+1) x ((W-1)/s+1).  With w_hwio[kh][kw][co][ci] = w[co][ci][2-kh][2-kw] the stride-1 form is the input gradient.
 * uda_conv3n_wgrad: dw[co][ci][kh][kw] (OIHW) = sum_p dy[p,co] * u(...), dy on the strided grid. */
int uda_conv3n_fwd(const uda_src_t* src, const float* w_hwio, int Cout, int stride, float* y, int64_t ldy,
                   double* stats /* [SLOTS][2][Cout] or NULL */, void* stream);
uint64_t uda_conv3n_workspace_bytes(int Cin, int Cout);
int uda_conv3n_wgrad(const uda_src_t* src, const float* dy, int64_t lddy, int Cout, int stride, float* dw,
                     float* workspace, uint64_t workspace_bytes, void* stream);

/* ---- patch discriminators (networks/GAN.py:86-148): Conv2d(4, stride 2, pad 2) = ksize-2
 * uda_conv_fwd on the space-to-depth image z[n,i,j,(a,b,c)] = x[n, 2i+a-2, 2j+b-2, c] (zero outside the valid
 * region valid_h x valid_w of the [N,Hs,Ws,C] source grid; Hz = (valid_h+5)/2).  uda_s2d_fwd also applies the
 * previous layer's LeakyReLU (slope; 1 = none); uda_s2d_bwd routes dz back to the source grid (zeros outside
 * the valid region), times the LeakyReLU gate read from the sign of z (z_sign NULL = no gate).
 * nchw_*: the source side is an NCHW tensor (the discriminator input / its gradient). */
/* weight [O, C, 4, 4] -> operand of the ksize-2 uda_conv_fwd on z: dgrad = 0: [O][row over (a,b,c)], wz[o,(u,v),(a,b,c)] =
 * w[o,c,2u+a,2v+b]; dgrad = 1: [4C][row over o] with flipped taps (its input gradient).  Rows as uda_relayout_ohwi writes them. */
int uda_relayout_s2d(const float* w, int O, int C, int dgrad, float* out, void* stream);
int uda_s2d_fwd(const float* src, int64_t ld_src, int nchw_in, int N, int Hs, int Ws, int C, int valid_h,
                int valid_w, float slope, float* z, int64_t ld_z, int Hz, int Wz, void* stream);
int uda_s2d_bwd(const float* dz, const float* z_sign, int64_t ld_z, int Hz, int Wz, float slope, int N, int Hs,
                int Ws, int C, int valid_h, int valid_w, float* dst, int64_t ld_dst, int nchw_out, void* stream);
/* uda_s2d_bwd (rows out) with the LeakyReLU gate read from the sign of the forward's SOURCE rows [N, Hs, Ws, C] (the previous
 * layer's raw output: z = lrelu(source), same signs) - for when the fp32 z image was never written, see below. */
int uda_s2d_bwd_gate(const float* dz, int64_t ld_z, int Hz, int Wz, const float* gate_rows, int64_t ld_gate, float slope,
                     int N, int Hs, int Ws, int C, int valid_h, int valid_w, float* dst, int64_t ld_dst, void* stream);
/* bf16x3 mode (GAN.py:102-107 / :135-140, layers 2-4): the space-to-depth operands in PACKED form without their fp32 images.
 * uda_x3_pack_s2d_fwd = uda_s2d_fwd + uda_x3_pack of z (out: uda_x3_packed_bytes(N*Hz*Wz, 4C) bytes); uda_x3_pack_s2d_bwd =
 * uda_s2d_bwd_gate + uda_x3_pack of the routed gradient (out: uda_x3_packed_bytes(N*Hs*Ws, C) bytes).  C % 8 == 0.  The results
 * are bit-identical to the two-pass forms (the split is exact); one read of the source and one packed write instead of a read,
 * an fp32 write, an fp32 read and the packed write. */
int uda_x3_pack_s2d_fwd(const float* src, int64_t ld_src, int N, int Hs, int Ws, int C, int valid_h, int valid_w, float slope,
                        int Hz, int Wz, void* out, void* stream);
int uda_x3_pack_s2d_bwd(const float* dz, int64_t ld_z, int Hz, int Wz, const float* gate_rows, int64_t ld_gate, float slope,
                        int N, int Hs, int Ws, int C, int valid_h, int valid_w, void* out, void* stream);

/* ---- batch-norm pieces (F.batch_norm, training and eval) */
/* stats: double[UDA_STAT_SLOTS][2][C] */
int uda_bn_finalize(const double* stats, int C, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, float momentum, float eps, float* scale,
                    float* shift, float* mean, float* invstd, void* stream);
/* k more momentum updates of the running statistics with unchanged batch statistics over `count`
 * elements (the 4 stochastic passes of Trainer_prototype_full.py:364-368 repeat the deterministic,
 * pre-dropout part of the network on the same batch) */
int uda_bn_running_replay(const float* mean, const float* invstd, int C, double count, int k, float momentum,
                          float eps, float* running_mean, float* running_var, void* stream);
int uda_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, int C, float eps, float* scale, float* shift,
                       void* stream);
/* TransNorm, the --use_TN normalisation (networks/sync_batchnorm/batchnorm.py:436-520, training branch :445-495,
 * eval branch :497-520).  Training: a batch is normalised per domain half (first N/2 images "source", the rest
 * "target"): the caller runs uda_bn_finalize once per half (its own statistics accumulator, count and running
 * buffers), then uda_tn_gain turns the two accumulators into gain[c] = 1 + C p_c / sum(p),
 * p_c = 1 / (1 + |mu_s/sqrt(var_s+eps) - mu_t/sqrt(var_t+eps)|) (unbiased variances, :474-483) and multiplies
 * both halves' scale/shift by it in place (the reference's z * (1 + alpha.detach()), :495).  Eval: the target
 * running statistics normalise and the gain comes from the two pairs of running statistics (:501-520). */
int uda_tn_gain(const double* stats0, const double* stats1, int C, double count0, double count1, float eps,
                float* scale0, float* shift0, float* scale1, float* shift1, float* gain, void* stream);
int uda_tn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean_source,
                       const float* running_var_source, const float* running_mean_target,
                       const float* running_var_target, int C, float eps, float* scale, float* shift, void* stream);
/* out = transform(src) + residual */
int uda_bn_apply(const uda_src_t* src, const float* residual, int64_t ldr, float* out, int64_t ldo,
                 void* stream);
/* out (double[UDA_STAT_SLOTS][nq][C], ADDED into): nq=1 sum, nq=2 sum and sum of squares of x */
int uda_colstats(const float* x, int64_t ldx, int64_t P, int C, int nq, double* out, void* stream);
/* the same into a channel WINDOW of a wider accumulator double[UDA_STAT_SLOTS][nq][out_C]: out points at the window's first
 * channel (slot 0, quantity 0).  The statistics of decoder.py:23's BatchNorm(305) over cat(up(x), low-level, boundary) are
 * gathered this way: the upsampled channels by uda_upsample_fwd_stats, the other 49 by one window pass. */
int uda_colstats_window(const float* x, int64_t ldx, int64_t P, int C, int nq, double* out, int out_C, void* stream);
/* g = dU*mask*act'(a);  sums (double[UDA_STAT_SLOTS][3][C], ADDED into) = (sum g, sum g*xhat, sum dU) */
int uda_bnbwd_reduce(const float* dU, int64_t ldu, const uda_src_t* y, const float* mean,
                     const float* invstd, double* sums, void* stream);
/* sums: double[UDA_STAT_SLOTS][3][C].  count = elements per channel of the batch statistics; +infinity for a FROZEN
 * (eval-mode) BatchNorm, DeepLab.freeze_bn() of deeplabv3.py:43-50: c1 = c2 = 0, dx = scale * g, dgamma / dbeta as usual with
 * mean / invstd = the running statistics.  q1_total ([C] or NULL = 0): sum of the upstream gradient over ALL positions of the
 * zero-padded block input (quirk Q1) - needed when the depthwise BatchNorm behind this one is frozen. */
int uda_bnbwd_finalize(const double* sums, int C, double count, int q1_border, int act,
                       const float* shift, const float* mean, const float* invstd, const float* q1_total,
                       float* c1, float* c2, float* dgamma, float* dbeta, void* stream);
/* out = addend + scale*(g - c1 - xhat*c2) */
int uda_bnbwd_apply(const float* dU, int64_t ldu, const uda_src_t* y, const float* mean,
                    const float* invstd, const float* c1, const float* c2, const float* addend,
                    int64_t ld_add, float* out, int64_t ldo, void* stream);
/* The same two passes with the upstream gradient in LOW-RANK form dU[p, c] = sum_{o < k} d[p, o] * w[o, c] (k = 1 or 2, w row-major
 * [k][C]): the input gradient of a 1x1 conv to k outputs - the decoder's heads, decoder.py:32 (305 -> 2) and :41 (256 -> 1) - is
 * formed inside the passes instead of being written by a conv and read back twice. */
int uda_bnbwd_reduce_lowrank(const float* d, int64_t ldd, int k, const float* w, const uda_src_t* y, const float* mean,
                             const float* invstd, double* sums, void* stream);
int uda_bnbwd_apply_lowrank(const float* d, int64_t ldd, int k, const float* w, const uda_src_t* y, const float* mean,
                            const float* invstd, const float* c1, const float* c2, const float* addend, int64_t ld_add,
                            float* out, int64_t ldo, void* stream);
/* The two apply passes with a packed destination: out_x3 (uda_x3_packed_bytes(P, C) bytes, 16-byte aligned) receives the result as
 * the bf16x3 operand uda_x3_pack would make of out - the same bytes, the split is exact and both destinations are written from one
 * value - in the same pass.  out == NULL: only the packed form is written (a gradient matrix that only bf16x3 convs read);
 * out_x3 == NULL: uda_bnbwd_apply / uda_bnbwd_apply_lowrank. */
int uda_bnbwd_apply_x3(const float* dU, int64_t ldu, const uda_src_t* y, const float* mean,
                       const float* invstd, const float* c1, const float* c2, const float* addend,
                       int64_t ld_add, float* out, int64_t ldo, void* out_x3, void* stream);
int uda_bnbwd_apply_lowrank_x3(const float* d, int64_t ldd, int k, const float* w, const uda_src_t* y, const float* mean,
                               const float* invstd, const float* c1, const float* c2, const float* addend, int64_t ld_add,
                               float* out, int64_t ldo, void* out_x3, void* stream);

/* ---- resampling / pooling (F.interpolate bilinear align_corners=True, adaptive_avg_pool2d) */
int uda_upsample_fwd(const float* x, int64_t ldx, int N, int h, int w, int C, float* out,
                     int64_t ldo, int H, int W, void* stream);
/* uda_upsample_fwd + per-channel (sum, sum of squares) of the output ADDED into channels [0, C) of
 * stats = double[UDA_STAT_SLOTS][2][stat_C]; needs 256 % (C / 4) == 0 */
int uda_upsample_fwd_stats(const float* x, int64_t ldx, int N, int h, int w, int C, float* out, int64_t ldo, int H, int W,
                           double* stats, int stat_C, void* stream);
/* (out = NULL: statistics only, the upsampled tensor is not written.)
 * uda_mc_seg_head: the segmentation head of a no-grad stochastic pass (Trainer_prototype_full.py:358-368; decoder.py:23-32,51-53):
 *     x1b[p, o] = bias[o] + sum_c w[o][c] * mask[p, c] * mask_scale * act(scale[c] * xf[p, c] + shift[c]),  o = 0, 1,
 *     xf[p, :] = cat(bilinear_up(feature)[p, 0:Cf], low[p mod P_low, 0:Cl], boundary[p])
 * WITHOUT the [P, Cf + Cl + 1] x_feature matrix: the upsampled channels are interpolated on the fly from feature [N*h*w, Cf], the
 * low-level channels come from the un-repeated rows low [P_low, Cl] (x.repeat(2) shares them), the boundary logit from its own
 * column.  weight: two rows of ldw floats (uda_relayout_ohwi of decoder.last_conv.3.weight); mask: uint8 [P][ldm] or NULL. */
int uda_mc_seg_head(const float* feature, int64_t ld_feat, int N, int h, int w, int Cf, const float* low, int64_t ld_low,
                    int Cl, int64_t P_low, const float* boundary, int64_t ld_bnd, int H, int W, const float* scale,
                    const float* shift, int act, const uint8_t* mask, int64_t ldm, float mask_scale, const float* weight,
                    int64_t ldw, const float* bias, float* out, int64_t ldo, void* stream);
int uda_upsample_bwd(const float* dout, int64_t ldo, int N, int H, int W, int C, float* dx,
                     int64_t ldx, int h, int w, void* stream);
/* NHWC [N*h*w, C<=4] -> contiguous NCHW [N][C][H][W] and its adjoint */
int uda_head_upsample_fwd(const float* x, int64_t ldx, int N, int h, int w, int C, float* out,
                          int H, int W, void* stream);
int uda_head_upsample_bwd(const float* dout, int N, int C, int H, int W, float* dx, int64_t ldx,
                          int h, int w, int accumulate, void* stream);
/* out[n,c] = scale * sum_{p in image n} x[p,c] */
int uda_gap_fwd(const float* x, int64_t ldx, int N, int HW, int C, float scale, float* out,
                int64_t ldo, void* stream);
/* out[p,c] = addend[p,c] + scale*g[n(p),c] */
int uda_broadcast_rows(const float* g, int64_t ldg, int N, int HW, int C, float scale,
                       const float* addend, int64_t ld_add, float* out, int64_t ldo, void* stream);

/* ---- dropout keep-mask, Philox4x32-10 counter stream (nn.Dropout at aspp.py:62, decoder.py:31,36,40).
 * Written in 4-byte words: round4(C) bytes of every row, i.e. also the lanes [C, round4(C)) - the mask must be a matrix of its
 * own (ldm >= round4(C), 4-byte aligned), not a column window with live bytes beside it. */
int uda_dropout_mask(uint8_t* mask, int64_t ldm, int64_t P, int C, float p, uint64_t seed,
                     uint64_t offset, void* stream);

/* ---- segmentation loss: BCELoss(sigmoid(o), map) + MSELoss(sigmoid(b), boundary), both 'mean'
 * (Trainer_prototype_full.py:18-19,292-294; Trainer_baseline.py:206-208; log clamp -100).
 * loss3 (device float[3]) = (total, bce, mse); workspace2 = device double[2].
 * bwd: d_o / d_b = gradient of the total times the device scalar *gscale. */
int uda_seg_loss_fwd(const float* o, const float* map, int64_t n_o, const float* b, const float* boundary,
                     int64_t n_b, float* loss3, double* workspace2, void* stream);
int uda_seg_loss_bwd(const float* o, const float* map, int64_t n_o, const float* b, const float* boundary,
                     int64_t n_b, const float* gscale, float* d_o, float* d_b, void* stream);
/* counts[c][3] = (intersection, predicted, ground-truth) pixels for sigmoid(logit) > thr
 * (utils/metrics.py:118-132,149-168: Dice, pixel accuracy and IoU follow from them) */
int uda_seg_counts(const float* logits, const float* target, int B, int C, int64_t HW, float thr,
                   uint64_t* counts, void* stream);

/* ---- category prototypes (utils/Utils.py:108-131, 159-225) */
/* preds [T][n] logits -> unbiased std over T of sigmoid(x/2), mean over T of sigmoid(x)  (T = 8).
 * T identical passes give a std of exactly 0 (the mean of the T values is a pairwise sum), as torch.std does. */
int uda_mc_stats(const float* preds, int T, int64_t n, float* std_map, float* mean_map, void* stream);
/* wts [P][4] for the classes (cup obj, disc obj, cup bck, disc bck);
 * mode 0: from a [B,2,H,W] map, nearest-resized to h x w;  mode 1: from sigmoid of [P,2] logits;
 * mode 2: retrified pseudo labels (sigmoid>0.75) x (bilinear(std)<0.04) x bilinear(mean) */
int uda_proto_weights(int mode, int B, int h, int w, int H, int W, const float* map, const float* logits,
                      int64_t ldl, const float* std_map, const float* mean_map, float* wts, float* mask0,
                      float* mask1, void* stream);
uint64_t uda_proto_workspace_bytes(int64_t P, int C);
/* sums (double[4][C+1], ADDED into): weighted channel sums, then the weight total, per class.
 * Supported widths: 1 <= C <= 1024, every one of them (the kernel's LDS plan is csrc/proto_plan.h); any P >= 1.  feat and wts
 * 16-byte aligned, ldf % 4 == 0 and ldf >= C rounded up to 4 (the lanes from C up to that multiple are read and discarded).  The
 * combine runs in a fixed order: the same inputs give the same bits. */
int uda_proto_reduce(const float* feat, int64_t ldf, int64_t P, int C, const float* wts, double* sums,
                     float* workspace, uint64_t workspace_bytes, void* stream);
int uda_proto_finalize(const double* sums, int C, float* centroids /* [4][C] */, void* stream);
/* Second moments of the four classes for the domain-gap report (uda_clr_amd/domain_gap.py): the centred, weighted
 * scatter of the features that utils/Utils.py:108-131 averages into prototypes and Trainer_prototype_full.py:428-444 aligns,
 *     scatter[k][i][j] += sum_p w_k[p] (f[p,i] - a_k[i]) (f[p,j] - a_k[j]),   k < 4,  i, j < C.
 * feat: the [P, C] rows uda_proto_reduce takes - 16-byte aligned, ldf % 4 == 0, ldf >= C rounded up to 4; the lanes from C up to that
 * multiple may hold anything (NaN included) and reach no result; nothing behind that lane of row P - 1 is read; offsets are 64-bit.
 * wts [P][4]: what uda_proto_weights writes (soft weights allowed; w_{k+2} = 1 - w_k is NOT assumed).  centre [4][C], or null for
 * zeros.  scatter: double [4][C][C], ADDED into.  Every C in 1..1024, any P >= 1; a bad argument returns the error before
 * anything is written.
 * Arithmetic: products and the sum over pixels on the exact-fp32 MFMA (bitwise an fmaf chain); one fp32 accumulator sums at most
 * PS_SLAB pixels (csrc/scatter_plan.h), slab partials are combined in fp64 in a fixed order, no atomics: the same inputs give the
 * same bits.  Only channel blocks i-block <= j-block are computed and the other triangle is a copy: [k][i][j] and [k][j][i] are
 * bitwise equal (given that they were on entry).  The workspace holds a fixed number of fp64 partial sets and depends on C alone. */
uint64_t uda_proto_scatter_workspace_bytes(int C);
int uda_proto_scatter(const float* feat, int64_t ldf, int64_t P, int C, const float* wts /* [P][4] */,
                      const float* centre /* [4][C], null = zeros */, double* scatter /* [4][C][C], ADDED into */,
                      void* workspace, uint64_t workspace_bytes, void* stream);
/* adjoint of centroid = sum/count: d_feat[P,C] (optional, optionally accumulated) and d_w[P,4] (optional) */
int uda_proto_bwd(const float* feat, int64_t ldf, int64_t P, int C, const float* wts, const double* sums,
                  const float* dC, float* coef_ws /* float[4][C+1] */, float* d_feat, int64_t ldd,
                  int accumulate, float* d_w, void* stream);

/* out[p][k] = sum_c feat[p,c]*coef[k][c] + coef[k][C], k < 4 (coef: float[4][C+1]) and its adjoint
 * d_feat[p,c] (+)= sum_k wts[p][k]*coef[k][c].  Used by the prototype-guided discriminative loss
 * (no shipped source - parity unpinned). */
int uda_feat_dot4(const float* feat, int64_t ldf, int64_t P, int C, const float* coef, float* out, void* stream);
int uda_feat_rank4(const float* wts, const float* coef, int64_t P, int C, float* d_feat, int64_t ldd,
                   int accumulate, void* stream);

/* ---- torch.optim.Adam update (no weight decay / amsgrad) over one flat fp32 buffer
 * (train_use_fix_initial.py:210-214).  The hyper-parameters arrive as doubles: 1 - beta, lr / (1 - beta1^step) and
 * sqrt(1 - beta2^step) are formed in double and rounded to fp32 where torch rounds them.  Used by uda_clr_amd.optim.FlatAdam. */
int uda_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr,
                  double beta1, double beta2, double eps, int64_t step, void* stream);

/* ---- "bilinear upsample, then 3x3 conv" without the high-resolution GEMM (networks/decoder.py:50-53 feeding
 * last_conv_boundary[0], decoder.py:33): the channel mixing of the upsampled part commutes with the interpolation, so the
 * caller runs the nine tap GEMMs at LOW resolution (g = f W_all^T, [N*h*w, 9*C], tap-major columns) and these kernels do
 * the interpolation.  fwd: y[p,:] = addend[p % addend_rows,:] + sum_t [p + d_t inside H x W] bilinear(g_t)(p + d_t),
 * align_corners=True, d_t = ((t/3) - 1, (t%3) - 1) * dil.  bwd: dg = adjoint of that sum applied to dy (gather form).
 * stats (double[UDA_STAT_SLOTS][2][C], ADDED into, or null): per-channel sum / sum of squares of y for the next BatchNorm,
 * for every geometry: accumulated by the interpolation kernel where its launch plan (csrc/upconv_plan.h) says so, by a
 * uda_colstats launch over y after it on the same stream otherwise.  Since version 3 that includes operands beyond the 32-bit
 * extents of the strip kernels (N*h*w*ldg*4 >= 2^31 bytes of g, ...), where a call with stats was refused before. */
int uda_upconv_fwd(const float* g, int64_t ldg, int N, int h, int w, int C, int dil, const float* addend, int64_t ld_add,
                   int64_t addend_rows, float* y, int64_t ldy, int H, int W, double* stats, void* stream);
int uda_upconv_bwd(const float* dy, int64_t ldy, int N, int H, int W, int C, int dil, float* dg, int64_t ldg, int h, int w,
                   void* stream);
/* uda_upconv_bwd with a packed destination: dg_x3 (uda_x3_packed_bytes(N*h*w, 9*C) bytes) receives what uda_x3_pack would make of
 * dg, in the same pass; dg == NULL: only the packed form is written (ldg is not read, the launch is planned for ldg = 9*C). */
int uda_upconv_bwd_x3(const float* dy, int64_t ldy, int N, int H, int W, int C, int dil, float* dg, int64_t ldg, void* dg_x3,
                      int h, int w, void* stream);
/* The launch planned for uda_upconv_fwd (op 0) / uda_upconv_bwd (op 1) as text: "fwd tile", "fwd strip3", "fwd strip4",
 * "fwd pixel", "bwd wave" or "bwd thread", then the grid and for the tile kernel R, RC and lds; a forward route with want_stats
 * ends in "stats fused" or "stats colstats"; "none" for refused arguments.  has_addend ... want_stats are not read for op 1.
 * Same contract as uda_dwconv_route. */
int uda_upconv_route(int op, int N, int h, int w, int H, int W, int C, int dil, int64_t ldg, int has_addend, int64_t ld_add,
                     int64_t addend_rows, int want_stats, char* buf, int len);
/* every "<op> <kernel>" uda_upconv_route can begin with, one per line */
const char* uda_upconv_route_list(void);

/* ---- evaluation post-processing of the predicted probability maps (utils/Utils.py:427-463: postprocessing +
 * get_largest_fillhole), per image and channel (0 cup, 1 disc): threshold -> 5 x 7x7 median (zero padded) -> erosion by the
 * L1 ball of radius 7 (outside = set, skimage's convention) -> largest 8-connected component (first maximum in raster order of
 * the components' first pixels) -> holes filled (background not 4-connected to the border).
 * pred f32 [B,2,H,W] -> out uint8 [B,2,H,W] in {0,1}.  sweeps: launches of each of the two tile-wise propagations (a launch
 * carries labels across whole 32x32 tiles); not_converged: DEVICE int[2], set to the number of tiles an extra sweep still
 * changed (components, flood) - 0 means the result is final, otherwise call again with more sweeps. */
size_t uda_postprocess_workspace_bytes(int B, int H, int W);
int uda_postprocess(const float* pred, int B, int H, int W, float thr_cup, float thr_disc, int sweeps, uint8_t* out,
                    int* not_converged, void* workspace, size_t workspace_bytes, void* stream);

/* ---- prediction pictures (utils/Utils.py:515-585, save_per_img): the display mask per structure, the contour overlay and the
 * byte image it is painted on.  Channel 0 = cup, 1 = disc.
 * uda_display_masks: prob f32 [B,2,H,W] (read-only) -> out uint8 [B,2,H,W] in {0,1}: the outermost row / column ring read as 0 ->
 *   > thr (both channels) -> the chain of uda_postprocess (5 medians, erosion, largest component, fill) -> dilation by the L1
 *   ball of radius 7 (outside = unset) -> holes filled once more.  The reference's second largest-component step changes nothing
 *   (a diamond dilation of one 8-connected set is 8-connected) and is not run.  sweeps and not_converged as uda_postprocess, with
 *   DEVICE int[3]: components, first flood, second flood.  Limits and workspace rule as uda_postprocess.
 * uda_overlay_u8: image, out uint8 [B,H,W,3] (out may not alias image), masks uint8 [B,2,H,W] (nonzero = set).  The vertices of
 *   find_contours(mask, 0.5) on a binary mask are the midpoints of all 4-adjacent in-image pixel pairs that differ; each paints
 *   the seven pixels (int(y + dy), int(x + dx)), (dy, dx) in (0,0) (1,0) (1,1) (0,1) (-1,0) (-1,-1) (0,-1).  Channel 1's outline is
 *   (0, 255, 0), channel 0's (0, 0, 255) on top of it; every other pixel is the image's.  A target whose row or column lies outside
 *   the image is dropped (the reference raises at H / W and wraps at -1).  Computed as a gather, one thread per output pixel:
 *   every byte of out is written once, bit-identical from run to run and for an image alone or inside any batch.
 * uda_image_u8: x f32 [B,3,H,W] in [-1, 1] -> out uint8 [B,H,W,3] = clip(rint((x + 1) * 127.5), 0, 255), fp32, no fma.
 * H, W >= 1, H * W < 2^30; a null pointer, a bad size or a short workspace returns the error before any launch. */
size_t uda_display_masks_workspace_bytes(int B, int H, int W);
int uda_display_masks(const float* prob, int B, int H, int W, float thr, int sweeps, uint8_t* out, int* not_converged,
                      void* workspace, size_t workspace_bytes, void* stream);
int uda_overlay_u8(const uint8_t* image, const uint8_t* masks, int B, int H, int W, uint8_t* out, void* stream);
int uda_image_u8(const float* x, int B, int H, int W, uint8_t* out, void* stream);

/* ---- exact surface distances of one (prediction, ground truth) mask pair per image and class: what the per-image ASD /
 * ASSD / Hausdorff figures of an evaluation are closed forms of.  The reference keeps the 1-D scan of a squared distance
 * transform (utils/metrics.py:62-68, `_upscan`) without its callers; the masks are those of utils/Utils.py:438-463.
 * Conventions of medpy.metric.binary, distances in pixels:
 *   border(M) = M & ~erosion(M, 4-connected cross), everything outside the image unset;
 *   d2_X[y,x] = exact squared Euclidean distance (an integer) to the nearest pixel of border(X);
 *   directed entry A -> G:  n = |border(A)|,  s = sum over border(A) of sqrt(d2_G),  m = max over border(A) of d2_G.
 * pred, gt uint8 [B,2,H,W], nonzero = set.  1 <= H, W <= 1024 (and B <= 8192); anything else, or a workspace below
 * uda_surface_distance_workspace_bytes, returns the error before any launch.
 *   table  double [B][2 class][2 dir: 0 = pred -> gt, 1 = gt -> pred][3: n, s, m].  If either border set of an (image, class)
 *          is empty, both its entries are (n as counted, NaN, -1).  s is summed in a fixed order: bit-identical from run to
 *          run and independent of the batch an image sits in.
 *   counts int64 [B][2][3] = |pred & gt|, |pred|, |gt| (the per-image Dice counts).
 *   d2     null, or int32 [B][2][2: 0 = to the gt border, 1 = to the pred border][H][W]; -1 where that border set is empty. */
size_t uda_surface_distance_workspace_bytes(int B, int H, int W);
int uda_surface_distance(const uint8_t* pred, const uint8_t* gt, int B, int H, int W, double* table, int64_t* counts,
                         int32_t* d2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the same four passes (table, counts and d2 bit-identical to uda_surface_distance on the same masks) and a fifth over
 * the border sets and distance maps they leave: what hd95 (any percentile of the distances), the surface Dice at a tolerance
 * and the vertical cup-to-disc ratio are closed forms of.  Integers only, bit-identical from run to run, an image's rows the
 * same alone and inside any batch.
 *   quantiles HOST double[Q], 0 <= q <= 1, 0 <= Q <= 8;  tol2 HOST int32[T], squared tolerances >= 0, 0 <= T <= 8.
 *   order  int64 [B][2 class][3 set: 0 = pred -> gt, 1 = gt -> pred, 2 = both pooled][Q][2]: for a set of n squared distances,
 *          v = (double)(n - 1) * q (one IEEE multiply), lo = floor(v), hi = min(lo + 1, n - 1): the lo-th and the hi-th smallest
 *          squared distance (0-based).  (-1, -1) where either border set of the (image, class) is empty.
 *   within int64 [B][2][2 dir][T]: border pixels of that direction with d2 <= tol2[t]; -1 where either border set is empty.
 *   extent int64 [B][2][2 slot: 0 = ground truth, 1 = prediction][2]: smallest and largest row that holds a set pixel of that
 *          mask; (-1, -1) for an empty mask, whatever the other mask holds.
 * Limits and workspace as uda_surface_distance; Q or T out of range, a quantile outside [0, 1] or NaN, a negative tol2: the
 * error is returned before any launch and nothing is written.  order may be null at Q = 0, within at T = 0. */
size_t uda_surface_profile_workspace_bytes(int B, int H, int W);
int uda_surface_profile(const uint8_t* pred, const uint8_t* gt, int B, int H, int W, const double* quantiles, int Q,
                        const int32_t* tol2, int T, double* table, int64_t* counts, int64_t* order, int64_t* within,
                        int64_t* extent, int32_t* d2, void* workspace, size_t workspace_bytes, void* stream);

/* ---- optic-disc morphometry of one (cup, disc) mask pair per image: the integers that the horizontal, vertical and area cup-to-disc
 * ratios, the rim-to-disc profile around the disc, the cup's decentration and an ellipse summary of each structure are closed forms
 * of (utils/metrics.py, morphometry_from_moments).  The reference (utils/metrics.py, utils/Utils.py) has none of these figures: the
 * definitions are this project's.  Integers only, no floating-point atomics: bit-identical from run to run, an image's rows the same
 * alone and inside any batch.
 *   masks   uint8 [B][2: 0 cup, 1 disc][H][W], nonzero = set; never written.
 *   sectors DEVICE int64 [K][2] = (x, y) of K boundary rays in strictly counter-clockwise order, x to the right and y UP, |x|, |y| <=
 *           2^30 (utils.metrics.sector_table); K a multiple of 8, 8 <= K <= 360.  An argument, so that the kernel and any restatement
 *           of it decide on the same numbers.
 * Per image b and class k, r and c a pixel's row and column, all int64:
 *   moments [B][2][6] = (n, sum r, sum c, sum r^2, sum c^2, sum r*c) over the set pixels; zeros for an empty plane.
 *   extent  [B][2][4] = (first row, last row, first column, last column) with a set pixel; (-1, -1, -1, -1) for an empty plane.
 *   overlap [B]       = pixels set in both planes.
 *   radial  [B][2][K]: with (n, Sr, Sc) the DISC plane's n, sum r, sum c (the disc centroid is the origin for both classes) and
 *           u = (ux, uy) = (n * c - Sc, -(n * r - Sr)), cross(a, u) = a.x * u.y - a.y * u.x, s_K = s_0: a set pixel with u != 0
 *           belongs to the one sector j with cross(s_j, u) >= 0 and cross(s_j+1, u) < 0 (a pixel exactly on a boundary ray to the
 *           sector that starts there); radial[b][k][j] = the largest ux^2 + uy^2 over the pixels of class k in sector j, -1 if the
 *           sector holds none, -1 everywhere if the disc plane is empty.  A pixel with u = 0 is in no sector.  |u| < 2^30, so the
 *           cross products stay below 2^61 and |u|^2 below 2^60.  sqrt(radial) / n is a distance in pixels.
 * Limits as uda_surface_distance (1 <= H, W <= 1024, B <= 8192); a null pointer, a bad size, a K that is no multiple of 8 in 8..360
 * or a workspace below uda_disc_morphometry_workspace_bytes returns the error before any launch and writes nothing. */
size_t uda_disc_morphometry_workspace_bytes(int B, int H, int W, int K);
int uda_disc_morphometry(const uint8_t* masks, int B, int H, int W, const int64_t* sectors, int K, int64_t* moments, int64_t* extent,
                         int64_t* overlap, int64_t* radial, void* workspace, size_t workspace_bytes, void* stream);

/* ---- MC-dropout uncertainty at evaluation, and the integer tables that calibration and selective-prediction figures are closed
 * forms of (utils/metrics.py, calibration_from_table / selective_from_table).  The reference trusts a target pseudo-label where the
 * unbiased std over its T = 8 stochastic passes of sigmoid(x / 2) is below 0.04 (utils/Utils.py:165-166 `torch.sigmoid(preds / 2.0)`, `torch.std(preds, dim=0)`;
 * :197-200 `std_map_small < 0.04`) and never scores that rule against labels; the tables and the maps beyond std and mean are this project's.
 * uda_mc_uncertainty: logits f32 [T][n], 2 <= T <= 32, n > 0; one read of the logits; every output f32 [n] (std_u8: uint8 [n]) and
 *   optional - null = not written, at least one given:
 *     mean_prob   = mean_t sigmoid(x_t)
 *     std_half    = unbiased std over t of sigmoid(x_t / 2), two-pass (utils/Utils.py:165-166, at full resolution)
 *     entropy     = H(mean_prob), H(p) = -p log p - (1 - p) log(1 - p) in nats, 0 log 0 = 0
 *     mutual_info = max(0, H(mean_prob) - mean_t H(sigmoid(x_t)))
 *     std_u8      = min(255, (int)floorf(std_half * u8_scale)) of the very fp32 value stored to std_half (u8_scale finite, > 0)
 *   An element's outputs depend on its own T logits only: any chunking of n gives the same bits.  16-byte loads and stores where n
 *   % 4 == 0 and every pointer given is 16-byte (std_u8: 4-byte) aligned, element-wise otherwise.  uda_mc_stats is unchanged.
 * uda_selective_tables: prob, unc f32 [B][2][H][W] (either may be null); pred, gt uint8 [B][2][H][W], nonzero = set, gt null = pred;
 *   M confidence bins in 1..64; edges HOST float[K - 1], finite and strictly ascending, K uncertainty bins in 1..64 (read before the
 *   call returns, passed to the kernel by value); 1 <= H, W <= 1024, B <= 8192.  All outputs int64, exact functions of the floats:
 *     rel     [B][2][M][5] = (n, n_pos, sum q, sum q over gt-set pixels, sum q^2) per bin b = min(M - 1, (int)floorf(p * (float)M)),
 *             q = (int)rintf(p * 65536.0f) (an exact multiply; sum q^2 <= 2^52).  Null = not wanted; needs prob.
 *     risk    [B][2][K][4] = (TP, FP, FN, TN) of pred against gt per bin k = #{j : edges[j] <= u}: a value on an edge goes to the
 *             upper bin, +inf to the last.  Null = not wanted; needs unc.  At least one of rel and risk.
 *     invalid [B][2][2] = pixels whose p is NaN or outside [0, 1], pixels whose u is NaN or negative (-0.0 is not): each is left
 *             out of that table only.  A column whose table is not asked for stays 0.
 *   The entry zeroes the outputs it was given; no workspace.  Integer sums only: bit-identical from run to run, an image's rows the
 *   same alone and inside any batch.  A bad argument returns the error before anything is written. */
int uda_mc_uncertainty(const float* logits, int T, int64_t n, float* mean_prob, float* std_half, float* entropy, float* mutual_info,
                       uint8_t* std_u8, float u8_scale, void* stream);
int uda_selective_tables(const float* prob, const float* unc, const uint8_t* pred, const uint8_t* gt, int B, int H, int W, int M,
                         const float* edges, int K, int64_t* rel, int64_t* risk, int64_t* invalid, void* stream);

/* ---- test-time augmentation at evaluation (uda_clr_amd/tta.py): the image is predicted under V views, the predictions
 * are mapped back to the image's frame and reduced per element by the statistics of uda_mc_uncertainty (the same code: equal logits
 * give equal bits).  The reference evaluates one view (train_process/Trainer_prototype_full.py:358-368 are its only repeated
 * passes); every definition here is this project's.
 * A view is (g, h, w): g in 0..7, h and w multiples of 16 in 16..1024.  With R = bilinear(image -> (h, w)), align_corners=True (the
 * index and weight arithmetic of uda_head_upsample_fwd, every product and sum of the lerp rounded on its own),
 *     F[i][j] = R[(g & 2) ? h - 1 - i : i][(g & 1) ? w - 1 - j : j],   U = F if !(g & 4), else U[i][j] = F[j][i] (U is [w][h]):
 *   0 identity, 1 left-right mirror, 2 top-bottom mirror, 3 half turn, 4 transpose, 5 and 6 the quarter turns
 *   (torch.rot90(R, 1, (-2, -1)) and torch.rot90(R, -1, (-2, -1))), 7 anti-transpose.
 *   The inverse of a view, applied to logits L of U's shape: F'[a][b] = (g & 4) ? L[b][a] : L[a][b], R'[a][b] = F' at the mirrored
 *   indices as above, then bilinear(R' -> (H, W)), align_corners=True.
 * uda_tta_view: image f32 [B][C][H][W] -> out f32 [B][C][h'][w'] = U, (h', w') = (g & 4) ? (w, h) : (h, w).  With h == H and w == W the
 *   values are copied, no arithmetic.  16-byte stores along the rows of U; a transposed view goes through an LDS tile.
 * uda_tta_fuse: HOST arrays logits[V] (device pointers), g[V], h[V], w[V], 2 <= V <= 32, read before the call returns and passed to the
 *   kernel by value; tensor v is f32 [B][C][h_v'][w_v'], contiguous, 16-byte aligned.  For every element [b][c][y][x] of the H x W frame
 *   z_v, v = 0..V-1 in order, is the stored logit itself where (h_v, w_v) == (H, W) and the 4-tap interpolation of the inverse-mapped
 *   logits otherwise; the outputs are those of uda_mc_uncertainty on (z_0, ..., z_V-1): mean_prob, std_half, entropy, mutual_info f32
 *   [B][C][H][W], std_u8 uint8 [B][C][H][W] with u8_scale; null = not written, at least one given; float outputs 16-byte aligned,
 *   std_u8 4-byte aligned.  An element's outputs depend on its own taps only: an image alone and inside a batch gives the same bits.
 * 1 <= B <= 8192, 1 <= C <= 4, H and W multiples of 16 in 16..1024.  A null pointer (a null logits[v] included), V, g, a size, B or C
 * out of range returns the error before any launch and writes nothing.  No workspace, no atomics. */
int uda_tta_view(const float* image, int B, int C, int H, int W, int g, int h, int w, float* out, void* stream);
int uda_tta_fuse(const float* const* logits, const int* g, const int* h, const int* w, int V, int B, int C, int H, int W,
                 float* mean_prob, float* std_half, float* entropy, float* mutual_info, uint8_t* std_u8, float u8_scale, void* stream);

/* ---- device-side tail of the input pipeline. The reference's dataloader workers run these per sample
 * on the CPU with scipy.ndimage; here they run per uint8 BATCH on the GPU, bit-identical to the scipy calls.
 * uda_normalize_tf: dataloaders/custom_transforms.py:432-466 (Normalize_tf), :414-429 (GetBoundary), :504-507 (ToTensor).
 *   image_hwc uint8 [B,H,W,3], label uint8 [B,H,W] (grey code: > 200 background, 51..200 disc rim, <= 50 cup) ->
 *   image f32 [B,3,H,W] = v/127.5 - 1, map f32 [B,2,H,W] (cup, disc), boundary f32 [B,1,H,W] = uint8 Gaussian (sigma 3,
 *   scipy semantics: axis 0 then axis 1, each truncated to uint8, 'reflect') of the |dilate5 - erode5| ring, / 255.
 *   gauss_w: HOST pointer to radius+1 doubles, w[0] the centre tap, w[k] the taps at distance k (as numpy computes them). */
size_t uda_normalize_tf_workspace_bytes(int B, int H, int W);
int uda_normalize_tf(const uint8_t* image_hwc, const uint8_t* label, int B, int H, int W, const double* gauss_w, int radius,
                     float* image, float* map, float* boundary, void* workspace, size_t workspace_bytes, void* stream);
/* custom_transforms.py:95-147 (elastic_transform).  uda_field_smooth: out = alpha * gaussian_filter(noise, sigma,
 * mode='constant') on [B,H,W] float64 planes, in scipy's own summation order (bit-identical to the reference's field;
 * weights_dev: DEVICE pointer to radius+1 doubles, centre first; tmp: [B,H,W] doubles).
 * uda_elastic_warp: map_coordinates(order=1) of image (mode 'constant', 0 outside) and label (mode 'nearest') at
 * (h + dx, w + dy), rounded to uint8; apply (uint8 [B] or null) = 0 copies a sample through. */
int uda_field_smooth(const double* noise, int B, int H, int W, const double* weights_dev, int radius, double alpha, double* tmp,
                     double* out, void* stream);
/* custom_transforms.py:150-250 (add_salt_pepper_noise, adjust_light, eraser) on a uint8 batch IN PLACE, in that order, with the
 * per-sample parameters the dataloader workers drew: sp_pos int32 [B, sp_max, 2] (row, column), sp_count int32 [B], sp_value
 * int32 [B] (1 salt / 0 pepper, as the reference writes them); lut uint8 [B, 256] (identity when adjust_light did not fire);
 * erase_box int32 [B, 5] = (top, left, height, width, grey level), height 0 = no erasing. */
int uda_photometric_u8(uint8_t* image_hwc, int B, int H, int W, const int* sp_pos, const int* sp_count, const int* sp_value,
                       int sp_max, const uint8_t* lut, const int* erase_box, void* stream);
int uda_elastic_warp(const uint8_t* image_hwc, const uint8_t* label, const double* dx, const double* dy, const uint8_t* apply,
                     int B, int H, int W, uint8_t* image_out, uint8_t* label_out, void* stream);
/* custom_transforms.py:152-182,208-223,315-355 (RandomCrop, RandomFlip, RandomRotate, RandomScaleCrop): the PIL geometry at the
 * head of the chain, for a whole batch, from a device-resident copy of the decoded dataset and the draws the workers recorded.
 *   image_pool uint8: the sources' [H0,W0,3] images back to back; label_pool uint8: their [H0,W0] masks; offsets int64
 *   [n_sources]: first PIXEL of each source (x1 in label_pool, x3 in image_pool); sizes int32 [n_sources,2] = (H0, W0);
 *   src_index int64 [B]; records int32 [B,10] = (scale fired, scaled w, scaled h, pad width, crop x1, crop y1 in the padded
 *   image, counter-clockwise quarter turns, flip left-right, flip top-bottom, crop size); S the crop size.
 *   -> image_out uint8 [B,S,S,3], label_out uint8 [B,S,S]: byte for byte what Pillow gives (8-bit BILINEAR resample in its
 *   integer arithmetic, NEAREST mask with its accumulated double index; fill 0 / 255 in the pad).  Scaled sizes must keep
 *   in / out <= 2.5 per axis (the transform draws >= 0.5).  A source index outside [0, n_sources) yields the fill. */
size_t uda_geometry_u8_workspace_bytes(int B, int S);
int uda_geometry_u8(const uint8_t* image_pool, const uint8_t* label_pool, const int64_t* offsets, const int* sizes, int n_sources,
                    const int64_t* src_index, const int* records, int B, int S, uint8_t* image_out, uint8_t* label_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- Fourier Domain Adaptation of the source batch (Yang & Soatto, CVPR 2020; uda_clr_amd/ops.py fda_transfer): a source
 * image takes the amplitude spectrum of a target image on the (2 band + 1)^2 lowest frequencies Omega = [-band, band]^2 and keeps its
 * own phase.  The reference has no such stage (train_process/Trainer_prototype_full.py aligns features and categories, not images):
 * every definition here is this project's.  Per channel, with F[u,v] = sum_y sum_x s[y,x] e^{-2 pi i (u y / H + v x / W)},
 *     out = src + (1 / HW) sum_{(u,v) in Omega} (|F_t[u,v]| P[u,v] - F_s[u,v]) e^{+2 pi i (u y / H + v x / W)},
 *     P = F_s / |F_s|, and P = (1, 0) where |F_s[u,v]| <= 1e-6 H W (the zero-magnitude rule: numpy.angle(0) = 0),
 * which is what fft2 / fftshift / swap the window [H/2 - band, H/2 + band] x [W/2 - band, W/2 + band] of the amplitude / ifftshift /
 * ifft2 / real part gives.  All arithmetic from the bytes to the rounding is float64; twiddles are read from tables indexed by the
 * integers (v x) mod W and (u y) mod H; every sum has one order fixed by the shapes, no atomics: equal inputs give equal bytes.
 *   0 <= band <= UDA_FDA_MAX_BAND, 2 band + 2 <= min(H, W) (Omega stays clear of the Nyquist frequencies), 2 <= H, W <= 2048,
 *   1 <= B, Bt <= 8192.  A null pointer, a value out of range, sizes that differ or a workspace that is too small return the error
 *   before any launch and write nothing.  workspace: 16-byte aligned, uda_fda_workspace_bytes(B, Bt, H, W, band) bytes (Bt = 0: what
 *   uda_fda_spectrum needs for B images); 0 for arguments out of range.
 * uda_fda_spectrum: image_hwc uint8 [N,H,W,3] -> spectrum float64 [N,3,2 band + 1,band + 1,2] = (re, im) of F[n,c,u,v] at u = -band..band
 *   (index u + band), v = 0..band; the other half of Omega is F[-u,-v] = conj(F[u,v]).  16-byte aligned.
 * uda_fda_transfer: src_hwc uint8 [B,H,W,3], tgt_hwc uint8 [Bt,Ht,Wt,3] with (Ht, Wt) == (H, W); pair int32 [B] (DEVICE): source b takes
 *   the amplitudes of target pair[b] - a value outside [0, Bt) is clamped into it, not checked; apply uint8 [B] (DEVICE) or null = all:
 *   a sample with apply[b] == 0 is copied byte for byte.  -> out uint8 [B,H,W,3] = clip(rint(value), 0, 255), rint to even on ties. */
#define UDA_FDA_MAX_BAND 64
size_t uda_fda_workspace_bytes(int B, int Bt, int H, int W, int band);
int uda_fda_spectrum(const uint8_t* image_hwc, int N, int H, int W, int band, double* spectrum, void* workspace, size_t workspace_bytes,
                     void* stream);
int uda_fda_transfer(const uint8_t* src_hwc, int B, int H, int W, const uint8_t* tgt_hwc, int Bt, int Ht, int Wt, const int* pair,
                     const uint8_t* apply, int band, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- whole-photograph prediction (uda_clr_amd/wholephoto.py): from a fundus photograph of any size to the S x S ROI the
 * generator takes, and back.  The reference reads ROIs that were cut beforehand (dataloaders/fundus_dataloader.py:41 `ROIs/image`) and
 * ships no such stage: every definition here is this project's, except the ROI resample, which is Pillow's.
 *   pool uint8: the photographs' [H,W,3] images back to back, pool_pixels pixels in all; offsets int64 [n_sources]: first PIXEL of each;
 *   sizes int32 [n_sources,2] = (H, W), 1 <= H, W <= 8192; src_index int64 [B]: the photographs of this batch.  1 <= B <= 8192; S a
 *   multiple of 16 in 16..1024.  A source index outside [0, n_sources), or a table row that does not describe H x W pixels inside the
 *   pool, counts as "no photograph".  Nothing outside [pool, pool + 3 * pool_pixels) is read.
 *   Normalised outputs: f32 = fl(fl((float)v * fl(1 / 127.5f)) - 1.0f), product and difference each rounded to fp32, no fma: the bits of
 *   torch's `u8.float() / 127.5 - 1.0` on the device (a product with the rounded reciprocal - for 126 of the 256 byte values not the
 *   correctly rounded quotient that uda_normalize_tf stores).
 *   No allocations, no workspace, no atomics; integers up to that last conversion: bit-identical from run to run, an image's output the
 *   same alone and inside any batch.  A null pointer, B or S out of range returns the error before the launch and writes nothing.
 * uda_photo_reduce_u8: the coarse canvas.  f = max(1, ceil(max(H, W) / S)), h = ceil(H / f), w = ceil(W / f); canvas pixel (r, c), r < h,
 *   c < w, is per channel (sum + cnt / 2) / cnt in integers over rows [r f, min(H, (r + 1) f)) x columns [c f, min(W, (c + 1) f)), cnt the
 *   pixels of that block; the rest of the S x S canvas is 0.  -> canvas_u8 uint8 [B,S,S,3], canvas_f32 f32 [B,3,S,S] (normalised as
 *   above: -1 where the canvas is 0), either may be null, not both; factor int32 [B] = f.  Every byte is written exactly once.  No
 *   photograph: an all-zero canvas and factor 0.
 * uda_roi_cut_u8: boxes int32 [B,3] = (x0, y0, R), the R x R window with top-left (x0, y0) in photograph coordinates, any part of which
 *   may lie outside the photograph and reads as 0; 8 <= R <= 2.5 S (at most 5 taps per axis, as uda_geometry_u8).  -> roi_u8 uint8
 *   [B,S,S,3] = byte for byte Pillow's im.crop((x0, y0, x0 + R, y0 + R)).resize((S, S), Image.BILINEAR) (the 8-bit triangle filter with
 *   its 22-bit integer weights, horizontal pass, then vertical pass over its uint8 result, R = S a plain copy), roi_f32 f32 [B,3,S,S]
 *   normalised as above; either may be null, not both.  Only the rows and columns the window needs are read (to 16-byte words).  The
 *   boxes are device memory and are not checked by the entry: no photograph, an R outside 8..2.5 S or |x0|, |y0| > 2^20 give an
 *   all-zero ROI (callers with the boxes on the host check them there).
 * uda_roi_paste_u8: masks uint8 [B,2,S,S] (cup, disc; nonzero = set; never written), boxes as above, sizes int32 [B,2] = (H, W) of THIS
 *   batch's photographs, out_offsets int64 [B]: first byte of each photograph's [H,W] grey mask in out (out_bytes bytes in all).  BEAL
 *   coding, that of utils.Utils.save_mask_batch: 0 = cup (also where the disc is not set), 128 = disc only, 255 = background; a pixel
 *   outside the window is 255.  Window pixel (i, j), 0 <= i, j < R, takes each plane's bilinear upsample (half-pixel centres, edge clamp)
 *   of the 0/1 mask, exactly: per axis with D = 2 R, a = clamp((2 i + 1) S - R, 0, (S - 1) D), i0 = a / D, fa = a - i0 D, i1 = min(i0 + 1,
 *   S - 1), weights (D - fa, fa); v = sum over the 2 x 2 neighbours of m wy wx <= D^2 < 2^25; the plane is set iff 2 v > D^2 (a tie is
 *   not set).  Every byte of each [H,W] mask is written exactly once and nothing else; a row of sizes / out_offsets that does not lie
 *   inside out writes nothing; a box that uda_roi_cut_u8 would not take gives an all-255 mask. */
int uda_photo_reduce_u8(const uint8_t* pool, int64_t pool_pixels, const int64_t* offsets, const int* sizes, int n_sources,
                        const int64_t* src_index, int B, int S, uint8_t* canvas_u8, float* canvas_f32, int* factor, void* stream);
int uda_roi_cut_u8(const uint8_t* pool, int64_t pool_pixels, const int64_t* offsets, const int* sizes, int n_sources,
                   const int64_t* src_index, const int* boxes, int B, int S, uint8_t* roi_u8, float* roi_f32, void* stream);
int uda_roi_paste_u8(const uint8_t* masks, const int* boxes, const int* sizes, const int64_t* out_offsets, int B, int S, uint8_t* out,
                     int64_t out_bytes, void* stream);

/* Trainer_prototype_full.py:335-355, 378-398 (EMA of the eight centroids, gradient through the current term only) + :428-444
 * (intra = sum_k MSE(src_k, tgt_k), inter = MSE(src_1, src_3) + MSE(src_0, src_2)) on two [4][C] centroid matrices in one
 * launch: new = prev ? keep * prev + decay * cur : cur (keep = 1 - decay as the caller's double expression rounds it);
 * losses2 = (intra, inter).  prev_* may be null (first use).
 * uda_proto_align_bwd: d intra / d cur_src = g * w_src * 2 (new_src - new_tgt) / C, d cur_tgt = -g * w_tgt * (...). */
int uda_proto_align_fwd(const float* cur_src, const float* cur_tgt, const float* prev_src, const float* prev_tgt, float keep,
                        float decay, int C, float* new_src, float* new_tgt, float* losses2, void* stream);
int uda_proto_align_bwd(const float* new_src, const float* new_tgt, const float* g_intra, float w_src, float w_tgt, int C,
                        float* d_cur_src, float* d_cur_tgt, void* stream);
/* Trainer_prototype_full.py:456-458, 479-513: scale * (BCEWithLogitsLoss(d1, label) + BCEWithLogitsLoss(d2, label)) on the two
 * patch-discriminator outputs (n1, n2 elements), forward in one launch, both gradients in one launch (g: device scalar). */
int uda_adv_loss_fwd(const float* d1, int n1, const float* d2, int n2, float label, float scale, float* loss, void* stream);
int uda_adv_loss_bwd(const float* d1, int n1, const float* d2, int n2, float label, float scale, const float* g, float* g1,
                     float* g2, void* stream);
/* Trainer_prototype_full.py:452-454: the first discriminator layer fed by generator LOGITS (NCHW): z = s2d(pre(x)),
 * pre_op 1 = sigmoid(x) (boundary branch), 2 = -sigmoid(x) * log(sigmoid(x) + 1e-7) (uncertainty map); the adjoint routes
 * dz back to the logits and multiplies by pre'(x).  No full-resolution intermediate map is materialised. */
int uda_adv_s2d_fwd(const float* logits_nchw, int N, int C, int H, int W, int pre_op, float* z, int64_t ld_z, int Hz, int Wz,
                    void* stream);
int uda_adv_s2d_bwd(const float* dz, int64_t ld_z, int Hz, int Wz, const float* logits_nchw, int N, int C, int H, int W,
                    int pre_op, float* d_logits_nchw, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UDA_CLR_HIP_H */
