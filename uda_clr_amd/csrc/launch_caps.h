// Workgroup caps of the grid-stride launches, as plain numbers so that tests/test_capped_cases_cpu.py can read them.
//
// These launches take grid = min(ceil(work / 256), CAP) workgroups of 256 threads and walk the remainder with
//     for (e = blockIdx.x * 256 + threadIdx.x; e < work; e += gridDim.x * 256)
// so a kernel case runs the loop body a second time only when work > CAP * 256.  The "capped" cases of tests/kernel_cases.py derive
// that condition from the numbers below: a changed cap fails the CPU check instead of turning a two-pass case into a one-pass one.
// Host only; no kernel reads these.  Caps that belong to a launch plan stay with their plan, as plain numbers too: DW_DGRAD_MAX_WG
// (dw_plan.h), UPCONV_STRIP_MAX_WG / UPCONV_FLAT_MAX_WG (upconv_plan.h), H7W_MAX_WG / N3_MAX_WG_SMALL / N3_MAX_WG_LARGE (drn_head.hip).
#pragma once

#define RESAMPLE_MAX_WG 16384        /* upsample_fwd / upsample_bwd / head_upsample_fwd / head_upsample_bwd / broadcast_rows / dropout_mask */
#define UPSAMPLE_STATS_MAX_WG 4096   /* upsample_fwd_kernel<true, true>: one LDS reduction + 2C fp64 atomics per workgroup */
#define S2D_MAX_WG 16384             /* s2d_fwd / s2d_fwd4 / s2d_bwd / s2d_bwd4, their gate and adversarial-input forms */
#define RELAYOUT_S2D_MAX_WG 8192     /* relayout_s2d */
#define RELAYOUT_MAX_WG 4096         /* relayout_ohwi / relayout_dgrad (grid_for) */
#define WGRAD_REDUCE_MAX_WG 4096     /* wgrad_reduce_kernel<8 | 64> */
