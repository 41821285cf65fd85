// LDS plan of proto_reduce_kernel (losses_proto.hip), as plain numbers so that tests/test_loss_proto_cases_cpu.py can read them.
// One workgroup of PR_THREADS threads splits into G = ceil(C / 4) channel groups x PP = PR_THREADS / G pixel lanes and stages,
// for the four classes k,
//   the channel sums  at red[(k * PP + pl) * 4G + c],                   c < 4G, pl < PP : 4 * PP * 4G floats from red[0]
//   the weight totals at red[PR_LDS_SUM_FLOATS + k * PP + pl],          pl < PP         : 4 * PP floats behind them.
// PP * G <= PR_THREADS, so the first region needs at most 16 * PR_THREADS = 4096 floats for every C; the second needs 4 * PP,
// which is largest at C <= 4 (G = 1, PP = PR_THREADS): 1024 floats.  20 KiB in all.
#pragma once

#define PR_THREADS 256
#define PR_MAX_C 1024            /* widest feature uda_proto_reduce accepts (G <= PR_THREADS) */
#define PR_LDS_SUM_FLOATS 4096
#define PR_LDS_CNT_FLOATS 1024

constexpr bool pr_lds_plan_fits() {
    for (int C = 1; C <= PR_MAX_C; ++C) {
        const int G = (C + 3) >> 2, PP = PR_THREADS / G;
        if (PP < 1 || 4 * PP * 4 * G > PR_LDS_SUM_FLOATS || 4 * PP > PR_LDS_CNT_FLOATS) return false;
    }
    return true;
}
static_assert(pr_lds_plan_fits(), "proto_reduce_kernel: an LDS region is too small for some C in [1, PR_MAX_C]");
