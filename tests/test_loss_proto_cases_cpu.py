"""not-gpu: the edge cases of the loss / metric / prototype kernels (kernel_cases.LOSS_PROTO_EDGE_CASES and the two older cases
their rules rewrote) can pass and can fail.

  * With SpecKernels standing in for HipKernels every case passes on the CPU: its input conditions hold (no undecided logit in
    the counts, at most 0.5 % undecided pixels in the retrified weights, every class with weight) and the fp32 statement meets
    the float64 one within the case's tolerance.
  * Five planted wrong implementations (SpecKernels subclasses) each fail exactly the cases listed with them and no other.
  * The LDS plan of the prototype reduce (csrc/proto_plan.h) holds every index the kernel forms, for every C the entry accepts."""
import os
import re

import pytest
import torch

import kernel_cases as kc
from kernel_spec import SpecKernels

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BY_NAME = dict(kc.CASES)
NAMES = [c[0] for c in kc.LOSS_PROTO_EDGE_CASES] + list(kc.LOSS_PROTO_CHANGED)


def _fails(name, impl, monkeypatch):
    monkeypatch.setattr(kc, "_HIP", impl)
    err, tol = _BY_NAME[name](CPU)
    assert kc.footprint_violations() == []
    return not err <= tol


def test_the_minimum_set_is_there():
    assert len(NAMES) == len(set(NAMES)) == 37 and all(n in _BY_NAME for n in NAMES)
    widths = sorted(int(re.search(r"C=(\d+)", n).group(1)) for n in NAMES if n.startswith("proto edge"))
    assert widths == [1, 4, 7, 12, 60, 61, 305, 305, 1024]
    assert kc.TAIL_P > 8192 * 4                       # uda_proto_bwd's grid cap x waves per workgroup: the loop takes a second step


@pytest.mark.parametrize("name", NAMES)
def test_spec_kernels_pass_the_case_on_the_cpu(name, monkeypatch):
    assert not _fails(name, kc.SPEC, monkeypatch)
    assert len(kc._FRAMES) > 0


# ---- planted faults
class CountLanesFrom16Dropped(SpecKernels):
    """weight totals that leave out pixel lanes 16.. of a workgroup (what a count region of 4 x 16 floats can hold)"""
    def proto_reduce(self, feat, wts, sums):
        P, C = feat.shape
        PP = 256 // ((C + 3) // 4)
        lane = (torch.arange(P) % (PP * 32)) % PP            # pixel p of a workgroup's PP * 32: step p // PP, lane p % PP
        super().proto_reduce(feat, wts, sums)
        sums[:, C] -= (wts.double() * (lane >= 16).double().unsqueeze(1)).sum(0).to(sums.device)


class ThresholdOff(SpecKernels):
    def seg_counts(self, logits, target, thr):
        return super().seg_counts(logits, target, thr + 1e-3)


class NearestSwapped(SpecKernels):
    """nearest index with the scales H / w and W / h"""
    def proto_weights(self, mode, B, h, w, map_=None, **kw):
        if mode != 0:
            return super().proto_weights(mode, B, h, w, map_=map_, **kw)
        H, W = map_.shape[2:]
        ih = (torch.arange(h).float() * (float(H) / w)).floor().long().clamp(max=H - 1)
        iw = (torch.arange(w).float() * (float(W) / h)).floor().long().clamp(max=W - 1)
        m = map_[:, :, ih][:, :, :, iw]
        a, b = m[:, 0], m[:, 1]
        return torch.stack([t.reshape(-1) for t in (a, b, 1 - a, 1 - b)], 1).contiguous(), None, None


class BackwardStopsAtTheGrid(SpecKernels):
    """proto_bwd that never takes the grid-stride step: pixels from 8192 x 4 on are left as they were"""
    def proto_bwd(self, feat, wts, sums, dC, d_feat=None, accumulate=False, want_dw=False):
        n = min(feat.shape[0], 32768)
        dw = super().proto_bwd(feat[:n], wts[:n], sums, dC, None if d_feat is None else d_feat[:n], accumulate, want_dw)
        if dw is not None:
            dw = torch.cat([dw, torch.zeros(feat.shape[0] - n, 4)])
        return dw


class AdamWithoutBc2(SpecKernels):
    def adam_step(self, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
        exp_avg.lerp_(grads, 1 - beta1)
        exp_avg_sq.mul_(beta2).addcmul_(grads, grads, value=1 - beta2)
        params.addcdiv_(exp_avg, exp_avg_sq.sqrt() + eps, value=-lr / (1 - beta1 ** step))


FAULTS = {
    "count lanes from 16 on dropped": (CountLanesFrom16Dropped, lambda n: n.startswith("proto edge") and int(re.search(r"PP=(\d+)", n).group(1)) > 16),
    "seg_counts threshold + 1e-3": (ThresholdOff, lambda n: n.startswith("seg counts")),
    "nearest index with h and w swapped": (NearestSwapped, lambda n: n in ("proto weights hard 50x37 -> 13x9", "proto weights hard 7x5 -> 7x5")),
    "proto_bwd without the grid-stride step": (BackwardStopsAtTheGrid, lambda n: n.startswith("proto edge P=%d" % kc.TAIL_P)),
    "adam without bc2": (AdamWithoutBc2, lambda n: n.startswith("adam n=")),
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_a_planted_fault_fails_its_cases_and_no_other(fault, monkeypatch):
    impl, mine = FAULTS[fault]
    expected = [n for n in NAMES if mine(n)]
    assert expected
    assert [n for n in NAMES if _fails(n, impl(), monkeypatch)] == expected


# ---- the LDS plan of proto_reduce_kernel
def _plan():
    txt = open(os.path.join(ROOT, "uda_clr_amd", "csrc", "proto_plan.h")).read()
    return {k: int(v) for k, v in re.findall(r"^#define\s+(PR_\w+)\s+(\d+)\b", txt, flags=re.M)}


def _last_indices(C, threads, count_base):
    """the largest LDS index proto_reduce_kernel forms in each region for width C (losses_proto.hip: G channel groups x PP lanes)"""
    G = (C + 3) >> 2
    PP = threads // G
    Cp = 4 * G
    last_sum = max((k * PP + pl) * Cp + c0 + j for k in (0, 3) for pl in (0, PP - 1) for c0 in (0, Cp - 4) for j in (0, 3))
    last_cnt = count_base + 3 * PP + PP - 1
    return last_sum, last_cnt, PP


def test_every_lds_index_of_the_reduce_lies_inside_the_declared_array():
    plan = _plan()
    assert set(plan) == {"PR_THREADS", "PR_MAX_C", "PR_LDS_SUM_FLOATS", "PR_LDS_CNT_FLOATS"}, plan
    assert plan["PR_THREADS"] == 256 and plan["PR_MAX_C"] == 1024
    total = plan["PR_LDS_SUM_FLOATS"] + plan["PR_LDS_CNT_FLOATS"]
    assert total * 4 <= 64 * 1024
    for C in range(1, plan["PR_MAX_C"] + 1):
        last_sum, last_cnt, PP = _last_indices(C, plan["PR_THREADS"], plan["PR_LDS_SUM_FLOATS"])
        assert PP >= 1 and last_sum < plan["PR_LDS_SUM_FLOATS"] and last_cnt < total, (C, PP, last_sum, last_cnt)
    # the check can fail: with the 64 count floats the array used to have, exactly the widths 1 .. 60 run over
    assert [C for C in range(1, 1025) if _last_indices(C, 256, 4096)[1] >= 4096 + 64] == list(range(1, 61))
    # and the kernel and its entry use the plan's names, not numbers of their own
    src = open(os.path.join(ROOT, "uda_clr_amd", "csrc", "losses_proto.hip")).read()
    assert "__shared__ float red[PR_LDS_SUM_FLOATS + PR_LDS_CNT_FLOATS];" in src and "PP = PR_THREADS / G" in src
    assert src.count("red[PR_LDS_SUM_FLOATS + k * PP + ") == 2 and "red[4 * 1024" not in src and "C <= PR_MAX_C" in src
