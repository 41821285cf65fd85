#!/usr/bin/env python
"""Dev tool: DeepLab(backbone='xception') throughput on one MI355X (bench.py's --backbone choices are fixed).

    python tests/bench_xception.py [--steps 10 --warmup 3 --batch 16 --size 512]     one JSON line per workload
    python tests/bench_xception.py --kernels                                           depthwise kernel table

Workloads: ``source_only`` (Trainer_baseline's step, B images) and ``prototype_full`` (Trainer_prototype_full.train_step,
B source + B target images), both on bench.py's synthetic batches, timed between device synchronisations after warm-up.
``--kernels`` times the depthwise entry points at Xception's 512^2 / B = 16 shapes with the kernel family the library's
launch plan chooses (family "") and pinned to the channel-blocked one (family "cb"), and reports achieved bytes/s from ALGORITHMIC bytes (input + output once).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(name, B, S, steps, warmup, dev):
    from bench import synth_batch
    from uda_clr_amd.networks.GAN import BoundaryDiscriminator, UncertaintyDiscriminator
    from uda_clr_amd.networks.deeplabv3 import DeepLab
    from uda_clr_amd.train_process import Trainer_baseline, Trainer_prototype_full
    torch.manual_seed(1337)
    model = DeepLab(num_classes=2, backbone="xception", output_stride=16, method=name).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.99))
    img, tmap, tbd = synth_batch(B, S, 1337, dev)
    imgT = synth_batch(B, S, 4242, dev)[0]
    out = os.path.join("/tmp", "uda_bench_xception_%d" % os.getpid())
    if name == "source_only":
        tr = Trainer_baseline.Trainer(cuda=True, model_gen=model, optimizer_gen=opt, val_loader=[], domain_loaderS=[],
                                      domain_loaderT=[], out=out, max_epoch=1, batch_size=B, warmup_epoch=-1)

        def step():
            opt.zero_grad(set_to_none=True)
            oS, bS = model(img)[:2]
            loss = tr.ops.seg_loss(oS, bS, tmap, tbd)
            loss.backward()
            opt.step()
            return loss
        per_step = B
    else:
        d1, d2 = BoundaryDiscriminator().to(dev).train(), UncertaintyDiscriminator().to(dev).train()
        od = torch.optim.SGD(d1.parameters(), lr=2.5e-5, momentum=0.99, weight_decay=5e-4)
        od2 = torch.optim.SGD(d2.parameters(), lr=2.5e-5, momentum=0.99, weight_decay=5e-4)
        tr = Trainer_prototype_full.Trainer(
            cuda=True, model_gen=model, model_dis=d1, model_uncertainty_dis=d2, optimizer_gen=opt, optimizer_dis=od,
            optimizer_uncertainty_dis=od2, val_loader=[], domain_loaderS=[], domain_loaderT=[], out=out, max_epoch=1,
            use_global=True, use_pid=True, retrify_pesudo=True, global_pro_weight=0.9, pro_weight=0.1, batch_size=B,
            warmup_epoch=-1)
        tr.epoch = 0
        sampleS, sampleT = {"image": img, "map": tmap, "boundary": tbd}, {"image": imgT}

        def step():
            return tr.train_step(sampleS, sampleT)
        per_step = 2 * B
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    for _ in range(steps):
        last = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    loss = float(last.item()) if torch.is_tensor(last) else float(last[0])
    return {"metric": "xception_%s_img_per_s" % name, "workload": name, "backbone": "xception", "output_stride": 16,
            "batch": B, "size": S, "images_per_step": per_step, "steps": steps, "warmup": warmup,
            "img_per_s": round(per_step / dt, 2), "ms_per_step": round(1e3 * dt, 2),
            "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2), "loss": loss,
            "device": torch.cuda.get_device_name(dev)}


# (C, output map, stride, dilation, calls per forward) of Xception at 512^2: OS16, then the OS8 middle / exit flow
KERNEL_SHAPES = [(728, 32, 1, 1, 50), (728, 32, 2, 1, 1), (1024, 32, 1, 1, 1), (1024, 32, 1, 2, 1), (1536, 32, 1, 2, 2),
                 (728, 64, 1, 2, 50), (1024, 64, 1, 4, 1), (1536, 64, 1, 4, 2)]


def kernels(B, dev, reps=20):
    from uda_clr_amd.acts import ACT_RELU, Act
    from uda_clr_amd.kernels import HipKernels
    K = HipKernels()
    rows = []
    for C, Ho, stride, dil, count in KERNEL_SHAPES:
        H = Ho * stride
        P, Po = B * H * H, B * Ho * Ho
        x = torch.randn(P, C, device=dev)
        sc, sh = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
        src = Act(x, B, H, H, sc, sh, ACT_RELU)
        w9 = torch.randn(9, C, device=dev)
        y = torch.empty(Po, C, device=dev)
        dy = torch.randn(Po, C, device=dev)
        dx = torch.empty(P, C, device=dev)
        dw = torch.empty(C, 1, 3, 3, device=dev)
        st = torch.zeros(16, 2, C, dtype=torch.float64, device=dev)
        for fam in ("", "cb"):
            if fam == "" and C > 1024:
                continue                          # the routed entry IS the channel-blocked kernel there
            ops = {"fwd": (lambda: K.dwconv_fwd(src, w9, stride, dil, 0, y, st, family=fam), 4 * (P + Po) * C),
                   "dgrad": (lambda: K.dwconv_dgrad(dy, w9, stride, dil, B, H, H, dx, family=fam), 4 * (P + Po) * C),
                   "wgrad": (lambda: K.dwconv_wgrad(src, dy, stride, dil, 0, dw, family=fam), 4 * (P + Po) * C)}
            for op, (fn, nbytes) in ops.items():
                for _ in range(3):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us = 1e3 * e0.elapsed_time(e1) / reps
                rows.append({"C": C, "map": Ho, "stride": stride, "dil": dil, "calls": count, "op": op,
                             "family": fam or "routed", "us": round(us, 1), "TB_per_s": round(nbytes / us / 1e6, 2)})
                print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--workload", choices=("source_only", "prototype_full", "both"), default="both")
    ap.add_argument("--kernels", action="store_true", help="the depthwise kernel table instead of the workloads")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from uda_clr_amd.kernels import load_library
    load_library()
    if args.kernels:
        kernels(args.batch, dev)
        return
    names = ("source_only", "prototype_full") if args.workload == "both" else (args.workload,)
    for name in names:
        print(json.dumps(workload(name, args.batch, args.size, args.steps, args.warmup, dev)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
