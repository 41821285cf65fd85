#!/usr/bin/env python
"""Dev tool: DeepLab(backbone='drn') on one MI355X (bench.py's --backbone choices are fixed).

    python tests/bench_drn.py [--steps 10 --warmup 3 --batch 8 --size 512] [--out profiles/drn_bench.jsonl]
    python tests/bench_drn.py --kernels [--out profiles/drn_head_kernels]        head-kernel table (.jsonl + .md)

Workloads: ``source_only`` (Trainer_baseline's step, B images) and ``prototype_full`` (Trainer_prototype_full.train_step,
B source + B target images), both on bench.py's synthetic batches, timed between device synchronisations after warm-up.

``--kernels`` times every kernel of uda_clr_amd/csrc/drn_head.hip at the DRN head's 512^2 shapes, B = 8 and 16, against the
route the library had for the same shape before them, in one process: the implicit-GEMM entries uda_conv_fwd /
uda_conv_wgrad at stride 1 (the stride-2 convs: stride 1 + uda_rows_stride + uda_colstats forward, the weight gradient on the
zero-stuffed gradient).  The 7x7 stride-1 stem had no earlier route and is reported alone.  Warm-up, then ``reps`` launches
between two HIP events; GB/s from ALGORITHMIC bytes (every operand and result once), TF from 2 * 9 * Cin * Cout * Pout.
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
    model = DeepLab(num_classes=2, backbone="drn", method=name).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.99))
    img, tmap, tbd = synth_batch(B, S, 1337, dev)
    imgT = synth_batch(B, S, 4242, dev)[0]
    out = os.path.join("/tmp", "uda_bench_drn_%d" % os.getpid())
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
    return {"metric": "drn_%s_img_per_s" % name, "workload": name, "backbone": "drn", "output_stride": 8,
            "batch": B, "size": S, "images_per_step": per_step, "steps": steps, "warmup": warmup,
            "img_per_s": round(per_step / dt, 2), "ms_per_step": round(1e3 * dt, 2),
            "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2), "loss": loss,
            "device": torch.cuda.get_device_name(dev)}


# (layer, Cin, Cout, stride, input side at 512^2): the narrow 3x3 convs of the head and of layer3; "dgrad" runs Cout -> Cin at stride 1 on the
# input grid (the zero-stuffed gradient for the stride-2 layers)
HEAD_CONVS = [("layer1.0", 16, 16, 1, 512), ("layer2.0", 16, 32, 2, 512), ("layer3.0.conv2", 64, 64, 2, 256),
              ("layer3.1.conv2", 64, 64, 1, 128)]      # (layer3.1 / layer3.2: the same 64 -> 64 width at stride 1, 1/4 resolution)


def _time(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernels(batches, dev, reps, out):
    from uda_clr_amd.acts import ACT_RELU, Act
    from uda_clr_amd.kernels import HipKernels
    K = HipKernels()
    rows = []

    def add(B, layer, op, route, us, nbytes, flops, note=""):
        rows.append({"B": B, "layer": layer, "op": op, "route": route, "us": round(us, 1), "GB_per_s": round(nbytes / us / 1e3, 1),
                     "TF": round(flops / us / 1e6, 2), "note": note})
        print(json.dumps(rows[-1]), flush=True)

    for B in batches:
        S = 512
        P = B * S * S
        x = torch.randn(B, 3, S, S, device=dev)
        w7 = torch.randn(16, 3, 7, 7, device=dev) / 12.0
        y = torch.empty(P, 16, device=dev)
        st = torch.zeros(16, 2, 16, dtype=torch.float64, device=dev)
        dy = torch.randn(P, 16, device=dev)
        dw7 = torch.empty_like(w7)
        w7h = K.relayout_hwio(w7)
        fl = 2.0 * 147 * 16 * P
        add(B, "layer0.0", "fwd", "stem7s1 (new; no earlier route)", _time(lambda: K.stem7s1_fwd(x, w7h, y, st), reps), 4.0 * P * (3 + 16), fl)
        add(B, "layer0.0", "wgrad", "stem7s1 (new; no earlier route)", _time(lambda: K.stem7s1_wgrad(x, dy, dw7), reps), 4.0 * P * (3 + 16), fl)
        del x, y, dy
        for layer, ci, co, s, side in HEAD_CONVS:
            H = side
            Ho = (H - 1) // s + 1
            Pi, Po = B * H * H, B * Ho * Ho
            xin = torch.randn(Pi, ci, device=dev)
            sc, sh = torch.rand(ci, device=dev) + 0.5, 0.3 * torch.randn(ci, device=dev)
            src = Act(xin, B, H, H, sc, sh, ACT_RELU)
            w = torch.randn(co, ci, 3, 3, device=dev) / (3.0 * ci ** 0.5)
            w_hwio, w_hwio_d = K.relayout_hwio(w), K.relayout_hwio(w, True)
            w_ohwi, w_dg = K.relayout_ohwi(w), K.relayout_dgrad(w)
            yo = torch.empty(Po, co, device=dev)
            yfull = torch.empty(Pi, co, device=dev)
            st = torch.zeros(16, 2, co, dtype=torch.float64, device=dev)
            g = torch.randn(Po, co, device=dev)
            gfull = torch.zeros(Pi, co, device=dev)
            if s != 1:
                K.rows_stride(g, B, H, H, s, gfull, scatter=True)
            else:
                gfull.copy_(g)
            gsrc = Act(gfull, B, H, H)
            dx = torch.empty(Pi, ci, device=dev)
            dw = torch.empty_like(w)
            fl = 2.0 * 9 * ci * co * Po
            by = 4.0 * (Pi * ci + Po * co)
            # ---- forward
            add(B, layer, "fwd", "conv3n (new)", _time(lambda: K.conv3n_fwd(src, w_hwio, s, yo, st), reps), by, fl)
            if s == 1:
                add(B, layer, "fwd", "uda_conv_fwd", _time(lambda: K.conv(src, w_ohwi, 3, 1, yo, stats=st), reps), by, fl)
            else:
                def old_fwd():
                    K.conv(src, w_ohwi, 3, 1, yfull)
                    K.rows_stride(yfull, B, H, H, s, yo)
                    K.colstats(yo, st)
                add(B, layer, "fwd", "uda_conv_fwd stride 1 + rows_stride + colstats", _time(old_fwd, reps), by, fl)
            # ---- weight gradient
            add(B, layer, "wgrad", "conv3n (new)", _time(lambda: K.conv3n_wgrad(src, g, s, dw), reps), by, fl)
            add(B, layer, "wgrad", "uda_conv_wgrad" + (" on the zero-stuffed gradient" if s != 1 else ""),
                _time(lambda: K.conv_wgrad(src, gfull, 3, 1, dw), reps), by, fl,
                "" if s == 1 else "zero stuffing (uda_rows_stride) not included: the input gradient needs it on either route")
            # ---- input gradient: stride-1 conv Cout -> Cin of the (zero-stuffed) gradient
            byd = 4.0 * (Po * co + Pi * ci)
            add(B, layer, "dgrad", "conv3n stride 1 (new)", _time(lambda: K.conv3n_fwd(gsrc, w_hwio_d, 1, dx), reps), byd, fl)
            add(B, layer, "dgrad", "uda_conv_fwd", _time(lambda: K.conv(gsrc, w_dg, 3, 1, dx), reps), byd, fl)
            del xin, yo, yfull, g, gfull, dx
            torch.cuda.empty_cache()
    if out:
        with open(out + ".jsonl", "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
        with open(out + ".md", "w") as f:
            f.write("# DRN-D-54 head kernels at 512^2 on MI355X (%s)\n\n" % torch.cuda.get_device_properties(dev).gcnArchName)
            f.write("Written by `python tests/bench_drn.py --kernels`: one process, 5 warm-up launches, %d timed launches between two HIP\n"
                    "events per row.  GB/s from algorithmic bytes (operand and result once), TF from 2 * taps * Cin * Cout * Pout (the\n"
                    "strided output grid: the older stride-2 routes compute four times that).  `dgrad` is the stride-1 conv Cout -> Cin of\n"
                    "the gradient on the input grid (zero-stuffed for the stride-2 layers).\n\n" % reps)
            f.write("| B | layer | op | route | us | GB/s | TF | new / old |\n|---|---|---|---|---|---|---|---|\n")
            for i, r in enumerate(rows):
                ratio = ""
                if "(new)" in r["route"] and i + 1 < len(rows) and rows[i + 1]["op"] == r["op"] and rows[i + 1]["layer"] == r["layer"]:
                    ratio = "%.2f" % (r["us"] / rows[i + 1]["us"])
                f.write("| %d | %s | %s | %s | %.1f | %.1f | %.2f | %s |\n" % (r["B"], r["layer"], r["op"], r["route"], r["us"],
                                                                             r["GB_per_s"], r["TF"], ratio))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--workload", choices=("source_only", "prototype_full", "both"), default="both")
    ap.add_argument("--kernels", action="store_true", help="the head-kernel table instead of the workloads")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="", help="workloads: a .jsonl file to append to; --kernels: path stem of the .jsonl / .md table")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from uda_clr_amd.kernels import load_library
    load_library()
    if args.kernels:
        kernels((8, 16), dev, args.reps, args.out)
        return
    names = ("source_only", "prototype_full") if args.workload == "both" else (args.workload,)
    for name in names:
        row = json.dumps(workload(name, args.batch, args.size, args.steps, args.warmup, dev))
        print(row, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(row + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
