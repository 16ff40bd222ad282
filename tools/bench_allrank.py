#!/usr/bin/env python3
"""FC-only make_model ranker (config.json "model": 136 -> 128 -> 256 -> 128 -> 1, Identity activations): the folded FusedRanker step
(csrc/ltr_linear.hip) against the module step the reference trains with (`net(X, None, None)` -> loss -> backward -> Adam,
main_batch_execution.py:128-170), for approxNDCG, ListNet and lambdaLoss ndcgLoss2PP_scheme.

Per (loss, B, S) one JSON line to profiles/r06_allrank_fc.jsonl (or --out): slates/s of both steps (Adam included), the time between
the fused step's kernel events (the one-launch kernel, or scores + loss + gradient partials), and the fraction of the HBM roofline
from the algorithmic bytes B S (F + 1) 4 (X and the labels, read once) at --hbm-tbs.  Kernel times of a separate
`rocprofv3 --kernel-trace --stats` run are the per-kernel record.
    python tools/bench_allrank.py [--steps 20] [--warmup 5] [--shapes 25000x128,100000x32,100x100,100x1000]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
MODEL = {"fc_model": {"sizes": [128, 256, 128], "input_norm": False, "activation": None, "dropout": 0.0}, "transformer": False,
         "post_model": {"output_activation": "Sigmoid", "d_output": 1}}
F = 136


def _timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="25000x128,100000x32,100x100,100x1000")
    ap.add_argument("--losses", default="approxNDCG,listnet,lambdaLoss")
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak used for the roofline fraction (TB/s)")
    ap.add_argument("--no-module", action="store_true", help="fused step only (profiling runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_allrank_fc.jsonl"))
    a = ap.parse_args()
    import copy
    from architeture.multiLayer import make_model
    from losses.approxNDCG import approxNDCGLoss
    from losses.lambdaL import lambdaLoss
    from losses.listnet import listnetLoss
    from ltr_mi355x.scorer import FusedRanker
    dev = torch.device("cuda:0")
    module_loss = {"approxNDCG": lambda s, y: approxNDCGLoss(s, y), "listnet": lambda s, y: listnetLoss(y, s),
                   "lambdaLoss": lambda s, y: lambdaLoss(s, y, weighing_scheme="ndcgLoss2PP_scheme")}
    rows = []
    for shape in a.shapes.split(","):
        B, S = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(B, S, F, device=dev, generator=g)
        y = torch.randint(0, 5, (B, S), device=dev, generator=g).float()
        for loss in a.losses.split(","):
            torch.manual_seed(0)
            net = make_model(**copy.deepcopy(MODEL), n_features=F).to(dev)
            kw = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else {}
            r = FusedRanker(net, loss=loss, **kw)
            opt = torch.optim.Adam(net.parameters(), lr=1e-3)
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            r.kernel_events = ev

            def fused():
                r.step(X, y)
                opt.step()
            t_fused = _timed(fused, a.steps, a.warmup)
            kt = []
            for _ in range(3):
                fused()
                torch.cuda.synchronize()
                kt.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            t_kernel = min(kt)
            row = dict(loss=loss, B=B, S=S, F=F, one_launch=S in (32, 64, 128), fused_step_s=t_fused, fused_slates_per_s=B / t_fused,
                       fused_kernel_s=t_kernel, hbm_fraction=B * S * (F + 1) * 4 / t_kernel / (a.hbm_tbs * 1e12))
            if not a.no_module:
                r.kernel_events = None
                torch.manual_seed(0)
                net2 = make_model(**copy.deepcopy(MODEL), n_features=F).to(dev)
                opt2 = torch.optim.Adam(net2.parameters(), lr=1e-3)

                def module():
                    opt2.zero_grad()
                    module_loss[loss](net2(X, None, None), y).backward()
                    opt2.step()
                t_mod = _timed(module, a.steps, a.warmup)
                row.update(module_step_s=t_mod, module_slates_per_s=B / t_mod, speedup=t_mod / t_fused)
            row["time"] = time.strftime("%Y-%m-%dT%H:%M:%S")
            print(json.dumps(row), flush=True)
            rows.append(row)
            del r, net, opt
        del X, y
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
