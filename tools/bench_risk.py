#!/usr/bin/env python3
"""Risk-sensitive losses: the module step the reference trains with (`net(X, None, None)` -> riskLoss(scores, y, y_base) -> backward,
main_batch_execution.py:128-170) against the fused FusedRanker step with y_base and with the cached baseline columns (base_cols,
FusedRanker.baseline_columns), for geoRiskLambdaLoss and tRiskListnetLoss at two shapes:
  td2003 : DoubleLayerNet(64), S = 1 000, 3 baselines, B = 256 (the TD2003 collection's baseline runs)
  web10k : DoubleLayerNet(136), S = 128, 3 baselines, B = 2 000
tRisk takes the mean of the baselines, as the reference driver does.  Eval mode (no dropout); no optimizer step in any of the timings.

One JSON line per (loss, shape) to profiles/r08_risk_fused.jsonl (or --out): ms per step of each path and the speed-ups.
    python tools/bench_risk.py [--steps 10] [--warmup 3] [--shapes td2003,web10k] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
SHAPES = {"td2003": dict(F=64, S=1000, B=256), "web10k": dict(F=136, S=128, B=2000)}
NB = 3


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
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="td2003,web10k")
    ap.add_argument("--losses", default="geoRiskLambdaLoss,tRiskListnetLoss")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_risk_fused.jsonl"))
    a = ap.parse_args()
    from architeture.doubleLayer import DoubleLayerNet
    from losses.riskLosses import riskLosses as RL
    from ltr_mi355x.scorer import FusedRanker
    dev = torch.device("cuda:0")
    rows = []
    for shape in a.shapes.split(","):
        F, S, B = SHAPES[shape]["F"], SHAPES[shape]["S"], SHAPES[shape]["B"]
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.randn(B, S, F, device=dev, generator=g)
        y = torch.randint(0, 5, (B, S), device=dev, generator=g).float()
        yb3 = torch.randn(B, S, NB, device=dev, generator=g)
        for name in a.losses.split(","):
            torch.manual_seed(1)
            net = DoubleLayerNet(F).to(dev).eval()
            yb = yb3.mean(dim=2) if name.startswith("tRisk") else yb3
            fn = getattr(RL, name)

            def module_step():
                net.zero_grad(set_to_none=True)
                fn(net(X, None, None).squeeze(-1), y, yb).backward()

            t_mod = _timed(module_step, a.steps, a.warmup)
            ranker = FusedRanker(net, loss=name)
            t_fused = _timed(lambda: ranker.step(X, y, y_base=yb), a.steps, a.warmup)
            torch.cuda.synchronize()
            cols = ranker.baseline_columns(y, yb)
            t_cols = _timed(lambda: ranker.baseline_columns(y, yb), 1, 0)
            t_cached = _timed(lambda: ranker.step(X, y, base_cols=cols), a.steps, a.warmup)
            row = {"loss": name, "shape": shape, "B": B, "S": S, "F": F, "n_base": NB if not name.startswith("tRisk") else 1,
                   "steps": a.steps, "module_ms": round(t_mod, 4), "fused_y_base_ms": round(t_fused, 4),
                   "fused_base_cols_ms": round(t_cached, 4), "baseline_columns_once_ms": round(t_cols, 4),
                   "speedup_fused_vs_module": round(t_mod / t_fused, 3), "speedup_base_cols_vs_module": round(t_mod / t_cached, 3),
                   "speedup_base_cols_vs_y_base": round(t_fused / t_cached, 3), "device": torch.cuda.get_device_name(dev)}
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
