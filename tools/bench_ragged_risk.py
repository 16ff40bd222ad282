#!/usr/bin/env python3
"""The risk-sensitive losses on ragged batches: FusedRanker.step_ragged(..., y_base= / base_cols=) timed on one device, one process;
variants alternate block by block inside it, device events around every block.

  config B  equal lengths, step_ragged against step of the same build (the cost of the offset / query-list indirection and of the
            per-tier launches): 256 queries x 1000 documents x 64 features with three baselines (TD2003's shape; DoubleLayerNet(64)
            only: the compiled make_model comparison network has 136 inputs) and 2000 x 128 x 136 on both rankers.  The folded
            make_model ranker's `step` runs its launch chain here (_one_pass=False), the route step_ragged takes.
  config A  2 000 queries per step, F = 136, three baselines, lengths from tools/bench_ragged.py's SYNTHETIC log-normal distribution
            (seed 20) clipped to >= 2: ms per step of the six losses on both rankers, with y_base and with base_cols.  There is no
            padded competitor: the reference soft-maxes labels and scores over the whole row, so a padded document changes every
            probability -- a padded run would time a different loss.

One JSON line per (config, ranker, loss) is appended to --out: ms per step of each variant (median over the blocks, min / max).

  python tools/bench_ragged_risk.py [--steps 40] [--blocks 4] [--out profiles/r12_ragged_risk.jsonl] [--only A|B] [--losses a,b]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LOSSES = ["geoRiskListnetLoss", "geoRiskLambdaLoss", "zRiskListnetLoss", "zRiskLambdaLoss", "tRiskListnetLoss", "tRiskLambdaLoss"]
NB = 3


def make_net(kind, F, dev):
    torch.manual_seed(0)
    if kind == "double":
        from architeture.doubleLayer import DoubleLayerNet
        return DoubleLayerNet(F).to(dev).eval()
    from architeture.multiLayer import make_model
    return make_model(dict(sizes=[128, 256, 128], input_norm=False, activation=None, dropout=0.0), False,
                      dict(output_activation="Sigmoid", d_output=1), F).to(dev).eval()


def run(config, kind, loss, sizes, F, dev, steps, blocks, rect):
    from bench_ragged import timed
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.scorer import FusedRanker
    ranker = FusedRanker(make_net(kind, F, dev), loss=loss)
    Q, n = len(sizes), int(sizes.sum())
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, F, generator=g).to(dev)
    y = torch.randint(0, 5, (n,), generator=g).float().to(dev)
    yb = (torch.randn(n, NB, generator=g) * 2.0).to(dev)
    if loss.startswith("tRisk"):
        yb = yb.mean(dim=1)
    slates = RaggedSlates(np.concatenate(([0], np.cumsum(sizes))), device=dev)
    cols = ranker.baseline_columns_ragged(y, yb, slates)
    variants = {"ragged_y_base": lambda: ranker.step_ragged(X, y, slates, y_base=yb),
                "ragged_base_cols": lambda: ranker.step_ragged(X, y, slates, base_cols=cols)}
    if rect:
        S = int(sizes[0])
        kw = dict(_one_pass=False) if kind == "make_model" else {}
        Xr, yr, ybr = X.view(Q, S, F), y.view(Q, S), yb.view(Q, S, -1) if yb.dim() == 2 else yb.view(Q, S)
        rcols = ranker.baseline_columns(yr, ybr)
        variants["step_y_base"] = lambda: ranker.step(Xr, yr, y_base=ybr, **kw)
        variants["step_base_cols"] = lambda: ranker.step(Xr, yr, base_cols=rcols, **kw)
    per = max(1, steps // blocks)
    for fn in variants.values():                       # warm every shape that is timed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k].append(timed(fn, per))
    out = {"config": config, "net": kind, "loss": loss, "queries": Q, "n_docs": n, "features": F, "baselines": NB,
           "lengths": {"min": int(sizes.min()), "median": float(np.median(sizes)), "mean": float(sizes.mean()), "max": int(sizes.max()),
                       "synthetic": True},
           "tier_launches": len(slates.tiers()), "steps_per_variant": per * blocks, "blocks": blocks}
    for k, v in ms.items():
        out[f"{k}_ms_per_step"] = float(np.median(v))
        out[f"{k}_ms_min_max"] = [float(min(v)), float(max(v))]
    if rect:
        out["ratio_ragged_over_step_y_base"] = out["ragged_y_base_ms_per_step"] / out["step_y_base_ms_per_step"]
        out["ratio_ragged_over_step_base_cols"] = out["ragged_base_cols_ms_per_step"] / out["step_base_cols_ms_per_step"]
    return out


def main():
    from bench_ragged import lengths_a
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_ragged_risk.jsonl"))
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--losses", default=",".join(LOSSES))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    losses = [l for l in a.losses.split(",") if l]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)

    def emit(line):
        print(json.dumps(line), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    if a.only in (None, "B"):
        for loss in losses:
            emit(run("B-256x1000x64", "double", loss, np.full(256, 1000, dtype=np.int64), 64, dev, a.steps, a.blocks, True))
            for kind in ("double", "make_model"):
                emit(run("B-2000x128x136", kind, loss, np.full(2000, 128, dtype=np.int64), 136, dev, a.steps, a.blocks, True))
    if a.only in (None, "A"):
        sizes = np.maximum(lengths_a(), 2)
        for kind in ("double", "make_model"):
            for loss in losses:
                emit(run("A", kind, loss, sizes, 136, dev, a.steps, a.blocks, False))


if __name__ == "__main__":
    main()
