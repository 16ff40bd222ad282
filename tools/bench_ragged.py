#!/usr/bin/env python3
"""step_ragged against what a ragged collection cost before it: the same queries padded to the batch's longest slate with -1 labels
through FusedRanker.step.  One process; the two variants alternate inside it, block by block; device events around every block.

  config A  2 000 queries per step, F = 136, lengths from a SYNTHETIC long-tailed distribution: log-normal (sigma 0.9) with mean 120,
            rounded and clipped to 1 .. 1251, numpy PCG64 seed 20.  It has the shape of a web-search collection's documents per
            query; it is not the histogram of MSLR-WEB30K or of any other real collection.
            approxNDCG and lambdaLoss (ndcgLoss2PP_scheme) on DoubleLayerNet and on the folded make_model ranker; ListNet is timed
            ragged-only (a padded document changes its softmaxes: there is no padded equivalent).
  config B  2 000 queries of exactly 100 documents: step_ragged vs step on the same data (the cost of the index indirection).

One JSON line per configuration is appended to --out: lengths summary, n_docs, padded n_docs, ms per step of each variant (median
over the blocks, min / max next to it) and the work ratios the time ratio is to be read against (padded docs / real docs for the
scorer, sum S_max^2 / sum S_q^2 for the pair loss).

  python tools/bench_ragged.py [--steps 200] [--blocks 4] [--out profiles/r11_ragged.jsonl] [--only A|B]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))


def lengths_a(n=2000, seed=20, mean=120.0, sigma=0.9, hi=1251):
    rng = np.random.default_rng(seed)
    v = rng.lognormal(np.log(mean) - 0.5 * sigma * sigma, sigma, size=n)
    return np.clip(np.rint(v), 1, hi).astype(np.int64)


def make_net(kind, dev):
    torch.manual_seed(0)
    if kind == "double":
        from architeture.doubleLayer import DoubleLayerNet
        return DoubleLayerNet(136).to(dev).eval()
    from architeture.multiLayer import make_model
    return make_model(dict(sizes=[128, 256, 128], input_norm=False, activation=None, dropout=0.0), False,
                      dict(output_activation="Sigmoid", d_output=1), 136).to(dev).eval()


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def run(name, kind, loss, sizes, dev, steps, blocks, padded=True):
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.scorer import FusedRanker
    extra = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else {}
    net = make_net(kind, dev)
    ranker = FusedRanker(net, loss=loss, **extra)
    Q, n, smax = len(sizes), int(sizes.sum()), int(sizes.max())
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, 136, generator=g).to(dev)
    y = torch.randint(0, 5, (n,), generator=g).float().to(dev)
    slates = RaggedSlates(np.concatenate(([0], np.cumsum(sizes))), device=dev)
    variants = {"ragged": lambda: ranker.step_ragged(X, y, slates)}
    if padded:
        rows = torch.as_tensor(np.repeat(np.arange(Q) * smax, sizes) + np.arange(n) - np.repeat(slates.offsets_host[:-1], sizes), device=dev)
        Xp = torch.zeros(Q * smax, 136, device=dev)
        yp = torch.full((Q * smax,), -1.0, device=dev)
        Xp[rows] = X
        yp[rows] = y
        Xp, yp = Xp.view(Q, smax, 136), yp.view(Q, smax)
        variants["padded"] = lambda: ranker.step(Xp, yp)
    per = max(1, steps // blocks)
    for fn in variants.values():                       # warm every shape that is timed
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            ms[k].append(timed(fn, per))
    out = {"config": name, "net": kind, "loss": loss, "queries": Q, "n_docs": n, "padded_n_docs": Q * smax,
           "lengths": {"min": int(sizes.min()), "median": float(np.median(sizes)), "mean": float(sizes.mean()), "max": smax,
                       "synthetic": True},
           "tier_launches": len(slates.tiers()), "steps_per_variant": per * blocks, "blocks": blocks,
           "work_ratio_docs": Q * smax / n, "work_ratio_pairs": Q * float(smax) ** 2 / float((sizes.astype(np.float64) ** 2).sum())}
    for k, v in ms.items():
        out[f"{k}_ms_per_step"] = float(np.median(v))
        out[f"{k}_ms_min_max"] = [float(min(v)), float(max(v))]
    if padded:
        out["time_ratio_padded_over_ragged"] = out["padded_ms_per_step"] / out["ragged_ms_per_step"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_ragged.jsonl"))
    ap.add_argument("--only", choices=["A", "B"])
    ap.add_argument("--ragged-only", action="store_true", help="config A without the padded variant (kernel-trace runs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []
    if a.only in (None, "A"):
        sizes = lengths_a()
        for kind in ("double", "make_model"):
            for loss in ("approxNDCG", "lambdaLoss"):
                lines.append(run("A", kind, loss, sizes, dev, a.steps, a.blocks, padded=not a.ragged_only))
            lines.append(run("A", kind, "listnet", sizes, dev, a.steps, a.blocks, padded=False))
    if a.only in (None, "B"):
        sizes = np.full(2000, 100, dtype=np.int64)
        for kind in ("double", "make_model"):
            for loss in ("approxNDCG", "lambdaLoss"):
                lines.append(run("B", kind, loss, sizes, dev, a.steps, a.blocks))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for l in lines:
            print(json.dumps(l), flush=True)
            f.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
