#!/usr/bin/env python3
"""WideFusedRanker.step against the only other way to train a scorer wider than 136 features: the module path
(net(X, None, None) -> loss -> backward(): library GEMMs and ATen autograd, scorer.wide_forward).  One process; the two variants
alternate inside it, block by block, after a warm-up; device events around every block of steps.

  DoubleLayerNet and TripleLayerNet at F = 220 (Istella) and F = 700 (Yahoo LTRC), approxNDCG, 2 000 queries x slate 100, train mode;
  one ragged line at F = 220 (the same 200 000 documents as queries of unequal length, WideFusedRanker.step_ragged alone).

One JSON line per shape is appended to --out: ms per step of each variant (median over the blocks, min / max next to it), the
algorithmic FLOPs and bytes of one step computed from the shapes, and the share of the fp32-MFMA peak (157.3 TFLOP/s) and of the
HBM peak (8 TB/s) the chain's time amounts to -- the larger share names the bound.

  python tools/bench_wide.py [--seconds 1.0] [--blocks 5] [--out profiles/wide_scorers.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))

PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12


def make_net(kind, F, dev):
    torch.manual_seed(0)
    if kind == "double":
        from architeture.doubleLayer import DoubleLayerNet
        return DoubleLayerNet(F).to(dev).train()
    from architeture.tripleLayer import TripleLayerNet
    return TripleLayerNet(F).to(dev).train()


def work(kind, F, n):
    """(FLOPs, bytes) of one chain step over n documents, from the shapes: 2 n K N per GEMM (forward, dh, dW); every activation,
    gradient and operand tensor counted once per launch that reads or writes it (fp32), the weights once per GEMM."""
    if kind == "double":
        H = F
        flops = 2 * n * (F * H + H * H + H) + 2 * n * (H * H) + 2 * n * (H * H + H * F) + 4 * n * H
        # fc1 X, h1 | fc2 h1, h2 | scores h2 | dw3 h2 | dz2 h2, dz2 | dW2 dz2, h1 | db2 dz2 | dz1 dz2, h1, dz1 | dW1 dz1, X | db1 dz1
        byts = 4 * (2 * n * F + 15 * n * H + 2 * H * F + 3 * H * H)
        return flops, byts
    H = 32
    flops = 2 * n * (F * H + H) + 2 * n * H * F + 4 * n * H
    # fc1 X, h | scores h | dw3 h | dz1 h, dz1 | dW1 dz1, X | db1 dz1
    byts = 4 * (2 * n * F + 7 * n * H + 2 * H * F)
    return flops, byts


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))


def run(kind, F, dev, seconds, blocks, ragged=False):
    from losses.approxNDCG import approxNDCGLoss
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.wide import WideFusedRanker
    Q, S = 2000, 100
    n = Q * S
    net = make_net(kind, F, dev)
    ranker = WideFusedRanker(net, loss="approxNDCG")
    g = torch.Generator().manual_seed(1)
    X = torch.randn(Q, S, F, generator=g).to(dev)
    y = torch.randint(0, 5, (Q, S), generator=g).float().to(dev)
    if ragged:
        rng = np.random.default_rng(20)
        cuts = np.sort(rng.choice(np.arange(1, n), size=Q - 1, replace=False))
        bounds = np.concatenate(([0], cuts, [n]))
        while (np.diff(bounds) > 2048).any():               # re-draw the rare query past the slate limit
            cuts = np.sort(rng.choice(np.arange(1, n), size=Q - 1, replace=False))
            bounds = np.concatenate(([0], cuts, [n]))
        slates = RaggedSlates(bounds, device=dev)
        X2, y2 = X.view(n, F), y.view(n)
        variants = {"wide_step_ragged": lambda: ranker.step_ragged(X2, y2, slates)}
    else:
        def module_path():
            for p in net.parameters():
                p.grad = None
            approxNDCGLoss(net(X, None, None).squeeze(-1), y).backward()
        variants = {"wide_step": lambda: ranker.step(X, y), "module_path": module_path}
    steps = {}
    for name, fn in variants.items():                       # warm-up, then size a block to seconds / blocks
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        steps[name] = max(2, int(seconds / blocks / (timed(fn, 3) * 1e-3)))
    times = {name: [] for name in variants}
    for _ in range(blocks):
        for name, fn in variants.items():
            times[name].append(timed(fn, steps[name]))
    flops, byts = work(kind, F, n)
    first = next(iter(variants))
    t = float(np.median(times[first])) * 1e-3
    line = dict(net=kind, F=F, queries=Q, n_docs=n, slate=None if ragged else S, loss="approxNDCG", train=True, ragged=ragged,
                steps_per_block=steps, blocks=blocks, chain_flops=flops, chain_bytes=byts,
                share_of_fp32_mfma_peak=flops / t / PEAK_FLOPS, share_of_hbm_peak=byts / t / PEAK_BYTES)
    line["bound_by"] = "fp32 MFMA" if line["share_of_fp32_mfma_peak"] > line["share_of_hbm_peak"] else "HBM"
    for name, v in times.items():
        line[name] = stats(v)
    if "module_path" in times:
        line["module_over_wide"] = line["module_path"]["median_ms"] / line["wide_step"]["median_ms"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wide_scorers.jsonl"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = [("double", 220, False), ("triple", 220, False), ("double", 700, False), ("triple", 700, False), ("double", 220, True)]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for kind, F, ragged in shapes:
            line = run(kind, F, dev, a.seconds, a.blocks, ragged)
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
