#!/usr/bin/env python3
"""ltr_slates_build against the row gather the package already had, in one process.

  batch      10 000 queries, F = 136, lengths from the SYNTHETIC long-tailed distribution of tools/bench_ragged.py config A (log-normal,
             sigma 0.9, mean 120, clipped to 1 .. 1251, numpy PCG64 seed 20): the shape of a web-search collection's documents per
             query, not the histogram of any real one.
  build      ltr_slates_build, to_slates' launch: S = 128, mode sample -- the selection (key ranking for every query longer than S),
             X_out, y_out, mask and rows in one launch, a new seed every call.  build_first: the same with mode first (no ranking).
  yardstick  ltr_gather_rows_f32 moving the same number of 136-float rows (n_queries * S) out of the same X: the build's own row map,
             its padding slots pointed at real rows so that every row is read and written.

The C entry points are called directly into preallocated outputs and alternate, one call each per repetition, device events around
every call; the medians and the rows/s ratio build / yardstick go to --out as one JSON line.  Bytes: the yardstick reads and writes
n_queries * S rows; the build reads only the real rows (and their labels) and writes n_queries * S rows plus labels, mask and row map.

  python tools/bench_slates.py [--reps 30] [--warmup 5] [--out profiles/slates_build.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))


def main():
    from bench_ragged import lengths_a
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--slate", type=int, default=128)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slates_build.jsonl"))
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps must be at least 20")
    from ltr_mi355x import lib
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.slates import to_slates
    dev = torch.device("cuda:0")
    F, S, Q = 136, a.slate, a.queries
    sizes = lengths_a(n=Q)
    n = int(sizes.sum())
    slates = RaggedSlates(np.concatenate(([0], np.cumsum(sizes))), device=dev)
    g = torch.Generator().manual_seed(1)
    X = torch.randn(n, F, generator=g).to(dev)
    y = torch.randint(0, 5, (n,), generator=g).float().to(dev)
    X3, y2, fixed = to_slates(X, y, slates, S, mode="sample", seed=0)       # the outputs every timed call writes again
    idx = fixed.rows.reshape(-1).clone()
    idx = torch.where(idx < 0, torch.arange(Q * S, device=dev) % n, idx)
    out = torch.empty(Q * S, F, device=dev)
    h, st = lib(), torch.cuda.current_stream().cuda_stream
    epoch = [0]

    def build(mode):
        epoch[0] += 1
        rc = h.ltr_slates_build(X.data_ptr(), y.data_ptr(), slates.offsets.data_ptr(), None, Q, S, F, mode, epoch[0], -1.0, X3.data_ptr(),
                                y2.data_ptr(), fixed.mask.data_ptr(), fixed.rows.data_ptr(), st)
        assert rc == 0, rc

    def gather():
        rc = h.ltr_gather_rows_f32(X.data_ptr(), n, idx.data_ptr(), Q * S, F, out.data_ptr(), st)
        assert rc == 0, rc

    # build_first: the same launch without the key ranking (mode first), to read the ranking's share from
    variants = {"build": lambda: build(1), "gather_rows": gather, "build_first": lambda: build(0)}
    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    kept = int(fixed.kept.sum())
    row_b = 4 * F
    line = {"bench": "slates_build", "queries": Q, "S": S, "F": F, "mode": "sample", "n_docs": n, "rows_moved": Q * S, "real_rows": kept,
            "sampled_queries": int((sizes > S).sum()),
            "lengths": {"min": int(sizes.min()), "median": float(np.median(sizes)), "mean": float(sizes.mean()), "max": int(sizes.max()),
                        "synthetic": True},
            "reps": a.reps, "warmup": a.warmup, "timing": "device events around each C-ABI call, outputs preallocated"}
    for k, v in ms.items():
        med = float(np.median(v))
        line[f"{k}_ms"] = med
        line[f"{k}_ms_min_max"] = [float(min(v)), float(max(v))]
        line[f"{k}_rows_per_s"] = Q * S / (med * 1e-3)
    line["build_bytes"] = kept * (row_b + 4) + Q * S * (row_b + 4 + 1 + 8)
    line["gather_rows_bytes"] = Q * S * (2 * row_b + 8)
    line["build_GBps"] = line["build_bytes"] / (line["build_ms"] * 1e-3) / 1e9
    line["gather_rows_GBps"] = line["gather_rows_bytes"] / (line["gather_rows_ms"] * 1e-3) / 1e9
    line["ratio_build_over_gather_rows_per_s"] = line["build_rows_per_s"] / line["gather_rows_rows_per_s"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(line) + "\n")
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
