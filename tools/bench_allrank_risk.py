#!/usr/bin/env python3
"""Risk-sensitive losses on the FC-only make_model ranker (config.json "model": FC F -> 128 -> 256 -> 128 -> 1, Identity activations):
the module step the reference trains with (`model(X, None, None)` -> riskLoss(scores, y, y_base) -> backward,
main_batch_execution.py:93-94, :128-170) against the folded FusedRanker step (ltr_mi355x/linear.py) with y_base and with the cached
baseline columns, for geoRiskLambdaLoss and tRiskListnetLoss at three shapes:
  web10k : F = 136, S = 128, B = 2 000        td2003 : F = 64, S = 1 000, B = 256        driver : F = 136, S = 100, B = 100
and, where the one-pass kernels apply (Listnet forms, S in {32, 64, 128}), the multi-launch chain forced through the same ranker.
tRisk takes the mean of the three baselines, as the reference driver does.  Eval mode; no optimizer step in any timing.

Every path is warmed at its shape first.  Then `--rounds` rounds; in each round every path in turn runs one window of `--steps` steps
between two device events after a synchronise (so the paths alternate and share whatever else the host is doing).  Reported per path:
the median window (ms per step) and the spread of the windows, (max - min) / median.  `fused_slower_than_module_beyond_spread` is the
gate: median fused > median module x (1 + module spread).

One JSON line per (loss, shape) to profiles/r10_allrank_risk.jsonl (or --out).
    python tools/bench_allrank_risk.py [--steps 20] [--warmup 5] [--rounds 7] [--shapes web10k,td2003,driver] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
SHAPES = {"web10k": dict(F=136, S=128, B=2000), "td2003": dict(F=64, S=1000, B=256), "driver": dict(F=136, S=100, B=100)}
NB = 3


# kernel launches per step of each timed path, read off ltr_mi355x/linear.py (not counted in a trace): fold 1, tail 1, unfold 3 in all;
# one-pass: + risk_rows + risk_combine; chain: + scores + matrix + scores_grad + grad_partials.  With y_base a Listnet form adds
# baseline_columns' one launch, a Lambda form runs the uncached matrix as two launches (all systems' column sums, then the rows).


def launches(path, one_pass):
    n = 7 if (one_pass and path != "chain_base_cols") else 9
    return n + 1 if path == "fused_y_base" else n


def _window(fn, steps):
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", default="web10k,td2003,driver")
    ap.add_argument("--losses", default="geoRiskLambdaLoss,tRiskListnetLoss")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_allrank_risk.jsonl"))
    a = ap.parse_args()
    from architeture.multiLayer import make_model
    from losses.riskLosses import riskLosses as RL
    from ltr_mi355x.scorer import FusedRanker
    if not torch.cuda.is_available():
        raise SystemExit("bench_allrank_risk.py measures on the GPU; none found")
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
            net = make_model(dict(sizes=[128, 256, 128], input_norm=False, activation=None, dropout=0.0), False,
                             dict(output_activation="Sigmoid", d_output=1), F).to(dev).eval()
            yb = yb3.mean(dim=2) if name.startswith("tRisk") else yb3
            fn = getattr(RL, name)

            def module_step():
                net.zero_grad(set_to_none=True)
                fn(net(X, None, None).squeeze(-1), y, yb).backward()

            ranker = FusedRanker(net, loss=name)
            cols = ranker.baseline_columns(y, yb)
            paths = {"module": module_step, "fused_y_base": lambda: ranker.step(X, y, y_base=yb),
                     "fused_base_cols": lambda: ranker.step(X, y, base_cols=cols)}
            one_pass = "Lambda" not in name and S in (32, 64, 128)
            if one_pass:
                paths["chain_base_cols"] = lambda: ranker.step(X, y, base_cols=cols, _one_pass=False)
            for f in paths.values():
                for _ in range(a.warmup):
                    f()
            torch.cuda.synchronize()
            wins = {k: [] for k in paths}
            for _ in range(a.rounds):
                for k, f in paths.items():
                    wins[k].append(_window(f, a.steps))
            med = {k: statistics.median(v) for k, v in wins.items()}
            spread = {k: (max(v) - min(v)) / med[k] for k, v in wins.items()}
            for _ in range(a.warmup):
                ranker.baseline_columns(y, yb)
            w_cols = [_window(lambda: ranker.baseline_columns(y, yb), max(1, a.steps // 10)) for _ in range(a.rounds)]
            t_cols = statistics.median(w_cols)
            row = {"loss": name, "shape": shape, "B": B, "S": S, "F": F, "n_base": NB if not name.startswith("tRisk") else 1,
                   "steps": a.steps, "rounds": a.rounds, "path": "one_pass" if one_pass else "chain",
                   "launches_fused_y_base": launches("fused_y_base", one_pass),
                   "launches_fused_base_cols": launches("fused_base_cols", one_pass),
                   "module_ms": round(med["module"], 4), "module_spread": round(spread["module"], 4),
                   "fused_y_base_ms": round(med["fused_y_base"], 4), "fused_y_base_spread": round(spread["fused_y_base"], 4),
                   "fused_base_cols_ms": round(med["fused_base_cols"], 4), "fused_base_cols_spread": round(spread["fused_base_cols"], 4),
                   "baseline_columns_once_ms": round(t_cols, 4), "baseline_columns_once_spread": round((max(w_cols) - min(w_cols)) / t_cols, 4),
                   "speedup_y_base_vs_module": round(med["module"] / med["fused_y_base"], 3),
                   "speedup_base_cols_vs_module": round(med["module"] / med["fused_base_cols"], 3),
                   "fused_slower_than_module_beyond_spread": bool(max(med["fused_y_base"], med["fused_base_cols"])
                                                                  > med["module"] * (1.0 + spread["module"])),
                   "device": torch.cuda.get_device_name(dev)}
            if one_pass:
                row.update({"chain_base_cols_ms": round(med["chain_base_cols"], 4), "chain_base_cols_spread": round(spread["chain_base_cols"], 4),
                            "launches_chain_base_cols": launches("chain_base_cols", one_pass),
                            "speedup_one_pass_vs_chain": round(med["chain_base_cols"] / med["fused_base_cols"], 3)})
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
