#!/usr/bin/env python3
"""Long-slate attention micro-benchmark: the attention core forward + backward at B = 16 slates, h = 8 heads, dk in {16, 17},
S in {512, 1024, 2048}, one JSON line per (leg, shape):

  tiled      ltr_enc_attention_fwd_tiled + ltr_enc_attention_bwd_tiled (csrc/ltr_attention_tiled.h), every S
  whole_row  ltr_enc_attention_fwd_lse + ltr_enc_attention_bwd_lse (the whole-row kernels), S = 512 only
  torch      the materialised formulation (bf16 matmul, fp32 softmax, bf16 matmul; autograd backward), as a yardstick

plus the config-5 network of tools/bench_encoder.py at S = 1024 (same tokens per step as its default 256 x 256) in a child process.
torch.cuda.Event timing on the current stream; dropout 0.1 on the kernel legs (the torch leg has none: it only bounds the cost of
the materialised scores)."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))

import torch  # noqa: E402


def timeit(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--no-network", action="store_true")
    a = ap.parse_args()
    from ltr_mi355x._lib import check, lib
    from ltr_mi355x.functional import _ptr, _stream
    dev = "cuda:0"
    L = lib()
    B, h, p = a.batch, a.heads, a.dropout
    for dk in (16, 17):
        for S in (512, 1024, 2048):
            d, T = h * dk, B * S
            torch.manual_seed(S + dk)
            qkv = (torch.randn(T, 3 * d, device=dev) * 1.5).to(torch.bfloat16)
            q16 = qkv.view(torch.int16)
            mask = torch.zeros(B, S, dtype=torch.uint8, device=dev)
            dctx = torch.randn(T, d, device=dev).to(torch.bfloat16).view(torch.int16)
            ctx = torch.empty(T, d, dtype=torch.int16, device=dev)
            lse = torch.empty(B * h, S, device=dev)
            dqkv = torch.empty(T, 3 * d, dtype=torch.int16, device=dev)
            legs = {"tiled": ("ltr_enc_attention_fwd_tiled", "ltr_enc_attention_bwd_tiled")}
            if S <= 512:
                legs["whole_row"] = ("ltr_enc_attention_fwd_lse", "ltr_enc_attention_bwd_lse")
            for leg, (fwd, bwd) in legs.items():
                f = lambda fwd=fwd: check(getattr(L, fwd)(_ptr(q16), _ptr(mask), B, S, h, dk, p, 5, 0, _ptr(ctx), _ptr(lse), _stream()), fwd)  # noqa: E731
                g = lambda bwd=bwd: check(getattr(L, bwd)(_ptr(q16), _ptr(ctx), _ptr(dctx), _ptr(lse), _ptr(mask), B, S, h, dk, p, 5, 0,  # noqa: E731
                                                          _ptr(dqkv), _stream()), bwd)
                t_f = timeit(f, a.iters, a.warmup)
                t_b = timeit(g, a.iters, a.warmup)
                emit(leg, B, S, h, dk, p, t_f, t_b)
            # torch's materialised formulation
            x = qkv.view(B, S, 3, h, dk).permute(2, 0, 3, 1, 4)
            qt, kt, vt = (x[j].contiguous().requires_grad_(True) for j in range(3))
            go = torch.randn(B, h, S, dk, device=dev).to(torch.bfloat16)
            state = {}

            def tf():
                sc = torch.matmul(qt, kt.transpose(-2, -1)).float() / math.sqrt(dk)
                sc = sc.masked_fill(mask.view(B, 1, 1, S) == 1, float("-inf"))
                state["o"] = torch.matmul(torch.softmax(sc, -1).to(torch.bfloat16), vt)

            def tb():
                torch.autograd.backward(state["o"], go)

            def tfb():
                tf()
                tb()
            t_f = timeit(tf, a.iters, a.warmup)
            t_fb = timeit(tfb, a.iters, a.warmup)
            emit("torch", B, S, h, dk, 0.0, t_f, t_fb - t_f)
            del qt, kt, vt, state
            torch.cuda.empty_cache()
    if not a.no_network:
        # config-5 network (tools/bench_encoder.py defaults: 6 layers, d 128, d_ff 2048, h 8, dropout 0.1) at S = 1024, 64 slates
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_encoder.py"), "--slate", "1024", "--batch", "64", "--steps", "5",
               "--warmup", "2"]
        out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout.strip().splitlines()[-1]
        rec = json.loads(out)
        rec["leg"] = "config5_network_S1024"
        print(json.dumps(rec), flush=True)


def emit(leg, B, S, h, dk, p, t_f, t_b):
    print(json.dumps({"leg": leg, "B": B, "S": S, "h": h, "dk": dk, "drop_p": p, "fwd_ms": round(t_f * 1e3, 4),
                      "bwd_ms": round(t_b * 1e3, 4), "fwd_bwd_ms": round((t_f + t_b) * 1e3, 4),
                      "us_per_slate": round((t_f + t_b) / B * 1e6, 3)}), flush=True)


if __name__ == "__main__":
    main()
