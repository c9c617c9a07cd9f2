#!/usr/bin/env python3
"""flash_attn_prefill_func against what served a windowed prompt before it: the table of README.md and DESIGN.md 3.26 (profiles/prefill_window_bench.log).

  gpt-oss points   b 1, d 64, h 64 / h_k 8, bf16, causal, sinks, sq = sk in 2k / 8k / 32k, window (127, 0) and none: the yardstick is flash_attn_with_kvcache
                   with the same window and sinks (the 16-row decode kernels).
  unwindowed points  b 1, d 128, h 32 / h_k 8, bf16, causal, no window, no sinks, the same lengths: the yardstick is flash_attn_func.
Every call of a point is interleaved in one process, device events around windows of at least --window-ms of work each, the median of --rounds windows.  The
yardstick is timed twice ("yard" and "yard again"): the ratio of the two is the noise figure of the point.  Before timing, the two results are compared."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flash-attention-turing_amd"))
import flash_attn_turing as F  # noqa: E402


def gpt_oss(s, window):
    q = torch.randn(1, s, 64, 64, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(1, s, 8, 64, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    sinks = torch.randn(64, device="cuda")
    new = lambda: F.flash_attn_prefill_func(q, k, v, causal=True, window_size=window, sinks=sinks)
    yard = lambda: F.flash_attn_with_kvcache(q, k, v, causal=True, window_size=window, sinks=sinks)
    return new, yard


def unwindowed(s):
    q = torch.randn(1, s, 32, 128, device="cuda", dtype=torch.bfloat16)
    k, v = (torch.randn(1, s, 8, 128, device="cuda", dtype=torch.bfloat16) for _ in range(2))
    return (lambda: F.flash_attn_prefill_func(q, k, v, causal=True)), (lambda: F.flash_attn_func(q, k, v, causal=True))


def window(f, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--seqs", type=int, nargs="+", default=[2048, 8192, 32768])
    a = ap.parse_args()
    points = [(f"gpt-oss d64 h64/8 window {w}", s, lambda s=s, w=w: gpt_oss(s, w)) for w in ((127, 0), (-1, -1)) for s in a.seqs]
    points += [("d128 h32/8 no window vs flash_attn_func", s, lambda s=s: unwindowed(s)) for s in a.seqs]
    for name, s, make in points:
        new, yard = make()
        diff = (new().float() - yard().float()).abs().max().item()
        fns = {"new": new, "yard": yard, "yard again": yard}
        n = {k: max(3, math.ceil(a.window_ms / window(f, 3))) for k, f in fns.items()}      # (the first window is the warm-up)
        ms = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, f in fns.items():
                ms[k].append(window(f, n[k]))
        med = {k: statistics.median(x) for k, x in ms.items()}
        print(f"{name:42s} s={s:6d}  new {med['new']:9.4f} ms  yard {med['yard']:9.4f} ms  yard/new {med['yard'] / med['new']:6.2f}  "
              f"yard again/yard {med['yard again'] / med['yard']:.3f}  max|new - yard| {diff:.2e}  calls a window {n['new']} / {n['yard']}  "
              f"spread new {min(ms['new']):.4f}-{max(ms['new']):.4f} yard {min(ms['yard']):.4f}-{max(ms['yard']):.4f}", flush=True)


if __name__ == "__main__":
    main()
