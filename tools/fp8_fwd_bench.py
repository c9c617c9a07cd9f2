#!/usr/bin/env python3
"""flash_attn_fp8_func against flash_attn_func (fp16) at b 1, h 32, d 128, non-causal and causal, 2k / 4k / 16k: the table of README.md and DESIGN.md 3.25
(profiles/fp8_fwd_bench.log).

Default: both calls interleaved in one process, device events around windows of at least --window-ms of work each, the median of --rounds windows.
--once SEQ CAUSAL: a few calls of both at one shape and nothing else, the workload of a counter run (rocprofv3 --pmc ... -- python tools/fp8_fwd_bench.py
--once 16384 0; profiles/fp8_fwd_pmc.log)."""
import argparse
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "flash-attention-turing_amd"))
import flash_attn_turing as F  # noqa: E402

PEAK_FP8 = 5.0e15       # dense e4m3 MFMA peak of an MI355X, FLOP/s


def calls(s, causal):
    q16, k16, v16 = (torch.randn(1, s, 32, 128, device="cuda", dtype=torch.float16) for _ in range(3))
    q8, k8, v8 = (t.to(torch.float8_e4m3fn) for t in (q16, k16, v16))
    return {"fp16": lambda: F.flash_attn_func(q16, k16, v16, causal=causal), "fp8": lambda: F.flash_attn_fp8_func(q8, k8, v8, causal=causal)}


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--once", nargs=2, type=int, metavar=("SEQ", "CAUSAL"))
    a = ap.parse_args()
    if a.once:
        fns = calls(a.once[0], bool(a.once[1]))
        for _ in range(4):
            for f in fns.values():
                f()
        torch.cuda.synchronize()
        return
    for causal in (False, True):
        for s in (2048, 4096, 16384):
            fns = calls(s, causal)
            n = {k: max(20, math.ceil(a.window_ms / window(f, 20))) for k, f in fns.items()}      # (the first window is the warm-up)
            ms = {k: [] for k in fns}
            for _ in range(a.rounds):
                for k, f in fns.items():
                    ms[k].append(window(f, n[k]))
            flop = 4 * s * s * 128 * 32 * (0.5 if causal else 1.0)
            m16, m8 = statistics.median(ms["fp16"]), statistics.median(ms["fp8"])
            print(f"causal={int(causal)} s={s:6d}  fp16 {m16:8.4f} ms ({flop / m16 / 1e9:7.1f} TFLOP/s)  fp8 {m8:8.4f} ms ({flop / m8 / 1e9:7.1f} TFLOP/s, "
                  f"{flop / m8 * 1e3 / PEAK_FP8:.3f} of FP8 peak)  fp8/fp16 time {m8 / m16:.2f}  calls a window {n['fp16']} / {n['fp8']}  "
                  f"spread fp16 {min(ms['fp16']):.4f}-{max(ms['fp16']):.4f} fp8 {min(ms['fp8']):.4f}-{max(ms['fp8']):.4f}", flush=True)


if __name__ == "__main__":
    main()
