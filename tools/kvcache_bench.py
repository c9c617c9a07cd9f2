#!/usr/bin/env python3
"""Decode over a KV cache: the split-KV path (flash_attn_with_kvcache) against the existing fwd path on the same data (equal lengths, no
append: fwd(q, k_cache[:, :L], v_cache[:, :L])), in process and interleaved (A, B, A, B ... rounds; medians).  One JSON line per grid point:
ms per call of both paths, the bytes the decode path moves (valid K/V prefix read once, q, out, lse, and the fp32 partials of a split launch:
written and read once), its effective TB/s, that as a fraction of 6.3 TB/s achievable and 8 TB/s peak HBM, the split count, the speedup.

Every point rotates over enough distinct caches that the working set exceeds 256 MiB, so that K/V come from HBM and not from the 256 MiB
Infinity Cache.  Usage: python tools/kvcache_bench.py [--quick] [--rounds N] [--paged P ...]

--paged P (repeatable) measures a paged cache instead: per grid point and page size P, the paged call (block_table over a pool whose pages
are assigned by a random permutation) against the contiguous call on the same data (the pool gathered into (b, L, h_k, d)), interleaved,
medians; ms and TB/s of both and paged / contiguous."""
import argparse
import itertools
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flash-attention-turing_amd"))
import flash_attn_turing as F  # noqa: E402
from flash_attn_turing import capi  # noqa: E402

HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12
WORKING_SET = 256 << 20


def grid(quick):
    bs, heads, ds, ls, sqs = (1, 8, 32), ((32, 32), (32, 8), (32, 1)), (64, 128), (4096, 32768, 131072), (1, 4)
    if quick:
        bs, ls = (1, 8), (32768,)
    for b, (h, hk), d, L, sq in itertools.product(bs, heads, ds, ls, sqs):
        for dt in ((torch.float16, torch.bfloat16) if d == 128 else (torch.float16,)):
            yield dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=dt)


def time_rotation(fn, n, rounds_iters):
    """ms per call of fn(i) over the rotation i = 0..n-1, repeated until a timed batch holds at least rounds_iters calls"""
    reps = max(1, math.ceil(rounds_iters / n))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        for i in range(n):
            fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / (reps * n)


def run_point(pt, rounds):
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    kv_bytes = 2 * b * L * hk * d * 2
    n = max(1, min(512, math.ceil(WORKING_SET / kv_bytes)))
    caches = []
    for _ in range(n):
        kc = torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2)
        vc = torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2)
        caches.append((kc, vc))
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    p = capi.kvcache_params(q, caches[0][0], caches[0][1], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs)
    ws = capi.kvcache_workspace_bytes(p)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws)))
    kv = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs)
    fw = lambda i: F.fwd(q, caches[i][0][:, :L], caches[i][1][:, :L], False)
    kv(0), fw(0)
    torch.cuda.synchronize()
    t_kv, t_fw = [], []
    for _ in range(rounds):
        t_kv.append(time_rotation(kv, n, 20))
        t_fw.append(time_rotation(fw, n, 20))
    ms_kv, ms_fw = statistics.median(t_kv), statistics.median(t_fw)
    rows = b * h * sq
    moved = kv_bytes + 2 * rows * d * 2 + rows * 4 + (2 * n_split * rows * (d + 1) * 4 if n_split > 1 else 0)
    tbps = moved / (ms_kv * 1e-3) / 1e12
    del caches
    torch.cuda.empty_cache()
    return dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), caches_rotated=n,
                ms_kvcache=round(ms_kv, 5), ms_fwd=round(ms_fw, 5), bytes=moved, tbps=round(tbps, 3),
                frac_of_6p3=round(tbps * 1e12 / HBM_ACHIEVABLE, 3), frac_of_8=round(tbps * 1e12 / HBM_PEAK, 3), n_split=n_split,
                speedup_vs_fwd=round(ms_fw / ms_kv, 2))


def run_paged_point(pt, page, rounds):
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    assert L % page == 0, (L, page)
    kv_bytes = 2 * b * L * hk * d * 2
    n = max(1, min(512, math.ceil(WORKING_SET / kv_bytes)))
    nb = b * (L // page)
    gen = torch.Generator(device="cpu").manual_seed(page)
    sets = []
    for _ in range(n):
        kp = torch.empty(nb, page, hk, d, device=dev, dtype=dt).uniform_(-2, 2)
        vp = torch.empty(nb, page, hk, d, device=dev, dtype=dt).uniform_(-2, 2)
        table = torch.randperm(nb, generator=gen).view(b, L // page).to(device=dev, dtype=torch.int32)
        idx = table.long()
        kc, vc = kp[idx].reshape(b, L, hk, d), vp[idx].reshape(b, L, hk, d)
        sets.append((kp, vp, table, kc, vc))
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    pg = lambda i: F.flash_attn_with_kvcache(q, sets[i][0], sets[i][1], cache_seqlens=cs, block_table=sets[i][2])
    ct = lambda i: F.flash_attn_with_kvcache(q, sets[i][3], sets[i][4], cache_seqlens=cs)
    assert torch.equal(pg(0), ct(0))
    torch.cuda.synchronize()
    t_pg, t_ct = [], []
    for _ in range(rounds):
        t_pg.append(time_rotation(pg, n, 20))
        t_ct.append(time_rotation(ct, n, 20))
    ms_pg, ms_ct = statistics.median(t_pg), statistics.median(t_ct)
    p = capi.kvcache_params(q, sets[0][3], sets[0][4], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs)
    ws = capi.kvcache_workspace_bytes(p)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws)))
    rows = b * h * sq
    moved = kv_bytes + 2 * rows * d * 2 + rows * 4 + (2 * n_split * rows * (d + 1) * 4 if n_split > 1 else 0)
    del sets
    torch.cuda.empty_cache()
    return dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), page_block_size=page, caches_rotated=n,
                ms_paged=round(ms_pg, 5), ms_contiguous=round(ms_ct, 5), bytes=moved, kv_gb=round(kv_bytes / 1e9, 3),
                tbps_paged=round(moved / (ms_pg * 1e-3) / 1e12, 3), tbps_contiguous=round(moved / (ms_ct * 1e-3) / 1e12, 3), n_split=n_split,
                paged_over_contiguous=round(ms_pg / ms_ct, 3))


def _with_ws(p, ws):
    buf = torch.empty(ws // 4, device="cuda:0", dtype=torch.float32)
    p.workspace, p.workspace_bytes = buf.data_ptr(), ws
    p._ws = buf
    return p


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--quick", action="store_true", help="b in {1, 8}, L = 32k only")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--paged", type=int, action="append", metavar="P", help="page size (a multiple of 16); repeat for several")
    a = ap.parse_args()
    print(json.dumps({"library": F.build_info(), "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count}),
          flush=True)
    with torch.no_grad():
        for pt in grid(a.quick):
            if a.paged:
                for page in a.paged:
                    print(json.dumps(run_paged_point(pt, page, a.rounds)), flush=True)
            else:
                print(json.dumps(run_point(pt, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
