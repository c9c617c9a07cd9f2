#!/usr/bin/env python3
"""Decode over a KV cache: the split-KV path (flash_attn_with_kvcache) against the existing fwd path on the same data (equal lengths, no
append: fwd(q, k_cache[:, :L], v_cache[:, :L])), in process and interleaved (A, B, A, B ... rounds; medians).  One JSON line per grid point:
ms per call of both paths, the bytes the decode path moves (valid K/V prefix read once, q, out, lse, and the fp32 partials of a split launch:
written and read once), its effective TB/s, that as a fraction of 6.3 TB/s achievable and 8 TB/s peak HBM, the split count, the speedup.

Every point rotates over enough distinct caches that the working set exceeds 256 MiB, so that K/V come from HBM and not from the 256 MiB
Infinity Cache.  Usage: python tools/kvcache_bench.py [--quick] [--rounds N] [--paged P ...]

--paged P (repeatable) measures a paged cache instead: per grid point and page size P, the paged call (block_table over a pool whose pages
are assigned by a random permutation) against the contiguous call on the same data (the pool gathered into (b, L, h_k, d)), interleaved,
medians; ms and TB/s of both and paged / contiguous.

--window LEFT (repeatable) measures a sliding window instead: per grid point, the windowed call (causal, window_size=(LEFT, 0)) against the
unwindowed causal call on the same caches and against the unwindowed causal call on caches of the window's length (LEFT + 1 rows),
interleaved, medians.  TB/s counts the bytes the window actually reads.  Caches rotate until the windows alone exceed 256 MiB.

--kv-dtype fp8 measures the 8-bit (torch.float8_e4m3fn) cache instead: per grid point, the 8-bit call with per-(batch, head) descales against
the 16-bit call on the same logical cache (the 8-bit codes widened, which is exact), interleaved, medians; ms of both, TB/s of each over the
bytes it really reads, the fraction of 6.3 TB/s, and the ratio.  Caches rotate until the 8-bit K/V alone exceed 256 MiB.

--rotary [DIM] measures the rotary embedding instead (DIM = rotary_dim, default head_dim; --rotary-neox for the non-interleaved pairing): per
grid point with seqlen_q = seqlen_new = 1, appending at the cache's last row, (A) the rotary call; (B) the plain call with append on
pre-rotated q / k - the same work minus the rotation, the floor - timed TWICE (B, B2), so that the spread of one thing measured twice in the
same run stands next to A / B; (C) what a caller does without the feature: torch ops on the GPU (cos / sin rows gathered by cache_seqlens on
the device, the rotation of q and k in fp32) followed by the plain call.  All four interleaved, medians.  A and C must agree bit for bit.

--ragged measures ragged query batches (cu_seqlens_q) instead, three families of points, one JSON line each (`ragged` names the family):
"uniform" - the ragged call with every sq_i = 1 against the dense call of the same shape (same bytes, same math), the dense call timed TWICE
so that the spread of one thing measured twice stands next to ragged / dense; 16-bit and FP8, contiguous and paged; outputs must agree bit for
bit.  "mixed" - one scheduler step (e.g. 60 x sq 1 + 3 x sq 4 + 1 x sq 256, lengths 1k-32k, paged) as ONE ragged call against what a caller
does without the feature: one dense call per distinct sq on gathered q rows / cache_seqlens / block_table rows (the gathers run on the device
and are counted; scattering the outputs back is not).  "chunk" - one sequence of sq = 128 / 512 / 2048 rows over 8k keys, causal, as a ragged
call against fwd on the same prefix: where the decode tiling (K / V re-read once per 16 packed rows) stops paying.  All arms interleaved,
medians.

--softcap CAP measures soft-capped scores instead (with --kv-dtype fp8 over the 8-bit cache; --softmax-scale S for a scale other than
1 / sqrt(d), which selects no other code): per grid point, the soft-capped call (A) against the same call without the cap (B), B timed TWICE
(B, B2) so that the spread of one thing measured twice in the same run stands next to A / B; interleaved, medians.  TB/s over the bytes
both read.

--sinks measures attention sinks instead, on a grid of its own - the gpt-oss shape: head_dim 64, 64 query heads over 8 KV heads, one query,
b in {1, 8, 64} x L in {4k, 32k, 128k}, each point as the 128-token sliding-window layer (causal, window (127, 0)) and as the full-causal
layer; with --kv-dtype fp8 over the 8-bit cache, with --paged P through a block table of P-row pages (the first P given).  Per point, the
sink call (A) against the same call without sinks (B), B timed TWICE (B, B2) so that the spread of one thing measured twice in the same run
stands next to A / B; interleaved, medians.  `hbm_bound` marks the points whose K/V read is at least 1 GB, `inside_scatter` whether A lies
between B and B2.  With --baseline-library PATH it becomes an A / B of the sink call itself through the C ABI of this build (A) and of the
library at PATH (B), e.g. tools/abl/libfa_sinkplain.so built with -DFA_KVC_SINK_PLAIN=1; A is timed twice; the outputs must agree bit for bit.

--tree N (N in 8, 32, 64) measures tree attention masks instead: per point of the grid, with seqlen_q = N in place of the grid's query counts,
(A) the tree call under the binary-heap tree (parent (t - 1) // 2; the words from tree_mask_from_parents) against (B) the causal=True call of
the same shape - the same steps over the same keys, a compare in place of the bit test - B timed TWICE (B, B2) so that the spread of one thing
measured twice in the same run stands next to A / B; interleaved, medians; with --kv-dtype fp8 over the 8-bit cache.  `hbm_bound` marks the
points whose K/V are at least 1 GB, `inside_scatter` whether A lies between B and B2.  With --baseline-library PATH it becomes an A / B of the
tree call itself through the C ABI of this build (A, timed twice) and of the library at PATH (B), e.g. tools/abl/libfa_treeuniform.so built with
-DFA_KVC_TREE_UNIFORM=1; the outputs must agree bit for bit.

--prefill measures the 64-row kernels for prompt chunks instead, on a grid of its own: one causal chunk of sq in {64, 128, 512, 2048} rows over
L in {8k, 32k} keys, h 32 / h_k 8, head_dim 128 and 64 (--head-dim / --length replace them), fp16; with --kv-dtype fp8 over the 8-bit cache, with
--paged P through a block table of P-row pages (repeatable: one line per page size).  Per point, (A) the prefill=True call against (B) the
prefill=False call on the same caches, B timed TWICE (B, B2) so that the spread of one thing measured twice in the same run stands next to
A / B; on the 16-bit contiguous points also (C) fwd on the same prefix.  All arms interleaved, medians; `max_abs_diff` is A against B.

--head-dim D (repeatable) replaces the grid's head dims (64, 128).  head_dim 256 exists for the decode call only: its points carry no fwd arm.
--equal-bytes (with --head-dim 256) measures the head_dim-256 call against its yardstick instead: per grid point with one query, (A) the
d-256 call; (B, B2) the d-128 call on the same b and L with twice the KV heads and twice the query heads - the same cache bytes (the very
same buffers, viewed as (b, L, 2 h_k, 128)), the same FLOPs, the same row-tile count - timed TWICE so that the scatter of one thing measured
twice in the same run stands next to A / B; interleaved, medians.  `hbm_bound` marks the points whose K/V are at least 1 GB.

--mla measures MLA decode over a latent KV cache (flash_mla_with_kvcache): h in {16, 128}, seqlen_q 1, b in {1, 8, 64}, L in {4k, 32k, 128k} (--length
replaces them), bf16, contiguous and, with --paged P, through a block table of P-row pages.  Per point, (A) the MLA call - time and
b * L * 1152 B / time as a fraction of 6.3 TB/s; (B, B2) the yardstick, the head_dim-256 flash_attn_with_kvcache call with h_k = 1 and the same h, b and L
(1024 B per key: nearly the same bytes, fewer FLOPs), timed TWICE so that the scatter of one thing measured twice in the same run stands next to
A / B; interleaved, medians.

--mla --kv-dtype fp8 / --mla-sparse --kv-dtype fp8 measure the two MLA calls over an FP8 latent cache (656-byte rows) on the same grids: per point the FP8
call against the same call over the dequantised bf16 cache (the two give the same bits: asserted), the bf16 call timed twice as its own noise figure;
interleaved in one process, medians (profiles/kvcache_mla_fp8_bench.log).
--mla-sparse measures sparse MLA decode (flash_mla_sparse_with_kvcache): bf16, seqlen_q 1, h in {16, 128}, b in {1, 8, 64}, topk 2048, pages of 64 (--paged P
replaces the page size).  The yardstick is the DENSE flash_mla_with_kvcache call at L = topk - the same rows, the same bytes - timed TWICE (B, B2: its own
noise figure).  Against it, interleaved in one process: (i) the identity list 0 .. topk - 1 on the same caches; and per L in {32k, 128k} (--length replaces
them) on one cache of that length, rotating over lists, (ii) 2048 random positions, sorted, (iii) the same positions unsorted.  At b in {1, 8} a second line
per point records arm (i) under forced num_splits 8, 16, 32, 64 next to the automatic count, timed twice (profiles/kvcache_mla_sparse_bench.log).

--mla-indexer-prefill measures flash_mla_indexer_prefill_logits on one prompt chunk (b 1, sq 128 / 512 / 2048 over 4k / 32k / 128k keys; bf16 q_idx, FP8 keys with
scales, 64 heads, pages of 64, causal) against flash_mla_indexer_logits on the same inputs, interleaved, the decode call timed twice, the bits asserted equal
first; ms, the ratio and sq x n x 64 x 128 x 2 FLOP over time under the mask, and the selection launch (profiles/mla_indexer_prefill_bench.log).
--mla-indexer / --mla-indexer-prefill with --q-dtype fp8 measure the same two calls on e4m3 index queries against the calls on the widened (bf16) queries over the
same caches, interleaved, the bf16-q call timed twice, the bits asserted on integer data first (profiles/mla_indexer_fp8q_bench.log).
--mla-indexer measures the DeepSeek-V3.2 indexer (flash_mla_indexer_logits / flash_mla_indexer_topk): bf16 q_idx, FP8 keys with per-token scales, 64 index
heads, seqlen_q 1, topk 2048, pages of 64 (--paged P replaces the page size), b in {1, 8, 64} x L in {4k, 32k, 128k} (--length replaces them).  Per point,
interleaved in one process: the logits call; the torch formulation of the logits (dequantise, einsum, relu, weighted sum, * k_scale; it reads the pool
as a contiguous cache, i.e. without the gather a paged cache would cost it) timed TWICE as its own noise figure; the selection; torch.topk on the same
logits.  The logits call is also stated against b * L * 132 B / time as a fraction of 6.3 TB/s.  Caches rotate over 256 MiB (profiles/kvcache_mla_indexer_bench.log).

--mla-prefill-bwd measures the MLA prefill backward (flash_mla_prefill_bwd) on the grid of --mla-prefill: both launches, the dQ launch and the dK/dV launch
alone, against (a) bwd at head_dim 128 on the same b, s, h (640 / 832 of the FLOPs per pair) and (b) autograd's backward of the torch formulation in bf16 where
its score matrices fit; each yardstick twice, interleaved in one process, medians; TFLOP/s at 2 sq sk h (3 x 192 + 2 x 128), halved under the mask
(profiles/mla_prefill_bwd_bench.log).
--mla-prefill measures MLA prefill attention (flash_mla_prefill_func: 192-wide q / k, 128-wide v) on a grid of its own: bf16, h = h_k in {16, 128}, b in
{1, 4}; sq = sk in {512, 2048, 8192} causal, and a 2048-row chunk over an 8k and a 32k context, non-causal (--quick: b 1, and h 128 up to 2048 rows only).  Per
point, interleaved in one process, medians: the new call against (a) fwd at head_dim 128 on the same b, s, h - 0.8 x the FLOPs - and (b) what a caller could
do before: flash_attn_with_kvcache at head_dim 256 on zero-padded q / k / v with the same softmax_scale; each yardstick is timed TWICE as its own noise
figure.  TFLOP/s of the new call at 2 sq sk h (192 + 128) per batch entry, halved under the mask, of fwd at its own 2 sq sk h (128 + 128)
(profiles/mla_prefill_bench.log).  With --baseline-library PATH (e.g. tools/abl/libfa_mlap_rows32.so built with -DFA_MLAP_WAVE_ROWS=32) the point becomes an
A / B of the new call itself through the C ABI of this build (A, timed twice) and of the library at PATH (B).

--merge measures flash_attn_merge_states alone: 2, 4, 8 contiguous bf16 parts of (rows, 4 heads, d_v 128 / 512), rows from 4k to 1M (points over 40 GiB are left out); bytes moved (the parts
read, one result written, out and lse) / time against 6.3 TB/s, next to the torch formulation of the same merge (logaddexp, exp, weighted sum; timed twice),
interleaved in one process, medians (profiles/merge_states_bench.log).
--shared-prefix measures flash_attn_with_shared_prefix (b 8 / 64, sq 1, h 32 / h_k 8, d 128, pages of 16, 16-bit and FP8 caches, a shared prefix of 2k / 8k /
32k keys and 128 own keys per sequence) against flash_attn_with_kvcache on the same tables (timed twice), interleaved, medians
(profiles/shared_prefix_bench.log).
--baseline-library PATH records an interleaved A/B of the plain (no window) call through the C ABI of this build and of the library at
PATH (e.g. a build of the parent commit), on the same data; the outputs must agree bit for bit.  --length L (repeatable) replaces the
grid's cache lengths."""
import argparse
import ctypes
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


def grid(quick, lengths=None, head_dims=None):
    bs, heads, ds, ls, sqs = (1, 8, 32), ((32, 32), (32, 8), (32, 1)), (64, 128), (4096, 32768, 131072), (1, 4)
    if quick:
        bs, ls = (1, 8), (32768,)
    if lengths:
        ls = tuple(lengths)
    if head_dims:
        ds = tuple(head_dims)
    for b, (h, hk), d, L, sq in itertools.product(bs, heads, ds, ls, sqs):
        for dt in ((torch.float16, torch.bfloat16) if d >= 128 else (torch.float16,)):
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
    has_fwd = d <= 128                                        # (head_dim 256: the decode call only)
    kv(0), has_fwd and fw(0)
    torch.cuda.synchronize()
    t_kv, t_fw = [], []
    for _ in range(rounds):
        t_kv.append(time_rotation(kv, n, 20))
        t_fw.append(time_rotation(fw, n, 20) if has_fwd else float("nan"))
    ms_kv, ms_fw = statistics.median(t_kv), statistics.median(t_fw)
    rows = b * h * sq
    moved = kv_bytes + 2 * rows * d * 2 + rows * 4 + (2 * n_split * rows * (d + 1) * 4 if n_split > 1 else 0)
    tbps = moved / (ms_kv * 1e-3) / 1e12
    del caches
    torch.cuda.empty_cache()
    return dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), caches_rotated=n,
                ms_kvcache=round(ms_kv, 5), ms_fwd=round(ms_fw, 5) if has_fwd else None, bytes=moved, tbps=round(tbps, 3),
                frac_of_6p3=round(tbps * 1e12 / HBM_ACHIEVABLE, 3), frac_of_8=round(tbps * 1e12 / HBM_PEAK, 3), n_split=n_split,
                speedup_vs_fwd=round(ms_fw / ms_kv, 2) if has_fwd else None)


def run_equal_bytes_point(pt, rounds):
    """(A) the head_dim-256 call, (B, B2) the head_dim-128 call with twice the heads on the SAME buffers, twice; interleaved"""
    dev = torch.device("cuda:0")
    b, h, hk, d, L, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["dtype"]
    assert d == 256 and pt["seqlen_q"] == 1
    kv_bytes = 2 * b * L * hk * d * 2
    n = _rotation(kv_bytes, kv_bytes)
    caches = [(torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2), torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2)) for _ in range(n)]
    halves = [(kc.view(b, L, 2 * hk, 128), vc.view(b, L, 2 * hk, 128)) for kc, vc in caches]
    q = torch.randn(b, 1, h, d, device=dev, dtype=dt)
    q128 = q.view(b, 1, 2 * h, 128)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    f256 = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs)
    f128 = lambda i: F.flash_attn_with_kvcache(q128, halves[i][0], halves[i][1], cache_seqlens=cs)
    f256(0), f128(0)
    torch.cuda.synchronize()
    ms = _interleaved({"d128": f128, "d256": f256, "d128_again": f128}, n, rounds)
    splits = []
    for qq, (kc, vc), hh in ((q, caches[0], h), (q128, halves[0], 2 * h)):
        p = capi.kvcache_params(qq, kc, vc, torch.empty_like(qq), torch.empty(b, hh, 1, device=dev), cache_seqlens=cs)
        ws = capi.kvcache_workspace_bytes(p)
        splits.append(max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws))))
    del caches, halves
    torch.cuda.empty_cache()
    tb = lambda t: round(kv_bytes / (t * 1e-3) / 1e12, 3)
    lo, hi = sorted((ms["d128"], ms["d128_again"]))
    return dict(equal_bytes=True, b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=1, dtype=str(dt).replace("torch.", ""), kv_gb=round(kv_bytes / 1e9, 3), hbm_bound=kv_bytes >= 1e9,
                caches_rotated=n, n_split_d256=splits[0], n_split_d128=splits[1], ms_d256=round(ms["d256"], 5), ms_d128=round(ms["d128"], 5),
                ms_d128_again=round(ms["d128_again"], 5), d256_over_d128=round(ms["d256"] / ms["d128"], 4), d128_again_over_d128=round(ms["d128_again"] / ms["d128"], 4),
                inside_scatter=bool(lo <= ms["d256"] <= hi), tbps_d256=tb(ms["d256"]), tbps_d128=tb(ms["d128"]),
                frac_of_6p3_d256=round(kv_bytes / (ms["d256"] * 1e-3) / HBM_ACHIEVABLE, 3), frac_of_6p3_d128=round(kv_bytes / (ms["d128"] * 1e-3) / HBM_ACHIEVABLE, 3))


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


def _rotation(kv_bytes, read_bytes, budget=32 << 30):
    """caches to rotate over: enough that the bytes one call reads, summed over the rotation, exceed the working set (at most 512, and no
    more than the memory budget allows)"""
    n = max(1, min(512, math.ceil(WORKING_SET / max(read_bytes, 1))))
    return max(1, min(n, budget // max(kv_bytes, 1)))


def run_window_point(pt, left, rounds):
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    lw = min(L, left + 1)                                     # rows of the short cache: the window's length
    keys = min(L, left + sq)                                  # keys the window reads per (batch, KV head): lo of row 0 .. L
    kv_bytes, win_bytes, short_bytes = (2 * b * n_ * hk * d * 2 for n_ in (L, keys, lw))
    n = _rotation(kv_bytes, win_bytes)
    n_s = _rotation(short_bytes, short_bytes)
    mk = lambda rows: (torch.empty(b, rows, hk, d, device=dev, dtype=dt).uniform_(-2, 2), torch.empty(b, rows, hk, d, device=dev, dtype=dt).uniform_(-2, 2))
    big = [mk(L) for _ in range(n)]
    short = [mk(lw) for _ in range(n_s)]
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    cs_s = torch.full((b,), lw, dtype=torch.int32, device=dev)
    win = lambda i: F.flash_attn_with_kvcache(q, big[i % n][0], big[i % n][1], cache_seqlens=cs, causal=True, window_size=(left, 0))
    full = lambda i: F.flash_attn_with_kvcache(q, big[i % n][0], big[i % n][1], cache_seqlens=cs, causal=True)
    sh = lambda i: F.flash_attn_with_kvcache(q, short[i % n_s][0], short[i % n_s][1], cache_seqlens=cs_s, causal=True)
    win(0), full(0), sh(0)
    torch.cuda.synchronize()
    t_w, t_f, t_s = [], [], []
    for _ in range(rounds):
        t_w.append(time_rotation(win, n, 20))
        t_f.append(time_rotation(full, n, 20))
        t_s.append(time_rotation(sh, n_s, 20))
    ms_w, ms_f, ms_s = statistics.median(t_w), statistics.median(t_f), statistics.median(t_s)
    p = capi.kvcache_params(q, big[0][0], big[0][1], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs, causal=True)
    opt = capi.kvcache_options((left, 0))
    ws = capi.kvcache_workspace_bytes(p, opt)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws), opt))
    ws_f = capi.kvcache_workspace_bytes(p)
    n_split_f = max(1, ws_f and capi.kvcache_num_splits(_with_ws(p, ws_f)))
    rows = b * h * sq
    moved = win_bytes + 2 * rows * d * 2 + rows * 4 + (2 * n_split * rows * (d + 1) * 4 if n_split > 1 else 0)
    del big, short
    torch.cuda.empty_cache()
    return dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), window=[left, 0], causal=True,
                caches_rotated=[n, n_s], ms_window=round(ms_w, 5), ms_unwindowed=round(ms_f, 5), ms_short_cache=round(ms_s, 5),
                window_bytes=moved, tbps_window=round(moved / (ms_w * 1e-3) / 1e12, 3), n_split_window=n_split, n_split_unwindowed=n_split_f,
                unwindowed_over_window=round(ms_f / ms_w, 2), window_over_short=round(ms_w / ms_s, 3))


def run_fp8_point(pt, rounds):
    """the 8-bit call (A) and the 16-bit call on the same logical cache (B), interleaved"""
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    kv16, kv8 = 2 * b * L * hk * d * 2, 2 * b * L * hk * d
    n = _rotation(kv16 + kv8, kv8)                            # the smaller working set (the 8-bit one) must exceed the cache too
    f8 = torch.float8_e4m3fn

    def mk():
        c8, c16 = torch.empty(b, L, hk, d, device=dev, dtype=f8), torch.empty(b, L, hk, d, device=dev, dtype=dt)
        for i in range(b):                                    # (per batch entry: bounds the fp32 temporaries of the conversion)
            c8[i] = torch.empty(L, hk, d, device=dev, dtype=dt).uniform_(-2, 2).to(f8)
            c16[i] = c8[i].to(dt)
        return c8, c16

    sets = [mk() + mk() for _ in range(n)]                    # (k8, k16, v8, v16)
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    kds, vds = torch.empty(b, hk, device=dev).uniform_(0.5, 2.0), torch.empty(b, hk, device=dev).uniform_(0.5, 2.0)
    f_8 = lambda i: F.flash_attn_with_kvcache(q, sets[i][0], sets[i][2], cache_seqlens=cs, k_descale=kds, v_descale=vds)
    f_16 = lambda i: F.flash_attn_with_kvcache(q, sets[i][1], sets[i][3], cache_seqlens=cs)
    f_8(0), f_16(0)
    torch.cuda.synchronize()
    t_8, t_16 = [], []
    for _ in range(rounds):
        t_8.append(time_rotation(f_8, n, 20))
        t_16.append(time_rotation(f_16, n, 20))
    ms_8, ms_16 = statistics.median(t_8), statistics.median(t_16)
    p = capi.kvcache_params(q, sets[0][1], sets[0][3], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs)
    ws = capi.kvcache_workspace_bytes(p)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws)))
    rows = b * h * sq
    other = 2 * rows * d * 2 + rows * 4 + (2 * n_split * rows * (d + 1) * 4 if n_split > 1 else 0)
    tb8, tb16 = (kv8 + other + 2 * b * hk * 4) / (ms_8 * 1e-3) / 1e12, (kv16 + other) / (ms_16 * 1e-3) / 1e12
    del sets
    torch.cuda.empty_cache()
    return dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), kv_gb_16bit=round(kv16 / 1e9, 3), caches_rotated=n,
                ms_fp8=round(ms_8, 5), ms_16bit=round(ms_16, 5), bytes_fp8=kv8 + other + 2 * b * hk * 4, bytes_16bit=kv16 + other,
                tbps_fp8=round(tb8, 3), tbps_16bit=round(tb16, 3), frac_of_6p3_fp8=round(tb8 * 1e12 / HBM_ACHIEVABLE, 3),
                frac_of_6p3_16bit=round(tb16 * 1e12 / HBM_ACHIEVABLE, 3), n_split=n_split, fp8_over_16bit=round(ms_8 / ms_16, 3))


def run_softcap_point(pt, softcap, scale, fp8, rounds):
    """(A) the soft-capped call, (B, B2) the same call without the cap, twice; interleaved"""
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    es = 1 if fp8 else 2
    kv_bytes = 2 * b * L * hk * d * es
    n = _rotation(kv_bytes, kv_bytes)
    cdt = torch.float8_e4m3fn if fp8 else dt

    def mk():
        c = torch.empty(b, L, hk, d, device=dev, dtype=cdt)
        for i in range(b):                                    # (per batch entry: bounds the temporaries of the conversion)
            c[i] = torch.empty(L, hk, d, device=dev, dtype=dt).uniform_(-2, 2).to(cdt)
        return c

    caches = [(mk(), mk()) for _ in range(n)]
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    kw = dict(k_descale=torch.empty(b, hk, device=dev).uniform_(0.5, 2.0), v_descale=torch.empty(b, hk, device=dev).uniform_(0.5, 2.0)) if fp8 else {}
    capped = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs, softmax_scale=scale, softcap=softcap, **kw)
    plain = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs, softmax_scale=scale, **kw)
    diff = float((capped(0).float() - plain(0).float()).abs().max())
    torch.cuda.synchronize()
    ms = _interleaved({"plain": plain, "capped": capped, "plain2": plain}, n, rounds)
    p = capi.kvcache_params(q, caches[0][0], caches[0][1], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs)
    opt = capi.kvcache_options(cache_dtype=capi.FA_CACHE_FP8_E4M3 if fp8 else 0, softcap=softcap, softmax_scale=scale)
    ws = capi.kvcache_workspace_bytes(p, opt)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws), opt))
    rows = b * h * sq
    moved = kv_bytes + 2 * rows * d * 2 + rows * 4 + (2 * n_split * rows * (d + 1) * 4 if n_split > 1 else 0)
    del caches
    torch.cuda.empty_cache()
    return dict(softcap=softcap, softmax_scale=scale, b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), kv="fp8" if fp8 else "16bit",
                kv_gb=round(kv_bytes / 1e9, 3), caches_rotated=n, n_split=n_split, ms_capped=round(ms["capped"], 5), ms_plain=round(ms["plain"], 5),
                ms_plain_again=round(ms["plain2"], 5), capped_over_plain=round(ms["capped"] / ms["plain"], 4), plain_again_over_plain=round(ms["plain2"] / ms["plain"], 4),
                tbps_capped=round(moved / (ms["capped"] * 1e-3) / 1e12, 3), tbps_plain=round(moved / (ms["plain"] * 1e-3) / 1e12, 3), max_abs_diff_to_plain=round(diff, 5))


def sinks_grid(quick, lengths=None):
    bs, ls = ((1, 8), (32768, 131072)) if quick else ((1, 8, 64), (4096, 32768, 131072))
    if lengths:
        ls = tuple(lengths)
    for b, L, layer in itertools.product(bs, ls, ("window", "causal")):
        if b * L <= 8 * 131072:                               # (64 x 128k is 17 GB of K / V: left out)
            yield dict(b=b, h=64, h_k=8, d=64, L=L, seqlen_q=1, dtype=torch.bfloat16, layer=layer)


def run_sinks_point(pt, fp8, page, rounds):
    """(A) the sink call, (B, B2) the same call without sinks, twice; interleaved.  layer "window": causal with window (127, 0), "causal": full"""
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    window = (127, 0) if pt["layer"] == "window" else (-1, -1)
    es = 1 if fp8 else 2
    kv_bytes = 2 * b * L * hk * d * es
    read_bytes = 2 * b * min(L, 127 + sq) * hk * d * es if pt["layer"] == "window" else kv_bytes
    n = _rotation(kv_bytes, read_bytes)
    cdt = torch.float8_e4m3fn if fp8 else dt
    rows_c = page if page else L                              # a cache of (b, L, ...) rows, or a pool of b * L / page pages
    nb = b * (L // page) if page else b

    def mk():
        c = torch.empty(nb, rows_c, hk, d, device=dev, dtype=cdt)
        step = max(1, nb // b)
        for i in range(0, nb, step):                          # (in pieces: bounds the temporaries of the conversion)
            c[i:i + step] = torch.empty(min(step, nb - i), rows_c, hk, d, device=dev, dtype=dt).uniform_(-2, 2).to(cdt)
        return c

    caches = [(mk(), mk()) for _ in range(n)]
    gen = torch.Generator(device="cpu").manual_seed(page or 1)
    tables = [torch.randperm(nb, generator=gen).view(b, L // page).to(device=dev, dtype=torch.int32) for _ in range(n)] if page else None
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    sinks = torch.empty(h, device=dev).uniform_(0.0, 6.0)
    kw = dict(k_descale=torch.empty(b, hk, device=dev).uniform_(0.5, 2.0), v_descale=torch.empty(b, hk, device=dev).uniform_(0.5, 2.0)) if fp8 else {}
    call = lambda i, **extra: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs, causal=True, window_size=window,
                                                        **(dict(block_table=tables[i]) if page else {}), **kw, **extra)
    with_sinks = lambda i: call(i, sinks=sinks)
    plain = lambda i: call(i)
    diff = float((with_sinks(0).float() - plain(0).float()).abs().max())
    torch.cuda.synchronize()
    ms = _interleaved({"plain": plain, "sinks": with_sinks, "plain2": plain}, n, rounds)
    if page:
        p = capi.kvcache_params(q, caches[0][0], caches[0][1], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs, causal=True, block_table=tables[0])
    else:
        p = capi.kvcache_params(q, caches[0][0], caches[0][1], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs, causal=True)
    opt = capi.kvcache_options(window, cache_dtype=capi.FA_CACHE_FP8_E4M3 if fp8 else 0, sinks=sinks)
    ws = capi.kvcache_workspace_bytes(p, opt)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws), opt))
    del caches
    torch.cuda.empty_cache()
    lo, hi = sorted((ms["plain"], ms["plain2"]))
    return dict(sinks=True, layer=pt["layer"], b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), kv="fp8" if fp8 else "16bit",
                page_block_size=page or None, read_gb=round(read_bytes / 1e9, 4), hbm_bound=read_bytes >= 1e9, caches_rotated=n, n_split=n_split,
                ms_sinks=round(ms["sinks"], 5), ms_plain=round(ms["plain"], 5), ms_plain_again=round(ms["plain2"], 5),
                sinks_over_plain=round(ms["sinks"] / ms["plain"], 4), plain_again_over_plain=round(ms["plain2"] / ms["plain"], 4),
                inside_scatter=bool(lo <= ms["sinks"] <= hi), tbps_sinks=round(read_bytes / (ms["sinks"] * 1e-3) / 1e12, 3),
                tbps_plain=round(read_bytes / (ms["plain"] * 1e-3) / 1e12, 3), max_abs_diff_to_plain=round(diff, 5))


def run_sinks_ab_point(pt, base, fp8, page, rounds):
    """the sink call through this build's C ABI (A, A2: timed twice) and through the baseline library's (B), interleaved, on the same caches"""
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    window = (127, 0) if pt["layer"] == "window" else (-1, -1)
    es = 1 if fp8 else 2
    kv_bytes = 2 * b * L * hk * d * es
    read_bytes = 2 * b * min(L, 127 + sq) * hk * d * es if pt["layer"] == "window" else kv_bytes
    n = _rotation(kv_bytes, read_bytes)
    cdt = torch.float8_e4m3fn if fp8 else dt
    rows_c, nb = (page, b * (L // page)) if page else (L, b)
    mk = lambda: torch.empty(nb, rows_c, hk, d, device=dev, dtype=torch.float16).uniform_(-2, 2).to(cdt)
    caches = [(mk(), mk()) for _ in range(n)]
    gen = torch.Generator(device="cpu").manual_seed(page or 1)
    tables = [torch.randperm(nb, generator=gen).view(b, L // page).to(device=dev, dtype=torch.int32) if page else None for _ in range(n)]
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    sinks = torch.empty(h, device=dev).uniform_(0.0, 6.0)
    kds, vds = (torch.empty(b, hk, device=dev).uniform_(0.5, 2.0) for _ in range(2)) if fp8 else (None, None)
    opt = capi.kvcache_options(window, cache_dtype=capi.FA_CACHE_FP8_E4M3 if fp8 else 0, k_descale=kds, v_descale=vds, sinks=sinks)
    libs = {"A": capi.lib(), "B": base}
    for lib in libs.values():
        lib.fa_run_mha_fwd_kvcache_ex.argtypes = [ctypes.POINTER(capi.KvcacheParams), ctypes.c_void_p, ctypes.c_void_p]
        lib.fa_run_mha_fwd_kvcache_ex.restype = ctypes.c_int
        lib.fa_kvcache_workspace_bytes_ex.argtypes = [ctypes.POINTER(capi.KvcacheParams), ctypes.c_void_p]
        lib.fa_kvcache_workspace_bytes_ex.restype = ctypes.c_int64
    params = {}
    for tag, lib in libs.items():
        o, lse = torch.empty_like(q), torch.empty(b, h, sq, device=dev)
        ps = [capi.kvcache_params(q, kc, vc, o, lse, cache_seqlens=cs, causal=True, **(dict(block_table=tables[i]) if page else {})) for i, (kc, vc) in enumerate(caches)]
        ws = int(lib.fa_kvcache_workspace_bytes_ex(ctypes.byref(ps[0]), ctypes.byref(opt)))
        assert ws >= 0, ws
        buf = torch.empty(max(ws, 16) // 4, device=dev, dtype=torch.float32)
        for p in ps:
            p.workspace, p.workspace_bytes = (buf.data_ptr(), ws) if ws > 0 else (None, 0)
        params[tag] = (ps, o, lse, buf, ws)
    stream = torch.cuda.current_stream().cuda_stream

    def call(tag):
        lib, ps = libs[tag], params[tag][0]
        return lambda i: capi.check(lib.fa_run_mha_fwd_kvcache_ex(ctypes.byref(ps[i]), ctypes.byref(opt), stream))

    fa, fb = call("A"), call("B")
    fa(0), fb(0)
    torch.cuda.synchronize()
    same = torch.equal(params["A"][1].view(torch.int16), params["B"][1].view(torch.int16)) and torch.equal(params["A"][2].view(torch.int32), params["B"][2].view(torch.int32))
    ms = _interleaved({"this": fa, "baseline": fb, "this2": fa}, n, rounds)
    split = params["A"][4] > 0
    del caches, params
    torch.cuda.empty_cache()
    lo, hi = sorted((ms["this"], ms["this2"]))
    return dict(sinks=True, ab=True, layer=pt["layer"], b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), kv="fp8" if fp8 else "16bit",
                page_block_size=page or None, read_gb=round(read_bytes / 1e9, 4), hbm_bound=read_bytes >= 1e9, caches_rotated=n, split=bool(split),
                ms_this=round(ms["this"], 5), ms_baseline=round(ms["baseline"], 5), ms_this_again=round(ms["this2"], 5),
                this_over_baseline=round(ms["this"] / ms["baseline"], 4), this_again_over_this=round(ms["this2"] / ms["this"], 4),
                baseline_inside_scatter=bool(lo <= ms["baseline"] <= hi), bit_identical=bool(same))


def tree_grid(quick, n_tree, lengths=None, head_dims=None):
    """the grid's points with seqlen_q = n_tree, each (b, heads, d, L, dtype) once"""
    seen = set()
    for pt in grid(quick, lengths, head_dims):
        key = (pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["dtype"])
        if key not in seen:
            seen.add(key)
            yield dict(pt, seqlen_q=n_tree)


def _tree_setup(pt, fp8):
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    kv_bytes = 2 * b * L * hk * d * (1 if fp8 else 2)
    n = _rotation(kv_bytes, kv_bytes)
    cdt = torch.float8_e4m3fn if fp8 else dt

    def mk():
        c = torch.empty(b, L, hk, d, device=dev, dtype=cdt)
        for i in range(b):                                    # (per batch entry: bounds the temporaries of the conversion)
            c[i] = torch.empty(L, hk, d, device=dev, dtype=dt).uniform_(-2, 2).to(cdt)
        return c

    caches = [(mk(), mk()) for _ in range(n)]
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    parents = torch.tensor([-1] + [(t - 1) // 2 for t in range(1, sq)], device=dev)
    words = F.tree_mask_from_parents(parents).expand(b, sq).contiguous()
    kds, vds = (torch.empty(b, hk, device=dev).uniform_(0.5, 2.0) for _ in range(2)) if fp8 else (None, None)
    return dev, kv_bytes, n, caches, q, cs, words, kds, vds


def run_tree_point(pt, fp8, rounds):
    """(A) the tree call under the binary-heap tree, (B, B2) the causal call of the same shape, twice; interleaved"""
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    dev, kv_bytes, n, caches, q, cs, words, kds, vds = _tree_setup(pt, fp8)
    kw = dict(k_descale=kds, v_descale=vds) if fp8 else {}
    tree = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs, tree_mask=words, **kw)
    causal = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs, causal=True, **kw)
    diff = float((tree(0).float() - causal(0).float()).abs().max())
    torch.cuda.synchronize()
    ms = _interleaved({"causal": causal, "tree": tree, "causal2": causal}, n, rounds)
    p = capi.kvcache_params(q, caches[0][0], caches[0][1], torch.empty_like(q), torch.empty(b, h, sq, device=dev), cache_seqlens=cs)
    opt = capi.kvcache_options(cache_dtype=capi.FA_CACHE_FP8_E4M3 if fp8 else 0, tree_mask=words)
    ws = capi.kvcache_workspace_bytes(p, opt)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws), opt))
    rows = b * h * sq
    moved = kv_bytes + 2 * rows * d * 2 + rows * 4 + (2 * n_split * rows * (d + 1) * 4 if n_split > 1 else 0)
    del caches
    torch.cuda.empty_cache()
    lo, hi = sorted((ms["causal"], ms["causal2"]))
    return dict(tree=sq, b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), kv="fp8" if fp8 else "16bit", kv_gb=round(kv_bytes / 1e9, 3),
                hbm_bound=kv_bytes >= 1e9, caches_rotated=n, n_split=n_split, ms_tree=round(ms["tree"], 5), ms_causal=round(ms["causal"], 5),
                ms_causal_again=round(ms["causal2"], 5), tree_over_causal=round(ms["tree"] / ms["causal"], 4), causal_again_over_causal=round(ms["causal2"] / ms["causal"], 4),
                inside_scatter=bool(lo <= ms["tree"] <= hi), tbps_tree=round(moved / (ms["tree"] * 1e-3) / 1e12, 3), tbps_causal=round(moved / (ms["causal"] * 1e-3) / 1e12, 3),
                max_abs_diff_to_causal=round(diff, 5))


def run_tree_ab_point(pt, base, fp8, rounds):
    """the tree call through this build's C ABI (A, A2: timed twice) and through the baseline library's (B), interleaved, on the same caches"""
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    dev, kv_bytes, n, caches, q, cs, words, kds, vds = _tree_setup(pt, fp8)
    opt = capi.kvcache_options(cache_dtype=capi.FA_CACHE_FP8_E4M3 if fp8 else 0, k_descale=kds, v_descale=vds, tree_mask=words)
    libs = {"A": capi.lib(), "B": base}
    for lib in libs.values():
        lib.fa_run_mha_fwd_kvcache_ex.argtypes = [ctypes.POINTER(capi.KvcacheParams), ctypes.c_void_p, ctypes.c_void_p]
        lib.fa_run_mha_fwd_kvcache_ex.restype = ctypes.c_int
        lib.fa_kvcache_workspace_bytes_ex.argtypes = [ctypes.POINTER(capi.KvcacheParams), ctypes.c_void_p]
        lib.fa_kvcache_workspace_bytes_ex.restype = ctypes.c_int64
    params = {}
    for tag, lib in libs.items():
        o, lse = torch.empty_like(q), torch.empty(b, h, sq, device=dev)
        ps = [capi.kvcache_params(q, kc, vc, o, lse, cache_seqlens=cs) for kc, vc in caches]
        ws = int(lib.fa_kvcache_workspace_bytes_ex(ctypes.byref(ps[0]), ctypes.byref(opt)))
        assert ws >= 0, ws
        buf = torch.empty(max(ws, 16) // 4, device=dev, dtype=torch.float32)
        for p in ps:
            p.workspace, p.workspace_bytes = (buf.data_ptr(), ws) if ws > 0 else (None, 0)
        params[tag] = (ps, o, lse, buf, ws)
    stream = torch.cuda.current_stream().cuda_stream

    def call(tag):
        lib, ps = libs[tag], params[tag][0]
        return lambda i: capi.check(lib.fa_run_mha_fwd_kvcache_ex(ctypes.byref(ps[i]), ctypes.byref(opt), stream))

    fa, fb = call("A"), call("B")
    fa(0), fb(0)
    torch.cuda.synchronize()
    same = torch.equal(params["A"][1].view(torch.int16), params["B"][1].view(torch.int16)) and torch.equal(params["A"][2].view(torch.int32), params["B"][2].view(torch.int32))
    ms = _interleaved({"this": fa, "baseline": fb, "this2": fa}, n, rounds)
    split = params["A"][4] > 0
    del caches, params
    torch.cuda.empty_cache()
    lo, hi = sorted((ms["this"], ms["this2"]))
    return dict(tree=sq, ab=True, b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), kv="fp8" if fp8 else "16bit", kv_gb=round(kv_bytes / 1e9, 3),
                hbm_bound=kv_bytes >= 1e9, caches_rotated=n, split=bool(split), ms_this=round(ms["this"], 5), ms_baseline=round(ms["baseline"], 5),
                ms_this_again=round(ms["this2"], 5), this_over_baseline=round(ms["this"] / ms["baseline"], 4), this_again_over_this=round(ms["this2"] / ms["this"], 4),
                baseline_inside_scatter=bool(lo <= ms["baseline"] <= hi), bit_identical=bool(same))


def torch_rotate(x, cos, sin, pos, interleaved):
    """the rotation with torch ops on x's device: x (b, s, heads, d), pos (b,) long - every row of sequence i at pos[i] (s = 1 here)"""
    rd = 2 * cos.shape[1]
    c, s = cos[pos].float()[:, None, None, :], sin[pos].float()[:, None, None, :]
    xf = x.float()
    if interleaved:
        xa, xb = xf[..., 0:rd:2], xf[..., 1:rd:2]
        y = torch.stack((xa * c - xb * s, xb * c + xa * s), dim=-1).flatten(-2)
    else:
        xa, xb = xf[..., :rd // 2], xf[..., rd // 2:rd]
        y = torch.cat((xa * c - xb * s, xb * c + xa * s), dim=-1)
    y = y.to(x.dtype)
    return y if rd == x.shape[-1] else torch.cat((y, x[..., rd:]), dim=-1)


def run_rotary_point(pt, rotary_dim, interleaved, rounds):
    """(A) the rotary call, (B, B2) the plain call with append on pre-rotated inputs, twice, (C) torch rotation + the plain call; interleaved"""
    dev = torch.device("cuda:0")
    b, h, hk, d, L, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["dtype"]
    rd = min(rotary_dim or d, d)
    kv_bytes = 2 * b * L * hk * d * 2
    n = _rotation(kv_bytes, kv_bytes)
    caches = [(torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2), torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2))
              for _ in range(n)]
    q, k, v = (torch.randn(b, 1, hh, d, device=dev, dtype=dt) for hh in (h, hk, hk))
    cs = torch.full((b,), L - 1, dtype=torch.int32, device=dev)
    inv = 10000.0 ** (-torch.arange(0, rd, 2, dtype=torch.float64, device=dev) / rd)
    ang = torch.arange(L, dtype=torch.float64, device=dev)[:, None] * inv[None, :]
    cos, sin = ang.cos().to(dt), ang.sin().to(dt)
    pos = cs.long()
    q_rot, k_rot = torch_rotate(q, cos, sin, pos, interleaved), torch_rotate(k, cos, sin, pos, interleaved)
    f_a = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], k=k, v=v, cache_seqlens=cs, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=interleaved)
    f_b = lambda i: F.flash_attn_with_kvcache(q_rot, caches[i][0], caches[i][1], k=k_rot, v=v, cache_seqlens=cs)
    f_c = lambda i: F.flash_attn_with_kvcache(torch_rotate(q, cos, sin, cs.long(), interleaved), caches[i][0], caches[i][1],
                                              k=torch_rotate(k, cos, sin, cs.long(), interleaved), v=v, cache_seqlens=cs)
    o_a, o_b, o_c = f_a(0), f_b(0), f_c(0)
    torch.cuda.synchronize()
    same = torch.equal(o_a.view(torch.int16), o_b.view(torch.int16)) and torch.equal(o_a.view(torch.int16), o_c.view(torch.int16))
    t = {"a": [], "b": [], "b2": [], "c": []}
    for _ in range(rounds):
        t["a"].append(time_rotation(f_a, n, 20))
        t["b"].append(time_rotation(f_b, n, 20))
        t["c"].append(time_rotation(f_c, n, 20))
        t["b2"].append(time_rotation(f_b, n, 20))
    ms = {k_: statistics.median(v_) for k_, v_ in t.items()}
    del caches
    torch.cuda.empty_cache()
    return dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=1, seqlen_new=1, dtype=str(dt).replace("torch.", ""), rotary_dim=rd, interleaved=bool(interleaved),
                kv_gb=round(kv_bytes / 1e9, 3), caches_rotated=n, ms_rotary=round(ms["a"], 5), ms_prerotated=round(ms["b"], 5), ms_prerotated_again=round(ms["b2"], 5),
                ms_torch_rotation=round(ms["c"], 5), rotary_over_prerotated=round(ms["a"] / ms["b"], 4), prerotated_again_over_prerotated=round(ms["b2"] / ms["b"], 4),
                torch_rotation_over_rotary=round(ms["c"] / ms["a"], 3), bit_identical=bool(same))


def _interleaved(fns, n, rounds):
    """median ms per call of each arm, the arms taken in turn within every round"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(time_rotation(f, n, 20))
    return {k: statistics.median(v) for k, v in t.items()}


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def run_ragged_uniform_point(b, h, hk, d, L, dt, fp8, page, rounds):
    """every sq_i = 1: the ragged call against the dense call of the same shape, the dense call twice"""
    dev = torch.device("cuda:0")
    es = 1 if fp8 else 2
    kv_bytes = 2 * b * L * hk * d * es
    n = _rotation(kv_bytes, kv_bytes)
    cdt = torch.float8_e4m3fn if fp8 else dt
    sets = []
    for i in range(n):
        shape = (b * (L // page), page, hk, d) if page else (b, L, hk, d)
        mk = lambda: (torch.empty(shape, device=dev, dtype=dt).uniform_(-2, 2).to(cdt) if not fp8 else
                      torch.randint(0, 0x78, shape, device=dev, dtype=torch.uint8).view(cdt))
        table = torch.randperm(b * (L // page), generator=torch.Generator().manual_seed(i)).view(b, L // page).to(device=dev, dtype=torch.int32) if page else None
        sets.append((mk(), mk(), table))
    q = torch.randn(b, 1, h, d, device=dev, dtype=dt)
    qp = q.view(b, h, d)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    cu = torch.arange(b + 1, dtype=torch.int32, device=dev)
    kw = dict(k_descale=torch.empty(b, hk, device=dev).uniform_(0.5, 2.0), v_descale=torch.empty(b, hk, device=dev).uniform_(0.5, 2.0)) if fp8 else {}
    dense = lambda i: F.flash_attn_with_kvcache(q, sets[i][0], sets[i][1], cache_seqlens=cs, block_table=sets[i][2], **kw)
    ragged = lambda i: F.flash_attn_with_kvcache(qp, sets[i][0], sets[i][1], cache_seqlens=cs, block_table=sets[i][2], cu_seqlens_q=cu, max_seqlen_q=1, **kw)
    same = _bits_equal(dense(0).view(b, h, d), ragged(0))
    torch.cuda.synchronize()
    ms = _interleaved({"dense": dense, "ragged": ragged, "dense2": dense}, n, rounds)
    p = capi.kvcache_params(q, sets[0][0], sets[0][1], torch.empty_like(q), torch.empty(b, h, 1, device=dev), cache_seqlens=cs, block_table=sets[0][2])
    opt = capi.kvcache_options(cache_dtype=capi.FA_CACHE_FP8_E4M3) if fp8 else None
    ws = capi.kvcache_workspace_bytes(p, opt)
    n_split = max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws), opt))
    del sets
    torch.cuda.empty_cache()
    return dict(ragged="uniform", b=b, h=h, h_k=hk, d=d, L=L, dtype=str(dt).replace("torch.", ""), kv="fp8" if fp8 else "16bit", page_block_size=page or 0,
                kv_gb=round(kv_bytes / 1e9, 3), caches_rotated=n, n_split_dense=n_split, ms_dense=round(ms["dense"], 5), ms_ragged=round(ms["ragged"], 5),
                ms_dense_again=round(ms["dense2"], 5), ragged_over_dense=round(ms["ragged"] / ms["dense"], 4), dense_again_over_dense=round(ms["dense2"] / ms["dense"], 4),
                tbps_ragged=round(kv_bytes / (ms["ragged"] * 1e-3) / 1e12, 3), bit_identical=bool(same))


def run_ragged_mixed_point(name, sq, h, hk, d, dt, page, rounds):
    """one scheduler step as ONE ragged call against one dense call per distinct sq on gathered inputs; paged cache, lengths 1k .. 32k"""
    dev = torch.device("cuda:0")
    b, total, cap = len(sq), sum(sq), 32768
    g = torch.Generator().manual_seed(len(sq) + total)
    lens = [int(x) for x in torch.randint(1024, cap - max(sq), (b,), generator=g)]
    lens = [max(L, s) for L, s in zip(lens, sq)]
    cols = cap // page
    kv_bytes = 2 * sum(lens) * hk * d * 2
    n = max(1, min(_rotation(2 * b * cap * hk * d * 2, kv_bytes), 4))
    sets = []
    for i in range(n):
        kp = torch.empty(b * cols, page, hk, d, device=dev, dtype=dt).uniform_(-2, 2)
        vp = torch.empty(b * cols, page, hk, d, device=dev, dtype=dt).uniform_(-2, 2)
        table = torch.randperm(b * cols, generator=torch.Generator().manual_seed(i)).view(b, cols).to(device=dev, dtype=torch.int32)
        sets.append((kp, vp, table))
    q = torch.randn(total, h, d, device=dev, dtype=dt)
    cs = torch.tensor(lens, dtype=torch.int32, device=dev)
    cu_l = [0]
    for s_ in sq:
        cu_l.append(cu_l[-1] + s_)
    cu = torch.tensor(cu_l, dtype=torch.int32, device=dev)
    groups = []
    for s_ in sorted(set(sq)):
        idx = [i for i in range(b) if sq[i] == s_]
        rows = torch.tensor([[cu_l[i] + t for t in range(s_)] for i in idx], device=dev)
        groups.append((s_, torch.tensor(idx, device=dev), rows))
    ragged = lambda i: F.flash_attn_with_kvcache(q, sets[i][0], sets[i][1], cache_seqlens=cs, causal=True, block_table=sets[i][2], cu_seqlens_q=cu, max_seqlen_q=max(sq))

    def loop(i):
        outs = []
        for s_, idx, rows in groups:             # the gathers a caller needs today, on the device: q rows, lengths, table rows
            outs.append(F.flash_attn_with_kvcache(q[rows], sets[i][0], sets[i][1], cache_seqlens=cs[idx], causal=True, block_table=sets[i][2][idx]))
        return outs

    o_r, o_l = ragged(0), loop(0)
    same = all(_bits_equal(o_r[rows], o) for (_, _, rows), o in zip(groups, o_l))
    torch.cuda.synchronize()
    ms = _interleaved({"loop": loop, "ragged": ragged, "loop2": loop}, n, rounds)
    del sets
    torch.cuda.empty_cache()
    return dict(ragged="mixed", step=name, b=b, total_q=total, distinct_sq=len(groups), h=h, h_k=hk, d=d, dtype=str(dt).replace("torch.", ""), page_block_size=page,
                kv_gb=round(kv_bytes / 1e9, 3), caches_rotated=n, ms_ragged=round(ms["ragged"], 5), ms_dense_loop=round(ms["loop"], 5), ms_dense_loop_again=round(ms["loop2"], 5),
                loop_over_ragged=round(ms["loop"] / ms["ragged"], 3), loop_again_over_loop=round(ms["loop2"] / ms["loop"], 4), bit_identical=bool(same))


def run_ragged_chunk_point(sq, h, hk, d, dt, rounds, L=8192):
    """one sequence bringing a chunk of sq rows over L keys, causal: the ragged decode call against fwd on the same prefix"""
    dev = torch.device("cuda:0")
    kv_bytes = 2 * L * hk * d * 2
    n = _rotation(kv_bytes, kv_bytes)
    caches = [(torch.empty(1, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2), torch.empty(1, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2)) for _ in range(n)]
    q = torch.randn(sq, h, d, device=dev, dtype=dt)
    q4 = q[None]
    cs = torch.tensor([L], dtype=torch.int32, device=dev)
    cu = torch.tensor([0, sq], dtype=torch.int32, device=dev)
    ragged = lambda i: F.flash_attn_with_kvcache(q, caches[i][0], caches[i][1], cache_seqlens=cs, causal=True, cu_seqlens_q=cu, max_seqlen_q=sq)
    fw = lambda i: F.fwd(q4, caches[i][0], caches[i][1], True)
    err = float((ragged(0).float() - fw(0)[0][0].float()).abs().max())
    torch.cuda.synchronize()
    ms = _interleaved({"fwd": fw, "ragged": ragged, "fwd2": fw}, n, rounds)
    del caches
    torch.cuda.empty_cache()
    return dict(ragged="chunk", sq=sq, L=L, h=h, h_k=hk, d=d, dtype=str(dt).replace("torch.", ""), caches_rotated=n, ms_ragged=round(ms["ragged"], 5),
                ms_fwd=round(ms["fwd"], 5), ms_fwd_again=round(ms["fwd2"], 5), ragged_over_fwd=round(ms["ragged"] / ms["fwd"], 3),
                fwd_again_over_fwd=round(ms["fwd2"] / ms["fwd"], 4), max_abs_diff=round(err, 5))


def run_ragged(quick, rounds):
    dt = torch.float16
    for b, L, d in itertools.product((1, 8, 64), (4096, 32768), (64, 128)):
        if quick and (b, L) not in ((8, 32768), (64, 4096)):
            continue
        for fp8, page in ((False, None), (True, None), (False, 256)) if d == 128 else ((False, None),):
            yield run_ragged_uniform_point(b, 32, 8, d, L, dt, fp8, page, rounds)
    yield run_ragged_mixed_point("60x1+3x4+1x256", [1] * 60 + [4] * 3 + [256], 32, 8, 128, dt, 256, rounds)
    yield run_ragged_mixed_point("32x1+32x5", [1, 5] * 32, 32, 8, 128, dt, 256, rounds)
    if not quick:
        yield run_ragged_mixed_point("24x1+4x2+3x4+1x8", [1] * 24 + [2] * 4 + [4] * 3 + [8], 32, 8, 128, dt, 256, rounds)
        yield run_ragged_mixed_point("60x1+3x4+1x256 d64", [1] * 60 + [4] * 3 + [256], 32, 8, 64, dt, 256, rounds)
    for sq in (128, 512, 2048):
        yield run_ragged_chunk_point(sq, 32, 8, 128, dt, rounds)


def run_prefill_point(sq, L, h, hk, d, dt, fp8, page, rounds):
    """one sequence bringing a causal chunk of sq rows over L keys: prefill=True against prefill=False (timed twice) and, 16-bit contiguous, fwd"""
    dev = torch.device("cuda:0")
    es = 1 if fp8 else 2
    kv_bytes = 2 * L * hk * d * es
    n = _rotation(kv_bytes, kv_bytes)
    cdt = torch.float8_e4m3fn if fp8 else dt
    sets = []
    for i in range(n):
        shape = (L // page, page, hk, d) if page else (1, L, hk, d)
        mk = lambda: (torch.empty(shape, device=dev, dtype=dt).uniform_(-2, 2) if not fp8 else torch.randint(0, 0x78, shape, device=dev, dtype=torch.uint8).view(cdt))
        table = torch.randperm(L // page, generator=torch.Generator().manual_seed(i)).view(1, L // page).to(device=dev, dtype=torch.int32) if page else None
        sets.append((mk(), mk(), table))
    q = torch.randn(1, sq, h, d, device=dev, dtype=dt)
    cs = torch.tensor([L], dtype=torch.int32, device=dev)
    kw = dict(k_descale=torch.empty(1, hk, device=dev).uniform_(0.5, 2.0), v_descale=torch.empty(1, hk, device=dev).uniform_(0.5, 2.0)) if fp8 else {}
    wide = lambda i: F.flash_attn_with_kvcache(q, sets[i][0], sets[i][1], cache_seqlens=cs, causal=True, block_table=sets[i][2], prefill=True, **kw)
    narrow = lambda i: F.flash_attn_with_kvcache(q, sets[i][0], sets[i][1], cache_seqlens=cs, causal=True, block_table=sets[i][2], **kw)
    arms = {"narrow": narrow, "wide": wide, "narrow2": narrow}
    with_fwd = not fp8 and not page
    if with_fwd:
        arms["fwd"] = lambda i: F.fwd(q, sets[i][0], sets[i][1], True)
    err = float((wide(0).float() - narrow(0).float()).abs().max())
    torch.cuda.synchronize()
    ms = _interleaved(arms, n, rounds)
    p = capi.kvcache_params(q, sets[0][0], sets[0][1], torch.empty_like(q), torch.empty(1, h, sq, device=dev), cache_seqlens=cs, causal=True, block_table=sets[0][2])
    splits = []
    for rt in (None, 64):
        opt = capi.kvcache_options(cache_dtype=capi.FA_CACHE_FP8_E4M3 if fp8 else 0, row_tile=rt)
        ws = capi.kvcache_workspace_bytes(p, opt)
        splits.append(max(1, ws and capi.kvcache_num_splits(_with_ws(p, ws), opt)))
    del sets
    torch.cuda.empty_cache()
    row = dict(prefill="chunk", sq=sq, L=L, h=h, h_k=hk, d=d, dtype=str(dt).replace("torch.", ""), kv="fp8" if fp8 else "16bit", page_block_size=page or 0,
               caches_rotated=n, n_split_16=splits[0], n_split_64=splits[1], ms_prefill=round(ms["wide"], 5), ms_16row=round(ms["narrow"], 5),
               ms_16row_again=round(ms["narrow2"], 5), prefill_over_16row=round(ms["wide"] / ms["narrow"], 4),
               again_over_16row=round(ms["narrow2"] / ms["narrow"], 4), max_abs_diff=round(err, 5))
    if with_fwd:
        row.update(ms_fwd=round(ms["fwd"], 5), prefill_over_fwd=round(ms["wide"] / ms["fwd"], 3))
    return row


def run_prefill(lengths, head_dims, fp8, pages, rounds):
    for d, L, sq in itertools.product(tuple(head_dims or (128, 64)), tuple(lengths or (8192, 32768)), (64, 128, 512, 2048)):
        for page in (pages or [None]):
            yield run_prefill_point(sq, L, 32, 8, d, torch.float16, fp8, page, rounds)


def run_mla_point(b, h, L, page, rounds):
    """(A) flash_mla_with_kvcache over a bf16 latent cache, (B, B2) the d-256 decode call with one KV head on the same h, b, L, twice; interleaved"""
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    mla_bytes, ref_bytes = b * L * 576 * 2, 2 * b * L * 256 * 2
    n = _rotation(mla_bytes + ref_bytes, ref_bytes)
    sets = []
    for i in range(n):
        if page:
            nb = b * L // page
            table = torch.randperm(nb, generator=torch.Generator().manual_seed(i)).view(b, L // page).to(device=dev, dtype=torch.int32)
            shape = lambda d: (nb, page, 1, d)
        else:
            table, shape = None, lambda d: (b, L, 1, d)
        sets.append((torch.empty(shape(576), device=dev, dtype=dt).uniform_(-2, 2), torch.empty(shape(256), device=dev, dtype=dt).uniform_(-2, 2),
                     torch.empty(shape(256), device=dev, dtype=dt).uniform_(-2, 2), table))
    q = torch.randn(b, 1, h, 576, device=dev, dtype=dt)
    q256 = torch.randn(b, 1, h, 256, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    mla = lambda i: F.flash_mla_with_kvcache(q, sets[i][0], cs, block_table=sets[i][3])
    ref = lambda i: F.flash_attn_with_kvcache(q256, sets[i][1], sets[i][2], cache_seqlens=cs, block_table=sets[i][3])
    mla(0), ref(0)
    torch.cuda.synchronize()
    ms = _interleaved({"d256": ref, "mla": mla, "d256_again": ref}, n, rounds)
    p = capi.mla_params(q, sets[0][0], torch.empty(b, 1, h, 512, device=dev, dtype=dt), torch.empty(b, h, 1, device=dev), cs, block_table=sets[0][3])
    ws = capi.mla_workspace_bytes(p)
    n_split = max(1, ws and capi.mla_num_splits(_with_ws(p, ws)))
    p2 = capi.kvcache_params(q256, sets[0][1], sets[0][2], torch.empty_like(q256), torch.empty(b, h, 1, device=dev), cache_seqlens=cs, block_table=sets[0][3])
    ws2 = capi.kvcache_workspace_bytes(p2)
    n_split2 = max(1, ws2 and capi.kvcache_num_splits(_with_ws(p2, ws2)))
    del sets
    torch.cuda.empty_cache()
    lo, hi = sorted((ms["d256"], ms["d256_again"]))
    return dict(mla=True, b=b, h=h, L=L, seqlen_q=1, dtype="bfloat16", page_block_size=page or 0, caches_rotated=n, kv_gb=round(mla_bytes / 1e9, 3),
                n_split_mla=n_split, n_split_d256=n_split2, ms_mla=round(ms["mla"], 5), ms_d256=round(ms["d256"], 5), ms_d256_again=round(ms["d256_again"], 5),
                tbps_mla=round(mla_bytes / (ms["mla"] * 1e-3) / 1e12, 3), frac_of_6p3_mla=round(mla_bytes / (ms["mla"] * 1e-3) / HBM_ACHIEVABLE, 3),
                frac_of_6p3_d256=round(ref_bytes / (ms["d256"] * 1e-3) / HBM_ACHIEVABLE, 3), mla_over_d256=round(ms["mla"] / ms["d256"], 4),
                d256_again_over_d256=round(ms["d256_again"] / ms["d256"], 4), inside_scatter=bool(lo <= ms["mla"] <= hi))


def run_mla(lengths, pages, rounds):
    for h, b, L in itertools.product((16, 128), (1, 8, 64), tuple(lengths or (4096, 32768, 131072))):
        for page in ([None] + list(pages or [])):
            yield run_mla_point(b, h, L, page, rounds)


def run_mla_sparse_point(b, h, lengths, page, rounds, topk=2048):
    """the dense MLA call at L = topk twice (the yardstick and its noise), (i) the identity list on the same caches, and per L (ii) sorted / (iii) unsorted random
    positions on one cache of L rows; then, at b <= 8, arm (i) under forced split counts"""
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    read_bytes = b * topk * 576 * 2
    n = _rotation(read_bytes, read_bytes, budget=8 << 30)

    def cache(L, seed):
        nb = b * L // page
        table = torch.randperm(nb, generator=torch.Generator().manual_seed(seed)).view(b, L // page).to(device=dev, dtype=torch.int32)
        return torch.empty(nb, page, 1, 576, device=dev, dtype=dt).uniform_(-2, 2), table

    small = [cache(topk, i) for i in range(n)]
    q = torch.randn(b, 1, h, 576, device=dev, dtype=dt)
    cs = torch.full((b,), topk, dtype=torch.int32, device=dev)
    ident = torch.arange(topk, dtype=torch.int32, device=dev).view(1, 1, topk).expand(b, 1, topk).contiguous()
    dense = lambda i: F.flash_mla_with_kvcache(q, small[i % n][0], cs, block_table=small[i % n][1])
    arm_i = lambda i, ns=0: F.flash_mla_sparse_with_kvcache(q, small[i % n][0], cs, ident, block_table=small[i % n][1], num_splits=ns)
    assert _bits_equal(F.flash_mla_sparse_with_kvcache(q, small[0][0], cs, ident, block_table=small[0][1], num_splits=1),
                       F.flash_mla_with_kvcache(q, small[0][0], cs, block_table=small[0][1], num_splits=1)), "the identity list is not the dense call"
    arms = {"dense": dense, "sparse_identity": arm_i}
    big, lists = {}, {}
    n_lists = max(n, 4)
    gen = torch.Generator().manual_seed(1234 + b + h)
    for L in lengths:
        big[L] = cache(L, 1000 + L)
        pos = torch.stack([torch.stack([torch.randperm(L, generator=gen)[:topk] for _ in range(b)]) for _ in range(n_lists)]).to(torch.int32).unsqueeze(2)
        lists[L] = (pos.sort(-1).values.to(dev), pos.to(dev))
        csL = torch.full((b,), L, dtype=torch.int32, device=dev)
        arms[f"sparse_sorted_L{L}"] = lambda i, L=L, csL=csL: F.flash_mla_sparse_with_kvcache(q, big[L][0], csL, lists[L][0][i % n_lists], block_table=big[L][1])
        arms[f"sparse_unsorted_L{L}"] = lambda i, L=L, csL=csL: F.flash_mla_sparse_with_kvcache(q, big[L][0], csL, lists[L][1][i % n_lists], block_table=big[L][1])
    arms["dense_again"] = dense
    for f in arms.values():
        f(0)
    torch.cuda.synchronize()
    ms = _interleaved(arms, max(n, n_lists), rounds)
    o, lse = torch.empty(b, 1, h, 512, device=dev, dtype=dt), torch.empty(b, h, 1, device=dev)
    ps = capi.mla_sparse_params(q, small[0][0], o, lse, ident, cs, block_table=small[0][1])
    ws = capi.mla_sparse_workspace_bytes(ps)
    n_split = max(1, ws and capi.mla_sparse_num_splits(_with_ws(ps, ws)))
    pd = capi.mla_params(q, small[0][0], o, lse, cs, block_table=small[0][1])
    wsd = capi.mla_workspace_bytes(pd)
    n_split_d = max(1, wsd and capi.mla_num_splits(_with_ws(pd, wsd)))
    lo, hi = sorted((ms["dense"], ms["dense_again"]))
    line = dict(mla_sparse=True, b=b, h=h, topk=topk, seqlen_q=1, dtype="bfloat16", page_block_size=page, caches_rotated=n, lists_rotated=n_lists,
                read_mb=round(read_bytes / 1e6, 2), n_split_sparse=n_split, n_split_dense=n_split_d,
                ms={k: round(v, 5) for k, v in ms.items()}, dense_spread=round(hi / lo, 4),
                over_dense={k: round(v / ms["dense"], 4) for k, v in ms.items() if k != "dense"},
                frac_of_6p3={k: round(read_bytes / (v * 1e-3) / HBM_ACHIEVABLE, 4) for k, v in ms.items()})
    yield line
    if b <= 8:
        forced = {"auto": arm_i}
        for ns in (8, 16, 32, 64):
            forced[f"splits{ns}"] = lambda i, ns=ns: arm_i(i, ns)
        forced["auto_again"] = arm_i
        for f in forced.values():
            f(0)
        torch.cuda.synchronize()
        ms = _interleaved(forced, n, rounds)
        lo, hi = sorted((ms["auto"], ms["auto_again"]))
        best = min((k for k in ms if k.startswith("splits")), key=lambda k: ms[k])
        yield dict(mla_sparse_forced_splits=True, b=b, h=h, topk=topk, page_block_size=page, n_split_auto=n_split, ms={k: round(v, 5) for k, v in ms.items()},
                   auto_spread=round(hi / lo, 4), best_forced=best, auto_over_best=round(lo / ms[best], 4), beats_auto_beyond_spread=bool(ms[best] * (hi / lo) < lo))
    del small, big, lists
    torch.cuda.empty_cache()


def run_mla_sparse(lengths, pages, rounds):
    for h, b in itertools.product((16, 128), (1, 8, 64)):
        yield from run_mla_sparse_point(b, h, tuple(lengths or (32768, 131072)), (pages or [64])[0], rounds)


def _mla_fp8_cache(shape_lead, dt, dev, seed):
    """(an FP8 latent cache (*lead, 1, 656) of random NaN-free codes under tile scales in [2^-8, 2^-6] with N(0, 1) rope elements, its dequantised 16-bit
    twin (*lead, 1, 576)), built a million rows at a time to bound the temporaries"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    total = shape_lead[0] * shape_lead[1]
    c8 = torch.empty(total, 656, device=dev, dtype=torch.uint8)
    c16 = torch.empty(total, 576, device=dev, dtype=dt)
    for r0 in range(0, total, 1 << 20):
        rows = min(1 << 20, total - r0)
        codes = torch.randint(0, 256, (rows, 512), device=dev, generator=gen, dtype=torch.int16)
        codes = torch.where((codes & 0x7F) == 0x7F, codes ^ 0x41, codes).to(torch.uint8)
        scale = torch.exp2(torch.rand(rows, 4, device=dev, generator=gen) * 2.0 - 8.0)
        rope = torch.randn(rows, 64, device=dev, generator=gen).to(dt)
        c8[r0:r0 + rows] = torch.cat([codes, scale.view(torch.uint8).view(rows, 16), rope.view(torch.uint8).view(rows, 128)], dim=-1)
        c16[r0:r0 + rows] = F.dequantize_mla_kv_cache(c8[r0:r0 + rows], dt)
    return c8.view(*shape_lead, 1, 656), c16.view(*shape_lead, 1, 576)


def run_mla_fp8_point(b, h, L, page, rounds):
    """(A) flash_mla_with_kvcache over an FP8 latent cache (656-byte rows), (B, B2) the same call over the dequantised bf16 cache, twice; interleaved.  The two
    give the same bits (asserted on the first cache)."""
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    b8, b16 = b * L * 656, b * L * 576 * 2
    n = _rotation(b8 + b16, b8)
    sets = []
    for i in range(n):
        if page:
            nb = b * L // page
            table = torch.randperm(nb, generator=torch.Generator().manual_seed(i)).view(b, L // page).to(device=dev, dtype=torch.int32)
            sets.append(_mla_fp8_cache((nb, page), dt, dev, i) + (table,))
        else:
            sets.append(_mla_fp8_cache((b, L), dt, dev, i) + (None,))
    q = torch.randn(b, 1, h, 576, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    fp8 = lambda i: F.flash_mla_with_kvcache(q, sets[i][0], cs, block_table=sets[i][2])
    ref = lambda i: F.flash_mla_with_kvcache(q, sets[i][1], cs, block_table=sets[i][2])
    assert _bits_equal(fp8(0), ref(0)), "the FP8 call is not the 16-bit call on the dequantised cache"
    torch.cuda.synchronize()
    ms = _interleaved({"bf16": ref, "fp8": fp8, "bf16_again": ref}, n, rounds)
    p = capi.mla_params(q, sets[0][0], torch.empty(b, 1, h, 512, device=dev, dtype=dt), torch.empty(b, h, 1, device=dev), cs, block_table=sets[0][2])
    ws = capi.mla_workspace_bytes(p)
    n_split = max(1, ws and capi.mla_num_splits(_with_ws(p, ws)))
    del sets
    torch.cuda.empty_cache()
    lo, hi = sorted((ms["bf16"], ms["bf16_again"]))
    return dict(mla_fp8=True, b=b, h=h, L=L, seqlen_q=1, dtype="bfloat16", page_block_size=page or 0, caches_rotated=n, kv_gb_fp8=round(b8 / 1e9, 3),
                kv_gb_bf16=round(b16 / 1e9, 3), n_split=n_split, ms_fp8=round(ms["fp8"], 5), ms_bf16=round(ms["bf16"], 5), ms_bf16_again=round(ms["bf16_again"], 5),
                frac_of_6p3_fp8=round(b8 / (ms["fp8"] * 1e-3) / HBM_ACHIEVABLE, 3), frac_of_6p3_bf16=round(b16 / (ms["bf16"] * 1e-3) / HBM_ACHIEVABLE, 3),
                fp8_over_bf16=round(ms["fp8"] / ms["bf16"], 4), bf16_again_over_bf16=round(ms["bf16_again"] / ms["bf16"], 4), inside_scatter=bool(lo <= ms["fp8"] <= hi))


def run_mla_fp8(lengths, pages, rounds):
    for h, b, L in itertools.product((16, 128), (1, 8, 64), tuple(lengths or (4096, 32768, 131072))):
        for page in ([None] + list(pages or [])):
            yield run_mla_fp8_point(b, h, L, page, rounds)


def run_mla_sparse_fp8_point(b, h, lengths, page, rounds, topk=2048):
    """per L, sorted and unsorted random lists of topk positions over one paged cache of L rows: the sparse call over the FP8 cache against the same call over
    the dequantised bf16 cache, the bf16 sorted arm of the first L timed twice; interleaved.  The two give the same bits (asserted per L)."""
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    n_lists = 4
    gen = torch.Generator().manual_seed(1234 + b + h)
    q = torch.randn(b, 1, h, 576, device=dev, dtype=dt)
    arms, keep = {}, []
    for L in lengths:
        nb = b * L // page
        table = torch.randperm(nb, generator=torch.Generator().manual_seed(1000 + L)).view(b, L // page).to(device=dev, dtype=torch.int32)
        c8, c16 = _mla_fp8_cache((nb, page), dt, dev, L)
        pos = torch.stack([torch.stack([torch.randperm(L, generator=gen)[:topk] for _ in range(b)]) for _ in range(n_lists)]).to(torch.int32).unsqueeze(2)
        srt, uns = pos.sort(-1).values.to(dev), pos.to(dev)
        csL = torch.full((b,), L, dtype=torch.int32, device=dev)
        keep.append((c8, c16, table, srt, uns, csL))
        for name, cache in (("bf16", c16), ("fp8", c8)):
            arms[f"{name}_sorted_L{L}"] = lambda i, cache=cache, table=table, srt=srt, csL=csL: F.flash_mla_sparse_with_kvcache(q, cache, csL, srt[i % n_lists], block_table=table)
            arms[f"{name}_unsorted_L{L}"] = lambda i, cache=cache, table=table, uns=uns, csL=csL: F.flash_mla_sparse_with_kvcache(q, cache, csL, uns[i % n_lists], block_table=table)
        assert _bits_equal(arms[f"fp8_unsorted_L{L}"](0), arms[f"bf16_unsorted_L{L}"](0)), "the FP8 call is not the 16-bit call on the dequantised cache"
    first = f"bf16_sorted_L{lengths[0]}"
    arms["bf16_again"] = arms[first]
    torch.cuda.synchronize()
    ms = _interleaved(arms, n_lists, rounds)
    lo, hi = sorted((ms[first], ms["bf16_again"]))
    del keep
    torch.cuda.empty_cache()
    return dict(mla_sparse_fp8=True, b=b, h=h, topk=topk, seqlen_q=1, dtype="bfloat16", page_block_size=page, lists_rotated=n_lists,
                read_mb_fp8=round(b * topk * 656 / 1e6, 2), read_mb_bf16=round(b * topk * 1152 / 1e6, 2), ms={k: round(v, 5) for k, v in ms.items()},
                bf16_spread=round(hi / lo, 4),
                fp8_over_bf16={k[4:]: round(ms[k] / ms["bf16" + k[3:]], 4) for k in ms if k.startswith("fp8_")})


def run_mla_sparse_fp8(lengths, pages, rounds):
    for h, b in itertools.product((16, 128), (1, 8, 64)):
        yield run_mla_sparse_fp8_point(b, h, tuple(lengths or (32768, 131072)), (pages or [64])[0], rounds)


def run_mla_indexer_point(b, L, page, rounds, topk=2048, h=64):
    """the logits call, the torch formulation of it (twice), the selection and torch.topk on the same logits; interleaved"""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(b * 1000003 + L)
    kbytes = b * L * 132
    n = max(1, min(512, math.ceil(WORKING_SET / kbytes)))
    cols = L // page
    q = torch.randn(b, 1, h, 128, device=dev, generator=gen).to(torch.bfloat16)
    w = torch.randn(b, 1, h, device=dev, generator=gen) * (h ** -0.5)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    sets = []
    for _ in range(n):
        pool = torch.randn(b * cols, page, 128, device=dev, generator=gen).to(torch.float8_e4m3fn)
        scales = torch.rand(b * cols, page, device=dev, generator=gen) + 0.5
        table = torch.randperm(b * cols, device=dev, generator=gen).to(torch.int32).view(b, cols)
        sets.append((pool, scales, table))
    ours = lambda i: F.flash_mla_indexer_logits(q, w, sets[i % n][0], cs, k_scale=sets[i % n][1], block_table=sets[i % n][2], causal=True)

    def torch_logits(i):
        pool, scales, _ = sets[i % n]
        kf = pool.view(b, L, 128).to(torch.bfloat16)
        s = torch.einsum("bthd,bjd->bthj", q, kf).float()
        return torch.einsum("bth,bthj->btj", w, torch.relu(s)) * scales.view(b, 1, L)

    logits = [ours(i) for i in range(min(n, 8))]
    sel = lambda i: F.flash_mla_indexer_topk(logits[i % len(logits)], cs, topk, causal=True)
    tsel = lambda i: torch.topk(logits[i % len(logits)], topk, dim=-1).indices
    # what is timed computes the same thing: the selected sets agree wherever the logits have no equal entries at the threshold
    same = bool(torch.equal(torch.sort(tsel(0), dim=-1).values.int(), sel(0)))
    ms = _interleaved({"logits": ours, "torch_logits": torch_logits, "torch_logits_again": torch_logits, "topk": sel, "torch_topk": tsel}, n, rounds)
    tbs = kbytes / (ms["logits"] * 1e-3) / 1e12
    return dict(mla_indexer=True, b=b, L=L, h=h, topk=topk, seqlen_q=1, dtype="bfloat16", k_format="fp8_e4m3+scale", page_block_size=page, caches_rotated=n,
                ms={k: round(v, 5) for k, v in ms.items()}, key_bytes=kbytes, logits_tb_s=round(tbs, 3), logits_fraction_of_6p3_tb_s=round(tbs * 1e12 / HBM_ACHIEVABLE, 3),
                torch_logits_over_logits=round(ms["torch_logits"] / ms["logits"], 2), torch_noise=round(ms["torch_logits_again"] / ms["torch_logits"], 3),
                torch_topk_over_topk=round(ms["torch_topk"] / ms["topk"], 2),
                torch_total_over_total=round((ms["torch_logits"] + ms["torch_topk"]) / (ms["logits"] + ms["topk"]), 2), same_selection=same)


def run_mla_indexer(lengths, pages, rounds):
    for b, L in itertools.product((1, 8, 64), tuple(lengths or (4096, 32768, 131072))):
        yield run_mla_indexer_point(b, L, (pages or [64])[0], rounds)


def run_mla_indexer_prefill_point(sq, L, page, rounds, topk=2048, h=64):
    """the prefill logits call against the decode logits call (timed twice: its own scatter) on one prompt chunk, and the selection launch; interleaved, bits asserted first"""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(sq * 1000003 + L)
    cols = L // page
    q = torch.randn(1, sq, h, 128, device=dev, generator=gen).to(torch.bfloat16)
    w = torch.randn(1, sq, h, device=dev, generator=gen) * (h ** -0.5)
    cs = torch.full((1,), L, dtype=torch.int32, device=dev)
    pool = torch.randn(cols, page, 128, device=dev, generator=gen).to(torch.float8_e4m3fn)
    scales = torch.rand(cols, page, device=dev, generator=gen) + 0.5
    table = torch.randperm(cols, device=dev, generator=gen).to(torch.int32).view(1, cols)
    kw = dict(k_scale=scales, block_table=table, causal=True)
    new = lambda: F.flash_mla_indexer_prefill_logits(q, w, pool, cs, **kw)
    old = lambda: F.flash_mla_indexer_logits(q, w, pool, cs, **kw)
    visible = torch.arange(L, device=dev).view(1, 1, L) < (L - sq + 1 + torch.arange(sq, device=dev)).clamp(0, L).view(1, sq, 1)
    lg = new()
    same = bool(torch.equal(lg.view(torch.int32)[visible], old().view(torch.int32)[visible]))
    assert same, "the prefill logits differ from the decode call's"
    p = capi.mla_indexer_params(q, w, pool, lg, cs, k_scale=scales, block_table=table, causal=True)
    tq, wg_keys, n_chunks = capi.mla_indexer_prefill_launch(p)
    sel = lambda: F.flash_mla_indexer_topk(lg, cs, topk, causal=True)
    ms = _mlap_time({"prefill_logits": new, "logits": old, "logits_again": old, "topk": sel}, rounds)
    pairs = int(visible.sum())                  # (token, key) pairs under the mask
    flop = pairs * h * 128 * 2
    del visible
    return dict(mla_indexer_prefill=True, b=1, seqlen_q=sq, L=L, h=h, topk=topk, dtype="bfloat16", k_format="fp8_e4m3+scale", page_block_size=page, tokens_per_wg=tq,
                wg_keys=wg_keys, n_chunks=n_chunks, ms={k: round(v, 5) for k, v in ms.items()}, prefill_over_logits=round(ms["prefill_logits"] / ms["logits"], 4),
                logits_noise=round(ms["logits_again"] / ms["logits"], 4), token_key_pairs=pairs, prefill_tflops=round(flop / (ms["prefill_logits"] * 1e-3) / 1e12, 1),
                logits_tflops=round(flop / (ms["logits"] * 1e-3) / 1e12, 1), bit_identical=same)


def run_mla_indexer_prefill(lengths, pages, rounds):
    for sq, L in itertools.product((128, 512, 2048), tuple(lengths or (4096, 32768, 131072))):
        yield run_mla_indexer_prefill_point(sq, L, (pages or [64])[0], rounds)
        torch.cuda.empty_cache()


def _fp8q_exact_bits(fn, h, page, dev):
    """before timing: on integer data (every partial sum an integer below 2^24) the FP8-q call `fn` gives the bits of the same call on q.to(bfloat16)"""
    gen = torch.Generator(device=dev).manual_seed(7)
    sq, L = 9, 4 * page
    q8 = torch.randint(-8, 9, (1, sq, h, 128), device=dev, generator=gen).float().to(torch.float8_e4m3fn)
    pool = torch.randint(-8, 9, (4, page, 128), device=dev, generator=gen).float().to(torch.float8_e4m3fn)
    w = 2.0 ** torch.randint(-2, 3, (1, sq, h), device=dev, generator=gen).float()
    sc = 2.0 ** torch.randint(-3, 4, (4, page), device=dev, generator=gen).float()
    cs = torch.full((1,), L - 5, dtype=torch.int32, device=dev)
    table = torch.randperm(4, device=dev, generator=gen).to(torch.int32).view(1, 4)
    kw = dict(k_scale=sc, block_table=table, causal=True)
    n = (L - 5 - sq + 1 + torch.arange(sq, device=dev)).view(1, sq, 1)
    vis = torch.arange(L, device=dev).view(1, 1, L) < n
    return bool(torch.equal(fn(q8, w, pool, cs, **kw).view(torch.int32)[vis], fn(q8.to(torch.bfloat16), w, pool, cs, **kw).view(torch.int32)[vis]))


def run_mla_indexer_fp8q_point(b, L, page, rounds, h=64):
    """--mla-indexer --q-dtype fp8: the decode logits call on e4m3 queries against the same call on the widened (bf16) queries over the same caches (timed twice);
    interleaved, caches rotated over the working set"""
    dev = torch.device("cuda:0")
    exact = _fp8q_exact_bits(F.flash_mla_indexer_logits, h, page, dev)
    assert exact, "on integer data the FP8-q logits differ from the bf16-q call's"
    gen = torch.Generator(device=dev).manual_seed(b * 1000003 + L)
    kbytes = b * L * 132
    n = max(1, min(512, math.ceil(WORKING_SET / kbytes)))
    cols = L // page
    q8 = torch.randn(b, 1, h, 128, device=dev, generator=gen).to(torch.float8_e4m3fn)
    q16 = q8.to(torch.bfloat16)
    w = torch.randn(b, 1, h, device=dev, generator=gen) * (h ** -0.5)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    sets = []
    for _ in range(n):
        pool = torch.randn(b * cols, page, 128, device=dev, generator=gen).to(torch.float8_e4m3fn)
        scales = torch.rand(b * cols, page, device=dev, generator=gen) + 0.5
        table = torch.randperm(b * cols, device=dev, generator=gen).to(torch.int32).view(b, cols)
        sets.append((pool, scales, table))
    call = lambda q: (lambda i: F.flash_mla_indexer_logits(q, w, sets[i % n][0], cs, k_scale=sets[i % n][1], block_table=sets[i % n][2], causal=True))
    ms = _interleaved({"fp8q_logits": call(q8), "bf16q_logits": call(q16), "bf16q_logits_again": call(q16)}, n, rounds)
    tbs = {k: kbytes / (v * 1e-3) / 1e12 for k, v in ms.items()}
    flop = b * L * h * 128 * 2
    return dict(mla_indexer_fp8q=True, b=b, L=L, h=h, seqlen_q=1, q_format="fp8_e4m3", k_format="fp8_e4m3+scale", page_block_size=page, caches_rotated=n,
                ms={k: round(v, 5) for k, v in ms.items()}, fp8q_over_bf16q=round(ms["fp8q_logits"] / ms["bf16q_logits"], 4),
                bf16q_noise=round(ms["bf16q_logits_again"] / ms["bf16q_logits"], 4), key_bytes=kbytes,
                fp8q_fraction_of_6p3_tb_s=round(tbs["fp8q_logits"] * 1e12 / HBM_ACHIEVABLE, 3), bf16q_fraction_of_6p3_tb_s=round(tbs["bf16q_logits"] * 1e12 / HBM_ACHIEVABLE, 3),
                fp8q_tflops=round(flop / (ms["fp8q_logits"] * 1e-3) / 1e12, 1), bf16q_tflops=round(flop / (ms["bf16q_logits"] * 1e-3) / 1e12, 1), exact_bits=exact)


def run_mla_indexer_prefill_fp8q_point(sq, L, page, rounds, h=64):
    """--mla-indexer-prefill --q-dtype fp8: the prefill logits call on e4m3 queries against the same call on the widened (bf16) queries over the same cache (timed twice)"""
    dev = torch.device("cuda:0")
    exact = _fp8q_exact_bits(F.flash_mla_indexer_prefill_logits, h, page, dev)
    assert exact, "on integer data the FP8-q prefill logits differ from the bf16-q call's"
    gen = torch.Generator(device=dev).manual_seed(sq * 1000003 + L)
    cols = L // page
    q8 = torch.randn(1, sq, h, 128, device=dev, generator=gen).to(torch.float8_e4m3fn)
    q16 = q8.to(torch.bfloat16)
    w = torch.randn(1, sq, h, device=dev, generator=gen) * (h ** -0.5)
    cs = torch.full((1,), L, dtype=torch.int32, device=dev)
    pool = torch.randn(cols, page, 128, device=dev, generator=gen).to(torch.float8_e4m3fn)
    scales = torch.rand(cols, page, device=dev, generator=gen) + 0.5
    table = torch.randperm(cols, device=dev, generator=gen).to(torch.int32).view(1, cols)
    kw = dict(k_scale=scales, block_table=table, causal=True)
    new = lambda: F.flash_mla_indexer_prefill_logits(q8, w, pool, cs, **kw)
    old = lambda: F.flash_mla_indexer_prefill_logits(q16, w, pool, cs, **kw)
    ms = _mlap_time({"fp8q_prefill_logits": new, "bf16q_prefill_logits": old, "bf16q_prefill_logits_again": old}, rounds)
    n_t = (L - sq + 1 + torch.arange(sq)).clamp(0, L)
    pairs = int(n_t.sum())                      # (token, key) pairs under the mask
    flop = pairs * h * 128 * 2
    return dict(mla_indexer_prefill_fp8q=True, b=1, seqlen_q=sq, L=L, h=h, q_format="fp8_e4m3", k_format="fp8_e4m3+scale", page_block_size=page,
                ms={k: round(v, 5) for k, v in ms.items()}, fp8q_over_bf16q=round(ms["fp8q_prefill_logits"] / ms["bf16q_prefill_logits"], 4),
                bf16q_noise=round(ms["bf16q_prefill_logits_again"] / ms["bf16q_prefill_logits"], 4), token_key_pairs=pairs,
                fp8q_tflops=round(flop / (ms["fp8q_prefill_logits"] * 1e-3) / 1e12, 1), bf16q_tflops=round(flop / (ms["bf16q_prefill_logits"] * 1e-3) / 1e12, 1),
                exact_bits=exact)


def run_mla_indexer_fp8q(lengths, pages, rounds, prefill):
    grid = itertools.product((128, 512, 2048) if prefill else (1, 8, 64), tuple(lengths or (4096, 32768, 131072)))
    for x, L in grid:
        yield (run_mla_indexer_prefill_fp8q_point if prefill else run_mla_indexer_fp8q_point)(x, L, (pages or [64])[0], rounds)
        torch.cuda.empty_cache()


def _mlap_time(fns, rounds, iters=3):
    """median ms per call of each arm, the arms taken in turn within every round, `iters` calls per timed batch"""
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) / iters)
    return {k: statistics.median(v) for k, v in t.items()}


def run_mla_prefill_point(b, h, sq, sk, causal, rounds, base=None):
    """flash_mla_prefill_func against fwd at head_dim 128 and against the zero-padded head_dim-256 KV-cache call, each yardstick twice; or, with a baseline
    library, the C ABI call of this build (twice) against the baseline's"""
    dev, dt = torch.device("cuda:0"), torch.bfloat16
    scale = 192 ** -0.5
    q, k, v = (torch.randn(b, s, h, d, device=dev, dtype=dt) for s, d in ((sq, 192), (sk, 192), (sk, 128)))
    flops = 2.0 * sq * sk * h * (192 + 128) * b * (0.5 if causal else 1.0)
    row = dict(mla_prefill=True, b=b, h=h, sq=sq, sk=sk, causal=bool(causal), dtype="bfloat16")
    if base is not None:
        o, lse = torch.empty(b, sq, h, 128, device=dev, dtype=dt), torch.empty(b, h, sq, device=dev)
        o2, lse2 = torch.empty_like(o), torch.empty_like(lse)
        p, p2 = capi.mla_prefill_params(q, k, v, o, lse, causal=causal), capi.mla_prefill_params(q, k, v, o2, lse2, causal=causal)
        stream = torch.cuda.current_stream().cuda_stream
        base.fa_run_mla_prefill_fwd.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        mine = lambda: capi.check(capi.lib().fa_run_mla_prefill_fwd(ctypes.byref(p), stream))
        other = lambda: base.fa_run_mla_prefill_fwd(ctypes.byref(p2), stream)
        mine(), other()
        torch.cuda.synchronize()
        err = float((o.float() - o2.float()).abs().max())
        ms = _mlap_time({"this": mine, "baseline": other, "this_again": mine}, rounds)
        row.update(ms_this=round(ms["this"], 5), ms_this_again=round(ms["this_again"], 5), ms_baseline=round(ms["baseline"], 5),
                   baseline_over_this=round(ms["baseline"] / ms["this"], 4), again_over_this=round(ms["this_again"] / ms["this"], 4),
                   tflops_this=round(flops / (ms["this"] * 1e-3) / 1e12, 1), tflops_baseline=round(flops / (ms["baseline"] * 1e-3) / 1e12, 1), max_abs_diff=round(err, 5))
        return row
    q1, k1, v1 = (torch.randn(b, s, h, 128, device=dev, dtype=dt) for s in (sq, sk, sk))
    pad = lambda t: torch.nn.functional.pad(t, (0, 256 - t.shape[-1]))
    q2, k2, v2 = pad(q), pad(k), pad(v)
    new = lambda: F.flash_mla_prefill_func(q, k, v, causal=causal)
    fwd = lambda: F.fwd(q1, k1, v1, causal)
    old = lambda: F.flash_attn_with_kvcache(q2, k2, v2, causal=causal, softmax_scale=scale)
    # (the padded call has limits of its own: one sequence of its cache must span less than 2^31 bytes, which h 128 x 256 columns reach at 32768 keys)
    arms = {"fwd128": fwd, "pad256": old, "new": new, "fwd128_again": fwd, "pad256_again": old}
    if sk * h * 256 * 2 >= 1 << 31:
        arms = {k_: f for k_, f in arms.items() if not k_.startswith("pad256")}
        err = float("nan")
    else:
        err = float((new().float() - old()[..., :128].float()).abs().max())
    fwd(), new()
    torch.cuda.synchronize()
    ms = _mlap_time(arms, rounds)
    del q2, k2, v2
    torch.cuda.empty_cache()
    if "pad256" not in ms:
        row.update(ms_new=round(ms["new"], 5), ms_fwd128=round(ms["fwd128"], 5), ms_fwd128_again=round(ms["fwd128_again"], 5), ms_pad256=None,
                   tflops_new=round(flops / (ms["new"] * 1e-3) / 1e12, 1), tflops_fwd128=round(0.8 * flops / (ms["fwd128"] * 1e-3) / 1e12, 1),
                   new_over_fwd128=round(ms["new"] / ms["fwd128"], 4), fwd128_again_over_fwd128=round(ms["fwd128_again"] / ms["fwd128"], 4),
                   pad256_refused="one sequence of the padded cache spans 2^31 bytes or more")
        return row
    row.update(ms_new=round(ms["new"], 5), ms_fwd128=round(ms["fwd128"], 5), ms_fwd128_again=round(ms["fwd128_again"], 5), ms_pad256=round(ms["pad256"], 5),
               ms_pad256_again=round(ms["pad256_again"], 5), tflops_new=round(flops / (ms["new"] * 1e-3) / 1e12, 1),
               tflops_fwd128=round(0.8 * flops / (ms["fwd128"] * 1e-3) / 1e12, 1), new_over_fwd128=round(ms["new"] / ms["fwd128"], 4),
               fwd128_again_over_fwd128=round(ms["fwd128_again"] / ms["fwd128"], 4), new_over_pad256=round(ms["new"] / ms["pad256"], 4),
               pad256_again_over_pad256=round(ms["pad256_again"] / ms["pad256"], 4), max_abs_diff_to_pad256=round(err, 5))
    return row


def run_mla_prefill(quick, rounds, base=None):
    shapes = [(s, s, True) for s in (512, 2048, 8192)] + [(2048, 8192, False), (2048, 32768, False)]
    for h, b in itertools.product((16, 128), (1,) if quick else (1, 4)):
        for sq, sk, causal in shapes:
            if quick and h == 128 and max(sq, sk) > 2048:
                continue
            yield run_mla_prefill_point(b, h, sq, sk, causal, rounds, base)


def run_mla_prefill_bwd_point(b, h, sq, sk, causal, rounds):
    """flash_mla_prefill_bwd (both launches, and each alone) against (a) bwd at head_dim 128 on the same b, s, h and (b) autograd's backward of the torch
    formulation (einsum, masked softmax, einsum) in bf16 where its score matrices fit; each yardstick twice"""
    from flash_attn_turing import _C

    dev, dt = torch.device("cuda:0"), torch.bfloat16
    scale = 192 ** -0.5
    q, k, v = (torch.randn(b, s, h, d, device=dev, dtype=dt) for s, d in ((sq, 192), (sk, 192), (sk, 128)))
    dout = torch.randn(b, sq, h, 128, device=dev, dtype=dt)
    flops = 2.0 * sq * sk * h * (3 * 192 + 2 * 128) * b * (0.5 if causal else 1.0)
    row = dict(mla_prefill_bwd=True, b=b, h=h, sq=sq, sk=sk, causal=bool(causal), dtype="bfloat16")
    out, lse = F.flash_mla_prefill_func(q, k, v, causal=causal, return_softmax_lse=True)
    dsum = _C.bwd_mla_prefill(dout, q, k, v, out, lse, None, None, causal, None)[3]
    new = lambda: F.flash_mla_prefill_bwd(dout, q, k, v, out, lse, causal=causal)
    dq_only = lambda: _C.bwd_mla_prefill(dout, q, k, v, out, lse, None, None, causal, None, 1, dsum)
    dkdv_only = lambda: _C.bwd_mla_prefill(dout, q, k, v, out, lse, None, None, causal, None, 2, dsum)
    q1, k1, v1, do1 = (torch.randn(b, s, h, 128, device=dev, dtype=dt) for s in (sq, sk, sk, sq))
    o1, l1 = F.fwd(q1, k1, v1, causal)
    bwd = lambda: F.bwd(q1, k1, v1, o1, l1, do1, causal)
    arms = {"bwd128": bwd, "new": new, "dq": dq_only, "dkdv": dkdv_only, "bwd128_again": bwd}
    if b * h * sq * sk <= 1 << 30:
        with torch.enable_grad():
            ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
            s_ = torch.einsum("bthd,bjhd->bhtj", ql, kl) * scale
            if causal:
                s_ = s_.masked_fill(torch.arange(sk, device=dev).view(1, -1) > sk - sq + torch.arange(sq, device=dev).view(-1, 1), float("-inf"))
            o_t = torch.einsum("bhtj,bjhd->bthd", torch.softmax(s_, dim=-1), vl)
        ref = lambda: torch.autograd.grad(o_t, (ql, kl, vl), dout, retain_graph=True)
        arms.update(torch=ref, torch_again=ref)
        row["rel_diff_to_torch"] = [round(float((x.double() - y.double()).norm() / y.double().norm()), 5) for x, y in zip(new(), ref())]
    bwd(), new()
    torch.cuda.synchronize()
    ms = _mlap_time(arms, rounds)
    row.update({f"ms_{n}": round(t, 5) for n, t in ms.items()})
    row.update(tflops_new=round(flops / (ms["new"] * 1e-3) / 1e12, 1), tflops_bwd128=round(640.0 / 832.0 * flops / (ms["bwd128"] * 1e-3) / 1e12, 1),
               new_over_bwd128=round(ms["new"] / ms["bwd128"], 4), bwd128_again_over_bwd128=round(ms["bwd128_again"] / ms["bwd128"], 4),
               dq_plus_dkdv_over_new=round((ms["dq"] + ms["dkdv"]) / ms["new"], 4))
    if "torch" in ms:
        row.update(new_over_torch=round(ms["new"] / ms["torch"], 4), torch_again_over_torch=round(ms["torch_again"] / ms["torch"], 4))
    else:
        row["torch_skipped"] = "the score matrices of the torch formulation exceed 2^30 elements"
    return row


def run_mla_prefill_bwd(quick, rounds):
    """the grid of --mla-prefill"""
    shapes = [(s, s, True) for s in (512, 2048, 8192)] + [(2048, 8192, False), (2048, 32768, False)]
    for h, b in itertools.product((16, 128), (1,) if quick else (1, 4)):
        for sq, sk, causal in shapes:
            if quick and h == 128 and max(sq, sk) > 2048:
                continue
            yield run_mla_prefill_bwd_point(b, h, sq, sk, causal, rounds)


def run_merge_point(n, dv, rows, rounds, h=4, dt=torch.bfloat16):
    """flash_attn_merge_states alone on `n` contiguous parts of (rows, h, d_v) against the torch formulation of the same merge (the five ops README.md printed
    before the call existed, folded over the parts; timed twice: its noise figure); bytes moved = n parts read + one written, out and lse, against 6.3 TB/s"""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(n * 1000 + dv)
    outs = [torch.randn(rows, h, dv, device=dev, dtype=dt, generator=gen) for _ in range(n)]
    lses = [torch.randn(h, rows, device=dev, generator=gen) * 4 for _ in range(n)]

    def torch_merge():
        lse = lses[0]
        for l in lses[1:]:
            lse = torch.logaddexp(lse, l)
        acc = None
        for o, l in zip(outs, lses):
            term = torch.exp(l - lse).t().unsqueeze(-1) * o.float()
            acc = term if acc is None else acc + term
        return acc.to(dt), lse

    ours = lambda: F.flash_attn_merge_states(outs, lses)
    a, b_ = ours(), torch_merge()
    diff = float((a[0].float() - b_[0].float()).abs().max())
    ms = _mlap_time({"torch": torch_merge, "merge": ours, "torch_again": torch_merge}, rounds, iters=5)
    nbytes = (n + 1) * (rows * h * dv * 2 + rows * h * 4)
    return dict(mode="merge", n_parts=n, d_v=dv, rows=rows, h=h, dtype=str(dt).replace("torch.", ""), mbytes=round(nbytes / 2 ** 20, 1), ms_merge=round(ms["merge"], 4),
                tb_s=round(nbytes / ms["merge"] / 1e9, 3), frac_of_6p3=round(nbytes / ms["merge"] / 1e9 / 6.3, 3), ms_torch=round(ms["torch"], 4),
                ms_torch_again=round(ms["torch_again"], 4), merge_over_torch=round(ms["merge"] / ms["torch"], 3), max_abs_diff=diff)


def run_merge(quick, rounds):
    for n in (2, 4, 8):
        for dv in (128, 512):
            for rows in ((4096, 65536) if quick else (4096, 16384, 65536, 262144, 1048576)):
                if ((n + 1) * 2 + 3 * 4) * rows * 4 * dv > (40 << 30):          # (parts, result and the torch formulation's fp32 terms: skip what would take over 40 GiB)
                    continue
                yield run_merge_point(n, dv, rows, rounds)


def run_shared_prefix_point(b, prefix, fp8, rounds, own=128, h=32, hk=8, d=128, page=16, dt=torch.float16):
    """flash_attn_with_shared_prefix against flash_attn_with_kvcache on the same tables (timed twice: its noise figure): sq 1, pages of 16, a shared prefix and
    `own` keys per sequence"""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(b * 7 + prefix)
    n_pre, n_own = prefix // page, own // page
    nb = n_pre + b * n_own
    kp, vp = (torch.randn(nb, page, hk, d, device=dev, dtype=dt, generator=gen) for _ in range(2))
    kw = {}
    if fp8:
        kp, vp = kp.to(torch.float8_e4m3fn), vp.to(torch.float8_e4m3fn)
        kw = dict(k_descale=torch.full((b, hk), 0.5, device=dev), v_descale=torch.full((b, hk), 0.5, device=dev))
    perm = torch.randperm(nb, device=dev, generator=gen)
    table = torch.cat([perm[:n_pre].unsqueeze(0).expand(b, n_pre), perm[n_pre:].view(b, n_own)], dim=1).to(torch.int32).contiguous()
    q = torch.randn(b, 1, h, d, device=dev, dtype=dt, generator=gen)
    cs = torch.full((b,), prefix + own, dtype=torch.int32, device=dev)
    new = lambda: F.flash_attn_with_shared_prefix(q, kp, vp, prefix, cache_seqlens=cs, block_table=table, **kw)
    plain = lambda: F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table, **kw)
    diff = float((new().float() - plain().float()).abs().max())
    ms = _mlap_time({"plain": plain, "shared_prefix": new, "plain_again": plain}, rounds, iters=5)
    return dict(mode="shared_prefix", b=b, seqlen_q=1, h=h, h_k=hk, d=d, page=page, kv_dtype="fp8" if fp8 else "fp16", prefix=prefix, own=own,
                ms_shared_prefix=round(ms["shared_prefix"], 4), ms_plain=round(ms["plain"], 4), ms_plain_again=round(ms["plain_again"], 4),
                shared_over_plain=round(ms["shared_prefix"] / ms["plain"], 3), max_abs_diff=diff)


def run_shared_prefix(quick, rounds):
    for fp8 in (False, True):
        for b in (8, 64):
            for prefix in ((8192,) if quick else (2048, 8192, 32768)):
                yield run_shared_prefix_point(b, prefix, fp8, rounds)


def _io_point(mode, b, rows, ours, torch_form, same, nbytes, rounds):
    ms = _mlap_time({"torch": torch_form, "ours": ours, "torch_again": torch_form}, rounds, iters=3)
    return dict(mode=mode, b=b, rows_per_seq=rows, page=64, dtype="bfloat16", kv_dtype="fp8", mbytes=round(nbytes / 2 ** 20, 2), ms_ours=round(ms["ours"], 4),
                tb_s=round(nbytes / ms["ours"] / 1e9, 3), frac_of_6p3=round(nbytes / ms["ours"] / 1e9 / 6.3, 4), ms_torch=round(ms["torch"], 4),
                ms_torch_again=round(ms["torch_again"], 4), ours_over_torch=round(ms["ours"] / ms["torch"], 3), bits_equal=bool(same))


def run_mla_cache_io(quick, rounds, page=64, dt=torch.bfloat16):
    """flash_mla_cache_append, flash_mla_index_cache_append (1 and 2048 new rows a sequence) and flash_mla_cache_gather (4k and 32k rows a sequence) on FP8 caches
    in pages of 64, bf16, b in {1, 8, 64}, each against its torch formulation (timed twice: its noise figure): the quantiser in torch ops plus an indexed write
    through the table; a table gather plus dequantize_mla_kv_cache.  Bytes moved (rows read + rows written) / time against 6.3 TB/s"""
    dev = torch.device("cuda:0")
    for b in ((1, 8) if quick else (1, 8, 64)):
        gen = torch.Generator(device=dev).manual_seed(b)
        for s_new in (1, 2048):
            cols = 4096 // page
            nb = b * cols
            table = torch.randperm(nb, device=dev, generator=gen).view(b, cols).to(torch.int32)
            lens = torch.full((b,), 1000, dtype=torch.int32, device=dev)
            pos = lens.long().unsqueeze(1) + torch.arange(s_new, device=dev)
            slot = (table.long().gather(1, pos // page) * page + pos % page).flatten()
            kv_new = torch.randn(b, s_new, 1, 576, device=dev, generator=gen).to(dt)
            pool, pool_t = (torch.zeros(nb, page, 1, 656, dtype=torch.uint8, device=dev) for _ in range(2))

            def torch_append():
                pool_t.view(-1, 656)[slot] = F.quantize_mla_kv_cache(kv_new).view(-1, 656)

            ours = lambda: F.flash_mla_cache_append(pool, kv_new, lens, block_table=table)
            ours(), torch_append()
            # (bits against the quantiser run on the CPU: run on the GPU, quantize_mla_kv_cache's `/ 448.0` gave other bits in some scales - measured, pool != pool_t)
            pool_t.view(-1, 656)[slot] = F.quantize_mla_kv_cache(kv_new.cpu()).view(-1, 656).to(dev)
            yield _io_point("mla_cache_append", b, s_new, ours, torch_append, torch.equal(pool, pool_t), b * s_new * (1152 + 656), rounds)
            k_new = torch.randn(b, s_new, 128, device=dev, generator=gen).to(dt)
            kc, kc_t = (torch.zeros(nb, page, 128, dtype=torch.uint8, device=dev) for _ in range(2))
            ks, ks_t = (torch.zeros(nb, page, device=dev) for _ in range(2))

            def torch_index_append():
                codes, scale = F.quantize_mla_index_keys(k_new)
                kc_t.view(-1, 128)[slot] = codes.view(-1, 128)
                ks_t.view(-1)[slot] = scale.view(-1)

            ours = lambda: F.flash_mla_index_cache_append(kc, k_new, lens, k_scale=ks, block_table=table)
            ours(), torch_index_append()
            yield _io_point("mla_index_cache_append", b, s_new, ours, torch_index_append, torch.equal(kc, kc_t) and torch.equal(ks, ks_t), b * s_new * (256 + 132), rounds)
            del kv_new, pool, pool_t, k_new, kc, kc_t, ks, ks_t
        for n in ((4096,) if quick else (4096, 32768)):
            cols = n // page
            nb = b * cols
            pool = torch.randint(0, 120, (nb, page, 1, 656), dtype=torch.uint8, device=dev, generator=gen)      # codes below 0x78, scales and rope elements small and finite
            table = torch.randperm(nb, device=dev, generator=gen).view(b, cols).to(torch.int32)
            lens = torch.full((b,), n, dtype=torch.int32, device=dev)
            cu = torch.arange(0, b * n + 1, n, dtype=torch.int32, device=dev)
            out = torch.empty(b * n, 576, dtype=dt, device=dev)
            ours = lambda: F.flash_mla_cache_gather(pool, lens, out, block_table=table, cu_seqlens_out=cu)
            torch_gather = lambda: F.dequantize_mla_kv_cache(pool[table.long()].flatten(1, 2), dt).view(-1, 576)
            same = torch.equal(ours().view(torch.int16), torch_gather().view(torch.int16))
            yield _io_point("mla_cache_gather", b, n, ours, torch_gather, same, b * n * (656 + 1152), rounds)
            del pool, out
            torch.cuda.empty_cache()


def _baseline_lib(path):
    L = ctypes.CDLL(os.path.abspath(path))
    L.fa_run_mha_fwd_kvcache.argtypes = [ctypes.POINTER(capi.KvcacheParams), ctypes.c_void_p]
    L.fa_run_mha_fwd_kvcache.restype = ctypes.c_int
    L.fa_kvcache_workspace_bytes.argtypes = [ctypes.POINTER(capi.KvcacheParams)]
    L.fa_kvcache_workspace_bytes.restype = ctypes.c_int64
    L.fa_build_info.restype = ctypes.c_char_p
    return L


def run_ab_point(pt, base, rounds):
    """the plain call through this build's C ABI (A) and the baseline library's (B), interleaved, on the same caches"""
    dev = torch.device("cuda:0")
    b, h, hk, d, L, sq, dt = pt["b"], pt["h"], pt["h_k"], pt["d"], pt["L"], pt["seqlen_q"], pt["dtype"]
    kv_bytes = 2 * b * L * hk * d * 2
    n = _rotation(kv_bytes, kv_bytes)
    caches = [(torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2), torch.empty(b, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2))
              for _ in range(n)]
    q = torch.randn(b, sq, h, d, device=dev, dtype=dt)
    cs = torch.full((b,), L, dtype=torch.int32, device=dev)
    outs = {}
    libs = {"A": capi.lib(), "B": base}
    params = {}
    for tag, lib in libs.items():
        o, lse = torch.empty_like(q), torch.empty(b, h, sq, device=dev)
        ps = [capi.kvcache_params(q, kc, vc, o, lse, cache_seqlens=cs) for kc, vc in caches]
        ws = int(lib.fa_kvcache_workspace_bytes(ctypes.byref(ps[0])))
        buf = torch.empty(max(ws, 16) // 4, device=dev, dtype=torch.float32)
        for p in ps:
            p.workspace, p.workspace_bytes = (buf.data_ptr(), ws) if ws > 0 else (None, 0)
        params[tag] = (ps, o, lse, buf)
    stream = torch.cuda.current_stream().cuda_stream

    def call(tag):
        lib, (ps, _, _, _) = libs[tag], params[tag]
        return lambda i: capi.check(lib.fa_run_mha_fwd_kvcache(ctypes.byref(ps[i]), stream))

    fa, fb = call("A"), call("B")
    fa(0), fb(0)
    torch.cuda.synchronize()
    same = torch.equal(params["A"][1], params["B"][1]) and torch.equal(params["A"][2], params["B"][2])
    t_a, t_b = [], []
    for _ in range(rounds):
        t_a.append(time_rotation(fa, n, 20))
        t_b.append(time_rotation(fb, n, 20))
    ms_a, ms_b = statistics.median(t_a), statistics.median(t_b)
    del caches, params
    torch.cuda.empty_cache()
    return dict(b=b, h=h, h_k=hk, d=d, L=L, seqlen_q=sq, dtype=str(dt).replace("torch.", ""), kv_gb=round(kv_bytes / 1e9, 3), caches_rotated=n,
                ms_this=round(ms_a, 5), ms_baseline=round(ms_b, 5), this_over_baseline=round(ms_a / ms_b, 4), bit_identical=bool(same))


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
    ap.add_argument("--window", type=int, action="append", metavar="LEFT", help="sliding window (LEFT, 0), causal; repeat for several")
    ap.add_argument("--baseline-library", metavar="PATH", help="A/B of the plain call against this libflash_attn_gfx950.so")
    ap.add_argument("--kv-dtype", choices=("fp16", "fp8"), default="fp16", help="fp8: the 8-bit cache against the 16-bit call on the same logical cache")
    ap.add_argument("--length", type=int, action="append", metavar="L", help="cache length(s) instead of the grid's")
    ap.add_argument("--rotary", type=int, nargs="?", const=0, default=None, metavar="DIM",
                    help="the rotary call against the plain call on pre-rotated inputs and against a torch rotation (seqlen_q = 1 points; DIM = rotary_dim, default head_dim)")
    ap.add_argument("--rotary-neox", action="store_true", help="with --rotary: the non-interleaved (GPT-NeoX) pairing instead of the interleaved default")
    ap.add_argument("--ragged", action="store_true", help="ragged query batches (cu_seqlens_q): uniform batches against the dense call, mixed steps against a loop of dense calls, "
                                                          "long chunks against fwd")
    ap.add_argument("--softcap", type=float, default=None, metavar="CAP", help="the soft-capped call against the same call without the cap (timed twice); with --kv-dtype fp8 "
                                                                               "over the 8-bit cache")
    ap.add_argument("--softmax-scale", type=float, default=None, metavar="S", help="with --softcap: softmax_scale of both arms (default 1 / sqrt(head_dim))")
    ap.add_argument("--sinks", action="store_true", help="attention sinks on the gpt-oss shape (d 64, h 64 / h_k 8, window (127, 0) and full causal): the sink call against the "
                                                         "same call without sinks (timed twice); with --kv-dtype fp8 over the 8-bit cache, with --paged P through a block table")
    ap.add_argument("--tree", type=int, default=None, metavar="N", choices=(8, 32, 64), help="tree attention masks: the tree call under the binary-heap tree with seqlen_q = N against "
                                                                                             "the causal call of the same shape (timed twice); with --kv-dtype fp8 over the 8-bit cache")
    ap.add_argument("--prefill", action="store_true", help="the 64-row kernels for prompt chunks (prefill=True) against the 16-row kernels (timed twice) and, on the 16-bit "
                                                           "contiguous points, fwd; with --kv-dtype fp8 / --paged P over those caches")
    ap.add_argument("--head-dim", type=int, action="append", metavar="D", choices=(64, 128, 256), help="head dim(s) instead of the grid's 64 and 128 (256: the decode call only)")
    ap.add_argument("--equal-bytes", action="store_true", help="with --head-dim 256: the d-256 call against the d-128 call with twice the heads on the same buffers (timed twice)")
    ap.add_argument("--mla", action="store_true", help="MLA decode over a latent KV cache (flash_mla_with_kvcache) against the head_dim-256 decode call with one KV head "
                                                       "(timed twice); contiguous and, with --paged P, through a block table")
    ap.add_argument("--mla-sparse", action="store_true", help="sparse MLA decode (flash_mla_sparse_with_kvcache, topk 2048, pages of 64 or --paged P) against the dense MLA call "
                                                              "at L = topk (timed twice): the identity list, sorted and unsorted random positions of L in {32k, 128k}; forced splits")
    ap.add_argument("--mla-indexer", action="store_true", help="the DeepSeek-V3.2 indexer (flash_mla_indexer_logits / flash_mla_indexer_topk; bf16, FP8 keys with scales, 64 heads, "
                                                               "topk 2048, pages of 64 or --paged P): the logits call against its HBM bound and the torch formulation (timed twice), the "
                                                               "selection against torch.topk")
    ap.add_argument("--mla-indexer-prefill", action="store_true", help="flash_mla_indexer_prefill_logits against flash_mla_indexer_logits (timed twice) on one prompt chunk, and "
                                                                       "the selection launch: bf16, FP8 keys with scales, 64 heads, pages of 64, causal, b 1, sq in {128, 512, "
                                                                       "2048} x L in {4k, 32k, 128k}; bits asserted equal before timing")
    ap.add_argument("--q-dtype", choices=("bf16", "fp8"), default="bf16", help="with --mla-indexer / --mla-indexer-prefill, fp8: the call on e4m3 index queries against the same call "
                    "on the widened (bf16) queries over the same FP8 cache (timed twice), on the grids of the two tables; the bits asserted on integer data first")
    ap.add_argument("--mla-prefill", action="store_true", help="MLA prefill attention (flash_mla_prefill_func, bf16, h = h_k in {16, 128}) against fwd at head_dim 128 and "
                                                               "against the zero-padded head_dim-256 KV-cache call, each yardstick timed twice; with --baseline-library an A / B of "
                                                               "the call itself against that library")
    ap.add_argument("--mla-prefill-bwd", action="store_true", help="the MLA prefill backward (flash_mla_prefill_bwd, bf16, the grid of --mla-prefill): both launches and "
                                                                   "each alone against bwd at head_dim 128 and against autograd of the torch formulation, each timed twice")
    ap.add_argument("--merge", action="store_true", help="flash_attn_merge_states alone (2, 4, 8 parts; d_v 128, 512; 4k .. 1M rows of 4 heads, bf16): bytes moved / time "
                                                         "against 6.3 TB/s, next to the torch formulation of the merge (timed twice)")
    ap.add_argument("--shared-prefix", action="store_true", help="flash_attn_with_shared_prefix (b 8 / 64, sq 1, h 32 / h_k 8, d 128, pages of 16, 16-bit and FP8 caches, prefix "
                                                                 "2k / 8k / 32k, 128 own keys) against flash_attn_with_kvcache on the same tables (timed twice)")
    ap.add_argument("--mla-cache-io", action="store_true", help="flash_mla_cache_append / flash_mla_index_cache_append (1 and 2048 new rows a sequence) and "
                                                                "flash_mla_cache_gather (4k and 32k rows) on FP8 caches, pages of 64, bf16, b in {1, 8, 64}: bytes moved / "
                                                                "time against 6.3 TB/s, next to the torch formulation of each (timed twice)")
    a = ap.parse_args()
    base = _baseline_lib(a.baseline_library) if a.baseline_library else None
    print(json.dumps({"library": F.build_info(), "device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count}),
          flush=True)
    if base is not None:
        print(json.dumps({"baseline_library": base.fa_build_info().decode()}), flush=True)
    with torch.no_grad():
        if a.merge or a.shared_prefix or a.mla_cache_io:
            for line in (run_merge if a.merge else run_shared_prefix if a.shared_prefix else run_mla_cache_io)(a.quick, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if a.mla_prefill_bwd:
            for line in run_mla_prefill_bwd(a.quick, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if a.mla_prefill:
            for line in run_mla_prefill(a.quick, a.rounds, base):
                print(json.dumps(line), flush=True)
            return
        if a.ragged and base is None:
            for line in run_ragged(a.quick, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if (a.mla_indexer_prefill or a.mla_indexer) and a.q_dtype == "fp8":
            for line in run_mla_indexer_fp8q(a.length, a.paged, a.rounds, a.mla_indexer_prefill):
                print(json.dumps(line), flush=True)
            return
        if a.mla_indexer_prefill:
            for line in run_mla_indexer_prefill(a.length, a.paged, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if a.mla_indexer:
            for line in run_mla_indexer(a.length, a.paged, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if a.mla_sparse:
            for line in (run_mla_sparse_fp8 if a.kv_dtype == "fp8" else run_mla_sparse)(a.length, a.paged, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if a.mla:
            for line in (run_mla_fp8 if a.kv_dtype == "fp8" else run_mla)(a.length, a.paged, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if a.prefill:
            for line in run_prefill(a.length, a.head_dim, a.kv_dtype == "fp8", a.paged, a.rounds):
                print(json.dumps(line), flush=True)
            return
        if a.sinks:
            for pt in sinks_grid(a.quick, a.length):
                page = a.paged[0] if a.paged else 0
                row = run_sinks_point(pt, a.kv_dtype == "fp8", page, a.rounds) if base is None else run_sinks_ab_point(pt, base, a.kv_dtype == "fp8", page, a.rounds)
                print(json.dumps(row), flush=True)
            return
        if a.tree is not None:
            for pt in tree_grid(a.quick, a.tree, a.length, a.head_dim):
                fp8 = a.kv_dtype == "fp8"
                print(json.dumps(run_tree_point(pt, fp8, a.rounds) if base is None else run_tree_ab_point(pt, base, fp8, a.rounds)), flush=True)
            return
        for pt in grid(a.quick, a.length, a.head_dim):
            if a.equal_bytes:
                if pt["d"] == 256 and pt["seqlen_q"] == 1:
                    print(json.dumps(run_equal_bytes_point(pt, a.rounds)), flush=True)
            elif base is not None:
                print(json.dumps(run_ab_point(pt, base, a.rounds)), flush=True)
            elif a.softcap is not None:
                print(json.dumps(run_softcap_point(pt, a.softcap, a.softmax_scale, a.kv_dtype == "fp8", a.rounds)), flush=True)
            elif a.rotary is not None:
                if pt["seqlen_q"] == 1:
                    print(json.dumps(run_rotary_point(pt, a.rotary, not a.rotary_neox, a.rounds)), flush=True)
            elif a.kv_dtype == "fp8":
                print(json.dumps(run_fp8_point(pt, a.rounds)), flush=True)
            elif a.window:
                for left in a.window:
                    print(json.dumps(run_window_point(pt, left, a.rounds)), flush=True)
            elif a.paged:
                for page in a.paged:
                    print(json.dumps(run_paged_point(pt, page, a.rounds)), flush=True)
            else:
                print(json.dumps(run_point(pt, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
