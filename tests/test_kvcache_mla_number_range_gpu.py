"""GPU: MLA decode - flash_mla_with_kvcache, flash_mla_sparse_with_kvcache, 16-bit and FP8 latent caches - across the number range and past 32-bit offsets.

The other MLA suites draw q and the cache from N(0, 1), FP8 tile scales from [2^-12, 2^4], and allocate little; they pin WHICH keys are seen.  This file pins
what the kernels do with the NUMBERS: every finite 16-bit value, every e4m3 code under scales over the whole fp32 precondition, every tile amax of the
quantising append, a running max that moves, an inf that reaches the score and not the value, and addresses past 2^31 and 2^32 bytes.  The cases are built
on the CPU by tests/_mla_cases.py from fixed seeds and checked there by tests/test_kvcache_mla_number_range_cpu.py.  "Every family": dense and sparse,
contiguous and pages of 16, 16-bit and FP8 cache; every section at fp16 and bf16.

  A. One visible key copies every finite 16-bit value.  Rows of all finite patterns in columns 0 .. 511 (63488 in fp16 over 124 rows, 65280 in bf16 over 128),
     dense (one sequence per row, L = 1, h 24, sq 2, capacity 96, num_splits 1 and 3: the combine runs) and sparse (one cache of 128 rows, token t names row
     t through one valid slot: slot 17 of 32, slot 80 of 96 - the last step).  out must hold the row's bits (a zero of either sign for +-0: the accumulator
     starts at +0).  The argument of test_kvcache_number_formats_gpu.py section A carries over to the MLA epilogue (out = pack2(oacc x (1 / lsum)), P packed to
     16 bits in front of the P.V MFMA): with one key P = exp2(residue) rounds to exactly 1 and lsum = exp2(residue), |residue| <= |s c| 2^-24.  But here the
     value IS the key, so q cannot be N(0, 1) on columns that hold 3e38 - see _mla_cases.rope_only_q: q is 0, or 0 in columns 0 .. 511 and N(0, 1) / 64 in the
     rope columns (|s c| < 1: 1 / lsum is within 2^-24 of 1, far below half an ulp of the output and half a step of its subnormal grid).
  B. Every finite 16-bit cache element and every finite 16-bit q reach the LSE: softmax_scale 1, one key, num_splits 1.  (i) q one-hot (1.0 at column j), the
     key row holds the patterns, rope columns included: LSE = kv[j]; the 640 (token, head) pairs of a sequence read its 576 columns.  (ii) the key is one-hot
     at column j, 65536 query rows (512 sequences x 128 heads dense, 8 x 64 tokens x 128 heads sparse) hold patterns everywhere: LSE = q[row, j].  bf16
     patterns end below 2^30 (SCORE_LIMIT_EXP of the number-formats suite: the contract |score| x log2 e < 2^31).  Bound: that suite's |lse - x| <= 2^-20
     max(|x|, 1), x in float64.  Its derivation carries over: the one MLA body (fa_kvcache_mla_attn.hpp compute_step / epilogue, which the three MLA sources instantiate)
     takes p = fast_exp2(fma(s, c, -(m c))) and lse = m sc + logf(lsum) exactly as kvcache_attn does - read again for this file - so l = exp2(residue of
     m c), |residue| <= |x log2 e| 2^-24, and the few fp32 roundings of m sc + logf(l) stay relative 2^-23 each.  FP8 version of (i): every NaN-free code in
     all four tiles under four scales, LSE = fp32(code) x scale rounded once to the dtype, the expectation from numpy (see C).  FP8 version of (ii): the
     bit-for-bit relation to the 16-bit call on the dequantised cache.
  C. FP8 tile scales across the fp32 range, one visible key whose row holds the 254 NaN-free codes twice.  Scales 2^e for e = -117 .. 118 - every e at which
     all products 2^-9 x 2^e .. 448 x 2^e are zero or normal fp32 numbers, the stated precondition; products that are fp32 subnormals stay outside it and
     are NOT tested - then 0.3, 3.7, 1 / 448, 65504 / 448 and the fp32 value above each, -1, -0.3, 0.  Expectation from numpy alone: float32 product, one
     rounding (astype(float16); round-to-nearest-even on the integer bits for bf16).  Rows that stay finite in the dtype: out has those bits (+-0 as in A) -
     rounding into the fp16 subnormals, ties, the bf16 top binades.  All rows, the fp16 rows that overflow (from 448 x 2^8) included: the call equals the
     16-bit call on dequantize_mla_kv_cache under same_nan.  Rows with scale 0, -1, -0.3: that relation bit for bit, signs of zero included (helper and
     kernel agree: a +0 code under a negative scale is -0 in both; nothing had to be settled).
  D. The quantising append at every tile amax: 32768 tiles in one call (64 sequences x 128 new rows), amax = every finite positive pattern of the dtype (the
     2^-24 clamp is reached exactly by fp16's smallest subnormal and undercut by 13184 bf16 patterns), a few tiles all zero; even tiles filled with random
     patterns below amax, odd tiles with the 16-bit values on and beside scale x midpoint for the e4m3 midpoints (the CPU file: every whole triple straddles a
     code boundary; 40613 / 37271 exact ties in fp16 / bf16).  New rows start at every offset within a page.  The cache rows equal quantize_mla_kv_cache(kv_new)
     from the CPU byte for byte, every other byte is kept, and - independently of the helper - the scale words are numpy's float32 quotient max(amax, 2^-24) /
     448.  A reciprocal-multiply differs from that quotient on thousands of these amax values (counted in the CPU file), so this sweep does separate them.
  E. Softmax extremes, the MLA counterpart of test_softmax_extremes: L 224 on capacity 256 (7 steps; 3 splits of 3, 3, 1 steps), h 24 (a partly filled second
     wave), sq 2; ramps of 0.14 nats a key up and down, a key 15 nats above the rest in the last step of the last split, q and keys x 6, a block confined to
     the first / last split whose LSE lies more than 100 above the others' (asserted in fp64).  Dense: num_splits 1 / 3 / 0, causal and not, both layouts;
     sparse: the same keys listed in order, reversed and shuffled, padded 224 -> 256 with -1.  fp64 through scores64 / exact / expect at U.TOL and U.LSE_TOL,
     the ramps with the factor 2 of test_softmax_extremes (a handful of effective keys per row) and no more.  FP8: the quantised cache through the relation,
     and one fp64 anchor per pattern.
  F. +-inf in a rope column - the one place where an inf reaches the score and not the value.  +inf in column 540 of the last row of sequence 0, -inf in
     column 550 of the last row of sequence 1 (lens 100, 33).  By the rule of test_nonfinite_inputs_propagate_like_fp64_math: the NaN pattern of O and LSE is
     fp64's (the sign of q's element decides between a NaN row and a dropped key), no inf comes out, rows that cannot see the row (token 0 under causal; the
     sparse token that does not name it) keep the clean run's bits, rows whose key drops out match fp64 at the existing tolerances, two runs agree.
  G. Addressing.  (i) page pools just above 2^32 bytes (233100 pages of 18432 B; 409300 FP8 pages of 10496 B; torch.empty, only the named pages written):
     the table names page 0, the last page, the pages around byte offsets 2^31 and 2^32 and a page whose start address has bit 31 of its low word set - the
     sparse paged kernels assemble the 64-bit row address from two 32-bit lane reads; bits equal the same call on a small pool, the append into far pages
     included.  (ii) a batch stride of 2^31 + 64 elements (FP8: 2^32 + 1024 bytes) for the cache and q, then for q and out through the C ABI: bits of the compact
     call, with and without kv_new, dense and sparse.  (iii) the longest sequence the host check admits (1864128 rows of 1152 B; FP8: 3273600 rows of 656 B -
     3273728 would already be 2^31 + 81920 bytes): sparse over the last rows against fp64; dense over all of it bit for bit against the paged call over the
     same memory with an identity table (per-block descriptors and 64-bit page offsets; an error the two paths share would not show there, hence also) against
     fp64 math run in chunks on the GPU; 16 rows more are refused with "one sequence spans .. (limit 2^31)" by both Python calls.

Measured on the MI355X (38 cases, 8 s; also in DESIGN.md section 3.5a-MLA; every run prints the lines that start with MARGIN).  A, C, D, G: every case bit
for bit; no kernel had to change.  B, worst |lse - x| (the same figure for dense and sparse, contiguous and paged): fp16 cache elements and fp16 q 3.9e-3 at
|x| = 4.6e4 (0.090 of the bound), bf16 cache elements and bf16 q below 2^30 64 at |x| = 7.5e8 (0.089 of the bound), e4m3 code x tile scale 4.9e-4 at |x| = 5.9e3 (0.087 of
the bound, both dtypes).  E, worst raw metric as a fraction of its tolerance (x 2 for the ramps), fp16 / bf16, over all calls of a pattern - max_abs is
measured without the one-ulp allowance of _util.assert_close, so a value above 1 is one output ulp at |O| in [8, 16):
    ramp_up           max_abs 0.20 / 0.20   mean_abs 0.11 / 0.11   mean_rel 0.004 / 0.006   LSE 0.004 / 0.003
    ramp_down         max_abs 0.02 / 0.02   mean_abs 0.04 / 0.04   mean_rel 0.05 / 0.09     LSE 0.000 / 0.000
    spike_last_split  max_abs 0.10 / 0.05   mean_abs 0.001 / 0.000 mean_rel 0.000 / 0.000   LSE 0.005 / 0.005
    scaled            max_abs 0.78 / 0.78   mean_abs 0.23 / 0.30   mean_rel 0.27 / 0.05     LSE 0.019 / 0.012
    lse_gap_first     max_abs 1.56 / 1.56   mean_abs 0.44 / 0.43   mean_rel 0.002 / 0.002   LSE 0.013 / 0.010
    lse_gap_last      max_abs 1.56 / 1.56   mean_abs 0.97 / 0.79   mean_rel 0.005 / 0.005   LSE 0.012 / 0.017
F: 1152 NaN LSE entries, 1152 rows whose key dropped out and 1152 rows that kept the clean run's bits per dtype, over all calls.  G (i): 69 of the 133 rows
read had bit 31 of their low address word set, under two different high words.
What the sections catch, tried on scratch builds with one arithmetic line changed (numbers only): pack2 made truncating in the FP8 kernels fails C (36192 of
835584 finite elements, 0x0000 for 0x0001 first); the append's division made a reciprocal-multiply fails D (17420 / 10792 scale words in fp16 / bf16); the
dense 16-bit body without `oacc *= alpha` fails E (max_abs 10 on ramp_up and spike_last_split, 0.9 on lse_gap_last).  The paged sparse address without the
(uint32_t) on its low word was NOT run: with bit 31 set - which G (i) asserts of a row it reads - it forms a wild 64-bit address, a GPU fault by design."""
import numpy as np
import pytest
import torch

import _mla_cases as C
import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_mla_fp8_gpu import logical_of, page_bytes, random_rows, same2
from test_kvcache_mla_sparse_gpu import expect, random_lists
from test_kvcache_number_formats_gpu import SCORE_LIMIT_EXP, _copy_mismatch, _lse_bound
from test_kvcache_prefill_gpu import visible
from test_kvcache_softcap_gpu import _rand, _same
from test_kvcache_tree_gpu import check, exact, scores64, split_rows

pytestmark = pytest.mark.gpu

DTS = ["fp16", "bf16"]
DT = C.DT
DK, DV, RB = C.DK, C.DV, C.RB
NAN = float("nan")
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(DK)))


def dense(q, kv, cs, **kw):
    return F.flash_mla_with_kvcache(q, kv, cs, return_softmax_lse=True, **kw)


def sparse(q, kv, cs, idx, **kw):
    return F.flash_mla_sparse_with_kvcache(q, kv, cs, idx, return_softmax_lse=True, **kw)


def _fill(t):
    return 0xFF if t.dtype == torch.uint8 else NAN


def layouts(kv, seed):
    """[(name, cache, keywords)]: the contiguous cache and the same rows in pages of 16 under a shuffled table, spare pages NaN / 0xff"""
    pool, table = page_bytes(kv, 16, seed, fill=_fill(kv))
    return [("contiguous", kv, dict()), ("paged", pool, dict(block_table=table))]


def _one_slot(b, sq, topk, slot, rows):
    """int32 (b, sq, topk) of -1 with `rows` (broadcast to (b, sq)) at `slot`"""
    idx = torch.full((b, sq, topk), -1, dtype=torch.int32)
    idx[:, :, slot] = torch.as_tensor(rows, dtype=torch.int32)
    return idx


def _summary(fails):
    return f"{len(fails)} failing cases:\n" + "\n".join(fails[:30])


# ---- A. one visible key copies every finite 16-bit value ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", DTS)
def test_a_one_visible_key_copies_every_finite_16bit_value(gpu, dtname):
    dt = DT[dtname]
    rows = C.a_rows(dt)
    R, h, sq = rows.shape[0], 24, 2
    bits = rows[:, :DV].contiguous().view(torch.int16)
    gen = torch.Generator().manual_seed(91100)
    fails = []
    kv = torch.full((R, 96, 1, DK), NAN, dtype=dt)
    kv[:, 0, 0] = rows
    dense_lay = layouts(kv.to(gpu), 3)
    cache = rows[torch.arange(128) % R].view(1, 128, 1, DK).to(gpu)
    sparse_lay = layouts(cache, 4)
    for qkind in ("zero", "rope"):
        mk = (lambda shape: torch.zeros(*shape, dtype=dt)) if qkind == "zero" else (lambda shape: C.rope_only_q(shape, dt, gen))
        q = mk((R, sq, h, DK)).to(gpu)
        want = bits.view(R, 1, 1, DV).expand(R, sq, h, DV).contiguous()
        for ns in (1, 3):
            for name, c, kw in dense_lay:
                out, lse = dense(q, c, 1, num_splits=ns, **kw)
                bad = _copy_mismatch(out, want)
                if bad is not None or not torch.isfinite(lse).all():
                    fails.append(f"dense {name} q={qkind} splits={ns}: {bad or 'non-finite LSE'}")
        qs = mk((1, R, h, DK)).to(gpu)
        wants = bits.view(1, R, 1, DV).expand(1, R, h, DV).contiguous()
        for topk, slot in ((32, 17), (96, 80)):
            idx = _one_slot(1, R, topk, slot, torch.arange(R).view(1, R)).to(gpu)
            for ns in (1, 3):
                for name, c, kw in sparse_lay:
                    out, lse = sparse(qs, c, 128, idx, num_splits=ns, **kw)
                    bad = _copy_mismatch(out, wants)
                    if bad is not None or not torch.isfinite(lse).all():
                        fails.append(f"sparse {name} q={qkind} topk={topk} splits={ns}: {bad or 'non-finite LSE'}")
    assert not fails, f"{dtname}: " + _summary(fails)


# ---- B. every finite 16-bit cache element and q reach the LSE -----------------------------------------------------------------------------------------------------

def _lse_cases(calls, x, fails, worst):
    """calls: [(tag, lse (.., ) tensor)], x float64 numpy of the same shape: finite, and |lse - x| within the bound"""
    for tag, lse in calls:
        got = lse.double().cpu().numpy()
        if not np.isfinite(got).all():
            fails.append(f"{tag}: {int((~np.isfinite(got)).sum())} non-finite LSE entries, first for x = {x[~np.isfinite(got)][0]!r}")
            continue
        ratio = np.abs(got - x) / _lse_bound(x)
        worst[tag] = (float(np.abs(got - x).max()), float(ratio.max()))
        if ratio.max() > 1.0:
            at = tuple(np.argwhere(ratio > 1.0)[0])
            fails.append(f"{tag}: |lse - x| exceeds the bound on {int((ratio > 1).sum())} rows, worst {ratio.max():.2f} x the bound; first: x {x[at]!r} lse {got[at]!r}")


@pytest.mark.parametrize("dtname", DTS)
def test_b_every_finite_16bit_cache_element_reaches_the_lse(gpu, dtname):
    dt = DT[dtname]
    keys = C.b_key_rows(dt, SCORE_LIMIT_EXP if dtname == "bf16" else None)
    b = keys.shape[0]
    q, j = C.b_onehot_q(b, dt)
    x = keys.double()[torch.arange(b).view(-1, 1, 1), j].permute(0, 2, 1).numpy()           # (b, h, sq)
    kv = torch.full((b, 16, 1, DK), NAN, dtype=dt)
    kv[:, 0, 0] = keys
    kvs = torch.full((b, 32, 1, DK), NAN, dtype=dt)
    kvs[:, 5, 0] = keys
    idx = _one_slot(b, C.B_SQ, 32, 17, 5).to(gpu)
    qg = q.to(gpu)
    calls = [(f"dense {n}", dense(qg, c, 1, num_splits=1, softmax_scale=1.0, **kw)[1]) for n, c, kw in layouts(kv.to(gpu), 5)]
    calls += [(f"sparse {n}", sparse(qg, c, 32, idx, num_splits=1, softmax_scale=1.0, **kw)[1]) for n, c, kw in layouts(kvs.to(gpu), 6)]
    fails, worst = [], {}
    _lse_cases(calls, x, fails, worst)
    print(f"MARGIN B cache element {dtname}: worst |lse - x| and worst ratio to the bound: {worst}")
    assert not fails, f"{dtname}: " + _summary(fails)


@pytest.mark.parametrize("dtname", DTS)
def test_b_every_e4m3_code_times_its_tile_scale_reaches_the_lse(gpu, dtname):
    dt = DT[dtname]
    rows = C.b_fp8_rows(dt)
    b = rows.shape[0]
    bits = C.dequant_expect_bits(rows[:, :DV].numpy(), rows[:, DV:DV + 16].contiguous().view(torch.float32).numpy(), dtname)
    full = torch.cat([torch.from_numpy(bits.view(np.int16)).view(dt).double(), rows[:, DV + 16:].contiguous().view(dt).double()], dim=-1)      # (b, 576)
    assert torch.isfinite(full).all()
    q, j = C.b_onehot_q(b, dt)
    x = full[torch.arange(b).view(-1, 1, 1), j].permute(0, 2, 1).numpy()
    kv = torch.full((b, 16, 1, RB), 0xFF, dtype=torch.uint8)
    kv[:, 0, 0] = rows
    kvs = torch.full((b, 32, 1, RB), 0xFF, dtype=torch.uint8)
    kvs[:, 5, 0] = rows
    idx = _one_slot(b, C.B_SQ, 32, 17, 5).to(gpu)
    qg = q.to(gpu)
    calls = [(f"fp8 dense {n}", dense(qg, c, 1, num_splits=1, softmax_scale=1.0, **kw)[1]) for n, c, kw in layouts(kv.to(gpu), 7)]
    calls += [(f"fp8 sparse {n}", sparse(qg, c, 32, idx, num_splits=1, softmax_scale=1.0, **kw)[1]) for n, c, kw in layouts(kvs.to(gpu), 8)]
    fails, worst = [], {}
    _lse_cases(calls, x, fails, worst)
    print(f"MARGIN B fp8 code x scale {dtname}: worst |lse - x| and worst ratio to the bound: {worst}")
    assert not fails, f"{dtname}: " + _summary(fails)


@pytest.mark.parametrize("dtname", DTS)
def test_b_every_finite_16bit_q_reaches_the_lse(gpu, dtname):
    dt = DT[dtname]
    lim = SCORE_LIMIT_EXP if dtname == "bf16" else None
    nseq, h = 512, 128
    jseq = (torch.arange(nseq) * 7 + 3) % DK
    qr = C.b_query_rows(dt, lim, nseq * h, jseq.repeat_interleave(h))
    x = qr[torch.arange(nseq * h), jseq.repeat_interleave(h)].double().view(nseq, h)
    onehot = torch.zeros(nseq, DK, dtype=dt)
    onehot[torch.arange(nseq), jseq] = 1.0
    fails, worst = [], {}
    # dense: 512 sequences x 128 heads
    kv = torch.zeros(nseq, 16, 1, DK, dtype=dt)
    kv[:, 0, 0] = onehot
    qd = qr.view(nseq, 1, h, DK).to(gpu)
    kvg = kv.to(gpu)
    calls = [(f"dense {n}", dense(qd, c, 1, num_splits=1, softmax_scale=1.0, **kw)[1]) for n, c, kw in layouts(kvg, 9)]
    kv8 = F.quantize_mla_kv_cache(kv).to(gpu)
    assert same2(dense(qd, kv8, 1, num_splits=1, softmax_scale=1.0), dense(qd, F.dequantize_mla_kv_cache(kv8, dt), 1, num_splits=1, softmax_scale=1.0)), "fp8 dense"
    _lse_cases(calls, x.view(nseq, h, 1).numpy(), fails, worst)
    # sparse: 8 sequences x 64 tokens x 128 heads; token t of sequence i names row t, which is one-hot at the column of dense sequence 64 i + t
    kvs = onehot.view(8, 64, 1, DK).to(gpu)
    qs = qr.view(8, 64, h, DK).to(gpu)
    idx = _one_slot(8, 64, 32, 17, torch.arange(64).view(1, 64)).to(gpu)
    calls = [(f"sparse {n}", sparse(qs, c, 64, idx, num_splits=1, softmax_scale=1.0, **kw)[1]) for n, c, kw in layouts(kvs, 10)]
    kvs8 = F.quantize_mla_kv_cache(kvs.cpu()).to(gpu)
    assert same2(sparse(qs, kvs8, 64, idx, num_splits=1, softmax_scale=1.0), sparse(qs, F.dequantize_mla_kv_cache(kvs8, dt), 64, idx, num_splits=1, softmax_scale=1.0)), "fp8 sparse"
    _lse_cases(calls, x.view(8, 64, h).permute(0, 2, 1).numpy(), fails, worst)
    print(f"MARGIN B q {dtname}: worst |lse - x| and worst ratio to the bound: {worst}")
    assert not fails, f"{dtname}: " + _summary(fails)


# ---- C. FP8 tile scales across the fp32 range ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", DTS)
def test_c_fp8_tile_scales_across_the_fp32_range(gpu, dtname):
    dt = DT[dtname]
    rows = C.c_rows(dt)
    b, h, sq = rows.shape[0], 24, 2
    scales = rows[:, DV:DV + 16].contiguous().view(torch.float32)
    bits = torch.from_numpy(C.dequant_expect_bits(rows[:, :DV].numpy(), scales.numpy(), dtname).view(np.int16))
    finite = torch.isfinite(bits.view(dt).float()).all(-1)
    signed = (scales <= 0).any(-1)                                   # the rows with scale 0, -1, -0.3
    assert int(finite.sum()) == (b - 28 if dtname == "fp16" else b) and int(signed.sum()) == 1 and finite[signed].all()
    assert int(((bits.view(dt) == 0) & torch.signbit(bits.view(dt).float()))[signed].sum()) >= 2, "a +0 code under a negative scale must be -0 in the expectation"
    want = bits[finite].view(-1, 1, 1, DV).expand(-1, sq, h, DV).contiguous()
    gen = torch.Generator().manual_seed(93100)
    q = C.rope_only_q((b, sq, h, DK), dt, gen).to(gpu)
    kv = torch.full((b, 48, 1, RB), 0xFF, dtype=torch.uint8)
    kv[:, 0, 0] = rows
    kvs = torch.full((b, 96, 1, RB), 0xFF, dtype=torch.uint8)
    kvs[:, 5, 0] = rows
    idx = _one_slot(b, sq, 96, 70, 5).to(gpu)
    fails = []

    def judge(tag, got, ref):
        bad = _copy_mismatch(got[0][finite.to(gpu)], want)
        if bad is not None:
            fails.append(f"{tag}: rows that stay finite differ from the numpy expectation: {bad}")
        if not same2(got, ref):
            fails.append(f"{tag}: differs from the 16-bit call on the dequantised cache (same_nan; overflow rows included)")
        s = signed.to(gpu)
        if not (_same(got[0][s], ref[0][s]) and _same(got[1][s], ref[1][s])):
            fails.append(f"{tag}: the row with scales -1, -0.3, 0 differs from the 16-bit call in some bit")
        if not torch.isfinite(got[1][finite.to(gpu)]).all():
            fails.append(f"{tag}: non-finite LSE on a finite row")

    kvg, kvsg = kv.to(gpu), kvs.to(gpu)
    kv16, kvs16 = F.dequantize_mla_kv_cache(kvg, dt), F.dequantize_mla_kv_cache(kvsg, dt)
    for ns in (1, 3):
        ref = dense(q, kv16, 1, num_splits=ns)
        for name, c, kw in layouts(kvg, 11):
            judge(f"dense {name} splits={ns}", dense(q, c, 1, num_splits=ns, **kw), ref)
        ref = sparse(q, kvs16, 96, idx, num_splits=ns)
        for name, c, kw in layouts(kvsg, 12):
            judge(f"sparse {name} splits={ns}", sparse(q, c, 96, idx, num_splits=ns, **kw), ref)
    assert not fails, f"{dtname}: " + _summary(fails)


# ---- D. the quantising append at every tile amax ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", DTS)
@pytest.mark.parametrize("P", [0, 16])
def test_d_append_quantises_every_tile_amax_like_the_helper(gpu, dtname, P):
    dt = DT[dtname]
    kv_new, amax, _ = C.d_kv_new(dt)
    q8 = F.quantize_mla_kv_cache(kv_new)                             # CPU
    pre, cap, b, s_new = C.d_prefix_lengths(), C.D_CAP, C.D_B, C.D_SNEW
    gen = torch.Generator().manual_seed(94100 + P)
    before = random_rows((b, cap, 1), dt, gen)
    want = before.clone()
    for i, L in enumerate(pre):
        want[i, L:L + s_new] = q8[i]
    cs = torch.tensor(pre, dtype=torch.int32, device=gpu)
    q = torch.zeros(b, 1, 16, DK, dtype=dt, device=gpu)              # (attention is not the subject: q = 0 keeps every score 0 whatever the rows hold)
    cache, ready, table = before.to(gpu), want.to(gpu), None
    if P:
        cache, table = page_bytes(cache, P, 5, fill=0xA5)
        ready, _ = page_bytes(ready, P, 5, fill=0xA5)
    dense(q, cache, cs, kv_new=kv_new.to(gpu), causal=True, num_splits=1, block_table=table)
    after = (logical_of(cache, table, cap) if P else cache).cpu()
    new = torch.stack([after[i, L:L + s_new] for i, L in enumerate(pre)])                         # (b, s_new, 1, 656)
    # independently of the helper: the scale words are the correctly rounded float32 quotient
    words = new[..., DV:DV + 16].contiguous().view(torch.float32).reshape(-1).numpy()
    quot, _ = C.d_scale_words(amax, dt)
    wrong = np.flatnonzero(words.view(np.uint32) != quot.view(np.uint32))
    assert wrong.size == 0, (f"{dtname} P{P}: {wrong.size} scale words differ from float32(max(amax, 2^-24)) / float32(448); first: tile {wrong[0]} amax bits "
                             f"{int(amax[wrong[0]]):#06x} got {words[wrong[0]]!r} want {quot[wrong[0]]!r}")
    for what, sl in (("codes", slice(0, DV)), ("scale words", slice(DV, DV + 16)), ("rope bytes", slice(DV + 16, RB))):
        diff = (new[..., sl] != q8[..., sl]).nonzero()
        assert diff.numel() == 0, f"{dtname} P{P}: {diff.shape[0]} {what} differ from quantize_mla_kv_cache; first (sequence, new row, -, byte) {diff[0].tolist()}"
    assert torch.equal(after, want), f"{dtname} P{P}: a row outside the new ones changed"
    assert torch.equal(cache, ready), f"{dtname} P{P}: a byte outside the new rows (pages no sequence owns included) changed"


# ---- E. softmax extremes ------------------------------------------------------------------------------------------------------------------------------------------------

def _e_check(out, lse, xo, xl, nvis, dtname, tag, scale, worst):
    """split_rows (finite, dead rows, LSE under LSE_TOL) and assert_close at `scale` per group; records the raw metrics as ratios to the tolerance"""
    parts = split_rows(out, lse, xo, xl, nvis, tag)
    worst["lse"] = max(worst.get("lse", 0.0), float((lse.double().cpu() - xl).abs().max()) / U.LSE_TOL)
    for name, (got, want, sk) in parts.items():
        raw = U.assert_close(got, want, dtname, f"mla extremes O {tag} {name} rows", scale=scale, sk=sk)
        for k, v in raw.items():
            worst[k] = max(worst.get(k, 0.0), v / (U.TOL[dtname][k] * scale))


@pytest.mark.parametrize("dtname", DTS)
@pytest.mark.parametrize("pattern", C.E_PATTERNS)
def test_e_softmax_extremes(gpu, pattern, dtname):
    dt = DT[dtname]
    q, kv = C.e_case(pattern, dt)
    L, cap, sq = C.E_L, C.E_CAP, C.E_SQ
    scale = 2.0 if pattern.startswith("ramp") else 1.0
    worst = {}
    s = scores64(q, kv, SCALE)
    qg, kvg = q.to(gpu), kv.to(gpu)
    cs = torch.tensor([L], dtype=torch.int32, device=gpu)
    lay = layouts(kvg, 13)
    for causal in (False, True):
        vis = visible([L], sq, cap, causal)
        xo, xl, nvis = exact(s, kv[..., :DV], vis)
        if pattern in C.E_GAP_BLOCK:
            rest = vis.clone()
            rest[:, :, C.E_GAP_BLOCK[pattern]] = False
            assert float((xl - exact(s, kv[..., :DV], rest)[1]).min()) > 100.0, "the case must put an LSE gap > 100 between splits"
        for ns in (1, 3, 0):
            for name, c, kw in lay:
                out, lse = dense(qg, c, cs, causal=causal, num_splits=ns, **kw)
                _e_check(out, lse, xo, xl, nvis, dtname, f"{pattern} {dtname} dense {name} causal={causal} splits={ns}", scale, worst)
    lists = C.e_lists()
    for lname, idx in lists.items():
        xo, xl, nvis = expect(q, kv, idx, [L])
        ig = idx.to(gpu)
        for ns in (1, 3, 0):
            for name, c, kw in lay:
                out, lse = sparse(qg, c, cs, ig, num_splits=ns, **kw)
                _e_check(out, lse, xo, xl, nvis, dtname, f"{pattern} {dtname} sparse {lname} {name} splits={ns}", scale, worst)
    # FP8: the quantised cache through the bit-for-bit relation, and one fp64 anchor over the dequantised cache
    kv8 = F.quantize_mla_kv_cache(kv)
    kvl = F.dequantize_mla_kv_cache(kv8, dt)
    kv8g, kvlg = kv8.to(gpu), kvl.to(gpu)
    for ns in (1, 3, 0):
        for name, c, kw in layouts(kv8g, 14):
            for causal in (False, True):
                assert same2(dense(qg, c, cs, causal=causal, num_splits=ns, **kw), dense(qg, kvlg, cs, causal=causal, num_splits=ns)), f"fp8 dense {name} causal={causal} splits={ns}"
            for lname, idx in lists.items():
                assert same2(sparse(qg, c, cs, idx.to(gpu), num_splits=ns, **kw), sparse(qg, kvlg, cs, idx.to(gpu), num_splits=ns)), f"fp8 sparse {lname} {name} splits={ns}"
    xo, xl, nvis = exact(scores64(q, kvl, SCALE), kvl[..., :DV], visible([L], sq, cap, False))
    out, lse = dense(qg, kv8g, cs, num_splits=3)
    _e_check(out, lse, xo, xl, nvis, dtname, f"{pattern} {dtname} fp8 dense splits=3", scale, worst)
    xo, xl, nvis = expect(q, kvl, lists["shuffled"], [L])
    out, lse = sparse(qg, kv8g, cs, lists["shuffled"].to(gpu), num_splits=3)
    _e_check(out, lse, xo, xl, nvis, dtname, f"{pattern} {dtname} fp8 sparse shuffled splits=3", scale, worst)
    print(f"MARGIN E {pattern} {dtname}: worst raw metric / (tolerance x {scale}): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ---- F. +-inf in a rope column ------------------------------------------------------------------------------------------------------------------------------------------

def _f_judge(got_b, got_b2, got_c, ref_b, ref_c, dtname, tag):
    """the rule of test_nonfinite_inputs_propagate_like_fp64_math over one call: (out, lse) of the bad run, of its repeat and of the clean run, the fp64
    (O, LSE) on the bad and on the clean cache.  Returns the numbers of NaN LSE entries, of rows whose key dropped out and of rows that kept their bits."""
    (ob, lb), (oc, lc), (ro_b, rl_b), (ro_c, rl_c) = got_b, got_c, ref_b, ref_c
    assert _same(ob, got_b2[0]) and _same(lb, got_b2[1]), f"{tag}: two runs differ"
    assert not torch.isinf(ob).any().item() and not torch.isinf(lb).any().item(), f"{tag}: an inf came out"
    xo, xl = ob.float().cpu(), lb.cpu()
    assert torch.equal(torch.isnan(xl), torch.isnan(rl_b)), f"{tag}: LSE NaN pattern {torch.isnan(xl).nonzero().tolist()} != fp64 {torch.isnan(rl_b).nonzero().tolist()}"
    assert torch.equal(torch.isnan(xo), torch.isnan(ro_b)), f"{tag}: O NaN pattern differs from fp64 math (rows {torch.isnan(ro_b).any(-1).nonzero().tolist()})"
    nan = torch.isnan(rl_b).permute(0, 2, 1)                                             # (b, sq, h)
    same_ref = (ro_b == ro_c).all(-1) & (rl_b == rl_c).permute(0, 2, 1)
    keep = (~nan & same_ref).to(ob.device)
    assert _same(ob[keep], oc[keep]) and _same(lb.permute(0, 2, 1)[keep], lc.permute(0, 2, 1)[keep]), f"{tag}: a row that cannot see the inf changed"
    dropped = (~nan & ~same_ref).nonzero().tolist()
    for i, t, hq in dropped:
        U.assert_close(xo[i, t, hq].numpy(), ro_b[i, t, hq].numpy(), dtname, f"{tag} b{i} t{t} h{hq}")
        assert abs(float(xl[i, hq, t]) - float(rl_b[i, hq, t])) <= U.LSE_TOL, f"{tag}: LSE of a row whose key dropped out, b{i} t{t} h{hq}"
    return int(torch.isnan(rl_b).sum()), len(dropped), int(keep.sum())


@pytest.mark.parametrize("dtname", DTS)
def test_f_inf_in_a_rope_column_propagates_like_fp64_math(gpu, dtname):
    dt = DT[dtname]
    q, kv, bad, idx = C.f_case(dt)
    qg, ig = q.to(gpu), idx.to(gpu)
    cs = torch.tensor(C.F_LENS, dtype=torch.int32, device=gpu)
    n_nan = n_drop = n_keep = 0
    kv8c, kv8b = F.quantize_mla_kv_cache(kv), F.quantize_mla_kv_cache(bad)
    assert torch.equal(kv8c[..., :DV + 16], kv8b[..., :DV + 16]) and not torch.equal(kv8c, kv8b)       # the rope bytes carry the inf, nothing else differs
    for fam, clean, dirty in (("16-bit", kv, bad), ("fp8", kv8c, kv8b)):
        # the fp64 reference of the FP8 family runs over the dequantised caches
        lc_, lb_ = (clean, dirty) if fam == "16-bit" else (F.dequantize_mla_kv_cache(clean, dt), F.dequantize_mla_kv_cache(dirty, dt))
        lay_c, lay_b = layouts(clean.to(gpu), 15), layouts(dirty.to(gpu), 15)
        for causal in (False, True):
            ref_c, ref_b = C.f_dense_ref(q, lc_, causal), C.f_dense_ref(q, lb_, causal)
            for ns in (1, 3, 0):
                for (name, cc, kw), (_, cb, _) in zip(lay_c, lay_b):
                    run = lambda c: dense(qg, c, cs, causal=causal, num_splits=ns, **kw)
                    got = run(cb)
                    a, d, k = _f_judge(got, run(cb), run(cc), ref_b, ref_c, dtname, f"{fam} dense {name} causal={causal} splits={ns}")
                    n_nan, n_drop, n_keep = n_nan + a, n_drop + d, n_keep + k
                    if fam == "fp8":
                        assert same2(got, dense(qg, lb_.to(gpu), cs, causal=causal, num_splits=ns)), f"fp8 dense {name} causal={causal} splits={ns}: the relation"
        ref_c, ref_b = C.f_sparse_ref(q, lc_, idx), C.f_sparse_ref(q, lb_, idx)
        for ns in (1, 3, 0):
            for (name, cc, kw), (_, cb, _) in zip(lay_c, lay_b):
                run = lambda c: sparse(qg, c, cs, ig, num_splits=ns, **kw)
                got = run(cb)
                a, d, k = _f_judge(got, run(cb), run(cc), ref_b, ref_c, dtname, f"{fam} sparse {name} splits={ns}")
                n_nan, n_drop, n_keep = n_nan + a, n_drop + d, n_keep + k
                assert _same(got[0][:, 0], run(cc)[0][:, 0]), f"{fam} sparse {name} splits={ns}: the token that does not name the row changed"
                if fam == "fp8":
                    assert same2(got, sparse(qg, lb_.to(gpu), cs, ig, num_splits=ns)), f"fp8 sparse {name} splits={ns}: the relation"
    print(f"F {dtname}: {n_nan} NaN LSE entries, {n_drop} rows whose key dropped out, {n_keep} rows that kept the clean run's bits")
    assert n_nan > 0 and n_drop > 0 and n_keep > 0, "the case must produce NaN rows, dropped keys and untouched rows"


# ---- G. addressing past 2^31 and 2^32 bytes ------------------------------------------------------------------------------------------------------------------------------

def _freed(fn, *args):
    torch.cuda.empty_cache()
    try:
        fn(*args)
    finally:
        torch.cuda.empty_cache()


def _g_lists(gen):
    """sparse lists (2, 2, 64) over G_LENS: random ones, and in token 0 the first and the last row of every page the sequence owns"""
    idx = random_lists(C.G_LENS, 2, 64, gen, cap=C.G_CAP, dead_steps=False)
    for i, L in enumerate(C.G_LENS):
        edge = sorted({r for c in range((L + 15) // 16) for r in (16 * c, min(16 * c + 15, L - 1))})
        idx[i, 0, :len(edge)] = torch.tensor(edge, dtype=torch.int32)
    return idx


def _g_pool(gpu, dtname, fp8):
    dt = DT[dtname]
    rb = C.ROW8 if fp8 else C.ROW16
    n, P, cap, lens = C.G_POOL[rb], C.G_P, C.G_CAP, C.G_LENS
    pool = torch.empty((n, P, 1, RB if fp8 else DK), dtype=torch.uint8 if fp8 else dt, device=gpu)
    assert pool.numel() * pool.element_size() > 2 ** 32 and pool.is_contiguous()
    base = pool.data_ptr()
    table = C.g_pages(rb, base)
    gen = torch.Generator().manual_seed(97000 + int(fp8))
    logical = (random_rows((2, cap, 1), dt, gen) if fp8 else _rand((2, cap, 1, DK), dt, gen)).to(gpu)
    for i in range(2):
        for c in range(cap // P):
            pool[int(table[i, c])] = logical[i, P * c:P * c + P]
    small, stable = page_bytes(logical, P, 31, fill=_fill(logical))
    tg = table.to(gpu)
    rows = [base + int(table[i, r // P]) * P * rb + (r % P) * rb for i, L in enumerate(lens) for r in range(L)]
    low = [a & 0xFFFFFFFF for a in rows]
    print(f"G(i) {dtname} fp8={fp8}: pool at {base:#x}, {n} pages, table {table.tolist()}; low address words of the rows read: min {min(low):#010x} max {max(low):#010x}, "
          f"{sum(1 for w in low if w & 0x80000000)} of {len(low)} with bit 31 set; high words {sorted({a >> 32 for a in rows})}")
    assert any(w & 0x80000000 for w in low) and len({a >> 32 for a in rows}) >= 2, "the rows read must include one whose low address word has bit 31 set, under more than one high word"
    q = _rand((2, 2, 24, DK), dt, gen, 1 / 16).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    idx = _g_lists(gen).to(gpu)
    for ns in (1, 3):
        for causal in (False, True):
            assert same2(dense(q, pool, cs, causal=causal, num_splits=ns, block_table=tg), dense(q, small, cs, causal=causal, num_splits=ns, block_table=stable)), \
                f"dense causal={causal} splits={ns}: the pool above 4 GiB differs from the small pool"
        assert same2(sparse(q, pool, cs, idx, num_splits=ns, block_table=tg), sparse(q, small, cs, idx, num_splits=ns, block_table=stable)), \
            f"sparse splits={ns}: the pool above 4 GiB differs from the small pool"
    # the append into far pages: rows 98, 99 of sequence 0 (the page at 2^32) and 31, 32 of sequence 1 (the last page and the page behind 2^32)
    kv_new = _rand((2, 2, 1, DK), dt, gen, 3.0).to(gpu)
    pre = torch.tensor([L - 2 for L in lens], dtype=torch.int32, device=gpu)
    a = dense(q, pool, pre, kv_new=kv_new, causal=True, num_splits=1, block_table=tg)
    b_ = dense(q, small, pre, kv_new=kv_new, causal=True, num_splits=1, block_table=stable)
    assert same2(a, b_), "append: attention differs"
    big_pages, small_pages = pool[tg.long()], small[stable.long()]
    assert torch.equal(big_pages.view(torch.uint8), small_pages.view(torch.uint8)), "append: the far pages differ from the small pool's"
    assert not torch.equal(small_pages.reshape(2, cap, 1, -1).view(torch.uint8), logical.view(torch.uint8)), "the append must have changed the rows"


@pytest.mark.parametrize("dtname", DTS)
@pytest.mark.parametrize("fp8", [False, True])
def test_g_page_pool_larger_than_4_gib(gpu, dtname, fp8):
    _freed(_g_pool, gpu, dtname, fp8)


def _far(gpu, shape, dt, stride_b):
    """an uninitialised (2, *shape) tensor whose batch entries lie stride_b elements apart, over one allocation"""
    n = int(np.prod(shape))
    inner = [int(np.prod(shape[k + 1:])) for k in range(len(shape))]
    return torch.empty(stride_b + n, dtype=dt, device=gpu).as_strided((2, *shape), (stride_b, *inner))


def _g_far_batch(gpu, dtname, fp8):
    dt = DT[dtname]
    cap, lens, sq, h = 64, [40, 50], 2, 24
    gen = torch.Generator().manual_seed(97500 + int(fp8))
    far16 = 2 ** 31 + 64                                               # elements
    kvc = (random_rows((2, cap, 1), dt, gen) if fp8 else _rand((2, cap, 1, DK), dt, gen)).to(gpu)
    qc = _rand((2, sq, h, DK), dt, gen, 1 / 16).to(gpu)
    kv_new = _rand((2, 2, 1, DK), dt, gen, 3.0).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    idx = random_lists(lens, sq, 64, gen, cap=cap, dead_steps=False).to(gpu)
    kvf = _far(gpu, (cap, 1, RB), torch.uint8, 2 ** 32 + 1024) if fp8 else _far(gpu, (cap, 1, DK), dt, far16)
    qf = _far(gpu, (sq, h, DK), dt, far16)
    assert kvf.stride(0) * kvf.element_size() > 2 ** 32 and qf.stride(0) * 2 > 2 ** 32
    kvf.copy_(kvc)
    qf.copy_(qc)
    for ns in (1, 3):
        assert same2(dense(qf, kvf, cs, causal=True, num_splits=ns), dense(qc, kvc, cs, causal=True, num_splits=ns)), f"dense splits={ns}"
        assert same2(sparse(qf, kvf, cs, idx, num_splits=ns), sparse(qc, kvc, cs, idx, num_splits=ns)), f"sparse splits={ns}"
    kv2 = kvc.clone()
    assert same2(dense(qf, kvf, cs, kv_new=kv_new, causal=True), dense(qc, kv2, cs, kv_new=kv_new, causal=True)), "append"
    assert torch.equal(kvf.contiguous(), kv2) and not torch.equal(kv2, kvc), "append: the far batch entry's rows"
    del kvf
    torch.cuda.empty_cache()
    # q and out far apart, through the C ABI (the Python calls allocate out themselves)
    of = _far(gpu, (sq, h, DV), dt, far16)
    lse = torch.empty(2, h, sq, device=gpu)
    want = dense(qc, kv2, cs, causal=True, num_splits=1)
    of[0], of[1] = NAN, NAN
    capi.run_mla_fwd_kvcache(capi.mla_params(qf, kv2, of, lse, cs, causal=True, num_splits=1))
    torch.cuda.synchronize()
    assert same2((of.contiguous(), lse), want), "C ABI dense, q and out far apart"
    want = sparse(qc, kv2, cs, idx, num_splits=1)
    of[0], of[1] = NAN, NAN
    capi.run_mla_sparse_fwd_kvcache(capi.mla_sparse_params(qf, kv2, of, lse, idx, cs, num_splits=1))
    torch.cuda.synchronize()
    assert same2((of.contiguous(), lse), want), "C ABI sparse, q and out far apart"


@pytest.mark.parametrize("dtname", DTS)
@pytest.mark.parametrize("fp8", [False, True])
def test_g_batch_stride_beyond_2_to_the_31(gpu, dtname, fp8):
    _freed(_g_far_batch, gpu, dtname, fp8)


def _fp64_in_chunks(q, kv, chunk=1 << 17):
    """fp64 softmax(q . kv x SCALE) @ kv[:, :512] over ALL rows of kv (1, cap, 1, 576) on its device, for q (1, 1, 1, 576): O (1, 1, 1, 512), LSE (1, 1, 1)"""
    qd = q.double().view(DK)
    cap = kv.shape[1]
    s = torch.cat([(kv[0, a:a + chunk, 0].double() @ qd) * SCALE for a in range(0, cap, chunk)])
    lse = torch.logsumexp(s, 0)
    o = sum(torch.exp(s[a:a + chunk] - lse) @ kv[0, a:a + chunk, 0, :DV].double() for a in range(0, cap, chunk))
    return o.view(1, 1, 1, DV).cpu(), lse.view(1, 1, 1).cpu()


def _g_longest(gpu, dtname):
    dt = DT[dtname]
    cap = C.G_LONGEST[C.ROW16]
    gen = torch.Generator().manual_seed(98000)
    kv = torch.empty((1, cap, 1, DK), dtype=dt, device=gpu).normal_(generator=torch.Generator(device=gpu).manual_seed(98001))
    assert cap * C.ROW16 < 2 ** 31 <= (cap + 16) * C.ROW16
    # sparse: 32 of the last 64 rows, against fp64 over the gathered rows
    q = _rand((1, 2, 24, DK), dt, gen)
    tail = kv[:, cap - 64:].cpu()
    local = torch.stack([torch.randperm(64, generator=gen)[:32] for _ in range(2)]).view(1, 2, 32).to(torch.int32)
    xo, xl, nvis = expect(q, tail, local, [64])
    for ns in (1, 0):
        out, lse = sparse(q.to(gpu), kv, cap, (local + (cap - 64)).to(gpu), num_splits=ns)
        check(out, lse, xo, xl, nvis, dtname, f"longest sequence {dtname} sparse splits={ns}")
    # dense over all of it: the paged call over the same memory with an identity table, bit for bit; and fp64 in chunks
    q1 = _rand((1, 1, 1, DK), dt, gen).to(gpu)
    table = torch.arange(cap // 16, dtype=torch.int32, device=gpu).view(1, -1)
    got = dense(q1, kv, cap, num_splits=0)
    assert same2(dense(q1, kv.view(cap // 16, 16, 1, DK), cap, num_splits=0, block_table=table), got), "the paged call over the same memory differs"
    xo, xl = _fp64_in_chunks(q1, kv)
    check(got[0], got[1], xo, xl, torch.full((1, 1), cap), dtname, f"longest sequence {dtname} dense")
    # 16 rows more are refused (no launch)
    more = torch.empty((1, cap + 16, 1, DK), dtype=dt, device=gpu)
    with pytest.raises(Exception, match=r"one sequence spans \d+ bytes \(limit 2\^31\)"):
        dense(q1, more, 1)
    with pytest.raises(Exception, match=r"one sequence spans \d+ bytes \(limit 2\^31\)"):
        sparse(q1, more, 1, torch.full((1, 1, 32), -1, dtype=torch.int32, device=gpu))
    del more, kv
    torch.cuda.empty_cache()
    # FP8, 656-byte rows: the sparse call over the last rows equals the call on those rows alone
    cap8 = C.G_LONGEST[C.ROW8]
    assert cap8 * RB < 2 ** 31 <= (cap8 + 16) * RB
    kv8 = torch.empty((1, cap8, 1, RB), dtype=torch.uint8, device=gpu)
    # (quantised N(0, 1) rows, as in test_against_fp64_on_the_dequantised_cache: the fp64 anchor below uses tolerances made for values of order 1, and
    # random_rows' scales up to 16 put values up to 7168 - one fp16 ulp is 4 there - into the value)
    tail8 = F.quantize_mla_kv_cache(_rand((1, 64, 1, DK), dt, gen)).to(gpu)
    kv8[:, cap8 - 64:] = tail8
    got = sparse(q.to(gpu), kv8, cap8, (local + (cap8 - 64)).to(gpu), num_splits=1)
    assert same2(got, sparse(q.to(gpu), F.dequantize_mla_kv_cache(tail8, dt), 64, local.to(gpu), num_splits=1)), "fp8 sparse over the last rows of the longest cache"
    xo, xl, nvis = expect(q, F.dequantize_mla_kv_cache(tail8, dt).cpu(), local, [64])
    check(got[0], got[1], xo, xl, nvis, dtname, f"longest sequence {dtname} fp8 sparse")
    with pytest.raises(Exception, match=r"one sequence spans \d+ bytes \(limit 2\^31\)"):
        sparse(q1, torch.empty((1, cap8 + 16, 1, RB), dtype=torch.uint8, device=gpu), 1, torch.full((1, 1, 32), -1, dtype=torch.int32, device=gpu))


@pytest.mark.parametrize("dtname", DTS)
def test_g_the_longest_sequence_the_host_check_admits(gpu, dtname):
    _freed(_g_longest, gpu, dtname)
