"""GPU: flash_attn_with_kvcache at head_dim 256 (fa_fwd_kvcache_d256.hip) - everything the decode call supports at 128, once more at 256.

Expectations are the ones the existing suites state: _util.check_kvcache_rows (the C oracle on each sequence's valid prefix, the relative
metric against fp64 math) and test_kvcache_window_gpu.check_window_rows under _util.TOL / _util.LSE_TOL; the soft-capped call under the rule
of test_kvcache_softcap_gpu.py (exact / check); bit-for-bit contracts as the paged, FP8, rotary and ragged suites state them.  No new
tolerance.  Every test fails on a library without head_dim 256, where the call raises.  Capacities stay <= 1200 keys."""
import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from test_kvcache_fp8_gpu import _descale, deq, quantise
from test_kvcache_ragged_gpu import _cu
from test_kvcache_rotary_gpu import assert_same, expected_cache, rotary_and_plain, tables
from test_kvcache_softcap_gpu import assert_groups, exact, split_rows
from test_kvcache_window_gpu import _bounds, check_window_rows

pytestmark = pytest.mark.gpu

D = 256
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
F8 = torch.float8_e4m3fn
NAN = float("nan")


def _rand(shape, dt, gen, dev, mult=1.0):
    return (torch.randn(*shape, device=dev, dtype=torch.float32, generator=gen) * mult).to(dt)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _page(k, v, P, seed, extra=2):
    """a pool + shuffled block table holding the logical caches (b, cap, hk, d) of any element size; unreferenced pages hold a NaN pattern"""
    b, cap, hk, d = k.shape
    cols = cap // P
    nb = b * cols + extra
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))
    table = perm[: b * cols].view(b, cols).to(torch.int32).to(k.device)
    it = {1: torch.uint8, 2: torch.int16}[k.element_size()]
    kp = torch.full((nb, P, hk, d), 0x7F if k.element_size() == 1 else U.SENT16, dtype=it, device=k.device)
    vp = kp.clone()
    kp[table.long()] = k.view(it).reshape(b, cols, P, hk, d)
    vp[table.long()] = v.view(it).reshape(b, cols, P, hk, d)
    return kp.view(k.dtype), vp.view(k.dtype), table


def _unpage(pool, table):
    b, cols = table.shape
    it = {1: torch.uint8, 2: torch.int16}[pool.element_size()]
    return torch.stack([torch.cat([pool.view(it)[table[i, c]] for c in range(cols)]) for i in range(b)]).view(pool.dtype)


# ---- 1. mixed lengths against the fp32 reference ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
def test_mixed_lengths_against_reference(gpu, dtname, causal):
    """lengths 0, 1, 63, 64, 65, a non-multiple of the split chunk and the capacity; MHA, GQA 4, MQA 8; seqlen_q 1, 2, 4, 16 and 17 (a second
    row tile under MHA, up to nine under MQA); dead rows exactly O = 0, LSE = 0"""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(11 + D + int(causal))
    cap = 1200
    lens = [0, 1, 63, 64, 65, 777, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for h, hk in ((4, 4), (8, 2), (8, 1)):
        k_cache, v_cache = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
        for sq in (1, 2, 4, 16, 17):
            q = _rand((b, sq, h, D), dt, gen, gpu)
            out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, causal=causal, return_softmax_lse=True)
            assert out.shape == q.shape and out.dtype == dt and lse.shape == (b, h, sq) and lse.dtype == torch.float32
            U.check_kvcache_rows(out, lse, q, k_cache, v_cache, lens, causal, dtname, f"d256 {dtname} h{h}/{hk} sq{sq} causal={causal}")


# ---- 2. where the columns of O and the d-chunks of Q K^T go ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("kv", ["16bit", "fp8"])
def test_every_output_column_comes_from_its_v_column(gpu, dtname, kv):
    """every V row is the same ramp - c / 256 with a 16-bit cache (exact in fp16 and bf16); with an 8-bit cache the e4m3 value of code c (the
    two NaN codes replaced by their neighbours), exact in e4m3, fp16 and bf16 alike.  O is a convex combination of equal rows, so it must
    equal the ramp to one ulp of the output in every live row, whatever P is - a d-chunk or O-block permutation, or a wrong column in the
    32-byte store, cannot pass.  One and three splits."""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(3)
    lens = [1, 33, 200, 640]
    b, cap, h, hk = len(lens), 640, 8, 2
    if kv == "16bit":
        ramp = torch.arange(D, device=gpu) / 256.0
    else:
        codes = torch.arange(D, dtype=torch.int16).to(torch.uint8)
        codes[0x7F], codes[0xFF] = 0x7E, 0xFE
        ramp = codes.view(F8).float().to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k = _rand((b, cap, hk, D), dt, gen, gpu)
    v = ramp.to(dt).expand(b, cap, hk, D).contiguous()
    assert torch.equal(v[0, 0, 0].float(), ramp.float())
    if kv == "fp8":
        k, v = k.to(F8), v.to(F8)
        assert torch.equal(v[0, 0, 0].float(), ramp.float())
    for sq in (1, 5, 17):
        q = _rand((b, sq, h, D), dt, gen, gpu)
        for ns in (1, 3):
            out = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, num_splits=ns).float()
            err = (out - ramp.float()).abs()
            assert bool((err <= U.ULP[dtname] * ramp.float().abs()).all()), (dtname, kv, sq, ns, float(err.max()), int(err.flatten(0, 2).max(0).values.argmax()))


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("kv", ["16bit", "fp8"])
def test_every_group_of_eight_q_elements_meets_its_k_elements(gpu, dtname, kv):
    """batch entry i has q non-zero only in d-elements 8 i .. 8 i + 7 (32 groups): the scores depend on K's elements of that group alone, so a
    wrong pairing of the d-chunks of K and Q^T (the 8-bit kernels load K with a permutation that Q must follow) moves LSE and O"""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(5)
    b, cap, h, hk, sq = 32, 96, 4, 2, 2
    lens = [96 - (i % 5) for i in range(b)]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
    q = torch.zeros(b, sq, h, D, dtype=dt, device=gpu)
    for i in range(b):
        q[i, :, :, 8 * i:8 * i + 8] = _rand((sq, h, 8), dt, gen, gpu, mult=8.0)
    if kv == "fp8":
        k8, v8 = k.to(F8), v.to(F8)
        out, lse = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, return_softmax_lse=True)
        k, v = k8.to(dt), v8.to(dt)                            # (exact)
    else:
        out, lse = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, return_softmax_lse=True)
    U.check_kvcache_rows(out, lse, q, k, v, lens, False, dtname, f"d256 d-groups {dtname} {kv}")
    # the case tells the groups apart: LSE of neighbouring entries differs by far more than the tolerance
    assert float((lse[1:] - lse[:-1]).abs().mean()) > 100 * U.LSE_TOL


# ---- 3. append ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("kv", ["16bit", "fp8"])
@pytest.mark.parametrize("P", [0, 16, 48])
def test_append_writes_its_rows_and_nothing_else(gpu, dtname, kv, P):
    """three new rows per sequence land in the cache bit for bit - the 8-bit codes are the documented quantiser's - and every other byte of the
    cache (the pool: pages of other sequences and unreferenced ones included) keeps its bits; contiguous, and paged with rows crossing a page.
    The rows of the bit contract are 3 x N(0, 1), which reaches further into the quantiser's range.  That the call attends to what it appended
    is checked on a second call with N(0, 1) rows, the data of test_kvcache_gpu.py's append test: with rows three times as large the softmax of
    a 50-key causal row collapses onto the new keys, and the raw relative metric over its 3 x 4 x 256 elements is set by the few that cancel
    to about 0 - measured on the first GPU run of this file (bf16, contiguous, L = 50): max_abs and mean_abs inside their bounds, the C oracle's
    own mean_rel 5.3e-2 of a bound of 8e-2, the kernel's 1.7e-1.  The case was ill-conditioned for that metric, not the tolerance too tight."""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(17 + P)
    cap, sn, h, hk = 96, 3, 4, 2
    lens = [0, 15, 46, 47, 93, 60]                              # rows 15 .. 17 cross a 16-row page, 46 .. 48 and 47 .. 49 a 48-row page; 93 .. 95 end at the capacity
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kds, vds = (_descale(b, hk, torch.Generator().manual_seed(1), gpu), _descale(b, hk, torch.Generator().manual_seed(2), gpu)) if kv == "fp8" else (None, None)
    k0, v0 = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
    if kv == "fp8":
        k0, v0 = quantise(k0, kds).to(gpu), quantise(v0, vds).to(gpu)
    k_new, v_new = _rand((b, sn, hk, D), dt, gen, gpu, mult=3.0), _rand((b, sn, hk, D), dt, gen, gpu, mult=3.0)
    q = _rand((b, sn, h, D), dt, gen, gpu)
    rows_k, rows_v = (quantise(k_new, kds), quantise(v_new, vds)) if kv == "fp8" else (k_new, v_new)
    k_exp, v_exp = expected_cache(k0, rows_k, lens).to(gpu), expected_cache(v0, rows_v, lens).to(gpu)
    kw = dict(k_descale=kds, v_descale=vds) if kv == "fp8" else {}
    if P:
        kc, vc, table = _page(k0, v0, P, seed=P)
        kp_exp, vp_exp, _ = _page(k_exp, v_exp, P, seed=P)
        out, lse = F.flash_attn_with_kvcache(q, kc, vc, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, block_table=table, **kw)
        torch.cuda.synchronize()
        assert _same(kc, kp_exp) and _same(vc, vp_exp), "pool bytes differ from: the new rows in place, everything else untouched"
        assert _same(_unpage(kc, table), k_exp)
    else:
        kc, vc = k0.clone(), v0.clone()
        out, lse = F.flash_attn_with_kvcache(q, kc, vc, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, **kw)
        torch.cuda.synchronize()
        assert _same(kc, k_exp) and _same(vc, v_exp), "cache bytes differ from: the new rows in place, everything else untouched"
    assert not _same(k_exp, k0) and cs.tolist() == lens
    # ... and the call attends to what it appended (N(0, 1) rows, over the caches as the first call left them)
    k_new, v_new = _rand((b, sn, hk, D), dt, gen, gpu), _rand((b, sn, hk, D), dt, gen, gpu)
    out, lse = F.flash_attn_with_kvcache(q, kc, vc, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, **(dict(block_table=table) if P else {}), **kw)
    rows_k, rows_v = (quantise(k_new, kds), quantise(v_new, vds)) if kv == "fp8" else (k_new, v_new)
    k_exp, v_exp = expected_cache(k0, rows_k, lens).to(gpu), expected_cache(v0, rows_v, lens).to(gpu)
    assert _same(_unpage(kc, table) if P else kc, k_exp) and _same(_unpage(vc, table) if P else vc, v_exp)
    k_log, v_log = (deq(k_exp, kds), deq(v_exp, vds)) if kv == "fp8" else (k_exp, v_exp)
    U.check_kvcache_rows(out, lse, q, k_log, v_log, [L + sn for L in lens], True, dtname, f"d256 append {dtname} {kv} P{P}")


# ---- 4. paged against contiguous ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("kv", ["16bit", "fp8"])
def test_paged_and_contiguous_give_the_same_bits(gpu, dtname, kv):
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(29)
    cap, h, hk = 576, 8, 2
    lens = [0, 1, 47, 48, 49, 333, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
    kw = {}
    if kv == "fp8":
        kds, vds = _descale(b, hk, torch.Generator().manual_seed(3), gpu), _descale(b, hk, torch.Generator().manual_seed(4), gpu)
        k, v, kw = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu), dict(k_descale=kds, v_descale=vds)
    for P in (16, 48):
        kp, vp, table = _page(k, v, P, seed=100 + P)
        for sq, causal, window, ns in ((1, False, (-1, -1), 0), (1, False, (-1, -1), 1), (17, True, (-1, -1), 3), (4, True, (31, 0), 2), (3, False, (127, 3), 1)):
            q = _rand((b, sq, h, D), dt, gen, gpu)
            args = dict(cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, **kw)
            o_p, l_p = F.flash_attn_with_kvcache(q, kp, vp, block_table=table, **args)
            o_c, l_c = F.flash_attn_with_kvcache(q, k, v, **args)
            assert _same(o_p, o_c) and _same(l_p, l_c), (dtname, kv, P, sq, causal, window, ns)
    k_log, v_log = (deq(k, kds), deq(v, vds)) if kv == "fp8" else (k, v)
    check_window_rows(o_p, l_p, q, k_log, v_log, lens, window, causal, dtname, f"d256 paged {dtname} {kv}")


# ---- 5. the 8-bit cache, read side -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
def test_fp8_cache_equals_the_16bit_call_on_the_dequantised_cache(gpu, dtname, causal):
    """per-(batch, head) descales, and once an expand()-ed scalar, against the reference on the dequantised cache under the 16-bit tolerances"""
    dt = DT[dtname]
    g = torch.Generator().manual_seed(41 + int(causal))
    gen = torch.Generator(device=gpu).manual_seed(41)
    cap = 1200
    lens = [0, 1, 63, 64, 65, 777, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for (h, hk), sq in (((4, 4), 1), ((8, 2), 4), ((8, 1), 17)):
        kds, vds = _descale(b, hk, g, gpu), _descale(b, hk, g, gpu)
        k8, v8 = quantise(torch.randn(b, cap, hk, D, generator=g), kds).to(gpu), quantise(torch.randn(b, cap, hk, D, generator=g), vds).to(gpu)
        q = _rand((b, sq, h, D), dt, gen, gpu)
        out, lse = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=causal, return_softmax_lse=True, k_descale=kds, v_descale=vds)
        U.check_kvcache_rows(out, lse, q, deq(k8, kds), deq(v8, vds), lens, causal, dtname, f"d256 fp8 {dtname} h{h}/{hk} sq{sq} causal={causal}")
    one_k, one_v = torch.tensor(0.37, device=gpu).expand(b, hk), torch.tensor(2.9, device=gpu).expand(b, hk)
    assert one_k.stride() == (0, 0)
    out_e, lse_e = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=causal, return_softmax_lse=True, k_descale=one_k, v_descale=one_v)
    out_d, lse_d = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=causal, return_softmax_lse=True, k_descale=one_k.contiguous(), v_descale=one_v.contiguous())
    assert _same(out_e, out_d) and _same(lse_e, lse_d)
    U.check_kvcache_rows(out_e, lse_e, q, deq(k8, one_k), deq(v8, one_v), lens, causal, dtname, f"d256 fp8 scalar descale {dtname} causal={causal}")


# ---- 6. sliding windows ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("window", [(0, 0), (31, 0), (127, 3), (7, -1)])
def test_sliding_windows_against_reference_with_unseen_rows_poisoned(gpu, dtname, window):
    """rows below the first row's window and at or past L hold NaN, +inf, -inf and 65504 in the caches the kernel reads; the expectation is
    computed from the clean caches"""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(53 + window[0])
    causal = window[1] == 0
    cap = 640
    lens = [0, 1, 31, 32, 33, 437, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for (h, hk), sq, ns in (((4, 4), 1, 1), ((8, 2), 4, 0), ((8, 1), 17, 2), ((8, 2), 16, 5)):
        k, v = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
        kp, vp = k.clone(), v.clone()
        for i, L in enumerate(lens):
            lo = min(_bounds(L, sq, t, window, causal)[0] for t in range(sq))
            for c in (kp, vp):
                if lo > 0:
                    U.poison_(c[i, :lo])
                if L < cap:
                    U.poison_(c[i, L:])
        q = _rand((b, sq, h, D), dt, gen, gpu)
        out, lse = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(lse).all()), "a poisoned row reached a result"
        check_window_rows(out, lse, q, k, v, lens, window, causal, dtname, f"d256 {dtname} w={window} h{h}/{hk} sq{sq} ns={ns}")


# ---- 7. splits ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_split_counts_meet_the_tolerance_and_are_deterministic(gpu, dtname):
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(61)
    cap, h, hk, sq = 1200, 8, 2, 2
    lens = [1200, 777, 65, 0]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
    q = _rand((b, sq, h, D), dt, gen, gpu)
    kn, vn = k.clone(), v.clone()
    for i, L in enumerate(lens):                            # rows at or past L hold NaN: nothing may change
        kn[i, L:], vn[i, L:] = NAN, NAN
    for ns in (1, 2, 5, 0):
        out, lse = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True)
        out2, lse2 = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True)
        assert _same(out, out2) and _same(lse, lse2), f"num_splits={ns}: not deterministic"
        out3, lse3 = F.flash_attn_with_kvcache(q, kn, vn, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True)
        assert _same(out, out3) and _same(lse, lse3), f"num_splits={ns}: a cache row at or past L was read"
        U.check_kvcache_rows(out, lse, q, k, v, lens, False, dtname, f"d256 {dtname} num_splits={ns}")


@pytest.mark.parametrize("num_splits", [1, 2, 5, 0])
def test_nan_in_a_visible_k_row_makes_the_row_nan(gpu, num_splits):
    """K row 700 of (batch 0, KV head 1) holds a NaN: the rows of that KV head's query heads that see it are NaN in O and LSE, for every split
    count; every other row keeps the bits of the clean call"""
    dt = torch.float16
    gen = torch.Generator(device=gpu).manual_seed(67)
    cap, h, hk, sq = 1200, 8, 2, 3
    lens = [1200, 650]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((2, cap, hk, D), dt, gen, gpu), _rand((2, cap, hk, D), dt, gen, gpu)
    q = _rand((2, sq, h, D), dt, gen, gpu)
    out0, lse0 = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True)
    kb = k.clone()
    kb[0, 700, 1, 200] = NAN
    kb[1, 700, 1, 200] = NAN                                # (past L = 650 of batch 1: never read)
    out, lse = F.flash_attn_with_kvcache(q, kb, v, cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True)
    hit = torch.zeros(2, sq, h, dtype=torch.bool, device=gpu)
    hit[0, :, 4:] = True                                    # KV head 1 serves query heads 4 .. 7
    assert bool(torch.isnan(out[hit]).all()) and bool(torch.isnan(lse.permute(0, 2, 1)[hit]).all())
    assert torch.equal(_bits(out)[~hit], _bits(out0)[~hit]) and torch.equal(_bits(lse.permute(0, 2, 1))[~hit], _bits(lse0.permute(0, 2, 1))[~hit])


# ---- 8. rotary -----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("rotary_dim", [256, 64])
@pytest.mark.parametrize("inter", [False, True])
def test_rotary_equals_the_plain_call_on_rotated_inputs(gpu, dtname, rotary_dim, inter):
    """out, lse and every cache byte of the rotary call are those of the plain call on q / k rotated with torch in fp32 (rotate_ref): 16-bit
    contiguous, 8-bit paged; plain, causal and windowed (the query-position rule); one, three and automatic splits"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(71 + rotary_dim + int(inter))
    cap, h, hk = 320, 8, 2
    ro = cap + 8
    cos, sin = tables(ro, rotary_dim, dt)
    for (sq, sn), causal, window, ns in (((1, 1), False, (-1, -1), 0), ((4, 4), True, (-1, -1), 1), ((17, 3), False, (37, 0), 3)):
        lens = [0, 1, 63, 64, 65, cap - sn]
        b = len(lens)
        rnd = lambda *shape: torch.randn(*shape, generator=gen).to(dt)
        k0, v0 = rnd(b, cap, hk, D), rnd(b, cap, hk, D)
        q, k_new, v_new = rnd(b, sq, h, D), rnd(b, sn, hk, D), rnd(b, sn, hk, D)
        tag = f"d256 {dtname} rd{rotary_dim} inter={inter} sq{sq} sn{sn} causal={causal} win={window} ns={ns}"
        out, lse, ka, va, q_rot, k_rot = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=causal, window=window, num_splits=ns, tag=tag)
        assert_same(ka, expected_cache(k0, k_rot, lens).to(gpu), tag + ": k_cache against rotate_ref")
        assert_same(va, expected_cache(v0, v_new, lens).to(gpu), tag + ": v_cache against v")
        if rotary_dim < D:
            assert torch.equal(_bits(ka.cpu())[0, :sn, :, rotary_dim:], _bits(k_new)[0, :, :, rotary_dim:]), tag + ": elements past rotary_dim pass through"
        assert not torch.equal(_bits(k_rot)[2], _bits(k_new)[2]), tag + ": the rotation does something"
        # the same through an 8-bit paged cache: the rotated row is rounded to q's dtype, then quantised
        kds, vds = _descale(b, hk, gen, "cpu"), _descale(b, hk, gen, "cpu")
        k8, v8 = quantise(k0, kds), quantise(v0, vds)
        kp, vp, table = _page(k8, v8, 16, seed=sq)
        out8, lse8, kpa, vpa, _, _ = rotary_and_plain(gpu, q, k_new, v_new, kp, vp, lens, cos, sin, inter, causal=causal, window=window, num_splits=ns,
                                                      block_table=table, k_descale=kds, v_descale=vds, tag=tag + " fp8 paged")
        assert_same(_unpage(kpa, table.to(gpu)), expected_cache(k8, quantise(k_rot, kds), lens).to(gpu), tag + ": 8-bit k_cache against quantise(rotate_ref)")


# ---- 9. ragged query batches ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("variant", ["append", "paged", "fp8"])
def test_sequence_of_a_ragged_call_is_the_dense_call_on_it_alone(gpu, dtname, variant):
    """sq_i in {0, 1, 3, 16, 17}: out and lse of sequence i are the bits of the dense call on it alone, for one split and a forced three; with
    an append the cache bytes are those the dense appends leave; over a paged and over an 8-bit cache alike"""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(83)
    sq = [1, 0, 3, 16, 17, 1]
    sn = sq if variant == "append" else [0] * len(sq)
    lens0 = [0, 77, 63, 300, 555, 621]
    cap, h, hk, P = 640, 8, 2, 16
    b, total = len(sq), sum(sq)
    cs = torch.tensor(lens0, dtype=torch.int32, device=gpu)
    cu = _cu(sq, gpu)
    k, v = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
    q = _rand((total, h, D), dt, gen, gpu)
    kn, vn = _rand((total, hk, D), dt, gen, gpu), _rand((total, hk, D), dt, gen, gpu)
    kw, table = {}, None
    if variant == "fp8":
        kds, vds = _descale(b, hk, torch.Generator().manual_seed(5), gpu), _descale(b, hk, torch.Generator().manual_seed(6), gpu)
        k, v, kw = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu), dict(k_descale=kds, v_descale=vds)
    if variant == "paged":
        k, v, table = _page(k, v, P, seed=9)
    for causal, ns in ((True, 1), (False, 3), (True, 3)):
        kr, vr, kd_, vd_ = k.clone(), v.clone(), k.clone(), v.clone()
        app = dict(k=kn, v=vn, cu_seqlens_k_new=cu) if variant == "append" else {}
        out, lse = F.flash_attn_with_kvcache(q, kr, vr, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max(sq),
                                             block_table=table, **app, **kw)
        assert out.shape == q.shape and lse.shape == (h, total)
        for i in range(b):
            if sq[i] == 0:
                continue
            c0 = sum(sq[:i])
            kwi = {n: t[i:i + 1] for n, t in kw.items()}
            if table is not None:
                kwi["block_table"] = table[i:i + 1]
            appi = dict(k=kn[c0:c0 + sn[i]][None], v=vn[c0:c0 + sn[i]][None]) if variant == "append" else {}
            od, ld = F.flash_attn_with_kvcache(q[c0:c0 + sq[i]][None], kd_ if table is not None else kd_[i:i + 1], vd_ if table is not None else vd_[i:i + 1],
                                               cache_seqlens=cs[i:i + 1], causal=causal, num_splits=ns, return_softmax_lse=True, **appi, **kwi)
            assert _same(out[c0:c0 + sq[i]], od[0]) and _same(lse[:, c0:c0 + sq[i]], ld[0]), (dtname, variant, causal, ns, i)
        assert _same(kr, kd_) and _same(vr, vd_), "cache bytes differ from the per-sequence dense calls"
        assert _same(kr, k) != (variant == "append")
    # ... and the dense call is right: the ragged result against the reference, sequence by sequence
    k_log, v_log = (_unpage(kr, table), _unpage(vr, table)) if table is not None else (kr, vr)
    if variant == "fp8":
        k_log, v_log = deq(k_log, kds), deq(v_log, vds)
    for i in range(b):
        L = lens0[i] + sn[i]
        if sq[i] and sq[i] <= L:
            c0 = sum(sq[:i])
            U.check_kvcache_rows(out[c0:c0 + sq[i]][None], lse[:, c0:c0 + sq[i]][None], q[c0:c0 + sq[i]][None], k_log[i:i + 1], v_log[i:i + 1], [L], True, dtname,
                                 f"d256 ragged {variant} {dtname} seq{i}")


# ---- 10. soft-capped scores ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("causal", [False, True])
def test_softcap_30_with_a_scale_of_its_own_against_fp64(gpu, dtname, causal):
    """softcap = 30 and softmax_scale = 2 / sqrt(d) on q x 4 (raw scores reach the cap's bend) under the rule of test_kvcache_softcap_gpu.py:
    dead rows and LSE per call, O over the calls of one split count together, per group; the capped paged call gives the capped contiguous
    call's bits"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(97 + int(causal))
    cap, softcap, scale = 1024, 30.0, 2.0 / 16.0
    lens = [0, 1, 31, 33, 64, 100, 777, 1000]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    parts = {ns: [] for ns in (1, 0, 5)}
    for sq, h, hk in ((1, 4, 4), (3, 8, 2), (17, 8, 1)):
        k, v = torch.randn(b, cap, hk, D, generator=gen).to(dt), torch.randn(b, cap, hk, D, generator=gen).to(dt)
        q = (torch.randn(b, sq, h, D, generator=gen) * 4.0).to(dt)
        kg, vg, qg = k.to(gpu), v.to(gpu), q.to(gpu)
        tag = f"d256 {dtname} sq{sq} h{h}/{hk} causal={causal} cap=30 scale=2/sqrt(d)"
        xo, xl, nvis = exact(q, k, v, lens, scale=scale, cap=softcap, causal=causal)
        x0, _, _ = exact(q, k, v, lens, causal=causal)
        assert float((xo - x0).abs().mean()) >= 4 * U.TOL[dtname]["mean_abs"], f"{tag}: the case does not tell the two arguments from the defaults"
        for ns in parts:
            out, lse = F.flash_attn_with_kvcache(qg, kg, vg, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, softmax_scale=scale, softcap=softcap)
            assert bool(torch.isfinite(out).all()), tag
            parts[ns].append(split_rows(out, lse, xo, xl, nvis, f"{tag} splits={ns}"))
        kp, vp, table = _page(kg, vg, 16, seed=sq)
        o_p, l_p = F.flash_attn_with_kvcache(qg, kp, vp, cache_seqlens=cs, causal=causal, num_splits=5, return_softmax_lse=True, softmax_scale=scale, softcap=softcap,
                                             block_table=table)
        assert _same(o_p, out) and _same(l_p, lse), f"{tag}: paged differs from contiguous"
    for ns, pl in parts.items():
        assert_groups(pl, dtname, f"d256 {dtname} causal={causal} cap=30 splits={ns}, the three calls")


# ---- 11. graph capture -----------------------------------------------------------------------------------------------------------------------------------

def test_graph_capture_replays_with_new_lengths(gpu):
    """one capture on one stream (the automatic split: attention and combine), replayed with cache_seqlens changed in between"""
    dt, h, hk, cap = torch.float16, 8, 2, 1200
    gen = torch.Generator(device=gpu).manual_seed(13)
    b = 2
    k, v = _rand((b, cap, hk, D), dt, gen, gpu), _rand((b, cap, hk, D), dt, gen, gpu)
    q = _rand((b, 1, h, D), dt, gen, gpu)
    cs = torch.tensor([100, 1000], dtype=torch.int32, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, return_softmax_lse=True)
    for lens in ([100, 1000], [650, 1], [1200, 0]):
        cs.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        out_e, lse_e = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, return_softmax_lse=True)
        assert _same(out_g, out_e) and _same(lse_g, lse_e), lens
        U.check_kvcache_rows(out_g, lse_g, q, k, v, lens, False, "fp16", f"d256 graph {lens}")


# ---- 12. what stays rejected -------------------------------------------------------------------------------------------------------------------------------

def test_other_head_dims_and_the_prefill_entry_points_still_raise(gpu):
    dt = torch.float16
    q, k = torch.zeros(1, 16, 2, D, device=gpu, dtype=dt), torch.zeros(1, 16, 2, D, device=gpu, dtype=dt)
    with pytest.raises(RuntimeError, match="head_dim 256 unsupported"):
        F.fwd(q, k, k, False)
    with pytest.raises(RuntimeError, match="head_dim 256 unsupported"):
        F.flash_attn_func(q, k, k)
    for d in (96, 192):
        qd, cd = torch.zeros(1, 1, 2, d, device=gpu, dtype=dt), torch.zeros(1, 32, 2, d, device=gpu, dtype=dt)
        with pytest.raises((ValueError, RuntimeError), match=f"head_dim {d} unsupported"):
            F.flash_attn_with_kvcache(qd, cd, cd, cache_seqlens=4)
        with pytest.raises(RuntimeError, match=f"head_dim {d} unsupported"):                # the library itself, under the Python check
            F._C.fwd_kvcache(qd, cd, cd, None, None, torch.full((1,), 4, dtype=torch.int32, device=gpu), False, 0, None, -1, -1)
    # an 8-bit d-256 view whose row stride is no multiple of 16 elements: the library's stride rule, unchanged
    buf = torch.zeros(1, 32, 2 * D + 8, device=gpu, dtype=torch.uint8).view(F8)
    c8 = buf[:, :, :2 * D].view(1, 32, 2, D)
    assert c8.stride(1) % 16 == 8
    with pytest.raises(RuntimeError, match="16"):
        F.flash_attn_with_kvcache(torch.zeros(1, 1, 2, D, device=gpu, dtype=dt), c8, c8, cache_seqlens=4)
    t = torch.zeros(40, 136, device=gpu, dtype=dt)
    with pytest.raises(ValueError, match="rotary_dim"):
        F.flash_attn_with_kvcache(q[:, :1], k, k, k=k[:, :1], v=k[:, :1], cache_seqlens=4, rotary_cos=t, rotary_sin=t)
