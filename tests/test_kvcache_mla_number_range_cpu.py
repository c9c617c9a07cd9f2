"""CPU: the cases of tests/test_kvcache_mla_number_range_gpu.py are what that file says they are.  No kernel runs here.  The builders live in
tests/_mla_cases.py; this file counts their pattern sets, checks the numpy expectation of the FP8 dequantisation (and its bf16 rounder) against torch
and against dequantize_mla_kv_cache, checks that the midpoint tiles of the quantising append straddle code boundaries under quantize_mla_kv_cache,
counts the amax values on which a reciprocal-multiply would differ from the division, asserts the LSE gap of the softmax extremes, the NaN pattern of
the fp64 reference of the rope-column infinities, the pages of the pools larger than 4 GiB and the refusal of a sequence of 2^31 bytes."""
import numpy as np
import pytest
import torch

import _mla_cases as C
import flash_attn_turing as F
from test_kvcache_number_formats_gpu import SCORE_LIMIT_EXP
from test_kvcache_prefill_gpu import visible
from test_kvcache_tree_gpu import exact, scores64

DTS = ["fp16", "bf16"]
N_FINITE = {"fp16": 63488, "bf16": 65280}
N_POSITIVE = {"fp16": 31743, "bf16": 32639}
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(C.DK)))


def _u16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


# ---- A, B, D: the pattern sets are complete ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", DTS)
def test_a_and_b_hold_every_finite_pattern(dtname):
    dt = C.DT[dtname]
    rows = C.a_rows(dt)
    assert rows.shape == ({"fp16": 124, "bf16": 128}[dtname], C.DK)
    assert len(np.unique(_u16(rows[:, :C.DV]))) == N_FINITE[dtname] and torch.isfinite(rows.float()).all()
    lim = SCORE_LIMIT_EXP if dtname == "bf16" else None
    n = C.finite_patterns(dt, lim).numel()
    assert n == (N_FINITE["fp16"] if dtname == "fp16" else 2 * 128 * (127 + SCORE_LIMIT_EXP))       # bf16: exponent fields 0 .. 156
    keys = C.b_key_rows(dt, lim)
    assert len(np.unique(_u16(keys))) == n and (keys.float().abs() < 2.0 ** 31).all()
    # B (i): the 640 (token, head) pairs of a sequence read all 576 columns
    q, j = C.b_onehot_q(keys.shape[0], dt)
    assert all(len(torch.unique(j[i])) == C.DK for i in (0, 1, keys.shape[0] - 1)) and (q.sum(-1) == 1).all()
    read = keys[torch.arange(keys.shape[0]).view(-1, 1, 1), j]
    assert len(np.unique(_u16(read))) == n
    # B (ii): 65536 query rows, the one-hot column of a row's sequence holds pattern r % n
    jrow = (torch.arange(65536) // 128 * 7 + 3) % C.DK
    qr = C.b_query_rows(dt, lim, 65536, jrow)
    assert len(np.unique(_u16(qr[torch.arange(65536), jrow]))) == n and len(np.unique(_u16(qr))) == n


@pytest.mark.parametrize("dtname", DTS)
def test_b_and_c_fp8_rows_hold_every_code_in_every_tile_inside_the_precondition(dtname):
    dt = C.DT[dtname]
    rows = C.b_fp8_rows(dt)
    for k in range(len(C.B8_SCALES)):
        for g in range(4):
            assert len(np.unique(rows[2 * k:2 * k + 2, 128 * g:128 * g + 128].numpy())) == 254
    crow = C.c_rows(dt)
    sc = C.c_scales()
    assert crow.shape == (62, C.RB) and len(np.unique(crow[:, :C.DV].numpy())) == 254
    e = np.log2(np.abs(sc.numpy().astype(np.float64)[:59].reshape(-1)))
    assert np.array_equal(e, np.arange(C.C_EXP[0], C.C_EXP[1] + 1).astype(np.float64))
    # the precondition: every fp32(code) x scale is zero or a normal fp32 number - and the sweep reaches both ends of it
    val = C.e4m3_values()[crow[:, :C.DV].numpy()].reshape(62, 4, 128)
    prod = np.abs(val * sc.numpy().astype(np.float64)[:, :, None])
    nz = prod[prod > 0]
    assert nz.min() == 2.0 ** -126 and nz.max() == 448 * 2.0 ** 118 and nz.max() < 2.0 ** 128
    for s in (0.3, 3.7, 1 / 448, 65504 / 448, -1.0, -0.3, 0.0):
        assert (sc == np.float32(s)).any(), s


# ---- C: the expectation -----------------------------------------------------------------------------------------------------------------------------------------

def test_c_bf16_rounder_is_torchs():
    gen = torch.Generator().manual_seed(93500)
    bits = torch.randint(-2 ** 31, 2 ** 31, (1 << 20,), generator=gen, dtype=torch.int64).to(torch.int32)
    hi = torch.arange(65536, dtype=torch.int32)
    edge = torch.cat([(hi << 16) | lo for lo in (0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF)])       # every bf16 value with the ties and their neighbours behind it
    x = torch.cat([bits, edge]).view(torch.float32)
    x = x[~torch.isnan(x)]
    assert x.numel() > 1_300_000
    assert np.array_equal(C.round_bf16_bits(x.numpy()), _u16(x.to(torch.bfloat16)))


@pytest.mark.parametrize("dtname", DTS)
def test_c_numpy_expectation_is_dequantize_mla_kv_cache(dtname):
    dt = C.DT[dtname]
    assert np.array_equal(C.e4m3_values()[C.nan_free_codes().numpy()], C.nan_free_codes().view(torch.float8_e4m3fn).double().numpy())
    n_over = 0
    for rows in (C.c_rows(dt), C.b_fp8_rows(dt)):
        want = C.dequant_expect_bits(rows[:, :C.DV].numpy(), rows[:, C.DV:C.DV + 16].contiguous().view(torch.float32).numpy(), dtname)
        got = F.dequantize_mla_kv_cache(rows, dt)
        assert np.array_equal(_u16(got[:, :C.DV]), want)
        assert np.array_equal(got[:, C.DV:].contiguous().view(torch.uint8).numpy(), rows[:, C.DV + 16:].numpy())
        n_over += int(torch.isinf(got).any(-1).sum())
        assert not torch.isnan(got).any()
    # fp16 overflows from 448 x 2^8 on: rows 32 .. 58 of the sweep and the row of 65504 / 448's upper neighbour stay finite or not as the GPU file expects
    assert n_over == ({"fp16": 28, "bf16": 0}[dtname]), n_over


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", DTS)
def test_d_tiles_sweep_every_amax_and_midpoints_straddle_code_boundaries(dtname):
    dt = C.DT[dtname]
    kv_new, amax, (tt, cc, kk) = C.d_kv_new(dt)
    assert kv_new.shape == (C.D_B, C.D_SNEW, 1, C.DK) and torch.isfinite(kv_new.float()).all()
    assert len(torch.unique(amax[amax > 0])) == N_POSITIVE[dtname] == int((amax > 0).sum()) and int((amax == 0).sum()) == 32768 - N_POSITIVE[dtname]
    tiles = kv_new[..., :C.DV].reshape(-1, 128)
    assert torch.equal(tiles.float().abs().amax(-1), C.i16(amax).view(dt).float())
    mags = tiles.view(torch.int16).to(torch.int32) & 0x7FFF
    even = torch.arange(32768) % 2 == 0
    sub = 0x03FF if dtname == "fp16" else 0x007F
    assert int(((mags[even] > 0) & (mags[even] <= sub)).sum()) > 1000 and int((tiles[even] == 0).sum()) > 20000 and int((tiles[even] < 0).sum()) > 500000
    # the 2^-24 clamp: fp16 reaches it exactly (its smallest subnormal), bf16 goes below it
    n_clamped = int(((C.i16(amax).view(dt).float() <= 2.0 ** -24) & (amax > 0)).sum())
    assert n_clamped == (1 if dtname == "fp16" else 103 * 128), n_clamped
    # the scale words: the helper's are the correctly rounded quotient; a reciprocal-multiply differs on `n_recip` of the amax values
    q8 = F.quantize_mla_kv_cache(kv_new)
    words = q8[..., C.DV:C.DV + 16].contiguous().view(torch.float32).reshape(-1).numpy()
    quot, recip = C.d_scale_words(amax, dt)
    assert np.array_equal(words.view(np.uint32), quot.view(np.uint32))
    n_recip = int((quot.view(np.uint32) != recip.view(np.uint32)).sum())
    print(f"D {dtname}: a reciprocal-multiply scale differs from the division on {n_recip} of {N_POSITIVE[dtname]} amax values")
    assert n_recip > 1000, "the sweep must separate the division from a reciprocal-multiply"
    # the midpoint triples: the 16-bit values on either side of scale x midpoint get different codes
    codes = (q8[..., :C.DV].reshape(-1, 128).to(torch.int32) & 0x7F)
    lo, mid, hi = codes[tt, (cc - 1) % 128], codes[tt, cc], codes[tt, (cc + 1) % 128]
    straddle = hi > lo
    # (a triple is whole only where its upper neighbour is below amax; below the 2^-24 clamp - 40 % of the bf16 tiles - the scale no longer follows amax and
    # most triples are cut off at amax: those tiles exercise the clamp, not the ties)
    mag = tiles.view(torch.int16).to(torch.int32) & 0x7FFF
    whole = mag[tt, (cc + 1) % 128] == mag[tt, cc] + 1
    frac = float(straddle[whole].float().mean())
    print(f"D {dtname}: {int(whole.sum())} of {whole.numel()} midpoint triples are whole, {int(straddle[whole].sum())} of them straddle a code boundary ({frac:.4f})")
    assert frac > 0.99 and int(whole.sum()) > 400000 and (hi >= mid).all() and (mid >= lo).all()
    assert len(torch.unique(kk[straddle & whole])) == 126, "every midpoint between neighbouring codes is straddled somewhere"
    # ... and exact ties exist: the centre divided by the scale IS the midpoint in fp32
    x = tiles[tt, cc].float().abs().numpy() / quot[tt.numpy()]
    ties = int((x.astype(np.float64) == C.e4m3_midpoints()[kk.numpy()]).sum())
    print(f"D {dtname}: {ties} exact ties")
    assert ties > 100
    pre = C.d_prefix_lengths()
    assert set(p % 16 for p in pre) == set(range(16)) and max(pre) + C.D_SNEW <= C.D_CAP


# ---- E ------------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", DTS)
def test_e_references_are_finite_and_the_gap_exceeds_100(dtname):
    dt = C.DT[dtname]
    for pattern in C.E_PATTERNS:
        q, kv = C.e_case(pattern, dt)
        s = scores64(q, kv, SCALE)
        for causal in (False, True):
            vis = visible([C.E_L], C.E_SQ, C.E_CAP, causal)
            xo, xl, nvis = exact(s, kv[..., :C.DV], vis)
            assert torch.isfinite(xo).all() and torch.isfinite(xl).all() and int(nvis.min()) >= C.E_L - 1
            if pattern in C.E_GAP_BLOCK:
                rest = vis.clone()
                rest[:, :, C.E_GAP_BLOCK[pattern]] = False
                gap = float((xl - exact(s, kv[..., :C.DV], rest)[1]).min())
                assert gap > 100.0, f"{pattern} {dtname} causal={causal}: LSE gap {gap}"
        sv = s[0, 0, :, :, :C.E_L]
        if pattern == "ramp_up":
            step = float((sv[..., 32:] - sv[..., :-32]).mean()) / 32
            assert 0.1 <= step <= 0.3, step
        if pattern == "spike_last_split":
            top = sv[0, 0].topk(2).values
            assert int(sv[0, 0].argmax()) == C.E_L - 4 >= 2 * C.E_SPLIT and 12.0 <= float(top[0] - top[1]) <= 18.0
        if pattern == "scaled":
            assert float(torch.softmax(sv, -1).amax(-1).mean()) > 0.8
    lists = C.e_lists()
    for name, idx in lists.items():
        assert all(sorted(idx[0, t, :C.E_L].tolist()) == list(range(C.E_L)) for t in range(C.E_SQ)) and (idx[:, :, C.E_L:] == -1).all()
    assert lists["reversed"][0, 0, 0] == C.E_L - 1 and not torch.equal(lists["shuffled"][0, 0], lists["shuffled"][0, 1])


# ---- F ------------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", DTS)
def test_f_fp64_reference_has_nan_rows_dropped_keys_and_untouched_rows(dtname):
    dt = C.DT[dtname]
    q, kv, bad, idx = C.f_case(dt)
    assert int(torch.isinf(bad.float()).sum()) == 2 and not torch.isinf(bad[..., :C.DV].float()).any() and torch.isfinite(kv.float()).all()
    for causal in (False, True):
        (oc, lc), (ob, lb) = C.f_dense_ref(q, kv, causal), C.f_dense_ref(q, bad, causal)
        assert torch.isfinite(oc).all() and not torch.isinf(ob).any() and not torch.isinf(lb).any()
        nan = torch.isnan(lb)                                                 # (2, 24, 2)
        assert torch.equal(torch.isnan(ob).all(-1), nan.permute(0, 2, 1)) and torch.equal(torch.isnan(ob).any(-1), nan.permute(0, 2, 1))
        for i, row, col, val in C.F_POS:
            sees = torch.ones(C.F_SQ, dtype=torch.bool) if not causal else torch.tensor([False, True])
            plus = (q[i, :, :, col].float() * val) > 0                        # (2, 24): the score is +inf
            assert torch.equal(nan[i].t(), plus & sees.view(-1, 1)), "the sign of q's rope element decides between a NaN row and a dropped key"
            dropped = ~plus & sees.view(-1, 1)
            assert plus.any() and dropped.any()
            assert (lb[i].t()[dropped] < lc[i].t()[dropped]).all(), "a dropped key lowers the LSE"
            if causal:
                assert torch.equal(ob[i, 0], oc[i, 0]) and torch.equal(lb[i, :, 0], lc[i, :, 0])
    os_, ls = C.f_sparse_ref(q, bad, idx)
    oc, lc = C.f_sparse_ref(q, kv, idx)
    assert torch.equal(os_[:, 0], oc[:, 0]) and torch.isnan(ls[:, :, 1]).any() and not torch.isnan(ls[:, :, 0]).any() and torch.isfinite(oc).all()
    for i, row, _, _ in C.F_POS:
        assert (idx[i, 1] == row).sum() == 1 and not (idx[i, 0] == row).any() and ((idx[i] >= -1) & (idx[i] < C.F_LENS[i])).all()


# ---- G ------------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row_bytes", [C.ROW16, C.ROW8])
@pytest.mark.parametrize("base", [0x7F3A_0020_0000, 0x7F3A_8020_0000, 0x7F3A_FFE0_0000])
def test_g_pages_sit_on_the_boundaries(row_bytes, base):
    pb, n = row_bytes * C.G_P, C.G_POOL[row_bytes]
    assert n * pb > 2 ** 32 and (n - 256) * pb < 2 ** 32
    t = C.g_pages(row_bytes, base)
    pages = t.flatten().tolist()
    assert t.shape == (2, C.G_CAP // C.G_P) and len(set(pages)) == 14 and min(pages) == 0 and max(pages) == n - 1
    for off in (2 ** 31, 2 ** 32):
        at = [p for p in pages if p * pb <= off < (p + 1) * pb]
        assert len(at) == 1 and at[0] - 1 in pages and at[0] + 1 in pages
    # what the calls READ: sequence 0 its 7 pages, sequence 1 its first 3; the append writes rows 98, 99 of sequence 0 and 31, 32 of sequence 1
    used = t[0].tolist() + t[1, :3].tolist()
    assert all(p in used for p in (0, n - 1, 2 ** 31 // pb, 2 ** 32 // pb, 2 ** 32 // pb + 1))
    assert t[0, 6] == 2 ** 32 // pb and t[1, 1] == n - 1 and t[1, 2] == 2 ** 32 // pb + 1
    low = [(base + p * pb) & 0xFFFFFFFF for p in used]
    assert any(w & 0x80000000 for w in low) and all((base + p * pb) >> 32 for p in used)
    sign = int(t[0, 5])
    assert (base + sign * pb) & 0x80000000 and (base + sign * pb) >> 32


def test_g_longest_sequence_is_the_host_limit():
    for rb, cap in C.G_LONGEST.items():
        assert cap % 16 == 0 and cap * rb < 2 ** 31 <= (cap + 16) * rb


@pytest.mark.parametrize("fp8", [False, True])
def test_g_one_row_block_more_than_the_limit_is_refused_by_the_c_abi(fp8):
    """no launch: the parameter check of the workspace query refuses a capacity of 2^31 bytes or more with the message of the 16-bit / FP8 cache check"""
    from flash_attn_turing import capi

    dt = torch.float16
    rb = C.ROW8 if fp8 else C.ROW16
    cap = C.G_LONGEST[rb]
    kv = torch.zeros(1, 32, 1, C.RB, dtype=torch.uint8) if fp8 else torch.zeros(1, 32, 1, C.DK, dtype=dt)
    q, o, lse = torch.zeros(1, 1, 1, C.DK, dtype=dt), torch.zeros(1, 1, 1, C.DV, dtype=dt), torch.zeros(1, 1, 1)
    cs = torch.ones(1, dtype=torch.int32)
    idx = torch.full((1, 1, 32), -1, dtype=torch.int32)
    for make, query in ((lambda: capi.mla_params(q, kv, o, lse, cs), capi.mla_workspace_bytes),
                        (lambda: capi.mla_sparse_params(q, kv, o, lse, idx, cs), capi.mla_sparse_workspace_bytes)):
        p = make()
        p.seqlen_cache = cap
        assert query(p) >= 0
        p.seqlen_cache = cap + 16
        with pytest.raises(Exception, match=r"one sequence spans \d+ bytes \(limit 2\^31\)"):
            query(p)
