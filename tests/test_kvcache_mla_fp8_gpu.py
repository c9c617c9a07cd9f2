"""GPU: the FP8 latent cache (656-byte rows) of flash_mla_with_kvcache and flash_mla_sparse_with_kvcache.

The contract is a relation that must hold TO THE BIT: a call on an FP8 cache equals the same call on dequantize_mla_kv_cache(cache, q.dtype) - the codes
are dequantised where the LDS images are written, everything behind is the 16-bit kernel's code - so nearly every test here compares bits and has no
tolerance.  One case per dtype goes against fp64 math under the existing tolerances (_util.assert_close through `check`, _util.LSE_TOL): no new
number.  The quantising append is compared byte for byte with quantize_mla_kv_cache.  Bytes that must never reach a result hold 0xff: NaN codes, NaN
scales and NaN rope elements at once.  Shapes sit on the kernel's boundaries (64 packed rows a workgroup, 16 a wave, 32 keys a step, 16 keys a page
block), as in test_kvcache_mla_gpu.py."""
import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_prefill_gpu import visible
from test_kvcache_softcap_gpu import DT, _rand, _same
from test_kvcache_tree_gpu import check, exact, scores64

pytestmark = pytest.mark.gpu

NAN = float("nan")
DK, DV, RB = 576, 512, 656
CAP = 1008                              # 63 pages of 16 = 21 of 48
HS = [1, 16, 24, 128]
SQS = [1, 2, 5]
LENS = [0, 1, 31, 33, 100, 777]
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(DK)))


# ---- caches, pages, comparisons -------------------------------------------------------------------------------------------------------------------

def random_rows(lead, dt, gen):
    """uint8 (*lead, 656): uniformly random NaN-free codes (subnormal codes and both zeros included), tile scales log-uniform in [2^-12, 2^4] - every
    product code x scale is zero or normal in fp32: at least 2^-9 x 2^-12 - and N(0, 1) rope elements"""
    codes = torch.randint(0, 256, (*lead, 512), generator=gen, dtype=torch.int64)
    codes = torch.where((codes & 0x7F) == 0x7F, codes ^ 0x41, codes).to(torch.uint8)      # 0x7f -> 0x3e, 0xff -> 0xbe
    scale = torch.exp2(torch.rand(*lead, 4, generator=gen) * 16.0 - 12.0).float()
    rope = _rand((*lead, 64), dt, gen)
    return torch.cat([codes, scale.view(torch.uint8).view(*lead, 16), rope.view(torch.uint8).view(*lead, 128)], dim=-1)


def fill_past(cache, lens, value=0xFF):
    """rows at or past L_i of a contiguous cache (b, cap, 1, 656) <- value"""
    out = cache.clone()
    for i, L in enumerate(lens):
        out[i, L:] = value
    return out


def page_bytes(logical, P, seed, extra=2, fill=0xFF):
    """pool (num_blocks, P, 1, 656) + table of the logical cache under a random page permutation; spare pages hold `fill`"""
    b, cap = logical.shape[:2]
    cols = cap // P
    nb = b * cols + extra
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))
    table = perm[:b * cols].view(b, cols).to(torch.int32).to(logical.device)
    pool = torch.full((nb, P, 1, logical.shape[-1]), fill, dtype=logical.dtype, device=logical.device)
    pool[table.long()] = logical.reshape(b, cols, P, 1, -1)
    return pool, table


def logical_of(pool, table, cap):
    return pool[table.long()].reshape(table.shape[0], cap, 1, pool.shape[-1])


def same_nan(a, b):
    """bit for bit, NaN positions comparing as NaN"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and _same(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))


def same2(a, b):
    return same_nan(a[0], b[0]) and same_nan(a[1], b[1])


def dense(q, kv, cs, **kw):
    return F.flash_mla_with_kvcache(q, kv, cs, return_softmax_lse=True, **kw)


def sparse(q, kv, cs, idx, **kw):
    return F.flash_mla_sparse_with_kvcache(q, kv, cs, idx, return_softmax_lse=True, **kw)


def lists_for(lens, sq, topk, gen, kind, cap=CAP):
    """int32 (b, sq, topk).  identity: 0 .. L - 1 then -1; sorted / unsorted: a random subset of [0, L) per token, in order or shuffled, the other slots -1
    or out of range (>= L, INT_MIN, INT_MAX) and, unsorted, interleaved with the valid ones"""
    idx = torch.full((len(lens), sq, topk), -1, dtype=torch.int64)
    for i, L in enumerate(lens):
        for t in range(sq):
            if kind == "identity":
                n = min(L, topk)
                idx[i, t, :n] = torch.arange(n)
                continue
            n = min(L, int(torch.randint(1, topk + 1, (1,), generator=gen)))
            pos = torch.randperm(L, generator=gen)[:n]
            junk = torch.tensor([-1, L, cap - 1 if cap - 1 >= L else L, cap, -2 ** 31, 2 ** 31 - 1])[torch.randint(0, 6, (topk,), generator=gen)]
            if kind == "sorted":
                junk[:n] = pos.sort().values
            else:
                junk[torch.randperm(topk, generator=gen)[:n]] = pos
            idx[i, t] = junk
    return idx.to(torch.int32)


# ---- 1. contract 1: FP8 == 16-bit on the dequantised cache, bit for bit --------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("h", HS)
def test_dense_equals_the_16bit_call_on_the_dequantised_cache(gpu, dtname, h):
    """causal and not, splits 0 / 1 / 3, contiguous and pages of 16 / 48; rows at or past L_i and spare pages hold 0xff (contract 4), and the paged calls
    are compared with the CONTIGUOUS 16-bit call (contract 3)"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(81000 + h)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    for sq in SQS:
        q = _rand((len(LENS), sq, h, DK), dt, gen, 1 / 16).to(gpu)
        kv8 = fill_past(random_rows((len(LENS), CAP, 1), dt, gen), LENS).to(gpu)
        kv16 = F.dequantize_mla_kv_cache(kv8, dt)
        assert torch.isnan(kv16[1, 1:]).all().item() and not torch.isnan(kv16[5, :777]).any().item()
        pools = [page_bytes(kv8, P, 7 + P) for P in (16, 48)]
        for causal in (False, True):
            for ns in (0, 1, 3):
                tag = f"{dtname} h{h} sq{sq} causal={causal} splits={ns}"
                want = dense(q, kv16, cs, causal=causal, num_splits=ns)
                assert not torch.isnan(want[0]).any().item(), tag
                assert same2(dense(q, kv8, cs, causal=causal, num_splits=ns), want), tag
                assert same2(dense(q, kv8.view(torch.float8_e4m3fn), cs, causal=causal, num_splits=ns), want), tag + " (float8_e4m3fn)"
                for pool, table in pools:
                    assert same2(dense(q, pool, cs, causal=causal, num_splits=ns, block_table=table), want), f"{tag} P{pool.shape[1]}"


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("topk", [32, 64, 2048])
def test_sparse_equals_the_16bit_call_on_the_dequantised_cache(gpu, dtname, topk):
    """identity, random sorted and random unsorted lists with -1 padding and out-of-range entries, splits 0 / 1 / 2, contiguous and pages of 16 / 48;
    every cache row no valid slot names holds 0xff (contract 4); the identity list equals the dense call (contract 3)"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(82000 + topk)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    for h, sq in ((16, 2), (128, 1)) if topk == 2048 else ((1, 1), (24, 2), (128, 5)):
        q = _rand((len(LENS), sq, h, DK), dt, gen, 1 / 16).to(gpu)
        rows = random_rows((len(LENS), CAP, 1), dt, gen)
        for kind in ("identity", "sorted", "unsorted"):
            idx = lists_for(LENS, sq, topk, gen, kind)
            named = torch.zeros(len(LENS), CAP, dtype=torch.bool)
            for i, L in enumerate(LENS):
                ok = idx[i][(idx[i] >= 0) & (idx[i] < L)].long()
                named[i, ok] = True
            kv8 = torch.where(named[:, :, None, None], rows, torch.full_like(rows, 0xFF)).to(gpu)
            kv16 = F.dequantize_mla_kv_cache(kv8, dt)
            ig = idx.to(gpu)
            pools = [page_bytes(kv8, P, 11 + P) for P in (16, 48)]
            for ns in (0, 1, 2):
                tag = f"{dtname} topk{topk} h{h} sq{sq} {kind} splits={ns}"
                want = sparse(q, kv16, cs, ig, num_splits=ns)
                assert not torch.isnan(want[0]).any().item(), tag
                assert same2(sparse(q, kv8, cs, ig, num_splits=ns), want), tag
                for pool, table in pools:
                    assert same2(sparse(q, pool, cs, ig, num_splits=ns, block_table=table), want), f"{tag} P{pool.shape[1]}"
            if kind == "identity":
                n = torch.tensor([min(L, topk) for L in LENS], dtype=torch.int32, device=gpu)
                assert same2(sparse(q, kv8, cs, ig, num_splits=1), dense(q, kv8, n, num_splits=1)), f"{dtname} topk{topk} h{h} sq{sq}: identity list != dense call"


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_pages_of_64_and_run_to_run_determinism(gpu, dtname):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(83000)
    cap, lens, h, sq = 1024, [1, 63, 65, 1000], 24, 2
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    q = _rand((len(lens), sq, h, DK), dt, gen, 1 / 16).to(gpu)
    kv8 = fill_past(random_rows((len(lens), cap, 1), dt, gen), lens).to(gpu)
    kv16 = F.dequantize_mla_kv_cache(kv8, dt)
    pool, table = page_bytes(kv8, 64, 3)
    idx = lists_for(lens, sq, 64, gen, "unsorted", cap=cap).to(gpu)
    for ns in (0, 1, 3):
        want = dense(q, kv16, cs, causal=True, num_splits=ns)
        for _ in range(2):
            assert same2(dense(q, pool, cs, causal=True, num_splits=ns, block_table=table), want), f"dense splits={ns}"
            assert same2(dense(q, kv8, cs, causal=True, num_splits=ns), want), f"dense splits={ns}"
        swant = sparse(q, kv16, cs, idx, num_splits=min(ns, 2))
        for _ in range(2):
            assert same2(sparse(q, pool, cs, idx, num_splits=min(ns, 2), block_table=table), swant), f"sparse splits={ns}"
            assert same2(sparse(q, kv8, cs, idx, num_splits=min(ns, 2)), swant), f"sparse splits={ns}"


# ---- 2. fp64 ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_against_fp64_on_the_dequantised_cache(gpu, dtname):
    """the cache is quantize_mla_kv_cache of N(0, 1) rows; the expectation is fp64 math over dequantize_mla_kv_cache of it - the existing tolerances"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(84000)
    h, sq = 24, 2
    q = _rand((len(LENS), sq, h, DK), dt, gen)
    kv8 = F.quantize_mla_kv_cache(_rand((len(LENS), CAP, 1, DK), dt, gen))
    kvl = F.dequantize_mla_kv_cache(kv8, dt)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    s = scores64(q, kvl, SCALE)
    xo, xl, nvis = exact(s, kvl[..., :DV], visible(LENS, sq, CAP, True))
    for ns in (0, 3):
        out, lse = dense(q.to(gpu), kv8.to(gpu), cs, causal=True, num_splits=ns)
        check(out, lse, xo, xl, nvis, dtname, f"fp8 mla {dtname} splits={ns}")
    idx = lists_for(LENS, sq, 64, gen, "unsorted")
    ok = (idx.long() >= 0) & (idx.long() < torch.tensor(LENS).view(-1, 1, 1))
    pos = torch.where(ok, idx.long(), torch.zeros_like(idx, dtype=torch.int64))
    g = kvl[torch.arange(len(LENS)).view(-1, 1, 1), pos, 0].reshape(len(LENS) * sq, 64, 1, DK)
    so, sl, sn = exact(scores64(q.reshape(len(LENS) * sq, 1, h, DK), g, SCALE), g[..., :DV], ok.reshape(len(LENS) * sq, 1, 64))
    out, lse = sparse(q.to(gpu), kv8.to(gpu), cs, idx.to(gpu), num_splits=2)
    check(out, lse, so.reshape(len(LENS), sq, h, DV), sl.reshape(len(LENS), sq, h).permute(0, 2, 1), sn.reshape(len(LENS), sq), dtname, f"fp8 sparse mla {dtname}")


# ---- 3. a single visible key ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_single_key_returns_its_dequantised_columns_bit_for_bit(gpu, dtname):
    """one visible key whose row holds every NaN-free code (254 of them, both zeros and the subnormals included) twice, under four different tile scales:
    the softmax weight is exactly 1 and out is the first 512 dequantised columns, down the contiguous and paged kernels of both functions.  Changing only
    the rope bytes moves lse and never out.  The two NaN codes cannot sit in that row - one NaN column makes the key's score, hence the whole row, NaN -
    and get a row of their own: every output is NaN."""
    dt = DT[dtname]
    h, b = 24, 3
    codes = torch.arange(256, dtype=torch.int64)
    codes = torch.where((codes & 0x7F) == 0x7F, torch.zeros_like(codes), codes).to(torch.uint8)
    scales = torch.tensor([[2.0 ** -7, 0.3, 1.0, 3.7], [3.7, 2.0 ** -7, 0.3, 1.0], [0.01, 5.5, 2.0 ** -12, 16.0]], dtype=torch.float32)
    gen = torch.Generator().manual_seed(85000)
    rope = _rand((b, 64), dt, gen)
    row = torch.cat([codes.repeat(2).expand(b, 512), scales.view(torch.uint8).view(b, 16), rope.view(torch.uint8).view(b, 128)], dim=-1)
    kv8 = torch.full((b, 64, 1, RB), 0xFF, dtype=torch.uint8)
    kv8[:, 5, 0] = row
    kv8 = kv8.to(gpu)
    want = F.dequantize_mla_kv_cache(row.to(gpu), dt)[:, :DV]
    assert not torch.isnan(want).any().item() and len(torch.unique(row[:, :512])) == 254
    q = _rand((b, 2, h, DK), dt, gen, 1 / 64).to(gpu)
    idx = torch.full((b, 2, 32), -1, dtype=torch.int32, device=gpu)
    idx[:, :, 17] = 5
    pool, table = page_bytes(kv8, 16, 2)
    kv8b = kv8.clone()
    kv8b[:, 5, 0, 528:] = _rand((b, 64), dt, gen).view(torch.uint8).view(b, 128).to(gpu)       # other rope elements, nothing else
    poolb, tableb = page_bytes(kv8b, 16, 2)
    # (the one column that cannot come back bit for bit is code 0x80, -0: the accumulator starts at +0 and +0 + 1 x -0 is +0 in IEEE arithmetic, for the
    # 16-bit call on the dequantised row as well - asserted below - so the expectation is the row with +0 in that column)
    assert (want[:, 128] == 0).all().item() and torch.signbit(want[:, 128]).all().item()
    exp = (want + 0.0).unsqueeze(1).unsqueeze(1).expand(b, 2, h, DV).contiguous()
    assert _same(sparse(q, F.dequantize_mla_kv_cache(kv8, dt), 64, idx, num_splits=1)[0], exp)
    for ns in (0, 1, 2):
        for kw, kwb in ((dict(), dict()), (dict(block_table=table), dict(block_table=tableb))):
            c, cb_ = (pool, poolb) if kw else (kv8, kv8b)
            o1, l1 = sparse(q, c, 64, idx, num_splits=ns, **kw)
            o2, l2 = sparse(q, cb_, 64, idx, num_splits=ns, **kwb)
            assert _same(o1, exp) and _same(o2, exp), f"sparse splits={ns} paged={bool(kw)}"
            assert not torch.equal(l1, l2), "the rope bytes did not reach the LSE"
    # dense: the key must be row 0 (L = 1)
    kvd, kvdb = kv8[:, 5:].contiguous(), kv8b[:, 5:].contiguous()
    poold, tabled = page_bytes(kvd[:, :48], 16, 4)
    pooldb, _ = page_bytes(kvdb[:, :48], 16, 4)
    for ns in (0, 1, 3):
        for causal in (False, True):
            rows = slice(1, 2) if causal else slice(0, 2)       # causal with L = 1 and two query rows: row 0 sees nothing, row 1 sees key 0
            for c, cb_, kw in ((kvd, kvdb, dict()), (poold, pooldb, dict(block_table=tabled))):
                o1, l1 = dense(q, c, 1, causal=causal, num_splits=ns, **kw)
                o2, l2 = dense(q, cb_, 1, causal=causal, num_splits=ns, **kw)
                tag = f"dense splits={ns} causal={causal} paged={bool(kw)}"
                assert _same(o1[:, rows].contiguous(), exp[:, rows].contiguous()) and _same(o2[:, rows].contiguous(), exp[:, rows].contiguous()), tag
                assert not torch.equal(l1[:, :, rows], l2[:, :, rows]), tag
                if causal:
                    assert (o1[:, 0] == 0).all().item() and (l1[:, :, 0] == 0).all().item(), tag
    # the NaN codes
    kvn = kvd.clone()
    kvn[0, 0, 0, 7], kvn[1, 0, 0, 300], kvn[2, 0, 0, 511] = 0x7F, 0xFF, 0x7F
    o, l = dense(q, kvn, 1)
    assert torch.isnan(o).all().item() and torch.isnan(l).all().item()


# ---- 4. the quantising append -----------------------------------------------------------------------------------------------------------------------

def all_patterns(dt, gen):
    """(128, 576): all 65536 16-bit patterns, shuffled, over the 512 compressed columns of 128 rows; N(0, 1) rope elements"""
    pat = torch.arange(65536, dtype=torch.int32)[torch.randperm(65536, generator=gen)].to(torch.int16).view(128, 512).view(dt)
    return torch.cat([pat, _rand((128, 64), dt, gen)], dim=-1)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [0, 16, 48])
def test_append_writes_the_helpers_bytes(gpu, dtname, P):
    """all 65536 16-bit patterns (NaN, +-inf, subnormals among them) over 4 x 32 new rows; a sequence whose new rows hold an all-zero tile, an all-NaN
    tile, all-inf tiles, an all-zero row and ordinary values and run past the capacity (rows dropped); a sequence of ordinary values.  The lengths make
    the new rows cross pages.  The cache bytes equal quantize_mla_kv_cache(kv_new) - computed on the CPU - byte for byte; every other row, and every page
    no sequence owns, keeps its bytes; attention after the append equals the call without kv_new on the pre-quantised cache (the NaN patterns make
    sequences 0 .. 4 NaN in both; sequence 5 is finite)."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(86000 + P)
    b, s_new, cap, h = 6, 32, 96, 16
    pre = [0, 9, 40, 63, 80, 20]                         # 80 + 32 > 96: the last 16 new rows of sequence 4 are dropped
    kv_new = _rand((b, s_new, 1, DK), dt, gen, 3.0)
    kv_new[:4, :, 0] = all_patterns(dt, gen).view(4, 32, DK)
    kv_new[4, 1, 0, :128] = 0.0
    kv_new[4, 2, 0, 128:256] = NAN
    kv_new[4, 3, 0, 256:384] = float("inf")
    kv_new[4, 4, 0, 384:512] = -float("inf")
    kv_new[4, 5, 0, :512] = 0.0
    q8 = F.quantize_mla_kv_cache(kv_new)                 # CPU
    before = random_rows((b, cap, 1), dt, gen)
    want = before.clone()
    for i, L in enumerate(pre):
        n = min(s_new, cap - L)
        want[i, L:L + n] = q8[i, :n]
    cs = torch.tensor(pre, dtype=torch.int32, device=gpu)
    lens = torch.tensor([min(L + s_new, cap) for L in pre], dtype=torch.int32, device=gpu)
    q = _rand((b, 2, h, DK), dt, gen, 1 / 16).to(gpu)
    cache, ready, table = before.to(gpu), want.to(gpu), None
    if P:
        cache, table = page_bytes(cache, P, 5, fill=0xA5)
        ready, _ = page_bytes(ready, P, 5, fill=0xA5)
    for ns in (0, 2):
        c = cache.clone()
        got = dense(q, c, cs, kv_new=kv_new.to(gpu), causal=True, num_splits=ns, block_table=table)
        after = logical_of(c, table, cap) if P else c
        diff = (after.cpu() != want).any(-1).nonzero()
        assert diff.numel() == 0, f"{dtname} P{P} splits={ns}: cache rows differ from the helper at (sequence, row) {diff[:8, :2].tolist()}"
        assert torch.equal(c, ready)                    # (paged: the pages no sequence owns included)
        plain = dense(q, ready, lens, causal=True, num_splits=ns, block_table=table)
        assert same2(got, plain), f"{dtname} P{P} splits={ns}: attention after the append != the call on the pre-quantised cache"
        assert not torch.isnan(got[0][5]).any().item() and torch.isnan(got[0][:5]).all().item()


# ---- 5. NaN rules -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [0, 16])
def test_nan_code_and_nan_scale_in_visible_and_hidden_rows(gpu, dtname, P):
    """sequence 0: a NaN code in a visible row; 1: a NaN scale in a visible row; 2: both in a row at L (hidden); 3: clean.  Dense: sequences 0 and 1 are
    NaN, 2 and 3 are the clean call's bits.  Sparse: the same with visible = listed by the token, hidden = below L but listed by no token, and only the
    token that lists the row is NaN."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(87000)
    b, cap, h, sq, L = 4, 96, 24, 2, 70
    q = _rand((b, sq, h, DK), dt, gen, 1 / 16).to(gpu)
    clean = random_rows((b, cap, 1), dt, gen)
    bad = clean.clone()
    bad[0, 40, 0, 130] = 0x7F
    bad[1, 41, 0, 512 + 8:512 + 12] = torch.tensor([0, 0, 0xC0, 0x7F], dtype=torch.uint8)       # scale of tile 2 = NaN
    bad[2, L, 0, 5], bad[2, L, 0, 512:516] = 0xFF, torch.tensor([0, 0, 0xC0, 0xFF], dtype=torch.uint8)
    cs = torch.full((b,), L, dtype=torch.int32, device=gpu)

    def lay(c):
        return page_bytes(c.to(gpu), P, 9) if P else (c.to(gpu), None)
    (cg, table), (bg, _) = lay(clean), lay(bad)
    for ns in (0, 1, 3):
        for causal in (False, True):
            want = dense(q, cg, cs, causal=causal, num_splits=ns, block_table=table)
            o, l = dense(q, bg, cs, causal=causal, num_splits=ns, block_table=table)
            assert torch.isnan(o[:2]).all().item() and torch.isnan(l[:2]).all().item(), f"dense splits={ns} causal={causal}"
            assert _same(o[2:], want[0][2:]) and _same(l[2:], want[1][2:]), f"dense splits={ns} causal={causal}"
    idx = lists_for([L] * b, sq, 64, gen, "unsorted", cap=cap)
    idx[idx == 40], idx[idx == 41] = 39, 42             # no token lists rows 40 / 41 ...
    idx[0, 1, 3], idx[1, 0, 60] = 40, 41                # ... but token 1 of sequence 0 and token 0 of sequence 1
    bad2 = bad.clone()
    bad2[3, 40], bad2[3, 41] = bad[0, 40], bad[1, 41]   # sequence 3: the same rows below L, listed by no token
    (bg2, _), ig = lay(bad2), idx.to(gpu)
    for ns in (0, 1, 2):
        want = sparse(q, cg, cs, ig, num_splits=ns, block_table=table)
        o, l = sparse(q, bg2, cs, ig, num_splits=ns, block_table=table)
        assert torch.isnan(o[0, 1]).all().item() and torch.isnan(o[1, 0]).all().item() and torch.isnan(l[0, :, 1]).all().item() and torch.isnan(l[1, :, 0]).all().item()
        assert _same(o[0, 0], want[0][0, 0]) and _same(o[1, 1], want[0][1, 1]) and _same(o[2:], want[0][2:]) and _same(l[2:], want[1][2:]), f"sparse splits={ns}"


# ---- 6. views, capture, the C ABI ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("pitch", [672, 1312])
def test_strided_views_with_guard_bands(gpu, dtname, pitch):
    """the cache as a view with rows `pitch` bytes apart, starting 16 bytes into its buffer and with a guard row between sequences: both calls read it in
    place, the append writes the 656 bytes of its rows and nothing between them"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(88000 + pitch)
    b, cap, h, sq, L = 3, 64, 16, 2, 33
    rows = random_rows((b, cap, 1), dt, gen).to(gpu)
    buf = torch.full((b, cap + 1, 1, pitch), 0xEE, dtype=torch.uint8, device=gpu).flatten()
    buf = torch.cat([buf, torch.full((16,), 0xEE, dtype=torch.uint8, device=gpu)])
    view = buf[16:].view(b, cap + 1, 1, pitch)[:, :cap, :, :RB]
    assert view.stride() == ((cap + 1) * pitch, pitch, pitch, 1) and view.storage_offset() == 16
    view.copy_(rows)
    q = _rand((b, sq, h, DK), dt, gen, 1 / 16).to(gpu)
    kv_new = _rand((b, sq, 1, DK), dt, gen, 3.0)
    cs = torch.full((b,), L, dtype=torch.int32, device=gpu)
    idx = lists_for([L] * b, sq, 32, gen, "unsorted", cap=cap).to(gpu)
    assert same2(sparse(q, view, cs, idx), sparse(q, rows, cs, idx))
    assert same2(dense(q, view.view(torch.float8_e4m3fn), cs, causal=True), dense(q, rows, cs, causal=True))
    ref = rows.clone()
    want = dense(q, ref, cs, kv_new=kv_new.to(gpu), causal=True)
    assert same2(dense(q, view, cs, kv_new=kv_new.to(gpu), causal=True), want)
    assert torch.equal(view, ref) and torch.equal(ref[:, L:L + sq].cpu(), F.quantize_mla_kv_cache(kv_new))
    guard = torch.ones_like(buf, dtype=torch.bool)
    guard[16:].view(b, cap + 1, 1, pitch)[:, :cap, :, :RB] = False
    assert (buf[guard] == 0xEE).all().item(), "the append wrote between the rows of the view"


def test_captured_calls_replay_with_new_lengths_table_and_indices(gpu):
    dt, h, sq, b, P, cap = torch.bfloat16, 128, 1, 2, 64, 2048
    gen = torch.Generator().manual_seed(89000)
    kv8 = random_rows((b, cap, 1), dt, gen).to(gpu)
    q = _rand((b, sq, h, DK), dt, gen, 1 / 16).to(gpu)
    kv_new = _rand((b, sq, 1, DK), dt, gen, 3.0).to(gpu)
    pool, table = page_bytes(kv8, P, 5)
    cs = torch.tensor([100, 2000], dtype=torch.int32, device=gpu)
    idx = lists_for([100, 2000], sq, 64, gen, "unsorted", cap=cap).to(gpu)
    kw = dict(kv_new=kv_new, block_table=table, causal=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dense(q, pool, cs, **kw)
        sparse(q, pool, cs, idx, block_table=table)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        d_g = dense(q, pool, cs, **kw)
        s_g = sparse(q, pool, cs, idx, block_table=table)
    first = (d_g[0].clone(), s_g[0].clone())
    cs.copy_(torch.tensor([1500, 5], dtype=torch.int32))
    table.copy_(table.flip(0))                       # the sequences swap their pages
    idx.copy_(lists_for([1500, 5], sq, 64, gen, "sorted", cap=cap))
    g.replay()
    torch.cuda.synchronize()
    assert same2(d_g, dense(q, pool, cs, **kw)) and same2(s_g, sparse(q, pool, cs, idx, block_table=table))
    assert not _same(d_g[0], first[0]) and not _same(s_g[0], first[1])
    kv16 = F.dequantize_mla_kv_cache(logical_of(pool, table, cap), dt)
    assert same2(s_g, sparse(q, kv16, cs, idx)) and same2(d_g, dense(q, kv16, cs + sq, causal=True))


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_c_abi_with_a_caller_workspace_and_a_forced_split_is_the_python_call(gpu, dtname):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(90000)
    h, sq, b = 24, 2, len(LENS)
    q = _rand((b, sq, h, DK), dt, gen, 1 / 16).to(gpu)
    kv8 = random_rows((b, CAP, 1), dt, gen).to(gpu)
    kv_new = _rand((b, sq, 1, DK), dt, gen, 3.0).to(gpu)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    idx = lists_for(LENS, sq, 96, gen, "unsorted").to(gpu)
    pool, table = page_bytes(kv8, 48, 21)
    rows = b * h * sq
    for paged in (False, True):
        bt = table if paged else None
        base = pool if paged else kv8
        want = dense(q, base.clone(), cs, kv_new=kv_new, causal=True, num_splits=3, softmax_scale=0.07, block_table=bt)
        out = torch.full((b, sq, h, DV), NAN, dtype=dt, device=gpu)
        lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=gpu)
        kvg = base.clone()
        p = capi.mla_params(q, kvg, out, lse, cs, kv_new=kv_new, causal=True, num_splits=3, block_table=bt, softmax_scale=0.07)
        assert isinstance(p, capi.MlaParamsV2) and p.kv_format == capi.FA_MLA_KV_FP8_ROWS656
        nbytes = capi.mla_workspace_bytes(p)
        assert nbytes == 3 * rows * DV * 4 + (3 * rows * 4 + 15) // 16 * 16 and capi.mla_num_splits(p) == 1
        ws = torch.full((nbytes // 4 + 64,), NAN, device=gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
        assert capi.mla_num_splits(p) == 3
        capi.run_mla_fwd_kvcache(p)
        torch.cuda.synchronize()
        assert same2((out, lse), want) and torch.isnan(ws[-64:]).all().item(), f"dense paged={paged}"
        after = logical_of(kvg, table, CAP) if paged else kvg
        for i, L in enumerate(LENS):
            assert torch.equal(after[i, L:L + sq].cpu(), F.quantize_mla_kv_cache(kv_new[i].cpu()))
        swant = sparse(q, base, cs, idx, num_splits=2, softmax_scale=0.07, block_table=bt)
        out.fill_(NAN); lse.fill_(NAN)
        sp = capi.mla_sparse_params(q, base, out, lse, idx, cs, num_splits=2, block_table=bt, softmax_scale=0.07)
        assert isinstance(sp, capi.MlaSparseParamsV2)
        nbytes = capi.mla_sparse_workspace_bytes(sp)
        assert nbytes == 2 * rows * DV * 4 + (2 * rows * 4 + 15) // 16 * 16
        ws = torch.full((nbytes // 4 + 64,), NAN, device=gpu)
        sp.workspace, sp.workspace_bytes = ws.data_ptr(), nbytes
        assert capi.mla_sparse_num_splits(sp) == 2
        capi.run_mla_sparse_fwd_kvcache(sp)
        torch.cuda.synchronize()
        assert same2((out, lse), swant) and torch.isnan(ws[-64:]).all().item(), f"sparse paged={paged}"
