"""GPU: the stand-alone append and gather of the MLA caches (flash_mla_cache_append, flash_mla_cache_gather, flash_mla_index_cache_append).

Everything is compared for byte equality: there is no tolerance anywhere in this feature (one reading of "equal", stated at _same_dequantised: where the
dequantised reference holds a NaN, any NaN will do - measured on an MI355X, code 0x7f gathers as 0xfe00 in fp16 and 0xffc0 in bf16, and
dequantize_mla_kv_cache gives 0x7f80 / 0xffff on the CPU and 0x7f80 / 0x7fc0 on the GPU).  Shapes are the smallest at which these row movers can go wrong
(tests/_mla_cache_io_cases.py): capacity 96 under pages of 16 and 48, b = 4, lengths around the page edges and the capacity, appends that cross pages, run
past the capacity and leave a workgroup partly filled, gathers that start inside a page and run past the length.  Expected caches come from the integer
placement model and the torch statement of the formats (quantize_mla_kv_cache, dequantize_mla_kv_cache, quantize_mla_index_keys), computed once per dtype."""
import functools
import statistics

import numpy as np
import pytest
import torch

import _mla_cache_io_cases as C
import _mla_cases as M
import flash_attn_turing as F

pytestmark = pytest.mark.gpu

DT = C.DT
B, CAP = C.B, C.CAP
SENT = 0xA5                                     # the byte every cache, pool and output buffer is filled with before a call
INT_MAX = 2 ** 31 - 1


def _i32(x, dev):
    return torch.tensor(list(x), dtype=torch.int32, device=dev)


def _raw(t):
    """the bytes of a tensor, on the host"""
    return t.detach().cpu().contiguous().view(torch.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_raw(a), _raw(b))


def _same_dequantised(got, want):
    """_same for rows that went through the dequantisation, except that where the reference holds a NaN any NaN will do.  A NaN code has no value beyond being
    NaN, and the reference does not pin its bits: dequantize_mla_kv_cache gives code 0x7f as 0xffff in bf16 on the CPU and as 0x7fc0 on the GPU, the kernels'
    conversion (dequant8, the one the attention kernels use) gives 0xffc0.  Every other element, and every byte outside the rows, is compared as it is."""
    g, w = got.detach().cpu(), want.detach().cpu()
    nan = torch.isnan(w)
    zero = torch.zeros((), dtype=w.dtype)
    return g.shape == w.shape and g.dtype == w.dtype and bool(torch.isnan(g[nan]).all()) and _same(torch.where(nan, zero, g), torch.where(nan, zero, w))


def _sentinel(shape, dtype):
    """a tensor of `dtype` whose every byte is SENT"""
    es = torch.empty(0, dtype=dtype).element_size()
    return torch.full((*shape[:-1], shape[-1] * es), SENT, dtype=torch.uint8).view(dtype)


@functools.lru_cache(maxsize=None)
def _new_latent(dtname):
    """(B, 20, 1, 576) new latent rows: N(0, 1) x 2^(row % 7 - 3), a few NaN / inf / zero tiles; and their FP8 rows, computed once"""
    g = torch.Generator().manual_seed(7100 + len(dtname))
    x = torch.randn(B, 20, 1, 576, generator=g) * (2.0 ** (torch.arange(20) % 7 - 3)).view(1, 20, 1, 1)
    x[0, 1, 0, 5], x[1, 2, 0, 130], x[2, 0, 0, 300], x[3, 4, 0, 511] = float("nan"), float("inf"), float("-inf"), float("nan")
    x[1, 0, 0, 128:256] = 0
    x[2, 3, 0, :512] = float("inf")
    x = x.to(DT[dtname])
    return x, F.quantize_mla_kv_cache(x)


def _packed(x, counts, extra=3):
    """rows [:n_i] of x[i] packed, followed by `extra` rows nobody owns"""
    rows = [x[i, :n] for i, n in enumerate(counts)] + [x[0, :extra] * 0 + 7]
    return torch.cat(rows)


def _expected_after_append(cache0, rows, lens, news):
    """the logical cache (B, CAP, ...) after new row s of sequence i (rows[i, s]) went where the placement model says"""
    want = cache0.clone()
    for i, s, pos in C.placed_rows(lens, news):
        want[i, pos] = rows[i, s]
    return want


# ---- latent append ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16, 48])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_dense_append_equals_the_append_of_the_decode_call(gpu, dtname, fp8, page):
    dt = DT[dtname]
    x, x8 = _new_latent(dtname)
    cache0 = _sentinel((B, CAP, 1, 656), torch.uint8) if fp8 else _sentinel((B, CAP, 1, 576), dt)
    q = torch.zeros(B, 1, 16, 576, dtype=dt, device=gpu)
    nb = B * (CAP // (page or CAP)) + 3
    table = None if page is None else C.make_table(B, CAP, page, nb, 11)
    for (lens, _), s_new in zip(C.APPEND_CASES, (20, 5, 1, 3)):
        start = cache0 if page is None else C.to_pool(cache0, table, page, nb, SENT if fp8 else cache0[0, 0, 0, 0])
        mine, theirs = start.clone().to(gpu), start.clone().to(gpu)
        bt = None if table is None else table.to(gpu)
        kv_new = x[:, :s_new].to(gpu)
        assert F.flash_mla_cache_append(mine, kv_new, _i32(lens, gpu), block_table=bt) is None
        F.flash_mla_with_kvcache(q, theirs, _i32(lens, gpu), kv_new=kv_new, block_table=bt)
        assert _same(mine, theirs), (lens, s_new)
        want = _expected_after_append(cache0, x8 if fp8 else x, lens, [s_new] * B)
        logical = mine.cpu() if page is None else C.from_pool(mine.cpu(), table, page)
        assert _same(logical, want), (lens, s_new)
        assert not _same(mine, start)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_packed_paged_split_and_strided_appends_agree(gpu, dtname, fp8):
    dt = DT[dtname]
    x, x8 = _new_latent(dtname)
    cache0 = _sentinel((B, CAP, 1, 656), torch.uint8) if fp8 else _sentinel((B, CAP, 1, 576), dt)
    fill = SENT if fp8 else cache0[0, 0, 0, 0]
    for lens, news in C.APPEND_CASES:
        want = _expected_after_append(cache0, x8 if fp8 else x, lens, news)
        dl, cu = _i32(lens, gpu), C.cu_of(news).to(gpu)
        rows = _packed(x, news).to(gpu)
        assert rows.shape[0] == sum(news) + 3
        # packed, contiguous
        c = cache0.clone().to(gpu)
        F.flash_mla_cache_append(c, rows, dl, cu_seqlens_new=cu)
        assert _same(c, want), (lens, news)
        # packed over pages of 16 and 48: the logical cache is the same and every other byte of the pool survives
        for page in C.PAGES:
            nb = B * (CAP // page) + 3
            table = C.make_table(B, CAP, page, nb, 13 + page)
            pool = C.to_pool(cache0, table, page, nb, fill).to(gpu)
            F.flash_mla_cache_append(pool, rows, dl, block_table=table.to(gpu), cu_seqlens_new=cu)
            assert _same(pool, C.to_pool(want, table, page, nb, fill)), (lens, news, page)
        # sequence i of the packed call equals the dense call on it alone
        for i, n in enumerate(news):
            c = cache0[i:i + 1].clone().to(gpu)
            F.flash_mla_cache_append(c, x[i:i + 1, :n].to(gpu), dl[i:i + 1])
            assert _same(c, want[i:i + 1]), (lens, news, i)
        # k_pe split (two views of one buffer), packed and dense
        c = cache0.clone().to(gpu)
        F.flash_mla_cache_append(c, rows[..., :512], dl, k_pe=rows[..., 512:], cu_seqlens_new=cu)
        assert _same(c, want), (lens, news)
        n = min(news)
        if n:
            a, b_ = cache0.clone().to(gpu), cache0.clone().to(gpu)
            xd = x[:, :n].to(gpu)
            F.flash_mla_cache_append(a, xd, dl)
            F.flash_mla_cache_append(b_, xd[..., :512].contiguous(), dl, k_pe=xd[..., 512:].contiguous())
            assert _same(a, b_) and not _same(a, cache0)
        # strided kv_new: rows of a wider buffer behind an offset, packed; every other row of a longer tensor, dense
        wide = torch.zeros(rows.shape[0] + 1, 1, 640, dtype=dt, device=gpu)
        wide[1:, :, 8:584] = rows
        c = cache0.clone().to(gpu)
        F.flash_mla_cache_append(c, wide[1:, :, 8:584], dl, cu_seqlens_new=cu)
        assert _same(c, want), (lens, news)
    lens = C.APPEND_CASES[0][0]
    skip = torch.zeros(B, 10, 1, 576, dtype=dt)
    skip[:, ::2] = x[:, :5]
    c = cache0.clone().to(gpu)
    F.flash_mla_cache_append(c, skip.to(gpu)[:, ::2], _i32(lens, gpu))
    assert _same(c, _expected_after_append(cache0, x8 if fp8 else x, lens, [5] * B))


@pytest.mark.parametrize("fp8", [False, True])
def test_wild_table_entries_write_only_inside_the_pool(gpu, fp8):
    dt, page, nb = torch.bfloat16, 16, 9
    x, x8 = _new_latent("bf16")
    width = 656 if fp8 else 576
    # the pool sits between two guard bands of one allocation
    buf = _sentinel((nb + 8, page, 1, width), torch.uint8 if fp8 else dt).to(gpu)
    pool = buf[4:4 + nb]
    lens, news = (15, 0, 47, 95), (3, 20, 5, 1)
    table = torch.tensor([[-1, INT_MAX, 2, 3, 4, 5], [-1, INT_MAX, -2 ** 31, 1, 2, 3], [0, 1, -1, INT_MAX, 4, 5], [0, 1, 2, 3, 4, INT_MAX]], dtype=torch.int32)
    F.flash_mla_cache_append(pool, _packed(x, news).to(gpu), _i32(lens, gpu), block_table=table.to(gpu), cu_seqlens_new=C.cu_of(news).to(gpu))
    got = buf.cpu()
    start = _sentinel((nb + 8, page, 1, width), torch.uint8 if fp8 else dt)
    assert _same(got[:4], start[:4]) and _same(got[4 + nb:], start[4 + nb:])
    # rows that do not collide in the clamped page are where the model says; every row that was not a target keeps the sentinel
    want, hit = start[4:4 + nb].clone(), {}
    for i, s, pos in C.placed_rows(lens, news):
        hit.setdefault(C.physical(table.tolist(), i, pos, page, nb), []).append((i, s))
    assert any(p == nb - 1 for p, _ in hit) and any(len(v) > 1 for v in hit.values())
    mask = torch.ones(nb, page, dtype=torch.bool)
    for (p, r), who in hit.items():
        mask[p, r] = False
        if len(who) == 1:
            want[p, r] = (x8 if fp8 else x)[who[0][0], who[0][1]]
        else:       # several rows landed on one slot of the clamped page: whatever their stores left there
            want[p, r] = got[4 + p, r]
    assert _same(got[4:4 + nb], want) and _same(got[4:4 + nb][mask], start[4:4 + nb][mask])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_fp8_append_equals_quantize_mla_kv_cache_on_every_finite_pattern(gpu, dtname):
    rows = M.a_rows(DT[dtname])                 # every finite pattern of the dtype in columns 0 .. 511
    n = rows.shape[0] // 2
    kv_new = rows[:2 * n].view(2, n, 1, 576)
    cache = _sentinel((2, CAP, 1, 656), torch.uint8).to(gpu)
    F.flash_mla_cache_append(cache, kv_new.to(gpu), 3)
    want = _sentinel((2, CAP, 1, 656), torch.uint8)
    want[:, 3:3 + n] = F.quantize_mla_kv_cache(kv_new)
    assert _same(cache, want)


# ---- gather --------------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _latent_cache(dtname, fp8):
    """the logical cache (B, CAP, 1, W) of the gather tests and what a gather of its rows must give (B, CAP, 576), computed once.  FP8: every NaN-free code under
    the scales of _mla_cases.c_scales(), rows of NaN codes, and quantised N(0, 1) rows"""
    dt = DT[dtname]
    g = torch.Generator().manual_seed(7200 + len(dtname))
    lat = (torch.randn(B * CAP, 576, generator=g) * 2.0 ** (torch.arange(B * CAP) % 9 - 4).view(-1, 1)).to(dt)
    if not fp8:
        lat[5, 7], lat[100, 530], lat[200, 0] = float("nan"), float("inf"), -0.0
        cache = lat.view(B, CAP, 1, 576)
        return cache, cache.view(B, CAP, 576).clone()
    rows = F.quantize_mla_kv_cache(lat)
    c = M.c_rows(dt)
    rows[1:2 * c.shape[0]:2] = c                                     # spread over the sequences and pages
    rows[0, :512:3], rows[190, 1:512:2] = 0x7F, 0xFF                  # NaN codes of both signs
    cache = rows.view(B, CAP, 1, 656)
    return cache, F.dequantize_mla_kv_cache(cache, dt).view(B, CAP, 576)


def _spoil(cache, lens):
    """rows at or past L_i hold 0xff bytes: NaN codes, NaN scales, NaN elements"""
    c = cache.clone()
    for i, L in enumerate(lens):
        c[i, min(max(L, 0), CAP):] = torch.full((), -1, dtype=torch.int8).view(torch.uint8) if c.dtype == torch.uint8 else torch.full((), -1, dtype=torch.int16).view(c.dtype)
    return c


def _expected_gather(ref, lens, starts, counts, out0, packed):
    want = out0.clone()
    cu = [0] + list(np.cumsum(counts))
    for i, r, pos in C.gathered_rows(lens, starts, counts):
        row = ref[i, pos] if pos is not None else torch.zeros(576, dtype=ref.dtype)
        if packed:
            want[cu[i] + r] = row
        else:
            want[i, r] = row
    return want


@pytest.mark.parametrize("page", [None, 16, 48])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_gather_equals_the_rows_the_attention_kernels_compute_with(gpu, dtname, fp8, page):
    dt = DT[dtname]
    cache, ref = _latent_cache(dtname, fp8)
    ff = torch.full((), -1, dtype=torch.int8).view(torch.uint8) if fp8 else torch.full((), -1, dtype=torch.int16).view(dt)
    same = _same_dequantised if fp8 else _same          # (a 16-bit row is copied: its NaNs keep their bits)
    assert torch.isnan(ref).any()
    for lens, starts, counts in C.GATHER_CASES:
        spoiled = _spoil(cache, lens)
        total = sum(counts)
        if page is None:
            kv, bt = spoiled.to(gpu), None
        else:
            nb = B * (CAP // page) + 3
            table = C.make_table(B, CAP, page, nb, 17 + page)
            pool = C.to_pool(spoiled, table, page, nb, ff)        # unreferenced pages hold 0xff
            # pages and table entries that no requested row needs: 0xff as well (the entry reads -1)
            need = {(i, pos // page) for i, r, pos in C.gathered_rows(lens, starts, counts) if pos is not None}
            for i in range(B):
                for col in range(CAP // page):
                    if (i, col) not in need:
                        pool[int(table[i, col])] = ff
                        table[i, col] = -1
            kv, bt = pool.to(gpu), table.to(gpu)
        # packed into a slice of a wider workspace, three rows past cu[b]: the gaps and the surplus rows keep the sentinel
        wide = _sentinel((total + 3, 640), dt).to(gpu)
        out = wide[:, 32:608]
        got = F.flash_mla_cache_gather(kv, _i32(lens, gpu), out, block_table=bt, cu_seqlens_out=C.cu_of(counts).to(gpu), seq_starts=_i32(starts, gpu))
        assert got is out
        want = _sentinel((total + 3, 640), dt)
        want[:, 32:608] = _expected_gather(ref, lens, starts, counts, want[:, 32:608], True)
        assert same(wide, want), (lens, starts, counts)
    # dense, 33 rows a sequence, with and without starts and lengths
    lens, starts, _ = C.GATHER_CASES[0]
    kv, bt = cache.to(gpu), None
    if page is not None:
        nb = B * (CAP // page) + 3
        table = C.make_table(B, CAP, page, nb, 19 + page)
        kv, bt = C.to_pool(cache, table, page, nb, ff).to(gpu), table.to(gpu)
    for L, S in ((lens, starts), (None, starts), (lens, None), (None, None)):
        out = _sentinel((B, 33, 576), dt).to(gpu)
        F.flash_mla_cache_gather(kv, None if L is None else _i32(L, gpu), out, block_table=bt, seq_starts=None if S is None else _i32(S, gpu))
        assert same(out, _expected_gather(ref, L, S, [33] * B, _sentinel((B, 33, 576), dt), False)), (L, S)
    out = _sentinel((B, CAP, 576), dt).to(gpu)
    F.flash_mla_cache_gather(kv, 48, out, block_table=bt)           # an int length
    assert same(out, _expected_gather(ref, [48] * B, None, [CAP] * B, _sentinel((B, CAP, 576), dt), False))


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_fp8_paged_decode_equals_the_16_bit_call_on_gathered_rows(gpu, dtname):
    dt, page = DT[dtname], 16
    g = torch.Generator().manual_seed(7300)
    lat = torch.randn(B, CAP, 1, 576, generator=g).to(dt)
    nb = B * (CAP // page) + 2
    table = C.make_table(B, CAP, page, nb, 23)
    pool = C.to_pool(F.quantize_mla_kv_cache(lat), table, page, nb, 0xFF).to(gpu)
    q = (torch.randn(B, 2, 16, 576, generator=g) / 8).to(dt).to(gpu)
    lens = _i32((96, 47, 17, 1), gpu)
    rows = F.flash_mla_cache_gather(pool, lens, torch.empty(B, CAP, 576, dtype=dt, device=gpu), block_table=table.to(gpu))
    for causal in (False, True):
        o8, l8 = F.flash_mla_with_kvcache(q, pool, lens, block_table=table.to(gpu), causal=causal, num_splits=2, return_softmax_lse=True)
        o16, l16 = F.flash_mla_with_kvcache(q, rows.view(B, CAP, 1, 576), lens, causal=causal, num_splits=2, return_softmax_lse=True)
        assert _same(o8, o16) and _same(l8, l16) and o8.float().abs().sum() > 0


# ---- index-key append ------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _quantised_keys(dtname, fmt):
    rows = C.index_key_rows(dtname)
    return (rows,) + tuple(F.quantize_mla_index_keys(rows, fmt))


@pytest.mark.parametrize("fmt", ["fp32", "ue8m0"])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_index_append_quantises_every_pattern_like_quantize_mla_index_keys(gpu, dtname, fmt):
    """all 65536 patterns (512 rows), the amax sweep and the rows of only NaN / inf, packed over four sequences of a cache of 192 rows"""
    rows, codes, scale = _quantised_keys(dtname, fmt)
    n, cap = rows.shape[0], 192
    counts = [n // 4] * 3 + [n - 3 * (n // 4)]
    lens = (0, 3, 16, 7)
    assert max(l + c for l, c in zip(lens, counts)) <= cap
    cache = _sentinel((B, cap, 128), torch.uint8).to(gpu)
    sbuf = _sentinel((B, 2 * cap), torch.float32).to(gpu)
    F.flash_mla_index_cache_append(cache, rows.to(gpu), _i32(lens, gpu), k_scale=sbuf[:, ::2], cu_seqlens_new=C.cu_of(counts).to(gpu), scale_format=fmt)
    want_c, want_s = _sentinel((B, cap, 128), torch.uint8), _sentinel((B, 2 * cap), torch.float32)
    cu = C.cu_of(counts).tolist()
    for i in range(B):
        want_c[i, lens[i]:lens[i] + counts[i]] = codes[cu[i]:cu[i + 1]]
        want_s[i, 2 * lens[i]:2 * (lens[i] + counts[i]):2] = scale[cu[i]:cu[i + 1]]
    assert _same(sbuf, want_s)
    bad = (cache.cpu() != want_c).nonzero()
    assert bad.numel() == 0, (bad[:4], cache.cpu()[tuple(bad[0])], want_c[tuple(bad[0])])


@pytest.mark.parametrize("kind", ["copy", "fp32", "ue8m0"])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_index_append_packed_dense_and_paged_agree(gpu, dtname, kind):
    dt, fp8 = DT[dtname], kind != "copy"
    g = torch.Generator().manual_seed(7400)
    x = (torch.randn(B, 20, 128, generator=g) * 2.0 ** (torch.arange(20) % 11 - 5).view(1, 20, 1)).to(dt)
    x[1, 2, 9], x[2, 0, 100] = float("nan"), float("inf")
    fmt = dict(scale_format=kind) if fp8 else {}
    codes, scale = F.quantize_mla_index_keys(x, kind) if fp8 else (x, None)
    cache0 = _sentinel((B, CAP, 128), torch.uint8 if fp8 else dt)
    scale0 = _sentinel((B, CAP), torch.float32)
    for lens, news in C.APPEND_CASES:
        want_c = _expected_after_append(cache0, codes, lens, news)
        want_s = _expected_after_append(scale0, scale, lens, news) if fp8 else None
        dl, cu = _i32(lens, gpu), C.cu_of(news).to(gpu)
        rows = _packed(x, news).to(gpu)
        c, s = cache0.clone().to(gpu), scale0.clone().to(gpu) if fp8 else None
        assert F.flash_mla_index_cache_append(c, rows, dl, k_scale=s, cu_seqlens_new=cu, **fmt) is None
        assert _same(c, want_c) and (not fp8 or _same(s, want_s)), (lens, news)
        for page in C.PAGES:
            nb = B * (CAP // page) + 3
            table = C.make_table(B, CAP, page, nb, 29 + page)
            pc = C.to_pool(cache0, table, page, nb, cache0[0, 0, 0]).to(gpu)
            ps = C.to_pool(scale0, table, page, nb, scale0[0, 0]).to(gpu) if fp8 else None
            F.flash_mla_index_cache_append(pc, rows, dl, k_scale=ps, block_table=table.to(gpu), cu_seqlens_new=cu, **fmt)
            assert _same(pc, C.to_pool(want_c, table, page, nb, cache0[0, 0, 0])), (lens, news, page)
            assert not fp8 or _same(ps, C.to_pool(want_s, table, page, nb, scale0[0, 0])), (lens, news, page)
        for i, n in enumerate(news):
            c, s = cache0[i:i + 1].clone().to(gpu), scale0[i:i + 1].clone().to(gpu) if fp8 else None
            F.flash_mla_index_cache_append(c, x[i:i + 1, :n].to(gpu), dl[i:i + 1], k_scale=s, **fmt)
            assert _same(c, want_c[i:i + 1]) and (not fp8 or _same(s, want_s[i:i + 1])), (lens, news, i)


@pytest.mark.parametrize("fmt", ["fp32", "ue8m0"])
def test_indexer_reads_what_the_append_wrote(gpu, fmt):
    dt, page = torch.bfloat16, 16
    g = torch.Generator().manual_seed(7500)
    x = torch.randn(B, 20, 128, generator=g).to(dt)
    codes, scale = F.quantize_mla_index_keys(x, fmt)
    lens, news = (0, 16, 47, 90), (20, 5, 3, 20)
    nb = B * (CAP // page)
    table = C.make_table(B, CAP, page, nb, 31)
    # the cache placed by torch, and the cache the call writes
    tc, ts = torch.zeros(B, CAP, 128, dtype=torch.uint8), torch.zeros(B, CAP)
    for i, s, pos in C.placed_rows(lens, news):
        tc[i, pos], ts[i, pos] = codes[i, s], scale[i, s]
    pc, ps = torch.zeros(nb, page, 128, dtype=torch.uint8, device=gpu), torch.zeros(nb, page, device=gpu)
    F.flash_mla_index_cache_append(pc, _packed(x, news).to(gpu), _i32(lens, gpu), k_scale=ps, block_table=table.to(gpu), cu_seqlens_new=C.cu_of(news).to(gpu),
                                   scale_format=fmt)
    after = [min(l + n, CAP) for l, n in zip(lens, news)]
    q = torch.randn(B, 1, 16, 128, generator=g).to(dt).to(gpu)
    w = torch.randn(B, 1, 16, generator=g).to(gpu)
    a = F.flash_mla_indexer_logits(q, w, pc.view(torch.float8_e4m3fn), _i32(after, gpu), k_scale=ps, block_table=table.to(gpu), causal=False)
    b_ = F.flash_mla_indexer_logits(q, w, tc.to(gpu), _i32(after, gpu), k_scale=ts.to(gpu), causal=False)
    for i, L in enumerate(after):
        assert _same(a[i, :, :L], b_[i, :, :L]) and a[i, :, lens[i]:L].abs().sum() > 0


# ---- graph capture -----------------------------------------------------------------------------------------------------------------------------------

def _captured(calls):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls()
    return graph


def test_captured_calls_replay_with_the_lengths_then_in_memory(gpu):
    dt = torch.bfloat16
    x, x8 = _new_latent("bf16")
    cache0 = _sentinel((B, CAP, 1, 656), torch.uint8)
    lens0, lens1, news = (0, 0, 0, 0), C.APPEND_CASES[0][0], C.APPEND_CASES[0][1]
    dl, cu = _i32(lens0, gpu), C.cu_of(news).to(gpu)
    rows = _packed(x, news).to(gpu)
    # latent append
    c = cache0.clone().to(gpu)
    graph = _captured(lambda: F.flash_mla_cache_append(c, rows, dl, cu_seqlens_new=cu))
    c.copy_(cache0)
    dl.copy_(_i32(lens1, gpu))
    graph.replay()
    torch.cuda.synchronize()
    want = _expected_after_append(cache0, x8, lens1, news)
    assert _same(c, want)
    # gather of what was written
    out = _sentinel((B, 33, 576), dt).to(gpu)
    after = _i32([0] * B, gpu)
    graph = _captured(lambda: F.flash_mla_cache_gather(c, after, out, seq_starts=dl))
    after.copy_(_i32([min(max(l, 0) + n, CAP) for l, n in zip(lens1, news)], gpu))
    graph.replay()
    torch.cuda.synchronize()
    ref = F.dequantize_mla_kv_cache(want, dt).view(B, CAP, 576)
    assert _same_dequantised(out, _expected_gather(ref, after.tolist(), lens1, [33] * B, _sentinel((B, 33, 576), dt), False))
    # index append
    xi = x[:, :, 0, :128].contiguous()
    codes, scale = F.quantize_mla_index_keys(xi, "ue8m0")
    ic0, is0 = _sentinel((B, CAP, 128), torch.uint8), _sentinel((B, CAP), torch.float32)
    ic, isc = ic0.clone().to(gpu), is0.clone().to(gpu)
    dl.copy_(_i32(lens0, gpu))
    irows = _packed(xi, news).to(gpu)
    graph = _captured(lambda: F.flash_mla_index_cache_append(ic, irows, dl, k_scale=isc, cu_seqlens_new=cu, scale_format="ue8m0"))
    ic.copy_(ic0)
    isc.copy_(is0)
    dl.copy_(_i32(lens1, gpu))
    graph.replay()
    torch.cuda.synchronize()
    assert _same(ic, _expected_after_append(ic0, codes, lens1, news)) and _same(isc, _expected_after_append(is0, scale, lens1, news))


# ---- one speed relation ------------------------------------------------------------------------------------------------------------------------------

def torch_gather(pool, table, n, dtype):
    """the gather in torch ops: the pages of every sequence through the table, then dequantize_mla_kv_cache"""
    rows = pool[table.long()].flatten(1, 2)[:, :n]             # (b, n, 1, 656)
    return F.dequantize_mla_kv_cache(rows, dtype).view(-1, 576)


def test_fp8_paged_gather_is_faster_than_the_torch_formulation(gpu):
    """b 8 x 4096 rows, pages of 64, bf16: median of 5 interleaved rounds, bound 1.0 with no margin - a call that does not beat what callers could already do
    has no reason to exist"""
    b, n, page, dt = 8, 4096, 64, torch.bfloat16
    g = torch.Generator().manual_seed(7600)
    nb = b * n // page
    pool = F.quantize_mla_kv_cache(torch.randn(nb, page, 1, 576, generator=g).to(dt)).to(gpu)
    table = torch.randperm(nb, generator=g).view(b, n // page).to(torch.int32).to(gpu)
    lens, cu = _i32([n] * b, gpu), _i32(range(0, b * n + 1, n), gpu)
    out = torch.empty(b * n, 576, dtype=dt, device=gpu)
    ours = lambda: F.flash_mla_cache_gather(pool, lens, out, block_table=table, cu_seqlens_out=cu)
    theirs = lambda: torch_gather(pool, table, n, dt)
    assert torch.equal(ours().view(torch.int16), theirs().view(torch.int16))

    def timed(fn, reps=5):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / reps

    for fn in (ours, theirs):
        timed(fn, 2)
    t_ours, t_theirs = [], []
    for _ in range(5):
        t_ours.append(timed(ours))
        t_theirs.append(timed(theirs))
    ratio = statistics.median(t_ours) / statistics.median(t_theirs)
    print(f"flash_mla_cache_gather {statistics.median(t_ours) * 1e3:.1f} us, torch formulation {statistics.median(t_theirs) * 1e3:.1f} us, ratio {ratio:.3f}")
    assert ratio <= 1.0, ratio
