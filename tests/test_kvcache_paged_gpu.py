"""GPU: decode attention over a PAGED KV cache (flash_attn_with_kvcache(..., block_table=...), fa_kvcache_params.block_table).

Expectations: the C oracle and fp64 math on each sequence's logically gathered prefix (_util.check_kvcache_rows, the repo's tolerance
rules); and, because only the addressing differs, bit identity with the contiguous call on the gathered cache of the same capacity.
Pages are assigned by random permutations of the pool; everything the contract says is never read is poisoned with NaN."""
import statistics

import pytest
import torch

import _util as U
import flash_attn_turing as F

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
INT32_MAX = 2**31 - 1


def _rand(shape, dt, gen, dev):
    return torch.randn(*shape, device=dev, dtype=torch.float32, generator=gen).to(dt)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _page(logical_k, logical_v, P, lens, gen, extra=3, poison=True, bad_entry=-1, table_lens=None):
    """a pool + block table holding the logical caches (b, cap, hk, d): pages by a random permutation of a pool with `extra` unreferenced
    pages; with poison, pool rows past L_i, the unreferenced pages and the table entries of pages at or past ceil(T_i / P) are garbage
    (T = table_lens, default lens)"""
    b, cap, hk, d = logical_k.shape
    cols = cap // P
    nb = b * cols + extra
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(int(torch.randint(0, 2**30, (1,), generator=gen, device=logical_k.device).item())))
    table = perm[: b * cols].view(b, cols).to(torch.int32)
    fill = float("nan") if poison else 0.0
    kp = torch.full((nb, P, hk, d), fill, dtype=logical_k.dtype, device=logical_k.device)
    vp = torch.full_like(kp, fill)
    idx = table.long().to(logical_k.device)
    kp[idx] = logical_k.reshape(b, cols, P, hk, d)
    vp[idx] = logical_v.reshape(b, cols, P, hk, d)
    if poison:
        for i, L in enumerate(lens):
            for j in range(cols):
                lo = max(L - j * P, 0)
                if lo < P:
                    kp[table[i, j], lo:] = float("nan")
                    vp[table[i, j], lo:] = float("nan")
            need = -(-(lens if table_lens is None else table_lens)[i] // P)
            table[i, need:] = bad_entry if i % 2 == 0 else INT32_MAX
    return kp, vp, table.to(logical_k.device)


def _gather(kp, table, cap):
    """the logical cache (b, cap, hk, d) a table describes (entries clamped to the pool like the kernels do)"""
    nb, P = kp.shape[:2]
    cols = cap // P
    t = table[:, :cols].long().clamp(0, nb - 1)
    t = torch.where(table[:, :cols] < 0, torch.full_like(t, nb - 1), t)
    return kp[t].reshape(table.shape[0], cols * P, *kp.shape[2:])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_paged_against_reference(gpu, dtname, d, causal):
    """P 16 / 48 / 64 / 256; MHA, GQA, MQA; seqlen_q 1, 4, 16; lengths 0, 1, P-1, P, P+1, a split-chunk boundary (512 of 768 under three
    splits), the full capacity; the poisoned pool gives the oracle's answer and the contiguous call's bits"""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(101 + d + int(causal))
    cap = 768
    for P in (16, 48, 64, 256):
        lens = [0, 1, P - 1, P, P + 1, 512, cap]
        b = len(lens)
        cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
        for h, hk in ((8, 8), (32, 8), (16, 1)):
            k_log, v_log = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
            kp, vp, table = _page(k_log, v_log, P, lens, gen)
            for sq in (1, 4, 16):
                q = _rand((b, sq, h, d), dt, gen, gpu)
                ns = 3 if sq == 4 else 0
                out, lse = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True,
                                                     block_table=table)
                assert out.shape == q.shape and lse.shape == (b, h, sq)
                tag = f"{dtname} d{d} P{P} h{h}/{hk} sq{sq} causal={causal}"
                out_c, lse_c = F.flash_attn_with_kvcache(q, k_log, v_log, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True)
                assert _same(out, out_c) and torch.equal(lse, lse_c), tag
                U.check_kvcache_rows(out, lse, q, k_log, v_log, lens, causal, dtname, tag)


@pytest.mark.parametrize("num_splits", [1, 3, 0])
def test_bit_identical_to_contiguous(gpu, num_splits):
    dt, d, h, hk, cap = torch.float16, 128, 32, 8, 4608
    gen = torch.Generator(device=gpu).manual_seed(7 + num_splits)
    lens = [4608, 1, 2049, 0, 700]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k_log, v_log = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    for P, causal, sq in ((16, False, 1), (64, True, 3), (256, False, 2), (48 * 4, True, 1)):
        kp, vp, table = _page(k_log, v_log, P, lens, gen, poison=False)
        q = _rand((b, sq, h, d), dt, gen, gpu)
        out, lse = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=causal, num_splits=num_splits, return_softmax_lse=True,
                                             block_table=table)
        out_c, lse_c = F.flash_attn_with_kvcache(q, k_log, v_log, cache_seqlens=cs, causal=causal, num_splits=num_splits, return_softmax_lse=True)
        assert _same(out, out_c) and torch.equal(lse, lse_c), (P, causal, sq)
    U.check_kvcache_rows(out, lse, q, k_log, v_log, lens, True, "fp16", f"bits num_splits={num_splits}")


@pytest.mark.parametrize("causal", [False, True])
def test_append_through_table(gpu, causal):
    """new rows land at their page and row (a run crossing a page boundary among them) and are attended; every other pool byte - other
    pages, rows past L, unreferenced pages - is unchanged; rows past the capacity are dropped; cache_seqlens is not updated"""
    dt, d, h, hk, P, sn = torch.bfloat16, 64, 8, 2, 16, 5
    cap = 4 * P
    gen = torch.Generator(device=gpu).manual_seed(31 + int(causal))
    lens = [14, 0, 30, cap - 2, 40]                         # 14..18 crosses 16; cap-2: three of five rows do not fit
    b = len(lens)
    k_log, v_log = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    kp, vp, table = _page(k_log, v_log, P, lens, gen, extra=4, table_lens=[min(L + sn, cap) for L in lens])
    k_new, v_new = _rand((b, sn, hk, d), dt, gen, gpu), _rand((b, sn, hk, d), dt, gen, gpu)
    q = _rand((b, sn, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k0, v0 = kp.clone(), vp.clone()
    out, lse = F.flash_attn_with_kvcache(q, kp, vp, k=k_new, v=v_new, cache_seqlens=cs, causal=causal, return_softmax_lse=True, block_table=table)
    torch.cuda.synchronize()
    assert cs.tolist() == lens, "cache_seqlens must not be updated by the library"
    k_exp, v_exp = k0.clone(), v0.clone()
    for i, L in enumerate(lens):
        for t in range(sn):
            j = L + t
            if j >= cap:
                continue
            k_exp[table[i, j // P], j % P] = k_new[i, t]
            v_exp[table[i, j // P], j % P] = v_new[i, t]
    assert _same(kp, k_exp) and _same(vp, v_exp)
    eff = [min(L + sn, cap) for L in lens]
    U.check_kvcache_rows(out, lse, q, _gather(kp, table, cap), _gather(vp, table, cap), eff, causal, "bf16", f"paged append causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
def test_never_read_poison_is_bit_identical(gpu, causal):
    """NaN in rows past L, in unreferenced pages, and -1 / INT32_MAX in table entries past ceil(L / P): the same bits as clean inputs"""
    dt, d, h, hk, cap = torch.float16, 128, 16, 4, 1024
    gen = torch.Generator(device=gpu).manual_seed(41)
    lens = [1000, 0, 17, 511, 64, 1024]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k_log, v_log = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    for P, bad in ((16, -1), (64, INT32_MAX), (256, -1)):
        seed = int(torch.randint(0, 2**30, (1,)).item())
        kc, vc, tc = _page(k_log, v_log, P, lens, torch.Generator(device=gpu).manual_seed(seed), poison=False)
        kx, vx, tx = _page(k_log, v_log, P, lens, torch.Generator(device=gpu).manual_seed(seed), poison=True, bad_entry=bad)
        for sq, ns in ((1, 0), (4, 1), (2, 5)):
            q = _rand((b, sq, h, d), dt, gen, gpu)
            o1, l1 = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, block_table=tc)
            o2, l2 = F.flash_attn_with_kvcache(q, kx, vx, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, block_table=tx)
            assert _same(o1, o2) and torch.equal(l1, l2), (P, sq, ns)
            assert not torch.isnan(o2).any()
    U.check_kvcache_rows(o2, l2, q, k_log, v_log, lens, causal, "fp16", "poisoned")


def test_out_of_range_entries_are_clamped(gpu):
    """the pool sits inside one allocation between two NaN guard pages; needed entries of -1 and num_blocks read (and the append writes)
    page num_blocks - 1, never a guard page; the other sequences keep their bits"""
    dt, d, h, hk, P = torch.float16, 128, 8, 2, 64
    cap, nb = 4 * P, 12
    gen = torch.Generator(device=gpu).manual_seed(51)
    buf_k = torch.full((nb + 2, P, hk, d), float("nan"), dtype=dt, device=gpu)
    buf_v = torch.full_like(buf_k, float("nan"))
    kp, vp = buf_k[1:nb + 1], buf_v[1:nb + 1]
    kp.copy_(_rand(kp.shape, dt, gen, gpu))
    vp.copy_(_rand(vp.shape, dt, gen, gpu))
    table = torch.tensor([[3, 4, 5, 6], [0, -1, 2, 7], [8, 9, nb, 10], [1, 11, 2, 3]], dtype=torch.int32, device=gpu)
    fixed = torch.where((table < 0) | (table >= nb), torch.full_like(table, nb - 1), table)
    lens = [cap, 3 * P, cap, 2 * P + 5]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    q = _rand((b, 2, h, d), dt, gen, gpu)
    for ns in (1, 0):
        o, l = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, block_table=table)
        of, lf = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, block_table=fixed)
        assert _same(o, of) and torch.equal(l, lf), ns
        assert not torch.isnan(o).any()
    U.check_kvcache_rows(o, l, q, _gather(kp, fixed, cap), _gather(vp, fixed, cap), lens, False, "fp16", "clamped")
    # the append through the bad entries: rows P..P+2 of sequence 1 (entry -1) and 2P..2P+2 of sequence 2 (entry nb) go to page nb - 1
    guard_k, guard_v = buf_k[[0, nb + 1]].clone(), buf_v[[0, nb + 1]].clone()
    k_new, v_new = _rand((b, 3, hk, d), dt, gen, gpu), _rand((b, 3, hk, d), dt, gen, gpu)
    cs2 = torch.tensor([0, P, 2 * P + 8, 2 * P + 5], dtype=torch.int32, device=gpu)
    F.flash_attn_with_kvcache(q[:, :1], kp, vp, k=k_new, v=v_new, cache_seqlens=cs2, block_table=table)
    torch.cuda.synchronize()
    assert _same(buf_k[[0, nb + 1]], guard_k) and _same(buf_v[[0, nb + 1]], guard_v), "a guard page was written"
    assert _same(kp[nb - 1, 0:3], k_new[1]) and _same(vp[nb - 1, 0:3], v_new[1])       # sequence 1, entry -1
    assert _same(kp[nb - 1, 8:11], k_new[2]) and _same(vp[nb - 1, 8:11], v_new[2])     # sequence 2, entry num_blocks
    assert _same(kp[3, 0:3], k_new[0]) and _same(kp[2, 5:8], k_new[3])


def test_shared_prefix_pages(gpu):
    """two sequences reference the same physical prefix pages (read-only sharing); both match the reference"""
    dt, d, h, hk, P = torch.bfloat16, 128, 32, 8, 64
    gen = torch.Generator(device=gpu).manual_seed(61)
    nb = 10
    kp, vp = _rand((nb, P, hk, d), dt, gen, gpu), _rand((nb, P, hk, d), dt, gen, gpu)
    table = torch.tensor([[7, 2, 5, 0], [7, 2, 9, 3], [7, 1, 1, 1]], dtype=torch.int32, device=gpu)
    lens = [4 * P, 3 * P + 10, 2 * P]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    q = _rand((b, 4, h, d), dt, gen, gpu)
    out, lse = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=True, return_softmax_lse=True, block_table=table)
    U.check_kvcache_rows(out, lse, q, _gather(kp, table, 4 * P), _gather(vp, table, 4 * P), lens, True, "bf16", "shared pages")


def test_large_pool_strided_table_and_interleaved_kv(gpu):
    """k and v views of one (num_blocks, 2, P, h_k, d) pool above 2^32 bytes, the used pages past that mark, a table that is a strided view"""
    dt, d, h, hk, P = torch.float16, 128, 4, 1, 256
    page_bytes = 2 * P * hk * d * 2
    nb = (5 << 30) // page_bytes + 64                          # ~5 GiB of pool
    try:
        pool = torch.empty((nb, 2, P, hk, d), dtype=dt, device=gpu)
    except torch.OutOfMemoryError:
        pytest.fail("a 5 GiB pool does not fit on the device")
    kp, vp = pool[:, 0], pool[:, 1]
    gen = torch.Generator(device=gpu).manual_seed(71)
    first = (1 << 32) // page_bytes + 7                         # byte offset of the first used page > 2^32
    cols, b = 6, 3
    used = first + torch.randperm(nb - first, generator=torch.Generator().manual_seed(3))[: b * cols]
    tbuf = torch.full((b, 2 * cols + 5), -7, dtype=torch.int32)
    tbuf[:, 3:3 + cols] = used.view(b, cols).to(torch.int32)
    table = tbuf.to(gpu)[:, 3:3 + cols]
    assert table.stride(0) == 2 * cols + 5 and table.stride(1) == 1
    pool[used.to(gpu)] = _rand((b * cols, 2, P, hk, d), dt, gen, gpu)
    lens = [cols * P, 2 * P + 1, 5]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    q = _rand((b, 2, h, d), dt, gen, gpu)
    before = F._C.densify_copies()
    out, lse = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, return_softmax_lse=True, block_table=table)
    assert F._C.densify_copies() == before
    k_log, v_log = _gather(kp, table, cols * P), _gather(vp, table, cols * P)
    out_c, lse_c = F.flash_attn_with_kvcache(q, k_log, v_log, cache_seqlens=cs, return_softmax_lse=True)
    assert _same(out, out_c) and torch.equal(lse, lse_c)
    U.check_kvcache_rows(out, lse, q, k_log, v_log, lens, False, "fp16", "large pool")
    # the append lands past 2^32 bytes as well
    k_new, v_new = _rand((b, 2, hk, d), dt, gen, gpu), _rand((b, 2, hk, d), dt, gen, gpu)
    cs2 = torch.tensor([0, P - 1, 3 * P], dtype=torch.int32, device=gpu)
    F.flash_attn_with_kvcache(q, kp, vp, k=k_new, v=v_new, cache_seqlens=cs2, block_table=table)
    torch.cuda.synchronize()
    tl = table.cpu()
    for i, L in enumerate(cs2.tolist()):
        for t in range(2):
            j = L + t
            assert _same(kp[tl[i, j // P], j % P], k_new[i, t]) and _same(vp[tl[i, j // P], j % P], v_new[i, t]), (i, j)
    del pool, kp, vp
    torch.cuda.empty_cache()


def test_graph_replay_with_new_lengths_and_table(gpu):
    dt, d, h, hk, P, cap = torch.float16, 128, 32, 8, 64, 2048
    gen = torch.Generator(device=gpu).manual_seed(81)
    b = 2
    nb = b * cap // P + 8
    kp, vp = _rand((nb, P, hk, d), dt, gen, gpu), _rand((nb, P, hk, d), dt, gen, gpu)
    table = torch.randperm(nb, device=gpu)[: b * cap // P].view(b, cap // P).to(torch.int32)
    q = _rand((b, 1, h, d), dt, gen, gpu)
    cs = torch.tensor([100, 2000], dtype=torch.int32, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, return_softmax_lse=True, block_table=table)
    for step, lens in enumerate(([100, 2000], [1500, 1], [2048, 0], [64, 65])):
        cs.copy_(torch.tensor(lens, dtype=torch.int32))
        if step:
            table.copy_(torch.randperm(nb, device=gpu)[: table.numel()].view_as(table).to(torch.int32))
        g.replay()
        torch.cuda.synchronize()
        out_e, lse_e = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, return_softmax_lse=True, block_table=table)
        assert _same(out_g, out_e) and torch.equal(lse_g, lse_e), lens
        U.check_kvcache_rows(out_g, lse_g, q, _gather(kp, table, cap), _gather(vp, table, cap), lens, False, "fp16", f"graph {lens}")


def test_binding_checks(gpu):
    dt, d = torch.float16, 64
    q = torch.randn(2, 1, 4, d, device=gpu, dtype=dt)
    kp, vp = torch.randn(8, 16, 2, d, device=gpu, dtype=dt), torch.randn(8, 16, 2, d, device=gpu, dtype=dt)
    table = torch.arange(8, dtype=torch.int32, device=gpu).view(2, 4)
    cs = torch.tensor([10, 60], dtype=torch.int32, device=gpu)
    before = F._C.densify_copies()
    ref = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table)
    assert F._C.densify_copies() == before
    # positional calls of the binding are unchanged; block_table is the trailing argument
    o, _ = F._C.fwd_kvcache(q, kp, vp, None, None, cs, False, 0, table)
    assert torch.equal(o, ref)
    with pytest.raises(RuntimeError, match="int32"):
        F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table.long())
    with pytest.raises(RuntimeError, match="batch_size"):
        F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table[:1])
    with pytest.raises(RuntimeError, match="contiguous"):
        F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=torch.arange(8, dtype=torch.int32, device=gpu).view(4, 2).t())
    with pytest.raises(RuntimeError, match="same GPU device"):
        F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table.cpu())
    with pytest.raises(RuntimeError, match="page_block_size 8"):
        F.flash_attn_with_kvcache(q, kp[:, :8], vp[:, :8], cache_seqlens=cs, block_table=table)
    with pytest.raises(RuntimeError, match="same shape"):
        F.flash_attn_with_kvcache(q, kp, vp[:4], cache_seqlens=cs, block_table=table)
    with pytest.raises(TypeError):
        F.flash_attn_with_kvcache(q, kp, vp, None, None, cs, False, 0, False, table)      # keyword-only


def _median_ms(fn, rounds=7, iters=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ts)


def test_paged_decode_close_to_contiguous(gpu):
    """b8 h32 h_k8 d128, 32k keys, one query, P = 256 over a randomly permuted pool: at most 1.25x the contiguous call on the same data
    (profiles/kvcache_paged_bench.log has the measured ratios)"""
    dt, d, h, hk, L, P, b = torch.float16, 128, 32, 8, 32768, 256, 8
    gen = torch.Generator(device=gpu).manual_seed(91)
    nb = b * L // P
    kp, vp = _rand((nb, P, hk, d), dt, gen, gpu), _rand((nb, P, hk, d), dt, gen, gpu)
    table = torch.randperm(nb, generator=torch.Generator().manual_seed(5)).view(b, L // P).to(device=gpu, dtype=torch.int32)
    kc, vc = _gather(kp, table, L), _gather(vp, table, L)
    q = _rand((b, 1, h, d), dt, gen, gpu)
    cs = torch.full((b,), L, dtype=torch.int32, device=gpu)
    t_c, t_p = [], []
    for _ in range(3):
        t_c.append(_median_ms(lambda: F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs)))
        t_p.append(_median_ms(lambda: F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table)))
    tc, tp = statistics.median(t_c), statistics.median(t_p)
    assert tp <= 1.25 * tc, (tp, tc)
