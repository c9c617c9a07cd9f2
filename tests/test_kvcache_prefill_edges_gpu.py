"""GPU: the 64-row prefill kernels (flash_attn_with_kvcache(..., prefill=True), fa_fwd_kvcache_prefill.hip) where test_kvcache_prefill_gpu.py does
not reach: strided q / k / v / caches / pools / tables, offsets past 2^31 elements and 2^32 bytes, softmax_scale (alone and folded with
k_descale), the plain ragged grid, more than 64 and more than 512 sequences in the slot lookup, softmax extremes across steps, LDS stages and
splits, pages of 32 / 64 / 256 rows, and packing ratios of 64 and above.

Expectations are fp64 math over the visible keys (scores64 / exact of the tree suite with the visibility rule of the prefill suite, or the C
oracle through _util.check_kvcache_rows where the 16-row test it mirrors uses that); tolerances are _util.TOL and _util.LSE_TOL, no new number.
Rows that see no key are asserted exactly.  Everything the docstring of flash_attn_with_kvcache promises to the bit - strides do not change
the summation order, paged == contiguous, a sequence of a ragged call == the dense call on it alone, None == the default scale passed
explicitly - is asserted to the bit.  Shapes are small: the point is tile, step, stage and page boundaries."""
import math

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_fp8_gpu import _descale, deq, quantise
from test_kvcache_fp8_gpu import _page as _page8
from test_kvcache_prefill_gpu import chunk_case, visible
from test_kvcache_softcap_gpu import DT, _rand, _same
from test_kvcache_tree_gpu import check, exact, scores64
from test_kvcache_window_gpu import _page

pytestmark = pytest.mark.gpu

NAN = float("nan")
F8 = torch.float8_e4m3fn
POISON8 = (0x7F, 0x7E, 0xFE, 0xFF)      # e4m3fn has no inf: NaN, 448, -448, NaN with the sign set
CAP = 1008                              # 21 pages of 48 rows, as in the prefill suite
SPLITS = [0, 1, 3]
ONE_OF_EACH = [("fp16", 128), ("bf16", 64)]


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _eq(a, b):
    """the same bits, wherever the two tensors live and however they are laid out"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a).cpu(), _bits(b).cpu())


def _call(q, kc, vc, **kw):
    return F.flash_attn_with_kvcache(q, kc, vc, return_softmax_lse=True, prefill=True, **kw)


def _quantised_case(k, v, k_new, v_new, prefixes, gen, gpu):
    """the 8-bit version of a chunk_case: descales, the quantised caches before and after the append (the append's contract, on the CPU)"""
    b, hk, sq = k.shape[0], k.shape[2], k_new.shape[1]
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = quantise(k, kds), quantise(v, vds)
    kl8, vl8 = k8.clone(), v8.clone()
    kn8, vn8 = quantise(k_new, kds), quantise(v_new, vds)
    for i, pre in enumerate(prefixes):
        kl8[i, pre:pre + sq], vl8[i, pre:pre + sq] = kn8[i], vn8[i]
    return kds, vds, k8, v8, kl8, vl8


# ---- A. layouts --------------------------------------------------------------------------------------------------------------------------------

def _poison_buf(shape, dt, dev):
    """a buffer holding the poison cycle along its last dim (_util.poison_; an 8-bit buffer cycles through POISON8)"""
    if dt == F8:
        codes = torch.tensor(POISON8, dtype=torch.uint8, device=dev)
        return codes[torch.arange(shape[-1], device=dev) % len(POISON8)].expand(*shape).contiguous().view(F8)
    return U.poison_(torch.empty(shape, dtype=dt, device=dev))


def _embed(x, pad, off):
    """x's values as a view of a poison buffer with `pad` extra elements per dim, the view starting at `off`: (view, buffer, index of the view)"""
    buf = _poison_buf([s + p for s, p in zip(x.shape, pad)], x.dtype, x.device)
    sl = tuple(slice(o, o + s) for o, s in zip(off, x.shape))
    _bits(buf)[sl] = _bits(x)
    return buf[sl], buf, sl


def _gap_bits(buf, sl):
    inside = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    inside[sl] = True
    return _bits(buf)[~inside]


def _cache_layouts(kg, vg, P, seed, fp8):
    """the logical caches kg / vg (b, cap, hk, d) on the device in three kinds of storage: (name, k, v, keywords, logical, guards) - `logical()`
    reads the logical caches back, `guards` are (buffer, index of the view) pairs whose gaps hold poison.  An 8-bit cache keeps every stride a
    multiple of 16 elements."""
    b, cap, hk, d = kg.shape
    e = 16 if fp8 else 8
    out = []
    # K and V views with different row and head strides
    kv_, kb, ksl = _embed(kg, (0, 3, 1, e), (0, 1, 1, 0))
    vv_, vb, vsl = _embed(vg, (0, 1, 2, 2 * e), (0, 1, 1, e))
    assert kv_.stride(1) != vv_.stride(1) and kv_.stride(2) != vv_.stride(2), "K and V must differ in row stride and in head stride"
    out.append(("padded views", kv_, vv_, dict(), lambda: (kv_, vv_), [(kb, ksl), (vb, vsl)]))
    # K and V interleaved in one allocation
    kv = torch.stack((_bits(kg), _bits(vg)), dim=2).view(kg.dtype)
    ki, vi = kv[:, :, 0], kv[:, :, 1]
    out.append(("interleaved", ki, vi, dict(), lambda: (ki, vi), []))
    # paged: a page stride above P x the row stride, the two pools padded differently, the table a column slice of a wider tensor
    kp, vp, table = (_page8(kg, vg, P, seed) if fp8 else _page(kg, vg, P, seed))[:3]
    cols = table.shape[1]
    tbuf = torch.full((b, cols + 5), -7, dtype=torch.int32, device=kg.device)
    tbuf[:, 3:3 + cols] = table
    tv = tbuf[:, 3:3 + cols]
    assert tv.stride(0) == cols + 5 and tv.stride(1) == 1
    kpv, kpb, kpsl = _embed(kp, (0, 2, 1, e), (0, 1, 1, 0))
    vpv, vpb, vpsl = _embed(vp, (0, 1, 2, 2 * e), (0, 0, 2, e))
    assert kpv.stride(0) > P * kpv.stride(1) and kpv.stride(0) != vpv.stride(0) and kpv.stride(1) != vpv.stride(1) and kpv.stride(2) != vpv.stride(2)

    def gathered():
        return tuple(_bits(x)[tv.long()].reshape(b, cols * P, hk, d).view(x.dtype) for x in (kpv, vpv))

    out.append(("padded pools", kpv, vpv, dict(block_table=tv), gathered, [(kpb, kpsl), (vpb, vpsl)]))
    return out


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "8bit"])
@pytest.mark.parametrize("dtname,d", ONE_OF_EACH)
def test_strided_storage_gives_the_bits_of_contiguous_storage(gpu, dtname, d, fp8):
    """q and the chunk's k / v are slices of one packed (b, sq, h + 2 h_k, d) qkv buffer, itself a view of a buffer with 8 poison elements
    behind every head (batch, row and head stride of q all differ from o's; the append reads k / v through their strides); the
    caches are views whose K and V differ in row and head stride, K and V interleaved in one allocation, and padded page pools behind a
    strided table.  Every gap holds the poison cycle, so a read from the wrong place is a NaN or an inf in the result and not a small error.
    Asserted: out / lse against fp64; out, lse and the logical caches after the append bit for bit against the call on contiguous tensors
    (the kernel's summation order does not depend on strides; for the pools that is the contiguous cache, which a paged call equals to the
    bit); every poison element of the gaps keeps its bits."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(71000 + d + int(fp8))
    prefixes = [0, 33, 777]
    cs = torch.tensor(prefixes, dtype=torch.int32, device=gpu)
    for sq in (17, 100):
        lens = [p + sq for p in prefixes]
        for h, hk in ((32, 8), (6, 2)):
            q, k, v, k_new, v_new, kl, vl = chunk_case(dt, d, sq, h, hk, gen, prefixes=prefixes)
            lkw = dict()
            if fp8:
                kds, vds, k, v, kl, vl = _quantised_case(k, v, k_new, v_new, prefixes, gen, gpu)
                lkw = dict(k_descale=kds, v_descale=vds)
            s = scores64(q, deq(kl, kds) if fp8 else kl)
            vref = deq(vl, vds) if fp8 else vl
            want = {c: exact(s, vref, visible(lens, sq, CAP, c)) for c in (False, True)}
            # (the packed buffer's rows are padded by 8 poison elements per head: q's head stride is d + 8 where o's is d)
            qkv, _, _ = _embed(torch.cat((q, k_new, v_new), dim=2).to(gpu), (0, 0, 0, 8), (0, 0, 0, 0))
            qs, kns, vns = qkv[:, :, :h], qkv[:, :, h:h + hk], qkv[:, :, h + hk:]
            assert not qs.is_contiguous() and not kns.is_contiguous() and not vns.is_contiguous() and qs.stride(2) == d + 8
            qc, knc, vnc, kg, vg = (t.to(gpu) for t in (q, k_new, v_new, k, v))
            copies = F._C.densify_copies()
            for causal in (False, True):
                for ns in SPLITS:
                    tag = f"layouts {'fp8 ' if fp8 else ''}{dtname} d{d} h{h}/{hk} sq{sq} causal={causal} splits={ns}"
                    kw = dict(cache_seqlens=cs, causal=causal, num_splits=ns, **lkw)
                    kc, vc = kg.clone(), vg.clone()
                    ref = _call(qc, kc, vc, k=knc, v=vnc, **kw)
                    assert _eq(kc, kl) and _eq(vc, vl), f"{tag}: the append on contiguous caches wrote something else than the chunk's rows"
                    for name, kk, vv, skw, logical, guards in _cache_layouts(kg, vg, 48, 13, fp8):
                        before = [_gap_bits(buf, sl).clone() for buf, sl in guards]
                        out, lse = _call(qs, kk, vv, k=kns, v=vns, **skw, **kw)
                        assert _same(out, ref[0]) and _same(lse, ref[1]), f"{tag}, {name}: other bits than on contiguous storage"
                        klog, vlog = logical()
                        assert _eq(klog, kl) and _eq(vlog, vl), f"{tag}, {name}: the logical caches after the append"
                        for (buf, sl), b0 in zip(guards, before):
                            assert torch.equal(_gap_bits(buf, sl), b0), f"{tag}, {name}: a gap element changed"
                        if name == "padded views":
                            check(out, lse, *want[causal], dtname, f"{tag}, {name}")
            assert F._C.densify_copies() == copies, "a strided tensor was copied instead of addressed"


# ---- B. 64-bit offsets -------------------------------------------------------------------------------------------------------------------------

def _run_c_abi(q, kc, vc, o, lse, cs, causal, num_splits, k_new=None, v_new=None, block_table=None, **ragged):
    """one 64-row launch through the C ABI (out / lse are the caller's buffers) with a NaN workspace of exactly the bytes the library asks for"""
    p = capi.kvcache_params(q, kc, vc, o, lse, cache_seqlens=cs, k_new=k_new, v_new=v_new, causal=causal, num_splits=num_splits, block_table=block_table,
                            cu_seqlens_q=ragged.get("cu_seqlens_q"), max_seqlen_q=ragged.get("max_seqlen_q"))
    opt = capi.kvcache_options(row_tile=64, cu_seqlens_q=ragged.get("cu_seqlens_q"), total_q=q.shape[0] if ragged else 0)
    assert capi.kvcache_row_tile(p, opt) == 64
    ws = torch.full((max(capi.kvcache_workspace_bytes(p, opt), 16) // 4 + 64,), NAN, device=q.device)
    p.workspace, p.workspace_bytes = ws.data_ptr(), (ws.numel() - 64) * 4
    capi.run_fwd_kvcache(p, options=opt)
    torch.cuda.synchronize()
    assert torch.isnan(ws[-64:]).all().item(), "the workspace was written past the bytes the library asked for"


def _far_batch_entry(gpu):
    dt, d, h, hk, cap, sq = torch.float16, 128, 8, 2, 256, 70
    stride_b = 2 ** 31 + 64
    gen = torch.Generator().manual_seed(72000)

    def big(rows, heads):
        t = torch.empty(stride_b + rows * heads * d, dtype=dt, device=gpu).as_strided((2, rows, heads, d), (stride_b, heads * d, d, 1))
        t.copy_(_rand((2, rows, heads, d), dt, gen).to(gpu))
        return t

    kc, vc, q, o = big(cap, hk), big(cap, hk), big(sq, h), big(sq, h)
    assert all(t.stride(0) * t.element_size() > 2 ** 32 for t in (kc, vc, q, o))
    lse = torch.empty(2, h, sq, device=gpu)
    # without an append: the second sequence sees more keys than query rows, the first fewer (its first rows are dead under causal)
    lens = [60, 200]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for causal in (False, True):
        o.fill_(NAN)
        lse.fill_(NAN)
        _run_c_abi(q, kc, vc, o, lse, cs, causal, 0)
        xo, xl, nvis = exact(scores64(q, kc), vc, visible(lens, sq, cap, causal))
        check(o, lse, xo, xl, nvis, "fp16", f"64-bit offsets causal={causal}")
    # with the append
    pre = [60, 180]
    cs = torch.tensor(pre, dtype=torch.int32, device=gpu)
    k_new, v_new = _rand((2, sq, hk, d), dt, gen, 3.0).to(gpu), _rand((2, sq, hk, d), dt, gen).to(gpu)
    k_exp, v_exp = kc.clone(memory_format=torch.contiguous_format), vc.clone(memory_format=torch.contiguous_format)
    for i, L in enumerate(pre):
        k_exp[i, L:L + sq], v_exp[i, L:L + sq] = k_new[i], v_new[i]
    o.fill_(NAN)
    lse.fill_(NAN)
    _run_c_abi(q, kc, vc, o, lse, cs, True, 0, k_new, v_new)
    assert _eq(kc, k_exp) and _eq(vc, v_exp), "the append at the far batch entry"
    xo, xl, nvis = exact(scores64(q, k_exp), v_exp, visible([L + sq for L in pre], sq, cap, True))
    check(o, lse, xo, xl, nvis, "fp16", "64-bit offsets append")
    # the Python surface on contiguous copies (its own out) gives the same bits
    out2, lse2 = _call(q.contiguous(), k_exp.clone(), v_exp.clone(), k=k_new, v=v_new, cache_seqlens=cs, causal=True)
    assert _eq(o, out2) and _same(lse, lse2)


def test_batch_stride_beyond_2_to_the_31(gpu):
    """K, V, q and O with a batch stride of 2^31 + 64 elements (as_strided over one ~4.3 GB allocation per tensor, only the rows in use filled),
    70 query rows - two tiles at h / h_k = 4 - through the C ABI at row_tile = 64: the far batch entry, with and without the append"""
    torch.cuda.empty_cache()
    try:
        _far_batch_entry(gpu)
    finally:
        torch.cuda.empty_cache()


def _large_pool(gpu):
    dt, d, h, hk, P, sq = torch.float16, 128, 4, 1, 256, 70
    page_bytes = 2 * P * hk * d * 2
    nb = (5 << 30) // page_bytes + 64                          # ~5 GiB of pool
    try:
        pool = torch.empty((nb, 2, P, hk, d), dtype=dt, device=gpu)
    except torch.OutOfMemoryError:
        pytest.fail("a 5 GiB pool does not fit on the device")
    kp, vp = pool[:, 0], pool[:, 1]
    gen = torch.Generator().manual_seed(72500)
    first = (1 << 32) // page_bytes + 7                         # byte offset of the first used page > 2^32
    cols, b = 6, 3
    cap = cols * P
    used = first + torch.randperm(nb - first, generator=torch.Generator().manual_seed(3))[: b * cols]
    assert int(used.min()) * page_bytes > 2 ** 32
    tbuf = torch.full((b, 2 * cols + 5), -7, dtype=torch.int32)
    tbuf[:, 3:3 + cols] = used.view(b, cols).to(torch.int32)
    table = tbuf.to(gpu)[:, 3:3 + cols]
    k, v = _rand((b, cap, hk, d), dt, gen), _rand((b, cap, hk, d), dt, gen)
    q = _rand((b, sq, h, d), dt, gen)
    k_new, v_new = _rand((b, sq, hk, d), dt, gen, 3.0), _rand((b, sq, hk, d), dt, gen)
    idx = used.to(gpu)
    pool[idx] = torch.stack((k.view(b * cols, P, hk, d), v.view(b * cols, P, hk, d)), dim=1).to(gpu)
    qg, kng, vng = q.to(gpu), k_new.to(gpu), v_new.to(gpu)
    gather = lambda x: x[table.long()].reshape(b, cap, hk, d)
    # without an append
    lens = [cap, 2 * P + 1, 5]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    before = F._C.densify_copies()
    for causal, ns in ((False, 0), (True, 3)):
        out, lse = _call(qg, kp, vp, cache_seqlens=cs, causal=causal, num_splits=ns, block_table=table)
        out_c, lse_c = _call(qg, k.to(gpu), v.to(gpu), cache_seqlens=cs, causal=causal, num_splits=ns)
        assert _same(out, out_c) and _same(lse, lse_c), ("large pool", causal, ns)
        check(out, lse, *exact(scores64(q, k), v, visible(lens, sq, cap, causal)), "fp16", f"large pool causal={causal} splits={ns}")
    # with the append: it lands past 2^32 bytes as well
    pre = [0, P - 1, 3 * P]
    cs = torch.tensor(pre, dtype=torch.int32, device=gpu)
    kl, vl = k.clone(), v.clone()
    for i, L in enumerate(pre):
        kl[i, L:L + sq], vl[i, L:L + sq] = k_new[i], v_new[i]
    out, lse = _call(qg, kp, vp, k=kng, v=vng, cache_seqlens=cs, causal=True, block_table=table)
    assert F._C.densify_copies() == before
    assert _eq(gather(kp), kl) and _eq(gather(vp), vl), "large pool: the logical caches after the append"
    out_c, lse_c = _call(qg, k.to(gpu), v.to(gpu), k=kng, v=vng, cache_seqlens=cs, causal=True)
    assert _same(out, out_c) and _same(lse, lse_c), "large pool, append"
    check(out, lse, *exact(scores64(q, kl), vl, visible([L + sq for L in pre], sq, cap, True)), "fp16", "large pool append")


def test_pool_pages_past_2_to_the_32_bytes(gpu):
    """k and v views of one (num_blocks, 2, P, h_k, d) pool of ~5 GiB with pages of 256 rows, every used page past byte 2^32, the table a
    strided view: the contiguous call's bits, fp64 values, and the append through the table"""
    torch.cuda.empty_cache()
    try:
        _large_pool(gpu)
    finally:
        torch.cuda.empty_cache()


# ---- C. softmax_scale ----------------------------------------------------------------------------------------------------------------------------

SCALES = [0.02, 0.35]


@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "8bit"])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_softmax_scale(gpu, dtname, d, fp8):
    """softmax_scale 0.02 and 0.35 against scores64(q, k, scale=...) - over an 8-bit cache the scale meets k_descale in the kernel's `c` and
    `sc` - causal and not, split 0 / 1 / 3; 70 query rows at h / h_k = 4 (five tiles, the last one partly filled).  Precondition on the fp64
    expectations alone: at each scale O lies at least 4 x the mean_abs tolerance, and LSE at least 4 x LSE_TOL, from the expectation at the
    default scale, so a kernel that ignored the argument could not pass.  The default's fp32 value passed explicitly gives the bits of None."""
    dt = DT[dtname]
    h, hk, sq = 8, 2, 70
    gen = torch.Generator().manual_seed(73000 + d + int(fp8))
    prefixes = [0, 33, 777]
    lens = [p + sq for p in prefixes]
    cs = torch.tensor(prefixes, dtype=torch.int32, device=gpu)
    q, k, v, k_new, v_new, kl, vl = chunk_case(dt, d, sq, h, hk, gen, prefixes=prefixes)
    lkw = dict()
    if fp8:
        kds, vds, k, v, kl, vl = _quantised_case(k, v, k_new, v_new, prefixes, gen, gpu)
        lkw = dict(k_descale=kds, v_descale=vds)
    kref, vref = (deq(kl, kds), deq(vl, vds)) if fp8 else (kl, vl)
    default = float(np.float32(1 / math.sqrt(d)))
    qg, kng, vng, kg, vg = (t.to(gpu) for t in (q, k_new, v_new, k, v))
    tol = U.TOL[dtname]["mean_abs"]
    for causal in (False, True):
        vis = visible(lens, sq, CAP, causal)
        base = exact(scores64(q, kref), vref, vis)
        for scale in SCALES:
            xo, xl, nvis = exact(scores64(q, kref, scale=scale), vref, vis)
            gap_o, gap_l = float((xo - base[0]).abs().mean()), float((xl - base[1]).abs().mean())
            print(f"{dtname} d{d} fp8={fp8} causal={causal} scale {scale}: O mean gap {gap_o:.3e} ({gap_o / tol:.1f} x tol), LSE mean gap {gap_l:.3e}")
            assert gap_o >= 4 * tol and gap_l >= 4 * U.LSE_TOL, f"scale {scale} does not tell itself from the default"
            for ns in SPLITS:
                kc, vc = kg.clone(), vg.clone()
                out, lse = _call(qg, kc, vc, k=kng, v=vng, cache_seqlens=cs, causal=causal, num_splits=ns, softmax_scale=scale, **lkw)
                assert _eq(kc, kl) and _eq(vc, vl)
                check(out, lse, xo, xl, nvis, dtname, f"scale {scale} {'fp8 ' if fp8 else ''}{dtname} d{d} causal={causal} splits={ns}")
        for ns in SPLITS:
            kw = dict(k=kng, v=vng, cache_seqlens=cs, causal=causal, num_splits=ns, **lkw)
            a = _call(qg, kg.clone(), vg.clone(), **kw)
            e = _call(qg, kg.clone(), vg.clone(), softmax_scale=default, **kw)
            assert _same(a[0], e[0]) and _same(a[1], e[1]), f"the default scale passed explicitly: other bits than None (causal={causal} splits={ns})"
            check(*e, *base, dtname, f"explicit default scale {'fp8 ' if fp8 else ''}{dtname} d{d} causal={causal} splits={ns}")


# ---- D. the plain ragged grid -------------------------------------------------------------------------------------------------------------------

def grid_is_compact(total_q, b, max_seqlen_q, h, hk, tile=64):
    """kvcache_ragged_slots of the library restated: a ragged launch looks its tile slots up in cu_seqlens_q (compact) iff
    ceil(total_q * r / tile) + b < b * ceil(max_seqlen_q * r / tile) with r = h / h_k; otherwise slot = sequence x tiles(max_seqlen_q) + tile
    (plain).  total_q counts the rows of q, those past cu_seqlens_q[-1] included."""
    r = h // hk
    return -((-total_q * r) // tile) + b < b * -((-max_seqlen_q * r) // tile)


def test_the_restated_grid_rule():
    """(no device work) sides worked out by hand: the five cases of test_plain_ragged_grid without their surplus rows, e.g. 3 x 64 rows at
    h / h_k = 1: 3 + 3 = 6 >= 3 x 1, and the ragged cases of test_kvcache_prefill_gpu.py, e.g. sq (63, 0, 4, 130, 1, 64, 65) at h / h_k = 4:
    21 + 7 = 28 < 7 x 9 = 63"""
    assert not grid_is_compact(192, 3, 64, 8, 8) and not grid_is_compact(192, 3, 64, 32, 8)
    assert not grid_is_compact(100, 4, 40, 6, 2) and not grid_is_compact(113, 4, 40, 32, 8) and not grid_is_compact(192, 3, 100, 8, 8)
    assert grid_is_compact(327, 7, 130, 32, 8) and grid_is_compact(327, 7, 130, 6, 2) and grid_is_compact(181, 3, 100, 32, 8) and grid_is_compact(181, 3, 100, 6, 2)


D_CAP = 336             # 7 pages of 48 rows
PLAIN_CASES = {
    "64-64-64 h8k8": ([64, 64, 64], 64, (8, 8)),
    "64-64-64 h32k8": ([64, 64, 64], 64, (32, 8)),
    "40-0-20-40 h6k2": ([40, 0, 20, 40], 40, (6, 2)),           # an empty sequence; sequence 2 fills one of its two slots
    "40-0-33-40 h32k8": ([40, 0, 33, 40], 40, (32, 8)),
    "max_seqlen_q 100 above every sq h8k8": ([64, 64, 64], 100, (8, 8)),    # the second slot of every sequence takes the early return
}
D_LENS = {3: [100, 33, 270], 4: [100, 5, 0, 290]}       # the prefixes when the call appends, the lengths when it does not


@pytest.mark.parametrize("case", list(PLAIN_CASES))
@pytest.mark.parametrize("dtname,d", ONE_OF_EACH)
def test_plain_ragged_grid(gpu, dtname, d, case):
    """ragged calls whose grid is NOT compact (asserted from grid_is_compact): slot = sequence x tiles(max_seqlen_q) + tile, and the slots of a
    sequence shorter than max_seqlen_q return early.  16-bit and 8-bit caches, contiguous and paged at P = 48, with and without the append,
    causal and not, num_splits 1 and a forced 3: each sequence against fp64, and bit for bit - out, lse, cache bytes - against the dense
    prefill call on it alone.  The ragged call reads q / k / v through padded views with poison in the gaps, the dense calls contiguous slices.  Through the C ABI, out / lse rows past cu_seqlens_q[-1] are pre-filled and keep their bits."""
    dt = DT[dtname]
    sqs, mx, (h, hk) = PLAIN_CASES[case]
    b, total, extra = len(sqs), sum(sqs), 3
    lens = D_LENS[b]
    assert not grid_is_compact(total + extra, b, mx, h, hk) and not grid_is_compact(total, b, mx, h, hk), "the case drifted to the compact grid"
    gen = torch.Generator().manual_seed(74000 + d + h)
    c0s = [0] + list(np.cumsum(sqs))
    cu = torch.tensor(c0s, dtype=torch.int32, device=gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, D_CAP, hk, d), dt, gen), _rand((b, D_CAP, hk, d), dt, gen)
    q = _rand((total + extra, h, d), dt, gen)
    q[total:] = NAN
    k_new, v_new = _rand((total, hk, d), dt, gen, 3.0), _rand((total, hk, d), dt, gen)
    qg, kng, vng = q.to(gpu), k_new.to(gpu), v_new.to(gpu)
    # the ragged call reads q, k and v through views padded by a head and by 8 elements per head (poison in the gaps); the dense calls it is
    # compared with read contiguous slices
    qr, knr, vnr = (_embed(t, (0, 1, 8), (0, 0, 0))[0] for t in (qg, kng, vng))
    assert qr.stride(0) == (h + 1) * (d + 8) and qr.stride(1) == d + 8
    for fp8 in (False, True):
        if fp8:
            kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
            kb, vb = quantise(k, kds), quantise(v, vds)
            new = [(quantise(k_new[c0s[i]:c0s[i + 1]][None], kds[i:i + 1])[0], quantise(v_new[c0s[i]:c0s[i + 1]][None], vds[i:i + 1])[0]) for i in range(b)]
            lkw = dict(k_descale=kds, v_descale=vds)
        else:
            kb, vb = k, v
            new = [(k_new[c0s[i]:c0s[i + 1]], v_new[c0s[i]:c0s[i + 1]]) for i in range(b)]
            lkw = dict()
        kl, vl = kb.clone(), vb.clone()
        for i, s in enumerate(sqs):
            kl[i, lens[i]:lens[i] + s], vl[i, lens[i]:lens[i] + s] = new[i]
        want = {}
        for append in (False, True):
            kr, vr = ((deq(kl, kds), deq(vl, vds)) if append else (deq(kb, kds), deq(vb, vds))) if fp8 else ((kl, vl) if append else (kb, vb))
            for i, s in enumerate(sqs):
                if s:
                    sc = scores64(q[c0s[i]:c0s[i + 1]][None], kr[i:i + 1])
                    for causal in (False, True):
                        want[append, causal, i] = exact(sc, vr[i:i + 1], visible([lens[i] + (s if append else 0)], s, D_CAP, causal))
        kg, vg = kb.to(gpu), vb.to(gpu)
        for paged in (False, True):
            pkw = dict(lkw)
            kk, vv = kg, vg
            if paged:
                kk, vv, table = (_page8(kg, vg, 48, 5) if fp8 else _page(kg, vg, 48, 5))[:3]
                pkw["block_table"] = table
            for ns in (1, 3):
                for append in (False, True):
                    for causal in (False, True):
                        tag = f"plain grid {case} {'fp8 ' if fp8 else ''}{'paged ' if paged else ''}{dtname} d{d} splits={ns} append={append} causal={causal}"
                        kw = dict(num_splits=ns, causal=causal)
                        kr, vr = kk.clone(), vv.clone()
                        rag = dict(k=knr, v=vnr, cu_seqlens_k_new=cu) if append else dict()
                        out, lse = _call(qr, kr, vr, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=mx, **rag, **pkw, **kw)
                        assert out.shape == qg.shape and lse.shape == (h, total + extra)
                        kd, vd = kk.clone(), vv.clone()
                        for i, s in enumerate(sqs):
                            if s == 0:
                                continue
                            c0 = c0s[i]
                            one = {key: val[i:i + 1] for key, val in pkw.items()}
                            if append:
                                one.update(k=kng[c0:c0 + s][None], v=vng[c0:c0 + s][None])
                            od, ld = _call(qg[c0:c0 + s][None], kd if paged else kd[i:i + 1], vd if paged else vd[i:i + 1], cache_seqlens=cs[i:i + 1], **one, **kw)
                            assert _same(out[c0:c0 + s], od[0]) and _same(lse[:, c0:c0 + s], ld[0]), f"{tag}: sequence {i} differs from the dense call on it alone"
                            check(out[c0:c0 + s][None], lse[:, c0:c0 + s][None], *want[append, causal, i], dtname, f"{tag} seq{i}")
                        assert _same(kr, kd) and _same(vr, vd), f"{tag}: cache bytes"
                        if append and not paged:
                            assert _eq(kr, kl) and _eq(vr, vl), f"{tag}: the logical caches after the append"
    # rows of out / lse past cu_seqlens_q[-1] keep their bits (the C ABI: out and lse are the caller's)
    kg, vg = k.to(gpu), v.to(gpu)
    for ns in (1, 3):
        for causal in (False, True):
            o = torch.full((total + extra, h, d), U.SENT16, dtype=torch.int16, device=gpu).view(dt)
            l = torch.full((h, total + extra), -7.25, device=gpu)
            _run_c_abi(qg, kg, vg, o, l, cs, causal, ns, cu_seqlens_q=cu, max_seqlen_q=mx)
            assert (U.bits(o[total:]) == U.SENT16).all().item() and (l[:, total:] == -7.25).all().item(), "rows past cu_seqlens_q[-1] were written"
            out, lse = _call(qg, kg, vg, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=mx, num_splits=ns, causal=causal)
            assert _same(o[:total], out[:total]) and _same(l[:, :total], lse[:, :total])


# ---- E. many sequences ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [65, 130, 513, 600])
@pytest.mark.parametrize("dtname,d,heads", [("fp16", 128, (32, 8)), ("bf16", 64, (6, 2))], ids=["fp16-d128-h32k8", "bf16-d64-h6k2"])
def test_many_sequences(gpu, b, dtname, d, heads):
    """kvc_slot_lookup<64> with more than one sequence per lane (b > 64) and a second round of 512 (b > 512): sq_i from {0, 1, 3, 17, 64,
    65} with empty sequences in the first 64 and past index 512, caches of 128 rows with lengths in [0, 128], causal, num_splits 1 and a forced
    2, on the compact grid (asserted).  Every sequence bit for bit against the dense prefill call (batched by sq: a dense batch entry is tiled
    like a sequence of the ragged call), a sample of at least 40 against fp64."""
    dt = DT[dtname]
    h, hk = heads
    cap, mx = 128, 65
    rng = np.random.default_rng(75000 + b)
    sq = [int(x) for x in rng.choice([0, 1, 3, 17, 64, 65], size=b)]
    lens = [int(x) for x in rng.integers(0, cap + 1, size=b)]
    sq[0], sq[b - 1], sq[5], lens[1], lens[2] = 64, 65, 0, 0, cap
    special = [i for i in (0, 63, 64, 65, 511, 512, 513, b - 1) if i < b]
    for i in special:
        sq[i] = sq[i] or 3
    if b > 520:
        sq[520] = 0
    assert 0 in sq[:64] and (b <= 520 or 0 in sq[513:])
    total = sum(sq)
    assert grid_is_compact(total, b, mx, h, hk), "the case drifted to the plain grid"
    gen = torch.Generator(device=gpu).manual_seed(75000 + b)
    rnd = lambda *shape: torch.randn(*shape, device=gpu, dtype=torch.float32, generator=gen).to(dt)
    kc, vc, q = rnd(b, cap, hk, d), rnd(b, cap, hk, d), rnd(total, h, d)
    cul = [0] + [int(x) for x in np.cumsum(sq)]
    cu, cs = torch.tensor(cul, dtype=torch.int32, device=gpu), torch.tensor(lens, dtype=torch.int32, device=gpu)
    sample = sorted(set(special) | set(range(0, b, max(1, b // 60))))
    sample = [i for i in sample if sq[i] > 0]
    assert len(sample) >= 40
    want = {i: exact(scores64(q[cul[i]:cul[i + 1]][None], kc[i:i + 1]), vc[i:i + 1], visible([lens[i]], sq[i], cap, True)) for i in sample}
    for ns in (1, 2):
        out, lse = _call(q, kc, vc, cache_seqlens=cs, causal=True, num_splits=ns, cu_seqlens_q=cu, max_seqlen_q=mx)
        for s in sorted(set(sq) - {0}):
            idx = [i for i in range(b) if sq[i] == s]
            rows = torch.tensor([[cul[i] + t for t in range(s)] for i in idx], device=gpu)
            ii = torch.tensor(idx, device=gpu)
            od, ld = _call(q[rows], kc[ii], vc[ii], cache_seqlens=cs[ii], causal=True, num_splits=ns)
            assert _same(out[rows], od), f"b{b} splits={ns}: a sequence of {s} rows differs from its dense call in out"
            assert _same(lse[:, rows].permute(1, 0, 2).contiguous(), ld), f"b{b} splits={ns}: a sequence of {s} rows differs from its dense call in lse"
        for i in sample:
            check(out[cul[i]:cul[i + 1]][None], lse[:, cul[i]:cul[i + 1]][None], *want[i], dtname, f"b{b} {dtname} h{h}/{hk} splits={ns} seq{i}")


# ---- F. softmax extremes --------------------------------------------------------------------------------------------------------------------------

X_CAP, X_L, X_SQ = 3072, 3000, 70       # 94 steps of 32 keys; 70 query rows at h / h_k = 4: five tiles whose waves end at different causal limits


def _extreme_case(pattern):
    """the patterns of test_kvcache_edges_gpu.py::test_softmax_extremes for 70 query rows of 4 heads over one KV head.  What had to move: the
    spike is the key of the LAST query row (under causal the first one does not see the last split), and the block of lse_gap_last ends where
    the first row's keys end (L - sq), so that every row sees it under causal as well; both still lie in the last of 7 splits."""
    d, h, cap, L, sq = 128, 4, X_CAP, X_L, X_SQ
    gen = torch.Generator().manual_seed(76000)
    q = torch.randn(1, sq, h, d, generator=gen) * 0.5 + 1.0
    k = torch.randn(1, cap, 1, d, generator=gen) * 0.5
    v = torch.randn(1, cap, 1, d, generator=gen)
    chunk = -(-(-(-cap // 32)) // 7) * 32                  # the chunk of 7 splits
    rest = None
    if pattern.startswith("ramp"):
        ramp = 1.0 if pattern == "ramp_up" else -1.0
        k = k + (ramp * torch.arange(cap).float() / 64.0 / d ** 0.5).view(1, cap, 1, 1)
    elif pattern == "spike_last_split":
        assert L - sq - 5 >= 6 * chunk
        k[0, L - sq - 5, 0] = q[0, sq - 1, 0]               # score |q|^2 / sqrt(d) ~ 14 above the rest, for every row (q's mean is 1)
    elif pattern == "scaled_by_6":
        q, k = q * 6.0, torch.randn(1, cap, 1, d, generator=gen) * 6.0
    else:
        # a block of keys along the mean direction of q's 280 rows (each lies within a few degrees of it), 140 / sqrt(d) x |q| ~ 125 nats
        # above the other keys' scores for every row (the 16-row test has two rows and uses the first one's direction at 130)
        block = slice(0, chunk) if pattern == "lse_gap_first" else slice(L - sq - 40, L - sq)
        assert pattern == "lse_gap_first" or block.start >= 6 * chunk
        qdir = q[0].mean(dim=(0, 1)) / q[0].mean(dim=(0, 1)).norm()
        k[0, block, 0] = k[0, block, 0] + 140.0 * qdir
        rest = slice(chunk, L) if pattern == "lse_gap_first" else slice(0, L - sq - 40)
    return q.half(), k.half(), v.half(), rest


@pytest.mark.parametrize("num_splits", [1, 7, 0])
@pytest.mark.parametrize("pattern", ["ramp_up", "ramp_down", "spike_last_split", "scaled_by_6", "lse_gap_first", "lse_gap_last"])
def test_softmax_extremes(gpu, pattern, num_splits):
    """the running max and alpha of compute_step across 94 steps, both LDS stages and the empty-partial rule across splits: scores that rise /
    fall along the key axis, one dominant key in the last split, q and k scaled by 6 (near one-hot rows), and splits whose LSE lies more than
    100 above the others.  Asserted as the 16-row test asserts: _util.check_kvcache_rows (C oracle and fp64), scale = 2 for the ramps."""
    q, k, v, rest = _extreme_case(pattern)
    L = X_L
    qg, kg, vg = q.to(gpu), k.to(gpu), v.to(gpu)
    cs = torch.tensor([L], dtype=torch.int32, device=gpu)
    for causal in (False, True):
        out, lse = _call(qg, kg, vg, cache_seqlens=cs, causal=causal, num_splits=num_splits)
        assert torch.isfinite(out).all().item() and torch.isfinite(lse).all().item(), (pattern, causal)
        if rest is not None:
            _, rl = U.fp64_math(q[0], k[0, :L], v[0, :L], causal)
            _, rl_rest = U.fp64_math(q[0], k[0, rest], v[0, rest], False)
            assert (rl - rl_rest).min().item() > 100.0, "the case must put an LSE gap > 100 between splits"
        U.check_kvcache_rows(out, lse, q, k, v, [L], causal, "fp16", f"prefill {pattern} n{num_splits} causal={causal}", scale=2.0 if pattern.startswith("ramp") else 1.0)


@pytest.mark.parametrize("num_splits", [1, 3, 0])
@pytest.mark.parametrize("L", [130, 30])
def test_causal_late_start(gpu, L, num_splits):
    """causal, 100 query rows at h / h_k = 4 over L = 130 keys (row t sees keys 0 .. 30 + t: in every step past its limit a lane has mx = -inf
    for the whole step beside live lanes of its wave, and in a later split a tile's first rows see nothing - m_run stays kNegBig - while its
    last rows do) and over L = 30 (rows 0 .. 69 are dead: whole dead tiles, then a tile whose first rows are dead and whose last rows are
    live).  The NEWEST key each row sees, j = L - sq + t, scores about +40 for that row and about 0 for every other: the row's result is that
    key's V row, so a limit off by one key shows as a wrong row and not as a small error.  fp64 values, dead rows exactly 0."""
    dt, d, h, hk, sq, cap = torch.float16, 128, 4, 1, 100, 256
    gen = torch.Generator().manual_seed(76500 + L)
    a = math.sqrt(40.0 * math.sqrt(d))
    q, k, v = _rand((1, sq, h, d), dt, gen, 0.5), _rand((1, cap, hk, d), dt, gen, 0.5), _rand((1, cap, hk, d), dt, gen)
    for t in range(sq):
        q[0, t, :, t] = a
        if 0 <= L - sq + t:
            k[0, L - sq + t, 0, t] = a
    s = scores64(q, k)
    vis = visible([L], sq, cap, True)
    xo, xl, nvis = exact(s, v, vis)
    assert int((nvis == 0).sum()) == max(sq - L, 0)
    live = [t for t in range(sq) if L - sq + t >= 0]
    top = torch.stack([s[0, 0, :, t, L - sq + t] for t in live])
    others = torch.stack([s[0, 0, :, t, :L - sq + t].amax(-1) if L - sq + t > 0 else torch.full((h,), -50.0, dtype=torch.float64) for t in live])
    assert float(top.min()) > 35.0 and float((top - others).min()) > 25.0, "the newest visible key must dominate its row"
    cs = torch.tensor([L], dtype=torch.int32, device=gpu)
    out, lse = _call(q.to(gpu), k.to(gpu), v.to(gpu), cache_seqlens=cs, causal=True, num_splits=num_splits)
    check(out, lse, xo, xl, nvis, "fp16", f"late start L{L} splits={num_splits}")


# ---- G. pages and packing ratios -------------------------------------------------------------------------------------------------------------------

G_PREFIXES = [0, 31, 33, 255, 257, 777]


@pytest.mark.parametrize("P", [32, 64, 256])
@pytest.mark.parametrize("dtname,d", ONE_OF_EACH)
def test_page_sizes(gpu, dtname, d, P):
    """the page cursor of fetch_pages at P = 32 (a step is exactly one page), 64 and 256 (many steps inside a page; at a forced 5 splits a
    split starts deep inside one): paged == contiguous to the bit, the append going through the table, and fp64 values; 16-bit and 8-bit
    caches, causal and not, split 0 / 1 / 3 / 5.  Table entries past the pages a sequence needs are out of range."""
    dt = DT[dtname]
    cap = 1280 if P == 256 else 1024
    gen = torch.Generator().manual_seed(77000 + d + P)
    b = len(G_PREFIXES)
    cs = torch.tensor(G_PREFIXES, dtype=torch.int32, device=gpu)
    for sq, (h, hk) in ((17, (32, 8)), (100, (6, 2))):
        lens = [p + sq for p in G_PREFIXES]
        q, k, v, k_new, v_new, kl, vl = chunk_case(dt, d, sq, h, hk, gen, prefixes=G_PREFIXES, cap=cap)
        qg, kng, vng = q.to(gpu), k_new.to(gpu), v_new.to(gpu)
        for fp8 in (False, True):
            lkw = dict()
            kb, vb, klb, vlb = k, v, kl, vl
            if fp8:
                kds, vds, kb, vb, klb, vlb = _quantised_case(k, v, k_new, v_new, G_PREFIXES, gen, gpu)
                lkw = dict(k_descale=kds, v_descale=vds)
            s = scores64(q, deq(klb, kds) if fp8 else klb)
            vref = deq(vlb, vds) if fp8 else vlb
            kg, vg = kb.to(gpu), vb.to(gpu)
            kp, vp, table = (_page8(kg, vg, P, 7 + P) if fp8 else _page(kg, vg, P, 7 + P))[:3]
            for i, L in enumerate(lens):
                table[i, (L + P - 1) // P:] = 1 << 30 if i % 2 else -7
            gather = lambda x: _bits(x)[table.long().clamp(0, x.shape[0] - 1)].reshape(b, cap, hk, d).view(x.dtype)
            for causal in (False, True):
                xo, xl, nvis = exact(s, vref, visible(lens, sq, cap, causal))
                for ns in (0, 1, 3, 5):
                    tag = f"P{P} {'fp8 ' if fp8 else ''}{dtname} d{d} h{h}/{hk} sq{sq} causal={causal} splits={ns}"
                    kw = dict(k=kng, v=vng, cache_seqlens=cs, causal=causal, num_splits=ns, **lkw)
                    kc, vc, kpc, vpc = kg.clone(), vg.clone(), kp.clone(), vp.clone()
                    ref = _call(qg, kc, vc, **kw)
                    out, lse = _call(qg, kpc, vpc, block_table=table, **kw)
                    assert _same(out, ref[0]) and _same(lse, ref[1]), f"{tag}: paged differs from contiguous"
                    assert _eq(kc, klb) and _eq(vc, vlb), f"{tag}: the append on the contiguous cache"
                    gk, gv = gather(kpc), gather(vpc)
                    for i, L in enumerate(lens):
                        assert _eq(gk[i, :L], klb[i, :L]) and _eq(gv[i, :L], vlb[i, :L]), f"{tag}: the append through the table, sequence {i}"
                    check(out, lse, xo, xl, nvis, dtname, tag)


@pytest.mark.parametrize("dtname,d,heads", [("fp16", 64, (64, 1)), ("bf16", 64, (80, 1)), ("fp16", 128, (128, 2))], ids=["h64k1", "h80k1", "h128k2"])
def test_packing_ratios_of_64_and_above(gpu, dtname, d, heads):
    """h / h_k = 64 (a tile is exactly one token), 80 (a token's heads straddle tiles, and a tile's first and last row can belong to the same
    token) and 64 over two KV heads: t_last and the causal k_hi of a tile.  sq 1 / 2 / 5 over 0 / 1 / 33 / 100 keys without an append, so that
    L < sq leaves dead rows; causal and not, split 0 / 1 / 3; fp64 values, dead rows exactly 0."""
    dt = DT[dtname]
    h, hk = heads
    gen = torch.Generator().manual_seed(78000 + h)
    lens, cap = [0, 1, 33, 100], 128
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((len(lens), cap, hk, d), dt, gen, 3.0), _rand((len(lens), cap, hk, d), dt, gen)
    kg, vg = k.to(gpu), v.to(gpu)
    for sq in (1, 2, 5):
        q = _rand((len(lens), sq, h, d), dt, gen)
        s = scores64(q, k)
        for causal in (False, True):
            xo, xl, nvis = exact(s, v, visible(lens, sq, cap, causal))
            assert int((nvis == 0).sum()) == (sq if not causal else sum(max(sq - L, 0) for L in lens))
            for ns in SPLITS:
                out, lse = _call(q.to(gpu), kg, vg, cache_seqlens=cs, causal=causal, num_splits=ns)
                check(out, lse, xo, xl, nvis, dtname, f"ratio {h // hk} {dtname} d{d} sq{sq} causal={causal} splits={ns}")
