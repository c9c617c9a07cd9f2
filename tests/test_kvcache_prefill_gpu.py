"""GPU: the 64-row attention kernels for prompt chunks (flash_attn_with_kvcache(..., prefill=True), fa_kvcache_options_v8.row_tile = 64).

Values are compared with fp64 math over the visible keys (the masked softmax of the tree suite, with the visibility rule written here: key j
< L_i, under causal j <= L_i - sq + t) through _util.assert_close without an oracle and _util.LSE_TOL: the tolerances of the 16-row path,
no new number.  Rows that see no key are asserted exactly, O = 0 and LSE = 0.  Shapes are small: the point is tile and step boundaries - 64
rows per workgroup, 16 per wave, 32 keys per step - not workload size.  Everything else is a relation that must hold to the bit, the NaN
rules, what is never read, graph capture, and one timing relation against the 16-row kernels."""
import statistics

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_fp8_gpu import _descale, deq, quantise
from test_kvcache_fp8_gpu import _page as _page8
from test_kvcache_softcap_gpu import DT, _rand, _same
from test_kvcache_tree_gpu import check, exact, scores64
from test_kvcache_window_gpu import _page

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
CAP = 1008                              # 21 pages of 48 rows = 63 pages of 16: holds the longest prefix (777) plus the longest chunk (100)
SQS = [1, 5, 16, 17, 33, 100]
HEADS = [(8, 8), (32, 8), (6, 2), (16, 1)]          # packing ratios 1, 4, 3 (a 64-row tile cuts through a token's heads) and 16
PREFIXES = [0, 1, 31, 33, 100, 777]
SPLITS = [0, 1, 3]


def visible(lens, sq, cap, causal):
    """bool (b, sq, cap): row t of sequence i sees key j iff j < L_i and, under causal, j <= L_i - sq + t"""
    j = torch.arange(cap).view(1, 1, cap)
    t = torch.arange(sq).view(1, sq, 1)
    L = torch.tensor(lens).view(-1, 1, 1)
    vis = j < L
    if causal:
        vis = vis & (j <= L - sq + t)
    return vis.expand(len(lens), sq, cap).clone()


def chunk_case(dt, d, sq, h, hk, gen, prefixes=PREFIXES, cap=CAP):
    """q, the cache holding the prefixes, and the chunk's k / v with K at 3 x the prefix's scale, so that the chunk's own keys carry weight
    against a long prefix (causal or not then matters); the logical caches after the append"""
    b = len(prefixes)
    k, v, q = _rand((b, cap, hk, d), dt, gen), _rand((b, cap, hk, d), dt, gen), _rand((b, sq, h, d), dt, gen)
    k_new, v_new = _rand((b, sq, hk, d), dt, gen, 3.0), _rand((b, sq, hk, d), dt, gen)
    kl, vl = k.clone(), v.clone()
    for i, pre in enumerate(prefixes):
        kl[i, pre:pre + sq], vl[i, pre:pre + sq] = k_new[i], v_new[i]
    return q, k, v, k_new, v_new, kl, vl


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("heads", HEADS, ids=lambda x: f"h{x[0]}k{x[1]}")
def test_prefill_against_fp64(gpu, dtname, d, heads):
    """The chunk is appended by the call itself (k / v at cache_seqlens = the prefix lengths, one batch entry per prefix length), causal and
    not, split 0 / 1 / 3.  Every call has its LSE and its dead rows asserted on its own; O is asserted per call as well.  From 17 rows on the
    case must tell causal from non-causal and the length limit from none: the fp64 expectations lie at least 4 x the mean_abs tolerance apart."""
    dt = DT[dtname]
    h, hk = heads
    gen = torch.Generator().manual_seed(51000 + d + h)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    tol = U.TOL[dtname]["mean_abs"]
    for sq in SQS:
        q, k, v, k_new, v_new, kl, vl = chunk_case(dt, d, sq, h, hk, gen)
        lens = [p + sq for p in PREFIXES]
        s = scores64(q, kl)
        qg, kng, vng = (t.to(gpu) for t in (q, k_new, v_new))
        want = {c: exact(s, vl, visible(lens, sq, CAP, c)) for c in (False, True)}
        if sq >= 17:
            nolimit = exact(s, vl, torch.ones(len(lens), sq, CAP, dtype=torch.bool))[0]
            for name, a, b_ in (("causal from non-causal", want[True][0], want[False][0]), ("the length limit from none", want[False][0], nolimit)):
                gap = float((a - b_).abs().mean())
                print(f"{dtname} d{d} h{h}/{hk} sq{sq}: {name}: mean gap of the expectations {gap:.3e} ({gap / tol:.1f} x mean_abs tol)")
                assert gap >= 4 * tol, f"sq{sq}: the case does not tell {name} (gap {gap:.3e})"
        for causal in (False, True):
            xo, xl, nvis = want[causal]
            for ns in SPLITS:
                tag = f"{dtname} d{d} h{h}/{hk} sq{sq} causal={causal} splits={ns}"
                kg, vg = k.to(gpu), v.to(gpu)
                out, lse = F.flash_attn_with_kvcache(qg, kg, vg, k=kng, v=vng, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, prefill=True)
                assert out.shape == q.shape and out.dtype == dt and lse.shape == (len(lens), h, sq) and lse.dtype == torch.float32
                assert _same(kg.cpu(), kl) and _same(vg.cpu(), vl), f"{tag}: the append wrote something else than the chunk's rows"
                check(out, lse, xo, xl, nvis, dtname, tag)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("heads", [(32, 8), (6, 2)], ids=lambda x: f"h{x[0]}k{x[1]}")
def test_prefill_over_an_fp8_cache_against_fp64(gpu, dtname, d, heads):
    """the same over an 8-bit cache with non-trivial descales, the chunk quantised by the call's append: against fp64 math on the dequantised
    cache after the append, whose bytes are asserted first"""
    dt = DT[dtname]
    h, hk = heads
    gen = torch.Generator().manual_seed(52000 + d + h)
    b = len(PREFIXES)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    for sq in (5, 17, 100):
        q, k, v, k_new, v_new, _, _ = chunk_case(dt, d, sq, h, hk, gen)
        kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
        k8, v8 = quantise(k, kds), quantise(v, vds)
        kl8, vl8 = k8.clone(), v8.clone()
        kn8, vn8 = quantise(k_new, kds), quantise(v_new, vds)
        for i, pre in enumerate(PREFIXES):
            kl8[i, pre:pre + sq], vl8[i, pre:pre + sq] = kn8[i], vn8[i]
        lens = [p + sq for p in PREFIXES]
        s = scores64(q, deq(kl8, kds))
        for causal in (False, True):
            xo, xl, nvis = exact(s, deq(vl8, vds), visible(lens, sq, CAP, causal))
            for ns in SPLITS:
                tag = f"fp8 {dtname} d{d} h{h}/{hk} sq{sq} causal={causal} splits={ns}"
                kg, vg = k8.to(gpu), v8.to(gpu)
                out, lse = F.flash_attn_with_kvcache(q.to(gpu), kg, vg, k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=cs, causal=causal, num_splits=ns,
                                                     return_softmax_lse=True, k_descale=kds, v_descale=vds, prefill=True)
                assert _same(kg.cpu(), kl8) and _same(vg.cpu(), vl8), f"{tag}: the append wrote other codes than the quantised chunk"
                check(out, lse, xo, xl, nvis, dtname, tag)


# ---- 2. relations that hold to the bit -------------------------------------------------------------------------------------------------------

def _layouts(k, v, gen, gpu, P, seed):
    """the same logical caches as (name, k, v, keywords): contiguous, paged, 8-bit, 8-bit paged - on the device.  The 8-bit pair is its own
    logical cache (the quantised one); relations are asserted within a cache element size."""
    b, hk = k.shape[0], k.shape[2]
    kg, vg = k.to(gpu), v.to(gpu)
    kp, vp, table, _ = _page(kg, vg, P, seed)
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
    kp8, vp8, table8 = _page8(k8, v8, P, seed + 1)
    return [("contiguous", kg, vg, dict()), ("paged", kp, vp, dict(block_table=table)), ("fp8", k8, v8, dict(k_descale=kds, v_descale=vds)),
            ("fp8 paged", kp8, vp8, dict(block_table=table8, k_descale=kds, v_descale=vds))]


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_is_contiguous_and_two_runs_are_identical(gpu, dtname, d):
    """paged == contiguous with pages of 16 and of 48 rows (a 32-key step straddles pages of 48), the append going through the table; two runs
    of the same call; 16-bit and 8-bit cache, causal and not, every split count: out and lse to the bit"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(53000 + d)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    for sq, (h, hk) in ((5, (6, 2)), (33, (32, 8)), (100, (8, 8)), (17, (16, 1))):
        q, k, v, k_new, v_new, _, _ = chunk_case(dt, d, sq, h, hk, gen)
        qg, kng, vng = q.to(gpu), k_new.to(gpu), v_new.to(gpu)
        for P in (16, 48):
            res = {}
            for name, kk, vv, lkw in _layouts(k, v, gen, gpu, P, 7 + P):
                for causal in (False, True):
                    for ns in SPLITS:
                        kw = dict(k=kng, v=vng, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, prefill=True, **lkw)
                        a = F.flash_attn_with_kvcache(qg, kk.clone(), vv.clone(), **kw)
                        again = F.flash_attn_with_kvcache(qg, kk.clone(), vv.clone(), **kw)
                        assert _same(again[0], a[0]) and _same(again[1], a[1]), ("second run", name, P, sq, causal, ns)
                        res[name, causal, ns] = a
            for causal in (False, True):
                for ns in SPLITS:
                    for x, y in (("contiguous", "paged"), ("fp8", "fp8 paged")):
                        assert _same(res[x, causal, ns][0], res[y, causal, ns][0]) and _same(res[x, causal, ns][1], res[y, causal, ns][1]), (x, y, P, sq, causal, ns)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_sequence_of_a_ragged_prefill_call_is_the_dense_prefill_call_on_it_alone(gpu, dtname, d):
    """sq_i in {0, 1, 4, 63, 64, 65, 130} (an empty sequence, tiles that end at, before and behind a sequence's rows), total_q >
    cu_seqlens_q[-1] with a NaN query in the surplus rows, num_splits = 1 and a forced 3; both layouts, 16-bit and 8-bit, with and without
    an append, causal and not: out, lse and every cache byte to the bit"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(54000 + d)
    sqs = [63, 0, 4, 130, 1, 64, 65]
    lens = [100, 5, 0, 300, 777, 33, 1]              # the prefixes when the call appends, the lengths when it does not
    b, total, extra = len(sqs), sum(sqs), 3
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for h, hk in ((32, 8), (6, 2)):
        k, v = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen)
        q = _rand((total + extra, h, d), dt, gen).to(gpu)
        q[total:] = NAN
        k_new, v_new = _rand((total, hk, d), dt, gen, 3.0).to(gpu), _rand((total, hk, d), dt, gen).to(gpu)
        for name, kk, vv, lkw in _layouts(k, v, gen, gpu, 48, 5)[:3]:
            for ns, append, causal in ((1, False, True), (1, True, False), (3, True, True), (3, False, False)):
                kw = dict(num_splits=ns, causal=causal, return_softmax_lse=True, prefill=True)
                kr, vr = kk.clone(), vv.clone()
                rag = dict(k=k_new, v=v_new, cu_seqlens_k_new=cu) if append else dict()
                out, lse = F.flash_attn_with_kvcache(q, kr, vr, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=130, **rag, **lkw, **kw)
                assert out.shape == q.shape and lse.shape == (h, total + extra)
                assert torch.isfinite(out[:total]).all().item() and torch.isfinite(lse[:, :total]).all().item()
                kd, vd = kk.clone(), vv.clone()
                paged = "block_table" in lkw
                for i, s in enumerate(sqs):
                    if s == 0:
                        continue
                    c0 = sum(sqs[:i])
                    one = {key: val[i:i + 1] for key, val in lkw.items()}
                    if append:
                        one.update(k=k_new[c0:c0 + s][None], v=v_new[c0:c0 + s][None])
                    od, ld = F.flash_attn_with_kvcache(q[c0:c0 + s][None], kd if paged else kd[i:i + 1], vd if paged else vd[i:i + 1], cache_seqlens=cs[i:i + 1], **one, **kw)
                    assert _same(out[c0:c0 + s], od[0]) and _same(lse[:, c0:c0 + s], ld[0]), (name, h, hk, ns, append, causal, i)
                if append:
                    assert _same(kr, kd) and _same(vr, vd), (name, "cache bytes", ns)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("heads", [(32, 8), (6, 2)], ids=lambda x: f"h{x[0]}k{x[1]}")
def test_rows_that_see_no_key_are_exactly_zero(gpu, dtname, d, heads):
    """fewer keys than query rows and no append: L_i in {0, 1, 33} below sq in {17, 64, 100}.  Without causal the L = 0 sequence is dead; under
    causal row t sees keys j <= L - sq + t, so the first sq - L rows of every sequence are dead - whole 64-row tiles whose key range is empty
    (no step in an unsplit call, an empty partial from every split), tiles that are partly dead, and waves whose 16 rows are all dead beside
    live ones.  Dead rows are asserted exactly O = 0, LSE = 0 (split_rows of the tree suite), the others against fp64; dense, and the three
    chunk sizes as one ragged call."""
    dt = DT[dtname]
    h, hk = heads
    gen = torch.Generator().manual_seed(59000 + d + h)
    lens, cap = [0, 1, 33], 128
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, d), dt, gen, 3.0), _rand((b, cap, hk, d), dt, gen)
    kg, vg = k.to(gpu), v.to(gpu)
    for sq in (17, 64, 100):
        q = _rand((b, sq, h, d), dt, gen)
        s = scores64(q, k)
        for causal in (False, True):
            xo, xl, nvis = exact(s, v, visible(lens, sq, cap, causal))
            dead = int((nvis == 0).sum())
            assert dead == (sq if not causal else sum(max(sq - L, 0) for L in lens)) and dead > 0
            for ns in SPLITS:
                out, lse = F.flash_attn_with_kvcache(q.to(gpu), kg, vg, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, prefill=True)
                check(out, lse, xo, xl, nvis, dtname, f"dead rows {dtname} d{d} h{h}/{hk} sq{sq} causal={causal} splits={ns}")
                assert (out[0] == 0).all().item() and (lse[0] == 0).all().item()          # L = 0
    # ragged: sequence i brings sqs[i] rows over lens[i] keys
    sqs = [17, 64, 100]
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    q = _rand((sum(sqs), h, d), dt, gen)
    for causal in (False, True):
        want = []
        for i, sq in enumerate(sqs):
            c0 = sum(sqs[:i])
            want.append(exact(scores64(q[c0:c0 + sq][None], k[i:i + 1]), v[i:i + 1], visible(lens[i:i + 1], sq, cap, causal)))
        assert sum(int((w[2] == 0).sum()) for w in want) == (17 if not causal else 17 + 63 + 67)
        for ns in SPLITS:
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), kg, vg, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, cu_seqlens_q=cu,
                                                 max_seqlen_q=100, prefill=True)
            for i, sq in enumerate(sqs):
                c0 = sum(sqs[:i])
                check(out[c0:c0 + sq][None], lse[:, c0:c0 + sq][None], *want[i], dtname, f"dead rows ragged {dtname} d{d} h{h}/{hk} seq{i} causal={causal} splits={ns}")


# ---- 3. what is never read ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paged", [False, True])
def test_rows_pages_and_table_entries_past_the_length_are_never_read_and_outputs_stay_in_bounds(gpu, paged):
    """through the C ABI with guarded outputs: cache rows at or past L_i and pool pages no sequence needs hold the poison cycle (NaN, +-inf,
    65504), table entries past the needed pages are out of range, and out / lse live in guarded buffers whose guard must survive - one split
    and a forced one.  The result is that of the Python surface on clean copies, to the bit."""
    dt, d, h, hk, sq, P = torch.float16, 128, 12, 4, 70, 48
    gen = torch.Generator().manual_seed(55000)
    lens0 = [0, 31, 100, 777]
    b = len(lens0)
    lens = [p + sq for p in lens0]
    cs = torch.tensor(lens0, dtype=torch.int32, device=gpu)
    q, k, v, k_new, v_new, kl, vl = chunk_case(dt, d, sq, h, hk, gen, prefixes=lens0)
    for causal, ns in ((True, 1), (False, 4), (True, 4)):
        kc, vc = k.to(gpu), v.to(gpu)
        for i, L in enumerate(lens):
            U.poison_(kc[i, L:]), U.poison_(vc[i, L:])
        kw = dict()
        if paged:
            kc, vc, table, spare = _page(kc, vc, P, 11)
            for pg in spare:
                U.poison_(kc[pg]), U.poison_(vc[pg])
            for i, L in enumerate(lens):
                table[i, (L + P - 1) // P:] = 1 << 30 if i % 2 else -7
            kw = dict(block_table=table)
        obuf, o, osl = U.guarded((b, sq, h, d), dt, gpu, (2, 2, 2, 16))
        qg, kng, vng = q.to(gpu), k_new.to(gpu), v_new.to(gpu)
        # (the C ABI states lse by its pointer alone, a dense (b, h, sq) block: the guard sits in front of it and behind it)
        lbuf = torch.full((b * h * sq + 64,), -7.25, device=gpu)
        lse_c = lbuf[32:32 + b * h * sq].view(b, h, sq)
        p = capi.kvcache_params(qg, kc, vc, o, lse_c, cache_seqlens=cs, k_new=kng, v_new=vng, causal=causal, num_splits=ns, block_table=kw.get("block_table"))
        opt = capi.kvcache_options(row_tile=64)
        assert capi.kvcache_row_tile(p, opt) == 64
        ws = torch.full((max(capi.kvcache_workspace_bytes(p, opt), 16) // 4 + 64,), NAN, device=gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), (ws.numel() - 64) * 4
        assert capi.kvcache_num_splits(p, opt) == ns
        capi.run_fwd_kvcache(p, options=opt)
        torch.cuda.synchronize()
        assert torch.isfinite(o.float()).all().item() and torch.isfinite(lse_c).all().item(), f"causal={causal} splits={ns}: something that must not be read leaked into a result"
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[osl] = False
        assert (U.bits(obuf)[mask] == U.SENT16).all().item(), "out was written outside its rows"
        assert torch.isnan(ws[-64:]).all().item(), "the workspace was written past the bytes the library asked for"
        assert (lbuf[:32] == -7.25).all().item() and (lbuf[-32:] == -7.25).all().item(), "lse was written outside its block"
        xo, xl, nvis = exact(scores64(q, kl), vl, visible(lens, sq, CAP, causal))
        check(o, lse_c, xo, xl, nvis, "fp16", f"never read, paged={paged} causal={causal} splits={ns}")
        # the Python surface on clean caches gives the same bits
        kc2, vc2 = k.to(gpu), v.to(gpu)
        if paged:
            kc2, vc2, table2, _ = _page(kc2, vc2, P, 11)
            kw = dict(block_table=table2)
        out2, lse2 = F.flash_attn_with_kvcache(qg, kc2, vc2, k=kng, v=vng, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, prefill=True, **kw)
        assert _same(o.contiguous(), out2) and _same(lse_c.contiguous(), lse2)


# ---- 4. NaN rules --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", SPLITS)
def test_a_nan_query_row_and_an_inf_score_make_exactly_their_rows_nan(gpu, dtname, num_splits):
    dt = DT[dtname]
    d, h, hk, sq, L = 128, 6, 2, 70, 200
    gen = torch.Generator().manual_seed(56000)
    q, k, v = _rand((1, sq, h, d), dt, gen).to(gpu), _rand((1, 256, hk, d), dt, gen).to(gpu), _rand((1, 256, hk, d), dt, gen).to(gpu)
    kw = dict(cache_seqlens=L, num_splits=num_splits, return_softmax_lse=True, prefill=True)
    clean = F.flash_attn_with_kvcache(q, k, v, **kw)
    assert torch.isfinite(clean[0]).all().item() and torch.isfinite(clean[1]).all().item()
    # a NaN query row: row (t = 37, head 4) alone
    qn = q.clone()
    qn[0, 37, 4, 5] = NAN
    out, lse = F.flash_attn_with_kvcache(qn, k, v, **kw)
    bad = torch.zeros(1, sq, h, dtype=torch.bool, device=gpu)
    bad[0, 37, 4] = True
    assert torch.isnan(out[bad]).all().item() and torch.isnan(lse.permute(0, 2, 1)[bad]).all().item()
    assert _same(out[~bad], clean[0][~bad]) and _same(lse.permute(0, 2, 1)[~bad], clean[1].permute(0, 2, 1)[~bad])
    # a +inf score: key 150 of KV head 1 has one +inf element, and the rows of its query heads whose q there is positive score +inf
    # (those with a negative q score -inf there: the key drops out of their softmax and the row stays finite)
    ki = k.clone()
    ki[0, 150, 1, 9] = INF
    out, lse = F.flash_attn_with_kvcache(q, ki, v, **kw)
    ratio = h // hk
    bad = torch.zeros(1, sq, h, dtype=torch.bool, device=gpu)
    bad[0, :, ratio:2 * ratio] = q[0, :, ratio:2 * ratio, 9] > 0
    assert bad.any().item() and not bad[0, :, ratio:2 * ratio].all().item()
    assert torch.isnan(out[bad]).all().item() and torch.isnan(lse.permute(0, 2, 1)[bad]).all().item()
    assert torch.isfinite(out[~bad]).all().item() and torch.isfinite(lse.permute(0, 2, 1)[~bad]).all().item()
    other = torch.ones(1, sq, h, dtype=torch.bool, device=gpu)
    other[0, :, ratio:2 * ratio] = False
    assert _same(out[other], clean[0][other]) and _same(lse.permute(0, 2, 1)[other], clean[1].permute(0, 2, 1)[other])
    # under causal the rows that do not see key 150 keep the clean bits
    kwc = dict(kw, causal=True)
    cleanc = F.flash_attn_with_kvcache(q, k, v, **kwc)
    out, lse = F.flash_attn_with_kvcache(q, ki, v, **kwc)
    sees = torch.arange(sq, device=gpu) + (L - sq) >= 150
    badc = bad & sees.view(1, sq, 1)
    assert torch.isnan(out[badc]).all().item() and torch.isfinite(out[~badc]).all().item()
    blind = (~sees).view(1, sq, 1).expand(1, sq, h)
    assert _same(out[blind], cleanc[0][blind])


# ---- 5. graph capture ----------------------------------------------------------------------------------------------------------------------------

def test_captured_prefill_call_replays_with_new_lengths(gpu):
    """one captured call (append, attention, combine: a single chain of launches on one stream); cache_seqlens is rewritten in place before the
    replay, which must give the bits of the eager call on the new lengths and the fp64 values of those lengths"""
    dt, d, h, hk, b, sq = torch.float16, 64, 32, 8, 2, 40
    gen = torch.Generator().manual_seed(57000)
    k, v = _rand((b, 2048, hk, d), dt, gen, 2.0), _rand((b, 2048, hk, d), dt, gen)
    q = _rand((b, sq, h, d), dt, gen)
    qg, kg, vg = q.to(gpu), k.to(gpu), v.to(gpu)
    cs = torch.tensor([100, 2000], dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, causal=True, return_softmax_lse=True, prefill=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(qg, kg, vg, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(qg, kg, vg, **kw)
    first = (out_g.clone(), lse_g.clone())
    lens = [1500, 45]
    cs.copy_(torch.tensor(lens, dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = F.flash_attn_with_kvcache(qg, kg, vg, **kw)
    assert _same(out_g, out_e) and _same(lse_g, lse_e)
    assert not _same(out_g, first[0])
    xo, xl, nvis = exact(scores64(q, k), v, visible(lens, sq, 2048, True))
    check(out_g, lse_g, xo, xl, nvis, "fp16", "graph replay")


# ---- 6. the purpose --------------------------------------------------------------------------------------------------------------------------------

def test_prefill_is_faster_than_the_16_row_kernels_on_a_1024_row_chunk(gpu):
    """b 1, 1024 query rows over 4096 keys, h 32 / h_k 8, d 128, fp16, causal, contiguous: the median of 5 interleaved rounds of prefill=True must
    lie below that of prefill=False.  The bound is 1.0 and carries no margin: a wide tile that is not faster than the tile it replaces has no
    purpose.  The ratio is printed; the first line of profiles/kvcache_prefill_bench.log is copied from this test's output on the run recorded
    with the change."""
    dt, d, h, hk, sq, L = torch.float16, 128, 32, 8, 1024, 4096
    gen = torch.Generator().manual_seed(58000)
    q, k, v = _rand((1, sq, h, d), dt, gen).to(gpu), _rand((1, L, hk, d), dt, gen).to(gpu), _rand((1, L, hk, d), dt, gen).to(gpu)
    wide = lambda: F.flash_attn_with_kvcache(q, k, v, causal=True, prefill=True)
    narrow = lambda: F.flash_attn_with_kvcache(q, k, v, causal=True)
    a, b_ = wide(), narrow()
    m = U.error_metrics(a.float().cpu().numpy(), b_.float().cpu().numpy())
    assert m["max_abs"] <= U.TOL["fp16"]["max_abs"], m                     # (the same values: both within the tolerance of fp64, so within one of each other)
    torch.cuda.synchronize()
    tw, tn = [], []
    for _ in range(5):
        for fn, ts in ((wide, tw), (narrow, tn)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / 3)
    w, n = statistics.median(tw), statistics.median(tn)
    line = f"test_prefill_is_faster: b1 sq{sq} L{L} h{h}/{hk} d{d} fp16 causal contiguous: prefill=True {w:.4f} ms, prefill=False {n:.4f} ms, ratio {w / n:.3f}"
    print(line)
    assert w < n, line
