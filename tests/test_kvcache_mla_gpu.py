"""GPU: MLA decode over a latent KV cache (flash_mla_with_kvcache, fa_run_mla_fwd_kvcache).

Values are compared with fp64 math over the visible keys - scores64 / exact / check of the tree suite with k = the logical latent cache (576
columns) and v = its first 512 columns - through _util.assert_close without an oracle and _util.LSE_TOL: the tolerances of the decode path,
no new number.  Shapes sit on the kernel's boundaries (64 packed rows a workgroup, 16 a wave, 32 keys a step, 16 keys a page block), not at the
workload's sizes.  Everything else is a relation that must hold to the bit, the integer visibility probe of tests/_visibility.py, the NaN
rules, what is never read, graph capture, and the C ABI."""
import numpy as np
import pytest
import torch

import _util as U
import _visibility as V
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_prefill_gpu import visible
from test_kvcache_softcap_gpu import DT, _rand, _same
from test_kvcache_tree_gpu import check, exact, scores64
from test_kvcache_window_gpu import _page

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
DK, DV = 576, 512
CAP = 1008                              # 63 pages of 16 = 21 of 48: holds the longest prefix (777) plus the rows appended
HS = [1, 16, 24, 128]                   # one lane of one wave; one wave of the tile; a tile that cuts through a token's heads at sq > 1; two tiles
SQS = [1, 2, 5]
PREFIXES = [0, 1, 31, 33, 100, 777]
SPLITS = [0, 1, 3]
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(DK)))        # the default: 576 ** -0.5 rounded once to fp32


def mla_case(dt, sq, h, gen, prefixes=PREFIXES, cap=CAP):
    """q, the latent cache holding the prefixes, and the new rows at 3 x the prefix's scale (chunk_case of the prefill suite: the new keys carry
    weight against a long prefix, so causal or not matters); the logical cache after the append"""
    b = len(prefixes)
    kv, q = _rand((b, cap, 1, DK), dt, gen), _rand((b, sq, h, DK), dt, gen)
    kv_new = _rand((b, sq, 1, DK), dt, gen, 3.0)
    kvl = kv.clone()
    for i, pre in enumerate(prefixes):
        kvl[i, pre:pre + sq] = kv_new[i]
    return q, kv, kv_new, kvl


def page_kv(logical, P, seed, fill=NAN):
    """pool + table of the logical latent cache under a random page permutation; spare pages hold `fill`"""
    pool, _, table, spare = _page(logical, logical, P, seed, fill=fill)
    return pool, table, spare


def logical_of(pool, table, cap):
    return pool[table.long()].reshape(table.shape[0], cap, 1, DK)


# ---- 1. values -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("h", HS)
def test_mla_against_fp64(gpu, dtname, h):
    """kv_new is appended by the call itself (at cache_seqlens = the prefix lengths, one batch entry per prefix length), causal and not, split
    0 / 1 / 3; the cache bytes after the append are asserted exactly.  At sq = 5 the case must tell causal from non-causal: the fp64
    expectations lie at least 4 x the mean_abs tolerance apart."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(61000 + h)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    tol = U.TOL[dtname]["mean_abs"]
    for sq in SQS:
        q, kv, kv_new, kvl = mla_case(dt, sq, h, gen)
        lens = [p + sq for p in PREFIXES]
        s = scores64(q, kvl, SCALE)
        want = {c: exact(s, kvl[..., :DV], visible(lens, sq, CAP, c)) for c in (False, True)}
        if sq == 5:
            gap = float((want[True][0] - want[False][0]).abs().mean())
            print(f"{dtname} h{h} sq{sq}: causal from non-causal: mean gap of the expectations {gap:.3e} ({gap / tol:.1f} x mean_abs tol)")
            assert gap >= 4 * tol, f"sq{sq}: the case does not tell causal from non-causal (gap {gap:.3e})"
        qg, kng = q.to(gpu), kv_new.to(gpu)
        for causal in (False, True):
            xo, xl, nvis = want[causal]
            for ns in SPLITS:
                tag = f"mla {dtname} h{h} sq{sq} causal={causal} splits={ns}"
                kvg = kv.to(gpu)
                out, lse = F.flash_mla_with_kvcache(qg, kvg, cs, kv_new=kng, causal=causal, num_splits=ns, return_softmax_lse=True)
                assert out.shape == (len(lens), sq, h, DV) and out.dtype == dt and lse.shape == (len(lens), h, sq) and lse.dtype == torch.float32
                assert _same(kvg.cpu(), kvl), f"{tag}: the append wrote something else than the new rows"
                check(out, lse, xo, xl, nvis, dtname, tag)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_dead_rows_and_lengths_below_seqlen_q(gpu, dtname):
    """without an append: prefix 0 is a dead sequence (O = 0, LSE = 0 exactly, asserted by check), and under causal with L < sq the first sq - L
    rows see nothing"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(61500)
    lens = [0, 1, 2, 4, 33, 777]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for h, sq in ((16, 5), (24, 3), (128, 1)):
        q, kv, _, _ = mla_case(dt, sq, h, gen, prefixes=lens)
        s = scores64(q, kv, SCALE)
        for causal in (False, True):
            xo, xl, nvis = exact(s, kv[..., :DV], visible(lens, sq, CAP, causal))
            assert int((nvis == 0).sum()) >= sq
            for ns in SPLITS:
                out, lse = F.flash_mla_with_kvcache(q.to(gpu), kv.to(gpu), cs, causal=causal, num_splits=ns, return_softmax_lse=True)
                assert (out[0] == 0).all().item() and (lse[0] == 0).all().item()
                check(out, lse, xo, xl, nvis, dtname, f"mla dead {dtname} h{h} sq{sq} causal={causal} splits={ns}")


# ---- 2. the value path -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_single_key_returns_its_first_512_columns_bit_for_bit(gpu, dtname):
    """q one-hot in column c (compressed and rope columns alike), one visible key: the softmax weight is exactly 1 and out is kv[0, :512]"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(62000)
    cols = [0, 7, 255, 511, 512, 575]
    b, h = len(cols), 24
    kv = _rand((b, 64, 1, DK), dt, gen).to(gpu)
    q = torch.zeros(b, 2, h, DK, dtype=dt, device=gpu)
    for i, c in enumerate(cols):
        q[i, :, :, c] = 1.5
    for ns in SPLITS:
        for causal in (False, True):
            out, lse = F.flash_mla_with_kvcache(q, kv, 1 if not causal else 2, causal=causal, num_splits=ns, return_softmax_lse=True)
            # (causal with L = 2: row 0 sees key 0 alone, row 1 keys 0 and 1)
            want = kv[:, 0, 0, :DV].unsqueeze(1).expand(b, h, DV)
            assert _same(out[:, 0].contiguous(), want.contiguous()), f"splits={ns} causal={causal}"
            if not causal:
                assert _same(out[:, 1].contiguous(), want.contiguous())
                x = (1.5 * kv[:, 0, 0].cpu().double()[torch.arange(b), cols] * SCALE).view(b, 1, 1).expand(b, h, 2)
                assert float((lse.double().cpu() - x).abs().max()) <= U.LSE_TOL


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_rope_columns_reach_the_lse_and_never_out(gpu, dtname):
    """with q[..., 512:] = 0, perturbing only kv[..., 512:] changes no bit of out or lse: the value is the first 512 columns; with the rope part of
    q in place the same perturbation moves the LSE (the columns are read for the scores)"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(62500)
    lens = [1, 33, 100, 777]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    q, kv, _, _ = mla_case(dt, 2, 24, gen, prefixes=lens)
    kv2 = kv.clone()
    kv2[..., DV:] = _rand((len(lens), CAP, 1, DK - DV), dt, gen, 5.0)
    q0 = q.clone()
    q0[..., DV:] = 0
    for ns in SPLITS:
        a = F.flash_mla_with_kvcache(q0.to(gpu), kv.to(gpu), cs, causal=True, num_splits=ns, return_softmax_lse=True)
        b_ = F.flash_mla_with_kvcache(q0.to(gpu), kv2.to(gpu), cs, causal=True, num_splits=ns, return_softmax_lse=True)
        assert _same(a[0], b_[0]) and _same(a[1], b_[1]), f"splits={ns}"
        c = F.flash_mla_with_kvcache(q.to(gpu), kv.to(gpu), cs, causal=True, num_splits=ns, return_softmax_lse=True)
        d = F.flash_mla_with_kvcache(q.to(gpu), kv2.to(gpu), cs, causal=True, num_splits=ns, return_softmax_lse=True)
        assert float((c[1] - d[1]).abs().mean()) > 0.1 and not _same(c[1], a[1])


# ---- 3. relations that hold to the bit -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [16, 48, 64])
def test_paged_is_contiguous_and_runs_are_identical(gpu, dtname, P):
    """shuffled tables, spare pages full of NaN, the append through the table: out, lse and every logical cache byte, for every split count"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(63000 + P)
    cap = CAP if P != 64 else 1024
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    for h, sq in ((24, 5), (128, 2)):
        q, kv, kv_new, kvl = mla_case(dt, sq, h, gen, cap=cap)
        qg, kng = q.to(gpu), kv_new.to(gpu)
        for causal in (False, True):
            for ns in SPLITS:
                kvg = kv.to(gpu)
                pool, table, spare = page_kv(kv.to(gpu), P, 7 + P)
                kw = dict(kv_new=kng, causal=causal, num_splits=ns, return_softmax_lse=True)
                oc, lc = F.flash_mla_with_kvcache(qg, kvg, cs, **kw)
                op, lp = F.flash_mla_with_kvcache(qg, pool, cs, block_table=table, **kw)
                tag = f"P{P} h{h} sq{sq} causal={causal} splits={ns}"
                assert _same(op, oc) and _same(lp, lc), tag
                assert _same(logical_of(pool, table, cap).cpu(), kvl) and _same(kvg.cpu(), kvl), tag
                assert torch.isnan(pool[spare].float()).all().item(), f"{tag}: a page no sequence references was written"
                o2, l2 = F.flash_mla_with_kvcache(qg, pool, cs, block_table=table, **kw)        # (the append rewrites the same rows)
                assert _same(o2, op) and _same(l2, lp), f"{tag}: two runs differ"


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_default_scale_and_a_power_of_two_between_scale_and_q(gpu, dtname):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(63500)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    q, kv, kv_new, _ = mla_case(dt, 2, 16, gen)
    qg, kng = q.to(gpu), kv_new.to(gpu)
    own = 192 ** -0.5 * 1.3
    for ns in SPLITS:
        kw = dict(kv_new=kng, causal=True, num_splits=ns, return_softmax_lse=True)
        a = F.flash_mla_with_kvcache(qg, kv.to(gpu), cs, **kw)
        b_ = F.flash_mla_with_kvcache(qg, kv.to(gpu), cs, softmax_scale=SCALE, **kw)
        assert _same(a[0], b_[0]) and _same(a[1], b_[1]), "softmax_scale=None is not the fp32 default"
        c = F.flash_mla_with_kvcache(qg, kv.to(gpu), cs, softmax_scale=own, **kw)
        d = F.flash_mla_with_kvcache(qg * 4, kv.to(gpu), cs, softmax_scale=own / 4, **kw)
        e = F.flash_mla_with_kvcache(qg * 0.5, kv.to(gpu), cs, softmax_scale=own * 2, **kw)
        assert _same(c[0], d[0]) and _same(c[1], d[1]) and _same(c[0], e[0]) and _same(c[1], e[1]), f"splits={ns}"
        assert not _same(a[1], c[1])
        if ns == 1:
            s = scores64(q, mla_logical(kv, kv_new), own)
            xo, xl, nvis = exact(s, mla_logical(kv, kv_new)[..., :DV], visible([p + 2 for p in PREFIXES], 2, CAP, True))
            check(c[0], c[1], xo, xl, nvis, dtname, f"mla {dtname} softmax_scale={own:.4f}")


def mla_logical(kv, kv_new, prefixes=PREFIXES):
    kvl = kv.clone()
    for i, pre in enumerate(prefixes):
        kvl[i, pre:pre + kv_new.shape[1]] = kv_new[i]
    return kvl


# ---- 4. visibility as integers -------------------------------------------------------------------------------------------------------------

def _mla_probe(c, dev):
    """The probe of tests/_visibility.py on this call: q = 0 makes every score exactly 0 whatever the latent row holds, and columns 0 .. 511 of
    the row - the value - carry the key's code at d = 512 (base 64, 4096 keys).  Memory a sequence does not own - rows at or past its length
    before the append, spare pages - holds the all-ones code, in the rope columns too."""
    V.check_conditions(c)
    assert c.d == DV and c.hk == 1 and not c.fp8 and not c.ragged and c.tree is None and c.window == (-1, -1)
    dt = V.torch_dtype(c.dtype)
    gen = torch.Generator(device="cpu").manual_seed(len(c.name) * 7919 + sum(c.lens))
    b, sq = len(c.lens), c.sq[0]
    _, v, table = V.build_cache(c, dev, gen)
    kv = torch.cat([v, torch.ones(*v.shape[:-1], DK - DV, dtype=v.dtype, device=dev)], dim=-1)
    q = torch.zeros(b, sq, c.h, DK, dtype=dt, device=dev)
    kw = dict(causal=c.causal, num_splits=c.splits, return_softmax_lse=True, block_table=table)
    if c.append:
        pos = torch.tensor([L - sq + t for L in c.lens for t in range(sq)], dtype=torch.long, device=dev)
        new = torch.cat([V.code_tensor(DV, c.cap, dev)[pos].to(dt), torch.ones(b * sq, DK - DV, dtype=dt, device=dev)], dim=-1)
        kw.update(kv_new=new.view(b, sq, 1, DK))
    cs = torch.tensor([L - sq if c.append else L for L in c.lens], dtype=torch.int32, device=dev)
    out, lse = F.flash_mla_with_kvcache(q, kv, cs, **kw)
    n_dec, hist_dec = V.decode(out.reshape(b * sq, c.h, DV), lse.permute(0, 2, 1).reshape(b * sq, c.h), torch.zeros(c.h, dtype=torch.long))
    V.assert_signature(c, n_dec, hist_dec, *V.expected(c))


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("page", [0, 16, 48])
def test_visible_key_sets_as_integers(gpu, dtname, page):
    """the exact set of keys per (sequence, head, row): length, causal, L_i after an append, over both layouts and every split count"""
    lens = (0, 1, 5, 31, 32, 33, 63, 64, 65, 100, 777, 1008)
    n = 0
    for h, sq in ((1, 1), (16, 1), (24, 5), (128, 2), (13, 5)):
        for causal in (False, True):
            for append in (False, True):
                for splits in (0, 1, 3):
                    ls = tuple(max(L, sq) for L in lens) if append else lens
                    c = V.Case("mla", f"mla h{h} sq{sq} causal={causal} append={append} splits={splits} page={page}", ls, (sq,) * len(ls), d=DV, dtype=dtname,
                               page=page, h=h, hk=1, append=append, causal=causal, splits=splits, cap=CAP)
                    _mla_probe(c, gpu)
                    n += 1
    assert n == 60


# ---- 5. edges --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_nan_rules(gpu, dtname):
    """a NaN in one query row makes that row NaN and leaves the other rows' bits alone; a NaN (or an inf whose score is +inf) in a visible key row
    makes the rows that see it NaN, and only those"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(65000)
    lens = [33, 100, 777]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    h, sq = 24, 2
    q, kv, _, _ = mla_case(dt, sq, h, gen, prefixes=lens)
    qg, kvg = q.to(gpu), kv.to(gpu)
    for ns in SPLITS:
        kw = dict(causal=True, num_splits=ns, return_softmax_lse=True)
        o0, l0 = F.flash_mla_with_kvcache(qg, kvg, cs, **kw)
        assert torch.isfinite(o0.float()).all().item()
        qn = qg.clone()
        qn[1, 1, 7, 530] = NAN                       # (a rope column)
        qn[2, 0, 23, 3] = NAN
        o1, l1 = F.flash_mla_with_kvcache(qn, kvg, cs, **kw)
        hit = torch.zeros(len(lens), sq, h, dtype=torch.bool, device=gpu)
        hit[1, 1, 7] = hit[2, 0, 23] = True
        assert torch.isnan(o1[hit].float()).all().item() and torch.isnan(l1.permute(0, 2, 1)[hit]).all().item(), f"splits={ns}"
        assert _same(o1[~hit], o0[~hit]) and _same(l1.permute(0, 2, 1)[~hit], l0.permute(0, 2, 1)[~hit]), f"splits={ns}: a NaN query row touched another row"
        # a key every row of its sequence sees (non-causal): that sequence is NaN, the others keep their bits
        kw = dict(causal=False, num_splits=ns, return_softmax_lse=True)
        o0, l0 = F.flash_mla_with_kvcache(qg, kvg, cs, **kw)
        for col in (5, 570):
            kn = kvg.clone()
            kn[1, 64, 0, col] = NAN
            o2, l2 = F.flash_mla_with_kvcache(qg, kn, cs, **kw)
            assert torch.isnan(o2[1].float()).all().item() and torch.isnan(l2[1]).all().item(), f"splits={ns} col={col}"
            assert _same(o2[[0, 2]], o0[[0, 2]]) and _same(l2[[0, 2]], l0[[0, 2]]), f"splits={ns} col={col}"
        # causal, the NaN in a rope column (no part of the value) of the last key: the last row sees it, the row in front does not
        kn = kvg.clone()
        kn[2, lens[2] - 1, 0, 540] = NAN
        kw = dict(causal=True, num_splits=ns, return_softmax_lse=True)
        o0, l0 = F.flash_mla_with_kvcache(qg, kvg, cs, **kw)
        o3, l3 = F.flash_mla_with_kvcache(qg, kn, cs, **kw)
        assert torch.isnan(o3[2, 1].float()).all().item() and torch.isnan(l3[2, :, 1]).all().item(), f"splits={ns}"
        assert _same(o3[2, 0], o0[2, 0]) and _same(l3[2, :, 0], l0[2, :, 0]) and _same(o3[:2], o0[:2]) and _same(l3[:2], l0[:2]), f"splits={ns}"


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [0, 16, 48])
def test_what_is_never_read(gpu, dtname, P):
    """cache rows at or past L_i, pages no sequence references and table entries past the needed pages may hold NaN / garbage; a needed entry
    outside the pool is clamped to the last page"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(65500 + P)
    lens = [0, 1, 31, 33, 100, 777]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    h, sq = 24, 2
    q, kv, _, _ = mla_case(dt, sq, h, gen, prefixes=lens)
    s = scores64(q, kv, SCALE)
    xo, xl, nvis = exact(s, kv[..., :DV], visible(lens, sq, CAP, True))
    dirty = kv.clone()
    for i, L in enumerate(lens):
        U.poison_(dirty[i, L:])
    qg = q.to(gpu)
    for ns in SPLITS:
        kw = dict(causal=True, num_splits=ns, return_softmax_lse=True)
        tag = f"never read {dtname} P{P} splits={ns}"
        if P == 0:
            out, lse = F.flash_mla_with_kvcache(qg, dirty.to(gpu), cs, **kw)
            check(out, lse, xo, xl, nvis, dtname, tag)
            continue
        pool, table, spare = page_kv(dirty.to(gpu), P, 11 + P)
        clean = F.flash_mla_with_kvcache(qg, pool, cs, block_table=table, **kw)
        check(clean[0], clean[1], xo, xl, nvis, dtname, tag)
        bad = table.clone()
        junk = torch.tensor([-1, 2 ** 31 - 1, -2 ** 31, 12345678], dtype=torch.int32, device=gpu)
        for i, L in enumerate(lens):
            need = (L + P - 1) // P
            bad[i, need:] = junk[torch.arange(table.shape[1] - need, device=gpu) % 4]
        out, lse = F.flash_mla_with_kvcache(qg, pool, cs, block_table=bad, **kw)
        assert _same(out, clean[0]) and _same(lse, clean[1]), f"{tag}: a table entry past the needed pages reached a result"
        # a needed entry outside the pool reads page num_blocks - 1: a copy of the last sequence's first page goes there and its entry is broken
        nb = pool.shape[0] + 1
        moved, t2 = torch.cat([pool, pool[table[5, 0].long()].unsqueeze(0)]), table.clone()
        for entry in (nb, -1, 2 ** 31 - 1):
            t2[5, 0] = entry
            out, lse = F.flash_mla_with_kvcache(qg, moved, cs, block_table=t2, **kw)
            assert _same(out[5], clean[0][5]) and _same(lse[5], clean[1][5]), f"{tag}: entry {entry} was not clamped to the last page"


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_strided_views_with_guard_bands_and_an_int_length(gpu, dtname):
    """q, the cache and kv_new as views into guarded buffers through the Python call; q and out as guarded views through the C ABI (the extension
    allocates out itself): nothing outside a view's extent is written, and cache_seqlens may be an int"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(66000)
    b, h, sq, L = 3, 24, 2, 100
    q, kv, kv_new, _ = mla_case(dt, sq, h, gen, prefixes=[L] * b)
    cs = torch.full((b,), L, dtype=torch.int32, device=gpu)
    kvg = kv.to(gpu)
    want = F.flash_mla_with_kvcache(q.to(gpu), kvg, cs, kv_new=kv_new.to(gpu), causal=True, return_softmax_lse=True)
    qb, qv, _ = U.guarded((b, sq, h, DK), dt, gpu, (2, 2, 2, 16))
    cb, cv, csl = U.guarded((b, CAP, 1, DK), dt, gpu, (2, 4, 0, 16))
    nb_, nv, _ = U.guarded((b, sq, 1, DK), dt, gpu, (2, 2, 0, 16))
    qv.copy_(q.to(gpu)); cv.copy_(kv.to(gpu)); nv.copy_(kv_new.to(gpu))
    keep_q, keep_n = qb.clone(), nb_.clone()
    got = F.flash_mla_with_kvcache(qv, cv, L, kv_new=nv, causal=True, return_softmax_lse=True)
    assert _same(got[0], want[0]) and _same(got[1], want[1])
    assert _same(cv.contiguous(), kvg) and _same(qb, keep_q) and _same(nb_, keep_n)
    mask = torch.ones(cb.shape, dtype=torch.bool, device=gpu)
    mask[csl] = False
    assert (U.bits(cb)[mask] == U.SENT16).all().item(), "the append wrote outside the cache view"
    # the C ABI with strided q / o
    ob, ov, osl = U.guarded((b, sq, h, DV), dt, gpu, (2, 2, 2, 16))
    lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=gpu)
    for ns in (1, 3):
        kv2 = kv.to(gpu)
        p = capi.mla_params(qv, kv2, ov, lse, cs, kv_new=nv, causal=True, num_splits=ns)
        ws = torch.full((max(capi.mla_workspace_bytes(p), 16) // 4 + 64,), NAN, device=gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), (ws.numel() - 64) * 4
        capi.run_mla_fwd_kvcache(p)
        torch.cuda.synchronize()
        ref = F.flash_mla_with_kvcache(q.to(gpu), kv.to(gpu), cs, kv_new=kv_new.to(gpu), causal=True, num_splits=ns, return_softmax_lse=True)
        assert _same(ov.contiguous(), ref[0]) and _same(lse, ref[1]), f"splits={ns}"
        omask = torch.ones(ob.shape, dtype=torch.bool, device=gpu)
        omask[osl] = False
        assert (U.bits(ob)[omask] == U.SENT16).all().item(), "out was written outside its view"
        assert torch.isnan(ws[-64:]).all().item(), "the workspace was written past the bytes the library asked for"


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------

def test_captured_call_replays_with_new_lengths_and_a_new_table(gpu):
    dt, h, sq, b, P, cap = torch.bfloat16, 128, 1, 2, 64, 4096
    gen = torch.Generator().manual_seed(67000)
    kv = _rand((b, cap, 1, DK), dt, gen).to(gpu)
    q = _rand((b, sq, h, DK), dt, gen).to(gpu)
    kv_new = _rand((b, sq, 1, DK), dt, gen, 3.0).to(gpu)
    pool, table, _ = page_kv(kv, P, 5, fill=0.0)
    cs = torch.tensor([100, 4000], dtype=torch.int32, device=gpu)
    kw = dict(kv_new=kv_new, block_table=table, causal=True, return_softmax_lse=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_mla_with_kvcache(q, pool, cs, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_mla_with_kvcache(q, pool, cs, **kw)
    first = (out_g.clone(), lse_g.clone())
    lens = [2500, 5]
    cs.copy_(torch.tensor(lens, dtype=torch.int32))
    table.copy_(table.flip(0))                       # the sequences swap their pages
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = F.flash_mla_with_kvcache(q, pool, cs, **kw)
    assert _same(out_g, out_e) and _same(lse_g, lse_e)
    assert not _same(out_g, first[0])
    kvl = logical_of(pool, table, cap).cpu()
    xo, xl, nvis = exact(scores64(q, kvl, SCALE), kvl[..., :DV], visible([L + sq for L in lens], sq, cap, True))
    check(out_g, lse_g, xo, xl, nvis, "bf16", "mla graph replay")


# ---- 7. the C ABI ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_c_abi_with_a_caller_workspace_and_a_forced_split_is_the_python_call(gpu, dtname):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(68000)
    h, sq = 24, 5
    q, kv, kv_new, kvl = mla_case(dt, sq, h, gen)
    b = len(PREFIXES)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    qg, kng = q.to(gpu), kv_new.to(gpu)
    pool, table, _ = page_kv(kv.to(gpu), 48, 21)
    for paged in (False, True):
        kvg = pool.clone() if paged else kv.to(gpu)
        want = F.flash_mla_with_kvcache(qg, kvg.clone(), cs, kv_new=kng, causal=True, num_splits=3, return_softmax_lse=True, softmax_scale=0.07,
                                        block_table=table if paged else None)
        out = torch.full((b, sq, h, DV), NAN, dtype=dt, device=gpu)
        lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=gpu)
        p = capi.mla_params(qg, kvg, out, lse, cs, kv_new=kng, causal=True, num_splits=3, block_table=table if paged else None, softmax_scale=0.07)
        rows = b * h * sq
        assert capi.mla_workspace_bytes(p) == 3 * rows * DV * 4 + (3 * rows * 4 + 15) // 16 * 16
        assert capi.mla_num_splits(p) == 1                     # no workspace yet
        ws = torch.full((capi.mla_workspace_bytes(p) // 4 + 64,), NAN, device=gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), capi.mla_workspace_bytes(p)
        assert capi.mla_num_splits(p) == 3
        capi.run_mla_fwd_kvcache(p)
        torch.cuda.synchronize()
        assert _same(out, want[0]) and _same(lse, want[1]), f"paged={paged}"
        assert torch.isnan(ws[-64:]).all().item()
        got = logical_of(kvg, table, CAP) if paged else kvg
        assert _same(got.cpu(), kvl)
        # a workspace too small for three splits caps the split; the result is that of the capped count
        p.workspace_bytes = 2 * rows * DV * 4 + (2 * rows * 4 + 15) // 16 * 16
        assert capi.mla_num_splits(p) == 2
        capi.run_mla_fwd_kvcache(p)
        two = F.flash_mla_with_kvcache(qg, kvg, cs, kv_new=kng, causal=True, num_splits=2, return_softmax_lse=True, softmax_scale=0.07,
                                       block_table=table if paged else None)
        assert _same(out, two[0]) and _same(lse, two[1])
