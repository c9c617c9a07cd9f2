"""GPU: sparse MLA decode over a latent KV cache (flash_mla_sparse_with_kvcache, fa_run_mla_sparse_fwd_kvcache).

Values are compared with fp64 math over the valid multiset of every (sequence, token) - scores64 / exact / check of the tree suite, fed the cache rows
GATHERED by the token's list (one "sequence" per token, one key per slot, the slot's validity as the visibility), so a position listed twice counts
twice - through _util.TOL and _util.LSE_TOL: the tolerances of the decode path, no new number.  Shapes sit on the kernel's boundaries (64 heads a
workgroup, 16 a wave, 32 slots a step), not at the workload's sizes.  Everything else is a relation that must hold to the bit, the integer visibility
probe of tests/_visibility.py, what is never read, the NaN rules, guard bands, the C ABI and graph capture."""
import math

import numpy as np
import pytest
import torch

import _util as U
import _visibility as V
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_softcap_gpu import DT, _rand, _same
from test_kvcache_tree_gpu import check, exact, scores64
from test_kvcache_window_gpu import _page

pytestmark = pytest.mark.gpu

NAN = float("nan")
DK, DV = 576, 512
CAP = 1008                              # 63 pages of 16 = 21 of 48
HS = [1, 16, 24, 128]                   # one lane; one wave; a partly filled second wave; two tiles
SQS = [1, 3]
TOPKS = [32, 96, 256]                   # one step; three steps (three one-step splits); eight steps
LENS = [0, 1, 31, 33, 100, 777]
PAGES = [16, 48]
SPLITS = [0, 1, 3]
I_MIN, I_MAX = -2 ** 31, 2 ** 31 - 1
SCALE = float(np.float32(1.0) / np.sqrt(np.float32(DK)))        # the default: 576 ** -0.5 rounded once to fp32


# ---- lists, the fp64 expectation, pages ---------------------------------------------------------------------------------------------------------

def valid_of(idx, lens):
    """bool (b, sq, topk): slot s of row (i, t) is valid iff 0 <= idx < L_i"""
    L = torch.tensor(lens, dtype=torch.int64).view(-1, 1, 1)
    return (idx.long() >= 0) & (idx.long() < L)


def invalid_entries(n, L, cap, gen):
    """n invalid entries of every kind: -1, values in [L, cap), INT_MIN, INT_MAX"""
    kind = torch.randint(0, 4, (n,), generator=gen)
    past = torch.randint(L, cap, (n,), generator=gen) if L < cap else torch.full((n,), cap)
    return torch.where(kind == 0, torch.full((n,), -1), torch.where(kind == 1, past, torch.where(kind == 2, torch.full((n,), I_MIN), torch.full((n,), I_MAX))))


def random_lists(lens, sq, topk, gen, cap=CAP, dead_steps=True, fill=0.6):
    """int32 (b, sq, topk): per token, distinct valid positions in random order with invalid entries of every kind interleaved; with dead_steps (three
    steps or more) the 32 slots of the first step and of a middle step are all invalid"""
    idx = torch.empty(len(lens), sq, topk, dtype=torch.int64)
    steps = topk // 32
    dead = [0, steps // 2] if dead_steps and steps >= 3 else []
    free = torch.tensor([s for s in range(topk) if s // 32 not in dead])
    for i, L in enumerate(lens):
        for t in range(sq):
            row = invalid_entries(topk, L, cap, gen)
            nv = min(L, max(1, int(fill * len(free))))
            slots = free[torch.randperm(len(free), generator=gen)[:nv]]
            row[slots] = torch.randperm(L, generator=gen)[:nv]
            idx[i, t] = row
    return idx.to(torch.int32)


def expect(q, kvl, idx, lens, scale=SCALE):
    """fp64 over the valid multiset: every (sequence, token) is one sequence of `exact`, its keys the rows its list names (an invalid slot gathers row 0
    and is not visible).  -> O (b, sq, h, 512), LSE (b, h, sq), valid slots per row (b, sq)"""
    b, sq, h, _ = q.shape
    topk = idx.shape[-1]
    ok = valid_of(idx, lens)
    pos = torch.where(ok, idx.long(), torch.zeros_like(idx, dtype=torch.int64))
    rows = kvl.cpu()[torch.arange(b).view(b, 1, 1), pos, 0]                    # (b, sq, topk, 576)
    g = rows.reshape(b * sq, topk, 1, DK)
    s = scores64(q.cpu().reshape(b * sq, 1, h, DK), g, scale)
    xo, xl, nvis = exact(s, g[..., :DV], ok.reshape(b * sq, 1, topk))
    return xo.reshape(b, sq, h, DV), xl.reshape(b, sq, h).permute(0, 2, 1), nvis.reshape(b, sq)


def case(dt, sq, h, gen, lens=LENS, cap=CAP):
    return _rand((len(lens), sq, h, DK), dt, gen), _rand((len(lens), cap, 1, DK), dt, gen)


def page_kv(logical, P, seed, fill=NAN):
    """pool + table of the logical latent cache under a random page permutation; spare pages hold `fill`"""
    pool, _, table, spare = _page(logical, logical, P, seed, fill=fill)
    return pool, table, spare


def sparse(q, kv, cs, idx, **kw):
    return F.flash_mla_sparse_with_kvcache(q, kv, cs, idx, return_softmax_lse=True, **kw)


def same2(a, b):
    return _same(a[0], b[0]) and _same(a[1], b[1])


# ---- 1. values -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("h", HS)
def test_sparse_against_fp64(gpu, dtname, h):
    """random distinct valid positions in random order, invalid entries of every kind interleaved, all-invalid steps at the front and in the middle
    of a list, different lists per token; both layouts, every split count.  At sq = 3 the case must tell tokens apart: the fp64 expectation of a token
    under its own list and under its neighbour's lie at least 4 x the mean_abs tolerance apart."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(71000 + h)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    tol = U.TOL[dtname]["mean_abs"]
    for sq in SQS:
        q, kv = case(dt, sq, h, gen)
        qg, kvg = q.to(gpu), kv.to(gpu)
        pools = {P: page_kv(kvg, P, 3 + P) for P in PAGES}
        for topk in TOPKS:
            idx = random_lists(LENS, sq, topk, gen)
            ok = valid_of(idx, LENS)
            assert (~ok).any().item() and all((idx == v).any().item() for v in (-1, I_MIN, I_MAX)) and ((idx >= 777) & (idx < CAP)).any().item()
            if topk >= 96:
                assert not ok[:, :, :32].any().item() and not ok[:, :, 32 * (topk // 64):32 * (topk // 64) + 32].any().item()
            xo, xl, nvis = expect(q, kv, idx, LENS)
            if sq == 3:
                other = expect(q, kv, idx.roll(1, dims=1), LENS)[0]
                gap = float((xo - other).abs().mean())
                print(f"{dtname} h{h} sq{sq} topk{topk}: own list from the neighbour's: mean gap of the expectations {gap:.3e} ({gap / tol:.1f} x mean_abs tol)")
                assert gap >= 4 * tol, f"topk{topk}: the case does not tell tokens apart (gap {gap:.3e})"
            ig = idx.to(gpu)
            for ns in SPLITS:
                out, lse = sparse(qg, kvg, cs, ig, num_splits=ns)
                assert out.shape == (len(LENS), sq, h, DV) and out.dtype == dt and lse.shape == (len(LENS), h, sq) and lse.dtype == torch.float32
                check(out, lse, xo, xl, nvis, dtname, f"sparse {dtname} h{h} sq{sq} topk{topk} splits={ns}")
                for P, (pool, table, _) in pools.items():
                    op, lp = sparse(qg, pool, cs, ig, num_splits=ns, block_table=table)
                    check(op, lp, xo, xl, nvis, dtname, f"sparse {dtname} h{h} sq{sq} topk{topk} splits={ns} P{P}")


# ---- 2. duplicates ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_a_position_listed_twice_counts_twice(gpu, dtname):
    """each chosen key twice: the fp64 result over the multiset (doubled weights), and an LSE log 2 above the de-duplicated list's"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(72000)
    h, sq, topk = 24, 3, 96
    lens = [1, 31, 33, 100, 777]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    q, kv = case(dt, sq, h, gen, lens=lens)
    once = random_lists(lens, sq, topk // 2, gen, dead_steps=False, fill=0.8)
    pad = torch.full_like(once, -1)
    twice = torch.cat([once, once.flip(-1)], dim=-1)
    xo1, xl1, n1 = expect(q, kv, torch.cat([once, pad], dim=-1), lens)
    xo2, xl2, n2 = expect(q, kv, twice, lens)
    assert torch.equal(n2, 2 * n1) and float((xl2 - (xl1 + math.log(2.0))).abs().max()) < 1e-12 and float((xo2 - xo1).abs().max()) < 1e-12
    for ns in SPLITS:
        out, lse = sparse(q.to(gpu), kv.to(gpu), cs, twice.to(gpu), num_splits=ns)
        check(out, lse, xo2, xl2, n2, dtname, f"duplicates {dtname} splits={ns}")
        err = float((lse.double().cpu() - (xl1 + math.log(2.0))).abs().max())
        assert err <= U.LSE_TOL, f"splits={ns}: LSE is not log 2 above the de-duplicated list's ({err:.3e})"


# ---- 3. dead rows ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [0, 16])
def test_dead_rows_are_exactly_zero(gpu, dtname, P):
    """L = 0, an all-invalid list, a list of entries >= L_i only: O = 0 and LSE = 0 exactly; the cache is NaN wherever nothing may be read"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(73000)
    lens = [0, 100, 100, 777]
    h, sq, topk = 24, 3, 96
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    q, kv = case(dt, sq, h, gen, lens=lens)
    idx = random_lists(lens, sq, topk, gen)
    idx[0] = torch.randint(-5, CAP, (sq, topk), generator=gen).to(torch.int32)          # L = 0: nothing is valid
    idx[1] = invalid_entries(sq * topk, 100, CAP, gen).view(sq, topk).to(torch.int32)   # every kind of invalid entry
    idx[2] = torch.randint(100, CAP, (sq, topk), generator=gen).to(torch.int32)         # entries >= L_i only
    idx[3, 1] = I_MIN                                                                   # one dead token between two live ones
    kv[0], kv[1], kv[2] = NAN, NAN, NAN
    xo, xl, nvis = expect(q, torch.nan_to_num(kv.float()).to(dt), idx, lens)
    assert int((nvis == 0).sum()) == 3 * sq + 1
    kvg, table = kv.to(gpu), None
    if P:
        kvg, table, _ = page_kv(kvg, P, 9)
    for ns in SPLITS:
        out, lse = sparse(q.to(gpu), kvg, cs, idx.to(gpu), num_splits=ns, block_table=table)
        assert (out[:3] == 0).all().item() and (lse[:3] == 0).all().item() and (out[3, 1] == 0).all().item() and (lse[3, :, 1] == 0).all().item(), f"splits={ns}"
        check(out, lse, xo, xl, nvis, dtname, f"dead rows {dtname} P{P} splits={ns}")


# ---- 4. a single valid slot ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_single_valid_slot_returns_its_row_bit_for_bit(gpu, dtname):
    """one valid entry at slot 37 of 96, everything else -1: the softmax weight is exactly 1 and out is that row's first 512 columns"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(74000)
    lens = [1, 33, 100, 777]
    pos = [0, 32, 7, 776]
    h, sq, topk = 24, 3, 96
    q, kv = case(dt, sq, h, gen, lens=lens)
    idx = torch.full((len(lens), sq, topk), -1, dtype=torch.int32)
    for i, j in enumerate(pos):
        idx[i, :, 37] = j
    qg, kvg = q.to(gpu), kv.to(gpu)
    want = kvg[torch.arange(len(lens)), pos, 0, :DV].view(len(lens), 1, 1, DV).expand(len(lens), sq, h, DV).contiguous()
    xl = expect(q, kv, idx, lens)[1]
    pool, table, _ = page_kv(kvg, 48, 4)
    for ns in SPLITS + [2]:
        for kvx, tb in ((kvg, None), (pool, table)):
            out, lse = sparse(qg, kvx, torch.tensor(lens, dtype=torch.int32, device=gpu), idx.to(gpu), num_splits=ns, block_table=tb)
            assert _same(out, want), f"splits={ns} paged={tb is not None}"
            assert float((lse.double().cpu() - xl).abs().max()) <= U.LSE_TOL


# ---- 5. relations that hold to the bit -----------------------------------------------------------------------------------------------------

def prefix_lists(ns, sq, topk, causal=False):
    """(b, sq, topk): 0, 1, .., n - 1 then -1; causal: cut at n - sq + t + 1 for token t"""
    idx = torch.full((len(ns), sq, topk), -1, dtype=torch.int32)
    for i, n in enumerate(ns):
        for t in range(sq):
            m = max(0, min(n, n - sq + t + 1)) if causal else n
            idx[i, t, :m] = torch.arange(m, dtype=torch.int32)
    return idx


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("h", [24, 128])
def test_identity_and_causal_prefix_lists_are_the_dense_call(gpu, dtname, h):
    """the list 0 .. n - 1 followed by -1 == flash_mla_with_kvcache at cache_seqlens = n (num_splits = 1 at every topk; a forced 3 with topk == capacity
    == 96), and the same list cut at n - seqlen_q + t + 1 per token == its causal call: out and lse, bit for bit"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(75000 + h)
    sq = 3
    for topk, cap, splits in ((32, CAP, (1,)), (96, CAP, (1,)), (256, CAP, (1,)), (96, 96, (1, 3))):
        ns = [min(L, topk) for L in LENS]
        q, kv = case(dt, sq, h, gen, cap=cap)
        qg, kvg = q.to(gpu), kv.to(gpu)
        cn = torch.tensor(ns, dtype=torch.int32, device=gpu)
        cl = torch.tensor([min(L, cap) for L in LENS], dtype=torch.int32, device=gpu)
        for causal in (False, True):
            ig = prefix_lists(ns, sq, topk, causal).to(gpu)
            for n_split in splits:
                dense = F.flash_mla_with_kvcache(qg, kvg, cn, causal=causal, num_splits=n_split, return_softmax_lse=True)
                tag = f"{dtname} h{h} topk{topk} cap{cap} causal={causal} splits={n_split}"
                assert same2(sparse(qg, kvg, cn, ig, num_splits=n_split), dense), tag
                assert same2(sparse(qg, kvg, cl, ig, num_splits=n_split), dense), f"{tag}: a longer sequence under the same list"


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", PAGES)
def test_paged_is_contiguous_runs_are_identical_and_the_default_scale(gpu, dtname, P):
    """shuffled tables, spare pages full of NaN: out and lse for every split count; two runs; softmax_scale=None == the fp32 default passed"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(76000 + P)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    for h, sq, topk in ((24, 3, 96), (128, 1, 256)):
        q, kv = case(dt, sq, h, gen)
        qg, kvg = q.to(gpu), kv.to(gpu)
        ig = random_lists(LENS, sq, topk, gen).to(gpu)
        pool, table, spare = page_kv(kvg, P, 7 + P)
        assert torch.isnan(pool[spare].float()).all().item()
        for ns in SPLITS:
            tag = f"P{P} h{h} sq{sq} topk{topk} splits={ns}"
            c = sparse(qg, kvg, cs, ig, num_splits=ns)
            p = sparse(qg, pool, cs, ig, num_splits=ns, block_table=table)
            assert torch.isfinite(c[0].float()).all().item() and same2(p, c), tag
            assert same2(sparse(qg, pool, cs, ig, num_splits=ns, block_table=table), p) and same2(sparse(qg, kvg, cs, ig, num_splits=ns), c), f"{tag}: two runs differ"
            assert same2(sparse(qg, kvg, cs, ig, num_splits=ns, softmax_scale=SCALE), c), f"{tag}: softmax_scale=None is not the fp32 default"
            assert not _same(sparse(qg, kvg, cs, ig, num_splits=ns, softmax_scale=192 ** -0.5)[1], c[1])


# ---- 6. visibility as integers -------------------------------------------------------------------------------------------------------------

def probe_lists(kind, lens, sq, topk, gen):
    """lists of distinct keys, padded with -1: sorted, reversed, strided by 7, random"""
    idx = torch.full((len(lens), sq, topk), -1, dtype=torch.int64)
    for i, L in enumerate(lens):
        for t in range(sq):
            if kind == "stride7":
                pos = torch.arange(t % 7, max(L, t % 7), 7)[:topk]
            else:
                pos = torch.randperm(L, generator=gen)[:min(L, topk - 8 * t)]
                if kind == "sorted":
                    pos = pos.sort().values
                elif kind == "reversed":
                    pos = pos.sort(descending=True).values
            idx[i, t, :len(pos)] = pos
    return idx.to(torch.int32)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("page", [0, 16, 48])
def test_selected_key_sets_as_integers(gpu, dtname, page):
    """The probe of tests/_visibility.py: q = 0 makes every score exactly 0, columns 0 .. 511 of cache row j carry the code of key j (base 64, 4096
    keys), the rope columns 1.  Memory no list of the sequence names - unselected rows below L_i, rows at or past L_i, spare pages - holds the
    all-ones code.  Count and digit histogram of every (sequence, token, head) against codes[valid idx].sum(0), computed in numpy from the lists."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(77000 + page)
    lens = (0, 1, 5, 31, 32, 33, 63, 64, 65, 100, 777, 1008)
    assert CAP <= V.capacity_of(DV) and CAP <= V.MAX_N
    codes = V.codes(DV, CAP)
    good = V.code_tensor(DV, CAP, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    n_cases = 0
    for (h, sq, topk), kind in zip(((1, 1, 32), (16, 3, 96), (24, 3, 256), (128, 1, 256)), ("random", "reversed", "stride7", "sorted")):
        idx = probe_lists(kind, lens, sq, topk, gen)
        ok_t = valid_of(idx, lens)
        ok = ok_t.numpy()
        assert all(len(set(idx[i, t][ok_t[i, t]].tolist())) == int(ok[i, t].sum()) for i in range(len(lens)) for t in range(sq)), "the probe needs distinct keys"
        n_exp = ok.sum(-1).reshape(-1)
        hist_exp = np.stack([codes[idx[i, t].numpy()[ok[i, t]]].sum(0) for i in range(len(lens)) for t in range(sq)])
        assert n_exp.max() <= V.MAX_N and hist_exp.max() <= V.MAX_DIGIT and n_exp.max() == (144 if kind == "stride7" else topk)
        named = torch.zeros(len(lens), CAP, dtype=torch.bool)
        for i in range(len(lens)):
            named[i, idx[i][ok_t[i]].long()] = True
        v = torch.where(named.to(gpu).unsqueeze(-1), good.unsqueeze(0), torch.full((), V.BAD, dtype=torch.uint8, device=gpu)).to(dt)
        kv = torch.cat([v, torch.ones(len(lens), CAP, DK - DV, dtype=dt, device=gpu)], dim=-1).unsqueeze(2)
        table = None
        if page:
            kv, table, _ = page_kv(kv, page, 13 + page, fill=float(V.BAD))
        q = torch.zeros(len(lens), sq, h, DK, dtype=dt, device=gpu)
        wide = torch.full((len(lens) + 1, sq + 2, topk + 32), 5, dtype=torch.int32, device=gpu)     # (5: a valid position for most sequences)
        view = wide[1:, 1:1 + sq, 32:]
        view.copy_(idx)
        assert not view.is_contiguous() and view.stride(2) == 1
        for splits in SPLITS:
            for ix in (idx.to(gpu), view):
                out, lse = sparse(q, kv, cs, ix, num_splits=splits, block_table=table)
                n_dec, hist_dec = V.decode(out.reshape(-1, h, DV), lse.permute(0, 2, 1).reshape(-1, h), torch.zeros(h, dtype=torch.long))
                tag = f"{kind} h{h} sq{sq} topk{topk} page={page} splits={splits} strided={ix is view}"
                assert torch.equal(n_dec.cpu(), torch.from_numpy(n_exp).view(-1, 1).expand(-1, h)), f"{tag}: counts differ"
                bad = (hist_dec.cpu() != torch.from_numpy(hist_exp).unsqueeze(1)).any(-1)
                assert not bad.any().item(), f"{tag}: {int(bad.sum())} (row, head) digit histograms differ, first (row, head) {bad.nonzero()[0].tolist()}"
                n_cases += 1
    assert n_cases == 24


# ---- 7. what is never read -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [0, 16, 48])
def test_what_is_never_read(gpu, dtname, P):
    """every cache row no valid slot names is poisoned (NaN, +-inf, 65504), pages no valid slot reaches are NaN, their table entries junk: the bits of
    the clean run.  A needed table entry outside the pool reads the last page."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(78000 + P)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    h, sq, topk = 24, 3, 96
    q, kv = case(dt, sq, h, gen)
    idx = random_lists(LENS, sq, topk, gen, fill=0.3)
    ok = valid_of(idx, LENS)
    named = torch.zeros(len(LENS), CAP, dtype=torch.bool)
    for i in range(len(LENS)):
        named[i, idx[i][ok[i]].long()] = True
    dirty = kv.clone()
    dirty[~named] = U.poison_(dirty[~named])
    assert int(named.sum()) < 0.2 * named.numel() and named[5, :777].any().item() and not named[5, :777].all().item()
    qg, ig = q.to(gpu), idx.to(gpu)
    xo, xl, nvis = expect(q, kv, idx, LENS)
    for ns in SPLITS:
        tag = f"never read {dtname} P{P} splits={ns}"
        if P == 0:
            clean = sparse(qg, kv.to(gpu), cs, ig, num_splits=ns)
            check(clean[0], clean[1], xo, xl, nvis, dtname, tag)
            assert same2(sparse(qg, dirty.to(gpu), cs, ig, num_splits=ns), clean), f"{tag}: a row no valid slot names reached a result"
            continue
        pool, table, _ = page_kv(kv.to(gpu), P, 11 + P)
        clean = sparse(qg, pool, cs, ig, num_splits=ns, block_table=table)
        check(clean[0], clean[1], xo, xl, nvis, dtname, tag)
        dpool, dtable, _ = page_kv(dirty.to(gpu), P, 11 + P)
        reached = named.view(len(LENS), CAP // P, P).any(-1).to(gpu)
        assert torch.equal(dtable, table) and (~reached).any().item()
        dpool[dtable[~reached].long()] = NAN
        junk = torch.tensor([-1, I_MAX, I_MIN, 12345678], dtype=torch.int32, device=gpu)
        bad = dtable.clone()
        bad[~reached] = junk[torch.arange(int((~reached).sum()), device=gpu) % 4]
        assert same2(sparse(qg, dpool, cs, ig, num_splits=ns, block_table=bad), clean), f"{tag}: a row, page or table entry no valid slot reaches reached a result"
        # a needed entry outside the pool reads page num_blocks - 1: a copy of a needed page of the last sequence goes there and its entry is broken
        col = int(reached[5].nonzero()[0])
        moved, t2 = torch.cat([pool, pool[table[5, col].long()].unsqueeze(0)]), table.clone()
        for entry in (moved.shape[0], -1, I_MAX):
            t2[5, col] = entry
            got = sparse(qg, moved, cs, ig, num_splits=ns, block_table=t2)
            assert same2(got, clean), f"{tag}: entry {entry} was not clamped to the last page"


# ---- 8. NaN rules --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [0, 48])
def test_nan_rules(gpu, dtname, P):
    """a NaN in one query row touches that row only; a NaN in a cache row named by token 1's list and not by token 0's makes every head of token 1 NaN
    and leaves token 0's bits alone; the same NaN row named only by an invalid slot (entry >= L_i) changes nothing"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(79000)
    lens = [33, 100, 777]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    h, sq, topk = 24, 2, 96
    q, kv = case(dt, sq, h, gen, lens=lens)
    idx = random_lists(lens, sq, topk, gen, fill=0.4)
    # row 20 of sequence 1: in token 1's list, not in token 0's; row 150 of sequence 1 (>= L = 100) is named by both tokens, as an invalid slot
    idx[1][idx[1] == 20] = 21
    idx[1, 1, 40] = 20
    idx[1, :, 33] = 150
    ok = valid_of(idx, lens)
    assert (idx[1, 1][ok[1, 1]] == 20).sum() == 1 and not (idx[1, 0] == 20).any() and not ok[1, :, 33].any()
    qg, kvg, ig = q.to(gpu), kv.to(gpu), idx.to(gpu)
    table = None

    def run(qx, kvx, ns):
        if P:
            pool, tb, _ = page_kv(kvx, P, 17)
            return sparse(qx, pool, cs, ig, num_splits=ns, block_table=tb)
        return sparse(qx, kvx, cs, ig, num_splits=ns)

    for ns in SPLITS:
        o0, l0 = run(qg, kvg, ns)
        assert torch.isfinite(o0.float()).all().item()
        qn = qg.clone()
        qn[1, 1, 7, 530] = NAN                       # (a rope column)
        qn[2, 0, 23, 3] = NAN
        o1, l1 = run(qn, kvg, ns)
        hit = torch.zeros(len(lens), sq, h, dtype=torch.bool, device=gpu)
        hit[1, 1, 7] = hit[2, 0, 23] = True
        assert torch.isnan(o1[hit].float()).all().item() and torch.isnan(l1.permute(0, 2, 1)[hit]).all().item(), f"splits={ns}"
        assert _same(o1[~hit], o0[~hit]) and _same(l1.permute(0, 2, 1)[~hit], l0.permute(0, 2, 1)[~hit]), f"splits={ns}: a NaN query row touched another row"
        for col in (5, 570):
            kn = kvg.clone()
            kn[1, 20, 0, col] = NAN
            o2, l2 = run(qg, kn, ns)
            assert torch.isnan(o2[1, 1].float()).all().item() and torch.isnan(l2[1, :, 1]).all().item(), f"splits={ns} col={col}"
            keep = torch.ones(len(lens), sq, dtype=torch.bool, device=gpu)
            keep[1, 1] = False
            assert _same(o2[keep], o0[keep]) and _same(l2.permute(0, 2, 1)[keep], l0.permute(0, 2, 1)[keep]), f"splits={ns} col={col}: another token was touched"
            kn = kvg.clone()
            kn[1, 150, 0, col] = NAN
            assert same2(run(qg, kn, ns), (o0, l0)), f"splits={ns} col={col}: a row named only by an invalid slot reached a result"


# ---- 9. guard bands and the C ABI ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_strided_views_with_guard_bands_and_the_c_abi(gpu, dtname):
    """q, the cache and indices as views into guarded buffers through the Python call; guarded q / o views, a caller workspace with a NaN tail, a
    forced and a capped split through the C ABI: the Python call's bits, nothing written outside a view"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(80000)
    h, sq, topk = 24, 3, 96
    b = len(LENS)
    q, kv = case(dt, sq, h, gen)
    idx = random_lists(LENS, sq, topk, gen)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    qg, kvg, ig = q.to(gpu), kv.to(gpu), idx.to(gpu)
    qb, qv, _ = U.guarded((b, sq, h, DK), dt, gpu, (2, 2, 2, 16))
    cb, cv, _ = U.guarded((b, CAP, 1, DK), dt, gpu, (2, 4, 0, 16))
    ib = torch.full((b + 2, sq + 2, topk + 64), 3, dtype=torch.int32, device=gpu)
    iv = ib[1:1 + b, 1:1 + sq, 32:32 + topk]
    qv.copy_(qg); cv.copy_(kvg); iv.copy_(ig)
    keep = [t.clone() for t in (qb, cb, ib)]
    for ns in SPLITS:
        want = sparse(qg, kvg, cs, ig, num_splits=ns)
        assert same2(sparse(qv, cv, cs, iv, num_splits=ns), want), f"splits={ns}"
    assert all(_same(a, b_) for a, b_ in zip((qb, cb, ib), keep)), "an input buffer was written"
    pool, table, _ = page_kv(kvg, 48, 21)
    rows = b * h * sq
    for paged in (False, True):
        kvx, tb = (pool, table) if paged else (cv, None)
        ob, ov, osl = U.guarded((b, sq, h, DV), dt, gpu, (2, 2, 2, 16))
        lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=gpu)
        p = capi.mla_sparse_params(qv, kvx, ov, lse, iv, cs, num_splits=3, block_table=tb, softmax_scale=0.07)
        need = capi.mla_sparse_workspace_bytes(p)
        assert need == 3 * rows * DV * 4 + (3 * rows * 4 + 15) // 16 * 16
        assert capi.mla_sparse_num_splits(p) == 1                     # no workspace yet
        ws = torch.full((need // 4 + 64,), NAN, device=gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), need
        assert capi.mla_sparse_num_splits(p) == 3
        capi.run_mla_sparse_fwd_kvcache(p)
        torch.cuda.synchronize()
        want = sparse(qg, kvx, cs, ig, num_splits=3, block_table=tb, softmax_scale=0.07)
        assert _same(ov.contiguous(), want[0]) and _same(lse, want[1]), f"paged={paged}"
        omask = torch.ones(ob.shape, dtype=torch.bool, device=gpu)
        omask[osl] = False
        assert (U.bits(ob)[omask] == U.SENT16).all().item(), "out was written outside its view"
        assert torch.isnan(ws[-64:]).all().item(), "the workspace was written past the bytes the library asked for"
        # a workspace too small for three splits caps the split; the result is that of the capped count
        p.workspace_bytes = 2 * rows * DV * 4 + (2 * rows * 4 + 15) // 16 * 16
        assert capi.mla_sparse_num_splits(p) == 2
        capi.run_mla_sparse_fwd_kvcache(p)
        torch.cuda.synchronize()
        two = sparse(qg, kvx, cs, ig, num_splits=2, block_table=tb, softmax_scale=0.07)
        assert _same(ov.contiguous(), two[0]) and _same(lse, two[1]), f"paged={paged}: the capped split"


# ---- 10. graph capture ---------------------------------------------------------------------------------------------------------------------------

def test_captured_call_replays_with_new_indices_lengths_and_table(gpu):
    dt, h, sq, b, P, cap, topk = torch.bfloat16, 128, 1, 2, 64, 4096, 256
    gen = torch.Generator().manual_seed(81000)
    kv = _rand((b, cap, 1, DK), dt, gen).to(gpu)
    q = _rand((b, sq, h, DK), dt, gen).to(gpu)
    pool, table, _ = page_kv(kv, P, 5, fill=0.0)
    lens = [100, 4000]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    ig = random_lists(lens, sq, topk, gen, cap=cap).to(gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sparse(q, pool, cs, ig, block_table=table)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = sparse(q, pool, cs, ig, block_table=table)
    first = (out_g.clone(), lse_g.clone())
    lens = [2500, 5]
    idx2 = random_lists(lens, sq, topk, gen, cap=cap)
    cs.copy_(torch.tensor(lens, dtype=torch.int32))
    ig.copy_(idx2)
    table.copy_(table.flip(0))                       # the sequences swap their pages
    g.replay()
    torch.cuda.synchronize()
    assert same2((out_g, lse_g), sparse(q, pool, cs, ig, block_table=table))
    assert not _same(out_g, first[0])
    kvl = pool[table.long()].reshape(b, cap, 1, DK).cpu()
    xo, xl, nvis = expect(q, kvl, idx2, lens)
    check(out_g, lse_g, xo, xl, nvis, "bf16", "sparse graph replay")
