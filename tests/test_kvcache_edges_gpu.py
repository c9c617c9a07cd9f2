"""GPU: decode attention over a KV cache at its edges (fa_fwd_kvcache.hip through flash_attn_with_kvcache and the C ABI).

Values are checked like tests/test_kvcache_gpu.py: against the C oracle on each sequence's valid prefix and the relative metric against fp64
math (_util.check_kvcache_rows, _util.assert_close, _util.LSE_TOL).  On top of that:
  * non-finite inputs: the NaN pattern of O and LSE is that of plain fp64 math on the same bits, under one split, two splits and the library's
    own split; rows that cannot see the bad value are bit-identical to a clean run;
  * memory that is not part of the problem (cache rows at and past L, heads a view skips, guard bands around views, NaN-prefilled O / LSE /
    workspace) is never read into a result and never written;
  * split boundaries, the split cap, long contexts, odd query-row packings, softmax extremes across waves and splits, 64-bit batch offsets,
    batch invariances and a decode loop replayed from a graph."""

import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
STEP = 32                # keys per wave step, the split granularity (kKvcStep)
MAX_SPLITS = 128         # the automatic rule's cap (kKvcMaxSplits)


def _rand(shape, dt, gen, dev):
    return torch.randn(*shape, device=dev, dtype=torch.float32, generator=gen).to(dt)


_bits, _poison_ = U.bits, U.poison_


def _ws(nbytes, dev, fill=float("nan"), guard=64):
    """fp32 workspace of nbytes (16-byte aligned) followed by `guard` sentinel floats; returns (workspace view, whole buffer)"""
    buf = torch.full((nbytes // 4 + guard,), fill, dtype=torch.float32, device=dev)
    return buf[:nbytes // 4], buf


def _params(q, kc, vc, o, lse, cs, causal=False, num_splits=0, k_new=None, v_new=None, ws=None):
    p = capi.kvcache_params(q, kc, vc, o, lse, cache_seqlens=cs, k_new=k_new, v_new=v_new, causal=causal, num_splits=num_splits)
    if ws is not None:
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return p


def _run(q, kc, vc, o, lse, cs, causal=False, num_splits=0, k_new=None, v_new=None, prefill=float("nan")):
    """one launch through the C ABI with a workspace sized for num_splits (0: the library's choice), prefilled with `prefill`;
    returns the split count the launch used"""
    p = _params(q, kc, vc, o, lse, cs, causal, num_splits, k_new, v_new)
    need = capi.kvcache_workspace_bytes(p)
    ws, buf = _ws(max(need, 16), q.device, prefill)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    n = capi.kvcache_num_splits(p)
    capi.run_fwd_kvcache(p)
    torch.cuda.synchronize()
    assert torch.isnan(buf[ws.numel():]).all().item() if prefill != prefill else (buf[ws.numel():] == prefill).all().item(), "workspace guard written"
    return n


# ---- 1. non-finite inputs ------------------------------------------------------------------------------------------------------------

_fp64_math = U.fp64_math


@pytest.mark.parametrize("num_splits", [1, 2, 0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("case", ["q_nan", "k_nan", "k_inf"])
def test_nonfinite_inputs_propagate_like_fp64_math(gpu, case, causal, num_splits):
    """one NaN in a query row, one NaN in a K element inside L, or one +inf in a K element: wherever fp64 math on the same bits gives NaN the
    kernel must give NaN (O and LSE alike), everywhere else finite; rows that cannot see the bad value keep the clean run's bits; rows whose
    score turns -inf lose that key and still match fp64 math; rows that see no key stay O = 0, LSE = 0 (a NaN query included); the split
    result stays deterministic.  A NaN row must not be taken for a dead one: that gave LSE 0 under one split, and under several a finite
    result built from the other splits only."""
    dt, d, h, hk, sq, cap = torch.float16, 128, 8, 2, 4, 1024
    gen = torch.Generator(device=gpu).manual_seed(31)
    lens = [1000, 700, 2, 0]
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, sq, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    qb, kb = q.clone(), k_cache.clone()
    if case == "q_nan":
        qb[0, 1, 3, 5] = float("nan")
        qb[2, 0, 1, 9] = float("nan")            # L = 2: under causal the row t = 0 sees no key at all (dead), otherwise both keys
    elif case == "k_nan":
        kb[0, lens[0] - sq + 1, 1, 7] = float("nan")      # under causal the query t = 0 stops one key short of it
        kb[2, 1, 0, 0] = float("nan")
    else:
        kb[1, 300, 0, 9] = float("inf")          # score +inf for query heads with q[..., 9] > 0 (NaN row), -inf where q[..., 9] < 0 (key dropped)
        kb[0, lens[0] - 1, 1, 2] = float("inf")
    kw = dict(cache_seqlens=cs, causal=causal, num_splits=num_splits, return_softmax_lse=True)
    o_c, l_c = F.flash_attn_with_kvcache(q, k_cache, v_cache, **kw)
    o_b, l_b = F.flash_attn_with_kvcache(qb, kb, v_cache, **kw)
    o_b2, l_b2 = F.flash_attn_with_kvcache(qb, kb, v_cache, **kw)
    assert torch.equal(_bits(o_b), _bits(o_b2)) and torch.equal(_bits(l_b), _bits(l_b2)), "not deterministic"
    assert not torch.isinf(o_b).any().item() and not torch.isinf(l_b).any().item()
    n_nan = 0
    for i, L in enumerate(lens):
        ro_b, rl_b = _fp64_math(qb[i], kb[i, :L], v_cache[i, :L], causal)
        ro_c, rl_c = _fp64_math(q[i], k_cache[i, :L], v_cache[i, :L], causal)
        xo, xl = o_b[i].cpu(), l_b[i].cpu()
        tag = f"{case} causal={causal} num_splits={num_splits} b{i} L{L}"
        assert torch.equal(torch.isnan(xl), torch.isnan(rl_b)), f"{tag}: LSE NaN pattern {torch.isnan(xl).nonzero().tolist()} != fp64 {torch.isnan(rl_b).nonzero().tolist()}"
        assert torch.equal(torch.isnan(xo), torch.isnan(ro_b)), f"{tag}: O NaN pattern differs from fp64 math (rows {torch.isnan(ro_b).any(-1).nonzero().tolist()})"
        n_nan += int(torch.isnan(rl_b).sum())
        for t in range(sq):
            for hq in range(h):
                if torch.isnan(rl_b[hq, t]):
                    continue
                if torch.equal(ro_b[t, hq], ro_c[t, hq]) and torch.equal(rl_b[hq, t], rl_c[hq, t]):
                    # unaffected row: the clean run's bits
                    assert torch.equal(_bits(o_b[i, t, hq]), _bits(o_c[i, t, hq])) and torch.equal(_bits(l_b[i, hq, t]), _bits(l_c[i, hq, t])), \
                        f"{tag}: row t{t} h{hq} cannot see the bad value but changed"
                else:
                    # a -inf score: the key drops out, the row is still finite fp64 math
                    U.assert_close(xo[t, hq].float().numpy(), ro_b[t, hq].numpy(), "fp16", f"{tag} t{t} h{hq}")
                    assert abs(float(xl[hq, t]) - float(rl_b[hq, t])) <= U.LSE_TOL, tag
                if not (ro_b[t, hq] != 0).any() and rl_b[hq, t] == 0:
                    assert (o_b[i, t, hq] == 0).all().item() and l_b[i, hq, t].item() == 0, f"{tag}: dead row t{t} h{hq}"
    assert n_nan > 0, "the case must produce NaN rows"


# ---- 2. memory that is not part of the problem ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("layout", ["rows", "head_major"])
def test_cache_past_length_and_skipped_heads_are_never_read(gpu, d, layout):
    """cache rows from L to capacity (row L itself and the rest of the last 32-key step included) and the heads a strided view skips hold
    NaN, +-inf and 65504: outputs stay finite and correct.  head_major: (b, h_k, cap, d).transpose(1, 2), row stride = d, so row L sits
    directly behind row L - 1 in memory."""
    dt, h, hk, cap = torch.bfloat16, 12, 3, 700
    gen = torch.Generator(device=gpu).manual_seed(41 + d)
    lens = [1, 31, 32, 33, 63, 64, 65, 500, cap - 1, cap, 0]
    b = len(lens)
    caches = []
    for _ in range(2):
        if layout == "rows":
            buf = _poison_(torch.empty(b, cap, 2 * hk, d, device=gpu, dtype=dt))
            c = buf[:, :, 1::2]
        else:
            buf = _poison_(torch.empty(b, hk, cap, d, device=gpu, dtype=dt))
            c = buf.transpose(1, 2)
            assert c.stride(1) == d
        for i, L in enumerate(lens):
            c[i, :L] = _rand((L, hk, d), dt, gen, gpu)
        caches.append(c)
    k_cache, v_cache = caches
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for sq, causal in ((1, False), (5, True)):
        q = _rand((b, sq, h, d), dt, gen, gpu)
        for ns in (0, 1, 3):
            out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True)
            assert torch.isfinite(out).all().item() and torch.isfinite(lse).all().item(), (layout, sq, ns)
            U.check_kvcache_rows(out, lse, q, k_cache, v_cache, lens, causal, "bf16", f"poisoned {layout} d{d} sq{sq} ns{ns}")


@pytest.mark.parametrize("num_splits", [1, 4, 0])
def test_prefilled_outputs_and_workspace_are_fully_written(gpu, num_splits):
    """O, LSE and an explicit workspace start as NaN: every element comes out finite, and the same bits as the torch entry point.  Short
    sequences in a large cache leave most splits empty: their O planes stay NaN and must never be read by the combine."""
    dt, d, h, hk, sq, cap = torch.float16, 64, 16, 2, 3, 4096
    gen = torch.Generator(device=gpu).manual_seed(43)
    lens = [0, 1, 40, 300, 4096]
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, sq, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for causal in (False, True):
        o = torch.full_like(q, float("nan"))
        lse = torch.full((b, h, sq), float("nan"), device=gpu)
        n = _run(q, k_cache, v_cache, o, lse, cs, causal, num_splits)
        assert n == (num_splits or n) and (num_splits == 1 or n > 1), n
        assert torch.isfinite(o).all().item() and torch.isfinite(lse).all().item(), (causal, n)
        o_t, lse_t = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, causal=causal, num_splits=n, return_softmax_lse=True)
        assert torch.equal(_bits(o), _bits(o_t)) and torch.equal(lse, lse_t)
        U.check_kvcache_rows(o, lse, q, k_cache, v_cache, lens, causal, "fp16", f"prefilled causal={causal} n{n}")


_guarded = U.guarded


@pytest.mark.parametrize("causal", [False, True])
def test_views_with_guard_bands_change_only_their_rows(gpu, causal):
    """O and the caches are views into sentinel-filled buffers with gaps between heads, rows and batch entries; after a launch with append
    every byte outside O's view and every cache byte outside rows [cs, cs + sn) is bit-identical.  One entry breaks the precondition
    (cs + sn > capacity): its rows at or past the capacity are dropped, not written into the guard band."""
    dt, d, h, hk, sq, cap, sn = torch.float16, 128, 8, 2, 3, 300, 3
    gen = torch.Generator(device=gpu).manual_seed(47)
    lens = [0, 33, 297, cap - 1, 150]
    b = len(lens)
    kbuf, kc, ksl = _guarded((b, cap, hk, d), dt, gpu, (1, 6, 2, 16))
    vbuf, vc, vsl = _guarded((b, cap, hk, d), dt, gpu, (2, 4, 1, 24))
    obuf, o, osl = _guarded((b, sq, h, d), dt, gpu, (1, 2, 3, 16))
    kc.copy_(_rand((b, cap, hk, d), dt, gen, gpu))
    vc.copy_(_rand((b, cap, hk, d), dt, gen, gpu))
    lbuf = torch.full((b * h * sq + 128,), float("nan"), device=gpu)
    lse = lbuf[64:64 + b * h * sq].view(b, h, sq)
    k_new, v_new = _rand((b, sn, hk, d), dt, gen, gpu), _rand((b, sn, hk, d), dt, gen, gpu)
    q = _rand((b, sq, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k0, v0, o0, l0 = (_bits(x).clone() for x in (kbuf, vbuf, obuf, lbuf))
    k_exp, v_exp = kc.clone(), vc.clone()
    for i, L in enumerate(lens):
        n = min(sn, cap - L)
        k_exp[i, L:L + n], v_exp[i, L:L + n] = k_new[i, :n], v_new[i, :n]
    _run(q, kc, vc, o, lse, cs, causal, 0, k_new, v_new)
    for name, buf, before, sl, exp in (("k_cache", kbuf, k0, ksl, k_exp), ("v_cache", vbuf, v0, vsl, v_exp)):
        inside = torch.zeros(buf.shape, dtype=torch.bool, device=gpu)
        inside[sl] = True
        assert torch.equal(_bits(buf)[~inside], before[~inside]), f"{name}: bytes outside the view changed"
        assert torch.equal(_bits(buf[sl]), _bits(exp)), f"{name}: rows other than [cs, cs + sn) changed, or the append is wrong"
    inside = torch.zeros(obuf.shape, dtype=torch.bool, device=gpu)
    inside[osl] = True
    assert torch.equal(_bits(obuf)[~inside], o0[~inside]), "O: bytes outside the view changed"
    assert torch.equal(_bits(lbuf)[:64], l0[:64]) and torch.equal(_bits(lbuf)[64 + b * h * sq:], l0[64 + b * h * sq:]), "LSE guard written"
    assert torch.isfinite(o).all().item() and torch.isfinite(lse).all().item()
    U.check_kvcache_rows(o, lse, q, k_exp, v_exp, [min(L + sn, cap) for L in lens], causal, "fp16", f"guarded causal={causal}")


# ---- 3. the split --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_splits", [1, 2, 3, 5, 7, 16, 64, 128, 500])
def test_split_chunk_boundaries(gpu, num_splits):
    """forced splits (500: more than the 129 steps of the capacity); lengths at chunk boundaries -1, 0, +1 (chunk = ceil(steps / n) x 32
    keys) and causal seqlen_q = 16 runs whose last split starts inside the causal band (rows of that split that see none of its keys).
    h = 8: a one-query check holds 1024 elements, so one element of O that is ~0 (relative error ~5 on an absolute error of 6e-6, the
    normal fp16 rounding) does not by itself decide the mean relative error."""
    dt, d, h, hk, cap = torch.float16, 128, 8, 2, 4100
    steps = -(-cap // STEP)
    n_eff = min(num_splits, steps)
    chunk = -(-steps // n_eff) * STEP
    n_chunks = -(-cap // chunk)
    js = sorted({1, n_chunks // 2, n_chunks - 1} - {0})
    lens = sorted({min(max(j * chunk + e, 0), cap) for j in js for e in (-1, 0, 1)} | {cap, 1})
    gen = torch.Generator(device=gpu).manual_seed(53 + num_splits)
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    band = [min(max(j * chunk + 8, 0), cap) for j in js]           # the last split holds 8 keys; causal rows t < 7 see none of them
    cs_band = torch.tensor(band, dtype=torch.int32, device=gpu)
    for sq, causal, c, ls in ((1, False, cs, lens), (16, True, cs, lens), (16, True, cs_band, band)):
        bb = len(ls)
        q = _rand((bb, sq, h, d), dt, gen, gpu)
        o, lse = torch.empty_like(q), torch.empty(bb, h, sq, device=gpu)
        n = _run(q, k_cache[:bb], v_cache[:bb], o, lse, c, causal, num_splits)
        assert n == n_eff, (n, n_eff)
        U.check_kvcache_rows(o, lse, q, k_cache, v_cache, ls, causal, "fp16", f"n{num_splits} chunk{chunk} sq{sq} causal={causal}")


def test_small_workspace_lowers_the_split(gpu):
    """a workspace smaller than the library's split needs lowers capi.kvcache_num_splits (down to one split for 0 bytes) and the
    results stay correct; a larger one than needed changes nothing"""
    dt, d, h, hk, cap = torch.bfloat16, 128, 8, 2, 16384
    gen = torch.Generator(device=gpu).manual_seed(59)
    lens = [16384, 9001]
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, 2, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    o, lse = torch.empty_like(q), torch.empty(b, h, 2, device=gpu)
    need = capi.kvcache_workspace_bytes(_params(q, k_cache, v_cache, o, lse, cs))
    p_full = _params(q, k_cache, v_cache, o, lse, cs, ws=_ws(need, gpu)[0])
    n_full = capi.kvcache_num_splits(p_full)
    assert n_full > 2
    seen = []
    for frac in (0.0, 0.3, 0.7, 1.0, 2.0):
        nbytes = int(need * frac) // 16 * 16
        ws, buf = _ws(max(nbytes, 16), gpu)
        p = _params(q, k_cache, v_cache, o, lse, cs, causal=True)
        p.workspace, p.workspace_bytes = ws.data_ptr(), nbytes
        n = capi.kvcache_num_splits(p)
        assert (n == 1) if frac == 0.0 else (n < n_full if frac < 1.0 else n == n_full), (frac, n, n_full)
        assert capi.kvcache_workspace_bytes(_params(q, k_cache, v_cache, o, lse, cs, num_splits=n)) <= max(nbytes, 0) or n == 1
        o.fill_(float("nan"))
        lse.fill_(float("nan"))
        capi.run_fwd_kvcache(p)
        torch.cuda.synchronize()
        assert torch.isnan(buf[ws.numel():]).all().item(), "workspace guard written"
        U.check_kvcache_rows(o, lse, q, k_cache, v_cache, lens, True, "bf16", f"workspace {frac} n{n}")
        seen.append(n)
    assert len(set(seen)) >= 3, seen


# ---- 4. long context -----------------------------------------------------------------------------------------------------------------

PRIME = {65536: 65521, 131072: 100003}


@pytest.mark.parametrize("dtname,d,cap", [("fp16", 128, 131072), ("bf16", 64, 131072), ("bf16", 128, 65536), ("fp16", 64, 65536)])
def test_long_context_at_the_split_cap(gpu, dtname, d, cap):
    """b1 h_k 2: the automatic rule reaches its cap of 128 splits; L = cap, cap - 1 and a prime.  Both capacities, both dtypes and both head
    dims, in pairs (the fp64 expectation of one 128k-key check costs about a second)."""
    dt, h, hk = DT[dtname], 4, 2
    gen = torch.Generator(device=gpu).manual_seed(61 + d + cap)
    k_cache, v_cache = _rand((1, cap, hk, d), dt, gen, gpu), _rand((1, cap, hk, d), dt, gen, gpu)
    for L in (cap, cap - 1, PRIME[cap]):
        q = _rand((1, 1, h, d), dt, gen, gpu)
        cs = torch.tensor([L], dtype=torch.int32, device=gpu)
        o, lse = torch.full_like(q, float("nan")), torch.full((1, h, 1), float("nan"), device=gpu)
        assert _run(q, k_cache, v_cache, o, lse, cs) == MAX_SPLITS
        U.check_kvcache_rows(o, lse, q, k_cache, v_cache, [L], False, dtname, f"long {dtname} d{d} cap{cap}")
    o_t, lse_t = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, return_softmax_lse=True)
    assert torch.equal(_bits(o), _bits(o_t)) and torch.equal(lse, lse_t)


# ---- 5. shapes -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("sq", [17, 31, 64, 128, 255])
def test_many_query_positions(gpu, sq, causal):
    """seqlen_q beyond 16 (several row tiles per KV head; GQA 3 so tiles end partway through a query position), with an L = 0 entry and,
    under causal, an entry shorter than seqlen_q (its first rows see no key)"""
    dt, d, h, hk, cap = torch.float16, 64, 6, 2, 1100
    gen = torch.Generator(device=gpu).manual_seed(67 + sq)
    lens = [1023, 0, sq // 2 + 1, 1100]
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, sq, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, causal=causal, return_softmax_lse=True)
    U.check_kvcache_rows(out, lse, q, k_cache, v_cache, lens, causal, "fp16", f"sq{sq} causal={causal}")


@pytest.mark.parametrize("ratio", [3, 5, 6, 7, 12, 16])
def test_gqa_ratios_that_split_a_query_position(gpu, ratio):
    """h / h_k that do not divide 16: the packed 16-row tiles end partway through a query position"""
    dt, d, hk, cap = torch.bfloat16, 128, 2, 900
    h = ratio * hk
    gen = torch.Generator(device=gpu).manual_seed(71 + ratio)
    lens = [0, 77, 900, 513]
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for sq, causal in ((1, False), (3, True), (7, False), (16, True)):
        q = _rand((b, sq, h, d), dt, gen, gpu)
        out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, causal=causal, return_softmax_lse=True)
        U.check_kvcache_rows(out, lse, q, k_cache, v_cache, lens, causal, "bf16", f"ratio{ratio} sq{sq} causal={causal}")


# ---- 6. the softmax across waves and splits ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_splits", [1, 7, 0])
@pytest.mark.parametrize("pattern", ["ramp_up", "ramp_down", "spike_last_split", "scaled_by_6", "lse_gap_first", "lse_gap_last"])
def test_softmax_extremes(gpu, pattern, num_splits):
    """scores that rise / fall along the key axis (the running max moves every step), one dominant key in the last split, q and k scaled by
    6 (near one-hot rows), and splits whose LSE lies more than 100 above the others (their weights underflow to exactly 0 in the merge)"""
    dt, d, h, hk, cap, sq = torch.float16, 128, 4, 4, 3072, 2
    L = 3000
    gen = torch.Generator(device="cpu").manual_seed(73)
    q = torch.randn(1, sq, h, d, generator=gen) * 0.5 + 1.0
    k = torch.randn(1, cap, hk, d, generator=gen) * 0.5
    v = torch.randn(1, cap, hk, d, generator=gen)
    chunk = -(-(-(-cap // STEP)) // 7) * STEP           # the chunk of 7 splits
    if pattern.startswith("ramp"):
        ramp = 1.0 if pattern == "ramp_up" else -1.0
        k = k + (ramp * torch.arange(cap).float() / 64.0 / d ** 0.5).view(1, cap, 1, 1)
    elif pattern == "spike_last_split":
        k[0, L - 5] = q[0, 0]                              # score |q|^2 / sqrt(d) ~ 14 above the rest for query 0
    elif pattern == "scaled_by_6":
        q, k = q * 6.0, torch.randn(1, cap, hk, d, generator=gen) * 6.0
    else:
        # a block of keys along q's direction, 130 / sqrt(d) x |q| ~ 115 nats above the other keys' scores (std ~ 0.6)
        block = slice(0, chunk) if pattern == "lse_gap_first" else slice(L - 40, L)
        qdir = q[0, 0] / q[0, 0].norm(dim=-1, keepdim=True)
        k[0, block] = k[0, block] + 130.0 * qdir.unsqueeze(0)
    q, k, v = (x.to(gpu, dt) for x in (q, k, v))
    cs = torch.tensor([L], dtype=torch.int32, device=gpu)
    for causal in (False, True):
        out, lse = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, causal=causal, num_splits=num_splits, return_softmax_lse=True)
        assert torch.isfinite(out).all().item() and torch.isfinite(lse).all().item(), (pattern, causal)
        if pattern.startswith("lse_gap"):
            _, rl = _fp64_math(q[0], k[0, :L], v[0, :L], causal)
            rest = slice(chunk, L) if pattern == "lse_gap_first" else slice(0, L - 40)
            _, rl_rest = _fp64_math(q[0], k[0, rest], v[0, rest], False)
            assert (rl - rl_rest).min().item() > 100.0, "the case must put an LSE gap > 100 between splits"
        # the ramps: the bound of test_running_max_rising_along_the_key_axis (a handful of effective keys per row)
        U.check_kvcache_rows(out, lse, q, k, v, [L], causal, "fp16", f"{pattern} n{num_splits} causal={causal}",
                             scale=2.0 if pattern.startswith("ramp") else 1.0)


# ---- 7. 64-bit offsets ---------------------------------------------------------------------------------------------------------------

def _far_batch_entry(gpu):
    dt, d, h, hk, cap, sq, sn = torch.float16, 128, 8, 2, 256, 2, 2
    stride_b = 2 ** 31 + 64
    gen = torch.Generator(device=gpu).manual_seed(79)

    def big(rows, heads):
        t = torch.empty(stride_b + rows * heads * d, dtype=dt, device=gpu).as_strided((2, rows, heads, d), (stride_b, heads * d, d, 1))
        t[0], t[1] = _rand((rows, heads, d), dt, gen, gpu), _rand((rows, heads, d), dt, gen, gpu)
        return t

    kc, vc, q, o = big(cap, hk), big(cap, hk), big(sq, h), big(sq, h)
    assert kc.stride(0) * kc.element_size() > 2 ** 32
    lens = [100, 200]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    lse = torch.empty(2, h, sq, device=gpu)
    for causal in (False, True):
        o[0], o[1] = float("nan"), float("nan")
        _run(q, kc, vc, o, lse, cs, causal)
        U.check_kvcache_rows(o, lse, q, kc, vc, lens, causal, "fp16", f"64-bit offsets causal={causal}")
    k_new, v_new = _rand((2, sn, hk, d), dt, gen, gpu), _rand((2, sn, hk, d), dt, gen, gpu)
    k_exp, v_exp = kc.clone(memory_format=torch.contiguous_format), vc.clone(memory_format=torch.contiguous_format)
    for i, L in enumerate(lens):
        k_exp[i, L:L + sn], v_exp[i, L:L + sn] = k_new[i], v_new[i]
    _run(q, kc, vc, o, lse, cs, True, 0, k_new, v_new)
    for i in (0, 1):
        assert torch.equal(_bits(kc[i]), _bits(k_exp[i])) and torch.equal(_bits(vc[i]), _bits(v_exp[i])), f"append at entry {i}"
    U.check_kvcache_rows(o, lse, q, k_exp, v_exp, [L + sn for L in lens], True, "fp16", "64-bit offsets append")


def test_batch_stride_beyond_2_to_the_31(gpu):
    """K, V, q and O with a batch stride of 2^31 + 64 elements (as_strided over one ~4.3 GB allocation per tensor, only the rows in use
    filled): the far batch entry, with and without append"""
    torch.cuda.empty_cache()
    try:
        _far_batch_entry(gpu)
    finally:
        torch.cuda.empty_cache()


# ---- 8. invariances ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_splits", [1, 6])
def test_batch_invariances(gpu, num_splits):
    """within one launch shape, bit for bit: entry i does not depend on the other entries' lengths, and permuting the batch permutes the outputs"""
    dt, d, h, hk, sq, cap = torch.bfloat16, 64, 8, 2, 3, 2000
    gen = torch.Generator(device=gpu).manual_seed(83)
    b = 5
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, sq, h, d), dt, gen, gpu)
    run = lambda qq, kk, vv, ls: F.flash_attn_with_kvcache(qq, kk, vv, cache_seqlens=torch.tensor(ls, dtype=torch.int32, device=gpu), causal=True,
                                                           num_splits=num_splits, return_softmax_lse=True)
    lens = [1500, 3, 0, 2000, 777]
    o, lse = run(q, k_cache, v_cache, lens)
    U.check_kvcache_rows(o, lse, q, k_cache, v_cache, lens, True, "bf16", f"invariance n{num_splits}")
    for other in ([1, 3, 2000, 2000, 64], [2000, 2000, 1, 0, 5]):
        ls = [lens[0]] + other[1:]
        o2, lse2 = run(q, k_cache, v_cache, ls)
        assert torch.equal(_bits(o2[0]), _bits(o[0])) and torch.equal(lse2[0], lse[0]), ("entry 0 depends on the others", ls)
    perm = [3, 0, 4, 2, 1]
    o3, lse3 = run(q[perm], k_cache[perm], v_cache[perm], [lens[i] for i in perm])
    assert torch.equal(_bits(o3), _bits(o[perm])) and torch.equal(lse3, lse[perm]), "permuting the batch must permute the outputs"


# ---- 9. decode loop in a graph -------------------------------------------------------------------------------------------------------

def test_decode_loop_replayed_from_a_graph(gpu):
    """append one token + attention + cache_seqlens += 1 captured once and replayed 40 steps: each step against the oracle over its
    prefix, the final cache bit for bit"""
    dt, d, h, hk, cap, steps = torch.float16, 128, 16, 4, 1100, 40
    gen = torch.Generator(device=gpu).manual_seed(89)
    lens0 = [50, 1000, 0]
    b = len(lens0)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    k_exp, v_exp = k_cache.clone(), v_cache.clone()
    q, k_new, v_new = _rand((b, 1, h, d), dt, gen, gpu), _rand((b, 1, hk, d), dt, gen, gpu), _rand((b, 1, hk, d), dt, gen, gpu)
    cs = torch.tensor(lens0, dtype=torch.int32, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, k_cache, v_cache, k=k_new, v=v_new, cache_seqlens=cs, causal=True)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, k_cache, v_cache, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True)
        cs.add_(1)
    torch.cuda.synchronize()
    assert cs.tolist() == lens0, "capture must not run the work"
    for step in range(steps):
        q.copy_(_rand((b, 1, h, d), dt, gen, gpu))
        k_new.copy_(_rand((b, 1, hk, d), dt, gen, gpu))
        v_new.copy_(_rand((b, 1, hk, d), dt, gen, gpu))
        g.replay()
        torch.cuda.synchronize()
        lens = [L + step + 1 for L in lens0]
        for i in range(b):
            k_exp[i, lens[i] - 1], v_exp[i, lens[i] - 1] = k_new[i, 0], v_new[i, 0]
        assert cs.tolist() == lens
        U.check_kvcache_rows(out_g, lse_g, q, k_exp, v_exp, lens, True, "fp16", f"graph step {step}")
    assert torch.equal(_bits(k_cache), _bits(k_exp)) and torch.equal(_bits(v_cache), _bits(v_exp)), "final cache"
