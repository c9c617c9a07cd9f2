"""GPU: tree attention masks on the decode path (flash_attn_with_kvcache(..., tree_mask=), fa_kvcache_options_v7).

Expectations: neither the C oracle nor the reference has a tree mask, so the value tests compare with fp64 math written here - the masked
softmax of the existing decode suites with the visibility rule of the feature (key j < L is seen iff j < L - sq or bit j - (L - sq) of the
row's word is set; the bits are decoded here with Python integers, not with the package's helpers) - through _util.assert_close without an
oracle (its "plain" rule from 64 keys on, its "floor" rule below) and _util.LSE_TOL: the project's numbers, no new tolerance.  The rows are
asserted in the two groups those rules make, as the sinks suite does; rows that see no key are asserted exactly, O = 0 and LSE = 0.  Every
value case with 17 or 64 query rows first asserts, on the fp64 expectation alone, that it is far (4 x the dtype's mean_abs tolerance) from
the causal expectation, from the all-visible one and from the one under the transposed mask, so a kernel that ignored the mask or swapped
its roles could not pass.  Everything else is a relation that must hold to the bit."""

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from test_kvcache_fp8_gpu import _descale, deq, quantise
from test_kvcache_fp8_gpu import _page as _page8
from test_kvcache_softcap_gpu import DT, _rand, _same, default_scale
from test_kvcache_window_gpu import _page

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
CAP = 1088                              # 1000 prefix keys + 64 draft tokens, rounded up to the page sizes used below
SQS = [1, 2, 5, 17, 64]
HEADS = [(8, 8), (32, 8), (16, 1), (6, 2)]          # packing ratios 1, 4, 16 and 3 (the 16-row tiles cut through a token's heads)
PREFIXES = [0, 1, 31, 33, 100, 777, 1000]
SPLITS = [0, 1, 3]
ALL64 = (1 << 64) - 1


# ---- masks (bool (sq, sq): row t, column u = "draft token t sees draft token u") and their words -------------------------------------------------

def _ancestors(parents):
    sq = len(parents)
    m = torch.zeros(sq, sq, dtype=torch.bool)
    for t in range(sq):
        a = t
        while a >= 0:
            m[t, a] = True
            a = parents[a]
    return m


def heap_mask(sq):
    """the binary-heap tree: parent (t - 1) // 2"""
    return _ancestors([(t - 1) // 2 if t else -1 for t in range(sq)])


def forest_mask(sq):
    """three roots (0, 1, 2); node t >= 3 hangs under t - 3 or, every fourth node, under t - 2: chains that branch"""
    return _ancestors([-1 if t < 3 else (t - 2 if t % 4 == 0 else t - 3) for t in range(sq)])


def random_mask(sq, gen):
    """random bits at density 0.5 with the diagonal set: not a tree, columns above the diagonal included"""
    return (torch.rand(sq, sq, generator=gen) < 0.5) | torch.eye(sq, dtype=torch.bool)


def tri_mask(sq):
    return torch.tril(torch.ones(sq, sq, dtype=torch.bool))


def words_of(m):
    """int64 (sq,) from a bool (sq, sq), with Python integers (bit 63 wraps into the sign)"""
    out = []
    for row in m.tolist():
        w = sum(1 << u for u, bit in enumerate(row) if bit)
        out.append(w - (1 << 64) if w >= (1 << 63) else w)
    return torch.tensor(out, dtype=torch.int64)


def visible(lens, sq, words, cap):
    """bool (b, sq, cap): the feature's rule, from the int64 words (b, sq) as Python integers"""
    b = len(lens)
    vis = torch.zeros(b, sq, cap, dtype=torch.bool)
    wl = words.tolist()
    for i, L in enumerate(lens):
        base = L - sq
        vis[i, :, :max(base, 0)] = True
        for t in range(sq):
            w = wl[i][t] & ALL64
            for u in range(sq):
                j = base + u
                if 0 <= j < L and (w >> u) & 1:
                    vis[i, t, j] = True
    return vis


# ---- fp64 ----------------------------------------------------------------------------------------------------------------------------------------

def scores64(q, k, scale=None):
    """fp64 (b, hk, ratio, sq, cap): (q . k) * scale.  q (b, sq, h, d), k the logical cache (b, cap, hk, d), any float dtype"""
    b, sq, h, d = q.shape
    hk = k.shape[2]
    qd = q.detach().cpu().double().view(b, sq, hk, h // hk, d).permute(0, 2, 3, 1, 4)
    kd = k.detach().cpu().double().permute(0, 2, 3, 1)[:, :, None]
    return torch.matmul(qd, kd) * (default_scale(d) if scale is None else float(np.float32(scale)))


def exact(s, v, vis):
    """the masked softmax in fp64: s from scores64, v the logical cache (b, cap, hk, d), vis bool (b, sq, cap).  Returns O (b, sq, h, d), LSE
    (b, h, sq) - rows without a visible key 0, 0 - and the visible keys per row (b, sq)"""
    b, hk, ratio, sq, cap = s.shape
    vm = vis[:, None, None]
    sm = s.masked_fill(~vm, -INF)
    m = sm.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(sm - m)
    den = p.sum(-1, keepdim=True)
    live = den > 0
    w = torch.where(live, p / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(p))
    # (a key no row sees has weight exactly 0: keep a non-finite V row it holds out of the product)
    vd = v.detach().cpu().double().permute(0, 2, 1, 3)
    vd = torch.where(vis.any(1)[:, None, :, None], vd, torch.zeros_like(vd))[:, :, None]
    o = torch.matmul(w, vd).permute(0, 3, 1, 2, 4).reshape(b, sq, hk * ratio, -1)
    lse = torch.where(live, m + torch.log(torch.where(live, den, torch.ones_like(den))), torch.zeros_like(den)).squeeze(-1)
    return o, lse.reshape(b, hk * ratio, sq), vis.sum(-1)


def split_rows(out, lse, xo, xl, nvis, tag):
    """out (b, sq, h, d) / lse (b, h, sq) of one call against the fp64 expectation, the part that is asserted row by row: rows without a visible
    key exactly O = 0 and LSE = 0, every LSE under LSE_TOL.  Returns the rows that see a key in the two groups of _util.check_mean_rel's
    rules, {"long" / "short": (got (n, d), expected (n, d), the fewest keys a row of the group sees)}."""
    out_c, lse_c = out.detach().float().cpu(), lse.detach().cpu()
    assert torch.isfinite(out_c).all().item() and torch.isfinite(lse_c).all().item(), f"{tag}: non-finite values"
    dead = nvis == 0
    if dead.any():
        assert (out_c[dead] == 0).all().item(), f"{tag}: a row without a visible key must be O = 0"
        assert (lse_c.permute(0, 2, 1)[dead] == 0).all().item(), f"{tag}: a row without a visible key must have LSE = 0"
    err = float((lse_c.double() - xl).abs().max())
    print(f"{tag}: LSE err {err:.3e}")
    assert err <= U.LSE_TOL, f"{tag}: LSE err {err}"
    d = out_c.shape[-1]
    parts = {}
    for name, sel in (("long", nvis >= U.PLAIN_SK_MIN), ("short", (nvis > 0) & (nvis < U.PLAIN_SK_MIN))):
        if sel.any():
            parts[name] = (out_c[sel].reshape(-1, d).numpy(), xo[sel].reshape(-1, d).numpy(), int(nvis[sel].min()))
    return parts


def assert_groups(parts_list, dtname, tag):
    """assert_close over the rows of one or several calls, per group, with sk = the fewest keys any row of the group sees"""
    for name in ("long", "short"):
        parts = [p[name] for p in parts_list if name in p]
        if not parts:
            continue
        got, want = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        raw = U.assert_close(got, want, dtname, f"tree O {tag} {name} rows", sk=min(p[2] for p in parts))
        print(f"{tag} {name} rows ({got.shape[0]} x {got.shape[1]}): {raw}")


def check(out, lse, xo, xl, nvis, dtname, tag):
    assert_groups([split_rows(out, lse, xo, xl, nvis, tag)], dtname, tag)


def tree_case(dt, d, sq, h, hk, gen, prefixes=PREFIXES, cap=CAP):
    """q, the cache holding the prefixes, and the draft tokens' k / v with K at 3 x the prefix's scale, so that the draft keys carry weight
    against a long prefix; the logical caches after the append"""
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
def test_tree_against_fp64(gpu, dtname, d, heads):
    """The draft tokens are appended by the call itself (k / v at cache_seqlens = the prefix lengths, one batch entry per prefix length).  Every
    call - five seqlen_q x three masks x three split counts - has its LSE asserted on its own; for O the rows of the calls of one seqlen_q and
    split count (the three masks) are asserted together, per group, as the sinks and soft-cap suites do."""
    dt = DT[dtname]
    h, hk = heads
    gen = torch.Generator().manual_seed(41000 + d + h)
    b = len(PREFIXES)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    tol = U.TOL[dtname]["mean_abs"]
    for sq in SQS:
        q, k, v, k_new, v_new, kl, vl = tree_case(dt, d, sq, h, hk, gen)
        lens = [p + sq for p in PREFIXES]
        s = scores64(q, kl)
        qg, kg, vg, kng, vng = (t.to(gpu) for t in (q, k, v, k_new, v_new))
        parts = {ns: [] for ns in SPLITS}
        masks = (("heap", heap_mask(sq)), ("forest", forest_mask(sq)), ("random", random_mask(sq, gen)))
        others = {}
        if sq >= 17:
            others = {"causal": exact(s, vl, visible(lens, sq, words_of(tri_mask(sq)).expand(b, sq), CAP))[0],
                      "all-visible": exact(s, vl, visible(lens, sq, torch.full((b, sq), -1, dtype=torch.int64), CAP))[0]}
        for mname, m in masks:
            tag = f"{dtname} d{d} h{h}/{hk} sq{sq} {mname}"
            words = words_of(m).expand(b, sq).contiguous()
            xo, xl, nvis = exact(s, vl, visible(lens, sq, words, CAP))
            assert int(nvis.min()) >= 1
            if sq >= 17:
                gaps = dict(others, transposed=exact(s, vl, visible(lens, sq, words_of(m.t()).expand(b, sq), CAP))[0])
                for oname, x in gaps.items():
                    gap = float((xo - x).abs().mean())
                    print(f"{tag}: mean |expectation - {oname} expectation| = {gap:.3e} ({gap / tol:.1f} x mean_abs tol)")
                    assert gap >= 4 * tol, f"{tag}: the case does not tell the mask from the {oname} one (gap {gap:.3e})"
            wg = words.to(gpu)
            for ns in SPLITS:
                out, lse = F.flash_attn_with_kvcache(qg, kg, vg, k=kng, v=vng, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, tree_mask=wg)
                assert out.shape == q.shape and out.dtype == dt and lse.shape == (b, h, sq) and lse.dtype == torch.float32
                parts[ns].append(split_rows(out, lse, xo, xl, nvis, f"{tag} splits={ns}"))
        assert _same(kg.cpu(), kl) and _same(vg.cpu(), vl), "the append wrote something else than the draft rows"
        for ns, pl in parts.items():
            assert_groups(pl, dtname, f"{dtname} d{d} h{h}/{hk} sq{sq} splits={ns}, the three masks")


# ---- 2. relations that hold to the bit -------------------------------------------------------------------------------------------------------

def _layouts(k, v, gen, gpu, P=16, seed=3):
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
def test_triangle_mask_is_the_causal_call_and_full_mask_the_plain_call(gpu, dtname, d):
    """out and lse, bit for bit, for num_splits 0, 1 and a forced 3: every seqlen_q and head combination, over the 16-bit and the 8-bit cache,
    contiguous and paged, with the draft tokens already in the cache and appended by the call; lengths below seqlen_q included (the first
    batch entries: the causal call's rows that see nothing are dead under the triangle mask as well)"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(42000 + d)
    lens = [0, 1, 3, 31, 33, 100, 777, 1064]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for sq in SQS:
        tri, full = words_of(tri_mask(sq)).expand(b, sq).contiguous().to(gpu), torch.full((b, sq), (1 << sq) - 1 if sq < 64 else -1, dtype=torch.int64, device=gpu)
        for h, hk in HEADS:
            k, v, q = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen), _rand((b, sq, h, d), dt, gen).to(gpu)
            for name, kk, vv, lkw in _layouts(k, v, gen, gpu):
                if (h, hk) != (32, 8) and name != "contiguous" and sq not in (5, 64):
                    continue                                # (every layout at two sizes for every head combination, and at all sizes for one)
                for ns in SPLITS:
                    kw = dict(cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, **lkw)
                    for words, causal in ((tri, True), (full, False)):
                        want = F.flash_attn_with_kvcache(q, kk, vv, causal=causal, **kw)
                        got = F.flash_attn_with_kvcache(q, kk, vv, tree_mask=words, **kw)
                        assert _same(got[0], want[0]) and _same(got[1], want[1]), (name, sq, h, hk, ns, causal)
            # with the append: cache_seqlens are the prefixes, the call brings the sq draft tokens
            k_new, v_new = _rand((b, sq, hk, d), dt, gen, 3.0).to(gpu), _rand((b, sq, hk, d), dt, gen).to(gpu)
            pre = torch.tensor([0, 1, 3, 31, 33, 100, 777, 1000], dtype=torch.int32, device=gpu)
            for ns in SPLITS:
                for words, causal in ((tri, True), (full, False)):
                    ka, va, kb, vb = k.to(gpu), v.to(gpu), k.to(gpu), v.to(gpu)
                    want = F.flash_attn_with_kvcache(q, ka, va, k=k_new, v=v_new, cache_seqlens=pre, causal=causal, num_splits=ns, return_softmax_lse=True)
                    got = F.flash_attn_with_kvcache(q, kb, vb, k=k_new, v=v_new, cache_seqlens=pre, num_splits=ns, return_softmax_lse=True, tree_mask=words)
                    assert _same(got[0], want[0]) and _same(got[1], want[1]) and _same(ka, kb) and _same(va, vb), ("append", sq, h, hk, ns, causal)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_is_contiguous_runs_are_identical_and_bits_from_sq_up_are_ignored(gpu, dtname, d):
    """paged == contiguous (pages of 16 and of 64 rows, the append going through the table), two runs of the same call, garbage in the bits at
    or above seqlen_q, and a strided mask tensor: all to the bit, 16-bit and 8-bit cache, every split count"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(43000 + d)
    b = len(PREFIXES)
    cs = torch.tensor(PREFIXES, dtype=torch.int32, device=gpu)
    for sq, (h, hk) in ((5, (6, 2)), (17, (32, 8)), (64, (16, 1)), (2, (8, 8))):
        q, k, v, k_new, v_new, _, _ = tree_case(dt, d, sq, h, hk, gen)
        qg, kng, vng = q.to(gpu), k_new.to(gpu), v_new.to(gpu)
        words = torch.stack([words_of(random_mask(sq, gen)) for _ in range(b)]).to(gpu)
        junk = torch.randint(-2**62, 2**62, (b, sq), generator=gen, dtype=torch.int64).to(gpu)
        high = words | ((junk << sq) if sq < 64 else 0)
        wide = torch.full((b, sq, 3), -1, dtype=torch.int64, device=gpu)
        wide[:, :, 1] = words
        for P in (16, 64):
            res = {}
            for name, kk, vv, lkw in _layouts(k, v, gen, gpu, P=P, seed=7 + P):
                for ns in SPLITS:
                    kw = dict(k=kng, v=vng, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, **lkw)
                    a = F.flash_attn_with_kvcache(qg, kk.clone(), vv.clone(), tree_mask=words, **kw)
                    for what, w in (("second run", words), ("high bits", high), ("strided", wide[:, :, 1])):
                        got = F.flash_attn_with_kvcache(qg, kk.clone(), vv.clone(), tree_mask=w, **kw)
                        assert _same(got[0], a[0]) and _same(got[1], a[1]), (what, name, P, sq, ns)
                    res[name, ns] = a
            for ns in SPLITS:
                for x, y in (("contiguous", "paged"), ("fp8", "fp8 paged")):
                    assert _same(res[x, ns][0], res[y, ns][0]) and _same(res[x, ns][1], res[y, ns][1]), (x, y, P, sq, ns)
        if sq > 1:      # (the mask matters: another one gives other bits)
            other = F.flash_attn_with_kvcache(qg, k.to(gpu), v.to(gpu), k=kng, v=vng, cache_seqlens=cs, return_softmax_lse=True, tree_mask=words ^ 1)
            base = F.flash_attn_with_kvcache(qg, k.to(gpu), v.to(gpu), k=kng, v=vng, cache_seqlens=cs, return_softmax_lse=True, tree_mask=words)
            assert not _same(other[0], base[0])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_sequence_of_a_ragged_tree_call_is_the_dense_tree_call_on_it_alone(gpu, dtname, d):
    """mixed sq_i with 0, 1 and 64, num_splits = 1 and a forced 3 (the existing split rule); both layouts, 16-bit and 8-bit, with and without an
    append; packed rows past cu_seqlens_q[-1] carry a NaN query and a garbage mask word and are never read"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(44000 + d)
    sqs = [1, 0, 5, 64, 17, 2, 64, 1]
    lens = [1, 5, 0, 64, 300, 777, 1000, 33]             # the prefixes when the call appends, the lengths when it does not
    b, total, extra = len(sqs), sum(sqs), 3
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    words = torch.cat([words_of(random_mask(s, gen) if i % 2 else heap_mask(s)) for i, s in enumerate(sqs) if s] + [torch.full((extra,), -1, dtype=torch.int64)]).to(gpu)
    for h, hk in ((32, 8), (6, 2), (16, 1)):
        k, v = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen)
        q = _rand((total + extra, h, d), dt, gen).to(gpu)
        q[total:] = NAN
        k_new, v_new = _rand((total, hk, d), dt, gen, 3.0).to(gpu), _rand((total, hk, d), dt, gen).to(gpu)
        for name, kk, vv, lkw in _layouts(k, v, gen, gpu, P=64, seed=5)[:3]:
            for ns, append in ((1, False), (1, True), (3, True), (3, False)):
                kw = dict(num_splits=ns, return_softmax_lse=True)
                kr, vr = kk.clone(), vv.clone()
                rag = dict(k=k_new, v=v_new, cu_seqlens_k_new=cu) if append else dict()
                out, lse = F.flash_attn_with_kvcache(q, kr, vr, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=64, tree_mask=words, **rag, **lkw, **kw)
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
                    od, ld = F.flash_attn_with_kvcache(q[c0:c0 + s][None], kd if paged else kd[i:i + 1], vd if paged else vd[i:i + 1], cache_seqlens=cs[i:i + 1],
                                                       tree_mask=words[c0:c0 + s][None], **one, **kw)
                    assert _same(out[c0:c0 + s], od[0]) and _same(lse[:, c0:c0 + s], ld[0]), (name, h, hk, ns, append, i)
                if append:
                    assert _same(kr, kd) and _same(vr, vd), (name, "cache bytes", ns)


# ---- 3. meaning ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", SPLITS)
def test_a_node_sees_the_prefix_its_ancestors_and_itself(gpu, dtname, num_splits):
    """a branching tree appended through k / v, its words from tree_mask_from_parents: the row of node t equals, to the project's tolerances,
    the seqlen_q = 1 call over a cache that holds the prefix followed by t's ancestors and t itself"""
    dt = DT[dtname]
    d, h, hk, sq = 128, 16, 4, 13
    parents = [-1, 0, 0, 1, 1, 2, 5, 5, 3, 8, 0, 10, 6]
    prefixes = [0, 33, 700]
    b = len(prefixes)
    gen = torch.Generator().manual_seed(45000)
    q, k, v, k_new, v_new, _, _ = tree_case(dt, d, sq, h, hk, gen, prefixes=prefixes)
    words = F.tree_mask_from_parents(torch.tensor(parents)).expand(b, sq).contiguous()
    cs = torch.tensor(prefixes, dtype=torch.int32, device=gpu)
    out, lse = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=cs, num_splits=num_splits,
                                         return_softmax_lse=True, tree_mask=words.to(gpu))
    tol = U.TOL[dtname]
    for t in range(sq):
        path, a = [], t
        while a >= 0:
            path.append(a)
            a = parents[a]
        path = sorted(path)
        kc, vc = k.clone(), v.clone()
        for i, pre in enumerate(prefixes):
            kc[i, pre:pre + len(path)], vc[i, pre:pre + len(path)] = k_new[i, path], v_new[i, path]
        one = F.flash_attn_with_kvcache(q[:, t:t + 1].to(gpu), kc.to(gpu), vc.to(gpu), cache_seqlens=cs + len(path), num_splits=num_splits, return_softmax_lse=True)
        m = U.error_metrics(out[:, t].float().cpu().numpy(), one[0][:, 0].float().cpu().numpy())
        assert m["max_abs"] <= tol["max_abs"] and m["mean_abs"] <= tol["mean_abs"], (t, m)
        assert float((lse[:, :, t] - one[1][:, :, 0]).abs().max()) <= U.LSE_TOL, t


# ---- 4. masked keys do not leak ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_masked_draft_keys_do_not_leak(gpu, dtname, d):
    """draft keys that no row sees hold K and V of magnitude 1e4: out and lse still meet the tolerances of the value test; with a NaN K row
    there instead (V finite) every row stays finite and keeps the bits of the clean call"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(46000 + d)
    prefixes = [0, 33, 1000]
    b = len(prefixes)
    cs = torch.tensor(prefixes, dtype=torch.int32, device=gpu)
    for sq, (h, hk), hidden in ((17, (6, 2), (3, 11, 16)), (64, (8, 8), (0, 31, 32, 63)), (5, (32, 8), (4,))):
        q, k, v, k_new, v_new, kl, vl = tree_case(dt, d, sq, h, hk, gen, prefixes=prefixes)
        m = random_mask(sq, gen)
        m[:, list(hidden)] = False                          # (the hidden tokens' own rows lose their diagonal: with a prefix they still see it)
        words = words_of(m).expand(b, sq).contiguous()
        lens = [p + sq for p in prefixes]
        xo, xl, nvis = exact(scores64(q, kl), vl, visible(lens, sq, words, CAP))
        big_k, big_v, nan_k = k_new.clone(), v_new.clone(), k_new.clone()
        for u in hidden:
            big_k[:, u] = torch.where(torch.rand(b, hk, d, generator=gen) < 0.5, 1e4, -1e4).to(dt)
            big_v[:, u] = torch.where(torch.rand(b, hk, d, generator=gen) < 0.5, 1e4, -1e4).to(dt)
            nan_k[:, u] = NAN
        for ns in SPLITS:
            kw = dict(cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, tree_mask=words.to(gpu))
            clean = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), k=k_new.to(gpu), v=v_new.to(gpu), **kw)
            check(clean[0], clean[1], xo, xl, nvis, dtname, f"clean {dtname} d{d} sq{sq} splits={ns}")
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), k=big_k.to(gpu), v=big_v.to(gpu), **kw)
            check(out, lse, xo, xl, nvis, dtname, f"1e4 in masked keys {dtname} d{d} sq{sq} splits={ns}")
            assert _same(out, clean[0]) and _same(lse, clean[1])
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), k=nan_k.to(gpu), v=v_new.to(gpu), **kw)
            assert torch.isfinite(out).all().item() and torch.isfinite(lse).all().item(), (sq, ns)
            assert _same(out, clean[0]) and _same(lse, clean[1])


# ---- 5. short sequences ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_lengths_below_seqlen_q_and_an_append_into_an_empty_cache(gpu, dtname, d):
    """cache_seqlens = 0 with an append: L = sq, the first draft token is key 0 and bit u is key u.  L < sq without an append: key j is bit
    j + sq - L, the bits below that belong to keys that do not exist.  Rows whose word is empty see nothing: O = 0, LSE = 0 exactly."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(47000 + d)
    for sq, (h, hk) in ((5, (6, 2)), (17, (32, 8)), (64, (16, 1)), (2, (8, 8)), (1, (8, 8))):
        m = random_mask(sq, gen)
        m[0] = False                                        # a dead row
        if sq > 2:
            m[sq - 2] = False
        # (a) the append into an empty cache
        b = 3
        k, v, q = _rand((b, 128, hk, d), dt, gen), _rand((b, 128, hk, d), dt, gen), _rand((b, sq, h, d), dt, gen)
        k_new, v_new = _rand((b, sq, hk, d), dt, gen, 3.0), _rand((b, sq, hk, d), dt, gen)
        words = torch.stack([words_of(m), words_of(heap_mask(sq)), words_of(m.t())])
        kl, vl = k.clone(), v.clone()
        kl[:, :sq], vl[:, :sq] = k_new, v_new
        xo, xl, nvis = exact(scores64(q, kl), vl, visible([sq] * b, sq, words, 128))
        assert int((nvis == 0).sum()) > 0
        assert torch.equal(visible([sq] * b, sq, words, 128)[0, :, :sq], m)        # the rule, spelt out: row t sees key j iff bit j
        for ns in SPLITS:
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=0, num_splits=ns,
                                                 return_softmax_lse=True, tree_mask=words.to(gpu))
            check(out, lse, xo, xl, nvis, dtname, f"append into an empty cache {dtname} d{d} sq{sq} splits={ns}")
        # (b) fewer keys than query rows
        lens = sorted({0, 1, sq // 2, sq - 1})
        b = len(lens)
        k, v, q = _rand((b, 128, hk, d), dt, gen, 3.0), _rand((b, 128, hk, d), dt, gen), _rand((b, sq, h, d), dt, gen)
        full = random_mask(sq, gen)
        words = words_of(full).expand(b, sq).contiguous()
        xo, xl, nvis = exact(scores64(q, k), v, visible(lens, sq, words, 128))
        for ns in SPLITS:
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=gpu), num_splits=ns,
                                                 return_softmax_lse=True, tree_mask=words.to(gpu))
            check(out, lse, xo, xl, nvis, dtname, f"L < sq {dtname} d{d} sq{sq} splits={ns}")
            assert (out[0] == 0).all().item() and (lse[0] == 0).all().item()          # L = 0


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------------------

def test_captured_tree_call_replays_with_new_mask_words_and_new_lengths(gpu):
    """one captured call (a single chain of launches on one stream); the mask words and cache_seqlens are rewritten in place before the replay,
    which must give the bits of the eager call on the new values"""
    dt, d, h, hk, b, sq = torch.float16, 64, 32, 8, 2, 8
    gen = torch.Generator().manual_seed(48000)
    k, v = _rand((b, 4096, hk, d), dt, gen, 2.0).to(gpu), _rand((b, 4096, hk, d), dt, gen).to(gpu)
    q = _rand((b, sq, h, d), dt, gen).to(gpu)
    cs = torch.tensor([100, 4000], dtype=torch.int32, device=gpu)
    words = words_of(heap_mask(sq)).expand(b, sq).contiguous().to(gpu)
    kw = dict(cache_seqlens=cs, return_softmax_lse=True, tree_mask=words)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, k, v, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, k, v, **kw)
    first = (out_g.clone(), lse_g.clone())
    lens = [2500, 5]
    new_words = torch.stack([words_of(random_mask(sq, gen)), words_of(forest_mask(sq))])
    cs.copy_(torch.tensor(lens, dtype=torch.int32))
    words.copy_(new_words)
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = F.flash_attn_with_kvcache(q, k, v, **kw)
    assert _same(out_g, out_e) and _same(lse_g, lse_e)
    assert not _same(out_g, first[0])
    xo, xl, nvis = exact(scores64(q, k), v, visible(lens, sq, new_words, 4096))
    check(out_g, lse_g, xo, xl, nvis, "fp16", "graph replay")


# ---- 7. bit 63 ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", SPLITS)
def test_row_63_sees_key_base_plus_63_iff_the_sign_bit_is_set(gpu, dtname, num_splits):
    dt = DT[dtname]
    d, h, hk, sq = 64, 6, 2, 64
    prefixes = [0, 33, 1000]
    b = len(prefixes)
    gen = torch.Generator().manual_seed(49000)
    q, k, v, k_new, v_new, kl, vl = tree_case(dt, d, sq, h, hk, gen, prefixes=prefixes)
    m = heap_mask(sq)
    m[63, 63] = False
    off, on = words_of(m).expand(b, sq).contiguous(), None
    m[63, 63] = True
    on = words_of(m).expand(b, sq).contiguous()
    assert off[0, 63].item() > 0 > on[0, 63].item() and (on[0, 63].item() ^ off[0, 63].item()) == -(1 << 63) and torch.equal(on[:, :63], off[:, :63])
    lens = [p + sq for p in prefixes]
    s = scores64(q, kl)
    res = {}
    for name, words in (("on", on), ("off", off)):
        xo, xl, nvis = exact(s, vl, visible(lens, sq, words, CAP))
        res[name] = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=torch.tensor(prefixes, dtype=torch.int32, device=gpu),
                                              num_splits=num_splits, return_softmax_lse=True, tree_mask=words.to(gpu))
        check(res[name][0], res[name][1], xo, xl, nvis, dtname, f"bit 63 {name} {dtname} splits={num_splits}")
        res[name + " x"] = xo
    # the two expectations are far apart in row 63 (the draft keys are heavy), and equal elsewhere; so are the results, to the bit elsewhere
    gap = float((res["on x"][:, 63] - res["off x"][:, 63]).abs().mean())
    assert gap >= 4 * U.TOL[dtname]["mean_abs"], gap
    assert _same(res["on"][0][:, :63], res["off"][0][:, :63]) and _same(res["on"][1][:, :, :63], res["off"][1][:, :, :63])
    assert not _same(res["on"][0][:, 63], res["off"][0][:, 63])
