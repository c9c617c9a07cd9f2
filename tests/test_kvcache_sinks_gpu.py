"""GPU: attention sinks on the decode path (flash_attn_with_kvcache(..., sinks=), fa_kvcache_options_v6).

Expectations: neither the C oracle nor the reference has sinks, so the value tests compare with fp64 math written here - the masked softmax of
test_kvcache_softcap_gpu.exact with the sink term added to the denominator and to the LSE - through _util.assert_close without an oracle (its
"plain" rule from 64 keys on, its "floor" rule below) and _util.LSE_TOL: the project's numbers, no new tolerance.  The rows are asserted in the
two groups those rules make (rows that see at least _util.PLAIN_SK_MIN keys, rows that see fewer), as the soft-cap suite does; rows that see no
key are asserted exactly: O = 0, LSE = float32(sinks[h]).  Every value case first asserts, on the fp64 expectation alone, that it is far (4 x
the dtype's mean_abs tolerance) from the expectation without sinks and from the expectation with the sinks rolled by one head, so a kernel
that ignored the argument or mapped rows to the wrong head could not pass.  Everything else is a relation that must hold to the bit."""

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from test_kvcache_fp8_gpu import _descale, deq, quantise
from test_kvcache_fp8_gpu import _page as _page8
from test_kvcache_rotary_cpu import rotate_ref
from test_kvcache_rotary_gpu import positions, tables
from test_kvcache_softcap_gpu import CAP, DT, _rand, _same, default_scale
from test_kvcache_window_gpu import _bounds, _page

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def make_sinks(h):
    """float32 (h,): distinct per head, neighbours far apart (a roll by one head moves every head's sink by 1.5 or more), between 2 and 8.5 -
    against the logsumexp of N(0, 1) scores over 1 .. 1000 keys (about 0 .. 7.4) the sink takes from under a percent to nearly all of the mass"""
    i = torch.arange(h)
    return (2.0 + 4.5 * ((i * 5) % 8).float() / 8.0 + 0.03 * i.float()).to(torch.float32)


def exact(q, k, v, lens, sinks=None, scale=None, window=(-1, -1), causal=False):
    """fp64: scores (q . k) * scale, masked (length, causal, window); softmax over what is left with exp(sinks[h] - M) added to the denominator,
    M = max(row max, sinks[h]); the LSE includes the sink.  q (b, sq, h, d), k / v the logical caches (b, capacity, hk, d) (any float dtype: a
    dequantised 8-bit cache comes as fp32), sinks (h,) or None (= -inf everywhere).  Returns O (b, sq, h, d), LSE (b, h, sq) - rows without a
    visible key: O = 0 and LSE = sinks[h], or 0 under a sink of -inf - and the visible keys per row (b, sq)."""
    b, sq, h, d = q.shape
    capacity, hk = k.shape[1], k.shape[2]
    qd, kd, vd = (t.detach().cpu().double() for t in (q, k, v))
    kd, vd = kd.repeat_interleave(h // hk, dim=2), vd.repeat_interleave(h // hk, dim=2)
    s = torch.einsum("bthd,bjhd->bhtj", qd, kd) * (default_scale(d) if scale is None else float(np.float32(scale)))
    mask = torch.zeros(b, 1, sq, capacity, dtype=torch.bool)
    nvis = torch.zeros(b, sq, dtype=torch.long)
    for i, L in enumerate(lens):
        for t in range(sq):
            lo, hi = _bounds(L, sq, t, window, causal)
            mask[i, 0, t, lo:hi] = True
            nvis[i, t] = hi - lo
    s = s.masked_fill(~mask, -INF)
    sk = (torch.full((h,), -INF, dtype=torch.float64) if sinks is None else sinks.detach().cpu().double()).view(1, h, 1, 1)
    m = torch.maximum(s.amax(-1, keepdim=True), sk)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True) + torch.exp(sk - m)
    live = den > 0
    w = torch.where(live, p / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(p))
    # (a masked key has weight exactly 0: keep a non-finite V row it holds out of the product)
    o = torch.einsum("bhtj,bjhd->bthd", w, torch.where(mask.any(2)[:, 0, :, None, None], vd, torch.zeros_like(vd)))
    lse = torch.where(live, m + torch.log(torch.where(live, den, torch.ones_like(den))), torch.zeros_like(den)).squeeze(-1)
    return o, lse, nvis


def split_rows(out, lse, xo, xl, nvis, sinks, tag):
    """out (b, sq, h, d) / lse (b, h, sq) of one call against the fp64 expectation, the part that is asserted row by row: rows without a visible
    key exactly O = 0 and LSE = float32(sinks[h]) (0 under -inf), every LSE under LSE_TOL.  Returns the rows that see a key in the two groups
    of _util.check_mean_rel's rules, {"long" / "short": (got (n, d), expected (n, d), the fewest keys a row of the group sees)}."""
    out_c, lse_c = out.detach().float().cpu(), lse.detach().cpu()
    assert torch.isfinite(out_c).all().item() and torch.isfinite(lse_c).all().item(), f"{tag}: non-finite values"
    dead = nvis == 0
    if dead.any():
        s32 = sinks.detach().cpu().to(torch.float32)
        want = torch.where(torch.isinf(s32), torch.zeros_like(s32), s32)
        got = lse_c.permute(0, 2, 1)[dead]
        assert (out_c[dead] == 0).all().item(), f"{tag}: a row without a visible key must be O = 0"
        assert torch.equal(got, want.expand_as(got)), f"{tag}: a row without a visible key must have LSE = float32(sinks[h])"
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
        raw = U.assert_close(got, want, dtname, f"sinks O {tag} {name} rows", sk=min(p[2] for p in parts))
        print(f"{tag} {name} rows ({got.shape[0]} x {got.shape[1]}): {raw}")


def check(out, lse, xo, xl, nvis, sinks, dtname, tag):
    assert_groups([split_rows(out, lse, xo, xl, nvis, sinks, tag)], dtname, tag)


def assert_tells_sinks_apart(xo, q, k, v, lens, sinks, dtname, tag, **kw):
    """on the fp64 expectation alone: mean |difference| to the expectation without sinks, and to the one with the sinks rolled by one head, is
    at least 4 x the dtype's mean_abs tolerance.  Returns the LSE of the expectation without sinks."""
    x0, xl0, _ = exact(q, k, v, lens, **kw)
    xr, _, _ = exact(q, k, v, lens, sinks=torch.roll(sinks, 1), **kw)
    g0, gr = float((xo - x0).abs().mean()), float((xo - xr).abs().mean())
    tol = U.TOL[dtname]["mean_abs"]
    print(f"{tag}: mean |expectation - no sinks| = {g0:.3e} ({g0 / tol:.1f} x mean_abs tol), - rolled sinks| = {gr:.3e} ({gr / tol:.1f} x)")
    assert g0 >= 4 * tol, f"{tag}: the case does not tell sinks from no sinks (gap {g0:.3e})"
    assert gr >= 4 * tol, f"{tag}: the case does not tell a head's sink from its neighbour's (gap {gr:.3e})"
    return xl0


COMBOS = [(1, 8, 8), (3, 32, 8), (17, 16, 2), (3, 16, 1), (1, 64, 8)]        # (seqlen_q, h, h_k): ratios 1, 4, 8, MQA with 3 rows, the gpt-oss heads
LENS = [0, 1, 31, 33, 64, 100, 777, 1000]


# ---- 4. values --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_sinks_against_fp64(gpu, dtname, d, causal):
    """Every call of the grid - the five head / seqlen_q combinations x three split counts - has its dead rows (O = 0, LSE = the sink, exactly)
    and its LSE asserted on its own.  For O the rows of the five calls of one split count are asserted together, per group, as the soft-cap
    suite does and for its reason: the relative metric over the few rows of one decode call hangs on single elements that lie next to zero."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(21000 + d + int(causal))
    b = len(LENS)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    parts = {ns: [] for ns in (1, 0, 5)}
    for sq, h, hk in COMBOS:
        k, v, q = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen), _rand((b, sq, h, d), dt, gen)
        sinks = make_sinks(h)
        tag = f"{dtname} d{d} sq{sq} h{h}/{hk} causal={causal}"
        xo, xl, nvis = exact(q, k, v, LENS, sinks=sinks, causal=causal)
        xl0 = assert_tells_sinks_apart(xo, q, k, v, LENS, sinks, dtname, tag, causal=causal)
        # the share of the sink, from the two LSEs: a few percent to most of the mass across lengths and heads
        share = (1.0 - torch.exp(xl0 - xl)).permute(0, 2, 1)[nvis > 0]          # (rows that see a key: a dead row has no share to speak of)
        assert float(share.min()) < 0.05 and float(share.max()) > 0.9, (tag, float(share.min()), float(share.max()))
        qg, kg, vg, sg = q.to(gpu), k.to(gpu), v.to(gpu), sinks.to(gpu)
        for ns in parts:
            out, lse = F.flash_attn_with_kvcache(qg, kg, vg, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, sinks=sg)
            assert out.shape == q.shape and out.dtype == dt and lse.shape == (b, h, sq) and lse.dtype == torch.float32
            parts[ns].append(split_rows(out, lse, xo, xl, nvis, sinks, f"{tag} splits={ns}"))
    for ns, pl in parts.items():
        assert_groups(pl, dtname, f"{dtname} d{d} causal={causal} splits={ns}, the five calls")


# ---- 5. range -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", [1, 5])
def test_sinks_far_above_and_far_below_the_scores(gpu, dtname, num_splits):
    """+60: the sink holds all the mass - out is 0 to 1e-20, lse is the sink, nothing overflows; -60: the call without sinks"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(22000)
    d, sq, h, hk, lens = 64, 3, 16, 2, [0, 1, 33, 100, 1000]
    b = len(lens)
    k, v, q = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen), _rand((b, sq, h, d), dt, gen)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True)
    qg, kg, vg = q.to(gpu), k.to(gpu), v.to(gpu)
    plain = F.flash_attn_with_kvcache(qg, kg, vg, **kw)
    for value in (60.0, -60.0):
        sinks = torch.full((h,), value) + 0.01 * torch.arange(h)
        out, lse = F.flash_attn_with_kvcache(qg, kg, vg, sinks=sinks.to(gpu), **kw)
        assert torch.isfinite(out).all().item() and torch.isfinite(lse).all().item(), value
        xo, xl, nvis = exact(q, k, v, lens, sinks=sinks, causal=True)
        if value > 0:
            assert float(out.float().abs().max()) <= 1e-20, float(out.float().abs().max())
            err = float((lse.cpu().double() - xl).abs().max())
            assert err <= U.LSE_TOL, err
            assert float((lse.cpu() - sinks.view(1, h, 1)).abs().max()) <= U.LSE_TOL
        else:
            check(out, lse, xo, xl, nvis, sinks, dtname, f"sinks -60 {dtname} splits={num_splits}")
            live = (nvis > 0).to(gpu)
            got, want = out[live].float().cpu().numpy(), plain[0][live].float().cpu().numpy()
            m = U.error_metrics(got, want)
            print(f"sinks -60 against the call without sinks: {m}")
            assert m["max_abs"] <= U.TOL[dtname]["max_abs"] and m["mean_abs"] <= U.TOL[dtname]["mean_abs"], m
            assert float((lse.permute(0, 2, 1)[live] - plain[1].permute(0, 2, 1)[live]).abs().max()) <= U.LSE_TOL


# ---- 6. relations that hold to the bit -----------------------------------------------------------------------------------------------------

def _dense_case(gpu, dt, d, gen, sq=3, h=32, hk=8, lens=(0, 1, 31, 33, 100, 777, 1000)):
    b = len(lens)
    k, v = _rand((b, CAP, hk, d), dt, gen).to(gpu), _rand((b, CAP, hk, d), dt, gen).to(gpu)
    q = _rand((b, sq, h, d), dt, gen).to(gpu)
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device=gpu)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_all_minus_inf_sinks_are_the_call_without_sinks(gpu, dtname, d):
    """out and lse, for num_splits 1, 0 and 5: 16-bit and 8-bit cache, contiguous and paged, plain, causal and windowed, dense and ragged; the
    dead rows of the empty sequence stay O = 0, LSE = 0"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(23000 + d)
    q, k, v, cs = _dense_case(gpu, dt, d, gen)
    b, sq, h, _ = q.shape
    hk = k.shape[2]
    off = torch.full((h,), -INF, device=gpu)
    kp, vp, table, _ = _page(k, v, 64, 5)
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
    kp8, vp8, table8 = _page8(k8, v8, 16, 7)
    sqs = [1, 0, 5, 3, 16, 1, 2]
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    qr = _rand((sum(sqs), h, d), dt, gen).to(gpu)
    layouts = [("contiguous", q, k, v, dict()), ("paged", q, kp, vp, dict(block_table=table)), ("fp8", q, k8, v8, dict(k_descale=kds, v_descale=vds)),
               ("fp8 paged", q, kp8, vp8, dict(block_table=table8, k_descale=kds, v_descale=vds)), ("ragged", qr, k, v, dict(cu_seqlens_q=cu, max_seqlen_q=16))]
    for name, qq, kk, vv, lkw in layouts:
        for causal, window in ((False, (-1, -1)), (True, (-1, -1)), (True, (127, 0)), (False, (7, 3))):
            for ns in (1, 0, 5):
                kw = dict(cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, **lkw)
                want = F.flash_attn_with_kvcache(qq, kk, vv, **kw)
                got = F.flash_attn_with_kvcache(qq, kk, vv, sinks=off, **kw)
                assert _same(got[0], want[0]) and _same(got[1], want[1]), (name, causal, window, ns)
                if name != "ragged":
                    assert (got[0][0] == 0).all().item() and (got[1][0] == 0).all().item()


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_sink_paged_call_gives_the_bits_of_the_contiguous_one_and_runs_are_identical(gpu, dtname, d):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(24000 + d)
    q, k, v, cs = _dense_case(gpu, dt, d, gen)
    b, h, hk = q.shape[0], q.shape[2], k.shape[2]
    sinks = make_sinks(h).to(gpu)
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
    for P in (16, 256):
        kp, vp, table, _ = _page(k, v, P, 11 + P)
        kp8, vp8, table8 = _page8(k8, v8, P, 13 + P)
        for causal, window in ((False, (-1, -1)), (True, (-1, -1)), (True, (127, 0))):
            for ns in (1, 0, 5):
                kw = dict(cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, sinks=sinks)
                a = F.flash_attn_with_kvcache(q, k, v, **kw)
                a2 = F.flash_attn_with_kvcache(q, k, v, **kw)
                p = F.flash_attn_with_kvcache(q, kp, vp, block_table=table, **kw)
                assert _same(a[0], a2[0]) and _same(a[1], a2[1]), ("not deterministic", P, causal, window, ns)
                assert _same(a[0], p[0]) and _same(a[1], p[1]), ("paged", P, causal, window, ns)
                a8 = F.flash_attn_with_kvcache(q, k8, v8, k_descale=kds, v_descale=vds, **kw)
                a82 = F.flash_attn_with_kvcache(q, k8, v8, k_descale=kds, v_descale=vds, **kw)
                p8 = F.flash_attn_with_kvcache(q, kp8, vp8, block_table=table8, k_descale=kds, v_descale=vds, **kw)
                assert _same(a8[0], a82[0]) and _same(a8[1], a82[1]), ("fp8 not deterministic", P, causal, window, ns)
                assert _same(a8[0], p8[0]) and _same(a8[1], p8[1]), ("fp8 paged", P, causal, window, ns)
                assert not _same(a[0], F.flash_attn_with_kvcache(q, k, v, **dict(kw, sinks=None))[0])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", [1, 0, 5])
def test_a_heads_sink_is_its_own_and_the_tensor_may_be_narrow_or_strided(gpu, dtname, num_splits):
    """changing one head's sink changes that head's bits and no other head's; a sinks tensor of q's dtype gives the bits of its float32
    widening; a strided view gives the bits of its contiguous copy"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(25000)
    q, k, v, cs = _dense_case(gpu, dt, 64, gen, sq=3, h=32, hk=4)
    h = q.shape[2]
    sinks = make_sinks(h).to(gpu)
    kw = dict(cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True)
    base = F.flash_attn_with_kvcache(q, k, v, sinks=sinks, **kw)
    for hh in (0, 5, 13, 31):                                 # (first and last head of a KV head's group, and two inside)
        s2 = sinks.clone()
        s2[hh] += 1.0
        got = F.flash_attn_with_kvcache(q, k, v, sinks=s2, **kw)
        others = [i for i in range(h) if i != hh]
        assert _same(got[0][:, :, others], base[0][:, :, others]) and _same(got[1][:, others], base[1][:, others]), hh
        assert not _same(got[0][:, :, hh], base[0][:, :, hh]) and not _same(got[1][:, hh], base[1][:, hh]), hh
    narrow = sinks.to(dt)
    a, bb = F.flash_attn_with_kvcache(q, k, v, sinks=narrow, **kw), F.flash_attn_with_kvcache(q, k, v, sinks=narrow.float(), **kw)
    assert _same(a[0], bb[0]) and _same(a[1], bb[1])
    wide = torch.full((h, 3), NAN, device=gpu)
    wide[:, 1] = sinks
    c = F.flash_attn_with_kvcache(q, k, v, sinks=wide[:, 1], **kw)
    assert wide[:, 1].stride(0) == 3 and _same(c[0], base[0]) and _same(c[1], base[1])
    rev = torch.flip(sinks, (0,)).contiguous()
    e = F.flash_attn_with_kvcache(q, k, v, sinks=torch.cat([rev, rev])[:h], **kw)
    assert not _same(e[0], base[0])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_sequence_of_a_ragged_sink_call_is_the_dense_sink_call_on_it_alone(gpu, dtname, d):
    """num_splits = 1 and a forced 3 (without a left-bounded window, the existing split rule); both layouts, 16-bit and 8-bit, with an append"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(26000 + d)
    sqs = [1, 0, 3, 17, 1, 3, 17, 1]
    lens = [1, 5, 0, 64, 65, 777, 900, 300]
    sns = [1, 0, 3, 17, 0, 2, 17, 1]
    b, total = len(sqs), sum(sqs)
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    cun = torch.tensor([0] + list(np.cumsum(sns)), dtype=torch.int32, device=gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for h, hk in ((32, 8), (64, 8), (16, 1)):
        sinks = make_sinks(h).to(gpu)
        k, v = _rand((b, CAP, hk, d), dt, gen).to(gpu), _rand((b, CAP, hk, d), dt, gen).to(gpu)
        q = _rand((total, h, d), dt, gen).to(gpu)
        k_new, v_new = _rand((sum(sns), hk, d), dt, gen).to(gpu), _rand((sum(sns), hk, d), dt, gen).to(gpu)
        kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
        k8, v8 = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
        kp, vp, table, _ = _page(k, v, 64, 3)
        layouts = [("contiguous", k, v, dict()), ("paged", kp, vp, dict(block_table=table)), ("fp8", k8, v8, dict(k_descale=kds, v_descale=vds))]
        for name, kk, vv, lkw in layouts:
            for causal, window, ns, append in ((False, (-1, -1), 1, False), (True, (-1, -1), 1, True), (True, (-1, -1), 3, False), (False, (-1, 2), 3, True),
                                               (True, (127, 0), 1, False)):
                kw = dict(causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, sinks=sinks)
                kr, vr = kk.clone(), vv.clone()
                rag = dict(k=k_new, v=v_new, cu_seqlens_k_new=cun) if append else dict()
                out, lse = F.flash_attn_with_kvcache(q, kr, vr, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=max(sqs), **rag, **lkw, **kw)
                assert out.shape == q.shape and lse.shape == (h, total)
                kd, vd = kk.clone(), vv.clone()
                paged = "block_table" in lkw
                for i, s in enumerate(sqs):
                    c0, n0 = sum(sqs[:i]), sum(sns[:i])
                    one = {key: val[i:i + 1] for key, val in lkw.items()}
                    if append and sns[i]:
                        one.update(k=k_new[n0:n0 + sns[i]][None], v=v_new[n0:n0 + sns[i]][None])
                    if s == 0:
                        continue
                    od, ld = F.flash_attn_with_kvcache(q[c0:c0 + s][None], kd if paged else kd[i:i + 1], vd if paged else vd[i:i + 1], cache_seqlens=cs[i:i + 1], **one, **kw)
                    assert _same(out[c0:c0 + s], od[0]) and _same(lse[:, c0:c0 + s], ld[0]), (name, h, hk, causal, window, ns, append, i)
                if append:          # (sequences without query rows append nothing in this case: sns follows sqs there)
                    assert _same(kr, kd) and _same(vr, vd), (name, "cache bytes", causal, window, ns)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("fp8", [False, True])
def test_rotary_with_sinks_is_the_sink_call_on_rotated_inputs(gpu, dtname, fp8):
    dt = DT[dtname]
    d, h, hk, sn, lens = 128, 16, 4, 3, [0, 5, 100, 700]
    b = len(lens)
    gen = torch.Generator().manual_seed(27000 + int(fp8))
    cos, sin = tables(CAP, 64, dt)
    k0, v0 = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen)
    q, k_new, v_new = _rand((b, sn, h, d), dt, gen), _rand((b, sn, hk, d), dt, gen), _rand((b, sn, hk, d), dt, gen)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, return_softmax_lse=True, sinks=make_sinks(h).to(gpu))
    if fp8:
        kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
        k0, v0 = quantise(k0, kds), quantise(v0, vds)
        kw.update(k_descale=kds, v_descale=vds)
    for causal, inter, ns in ((True, False, 1), (False, True, 4), (True, True, 0)):
        q_rot = rotate_ref(q, cos, sin, positions(lens, sn, causal, CAP), inter)
        k_rot = rotate_ref(k_new, cos, sin, positions(lens, sn, True, CAP), inter)
        ka, va, kb, vb = k0.to(gpu), v0.to(gpu), k0.to(gpu), v0.to(gpu)
        r = F.flash_attn_with_kvcache(q.to(gpu), ka, va, k=k_new.to(gpu), v=v_new.to(gpu), causal=causal, num_splits=ns, rotary_cos=cos.to(gpu), rotary_sin=sin.to(gpu),
                                      rotary_interleaved=inter, **kw)
        p = F.flash_attn_with_kvcache(q_rot.to(gpu), kb, vb, k=k_rot.to(gpu), v=v_new.to(gpu), causal=causal, num_splits=ns, **kw)
        assert _same(r[0], p[0]) and _same(r[1], p[1]) and _same(ka, kb) and _same(va, vb), (causal, inter, ns)
        assert not _same(r[0], F.flash_attn_with_kvcache(q_rot.to(gpu), kb, vb, causal=causal, num_splits=ns, **dict(kw, sinks=None))[0])


# ---- 7. FP8 cache, 8. windows ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_fp8_cache_with_sinks_against_fp64_on_the_dequantised_cache(gpu, dtname, d):
    """an 8-bit cache under per-(batch, head) descales: k_descale scales the scores and not the sink, v_descale stays in the final normalisation"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(28000 + d)
    lens, sq, h, hk = [0, 1, 31, 64, 333, 1000], 3, 32, 4
    b = len(lens)
    sinks = make_sinks(h)
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8 = quantise(torch.randn(b, CAP, hk, d, generator=gen), kds).to(gpu)
    v8 = quantise(torch.randn(b, CAP, hk, d, generator=gen), vds).to(gpu)
    q = _rand((b, sq, h, d), dt, gen)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for causal in (False, True):
        xo, xl, nvis = exact(q, deq(k8, kds), deq(v8, vds), lens, sinks=sinks, causal=causal)
        assert_tells_sinks_apart(xo, q, deq(k8, kds), deq(v8, vds), lens, sinks, dtname, f"fp8 {dtname} d{d}", causal=causal)
        for ns in (1, 0, 5):
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k8, v8, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, k_descale=kds, v_descale=vds,
                                                 sinks=sinks.to(gpu))
            check(out, lse, xo, xl, nvis, sinks, dtname, f"fp8 {dtname} d{d} causal={causal} splits={ns}")


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_window_with_sinks_against_fp64(gpu, dtname, d):
    """the gpt-oss window (127, 0) under causal, and (7, 3), whose rows near the start of a short sequence see no key at all: O = 0, LSE = the sink"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(29000 + d)
    lens, sq, h, hk = [0, 1, 5, 31, 100, 777, 1000], 17, 16, 2
    b = len(lens)
    sinks = make_sinks(h)
    k, v, q = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen), _rand((b, sq, h, d), dt, gen)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for window, causal in (((127, 0), True), ((7, 3), False)):
        xo, xl, nvis = exact(q, k, v, lens, sinks=sinks, window=window, causal=causal)
        if window == (7, 3):
            assert int((nvis[1:] == 0).sum()) > 0, "the case has no row with an empty window"
        assert_tells_sinks_apart(xo, q, k, v, lens, sinks, dtname, f"window {window} {dtname} d{d}", window=window, causal=causal)
        for ns in (1, 0, 3):
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns,
                                                 return_softmax_lse=True, sinks=sinks.to(gpu))
            check(out, lse, xo, xl, nvis, sinks, dtname, f"window {window} causal={causal} {dtname} d{d} splits={ns}")


# ---- 9. - 11. edges -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_nan_sink_and_nan_score(gpu, dtname, num_splits):
    """a NaN sink: the rows of that head are NaN in O and LSE - the rows of the empty sequence included - and every other head keeps its bits;
    a NaN query row under finite sinks is NaN as ever, the other rows keep their bits"""
    dt = DT[dtname]
    d, h, hk, sq, lens = 64, 8, 2, 2, [200, 70, 0, 33]
    b = len(lens)
    gen = torch.Generator().manual_seed(30000)
    k, v, q = _rand((b, 256, hk, d), dt, gen).to(gpu), _rand((b, 256, hk, d), dt, gen).to(gpu), _rand((b, sq, h, d), dt, gen).to(gpu)
    sinks = make_sinks(h).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, num_splits=num_splits, return_softmax_lse=True)
    clean = F.flash_attn_with_kvcache(q, k, v, sinks=sinks, **kw)
    assert torch.isfinite(clean[0]).all().item() and torch.isfinite(clean[1]).all().item()
    sn = sinks.clone()
    sn[5] = NAN
    out, lse = F.flash_attn_with_kvcache(q, k, v, sinks=sn, **kw)
    assert torch.isnan(out[:, :, 5]).all().item() and torch.isnan(lse[:, 5]).all().item()
    others = [i for i in range(h) if i != 5]
    assert _same(out[:, :, others], clean[0][:, :, others]) and _same(lse[:, others], clean[1][:, others])
    qn = q.clone()
    qn[1, 0, 3, 7] = NAN
    out, lse = F.flash_attn_with_kvcache(qn, k, v, sinks=sinks, **kw)
    assert torch.isnan(out[1, 0, 3]).all().item() and torch.isnan(lse[1, 3, 0]).item()
    keep = torch.ones(b, sq, h, dtype=torch.bool, device=gpu)
    keep[1, 0, 3] = False
    assert _same(out[keep], clean[0][keep]) and _same(lse.permute(0, 2, 1)[keep], clean[1].permute(0, 2, 1)[keep])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_rows_pages_and_packed_rows_out_of_sight_are_never_read(gpu, dtname, d):
    """cache rows at or past L, rows before a window and unreferenced pages hold NaN, and so do the packed query rows past cu_seqlens_q[-1] of a
    ragged call: the result is finite and the bits of the clean call"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(31000 + d)
    lens, sq, h, hk = [0, 1, 31, 33, 100, 777, 1000], 3, 16, 4
    b = len(lens)
    sinks = make_sinks(h).to(gpu)
    k, v = _rand((b, CAP, hk, d), dt, gen).to(gpu), _rand((b, CAP, hk, d), dt, gen).to(gpu)
    q = _rand((b, sq, h, d), dt, gen).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for window, causal in (((-1, -1), False), ((-1, -1), True), ((127, 0), True), ((100, 1), False)):
        kn, vn = k.clone(), v.clone()
        for i, L in enumerate(lens):
            lo, _ = _bounds(L, sq, 0, window, causal)
            for t in (kn, vn):
                t[i, :lo] = NAN
                t[i, L:] = NAN
        kp, vp, table, _ = _page(kn, vn, 16, 17)            # (unreferenced pages: NaN)
        for ns in (1, 0, 5):
            kw = dict(cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, sinks=sinks)
            want = F.flash_attn_with_kvcache(q, k, v, **kw)
            assert torch.isfinite(want[0]).all().item() and torch.isfinite(want[1]).all().item()
            assert (want[0][0] == 0).all().item() and torch.equal(want[1][0], sinks.view(h, 1).expand(h, sq))        # the empty sequence
            for got in (F.flash_attn_with_kvcache(q, kn, vn, **kw), F.flash_attn_with_kvcache(q, kp, vp, block_table=table, **kw)):
                assert _same(got[0], want[0]) and _same(got[1], want[1]), (window, causal, ns)
    # packed rows past cu_seqlens_q[-1]
    sqs = [3, 0, 1, 17, 1, 3, 1]
    total, extra = sum(sqs), 5
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    qr = _rand((total + extra, h, d), dt, gen).to(gpu)
    qp = qr.clone()
    qp[total:] = NAN
    kn, vn = k.clone(), v.clone()
    for i, L in enumerate(lens):
        kn[i, L:] = NAN
        vn[i, L:] = NAN
    for ns in (1, 3):
        kw = dict(cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=17, causal=True, num_splits=ns, return_softmax_lse=True, sinks=sinks)
        want, got = F.flash_attn_with_kvcache(qr, kn, vn, **kw), F.flash_attn_with_kvcache(qp, kn, vn, **kw)
        assert torch.isfinite(got[0][:total]).all().item() and torch.isfinite(got[1][:, :total]).all().item()
        assert _same(got[0][:total], want[0][:total]) and _same(got[1][:, :total], want[1][:, :total]), ns


def test_captured_sink_call_replays_with_new_lengths_and_new_sink_values(gpu):
    """one captured call (a single chain of launches on one stream); cache_seqlens and the sinks tensor are rewritten in place before the replay"""
    dt, d, h, hk, b = torch.float16, 64, 64, 8, 2
    gen = torch.Generator().manual_seed(32000)
    k, v = _rand((b, 4096, hk, d), dt, gen).to(gpu), _rand((b, 4096, hk, d), dt, gen).to(gpu)
    q = _rand((b, 1, h, d), dt, gen).to(gpu)
    cs = torch.tensor([100, 4000], dtype=torch.int32, device=gpu)
    sinks = make_sinks(h).to(gpu)
    kw = dict(cache_seqlens=cs, causal=True, window_size=(127, 0), return_softmax_lse=True, sinks=sinks)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, k, v, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, k, v, **kw)
    first = (out_g.clone(), lse_g.clone())
    lens = [2500, 1]
    new_sinks = torch.flip(make_sinks(h), (0,)) - 1.0
    cs.copy_(torch.tensor(lens, dtype=torch.int32))
    sinks.copy_(new_sinks)
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = F.flash_attn_with_kvcache(q, k, v, **kw)
    assert _same(out_g, out_e) and _same(lse_g, lse_e)
    assert not _same(out_g, first[0])
    xo, xl, nvis = exact(q, k, v, lens, sinks=new_sinks, window=(127, 0), causal=True)
    check(out_g, lse_g, xo, xl, nvis, new_sinks, "fp16", "graph replay")
