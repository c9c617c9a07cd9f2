"""GPU: ragged query batches on the decode path (cu_seqlens_q / max_seqlen_q / cu_seqlens_k_new of flash_attn_with_kvcache, fa_kvcache_options_v4).

Expectations come from outside the code under test: the C oracle and exact fp64 math through _util.check_kvcache_rows, called per sequence
with batch-1 slices (the project's rules and tolerances), for windows the fp64 statement of the visibility formula written below
(_window_exact: L_i - sq_i + t - left <= j <= L_i - sq_i + t + right, j < L_i) with the C oracle on every row's visible slice, and - the
contract of the feature - the DENSE call on each sequence alone, bit for bit in out, lse and every cache byte."""
import math

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
SQ = [1, 1, 5, 0, 16, 3, 130, 1]                        # decode, decode, speculative, idle, a tile of tokens, speculative, a prompt chunk, decode
CAP = 1280
LENS = [1, 0, 63, 64, 65, 777, CAP, 300]                # 0 (a dead row), 1, 63 / 64 / 65, a non-multiple of the split chunk (7 splits: 192 keys), the capacity
HEADS = [(8, 8), (32, 8), (12, 4), (32, 1)]             # MHA; GQA 4 (a tile holds 4 tokens); GQA 3 (tokens straddle tile borders); MQA (a token fills two tiles)


def _rand(shape, dt, gen, dev):
    return torch.randn(*shape, device=dev, dtype=torch.float32, generator=gen).to(dt)


def _cu(lengths, dev):
    return torch.tensor([0] + list(np.cumsum(lengths)), dtype=torch.int32, device=dev)


def _same(a, b):
    return a.shape == b.shape and torch.equal(U.bits(a), U.bits(b))


def _bytes(t):
    return t.contiguous().view(torch.uint8) if t.dtype == torch.float8_e4m3fn else U.bits(t)


def _dense_seq(i, q, kc, vc, cs, sq, **kw):
    """the dense call on sequence i alone: batch 1, seqlen_q = sq_i, on the caches / descales of i (views: appends land in the caller's caches)"""
    c0 = sum(sq[:i])
    extra = {k: (v[i:i + 1] if isinstance(v, torch.Tensor) and k in ("k_descale", "v_descale", "block_table") else v) for k, v in kw.items()}
    paged = "block_table" in kw
    return F.flash_attn_with_kvcache(q[c0:c0 + sq[i]][None], kc if paged else kc[i:i + 1], vc if paged else vc[i:i + 1], cache_seqlens=cs[i:i + 1],
                                     return_softmax_lse=True, **extra)


def _assert_bits_per_sequence(out, lse, q, kc, vc, cs, sq, tag, only=None, **kw):
    for i, s in enumerate(sq):
        if s == 0 or (only is not None and i not in only):
            continue
        c0 = sum(sq[:i])
        od, ld = _dense_seq(i, q, kc, vc, cs, sq, **kw)
        assert _same(out[c0:c0 + s], od[0]), f"{tag}: out of sequence {i} (sq {s}) differs from the dense call on it alone"
        assert _same(lse[:, c0:c0 + s], ld[0]), f"{tag}: lse of sequence {i} (sq {s}) differs from the dense call on it alone"


def _check_rows_per_sequence(out, lse, q, kc, vc, lens, sq, causal, dtname, tag):
    for i, s in enumerate(sq):
        if s == 0:
            continue
        c0 = sum(sq[:i])
        U.check_kvcache_rows(out[c0:c0 + s][None], lse[:, c0:c0 + s][None], q[c0:c0 + s][None], kc[i:i + 1], vc[i:i + 1], [lens[i]], causal, dtname,
                             f"{tag} seq{i} sq{s}")


def _page(kc, vc, P, seed, share=None, extra=3):
    """pool + shuffled block table holding the logical caches (b, cap, hk, d); share = (i, j): sequence j reads its first page from i's (the
    caller made the two logical pages equal); unreferenced pages hold a NaN pattern.  8-bit caches come as uint8 views."""
    b, cap, hk, d = kc.shape
    cols = cap // P
    nb = b * cols + extra
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))
    table = perm[: b * cols].view(b, cols).to(torch.int32).to(kc.device)
    if share is not None:
        table[share[1], 0] = table[share[0], 0]
    it = {1: torch.uint8, 2: torch.int16}[kc.element_size()]
    kp = torch.full((nb, P, hk, d), 0x7F if kc.element_size() == 1 else U.SENT16, dtype=it, device=kc.device)
    vp = kp.clone()
    idx = table.long()
    kp[idx] = kc.view(it).reshape(b, cols, P, hk, d)
    vp[idx] = vc.view(it).reshape(b, cols, P, hk, d)
    return kp.view(kc.dtype), vp.view(kc.dtype), table


def _unpage(pool, table, P):
    b, cols = table.shape
    return torch.stack([torch.cat([pool[table[i, c]] for c in range(cols)]) for i in range(b)])


# ---- 1. mixed steps: tolerance and the bit contract -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_mixed_step_against_reference_and_dense_calls(gpu, dtname, d, causal):
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(101 + d + int(causal))
    b, total = len(SQ), sum(SQ)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    cu = _cu(SQ, gpu)
    for h, hk in HEADS:
        kc, vc = _rand((b, CAP, hk, d), dt, gen, gpu), _rand((b, CAP, hk, d), dt, gen, gpu)
        q = _rand((total, h, d), dt, gen, gpu)
        for ns in (1, 7):
            tag = f"{dtname} d{d} h{h}/{hk} causal={causal} splits={ns}"
            out, lse = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max(SQ))
            assert out.shape == q.shape and out.dtype == dt and lse.shape == (h, total) and lse.dtype == torch.float32
            out2, lse2 = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max(SQ))
            assert _same(out, out2) and _same(lse, lse2), f"{tag}: not deterministic"
            _assert_bits_per_sequence(out, lse, q, kc, vc, cs, SQ, tag, causal=causal, num_splits=ns)
            if (h, hk) in ((32, 8), (12, 4)) or ns == 1:
                _check_rows_per_sequence(out, lse, q, kc, vc, LENS, SQ, causal, dtname, tag)
        # max_seqlen_q only sizes the launch: a larger value (the plain grid instead of the compact one, or the other way round) gives the same bits
        o_big = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs, causal=causal, num_splits=1, cu_seqlens_q=cu, max_seqlen_q=4096)
        o_one = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs, causal=causal, num_splits=1, cu_seqlens_q=cu, max_seqlen_q=max(SQ))
        assert _same(o_big, o_one)


# ---- 2. paged ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", [16, 256])
@pytest.mark.parametrize("causal", [False, True])
def test_paged_cache_gives_the_bits_of_the_contiguous_ragged_call(gpu, P, causal):
    b, total = len(SQ), sum(SQ)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    cu = _cu(SQ, gpu)
    for dtname, d, (h, hk) in (("fp16", 128, (32, 8)), ("bf16", 64, (12, 4)), ("fp16", 64, (32, 1))):
        dt = DT[dtname]
        gen = torch.Generator(device=gpu).manual_seed(7 + P + d)
        kc, vc = _rand((b, CAP, hk, d), dt, gen, gpu), _rand((b, CAP, hk, d), dt, gen, gpu)
        kc[5, :P], vc[5, :P] = kc[6, :P], vc[6, :P]           # sequences 5 and 6 share their first page for reading
        q = _rand((total, h, d), dt, gen, gpu)
        kp, vp, table = _page(kc, vc, P, seed=P + d, share=(6, 5))
        for ns in (1, 7, 0):
            kw = dict(cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max(SQ))
            out, lse = F.flash_attn_with_kvcache(q, kp, vp, block_table=table, **kw)
            out_c, lse_c = F.flash_attn_with_kvcache(q, kc, vc, **kw)
            assert _same(out, out_c) and _same(lse, lse_c), (dtname, d, h, hk, P, ns)
            if ns == 1:
                _assert_bits_per_sequence(out, lse, q, kp, vp, cs, SQ, f"paged P{P}", causal=causal, num_splits=1, block_table=table)
        _check_rows_per_sequence(out, lse, q, kc, vc, LENS, SQ, causal, dtname, f"paged P{P} {dtname} d{d} auto split")


# ---- 3. windows -------------------------------------------------------------------------------------------------------------------------------

def _bounds(L, sq, t, left, right, causal):
    """the visible keys [lo, hi) of query row t: L - sq + t - left <= j <= L - sq + t + right, j < L; -1 = unbounded; causal: right = 0"""
    pos = L - sq + t
    lo = 0 if left < 0 else max(pos - left, 0)
    r = 0 if causal else right
    hi = L if r < 0 else min(pos + r + 1, L)
    return lo, max(hi, lo) if hi > 0 else lo


def _window_exact(q, k, v, L, left, right, causal):
    """fp64 masked softmax of one sequence: q (sq, h, d), k / v (cap, hk, d) -> O (sq, h, d), LSE (h, sq); a row without a visible key: 0, 0"""
    sq, h, d = q.shape
    hk = k.shape[1]
    qd, kd, vd = (t.double().cpu() for t in (q, k, v))
    kd, vd = kd.repeat_interleave(h // hk, dim=1), vd.repeat_interleave(h // hk, dim=1)
    s = torch.einsum("thd,jhd->htj", qd, kd) / math.sqrt(d)
    mask = torch.zeros(sq, k.shape[0], dtype=torch.bool)
    for t in range(sq):
        lo, hi = _bounds(L, sq, t, left, right, causal)
        mask[t, lo:hi] = True
    s = s.masked_fill(~mask[None], float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True)
    live = mask.any(-1)[None, :, None].expand_as(den)
    o = torch.einsum("htj,jhd->thd", torch.where(live, p / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(p)), vd)
    lse = torch.where(live, m + torch.log(den), torch.zeros_like(den)).squeeze(-1)
    return o, lse


def _check_window_call(out, lse, q, kc, vc, sq, lens, left, right, causal, dtname, tag):
    """every live row of every sequence of ONE call against the C oracle on its visible slice (one key range per row) and the fp64 statement
    above; dead rows exactly 0.  out (total_q, h, d), lse (h, total_q); kc / vc the logical caches (b, cap, hk, d).
    The rows of a call are asserted together, as check_window_rows of the dense window suite does, in two groups: rows that see at least
    _util.PLAIN_SK_MIN keys (which must also meet the plain bounds) and rows that see fewer.  Why not one assertion per sequence: the relative
    metric is mean(|x - e| / max(|e|, 1e-6)), and a decoding sequence contributes one row of h x d elements - about a thousand.  An element
    whose exact value happens to lie within 1e-6 of zero carries the ordinary absolute error of a bf16 P (1e-4) as a relative error of 100,
    and alone puts the mean of a thousand elements at 0.1, above the bound, whatever kernel computed it; over the rows of a call the same
    element weighs a hundredth of that.  Bound, reference and cases are unchanged; every row is still asserted."""
    from oracle import attn_oracle as A

    mode = A.ROUND_FP16 if dtname == "fp16" else A.ROUND_BF16
    groups = {True: ([], [], [], [], [0]), False: ([], [], [], [], [0])}      # long rows / short rows: packed row, exact row, K slice, V slice, cu_k
    kn, vn = (t.detach().float().cpu().numpy() for t in (kc, vc))
    for i, s in enumerate(sq):
        if s == 0:
            continue
        c0 = sum(sq[:i])
        xo, _ = _window_exact(q[c0:c0 + s], kc[i], vc[i], lens[i], left, right, causal)
        for t in range(s):
            lo, hi = _bounds(lens[i], s, t, left, right, causal)
            if hi <= lo:
                assert (out[c0 + t] == 0).all().item() and (lse[:, c0 + t] == 0).all().item(), f"{tag}: dead row seq{i} t{t} must be O = 0, LSE = 0"
                continue
            rows, exact, ks, vs, cuk = groups[hi - lo >= U.PLAIN_SK_MIN]
            rows.append(c0 + t)
            exact.append(xo[t].numpy())
            ks.append(kn[i, lo:hi])
            vs.append(vn[i, lo:hi])
            cuk.append(cuk[-1] + hi - lo)
    qn, on, ln = q.detach().float().cpu().numpy(), out.float().cpu().numpy(), lse.cpu().numpy()
    for long_rows, (rows, exact, ks, vs, cuk) in groups.items():
        if not rows:
            continue
        o_ref, lse_ref = A.attn_fwd(qn[rows], np.concatenate(ks), np.concatenate(vs), causal=False, round_mode=mode, cu_seqlens_q=np.arange(len(rows) + 1, dtype=np.int32),
                                    cu_seqlens_k=np.asarray(cuk, dtype=np.int32), max_seqlen_q=1, max_seqlen_k=int(np.diff(cuk).max()))
        U.assert_close(on[rows], o_ref, dtname, f"ragged window O {tag} {'long' if long_rows else 'short'} rows", sk=int(np.diff(cuk).min()), oracle=o_ref, exact=np.stack(exact))
        err = float(np.abs(ln[:, rows].T - lse_ref[:, :, 0]).max())
        assert err <= U.LSE_TOL, f"{tag}: LSE err {err}"


@pytest.mark.parametrize("dtname,d,heads", [("fp16", 128, (32, 8)), ("bf16", 64, (12, 4)), ("fp16", 64, (32, 1)), ("bf16", 128, (8, 8))])
def test_windows(gpu, dtname, d, heads):
    """(left, 0) causal and (left, right) non-causal, left smaller and larger than the lengths: the dense call's bits at num_splits = 1; under a forced
    split the tolerance rules, and the dense call's bits for the sequences with sq_i == max_seqlen_q (the two calls then size the split alike)"""
    dt = DT[dtname]
    h, hk = heads
    gen = torch.Generator(device=gpu).manual_seed(31 + d + h)
    b, total, max_sq = len(SQ), sum(SQ), max(SQ)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    cu = _cu(SQ, gpu)
    kc, vc = _rand((b, CAP, hk, d), dt, gen, gpu), _rand((b, CAP, hk, d), dt, gen, gpu)
    q = _rand((total, h, d), dt, gen, gpu)
    P = 16
    kp, vp, table = _page(kc, vc, P, seed=d + h)
    longest = [i for i, s in enumerate(SQ) if s == max_sq]
    for (left, right), causal in (((5, 0), True), ((100, 0), True), ((2000, 0), True), ((0, 0), True), ((40, 3), False), ((700, 0), False), ((3, 200), False), ((-1, 2), False)):
        for ns in (1, 7):
            tag = f"{dtname} d{d} h{h}/{hk} window=({left},{right}) causal={causal} splits={ns}"
            kw = dict(cache_seqlens=cs, causal=causal, window_size=(left, right), num_splits=ns, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max_sq)
            out, lse = F.flash_attn_with_kvcache(q, kc, vc, **kw)
            out_p, lse_p = F.flash_attn_with_kvcache(q, kp, vp, block_table=table, **kw)
            assert _same(out, out_p) and _same(lse, lse_p), tag + ": paged differs from contiguous"
            _assert_bits_per_sequence(out, lse, q, kc, vc, cs, SQ, tag, only=None if ns == 1 else longest, causal=causal, window_size=(left, right), num_splits=ns)
            if ns == 7 or (left, right) in ((5, 0), (40, 3)):
                _check_window_call(out, lse, q, kc, vc, SQ, LENS, left, right, causal, dtname, tag)


# ---- 4. FP8 cache -----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("paged", [False, True])
def test_fp8_cache_read_and_append(gpu, paged):
    """an e4m3 cache with descales: the ragged call reads what the dense calls read (bits) and the dequantised 16-bit call within tolerance; the
    ragged append writes the codes the dense appends write, byte for byte"""
    sq = [1, 4, 0, 16, 2, 33]
    sn = [1, 4, 2, 16, 0, 33]
    lens0 = [0, 60, 7, 200, 511, 100]
    cap, P = 512, 16
    b, total, total_n = len(sq), sum(sq), sum(sn)
    for dtname, d, (h, hk), causal in (("fp16", 128, (32, 8), True), ("bf16", 64, (12, 4), False), ("fp16", 64, (8, 8), True), ("bf16", 128, (32, 1), True)):
        dt = DT[dtname]
        gen = torch.Generator(device=gpu).manual_seed(57 + d + h)
        cg = torch.Generator().manual_seed(57 + d + h)
        kd, vd = (0.25 * 16.0 ** torch.rand(b, hk, generator=cg) * 1.03).to(gpu), (0.25 * 16.0 ** torch.rand(b, hk, generator=cg) * 1.03).to(gpu)
        k8 = (torch.randn(b, cap, hk, d, generator=cg) / kd.cpu()[:, None, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(gpu)
        v8 = (torch.randn(b, cap, hk, d, generator=cg) / vd.cpu()[:, None, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(gpu)
        q = _rand((total, h, d), dt, gen, gpu)
        kn, vn = _rand((total_n, hk, d), dt, gen, gpu), _rand((total_n, hk, d), dt, gen, gpu)
        cs = torch.tensor(lens0, dtype=torch.int32, device=gpu)
        cu, cun = _cu(sq, gpu), _cu(sn, gpu)
        if paged:
            kr, vr, table = _page(k8.view(torch.uint8), v8.view(torch.uint8), P, seed=d)
            kr, vr = kr.view(torch.float8_e4m3fn), vr.view(torch.float8_e4m3fn)
            extra = dict(block_table=table)
        else:
            kr, vr, extra = k8.clone(), v8.clone(), dict()
        kd_, vd_ = kr.clone(), vr.clone()                       # the caches the dense calls append into
        for ns in (1, 3):
            kw = dict(causal=causal, num_splits=ns, k_descale=kd, v_descale=vd, **extra)
            out, lse = F.flash_attn_with_kvcache(q, kr, vr, k=kn, v=vn, cache_seqlens=cs, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max(sq), cu_seqlens_k_new=cun, **kw)
            for i in range(b):
                c0, n0 = sum(sq[:i]), sum(sn[:i])
                qi = q[c0:c0 + sq[i]][None] if sq[i] else q[:1][None]               # sq_i = 0: the dense call needs a query row; only its cache bytes count
                ki, vi = (kn[n0:n0 + sn[i]][None], vn[n0:n0 + sn[i]][None]) if sn[i] else (None, None)
                kwi = dict(kw, k_descale=kd[i:i + 1], v_descale=vd[i:i + 1])
                if paged:
                    kwi["block_table"] = table[i:i + 1]
                od, ld = F.flash_attn_with_kvcache(qi, kd_ if paged else kd_[i:i + 1], vd_ if paged else vd_[i:i + 1], k=ki, v=vi, cache_seqlens=cs[i:i + 1],
                                                   return_softmax_lse=True, **kwi)
                if sq[i]:
                    assert _same(out[c0:c0 + sq[i]], od[0]) and _same(lse[:, c0:c0 + sq[i]], ld[0]), (dtname, d, h, hk, paged, ns, i)
            assert torch.equal(_bytes(kr), _bytes(kd_)) and torch.equal(_bytes(vr), _bytes(vd_)), "appended codes differ from the dense appends"
        # the read side against the 16-bit call on the dequantised cache, through the reference rules
        kl = _unpage(kr.view(torch.uint8), table, P).view(torch.float8_e4m3fn) if paged else kr
        vl = _unpage(vr.view(torch.uint8), table, P).view(torch.float8_e4m3fn) if paged else vr
        k_deq = kl.cpu().float() * kd.cpu()[:, None, :, None]            # the dequantised cache, fp32 on the CPU (as the FP8 suite states it)
        v_deq = vl.cpu().float() * vd.cpu()[:, None, :, None]
        lens = [min(a + n, cap) for a, n in zip(lens0, sn)]
        live = [i for i in range(b) if sq[i] and (not causal or sq[i] <= lens[i])]
        for i in live:
            c0 = sum(sq[:i])
            U.check_kvcache_rows(out[c0:c0 + sq[i]][None], lse[:, c0:c0 + sq[i]][None], q[c0:c0 + sq[i]][None], k_deq[i:i + 1], v_deq[i:i + 1], [lens[i]], causal, dtname,
                                 f"fp8 {dtname} d{d} paged={paged} seq{i}")


# ---- 5. append --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("same_cu", [True, False])
@pytest.mark.parametrize("paged", [False, True])
def test_append_writes_what_the_dense_appends_write(gpu, same_cu, paged):
    """every cache byte equals the per-sequence dense appends, rows no sequence appends keep their bits, cache_seqlens and both cu_seqlens tensors
    are unchanged; cu_seqlens_k_new is cu_seqlens_q, or another one with sn_i != sq_i and some sn_i = 0; a sequence with sq_i = 0 still appends"""
    sq = [1, 3, 0, 16, 2, 40]
    sn = sq if same_cu else [2, 0, 5, 16, 1, 7]
    lens0 = [0, 5, 250, 100, 299 - 2, 17]
    cap, P = 304, 16
    b, total, total_n = len(sq), sum(sq), sum(sn)
    for dtname, d, (h, hk), causal in (("fp16", 128, (16, 4), True), ("bf16", 64, (12, 4), False), ("fp16", 64, (32, 1), True)):
        dt = DT[dtname]
        gen = torch.Generator(device=gpu).manual_seed(77 + d)
        kc, vc = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
        q = _rand((total, h, d), dt, gen, gpu)
        kn, vn = _rand((total_n, hk, d), dt, gen, gpu), _rand((total_n, hk, d), dt, gen, gpu)
        cs = torch.tensor(lens0, dtype=torch.int32, device=gpu)
        cu = _cu(sq, gpu)
        cun = cu if same_cu else _cu(sn, gpu)
        if paged:
            kr, vr, table = _page(kc, vc, P, seed=d)
            extra = dict(block_table=table)
        else:
            kr, vr, extra = kc.clone(), vc.clone(), dict()
        kd_, vd_ = kr.clone(), vr.clone()
        kn0, vn0, q0 = kn.clone(), vn.clone(), q.clone()
        out, lse = F.flash_attn_with_kvcache(q, kr, vr, k=kn, v=vn, cache_seqlens=cs, causal=causal, num_splits=1, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max(sq),
                                             cu_seqlens_k_new=cun, **extra)
        torch.cuda.synchronize()
        assert cs.tolist() == lens0 and cu.tolist() == [0] + list(np.cumsum(sq)) and cun.tolist() == [0] + list(np.cumsum(sn))
        assert _same(kn, kn0) and _same(vn, vn0) and _same(q, q0)
        for i in range(b):
            c0, n0 = sum(sq[:i]), sum(sn[:i])
            qi = q[c0:c0 + sq[i]][None] if sq[i] else q[:1][None]                   # (sq_i = 0: a throw-away query row, only the cache bytes are compared)
            ki, vi = (kn[n0:n0 + sn[i]][None], vn[n0:n0 + sn[i]][None]) if sn[i] else (None, None)
            kwi = dict(block_table=table[i:i + 1]) if paged else dict()
            od, ld = F.flash_attn_with_kvcache(qi, kd_ if paged else kd_[i:i + 1], vd_ if paged else vd_[i:i + 1], k=ki, v=vi, cache_seqlens=cs[i:i + 1], causal=causal,
                                               num_splits=1, return_softmax_lse=True, **kwi)
            if sq[i]:
                assert _same(out[c0:c0 + sq[i]], od[0]) and _same(lse[:, c0:c0 + sq[i]], ld[0]), (dtname, d, paged, same_cu, i)
        assert _same(kr, kd_) and _same(vr, vd_), "cache bytes differ from the per-sequence dense appends"
        # ... and against the statement itself: rows cache_seqlens[i] .. + sn_i - 1 hold the new rows, every other row its old bits
        kl = _unpage(kr, table, P) if paged else kr
        k_exp = kc.clone()
        for i in range(b):
            n0 = sum(sn[:i])
            k_exp[i, lens0[i]:lens0[i] + sn[i]] = kn[n0:n0 + sn[i]]
        assert _same(kl, k_exp)
        lens = [a + n for a, n in zip(lens0, sn)]
        vl = _unpage(vr, table, P) if paged else vr
        live = [i for i in range(b) if sq[i] and (not causal or sq[i] <= lens[i])]
        for i in live:
            c0 = sum(sq[:i])
            U.check_kvcache_rows(out[c0:c0 + sq[i]][None], lse[:, c0:c0 + sq[i]][None], q[c0:c0 + sq[i]][None], kl[i:i + 1], vl[i:i + 1], [lens[i]], causal, dtname,
                                 f"append {dtname} d{d} paged={paged} seq{i}")


def test_append_past_the_capacity_drops_rows_and_writes_nothing_outside(gpu):
    """the precondition cache_seqlens[i] + sn_i <= capacity, broken: the rows that do not fit are dropped, the neighbouring sequence's cache and the
    guard band around the caches keep their bits"""
    dt, d, h, hk, cap = torch.float16, 64, 8, 2, 64
    gen = torch.Generator(device=gpu).manual_seed(3)
    sq, sn, lens0 = [2, 1, 4], [6, 1, 4], [60, 64, -5]
    b = len(sq)
    kbuf, kc, _ = U.guarded((b, cap, hk, d), dt, gpu, (2, 0, 0, 16))
    vbuf, vc, _ = U.guarded((b, cap, hk, d), dt, gpu, (2, 0, 0, 16))
    kc.copy_(_rand((b, cap, hk, d), dt, gen, gpu)), vc.copy_(_rand((b, cap, hk, d), dt, gen, gpu))
    k0, v0, kb0 = kc.clone(), vc.clone(), kbuf.clone()
    q = _rand((sum(sq), h, d), dt, gen, gpu)
    kn, vn = _rand((sum(sn), hk, d), dt, gen, gpu), _rand((sum(sn), hk, d), dt, gen, gpu)
    cs = torch.tensor(lens0, dtype=torch.int32, device=gpu)
    out = F.flash_attn_with_kvcache(q, kc, vc, k=kn, v=vn, cache_seqlens=cs, cu_seqlens_q=_cu(sq, gpu), max_seqlen_q=4, cu_seqlens_k_new=_cu(sn, gpu))
    assert torch.isfinite(out.float()).all()
    k_exp, v_exp = k0.clone(), v0.clone()
    k_exp[0, 60:64], v_exp[0, 60:64] = kn[0:4], vn[0:4]         # 4 of 6 rows fit
    k_exp[2, 0:4], v_exp[2, 0:4] = kn[7:11], vn[7:11]           # a negative length counts as 0; sequence 1 is full: its row is dropped
    assert _same(kc, k_exp) and _same(vc, v_exp)
    mask = torch.ones_like(kbuf, dtype=torch.bool)
    mask[1:1 + b, :, :, 8:8 + d] = False
    assert torch.equal(U.bits(kbuf)[mask], U.bits(kb0)[mask]) and (U.bits(vbuf)[mask] == U.SENT16).all()


# ---- 6. uniform batches -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", [1, 4, 5, 17])
def test_uniform_ragged_batch_equals_the_dense_batch(gpu, s):
    for dtname, d, (h, hk), b in (("fp16", 128, (32, 8), 5), ("bf16", 64, (12, 4), 3), ("fp16", 64, (8, 8), 9), ("bf16", 128, (32, 1), 2)):
        dt = DT[dtname]
        gen = torch.Generator(device=gpu).manual_seed(s + d + b)
        cap = 640
        kc, vc = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
        qd = _rand((b, s, h, d), dt, gen, gpu)
        kn, vn = _rand((b, s, hk, d), dt, gen, gpu), _rand((b, s, hk, d), dt, gen, gpu)
        cs = torch.tensor([(37 * i + 20) % (cap - s) for i in range(b)], dtype=torch.int32, device=gpu)
        cu = _cu([s] * b, gpu)
        for causal, win in ((False, (-1, -1)), (True, (-1, -1)), (True, (9, 0)), (False, (50, 1))):
            k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
            od, ld = F.flash_attn_with_kvcache(qd, k1, v1, k=kn, v=vn, cache_seqlens=cs, causal=causal, window_size=win, num_splits=1, return_softmax_lse=True)
            orr, lr = F.flash_attn_with_kvcache(qd.reshape(b * s, h, d), k2, v2, k=kn.reshape(b * s, hk, d), v=vn.reshape(b * s, hk, d), cache_seqlens=cs, causal=causal,
                                                window_size=win, num_splits=1, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=s, cu_seqlens_k_new=cu)
            assert _same(orr.view(b, s, h, d), od), (dtname, d, s, causal, win)
            assert _same(lr.view(h, b, s).permute(1, 0, 2).contiguous(), ld), (dtname, d, s, causal, win)
            assert _same(k1, k2) and _same(v1, v2)


# ---- 7. dead rows -----------------------------------------------------------------------------------------------------------------------------

def test_dead_rows_are_exact_zeros(gpu):
    """L_i = 0, and causal rows in front of the first key (sq_i > L_i): O = 0, LSE = 0 exactly - for one split and for forced splits; the cache rows
    behind L_i are poisoned"""
    dt, d, h, hk, cap = torch.float16, 128, 16, 4, 256
    gen = torch.Generator(device=gpu).manual_seed(13)
    sq, lens = [1, 20, 3, 16], [0, 7, 0, 16]
    kc, vc = _rand((4, cap, hk, d), dt, gen, gpu), _rand((4, cap, hk, d), dt, gen, gpu)
    for i, L in enumerate(lens):
        U.poison_(kc[i, L:]), U.poison_(vc[i, L:])
    q = _rand((sum(sq), h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for ns in (1, 2, 8):
        for causal in (False, True):
            out, lse = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, cu_seqlens_q=_cu(sq, gpu), max_seqlen_q=20)
            assert torch.isfinite(out.float()).all() and torch.isfinite(lse).all()
            for i, (s, L) in enumerate(zip(sq, lens)):
                c0 = sum(sq[:i])
                dead = s if L == 0 else (max(s - L, 0) if causal else 0)
                assert (out[c0:c0 + dead] == 0).all() and (lse[:, c0:c0 + dead] == 0).all(), (ns, causal, i)
                if dead < s:
                    assert (lse[:, c0 + dead:c0 + s] != 0).all()
                    xo, xl = U.fp64_math(q[c0:c0 + s], kc[i, :L], vc[i, :L], causal)
                    assert (out[c0 + dead:c0 + s].double().cpu() - xo[dead:]).abs().max() < 2e-2 and (lse[:, c0 + dead:c0 + s].double().cpu() - xl[:, dead:]).abs().max() < 1e-3


# ---- 8. never read, never written ---------------------------------------------------------------------------------------------------------------

def test_surplus_rows_are_never_read_or_written(gpu):
    """through the C ABI with guarded outputs: total_q > cu_seqlens_q[b] with the surplus q / k_new rows poisoned and the surplus out / lse entries
    holding a sentinel that must survive (one split and a forced split: the combine skips them too); cache rows at or past L_i poisoned"""
    dt, d, h, hk, cap = torch.bfloat16, 64, 12, 4, 512
    gen = torch.Generator(device=gpu).manual_seed(29)
    sq, sn, lens0 = [3, 1, 0, 18], [3, 1, 2, 18], [100, 0, 500, 257]
    b, used, usedn, total, totaln = len(sq), sum(sq), sum(sn), sum(sq) + 9, sum(sn) + 5
    cu, cun = _cu(sq, gpu), _cu(sn, gpu)
    cs = torch.tensor(lens0, dtype=torch.int32, device=gpu)
    for ns in (1, 4):
        kc, vc = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
        for i in range(b):
            U.poison_(kc[i, lens0[i] + sn[i]:]), U.poison_(vc[i, lens0[i] + sn[i]:])
        q = U.poison_(torch.empty(total, h, d, dtype=dt, device=gpu))
        kn, vn = U.poison_(torch.empty(totaln, hk, d, dtype=dt, device=gpu)), U.poison_(torch.empty(totaln, hk, d, dtype=dt, device=gpu))
        q[:used], kn[:usedn], vn[:usedn] = _rand((used, h, d), dt, gen, gpu), _rand((usedn, hk, d), dt, gen, gpu), _rand((usedn, hk, d), dt, gen, gpu)
        obuf, o, _ = U.guarded((total, h, d), dt, gpu, (4, 2, 16))
        lse_c = torch.full((h, total), -7.25, device=gpu)          # (h, total_q), the sentinel in every entry
        p = capi.kvcache_params(q, kc, vc, o, lse_c, cache_seqlens=cs, k_new=kn, v_new=vn, causal=True, num_splits=ns, cu_seqlens_q=cu, max_seqlen_q=32)
        opt = capi.kvcache_options(cu_seqlens_q=cu, cu_seqlens_k_new=cun, total_q=total, total_k_new=totaln)
        ws = torch.empty(max(capi.kvcache_workspace_bytes(p, opt), 16) // 4, device=gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        assert capi.kvcache_num_splits(p, opt) == ns
        k_ref, v_ref = kc.clone(), vc.clone()
        capi.run_fwd_kvcache(p, options=opt)
        torch.cuda.synchronize()
        assert torch.isfinite(o[:used].float()).all() and torch.isfinite(lse_c[:, :used]).all(), f"splits={ns}: a poisoned row or a surplus row leaked into a result"
        assert (lse_c[:, used:] == -7.25).all(), "surplus lse entries were written"
        mask = torch.ones_like(obuf, dtype=torch.bool)
        mask[2:2 + used, 1:1 + h, 8:8 + d] = False
        assert (U.bits(obuf)[mask] == U.SENT16).all(), "out was written outside the rows of the sequences"
        # the same call through the Python surface on the used rows alone
        out2, lse2 = F.flash_attn_with_kvcache(q[:used].clone(), k_ref, v_ref, k=kn[:usedn].clone(), v=vn[:usedn].clone(), cache_seqlens=cs, causal=True, num_splits=ns,
                                               return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=32, cu_seqlens_k_new=cun)
        assert _same(o[:used].contiguous(), out2) and _same(lse_c[:, :used].contiguous(), lse2)
        assert _same(kc, k_ref) and _same(vc, v_ref)


def test_rows_before_a_window_are_never_read_and_nan_stays_in_its_sequence(gpu):
    dt, d, h, hk, cap = torch.float16, 128, 32, 8, 1024
    gen = torch.Generator(device=gpu).manual_seed(41)
    sq, lens = [1, 4, 16, 1, 2], [900, 333, 1024, 64, 700]
    left = 40
    b, total = len(sq), sum(sq)
    cu = _cu(sq, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kc, vc = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((total, h, d), dt, gen, gpu)
    kw = dict(cache_seqlens=cs, causal=True, window_size=(left, 0), return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=16)
    for ns in (1, 3):
        ref, lref = F.flash_attn_with_kvcache(q, kc, vc, num_splits=ns, **kw)
        kpz, vpz = kc.clone(), vc.clone()
        for i, (s, L) in enumerate(zip(sq, lens)):
            U.poison_(kpz[i, :max(L - s - left, 0)]), U.poison_(vpz[i, :max(L - s - left, 0)])
            U.poison_(kpz[i, L:]), U.poison_(vpz[i, L:])
        out, lse = F.flash_attn_with_kvcache(q, kpz, vpz, num_splits=ns, **kw)
        assert _same(out, ref) and _same(lse, lref), f"splits={ns}: a row before the window or at / past L_i was read"
        # NaN in one q row: that row NaN, every other row its bits; NaN in a visible K row of one sequence: its rows NaN, the other sequences' bits
        qn = q.clone()
        qn[cu[2] + 5, 3, 17] = float("nan")
        out, lse = F.flash_attn_with_kvcache(qn, kc, vc, num_splits=ns, **kw)
        r = int(cu[2]) + 5
        assert torch.isnan(out[r, 3]).all() and torch.isnan(lse[3, r])
        keep = torch.ones(total, h, dtype=torch.bool, device=gpu)
        keep[r, 3] = False
        assert torch.equal(U.bits(out)[keep], U.bits(ref)[keep]) and torch.equal(U.bits(lse)[keep.t()], U.bits(lref)[keep.t()])
        kn_ = kc.clone()
        kn_[4, lens[4] - 1, 2, 9] = float("nan")                    # the last key of sequence 4, KV head 2: seen by its last row's heads 8 .. 11
        out, lse = F.flash_attn_with_kvcache(q, kn_, vc, num_splits=ns, **kw)
        c4 = int(cu[4])
        assert torch.isnan(out[c4 + 1, 8:12]).all() and torch.isnan(lse[8:12, c4 + 1]).all()
        assert _same(out[:c4], ref[:c4]) and _same(lse[:, :c4], lref[:, :c4])
        assert _same(out[c4:, :8], ref[c4:, :8]) and _same(out[c4:, 12:], ref[c4:, 12:])


# ---- 9. graph capture -------------------------------------------------------------------------------------------------------------------------

def test_graph_capture_replays_with_new_cu_seqlens(gpu):
    """one capture, one replay: cu_seqlens_q / cache_seqlens / the new rows rewritten in place (same total_q), compared with an eager call"""
    dt, d, h, hk, cap = torch.float16, 128, 32, 8, 2048
    gen = torch.Generator(device=gpu).manual_seed(53)
    b, total = 6, 24
    sq_a, sq_b = [1, 1, 8, 4, 9, 1], [4, 0, 1, 16, 2, 1]
    lens_a, lens_b = [100, 2000, 64, 700, 9, 1], [31, 5, 1999, 1024, 300, 2031]
    kc, vc = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    k_eager, v_eager = kc.clone(), vc.clone()
    q, kn, vn = _rand((total, h, d), dt, gen, gpu), _rand((total, hk, d), dt, gen, gpu), _rand((total, hk, d), dt, gen, gpu)
    cu, cs = _cu(sq_a, gpu), torch.tensor(lens_a, dtype=torch.int32, device=gpu)
    kw = dict(causal=True, return_softmax_lse=True, max_seqlen_q=16)

    def call(kc_, vc_):
        return F.flash_attn_with_kvcache(q, kc_, vc_, k=kn, v=vn, cache_seqlens=cs, cu_seqlens_q=cu, cu_seqlens_k_new=cu, **kw)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(kc.clone(), vc.clone())                              # warm-up outside the capture (allocator, module load)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = call(kc, vc)
    cu.copy_(_cu(sq_b, gpu)), cs.copy_(torch.tensor(lens_b, dtype=torch.int32, device=gpu))
    q.copy_(_rand((total, h, d), dt, gen, gpu)), kn.copy_(_rand((total, hk, d), dt, gen, gpu))
    kc.copy_(k_eager), vc.copy_(v_eager)
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = call(k_eager, v_eager)
    assert _same(out_g, out_e) and _same(lse_g, lse_e), "the replay did not follow the rewritten cu_seqlens_q / cache_seqlens"
    assert _same(kc, k_eager) and _same(vc, v_eager)
    _check_rows_per_sequence(out_g, lse_g, q, kc, vc, [a + n for a, n in zip(lens_b, sq_b)], sq_b, True, "fp16", "graph replay")


# ---- 10. many sequences -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_sq", [2, 64])
def test_600_sequences(gpu, max_sq):
    """past the 512 sequences one round of the slot lookup covers (max_seqlen_q = 64: the compact grid, two rounds) and on the plain grid
    (max_seqlen_q = 2): the dense call's bits for every sequence, the reference rules for a sample"""
    dt, d, h, hk, cap, b = torch.float16, 64, 8, 2, 192, 600
    gen = torch.Generator(device=gpu).manual_seed(61)
    sq = [1 + (i * 7 + i // 5) % 2 for i in range(b)]
    lens = [(i * 37) % (cap - 2) + 2 for i in range(b)]
    kc, vc = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((sum(sq), h, d), dt, gen, gpu)
    cs, cu = torch.tensor(lens, dtype=torch.int32, device=gpu), _cu(sq, gpu)
    cul = cu.tolist()
    for ns in (1, 3):
        out, lse = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=cs, causal=True, num_splits=ns, return_softmax_lse=True, cu_seqlens_q=cu, max_seqlen_q=max_sq)
        # the dense calls, batched by sq (a dense batch entry is tiled like a sequence of the ragged call)
        for s in (1, 2):
            idx = [i for i in range(b) if sq[i] == s]
            rows = torch.tensor([[cul[i] + t for t in range(s)] for i in idx], device=gpu)
            ii = torch.tensor(idx, device=gpu)
            od, ld = F.flash_attn_with_kvcache(q[rows], kc[ii], vc[ii], cache_seqlens=cs[ii], causal=True, num_splits=ns, return_softmax_lse=True)
            assert _same(out[rows], od), (max_sq, ns, s)
            assert _same(lse[:, rows].permute(1, 0, 2).contiguous(), ld), (max_sq, ns, s)
    sample = [0, 1, 255, 511, 512, 513, 598, 599]
    for i in sample:
        c0 = cul[i]
        U.check_kvcache_rows(out[c0:c0 + sq[i]][None], lse[:, c0:c0 + sq[i]][None], q[c0:c0 + sq[i]][None], kc[i:i + 1], vc[i:i + 1], [lens[i]], True, "fp16", f"b600 seq{i}")


# ---- 11. what is refused ----------------------------------------------------------------------------------------------------------------------

def test_rotary_with_ragged_queries_is_refused(gpu):
    dt, d, h, hk, cap = torch.float16, 64, 8, 2, 64
    q = torch.zeros(5, h, d, dtype=dt, device=gpu)
    kc = torch.zeros(2, cap, hk, d, dtype=dt, device=gpu)
    kn = torch.zeros(5, hk, d, dtype=dt, device=gpu)
    cu = _cu([2, 3], gpu)
    cos = torch.ones(cap, 16, dtype=dt, device=gpu)
    with pytest.raises(ValueError, match="rotary_cos / rotary_sin together with cu_seqlens_q are not supported"):
        F.flash_attn_with_kvcache(q, kc, kc.clone(), k=kn, v=kn, cache_seqlens=torch.zeros(2, dtype=torch.int32, device=gpu), rotary_cos=cos, rotary_sin=torch.zeros_like(cos),
                                  cu_seqlens_q=cu, max_seqlen_q=3, cu_seqlens_k_new=cu)
    # the C ABI says the same
    lse = torch.zeros(h, 5, device=gpu)
    p = capi.kvcache_params(q, kc, kc, torch.empty_like(q), lse, cache_seqlens=torch.zeros(2, dtype=torch.int32, device=gpu), k_new=kn, v_new=kn, cu_seqlens_q=cu, max_seqlen_q=3)
    o = capi.kvcache_options(rotary_cos=cos, rotary_sin=cos, cu_seqlens_q=cu, cu_seqlens_k_new=cu, total_q=5, total_k_new=5)
    with pytest.raises(RuntimeError, match="not supported"):
        capi.run_fwd_kvcache(p, options=o)
