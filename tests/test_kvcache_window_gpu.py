"""GPU: sliding-window decode over a KV cache (flash_attn_with_kvcache(..., window_size=(left, right)), fa_kvcache_options).

Expectations: the C oracle has no window, so every live query row is checked against attn_fwd run NON-causally on that row's own visible
slice of keys (its varlen form batches the rows), with fp64 masked-softmax math as the exact statement of the relative metric
(_util.assert_close, LSE_TOL); a row that sees no key must be exactly O = 0, LSE = 0.  Layout changes (paged) must not change bits, and
cache rows the window never sees are poisoned with NaN."""
import math
import statistics

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _rand(shape, dt, gen, dev):
    return torch.randn(*shape, device=dev, dtype=torch.float32, generator=gen).to(dt)


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _bounds(L, sq, t, window, causal):
    """[lo, hi) of the keys query row t of a sequence of length L sees (upstream flash-attn's window convention)"""
    left, right = window
    if causal:
        right = 0
    lo = max(0, L - sq + t - left) if left >= 0 else 0
    hi = min(L, L - sq + t + right + 1) if right >= 0 else L
    return lo, max(hi, lo)


def _exact(q, k, v, lens, window, causal):
    """fp64 masked softmax over the logical cache: O (b, sq, h, d), LSE (b, h, sq); rows without a visible key O = 0, LSE = 0"""
    b, sq, h, d = q.shape
    cap, hk = k.shape[1], k.shape[2]
    qd, kd, vd = (t.double().cpu() for t in (q, k, v))
    kd, vd = kd.repeat_interleave(h // hk, dim=2), vd.repeat_interleave(h // hk, dim=2)
    s = torch.einsum("bthd,bjhd->bhtj", qd, kd) / math.sqrt(d)
    mask = torch.zeros(b, 1, sq, cap, dtype=torch.bool)
    for i, L in enumerate(lens):
        for t in range(sq):
            lo, hi = _bounds(L, sq, t, window, causal)
            mask[i, 0, t, lo:hi] = True
    s = s.masked_fill(~mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True)
    live = mask.any(-1, keepdim=True).expand_as(den)
    o = torch.where(live, p / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(p)) @ vd.permute(0, 2, 1, 3)
    lse = torch.where(live, (m + torch.log(den)), torch.zeros_like(den)).squeeze(-1)
    return o.permute(0, 2, 1, 3), lse


def check_window_rows(out, lse, q, k, v, lens, window, causal, dtname, tag):
    """every live (batch, query) row against the C oracle on its visible slice (non-causal, varlen-batched); dead rows exactly 0"""
    from oracle import attn_oracle as A

    b, sq, h, d = q.shape
    qn, kn, vn = (t.detach().float().cpu().numpy() for t in (q, k, v))
    rows, qs, ks, vs, cu = [], [], [], [], [0]
    for i, L in enumerate(lens):
        for t in range(sq):
            lo, hi = _bounds(L, sq, t, window, causal)
            if hi <= lo:
                assert (out[i, t] == 0).all().item() and (lse[i, :, t] == 0).all().item(), f"{tag}: dead row b{i} t{t} must be O = 0, LSE = 0"
                continue
            rows.append((i, t, hi - lo))
            qs.append(qn[i, t])
            ks.append(kn[i, lo:hi])
            vs.append(vn[i, lo:hi])
            cu.append(cu[-1] + hi - lo)
    if not rows:
        return
    mode = A.ROUND_FP16 if dtname == "fp16" else A.ROUND_BF16
    cu_q = np.arange(len(rows) + 1, dtype=np.int32)
    o_ref, lse_ref = A.attn_fwd(np.stack(qs), np.concatenate(ks), np.concatenate(vs), causal=False, round_mode=mode, cu_seqlens_q=cu_q,
                                cu_seqlens_k=np.asarray(cu, dtype=np.int32), max_seqlen_q=1, max_seqlen_k=max(r[2] for r in rows))
    xo, _ = _exact(q, k, v, lens, window, causal)
    idx_b, idx_t = [r[0] for r in rows], [r[1] for r in rows]
    got = out[idx_b, idx_t].float().cpu().numpy()
    exact = xo[idx_b, idx_t].numpy()
    U.assert_close(got, o_ref, dtname, f"kvcache window O {tag}", sk=min(r[2] for r in rows), oracle=o_ref, exact=exact)
    got_lse = lse.cpu().numpy()[idx_b, :, idx_t]
    err = float(np.abs(got_lse - lse_ref[:, :, 0]).max())
    assert err <= U.LSE_TOL, f"{tag}: LSE err {err}"


def _page(logical_k, logical_v, P, gen_seed, extra=2, fill=float("nan")):
    """a pool + block table holding the logical caches (b, cap, hk, d), pages by a random permutation; unreferenced pages hold `fill`"""
    b, cap, hk, d = logical_k.shape
    cols = cap // P
    nb = b * cols + extra
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(gen_seed))
    table = perm[: b * cols].view(b, cols).to(torch.int32).to(logical_k.device)
    kp = torch.full((nb, P, hk, d), fill, dtype=logical_k.dtype, device=logical_k.device)
    vp = torch.full_like(kp, fill)
    idx = table.long()
    kp[idx] = logical_k.reshape(b, cols, P, hk, d)
    vp[idx] = logical_v.reshape(b, cols, P, hk, d)
    return kp, vp, table, perm[b * cols:].tolist()


def _poison_unseen(k, v, lens, sq, window, causal):
    """NaN into every logical cache row no query row of the call sees: below max(0, L - sq - left) (the first row's lower bound) and
    at or past L"""
    k, v = k.clone(), v.clone()
    for i, L in enumerate(lens):
        lo, _ = _bounds(L, sq, 0, window, causal)
        for t in (k, v):
            t[i, :lo] = float("nan")
            t[i, L:] = float("nan")
    return k, v


WINDOWS_CAUSAL = [(0, 0), (1, 0), (31, 0), (32, 0), (33, 0)]
WINDOWS_OPEN = [(45, -1), (-1, 3), (20, 2), (0, 0), (100, 40)]


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_window_against_reference(gpu, dtname, d):
    """MHA, GQA, MQA and a ratio that does not divide 16; seqlen_q 1, 2, 4, 16, 33; causal windows (0,0) .. (33,0) and non-causal (left, -1),
    (-1, right), (left, right); lengths 0, 1, 31, 32, 33, a non-multiple of the split chunk and the full capacity; splits 1, 2, the cap, auto"""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(1000 + d)
    cap = 640
    lens = [0, 1, 31, 32, 33, 437, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    splits = [1, 2, 128, 0]
    n = 0
    for h, hk in ((8, 8), (16, 4), (12, 1), (6, 2)):
        k, v = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
        for sq in (1, 2, 4, 16, 33):
            q = _rand((b, sq, h, d), dt, gen, gpu)
            for causal, windows in ((True, WINDOWS_CAUSAL), (False, WINDOWS_OPEN)):
                for window in windows[n % 2::2]:            # every other window per (heads, seqlen_q), alternating
                    ns = splits[n % len(splits)]
                    n += 1
                    out, lse = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True,
                                                         window_size=window)
                    tag = f"{dtname} d{d} h{h}/{hk} sq{sq} causal={causal} w={window} ns={ns}"
                    check_window_rows(out, lse, q, k, v, lens, window, causal, dtname, tag)


@pytest.mark.parametrize("num_splits", [1, 2, 128, 0])
def test_window_4095_long_cache(gpu, num_splits):
    """the usual "last 4096 keys" window over an 8192-key cache; lengths around the window; seqlen_q 1 and 16; contiguous and paged alike"""
    dt, d, h, hk, cap = torch.float16, 128, 32, 8, 8192
    gen = torch.Generator(device=gpu).manual_seed(2000 + num_splits)
    lens = [0, 1, 4095, 4096, 4097, 5001, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    for sq in (1, 16):
        q = _rand((b, sq, h, d), dt, gen, gpu)
        kn, vn = _poison_unseen(k, v, lens, sq, (4095, 0), True)
        out, lse = F.flash_attn_with_kvcache(q, kn, vn, cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True,
                                             window_size=(4095, 0))
        check_window_rows(out, lse, q, k, v, lens, (4095, 0), True, "fp16", f"4095 sq{sq} ns={num_splits}")
        kp, vp, table, _ = _page(kn, vn, 256, 7 + sq)
        out_p, lse_p = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True,
                                                 window_size=(4095, 0), block_table=table)
        assert _same(out_p, out) and torch.equal(lse_p, lse), sq


@pytest.mark.parametrize("causal", [True, False])
def test_window_edges_at_every_residue(gpu, causal):
    """window edges at every residue mod 32 around a split boundary: 64 sequences of lengths 1000 .. 1063 put the lower edge (and, with a
    right side, the upper edge) at every residue of the base and of the split chunks"""
    dt, d, h, hk = torch.bfloat16, 64, 4, 2
    gen = torch.Generator(device=gpu).manual_seed(3000 + int(causal))
    cap = 1088
    lens = list(range(1000, 1064))
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    sq = 3
    q = _rand((b, sq, h, d), dt, gen, gpu)
    windows = [(600, 0), (159, 0), (160, 0), (161, 0)] if causal else [(600, -1), (159, 1), (161, 0), (300, 1)]
    for window in windows:
        for ns in (2, 3, 4, 0):
            kn, vn = _poison_unseen(k, v, lens, sq, window, causal)
            out, lse = F.flash_attn_with_kvcache(q, kn, vn, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, window_size=window)
            check_window_rows(out, lse, q, k, v, lens, window, causal, "bf16", f"edges w={window} ns={ns} causal={causal}")


@pytest.mark.parametrize("P", [16, 48, 256])
def test_paged_window_bits_and_never_read(gpu, P):
    """a windowed paged call gives the bits of the windowed contiguous call over the same logical cache; pool rows below the window and
    at or past L are NaN, and the table entries of pages wholly before the window point at a NaN-filled page"""
    dt, d, h, hk = torch.float16, 128, 16, 4
    gen = torch.Generator(device=gpu).manual_seed(4000 + P)
    cap = 1536 if P != 48 else 1440
    lens = [0, 1, 100, 700, 1001, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    for sq, window, causal in ((1, (255, 0), True), (4, (100, -1), False), (16, (300, 0), True), (2, (64, 5), False)):
        q = _rand((b, sq, h, d), dt, gen, gpu)
        kn, vn = _poison_unseen(k, v, lens, sq, window, causal)
        kp, vp, table, spare = _page(kn, vn, P, 11 * P + sq)
        nan_page = spare[0]
        for i, L in enumerate(lens):
            lo, _ = _bounds(L, sq, 0, window, causal)
            table[i, : lo // P] = nan_page                  # pages wholly before the window
        for ns in (1, 2, 0):
            out_c, lse_c = F.flash_attn_with_kvcache(q, kn, vn, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True,
                                                     window_size=window)
            out_p, lse_p = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True,
                                                     window_size=window, block_table=table)
            assert _same(out_p, out_c) and torch.equal(lse_p, lse_c), (P, sq, window, ns)
            check_window_rows(out_p, lse_p, q, k, v, lens, window, causal, "fp16", f"paged P{P} sq{sq} w={window} ns={ns}")


@pytest.mark.parametrize("paged", [False, True])
def test_append_with_window(gpu, paged):
    """k / v appended in the same call are written where they belong and attended through the window"""
    dt, d, h, hk, sn = torch.bfloat16, 128, 8, 2, 5
    P, cap = 16, 256
    gen = torch.Generator(device=gpu).manual_seed(5000 + int(paged))
    base = [0, 3, 60, 200, cap - sn]
    b = len(base)
    cs = torch.tensor(base, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    kn, vn = _rand((b, sn, hk, d), dt, gen, gpu), _rand((b, sn, hk, d), dt, gen, gpu)
    q = _rand((b, sn, h, d), dt, gen, gpu)
    lens = [c + sn for c in base]
    want_k, want_v = k.clone(), v.clone()
    for i, c in enumerate(base):
        want_k[i, c:c + sn], want_v[i, c:c + sn] = kn[i], vn[i]
    for window, causal in (((7, 0), True), ((20, 2), False)):
        if paged:
            kc, vc, table, _ = _page(k, v, P, 17, fill=0.0)
            out, lse = F.flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=cs, causal=causal, return_softmax_lse=True, window_size=window,
                                                 block_table=table)
            nb = kc.shape[0]
            got_k = kc[table.long().clamp(0, nb - 1)].reshape(b, cap, hk, d)
            got_v = vc[table.long().clamp(0, nb - 1)].reshape(b, cap, hk, d)
        else:
            kc, vc = k.clone(), v.clone()
            out, lse = F.flash_attn_with_kvcache(q, kc, vc, kn, vn, cache_seqlens=cs, causal=causal, return_softmax_lse=True, window_size=window)
            got_k, got_v = kc, vc
        assert _same(got_k, want_k) and _same(got_v, want_v), (paged, window)
        assert cs.tolist() == base
        check_window_rows(out, lse, q, want_k, want_v, lens, window, causal, "bf16", f"append paged={paged} w={window}")


@pytest.mark.parametrize("num_splits", [1, 2, 0])
def test_nan_contract_within_the_window(gpu, num_splits):
    """a NaN query row, or a NaN K row inside a row's window, makes that row's O and LSE NaN (fp64 math: the same rows); a NaN K / V row
    below every window leaves every row finite and correct"""
    dt, d, h, hk, cap, sq = torch.float16, 64, 8, 2, 1024, 4
    gen = torch.Generator(device=gpu).manual_seed(6000 + num_splits)
    lens = [900, 1024, 500]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    window = (200, 0)
    k, v = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, sq, h, d), dt, gen, gpu)
    # below every window: poison K and V rows, the result is the clean one
    kn, vn = k.clone(), v.clone()
    kn[0, 600], vn[0, 650] = float("nan"), float("nan")
    kn[2, 10], vn[2, 295] = float("nan"), float("nan")          # b2's windows start at 500 - 4 - 200 + t = 296 + t (295: inside the 32-key step)
    out, lse = F.flash_attn_with_kvcache(q, kn, vn, cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True, window_size=window)
    check_window_rows(out, lse, q, k, v, lens, window, True, "fp16", f"nan below window ns={num_splits}")
    # a NaN query row and a NaN K row inside some rows' windows
    qn = q.clone()
    qn[1, 2, 3] = float("nan")
    kn = k.clone()
    kn[0, 899 - 3 - 200, 1] = float("nan")                       # b0: seen by row t = 0 only (lo_t = 900 - 4 + t - 200), KV head 1
    out, lse = F.flash_attn_with_kvcache(qn, kn, v, cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True, window_size=window)
    xo, xl = _exact(qn, kn, v, lens, window, True)
    want_nan = torch.isnan(xl)                                   # (b, h, sq)
    assert want_nan.any()
    assert torch.equal(torch.isnan(lse.cpu()), want_nan), num_splits
    assert torch.equal(torch.isnan(out.float().cpu()).any(-1), want_nan.permute(0, 2, 1)), num_splits
    # every other row is finite and correct
    finite = ~want_nan.permute(0, 2, 1)
    assert torch.isfinite(out.float().cpu()[finite]).all()
    ok = out.float().cpu()[finite].numpy()
    assert np.abs(ok - xo[finite].numpy()).max() < 5e-3


def test_identity_and_determinism(gpu):
    """window_size=(-1, -1) and a left side >= the capacity give the bits of the call without the argument; repeated windowed calls
    give the same bits"""
    dt, d, h, hk, cap = torch.float16, 128, 32, 8, 2048
    gen = torch.Generator(device=gpu).manual_seed(7000)
    lens = [2048, 1, 0, 1500]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k, v = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    for sq, causal in ((1, True), (5, False), (5, True)):
        q = _rand((b, sq, h, d), dt, gen, gpu)
        for ns in (0, 3):
            ref, ref_lse = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True)
            for window in ((-1, -1), (cap, -1), (cap + 100, 0), (cap - 1, sq - 1), (-1, 10**6)):
                if not causal and window[1] == 0:
                    continue
                out, lse = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, window_size=window)
                assert _same(out, ref) and torch.equal(lse, ref_lse), (sq, causal, ns, window)
            first = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, window_size=(100, 2))
            for _ in range(3):
                again = F.flash_attn_with_kvcache(q, k, v, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, window_size=(100, 2))
                assert _same(again[0], first[0]) and torch.equal(again[1], first[1])
    # positional calls of the binding are unchanged; the window is the trailing pair
    q = _rand((b, 1, h, d), dt, gen, gpu)
    o0, _ = F._C.fwd_kvcache(q, k, v, None, None, cs, True, 0, None)
    o1, _ = F._C.fwd_kvcache(q, k, v, None, None, cs, True, 0, None, -1, -1)
    assert _same(o0, o1)
    with pytest.raises(RuntimeError, match="window_size"):
        F._C.fwd_kvcache(q, k, v, None, None, cs, True, 0, None, -2, 0)


def test_graph_replay_sliding_window(gpu):
    """a 40-step windowed decode loop with append over a paged cache, captured once and replayed with advancing lengths: the window slides
    across page boundaries, and every step equals eager execution bit for bit"""
    dt, d, h, hk, P, cap, W = torch.float16, 128, 16, 4, 16, 512, 48
    gen = torch.Generator(device=gpu).manual_seed(8000)
    b = 2
    nb = b * cap // P + 4
    kp, vp = _rand((nb, P, hk, d), dt, gen, gpu), _rand((nb, P, hk, d), dt, gen, gpu)
    table = torch.randperm(nb, generator=torch.Generator().manual_seed(3))[: b * cap // P].view(b, cap // P).to(device=gpu, dtype=torch.int32)
    steps = 40
    qs = _rand((steps, b, 1, h, d), dt, gen, gpu)
    ks, vs = _rand((steps, b, 1, hk, d), dt, gen, gpu), _rand((steps, b, 1, hk, d), dt, gen, gpu)
    start = torch.tensor([30, 200], dtype=torch.int32, device=gpu)
    q, kn, vn = qs[0].clone(), ks[0].clone(), vs[0].clone()
    cs = start.clone()
    kp_e, vp_e = kp.clone(), vp.clone()

    def step():
        return F.flash_attn_with_kvcache(q, kp, vp, kn, vn, cache_seqlens=cs, causal=True, return_softmax_lse=True, window_size=(W - 1, 0),
                                         block_table=table)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    kp.copy_(kp_e)
    vp.copy_(vp_e)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = step()
    for i in range(steps):
        q.copy_(qs[i]); kn.copy_(ks[i]); vn.copy_(vs[i])
        cs.copy_(start + i)
        g.replay()
        out_e, lse_e = F.flash_attn_with_kvcache(qs[i], kp_e, vp_e, ks[i], vs[i], cache_seqlens=start + i, causal=True, return_softmax_lse=True,
                                                 window_size=(W - 1, 0), block_table=table)
        torch.cuda.synchronize()
        assert _same(out_g, out_e) and torch.equal(lse_g, lse_e), i
    assert _same(kp, kp_e) and _same(vp, vp_e)
    lens = (start + steps).tolist()
    logical_k = kp[table.long()].reshape(b, cap, hk, d)
    logical_v = vp[table.long()].reshape(b, cap, hk, d)
    check_window_rows(out_g, lse_g, qs[-1], logical_k, logical_v, lens, (W - 1, 0), True, "fp16", "graph last step")


def _median_ms(fns, rounds=5, iters=20):
    """interleaved medians (ms per call) of several callables, each timed over `iters` calls per round"""
    ts = [[] for _ in fns]
    for f in fns:
        f(0)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for j, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(iters):
                f(i)
            e1.record()
            e1.synchronize()
            ts[j].append(e0.elapsed_time(e1) / iters)
    return [statistics.median(t) for t in ts]


def test_window_reads_only_the_window(gpu):
    """b1 h32 h_k8 d128 fp16, one query, L = 131072, window (4095, 0): well under the unwindowed call on the same cache and close to an
    unwindowed call on a 4096-row cache.  Caches rotate so that the windows alone exceed the 256 MiB Infinity Cache (HBM-bound on both
    sides).  profiles/kvcache_window_bench.log measured 6.9x and 1.03; the bounds leave room for box-to-box spread."""
    dt, d, h, hk, L, W = torch.float16, 128, 32, 8, 131072, 4096
    dev = gpu
    n = 20                                                          # 20 windows x 16 MiB = 320 MiB; 20 full caches = 10 GiB
    big = [(torch.empty(1, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2), torch.empty(1, L, hk, d, device=dev, dtype=dt).uniform_(-2, 2))
           for _ in range(n)]
    small = [(torch.empty(1, W, hk, d, device=dev, dtype=dt).uniform_(-2, 2), torch.empty(1, W, hk, d, device=dev, dtype=dt).uniform_(-2, 2))
             for _ in range(n)]
    q = torch.randn(1, 1, h, d, device=dev, dtype=dt)
    cs_big = torch.full((1,), L, dtype=torch.int32, device=dev)
    cs_small = torch.full((1,), W, dtype=torch.int32, device=dev)
    with torch.no_grad():
        win = lambda i: F.flash_attn_with_kvcache(q, big[i % n][0], big[i % n][1], cache_seqlens=cs_big, causal=True, window_size=(W - 1, 0))
        full = lambda i: F.flash_attn_with_kvcache(q, big[i % n][0], big[i % n][1], cache_seqlens=cs_big, causal=True)
        short = lambda i: F.flash_attn_with_kvcache(q, small[i % n][0], small[i % n][1], cache_seqlens=cs_small, causal=True)
        # the windowed call on the big cache computes what the plain call on its last W rows computes
        ref = F.flash_attn_with_kvcache(q, big[0][0][:, L - W:], big[0][1][:, L - W:], cache_seqlens=cs_small, causal=True)
        assert (win(0).float() - ref.float()).abs().max().item() < 2e-3
        t_win, t_full, t_short = _median_ms([win, full, short])
    print(f"window (4095, 0) at L = 131072: {t_win:.4f} ms; unwindowed {t_full:.4f} ms ({t_full / t_win:.2f}x); 4096-row cache {t_short:.4f} ms "
          f"(windowed / short = {t_win / t_short:.2f})")
    assert t_full >= 3.0 * t_win, (t_win, t_full)
    assert t_win <= 1.5 * t_short, (t_win, t_short)
