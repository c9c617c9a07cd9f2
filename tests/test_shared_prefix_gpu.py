"""GPU: flash_attn_with_shared_prefix against flash_attn_with_kvcache's own contract.

b 3, sq 1 and 2, h 8 / h_k 2, d 64 and 128, pages of 16 plus a contiguous case, shared prefix 32 keys, lengths [32, 33, 75]: the first sequence has no suffix, so
its suffix rows are dead and only the merge's emptiness rule gives the right answer.  Which keys a row sees is decoded exactly (tests/_visibility.py: K = 0, one-hot
V codes, the all-ones code wherever no sequence owns the row); values go against the C oracle and fp64 math over the logical cache with the decode suites' own
check (tests/_util.py check_kvcache_rows) and NO extra allowance, which is tighter than the bound that check plus 2^-p max_i |o_i| for the rounding of the parts."""
import statistics

import pytest
import torch

import _util as U
import _visibility as V

pytestmark = pytest.mark.gpu

B, H, HK, P, CAP, LS = 3, 8, 2, 16, 96, 32
LENS = (32, 33, 75)                 # cache_seqlens as the call gets them (before an append)
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _F():
    import flash_attn_turing as F

    return F


def held_back(sq, causal):
    """under causal with seqlen_q > 1 the last seqlen_q - 1 keys of the prefix (rounded up to 16) are not visible to every row and stay with the sequences' own
    parts: in a CONTIGUOUS cache those rows are read from each sequence's own batch entry (in a paged one they are the shared pages either way)"""
    return -(-(sq - 1) // 16) * 16 if causal else 0


# ---- 1. visibility, exactly --------------------------------------------------------------------------------------------------------------------

def share_prefix_(c, v, table):
    """make the first LS keys of every sequence the same physical rows - those of sequence 0 - and put the all-ones code wherever no sequence owns a row any more"""
    raw = v.view(torch.uint8) if c.fp8 else v              # (an 8-bit cache is patched through its bytes)
    bad = V.BAD * V.FP8_ONE if c.fp8 else float(V.BAD)
    if table is not None:
        n = LS // c.page
        raw[table[1:, :n].flatten().long()] = bad
        table[:, :n] = table[0, :n].clone()
    else:
        raw[1:, :LS - held_back(c.sq[0], c.causal)] = bad        # batch entry 0's rows stand for all: the others' are never read
    return table


def probe(c, dev):
    F = _F()
    V.check_conditions(c)
    dt = V.torch_dtype(c.dtype)
    gen = torch.Generator(device="cpu").manual_seed(len(c.name) * 31 + sum(c.lens))
    b, sq = len(c.lens), c.sq[0]
    q = torch.randn(b, sq, c.h, c.d, generator=gen).to(dev, dt)
    k, v, table = V.build_cache(c, dev, gen)
    table = share_prefix_(c, v, table)
    before = [L - sq if c.append else L for L in c.lens]
    assert all(x >= LS for x in before)
    kw = dict(cache_seqlens=torch.tensor(before, dtype=torch.int32, device=dev), causal=c.causal, block_table=table, return_softmax_lse=True)
    if c.append:
        pos = torch.tensor([L - sq + t for L in c.lens for t in range(sq)], dtype=torch.long, device=dev)
        v_new = V.code_tensor(c.d, c.cap, dev)[pos].to(dt).unsqueeze(1).expand(b * sq, c.hk, c.d).contiguous().view(b, sq, c.hk, c.d)
        kw.update(k=torch.zeros_like(v_new), v=v_new)
    if c.fp8:
        kw.update(k_descale=torch.full((b, c.hk), V.K_DESCALE, dtype=torch.float32, device=dev), v_descale=torch.ones(b, c.hk, dtype=torch.float32, device=dev))
    out, lse = F.flash_attn_with_shared_prefix(q, k, v, LS, **kw)
    assert out.shape == (b, sq, c.h, c.d) and lse.shape == (b, c.h, sq)
    n_dec, hist_dec = V.decode(out.reshape(b * sq, c.h, c.d), lse.permute(0, 2, 1).reshape(b * sq, c.h), torch.zeros(c.h, dtype=torch.long))
    V.assert_signature(c, n_dec, hist_dec, *V.expected(c))
    return n_dec


def vis_cases():
    out = []
    for d in (64, 128):
        for sq in (1, 2):
            for append in (False, True):
                for causal in (False, True):
                    lens = tuple(L + sq if append else L for L in LENS)
                    dt = "fp16" if (d + sq + append + causal) % 2 else "bf16"
                    out.append(V.Case("shared_prefix", f"d{d}_sq{sq}_{'append' if append else 'read'}_{'causal' if causal else 'full'}_{dt}", lens, (sq,) * B, d=d, dtype=dt,
                                      page=P, h=H, hk=HK, append=append, causal=causal, cap=CAP))
    out.append(V.Case("shared_prefix", "contiguous_sq2_causal", tuple(L + 2 for L in LENS), (2,) * B, d=64, dtype="bf16", page=0, h=H, hk=HK, append=True, causal=True, cap=CAP))
    out.append(V.Case("shared_prefix", "contiguous_sq1", LENS, (1,) * B, d=128, dtype="fp16", page=0, h=H, hk=HK, cap=CAP))
    out.append(V.Case("shared_prefix", "fp8_sq2_append", tuple(L + 2 for L in LENS), (2,) * B, d=128, dtype="fp16", fp8=True, page=P, h=H, hk=HK, append=True, cap=CAP))
    out.append(V.Case("shared_prefix", "fp8_sq1_causal", LENS, (1,) * B, d=64, dtype="bf16", fp8=True, page=P, h=H, hk=HK, causal=True, cap=CAP))
    return out


@pytest.mark.parametrize("c", vis_cases(), ids=lambda c: c.name)
def test_every_row_sees_exactly_the_keys_of_the_plain_call(gpu, c):
    """with K = 0 the merged LSE decodes to the integer n of visible keys across the boundary at the shared prefix, and out * n to the histogram of their one-hot
    codes: a key read twice, a key of the boundary lost, or a row of a page no sequence owns would change an integer"""
    n_dec = probe(c, gpu)
    sq = c.sq[0]
    assert n_dec.shape == (B * sq, c.h)
    if not c.causal:
        assert n_dec[:sq].eq(c.lens[0]).all().item() and n_dec[-1].eq(c.lens[2]).all().item()


# ---- 2. values ---------------------------------------------------------------------------------------------------------------------------------------

def value_inputs(d, sq, dtname, paged, fp8, append, dev, seed, causal=False):
    """random logical caches (b, CAP, hk, d) whose first LS rows are sequence 0's, as a pool under a random table (prefix pages shared, spare pages NaN) or
    contiguous (batch entries 1 .. hold NaN in the rows the call must not read); -> q, k_cache, v_cache, kw, k_log, v_log (float, what attention should see)"""
    dt = DT[dtname]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    q = torch.randn(B, sq, H, d, generator=gen).to(dev, dt)
    k_log, v_log = (torch.randn(B, CAP, HK, d, generator=gen).to(dev, dt) for _ in range(2))
    k_log[1:, :LS], v_log[1:, :LS] = k_log[0, :LS], v_log[0, :LS]
    kw = dict(cache_seqlens=torch.tensor(LENS, dtype=torch.int32, device=dev))
    if fp8:
        ks, vs = torch.full((B, HK), 0.5, device=dev), torch.full((B, HK), 0.25, device=dev)
        k8, v8 = ((x.float() / s[:, None, :, None]).to(torch.float8_e4m3fn) for x, s in ((k_log, ks), (v_log, vs)))
        k_log, v_log = k8.float() * ks[:, None, :, None], v8.float() * vs[:, None, :, None]
        kw.update(k_descale=ks, v_descale=vs)
        k_store, v_store = k8, v8
    else:
        k_store, v_store = k_log.clone(), v_log.clone()
    if append:
        k_new, v_new = (torch.randn(B, sq, HK, d, generator=gen).to(dev, dt) for _ in range(2))
        kw.update(k=k_new, v=v_new)
    if paged:
        npg, nshared = CAP // P, LS // P
        nb = nshared + B * (npg - nshared) + 4
        perm = torch.randperm(nb, generator=gen)
        table = torch.empty(B, npg, dtype=torch.int32)
        table[:, :nshared] = perm[:nshared]
        table[:, nshared:] = perm[nshared:nshared + B * (npg - nshared)].view(B, -1)
        table = table.to(dev)
        pools = []
        for x in (k_store, v_store):
            raw = x.view(torch.uint8 if fp8 else torch.int16)                              # (scattered through the bits: spare pages hold a NaN pattern)
            pool = torch.full((nb, P, HK, d), 0x7F if fp8 else U.SENT16, dtype=raw.dtype, device=dev)
            pool[table.flatten().long()] = raw.view(B * npg, P, HK, d)
            pools.append(pool.view(x.dtype))
        kw.update(block_table=table)
        k_store, v_store = pools
    else:
        for x in (k_store, v_store):
            x.view(torch.uint8 if fp8 else torch.int16)[1:, :LS - held_back(sq, causal)] = 0x7F if fp8 else U.SENT16
    return q, k_store, v_store, kw, k_log.float(), v_log.float()


VALUE_CASES = [(64, 1, "fp16", True, False, False, False), (64, 2, "bf16", True, False, True, True), (128, 1, "bf16", True, False, True, False),
               (128, 2, "fp16", True, False, False, True), (128, 2, "bf16", False, False, True, False), (64, 1, "fp16", False, False, False, True),
               (128, 2, "fp16", True, True, True, True), (64, 1, "bf16", True, True, False, False)]


@pytest.mark.parametrize("d,sq,dtname,paged,fp8,append,causal", VALUE_CASES)
def test_values_against_the_oracle_over_the_logical_cache(gpu, d, sq, dtname, paged, fp8, append, causal):
    F = _F()
    q, kc, vc, kw, k_log, v_log = value_inputs(d, sq, dtname, paged, fp8, append, gpu, 1234 + d + sq, causal)
    out, lse = F.flash_attn_with_shared_prefix(q, kc, vc, LS, causal=causal, return_softmax_lse=True, **kw)
    lens = list(LENS)
    if append:
        # what the next call sees: the appended rows as the cache stores them
        for i, L in enumerate(LENS):
            for name, log, new in (("k", k_log, kw["k"]), ("v", v_log, kw["v"])):
                row = new[i].float()
                if fp8:
                    s = kw[name + "_descale"][i][None, :, None]
                    row = (row / s).to(torch.float8_e4m3fn).float() * s
                log[i, L:L + sq] = row
        lens = [L + sq for L in LENS]
    U.check_kvcache_rows(out, lse, q, k_log, v_log, lens, causal, dtname, f"shared prefix d{d} sq{sq} paged{paged} fp8{fp8} append{append} causal{causal}",
                         scale=1.0)
    # the plain call on the same arguments, where the caller's cache lets it run (a shared table): within the same tolerance of each other
    if paged and not append:
        ref, ref_lse = F.flash_attn_with_kvcache(q, kc, vc, return_softmax_lse=True, causal=causal, **kw)
        m = U.error_metrics(out.float().cpu().numpy(), ref.float().cpu().numpy())
        assert m["max_abs"] <= U.TOL[dtname]["max_abs"] and (lse - ref_lse).abs().max().item() <= U.LSE_TOL, m


def test_prefix_len_0_is_the_plain_call_bit_for_bit(gpu):
    F = _F()
    q, kc, vc, kw, _, _ = value_inputs(128, 2, "fp16", True, False, False, gpu, 5)
    for causal in (False, True):
        a, la = F.flash_attn_with_shared_prefix(q, kc, vc, 0, causal=causal, return_softmax_lse=True, **kw)
        b_, lb = F.flash_attn_with_kvcache(q, kc, vc, causal=causal, return_softmax_lse=True, **kw)
        assert torch.equal(U.bits(a), U.bits(b_)) and torch.equal(U.bits(la), U.bits(lb))
    assert F.flash_attn_with_shared_prefix(q, kc, vc, 0, **kw).shape == q.shape


def test_graph_replay_with_new_lengths(gpu):
    """captured once, replayed with other lengths (a sequence without a suffix moves around): the replay equals the eager call of the moment bit for bit - the
    three launches read lengths and tables on the device - and meets the oracle"""
    F = _F()
    q, kc, vc, kw, k_log, v_log = value_inputs(128, 1, "fp16", True, False, False, gpu, 77)
    cs = kw["cache_seqlens"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_shared_prefix(q, kc, vc, LS, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_shared_prefix(q, kc, vc, LS, return_softmax_lse=True, **kw)
    for lens in (list(LENS), [96, 32, 40], [33, 64, 32]):
        cs.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        out_e, lse_e = F.flash_attn_with_shared_prefix(q, kc, vc, LS, return_softmax_lse=True, **kw)
        assert torch.equal(U.bits(out_g), U.bits(out_e)) and torch.equal(U.bits(lse_g), U.bits(lse_e)), lens
        U.check_kvcache_rows(out_g, lse_g, q, k_log, v_log, lens, False, "fp16", f"shared prefix graph {lens}")


# ---- 3. the purpose ------------------------------------------------------------------------------------------------------------------------------------

def test_shared_prefix_is_not_slower_than_the_plain_call_at_b64_prefix_8192(gpu):
    """b 64, sq 1, h 32 / h_k 8, d 128, fp16, pages of 16, a shared prefix of 8192 keys and 128 own keys per sequence: the median of 5 interleaved rounds of the new
    call must not exceed that of flash_attn_with_kvcache on the same tables.  The bound is 1.0 and carries no margin.  The plain call walks 64 x 8320 keys in
    quarter-filled 16-row tiles; the composite walks 8192 keys once in full 64-row tiles plus 64 x 128.  The ratio is printed (README.md records it)."""
    F = _F()
    dt, d, h, hk, b, pre, own = torch.float16, 128, 32, 8, 64, 8192, 128
    gen = torch.Generator().manual_seed(4242)
    n_pre, n_own = pre // P, own // P
    nb = n_pre + b * n_own
    kp, vp = (torch.randn(nb, P, hk, d, generator=gen).to(dt).to(gpu) for _ in range(2))
    perm = torch.randperm(nb, generator=gen)
    table = torch.cat([perm[:n_pre].unsqueeze(0).expand(b, n_pre), perm[n_pre:].view(b, n_own)], dim=1).to(torch.int32).contiguous().to(gpu)
    q = torch.randn(b, 1, h, d, generator=gen).to(dt).to(gpu)
    cs = torch.full((b,), pre + own, dtype=torch.int32, device=gpu)
    new = lambda: F.flash_attn_with_shared_prefix(q, kp, vp, pre, cache_seqlens=cs, block_table=table)
    plain = lambda: F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, block_table=table)
    a, r = new(), plain()
    m = U.error_metrics(a.float().cpu().numpy(), r.float().cpu().numpy())
    assert m["max_abs"] <= U.TOL["fp16"]["max_abs"], m
    torch.cuda.synchronize()
    tn, tp = [], []
    for _ in range(5):
        for fn, ts in ((new, tn), (plain, tp)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / 3)
    w, n = statistics.median(tn), statistics.median(tp)
    line = f"test_shared_prefix_is_not_slower: b{b} sq1 h{h}/{hk} d{d} fp16 pages of {P} prefix {pre} own {own}: shared prefix {w:.4f} ms, plain {n:.4f} ms, ratio {w / n:.3f}"
    print(line)
    assert w <= n, line
