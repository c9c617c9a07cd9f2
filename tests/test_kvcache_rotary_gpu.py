"""GPU: rotary embedding fused into the append of flash_attn_with_kvcache (rotary_cos / rotary_sin / rotary_interleaved).

The contract under test: a rotary call equals, BIT FOR BIT in out, lse and every cache byte, the same call without rotary on q_rot / k_rot
computed by the formula - here by rotate_ref (tests/test_kvcache_rotary_cpu.py: torch on the CPU, never the library under test).  So every
value check below is an exact comparison; the only tolerance in this file is the project's own, through _util.check_kvcache_rows, which ties
the rotated call to the C oracle as well.  Where NaN is planted, NaN positions are compared and bits everywhere else (payloads may differ
between torch and the GPU)."""
import ctypes

import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_rotary_cpu import rotate_ref

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
F8 = torch.float8_e4m3fn


def quantise(x, descale):
    """the append contract of the 8-bit cache (tests/test_kvcache_fp8_gpu.py's rule) with torch on the CPU: e4m3_rne(clamp(float(x) / descale,
    -448, 448)); x (b, s, hk, d) of q's dtype, descale (b, hk) or None"""
    xf = x.detach().float().cpu()
    if descale is not None:
        xf = xf / descale.detach().float().cpu()[:, None, :, None]
    return xf.clamp(-448.0, 448.0).to(F8)


def _rand(shape, gen, dt, scale=1.0):
    return (torch.randn(*shape, dtype=torch.float32, generator=gen) * scale).to(dt)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _nan_mask(t):
    if t.dtype == F8:
        return (_bits(t) & 0x7F) == 0x7F
    return torch.isnan(t)


def assert_same(a, b, what):
    """bit equality; where both hold NaN the payload is not compared"""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    a, b = a.detach().cpu(), b.detach().cpu()
    if torch.equal(_bits(a), _bits(b)):
        return
    na, nb = _nan_mask(a), _nan_mask(b)
    assert torch.equal(na, nb), f"{what}: NaN positions differ ({int(na.sum())} vs {int(nb.sum())})"
    diff = ((_bits(a) != _bits(b)) & ~na).nonzero()
    assert diff.numel() == 0, f"{what}: {diff.shape[0]} elements differ, first at {diff[0].tolist()}: {a[tuple(diff[0])].item()} vs {b[tuple(diff[0])].item()}"


def tables(seqlen_ro, rotary_dim, dt, base=10000.0):
    """cos / sin (seqlen_ro, rotary_dim / 2) of a RoPE with the usual frequencies, rounded to dt"""
    inv = base ** (-torch.arange(0, rotary_dim, 2, dtype=torch.float64) / rotary_dim)
    ang = torch.arange(seqlen_ro, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(dt), ang.sin().to(dt)


def positions(lens, rows, per_row, seqlen_ro):
    """(b, rows): max(L, 0) + t (or max(L, 0) for every t), clamped to the tables"""
    base = torch.tensor([max(int(x), 0) for x in lens], dtype=torch.long)[:, None]
    t = torch.arange(rows, dtype=torch.long)[None, :] if per_row else torch.zeros(1, rows, dtype=torch.long)
    return (base + t).clamp(max=seqlen_ro - 1)


def q_rule(causal, window):
    return bool(causal) or tuple(window) != (-1, -1)


def rotary_and_plain(gpu, q, k_new, v_new, k_cache, v_cache, lens, cos, sin, inter, *, causal=False, window=(-1, -1), num_splits=0, block_table=None,
                     k_descale=None, v_descale=None, q_per_row=None, tag=""):
    """run the rotary call and the plain call on rotate_ref'd q / k over clones of the same caches (all arguments live on the CPU or the GPU;
    the calls get GPU copies); assert out, lse and both caches agree bit for bit; returns (out, lse, k_cache, v_cache, q_rot, k_rot) of the rotary call"""
    dev = lambda t: None if t is None else t.to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    ro = cos.shape[0]
    per_row = q_rule(causal, window) if q_per_row is None else q_per_row
    q_rot = rotate_ref(q, cos, sin, positions(lens, q.shape[1], per_row, ro), inter)
    k_rot = rotate_ref(k_new, cos, sin, positions(lens, k_new.shape[1], True, ro), inter)
    kw = dict(cache_seqlens=cs, causal=causal, window_size=window, num_splits=num_splits, return_softmax_lse=True, block_table=dev(block_table),
              k_descale=dev(k_descale), v_descale=dev(v_descale))
    ka, va, kb, vb = dev(k_cache).clone(), dev(v_cache).clone(), dev(k_cache).clone(), dev(v_cache).clone()
    qg, kng, vng, cg, sg = dev(q), dev(k_new), dev(v_new), dev(cos), dev(sin)
    keep = [t.clone() for t in (qg, kng, vng, cg, sg)]
    out_r, lse_r = F.flash_attn_with_kvcache(qg, ka, va, k=kng, v=vng, rotary_cos=cg, rotary_sin=sg, rotary_interleaved=inter, **kw)
    out_p, lse_p = F.flash_attn_with_kvcache(dev(q_rot), kb, vb, k=dev(k_rot), v=vng, **kw)
    torch.cuda.synchronize()
    assert_same(out_r, out_p, f"{tag}: out")
    assert_same(lse_r, lse_p, f"{tag}: lse")
    assert_same(ka, kb, f"{tag}: k_cache")
    assert_same(va, vb, f"{tag}: v_cache")
    for t, t0, name in zip((qg, kng, vng, cg, sg), keep, ("q", "k", "v", "rotary_cos", "rotary_sin")):
        assert torch.equal(_bits(t), _bits(t0)), f"{tag}: {name} was written"
    assert cs.tolist() == [int(x) for x in lens], "cache_seqlens must not be updated by the library"
    return out_r, lse_r, ka, va, q_rot, k_rot


def expected_cache(cache, rows, lens):
    """the logical cache (b, cap, hk, d) after `rows` (b, sn, hk, d; same dtype) landed at lens[i] .. lens[i] + sn - 1 (rows past the capacity dropped)"""
    e = cache.detach().cpu().clone()
    rows = rows.detach().cpu()
    for i, L in enumerate(lens):
        L = max(int(L), 0)
        n = min(rows.shape[1], e.shape[1] - L)
        if n > 0:
            _bits(e)[i, L:L + n] = _bits(rows)[i, :n]
    return e


# ---- 7. the grid ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_grid_equals_the_plain_call_on_rotated_inputs(gpu, dtname, d):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(100 + d + (dtname == "bf16"))
    cap = 320
    ro = cap + 8
    cases = 0
    for h, hk in ((8, 8), (32, 8), (32, 1)):
        for sq, sn in ((1, 1), (2, 2), (4, 4), (16, 16), (4, 1), (1, 3)):
            lens = [0, 1, 63, 64, 65, cap - sn]
            b = len(lens)
            k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
            q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sn, hk, d), gen, dt), _rand((b, sn, hk, d), gen, dt)
            for rd in sorted({16, 32, d // 2, d}):
                cos, sin = tables(ro, rd, dt)
                for inter in (False, True):
                    for causal, window in ((False, (-1, -1)), (True, (-1, -1)), (False, (37, 0))):
                        ns = (0, 1, 3)[(cases + cases // 3) % 3]
                        tag = f"{dtname} d{d} h{h}/{hk} sq{sq} sn{sn} rd{rd} inter={inter} causal={causal} win={window} ns={ns}"
                        out, lse, ka, va, q_rot, k_rot = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=causal, window=window,
                                                                          num_splits=ns, tag=tag)
                        # the cache straight from the formula (not through the library's plain append): rotated rows in place, every other byte as it was
                        assert_same(ka, expected_cache(k0, k_rot, lens).to(gpu), tag + ": k_cache against rotate_ref")
                        assert_same(va, expected_cache(v0, v_new, lens).to(gpu), tag + ": v_cache against v")
                        if rd < d:
                            assert torch.equal(_bits(ka.cpu())[0, :sn, :, rd:], _bits(k_new)[0, :, :, rd:]), tag + ": elements past rotary_dim pass through"
                        assert not torch.equal(_bits(k_rot)[2], _bits(k_new)[2]), tag + ": the rotation does something"
                        cases += 1
    assert cases == 3 * 6 * len({16, 32, d // 2, d}) * 2 * 3


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_rotated_call_against_the_oracle(gpu, dtname, d, causal):
    """the rotary call's out / lse against the C oracle on rotate_ref'd q over the cache that rotate_ref says it leaves (_util.check_kvcache_rows:
    the project's stated tolerance)"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(7 + d)
    cap, h, hk, sq = 600, 32, 8, 4
    lens = [0, 1, 63, 64, 65, 333, cap - sq]
    b = len(lens)
    k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
    q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sq, hk, d), gen, dt), _rand((b, sq, hk, d), gen, dt)
    for rd, inter in ((d, False), (d // 2, True)):
        cos, sin = tables(cap, rd, dt)
        out, lse, ka, va, q_rot, k_rot = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=causal, tag=f"oracle {dtname} d{d}")
        k_exp, v_exp = expected_cache(k0, k_rot, lens), expected_cache(v0, v_new, lens)
        U.check_kvcache_rows(out, lse, q_rot, k_exp, v_exp, [L + sq for L in lens], causal, dtname, f"rotary {dtname} d{d} rd{rd} inter={inter} causal={causal}")


# ---- 8. the query-position rule --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_query_position_rule(gpu, dtname):
    """no mask and no window: every query row at cache_seqlens[i]; causal=True or any window_size other than (-1, -1) - also one that the host
    normalises away - : row t at cache_seqlens[i] + t"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(3)
    d, h, hk, sq, cap = 128, 8, 4, 4, 256
    lens = [0, 17, 100, cap - sq]
    b = len(lens)
    k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
    q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sq, hk, d), gen, dt), _rand((b, sq, hk, d), gen, dt)
    cos, sin = tables(cap, d, dt, base=50.0)                   # a small base: neighbouring positions differ in every pair
    for inter in (False, True):
        for causal, window, per_row in ((False, (-1, -1), False), (True, (-1, -1), True), (False, (-1, 0), True), (True, (-1, 0), True), (False, (cap + 5, -1), True),
                                        (False, (cap - 1, 7), True), (False, (37, 0), True)):
            tag = f"{dtname} causal={causal} window={window} inter={inter}"
            out = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=causal, window=window, q_per_row=per_row, tag=tag)[0]
            # ... and the other rule gives another result, so the comparison above tells the two apart
            cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
            q_other = rotate_ref(q, cos, sin, positions(lens, sq, not per_row, cap), inter)
            k_rot = rotate_ref(k_new, cos, sin, positions(lens, sq, True, cap), inter)
            out_o = F.flash_attn_with_kvcache(q_other.to(gpu), k0.to(gpu), v0.to(gpu), k=k_rot.to(gpu), v=v_new.to(gpu), cache_seqlens=cs, causal=causal, window_size=window)
            assert not torch.equal(_bits(out[:, 1:]), _bits(out_o[:, 1:])), tag
            assert torch.equal(_bits(out[:, 0]), _bits(out_o[:, 0])), tag     # row 0 sits at cache_seqlens[i] under both rules


# ---- 9. paged and FP8 ------------------------------------------------------------------------------------------------------------------------

def page(k, v, P, seed, share=(), extra=2, fill=0xFF):
    """a pool + block table holding the logical caches (b, cap, hk, d) (any element size), pages by a random permutation; unreferenced pages hold
    the byte `fill` (NaN in every format here); share = ((i, j, col), ...): sequence j reads column col through sequence i's page"""
    b, cap, hk, d = k.shape
    cols = cap // P
    nb = b * cols + extra
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))
    table = perm[: b * cols].view(b, cols).to(torch.int32)
    for i, j, col in share:
        table[j, col] = table[i, col]
    idx = table.long()
    pools = []
    for t in (k, v):
        pool = torch.full((nb, P, hk, d * t.element_size()), fill, dtype=torch.uint8)
        pool[idx] = t.detach().cpu().contiguous().view(torch.uint8).reshape(b, cols, P, hk, d * t.element_size())
        pools.append(pool.view(t.dtype))
    return pools[0], pools[1], table


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("P", [16, 48, 256])
@pytest.mark.parametrize("fp8", [False, True])
def test_paged_and_fp8_caches(gpu, dtname, P, fp8):
    """appended rows crossing a page, pages shared for reading, 8-bit caches with and without descales: pool bytes equal the formula (quantised
    by the 8-bit cache's rule where the cache is 8-bit), and the paged call gives the bits of the contiguous one"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(40 + P)
    cap = {16: 320, 48: 336, 256: 768}[P]
    sn = 5
    lens = [P - 2, 0, 2 * P - 3, cap - sn]                    # rows P - 2 .. P + 2 and 2 P - 3 .. 2 P + 1 cross a page
    b = len(lens)
    for d, h, hk, rd, inter, causal, ds in ((128, 32, 8, 64, False, True, True), (64, 8, 8, 64, True, False, False), (128, 8, 1, 16, True, True, True)):
        kds = vds = None
        if fp8 and ds:
            kds, vds = 0.25 * 16.0 ** torch.rand(b, hk, generator=gen), 0.25 * 16.0 ** torch.rand(b, hk, generator=gen)
            kds[0, 0] = 1.0
            kds[3], vds[3] = kds[2], vds[2]                       # (the shared page holds ONE set of codes)
        k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
        k0[3, :P], v0[3, :P] = k0[2, :P], v0[2, :P]           # sequences 2 and 3 share their first page (both are longer than it)
        if fp8:
            k0, v0 = quantise(k0, kds), quantise(v0, vds)
        q, k_new, v_new = _rand((b, sn, h, d), gen, dt), _rand((b, sn, hk, d), gen, dt, 3.0), _rand((b, sn, hk, d), gen, dt, 3.0)
        cos, sin = tables(cap, rd, dt)
        tag = f"{dtname} P{P} fp8={fp8} d{d} h{h}/{hk} rd{rd}"
        out_c, lse_c, kc, vc, q_rot, k_rot = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=causal, k_descale=kds, v_descale=vds,
                                                              tag=tag + " contiguous")
        k_rows, v_rows = (quantise(k_rot, kds), quantise(v_new, vds)) if fp8 else (k_rot, v_new)
        k_exp, v_exp = expected_cache(k0, k_rows, lens), expected_cache(v0, v_rows, lens)
        assert_same(kc, k_exp.to(gpu), tag + ": contiguous k_cache against the formula")
        assert_same(vc, v_exp.to(gpu), tag + ": contiguous v_cache against the formula")
        kp, vp, table = page(k0, v0, P, seed=5, share=((2, 3, 0),))
        assert table[2, 0] == table[3, 0]
        out_p, lse_p, kpa, vpa, _, _ = rotary_and_plain(gpu, q, k_new, v_new, kp, vp, lens, cos, sin, inter, causal=causal, block_table=table, k_descale=kds,
                                                        v_descale=vds, tag=tag + " paged")
        kpe, vpe, table_e = page(k_exp, v_exp, P, seed=5, share=((2, 3, 0),))
        assert torch.equal(table, table_e)
        assert_same(kpa, kpe.to(gpu), tag + ": pool K bytes against the formula")
        assert_same(vpa, vpe.to(gpu), tag + ": pool V bytes against the formula")
        assert_same(out_p, out_c, tag + ": paged out against contiguous")
        assert_same(lse_p, lse_c, tag + ": paged lse against contiguous")


# ---- 10. what is never read; the clamp ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("inter", [False, True])
def test_table_rows_that_are_not_addressed_are_never_read(gpu, dtname, inter):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(77)
    d, h, hk, cap, sq, sn, rd = 128, 32, 8, 512, 3, 2, 64
    lens = [0, 5, 250, cap - sn]
    b = len(lens)
    ro = cap + 13                                              # seqlen_ro > seqlen_cache
    k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
    q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sn, hk, d), gen, dt), _rand((b, sn, hk, d), gen, dt)
    cos, sin = tables(ro, rd, dt)
    for causal in (False, True):
        tag = f"{dtname} inter={inter} causal={causal}"
        want = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=causal, tag=tag)
        used = torch.zeros(ro, dtype=torch.bool)
        used[positions(lens, sn, True, ro).flatten()] = True
        used[positions(lens, sq, causal, ro).flatten()] = True
        assert 0 < int(used.sum()) < 20
        # NaN in every row that is not addressed, inside a wider buffer with NaN in the gaps between the rows (a strided view)
        wide_c, wide_s = torch.full((ro, rd + 8), float("nan"), dtype=dt), torch.full((ro, rd + 24), float("nan"), dtype=dt)
        cos_v, sin_v = wide_c[:, :rd // 2], wide_s[:, 16:16 + rd // 2]
        cos_v[used], sin_v[used] = cos[used], sin[used]
        cg, sg = wide_c.to(gpu)[:, :rd // 2], wide_s.to(gpu)[:, 16:16 + rd // 2]
        assert not cg.is_contiguous() and cg.stride(0) == rd + 8 and sg.stride(0) == rd + 24
        for cos_t, sin_t, what in ((cg, sg, "different row strides"), (cg, wide_c.to(gpu).clone()[:, :rd // 2].copy_(sin_v.to(gpu)), "one row stride")):
            ka, va = k0.to(gpu), v0.to(gpu)
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), ka, va, k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=gpu),
                                                 causal=causal, return_softmax_lse=True, rotary_cos=cos_t, rotary_sin=sin_t, rotary_interleaved=inter)
            for got, exp, name in zip((out, lse, ka, va), want[:4], ("out", "lse", "k_cache", "v_cache")):
                assert torch.equal(_bits(got), _bits(exp)), f"{tag} {what}: {name} changed when unused table rows hold NaN"
            assert not torch.isnan(out).any() and not torch.isnan(ka).any()


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_positions_are_clamped_to_the_tables(gpu, dtname):
    """seqlen_ro = seqlen_cache, seqlen_q = 4, seqlen_new = 1, causal, a full cache after the append: query positions seqlen_cache .. + 2 use
    table row seqlen_ro - 1; sentinel rows allocated behind the tables stay what they were and are not read"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(5)
    d, h, hk, cap, sq, sn = 64, 8, 2, 128, 4, 1
    lens = [cap - 1, 10, cap - 1]
    b = len(lens)
    k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
    q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sn, hk, d), gen, dt), _rand((b, sn, hk, d), gen, dt)
    cos, sin = tables(cap, d, dt, base=30.0)
    assert positions(lens, sq, True, cap).tolist()[0] == [cap - 1] * 4 and positions(lens, sq, True, cap).tolist()[1] == [10, 11, 12, 13]
    for inter in (False, True):
        want = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=True, tag=f"clamp {dtname} inter={inter}")
        bufs = []
        for t in (cos, sin):
            buf = torch.full((cap + 4, d // 2), U.SENT16, dtype=torch.int16).view(dt)
            buf[:cap] = t
            bufs.append(buf.to(gpu))
        ka, va = k0.to(gpu), v0.to(gpu)
        out, lse = F.flash_attn_with_kvcache(q.to(gpu), ka, va, k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=gpu), causal=True,
                                             return_softmax_lse=True, rotary_cos=bufs[0][:cap], rotary_sin=bufs[1][:cap], rotary_interleaved=inter)
        for got, exp, name in zip((out, lse, ka, va), want[:4], ("out", "lse", "k_cache", "v_cache")):
            assert torch.equal(_bits(got), _bits(exp)), name
        assert not torch.isnan(out).any()
        for buf in bufs:
            assert (_bits(buf[cap:]) == U.SENT16).all()


# ---- 11. inputs untouched, strided views, non-finite inputs -------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_strided_views_and_guard_bands(gpu, dtname):
    """q, k, v and the caches as views of larger buffers filled with a sentinel: same bits as the dense call, nothing outside the views written
    (inputs bit-identical after the call: rotary_and_plain checks that on every call of this file)"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(21)
    d, h, hk, cap, sq, sn = 128, 8, 4, 160, 3, 3
    lens = [0, 40, cap - sn]
    b = len(lens)
    k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
    q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sn, hk, d), gen, dt), _rand((b, sn, hk, d), gen, dt)
    cos, sin = tables(cap, 32, dt)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for inter in (False, True):
        want = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=True, tag=f"dense {dtname}")
        views, bufs = [], []
        for t in (q, k_new, v_new, k0, v0):
            buf, view, _ = U.guarded(tuple(t.shape), dt, gpu, (2, 2, 2, 16))
            view.copy_(t.to(gpu))
            views.append(view)
            bufs.append(buf)
        before = [bf.clone() for bf in bufs]
        qv, knv, vnv, kcv, vcv = views
        assert not qv.is_contiguous() and not kcv.is_contiguous()
        out, lse = F.flash_attn_with_kvcache(qv, kcv, vcv, k=knv, v=vnv, cache_seqlens=cs, causal=True, return_softmax_lse=True, rotary_cos=cos.to(gpu), rotary_sin=sin.to(gpu),
                                             rotary_interleaved=inter)
        for got, exp, name in zip((out, lse, kcv, vcv), want[:4], ("out", "lse", "k_cache", "v_cache")):
            assert torch.equal(_bits(got.contiguous()), _bits(exp)), name
        for i in range(3):
            assert torch.equal(_bits(bufs[i]), _bits(before[i])), "an input buffer was written"
        for i in (3, 4):                                       # the caches: only the view changed
            now, was = bufs[i].clone(), before[i].clone()
            _, vn, sl = U.guarded(tuple(k0.shape), dt, gpu, (2, 2, 2, 16))
            now[sl], was[sl] = 0, 0
            assert torch.equal(_bits(now), _bits(was)), "bytes outside the cache view were written"


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("fp8", [False, True])
def test_non_finite_inputs_follow_the_formula(gpu, dtname, fp8):
    """NaN / inf in k, in q and in a table row that IS used: NaN where the formula gives NaN, the formula's bits everywhere else"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(9)
    d, h, hk, cap, sq = 64, 8, 4, 96, 2
    lens = [0, 30, cap - sq]
    b = len(lens)
    k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
    if fp8:
        k0, v0 = quantise(k0, None), quantise(v0, None)
    q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sq, hk, d), gen, dt), _rand((b, sq, hk, d), gen, dt)
    cos, sin = tables(cap, 32, dt)
    k_new[0, 0, 0, 3], k_new[0, 1, 1, 17], k_new[1, 0, 2, 5], k_new[1, 1, 3, 40] = float("nan"), float("inf"), float("-inf"), float("nan")
    q[2, 0, 1, 2], q[2, 1, 5, 20] = float("inf"), float("nan")
    cos[31, 4], sin[cap - 1, 7] = float("nan"), float("inf")           # rows 31 (sequence 1, second row) and cap - 1 (sequence 2, second row) are used
    for inter in (False, True):
        for causal in (False, True):
            out, lse, ka, va, q_rot, k_rot = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, inter, causal=causal, tag=f"non-finite {dtname} fp8={fp8} inter={inter}")
            assert torch.isnan(k_rot).any() and torch.isnan(q_rot).any() and torch.isnan(out).any() and not torch.isnan(out).all()
            k_rows = quantise(k_rot, None) if fp8 else k_rot
            assert_same(ka, expected_cache(k0, k_rows, lens).to(gpu), "k_cache against the formula")


# ---- 12. graph capture ----------------------------------------------------------------------------------------------------------------------

def test_graph_capture_replays_with_new_lengths_and_tables(gpu):
    dt, d, h, hk, cap, sn = torch.float16, 128, 32, 8, 4096, 2
    gen = torch.Generator().manual_seed(13)
    b = 2
    k0, v0 = _rand((b, cap, hk, d), gen, dt).to(gpu), _rand((b, cap, hk, d), gen, dt).to(gpu)
    q, k_new, v_new = _rand((b, sn, h, d), gen, dt).to(gpu), _rand((b, sn, hk, d), gen, dt).to(gpu), _rand((b, sn, hk, d), gen, dt).to(gpu)
    cos_a, sin_a = tables(cap, d, dt)
    cos_b, sin_b = tables(cap, d, dt, base=500.0)
    cos, sin = cos_a.to(gpu), sin_a.to(gpu)
    cs = torch.tensor([100, 4000], dtype=torch.int32, device=gpu)
    kg, vg = k0.clone(), v0.clone()
    kw = dict(k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, rotary_cos=cos, rotary_sin=sin, rotary_interleaved=False)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, kg, vg, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, kg, vg, **kw)
    for lens, (ct, st) in (([100, 4000], (cos_a, sin_a)), ([2500, 1], (cos_b, sin_b)), ([cap - sn, 0], (cos_a, sin_b))):
        cs.copy_(torch.tensor(lens, dtype=torch.int32))
        cos.copy_(ct)
        sin.copy_(st)
        kg.copy_(k0)
        vg.copy_(v0)
        g.replay()
        torch.cuda.synchronize()
        ke, ve = k0.clone(), v0.clone()
        out_e, lse_e = F.flash_attn_with_kvcache(q, ke, ve, **kw)
        assert torch.equal(_bits(out_g), _bits(out_e)) and torch.equal(_bits(lse_g), _bits(lse_e)), lens
        assert torch.equal(_bits(kg), _bits(ke)) and torch.equal(_bits(vg), _bits(ve)), lens
        # ... and the eager call is the formula
        k_rot = rotate_ref(k_new, ct, st, positions(lens, sn, True, cap), False)
        assert_same(ke, expected_cache(k0, k_rot, lens).to(gpu), f"graph {lens}: k_cache against the formula")
        q_rot = rotate_ref(q, ct, st, positions(lens, sn, True, cap), False)
        U.check_kvcache_rows(out_g, lse_g, q_rot, ke, ve, [L + sn for L in lens], True, "fp16", f"graph {lens}")


# ---- the C ABI with a caller-owned workspace ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_splits", [0, 1, 5])
def test_c_abi_with_an_exact_workspace(gpu, num_splits):
    """fa_run_mha_fwd_kvcache_ex with fa_kvcache_options_v3 and a workspace of exactly fa_kvcache_workspace_bytes_ex bytes (filled with NaN first):
    the bits of the Python call; nothing behind the workspace is written; one byte less than the image is an error before any launch"""
    dt, d, h, hk, cap, sq = torch.bfloat16, 128, 32, 8, 2048, 2
    gen = torch.Generator().manual_seed(17)
    lens = [0, 1000, cap - sq]
    b = len(lens)
    k0, v0 = _rand((b, cap, hk, d), gen, dt), _rand((b, cap, hk, d), gen, dt)
    q, k_new, v_new = _rand((b, sq, h, d), gen, dt), _rand((b, sq, hk, d), gen, dt), _rand((b, sq, hk, d), gen, dt)
    cos, sin = tables(cap, 64, dt)
    want = rotary_and_plain(gpu, q, k_new, v_new, k0, v0, lens, cos, sin, True, causal=True, num_splits=num_splits, tag=f"python ns={num_splits}")
    qg, kng, vng, ka, va, cg, sg = (t.to(gpu) for t in (q, k_new, v_new, k0, v0, cos, sin))
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    out, lse = torch.empty_like(qg), torch.empty(b, h, sq, dtype=torch.float32, device=gpu)
    p = capi.kvcache_params(qg, ka, va, out, lse, cache_seqlens=cs, k_new=kng, v_new=vng, causal=True, num_splits=num_splits)
    o = capi.kvcache_options(rotary_cos=cg, rotary_sin=sg, rotary_interleaved=True)
    assert isinstance(o, capi.KvcacheOptionsV3) and o.struct_size == 112
    image = (b * sq * h * d * 2 + 15) // 16 * 16
    need = capi.kvcache_workspace_bytes(p, o)
    assert need == image + capi.kvcache_workspace_bytes(p)
    ws = torch.full((need // 2 + 64,), float("nan"), dtype=torch.bfloat16, device=gpu)
    p.workspace, p.workspace_bytes = ws.data_ptr(), need
    assert capi.kvcache_num_splits(p, o) == max(num_splits, 1) or num_splits == 0
    capi.run_fwd_kvcache(p, options=o)
    torch.cuda.synchronize()
    for got, exp, name in zip((out, lse, ka, va), want[:4], ("out", "lse", "k_cache", "v_cache")):
        assert torch.equal(_bits(got), _bits(exp)), name
    assert torch.isnan(ws[need // 2:]).all(), "bytes behind the workspace were written"
    assert torch.equal(_bits(ws[:image // 2].view(b, sq, h, d)), _bits(want[4].to(gpu))), "the image at the head of the workspace is the rotated q"
    p.workspace_bytes = image - 1
    rc = capi.lib().fa_run_mha_fwd_kvcache_ex(ctypes.byref(p), ctypes.byref(o), None)
    assert rc == capi.FA_ERR_BAD_SHAPE and str(image) in capi.last_error()
