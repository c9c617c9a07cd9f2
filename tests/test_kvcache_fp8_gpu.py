"""GPU: decode over an FP8 (torch.float8_e4m3fn) KV cache with per-(batch, KV head) descales.

Expectations: the call equals the 16-bit call on the DEQUANTISED cache (k_cache.float() * k_descale[:, None, :, None], fp32), so every value
check goes through the helpers and constants of the 16-bit decode tests (_util.check_kvcache_rows / assert_close; the windowed reference of
test_kvcache_window_gpu.py) on that dequantised cache: widening e4m3 to fp16 / bf16 is exact and the descales are applied in fp32, so the
8-bit kernels have the rounding points of the 16-bit ones and none of their own.  Test caches are quantised by torch on the CPU with the rule
of the append contract, never by the library under test."""
import ctypes

import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi
from test_kvcache_window_gpu import check_window_rows

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
F8 = torch.float8_e4m3fn
NAN8 = 0x7F


def quantise(x, descale):
    """the append contract with torch on the CPU: e4m3_rne(clamp(float(x) / descale, -448, 448)), IEEE fp32 quotient; x (b, s, hk, d),
    descale (b, hk) or None"""
    xf = x.detach().float().cpu()
    if descale is not None:
        xf = xf / descale.detach().float().cpu()[:, None, :, None]
    return xf.clamp(-448.0, 448.0).to(F8)


def deq(c8, descale):
    """fp32 dequantised cache (b, s, hk, d) on the CPU"""
    x = c8.detach().cpu().float()
    return x if descale is None else x * descale.detach().float().cpu()[:, None, :, None]


def _rand(shape, gen):
    return torch.randn(*shape, dtype=torch.float32, generator=gen)


def _descale(b, hk, gen, dev):
    """(b, hk) fp32 in [0.25, 4], no powers of two"""
    ds = 0.25 * 16.0 ** torch.rand(b, hk, generator=gen)
    ds = torch.where(torch.log2(ds) == torch.log2(ds).round(), ds * 1.1, ds)
    return ds.to(dev)


def _cache(shape, gen, dev, descale):
    """an 8-bit cache of N(0, 1) data quantised under `descale`, on the device"""
    return quantise(_rand(shape, gen), descale).to(dev)


def _u8(t):
    return t.view(torch.uint8)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _page(k8, v8, P, seed, extra=2, fill=NAN8):
    """a pool + block table holding the logical 8-bit caches (b, cap, hk, d), pages by a random permutation; unreferenced pages hold `fill`"""
    b, cap, hk, d = k8.shape
    cols = cap // P
    nb = b * cols + extra
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))
    table = perm[: b * cols].view(b, cols).to(torch.int32).to(k8.device)
    kp = torch.full((nb, P, hk, d), fill, dtype=torch.uint8, device=k8.device)
    vp = torch.full_like(kp, fill)
    idx = table.long()
    kp[idx] = _u8(k8).reshape(b, cols, P, hk, d)
    vp[idx] = _u8(v8).reshape(b, cols, P, hk, d)
    return kp.view(F8), vp.view(F8), table


# ---- 1. mixed lengths against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_mixed_lengths_against_reference(gpu, dtname, d, causal):
    """the grid of test_kvcache_gpu.py::test_mixed_lengths_against_reference over an 8-bit cache with per-(batch, head) descales, and once
    without descales"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(11 + d + int(causal))
    cap = 1200
    lens = [0, 1, 63, 64, 65, 777, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for h, hk in ((8, 8), (32, 8), (32, 1)):
        kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
        k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
        k_deq, v_deq = deq(k8, kds), deq(v8, vds)
        for sq in (1, 2, 4, 16):
            q = _rand((b, sq, h, d), gen).to(dt).to(gpu)
            out, lse = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=causal, return_softmax_lse=True, k_descale=kds, v_descale=vds)
            assert out.shape == q.shape and out.dtype == dt and lse.shape == (b, h, sq) and lse.dtype == torch.float32
            U.check_kvcache_rows(out, lse, q, k_deq, v_deq, lens, causal, dtname, f"fp8 {dtname} d{d} h{h}/{hk} sq{sq} causal={causal}")
        if (h, hk) == (32, 8):
            out, lse = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=causal, return_softmax_lse=True)
            U.check_kvcache_rows(out, lse, q, deq(k8, None), deq(v8, None), lens, causal, dtname, f"fp8 no descale {dtname} d{d} causal={causal}")


# ---- 2. descales are per batch and head --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_descale_is_per_batch_and_head(gpu, dtname, d):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(23 + d)
    b, h, hk, cap, sq = 3, 8, 4, 520, 2
    lens = [520, 300, 77]
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    # 64x between neighbouring heads and batch entries
    base = torch.tensor([[0.013, 0.832, 0.013, 0.832], [0.832, 0.013, 0.832, 0.013], [0.013 * 64 * 64, 0.832, 0.013, 0.832 / 64]])
    kds, vds = base.to(gpu), base.flip(1).contiguous().to(gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, None), _cache((b, cap, hk, d), gen, gpu, None)
    q = (_rand((b, sq, h, d), gen) * 0.5).to(dt).to(gpu)
    out, lse = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=True, return_softmax_lse=True, k_descale=kds, v_descale=vds)
    U.check_kvcache_rows(out, lse, q, deq(k8, kds), deq(v8, vds), lens, True, dtname, f"fp8 64x descales {dtname} d{d}")
    # a strided view holding the same values
    wide_k, wide_v = torch.full((b, 2, hk, 3), 7.0, device=gpu), torch.full((b, 2, hk, 3), 7.0, device=gpu)
    wide_k[:, 1, :, 2], wide_v[:, 0, :, 1] = kds, vds
    sk, sv = wide_k[:, 1, :, 2], wide_v[:, 0, :, 1]
    assert not sk.is_contiguous() and sk.stride(1) == 3
    out_s, lse_s = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=True, return_softmax_lse=True, k_descale=sk, v_descale=sv)
    assert _same(out, out_s) and _same(lse, lse_s)
    # an expand()-ed scalar against the dense tensor of the same value
    one_k, one_v = torch.tensor(0.37, device=gpu), torch.tensor(2.9, device=gpu)
    out_e, lse_e = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, return_softmax_lse=True, k_descale=one_k.expand(b, hk), v_descale=one_v.expand(b, hk))
    out_d, lse_d = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, return_softmax_lse=True, k_descale=torch.full((b, hk), 0.37, device=gpu),
                                             v_descale=torch.full((b, hk), 2.9, device=gpu))
    assert _same(out_e, out_d) and _same(lse_e, lse_d)
    U.check_kvcache_rows(out_e, lse_e, q, deq(k8, one_k.expand(b, hk)), deq(v8, one_v.expand(b, hk)), lens, False, dtname, f"fp8 scalar descale {dtname} d{d}")


# ---- 3. append -------------------------------------------------------------------------------------------------------------------------

def _special_rows(k_new, dt):
    """plant, into the first two new rows of every head, values that saturate, +-inf, NaN, values that land in the e4m3 subnormals and exact
    ties (ties and subnormals as planted for the heads whose descale is 1.0; under the other descales they are ordinary values)"""
    vals = torch.tensor([1e4, -1e4, float("inf"), float("-inf"), float("nan"), 449.0, -2000.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, -(2.0 ** -11), 5 * 2.0 ** -11,
                         17.0, 19.0, 1.0625, 1.1875, -1.0625, 36.0, 44.0, 464.0, 0.0, -0.0, 2.0 ** -12, 7 * 2.0 ** -10])
    n = vals.numel()
    k_new[:, 0, :, :n] = vals.to(dt)
    k_new[:, 1, :, -n:] = (vals * 1.5).to(dt)
    return k_new


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("layout", ["contiguous", "paged"])
def test_append_quantises_in_place_bit_for_bit(gpu, dtname, d, layout):
    """the cache bytes after the call equal the contract formula evaluated by torch on the CPU, every other byte untouched; the output is
    the reference on the expected cache"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(31 + d)
    b, h, hk, sn, P = 4, 8, 4, 5, 16
    cap = 320
    lens = [5, 0, 30, cap - sn]                              # 30 + 5 crosses the page at 32
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    kds[:, 0], vds[:, 1] = 1.0, 1.0                          # heads whose quotient is the value itself: exact ties stay ties
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
    k_new = _special_rows((_rand((b, sn, hk, d), gen) * 3).to(dt), dt).to(gpu)
    v_new = _special_rows((_rand((b, sn, hk, d), gen) * 3).to(dt), dt).flip(1).contiguous().to(gpu)
    q = _rand((b, sn, h, d), gen).to(dt).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    k_exp, v_exp = k8.clone(), v8.clone()
    kq, vq = quantise(k_new, kds).to(gpu), quantise(v_new, vds).to(gpu)
    for i, L in enumerate(lens):
        _u8(k_exp)[i, L:L + sn] = _u8(kq)[i]
        _u8(v_exp)[i, L:L + sn] = _u8(vq)[i]
    # the planted values do what they were planted for
    codes = _u8(kq)[:, 0, 0, :24].cpu()
    assert (codes[:, 0] == 0x7E).all() and (codes[:, 1] == 0xFE).all() and (codes[:, 2] == 0x7E).all() and (codes[:, 3] == 0xFE).all() and ((codes[:, 4] & 0x7F) == NAN8).all()
    assert ((codes[:, 7:12] & 0x78) == 0).all()              # subnormal or zero codes
    if layout == "paged":
        kp, vp, table = _page(k8, v8, P, seed=5)
        kp0, vp0 = kp.clone(), vp.clone()
        out, lse = F.flash_attn_with_kvcache(q, kp, vp, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, block_table=table,
                                             k_descale=kds, v_descale=vds)
        torch.cuda.synchronize()
        kpe, vpe, table_e = _page(k_exp, v_exp, P, seed=5)
        assert torch.equal(table, table_e)
        assert torch.equal(_u8(kp), _u8(kpe)) and torch.equal(_u8(vp), _u8(vpe)), "paged append: pool bytes differ from the contract formula"
        assert not torch.equal(_u8(kp), _u8(kp0))
    else:
        out, lse = F.flash_attn_with_kvcache(q, k8, v8, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, k_descale=kds, v_descale=vds)
        torch.cuda.synchronize()
        diff = (_u8(k8) != _u8(k_exp)).nonzero()
        assert diff.numel() == 0, f"appended K bytes differ from the contract formula at {diff[:5].tolist()}: got {_u8(k8)[tuple(diff[0])].item():#x} want {_u8(k_exp)[tuple(diff[0])].item():#x}"
        assert torch.equal(_u8(v8), _u8(v_exp)), "appended V bytes differ from the contract formula"
    assert cs.tolist() == lens, "cache_seqlens must not be updated by the library"
    # value check on the expected cache with the NaN codes taken out (their rows are the NaN contract's, checked below): the planted NaN
    # sits in new row 0 (K) / new row sn - 1 (V) of every sequence
    k_fin, v_fin = k_exp.clone(), v_exp.clone()
    _u8(k_fin)[(_u8(k_fin) & 0x7F) == NAN8] = 0
    _u8(v_fin)[(_u8(v_fin) & 0x7F) == NAN8] = 0
    if layout == "paged":
        kpf, vpf, _ = _page(k_fin, v_fin, P, seed=5)
        out, lse = F.flash_attn_with_kvcache(q, kpf, vpf, cache_seqlens=cs + sn, causal=True, return_softmax_lse=True, block_table=table, k_descale=kds, v_descale=vds)
    else:
        out, lse = F.flash_attn_with_kvcache(q, k_fin, v_fin, cache_seqlens=cs + sn, causal=True, return_softmax_lse=True, k_descale=kds, v_descale=vds)
    U.check_kvcache_rows(out, lse, q, deq(k_fin, kds), deq(v_fin, vds), [L + sn for L in lens], True, dtname, f"fp8 append {layout} {dtname} d{d}")


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_append_then_attend_sees_the_quantised_rows(gpu, dtname):
    """attention of the appending call runs over the quantised rows: same bits as a second call without append on the cache it left"""
    dt, d = DT[dtname], 128
    gen = torch.Generator().manual_seed(41)
    b, h, hk, sn, cap = 3, 16, 4, 3, 300
    lens = [5, 0, 297]
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
    k_new, v_new = _rand((b, sn, hk, d), gen).to(dt).to(gpu), _rand((b, sn, hk, d), gen).to(dt).to(gpu)
    q = _rand((b, sn, h, d), gen).to(dt).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    out, lse = F.flash_attn_with_kvcache(q, k8, v8, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, k_descale=kds, v_descale=vds)
    out2, lse2 = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs + sn, causal=True, return_softmax_lse=True, k_descale=kds, v_descale=vds)
    assert _same(out, out2) and _same(lse, lse2)
    U.check_kvcache_rows(out, lse, q, deq(k8, kds), deq(v8, vds), [L + sn for L in lens], True, dtname, f"fp8 append+attend {dtname}")


# ---- 4. layouts agree; windows -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_paged_and_contiguous_give_the_same_bits(gpu, dtname, d):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(51 + d)
    b, h, hk, cap = 3, 16, 4, 768
    lens = [768, 1, 401]
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for sq, causal in ((1, False), (4, True)):
        q = _rand((b, sq, h, d), gen).to(dt).to(gpu)
        ref = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=causal, return_softmax_lse=True, k_descale=kds, v_descale=vds)
        U.check_kvcache_rows(ref[0], ref[1], q, deq(k8, kds), deq(v8, vds), lens, causal, dtname, f"fp8 contiguous {dtname} d{d} sq{sq}")
        for P in (16, 48, 256):
            kp, vp, table = _page(k8, v8, P, seed=P)
            got = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=causal, return_softmax_lse=True, block_table=table, k_descale=kds, v_descale=vds)
            assert _same(got[0], ref[0]) and _same(got[1], ref[1]), (P, sq, causal)
        # shared pages: every sequence reads sequence 0's pages
        kp, vp, table = _page(k8, v8, 256, seed=9)
        shared = table[:1].expand(b, -1).contiguous()
        got = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=causal, return_softmax_lse=True, block_table=shared, k_descale=kds[:1].expand(b, hk),
                                        v_descale=vds[:1].expand(b, hk))
        want = F.flash_attn_with_kvcache(q, k8[:1].expand(b, -1, -1, -1).contiguous(), v8[:1].expand(b, -1, -1, -1).contiguous(), cache_seqlens=cs, causal=causal,
                                         return_softmax_lse=True, k_descale=kds[:1].expand(b, hk), v_descale=vds[:1].expand(b, hk))
        assert _same(got[0], want[0]) and _same(got[1], want[1]), ("shared", sq, causal)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_window_against_reference_in_both_layouts(gpu, dtname, d):
    """(W - 1, 0) causal, two-sided, and a window of one key, against the reference restricted to the window"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(61 + d)
    b, h, hk, cap = 4, 8, 2, 768
    lens = [768, 5, 100, 333]
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
    k_deq, v_deq = deq(k8, kds), deq(v8, vds)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kp, vp, table = _page(k8, v8, 48, seed=3)
    for sq, window, causal in ((1, (63, 0), True), (4, (127, 0), True), (4, (20, 2), False), (2, (0, 0), True), (1, (0, 0), False), (16, (100, 40), False)):
        q = _rand((b, sq, h, d), gen).to(dt).to(gpu)
        out, lse = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, causal=causal, window_size=window, return_softmax_lse=True, k_descale=kds, v_descale=vds)
        check_window_rows(out, lse, q, k_deq, v_deq, lens, window, causal, dtname, f"fp8 window {window} causal={causal} sq{sq} {dtname} d{d}")
        out_p, lse_p = F.flash_attn_with_kvcache(q, kp, vp, cache_seqlens=cs, causal=causal, window_size=window, return_softmax_lse=True, block_table=table,
                                                 k_descale=kds, v_descale=vds)
        assert _same(out, out_p) and _same(lse, lse_p), (window, causal, sq)


# ---- 5. splits ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_split_counts_agree_and_are_deterministic(gpu, dtname, d):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(3 + d)
    b, h, hk, cap = 2, 32, 8, 8192
    lens = [8000, 3001]
    kds = _descale(b, hk, gen, gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, None)
    q = _rand((b, 1, h, d), gen).to(dt).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    # split count and workspace from the C ABI: those of the 16-bit call of the same shape
    o, l = torch.empty_like(q), torch.empty(b, h, 1, device=gpu)
    p8 = capi.kvcache_params(q, k8, v8, o, l, cache_seqlens=cs)
    p16 = capi.kvcache_params(q, k8.to(dt), v8.to(dt), o, l, cache_seqlens=cs)
    opt = capi.kvcache_options(cache_dtype=capi.FA_CACHE_FP8_E4M3, k_descale=kds)
    ws = capi.kvcache_workspace_bytes(p16)
    assert ws > 0 and capi.kvcache_workspace_bytes(p8, opt) == ws
    buf = torch.empty(ws // 4, device=gpu)
    for p in (p8, p16):
        p.workspace, p.workspace_bytes = buf.data_ptr(), ws
    assert capi.kvcache_num_splits(p8, opt) == capi.kvcache_num_splits(p16) > 1
    k_deq, v_deq = deq(k8, kds), deq(v8, None)
    res = {}
    for ns in (1, 0, 37):
        out, lse = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, k_descale=kds)
        out2, lse2 = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True, k_descale=kds)
        assert _same(out, out2) and _same(lse, lse2), f"num_splits={ns}: not deterministic"
        U.check_kvcache_rows(out, lse, q, k_deq, v_deq, lens, False, dtname, f"fp8 num_splits={ns} {dtname} d{d}")
        res[ns] = (out.float(), lse)
    for ns in (0, 37):
        assert (res[ns][0] - res[1][0]).abs().max().item() <= 4e-3, ns
        assert (res[ns][1] - res[1][1]).abs().max().item() <= 1e-4, ns
    # the C ABI run gives the bits of the Python call
    capi.run_fwd_kvcache(p8, options=opt)
    torch.cuda.synchronize()
    out0, lse0 = F.flash_attn_with_kvcache(q, k8, v8, cache_seqlens=cs, return_softmax_lse=True, k_descale=kds)
    assert _same(o, out0) and _same(l, lse0)


# ---- 6. never read / NaN contract ------------------------------------------------------------------------------------------------------------

def _guarded8(shape, dev, pad, fill=NAN8):
    """an 8-bit buffer filled with `fill` with `pad` extra elements on every dim and the view of `shape` into it (offset pad // 2 on every dim
    but the last, 16 elements on the last: rows stay 16-byte aligned); pads must keep every stride a multiple of 16"""
    full = [s + p for s, p in zip(shape, pad)]
    buf = torch.full(full, fill, dtype=torch.uint8, device=dev)
    sl = tuple(slice(p // 2, p // 2 + s) for s, p in zip(shape[:-1], pad[:-1])) + (slice(16, 16 + shape[-1]),)
    return buf, buf[sl].view(F8), sl


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_unseen_rows_pages_and_heads_are_never_read(gpu, dtname, d):
    """NaN codes in every cache row at or past L_i, below a window, in unreferenced pages and in the heads a strided view skips leave O and
    LSE bit-identical to the call on a clean cache"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(71 + d)
    b, h, hk, cap, sq = 4, 8, 2, 576, 2
    lens = [0, 1, 300, 575]
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
    q = _rand((b, sq, h, d), gen).to(dt).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, return_softmax_lse=True, k_descale=kds, v_descale=vds)
    for window, causal in (((-1, -1), False), ((-1, -1), True), ((40, 0), True), ((33, 1), False)):
        clean = F.flash_attn_with_kvcache(q, k8, v8, causal=causal, window_size=window, **kw)
        assert torch.isfinite(clean[0]).all() and torch.isfinite(clean[1]).all()
        kn, vn = k8.clone(), v8.clone()
        for i, L in enumerate(lens):
            lo = max(0, L - sq - window[0]) if window[0] >= 0 else 0
            for t in (kn, vn):
                _u8(t)[i, L:] = NAN8
                _u8(t)[i, :lo] = NAN8
        got = F.flash_attn_with_kvcache(q, kn, vn, causal=causal, window_size=window, **kw)
        assert _same(got[0], clean[0]) and _same(got[1], clean[1]), ("contiguous", window, causal)
        # paged: the same poisoned logical cache, unreferenced pages full of NaN codes
        kp, vp, table = _page(kn, vn, 48, seed=7, extra=3)
        got = F.flash_attn_with_kvcache(q, kp, vp, causal=causal, window_size=window, block_table=table, **kw)
        assert _same(got[0], clean[0]) and _same(got[1], clean[1]), ("paged", window, causal)
        # a strided view: every other head of a buffer whose other heads, and the rows around the view, hold NaN codes
        kbuf = torch.full((b, cap + 32, 2 * hk, d), NAN8, dtype=torch.uint8, device=gpu)
        vbuf = torch.full((b, cap + 32, 2 * hk, d), NAN8, dtype=torch.uint8, device=gpu)
        kv_, vv_ = kbuf[:, 16:16 + cap, 1::2], vbuf[:, 8:8 + cap, 0::2]
        kv_.copy_(_u8(kn)), vv_.copy_(_u8(vn))
        before = F._C.densify_copies()
        got = F.flash_attn_with_kvcache(q, kv_.view(F8), vv_.view(F8), causal=causal, window_size=window, **kw)
        assert F._C.densify_copies() == before
        assert _same(got[0], clean[0]) and _same(got[1], clean[1]), ("strided", window, causal)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", [1, 0, 5])
def test_nan_code_in_a_visible_k_row_makes_exactly_its_rows_nan(gpu, dtname, num_splits):
    dt, d = DT[dtname], 128
    gen = torch.Generator().manual_seed(81)
    b, h, hk, cap, sq = 2, 8, 2, 2048, 4
    lens = [2000, 600]
    kds = _descale(b, hk, gen, gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, None)
    q = _rand((b, sq, h, d), gen).to(dt).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, causal=True, num_splits=num_splits, return_softmax_lse=True, k_descale=kds)
    clean = F.flash_attn_with_kvcache(q, k8, v8, **kw)
    # batch 0, KV head 1, key 1998: under the causal mask, visible to query positions t with 1998 <= 2000 - 4 + t, i.e. t >= 2; 0xff as well
    for code in (0x7F, 0xFF):
        kn = k8.clone()
        _u8(kn)[0, 1998, 1, 77] = code
        out, lse = F.flash_attn_with_kvcache(q, kn, v8, **kw)
        want = torch.zeros(b, sq, h, dtype=torch.bool, device=gpu)
        want[0, 2:, 4:] = True                               # query heads 4..7 read KV head 1
        assert torch.equal(torch.isnan(out).any(-1), want) and torch.equal(torch.isnan(out).all(-1), want), code
        assert torch.equal(torch.isnan(lse), want.permute(0, 2, 1)), code
        assert torch.equal(_bits(out)[~want], _bits(clean[0])[~want]) and torch.equal(_bits(lse)[~want.permute(0, 2, 1)], _bits(clean[1])[~want.permute(0, 2, 1)])


@pytest.mark.parametrize("layout", ["contiguous", "paged"])
def test_guard_bytes_around_a_strided_cache_view_survive_an_append(gpu, layout):
    dt, d = torch.float16, 64
    gen = torch.Generator().manual_seed(91)
    b, h, hk, sn, P = 3, 4, 2, 3, 16
    cap = 64
    lens = [0, 30, cap - sn]
    rows0 = b if layout == "contiguous" else b * (cap // P)
    shape = (rows0, cap if layout == "contiguous" else P, hk, d)
    pad = (2, 32, 2, 32)
    kbuf, kview, sl = _guarded8(shape, gpu, pad, fill=0xA5)
    vbuf, vview, _ = _guarded8(shape, gpu, pad, fill=0x5A)
    assert all(s % 16 == 0 for s in kview.stride()[:3]) and kview.data_ptr() % 16 == 0
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k0, v0 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
    table = None
    if layout == "contiguous":
        _u8(kview).copy_(_u8(k0)), _u8(vview).copy_(_u8(v0))
    else:
        table = torch.randperm(rows0, generator=gen).view(b, cap // P).to(torch.int32).to(gpu)
        _u8(kview)[table.long()] = _u8(k0).reshape(b, cap // P, P, hk, d)
        _u8(vview)[table.long()] = _u8(v0).reshape(b, cap // P, P, hk, d)
    k_new, v_new = _rand((b, sn, hk, d), gen).to(dt).to(gpu), _rand((b, sn, hk, d), gen).to(dt).to(gpu)
    q = _rand((b, sn, h, d), gen).to(dt).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kb0, vb0 = kbuf.clone(), vbuf.clone()
    out, lse = F.flash_attn_with_kvcache(q, kview, vview, k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, block_table=table,
                                         k_descale=kds, v_descale=vds)
    torch.cuda.synchronize()
    k_exp, v_exp = k0.clone(), v0.clone()
    kq, vq = quantise(k_new, kds).to(gpu), quantise(v_new, vds).to(gpu)
    for i, L in enumerate(lens):
        _u8(k_exp)[i, L:L + sn] = _u8(kq)[i]
        _u8(v_exp)[i, L:L + sn] = _u8(vq)[i]
    for buf, buf0, exp in ((kbuf, kb0, k_exp), (vbuf, vb0, v_exp)):
        want = buf0.clone()
        if layout == "contiguous":
            want[sl] = _u8(exp)
        else:
            inner = want[sl]
            inner[table.long()] = _u8(exp).reshape(b, cap // P, P, hk, d)
            want[sl] = inner
        assert torch.equal(buf, want), "bytes outside the appended rows changed (or the appended rows are wrong)"
    U.check_kvcache_rows(out, lse, q, deq(k_exp, kds), deq(v_exp, vds), [L + sn for L in lens], True, "fp16", f"fp8 guarded append {layout}")


# ---- 7. graph ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_graph_replays_with_new_lengths_descales_and_rows(gpu, dtname):
    dt, d = DT[dtname], 128
    gen = torch.Generator().manual_seed(13)
    b, h, hk, cap, sn = 2, 32, 8, 4096, 1
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = _cache((b, cap, hk, d), gen, gpu, kds), _cache((b, cap, hk, d), gen, gpu, vds)
    q = _rand((b, sn, h, d), gen).to(dt).to(gpu)
    k_new, v_new = _rand((b, sn, hk, d), gen).to(dt).to(gpu), _rand((b, sn, hk, d), gen).to(dt).to(gpu)
    cs = torch.tensor([100, 4000], dtype=torch.int32, device=gpu)
    kw = dict(k=k_new, v=v_new, cache_seqlens=cs, causal=True, return_softmax_lse=True, k_descale=kds, v_descale=vds)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, k8, v8, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, k8, v8, **kw)
    for step, lens in enumerate(([100, 4000], [2500, 1], [4095, 0])):
        cs.copy_(torch.tensor(lens, dtype=torch.int32))
        kds.copy_(_descale(b, hk, gen, gpu)), vds.copy_(_descale(b, hk, gen, gpu))
        k_new.copy_(_rand((b, sn, hk, d), gen).to(dt)), v_new.copy_(_rand((b, sn, hk, d), gen).to(dt))
        k_before, v_before = k8.clone(), v8.clone()
        g.replay()
        torch.cuda.synchronize()
        k_after, v_after = k8.clone(), v8.clone()
        # the eager call on the same state: restore the cache, run, compare outputs and cache bytes
        k8.copy_(k_before), v8.copy_(v_before)
        out_e, lse_e = F.flash_attn_with_kvcache(q, k8, v8, **kw)
        torch.cuda.synchronize()
        assert _same(out_g, out_e) and _same(lse_g, lse_e), lens
        assert torch.equal(_u8(k8), _u8(k_after)) and torch.equal(_u8(v8), _u8(v_after)), lens
        for i, L in enumerate(lens):
            assert torch.equal(_u8(k8)[i, L], _u8(quantise(k_new, kds))[i, 0].to(gpu)), (lens, i)
        # descales changed between replays, so rows quantised under old descales are read under new ones: the expectation dequantises
        # whatever codes the cache holds with the current descales - exactly what the contract says
        U.check_kvcache_rows(out_g, lse_g, q, deq(k8, kds), deq(v8, vds), [L + sn for L in lens], True, dtname, f"fp8 graph {lens} {dtname}")


# ---- 8. validation that needs device memory ------------------------------------------------------------------------------------------------

def test_validation_on_the_device(gpu):
    dt, d, b, hk = torch.float16, 64, 2, 2
    q = torch.randn(b, 1, 4, d, device=gpu, dtype=dt)
    c16 = torch.randn(b, 128, hk, d, device=gpu, dtype=dt)
    c8 = torch.zeros(b, 128, hk, d, dtype=torch.uint8, device=gpu).view(F8)
    ds = torch.ones(b, hk, device=gpu)
    for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.int8):
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            F.flash_attn_with_kvcache(q, _u8(c8).view(bad), _u8(c8).view(bad), cache_seqlens=4)
        with pytest.raises(RuntimeError, match="float8_e4m3fn"):
            F._C.fwd_kvcache(q, _u8(c8).view(bad), _u8(c8).view(bad))
    with pytest.raises(ValueError, match="same dtype"):
        F.flash_attn_with_kvcache(q, c8, c16, cache_seqlens=4)
    with pytest.raises(RuntimeError, match="same dtype"):
        F._C.fwd_kvcache(q, c16, c8)
    with pytest.raises(ValueError, match="descale needs"):
        F.flash_attn_with_kvcache(q, c16, c16, cache_seqlens=4, k_descale=ds)
    with pytest.raises(RuntimeError, match="descale"):
        F._C.fwd_kvcache(q, c16, c16, v_descale=ds)
    with pytest.raises(ValueError, match="float32"):
        F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, k_descale=ds.half())
    with pytest.raises(RuntimeError, match="float32"):
        F._C.fwd_kvcache(q, c8, c8, k_descale=ds.double())
    with pytest.raises(ValueError, match="shape"):
        F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, v_descale=torch.ones(b, hk + 1, device=gpu))
    with pytest.raises(RuntimeError, match="shape"):
        F._C.fwd_kvcache(q, c8, c8, v_descale=torch.ones(hk, device=gpu))
    with pytest.raises(ValueError, match="device"):
        F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, k_descale=ds.cpu())
    with pytest.raises(RuntimeError, match="device"):
        F._C.fwd_kvcache(q, c8, c8, k_descale=ds.cpu())
    with pytest.raises(RuntimeError, match="forward-only"):
        F.flash_attn_with_kvcache(q.clone().requires_grad_(True), c8, c8, cache_seqlens=4, k_descale=ds)
    # misaligned views: never copied, rejected with the stride rule (row stride 64 + 8, head offset 8 bytes, storage offset 8)
    big = torch.zeros(b, 128, hk, d + 8, dtype=torch.uint8, device=gpu).view(F8)
    before = F._C.densify_copies()
    for bad in (big[..., :d], big[..., 8:]):
        with pytest.raises(RuntimeError, match="16"):
            F.flash_attn_with_kvcache(q, bad, bad, cache_seqlens=4)
    flat = torch.zeros(b * 128 * hk * d + 16, dtype=torch.uint8, device=gpu).view(F8)
    off = flat[8:8 + b * 128 * hk * d].view(b, 128, hk, d)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        F.flash_attn_with_kvcache(q, off, off, cache_seqlens=4)
    assert F._C.densify_copies() == before
    # through the C ABI: the documented codes
    o, l = torch.empty_like(q), torch.empty(b, 4, 1, device=gpu)
    p = capi.kvcache_params(q, big[..., :d], big[..., :d], o, l)
    fp8 = capi.kvcache_options(cache_dtype=capi.FA_CACHE_FP8_E4M3)
    L = capi.lib()
    assert L.fa_run_mha_fwd_kvcache_ex(ctypes.byref(p), ctypes.byref(fp8), None) == capi.FA_ERR_BAD_STRIDE
    p = capi.kvcache_params(q, c8, c8, o, l)
    assert L.fa_run_mha_fwd_kvcache_ex(ctypes.byref(p), ctypes.byref(capi.kvcache_options(cache_dtype=2)), None) == capi.FA_ERR_BAD_DTYPE
    assert L.fa_run_mha_fwd_kvcache_ex(ctypes.byref(p), ctypes.byref(capi.kvcache_options(k_descale=ds)), None) == capi.FA_ERR_BAD_DTYPE
    p = capi.kvcache_params(q, c16, c16, o, l)
    assert L.fa_run_mha_fwd_kvcache_ex(ctypes.byref(p), ctypes.byref(capi.kvcache_options(v_descale=ds)), None) == capi.FA_ERR_BAD_DTYPE
    torch.cuda.synchronize()


# ---- 9. timing relation -------------------------------------------------------------------------------------------------------------------

def test_fp8_cache_call_is_faster_than_the_16bit_call_on_the_same_data(gpu):
    """the largest point of tools/kvcache_bench.py's grid (one query, d 128, batch 32 x 32 KV heads x 128k keys: K + V = 68.7 GB in 16 bits,
    34.4 GB in 8; measured by the tool's own function, interleaved in one process): the median time of the 8-bit call is below the median of
    the 16-bit call on the same logical data.  A floor, not a target: what the ratio reaches is recorded in profiles/kvcache_fp8_bench.log."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kvcache_bench as KB

    pt = dict(b=32, h=32, h_k=32, d=128, L=131072, seqlen_q=1, dtype=torch.float16)
    with torch.no_grad():
        r = KB.run_fp8_point(pt, rounds=5)
    print(r)
    assert r["kv_gb_16bit"] >= 1.0
    assert r["ms_fp8"] < r["ms_16bit"], r
