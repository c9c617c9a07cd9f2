"""GPU: decode attention over a KV cache (flash_attn_with_kvcache / fwd_kvcache / fa_run_mha_fwd_kvcache).

Expectations: the fp32 PyTorch statement of the contract (_util.torch_attention_ref) on each sequence's valid prefix of the cache, asserted
with _util.assert_close (the repo's tolerance rules).  Dead rows (no visible key) must be exactly O = 0, LSE = 0."""
import statistics

import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def _rand(shape, dt, gen, dev):
    return torch.randn(*shape, device=dev, dtype=torch.float32, generator=gen).to(dt)


_check_rows = U.check_kvcache_rows


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_mixed_lengths_against_reference(gpu, dtname, d, causal):
    """per-batch lengths 0, 1, 63, 64, 65, a non-multiple of the split chunk and the full capacity; seqlen_q 1, 2, 4, 16; MHA, GQA, MQA"""
    dt = DT[dtname]
    gen = torch.Generator(device=gpu).manual_seed(11 + d + int(causal))
    cap = 1200
    lens = [0, 1, 63, 64, 65, 777, cap]
    b = len(lens)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for h, hk in ((8, 8), (32, 8), (32, 1)):
        k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
        for sq in (1, 2, 4, 16):
            q = _rand((b, sq, h, d), dt, gen, gpu)
            out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, causal=causal, return_softmax_lse=True)
            assert out.shape == q.shape and out.dtype == dt and lse.shape == (b, h, sq) and lse.dtype == torch.float32
            _check_rows(out, lse, q, k_cache, v_cache, lens, causal, dtname, f"{dtname} d{d} h{h}/{hk} sq{sq} causal={causal}")


@pytest.mark.parametrize("causal", [False, True])
def test_append_writes_cache_and_attends_new_keys(gpu, causal):
    dt, d, h, hk, cap, sn = torch.float16, 128, 16, 4, 300, 3
    gen = torch.Generator(device=gpu).manual_seed(5)
    lens = [5, 0, 100, 297]
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    k0, v0 = k_cache.clone(), v_cache.clone()
    k_new, v_new = _rand((b, sn, hk, d), dt, gen, gpu), _rand((b, sn, hk, d), dt, gen, gpu)
    q = _rand((b, sn, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, k=k_new, v=v_new, cache_seqlens=cs, causal=causal, return_softmax_lse=True)
    torch.cuda.synchronize()
    assert cs.tolist() == lens, "cache_seqlens must not be updated by the library"
    k_exp, v_exp = k0.clone(), v0.clone()
    for i, L in enumerate(lens):
        k_exp[i, L:L + sn] = k_new[i]
        v_exp[i, L:L + sn] = v_new[i]
    # the appended rows bit for bit, every other row untouched
    assert torch.equal(k_cache.view(torch.int16), k_exp.view(torch.int16)) and torch.equal(v_cache.view(torch.int16), v_exp.view(torch.int16))
    _check_rows(out, lse, q, k_exp, v_exp, [L + sn for L in lens], causal, "fp16", f"append causal={causal}")


def test_strided_cache_view(gpu):
    """caches that are slices of larger buffers (row offset, every other head) - no copy, same bits as the contiguous cache"""
    dt, d, h, hk, cap = torch.bfloat16, 64, 12, 3, 700
    gen = torch.Generator(device=gpu).manual_seed(9)
    lens = [700, 1, 333]
    b = len(lens)
    kbuf, vbuf = _rand((b, cap + 24, 2 * hk, d), dt, gen, gpu), _rand((b, cap + 24, 2 * hk, d), dt, gen, gpu)
    k_cache, v_cache = kbuf[:, 8:8 + cap, 1::2], vbuf[:, 16:16 + cap, 0::2]
    assert not k_cache.is_contiguous()
    q = _rand((b, 2, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    before = F._C.densify_copies()
    out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, causal=True, return_softmax_lse=True)
    assert F._C.densify_copies() == before
    out_c, lse_c = F.flash_attn_with_kvcache(q, k_cache.contiguous(), v_cache.contiguous(), cache_seqlens=cs, causal=True, return_softmax_lse=True)
    assert torch.equal(out.view(torch.int16), out_c.view(torch.int16)) and torch.equal(lse, lse_c)
    _check_rows(out, lse, q, k_cache, v_cache, lens, True, "bf16", "strided")


def test_split_counts_agree_and_are_deterministic(gpu):
    dt, d, h, hk, cap = torch.float16, 128, 32, 8, 8192
    gen = torch.Generator(device=gpu).manual_seed(3)
    lens = [8000, 3001]
    b = len(lens)
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, 1, h, d), dt, gen, gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    # the library's own choice splits this launch (b x h_k = 16 workgroups)
    p = capi.kvcache_params(q, k_cache, v_cache, torch.empty_like(q), torch.empty(b, h, 1, device=gpu), cache_seqlens=cs)
    assert capi.kvcache_workspace_bytes(p) > 0
    res = {}
    for ns in (1, 0, 37):
        out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True)
        out2, lse2 = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, num_splits=ns, return_softmax_lse=True)
        assert torch.equal(out.view(torch.int16), out2.view(torch.int16)) and torch.equal(lse, lse2), f"num_splits={ns}: not deterministic"
        _check_rows(out, lse, q, k_cache, v_cache, lens, False, "fp16", f"num_splits={ns}")
        res[ns] = (out.float(), lse)
    for ns in (0, 37):
        assert (res[ns][0] - res[1][0]).abs().max().item() <= 4e-3, ns
        assert (res[ns][1] - res[1][1]).abs().max().item() <= 1e-4, ns


@pytest.mark.parametrize("causal", [False, True])
def test_equal_lengths_match_fwd(gpu, causal):
    dt, d, h, hk, cap, L = torch.bfloat16, 128, 16, 4, 2048, 1500
    gen = torch.Generator(device=gpu).manual_seed(21)
    b = 3
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, 4, h, d), dt, gen, gpu)
    out, lse = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=L, causal=causal, return_softmax_lse=True)
    o_f, lse_f = F.fwd(q, k_cache[:, :L], v_cache[:, :L], causal)
    tol = U.TOL["bf16"]
    diff = (out.float() - o_f.float()).abs()
    assert diff.max().item() <= tol["max_abs"] and diff.mean().item() <= tol["mean_abs"], (diff.max().item(), diff.mean().item())
    assert (lse - lse_f).abs().max().item() <= U.LSE_TOL
    _check_rows(out, lse, q, k_cache, v_cache, [L] * b, causal, "bf16", f"equal lengths causal={causal}")
    # cache_seqlens=None: the whole capacity
    out_all = F.flash_attn_with_kvcache(q, k_cache, v_cache, causal=causal)
    o_all, _ = F.fwd(q, k_cache, v_cache, causal)
    diff = (out_all.float() - o_all.float()).abs()
    assert diff.max().item() <= tol["max_abs"] and diff.mean().item() <= tol["mean_abs"], (diff.max().item(), diff.mean().item())


def test_graph_capture_replays_with_new_lengths(gpu):
    dt, d, h, hk, cap = torch.float16, 128, 32, 8, 4096
    gen = torch.Generator(device=gpu).manual_seed(13)
    b = 2
    k_cache, v_cache = _rand((b, cap, hk, d), dt, gen, gpu), _rand((b, cap, hk, d), dt, gen, gpu)
    q = _rand((b, 1, h, d), dt, gen, gpu)
    cs = torch.tensor([100, 4000], dtype=torch.int32, device=gpu)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, return_softmax_lse=True)
    for lens in ([100, 4000], [2500, 1], [4096, 0]):
        cs.copy_(torch.tensor(lens, dtype=torch.int32))
        g.replay()
        torch.cuda.synchronize()
        out_e, lse_e = F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs, return_softmax_lse=True)
        assert torch.equal(out_g.view(torch.int16), out_e.view(torch.int16)) and torch.equal(lse_g, lse_e), lens
        _check_rows(out_g, lse_g, q, k_cache, v_cache, lens, False, "fp16", f"graph {lens}")


def test_forward_only_and_int_lengths(gpu):
    dt, d = torch.float16, 64
    q = torch.randn(2, 1, 4, d, device=gpu, dtype=dt)
    kc, vc = torch.randn(2, 128, 2, d, device=gpu, dtype=dt), torch.randn(2, 128, 2, d, device=gpu, dtype=dt)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.flash_attn_with_kvcache(q.clone().requires_grad_(True), kc, vc, cache_seqlens=10)
    with torch.no_grad():
        out = F.flash_attn_with_kvcache(q.clone().requires_grad_(True), kc, vc, cache_seqlens=10)
    ref = F.flash_attn_with_kvcache(q, kc, vc, cache_seqlens=torch.tensor([10, 10], dtype=torch.int32, device=gpu))
    assert torch.equal(out, ref)
    with pytest.raises(ValueError):
        F.flash_attn_with_kvcache(q, kc, vc, k=kc[:, :1], cache_seqlens=10)
    with pytest.raises(RuntimeError, match="cache_seqlens"):
        F.flash_attn_with_kvcache(q, kc, vc, k=kc[:, :1], v=vc[:, :1])


def _median_ms(fn, rounds=5, iters=5):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ts)


def test_decode_faster_than_fwd(gpu):
    """b1 h32 h_k8 d128, 32k keys, one query: the split-KV path against fwd(q, k_cache[:, :L], v_cache[:, :L]) on the same data.
    Measured 7.0x (0.075 ms against 0.525 ms, profiles/kvcache_bench.log); the bound leaves room for box-to-box variation."""
    dt, d, h, hk, L = torch.float16, 128, 32, 8, 32768
    gen = torch.Generator(device=gpu).manual_seed(1)
    k_cache, v_cache = _rand((1, L, hk, d), dt, gen, gpu), _rand((1, L, hk, d), dt, gen, gpu)
    q = _rand((1, 1, h, d), dt, gen, gpu)
    cs = torch.tensor([L], dtype=torch.int32, device=gpu)
    t_fwd = _median_ms(lambda: F.fwd(q, k_cache[:, :L], v_cache[:, :L], False))
    t_kv = _median_ms(lambda: F.flash_attn_with_kvcache(q, k_cache, v_cache, cache_seqlens=cs))
    assert t_fwd / t_kv >= 2.0, (t_fwd, t_kv)
