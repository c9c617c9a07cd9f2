"""GPU: flash_attn_prefill_func / fa_run_prefill_fwd (fa_fwd_prefill.hip) against a plain fp64 reference (masked softmax with the sink as one more term):
values, the packed layout, the relations stated to the bit, what is never read, the sinks at their edges, and the adversarial-timing builds."""
import ctypes

import pytest
import torch

import _util as U
from test_stage_protocol_gpu import _must_differ, _must_match, libs  # noqa: F401  (libs: the product and the adversarial-timing builds)

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
WINDOWS = [(False, (-1, -1)), (True, (-1, -1)), (True, (17, 0)), (True, (40, 0)), (False, (40, 5)), (False, (-1, 3))]
SQ, SK, HK = 33, 100, 2     # h / h_k = 4: 132 packed rows = a full tile and a 4-row tile; 100 keys = three steps and a quarter; sq != sk: bottom-right alignment


def _call(q, k, v, **kw):
    import flash_attn_turing as F

    return F.flash_attn_prefill_func(q, k, v, return_softmax_lse=True, **kw)


_same = lambda a, b: a.shape == b.shape and a.dtype == b.dtype and torch.equal(U.bits(a.contiguous()), U.bits(b.contiguous()))  # noqa: E731


def _ref(q, k, v, causal, window, sinks, scale):
    """one sequence in fp64: q (sq, h, d), k / v (sk, h_k, d) -> o (sq, h, d), lse (h, sq); a row with no key and no sink is o = 0, lse = 0"""
    (sq, h, d), sk, ratio = q.shape, k.shape[0], q.shape[1] // k.shape[1]
    left, right = window[0], 0 if causal else window[1]
    q, k, v = q.double().cpu(), k.double().cpu().repeat_interleave(ratio, 1), v.double().cpu().repeat_interleave(ratio, 1)
    s = torch.einsum("qhd,khd->hqk", q, k) * (d ** -0.5 if scale is None else scale)
    t, j = torch.arange(sq)[:, None] + sk - sq, torch.arange(sk)[None]
    vis = (j >= t - left if left >= 0 else j >= 0) & (j <= t + right if right >= 0 else j >= 0)
    s = s.masked_fill(~vis, -INF)
    sink = torch.full((h,), -INF, dtype=torch.float64) if sinks is None else sinks.double().cpu()
    lse = torch.logsumexp(torch.cat([s, sink[:, None, None].expand(h, sq, 1)], -1), -1)
    dead = lse == -INF
    lse = lse.masked_fill(dead, 0.0)
    p = torch.exp(s - lse[..., None]).masked_fill(dead[..., None], 0.0)
    return torch.einsum("hqk,khd->qhd", p, v), lse


def _inputs(gpu, dtname, d, h, hk, sq, sk, seed, b=None):
    g, lead = torch.Generator().manual_seed(seed), () if b is None else (b,)
    return tuple(torch.randn(*lead, n, heads, d, generator=g).to(DT[dtname]).to(gpu) for n, heads in ((sq, h), (sk, hk), (sk, hk)))


def _check(out, lse, q, k, v, dtname, tag, causal, window, sinks, scale):
    o64, l64 = _ref(q, k, v, causal, window, sinks, scale)
    err = float((lse.double().cpu() - l64).abs().max())
    U.assert_close(out.float().cpu().numpy(), o64.numpy(), dtname, f"prefill_fwd O {tag}", sk=k.shape[0])
    assert err <= U.LSE_TOL, f"{tag}: LSE err {err:.3e} > {U.LSE_TOL}"


@pytest.mark.parametrize("scale", [None, 0.21])
@pytest.mark.parametrize("ratio", [1, 4])
@pytest.mark.parametrize("with_sinks", [False, True], ids=["nosink", "sinks"])
@pytest.mark.parametrize("causal,window", WINDOWS, ids=lambda x: str(x).replace(" ", ""))
@pytest.mark.parametrize("dtname", list(DT))
@pytest.mark.parametrize("d", [64, 128])
def test_values(gpu, d, dtname, causal, window, with_sinks, ratio, scale):
    h = HK * ratio
    q, k, v = _inputs(gpu, dtname, d, h, HK, SQ, SK, 100 + d + ratio, b=2)
    sinks = torch.randn(h, generator=torch.Generator().manual_seed(7)).to(gpu) * 2 if with_sinks else None
    out, lse = _call(q, k, v, causal=causal, window_size=window, sinks=sinks, softmax_scale=scale)
    assert out.shape == q.shape and out.dtype == q.dtype and lse.shape == (2, h, SQ) and lse.dtype == torch.float32
    for i in range(2):
        _check(out[i], lse[i], q[i], k[i], v[i], dtname, f"d{d} {dtname} {causal} {window} sinks={with_sinks} ratio{ratio} scale={scale} b{i}", causal, window, sinks, scale)


@pytest.mark.parametrize("with_sinks", [False, True], ids=["nosink", "sinks"])
@pytest.mark.parametrize("d", [64, 128])
def test_packed(gpu, d, with_sinks):
    """an empty sequence, sq_i = 1, sk_i < sq_i (rows that see no key), a sequence of two tiles: each equals the dense call on it alone; dead rows exact"""
    sqs, sks, h, hk, dtname = (0, 1, 50, 40), (5, 30, 20, 100), 8, 2, "bf16"
    q, k, v = _inputs(gpu, dtname, d, h, hk, sum(sqs), sum(sks), 200 + d)
    cu_q, cu_k = (torch.tensor([0] + list(n), dtype=torch.int32).cumsum(0).to(torch.int32).to(gpu) for n in (sqs, sks))
    sinks = torch.randn(h, generator=torch.Generator().manual_seed(8)).to(gpu) if with_sinks else None
    kw = dict(causal=True, window_size=(17, 0), sinks=sinks)
    out, lse = _call(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, **kw)
    assert out.shape == q.shape and lse.shape == (h, sum(sqs))
    for i, (sq, sk) in enumerate(zip(sqs, sks)):
        a, c = int(cu_q[i]), int(cu_k[i])
        if sq == 0: continue  # noqa: E701
        qi, ki, vi = q[a:a + sq], k[c:c + sk], v[c:c + sk]
        o1, l1 = _call(qi[None], ki[None], vi[None], **kw)
        assert _same(out[a:a + sq], o1[0]) and _same(lse[:, a:a + sq], l1[0]), f"sequence {i} differs from the dense call on it alone"
        _check(o1[0], l1[0], qi, ki, vi, dtname, f"packed d{d} seq{i}", True, (17, 0), sinks, None)
        dead = max(sq - sk, 0)
        want = sinks[:, None].expand(h, dead) if with_sinks else torch.zeros(h, dead, device=gpu)
        assert (o1[0, :dead] == 0).all().item() and torch.equal(l1[0][:, :dead], want), f"sequence {i}: dead rows"


@pytest.mark.parametrize("d", [64, 128])
def test_bit_relations(gpu, d):
    h = 8
    q, k, v = _inputs(gpu, "fp16", d, h, HK, SQ, SK, 300 + d, b=2)
    for kw in (dict(causal=True, window_size=(17, 0)), dict(causal=False)):
        want, again, alone = _call(q, k, v, **kw), _call(q, k, v, **kw), _call(q[1:], k[1:], v[1:], **kw)
        minus = _call(q, k, v, sinks=torch.full((h,), -INF, device=gpu), **kw)
        assert all(_same(x, y) for x, y in zip(want, again)), "two runs differ"
        assert all(_same(x, y) for x, y in zip(want, minus)), "sinks = -inf differs from sinks=None"
        assert all(_same(x[1:], y) for x, y in zip(want, alone)), "a batch entry differs from the call on it alone"
    wide = _call(q, k, v, window_size=(SK, SK))
    assert all(_same(x, y) for x, y in zip(want, wide)), "a window that hides nothing differs from (-1, -1)"


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("d", [64, 128])
def test_never_read(gpu, d, packed):
    """K / V rows below sk - sq - 20 = 240, which no row sees, and the rows behind each packed sequence hold NaN: masking alone gives 0 x NaN"""
    sq, sk, h, dtname, pad = 40, 300, 8, "bf16", 64
    kw = dict(causal=True, window_size=(20, 0))
    q, k, v = _inputs(gpu, dtname, d, h, HK, sq, sk, 400 + d, b=2)
    k[:, :sk - sq - 20], v[:, :sk - sq - 20] = NAN, NAN
    if packed:      # NaN rows: q past cu_seqlens_q[-1]; k / v as the keys of a sequence without queries and past cu_seqlens_k[-1]
        qb = torch.cat([q[0], q[1], torch.full_like(q[0], NAN)])
        kb, vb = (torch.cat([t[0], torch.full_like(t[0, :pad], NAN), t[1], torch.full_like(t[0, :pad], NAN)]) for t in (k, v))
        cu_q = torch.tensor([0, sq, sq, 2 * sq], dtype=torch.int32, device=gpu)
        cu_k = torch.tensor([0, sk, sk + pad, 2 * sk + pad], dtype=torch.int32, device=gpu)
        out, lse = _call(qb, kb, vb, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, **kw)
        outs, lses = [out[:sq], out[sq:2 * sq]], [lse[:, :sq], lse[:, sq:2 * sq]]
    else:
        out, lse = _call(q, k, v, **kw)
        outs, lses = list(out), list(lse)
    for i, (o, l) in enumerate(zip(outs, lses)):
        assert torch.isfinite(o.float()).all().item() and torch.isfinite(l).all().item(), "a key that no row sees was read"
        _check(o, l, q[i], k[i].nan_to_num(0.0), v[i].nan_to_num(0.0), dtname, f"never read d{d} b{i}", True, (20, 0), None, None)


@pytest.mark.parametrize("d", [64, 128])
def test_sinks_at_the_edges(gpu, d):
    """head 1: a sink 30 above every score gives out near 0 and lse near the sink; head 2: a NaN sink gives NaN rows; the other heads keep their bits"""
    h = 8
    q, k, v = _inputs(gpu, "fp16", d, h, HK, SQ, SK, 500 + d, b=1)
    base = torch.randn(h, generator=torch.Generator().manual_seed(9)).to(gpu)
    top = float((torch.einsum("qhd,khd->hqk", q[0].double(), k[0].double().repeat_interleave(h // HK, 1)) * d ** -0.5).max()) + 30.0
    sinks = torch.cat([base[:1], torch.tensor([top, NAN], device=gpu), base[3:]])
    kw = dict(causal=True, window_size=(17, 0))
    (o0, l0), (o1, l1) = _call(q, k, v, sinks=base, **kw), _call(q, k, v, sinks=sinks, **kw)
    assert o1[:, :, 1].abs().max().item() <= 1e-9 and (l1[:, 1] - top).abs().max().item() <= 1e-3
    assert torch.isnan(o1[:, :, 2]).all().item() and torch.isnan(l1[:, 2]).all().item()
    assert _same(o1[:, :, 3:], o0[:, :, 3:]) and _same(l1[:, 3:], l0[:, 3:]) and _same(o1[:, :, 0], o0[:, :, 0]) and _same(l1[:, 0], l0[:, 0])


@pytest.mark.parametrize("d", [64, 128])
def test_timing_builds_reproduce_the_product(gpu, libs, d):
    """the slow-reader and slow-writer builds, twice each, give the product's bits on a windowed packed call with sinks: key ranges of 0 to 9 steps"""
    from flash_attn_turing import capi

    sqs, sks, h, hk = (70, 70, 70, 70), (0, 20, 131, 300), 4, 2
    q, k, v = _inputs(gpu, "bf16", d, h, hk, sum(sqs), sum(sks), 600 + d)
    cu_q, cu_k = (torch.tensor([0] + list(n), dtype=torch.int32).cumsum(0).to(torch.int32).to(gpu) for n in (sqs, sks))
    sinks = torch.randn(h, generator=torch.Generator().manual_seed(10)).to(gpu)

    def run(L):
        o, lse = torch.full(q.shape, NAN, dtype=q.dtype, device=gpu), torch.full((h, q.shape[0]), NAN, device=gpu)
        p = capi.prefill_fwd_params(q, k, v, o, lse, cu_q, cu_k, causal=True, window_size=(200, 0), sinks=sinks)
        rc = L.fa_run_prefill_fwd(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_last_error().decode()
        torch.cuda.synchronize()
        return o, lse

    want = _must_match(libs, run, f"prefill_fwd d{d} packed windowed")
    assert torch.isfinite(want[0].float()).all().item() and torch.isfinite(want[1]).all().item()


def test_slow_writer_catches_the_racy_form(gpu, libs):
    """the teeth of the test above (test_slow_writer_catches_the_barrier_in_front_of_the_store for this file): with the step's barrier in front of store_step
    the waves that do not sleep read a stage whose sleeping quarter still holds its previous tenant.  No window, no causal mask, no sinks: 5 and 33 steps
    of 32 keys that all carry live keys, 140 packed rows a sequence (rows in all four waves of the first tile)."""
    from flash_attn_turing import capi

    sqs, sks, h, hk, d = (70, 70), (131, 1040), 4, 2, 128
    q, k, v = _inputs(gpu, "fp16", d, h, hk, sum(sqs), sum(sks), 700)
    cu_q, cu_k = (torch.tensor([0] + list(n), dtype=torch.int32).cumsum(0).to(torch.int32).to(gpu) for n in (sqs, sks))

    def run(L):
        o, lse = torch.full(q.shape, NAN, dtype=q.dtype, device=gpu), torch.full((h, q.shape[0]), NAN, device=gpu)
        p = capi.prefill_fwd_params(q, k, v, o, lse, cu_q, cu_k)
        rc = L.fa_run_prefill_fwd(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_last_error().decode()
        torch.cuda.synchronize()
        return o, lse

    _must_differ(libs, run, "fp16", "fa_fwd_prefill.hip")
