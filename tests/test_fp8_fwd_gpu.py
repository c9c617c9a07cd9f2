"""GPU: the FP8 (e4m3) dense attention forward (flash_attn_fp8_func / fa_run_fp8_fwd; fa_fwd_fp8.hip) - accuracy against fp64 within the budget of a
rounding model, a case that separates the quantisation contract from its neighbours, the relations stated to the bit, NaN codes."""
import functools

import pytest
import torch

import _util as U
import flash_attn_turing as F
from test_stage_protocol_gpu import _must_differ, _must_match, libs  # noqa: F401  (libs: the product and the adversarial-timing builds)

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn
SHAPES = [(1, 1), (3, 127), (65, 129), (130, 64), (200, 333)]      # one key; one short of / one past the 128-key step; a tile with a tail; dead rows; several steps
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
BUDGET = 1.25       # relative RMS error of out <= BUDGET x the rounding model's (the rule of test_accuracy_budget_gpu.py)
SCALE = float(torch.tensor(128 ** -0.5, dtype=torch.float32))


def _call(q, k, v, **kw):
    return F.flash_attn_fp8_func(q, k, v, return_softmax_lse=True, **kw)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(U.bits(a.contiguous()), U.bits(b.contiguous()))


@functools.lru_cache(maxsize=None)
def _inputs(sq, sk, h, hk, seed):
    """codes q (sq, h, 128), k / v (sk, hk, 128) of N(0, 1) tensors under per-head descales that are no powers of two, and the descales (1, h) / (1, hk)"""
    g = torch.Generator().manual_seed(seed)
    qd, kd, vd = (torch.linspace(lo, hi, n).reshape(1, n) for lo, hi, n in ((0.037, 0.21, h), (0.05, 0.5, hk), (0.043, 0.33, hk)))
    q, k, v = (torch.randn(s, n, 128, generator=g) for s, n in ((sq, h), (sk, hk), (sk, hk)))
    return (q / qd[0, :, None]).to(E4M3), (k / kd[0, :, None]).to(E4M3), (v / vd[0, :, None]).to(E4M3), qd, kd, vd


def _model(qc, kc, vc, qd, kd, vd, causal):
    """fp64 attention on the dequantised operands (out, lse), and the rounding model's out before its last rounding: the same computation walked in
    128-key steps with a running maximum, P replaced by e4m3(256 p) / 256 in the numerator only"""
    (sq, h), (sk, hk) = qc.shape[:2], kc.shape[:2]
    q = qc.double() * qd[0, :, None].double()
    k = (kc.double() * kd[0, :, None].double()).repeat_interleave(h // hk, 1)
    v = (vc.double() * vd[0, :, None].double()).repeat_interleave(h // hk, 1)
    s = torch.einsum("thd,jhd->htj", q, k) * SCALE
    t, j = torch.arange(sq)[:, None], torch.arange(sk)[None, :]
    s = s.masked_fill(~((j <= sk - sq + t) if causal else torch.ones(sq, sk, dtype=torch.bool)), float("-inf"))
    lse = torch.logsumexp(s, -1)
    dead = torch.isinf(lse)
    out = torch.einsum("htj,jhd->thd", torch.exp(s - lse.masked_fill(dead, 0)[..., None]), v)
    m, l, acc = torch.full((h, sq), -1e30, dtype=torch.float64), torch.zeros(h, sq, dtype=torch.float64), torch.zeros(sq, h, 128, dtype=torch.float64)
    for j0 in range(0, sk, 128):
        m_new = torch.maximum(m, s[..., j0:j0 + 128].amax(-1))
        p, alpha = torch.exp(s[..., j0:j0 + 128] - m_new[..., None]), torch.exp(m - m_new)
        p8 = (256 * p).float().to(E4M3).double() / 256
        l, acc, m = l * alpha + p.sum(-1), acc * alpha.T[..., None] + torch.einsum("htj,jhd->thd", p8, v[j0:j0 + 128]), m_new
    return out, lse.masked_fill(dead, 0), acc / l.T.clamp_min(1e-300)[..., None], dead


_expect = functools.lru_cache(maxsize=None)(lambda sq, sk, h, hk, seed, causal: _model(*_inputs(sq, sk, h, hk, seed), causal))


def _relrms(x, ref):
    return float(((x - ref) ** 2).sum().sqrt() / (ref ** 2).sum().sqrt().clamp_min(1e-300))


@pytest.mark.parametrize("heads", [(2, 2), (4, 1)], ids=lambda x: f"h{x[0]}_{x[1]}")
@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_accuracy_against_fp64(gpu, dtname, causal, packed, heads):
    h, hk = heads
    seqs = [(sq, sk, 7000 + n) for n, (sq, sk) in enumerate(SHAPES)]
    got = []
    if packed:
        seqs.insert(2, (0, 0, 0))       # an empty sequence in the middle of the batch
        ins = [_inputs(sq, sk, h, hk, seed) for sq, sk, seed in seqs]
        cu_q = torch.tensor([0] + [s[0] for s in seqs], dtype=torch.int32).cumsum(0).int().to(gpu)
        cu_k = torch.tensor([0] + [s[1] for s in seqs], dtype=torch.int32).cumsum(0).int().to(gpu)
        q, k, v = (torch.cat([i[n].view(torch.uint8) for i in ins]).view(E4M3).to(gpu) for n in range(3))
        qd, kd, vd = (torch.cat([i[n] for i in ins]).to(gpu) for n in (3, 4, 5))
        out, lse = _call(q, k, v, q_descale=qd, k_descale=kd, v_descale=vd, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal, out_dtype=DT[dtname])
        assert out.shape == (q.shape[0], h, 128) and out.dtype == DT[dtname] and lse.shape == (h, q.shape[0]) and lse.dtype == torch.float32
        got = [(out[a:b], lse[:, a:b]) for a, b in zip(cu_q.tolist()[:-1], cu_q.tolist()[1:])]
    else:
        for sq, sk, seed in seqs:
            qc, kc, vc, qd, kd, vd = (x.to(gpu) for x in _inputs(sq, sk, h, hk, seed))
            out, lse = _call(qc[None], kc[None], vc[None], q_descale=qd, k_descale=kd, v_descale=vd, causal=causal, out_dtype=DT[dtname])
            assert out.shape == (1, sq, h, 128) and out.dtype == DT[dtname] and lse.shape == (1, h, sq) and lse.dtype == torch.float32
            got.append((out[0], lse[0]))
    for (sq, sk, seed), (out, lse) in zip(seqs, got):
        if sq == 0:
            continue
        o64, l64, model, dead = _expect(sq, sk, h, hk, seed, causal)
        out, lse = out.double().cpu(), lse.double().cpu()
        assert (out[dead.T] == 0).all() and (lse[dead] == 0).all(), f"({sq}, {sk}): a row that sees no key must be exactly O = 0, LSE = 0"
        if dead.all():
            continue
        e_kernel, e_model, e_lse = _relrms(out, o64), _relrms(model.to(DT[dtname]).double(), o64), float((lse - l64).abs().max())
        print(f"fp8_fwd {dtname} causal={causal} {'packed' if packed else 'dense'} h={h}/{hk} ({sq}, {sk}): relrms kernel {e_kernel:.4e} model {e_model:.4e} lse {e_lse:.2e}")
        assert e_kernel <= BUDGET * e_model, f"({sq}, {sk}): relrms {e_kernel:.4e} > {BUDGET} x the model's {e_model:.4e}"
        assert e_lse <= U.LSE_TOL, f"({sq}, {sk}): LSE err {e_lse:.3e} > {U.LSE_TOL}"


def test_a_long_tail_of_small_weights(gpu):
    """The case that separates the contract from its neighbours (the budget above does not: on N(0, 1) inputs a model without the x 256 stays inside it).
    One query, key 0 with p = 1 and 2000 keys with the SAME weight p = exp(-128 * 128 ** -0.5) = 1.22e-5, in [2^-18, 2^-10); V is zero on key 0.  256 p is
    1.60 subnormal steps of e4m3, so the contract's numerator takes 2 steps a key and its denominator 1 + 2000 p = 1.0244.  Against that: P = e4m3(p) gives
    out = 0; a truncated 256 p gives half of out; a denominator over the rounded P is 1.0305: out lower by 5.9e-3, LSE higher by 5.9e-3.
    Bound of out (fp16, values of 0.01 .. 0.08: normal numbers): half a unit of fp16, 2^-11, plus 2^-12 for the fp32 sum of 2001 weights (<= 2001 x 2^-24)
    and the fp32 exponentials; LSE within _util.LSE_TOL."""
    q, k, v = (torch.zeros(n, 1, 128) for n in (1, 2001, 2001))
    q[0, 0, 0], k[0, 0, 0] = 8.0, 16.0
    v[1:, 0] = (torch.arange(128) % 7 + 1).float()
    q8, k8, v8 = q.to(E4M3), k.to(E4M3), v.to(E4M3)
    vd = torch.tensor([[0.37]])
    out, lse = _call(q8[None].to(gpu), k8[None].to(gpu), v8[None].to(gpu), v_descale=vd.to(gpu), out_dtype=torch.float16)
    _, l64, model, _ = _model(q8, k8, v8, torch.ones(1, 1), torch.ones(1, 1), vd, False)
    rel = float(((out[0].double().cpu() - model) / model).abs().max())
    print(f"fp8_fwd tail of small weights: out max rel err {rel:.3e}, lse err {float((lse[0].double().cpu() - l64).abs().max()):.2e}")
    assert rel <= 2.0 ** -11 + 2.0 ** -12 and float((lse[0].double().cpu() - l64).abs().max()) <= U.LSE_TOL


@pytest.mark.parametrize("causal", [False, True])
def test_bit_relations(gpu, causal):
    h, hk = 4, 2
    ins = [_inputs(sq, sk, h, hk, 7100 + n) for n, (sq, sk) in enumerate([(65, 129), (200, 333)])]
    cu_q, cu_k = (torch.tensor(c, dtype=torch.int32, device=gpu) for c in ([0, 65, 265], [0, 129, 462]))
    q, k, v = (torch.cat([i[n].view(torch.uint8) for i in ins]).view(E4M3).to(gpu) for n in range(3))
    qd, kd, vd = (torch.cat([i[n] for i in ins]).to(gpu) for n in (3, 4, 5))
    kw = dict(causal=causal, out_dtype=torch.bfloat16)
    out, lse = _call(q, k, v, q_descale=qd, k_descale=kd, v_descale=vd, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, **kw)
    again = _call(q, k, v, q_descale=qd, k_descale=kd, v_descale=vd, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, **kw)
    assert _same(out, again[0]) and _same(lse, again[1]), "two runs differ"
    for n, (a, b, c, d) in enumerate([(0, 65, 0, 129), (65, 265, 129, 462)]):
        one = _call(q[None, a:b], k[None, c:d], v[None, c:d], q_descale=qd[n:n + 1], k_descale=kd[n:n + 1], v_descale=vd[n:n + 1], **kw)
        assert _same(out[a:b], one[0][0]) and _same(lse[:, a:b], one[1][0]), f"sequence {n} of the packed call is not the dense call on it alone"
    # a batch entry of a dense call is the call on it alone; a factor of 2 moved from k_descale into softmax_scale changes no bit
    qb, kb, vb = (torch.stack([x[:64], x[64:128]]) for x in (q, k, v))
    both = _call(qb, kb, vb, q_descale=qd, k_descale=kd, v_descale=vd, **kw)
    for n in range(2):
        one = _call(qb[n:n + 1], kb[n:n + 1], vb[n:n + 1], q_descale=qd[n:n + 1], k_descale=kd[n:n + 1], v_descale=vd[n:n + 1], **kw)
        assert _same(both[0][n:n + 1], one[0]) and _same(both[1][n:n + 1], one[1]), f"batch entry {n} is not the call on it alone"
    moved = _call(qb, kb, vb, q_descale=qd, k_descale=kd / 2, v_descale=vd, softmax_scale=2 * SCALE, **kw)
    assert _same(both[0], moved[0]) and _same(both[1], moved[1]), "a factor of 2 moved from k_descale into softmax_scale changed a bit"
    # a row with exactly one visible key: row 0 under causal with sq = sk, every row with one key
    for sk in ([1] if not causal else [1, 64]):
        o1, _ = _call(qb[:, :sk], kb[:, :sk], vb[:, :sk], q_descale=qd, k_descale=kd, v_descale=vd, **kw)
        want = (vb[:, 0].float() * vd[:, :, None]).to(torch.bfloat16).repeat_interleave(h // hk, 1)
        assert _same(o1[:, 0], want), f"sk = {sk}: a row with one visible key is not float(v_code) * v_descale rounded once"


def test_nan_codes(gpu):
    qc, kc, vc, qd, kd, vd = (x.to(gpu) for x in _inputs(200, 200, 2, 2, 7200))
    q8, k8 = qc.view(torch.uint8).clone(), kc.view(torch.uint8).clone()
    q8[70, 1, 5] = 0x7F         # a NaN code in query row 70 of head 1
    k8[150, 0, 9] = 0x7F        # ... and in key 150 of head 0: causal hides it from rows 0 .. 149
    out, lse = _call(q8.view(E4M3)[None], k8.view(E4M3)[None], vc[None], q_descale=qd, k_descale=kd, v_descale=vd, causal=True)
    bad_o, bad_l = torch.isnan(out[0].float()).any(-1).cpu(), torch.isnan(lse[0]).T.cpu()      # (sq, h)
    want = torch.zeros(200, 2, dtype=torch.bool)
    want[70, 1] = True
    want[150:, 0] = True
    assert torch.equal(bad_o, want) and torch.equal(bad_l, want), f"NaN rows: O {bad_o.nonzero().tolist()[:8]} LSE {bad_l.nonzero().tolist()[:8]}"


# ---- the adversarial-timing builds (tests/test_stage_protocol_gpu.py) ------------------------------------------------------------------------------

def _stage_case(gpu, sqs, sks, h, hk, causal, seed, dtname="bf16"):
    """-> run(library): one packed call through the C ABI of the loaded library, fa_fp8_fwd_params filled here; N(0, 1) codes, so that neighbouring
    steps hold different rows"""
    import ctypes

    from flash_attn_turing import capi

    ins = [_inputs(sq, sk, h, hk, seed + n) for n, (sq, sk) in enumerate(zip(sqs, sks))]
    cu_q, cu_k = (torch.tensor([0] + list(n), dtype=torch.int32).cumsum(0).int().to(gpu) for n in (sqs, sks))
    q, k, v = (torch.cat([i[n].view(torch.uint8) for i in ins]).view(E4M3).to(gpu) for n in range(3))
    qd, kd, vd = (torch.cat([i[n] for i in ins]).to(gpu) for n in (3, 4, 5))

    def run(L):
        o, lse = torch.full((q.shape[0], h, 128), float("nan"), dtype=DT[dtname], device=gpu), torch.full((h, q.shape[0]), float("nan"), device=gpu)
        p = capi.Fp8FwdParams()
        p.q, p.k, p.v, p.o, p.lse = (t.data_ptr() for t in (q, k, v, o, lse))
        p.q_descale, p.k_descale, p.v_descale = (t.data_ptr() for t in (qd, kd, vd))
        p.cu_seqlens_q, p.cu_seqlens_k = cu_q.data_ptr(), cu_k.data_ptr()
        p.b, p.h, p.h_k, p.d, p.out_dtype, p.is_causal = len(sqs), h, hk, 128, capi.FA_BF16 if dtname == "bf16" else capi.FA_FP16, int(causal)
        p.total_q, p.total_k = q.shape[0], k.shape[0]
        for name, t in (("q_stride", q), ("k_stride", k), ("v_stride", v), ("o_stride", o)):
            setattr(p, name, capi.Strides(0, t.stride(0), t.stride(1)))
        (p.q_descale_batch_stride, p.q_descale_head_stride), (p.k_descale_batch_stride, p.k_descale_head_stride) = qd.stride(), kd.stride()
        p.v_descale_batch_stride, p.v_descale_head_stride = vd.stride()
        rc = L.fa_run_fp8_fwd(ctypes.byref(p), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.fa_last_error().decode()
        torch.cuda.synchronize()
        return o, lse

    return run


def test_timing_builds_reproduce_the_product(gpu, libs):
    """the slow-reader and slow-writer builds, twice each, give the product's bits on a packed causal call: key ranges of 0, 1, 2 and 6 steps of 128 keys,
    140 packed rows a sequence (rows in all four waves, a third tile of 12 rows)"""
    run = _stage_case(gpu, (70,) * 4, (0, 20, 131, 700), 4, 2, True, 7300)
    want = _must_match(libs, run, "fp8_fwd packed causal")
    assert torch.isfinite(want[0].float()).all().item() and torch.isfinite(want[1]).all().item()


def test_slow_writer_catches_the_racy_form(gpu, libs):
    """the teeth of the test above (test_slow_writer_catches_the_barrier_in_front_of_the_store for this file): with the step's barrier in front of store_step
    the waves that do not sleep read a stage whose sleeping quarter still holds its previous tenant.  Non-causal, 5 and 9 steps of 128 keys, rows in all four
    waves: every step carries live keys."""
    run = _stage_case(gpu, (70, 70), (513, 1040), 4, 2, False, 7400)
    _must_differ(libs, run, "bf16", "fa_fwd_fp8.hip")
