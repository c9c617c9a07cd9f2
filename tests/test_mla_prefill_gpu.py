"""GPU: MLA prefill attention (flash_mla_prefill_func / fa_run_mla_prefill_fwd; fa_fwd_mla_prefill.hip) - values against the fp64 model of
tests/_mla_prefill_cases.py, the accuracy budget against the rounding model, the exact set of visible keys, the relations stated to the bit, the
edges of the contract, graph capture, the adversarial-timing builds, and one speed relation."""
import ctypes
import statistics

import numpy as np
import pytest
import torch

import _accuracy as A
import _mla_prefill_cases as C
import _util as U
import _visibility as V

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _F():
    import flash_attn_turing as F

    return F


def _call(q, k, v, **kw):
    return _F().flash_mla_prefill_func(q, k, v, return_softmax_lse=True, **kw)


def _same(a, b):
    """two tensors byte for byte (NaN payloads included)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(U.bits(a.contiguous()), U.bits(b.contiguous()))


def _check_sequence(out, lse, q, k, v, causal, dtname, tag):
    """out (sq, h, 128), lse (h, sq) of one sequence against the fp64 model: the tolerances of fwd, LSE_TOL, dead rows exactly O = 0, LSE = 0"""
    o64, l64 = C.model(q.cpu(), k.cpu(), v.cpu(), causal)
    sq, sk = q.shape[0], k.shape[0]
    if sq == 0:
        return
    U.assert_close(out.float().cpu().numpy(), o64.numpy(), dtname, f"mla_prefill O {tag}", sk=sk)
    err = float((lse.double().cpu() - l64).abs().max())
    print(f"mla_prefill LSE {tag}: max err {err:.3e}")
    assert err <= U.LSE_TOL, f"{tag}: LSE err {err:.3e} > {U.LSE_TOL}"
    dead = torch.tensor([sk == 0 or (causal and t < sq - sk) for t in range(sq)])
    assert (out.cpu()[dead] == 0).all().item() and (lse.cpu()[:, dead] == 0).all().item(), f"{tag}: a row that sees no key must be exactly O = 0, LSE = 0"


# ---- 1. values --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", C.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_values_dense(gpu, dtname, heads, causal):
    h, hk = heads
    for n, (sq, sk) in enumerate(C.SHAPES):
        q, k, v = (t.to(gpu) for t in C.inputs(sq, sk, h, hk, dtname, 1000 + n, b=2))
        out, lse = _call(q, k, v, causal=causal)
        assert out.shape == (2, sq, h, C.DV) and out.dtype == q.dtype and lse.shape == (2, h, sq) and lse.dtype == torch.float32
        for i in range(2):
            _check_sequence(out[i], lse[i], q[i], k[i], v[i], causal, dtname, f"dense sq{sq} sk{sk} h{h}/{hk} {'causal' if causal else 'full'} b{i}")


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", C.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_values_packed(gpu, dtname, heads, causal):
    """the packed batch of the issue, and every dense shape as the sequences of one more packed call"""
    h, hk = heads
    for sqs, sks in ((C.PACKED_SQ, C.PACKED_SK), tuple(zip(*C.SHAPES))):
        q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sqs, sks, h, hk, dtname, 2000 + len(sqs)))
        out, lse = _call(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)
        assert out.shape == (sum(sqs), h, C.DV) and lse.shape == (h, sum(sqs))
        for i in range(len(sqs)):
            a, b, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
            _check_sequence(out[a:b], lse[:, a:b], q[a:b], k[c:d], v[c:d], causal, dtname, f"packed seq{i} sq{sqs[i]} sk{sks[i]} h{h}/{hk} {'causal' if causal else 'full'}")


# ---- 2. the accuracy budget -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_accuracy_budget(gpu, dtname, causal):
    """ordinary data, b 2, h 8 = h_k, sq = sk = 777: gain, relative RMS and LSE under the project's bounds (tests/_accuracy.py: budget_check), relative
    to the rounding model on the same inputs (P rounded to the dtype in front of P.V, exact row sums, O rounded once)"""
    b, h, s = 2, 8, 777
    q, k, v = C.inputs(s, s, h, h, dtname, 3000)
    scores = C.scores64(q, k)
    vis = C.causal_mask(s, s) if causal else torch.ones(s, s, dtype=torch.bool)
    om, lse64, o64 = A.rounding_model(scores, vis, v.double().permute(0, 2, 1, 3), dtname)
    yard = A.lse_yardstick(scores, vis, lse64)
    out, lse = _call(q.to(gpu), k.to(gpu), v.to(gpu), causal=causal)
    A.budget_check(f"mla_prefill {'causal' if causal else 'full'} b{b} h{h} s{s}", dtname, out.permute(0, 2, 1, 3), om, o64, None, lse, lse64, yard)


# ---- 3. visibility, exact ---------------------------------------------------------------------------------------------------------------------

def _vis_kv(c, rows, gpu):
    """K = 0 (192 wide) and V = the codes of `rows` at width 128 with three more rows of the bad code behind: (rows + 3, hk, .)"""
    dt = V.torch_dtype(c.dtype)
    v = torch.full((len(rows) + 3, c.hk, c.d), V.BAD, dtype=dt, device=gpu)
    v[: len(rows)] = V.code_tensor(c.d, c.cap, gpu)[rows].to(dt).unsqueeze(1)
    return torch.zeros(len(rows) + 3, c.hk, C.DQK, dtype=dt, device=gpu), v


def _vis_check(c, out, lse):
    n_dec, hist_dec = V.decode(out, lse, torch.tensor(c.sink_extra()))
    n_exp, hist_exp, rows = V.expected(c)            # (asserts the probe's conditions on the inputs: capacity, counts per digit, n <= 4096)
    V.assert_signature(c, n_dec, hist_dec, n_exp, hist_exp, rows)


@pytest.mark.parametrize("dtname", C.DTYPES)
def test_visible_keys_dense_causal(gpu, dtname):
    """every (sq, sk) of the causal table of _visibility.attn_pairs, sq > sk included; h / h_k rotates through 1, 4 and 6 / 1"""
    for j, (sq, sk) in enumerate(V.attn_pairs(True)):
        h, hk = V.ATTN_HEADS[(j + C.DTYPES.index(dtname)) % 3]
        c = V.Case(family="mla_prefill", name=f"mla_prefill/sq{sq}-sk{sk}-causal-{dtname}-h{h}_{hk}", lens=(sk,), sq=(sq,), d=C.DV, dtype=dtname, h=h, hk=hk, causal=True, cap=1024)
        gen = torch.Generator().manual_seed(sq * 1031 + sk)
        q = torch.randn(1, sq, h, C.DQK, generator=gen).to(gpu, V.torch_dtype(dtname))
        k, v = _vis_kv(c, torch.arange(sk, device=gpu), gpu)
        out, lse = _call(q, k[:sk].unsqueeze(0), v[:sk].unsqueeze(0), causal=True)
        _vis_check(c, out[0], lse[0].t())


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("heads", C.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_visible_keys_packed(gpu, dtname, heads, causal):
    h, hk = heads
    c = V.Case(family="mla_prefill", name=f"mla_prefill/packed-{'causal' if causal else 'full'}-{dtname}-h{h}_{hk}", lens=C.PACKED_SK, sq=C.PACKED_SQ, d=C.DV, dtype=dtname,
               h=h, hk=hk, causal=causal, cap=1024, ragged=True)
    gen = torch.Generator().manual_seed(17)
    q = torch.randn(sum(c.sq), h, C.DQK, generator=gen).to(gpu, V.torch_dtype(dtname))
    k, v = _vis_kv(c, torch.cat([torch.arange(L, device=gpu) for L in c.lens]), gpu)
    out, lse = _call(q, k[: sum(c.lens)], v[: sum(c.lens)], cu_seqlens_q=C.cu(c.sq, gpu), cu_seqlens_k=C.cu(c.lens, gpu), causal=causal)
    _vis_check(c, out, lse.t())


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_packed_sequence_equals_the_dense_call_on_it_alone(gpu, dtname, causal):
    h, hk = 6, 2
    sqs, sks = C.PACKED_SQ + (200,), C.PACKED_SK + (1040,)
    q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sqs, sks, h, hk, dtname, 4000))
    out, lse = _call(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)
    again, lse2 = _call(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)
    assert _same(out, again) and _same(lse, lse2), "two runs differ"
    for i in range(len(sqs)):
        a, b, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
        if a == b:
            continue
        o1, l1 = _call(q[a:b].unsqueeze(0), k[c:d].unsqueeze(0), v[c:d].unsqueeze(0), causal=causal)
        assert _same(out[a:b], o1[0]) and _same(lse[:, a:b], l1[0]), f"sequence {i} (sq {sqs[i]}, sk {sks[i]}) of the packed call differs from the dense call on it alone"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_dense_bits(gpu, dtname, causal):
    """a batch entry == the call on it alone; softmax_scale=None == 192 ** -0.5 passed; a power of two moved between q and softmax_scale; two runs"""
    q, k, v = (t.to(gpu) for t in C.inputs(130, 131, 6, 2, dtname, 4100, b=3))
    out, lse = _call(q, k, v, causal=causal)
    o2, l2 = _call(q, k, v, causal=causal)
    assert _same(out, o2) and _same(lse, l2), "two runs differ"
    for i in range(3):
        o1, l1 = _call(q[i:i + 1], k[i:i + 1], v[i:i + 1], causal=causal)
        assert _same(out[i], o1[0]) and _same(lse[i], l1[0]), f"batch entry {i} differs from the call on it alone"
    o3, l3 = _call(q, k, v, causal=causal, softmax_scale=C.SCALE)
    assert _same(out, o3) and _same(lse, l3), "softmax_scale=None and 192 ** -0.5 differ"
    # (fp16 moves the factor upwards only: a small element of q times 1 / 8 lands among fp16's subnormals and loses bits - asserted on the inputs)
    for p in ((4.0, 16.0) if dtname == "fp16" else (4.0, 0.125)):
        assert torch.equal((q * p).double(), q.double() * p), f"q x {p} is not exact in {dtname}: the relation does not apply to these inputs"
        o4, l4 = _call(q * p, k, v, causal=causal, softmax_scale=C.SCALE / p)
        assert _same(out, o4) and _same(lse, l4), f"a factor {p} moved from softmax_scale into q changes bits"


# ---- 5. edges ---------------------------------------------------------------------------------------------------------------------------------

def _run_capi(L, q, k, v, o, lse, cu_q=None, cu_k=None, causal=False, scale=None):
    from flash_attn_turing import capi

    p = capi.mla_prefill_params(q, k, v, o, lse, cu_q, cu_k, causal, scale)
    rc = L.fa_run_mla_prefill_fwd(ctypes.byref(p), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.fa_last_error().decode()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_guard_buffers_dense(gpu, dtname, causal):
    """q / k / v / o as views into larger buffers whose gaps hold NaN, +-inf and 65504 (inputs) or a sentinel (o): the result is the contiguous
    call's, bit for bit, and no byte of o's buffer outside the view changes"""
    from flash_attn_turing import capi

    dt = C.DT[dtname]
    b, sq, sk, h, hk = 2, 65, 97, 6, 2
    q, k, v = (t.to(gpu) for t in C.inputs(sq, sk, h, hk, dtname, 5000, b=b))
    want, lse_want = _call(q, k, v, causal=causal)
    views = []
    for t in (q, k, v):
        _, view, _ = U.guarded(tuple(t.shape), dt, gpu, (2, 4, 2, 16), fill=None)
        view.copy_(t)
        views.append(view)
    out, lse = _call(*views, causal=causal)
    assert _same(out, want) and _same(lse, lse_want), "gaps of strided views reached a result"
    obuf, oview, sl = U.guarded((b, sq, h, C.DV), dt, gpu, (2, 4, 2, 16))
    lse2 = torch.full((b, h, sq), NAN, device=gpu)
    _run_capi(capi.lib(), *views, oview, lse2, causal=causal)
    torch.cuda.synchronize()
    assert _same(oview, want) and _same(lse2, lse_want)
    mask = torch.ones(obuf.shape, dtype=torch.bool, device=gpu)
    mask[sl] = False
    assert (U.bits(obuf)[mask] == U.SENT16).all().item(), "a byte of o's buffer outside the view was written"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_guard_rows_packed(gpu, dtname, causal):
    """packed: rows of k / v past cu_seqlens_k[-1] and rows of q past cu_seqlens_q[-1] hold NaN / inf and change nothing; the rows of out / lse past
    cu_seqlens_q[-1] keep their sentinel; every sequence still equals the model (other sequences' rows never reach it)"""
    from flash_attn_turing import capi

    dt = C.DT[dtname]
    h, hk, extra = 4, 1, 5
    sqs, sks = C.PACKED_SQ, C.PACKED_SK
    q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sqs, sks, h, hk, dtname, 5100))
    want, lse_want = _call(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)
    tq, tk = sum(sqs), sum(sks)
    qb, kb, vb = (U.poison_(torch.empty((t.shape[0] + extra,) + tuple(t.shape[1:]), dtype=dt, device=gpu)) for t in (q, k, v))
    qb[:tq], kb[:tk], vb[:tk] = q, k, v
    o = torch.full((tq + extra, h, C.DV), U.SENT16, dtype=torch.int16, device=gpu).view(dt)
    lse = torch.full((h, tq + extra), 1234.5, device=gpu)
    _run_capi(capi.lib(), qb, kb, vb, o, lse, cu_q, cu_k, causal=causal)
    torch.cuda.synchronize()
    assert _same(o[:tq], want) and _same(lse[:, :tq], lse_want), "rows past cu_seqlens reached a result"
    assert (U.bits(o[tq:]) == U.SENT16).all().item() and (lse[:, tq:] == 1234.5).all().item(), "rows of out / lse past cu_seqlens_q[-1] were written"
    out2, lse2 = _call(qb, kb, vb, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)
    assert _same(out2[:tq], want) and _same(lse2[:, :tq], lse_want)
    for i in range(len(sqs)):
        a, b, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
        _check_sequence(want[a:b], lse_want[:, a:b], q[a:b], k[c:d], v[c:d], causal, dtname, f"guarded packed seq{i}")


@pytest.mark.parametrize("dtname", C.DTYPES)
def test_nan_query_row_and_nan_key_hit_the_rows_the_contract_names(gpu, dtname):
    b, sq, sk, h, hk = 1, 70, 100, 4, 2
    q, k, v = (t.to(gpu) for t in C.inputs(sq, sk, h, hk, dtname, 5200, b=b))
    base, lse_base = _call(q, k, v, causal=True)
    assert torch.isfinite(base.float()).all().item()
    # a NaN in query row (t = 37, head 3): that row alone
    qn = q.clone()
    qn[0, 37, 3, 190] = NAN
    out, lse = _call(qn, k, v, causal=True)
    hit = torch.zeros(sq, h, dtype=torch.bool, device=gpu)
    hit[37, 3] = True
    assert torch.isnan(out[0].float()).all(-1).eq(hit).all().item() and torch.isnan(lse[0].t()).eq(hit).all().item()
    assert _same(out[0][~hit], base[0][~hit]) and _same(lse[0].t()[~hit], lse_base[0].t()[~hit])
    # a NaN element of key 50 of KV head 1: the rows of query heads 2, 3 that see key 50 under the mask (j <= sk - sq + t: t >= 20), O and LSE
    kn = k.clone()
    kn[0, 50, 1, 130] = NAN
    out, lse = _call(q, kn, v, causal=True)
    hit = torch.zeros(sq, h, dtype=torch.bool, device=gpu)
    hit[50 - (sk - sq):, 2:] = True
    assert torch.isnan(out[0].float()).all(-1).eq(hit).all().item() and torch.isnan(lse[0].t()).eq(hit).all().item()
    assert _same(out[0][~hit], base[0][~hit]) and _same(lse[0].t()[~hit], lse_base[0].t()[~hit])
    # -inf as a score only drops the key: key 7 of KV head 0 is -inf x positive q
    kq = k.clone()
    kq[0, 7, 0] = 0
    kq[0, 7, 0, 0] = float("-inf")
    qp = q.clone()
    qp[..., 0] = qp[..., 0].abs() + 1
    out, lse = _call(qp, kq, v, causal=False)
    keep = [j for j in range(sk) if j != 7]
    o_want, l_want = _call(qp[:, :, :2], kq[:, keep, :1], v[:, keep, :1], causal=False)
    U.assert_close(out[0, :, :2].float().cpu().numpy(), o_want[0].double().cpu().numpy(), dtname, "mla_prefill -inf score drops the key", sk=sk - 1)
    assert float((lse[0, :2] - l_want[0]).abs().max()) <= U.LSE_TOL


@pytest.mark.parametrize("dtname", C.DTYPES)
def test_q_k_v_sliced_from_one_fused_buffer(gpu, dtname):
    b, s, h = 2, 130, 4
    q, k, v = (t.to(gpu) for t in C.inputs(s, s, h, h, dtname, 5300, b=b))
    fused = torch.cat([q, k, v], dim=-1)                 # (b, s, h, 512): head stride 512, row stride 2048, offsets 0 / 192 / 384
    fq, fk, fv = fused[..., :192], fused[..., 192:384], fused[..., 384:]
    assert not fq.is_contiguous() and fk.storage_offset() == 192 and fv.stride(2) == 512
    want, lse_want = _call(q, k, v, causal=True)
    out, lse = _call(fq, fk, fv, causal=True)
    assert _same(out, want) and _same(lse, lse_want)
    pk = torch.cat([q.flatten(0, 1), k.flatten(0, 1), v.flatten(0, 1)], dim=-1)
    cu = C.cu((s, s), gpu)
    out, lse = _call(pk[..., :192], pk[..., 192:384], pk[..., 384:], cu_seqlens_q=cu, cu_seqlens_k=cu, causal=True)
    assert _same(out.view(b, s, h, C.DV), want) and _same(lse.view(h, b, s).permute(1, 0, 2), lse_want)


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------------

def test_graph_replay_follows_new_cu_seqlens(gpu):
    """one capture, one replay: cu_seqlens_q / cu_seqlens_k rewritten in place (same totals), compared with an eager call"""
    h, hk = 6, 2
    sq_a, sk_a, sq_b, sk_b = (64, 0, 130, 18), (97, 33, 131, 5), (1, 17, 64, 130), (0, 5, 130, 131)
    assert sum(sq_a) == sum(sq_b) and sum(sk_a) == sum(sk_b)
    q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sq_a, sk_a, h, hk, "bf16", 6000))
    call = lambda: _call(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                    # warm-up outside the capture (allocator, module load)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = call()
    cu_q.copy_(C.cu(sq_b, gpu)), cu_k.copy_(C.cu(sk_b, gpu))
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = call()
    assert _same(out_g, out_e) and _same(lse_g, lse_e), "the replay did not follow the rewritten cu_seqlens"
    for i in range(len(sq_b)):
        a, b, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
        _check_sequence(out_g[a:b], lse_g[:, a:b], q[a:b], k[c:d], v[c:d], True, "bf16", f"graph replay seq{i}")


# ---- 7. the adversarial-timing builds ---------------------------------------------------------------------------------------------------------

TIMING = ("stage_slow_reader", "stage_slow_writer")
RACY = "stage_racy_slow_writer"
STEP_LENS = (0, 20, 40, 90, 128, 131, 1040)         # keys of a sequence: 0, 1, 2, 3, 4, 5 and 33 steps of 32


@pytest.fixture(scope="module")
def libs(gpu):
    from flash_attn_turing import capi
    from test_stage_protocol_gpu import _build_module

    fa_build = _build_module()
    fa_build.build_debug_variants(force=False)          # a no-op when build() has run (the .so files travel with the tree)
    out = {"product": capi.lib()}
    for name in TIMING + (RACY,):
        L = ctypes.CDLL(fa_build.debug_library_path(name))
        L.fa_run_mla_prefill_fwd.argtypes = [ctypes.POINTER(capi.MlaPrefillParams), ctypes.c_void_p]
        L.fa_run_mla_prefill_fwd.restype = ctypes.c_int
        L.fa_last_error.restype = ctypes.c_char_p
        out[name] = L
    return out


def _timing_case(gpu, dtname, causal, packed):
    dt = C.DT[dtname]
    h, hk, sq = 4, 2, 70
    n = len(STEP_LENS)
    if packed:
        q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs((sq,) * n, STEP_LENS, h, hk, dtname, 7000))
    else:
        q, k, v = (t.to(gpu) for t in C.inputs(sq, 1040, h, hk, dtname, 7001, b=2))
        cu_q = cu_k = None

    def run(L):
        o = torch.full(tuple(q.shape[:-1]) + (C.DV,), NAN, dtype=dt, device=gpu)
        lse = torch.full((h, q.shape[0]) if packed else (2, h, sq), NAN, device=gpu)
        _run_capi(L, q, k, v, o, lse, cu_q, cu_k, causal=causal)
        torch.cuda.synchronize()
        return o, lse

    return run


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_timing_builds_reproduce_the_product(gpu, libs, dtname, causal, packed):
    """the slow-reader and slow-writer builds, twice each, give the product's bits: lengths of 0, 1, 2, 3, 4, 5 and 33 steps in one packed call, and a
    dense call of 33 steps"""
    from test_stage_protocol_gpu import _must_match

    want = _must_match(libs, _timing_case(gpu, dtname, causal, packed), f"mla_prefill {dtname} {'causal' if causal else 'full'} {'packed' if packed else 'dense'}")
    assert torch.isfinite(want[0].float()).all().item() and torch.isfinite(want[1]).all().item()


@pytest.mark.parametrize("dtname", C.DTYPES)
def test_racy_form_is_exposed_by_the_slow_writer(gpu, libs, dtname):
    from test_stage_protocol_gpu import _must_differ

    _must_differ(libs, _timing_case(gpu, dtname, False, False), dtname, f"mla_prefill {dtname} dense")


# ---- 8. one speed relation --------------------------------------------------------------------------------------------------------------------

def test_faster_than_the_padded_head_dim_256_kvcache_call(gpu):
    """b 1, sq = sk = 1024, h = h_k = 16, bf16, causal: the median of 5 interleaved rounds of flash_mla_prefill_func must lie below that of what a user
    could do before it - flash_attn_with_kvcache at head_dim 256 on zero-padded q / k / v with the same softmax_scale, which re-reads K / V once per
    16-row tile.  The bound is 1.0 and carries no margin; the ratio is printed (profiles/mla_prefill_bench.log holds the run recorded with the change)."""
    F = _F()
    b, s, h = 1, 1024, 16
    q, k, v = (t.to(gpu) for t in C.inputs(s, s, h, h, "bf16", 8000, b=b))
    pad = lambda t: torch.nn.functional.pad(t, (0, 256 - t.shape[-1]))
    q2, k2, v2 = pad(q), pad(k), pad(v)
    new = lambda: F.flash_mla_prefill_func(q, k, v, causal=True)
    old = lambda: F.flash_attn_with_kvcache(q2, k2, v2, causal=True, softmax_scale=C.SCALE)
    a, o = new(), old()[..., :128]
    m = U.error_metrics(a.float().cpu().numpy(), o.float().cpu().numpy())
    assert m["max_abs"] <= U.TOL["bf16"]["max_abs"], m                     # (the same values: both within the tolerance of fp64, so within one of each other)
    torch.cuda.synchronize()
    tn, to = [], []
    for _ in range(5):
        for fn, ts in ((new, tn), (old, to)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / 3)
    n, w = statistics.median(tn), statistics.median(to)
    line = f"test_faster_than_padded_d256: b{b} sq{s} sk{s} h{h}/{h} bf16 causal: flash_mla_prefill_func {n:.4f} ms, padded head_dim-256 kvcache call {w:.4f} ms, ratio {n / w:.3f}"
    print(line)
    assert n < w, line
