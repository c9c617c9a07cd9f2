"""GPU: every kernel family's error on ordinary random data is bounded by the rounding model's (tests/_accuracy.py).

Per output tensor of a call, against the fp64 expectation (not rounded to the output type) and the rounding model run on the same inputs:
|gain| <= 2^-13 (fp16) / 2^-10 (bf16), relrms <= 1.25 x the model's, and for the LSE max error <= max(4 x the fp32 yardstick, 2^-20 max(|lse|, 1))
and |mean error| <= 2^-20 - on the whole tensor and on every length class (dense and packed: every sequence) that has 4096 live elements
of its own.  tests/test_accuracy_budget_cpu.py shows on these very inputs that the model passes and that a truncating pack, a factor of a
quarter ulp on O, a scale off by 2^-12, a 16-bit v_descale, 16-bit merge weights, a sink counted twice and one dropped key of 777 do not.
Not covered: non-finite inputs and the value formats (tests/test_kvcache_number_formats_gpu.py, the number-range and edges suites), which
keys a row sees (the visibility suites), speed.  One line per call, tensor and statistic is printed (profiles/accuracy_budget.log: a run's worst values per case)."""
import pytest
import torch

import _accuracy as A
import flash_attn_turing as F
from flash_attn_turing import _C, capi

pytestmark = pytest.mark.gpu

DTS = ["fp16", "bf16"]


def _dev(x, gpu):
    return x.to(gpu) if isinstance(x, torch.Tensor) else x


# ---- decode over a KV cache, MLA and sparse MLA --------------------------------------------------------------------------------------------------

def _decode_call(built, gpu, splits):
    """one call of the case on fresh device copies (the append writes the cache) -> out, lse on the CPU"""
    a = built.args
    kw = {k: _dev(v, gpu) for k, v in a["kw"].items()}
    q = a["q"].to(gpu)
    if built.kind == "kvcache":
        out, lse = F.flash_attn_with_kvcache(q, a["k_cache"].to(gpu), a["v_cache"].to(gpu), num_splits=splits, **kw)
    elif built.kind == "mla":
        out, lse = F.flash_mla_with_kvcache(q, a["kv_cache"].to(gpu), a["cache_seqlens"].to(gpu), num_splits=splits, **kw)
    else:
        out, lse = F.flash_mla_sparse_with_kvcache(q, a["kv_cache"].to(gpu), a["cache_seqlens"].to(gpu), a["indices"].to(gpu), num_splits=splits, **kw)
    assert out.dtype == A.DT[built.dtname] and lse.dtype == torch.float32
    return out.float().cpu(), lse.cpu()


@pytest.mark.parametrize("name", A.DECODE_NAMES)
@pytest.mark.parametrize("dtname", DTS)
def test_decode_families(gpu, dtname, name):
    """one case per attention family (tests/_accuracy.py KVCACHE_CASES, MLA_CASES): key counts 33, 100 and 777 in one batch, the appended rows at
    3 x scale and again at N(0, 1), num_splits 0, 1 and 3"""
    fails = []
    for hot in A.VARIANTS:
        built = A.decode_case(dtname, name, hot)
        base = A.model_of(built)
        for splits in A.SPLITS:
            out, lse = _decode_call(built, gpu, splits)
            x, l = A.flatten_kernel(built, out, lse)
            try:
                A.budget_entries(f"{built.kind} {name} {'hot' if hot else 'flat'} splits={splits} O", dtname, base, x, l)
            except AssertionError as err:
                fails.append(str(err))
    assert not fails, "\n".join(fails)


# ---- fwd, varlen_fwd, bwd, varlen_bwd ------------------------------------------------------------------------------------------------------------

@pytest.fixture(params=["mfma32", "mfma16"])
def pinned_set(request):
    """both pinned kernel sets, as tests/test_attention_edges_gpu.py pins them"""
    prev = capi.set_kernel_policy(capi.POLICY_MFMA16 if request.param == "mfma16" else capi.POLICY_MFMA32)
    yield request.param
    capi.set_kernel_policy(prev)


def _attn_inputs(c, gpu):
    dt = A.DT[c["dtname"]]
    t = {n: torch.from_numpy(c[n]).to(gpu, dt) for n in ("q", "k", "v", "do")}
    if c["packed"]:
        t.update(cu_q=torch.from_numpy(c["cu_q"]).to(gpu), cu_k=torch.from_numpy(c["cu_k"]).to(gpu), mq=max(c["lq"]), mk=max(c["lk"]))
    return t


FWD_PARAMS = [pytest.param(c, p, id=f"{c[0]}-{'packed' if p else 'dense'}") for c in A.ATTN_CASES for p in (False, True) if not (p and c[3] != A.ATTN_SQ)]
BWD_PARAMS = [pytest.param(c, p, id=f"{c[0]}-{'packed' if p else 'dense'}") for c in A.ATTN_CASES for p in (False, True) if c[3] == A.ATTN_SQ]


@pytest.mark.parametrize("case,packed", FWD_PARAMS)
@pytest.mark.parametrize("dtname", DTS)
def test_forward(gpu, dtname, case, packed, pinned_set):
    """fwd and varlen_fwd: sq = sk = 320 (one 256-row workgroup and a tail), h / h_k = 4 / 2, the packed batch with an empty sequence; and 1664
    keys, where the fp16 16x16x32 kernel takes the row sums of keys 1024 .. 1663 from the packed P (the model does the same there)"""
    name, d, causal, sk = case
    c = A.attn_case(dtname, d, causal, sk, packed)
    rowsum = "rounded" if (pinned_set == "mfma16" and dtname == "fp16" and sk > A.PP16_EXACT_KEYS) else "exact"
    base = A.attn_forward_model(c, rowsum)
    t = _attn_inputs(c, gpu)
    if packed:
        out, lse = _C.varlen_fwd(t["q"], t["k"], t["v"], t["cu_q"], t["cu_k"], t["mq"], t["mk"], causal)
    else:
        out, lse = _C.fwd(t["q"], t["k"], t["v"], causal)
    A.budget_entries(f"{'varlen_fwd' if packed else 'fwd'} {name} {pinned_set} O", dtname, base,
                     A.attn_flatten(c, out.float().cpu()), A.attn_flatten(c, lse.cpu(), is_lse=True))


def _capi_backward(c, t, gpu):
    """forward + backward through the C ABI with the head-group workspace attached: the dK / dV launch splits the two query heads of a KV head
    over fp32 planes and sums them"""
    q, k, v, do = t["q"], t["k"], t["v"], t["do"]
    o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    if c["packed"]:
        b, mq, mk = len(c["lq"]), t["mq"], t["mk"]
        lse, dsum = torch.zeros(b, c["h"], mq, device=gpu), torch.zeros(b, c["h"], mq, device=gpu)
        row = lambda x: capi.Strides(0, x.stride(0), x.stride(1))
        common = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(), cu_seqlens_q=t["cu_q"].data_ptr(),
                      cu_seqlens_k=t["cu_k"].data_ptr(), b=b, seqlen_q=mq, seqlen_k=mk, h=c["h"], h_k=c["hk"], d=c["d"], dtype=capi.dtype_code(q.dtype),
                      is_causal=int(c["causal"]), q_stride=row(q), k_stride=row(k), v_stride=row(v), o_stride=row(o), total_q=q.shape[0], total_k=k.shape[0])
        fp = capi.FwdParams(**common)
        bp = capi.BwdParams(dout=do.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), dsoftmax_sum=dsum.data_ptr(),
                            do_stride=row(do), dq_stride=row(dq), dk_stride=row(dk), dv_stride=row(dv), **common)
    else:
        b, sq = q.shape[:2]
        lse, dsum = torch.empty(b, c["h"], sq, device=gpu), torch.empty(b, c["h"], sq, device=gpu)
        fp = capi.fwd_params(q, k, v, o, lse, c["causal"])
        bp = capi.bwd_params(q, k, v, o, lse, do, dq, dk, dv, dsum, c["causal"])
    capi.run_fwd(fp)
    ws = capi.attach_workspace(bp, q)
    assert ws is not None, "the launch must split its head groups through the workspace"
    capi.run_bwd(bp)
    torch.cuda.synchronize()
    return dq, dk, dv


@pytest.mark.parametrize("case,packed", BWD_PARAMS)
@pytest.mark.parametrize("dtname", DTS)
def test_backward(gpu, dtname, case, packed, pinned_set):
    """bwd and varlen_bwd on the forward's shapes: dQ, dK and dV against the C oracle in rounding mode (the model) and torch fp64 autograd (ref64),
    through the host module and through the C ABI with the head-group workspace"""
    name, d, causal, sk = case
    c = A.attn_case(dtname, d, causal, sk, packed)
    t = _attn_inputs(c, gpu)
    q, k, v = (t[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
    if packed:
        out = F.flash_attn_varlen_func(q, k, v, t["cu_q"], t["cu_k"], t["mq"], t["mk"], causal=causal)
    else:
        out = F.flash_attn_func(q, k, v, causal=causal)
    out.backward(t["do"])
    host = (q.grad, k.grad, v.grad)
    fails = []
    for route, grads in (("host", host), ("capi+workspace", _capi_backward(c, t, gpu))):
        for tn, g in zip(("dq", "dk", "dv"), grads):
            x, _ = A.attn_grad_rows(c, tn, g.detach().float().cpu())
            try:
                A.budget_entries(f"{'varlen_bwd' if packed else 'bwd'} {name} {pinned_set} {route} {tn}", dtname, A.attn_grad_base(c, tn), x)
            except AssertionError as err:
                fails.append(str(err))
    assert not fails, "\n".join(fails)
