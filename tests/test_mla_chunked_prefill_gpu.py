"""GPU: flash_mla_chunked_prefill_func - the context part, the causal part over the chunk's own keys and their merge - against flash_mla_prefill_func over
the concatenated keys with causal=True.  Both sides are measured against the fp64 expectation of tests/_mla_prefill_cases.py with the forward suite's own
check (tests/_util.py assert_close, which is tighter than that bound plus 2^-p max_i |o_i| for the rounding of the parts); lse within 2^-20 max(|lse|, 1) of fp64.
h 4, sq 5 and 37, context 0, 16 and 70 keys, both dtypes; the packed batch has a sequence without context and one without query rows."""
import numpy as np
import pytest
import torch

import _merge_cases as M
import _mla_prefill_cases as C
import _util as U

pytestmark = pytest.mark.gpu

H, HK = 4, 2
SQS = (5, 37)
CTXS = (0, 16, 70)
PACKED_SQ = (5, 0, 37, 9)
PACKED_CTX = (16, 33, 0, 70)


def _F():
    import flash_attn_turing as F

    return F


def check_sequence(tag, dtname, out, lse, ref_out, ref_lse, q, k_ctx, v_ctx, k_new, v_new):
    """one sequence: the chunked call (out, lse) and the call over the concatenated keys (ref_out, ref_lse), each against fp64"""
    sq = q.shape[0]
    if sq == 0:
        return 0.0, 0.0
    k, v = torch.cat((k_ctx, k_new), 0), torch.cat((v_ctx, v_new), 0)
    o64, l64 = C.model(q.cpu(), k.cpu(), v.cpu(), True)
    for side, o, l in (("chunked", out, lse), ("concatenated", ref_out, ref_lse)):
        U.assert_close(o.float().cpu().numpy(), o64.numpy(), dtname, f"mla_chunked_prefill O {side} {tag}", sk=k.shape[0])
    bound = M.lse_bound(l64.numpy())
    worst = []
    for side, l in (("chunked", lse), ("concatenated", ref_lse)):
        err = np.abs(l.double().cpu().numpy() - l64.numpy())
        worst.append(float((err / bound).max()))
    print(f"mla_chunked_prefill LSE {tag}: worst err / (2^-20 max(|lse|, 1)) chunked {worst[0]:.3f}, concatenated {worst[1]:.3f}")
    return worst[0], worst[1]


@pytest.mark.parametrize("dtname", C.DTYPES)
def test_dense(gpu, dtname):
    """LSE figures measured on the run recorded with the change: see the assertion's message and README.md"""
    F = _F()
    worst = [0.0, 0.0]
    for sq in SQS:
        for ctx in CTXS:
            q, k_new, v_new = (t.to(gpu) for t in C.inputs(sq, sq, H, HK, dtname, 10 * sq + ctx, b=2))
            _, k_ctx, v_ctx = (t.to(gpu) for t in C.inputs(1, ctx, H, HK, dtname, 10 * sq + ctx + 1, b=2))
            out, lse = F.flash_mla_chunked_prefill_func(q, k_ctx, v_ctx, k_new, v_new, return_softmax_lse=True)
            assert out.shape == (2, sq, H, C.DV) and out.dtype == q.dtype and lse.shape == (2, H, sq) and lse.dtype == torch.float32
            assert torch.equal(U.bits(F.flash_mla_chunked_prefill_func(q, k_ctx, v_ctx, k_new, v_new)), U.bits(out))
            ref, ref_lse = F.flash_mla_prefill_func(q, torch.cat((k_ctx, k_new), 1), torch.cat((v_ctx, v_new), 1), causal=True, return_softmax_lse=True)
            if ctx == 0:
                # no context at all: every row of the first part is dead, and the merge hands back the second part bit for bit
                assert torch.equal(U.bits(out), U.bits(ref)) and torch.equal(U.bits(lse), U.bits(ref_lse)), (sq, "context 0 must be the causal call itself")
            for i in range(2):
                w = check_sequence(f"dense {dtname} sq{sq} ctx{ctx} b{i}", dtname, out[i], lse[i], ref[i], ref_lse[i], q[i], k_ctx[i], v_ctx[i], k_new[i], v_new[i])
                worst = [max(a, b_) for a, b_ in zip(worst, w)]
    assert worst[0] <= 1.0, f"lse of the chunked call: worst err {worst[0]:.3f} x the bound 2^-20 max(|lse|, 1) (the call over the concatenated keys: {worst[1]:.3f} x)"


@pytest.mark.parametrize("dtname", C.DTYPES)
def test_packed(gpu, dtname):
    F = _F()
    gen_seed = 900
    q, k_new, v_new, cu_q, _ = (t.to(gpu) for t in C.packed_inputs(PACKED_SQ, PACKED_SQ, H, HK, dtname, gen_seed))
    _, k_ctx, v_ctx, _, cu_c = (t.to(gpu) for t in C.packed_inputs((1,) * len(PACKED_CTX), PACKED_CTX, H, HK, dtname, gen_seed + 1))
    out, lse = F.flash_mla_chunked_prefill_func(q, k_ctx, v_ctx, k_new, v_new, cu_seqlens_q=cu_q, cu_seqlens_k_ctx=cu_c, return_softmax_lse=True)
    total = sum(PACKED_SQ)
    assert out.shape == (total, H, C.DV) and lse.shape == (H, total)
    # the reference: every sequence's context and chunk keys concatenated, packed
    ks, vs = [], []
    for i in range(len(PACKED_SQ)):
        a, b_, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_c[i]), int(cu_c[i + 1])
        ks += [k_ctx[c:d], k_new[a:b_]]
        vs += [v_ctx[c:d], v_new[a:b_]]
    cu_k = C.cu([s + c for s, c in zip(PACKED_SQ, PACKED_CTX)], device=gpu)
    ref, ref_lse = F.flash_mla_prefill_func(q, torch.cat(ks, 0), torch.cat(vs, 0), cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=True, return_softmax_lse=True)
    worst = [0.0, 0.0]
    for i in range(len(PACKED_SQ)):
        a, b_, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_c[i]), int(cu_c[i + 1])
        w = check_sequence(f"packed {dtname} seq{i} sq{PACKED_SQ[i]} ctx{PACKED_CTX[i]}", dtname, out[a:b_], lse[:, a:b_], ref[a:b_], ref_lse[:, a:b_], q[a:b_], k_ctx[c:d],
                           v_ctx[c:d], k_new[a:b_], v_new[a:b_])
        worst = [max(x, y) for x, y in zip(worst, w)]
        if PACKED_CTX[i] == 0:
            assert torch.equal(U.bits(out[a:b_]), U.bits(ref[a:b_])) and torch.equal(U.bits(lse[:, a:b_].contiguous()), U.bits(ref_lse[:, a:b_].contiguous())), i
    assert worst[0] <= 1.0, f"lse of the chunked call: worst err {worst[0]:.3f} x the bound 2^-20 max(|lse|, 1) (the call over the concatenated keys: {worst[1]:.3f} x)"
