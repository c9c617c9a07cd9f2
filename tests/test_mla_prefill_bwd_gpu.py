"""GPU: the MLA prefill backward (flash_mla_prefill_bwd / flash_mla_attn_func / fa_run_mla_prefill_bwd; fa_bwd_mla_prefill.hip) - values against the
fp64 autograd expectation of tests/_mla_prefill_bwd_cases.py, the accuracy budget against the rounding model, the exact set of (row, key) pairs, the
relations stated to the bit, the guards, graph capture, the adversarial-timing builds, and one speed relation."""
import ctypes
import statistics

import numpy as np
import pytest
import torch

import _accuracy as A
import _mla_prefill_bwd_cases as B
import _mla_prefill_cases as C
import _util as U
import _visibility as V

pytestmark = pytest.mark.gpu

NAN = float("nan")
NAMES = ("dQ", "dK", "dV")


def _F():
    import flash_attn_turing as F

    return F


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(U.bits(a.contiguous()), U.bits(b.contiguous()))


def _same3(a, b):
    return all(_same(x, y) for x, y in zip(a, b))


def _fwd(q, k, v, **kw):
    with torch.no_grad():
        return _F().flash_mla_prefill_func(q, k, v, return_softmax_lse=True, **kw)


def _raw(dout, q, k, v, **kw):
    """forward, then the raw backward"""
    out, lse = _fwd(q, k, v, **kw)
    return _F().flash_mla_prefill_bwd(dout, q, k, v, out, lse, **kw)


def _autograd(dout, q, k, v, **kw):
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    _F().flash_mla_attn_func(q, k, v, **kw).backward(dout)
    return q.grad, k.grad, v.grad


def _check_sequence(grads, want, dtname, tag, sq, sk, g):
    """dq (sq, h, 192), dk (sk, hk, 192), dv (sk, hk, 128) of one sequence against the fp64 expectation, within _util.TOL (the forward's value tolerance)"""
    for name, x, w, n in zip(NAMES, grads, want, (sk, sq * g, sq * g)):
        if x.numel():
            U.assert_close(x.float().cpu().numpy(), w.numpy(), dtname, f"mla_prefill_bwd {name} {tag}", sk=n if name == "dQ" else None)


# ---- 1. values --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", B.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_values_dense(gpu, dtname, heads, causal):
    """every shape, through the raw function and through flash_mla_attn_func(...).backward(dout): the same bits, and the fp64 expectation within TOL"""
    h, hk = heads
    for n, (sq, sk) in enumerate(B.SHAPES):
        q, k, v = C.inputs(sq, sk, h, hk, dtname, 1000 + n, b=2)
        dout = B.dout_like(q, 1500 + n)
        dq, dk, dv = _raw(*(t.to(gpu) for t in (dout, q, k, v)), causal=causal)
        assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape and dq.dtype == dk.dtype == dv.dtype == q.dtype
        assert dq.is_contiguous() and dk.is_contiguous() and dv.is_contiguous()
        auto = _autograd(*(t.to(gpu) for t in (dout, q, k, v)), causal=causal)
        assert _same3((dq, dk, dv), auto), f"sq{sq} sk{sk}: the raw function and the autograd node differ"
        for i in range(2):
            want = B.grads64(q[i], k[i], v[i], dout[i], causal)
            _check_sequence((dq[i], dk[i], dv[i]), want, dtname, f"dense sq{sq} sk{sk} h{h}/{hk} {'causal' if causal else 'full'} b{i}", sq, sk, h // hk)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", B.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_values_packed(gpu, dtname, heads, causal):
    """the packed batch of the forward's tests, and every dense shape as the sequences of one more packed call"""
    h, hk = heads
    for sqs, sks in ((B.PACKED_SQ, B.PACKED_SK), tuple(zip(*B.SHAPES))):
        q, k, v, cu_q, cu_k = C.packed_inputs(sqs, sks, h, hk, dtname, 2000 + len(sqs))
        dout = B.dout_like(q, 2500 + len(sqs))
        kw = dict(cu_seqlens_q=cu_q.to(gpu), cu_seqlens_k=cu_k.to(gpu), causal=causal)
        grads = _raw(*(t.to(gpu) for t in (dout, q, k, v)), **kw)
        assert _same3(grads, _autograd(*(t.to(gpu) for t in (dout, q, k, v)), **kw)), "the raw function and the autograd node differ"
        for i in range(len(sqs)):
            a, b, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
            want = B.grads64(q[a:b], k[c:d], v[c:d], dout[a:b], causal)
            _check_sequence((grads[0][a:b], grads[1][c:d], grads[2][c:d]), want, dtname,
                            f"packed seq{i} sq{sqs[i]} sk{sks[i]} h{h}/{hk} {'causal' if causal else 'full'}", sqs[i], sks[i], h // hk)


def test_sum_backward_fills_grad_of_the_leaves(gpu):
    """flash_mla_attn_func(q, k, v, causal=True).sum().backward() on 192 / 192 / 128-wide leaves, dense and packed; lse comes back non-differentiable"""
    F = _F()
    q, k, v = (t.to(gpu).requires_grad_(True) for t in C.inputs(65, 97, 4, 2, "bf16", 1900, b=2))
    out, lse = F.flash_mla_attn_func(q, k, v, causal=True, return_softmax_lse=True)
    assert out.requires_grad and not lse.requires_grad
    out.sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad.float()).all().item() and t.grad.abs().sum().item() > 0 for t in (q, k, v))
    with torch.no_grad():
        assert _same(F.flash_mla_attn_func(q, k, v, causal=True), F.flash_mla_prefill_func(q, k, v, causal=True))
    q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(C.PACKED_SQ, C.PACKED_SK, 6, 2, "fp16", 1901))
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    F.flash_mla_attn_func(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=True).sum().backward()
    assert all(t.grad is not None and t.grad.shape == t.shape and torch.isfinite(t.grad.float()).all().item() for t in (q, k, v))
    # a dout the kernels cannot address (a last dimension that is not contiguous) is made contiguous once: the same bits
    q2, k2, v2 = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o2 = F.flash_mla_attn_func(q2, k2, v2, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=True)
    o2.backward(torch.ones(C.DV, o2.shape[1], o2.shape[0], dtype=o2.dtype, device=gpu).permute(2, 1, 0))
    assert _same3((q.grad, k.grad, v.grad), (q2.grad, k2.grad, v2.grad))


def test_backward_through_a_sum_over_the_sequence_axis(gpu):
    """(f(q, k, v).sum(dim=1) * w).sum().backward(): autograd hands the node an EXPANDED dout (row stride 0), which no kernel addresses; the node makes it
    contiguous once and gives the gradients of the contiguous dout, and the raw function refuses such a dout with a ValueError that names it"""
    F = _F()
    for packed in (False, True):
        if packed:
            q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(C.PACKED_SQ, C.PACKED_SK, 6, 2, "bf16", 1950))
            kw = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=True)
            axis, w = 0, torch.randn(6, C.DV, device=gpu).to(q.dtype)
        else:
            q, k, v = (t.to(gpu) for t in C.inputs(65, 97, 4, 2, "bf16", 1951, b=2))
            kw = dict(causal=True)
            axis, w = 1, torch.randn(2, 4, C.DV, device=gpu).to(q.dtype)
        seen = []
        ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
        out = F.flash_mla_attn_func(ql, kl, vl, **kw)
        out.register_hook(lambda g: seen.append(tuple(g.stride())))
        (out.sum(dim=axis) * w).sum().backward()
        assert seen and seen[0][-3] == 0, f"the case does not deliver an expanded dout any more: strides {seen}"
        dout = w.unsqueeze(axis).expand(out.shape)
        assert dout.stride(-3) == 0
        want = _raw(dout.contiguous(), q, k, v, **kw)
        assert _same3((ql.grad, kl.grad, vl.grad), want), "the expanded dout gives other gradients than its contiguous copy"
        o, lse = _fwd(q, k, v, **kw)
        with pytest.raises(ValueError, match="dout"):
            F.flash_mla_prefill_bwd(dout, q, k, v, o, lse, **kw)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_query_rows_but_no_key_anywhere(gpu, dtname, causal):
    """dense (sq, 0) and packed with total_k = 0: every row is dead, dQ comes back exactly 0 over NaN-filled buffers (C ABI, with k / v / dk / dv NULL), and
    the Python functions return dk / dv without rows"""
    from flash_attn_turing import capi

    dt, h, hk, sq = C.DT[dtname], 6, 2, 70
    F = _F()
    for packed in (False, True):
        shape_q = (2 * sq, h) if packed else (2, sq, h)
        shape_k = (0, hk) if packed else (2, 0, hk)
        q = torch.randn(shape_q + (C.DQK,), device=gpu).to(dt)
        k, v = torch.empty(shape_k + (C.DQK,), dtype=dt, device=gpu), torch.empty(shape_k + (C.DV,), dtype=dt, device=gpu)
        dout = torch.randn(shape_q + (C.DV,), device=gpu).to(dt)
        kw = dict(cu_seqlens_q=C.cu((sq, sq), gpu), cu_seqlens_k=C.cu((0, 0), gpu), causal=causal) if packed else dict(causal=causal)
        out, lse = _fwd(q, k, v, **kw)
        assert (out == 0).all().item() and (lse == 0).all().item()
        dq, dk, dv = F.flash_mla_prefill_bwd(dout, q, k, v, out, lse, **kw)
        assert dq.shape == q.shape and (U.bits(dq) == 0).all().item() and dk.shape == k.shape and dv.shape == v.shape
        assert _same3((dq, dk, dv), _autograd(dout, q, k, v, **kw))
        dq2, dsum = torch.full(q.shape, NAN, dtype=dt, device=gpu), torch.full(lse.shape, NAN, device=gpu)
        p = capi.mla_prefill_bwd_params(dout, q, k, v, out, lse, dq2, k, v, dsum, kw.get("cu_seqlens_q"), kw.get("cu_seqlens_k"), causal, None)
        p.k = p.v = p.dk = p.dv = None
        capi.run_mla_prefill_bwd(p)
        torch.cuda.synchronize()
        assert (U.bits(dq2) == 0).all().item() and (dsum == 0).all().item(), "dQ (and D) of rows without any key must be written as exact zeros"


# ---- 2. the accuracy budget -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_accuracy_budget(gpu, dtname, causal):
    """ordinary data, b 2, h 8 = h_k, sq = sk = 777 (the forward's budget case) with dout ~ N(0, 1): per output tensor |gain| <= G and relative RMS <= 1.25 x
    the rounding model's on the same inputs (tests/_accuracy.py: budget_check), against the unrounded fp64 expectation.  One length class: the pooled
    statistic is the class's.  One line per tensor is printed (profiles/mla_prefill_bwd_accuracy.log is the run recorded with the change)."""
    b, h, s = 2, 8, 777
    q, k, v = C.inputs(s, s, h, h, dtname, 3000, b=b)
    dout = B.dout_like(q, 3001)
    model, exact = B.rounding_model(q, k, v, dout, causal, dtname)
    grads = _raw(*(t.to(gpu) for t in (dout, q, k, v)), causal=causal)
    fails = []
    for name, x, m, e in zip(NAMES, grads, model, exact):
        try:
            A.budget_check(f"mla_prefill_bwd {name} {'causal' if causal else 'full'} b{b} h{h} s{s}", dtname, x, m, e)       # (prints its line)
        except AssertionError as err:
            fails.append(str(err))
    assert not fails, "\n".join(fails)


# ---- 3. the exact (row, key) pairs ------------------------------------------------------------------------------------------------------------
# The probe of tests/test_attention_backward_visibility_gpu.py (tests/_visibility.py, "THE BACKWARD PROBE") at widths 192 / 128: lse = 0, out = 0 and all
# scores exactly 0 make P exactly 1 on the pairs the kernels treat as visible; V = 1 and dO_t = code(t) make dP = 2; softmax_scale = 2^-4 keeps every
# product exact, so every comparison is a bit equality.  Call A (Q = 0, K_j = code(j)): dQ_t = scale x 2 x hist_keys(t), dV_j = g x hist_rows(j), dK = 0.
# Call B (K = 0, Q_t = code(t)): dK_j = scale x 2 x g x hist_rows(j), dV as in A, dQ = 0.  The code sits on the first 64 columns; every other column is 0.
# All heads are hot: the largest integer is 2 x 4 x 32 = 256, exact in bf16 (asserted).

PROBE_SCALE = 2.0 ** -4
PROBE_SHAPES = tuple(s for s in B.SHAPES if max(s) <= V.BWD_CAP) + ((257, 1023), (1000, 300))


def _probe(gpu, dtname, sqs, sks, h, hk, causal, packed):
    from flash_attn_turing import capi

    dt, g = C.DT[dtname], h // hk
    code = torch.from_numpy(V.bwd_code(64).copy())
    pad = lambda x, w: torch.nn.functional.pad(x, (0, w - x.shape[-1]))
    hists = [V._seq_hists(L, s, causal, 64) for L, s in zip(sks, sqs)]
    hkeys = torch.from_numpy(np.concatenate([x[0] for x in hists]))                # (Rq, 64)
    hrows = torch.from_numpy(np.concatenate([x[1] for x in hists]))                # (Rk, 64)
    assert 2 * g * int(hrows.numpy().max(initial=0)) <= V.BWD_INT_EXACT[dtname] and 2 * int(hkeys.numpy().max(initial=0)) <= V.BWD_INT_EXACT[dtname]
    rq = torch.cat([torch.arange(s) for s in sqs])
    rk = torch.cat([torch.arange(L) for L in sks] + [torch.zeros(0, dtype=torch.long)])
    tq, tk, extra = len(rq), len(rk), 3
    b = 1 if packed else 2
    qshape, kshape = ((tq + extra, h), (tk + extra, hk)) if packed else ((b, tq + extra, h), (b, tk + extra, hk))

    def tensor(shape, w, rows, n):
        """the rows' values in front, poisoned rows behind (dense: behind every batch entry)"""
        t = U.poison_(torch.empty(shape + (w,), dtype=dt, device=gpu))
        t[..., :n, :, :] = rows.to(gpu, dt).unsqueeze(-2)
        return t

    qcode, kcode, docode = pad(code[rq], C.DQK).double(), pad(code[rk], C.DQK).double(), pad(code[rq], C.DV).double()
    cu_q, cu_k = (C.cu(sqs, gpu), C.cu(sks, gpu)) if packed else (None, None)
    for call in "AB":
        qb = tensor(qshape, C.DQK, qcode if call == "B" else torch.zeros_like(qcode), tq)
        kb = tensor(kshape, C.DQK, kcode if call == "A" else torch.zeros_like(kcode), tk)
        vb = tensor(kshape, C.DV, torch.ones(tk, C.DV), tk)
        dob = tensor(qshape, C.DV, docode, tq)
        ob = tensor(qshape, C.DV, torch.zeros(tq, C.DV), tq)
        sl = (lambda t, n: t) if packed else (lambda t, n: t[:, :n])       # packed: the poisoned rows stay in the tensors, past cu_seqlens[-1]
        q, k, v, do, o = sl(qb, tq), sl(kb, tk), sl(vb, tk), sl(dob, tq), sl(ob, tq)
        lse = torch.full((h, tq + extra) if packed else (b, h, tq), NAN, device=gpu)
        if packed:
            lse[:, :tq] = 0
        else:
            lse.zero_()
        dq, dk, dv = (torch.full(t.shape, NAN, dtype=dt, device=gpu) for t in (q, k, v))
        dsum = torch.full(lse.shape, NAN, device=gpu)
        p = capi.mla_prefill_bwd_params(do, q, k, v, o, lse, dq, dk, dv, dsum, cu_q, cu_k, causal, PROBE_SCALE)
        capi.run_mla_prefill_bwd(p)
        torch.cuda.synchronize()
        want_dq = pad(hkeys * 2, C.DQK).double() * PROBE_SCALE if call == "A" else torch.zeros(tq, C.DQK).double()
        want_dk = pad(hrows * 2 * g, C.DQK).double() * PROBE_SCALE if call == "B" else torch.zeros(tk, C.DQK).double()
        # dV_j = sum_t P_tj dO_t: the digit histogram of the rows that see key j on the code's 64 columns, 0 on the others
        want_dv = pad(hrows * g, C.DV).double()
        tag = f"{dtname} {'packed' if packed else 'dense'} sq{sqs} sk{sks} h{h}/{hk} {'causal' if causal else 'full'} call {call}"
        for name, x, w, n in zip(NAMES, (dq, dk, dv), (want_dq, want_dk, want_dv), (tq, tk, tk)):
            w = w.to(gpu, dt).unsqueeze(-2).expand(n, x.shape[-2], x.shape[-1])
            for i in range(b):
                got = x[:n] if packed else x[i]
                bad = (U.bits(got.contiguous()) != U.bits(w.contiguous())).any(-1)
                assert not bad.any().item(), f"{tag}: {name} differs from the model at (row or key, head) {bad.nonzero()[:6].tolist()} (batch entry {i})"
            if packed:
                assert torch.isnan(x[n:].float()).all().item(), f"{tag}: rows of {name} past cu_seqlens[-1] were written"
        if packed:
            assert torch.isnan(dsum[:, tq:]).all().item(), f"{tag}: D past cu_seqlens_q[-1] was written"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_row_key_pairs_dense(gpu, dtname, causal):
    """every shape (sq > sk under causal: dead rows, exactly 0; (1000, 300): keys that few rows see), h / h_k rotating through HEADS"""
    for n, (sq, sk) in enumerate(PROBE_SHAPES):
        h, hk = B.HEADS[(n + C.DTYPES.index(dtname)) % 3]
        _probe(gpu, dtname, (sq,), (sk,), h, hk, causal, packed=False)


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", B.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_row_key_pairs_packed(gpu, dtname, heads, causal):
    """the packed batch (an empty query sequence, an empty key sequence, more rows than keys) and one of larger sequences; poisoned rows past cu_seqlens[-1]"""
    h, hk = heads
    _probe(gpu, dtname, B.PACKED_SQ, B.PACKED_SK, h, hk, causal, packed=True)
    _probe(gpu, dtname, (150, 0, 200, 70), (100, 40, 520, 0), h, hk, causal, packed=True)


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_packed_sequence_equals_the_dense_call_on_it_alone(gpu, dtname, causal):
    h, hk = 6, 2
    sqs, sks = B.PACKED_SQ + (200, 150), B.PACKED_SK + (1040, 100)
    q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sqs, sks, h, hk, dtname, 4000))
    dout = B.dout_like(q, 4001).to(gpu)
    kw = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)
    grads = _raw(dout, q, k, v, **kw)
    assert _same3(grads, _raw(dout, q, k, v, **kw)), "two runs differ"
    for i in range(len(sqs)):
        a, b, c, d = int(cu_q[i]), int(cu_q[i + 1]), int(cu_k[i]), int(cu_k[i + 1])
        one = _raw(dout[a:b].unsqueeze(0), q[a:b].unsqueeze(0), k[c:d].unsqueeze(0), v[c:d].unsqueeze(0), causal=causal)
        assert _same3((grads[0][a:b], grads[1][c:d], grads[2][c:d]), tuple(t[0] for t in one)), \
            f"sequence {i} (sq {sqs[i]}, sk {sks[i]}) of the packed call differs from the dense call on it alone"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_dense_bits(gpu, dtname, causal):
    """a batch entry == the call on it alone; two runs"""
    q, k, v = (t.to(gpu) for t in C.inputs(130, 131, 6, 2, dtname, 4100, b=3))
    dout = B.dout_like(q, 4101).to(gpu)
    grads = _raw(dout, q, k, v, causal=causal)
    assert _same3(grads, _raw(dout, q, k, v, causal=causal)), "two runs differ"
    for i in range(3):
        one = _raw(dout[i:i + 1], q[i:i + 1], k[i:i + 1], v[i:i + 1], causal=causal)
        assert _same3(tuple(t[i] for t in grads), tuple(t[0] for t in one)), f"batch entry {i} differs from the call on it alone"


@pytest.mark.parametrize("dtname", C.DTYPES)
def test_q_k_v_dout_sliced_from_fused_buffers(gpu, dtname):
    b, s, h = 2, 130, 4
    q, k, v = (t.to(gpu) for t in C.inputs(s, s, h, h, dtname, 5300, b=b))
    dout = B.dout_like(q, 5301).to(gpu)
    out, lse = _fwd(q, k, v, causal=True)
    fused = torch.cat([q, k, v, dout, out], dim=-1)                 # (b, s, h, 768): head stride 768, offsets 0 / 192 / 384 / 512 / 640
    fq, fk, fv, fdo, fo = fused[..., :192], fused[..., 192:384], fused[..., 384:512], fused[..., 512:640], fused[..., 640:]
    assert not fq.is_contiguous() and fdo.storage_offset() == 512 and fv.stride(2) == 768
    want = _F().flash_mla_prefill_bwd(dout, q, k, v, out, lse, causal=True)
    got = _F().flash_mla_prefill_bwd(fdo, fq, fk, fv, fo, lse, causal=True)
    assert _same3(want, got)
    assert _same3(want, _autograd(fdo, fq, fk, fv, causal=True))


# ---- 5. guards --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_guard_buffers_dense(gpu, dtname, causal):
    """every input a view into a poisoned buffer, dq / dk / dv views into sentinel buffers (C ABI): the contiguous call's bits, and no byte outside the views changes"""
    from flash_attn_turing import capi

    dt = C.DT[dtname]
    b, sq, sk, h, hk = 2, 65, 97, 6, 2
    q, k, v = (t.to(gpu) for t in C.inputs(sq, sk, h, hk, dtname, 5000, b=b))
    dout = B.dout_like(q, 5001).to(gpu)
    out, lse = _fwd(q, k, v, causal=causal)
    want = _F().flash_mla_prefill_bwd(dout, q, k, v, out, lse, causal=causal)
    views = []
    for t in (dout, q, k, v, out):
        _, view, _ = U.guarded(tuple(t.shape), dt, gpu, (2, 4, 2, 16), fill=None)
        view.copy_(t)
        views.append(view)
    assert _same3(want, _F().flash_mla_prefill_bwd(*views, lse, causal=causal)), "gaps of strided views reached a result"
    outs = [U.guarded(tuple(t.shape), dt, gpu, (2, 4, 2, 16)) for t in (q, k, v)]
    dsum = torch.full(lse.shape, NAN, device=gpu)
    p = capi.mla_prefill_bwd_params(*views, lse, *(o[1] for o in outs), dsum, None, None, causal, None)
    capi.run_mla_prefill_bwd(p)
    torch.cuda.synchronize()
    assert _same3(want, tuple(o[1] for o in outs))
    for name, (buf, _, sl) in zip(NAMES, outs):
        mask = torch.ones(buf.shape, dtype=torch.bool, device=gpu)
        mask[sl] = False
        assert (U.bits(buf)[mask] == U.SENT16).all().item(), f"a byte of {name}'s buffer outside the view was written"


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_guard_rows_packed(gpu, dtname, causal):
    """packed: poisoned rows of every input past cu_seqlens[-1] change nothing; rows of dq / dk / dv past cu_seqlens[-1] keep their sentinel (C ABI)"""
    from flash_attn_turing import capi

    dt = C.DT[dtname]
    h, hk, extra = 4, 1, 5
    sqs, sks = B.PACKED_SQ, B.PACKED_SK
    q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sqs, sks, h, hk, dtname, 5100))
    dout = B.dout_like(q, 5101).to(gpu)
    kw = dict(cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)
    out, lse = _fwd(q, k, v, **kw)
    want = _F().flash_mla_prefill_bwd(dout, q, k, v, out, lse, **kw)
    tq, tk = sum(sqs), sum(sks)
    bufs = [U.poison_(torch.empty((t.shape[0] + extra,) + tuple(t.shape[1:]), dtype=dt, device=gpu)) for t in (dout, q, k, v, out)]
    for buf, t in zip(bufs, (dout, q, k, v, out)):
        buf[: t.shape[0]] = t
    lse_b = torch.full((h, tq + extra), NAN, device=gpu)
    lse_b[:, :tq] = lse
    outs = [torch.full(t.shape, U.SENT16, dtype=torch.int16, device=gpu).view(dt) for t in bufs[1:4]]
    dsum = torch.full(lse_b.shape, NAN, device=gpu)
    capi.run_mla_prefill_bwd(capi.mla_prefill_bwd_params(*bufs, lse_b, *outs, dsum, cu_q, cu_k, causal, None))
    torch.cuda.synchronize()
    for name, x, w, n in zip(NAMES, outs, want, (tq, tk, tk)):
        assert _same(x[:n], w), f"{name}: rows past cu_seqlens reached a result"
        assert (U.bits(x[n:]) == U.SENT16).all().item(), f"rows of {name} past cu_seqlens[-1] were written"
    assert _same3(want, tuple(t[:n] for t, n in zip(_F().flash_mla_prefill_bwd(*bufs, lse_b, **kw), (tq, tk, tk))))


# ---- 6. graph capture -------------------------------------------------------------------------------------------------------------------------

def test_graph_replay_follows_new_cu_seqlens(gpu):
    """forward plus backward in one capture, one replay: cu_seqlens rewritten in place (same totals), compared with the eager calls on the new lengths"""
    h, hk = 6, 2
    sq_a, sk_a, sq_b, sk_b = (64, 0, 130, 18), (97, 33, 131, 5), (1, 17, 64, 130), (0, 5, 130, 131)
    assert sum(sq_a) == sum(sq_b) and sum(sk_a) == sum(sk_b)
    q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sq_a, sk_a, h, hk, "bf16", 6000))
    dout = B.dout_like(q, 6001).to(gpu)
    call = lambda: _raw(dout, q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = call()
    cu_q.copy_(C.cu(sq_b, gpu)), cu_k.copy_(C.cu(sk_b, gpu))
    g.replay()
    torch.cuda.synchronize()
    assert _same3(got, call()), "the replay did not follow the rewritten cu_seqlens"
    want = B.packed_grads64(q.cpu(), k.cpu(), v.cpu(), dout.cpu(), cu_q.cpu(), cu_k.cpu(), True)
    for name, x, w in zip(NAMES, got, want):
        U.assert_close(x.float().cpu().numpy(), w.numpy(), "bf16", f"mla_prefill_bwd graph replay {name}")


# ---- 7. the adversarial-timing builds ---------------------------------------------------------------------------------------------------------

TIMING = ("stage_slow_reader", "stage_slow_writer")
RACY = "stage_racy_slow_writer"
STEP_LENS = (0, 20, 40, 90, 128, 131, 1040)         # rows or keys of a sequence: 0, 1, 2, 3, 4, 5 and 33 steps of 32 on the walked axis


@pytest.fixture(scope="module")
def libs(gpu):
    from flash_attn_turing import capi
    from test_stage_protocol_gpu import _build_module

    fa_build = _build_module()
    fa_build.build_debug_variants(force=False)          # a no-op when build() has run (the .so files travel with the tree)
    out = {"product": capi.lib()}
    for name in TIMING + (RACY,):
        L = ctypes.CDLL(fa_build.debug_library_path(name))
        L.fa_run_mla_prefill_bwd.argtypes = [ctypes.POINTER(capi.MlaPrefillBwdParams), ctypes.c_void_p]
        L.fa_run_mla_prefill_bwd.restype = ctypes.c_int
        L.fa_last_error.restype = ctypes.c_char_p
        out[name] = L
    return out


def _timing_case(gpu, dtname, causal, packed, walked):
    """walked = "keys": the dQ kernel's axis takes STEP_LENS (70 query rows a sequence); "rows": the dK/dV kernel's does (h / h_k = 1: STEP_LENS query rows against
    70 keys).  dense: 33 steps on that axis.  out / lse are the product's forward; every output and D are prefilled with NaN."""
    from flash_attn_turing import capi

    dt = C.DT[dtname]
    h, hk = (4, 2) if walked == "keys" else (2, 2)
    n = len(STEP_LENS)
    sqs, sks = ((70,) * n, STEP_LENS) if walked == "keys" else (STEP_LENS, (70,) * n)
    if packed:
        q, k, v, cu_q, cu_k = (t.to(gpu) for t in C.packed_inputs(sqs, sks, h, hk, dtname, 7000))
    else:
        q, k, v = (t.to(gpu) for t in C.inputs(max(sqs), max(sks), h, hk, dtname, 7001, b=2))
        cu_q = cu_k = None
    dout = B.dout_like(q, 7002).to(gpu)
    out, lse = _fwd(q, k, v, cu_seqlens_q=cu_q, cu_seqlens_k=cu_k, causal=causal)

    def run(L):
        dq, dk, dv = (torch.full(t.shape, NAN, dtype=dt, device=gpu) for t in (q, k, v))
        dsum = torch.full(lse.shape, NAN, device=gpu)
        p = capi.mla_prefill_bwd_params(dout, q, k, v, out, lse, dq, dk, dv, dsum, cu_q, cu_k, causal, None)
        rc = L.fa_run_mla_prefill_bwd(ctypes.byref(p), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, L.fa_last_error().decode()
        torch.cuda.synchronize()
        return (dq, dk, dv) if walked == "keys" else (dk, dv, dq)

    return run


@pytest.mark.parametrize("walked", ["keys", "rows"])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_timing_builds_reproduce_the_product(gpu, libs, dtname, causal, packed, walked):
    """the slow-reader and slow-writer builds, twice each, give the product's dq / dk / dv bits: 0, 1, 2, 3, 4, 5 and 33 steps on the walked axis of each kernel
    in one packed call, and a dense call of 33 steps"""
    from test_stage_protocol_gpu import _must_match

    want = _must_match(libs, _timing_case(gpu, dtname, causal, packed, walked), f"mla_prefill_bwd {dtname} {'causal' if causal else 'full'} {'packed' if packed else 'dense'} {walked}")
    assert all(torch.isfinite(t.float()).all().item() for t in want)


@pytest.mark.parametrize("walked", ["keys", "rows"])
@pytest.mark.parametrize("dtname", C.DTYPES)
def test_racy_form_is_exposed_by_the_slow_writer(gpu, libs, dtname, walked):
    """per kernel: "keys" compares dq alone (the dQ kernel's loop), "rows" dk and dv (the dK/dV kernel's), so neither loop can hide behind the other"""
    from test_stage_protocol_gpu import _must_differ

    run = _timing_case(gpu, dtname, False, False, walked)
    n = 1 if walked == "keys" else 2               # dq alone, or dk and dv: only the outputs of the kernel whose axis is walked are compared
    _must_differ(libs, lambda L: run(L)[:n], dtname, f"mla_prefill_bwd {dtname} dense {walked}")


# ---- 8. one speed relation --------------------------------------------------------------------------------------------------------------------

def torch_formulation(q, k, v, causal, scale=C.SCALE):
    """what a user had before: einsum, masked softmax, einsum in the inputs' dtype (h = h_k), differentiable"""
    s = torch.einsum("bthd,bjhd->bhtj", q, k) * scale
    if causal:
        sq, sk = q.shape[1], k.shape[1]
        s = s.masked_fill(~C.causal_mask(sq, sk).to(q.device), float("-inf"))
    return torch.einsum("bhtj,bjhd->bthd", torch.softmax(s, dim=-1), v)


def test_faster_than_autograd_of_the_torch_formulation(gpu):
    """b 1, sq = sk = 1024, h = h_k = 16, bf16, causal: the median of 5 interleaved rounds of the two raw launches of the new backward must lie below that of
    autograd's backward of the explicit torch formulation in bf16 on the same tensors.  The bound is 1.0 and carries no margin; the ratio is printed and
    recorded (profiles/mla_prefill_bwd_bench.log holds the run recorded with the change)."""
    F = _F()
    b, s, h = 1, 1024, 16
    q, k, v = (t.to(gpu) for t in C.inputs(s, s, h, h, "bf16", 8000, b=b))
    dout = B.dout_like(q, 8001).to(gpu)
    out, lse = _fwd(q, k, v, causal=True)
    new = lambda: F.flash_mla_prefill_bwd(dout, q, k, v, out, lse, causal=True)
    ql, kl, vl = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o_t = torch_formulation(ql, kl, vl, True)
    old = lambda: torch.autograd.grad(o_t, (ql, kl, vl), dout, retain_graph=True)
    for name, x, w in zip(NAMES, new(), old()):
        rel = float((x.double() - w.double()).norm() / w.double().norm())
        assert rel <= 0.05, (name, rel)              # (the same gradients; the yardstick rounds its softmax to bf16, so no more than that is asked)
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
    line = f"test_faster_than_torch_autograd: b{b} sq{s} sk{s} h{h}/{h} bf16 causal: flash_mla_prefill_bwd {n:.4f} ms, autograd of the torch formulation {w:.4f} ms, ratio {n / w:.3f}"
    print(line)
    assert n < w, line
