"""GPU: the exact (query row, key) pairs of bwd / varlen_bwd, under both pinned kernel sets.

The backward probe of tests/_visibility.py on the dQ and dK / dV kernels (fa_bwd.hip, fa_bwd_dq16.hip, fa_bwd_dkdv16.hip,
fa_bwd_dkdv_common.hpp): the raw entry points take O and LSE as arguments, and with lse = 0, o = 0 and every score exactly 0 the
kernels' P is exactly 1 on every pair they treat as visible and 0 elsewhere.  V = 1 and dO_t = code(t) make dP = 2, so call A (Q = 0,
K_j = code(j)) returns dQ_t = scale x 2 x the digit histogram of the keys row t sees and dV_j = the histogram of the rows that see key
j, summed over the group's hot query heads, with dK = 0; call B (K = 0, Q_t = code(t)) returns dK_j = scale x 2 x that sum, the same
dV and dQ = 0.  Every assertion is an integer equality with the model (`_visibility.visible` and its transpose `rows_seeing`) on every
(sequence, head, row or key, column), and a bit equality where the scale is a power of two (d = 64, and dV at every d).  Dead rows
(causal with sq > sk), keys nobody sees and empty sequences on either side come back exactly 0.

Three rows of the bad code (1 in every column) sit behind every q / dO / k / v view, the padded entries of a packed LSE and the floats
behind a dense LSE handed to the C ABI hold NaN, and the C ABI's outputs (and its workspace) start as NaN: a read of any of them, or an
element left unwritten, shows in a gradient.

Routes: the host module (which attaches the workspace the library asks for), and the C ABI with and without a workspace on GQA shapes,
where `bwd_workspace_bytes` > 0 asserts that the call with a workspace really splits its head groups."""
import itertools

import numpy as np
import pytest
import torch

import _visibility as V
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

BATCH = V.BWD_BATCH
NAN = float("nan")


@pytest.fixture(autouse=True, params=["mfma16", "mfma32"])
def pinned_set(gpu, request):
    prev = capi.set_kernel_policy(capi.POLICY_MFMA16 if request.param == "mfma16" else capi.POLICY_MFMA32)
    yield request.param
    capi.set_kernel_policy(prev)


def _nan(shape, dtype, gpu):
    return torch.full(shape, NAN, dtype=dtype, device=gpu)


def _run_capi(p, split, gpu):
    """the whole backward through the C ABI, with a NaN-prefilled workspace or with none"""
    need = capi.bwd_workspace_bytes(p)
    assert need > 0, "the launch must split its head groups when it is given the workspace"
    ws = None
    if split:
        ws = _nan((need // 4,), torch.float32, gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), need
    capi.run_bwd(p)
    torch.cuda.synchronize()


def _dense(c, hot, call, via, gpu):
    """BATCH copies of the case's one sequence -> (dQ (BATCH * sq, h, d), dK, dV (BATCH * sk, hk, d))"""
    sq, sk = c.sq[0], c.lens[0]
    q, k, v, do = (x.unsqueeze(0).repeat(BATCH, 1, 1, 1) for x in V.bwd_inputs(c, hot, call, gpu))
    q, do, k, v = q[:, :sq], do[:, :sq], k[:, :sk], v[:, :sk]
    o = torch.zeros(BATCH, sq, c.h, c.d, dtype=q.dtype, device=gpu)
    n = BATCH * c.h * sq
    lbuf = _nan((n + 64,), torch.float32, gpu)
    lbuf[:n] = 0
    lse = lbuf[:n].view(BATCH, c.h, sq)
    if via == "module":
        dq, dk, dv = F.bwd(q, k, v, o, lse, do, c.causal)
    else:
        dq, dk, dv = _nan(o.shape, q.dtype, gpu), _nan((BATCH, sk, c.hk, c.d), q.dtype, gpu), _nan((BATCH, sk, c.hk, c.d), q.dtype, gpu)
        p = capi.bwd_params(q, k, v, o, lse, do, dq, dk, dv, _nan((n,), torch.float32, gpu), c.causal)
        _run_capi(p, via == "split", gpu)
    assert dq.shape == (BATCH, sq, c.h, c.d) and dk.shape == dv.shape == (BATCH, sk, c.hk, c.d)
    return dq.reshape(BATCH * sq, c.h, c.d), dk.reshape(BATCH * sk, c.hk, c.d), dv.reshape(BATCH * sk, c.hk, c.d)


def _packed(c, hot, call, via, gpu):
    """the case's sequences as one packed call -> (dQ (total_q, h, d), dK, dV (total_k, hk, d))"""
    b, tq, tk, mq, mk = len(c.sq), sum(c.sq), sum(c.lens), max(c.sq), max(c.lens)
    cu_q = torch.tensor([0] + list(itertools.accumulate(c.sq)), dtype=torch.int32, device=gpu)
    cu_k = torch.tensor([0] + list(itertools.accumulate(c.lens)), dtype=torch.int32, device=gpu)
    q, k, v, do = V.bwd_inputs(c, hot, call, gpu)
    q, do, k, v = q[:tq], do[:tq], k[:tk], v[:tk]
    o = torch.zeros_like(q)
    live = torch.arange(mq, device=gpu).view(1, 1, mq) < torch.tensor(c.sq, device=gpu).view(b, 1, 1)
    lse = torch.where(live, 0.0, NAN).expand(b, c.h, mq).contiguous()                          # NaN in every padded entry
    if via == "module":
        dq, dk, dv = F.varlen_bwd(q, k, v, o, lse, do, cu_q, cu_k, mq, mk, c.causal)
    else:
        dq, dk, dv = _nan(q.shape, q.dtype, gpu), _nan(k.shape, q.dtype, gpu), _nan(k.shape, q.dtype, gpu)
        dsum = _nan((b, c.h, mq), torch.float32, gpu)
        row = lambda t: capi.Strides(0, t.stride(0), t.stride(1))
        p = capi.BwdParams(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), o=o.data_ptr(), lse=lse.data_ptr(), cu_seqlens_q=cu_q.data_ptr(), cu_seqlens_k=cu_k.data_ptr(),
                           b=b, seqlen_q=mq, seqlen_k=mk, h=c.h, h_k=c.hk, d=c.d, dtype=capi.dtype_code(q.dtype), is_causal=int(c.causal),
                           q_stride=row(q), k_stride=row(k), v_stride=row(v), o_stride=row(o), total_q=tq, total_k=tk,
                           dout=do.data_ptr(), dq=dq.data_ptr(), dk=dk.data_ptr(), dv=dv.data_ptr(), dsoftmax_sum=dsum.data_ptr(),
                           do_stride=row(do), dq_stride=row(dq), dk_stride=row(dk), dv_stride=row(dv))
        _run_capi(p, via == "split", gpu)
    assert dq.shape == (tq, c.h, c.d) and dk.shape == dv.shape == (tk, c.hk, c.d)
    return dq, dk, dv


def _probe(c, hot, via, gpu):
    """both calls of the case by one route, each gradient against the model"""
    for call in "AB":
        exp, rows, keys = V.expected_bwd(c, hot, call)
        if c.ragged:
            V.assert_bwd_signature(c, hot, call, _packed(c, hot, call, via, gpu), exp, rows, keys)
            continue
        tiled = V.replace(c, lens=c.lens * BATCH, sq=c.sq * BATCH)
        V.assert_bwd_signature(tiled, hot, call, _dense(c, hot, call, via, gpu), [np.tile(e, (BATCH, 1, 1)) for e in exp],
                               [(k, t) for k in range(BATCH) for _, t in rows], [(k, j) for k in range(BATCH) for _, j in keys])


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_dense_backward(gpu, d, dtype, causal, pinned_set):
    """bwd of the host module.  causal: every (sq, sk) of the tables, sq > sk included (dead rows: dQ = 0); non-causal: the diagonal.
    h / h_k rotates through 1, 4 and 6 / 1; the library splits the GQA groups whenever it would."""
    for c, hot in V.bwd_dense_cases(d, dtype, causal):
        _probe(c, hot, "module", gpu)


@pytest.mark.parametrize("via", ["split", "unsplit"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_dense_backward_group_split(gpu, d, dtype, causal, via, pinned_set):
    """the C ABI with a workspace (the head groups split over workgroups, fp32 planes summed by fa_bwd_sum_splits_kernel) and without
    (the group looped in one workgroup): the same cases both ways, every third (sq, sk) of the tables, h / h_k through 4 / 1, 6 / 1 and 8 / 2"""
    for c, hot in V.bwd_dense_cases(d, dtype, causal, gqa=True):
        _probe(c, hot, via, gpu)


@pytest.mark.parametrize("via", ["module", "split", "unsplit"])
@pytest.mark.parametrize("equal", [False, True])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_packed_backward(gpu, d, dtype, causal, equal, via, pinned_set):
    """varlen_bwd on the lengths of the tables as the sequences of one call, empty query and key sequences among them: skewed lengths
    (the compact grid) and equal ones (the plain grid), by the host module and by the C ABI with and without a workspace"""
    c, hot = V.bwd_packed_case(d, dtype, causal, equal, gqa=via != "module")
    _probe(c, hot, via, gpu)


@pytest.mark.parametrize("via", ["split", "unsplit"])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_one_hot_head(gpu, d, dtype, causal, via, pinned_set):
    """One query head of one KV group carries dO (and Q), its KV head alone K / V: every cold head's dQ and every cold KV head's dK / dV
    are exactly 0, the hot ones exactly 1 x the histogram.  Every head position of h / h_k = 2 / 2, 4 / 1, 6 / 1 and 8 / 2 is hot once on a
    dense and once on a packed call (split: the three shapes that have a group)."""
    for c, hot in V.bwd_head_cases(d, dtype, causal, via == "split"):
        if c.ratio == 1:
            _probe(c, hot, "module", gpu)                                       # (no group: the library asks for no workspace)
        else:
            _probe(c, hot, via, gpu)


def _span(r):
    return (r.start, r.stop) if len(r) else (0, 0)


@pytest.mark.parametrize("name", [p[0] for p in V.bwd_sensitivity_pairs()])
def test_one_length_moved_by_one(gpu, name, pinned_set):
    """the call with one length moved by one decodes to the model of the MOVED lengths, and differs from the model of the unmoved ones
    on exactly the rows (dQ) and keys (dK, dV) whose sets differ - the one-pair difference no tolerance sees"""
    _, base, moved, hot = next(p for p in V.bwd_sensitivity_pairs() if p[0] == name)
    wq, cnt = V.bwd_head_weights(moved, hot)
    seen_any = False
    for call in "AB":
        exp_m, rows_m, keys_m = V.expected_bwd(moved, hot, call)
        exp_b, rows_b, keys_b = V.expected_bwd(base, hot, call)
        grads = _packed(moved, hot, call, "module", gpu)
        V.assert_bwd_signature(moved, hot, call, grads, exp_m, rows_m, keys_m)
        dec = V.decode_bwd(moved, grads)
        for k, (index_m, index_b, weight, active) in enumerate(((rows_m, rows_b, wq > 0, call == "A"), (keys_m, keys_b, cnt > 0, call == "B"), (keys_m, keys_b, cnt > 0, True))):
            pos = {x: n for n, x in enumerate(index_b)}
            common = [(n, pos[x], x) for n, x in enumerate(index_m) if x in pos]
            im, ib = [x[0] for x in common], [x[1] for x in common]
            if k == 0:
                moved_sets = [_span(V.visible(moved.lens[i], moved.sq[i], t, moved.causal)[0]) != _span(V.visible(base.lens[i], base.sq[i], t, base.causal)[0]) for _, _, (i, t) in common]
            else:
                moved_sets = [_span(V.rows_seeing(moved.lens[i], moved.sq[i], j, moved.causal)) != _span(V.rows_seeing(base.lens[i], base.sq[i], j, base.causal)) for _, _, (i, j) in common]
            want = np.asarray(moved_sets)[:, None] & weight[None, :] & active
            got = (dec[k][im] != torch.from_numpy(exp_b[k][ib]).to(gpu)).any(dim=-1).cpu().numpy()
            assert np.array_equal(got, want), f"{name} call {call} {('dQ', 'dK', 'dV')[k]}: {int((got != want).sum())} (row or key, head) entries differ from the unmoved model where the sets agree, or agree where they differ"
            seen_any |= bool(want.any())
    assert seen_any, "the moved length must change a set"
