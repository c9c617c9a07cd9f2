"""GPU: the exact set of keys every query row of fwd / varlen_fwd sees, under both pinned kernel sets.

The probe of tests/_visibility.py on the dense and packed forward (fa_fwd_pp.hip, fa_fwd_pp16.hip): K = 0, so every score is exactly 0
and a row's LSE is log(number of visible keys); V carries the two-digit one-hot code of the key index, so out x count is the histogram
of the visible keys' digits.  Every assertion is an integer equality with the model `_visibility.visible` (length and the bottom-right
causal mask).  Rows past each K / V extent hold the bad code (1 in every column).  Dead rows (causal with sq > sk, empty key sequences)
are O = 0, LSE = 0 exactly, and the padded LSE entries of a packed call are exactly 0, as documented.

The backward has its own probe (tests/test_attention_backward_visibility_gpu.py): with the forward's uniform P, dK / dV are sums of
dO / n_i over rows and do not decode, but bwd / varlen_bwd take O and LSE as arguments, and lse = 0 makes P exactly 0 / 1."""
import itertools

import numpy as np
import pytest
import torch

import _visibility as V
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

BATCH = 2


@pytest.fixture(autouse=True, params=["mfma16", "mfma32"])
def pinned_set(gpu, request):
    prev = capi.set_kernel_policy(capi.POLICY_MFMA16 if request.param == "mfma16" else capi.POLICY_MFMA32)
    yield request.param
    capi.set_kernel_policy(prev)


def _kv(c, rows, gpu):
    """K = 0 and V = the codes of `rows` (key index per row, long tensor) with three more rows of the bad code behind: (rows + 3, hk, d)"""
    dt = V.torch_dtype(c.dtype)
    v = torch.full((len(rows) + 3, c.hk, c.d), V.BAD, dtype=dt, device=gpu)
    v[: len(rows)] = V.code_tensor(c.d, c.cap, gpu)[rows].to(dt).unsqueeze(1)
    return torch.zeros_like(v), v


def _check(c, out, lse, batch=1):
    """out (R, h, d), lse (R, h) of `batch` copies of the case's sequences against the model"""
    n_dec, hist_dec = V.decode(out, lse, torch.tensor(c.sink_extra()))
    n_exp, hist_exp, rows = V.expected(c)
    V.assert_signature(V.replace(c, lens=c.lens * batch, sq=c.sq * batch), n_dec, hist_dec, np.tile(n_exp, batch), np.tile(hist_exp, (batch, 1)),
                       [(i + k * len(c.lens), t) for k in range(batch) for i, t in rows])


def _dense(c, gpu):
    sq, sk = c.sq[0], c.lens[0]
    gen = torch.Generator(device="cpu").manual_seed(sq * 1031 + sk)
    q = torch.randn(BATCH, sq, c.h, c.d, generator=gen).to(gpu, V.torch_dtype(c.dtype))
    k1, v1 = _kv(c, torch.arange(sk, device=gpu), gpu)
    k, v = (x.unsqueeze(0).repeat(BATCH, 1, 1, 1) for x in (k1, v1))
    out, lse = F.fwd(q, k[:, :sk], v[:, :sk], c.causal)
    assert out.shape == q.shape and lse.shape == (BATCH, c.h, sq)
    _check(c, out.reshape(BATCH * sq, c.h, c.d), lse.permute(0, 2, 1).reshape(BATCH * sq, c.h), BATCH)


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_dense_forward(gpu, d, dtype, causal, pinned_set):
    """causal: every (sq, sk) of the tables, sq > sk included; non-causal: the diagonal.  h / h_k rotates through 1, 4 and 6 / 1."""
    i = (d == 128) * 2 + V.DTYPES.index(dtype)
    for j, (sq, sk) in enumerate(V.attn_pairs(causal)):
        _dense(V.attn_case(sq, sk, causal, d, dtype, V.ATTN_HEADS[(j + i) % 3]), gpu)


@pytest.mark.parametrize("equal", [False, True])
@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("d", [64, 128])
def test_packed_forward(gpu, d, dtype, causal, equal, pinned_set):
    """the same lengths as the sequences of one varlen_fwd call, empty query and key sequences among them: skewed lengths (the compact
    grid) and equal ones (the plain grid)"""
    i = (d == 128) * 2 + V.DTYPES.index(dtype)
    c = V.attn_packed(causal, d, dtype, V.ATTN_HEADS[(i + causal + equal) % 3], equal)
    cu_q = torch.tensor([0] + list(itertools.accumulate(c.sq)), dtype=torch.int32, device=gpu)
    cu_k = torch.tensor([0] + list(itertools.accumulate(c.lens)), dtype=torch.int32, device=gpu)
    total_q, max_q, max_k = sum(c.sq), max(c.sq), max(c.lens)
    gen = torch.Generator(device="cpu").manual_seed(total_q + d)
    q = torch.randn(total_q, c.h, c.d, generator=gen).to(gpu, V.torch_dtype(c.dtype))
    k, v = _kv(c, torch.cat([torch.arange(L, device=gpu) for L in c.lens]), gpu)
    out, lse = F.varlen_fwd(q, k[: sum(c.lens)], v[: sum(c.lens)], cu_q, cu_k, max_q, max_k, c.causal)
    assert out.shape == q.shape and lse.shape == (len(c.sq), c.h, max_q)
    t = torch.arange(max_q, device=gpu).unsqueeze(0)
    live = t < torch.tensor(c.sq, device=gpu).unsqueeze(1)                                      # (b, max_q)
    assert (lse.permute(0, 2, 1)[~live] == 0).all().item(), "padded LSE entries must be exactly 0"
    _check(c, out, lse.permute(0, 2, 1)[live])
