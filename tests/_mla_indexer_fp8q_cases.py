"""Shared inputs of the FP8 q_idx indexer tests (tests/test_mla_indexer_fp8q_cpu.py, tests/test_mla_indexer_fp8q_gpu.py): the inputs of
_mla_indexer_cases.py with the index queries as OCP e4m3 codes, and the one-hot patterns that check the operand mapping of the 16x16x128 MFMA with exact
integer data.  The fp64 model is C.logits_model on q.float(): float(code) is exact.  No GPU, no package import: plain torch."""
import torch

import _mla_indexer_cases as C

E4M3 = torch.float8_e4m3fn
ONE = 0x38                          # the code of 1.0


def code_values():
    """fp32 value of each of the 256 codes (0x7f and 0xff: NaN)"""
    return torch.arange(256, dtype=torch.uint8).view(E4M3).to(torch.float32)


def to_codes(x):
    """a tensor of values every one of which is an e4m3 value -> float8_e4m3fn, checked exact"""
    c = x.to(torch.float32).to(E4M3)
    assert torch.equal(c.to(torch.float32), x.to(torch.float32))
    return c


def exact_inputs(b, sq, h, gen, cap=C.CAP):
    """C.exact_inputs with an FP8 cache and q as e4m3 codes (integers in [-8, 8] are e4m3 values): (q8, w, k8, k_scale)"""
    q, w, k, sc = C.exact_inputs(b, sq, h, torch.bfloat16, True, gen, cap=cap)
    return to_codes(q), w, k, sc


def normal_quantised(b, sq, h, gen, cap=C.CAP):
    """C.normal_inputs over an FP8 cache, q quantised by the rule of quantize_mla_index_keys per (token, head) row (restated here in plain torch so that this
    module needs no package): (q8, weights * q_scale, k8, k_scale)"""
    q, w, k, sc = C.normal_inputs(b, sq, h, torch.bfloat16, True, gen, cap=cap)
    x = q.float()
    scale = torch.clamp(x.abs().amax(dim=-1, keepdim=True), min=2.0 ** -24) / torch.full((1,), 448.0)
    q8 = torch.clamp(x / scale, min=-448.0, max=448.0).to(E4M3)
    return q8, w * scale.squeeze(-1), k, sc


def one_hot_columns(qv=None, kv=None):
    """every column meets its column: sq 128, h 16, 128 keys.  Token t holds qv(t) (default 1) at column t of head t % 16, key j holds kv(j) (default 1) at
    column j; weights 1, no scale.  Returns (q8 (1, 128, 16, 128), w, k8 (1, 128, 128), want fp32 (128, 128)): want[t, j] = qv(t) kv(j) [t == j]"""
    n = 128
    t = torch.arange(n)
    qs = torch.ones(n) if qv is None else qv(t).float()
    ks = torch.ones(n) if kv is None else kv(t).float()
    q = torch.zeros(1, n, 16, C.D)
    q[0, t, t % 16, t] = qs
    k = torch.zeros(1, n, C.D)
    k[0, t, t] = ks
    return to_codes(q), torch.ones(1, n, 16), to_codes(k), torch.diag(qs * ks)


def one_hot_heads(h):
    """every head meets its weight: sq = h, 32 keys.  Token t has head t alone non-zero (column 0 = 1), every key has column 0 = 1, weights[t, hd] = hd + 1:
    logits[t, j] == t + 1"""
    q = torch.zeros(1, h, h, C.D)
    q[0, torch.arange(h), torch.arange(h), 0] = 1.0
    k = torch.zeros(1, 32, C.D)
    k[0, :, 0] = 1.0
    w = (torch.arange(h, dtype=torch.float32) + 1).view(1, 1, h).expand(1, h, h).contiguous()
    want = (torch.arange(h, dtype=torch.float32) + 1).view(h, 1).expand(h, 32).contiguous()
    return to_codes(q), w, to_codes(k), want


def every_code():
    """sq 256, 256 keys, h 16: token t carries code t at column t % 128 of head 0, key j carries code j at every column; weights 1, no scale.
    Returns (q8, w, k8, want fp32 (256, 256), finite bool (256, 256)): want[t, j] = max(float(code_t) * float(code_j), 0) where both codes are finite"""
    n = 256
    codes = torch.arange(n, dtype=torch.uint8)
    q = torch.zeros(1, n, 16, C.D, dtype=torch.uint8)
    q[0, torch.arange(n), 0, torch.arange(n) % 128] = codes
    k = codes.view(1, n, 1).expand(1, n, C.D).contiguous()
    v = code_values()
    fin = torch.isfinite(v)
    want = torch.clamp(v.view(n, 1) * v.view(1, n), min=0.0) + 0.0         # (fp32: exact, tests/test_mla_indexer_fp8q_cpu.py; + 0.0: a product -0 joins 127 terms +0)
    return q.view(E4M3), torch.ones(1, n, 16), k.view(E4M3), want, fin.view(n, 1) & fin.view(1, n)
