"""MLA prefill attention (flash_mla_prefill_func): the shapes of tests/test_mla_prefill_gpu.py and the fp64 model they are held to; CPU only, so
that tests/test_mla_prefill_cpu.py can validate the expectation (against torch's fp64 SDPA with an explicit mask) without a device.

Shapes: the smallest that cross every boundary of a 64-row tile (or a 128-row one) and of the 32-key step.  (200, 1040) is 33 steps: both LDS
stages are reused and the last step is partial.  h / h_k = 3 makes packed rows straddle the 16- and 64-row boundaries.  The packed batch holds an
empty query sequence, an empty key sequence, more rows than keys, and two sequences of several tiles."""
import itertools

import torch

import _util as U

DQK, DV = 192, 128
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DTYPES = ("fp16", "bf16")
SHAPES = ((1, 1), (1, 33), (17, 5), (64, 64), (65, 31), (63, 97), (130, 131), (200, 1040))       # (sq, sk)
HEADS = ((2, 2), (4, 1), (6, 2))                                                                  # (h, h_k)
PACKED_SQ = (0, 1, 17, 64, 130)
PACKED_SK = (33, 0, 5, 97, 131)
SCALE = 192 ** -0.5


def cu(lens, device="cpu"):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device=device)


def inputs(sq, sk, h, hk, dtname, seed, b=1):
    """q (b, sq, h, 192), k (b, sk, hk, 192), v (b, sk, hk, 128): N(0, 1) from a CPU generator, in the dtype, on the CPU"""
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(b, s, hh, d, generator=gen).to(DT[dtname]) for s, hh, d in ((sq, h, DQK), (sk, hk, DQK), (sk, hk, DV)))


def packed_inputs(sqs, sks, h, hk, dtname, seed):
    """q (total_q, h, 192), k (total_k, hk, 192), v (total_k, hk, 128) and the two cu_seqlens, on the CPU"""
    q, k, v = inputs(sum(sqs), sum(sks), h, hk, dtname, seed)
    return q[0], k[0], v[0], cu(sqs), cu(sks)


def model(q, k, v, causal):
    """one sequence in fp64: q (sq, h, 192), k (sk, hk, 192), v (sk, hk, 128) -> O (sq, h, 128), LSE (h, sq).  _util.fp64_math takes a V narrower
    than K and scales by 1 / sqrt(192), the width of q; dead rows are O = 0, LSE = 0."""
    assert q.shape[-1] == DQK and k.shape[-1] == DQK and v.shape[-1] == DV
    return U.fp64_math(q, k, v, causal)


def packed_model(q, k, v, cu_q, cu_k, causal):
    """the model of every sequence of a packed batch, in packed order: O (cu_q[-1], h, 128), LSE (h, cu_q[-1])"""
    os_, ls = [], []
    for i in range(len(cu_q) - 1):
        o, l = model(q[cu_q[i]:cu_q[i + 1]], k[cu_k[i]:cu_k[i + 1]], v[cu_k[i]:cu_k[i + 1]], causal)
        os_.append(o)
        ls.append(l)
    return torch.cat(os_, 0), torch.cat(ls, 1)


def sdpa(q, k, v, causal):
    """the same sequence through torch.nn.functional.scaled_dot_product_attention in fp64 with an EXPLICIT boolean mask (bottom-right aligned) and an
    explicit scale; dead rows (a mask row of all False) are set to 0 as the contract says.  Returns O (sq, h, 128) and the mask (sq, sk)."""
    sq, h = q.shape[0], q.shape[1]
    sk, hk = k.shape[0], k.shape[1]
    t = torch.arange(sq).view(-1, 1)
    j = torch.arange(sk).view(1, -1)
    mask = (j <= sk - sq + t) if causal else torch.ones(sq, sk, dtype=torch.bool)
    qt = q.double().permute(1, 0, 2).unsqueeze(0)
    kt = k.double().repeat_interleave(h // hk, dim=1).permute(1, 0, 2).unsqueeze(0)
    vt = v.double().repeat_interleave(h // hk, dim=1).permute(1, 0, 2).unsqueeze(0)
    live = mask.any(-1)
    safe = mask | ~live.view(-1, 1)             # a dead row attends to everything here and is zeroed below: SDPA's own answer for it is NaN
    if sk == 0:
        o = torch.zeros(sq, h, DV, dtype=torch.float64)
    else:
        o = torch.nn.functional.scaled_dot_product_attention(qt, kt, vt, attn_mask=safe.view(1, 1, sq, sk), scale=SCALE)[0].permute(1, 0, 2)
    return torch.where(live.view(-1, 1, 1), o, torch.zeros(()).double()), mask


def scores64(q, k):
    """fp64 scores of a dense batch, scaled: q (b, sq, h, 192), k (b, sk, hk, 192) -> (b, h, sq, sk)"""
    h, hk = q.shape[2], k.shape[2]
    return torch.einsum("bthd,bjhd->bhtj", q.double(), k.double().repeat_interleave(h // hk, dim=2)) * SCALE


def causal_mask(sq, sk):
    return torch.arange(sk).view(1, -1) <= sk - sq + torch.arange(sq).view(-1, 1)
