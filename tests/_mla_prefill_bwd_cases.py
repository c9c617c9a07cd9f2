"""The MLA prefill backward (flash_mla_prefill_bwd / flash_mla_attn_func): the shapes of tests/test_mla_prefill_bwd_gpu.py and the fp64 expectation
they are held to; CPU only, so that tests/test_mla_prefill_bwd_cpu.py can validate the expectation without a device.

Shapes are the forward's (tests/_mla_prefill_cases.py), imported and not copied, plus one for the dK/dV kernel: (150, 100) has more than 64 keys,
more than 2 x 32 packed rows and sq > sk, so that under `causal` the second key tile starts its row walk past row 0 (at h / h_k = 3: packed row 320).

The expectation is torch autograd in fp64 through the explicit formula of _util.fp64_math (scores, masked_fill, exp of the shifted scores, row sum,
division).  _util.fp64_math itself detaches its inputs, so `forward64` restates it line for line without the detach - and with the row sum of a dead row
replaced by 1 in front of the division, which leaves O = 0 there and keeps 0 / 0 out of the graph; tests/test_mla_prefill_bwd_cpu.py asserts that its O
equals fp64_math's bit for bit and its gradients those of fp64 scaled_dot_product_attention under the explicit mask."""
import math

import torch

import _mla_prefill_cases as C
import _util as U

SHAPES = C.SHAPES + ((150, 100),)
HEADS = C.HEADS
PACKED_SQ = C.PACKED_SQ
PACKED_SK = C.PACKED_SK


def forward64(q, k, v, causal, scale=None):
    """U.fp64_math on fp64 tensors WITHOUT the detach (so autograd sees q, k, v): one sequence, q (sq, h, 192), k (L, hk, 192), v (L, hk, 128) -> O (sq, h, 128)"""
    sq, h, _ = q.shape
    L, hk = k.shape[0], k.shape[1]
    if L == 0 or sq == 0:
        return torch.zeros(sq, h, v.shape[-1], dtype=torch.float64) + 0.0 * (q.sum() + k.sum() + v.sum())
    kt, vt = k.repeat_interleave(h // hk, dim=1), v.repeat_interleave(h // hk, dim=1)
    s = torch.einsum("thd,jhd->htj", q, kt)
    s = s / math.sqrt(q.shape[-1]) if scale is None else s * scale       # (None: fp64_math's own division)
    if causal:
        t = torch.arange(sq).view(-1, 1)
        j = torch.arange(L).view(1, -1)
        s = s.masked_fill((j > L - sq + t).unsqueeze(0), float("-inf"))
    m = s.detach().amax(dim=-1)
    dead = m == float("-inf")
    p = torch.exp(s - torch.where(dead, torch.zeros_like(m), m).unsqueeze(-1))
    l = p.sum(dim=-1)
    o = torch.einsum("htj,jhd->thd", p, vt) / torch.where(dead, torch.ones_like(l), l).t().unsqueeze(-1)
    return o


def grads64(q, k, v, dout, causal, scale=None):
    """(dq, dk, dv) of one sequence in fp64 by autograd through forward64; inputs of any dtype, taken as the numbers they hold"""
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    o = forward64(q, k, v, causal, scale)
    o.backward(dout.detach().double())
    return q.grad, k.grad, v.grad


def sdpa_grads64(q, k, v, dout, causal):
    """the same through fp64 scaled_dot_product_attention with the explicit mask (C.sdpa)"""
    q, k, v = (t.detach().double().clone().requires_grad_(True) for t in (q, k, v))
    o, _ = C.sdpa(q, k, v, causal)
    if o.requires_grad:                         # (no key or no row: C.sdpa returns constants)
        (o * dout.detach().double()).sum().backward()
    zero = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)
    return zero(q), zero(k), zero(v)


def packed_grads64(q, k, v, dout, cu_q, cu_k, causal, scale=None):
    gs = [grads64(q[cu_q[i]:cu_q[i + 1]], k[cu_k[i]:cu_k[i + 1]], v[cu_k[i]:cu_k[i + 1]], dout[cu_q[i]:cu_q[i + 1]], causal, scale) for i in range(len(cu_q) - 1)]
    return tuple(torch.cat([g[n] for g in gs], 0) for n in range(3))


def dout_like(q, seed):
    """dout ~ N(0, 1) in q's dtype, shaped like the forward's out"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(q.shape[:-1]) + (C.DV,), generator=gen).to(q.dtype)


# ---- the rounding model: an fp64 backward with the kernels' rounding points --------------------------------------------------------

def rounding_model(q, k, v, dout, causal, dtname, scale=C.SCALE, *, ds_rounding="nearest", d_factor=1.0, dk_scale=None, scale_error=0.0, drop_pair=None, drop_head=None):
    """dense batch q (b, sq, h, 192), k (b, sk, hk, 192), v (b, sk, hk, 128), dout (b, sq, h, 128) -> (dq, dk, dv) in fp64, each rounded once to the dtype,
    with the kernels' rounding points: O rounded to the dtype (the forward's output) and D = sum(dout * O) from it; P and dS rounded to the dtype in front
    of dV += P^T dO and dQ / dK += dS K / dS^T Q; everything else exact.  The keywords are the mutants of tests/test_mla_prefill_bwd_cpu.py:
    ds_rounding="truncate", d_factor (D times it), dk_scale (the factor on dK in place of scale), scale_error (dQ and dK times 1 + it), drop_pair = (row, key) left out everywhere,
    drop_head = a query head left out of dK.  Also returns the unrounded fp64 expectation (dq64, dk64, dv64)."""
    import _accuracy as A

    b, sq, h, _ = q.shape
    sk, hk = k.shape[1], k.shape[2]
    g = h // hk
    r16 = lambda x, mode="nearest": torch.from_numpy(A.round16(x.numpy(), dtname, mode))
    q64, k64, v64, do64 = (t.double() for t in (q, k, v, dout))
    kt, vt = k64.repeat_interleave(g, dim=2), v64.repeat_interleave(g, dim=2)
    s = torch.einsum("bthd,bjhd->bhtj", q64, kt) * scale
    vis = (C.causal_mask(sq, sk) if causal else torch.ones(sq, sk, dtype=torch.bool)).clone()
    lse = torch.logsumexp(s.masked_fill(~vis, float("-inf")), dim=-1, keepdim=True)
    p = torch.where(vis, torch.exp(s - lse), torch.zeros(()).double())
    o64 = torch.einsum("bhtj,bjhd->bthd", p, vt)
    dp = torch.einsum("bthd,bjhd->bhtj", do64, vt)

    def grads(p_, ds_, head_keep=None, kscale=scale):
        dq = torch.einsum("bhtj,bjhd->bthd", ds_, kt) * scale
        dsk = ds_ if head_keep is None else ds_ * head_keep.view(1, h, 1, 1)
        dk = (torch.einsum("bhtj,bthd->bjhd", dsk, q64) * kscale).view(b, sk, hk, g, -1).sum(3)
        dv = torch.einsum("bhtj,bthd->bjhd", p_, do64).view(b, sk, hk, g, -1).sum(3)
        return dq, dk, dv

    d_exact = (do64 * o64).sum(-1).permute(0, 2, 1).unsqueeze(-1)
    exact = grads(p, p * (dp - d_exact))
    o_r = r16(o64)
    d_r = (do64 * o_r).sum(-1).permute(0, 2, 1).unsqueeze(-1) * d_factor
    pm = p
    if drop_pair is not None:
        keep = torch.ones(sq, sk, dtype=torch.bool)
        keep[drop_pair] = False
        pm = torch.where(keep, p, torch.zeros(()).double())
    ds_r = r16(pm * (dp - d_r), ds_rounding)
    p_r = r16(pm)
    keep_h = None
    if drop_head is not None:
        keep_h = torch.ones(h, dtype=torch.float64)
        keep_h[drop_head] = 0.0
    dq_m, dk_m, dv_m = grads(p_r, ds_r, keep_h, scale if dk_scale is None else dk_scale)
    model = tuple(r16(x) for x in (dq_m * (1 + scale_error), dk_m * (1 + scale_error), dv_m))
    return model, exact
