"""Autograd-aware wrappers over the raw fwd/bwd entry points.

The reference ships only the four raw functions; its README (README.md:28-48) documents
``flash_attn_func(q, k, v, batch_size, seq_len, num_heads, head_dim)`` from an older API.
``flash_attn_func`` here accepts both that legacy call (the four ints are validated against
the tensor shapes and otherwise ignored) and the modern ``flash_attn_func(q, k, v, causal=False)``.
"""
import math
import numbers
import re

import torch

from . import _C


class FlashAttnFunc(torch.autograd.Function):
    """O = softmax(Q K^T / sqrt(d) + causal_mask) V on (batch, seqlen, heads, head_dim) tensors.

    The Python form of the autograd node, kept as the readable statement of what ``_C.attn_autograd`` does (flash_api.cpp:FlashAttnNode);
    ``flash_attn_func`` goes through the C++ node, which costs the host 42-52 us per forward + backward instead of ~85 (profiles/r4_host_overhead.log)."""

    @staticmethod
    def forward(ctx, q, k, v, causal):
        out, lse = _C.fwd(q, k, v, bool(causal))
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal = bool(causal)
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = _C.bwd(q, k, v, out, lse, dout, ctx.causal)      # strided dout is fine: the kernels take real strides
        return dq, dk, dv, None


class FlashAttnVarlenFunc(torch.autograd.Function):
    """Packed variable-length variant: q (total_q, h, d), k/v (total_k, h_k, d), int32 cu_seqlens."""

    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal):
        out, lse = _C.varlen_fwd(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), bool(causal))
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k)
        ctx.meta = (int(max_seqlen_q), int(max_seqlen_k), bool(causal))
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, cu_q, cu_k = ctx.saved_tensors
        max_q, max_k, causal = ctx.meta
        dq, dk, dv = _C.varlen_bwd(q, k, v, out, lse, dout, cu_q, cu_k, max_q, max_k, causal)
        return dq, dk, dv, None, None, None, None, None


def flash_attn_func(q, k, v, *legacy_dims, causal=False, return_lse=False):
    """Fused scaled-dot-product attention (scale fixed at 1/sqrt(head_dim), like the reference).

    q: (batch, seqlen_q, nheads, d); k, v: (batch, seqlen_k, nheads_k, d); fp16 or bf16 on a
    ROCm device.  ``causal`` uses bottom-right alignment (reference mask.h:172).  The legacy
    README form ``flash_attn_func(q, k, v, batch_size, seq_len, num_heads, head_dim)`` is accepted.
    """
    if legacy_dims:
        if len(legacy_dims) == 1 and isinstance(legacy_dims[0], bool):
            causal = legacy_dims[0]
        elif len(legacy_dims) == 4:
            b, s, h, d = (int(x) for x in legacy_dims)
            if (b, s, h, d) != (q.shape[0], q.shape[1], q.shape[2], q.shape[3]):
                raise ValueError(f"legacy dims {(b, s, h, d)} do not match q.shape {tuple(q.shape)}")
        else:
            raise TypeError("flash_attn_func(q, k, v[, batch_size, seq_len, num_heads, head_dim], causal=False)")
    if return_lse:
        out, lse = _C.fwd(q, k, v, bool(causal))
        return out, lse
    return _C.attn_autograd(q, k, v, bool(causal))


def flash_attn_varlen_func(q, k, v, cu_seqlens_q, cu_seqlens_k, max_seqlen_q, max_seqlen_k, causal=False):
    return _C.attn_varlen_autograd(q, k, v, cu_seqlens_q, cu_seqlens_k, int(max_seqlen_q), int(max_seqlen_k), bool(causal))


def _window_pair(window_size):
    """(left, right) as two ints >= -1; anything else is a ValueError"""
    try:
        left, right = window_size
    except (TypeError, ValueError):
        raise ValueError(f"window_size must be a pair of ints (left, right), got {window_size!r}") from None
    if any(isinstance(x, bool) or not isinstance(x, numbers.Integral) for x in (left, right)):
        raise ValueError(f"window_size must be a pair of ints (left, right), got {window_size!r}")
    left, right = int(left), int(right)
    if left < -1 or right < -1 or left > 2**31 - 1 or right > 2**31 - 1:
        raise ValueError(f"window_size {tuple(window_size)!r}: each side must be >= -1 (-1 = unbounded) and fit in int32")
    return left, right


def _check_cache_dtype(q, k_cache, v_cache, k_descale, v_descale, batch=None):
    """the cache has q's dtype, or is an FP8 e4m3fn cache with optional float32 (batch, nheads_k) descales on q's device (batch: q.shape[0],
    or the sequences of a ragged call)"""
    batch = q.shape[0] if batch is None else batch
    if k_cache.dtype != v_cache.dtype:
        raise ValueError(f"k_cache and v_cache must have the same dtype, got {k_cache.dtype} and {v_cache.dtype}")
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    if not fp8 and k_cache.dtype != q.dtype:
        raise ValueError(f"k_cache / v_cache must have the dtype of q ({q.dtype}) or be torch.float8_e4m3fn, got {k_cache.dtype}")
    for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
        if t is None:
            continue
        if not fp8:
            raise ValueError(f"{name} needs a torch.float8_e4m3fn cache (the cache is {k_cache.dtype})")
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 tensor")
        if k_cache.dim() != 4 or tuple(t.shape) != (batch, k_cache.shape[2]):
            raise ValueError(f"{name} must have shape (batch, nheads_k) = ({batch}, {k_cache.shape[2] if k_cache.dim() == 4 else '?'}), got {tuple(t.shape)}")
        if t.device != q.device:
            raise ValueError(f"{name} must be on q's device ({q.device}), got {t.device}")


def _check_rotary(q, k_cache, k, block_table, rotary_cos, rotary_sin, rotary_interleaved):
    """rotary_cos / rotary_sin: both or neither, (seqlen_ro, rotary_dim / 2) of q's dtype on q's device, last dim contiguous, rotary_dim a
    multiple of 16 in [16, d], seqlen_ro at least the cache capacity; they need k / v"""
    if not isinstance(rotary_interleaved, bool):
        raise ValueError(f"rotary_interleaved must be a bool, got {rotary_interleaved!r}")
    if rotary_cos is None and rotary_sin is None:
        return
    if rotary_cos is None or rotary_sin is None:
        raise ValueError("rotary_cos and rotary_sin must both be given or both be None")
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if not isinstance(t, torch.Tensor) or t.dtype != q.dtype:
            raise ValueError(f"{name} must be a tensor of q's dtype ({q.dtype}; fp32 tables are not supported), got {getattr(t, 'dtype', type(t))}")
        if t.dim() != 2:
            raise ValueError(f"{name} must have shape (seqlen_ro, rotary_dim / 2), got {tuple(t.shape)}")
        if t.device != q.device:
            raise ValueError(f"{name} must be on q's device ({q.device}), got {t.device}")
    if rotary_cos.shape != rotary_sin.shape:
        raise ValueError(f"rotary_cos and rotary_sin must have the same shape, got {tuple(rotary_cos.shape)} and {tuple(rotary_sin.shape)}")
    for name, t in (("rotary_cos", rotary_cos), ("rotary_sin", rotary_sin)):
        if t.stride(1) != 1:
            raise ValueError(f"{name}: the last dimension must be contiguous")
    rotary_dim = 2 * rotary_cos.shape[1]
    if rotary_dim < 16 or rotary_dim % 16 != 0 or rotary_dim > q.shape[-1]:
        raise ValueError(f"rotary_dim (2 x rotary_cos.shape[1] = {rotary_dim}) must be a multiple of 16 with 16 <= rotary_dim <= head_dim ({q.shape[-1]})")
    if k is None:
        raise ValueError("rotary_cos / rotary_sin are only applicable if k and v are passed in")
    capacity = k_cache.shape[1] * block_table.shape[1] if block_table is not None else k_cache.shape[1]
    if rotary_cos.shape[0] < max(capacity, 1):
        raise ValueError(f"seqlen_ro ({rotary_cos.shape[0]} rows of rotary_cos / rotary_sin) must be at least the cache capacity ({capacity})")


def _check_scale_and_cap(softmax_scale, softcap):
    """softmax_scale: None or a real number that is finite and > 0 as an fp32 value; softcap: a real number that is finite and >= 0 as an fp32
    value (0 = off); bools are not numbers here.  Returns (softmax_scale or None, softcap) as Python floats."""
    if softmax_scale is not None:
        if isinstance(softmax_scale, bool) or not isinstance(softmax_scale, numbers.Real):
            raise ValueError(f"softmax_scale must be None or a real number > 0, got {softmax_scale!r}")
        softmax_scale = float(softmax_scale)
        s32 = torch.tensor(softmax_scale, dtype=torch.float32).item()
        if not (math.isfinite(s32) and s32 > 0):
            raise ValueError(f"softmax_scale must be finite and > 0 (as an fp32 value), got {softmax_scale!r}")
    if isinstance(softcap, bool) or not isinstance(softcap, numbers.Real):
        raise ValueError(f"softcap must be a real number >= 0 (0.0 = no cap), got {softcap!r}")
    softcap = float(softcap)
    c32 = torch.tensor(softcap, dtype=torch.float32).item()
    if not (math.isfinite(c32) and c32 >= 0) or (softcap != 0 and c32 == 0):
        raise ValueError(f"softcap must be finite and >= 0 (as an fp32 value; 0.0 = no cap), got {softcap!r}")
    return softmax_scale, softcap


def _check_sinks(sinks, q, softcap):
    """sinks: a 1-D tensor (nheads,) on q's device, float32 or q's dtype, any stride; not with a soft cap, not at head_dim 256.  Returns it as
    float32 (q's dtype is widened with a torch op: exact, asynchronous, capturable)."""
    if not isinstance(sinks, torch.Tensor):
        raise ValueError(f"sinks must be None or a tensor of shape (nheads,), got {type(sinks).__name__}")
    if sinks.dtype != torch.float32 and sinks.dtype != q.dtype:
        raise ValueError(f"sinks must be float32 or have q's dtype ({q.dtype}), got {sinks.dtype}")
    if sinks.dim() != 1 or sinks.shape[0] != q.shape[-2]:
        raise ValueError(f"sinks must have shape (nheads,) = ({q.shape[-2]},): one logit per query head, got {tuple(sinks.shape)}")
    if sinks.device != q.device:
        raise ValueError(f"sinks must be on q's device ({q.device}), got {sinks.device}")
    if softcap != 0.0:
        raise ValueError("sinks together with softcap > 0 are not supported")
    if q.shape[-1] == 256:
        raise ValueError("sinks at head_dim 256 are not supported: flash_attn_with_kvcache has sinks at head_dim 64 and 128")
    return sinks if sinks.dtype == torch.float32 else sinks.float()


def _check_tree_mask(tree_mask, q, causal, window, softcap, sinks, rotary_cos, rotary_sin, cu_seqlens_q, max_seqlen_q):
    """tree_mask: an int64 tensor on q's device, (batch, seqlen_q) or, ragged, (total_q,), any strides; at most 64 query rows per sequence; not with
    causal, a window, a soft cap, sinks, rotary or head_dim 256"""
    if not isinstance(tree_mask, torch.Tensor):
        raise ValueError(f"tree_mask must be None or an int64 tensor, got {type(tree_mask).__name__}")
    if tree_mask.dtype != torch.int64:
        raise ValueError(f"tree_mask must be an int64 tensor (one 64-bit word per query row), got {tree_mask.dtype}")
    if cu_seqlens_q is None:
        if q.dim() == 4 and tuple(tree_mask.shape) != tuple(q.shape[:2]):
            raise ValueError(f"tree_mask must have shape (batch, seqlen_q) = {tuple(q.shape[:2])}, got {tuple(tree_mask.shape)}")
        sq = q.shape[1] if q.dim() == 4 else 0
    else:
        if q.dim() == 3 and tuple(tree_mask.shape) != (q.shape[0],):
            raise ValueError(f"tree_mask must have shape (total_q,) = ({q.shape[0]},) with cu_seqlens_q, got {tuple(tree_mask.shape)}")
        sq = max_seqlen_q if isinstance(max_seqlen_q, numbers.Integral) and not isinstance(max_seqlen_q, bool) else 0
    if tree_mask.device != q.device:
        raise ValueError(f"tree_mask must be on q's device ({q.device}), got {tree_mask.device}")
    if causal:
        raise ValueError("tree_mask together with causal=True is not supported (the lower-triangle mask is the causal call)")
    if window != (-1, -1):
        raise ValueError(f"tree_mask together with window_size {window} is not supported")
    if softcap != 0.0:
        raise ValueError("tree_mask together with softcap > 0 is not supported")
    if sinks is not None:
        raise ValueError("tree_mask together with sinks is not supported")
    if rotary_cos is not None or rotary_sin is not None:
        raise ValueError("tree_mask together with rotary_cos / rotary_sin is not supported: a node's position is its depth, not its index - rotate q and k before the call")
    if q.shape[-1] == 256:
        raise ValueError("tree_mask at head_dim 256 is not supported: flash_attn_with_kvcache has tree masks at head_dim 64 and 128")
    if sq > 64:
        raise ValueError(f"tree_mask: seqlen_q (ragged: max_seqlen_q) must be at most 64, the draft tokens one mask word holds, got {sq}")
    return tree_mask


def pack_tree_mask(mask):
    """bool (..., sq, sq) -> int64 (..., sq), the ``tree_mask`` of flash_attn_with_kvcache: bit u of word t is mask[..., t, u] ("draft token t sees
    draft token u"), sq <= 64; column 63 lands in the sign bit.  Torch ops only, on mask's device."""
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
        raise ValueError(f"mask must be a bool tensor, got {getattr(mask, 'dtype', type(mask).__name__)}")
    if mask.dim() < 2 or mask.shape[-1] != mask.shape[-2] or mask.shape[-1] > 64:
        raise ValueError(f"mask must have shape (..., sq, sq) with sq <= 64, got {tuple(mask.shape)}")
    sq = mask.shape[-1]
    # (1 << 63 wraps to the sign bit in int64 arithmetic, and the bits are disjoint: the sum is their OR)
    weights = torch.ones((), dtype=torch.int64, device=mask.device) << torch.arange(sq, dtype=torch.int64, device=mask.device)
    return (mask.to(torch.int64) * weights).sum(dim=-1)


def tree_mask_from_parents(parents):
    """int (..., sq) -> int64 (..., sq): parents[..., t] is the index of draft token t's parent, -1 for a root, always < t (a forest in topological
    order, as draft trees are built).  Word t has the bits of t's ancestors and of t itself.  Torch ops only, on parents' device: sq steps, each
    ORs a parent's finished word into its child's."""
    if not isinstance(parents, torch.Tensor) or parents.dtype.is_floating_point or parents.dtype.is_complex or parents.dtype == torch.bool:
        raise ValueError(f"parents must be an integer tensor, got {getattr(parents, 'dtype', type(parents).__name__)}")
    if parents.dim() < 1 or parents.shape[-1] > 64:
        raise ValueError(f"parents must have shape (..., sq) with sq <= 64, got {tuple(parents.shape)}")
    sq = parents.shape[-1]
    par = parents.to(torch.int64)
    one = torch.ones((), dtype=torch.int64, device=parents.device)
    words = torch.zeros(par.shape, dtype=torch.int64, device=parents.device)
    for t in range(sq):
        p = par[..., t]
        up = torch.gather(words, -1, p.clamp(0, max(t - 1, 0)).unsqueeze(-1)).squeeze(-1) if t > 0 else torch.zeros_like(p)
        words[..., t] = torch.where((p >= 0) & (p < t), up, torch.zeros_like(up)) | (one << t)
    return words


def _check_prefill(q, window, softcap, sinks, tree_mask, rotary_cos, rotary_sin):
    """prefill=True: the 64-row kernels serve the plain and the causal call; not a window, a soft cap, sinks, a tree mask, rotary or head_dim 256"""
    if window != (-1, -1):
        raise ValueError(f"prefill=True together with window_size {window} is not supported")
    if softcap != 0.0:
        raise ValueError("prefill=True together with softcap > 0 is not supported")
    if sinks is not None:
        raise ValueError("prefill=True together with sinks is not supported")
    if tree_mask is not None:
        raise ValueError("prefill=True together with tree_mask is not supported")
    if rotary_cos is not None or rotary_sin is not None:
        raise ValueError("prefill=True together with rotary_cos / rotary_sin is not supported")
    if q.shape[-1] == 256:
        raise ValueError("prefill=True at head_dim 256 is not supported: flash_attn_with_kvcache has the 64-row kernels at head_dim 64 and 128")


def _check_kvcache_head_dim(q):
    """decode over a KV cache has head_dim 64, 128 and 256 (fwd / bwd / varlen_*: 64 and 128)"""
    if q.shape[-1] not in (64, 128, 256):
        raise ValueError(f"head_dim {q.shape[-1]} unsupported: flash_attn_with_kvcache has head_dim 64, 128 and 256")


def _check_cu_seqlens(name, t, q, batch=None):
    """a cu_seqlens tensor: int32, shape (b + 1,), contiguous, on q's device"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32:
        raise ValueError(f"{name} must be an int32 tensor, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 1 or t.shape[0] < 1 or (batch is not None and t.shape[0] != batch + 1):
        raise ValueError(f"{name} must have shape (batch + 1,){'' if batch is None else f' = ({batch + 1},)'}, got {tuple(t.shape)}")
    if t.device != q.device:
        raise ValueError(f"{name} must be on q's device ({q.device}), got {t.device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _check_ragged(q, k_cache, k, v, cache_seqlens, block_table, k_descale, v_descale, rotary_cos, rotary_sin, cu_seqlens_q, max_seqlen_q, cu_seqlens_k_new):
    """the arguments of a ragged call (cu_seqlens_q given): packed q / k / v, the batch of every per-sequence tensor, no rotary"""
    if rotary_cos is not None or rotary_sin is not None:
        raise ValueError("rotary_cos / rotary_sin together with cu_seqlens_q are not supported (rotary with ragged queries is out of scope)")
    _check_cu_seqlens("cu_seqlens_q", cu_seqlens_q, q)
    b = cu_seqlens_q.shape[0] - 1
    if isinstance(max_seqlen_q, bool) or not isinstance(max_seqlen_q, numbers.Integral) or max_seqlen_q < 1 or max_seqlen_q > 2**31 - 1:
        raise ValueError(f"max_seqlen_q must be a Python int >= 1 with cu_seqlens_q, got {max_seqlen_q!r}")
    if q.dim() != 3:
        raise ValueError(f"q must be packed (total_q, nheads, d) with cu_seqlens_q, got shape {tuple(q.shape)}")
    if k is not None:
        if k.dim() == 4 or v.dim() == 4:
            raise ValueError("k and v must be packed (total_new, nheads_k, d) with cu_seqlens_q (a 4-D k belongs to the dense call)")
        if k.dim() != 3 or v.dim() != 3:
            raise ValueError(f"k and v must be packed (total_new, nheads_k, d) with cu_seqlens_q, got shapes {tuple(k.shape)} and {tuple(v.shape)}")
        if cu_seqlens_k_new is None:
            raise ValueError("packed k and v need cu_seqlens_k_new (it may be the same tensor as cu_seqlens_q)")
        _check_cu_seqlens("cu_seqlens_k_new", cu_seqlens_k_new, q, b)
    elif cu_seqlens_k_new is not None:
        raise ValueError("cu_seqlens_k_new given without k and v")
    if isinstance(cache_seqlens, torch.Tensor) and tuple(cache_seqlens.shape) != (b,):
        raise ValueError(f"cache_seqlens must have shape (batch,) = ({b},) (batch = len(cu_seqlens_q) - 1), got {tuple(cache_seqlens.shape)}")
    if block_table is not None:
        if not isinstance(block_table, torch.Tensor) or block_table.dim() != 2 or block_table.shape[0] != b:
            raise ValueError(f"block_table must have shape (batch, max_blocks_per_seq) with batch = len(cu_seqlens_q) - 1 = {b}, got {tuple(getattr(block_table, 'shape', ()))}")
    elif k_cache.dim() == 4 and k_cache.shape[0] != b:
        raise ValueError(f"k_cache / v_cache must have batch = len(cu_seqlens_q) - 1 = {b}, got {k_cache.shape[0]}")
    for name, t in (("k_descale", k_descale), ("v_descale", v_descale)):
        if isinstance(t, torch.Tensor) and t.dim() == 2 and t.shape[0] != b:
            raise ValueError(f"{name} must have shape (batch, nheads_k) with batch = len(cu_seqlens_q) - 1 = {b}, got {tuple(t.shape)}")
    return b


def flash_attn_with_kvcache(q, k_cache, v_cache, k=None, v=None, cache_seqlens=None, causal=False, num_splits=0, return_softmax_lse=False, *,
                            block_table=None, window_size=(-1, -1), k_descale=None, v_descale=None, rotary_cos=None, rotary_sin=None,
                            rotary_interleaved=True, cu_seqlens_q=None, max_seqlen_q=None, cu_seqlens_k_new=None, softmax_scale=None,
                            softcap=0.0, sinks=None, tree_mask=None, prefill=False):
    """Decode attention over a KV cache (upstream flash-attn's ``flash_attn_with_kvcache`` conventions; forward only).

    q: (batch, seqlen_q, nheads, d); k_cache, v_cache: (batch, seqlen_cache, nheads_k, d), any batch / row / head strides (used in place).
    cache_seqlens: int32 tensor (batch,) on q's device, a Python int (broadcast), or None (every sequence is seqlen_cache long).
    k, v (optional, both or neither): (batch, seqlen_new, nheads_k, d), written INTO the caches at rows cache_seqlens[i] ..
    cache_seqlens[i] + seqlen_new - 1 before attention runs over the first cache_seqlens[i] + seqlen_new keys; cache_seqlens is not
    updated (the caller advances it).  causal masks key j for query t when j > L_i - seqlen_q + t.  Scale is 1/sqrt(d) unless softmax_scale says otherwise.
    num_splits: 0 = chosen by the library, > 0 forces the key split.  Returns out (like q), and lse (batch, nheads, seqlen_q) fp32 if
    ``return_softmax_lse``.  Precondition: cache_seqlens[i] + seqlen_new <= seqlen_cache.
    Non-finite inputs follow fp32 math over the valid prefix, for every num_splits: a NaN query row, or a NaN / +inf score from a visible K row,
    gives NaN in that row's O and LSE; a row that sees no key is O = 0, LSE = 0.  Cache rows at or past L_i and heads the
    cache views skip are never read into a result.  Precondition, not checked: every finite score (q . k) * softmax_scale (* k_descale) has
    |score| * log2(e) < 2^31 (about 1.5e9, which only bf16 inputs can reach).  The kernels take exp2(s * c - fl(m * c)), whose argument carries
    the rounding residue of m * c: below the limit it is at most 64 and costs the LSE a relative 2^-24; from 2^32 on its exponential overflows
    or underflows and the row's O and LSE are unspecified (nothing is read or written out of bounds).  A row that sees a single key returns that
    V row bit for bit (over an FP8 cache: the fp32 product float(code) * v_descale rounded once to q's dtype); a V of -0 may come back as +0.

    head_dim d: 64, 128 or 256; anything else is a ValueError.  d = 256 (Gemma 2 2B / 9B, Gemma 3) exists for this call only - fwd, bwd,
    varlen_* and flash_attn_func stay at 64 / 128 - and supports everything below exactly as 128 does: the same tolerances and the same
    bit-for-bit relations.  Its attention kernels run one workgroup per compute unit (a lane holds about 400 registers) where 64 / 128 run two.

    block_table (keyword, optional): a paged cache.  k_cache, v_cache are then page pools (num_blocks, page_block_size, nheads_k, d), any
    page / row / head strides, page_block_size a multiple of 16; block_table is an int32 tensor (batch, max_blocks_per_seq) on q's device
    with a contiguous last dim: logical key j of sequence i is row j % page_block_size of page block_table[i, j // page_block_size].  The
    capacity is max_blocks_per_seq * page_block_size and takes the part of seqlen_cache above; the append writes through the table.
    Entries past the pages a sequence needs are never read.  A needed entry outside [0, num_blocks) breaks the precondition: it is
    clamped, min(uint32(entry), num_blocks - 1), so it reads (or the append writes) page num_blocks - 1 and nothing outside the pool.

    window_size (keyword, (left, right) ints >= -1): sliding-window (local) attention, upstream flash-attn's convention.  Key j of sequence i
    is visible to query t when L_i - seqlen_q + t - left <= j <= L_i - seqlen_q + t + right (and j < L_i); -1 = unbounded on that side,
    (-1, -1) = no window.  ``causal`` sets the right edge to 0 and ``right`` is then ignored: window_size=(W - 1, 0) with causal=True is the
    usual "last W keys" window.  A row that sees no key is O = 0, LSE = 0.  Lengths stay on the device and the window is a host value, so a
    windowed call needs no synchronisation and can be captured in a graph and replayed with new cache_seqlens.  A window with a left edge
    reads only the keys it can see: the split is sized from left + seqlen_q + right instead of the capacity (never more splits or workspace
    than without the window).  Cache rows below max(0, L_i - seqlen_q - left) and at or past L_i - in a paged cache, and the table entries of
    pages that lie wholly outside that range - are never read into a result.  The NaN contract above holds within the window.  Like under
    causal with seqlen_q > 1, the query rows of a call share K / V reads: the seqlen_q x (nheads / nheads_k) rows of a KV head go through the
    kernels in tiles of 16, and a non-finite V element in a row that another query row of the same tile sees, but this row does not, can make
    this row's O NaN (its weight for that row is 0, and 0 x NaN is NaN).

    8-bit cache: k_cache, v_cache of dtype ``torch.float8_e4m3fn`` (OCP e4m3; both the same), contiguous or a page pool as above, with
    k_descale, v_descale (keyword, optional): float32 tensors (batch, nheads_k) on q's device, any strides (an ``expand()``-ed scalar is
    fine), None = 1.0.  q, k, v, out stay fp16 / bf16 and lse fp32.  The call equals the 16-bit call on the dequantised cache
    ``K[i, j, g, :] = float(k_cache[i, j, g, :]) * k_descale[i, g]`` (V likewise) in exact arithmetic: the codes are widened to q's dtype
    without rounding in front of the same matrix instructions, k_descale folds into the softmax scale and v_descale into the final
    normalisation, in fp32; Q and P are never quantised.  Descales are read on the device: no synchronisation, and a captured call
    replays with the descale values (and lengths) then in memory.  Precondition, not checked: descales are finite and positive.  k / v
    rows are quantised into the cache in place, ``code = e4m3_rne(clamp(float(x) / descale, -448, 448))`` (correctly rounded fp32
    quotient, round to nearest even into the subnormals too, NaN stays NaN (0x7f / 0xff), +-inf saturate to +-448), and attention runs
    over the quantised rows - what the next call will see.  Everything above carries over: block_table (same page size rule, same
    clamping of bad entries), window_size, causal, GQA / MQA, num_splits (the split count and workspace are those of a 16-bit cache of
    the same shape), dead rows O = 0, LSE = 0, determinism per split count, and the rows, pages and heads that are never read; a NaN code
    in a visible K row makes that row's O and LSE NaN (e4m3fn has no inf); paged and contiguous calls over the same logical cache give
    the same bits.  Alignment (the kernels keep 16-byte loads): the row, head and batch / page strides of an 8-bit cache are multiples of
    16 elements and its storage offset a multiple of 16 bytes; a view that breaks this is rejected (RuntimeError), never copied.
    ``float8_e4m3fnuz``, ``float8_e5m2`` and any other cache dtype that is not q's are a ValueError, as is a descale with a 16-bit cache
    or one of the wrong dtype, shape or device.

    Rotary embedding: rotary_cos, rotary_sin (keyword, optional, both or neither): (seqlen_ro, rotary_dim / 2) tensors of q's dtype (not
    fp32) on q's device, last dim contiguous, any row stride; rotary_dim a multiple of 16 with 16 <= rotary_dim <= d (elements rotary_dim ..
    d - 1 pass through), seqlen_ro at least the cache capacity.  Only applicable if k and v are passed in (upstream's rule).  The appended
    row s of sequence i is rotated at position cache_seqlens[i] + s before it is written to the cache; query row t at cache_seqlens[i] + t if
    ``causal`` or a ``window_size`` other than (-1, -1) was passed, else every query row at cache_seqlens[i] (upstream's rule; decided from
    the arguments as passed).  rotary_interleaved (keyword, bool, default True as upstream): True pairs (x[2i], x[2i+1]) (GPT-J), False pairs
    (x[i], x[i + rotary_dim / 2]) (GPT-NeoX).  With c = cos[p, i], s = sin[p, i]: ``y_a = x_a * c - x_b * s``, ``y_b = x_b * c + x_a * s``
    in fp32 (each operation rounded on its own), rounded once to q's dtype - so the call equals, bit for bit in out, lse and every cache
    byte, the call without rotary on ``q_rot`` / ``k_rot`` computed that way with torch (v is appended as is), for the same num_splits.
    With an FP8 cache the rotated row (already in q's dtype) goes through the quantiser above.  Everything else carries over unchanged:
    block_table, window_size, causal, GQA / MQA (the query heads of a token share its position), seqlen_q > 1, dead rows, the NaN rules,
    what is never read, determinism per split count, the split count itself.  q, k, v and the tables are not written; table rows other
    than the positions used are never read, and on the device a position is clamped to seqlen_ro - 1.  The rotation is fused into the
    append launch (no extra launch, no host synchronisation: a captured call replays with the lengths then in memory); the rotated q
    passes through an image in the call's workspace.  Wrong dtype, rank, shape, device, rotary_dim or seqlen_ro, one table without the
    other, tables without k / v, or a rotary_interleaved that is not a bool: ValueError.

    Ragged query batches: cu_seqlens_q (keyword, optional): int32 tensor (batch + 1,) on q's device, contiguous, non-decreasing from 0.  q is
    then PACKED, (total_q, nheads, d): sequence i owns rows cu_seqlens_q[i] .. cu_seqlens_q[i + 1] - 1 (sq_i rows, 0 allowed), one scheduler
    step with decoding, speculating and prompt-chunk sequences as ONE call.  batch = len(cu_seqlens_q) - 1 is what cache_seqlens,
    block_table, a contiguous k_cache and the descales are checked against.  total_q may exceed cu_seqlens_q[-1]: the rows past it are
    never read and their out / lse entries are never written.  max_seqlen_q (Python int >= 1, required): precondition sq_i <=
    max_seqlen_q (a device value, not checked); it only sizes the launch and the key split, never which keys a row sees.  k, v (both or
    neither) are packed as well, (total_new, nheads_k, d), under cu_seqlens_k_new (same rules; it may be the very same tensor as
    cu_seqlens_q): sequence i appends its sn_i rows at cache rows cache_seqlens[i] .. cache_seqlens[i] + sn_i - 1 - through the table when
    paged, quantised into an FP8 cache - before attention runs; rows that would land at or past the capacity are dropped.  With L_i =
    min(max(cache_seqlens[i], 0) + sn_i, capacity), row t of sequence i sees key j < L_i; under ``causal`` only j <= L_i - sq_i + t; under
    window_size only L_i - sq_i + t - left <= j <= L_i - sq_i + t + right: the formulas above with sq_i in place of seqlen_q.  Returns
    out (total_q, nheads, d) and, with ``return_softmax_lse``, lse (nheads, total_q) fp32 (entry [head, cu_seqlens_q[i] + t]).  THE
    CONTRACT: sequence i of a ragged call equals, bit for bit in out, lse and every cache byte, the dense call on that sequence alone
    (batch 1, seqlen_q = sq_i) - for num_splits=1 always, and for a forced num_splits=n whenever both calls cut the keys at the same
    places: always without a left-bounded window, and with one for the sequences with sq_i == max_seqlen_q (the split of a windowed call
    is sized from left + max_seqlen_q + right).  Each sequence is tiled on its own (a 16-row tile never spans two sequences), and the
    launch is sized by the tokens present, not by batch x max_seqlen_q.  Everything above carries over: both cache layouts and the
    clamping of table entries, GQA / MQA, fp16 / bf16, head_dim 64 / 128 / 256, the FP8 cache and its descales, window_size, causal, num_splits,
    the NaN rules, dead rows O = 0, LSE = 0, determinism per split count, what is never read, and no host synchronisation - a captured
    call replays with the cu_seqlens, lengths, tables and descales then in memory (total_q, total_new, batch and max_seqlen_q are baked
    in).  Not supported, a ValueError: rotary_cos / rotary_sin together with cu_seqlens_q.  Also ValueErrors: cu_seqlens_k_new without
    k / v or without cu_seqlens_q, packed k without it, a 4-D q or k with cu_seqlens_q, a missing or non-positive max_seqlen_q, a
    cu_seqlens tensor of the wrong dtype, shape, device or layout, a per-sequence tensor of another batch.

    Scale and soft cap: softmax_scale (keyword, optional): None = 1/sqrt(d), computed as today; otherwise a Python real number, finite and
    > 0, rounded once to fp32: the scores are (q . k) * softmax_scale.  None and the fp32 default passed explicitly give the same bits (the
    value is the same and so are the kernels).  softcap (keyword, float, default 0.0 = off, upstream's convention): a finite value > 0 makes
    the scores ``softcap * tanh((q . k) * softmax_scale / softcap)`` (Gemma 2's logit soft-capping).  The mask - length, causal, window -
    comes after the cap, the softmax runs over the capped scores, and lse is their natural-log logsumexp.  tanh is evaluated as
    ``1 - 2 / (exp(2 x) + 1)`` with the hardware exponential and reciprocal: absolute error about 1e-7, times softcap in the score.  Both are
    host scalars baked into the call like the window: no synchronisation, and a captured call replays with them.  Everything above carries
    over for both: block_table and the clamping of table entries, GQA / MQA, fp16 / bf16, head_dim 64 / 128 / 256, window_size, causal,
    num_splits (the split count and the workspace do not depend on the two values), the FP8 cache (k_descale multiplies the score inside
    the tanh, v_descale stays in the final normalisation), rotary (a launch of its own in front of attention), cu_seqlens_q (sequence i of
    a soft-capped ragged call equals the soft-capped dense call on it alone, bit for bit, under the split rule above), paged == contiguous
    bit for bit, dead rows O = 0, LSE = 0, determinism per split count, what is never read.  Non-finite inputs: with softcap == 0 the rules
    above hold under any softmax_scale.  With softcap > 0 the contract is fp32 math on the CAPPED scores: a NaN score still makes the row's
    O and LSE NaN, but a raw score of +inf caps to +softcap - it is finite and the row is no longer NaN - and a raw score of -inf caps to
    -softcap - the key is no longer dropped.  A bool, 0, a negative value, NaN, inf or a non-number as softmax_scale, and a bool, a
    negative value, NaN, inf or a non-number as softcap: ValueError.

    Attention sinks: sinks (keyword, optional; ``sinks`` of transformers / the gpt-oss reference, ``s_aux`` of vLLM's flash-attn): a 1-D tensor
    (nheads,) on q's device, any stride, float32 or q's dtype (widened to float32 with a torch op: exact, no synchronisation,
    graph-capturable).  sinks[h] is one learned logit of QUERY head h in the units of the final scores - after softmax_scale and k_descale;
    it is never scaled.  It joins the softmax denominator and contributes no value: with the visible scores s_j of a row and
    M = max(max_j s_j, sinks[h]), in fp32 math ``out = sum_j exp(s_j - M) v_j / (sum_j exp(s_j - M) + exp(sinks[h] - M))`` and
    ``lse = M + log(sum_j exp(s_j - M) + exp(sinks[h] - M))``.  The returned LSE INCLUDES the sink, so ``exp(s_j - lse)`` are the
    probabilities actually used (they sum to less than 1; the rest sits on the sink).  The maximum covers the sink: a sink far above every
    score gives out near 0 and lse near sinks[h] without overflow, one far below gives the call without sinks.  The values are read on the
    device like the descales: no synchronisation, and a captured call replays with the sink values then in memory.  A row that sees no key
    has O = 0 and LSE = sinks[h] exactly (the sink holds all the mass); under sinks[h] = -inf it is dead as ever, O = 0, LSE = 0.
    sinks[h] = -inf for every head gives the call without sinks bit for bit, out and lse, for every num_splits.  A NaN sink makes the rows
    of its head NaN in O and LSE and leaves the other heads' bits alone; +inf breaks the precondition (unspecified result, nothing read or
    written out of bounds); the NaN / +inf score rules above are unchanged.  Everything above carries over: block_table and the clamping of
    table entries, GQA / MQA (the sink belongs to the query head), fp16 / bf16, head_dim 64 / 128, causal, window_size, num_splits (the
    split count and the workspace do not depend on sinks), the FP8 cache (k_descale does not touch the sink, v_descale stays in the final
    normalisation), softmax_scale, rotary (its own launch in front of attention), cu_seqlens_q (sequence i of a ragged sink call equals the
    dense sink call on it alone, bit for bit, under the split rule above), paged == contiguous bit for bit, determinism per split count,
    what is never read.  Not supported, a ValueError: sinks together with softcap > 0, and sinks at head_dim 256.  Also ValueErrors: a
    sinks of the wrong rank, length, device or dtype, or a non-tensor.

    Tree attention masks: tree_mask (keyword, optional; the draft trees of EAGLE / Medusa / SpecInfer, the tree-attention backend of vLLM, the
    custom mask of SGLang and FlashInfer): an int64 tensor on q's device, any strides, (batch, seqlen_q), or (total_q,) with cu_seqlens_q
    (entries past cu_seqlens_q[-1] are never read).  The sq_i query rows of sequence i are the nodes of a draft tree and the last sq_i keys
    of the sequence - in the usual call the rows just appended through k / v - are their K / V.  With base_i = L_i - sq_i, query row t sees
    key j iff 0 <= j < L_i and (j < base_i or bit j - base_i of tree_mask[i, t] is set): every node sees the whole cached prefix, and bit u
    of row t means "draft token t sees draft token u".  ``pack_tree_mask`` builds the words from a bool (sq, sq) matrix and
    ``tree_mask_from_parents`` from parent indices (ancestors plus self).  Bits at or above sq_i are ignored, and so are bits whose key
    index would be negative (L_i < sq_i).  Bit 63 is the sign bit and an ordinary bit.  Any bit pattern is legal: it need not be a tree,
    and the diagonal need not be set.  A row that sees no key is O = 0, LSE = 0, as everywhere else.  The mask is read on the device: no
    synchronisation, and a captured call replays with the mask words then in memory, like lengths and descales.  seqlen_q (ragged:
    max_seqlen_q) must be at most 64.  Two relations hold BIT FOR BIT in out and lse, for every num_splits: the lower-triangle mask (bit u
    of row t set iff u <= t) gives the causal=True call, and the mask with bits 0 .. sq - 1 all set gives the causal=False call - the tree
    kernels run the same steps over [0, L_i) and differ only in which scores they keep.  Everything above carries over: block_table and the
    clamping of table entries, GQA / MQA (the query heads of a token share its mask word), fp16 / bf16, head_dim 64 / 128, the FP8 cache
    and its descales, softmax_scale, num_splits (the split count and the workspace do not depend on the mask: they are those of the call
    without it), cu_seqlens_q (sequence i of a ragged tree call equals the dense tree call on it alone, bit for bit, under the split rule
    above), paged == contiguous bit for bit, determinism per split count, the NaN rules over the visible keys (a NaN K row that no row
    sees leaves every row finite; V rows below L_i must be finite, as under causal), and what is never read.  Not supported, a ValueError:
    tree_mask together with causal=True, with a window_size other than (-1, -1), with softcap > 0, with sinks, with rotary_cos /
    rotary_sin (a node's position is its depth, not its index: the engine rotates), at head_dim 256, and with seqlen_q / max_seqlen_q
    above 64.  Also ValueErrors: a tree_mask that is not a tensor, not int64, of the wrong rank or shape, or on another device.

    Prompt chunks: prefill (keyword, bool, default False).  By default the seqlen_q x (nheads / nheads_k) packed query rows of a KV head go
    through the kernels in tiles of 16 and every tile streams the visible K / V of its head on its own: right for decode, wrong for a chunk
    of a prompt (a 2048-token chunk at nheads / nheads_k = 4 is 512 tiles per KV head).  flash_attn_func / varlen cannot read a paged or 8-bit
    cache, take lengths from the device or append; with prefill=True the attention launch of THIS call uses kernels whose workgroup serves 64
    packed rows of one (sequence, KV head, key split): four waves of 16 rows each walk the same 32-key steps, and the K / V rows of a step
    are loaded once per workgroup into shared memory.  The append in front and the split partials and their combine behind are the same code.
    Each sequence is tiled on its own from its first packed row (a 64-row tile never spans two sequences); the automatic key split is the
    same rule evaluated with the wide grid's workgroup count, a forced num_splits cuts the keys where it cuts them with prefill=False, and
    under ``causal`` a tile reads no key past the last one its last row sees.  Supported: dense and cu_seqlens_q calls, contiguous and
    paged caches, the FP8 cache with descales (read and append side), k / v append (packed or dense), causal, GQA / MQA, fp16 / bf16,
    head_dim 64 / 128, softmax_scale, num_splits, return_softmax_lse, and graph capture - no host synchronisation: lengths, tables,
    descales and cu_seqlens are read on the device.  Values: fp32 math over the visible keys, the tolerances of the 16-row path.  The bits
    may differ from prefill=False because the summation order differs: NO bit relation between the two is promised.  Bit for bit: paged ==
    contiguous over the same logical cache; sequence i of a ragged prefill call == the dense prefill call on it alone, in out, lse and
    every cache byte, for num_splits=1 and for any forced split (there is no window, so the cuts coincide); run-to-run determinism per
    split count.  Unchanged: a row that sees no key is O = 0, LSE = 0; a NaN query row, or a NaN / +inf score, gives a NaN row; cache rows
    at or past L_i, packed rows past cu_seqlens_q[-1] and table entries of pages wholly past L_i never reach a result; a non-finite V
    element that another row of the tile sees, but this row does not, can make this row NaN (0 x NaN), as above.  prefill applies to the
    whole call: a decoding sequence in such a call fills 4 of 64 rows at nheads / nheads_k = 4.  Choosing the tile automatically, per call
    or per sequence, is out of scope (it would change the bits of existing calls).  Not supported, a ValueError that names the argument:
    prefill=True together with a window_size other than (-1, -1), with softcap > 0, with sinks, with tree_mask, with rotary_cos /
    rotary_sin, and at head_dim 256; also a prefill that is not a bool.
    """
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, k_cache, v_cache, k, v, sinks if isinstance(sinks, torch.Tensor) else None)):
        raise RuntimeError("flash_attn_with_kvcache is forward-only: run it under torch.no_grad() / torch.inference_mode() or pass tensors that do not require grad")
    if (k is None) != (v is None):
        raise ValueError("k and v must both be given or both be None")
    if cu_seqlens_q is not None:
        _check_cu_seqlens("cu_seqlens_q", cu_seqlens_q, q)
    _check_cache_dtype(q, k_cache, v_cache, k_descale, v_descale, None if cu_seqlens_q is None else cu_seqlens_q.shape[0] - 1)
    left, right = _window_pair(window_size)
    softmax_scale, softcap = _check_scale_and_cap(softmax_scale, softcap)
    # (the third overload of the extension only when one of the two is given: every other call resolves as it always did)
    extra = dict(softmax_scale=softmax_scale, softcap=softcap) if softmax_scale is not None or softcap != 0.0 else {}
    # (sinks: the extension's function of its own, which continues the third overload's arguments; every call without sinks goes where it always went)
    fwd_kvcache = _C.fwd_kvcache
    if sinks is not None:
        extra = dict(extra, sinks=_check_sinks(sinks, q, softcap))
        fwd_kvcache = _C.fwd_kvcache_sinks
    # (tree_mask: likewise a function of its own, which continues the arguments of fwd_kvcache_sinks)
    if tree_mask is not None:
        extra = dict(extra, tree_mask=_check_tree_mask(tree_mask, q, causal, (left, right), softcap, sinks, rotary_cos, rotary_sin, cu_seqlens_q, max_seqlen_q))
        fwd_kvcache = _C.fwd_kvcache_tree
    # (prefill: likewise a function of its own, which continues the arguments of fwd_kvcache_tree)
    if not isinstance(prefill, bool):
        raise ValueError(f"prefill must be a bool, got {prefill!r}")
    if prefill:
        _check_prefill(q, (left, right), softcap, sinks, tree_mask, rotary_cos, rotary_sin)
        extra = dict(extra, prefill=True)
        fwd_kvcache = _C.fwd_kvcache_prefill
    if cu_seqlens_q is None:
        if cu_seqlens_k_new is not None:
            raise ValueError("cu_seqlens_k_new given without cu_seqlens_q (packed k / v belong to a ragged call)")
        if max_seqlen_q is not None:
            raise ValueError("max_seqlen_q given without cu_seqlens_q")
        _check_rotary(q, k_cache, k, block_table, rotary_cos, rotary_sin, rotary_interleaved)
        _check_kvcache_head_dim(q)
        if isinstance(cache_seqlens, int):
            cache_seqlens = torch.full((q.shape[0],), cache_seqlens, dtype=torch.int32, device=q.device)
        out, lse = fwd_kvcache(q, k_cache, v_cache, k, v, cache_seqlens, bool(causal), int(num_splits), block_table, left, right,
                                  k_descale=k_descale, v_descale=v_descale, rotary_cos=rotary_cos, rotary_sin=rotary_sin, rotary_interleaved=rotary_interleaved, **extra)
        return (out, lse) if return_softmax_lse else out
    b = _check_ragged(q, k_cache, k, v, cache_seqlens, block_table, k_descale, v_descale, rotary_cos, rotary_sin, cu_seqlens_q, max_seqlen_q, cu_seqlens_k_new)
    _check_kvcache_head_dim(q)
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((b,), cache_seqlens, dtype=torch.int32, device=q.device)
    out, lse = fwd_kvcache(q, k_cache, v_cache, k, v, cache_seqlens, bool(causal), int(num_splits), block_table, left, right,
                              k_descale=k_descale, v_descale=v_descale, cu_seqlens_q=cu_seqlens_q, max_seqlen_q=int(max_seqlen_q),
                              cu_seqlens_k_new=cu_seqlens_k_new, **extra)
    return (out, lse) if return_softmax_lse else out


MLA_FP8_ROW_BYTES = 656     # one FP8 latent row: 512 e4m3 codes, four fp32 scales (one per 128 codes), 64 rope elements of q's dtype


def _mla_cache_is_fp8(kv_cache):
    """the FP8 latent cache of the two MLA calls: uint8 or float8_e4m3fn AND 656 bytes a row (anything else is judged as a 16-bit cache)"""
    return kv_cache.dtype in (torch.uint8, torch.float8_e4m3fn) and kv_cache.shape[-1] == MLA_FP8_ROW_BYTES


def _check_mla_fp8_view(kv_cache):
    """the kernels read and write an FP8 latent row with 16-byte accesses: a view they cannot address is refused, never copied"""
    if kv_cache.stride(3) != 1:
        raise ValueError("kv_cache: the last dimension of an FP8 latent cache must be contiguous")
    if kv_cache.stride(0) % 16 != 0 or kv_cache.stride(1) % 16 != 0 or kv_cache.stride(1) < MLA_FP8_ROW_BYTES:
        raise ValueError(f"kv_cache: the batch / page and row strides of an FP8 latent cache must be multiples of 16 bytes with rows at least 656 bytes apart, "
                         f"got strides {tuple(kv_cache.stride())}")
    if kv_cache.storage_offset() % 16 != 0 or (kv_cache.device.type != "meta" and kv_cache.data_ptr() % 16 != 0):
        raise ValueError(f"kv_cache: an FP8 latent cache must start at a multiple of 16 bytes, got storage offset {kv_cache.storage_offset()}")


def quantize_mla_kv_cache(kv):
    """(..., 576) fp16 / bf16 latent rows -> (..., 656) uint8 rows of the FP8 latent cache, by the rule of the quantising append of flash_mla_with_kvcache.

    Per 128-column tile g of the first 512 columns: amax_g = max |x| over the tile's finite elements (NaN and +-inf skipped, 0 if none),
    scale_g = max(amax_g, 2^-24) / 448 (the correctly rounded fp32 quotient), code = e4m3_rne(clamp(float(x) / scale_g, -448, 448)); NaN stays NaN with
    its sign (0x7f / 0xff), +-inf saturate to +-448.  Bytes 0 .. 511 the codes, 512 .. 527 the four fp32 scales (little endian), 528 .. 655 the 64 rope
    elements copied bit for bit.  Plain torch: runs on any device."""
    if not isinstance(kv, torch.Tensor) or kv.dtype not in (torch.float16, torch.bfloat16) or kv.dim() < 1 or kv.shape[-1] != 576:
        raise ValueError("kv must be an fp16 / bf16 tensor (..., 576)")
    lead = kv.shape[:-1]
    x = kv[..., :512].float().reshape(*lead, 4, 128)
    finite = torch.isfinite(x)
    amax = torch.where(finite, x.abs(), torch.zeros_like(x)).amax(dim=-1, keepdim=True)
    scale = torch.clamp(amax, min=2.0 ** -24) / 448.0
    y = torch.clamp(x / scale, min=-448.0, max=448.0)      # (NaN passes through clamp)
    nan = torch.isnan(y)
    codes = torch.where(nan, torch.zeros_like(y), y).to(torch.float8_e4m3fn).view(torch.uint8)
    sign = ((x.view(torch.int32) >> 24) & 0x80).to(torch.uint8)
    codes = torch.where(nan, sign | 0x7F, codes)
    out = torch.empty(*lead, MLA_FP8_ROW_BYTES, dtype=torch.uint8, device=kv.device)
    out[..., :512] = codes.reshape(*lead, 512)
    out[..., 512:528] = scale.reshape(*lead, 4).contiguous().view(torch.uint8).reshape(*lead, 16)
    out[..., 528:] = kv[..., 512:].contiguous().view(torch.uint8).reshape(*lead, 128)
    return out


def dequantize_mla_kv_cache(kv8, dtype):
    """(..., 656) uint8 / float8_e4m3fn rows of the FP8 latent cache -> (..., 576) rows of ``dtype`` (fp16 / bf16): what the MLA calls compute with.

    kv[c] = round_to_dtype(fp32(code[c]) * scale[c // 128]) for c < 512 - the fp32 product rounded once, to nearest-even - and kv[512 + r] the stored rope
    element.  flash_mla_with_kvcache / flash_mla_sparse_with_kvcache on an FP8 cache equal the same call on this tensor bit for bit.  Plain torch."""
    if not isinstance(kv8, torch.Tensor) or kv8.dtype not in (torch.uint8, torch.float8_e4m3fn) or kv8.dim() < 1 or kv8.shape[-1] != MLA_FP8_ROW_BYTES:
        raise ValueError("kv8 must be a uint8 / float8_e4m3fn tensor (..., 656)")
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"dtype must be torch.float16 or torch.bfloat16, got {dtype}")
    raw = kv8.contiguous().view(torch.uint8)
    lead = raw.shape[:-1]
    codes = raw[..., :512].contiguous().view(torch.float8_e4m3fn).float().reshape(*lead, 4, 128)
    scale = raw[..., 512:528].contiguous().view(torch.float32).reshape(*lead, 4, 1)
    out = torch.empty(*lead, 576, dtype=dtype, device=kv8.device)
    out[..., :512] = (codes * scale).to(dtype).reshape(*lead, 512)
    out[..., 512:] = raw[..., 528:].contiguous().view(dtype).reshape(*lead, 64)
    return out


# ---- argument rules the MLA decode calls and the indexer share: each is stated here once.  The exception type, the words and the place of a check in a call's
# order are part of the interface (tests and callers match on them); what differs between the calls is a parameter.

def _check_block_table(block_table, q, pool, like="q", pool_name="kv_cache", need_column=False):
    """block_table (or None) of a call whose queries are ``q`` (called ``like``) over the cache / page pool ``pool`` (called ``pool_name``); returns the capacity.
    need_column: the indexer sizes its logits by the capacity and refuses a table without columns; the MLA calls leave that to the library."""
    b = q.shape[0]
    if block_table is None:
        if pool.shape[0] != b:
            raise ValueError(f"{pool_name} batch ({pool.shape[0]}) must match {like}'s ({b})")
        return pool.shape[1]
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32:
        raise ValueError("block_table must be an int32 tensor")
    if block_table.dim() != 2 or block_table.shape[0] != b or block_table.device != q.device:
        raise ValueError(f"block_table must have shape (batch, max_blocks_per_seq) on {like}'s device")
    if pool.shape[1] < 1 or pool.shape[1] % 16 != 0:
        raise ValueError(f"page_block_size ({pool_name}.shape[1] with block_table) must be a positive multiple of 16, got {pool.shape[1]}")
    if need_column and block_table.shape[1] < 1:
        raise ValueError("block_table needs at least one column")
    return block_table.shape[1] * pool.shape[1]


def _check_cache_seqlens(cache_seqlens, b, device, like="q"):
    """cache_seqlens: an int32 tensor (batch,) on the device of the tensor called ``like``, or an int (not a bool).  Making a tensor of an int is the caller's."""
    if isinstance(cache_seqlens, bool) or not isinstance(cache_seqlens, (int, torch.Tensor)) or (
            isinstance(cache_seqlens, torch.Tensor) and (cache_seqlens.dtype != torch.int32 or cache_seqlens.shape != (b,) or cache_seqlens.device != device)):
        raise ValueError(f"cache_seqlens must be an int32 tensor (batch,) on {like}'s device or an int")


def _check_num_splits(num_splits):
    if isinstance(num_splits, bool) or not isinstance(num_splits, int) or num_splits < 0:
        raise ValueError(f"num_splits must be an int >= 0 (0 = chosen by the library), got {num_splits!r}")


def _check_mla_decode_inputs(fn, q, kv_cache, head_dim_v, block_table, kv_new=None):
    """what flash_mla_with_kvcache and flash_mla_sparse_with_kvcache (``fn``) check alike, in their order: q, head_dim_v, kv_cache (16-bit or FP8 rows) and
    block_table; returns the batch.  kv_new only counts into the forward-only check here: its own checks are the dense call's."""
    for name, t in (("q", q), ("kv_cache", kv_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be a rank-4 tensor")
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (q, kv_cache, kv_new if isinstance(kv_new, torch.Tensor) else None)):
        raise RuntimeError(f"{fn} is forward-only: run it under torch.no_grad() / torch.inference_mode() or pass tensors that do not require grad")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"q must be fp16 or bf16, got {q.dtype}")
    if q.shape[-1] != 576:
        raise ValueError(f"q must be 576 wide (512 absorbed no-rope columns, then 64 rope columns), got head_dim {q.shape[-1]}")
    if isinstance(head_dim_v, bool) or not isinstance(head_dim_v, int) or head_dim_v != 512:
        raise ValueError(f"head_dim_v must be 512, got {head_dim_v!r}")
    if q.shape[1] < 1 or q.shape[2] < 1:
        raise ValueError(f"q needs seqlen_q >= 1 and nheads >= 1, got shape {tuple(q.shape)}")
    fp8 = _mla_cache_is_fp8(kv_cache)
    if not fp8 and kv_cache.dtype != q.dtype:
        raise ValueError(f"kv_cache must have q's dtype ({q.dtype}), got {kv_cache.dtype} (an FP8 latent cache is uint8 / float8_e4m3fn rows of 656 bytes)")
    if kv_cache.shape[2] != 1:
        raise ValueError(f"kv_cache must have exactly one head (the latent row), got {kv_cache.shape[2]}")
    if not fp8 and kv_cache.shape[3] != 576:
        raise ValueError(f"kv_cache must be 576 wide, got {kv_cache.shape[3]}")
    if fp8:
        _check_mla_fp8_view(kv_cache)
    if kv_cache.device != q.device:
        raise ValueError("kv_cache must be on q's device")
    _check_block_table(block_table, q, kv_cache)
    return q.shape[0]


def flash_mla_with_kvcache(q, kv_cache, cache_seqlens, *, head_dim_v=512, kv_new=None, block_table=None, softmax_scale=None, causal=False, num_splits=0,
                           return_softmax_lse=False):
    """Multi-head latent attention (MLA) decode over a latent KV cache (DeepSeek-V2 / V3 / R1, Kimi K2; forward only).

    After weight absorption an MLA decode step is MQA over one "KV head": each key is the 576-element latent row (512 compressed-KV elements,
    then 64 rope elements) and each value is the first 512 elements of the SAME row.  The absorption matmuls and RoPE are the caller's.

    q: (batch, seqlen_q, nheads, 576) fp16 / bf16; columns 0 .. 511 the absorbed no-rope part, 512 .. 575 the rope part (RoPE applied).  nheads and
    seqlen_q are any value >= 1 (1 for decode, 2 - 4 for MTP verification).
    kv_cache: (batch, capacity, 1, 576) in q's dtype, any batch / row strides, used in place; or, with block_table (int32 (batch, max_blocks) on q's
    device, last dim contiguous), a page pool (num_blocks, page_block_size, 1, 576), page_block_size a multiple of 16, entries clamped
    min(uint32(entry), num_blocks - 1) as in flash_attn_with_kvcache.
    cache_seqlens: int32 tensor (batch,) on q's device, or a Python int (broadcast).
    FP8 latent cache: a kv_cache of dtype uint8 or float8_e4m3fn AND 656 wide - (batch, capacity, 1, 656) or a pool (num_blocks, page_block_size, 1, 656) -
    holds rows of 512 e4m3 codes, four fp32 scales (one per 128 codes) and the 64 rope elements in q's dtype (quantize_mla_kv_cache /
    dequantize_mla_kv_cache state the format).  The call equals the same call on dequantize_mla_kv_cache(kv_cache, q.dtype) BIT FOR BIT, for every
    num_splits; kv_new stays (batch, s_new, 1, 576) in q's dtype and is quantised into the cache by the rule of quantize_mla_kv_cache (whole 656-byte
    rows), attention running over the quantised rows.  Batch / page and row strides and the storage offset must be multiples of 16 bytes.  Scales are
    used as they are; precondition: every fp32(code) * scale is zero or a normal fp32 number.
    kv_new (keyword, optional): (batch, s_new, 1, 576), written INTO the cache at rows cache_seqlens[i] .. cache_seqlens[i] + s_new - 1 before
    attention runs; cache_seqlens is not updated (the caller advances it); rows at or past the capacity are dropped.
    In fp32 math over the visible keys, with L_i = cache_seqlens[i] (+ s_new): ``s_tj = (q_t . kv_j[0:576]) * softmax_scale``; key j is visible
    iff j < L_i and, under ``causal``, j <= L_i - seqlen_q + t; ``out_t = softmax_j(s_tj) @ kv_j[0:512]``.  A row that sees no key is O = 0,
    LSE = 0.  softmax_scale: None = 576 ** -0.5 rounded once to fp32 (None and that value passed explicitly give the same bits); models pass their
    own, e.g. ``192 ** -0.5 * mscale``; validated like softmax_scale of flash_attn_with_kvcache.  head_dim_v must be 512.
    Returns out (batch, seqlen_q, nheads, 512) in q's dtype and, with ``return_softmax_lse``, lse (batch, nheads, seqlen_q) fp32 (natural log).

    What carries over from flash_attn_with_kvcache: no host synchronisation (lengths and tables are read on the device: the call can be captured in
    a graph and replays with the values then in memory); a NaN in a query row, or a NaN / +inf score, makes that row's O and LSE NaN; cache rows
    at or past L_i, pages wholly past L_i and pages no sequence references never reach a result; paged and contiguous calls over the same
    logical cache give the same bits; run-to-run determinism per split count; num_splits (0 = chosen by the library over this call's grid of
    batch x ceil(seqlen_q * nheads / 64) workgroups).  As there, the query rows of a call share the reads of a key, and the value is the key: a
    non-finite element in columns 0 .. 511 of a row below L_i that ``causal`` hides from this query row but not from another row of the same
    64-row tile can make this row NaN (0 x NaN).
    Out of scope, and without a keyword here: cu_seqlens_q, window_size, softcap, sinks, tree_mask, rotary inside the call, other
    head dims, any backward.  Wrong shapes, dtypes or values are a ValueError that names the argument.
    """
    b = _check_mla_decode_inputs("flash_mla_with_kvcache", q, kv_cache, head_dim_v, block_table, kv_new)
    if kv_new is not None:
        if not isinstance(kv_new, torch.Tensor) or kv_new.dim() != 4 or kv_new.dtype != q.dtype or kv_new.device != q.device:
            raise ValueError("kv_new must be a rank-4 tensor of q's dtype on q's device")
        if kv_new.shape[0] != b or kv_new.shape[2] != 1 or kv_new.shape[3] != 576:
            raise ValueError(f"kv_new must have shape (batch, s_new, 1, 576), got {tuple(kv_new.shape)}")
    _check_cache_seqlens(cache_seqlens, b, q.device)
    softmax_scale, _ = _check_scale_and_cap(softmax_scale, 0.0)
    if not isinstance(causal, bool):
        raise ValueError(f"causal must be a bool, got {causal!r}")
    _check_num_splits(num_splits)
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((b,), cache_seqlens, dtype=torch.int32, device=q.device)
    out, lse = _C.fwd_mla_kvcache(q, kv_cache, kv_new, cache_seqlens, causal, num_splits, block_table, softmax_scale, head_dim_v)
    return (out, lse) if return_softmax_lse else out


def flash_mla_sparse_with_kvcache(q, kv_cache, cache_seqlens, indices, *, head_dim_v=512, block_table=None, softmax_scale=None, num_splits=0,
                                  return_softmax_lse=False):
    """Sparse MLA decode over a latent KV cache: each query token attends to the cache rows its own list of key positions names (DeepSeek-V3.2
    "DeepSeek Sparse Attention", the sparse call of FlashMLA; forward only).

    q, kv_cache, cache_seqlens, block_table, softmax_scale, head_dim_v, num_splits and return_softmax_lse are those of flash_mla_with_kvcache, checks
    included: q (batch, seqlen_q, nheads, 576) fp16 / bf16; kv_cache (batch, capacity, 1, 576) in q's dtype, or with block_table (int32 (batch,
    max_blocks)) a page pool (num_blocks, page_block_size, 1, 576), page_block_size a multiple of 16, entries clamped min(uint32(entry),
    num_blocks - 1); cache_seqlens an int32 tensor (batch,) or an int; softmax_scale None = 576 ** -0.5 rounded once to fp32; head_dim_v must be 512.
    indices: int32 tensor (batch, seqlen_q, topk) on q's device, last dim contiguous, any batch and row strides; topk a positive multiple of 32 (pad
    with -1).  indices[i, t, s] is a LOGICAL key position of sequence i (it goes through block_table when the cache is paged).  The list belongs to
    query token t: all heads of the token share it.
    In fp32 math, with L_i = min(max(cache_seqlens[i], 0), capacity): slot s of row (i, t) is valid iff 0 <= indices[i, t, s] < L_i; the valid slots
    form a multiset (a position listed twice counts twice; nothing is de-duplicated); ``s_ts = (q_t . kv[idx][0:576]) * softmax_scale``;
    ``out_t = softmax over the valid slots @ kv[idx][0:512]``; lse is the natural-log logsumexp over the valid slots.  A row with no valid slot is
    O = 0, LSE = 0.  The order of a list does not matter beyond rounding.  There is no ``causal``: the list is the mask.
    Returns out (batch, seqlen_q, nheads, 512) in q's dtype and, with ``return_softmax_lse``, lse (batch, nheads, seqlen_q) fp32.

    Never read (they may hold NaN or garbage): cache rows that no valid slot names, pages no valid slot reaches and their table entries; an invalid
    entry of any value (-1, >= L_i, INT_MIN, INT_MAX) reads nothing and contributes exactly nothing.  A NaN in a query row makes that row NaN; a NaN /
    +inf score of a valid slot makes the rows of that token NaN and no other token's (a workgroup never serves two tokens).  Indices, lengths and
    tables are read on the device: no host synchronisation, and a captured call replays with the indices then in memory.  Run-to-run deterministic per
    split count; paged and contiguous calls over the same logical cache give the same bits.  The list 0, 1, .., n - 1 followed by -1 gives the bits of
    the non-causal flash_mla_with_kvcache call at cache_seqlens = n with num_splits = 1 (and with a forced num_splits when topk == capacity); the same
    list cut at L_i - seqlen_q + t + 1 per token gives those of its causal call.  num_splits: 0 = chosen by the library over this call's grid of
    batch x seqlen_q x ceil(nheads / 64) workgroups; the split runs over the slots of the list in multiples of 32.
    An FP8 latent cache (uint8 / float8_e4m3fn, 656 wide: see flash_mla_with_kvcache) is read in place and gives the bits of the same call on
    dequantize_mla_kv_cache(kv_cache, q.dtype).
    Out of scope, and without a keyword here: kv_new (engines write the latent cache themselves), cu_seqlens_q, sinks, returning
    max logits, physical (pool-wide) indices, any backward.  Wrong shapes, dtypes or values are a ValueError that names the argument.
    """
    b, sq = _check_mla_decode_inputs("flash_mla_sparse_with_kvcache", q, kv_cache, head_dim_v, block_table), q.shape[1]
    _check_cache_seqlens(cache_seqlens, b, q.device)
    if not isinstance(indices, torch.Tensor) or indices.dtype != torch.int32:
        raise ValueError("indices must be an int32 tensor (batch, seqlen_q, topk)")
    if indices.dim() != 3 or indices.shape[0] != b or indices.shape[1] != sq:
        raise ValueError(f"indices must have shape (batch, seqlen_q, topk) = ({b}, {sq}, topk), got {tuple(indices.shape)}")
    if indices.shape[2] < 32 or indices.shape[2] % 32 != 0:
        raise ValueError(f"indices: topk must be a positive multiple of 32 (pad the lists with -1), got {indices.shape[2]}")
    if indices.stride(2) != 1:
        raise ValueError("indices: the last dimension must be contiguous")
    if indices.device != q.device:
        raise ValueError("indices must be on q's device")
    softmax_scale, _ = _check_scale_and_cap(softmax_scale, 0.0)
    _check_num_splits(num_splits)
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((b,), cache_seqlens, dtype=torch.int32, device=q.device)
    out, lse = _C.fwd_mla_sparse_kvcache(q, kv_cache, indices, cache_seqlens, num_splits, block_table, softmax_scale, head_dim_v)
    return (out, lse) if return_softmax_lse else out


# ---- the DeepSeek-V3.2 indexer: index logits and top-k selection in front of flash_mla_sparse_with_kvcache ----------------------------------------

def _check_indexer_lengths(cache_seqlens, b, device, like="q_idx"):
    """_check_cache_seqlens, then the tensor; unlike the MLA decode calls the indexer clamps an int to the int32 range instead of leaving one outside it to torch.full"""
    _check_cache_seqlens(cache_seqlens, b, device, like)
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((b,), max(min(cache_seqlens, 2 ** 31 - 1), -2 ** 31), dtype=torch.int32, device=device)
    return cache_seqlens


def _check_idx_cache_view(k_idx_cache, fp8):
    """the kernels read and write an index key with 16-byte accesses: a view they cannot address is refused, never copied"""
    unit = 16 if fp8 else 8
    what = "16 bytes" if fp8 else "8 elements"
    if k_idx_cache.stride(2) != 1:
        raise ValueError("k_idx_cache: the last dimension must be contiguous")
    if k_idx_cache.stride(0) % unit != 0 or k_idx_cache.stride(1) % unit != 0 or k_idx_cache.stride(1) < 128 or k_idx_cache.stride(0) < 0:
        raise ValueError(f"k_idx_cache: the batch / page and row strides must be multiples of {what} with rows at least 128 apart, got strides {tuple(k_idx_cache.stride())}")
    if k_idx_cache.storage_offset() % unit != 0 or (k_idx_cache.device.type != "meta" and k_idx_cache.data_ptr() % 16 != 0):
        raise ValueError(f"k_idx_cache must start at a multiple of {what}, got storage offset {k_idx_cache.storage_offset()}")


def _check_indexer_inputs(q_idx, weights, k_idx_cache, cache_seqlens, k_scale, block_table, causal):
    """the checks of flash_mla_indexer_logits; returns (q_idx with addressable strides, cache_seqlens as a tensor, capacity)"""
    if not isinstance(q_idx, torch.Tensor) or q_idx.dim() != 4:
        raise ValueError("q_idx must be a rank-4 tensor (batch, seqlen_q, index_heads, 128)")
    q8 = q_idx.dtype in (torch.uint8, torch.float8_e4m3fn)
    if not q8 and q_idx.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"q_idx must be fp16, bf16 or e4m3 codes (float8_e4m3fn / uint8), got {q_idx.dtype}")
    b, sq, h, d = q_idx.shape
    if d != 128:
        raise ValueError(f"q_idx must be 128 wide, got head_dim {d}")
    if h not in (16, 32, 64):
        raise ValueError(f"q_idx must have 16, 32 or 64 index heads, got {h}")
    if sq < 1:
        raise ValueError(f"q_idx needs seqlen_q >= 1, got shape {tuple(q_idx.shape)}")
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32:
        raise ValueError("weights must be a float32 tensor (batch, seqlen_q, index_heads)")
    if tuple(weights.shape) != (b, sq, h) or weights.device != q_idx.device:
        raise ValueError(f"weights must have shape (batch, seqlen_q, index_heads) = ({b}, {sq}, {h}) on q_idx's device, got {tuple(weights.shape)}")
    if not isinstance(k_idx_cache, torch.Tensor) or k_idx_cache.dim() != 3:
        raise ValueError("k_idx_cache must be a rank-3 tensor (batch, capacity, 128), or a page pool (num_blocks, page_block_size, 128) with block_table")
    fp8 = k_idx_cache.dtype in (torch.uint8, torch.float8_e4m3fn)
    if q8 and not fp8:
        raise ValueError(f"k_idx_cache must hold e4m3 codes (float8_e4m3fn / uint8) with an FP8 q_idx, got {k_idx_cache.dtype}")
    if not fp8 and k_idx_cache.dtype != q_idx.dtype:
        raise ValueError(f"k_idx_cache must have q_idx's dtype ({q_idx.dtype}) or hold e4m3 codes (float8_e4m3fn / uint8), got {k_idx_cache.dtype}")
    if k_idx_cache.shape[2] != 128:
        raise ValueError(f"k_idx_cache must be 128 wide, got {k_idx_cache.shape[2]}")
    if k_idx_cache.device != q_idx.device:
        raise ValueError("k_idx_cache must be on q_idx's device")
    _check_idx_cache_view(k_idx_cache, fp8)
    capacity = _check_block_table(block_table, q_idx, k_idx_cache, like="q_idx", pool_name="k_idx_cache", need_column=True)
    if capacity >= 2 ** 31 - 2 ** 14:
        raise ValueError(f"k_idx_cache / block_table: a capacity of {capacity} keys does not fit")
    if k_scale is not None:
        if not isinstance(k_scale, torch.Tensor) or k_scale.dtype != torch.float32:
            raise ValueError("k_scale must be a float32 tensor with one scale per cached token, or None")
        if tuple(k_scale.shape) != tuple(k_idx_cache.shape[:2]) or k_scale.device != q_idx.device:
            raise ValueError(f"k_scale must have shape {tuple(k_idx_cache.shape[:2])} (k_idx_cache without its last dimension) on q_idx's device, got {tuple(k_scale.shape)}")
        if k_scale.device.type != "meta" and k_scale.data_ptr() % 4 != 0:
            raise ValueError("k_scale must be 4-byte aligned")
    cache_seqlens = _check_indexer_lengths(cache_seqlens, b, q_idx.device)
    if not isinstance(causal, bool):
        raise ValueError(f"causal must be a bool, got {causal!r}")
    unit = 16 if q8 else 8                      # 16-byte loads: bytes of codes, or elements
    if q_idx.stride(3) != 1 or any(q_idx.stride(i) % unit != 0 for i in range(3)) or q_idx.data_ptr() % 16 != 0:
        # (a token's index queries are 16 KB, 8 KB of codes: unlike the cache they may be copied.  Codes are cloned: .contiguous() hands a contiguous tensor at
        # a misaligned address back as it is)
        q_idx = q_idx.clone(memory_format=torch.contiguous_format) if q8 else q_idx.contiguous()
    return q_idx, cache_seqlens, capacity


def flash_mla_indexer_logits(q_idx, weights, k_idx_cache, cache_seqlens, *, k_scale=None, block_table=None, causal=True):
    """Index logits of the DeepSeek-V3.2 "lightning indexer": one fp32 logit per (query token, cached key), the input of flash_mla_indexer_topk.

    q_idx: (batch, seqlen_q, index_heads, 128) fp16 / bf16, index_heads 16, 32 or 64.  RoPE and any scale of q are the caller's (fold a scale into weights).
    Or torch.float8_e4m3fn / torch.uint8 (OCP e4m3 codes) over an FP8 k_idx_cache - the dtype of q_idx says which path runs: see "FP8 q_idx" below.
    weights: (batch, seqlen_q, index_heads) float32, any strides: the learned per-head weights of the token.
    k_idx_cache: (batch, capacity, 128) in q_idx's dtype, or torch.float8_e4m3fn / torch.uint8 (OCP e4m3 codes), used in place; with block_table
    (int32 (batch, max_blocks), last dim contiguous) a page pool (num_blocks, page_block_size, 128), page_block_size a multiple of 16, entries clamped
    min(uint32(entry), num_blocks - 1).  Row and batch / page strides and the storage offset must be multiples of 16 bytes (8 elements of a 16-bit
    cache): anything else is a ValueError, never a copy.
    k_scale: None (= 1.0) or float32 (batch, capacity) / (num_blocks, page_block_size), one scale per cached token, any strided view - the values and
    the scales of one buffer laid out block by block can be passed as two views of it.
    cache_seqlens: int32 tensor (batch,) on q_idx's device, or an int.

    With L_i = min(max(cache_seqlens[i], 0), capacity), token t sees the keys j < n_t, n_t = L_i without ``causal``, else
    min(L_i, max(L_i - seqlen_q + t + 1, 0)) - the rule of flash_mla_with_kvcache.  In fp32 math, for j < n_t:
    ``logits[i, t, j] = k_scale[j] * sum_h weights[t, h] * relu(q_idx[t, h, :] . k[j, :])``, relu(x) = x > 0 ? x : 0, k the element of a 16-bit cache or
    float(code) of an FP8 one.  FP8 codes are widened exactly and multiplied with q_idx in q_idx's dtype; nothing is quantised.
    Returns logits (batch, seqlen_q, capacity) float32, freshly allocated; entries at j >= n_t are NOT written (flash_mla_indexer_topk never reads them).
    Never read, so they may hold NaN codes and NaN scales: cache rows and scales at or past L_i, pages wholly past L_i, pages no sequence references.
    Non-finite inputs have no value contract (memory safety only).  No host synchronisation: lengths, tables and scales are read on the device and
    a captured call replays with the values then in memory.  Deterministic; paged and contiguous calls over the same logical cache give the same bits.
    FP8 q_idx (quantize_mla_index_queries): k_idx_cache must hold e4m3 codes too (a 16-bit cache is a ValueError naming k_idx_cache); the per-(token, head)
    scale of the quantised queries is the caller's, folded into weights.  ``logits[i, t, j] = k_scale[j] * sum_h weights[t, h] * relu(sum_d float(qcode[t, h, d])
    * float(kcode[j, d]))``: an e4m3 x e4m3 product on v_mfma_f32_16x16x128_f8f6f4, every product exact in fp32, the order of the 128-term sum the
    instruction's; relu is the IEEE 754-2019 maximum here (a NaN code gives NaN).  A q_idx the kernels cannot address with 16-byte loads is made contiguous once.
    Out of scope: FP8 q_idx over a 16-bit cache, other head counts or widths, appending to the index cache, cu_seqlens_q.  Wrong shapes, dtypes or views are a
    ValueError that names the argument."""
    q_idx, cache_seqlens, capacity = _check_indexer_inputs(q_idx, weights, k_idx_cache, cache_seqlens, k_scale, block_table, causal)
    logits = torch.empty(q_idx.shape[0], q_idx.shape[1], capacity, dtype=torch.float32, device=q_idx.device)
    _C.mla_indexer_logits(q_idx, weights, k_idx_cache, cache_seqlens, logits, k_scale, block_table, causal)
    return logits


def _check_topk(topk):
    if isinstance(topk, bool) or not isinstance(topk, int) or topk < 32 or topk % 32 != 0:
        raise ValueError(f"topk must be a positive multiple of 32, got {topk!r}")


def flash_mla_indexer_topk(logits, cache_seqlens, topk, *, causal=True):
    """The ``indices`` of flash_mla_sparse_with_kvcache from index logits: per query token the topk visible key positions with the largest logits.

    logits: (batch, seqlen_q, capacity) float32, last dim contiguous, any batch / row strides (what flash_mla_indexer_logits returns, or a view).
    cache_seqlens, causal: as in flash_mla_indexer_logits; they give n_t, the keys token t sees.  topk: a positive multiple of 32.
    The selection is exact.  fp32 values are ordered by the integer key u(x) = bits(x) ^ (0xffffffff if the sign bit is set else 0x80000000): -0 < +0,
    and a NaN with the sign bit clear is above +inf.  Row (i, t): if n_t <= topk it is 0, 1, .., n_t - 1 followed by -1; otherwise the topk
    positions below n_t with the largest keys, ties at the threshold going to the lower positions, in ascending position order.  Entries at
    j >= n_t are never read.  Returns indices (batch, seqlen_q, topk) int32, contiguous.  No host synchronisation; deterministic."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 3 or logits.dtype != torch.float32:
        raise ValueError("logits must be a float32 tensor (batch, seqlen_q, capacity)")
    if logits.shape[1] < 1:
        raise ValueError(f"logits needs seqlen_q >= 1, got shape {tuple(logits.shape)}")
    if logits.shape[2] > 1 and logits.stride(2) != 1:
        raise ValueError("logits: the last dimension must be contiguous")
    if logits.stride(0) < 0 or logits.stride(1) < 0:
        raise ValueError("logits: strides must not be negative")
    _check_topk(topk)
    cache_seqlens = _check_indexer_lengths(cache_seqlens, logits.shape[0], logits.device, like="logits")
    if not isinstance(causal, bool):
        raise ValueError(f"causal must be a bool, got {causal!r}")
    indices = torch.empty(logits.shape[0], logits.shape[1], topk, dtype=torch.int32, device=logits.device)
    _C.mla_indexer_topk(logits, cache_seqlens, indices, causal)
    return indices


def flash_mla_index_with_kvcache(q_idx, weights, k_idx_cache, cache_seqlens, topk, *, k_scale=None, block_table=None, causal=True, return_logits=False):
    """flash_mla_indexer_logits followed by flash_mla_indexer_topk over a logits buffer allocated here: two launches, the bits of the two calls in
    sequence.  Returns indices (batch, seqlen_q, topk) int32 - what flash_mla_sparse_with_kvcache takes as it is - and, with ``return_logits``, the
    logits (batch, seqlen_q, capacity) float32 as well."""
    _check_topk(topk)
    q_idx, cache_seqlens, capacity = _check_indexer_inputs(q_idx, weights, k_idx_cache, cache_seqlens, k_scale, block_table, causal)
    logits = torch.empty(q_idx.shape[0], q_idx.shape[1], capacity, dtype=torch.float32, device=q_idx.device)
    _C.mla_indexer_logits(q_idx, weights, k_idx_cache, cache_seqlens, logits, k_scale, block_table, causal)
    indices = torch.empty(q_idx.shape[0], q_idx.shape[1], topk, dtype=torch.int32, device=q_idx.device)
    _C.mla_indexer_topk(logits, cache_seqlens, indices, causal)
    return (indices, logits) if return_logits else indices


def flash_mla_indexer_prefill_logits(q_idx, weights, k_idx_cache, cache_seqlens, *, k_scale=None, block_table=None, causal=True):
    """flash_mla_indexer_logits for a prompt chunk: the same arguments, checks and refusals, and the same bits in the same entries (with a 16-bit q_idx a NaN key
    below L_i alone differs: it gives NaN in its column for the tokens that see it, where flash_mla_indexer_logits leaves 0; with an FP8 q_idx both give NaN).

    flash_mla_indexer_logits gives a workgroup one token, which loads and widens the visible index-key cache once per token of the chunk.  Here a
    workgroup serves a tile of consecutive tokens of one sequence (4 or 8: capi.mla_indexer_prefill_launch) and stages each 32-key step once for all of
    them.  ``seqlen_q`` is any value >= 1; at seqlen_q = 1 the decode call is the one to use.
    Returns logits (batch, seqlen_q, capacity) float32, freshly allocated; entries at j >= n_t are NOT written.  Never read, so they may hold NaN codes
    and NaN scales: cache rows and scales at or past L_i, pages wholly past L_i, pages no sequence references, and keys at or past the n_t of a tile's
    last token.  No workspace, no atomics, no host synchronisation: a captured call replays with the lengths, tables and scales then in memory.
    Deterministic."""
    q_idx, cache_seqlens, capacity = _check_indexer_inputs(q_idx, weights, k_idx_cache, cache_seqlens, k_scale, block_table, causal)
    logits = torch.empty(q_idx.shape[0], q_idx.shape[1], capacity, dtype=torch.float32, device=q_idx.device)
    _C.mla_indexer_prefill_logits(q_idx, weights, k_idx_cache, cache_seqlens, logits, k_scale, block_table, causal)
    return logits


def flash_mla_index_prefill_with_kvcache(q_idx, weights, k_idx_cache, cache_seqlens, topk, *, k_scale=None, block_table=None, causal=True, return_logits=False):
    """flash_mla_index_with_kvcache for a prompt chunk: flash_mla_indexer_prefill_logits followed by flash_mla_indexer_topk over a logits buffer allocated
    here.  Two launches; the indices (and logits) of flash_mla_index_with_kvcache, entry for entry."""
    _check_topk(topk)
    q_idx, cache_seqlens, capacity = _check_indexer_inputs(q_idx, weights, k_idx_cache, cache_seqlens, k_scale, block_table, causal)
    logits = torch.empty(q_idx.shape[0], q_idx.shape[1], capacity, dtype=torch.float32, device=q_idx.device)
    _C.mla_indexer_prefill_logits(q_idx, weights, k_idx_cache, cache_seqlens, logits, k_scale, block_table, causal)
    indices = torch.empty(q_idx.shape[0], q_idx.shape[1], topk, dtype=torch.int32, device=q_idx.device)
    _C.mla_indexer_topk(logits, cache_seqlens, indices, causal)
    return (indices, logits) if return_logits else indices


def _check_prefill_view(name, t):
    """a tensor the prefill kernels address as it is: the last dimension contiguous, every other stride and the storage offset a multiple of 8 elements"""
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: the last dimension must be contiguous, got strides {tuple(t.stride())}")
    if any(s % 8 != 0 for s in t.stride()[:-1]) or t.storage_offset() % 8 != 0:
        raise ValueError(f"{name}: strides {tuple(t.stride())} (but the last) and the storage offset {t.storage_offset()} must be multiples of 8 elements "
                         "(16-byte loads); the view is not copied")


def flash_mla_prefill_func(q, k, v, *, cu_seqlens_q=None, cu_seqlens_k=None, softmax_scale=None, causal=False, return_softmax_lse=False):
    """MLA prefill attention (DeepSeek-V2 / V3 / R1, Kimi K2; the raw forward): multi-head attention with 192-wide queries and keys and 128-wide values.

    Before weight absorption an MLA layer is ordinary multi-head attention whose q / k rows are 128 no-rope columns followed by 64 rope columns (RoPE
    applied by the caller) and whose v rows are 128 wide.  This is the prompt side of flash_mla_with_kvcache.

    dense:  q (batch, seqlen_q, nheads, 192), k (batch, seqlen_k, nheads_k, 192), v (batch, seqlen_k, nheads_k, 128)
            -> out (batch, seqlen_q, nheads, 128) and, with ``return_softmax_lse``, lse (batch, nheads, seqlen_q) fp32 (natural log).
    packed: q (total_q, nheads, 192), k (total_k, nheads_k, 192), v (total_k, nheads_k, 128) with cu_seqlens_q / cu_seqlens_k, int32 (batch + 1,) on
            q's device, given both or neither -> out (total_q, nheads, 128), lse (nheads, total_q).  Sequence i owns rows cu_seqlens_q[i] ..
            cu_seqlens_q[i + 1] - 1 of q and cu_seqlens_k[i] .. cu_seqlens_k[i + 1] - 1 of k / v.  There is no max_seqlen argument: the launch is
            sized from total_q.  Rows of out / lse at or past cu_seqlens_q[-1] are not written (they hold whatever the allocation held).
    fp16 / bf16, one dtype for all three; nheads % nheads_k == 0 (GQA / MQA).  The last dimension is contiguous, every other stride and the storage
    offset are multiples of 8 elements; other views are refused, never copied.  One sequence (packed: the whole tensor) spans less than 2^31 bytes,
    the limit of flash_attn_func.

    In fp32 math over the visible keys, per sequence with sq_i rows and sk_i keys: ``s_tj = (q_t . k_j) * softmax_scale``; key j is visible to row t
    iff j < sk_i and, under ``causal``, j <= sk_i - sq_i + t (bottom-right aligned); ``out_t = softmax_j(s_tj) @ v_j``.  A row that sees no key
    (sq_i > sk_i under causal, sk_i = 0) is O = 0, LSE = 0; empty query sequences are allowed.  A NaN in a query row, or a NaN / +inf score, makes
    that row's O and LSE NaN; a -inf score only drops the key.  Non-finite V has no contract: the rows of a 64-row tile share the reads of a key, so
    a non-finite V row that ``causal`` hides from this query row but not from another row of the tile can make this row NaN (0 x NaN).
    softmax_scale: None = 192 ** -0.5 rounded once to fp32 (None and that value passed explicitly give the same bits); validated like softmax_scale
    of flash_mla_with_kvcache.

    No host synchronisation (cu_seqlens are read on the device: the call can be captured in a graph and replays with the values then in memory), no
    key split, so no workspace, and the call is deterministic.  Bit for bit: sequence i of a packed call equals the dense call on that sequence
    alone (out and lse), a batch entry of a dense call equals the call on it alone, and a power of two moved between q and softmax_scale changes
    nothing.  Chunked prefill over a cached prefix is flash_mla_chunked_prefill_func: the context part with causal=False, the new tokens with
    causal=True, and flash_attn_merge_states of the two results.
    The backward is flash_mla_prefill_bwd, the differentiable function flash_mla_attn_func.
    Out of scope, and without a keyword here: FP8 or paged inputs, other widths, window_size, softcap, sinks, a key split.  Wrong shapes,
    dtypes, views or values are a ValueError that names the argument.
    """
    softmax_scale = _check_mla_prefill_args(q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal, forward_only=True)
    out, lse = _C.fwd_mla_prefill(q, k, v, cu_seqlens_q, cu_seqlens_k, causal, softmax_scale)
    return (out, lse) if return_softmax_lse else out


def _check_mla_prefill_args(q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal, forward_only=False):
    """the argument checks of flash_mla_prefill_func, shared with its backward and with flash_mla_attn_func; returns softmax_scale as the extension takes it"""
    packed = cu_seqlens_q is not None or cu_seqlens_k is not None
    if packed and (cu_seqlens_q is None or cu_seqlens_k is None):
        raise ValueError("cu_seqlens_q and cu_seqlens_k come both or neither, got only " + ("cu_seqlens_q" if cu_seqlens_k is None else "cu_seqlens_k"))
    rank = 3 if packed else 4
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dim() != rank:
            raise ValueError(f"{name} must be a rank-{rank} tensor ({'(total, nheads, head_dim) with cu_seqlens' if packed else '(batch, seqlen, nheads, head_dim)'})")
    if forward_only and torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        bad = next(n for n, t in (("q", q), ("k", k), ("v", v)) if t.requires_grad)
        raise ValueError(f"{bad} requires grad: flash_mla_prefill_func is forward-only (the differentiable function is flash_mla_attn_func); run it under "
                         "torch.no_grad() or detach the inputs")
    if q.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"q must be fp16 or bf16, got {q.dtype}")
    for name, t in (("k", k), ("v", v)):
        if t.dtype != q.dtype:
            raise ValueError(f"{name} must have q's dtype ({q.dtype}), got {t.dtype}")
        if t.device != q.device:
            raise ValueError(f"{name} must be on q's device ({q.device}), got {t.device}")
    if q.shape[-1] != 192:
        raise ValueError(f"q must be 192 wide (128 no-rope columns, then 64 rope columns), got head_dim {q.shape[-1]}")
    if k.shape[-1] != 192:
        raise ValueError(f"k must be 192 wide (128 no-rope columns, then 64 rope columns), got head_dim {k.shape[-1]}")
    if v.shape[-1] != 128:
        raise ValueError(f"v must be 128 wide, got head_dim {v.shape[-1]}")
    if k.shape[:-1] != v.shape[:-1]:
        raise ValueError(f"k and v must agree in every dimension but the last, got {tuple(k.shape)} and {tuple(v.shape)}")
    if not packed and k.shape[0] != q.shape[0]:
        raise ValueError(f"k / v batch ({k.shape[0]}) must match q's ({q.shape[0]})")
    h, h_k = q.shape[-2], k.shape[-2]
    if h < 1 or h_k < 1 or h % h_k != 0:
        raise ValueError(f"nheads of q ({h}) must be a positive multiple of nheads_k of k / v ({h_k})")
    for name, t in (("q", q), ("k", k), ("v", v)):
        _check_prefill_view(name, t)
    if packed:
        _check_cu_seqlens("cu_seqlens_q", cu_seqlens_q, q)
        _check_cu_seqlens("cu_seqlens_k", cu_seqlens_k, q, batch=cu_seqlens_q.shape[0] - 1)
    softmax_scale, _ = _check_scale_and_cap(softmax_scale, 0.0)
    if not isinstance(causal, bool):
        raise ValueError(f"causal must be a bool, got {causal!r}")
    return softmax_scale


def _check_prefill_rows(name, t):
    """the rest of the rule for the backward's dout and out: the row stride (of the sequence dimension) is at least the row's width, as the library asks of
    every tensor - an expanded tensor (row stride 0) is refused here and not in the extension"""
    if t.stride(-3) < t.shape[-1] or any(s < 0 for s in t.stride()):
        raise ValueError(f"{name}: the row stride must be at least the row width {t.shape[-1]} and no stride negative, got strides {tuple(t.stride())} "
                         "(an expanded tensor?); the view is not copied")


def flash_mla_prefill_bwd(dout, q, k, v, out, lse, *, cu_seqlens_q=None, cu_seqlens_k=None, softmax_scale=None, causal=False):
    """The backward of flash_mla_prefill_func, raw (no autograd): (dq, dk, dv) from dout, the forward's inputs and its out and lse.

    q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal: exactly the forward's arguments, with the forward's checks.  ``out`` and ``dout`` are
    shaped like the forward's out ((batch, seqlen_q, nheads, 128) or (total_q, nheads, 128)), of q's dtype, under the same view rule as q / k / v (last
    dimension contiguous, every other stride and the storage offset multiples of 8 elements; refused, never copied) and with a row stride of at least 128
    (an expanded tensor is refused).  ``lse`` is the forward's: fp32,
    contiguous, (batch, nheads, seqlen_q) or (nheads, total_q).  Returns dq, dk, dv, contiguous and shaped like q, k, v.

    In fp32 math over the visible pairs (visibility exactly the forward's): P_tj = exp(s_tj - lse_t), exactly 0 on hidden pairs; D_t = sum_c dout_tc out_tc;
    dS = P (dout_t . v_j - D_t); dq_t = softmax_scale sum_j dS_tj k_j; dk_j = softmax_scale x the sum over the nheads / nheads_k heads of the group and over t
    of dS_tj q_t; dv_j = the same sum of P_tj dout_t.  fp32 accumulation, every output rounded once; P and dS are rounded to the dtype in front of their second
    matrix products.  A row that sees no key gets dq = 0, a key no row sees dk = dv = 0, both written; empty sequences on either side are allowed.  Packed
    rows of dq at or past cu_seqlens_q[-1] and of dk / dv at or past cu_seqlens_k[-1] are not written.  Non-finite inputs have no value contract.

    Two launches on the current stream (dq, then dk / dv), no atomics, no key or head split, no workspace besides D, no host synchronisation: graph-
    capturable and deterministic.  Bit for bit: sequence i of a packed call equals the dense call on it alone, and a batch entry the call on it alone.
    Out of scope: a head-group or key split with a workspace, other widths, window_size, softcap, sinks, FP8 or paged inputs, a fused single-kernel backward.
    """
    softmax_scale = _check_mla_prefill_args(q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal)
    o_shape = tuple(q.shape[:-1]) + (128,)
    for name, t in (("dout", dout), ("out", out)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != o_shape:
            raise ValueError(f"{name} must be a tensor shaped like the forward's out {o_shape}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if t.dtype != q.dtype:
            raise ValueError(f"{name} must have q's dtype ({q.dtype}), got {t.dtype}")
        if t.device != q.device:
            raise ValueError(f"{name} must be on q's device ({q.device}), got {t.device}")
        _check_prefill_view(name, t)
        _check_prefill_rows(name, t)
    l_shape = (q.shape[-2], q.shape[0]) if q.dim() == 3 else (q.shape[0], q.shape[2], q.shape[1])
    if not isinstance(lse, torch.Tensor) or lse.dtype != torch.float32 or tuple(lse.shape) != l_shape or not lse.is_contiguous() or lse.device != q.device:
        raise ValueError(f"lse must be the forward's lse: a contiguous float32 tensor {l_shape} on q's device")
    dq, dk, dv, _ = _C.bwd_mla_prefill(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, causal, softmax_scale)
    return dq, dk, dv


class _FlashMlaAttn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal):
        out, lse = _C.fwd_mla_prefill(q, k, v, cu_seqlens_q, cu_seqlens_k, causal, softmax_scale)
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k)
        ctx.softmax_scale, ctx.causal = softmax_scale, causal
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    def backward(ctx, dout, _dlse):
        q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k = ctx.saved_tensors
        # a dout the kernels can address is used as it is; any other view is made contiguous once
        # (autograd hands over expanded gradients as they are: the dout of out.sum(dim=1) has a row stride of 0, which no kernel addresses)
        if (dout.stride(-1) != 1 or any(s % 8 != 0 for s in dout.stride()[:-1]) or dout.storage_offset() % 8 != 0 or dout.stride(-3) < dout.shape[-1]
                or any(s < 0 for s in dout.stride())):
            dout = dout.contiguous()
        dq, dk, dv, _ = _C.bwd_mla_prefill(dout, q, k, v, out, lse, cu_seqlens_q, cu_seqlens_k, ctx.causal, ctx.softmax_scale)
        return dq, dk, dv, None, None, None, None


def flash_mla_attn_func(q, k, v, *, cu_seqlens_q=None, cu_seqlens_k=None, softmax_scale=None, causal=False, return_softmax_lse=False):
    """flash_mla_prefill_func, differentiable: the training forward of an MLA layer (192-wide q / k, 128-wide v; dense, or packed with cu_seqlens).

    Arguments, checks, values and bits are flash_mla_prefill_func's (without grad the two are the same call).  With grad enabled the result is an autograd
    node over flash_mla_prefill_func and flash_mla_prefill_bwd: gradients flow to q, k and v and to nothing else; ``lse`` (with ``return_softmax_lse``)
    is returned non-differentiable.  A non-contiguous ``dout`` whose last dimension is contiguous, whose other strides and storage offset are multiples
    of 8 elements and whose row stride is at least 128 is used as it is; any other - the expanded gradient of ``out.sum(dim=1)``, whose row stride is 0,
    included - is made contiguous once, the only copy this function makes.  See flash_mla_prefill_bwd for the math, the
    rounding points and what is out of scope.
    """
    softmax_scale = _check_mla_prefill_args(q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        out, lse = _FlashMlaAttn.apply(q, k, v, cu_seqlens_q, cu_seqlens_k, softmax_scale, causal)
    else:
        out, lse = _C.fwd_mla_prefill(q, k, v, cu_seqlens_q, cu_seqlens_k, causal, softmax_scale)
    return (out, lse) if return_softmax_lse else out


MERGE_MAX_PARTS = 8             # FA_MERGE_MAX_PARTS of the C ABI
MERGE_WIDTHS = (64, 128, 256, 512)


def flash_attn_merge_states(outs, lses):
    """Merge partial attention states: 2 .. 8 results ``(out_i, lse_i)`` of attention calls over DISJOINT key sets of the same query rows -> the result over the
    union of the keys (vLLM's ``merge_attn_states``, FlashInfer's ``merge_state``).  Forward only.

    dense:  outs[i] (batch, seqlen_q, nheads, d_v), lses[i] (batch, nheads, seqlen_q) -> out (batch, seqlen_q, nheads, d_v), lse (batch, nheads, seqlen_q)
    packed: outs[i] (total, nheads, d_v),           lses[i] (nheads, total)           -> out (total, nheads, d_v),           lse (nheads, total)
    outs: fp16 or bf16, one dtype, shape and device for all; d_v 64, 128, 256 or 512; the last dimension contiguous, every other stride and the storage offset
    multiples of 8 elements, each part with strides of its own.  lses: float32 (natural log), ANY strides - the LSE ``(1, nheads, batch * seqlen_q)`` of a call
    that took all query rows as one sequence is passed as its ``(batch, nheads, seqlen_q)`` view.  Views are used in place; a view the kernel cannot address is
    a ValueError that names the argument, never a copy.  out and lse are new contiguous tensors.

    In fp32 over the NON-EMPTY parts of a (row, head), in argument order: ``m = max_i lse_i``, ``w_i = exp(lse_i - m)``,
    ``out = (sum_i w_i out_i) / (sum_i w_i)`` rounded once to the dtype, ``lse = m + log(sum_i w_i)``.

    EMPTY - the one rule, used by every function built on this one: part i is empty for a (row, head) iff ``lse_i`` is -inf, or ``lse_i`` is +-0 and every
    element of that ``out_i`` row is +-0.  The second form is what every attention call of this library returns for a row that sees no key (O = 0, LSE = 0).
    Caveat: a LIVE row looks like that only when its scores sum to exactly one (lse = 0) and its V rows are all zero; it is then taken as empty, and the
    merged lse lacks its weight.  An empty part contributes nothing.  All parts empty gives out = 0, lse = 0 - the library's dead row again, so a merged state
    can feed another merge.  A part merged with empty parts, in any argument position, comes back bit for bit.  A NaN ``lse_i``, or a NaN in a non-empty
    part's row, makes that (row, head) NaN in out and lse and no other; ``lse_i`` = +inf has no contract.

    One launch on the current stream, no workspace, no atomics, no host synchronisation: deterministic and graph-capturable.  Nothing between the rows, heads
    and batch entries that the strides skip is read.  Out of scope: more than 8 parts in one call (merge the merges), parts of different dtypes, fp32 parts,
    a backward.  Wrong counts, shapes, dtypes, devices or views are a ValueError; a CPU call is refused by the extension (there is no fall-back).
    """
    for name, seq in (("outs", outs), ("lses", lses)):
        if not isinstance(seq, (list, tuple)) or not all(isinstance(t, torch.Tensor) for t in seq):
            raise ValueError(f"{name} must be a list or tuple of tensors")
    if not 2 <= len(outs) <= MERGE_MAX_PARTS:
        raise ValueError(f"outs must hold 2 .. {MERGE_MAX_PARTS} parts, got {len(outs)}")
    if len(lses) != len(outs):
        raise ValueError(f"lses must hold as many tensors as outs ({len(outs)}), got {len(lses)}")
    o0 = outs[0]
    if o0.dim() not in (3, 4):
        raise ValueError(f"outs[0] must be (batch, seqlen_q, nheads, d_v) or packed (total, nheads, d_v), got shape {tuple(o0.shape)}")
    if o0.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"outs[0] must be fp16 or bf16, got {o0.dtype}")
    if o0.shape[-1] not in MERGE_WIDTHS:
        raise ValueError(f"outs[0]: d_v must be one of {MERGE_WIDTHS}, got {o0.shape[-1]}")
    l_shape = (o0.shape[1], o0.shape[0]) if o0.dim() == 3 else (o0.shape[0], o0.shape[2], o0.shape[1])
    for i, (o, l) in enumerate(zip(outs, lses)):
        if tuple(o.shape) != tuple(o0.shape):
            raise ValueError(f"outs[{i}] must have the shape of outs[0] {tuple(o0.shape)}, got {tuple(o.shape)}")
        if o.dtype != o0.dtype:
            raise ValueError(f"outs[{i}] must have the dtype of outs[0] ({o0.dtype}), got {o.dtype}")
        if o.device != o0.device:
            raise ValueError(f"outs[{i}] must be on the device of outs[0] ({o0.device}), got {o.device}")
        if l.dtype != torch.float32:
            raise ValueError(f"lses[{i}] must be float32, got {l.dtype}")
        if tuple(l.shape) != l_shape:
            raise ValueError(f"lses[{i}] must have shape {l_shape} ({'(nheads, total)' if o0.dim() == 3 else '(batch, nheads, seqlen_q)'}), got {tuple(l.shape)}")
        if l.device != o0.device:
            raise ValueError(f"lses[{i}] must be on the device of outs[0] ({o0.device}), got {l.device}")
        _check_prefill_view(f"outs[{i}]", o)
        if torch.is_grad_enabled() and (o.requires_grad or l.requires_grad):
            raise ValueError(f"{'outs' if o.requires_grad else 'lses'}[{i}] requires grad: flash_attn_merge_states is forward-only; run it under torch.no_grad() or detach "
                             "the inputs")
    out, lse = _C.merge_states(list(outs), list(lses))
    return out, lse


def flash_attn_with_shared_prefix(q, k_cache, v_cache, shared_prefix_len, k=None, v=None, cache_seqlens=None, *, block_table=None, causal=False,
                                  softmax_scale=None, k_descale=None, v_descale=None, return_softmax_lse=False):
    """``flash_attn_with_kvcache`` for a batch whose sequences all start with the same ``shared_prefix_len`` cached keys (a system prompt; cascade attention
    in vLLM and FlashInfer): the prefix is read ONCE for the whole batch instead of once per sequence.  Forward only.

    Semantics: exactly those of ``flash_attn_with_kvcache(q, k_cache, v_cache, k, v, cache_seqlens, causal=causal, block_table=block_table,
    softmax_scale=softmax_scale, k_descale=k_descale, v_descale=v_descale)`` - which keys a row sees, the append of k / v, dead rows O = 0, LSE = 0, the NaN
    rules.  The values agree to rounding, not bit for bit: the parts are rounded to q's dtype before they are merged (at most one more half ulp of the
    largest part).  q is dense, (batch, seqlen_q, nheads, d); cache_seqlens an int32 tensor, an int or None as there.

    Preconditions, NOT checked (device values): the first ``shared_prefix_len`` keys of every sequence are the same physical rows - paged: the first
    ``shared_prefix_len / page_block_size`` block_table entries of every sequence are equal; contiguous: batch entry 0's first rows stand for all -;
    ``cache_seqlens[i] >= shared_prefix_len``; with an FP8 cache the descales of all sequences are equal.  Row 0 (of the table, the cache, the descales) is
    what is read for the prefix.
    Refused (ValueError): a shared_prefix_len that is not a Python int >= 0, not a multiple of page_block_size (paged) or of 16 (contiguous), or not below the
    capacity; an int cache_seqlens below it; a q whose batch stride is not seqlen_q x its row stride (the batch must flatten into one row dimension).
    shared_prefix_len = 0 is the plain call, bit for bit.

    How: three launches on the current stream, no host synchronisation (graph-capturable; lengths, tables and descales are read on the device).  (a) the
    prefix part: flash_attn_with_kvcache on q viewed as (1, batch * seqlen_q, nheads, d) over the first keys of row 0, causal=False, on the 64-row kernels
    (prefill=True) when batch * seqlen_q * nheads / nheads_k >= 64 and d != 256, else on the 16-row kernels.  (b) the suffix part: flash_attn_with_kvcache
    over ``block_table[:, Ls / page_block_size:]`` (contiguous: ``k_cache[:, Ls:]``) with ``cache_seqlens - Ls``, the caller's causal and the append.  (c)
    flash_attn_merge_states of the two, the LSE of (a) passed as a strided view; a sequence without a suffix has dead suffix rows, which the merge's
    emptiness rule leaves out.  Under ``causal`` with seqlen_q > 1 the earlier rows of a sequence may not see the last seqlen_q - 1 keys, which can lie in
    the prefix when the suffix is shorter than that: the split point Ls is therefore shared_prefix_len lowered by seqlen_q - 1 rounded up to the page (16
    rows), so every key (a) serves is visible to every row; if nothing is left, the plain call runs.  For seqlen_q = 1 Ls is shared_prefix_len.

    Supported: fp16 / bf16, head_dim 64 / 128 / 256, GQA / MQA, both cache layouts, the FP8 cache, the k / v append.  Out of scope, and without a keyword
    here: window_size, rotary, sinks, tree_mask, cu_seqlens_q, softcap, num_splits, several prefix levels.  It pays for long prefixes and large batches and
    loses to the plain call for short ones (three launches against one; README.md has the measured table).
    """
    if isinstance(shared_prefix_len, bool) or not isinstance(shared_prefix_len, int) or shared_prefix_len < 0:
        raise ValueError(f"shared_prefix_len must be a Python int >= 0, got {shared_prefix_len!r}")
    if not isinstance(causal, bool):
        raise ValueError(f"causal must be a bool, got {causal!r}")
    if (k is None) != (v is None):
        raise ValueError("k and v must both be given or both be None")
    plain = dict(causal=causal, block_table=block_table, softmax_scale=softmax_scale, k_descale=k_descale, v_descale=v_descale)
    if shared_prefix_len == 0:
        return flash_attn_with_kvcache(q, k_cache, v_cache, k, v, cache_seqlens, return_softmax_lse=return_softmax_lse, **plain)
    for name, t in (("q", q), ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError(f"{name} must be a rank-4 tensor")
    if block_table is not None and (not isinstance(block_table, torch.Tensor) or block_table.dim() != 2):
        raise ValueError("block_table must be a rank-2 int32 tensor (batch, max_blocks_per_seq)")
    granule = k_cache.shape[1] if block_table is not None else 16
    capacity = k_cache.shape[1] * (block_table.shape[1] if block_table is not None else 1)
    if granule < 1 or shared_prefix_len % granule != 0:
        raise ValueError(f"shared_prefix_len ({shared_prefix_len}) must be a multiple of " + (f"page_block_size ({granule})" if block_table is not None else "16"))
    if shared_prefix_len >= capacity:
        raise ValueError(f"shared_prefix_len ({shared_prefix_len}) must be below the cache capacity ({capacity}): nothing would be left for a suffix")
    if isinstance(cache_seqlens, int) and not isinstance(cache_seqlens, bool) and cache_seqlens < shared_prefix_len:
        raise ValueError(f"cache_seqlens ({cache_seqlens}) must be at least shared_prefix_len ({shared_prefix_len})")
    b, sq, h, d = q.shape
    if b > 1 and sq > 1 and q.stride(0) != sq * q.stride(1):
        raise ValueError(f"q: the batch stride ({q.stride(0)}) must be seqlen_q ({sq}) x the row stride ({q.stride(1)}) - the prefix part takes the "
                         "batch * seqlen_q query rows as one sequence; the view is not copied")
    # under causal the last seqlen_q - 1 keys are not visible to every row: they stay with the suffix part
    hold_back = -(-(sq - 1) // granule) * granule if causal else 0
    ls = shared_prefix_len - hold_back
    if ls <= 0:
        return flash_attn_with_kvcache(q, k_cache, v_cache, k, v, cache_seqlens, return_softmax_lse=return_softmax_lse, **plain)
    h_k = k_cache.shape[2]
    row_stride = q.stride(1) if sq > 1 else q.stride(0)
    q_rows = q.as_strided((1, b * sq, h, d), (b * sq * row_stride, row_stride, q.stride(2), q.stride(3)))
    descale_a = dict(k_descale=None if k_descale is None else k_descale[:1], v_descale=None if v_descale is None else v_descale[:1])
    wide = h_k > 0 and h % h_k == 0 and b * sq * (h // h_k) >= 64 and d != 256
    if block_table is not None:
        pages = ls // granule
        cache_a = dict(block_table=block_table[:1, :pages])
        ka, va = k_cache, v_cache
        kb, vb, cache_b = k_cache, v_cache, dict(block_table=block_table[:, pages:])
    else:
        cache_a, cache_b = {}, {}
        ka, va = k_cache[:1, :ls], v_cache[:1, :ls]
        kb, vb = k_cache[:, ls:], v_cache[:, ls:]
    # (a) every query row of the batch over the shared keys, read once: cache_seqlens=None is "the whole capacity", which is exactly the ls keys of the view
    out_a, lse_a = flash_attn_with_kvcache(q_rows, ka, va, None, None, None, causal=False, return_softmax_lse=True, softmax_scale=softmax_scale, prefill=wide,
                                           **cache_a, **descale_a)
    # (b) each sequence over its own keys
    if isinstance(cache_seqlens, torch.Tensor):
        seqlens_b = cache_seqlens - ls
    else:
        seqlens_b = None if cache_seqlens is None else cache_seqlens - ls
    out_b, lse_b = flash_attn_with_kvcache(q, kb, vb, k, v, seqlens_b, causal=causal, return_softmax_lse=True, softmax_scale=softmax_scale, k_descale=k_descale,
                                           v_descale=v_descale, **cache_b)
    # (c) lse_a is (1, h, b * sq): row i * sq + t of the flattened batch is (i, t)
    out, lse = flash_attn_merge_states((out_a.view(b, sq, h, d), out_b), (lse_a.as_strided((b, h, sq), (sq, b * sq, 1)), lse_b))
    return (out, lse) if return_softmax_lse else out


def flash_mla_chunked_prefill_func(q, k_ctx, v_ctx, k_new, v_new, *, cu_seqlens_q=None, cu_seqlens_k_ctx=None, softmax_scale=None, return_softmax_lse=False):
    """MLA chunked prefill over a cached context: the new tokens of every sequence attend to that sequence's context keys (all of them) and to the new tokens
    themselves (causally) - ``flash_mla_prefill_func`` over the concatenation ``[ctx_i, new_i]`` with causal=True, without building the concatenation.

    dense:  q (batch, seqlen_q, nheads, 192), k_ctx (batch, seqlen_ctx, nheads_k, 192), v_ctx (batch, seqlen_ctx, nheads_k, 128), k_new (batch, seqlen_q,
            nheads_k, 192), v_new (batch, seqlen_q, nheads_k, 128) -> out (batch, seqlen_q, nheads, 128), lse (batch, nheads, seqlen_q) with return_softmax_lse.
    packed: q (total_q, nheads, 192), k_new / v_new (total_q, nheads_k, .) under cu_seqlens_q and k_ctx / v_ctx (total_ctx, nheads_k, .) under
            cu_seqlens_k_ctx, given both or neither -> out (total_q, nheads, 128), lse (nheads, total_q).  A sequence may have no context and may have no
            query rows.  Rows of out / lse at or past cu_seqlens_q[-1] hold unspecified values.
    Every argument under the rules of flash_mla_prefill_func (dtypes, widths, views, softmax_scale).  Three launches on the current stream, no host
    synchronisation: flash_mla_prefill_func(q, k_ctx, v_ctx, causal=False), flash_mla_prefill_func(q, k_new, v_new, causal=True) with cu_seqlens_k =
    cu_seqlens_q, and flash_attn_merge_states of the two.  A sequence without context has dead rows (O = 0, LSE = 0) in the first part, which the merge's
    emptiness rule leaves out (flash_attn_merge_states has the rule and its caveat).  Values: fp32 math over all visible keys, each part rounded once to
    q's dtype before the merge.  Forward only; out of scope: everything that is out of scope for flash_mla_prefill_func, more than one context chunk per
    call (merge further chunks with flash_attn_merge_states).
    """
    tensors = (("q", q), ("k_ctx", k_ctx), ("v_ctx", v_ctx), ("k_new", k_new), ("v_new", v_new))
    for name, t in tensors:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a tensor")
    if torch.is_grad_enabled() and any(t.requires_grad for _, t in tensors):
        bad = next(n for n, t in tensors if t.requires_grad)
        raise ValueError(f"{bad} requires grad: flash_mla_chunked_prefill_func is forward-only (the differentiable function is flash_mla_attn_func); run it under "
                         "torch.no_grad() or detach the inputs")
    if (cu_seqlens_q is None) != (cu_seqlens_k_ctx is None):
        raise ValueError("cu_seqlens_q and cu_seqlens_k_ctx come both or neither, got only " + ("cu_seqlens_q" if cu_seqlens_k_ctx is None else "cu_seqlens_k_ctx"))
    rank = 3 if cu_seqlens_q is not None else 4
    for name, t in tensors:
        if t.dim() != rank:
            raise ValueError(f"{name} must be a rank-{rank} tensor ({'(total, nheads, head_dim) with cu_seqlens' if rank == 3 else '(batch, seqlen, nheads, head_dim)'})")
    if k_new.shape[-3] != q.shape[-3] or v_new.shape[-3] != q.shape[-3]:
        raise ValueError(f"k_new / v_new must have one row per query row ({q.shape[-3]}), got {k_new.shape[-3]} and {v_new.shape[-3]}")
    # the checks of flash_mla_prefill_func on each part, its messages with this function's argument names (k / v -> k_ctx / v_ctx, k_new / v_new)
    def checked(k, v, cu_k, causal, suffix):
        try:
            return _check_mla_prefill_args(q, k, v, cu_seqlens_q, cu_k, softmax_scale, causal, forward_only=True)
        except ValueError as e:
            raise ValueError(re.sub(r"\b(k|v|cu_seqlens_k)\b", lambda m: m.group(1) + suffix, str(e))) from None

    softmax_scale_ = checked(k_ctx, v_ctx, cu_seqlens_k_ctx, False, "_ctx")
    checked(k_new, v_new, cu_seqlens_q, True, "_new")
    out_c, lse_c = _C.fwd_mla_prefill(q, k_ctx, v_ctx, cu_seqlens_q, cu_seqlens_k_ctx, False, softmax_scale_)
    out_n, lse_n = _C.fwd_mla_prefill(q, k_new, v_new, cu_seqlens_q, cu_seqlens_q, True, softmax_scale_)
    out, lse = _C.merge_states([out_c, out_n], [lse_c, lse_n])
    return (out, lse) if return_softmax_lse else out


# ---- stand-alone append and gather for the MLA latent cache and the index-key cache ------------------------------------------------------------------------

class _Batch:
    """what _check_block_table asks of the tensor it calls ``like``: a batch and a device"""

    def __init__(self, b, device):
        self.shape, self.device = (b,), device


def _check_io_view(name, t):
    """a 16-bit tensor the row movers address as it is: the last dimension contiguous, every other stride and the storage offset a multiple of 8 elements"""
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        raise ValueError(f"{name}: the last dimension must be contiguous")
    if any(t.shape[i] > 1 and t.stride(i) % 8 != 0 for i in range(t.dim() - 1)):
        raise ValueError(f"{name}: every stride but the last must be a multiple of 8 elements (16-byte accesses), got strides {tuple(t.stride())}")
    if t.storage_offset() % 8 != 0 or (t.device.type != "meta" and t.data_ptr() % 16 != 0):
        raise ValueError(f"{name} must start at a multiple of 8 elements (16 bytes), got storage offset {t.storage_offset()}")


def _check_io_latent_cache(kv_cache):
    """kv_cache of the append and the gather: what flash_mla_with_kvcache takes; returns whether it holds FP8 rows"""
    if not isinstance(kv_cache, torch.Tensor) or kv_cache.dim() != 4:
        raise ValueError("kv_cache must be a rank-4 tensor")
    fp8 = _mla_cache_is_fp8(kv_cache)
    if not fp8 and kv_cache.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"kv_cache must be fp16 / bf16 and 576 wide, or an FP8 latent cache (uint8 / float8_e4m3fn rows of 656 bytes), got {kv_cache.dtype} "
                         f"rows {kv_cache.shape[-1]} wide")
    if kv_cache.shape[2] != 1:
        raise ValueError(f"kv_cache must have exactly one head (the latent row), got {kv_cache.shape[2]}")
    if not fp8 and kv_cache.shape[3] != 576:
        raise ValueError(f"kv_cache must be 576 wide, got {kv_cache.shape[3]}")
    if fp8:
        _check_mla_fp8_view(kv_cache)
    else:
        _check_io_view("kv_cache", kv_cache)
        if kv_cache.shape[1] > 1 and kv_cache.stride(1) < 576:
            raise ValueError(f"kv_cache: rows must be at least 576 elements apart, got strides {tuple(kv_cache.stride())}")
    return fp8


def _io_lengths(cache_seqlens, b, device, like):
    _check_cache_seqlens(cache_seqlens, b, device, like)
    if isinstance(cache_seqlens, int):
        cache_seqlens = torch.full((b,), max(min(cache_seqlens, 2 ** 31 - 1), -2 ** 31), dtype=torch.int32, device=device)
    return cache_seqlens.contiguous()


def _check_io_new_rows(name, t, cu_name, cu, cache, widths, trailing):
    """new rows of an append: dense (b, s_new, *trailing) or, with cu (named cu_name), packed (total_new, *trailing); returns the batch"""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"{name} must be an fp16 / bf16 tensor, got {getattr(t, 'dtype', type(t))}")
    rank = 1 + len(trailing) + (cu is None)
    shape = ("(batch, s_new, " if cu is None else "(total_new, ") + ", ".join(str(x) for x in trailing[:-1] + (" or ".join(str(w) for w in widths),)) + ")"
    if t.dim() != rank or tuple(t.shape[-len(trailing):-1]) != tuple(trailing[:-1]) or t.shape[-1] not in widths:
        raise ValueError(f"{name} must have shape {shape}{'' if cu is None else f' with {cu_name}'}, got {tuple(t.shape)}")
    if t.device != cache.device:
        raise ValueError(f"{name} must be on the cache's device")
    _check_io_view(name, t)
    if cu is None:
        return t.shape[0]
    _check_cu_seqlens(cu_name, cu, cache)
    return cu.shape[0] - 1


def flash_mla_cache_append(kv_cache, kv_new, cache_seqlens, *, k_pe=None, block_table=None, cu_seqlens_new=None):
    """Write latent rows into the cache flash_mla_with_kvcache / flash_mla_sparse_with_kvcache read, without running attention (in place; returns None).

    kv_cache: what flash_mla_with_kvcache takes - 16-bit (batch, capacity, 1, 576), or with block_table (int32 (batch, max_blocks)) a page pool (num_blocks,
    page_block_size, 1, 576); or the FP8 format, uint8 / float8_e4m3fn and 656 wide.
    kv_new: fp16 / bf16 (a 16-bit cache must have its dtype), dense (batch, s_new, 1, 576) or packed (total_new, 1, 576) with cu_seqlens_new, int32
    (batch + 1,) on the GPU.  With k_pe (the concat_and_cache_mla layout) kv_new is 512 wide and k_pe (..., 1, 64) has the same leading shape and dtype; the
    row written is their concatenation.  The last dimension is contiguous, other strides and the storage offset are multiples of 8 elements: anything else is
    a ValueError, never a copy.
    New row s of sequence i goes to logical position max(cache_seqlens[i], 0) + s; it is dropped at or past the capacity; in a paged cache it goes through
    block_table with the clamp min(uint32(entry), num_blocks - 1).  cache_seqlens (int32 (batch,) or an int) is not updated: the caller advances it.
    16-bit cache: the 1152 bytes are copied.  FP8 cache: the row is quantised by the rule of quantize_mla_kv_cache.  To the byte: a dense call leaves the
    cache as flash_mla_with_kvcache(q, kv_cache, cache_seqlens, kv_new=kv_new) does; sequence i of a packed call equals the dense call on it alone; paged ==
    contiguous; every byte that is not a target row keeps its value; packed rows at or past cu_seqlens_new[batch] are never read; nothing is written outside
    the pool, whatever the table or the lengths hold.  No host synchronisation: one launch, capturable in a graph.
    Out of scope: physical slots (slot_mapping), copying pages, advancing cache_seqlens."""
    fp8 = _check_io_latent_cache(kv_cache)
    b = _check_io_new_rows("kv_new", kv_new, "cu_seqlens_new", cu_seqlens_new, kv_cache, (576, 512), (1, 576))
    if not fp8 and kv_new.dtype != kv_cache.dtype:
        raise ValueError(f"kv_new must have kv_cache's dtype ({kv_cache.dtype}), got {kv_new.dtype}")
    if (kv_new.shape[-1] == 512) != (k_pe is not None):
        raise ValueError(f"kv_new must be 576 wide, or 512 wide together with k_pe (..., 1, 64), got {kv_new.shape[-1]} wide {'with' if k_pe is not None else 'without'} k_pe")
    if k_pe is not None:
        if not isinstance(k_pe, torch.Tensor) or k_pe.dtype != kv_new.dtype or tuple(k_pe.shape) != tuple(kv_new.shape[:-1]) + (64,) or k_pe.device != kv_new.device:
            raise ValueError(f"k_pe must have shape {tuple(kv_new.shape[:-1]) + (64,)} and kv_new's dtype and device, got {tuple(getattr(k_pe, 'shape', ()))}")
        _check_io_view("k_pe", k_pe)
    _check_block_table(block_table, _Batch(b, kv_cache.device), kv_cache, like="kv_new")
    cache_seqlens = _io_lengths(cache_seqlens, b, kv_cache.device, "kv_cache")
    if b == 0 or kv_new.shape[0] == 0 or (cu_seqlens_new is None and kv_new.shape[1] == 0):
        return None
    _C.mla_cache_append(kv_cache, kv_new, cache_seqlens, k_pe, block_table, cu_seqlens_new)
    return None


def flash_mla_cache_gather(kv_cache, cache_seqlens, out, *, block_table=None, cu_seqlens_out=None, seq_starts=None):
    """Gather rows of the latent cache into ``out``, dequantised if the cache is FP8: the packed (total_ctx, 576) input of the up-projection in front of
    flash_mla_chunked_prefill_func.  Returns out.

    kv_cache, block_table: as in flash_mla_cache_append.  out: fp16 / bf16, caller-allocated, packed (total, 576) with cu_seqlens_out int32 (batch + 1,) or
    dense (batch, n, 576) without it; the last dimension contiguous, the row stride a multiple of 8 elements and at least 576 (a slice of a wider workspace
    is fine).  Over a 16-bit cache out has the cache's dtype; over an FP8 cache its dtype says how the rope part is stored.
    Row r of sequence i (packed: r < cu_seqlens_out[i + 1] - cu_seqlens_out[i]; dense: r < n) is the cache row at logical position start_i + r, start_i =
    max(seq_starts[i], 0) (int32 (batch,) on the GPU; None = 0).  With L_i = min(max(cache_seqlens[i], 0), capacity) (cache_seqlens None = the capacity): a
    position below L_i gives the row's 1152 bytes, or dequantize_mla_kv_cache(row, out.dtype) bit for bit - what the attention kernels compute with; a
    position at or past L_i writes a row of +0 and does not read the cache.
    Never read, so they may hold 0xff bytes: rows at or past L_i, pages and table entries that no requested row needs, pages no sequence references.  Never
    written: out rows at or past cu_seqlens_out[batch], and the gaps of a strided out.  Paged == contiguous bit for bit.  No host synchronisation: one launch,
    capturable in a graph.  Out of scope: FP8 output, gathering the index-key cache, physical slots."""
    fp8 = _check_io_latent_cache(kv_cache)
    if not isinstance(out, torch.Tensor) or out.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"out must be an fp16 / bf16 tensor, got {getattr(out, 'dtype', type(out))}")
    if not fp8 and out.dtype != kv_cache.dtype:
        raise ValueError(f"out must have kv_cache's dtype ({kv_cache.dtype}), got {out.dtype}")
    packed = cu_seqlens_out is not None
    if out.dim() != (2 if packed else 3) or out.shape[-1] != 576:
        raise ValueError(f"out must have shape {'(total, 576) with cu_seqlens_out' if packed else '(batch, n, 576)'}, got {tuple(out.shape)}")
    if out.device != kv_cache.device:
        raise ValueError("out must be on kv_cache's device")
    _check_io_view("out", out)
    if out.shape[-2] > 1 and out.stride(-2) < 576:
        raise ValueError(f"out: rows must be at least 576 elements apart, got strides {tuple(out.stride())}")
    if packed:
        _check_cu_seqlens("cu_seqlens_out", cu_seqlens_out, kv_cache)
    b = cu_seqlens_out.shape[0] - 1 if packed else out.shape[0]
    _check_block_table(block_table, _Batch(b, kv_cache.device), kv_cache, like="out")
    if cache_seqlens is not None:
        cache_seqlens = _io_lengths(cache_seqlens, b, kv_cache.device, "kv_cache")
    if seq_starts is not None:
        if not isinstance(seq_starts, torch.Tensor) or seq_starts.dtype != torch.int32 or tuple(seq_starts.shape) != (b,) or seq_starts.device != kv_cache.device:
            raise ValueError(f"seq_starts must be an int32 tensor (batch,) = ({b},) on kv_cache's device")
        seq_starts = seq_starts.contiguous()
    if b == 0 or out.shape[0] == 0 or (not packed and out.shape[1] == 0):
        return out
    _C.mla_cache_gather(kv_cache, cache_seqlens, out, block_table, cu_seqlens_out, seq_starts, b)
    return out


_IDX_SCALE_FORMATS = {"fp32": 0, "ue8m0": 1}     # FA_IDX_SCALE_FP32 / FA_IDX_SCALE_UE8M0 of the C ABI


def _check_scale_format(scale_format):
    if not isinstance(scale_format, str) or scale_format not in _IDX_SCALE_FORMATS:
        raise ValueError(f"scale_format must be 'fp32' or 'ue8m0', got {scale_format!r}")
    return _IDX_SCALE_FORMATS[scale_format]


def quantize_mla_index_keys(k, scale_format="fp32"):
    """(..., 128) fp16 / bf16 index keys -> (codes uint8 (..., 128), scale float32 (...)): the rule of flash_mla_index_cache_append, what
    flash_mla_indexer_logits reads as k_idx_cache and k_scale.

    amax = max |x| over the row's finite elements (0 if none); scale = max(amax, 2^-24) / 448, the correctly rounded fp32 quotient; under
    scale_format="ue8m0" the scale is rounded up to a power of two on its bits, (bits(scale) + 0x007fffff) & 0x7f800000; code = e4m3_rne(clamp(float(x) /
    scale, -448, 448)), NaN kept with its sign (0x7f / 0xff), +-inf saturating: one 128-column tile of quantize_mla_kv_cache.  Plain torch: any device."""
    if not isinstance(k, torch.Tensor) or k.dtype not in (torch.float16, torch.bfloat16) or k.dim() < 1 or k.shape[-1] != 128:
        raise ValueError("k must be an fp16 / bf16 tensor (..., 128)")
    ue8m0 = _check_scale_format(scale_format) == 1
    x = k.float()
    amax = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(dim=-1, keepdim=True)
    scale = torch.clamp(amax, min=2.0 ** -24) / torch.full_like(amax, 448.0)     # (tensor / tensor: a division on every device, never a multiplication by 1 / 448)
    if ue8m0:
        scale = ((scale.view(torch.int32) + 0x007FFFFF) & 0x7F800000).view(torch.float32)
    y = torch.clamp(x / scale, min=-448.0, max=448.0)      # (NaN passes through clamp)
    nan = torch.isnan(y)
    codes = torch.where(nan, torch.zeros_like(y), y).to(torch.float8_e4m3fn).view(torch.uint8)
    sign = ((k.contiguous().view(torch.int16).to(torch.int32) >> 8) & 0x80).to(torch.uint8)      # (of the 16-bit pattern: a widening may drop a NaN's sign)
    return torch.where(nan, sign | 0x7F, codes), scale.squeeze(-1)


def quantize_mla_index_queries(q_idx, weights, scale_format="fp32"):
    """(..., heads, 128) fp16 / bf16 index queries and float32 weights (..., heads) -> (codes uint8 (..., heads, 128), weights * scale float32 (..., heads)): what
    flash_mla_indexer_logits and flash_mla_indexer_prefill_logits take as an FP8 q_idx and its weights.

    The row rule of quantize_mla_index_keys applied to each (token, head) row: amax over the row's finite elements, scale = max(amax, 2^-24) / 448 (rounded up to
    a power of two under scale_format="ue8m0"), code = e4m3_rne(clamp(float(x) / scale, -448, 448)), NaN kept with its sign, +-inf saturating.  The scale is
    folded into the head's weight as the fp32 product weights * scale, which is what the model does.  Plain torch, any device: a convenience, not a fused
    quantiser."""
    if not isinstance(q_idx, torch.Tensor) or q_idx.dtype not in (torch.float16, torch.bfloat16) or q_idx.dim() < 2 or q_idx.shape[-1] != 128:
        raise ValueError("q_idx must be an fp16 / bf16 tensor (..., heads, 128)")
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) != tuple(q_idx.shape[:-1]):
        raise ValueError(f"weights must be a float32 tensor of shape {tuple(q_idx.shape[:-1])} (q_idx without its last dimension)")
    codes, scale = quantize_mla_index_keys(q_idx, scale_format)
    return codes, weights * scale


def flash_mla_index_cache_append(k_idx_cache, k_idx_new, cache_seqlens, *, k_scale=None, block_table=None, cu_seqlens_new=None, scale_format="fp32"):
    """Write index keys into the cache flash_mla_indexer_logits reads (in place; returns None).

    k_idx_cache, k_scale: the two views flash_mla_indexer_logits takes - values (batch, capacity, 128) or a pool (num_blocks, page_block_size, 128) with
    block_table, and scales float32 (batch, capacity) / (num_blocks, page_block_size), any strides.  k_idx_new: fp16 / bf16, (batch, s_new, 128) or packed
    (total_new, 128) with cu_seqlens_new.  Placement, drop and clamp rules are those of flash_mla_cache_append.
    16-bit cache (k_idx_new's dtype): rows are copied; k_scale must be None.  FP8 cache (float8_e4m3fn / uint8): k_scale is required and takes one scale per
    token; rows and scales are those of quantize_mla_index_keys(k_idx_new, scale_format), byte for byte ("fp32", or "ue8m0": scales rounded up to powers of
    two, as DeepSeek-V3.2 stores them).  Every other byte of both buffers is untouched.  No host synchronisation: one launch, capturable in a graph.
    Out of scope: gathering the index-key cache (the indexer reads it in place), physical slots, advancing cache_seqlens."""
    if not isinstance(k_idx_cache, torch.Tensor) or k_idx_cache.dim() != 3:
        raise ValueError("k_idx_cache must be a rank-3 tensor (batch, capacity, 128), or a page pool (num_blocks, page_block_size, 128) with block_table")
    fp8 = k_idx_cache.dtype in (torch.uint8, torch.float8_e4m3fn)
    if not fp8 and k_idx_cache.dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"k_idx_cache must be fp16 / bf16 or hold e4m3 codes (float8_e4m3fn / uint8), got {k_idx_cache.dtype}")
    if k_idx_cache.shape[2] != 128:
        raise ValueError(f"k_idx_cache must be 128 wide, got {k_idx_cache.shape[2]}")
    _check_idx_cache_view(k_idx_cache, fp8)
    b = _check_io_new_rows("k_idx_new", k_idx_new, "cu_seqlens_new", cu_seqlens_new, k_idx_cache, (128,), (128,))
    if not fp8 and k_idx_new.dtype != k_idx_cache.dtype:
        raise ValueError(f"k_idx_new must have k_idx_cache's dtype ({k_idx_cache.dtype}), got {k_idx_new.dtype}")
    fmt = _check_scale_format(scale_format)
    if not fp8 and k_scale is not None:
        raise ValueError("k_scale must be None with a 16-bit k_idx_cache (rows are copied; there are no scales)")
    if fp8:
        if k_scale is None:
            raise ValueError("k_scale is required with an FP8 k_idx_cache: a float32 tensor with one scale per cached token")
        if not isinstance(k_scale, torch.Tensor) or k_scale.dtype != torch.float32:
            raise ValueError("k_scale must be a float32 tensor with one scale per cached token")
        if tuple(k_scale.shape) != tuple(k_idx_cache.shape[:2]) or k_scale.device != k_idx_cache.device:
            raise ValueError(f"k_scale must have shape {tuple(k_idx_cache.shape[:2])} (k_idx_cache without its last dimension) on k_idx_cache's device, got {tuple(k_scale.shape)}")
        if k_scale.device.type != "meta" and k_scale.data_ptr() % 4 != 0:
            raise ValueError("k_scale must be 4-byte aligned")
    _check_block_table(block_table, _Batch(b, k_idx_cache.device), k_idx_cache, like="k_idx_new", pool_name="k_idx_cache")
    cache_seqlens = _io_lengths(cache_seqlens, b, k_idx_cache.device, "k_idx_cache")
    if b == 0 or k_idx_new.shape[0] == 0 or (cu_seqlens_new is None and k_idx_new.shape[1] == 0):
        return None
    _C.mla_index_cache_append(k_idx_cache, k_idx_new, cache_seqlens, k_scale, block_table, cu_seqlens_new, fmt)
    return None
