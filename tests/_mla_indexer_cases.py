"""Shared models and inputs of the indexer tests (flash_mla_indexer_logits, flash_mla_indexer_topk, flash_mla_index_with_kvcache).

Two models, both checked against brute force in tests/test_mla_indexer_cpu.py on the inputs the GPU tests use:
  logits_model   torch fp64:  logit[i, t, j] = k_scale[j] * sum_h w[t, h] * relu(q[t, h, :] . k[j, :]), with the bound's magnitude next to it
  topk_model     integers: the key u(x) = bits ^ (sign ? 0xffffffff : 0x80000000) and a stable sort
No GPU, no package import: plain torch / numpy."""
import numpy as np
import torch

D = 128
CAP = 320
LENS = [0, 1, 31, 32, 33, 100, 257]
SENTINEL = -12345.678            # what a logits buffer holds where nothing may be written


def visible(L, sq, t, causal, cap):
    """n_t: keys token t of a sequence with cache_seqlens = L sees"""
    L = min(max(int(L), 0), cap)
    return L if not causal else min(L, max(L - sq + t + 1, 0))


def visible_mask(lens, sq, cap, causal):
    """bool (b, sq, cap): j < n_t"""
    n = torch.tensor([[visible(L, sq, t, causal, cap) for t in range(sq)] for L in lens], dtype=torch.int64)
    return torch.arange(cap).view(1, 1, cap) < n.unsqueeze(-1)


# ---- logits --------------------------------------------------------------------------------------------------------------------------------------

def keys_as_float64(k):
    """the values the kernel computes with: the element of a 16-bit cache, float(code) of an FP8 one (uint8 holds e4m3 codes)"""
    if k.dtype == torch.uint8:
        k = k.view(torch.float8_e4m3fn)
    return k.to(torch.float32).to(torch.float64)


def logits_model(q, w, k, k_scale, variant=None):
    """fp64 logits (b, sq, cap) over EVERY key of the logical cache k (b, cap, 128) - visibility is the caller's mask - and the magnitude
    |k_scale_j| * sum_h |w_h| * sum_d |q_hd k_jd| the tolerance is stated in.  variant (the CPU test's wrong formulas): "no_relu", "drop_head"."""
    q64, w64, k64 = q.to(torch.float64), w.to(torch.float64), keys_as_float64(k)
    s = torch.einsum("bthd,bjd->bthj", q64, k64)
    r = s if variant == "no_relu" else torch.clamp(s, min=0.0)
    if variant == "drop_head":
        w64 = w64.clone()
        w64[..., -1] = 0.0
    sc = torch.ones(k64.shape[:2], dtype=torch.float64) if k_scale is None else k_scale.to(torch.float64)
    out = torch.einsum("bth,bthj->btj", w64, r) * sc.unsqueeze(1)
    mag = torch.einsum("bthd,bjd->bthj", q64.abs(), k64.abs())
    mag = torch.einsum("bth,bthj->btj", w.to(torch.float64).abs(), mag) * sc.abs().unsqueeze(1)
    return out, mag


def logits_brute(q, w, k, k_scale, i, t, j):
    """one logit by loops over Python floats (fp64)"""
    kk = keys_as_float64(k)[i, j].tolist()
    tot = 0.0
    for h in range(q.shape[2]):
        s = sum(float(a) * b for a, b in zip(q[i, t, h].to(torch.float64).tolist(), kk))
        tot += float(w[i, t, h]) * (s if s > 0 else 0.0)
    return tot * (1.0 if k_scale is None else float(k_scale[i, j]))


def logits_fp32_formula(q, w, k, k_scale):
    """the contract's formula in torch fp32 on the same inputs: what a straightforward implementation computes (the CPU test holds it to the bound)"""
    kf = keys_as_float64(k).to(torch.float32)
    s = torch.einsum("bthd,bjd->bthj", q.to(torch.float32), kf)
    out = torch.einsum("bth,bthj->btj", w, torch.clamp(s, min=0.0))
    return out if k_scale is None else out * k_scale.unsqueeze(1)


TOL = 2.0 ** -15                 # |logit - fp64| <= TOL * magnitude: 192 roundings of 2^-24 (127 dot, 1 + 63 head sum, 1 scale) < 2^-16, x 2 for MFMA's internal order


def exact_inputs(b, sq, h, dtype, fp8, gen, cap=CAP):
    """integers in [-8, 8] for q_idx and the keys, signed powers of two in [2^-2, 2^2] for the weights, powers of two for k_scale: every partial sum
    stays below 2^24 (asserted), so fp32 math is exact in any order"""
    q = torch.randint(-8, 9, (b, sq, h, D), generator=gen).to(dtype)
    k = torch.randint(-8, 9, (b, cap, D), generator=gen).to(torch.float32)
    k = k.to(torch.float8_e4m3fn) if fp8 else k.to(dtype)
    w = (2.0 ** torch.randint(-2, 3, (b, sq, h), generator=gen).float()) * (torch.randint(0, 2, (b, sq, h), generator=gen).float() * 2 - 1)
    sc = 2.0 ** torch.randint(-3, 4, (b, cap), generator=gen).float()
    assert torch.equal(keys_as_float64(k), keys_as_float64(k).round()) and keys_as_float64(k).abs().max() <= 8
    # the largest partial sum: sum_h |w| * sum_d |q k|, before the (power of two) scale
    _, mag = logits_model(q, w, k, None)
    assert float(mag.max()) < 2.0 ** 24
    return q, w, k, sc


def normal_inputs(b, sq, h, dtype, fp8, gen, cap=CAP):
    """N(0, 1) q_idx, keys, weights; scales in [0.5, 2)"""
    q = torch.randn(b, sq, h, D, generator=gen).to(dtype)
    k = torch.randn(b, cap, D, generator=gen)
    k = k.to(torch.float8_e4m3fn) if fp8 else k.to(dtype)
    w = torch.randn(b, sq, h, generator=gen)
    sc = torch.rand(b, cap, generator=gen) * 1.5 + 0.5
    return q, w, k, sc


def paginate(k, sc, P, gen, spare=3):
    """logical (b, cap, 128) keys and (b, cap) scales -> pool (num_blocks, P, 128), scale pool (num_blocks, P), int32 table (b, cap / P) under a random
    page permutation; `spare` pages that nothing references hold NaN codes / NaN elements and NaN scales"""
    b, cap, _ = k.shape
    cols = cap // P
    assert cols * P == cap
    nb = b * cols + spare
    perm = torch.randperm(nb, generator=gen)
    table = perm[:b * cols].reshape(b, cols).to(torch.int32)
    raw = k.view(torch.uint8) if k.dtype == torch.float8_e4m3fn else k
    fill = 0x7F if raw.dtype == torch.uint8 else float("nan")
    pool = torch.full((nb, P, D), fill, dtype=raw.dtype)
    spool = torch.full((nb, P), float("nan"), dtype=torch.float32)
    pool[table.long().reshape(-1)] = raw.reshape(b * cols, P, D)
    spool[table.long().reshape(-1)] = sc.reshape(b * cols, P)
    if k.dtype == torch.float8_e4m3fn:
        pool = pool.view(torch.float8_e4m3fn)
    return pool, spool, table


# ---- top-k -----------------------------------------------------------------------------------------------------------------------------------------

def order_key(x):
    """u(x) of fp32 values, as uint32 in an int64 array"""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)
    return np.where(bits >> 31 != 0, bits ^ 0xFFFFFFFF, bits ^ 0x80000000)


def topk_row_model(row, n, topk):
    """one row: int32 (topk,).  A stable descending sort of the keys below n keeps equal keys in position order, so its first topk entries are the
    largest keys with ties at the threshold going to the lower positions; they are emitted in ascending position order"""
    out = np.full(topk, -1, dtype=np.int32)
    if n <= topk:
        out[:n] = np.arange(n, dtype=np.int32)
        return out
    u = order_key(row[:n])
    order = np.argsort(-u, kind="stable")
    out[:] = np.sort(order[:topk]).astype(np.int32)
    return out


def topk_model(logits, lens, topk, causal):
    """int32 (b, sq, topk) of fp32 logits (b, sq, cap) (torch or numpy)"""
    x = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    b, sq, cap = x.shape
    out = np.empty((b, sq, topk), dtype=np.int32)
    for i in range(b):
        for t in range(sq):
            out[i, t] = topk_row_model(x[i, t], visible(lens[i], sq, t, causal, cap), topk)
    return torch.from_numpy(out)


def topk_row_brute(row, n, topk):
    """the definition, by loops: repeatedly take the largest remaining key, the lowest position among equals"""
    if n <= topk:
        return list(range(n)) + [-1] * (topk - n)
    u = order_key(row[:n]).tolist()
    left = set(range(n))
    got = []
    for _ in range(topk):
        best = max(left, key=lambda j: (u[j], -j))
        left.remove(best)
        got.append(best)
    return sorted(got)


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def topk_rows(gen_seed=0):
    """name -> (fp32 row, n, topk): the selection cases of the GPU test, one row each (the test also stacks them to b 3 x sq 2)"""
    rng = np.random.default_rng(gen_seed)
    rows = {}
    for n in (1, 31, 32, 33, 4999):
        cap = n + 9
        x = rng.permutation(cap).astype(np.float32) - cap / 3                  # distinct values
        for topk in (32, 64, 2048):
            rows[f"distinct_n{n}_k{topk}"] = (x, n, topk)
    for topk in (32, 64):
        for n in (topk - 1, topk, topk + 1):
            rows[f"edge_n{n}_k{topk}"] = (rng.standard_normal(n + 5).astype(np.float32), n, topk)
    rows["edge_n2049_k2048"] = (rng.standard_normal(2060).astype(np.float32), 2049, 2048)
    rows["all_equal"] = (np.full(700, 1.5, dtype=np.float32), 700, 64)
    x = rng.standard_normal(3000).astype(np.float32)
    x[rng.permutation(3000)[:1500]] = 0.25                                     # the threshold falls into 1500 equal entries
    x[rng.permutation(3000)[:40]] = 5.0
    rows["heavy_ties"] = (x, 3000, 64)
    rows["heavy_ties_k2048"] = (x, 3000, 2048)
    base = np.uint32(0x3F800000)
    rows["low_byte_only"] = (f32(base + rng.integers(0, 256, 2500).astype(np.uint32)), 2500, 64)     # keys differ in bits 7 .. 0 alone: the last radix pass
    special = f32([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x7FC00000, 0xFFC00000, 0x7F800001,
                   0xFF800001, 0x3F800000, 0xBF800000])
    x = np.concatenate([special] * 6 + [rng.standard_normal(20).astype(np.float32)])
    rows["specials"] = (x[rng.permutation(len(x))], len(x), 32)
    rows["specials_k64"] = (rows["specials"][0], len(x), 64)
    x = rng.standard_normal(600).astype(np.float32)
    x[500:] = f32([0x7F800000, 0x7FC00000] * 50)                              # +inf and NaN at j >= n: never selected
    rows["poison_past_n"] = (x, 500, 64)
    return rows
