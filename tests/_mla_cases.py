"""Case builders of tests/test_kvcache_mla_number_range_gpu.py, on the CPU and without the library, so that tests/test_kvcache_mla_number_range_cpu.py can
check the cases themselves: pattern sets, the numpy expectation of the FP8 dequantisation, the tiles of the quantising append, the softmax-extreme caches, the
rope-column infinities and the pages of the pools larger than 4 GiB.  Fixed CPU-generator seeds throughout; sections A .. G are those of the GPU file."""
import numpy as np
import torch

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DK, DV, DR, RB = 576, 512, 64, 656
NAN, INF = float("nan"), float("inf")
ROW16, ROW8 = 2 * DK, RB                       # bytes of a latent row
CLAMP = np.float32(2.0 ** -24)                 # the append: scale = max(amax, 2^-24) / 448


def i16(a):
    """integer bit patterns 0 .. 65535 -> int16"""
    a = torch.as_tensor(a, dtype=torch.int32)
    return torch.where(a >= 32768, a - 65536, a).to(torch.int16)


def finite_patterns(dt, below_exp=None):
    """every finite bit pattern of dt as int16 (63488 in fp16, 65280 in bf16); below_exp: only |x| < 2^below_exp"""
    a = torch.arange(65536, dtype=torch.int32)
    em = 0x7C00 if dt == torch.float16 else 0x7F80
    p = i16(a[(a & em) != em])
    if below_exp is not None:
        p = p[p.view(dt).float().abs() < 2.0 ** below_exp]
    return p


def rope_only_q(shape, dt, gen, mult=1.0 / 64):
    """q that is 0 in columns 0 .. 511 and N(0, 1) x mult in the rope columns.  In MLA the value is the key: a row that holds every finite value of the dtype
    in columns 0 .. 511 meets a q that is non-zero there with a score far outside the contract (|score| x log2 e < 2^31; 3e38 in bf16), and even inside
    it the residue of m c would no longer be below half an output ulp.  With q = 0 there the products are exact zeros and the score comes from the rope
    columns alone, which hold N(0, 1)."""
    q = torch.zeros(*shape, dtype=torch.float32)
    q[..., DV:] = torch.randn(*shape[:-1], DR, generator=gen) * mult
    return q.to(dt)


# ---- A ---------------------------------------------------------------------------------------------------------------------------------------------------

def a_rows(dt, seed=91000):
    """(R, 576): columns 0 .. 511 hold every finite pattern of dt in a fixed shuffled order (R = 124 in fp16, 128 in bf16, the remainder repeats), columns
    512 .. 575 N(0, 1)"""
    gen = torch.Generator().manual_seed(seed)
    pats = finite_patterns(dt)
    pats = pats[torch.randperm(pats.numel(), generator=gen)]
    R = -(-pats.numel() // DV)
    lat = pats[torch.arange(R * DV) % pats.numel()].view(R, DV).view(dt)
    return torch.cat([lat, torch.randn(R, DR, generator=gen).to(dt)], dim=-1)


# ---- B ---------------------------------------------------------------------------------------------------------------------------------------------------

B_H, B_SQ = 128, 5                             # 640 (head, token) pairs of a sequence read its 576 columns (the last 64 pairs read a second time)


def b_onehot_q(b, dt):
    """(b, 5, 128, 576) one-hot 1.0 at column j = (128 t + h + 7 i) % 576 of row (i, t, h), and j as (b, 5, 128)"""
    i, t, h = torch.meshgrid(torch.arange(b), torch.arange(B_SQ), torch.arange(B_H), indexing="ij")
    j = (B_H * t + h + 7 * i) % DK
    q = torch.zeros(b, B_SQ, B_H, DK, dtype=dt)
    q.scatter_(3, j.unsqueeze(-1), torch.ones(b, B_SQ, B_H, 1, dtype=dt))
    return q, j


def b_key_rows(dt, below_exp):
    """(b, 576): the finite patterns of dt (|x| < 2^below_exp if given) over whole rows, rope columns included; the remainder repeats"""
    pats = finite_patterns(dt, below_exp)
    b = -(-pats.numel() // DK)
    return pats[(torch.arange(b * DK) * 1 + 0) % pats.numel()].view(b, DK).view(dt)


def b_query_rows(dt, below_exp, n_rows, j_of_row):
    """(n_rows, 576) of finite patterns everywhere, with q[r, j_of_row[r]] = pattern r % n: over 65536 rows every pattern is read"""
    pats = finite_patterns(dt, below_exp)
    n = pats.numel()
    r = torch.arange(n_rows).view(-1, 1)
    c = torch.arange(DK).view(1, -1)
    q = pats[(r * 7 + c * 131 + 1) % n]
    q.scatter_(1, j_of_row.view(-1, 1), pats[torch.arange(n_rows) % n].view(-1, 1))
    return q.view(dt)


def e4m3_values():
    """float64 (256,): the value of every e4m3fn code (NaN for 0x7f / 0xff), from the format's definition"""
    v = np.zeros(256)
    for c in range(256):
        e, m = (c >> 3) & 0xF, c & 7
        x = m / 8.0 * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        v[c] = np.nan if (c & 0x7F) == 0x7F else (-x if c & 0x80 else x)
    return v


def round_bf16_bits(x32):
    """float32 array -> uint16 bf16 bits, round to nearest-even on the integer bits (no NaN inputs)"""
    u = np.asarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def dequant_expect_bits(codes_u8, scales_f32, dtname):
    """numpy, independent of the library: codes (..., 512) uint8, scales (..., 4) float32 -> uint16 bits of round_to_dtype(fp32(code) x scale), the
    fp32 product rounded once"""
    val = e4m3_values().astype(np.float32)[np.asarray(codes_u8)]
    with np.errstate(over="ignore", invalid="ignore"):
        prod = val.reshape(*val.shape[:-1], 4, 128) * np.asarray(scales_f32, dtype=np.float32)[..., None]
        prod = prod.reshape(val.shape).astype(np.float32)
        if dtname == "fp16":
            return prod.astype(np.float16).view(np.uint16)
    return round_bf16_bits(prod)


def nan_free_codes():
    """uint8 (256,): the codes 0 .. 255 with the two NaN codes replaced by 0"""
    c = torch.arange(256, dtype=torch.int64)
    return torch.where((c & 0x7F) == 0x7F, torch.zeros_like(c), c).to(torch.uint8)


def fp8_rows(codes, scales, rope):
    """uint8 (n, 656) from codes (n, 512) uint8, scales (n, 4) float32, rope (n, 64) of the dtype"""
    n = codes.shape[0]
    return torch.cat([codes, scales.contiguous().view(torch.uint8).view(n, 16), rope.contiguous().view(torch.uint8).view(n, 128)], dim=-1)


B8_SCALES = [[2.0 ** -7, 0.3, 1.0, 3.7], [3.7, 2.0 ** -7, 0.3, 1.0], [0.01, 5.5, 2.0 ** -12, 16.0]]


def b_fp8_rows(dt, seed=92500):
    """(6, 656): per scale set two rows - tile g of the first holds codes 0 .. 127, of the second 128 .. 255 (the NaN codes replaced by 0) - so every
    NaN-free code sits in all four tiles under four different scales; N(0, 1) rope elements"""
    gen = torch.Generator().manual_seed(seed)
    c = nan_free_codes()
    codes = torch.stack([c[:128].repeat(4), c[128:].repeat(4)] * len(B8_SCALES))
    scales = torch.tensor(B8_SCALES, dtype=torch.float32).repeat_interleave(2, dim=0)
    return fp8_rows(codes, scales, torch.randn(codes.shape[0], DR, generator=gen).to(dt))


# ---- C ---------------------------------------------------------------------------------------------------------------------------------------------------

C_EXP = (-117, 118)        # 2^-9 x 2^-117 = 2^-126, the smallest normal fp32; 448 x 2^118 < 2^127: every product is zero or normal


def c_scales():
    """float32 (62, 4): 2^e for e = -117 .. 118, then 0.3, 3.7, 1 / 448, 65504 / 448 and the fp32 value just above each, -1, -0.3, 0 and one repeat"""
    s = [np.float32(2.0) ** np.float32(e) for e in range(C_EXP[0], C_EXP[1] + 1)]
    for x in (np.float32(0.3), np.float32(3.7), np.float32(1.0) / np.float32(448.0), np.float32(65504.0) / np.float32(448.0)):
        s += [x, np.nextafter(x, np.float32(np.inf), dtype=np.float32)]
    s += [np.float32(-1.0), np.float32(-0.3), np.float32(0.0), np.float32(1.0)]
    a = np.array(s, dtype=np.float32)
    assert a.size == 248
    # sequence i takes scales 4 i .. 4 i + 3: neighbouring binades share a row, so in fp16 the rows up to 2^7 stay finite and the rows from 2^8 on overflow
    return torch.from_numpy(a.reshape(62, 4).copy())


def c_rows(dt, seed=93000):
    """(62, 656): every NaN-free code twice (the tiles hold codes 0 .. 127, 128 .. 255, 0 .. 127, 128 .. 255), the scales of c_scales, N(0, 1) rope"""
    gen = torch.Generator().manual_seed(seed)
    sc = c_scales()
    return fp8_rows(nan_free_codes().repeat(2).expand(sc.shape[0], DV).contiguous(), sc, torch.randn(sc.shape[0], DR, generator=gen).to(dt))


# ---- D ---------------------------------------------------------------------------------------------------------------------------------------------------

D_B, D_SNEW = 64, 128                          # 8192 new rows, 32768 tiles


def e4m3_midpoints():
    """float64 (126,): the midpoints between neighbouring non-negative e4m3 values 0 .. 448"""
    v = e4m3_values()[:0x7F]
    return (v[:-1] + v[1:]) / 2


def d_kv_new(dt, seed=94000):
    """kv_new (64, 128, 1, 576) whose 32768 tiles of 128 columns have a chosen amax: every finite positive pattern of dt once (31743 in fp16, 32639 in bf16;
    subnormals and values below the 2^-24 clamp among them), the other tiles all zero, in a fixed shuffled order.  The amax element sits in a random column
    with a random sign.  Tiles with an even index fill the other 127 columns with random bit patterns of magnitude <= amax (both signs; columns 1 .. 4 after
    the amax hold +0, -0 and the smallest subnormal of both signs); tiles with an odd index hold, for 42 of the 126 e4m3 midpoints (rotating with the tile),
    the 16-bit value nearest to scale x midpoint and its two 16-bit neighbours, scale = max(amax, 2^-24) / 448 in fp32.  Rope columns N(0, 1).
    Returns kv_new, amax bits (32768,) int32 (0 = an all-zero tile) in tile order, and the (tile, column, midpoint index) of every midpoint triple's centre."""
    gen = torch.Generator().manual_seed(seed)
    em = 0x7C00 if dt == torch.float16 else 0x7F80
    pos = torch.arange(1, em, dtype=torch.int32)                   # positive finite patterns, in value order
    T = D_B * D_SNEW * 4
    amax = torch.zeros(T, dtype=torch.int32)
    amax[:pos.numel()] = pos
    amax = amax[torch.randperm(T, generator=gen)]
    mag = (torch.rand(T, 128, generator=gen) * (amax + 1).view(-1, 1).double()).floor().to(torch.int32).clamp(max=amax.view(-1, 1))
    col = torch.randint(0, 128, (T,), generator=gen)
    ar = torch.arange(T)
    edge = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    for k in range(4):
        mag[ar, (col + 1 + k) % 128] = torch.minimum(edge[k].expand(T), amax)
    sign = torch.randint(0, 2, (T, 128), generator=gen, dtype=torch.int32)
    for k in range(4):
        sign[ar, (col + 1 + k) % 128] = k % 2
    # the midpoint tiles
    odd = (ar % 2 == 1) & (amax > 0)
    amax_f = i16(amax).view(dt).float().numpy()
    scale = (np.maximum(amax_f, CLAMP) / np.float32(448.0)).astype(np.float64)
    mid = e4m3_midpoints()
    t_odd = ar[odd]
    k_idx = (torch.arange(42).view(1, -1) * 3 + (t_odd // 2).view(-1, 1)) % 126                 # (n_odd, 42)
    target = torch.from_numpy(scale[t_odd.numpy()]).view(-1, 1) * torch.from_numpy(mid)[k_idx]  # float64
    centre = target.to(dt).view(torch.int16).to(torch.int32)                                    # positive patterns
    triple = torch.stack([(centre - 1).clamp(min=0), centre, centre + 1], dim=-1).view(-1, 126)
    triple = torch.minimum(triple, amax[t_odd].view(-1, 1))
    cols = (col[t_odd].view(-1, 1) + 1 + torch.arange(126).view(1, -1)) % 128                   # the 126 columns behind the amax; one column keeps its random value
    mag[t_odd.view(-1, 1), cols] = triple
    sign[t_odd.view(-1, 1), cols] = torch.randint(0, 2, (t_odd.numel(), 42), generator=gen, dtype=torch.int32).repeat_interleave(3, dim=1)
    mag[ar, col] = amax
    bits = mag | (sign << 15)
    bits[amax == 0] = 0
    lat = i16(bits).view(dt).view(D_B, D_SNEW, 1, DV)
    kv_new = torch.cat([lat, torch.randn(D_B, D_SNEW, 1, DR, generator=gen).to(dt)], dim=-1)
    centres = (t_odd.view(-1, 1).expand(-1, 42), (col[t_odd].view(-1, 1) + 2 + 3 * torch.arange(42).view(1, -1)) % 128, k_idx)
    return kv_new, amax, centres


def d_prefix_lengths():
    """the rows in front of the 128 new ones, per sequence: 0 .. 31, so the new rows start at every offset within a page of 16 and cross eight pages"""
    return [(5 * i + 3) % 32 for i in range(D_B)]


D_CAP = 160


def d_scale_words(amax_bits, dt):
    """numpy, independent of the helper: np.float32(max(amax, 2^-24)) / np.float32(448), the correctly rounded quotient, and the reciprocal-multiply
    max(amax, 2^-24) x fl(1 / 448) a wrong kernel could use"""
    a = np.maximum(i16(amax_bits).view(dt).float().numpy(), CLAMP)
    return a / np.float32(448.0), a * (np.float32(1.0) / np.float32(448.0))


# ---- E ---------------------------------------------------------------------------------------------------------------------------------------------------

E_L, E_CAP, E_H, E_SQ, E_TOPK = 224, 256, 24, 2, 256
E_SPLIT = 96                                   # num_splits = 3 over 8 steps of 32 keys: splits of 96 keys, the visible ones 0 .. 95, 96 .. 191, 192 .. 223
E_PATTERNS = ["ramp_up", "ramp_down", "spike_last_split", "scaled", "lse_gap_first", "lse_gap_last"]
E_GAP_BLOCK = {"lse_gap_first": slice(0, E_SPLIT), "lse_gap_last": slice(2 * E_SPLIT, E_L)}


def e_case(pattern, dt, seed=95000):
    """q (1, 2, 24, 576) and the latent cache (1, 256, 1, 576) of a softmax extreme, rounded to dt.  q = 1 + N(0, 1) / 2 and keys N(0, 1) / 2: |q| is about 27,
    the default scale 1 / 24, so a key moved by x along qhat = q[0, 0, 0] / |q[0, 0, 0]| gains about 1.1 x nats for head 0 and 0.9 x for the others (all
    heads share the mean 1).  ramp: +-(j / 8) qhat, about 0.14 nats a key, so the running max moves at every step of a rising ramp; spike: key 220 (the last
    step of the last of three splits) = q[0, 0, 0] / 2, about 15 nats above scores of deviation 0.56; scaled: q and keys x 6 (score deviation 20: rows near
    one-hot); lse_gap: the keys of the first / the last of three splits lifted by 130 qhat, 115 nats or more."""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(1, E_SQ, E_H, DK, generator=gen) * 0.5 + 1.0
    kv = torch.randn(1, E_CAP, 1, DK, generator=gen) * 0.5
    qhat = q[0, 0, 0] / q[0, 0, 0].norm()
    if pattern.startswith("ramp"):
        kv = kv + (1.0 if pattern == "ramp_up" else -1.0) * (torch.arange(E_CAP).float() / 8.0).view(1, E_CAP, 1, 1) * qhat
    elif pattern == "spike_last_split":
        kv[0, E_L - 4, 0] = q[0, 0, 0] * 0.5
    elif pattern == "scaled":
        q, kv = q * 6.0, kv * 6.0
    else:
        blk = E_GAP_BLOCK[pattern]
        kv[0, blk] = kv[0, blk] + 130.0 * qhat
    return q.to(dt), kv.to(dt)


def e_lists(seed=95500):
    """{name: int32 (1, 2, 256)}: keys 0 .. 223 in order, reversed, shuffled (another shuffle per token), padded with -1"""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name in ("in_order", "reversed", "shuffled"):
        idx = torch.full((1, E_SQ, E_TOPK), -1, dtype=torch.int32)
        for t in range(E_SQ):
            keys = torch.arange(E_L, dtype=torch.int32)
            idx[0, t, :E_L] = keys if name == "in_order" else keys.flip(0) if name == "reversed" else keys[torch.randperm(E_L, generator=gen)]
        out[name] = idx
    return out


# ---- F ---------------------------------------------------------------------------------------------------------------------------------------------------

F_LENS, F_CAP, F_H, F_SQ, F_TOPK = [100, 33], 112, 24, 2, 64
F_POS = ((0, 99, 540, INF), (1, 32, 550, -INF))        # (sequence, row, rope column, value): the LAST row of each sequence - causal hides it from token 0


def f_case(dt, seed=96000):
    """q (2, 2, 24, 576), the clean cache (2, 112, 1, 576), the cache with +inf / -inf in one rope column of one visible row per sequence, and sparse lists
    (2, 2, 64) in which token 1 names that row and token 0 does not"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(2, F_SQ, F_H, DK, generator=gen).to(dt)
    kv = torch.randn(2, F_CAP, 1, DK, generator=gen).to(dt)
    bad = kv.clone()
    idx = torch.full((2, F_SQ, F_TOPK), -1, dtype=torch.int32)
    for i, row, colr, val in F_POS:
        bad[i, row, 0, colr] = val
        L = F_LENS[i]
        for t in range(F_SQ):
            n = min(L - 1, 40)
            keys = torch.randperm(L - 1, generator=gen)[:n].to(torch.int32)          # rows 0 .. L - 2: never the bad row
            slots = torch.randperm(F_TOPK, generator=gen)[:n + 1]
            idx[i, t, slots[:n]] = keys
            if t == 1:
                idx[i, t, slots[n]] = row
    return q, kv, bad, idx


# ---- G ---------------------------------------------------------------------------------------------------------------------------------------------------

G_LENS, G_CAP, G_P = [100, 33], 112, 16        # 7 pages a sequence
G_POOL = {ROW16: 233100, ROW8: 409300}         # pages of 16 rows: 18432 B x 233100 and 10496 B x 409300 are both just above 2^32 bytes
G_LONGEST = {ROW16: 1864128, ROW8: 3273600}    # the longest capacity (a multiple of 16) with capacity x row bytes < 2^31


def g_pages(row_bytes, base):
    """(2, 7) page numbers of a pool of G_POOL pages of 16 rows that starts at address `base`: page 0, the last page, the pages that hold byte offsets 2^31
    and 2^32 and their two neighbours, and the first other page whose start ADDRESS base + offset has bit 31 of its low word set under a non-zero high
    word (a pool larger than 4 GiB has one wherever it starts); the rest spread between.  Sequence 0 needs its 7 pages, sequence 1 three (L = 33); the pages
    the append of the GPU test writes - entry [0, 6] and entries [1, 1], [1, 2] - are the page at 2^32, the last page and the page behind 2^32."""
    pb, n = row_bytes * G_P, G_POOL[row_bytes]
    p31, p32 = 2 ** 31 // pb, 2 ** 32 // pb
    fixed = [0, p31 - 1, p31, p31 + 1, p32 - 1, p32, p32 + 1, n - 1, n // 7, n // 3 + 1, 5 * n // 7, 6 * n // 7 + 3, 12345]
    assert len(set(fixed)) == 13 and max(fixed) == n - 1
    sign = next(p for p in range(n) if p not in fixed and (base + p * pb) >> 32 and (base + p * pb) & 0x80000000)
    first, b31, at31, a31, b32, at32, a32, last, r0, r1, r2, r3, r4 = fixed
    return torch.tensor([[first, b31, at31, a31, b32, sign, at32], [r0, last, a32, r1, r2, r3, r4]], dtype=torch.int32)


def f_dense_ref(q, kv, causal):
    """fp64 math with IEEE propagation (_util.fp64_math) per sequence: O (2, 2, 24, 512), LSE (2, 24, 2)"""
    import _util as U

    r = [U.fp64_math(q[i], kv[i, :L], kv[i, :L, :, :DV], causal) for i, L in enumerate(F_LENS)]
    return torch.stack([o for o, _ in r]), torch.stack([l for _, l in r])


def f_sparse_ref(q, kv, idx):
    """the same over the rows each token's list names (every entry of f_case's lists is -1 or valid)"""
    import _util as U

    o = torch.zeros(2, F_SQ, F_H, DV, dtype=torch.float64)
    lse = torch.zeros(2, F_H, F_SQ, dtype=torch.float64)
    for i in range(2):
        for t in range(F_SQ):
            rows = kv[i, idx[i, t][idx[i, t] >= 0].long()]
            ot, lt = U.fp64_math(q[i, t:t + 1], rows, rows[..., :DV], False)
            o[i, t], lse[i, :, t] = ot[0], lt[:, 0]
    return o, lse
