"""Shared inputs and independent models of tests/test_mla_cache_io_cpu.py and tests/test_mla_cache_io_gpu.py: the integer model of placement, drop and clamp
of the two appends and of the gather's row selection, and the index-key quantiser in numpy, written from the rule and without flash_attn_turing."""
import numpy as np
import torch

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
CAP, B = 96, 4                                  # pages of 16 and of 48 both divide the capacity
PAGES = (16, 48)
LENS = (-3, 0, 1, 15, 16, 17, 47, 48, 95, 96)   # cache_seqlens are drawn from these
NEWS = (0, 1, 3, 5, 20)                         # new rows per sequence: appends cross pages, run past the capacity, leave a workgroup partly filled
STARTS = (0, 7, 16, 40, -2)
COUNTS = (0, 1, 5, 33, 96)

# (cache_seqlens, new rows per sequence) of the append tests: every length and every count occurs, 95 + 20 and 96 + 5 run past the capacity
APPEND_CASES = (((-3, 15, 47, 95), (3, 20, 5, 20)), ((0, 16, 48, 96), (1, 5, 20, 5)), ((1, 17, 95, 47), (20, 0, 3, 1)), ((96, 0, 17, 1), (1, 3, 0, 5)))
# (cache_seqlens, seq_starts, rows per sequence) of the gather tests
GATHER_CASES = (((-3, 15, 47, 95), (0, 7, 16, 40), (5, 33, 96, 1)), ((0, 16, 48, 96), (-2, 0, 40, 7), (1, 96, 5, 33)), ((1, 17, 96, 47), (0, 16, -2, 40), (0, 5, 96, 33)))


def placed_rows(cache_seqlens, counts, cap=CAP):
    """[(sequence, new row, logical position)] of the rows an append keeps: position max(len, 0) + s, dropped at or past the capacity"""
    return [(i, s, max(int(L), 0) + s) for i, (L, n) in enumerate(zip(cache_seqlens, counts)) for s in range(int(n)) if max(int(L), 0) + s < cap]


def gathered_rows(cache_seqlens, starts, counts, cap=CAP):
    """[(sequence, out row, logical position or None)]: position max(start, 0) + r, None (a row of +0) at or past L = min(max(len, 0), cap)"""
    out = []
    for i, n in enumerate(counts):
        L = cap if cache_seqlens is None else min(max(int(cache_seqlens[i]), 0), cap)
        st = 0 if starts is None else max(int(starts[i]), 0)
        out += [(i, r, st + r if st + r < L else None) for r in range(int(n))]
    return out


def physical(table, i, pos, page, num_blocks):
    """(page, row) of logical position pos of sequence i: entry clamped min(uint32(entry), num_blocks - 1)"""
    entry = int(table[i][pos // page]) & 0xFFFFFFFF
    return min(entry, num_blocks - 1), pos % page


def make_table(b, cap, page, num_blocks, seed):
    """a block table whose pages are distinct (a permutation of the pool), so that a paged cache holds exactly the rows of the contiguous one"""
    cols = cap // page
    assert b * cols <= num_blocks
    perm = torch.randperm(num_blocks, generator=torch.Generator().manual_seed(seed))[:b * cols]
    return perm.view(b, cols).to(torch.int32)


def to_pool(dense, table, page, num_blocks, fill):
    """dense (b, cap, ...) -> pool (num_blocks, page, ...) through the table; pages the table does not name hold `fill`"""
    b, cap = dense.shape[:2]
    pool = fill.expand(num_blocks, page, *dense.shape[2:]).clone() if isinstance(fill, torch.Tensor) else torch.full((num_blocks, page, *dense.shape[2:]), fill, dtype=dense.dtype)
    for i in range(b):
        for c in range(cap // page):
            pool[int(table[i, c])] = dense[i, c * page:(c + 1) * page]
    return pool


def from_pool(pool, table, page):
    """the logical (b, cap, ...) cache a table spells over a pool"""
    return torch.stack([torch.cat([pool[int(e)] for e in row]) for row in table])


def cu_of(counts):
    return torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32)


# ---- the index-key quantiser, from the rule -----------------------------------------------------------------------------------------------------------------

def _e4m3_nonneg():
    """float64 (127,): the values of the codes 0x00 .. 0x7e"""
    v = np.zeros(127)
    for c in range(127):
        e, m = c >> 3, c & 7
        v[c] = m / 8.0 * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return v


def bits_to_f32(bits_u16, dtname):
    bits_u16 = np.asarray(bits_u16, dtype=np.uint16)
    if dtname == "fp16":
        return bits_u16.view(np.float16).astype(np.float32)
    return (bits_u16.astype(np.uint32) << 16).view(np.float32)


def np_quantize_index_keys(bits_u16, dtname, scale_format="fp32"):
    """(n, 128) uint16 bit patterns of the dtype -> (codes uint8 (n, 128), scale float32 (n,)).  amax over the finite elements (0 if none), scale = max(amax,
    2^-24) / 448 in fp32, "ue8m0": rounded up to a power of two on the bits; code = e4m3 nearest-even of clamp(x / scale, -448, 448) by comparison with the
    midpoints of the code values; NaN -> 0x7f | sign; +-inf saturate."""
    x = bits_to_f32(bits_u16, dtname)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        finite = np.isfinite(x)
        amax = np.where(finite, np.abs(x), np.float32(0)).max(axis=-1).astype(np.float32)
        scale = (np.maximum(amax, np.float32(2.0 ** -24)) / np.float32(448.0)).astype(np.float32)
        if scale_format == "ue8m0":
            scale = ((scale.view(np.uint32) + np.uint32(0x007FFFFF)) & np.uint32(0x7F800000)).view(np.float32)
        else:
            assert scale_format == "fp32"
        y = (x / scale[:, None]).astype(np.float32)
        a = np.minimum(np.abs(y).astype(np.float64), 448.0)          # (NaN stays NaN; handled below)
    v = _e4m3_nonneg()
    mid = (v[:-1] + v[1:]) / 2
    a0 = np.where(np.isnan(a), 0.0, a)
    code = np.searchsorted(mid, a0, side="left")                      # the number of midpoints below |y|: the code unless |y| IS a midpoint
    tie = (code < 126) & (mid[np.minimum(code, 125)] == a0)
    code = np.where(tie & (code % 2 == 1), code + 1, code).astype(np.uint8)
    sign = ((np.asarray(bits_u16, dtype=np.uint16) >> 8) & 0x80).astype(np.uint8)
    code = np.where(np.isnan(x), np.uint8(0x7F), code) | sign
    return code.astype(np.uint8), scale


def pattern_rows(dtname):
    """(512, 128) of the dtype: all 65536 bit patterns, 128 consecutive ones a row (NaN and inf patterns included)"""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(512, 128).view(DT[dtname])


def amax_sweep_rows(dtname):
    """rows whose amax runs over 2^-30 (below the clamp; 0 in fp16) .. the largest finite value: per exponent one row with +-2^e at column e % 128 among smaller
    elements, then the largest finite value and the smallest subnormal"""
    dt = DT[dtname]
    top = 15 if dtname == "fp16" else 127
    rows = []
    frac = (torch.arange(128, dtype=torch.float64) * 37 % 128) / 128.0
    for e in range(-30, top + 1):
        r = (frac * 2.0 ** e * torch.where(torch.arange(128) % 3 == 0, -1.0, 1.0)).to(torch.float32)
        r[e % 128] = 2.0 ** e * (-1.0 if e % 2 else 1.0)
        rows.append(r.to(dt))
    big = torch.tensor([0x7BFF if dtname == "fp16" else 0x7F7F], dtype=torch.int16).view(dt)
    tiny = torch.tensor([0x0001], dtype=torch.int16).view(dt)
    exact = [torch.tensor([v]).to(dt) for v in (448.0, 7.0)]         # scale exactly 1 and 2^-6: powers of two that UE8M0 must leave as they are
    for edge in (big, tiny, *exact):
        r = torch.zeros(128, dtype=dt)
        r[5] = edge[0]
        rows.append(r)
    return torch.stack(rows)


def nonfinite_rows(dtname):
    """(5, 128): only NaN, only +inf, only -inf, NaN / +-inf mixed, only 0xffff - no finite element anywhere"""
    dt = DT[dtname]
    nan, inf = float("nan"), float("inf")
    mixed = torch.tensor([nan, inf, -inf, -nan] * 32)
    neg_nan = torch.full((128,), -1, dtype=torch.int16).view(dt)      # 0xffff: a NaN with the sign bit set
    return torch.stack([torch.full((128,), nan).to(dt), torch.full((128,), inf).to(dt), torch.full((128,), -inf).to(dt), mixed.to(dt), neg_nan])


def index_key_rows(dtname):
    """every row the quantiser tests use: 512 pattern rows, the amax sweep, the rows without a finite element"""
    return torch.cat([pattern_rows(dtname), amax_sweep_rows(dtname), nonfinite_rows(dtname)])


def u16(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)
