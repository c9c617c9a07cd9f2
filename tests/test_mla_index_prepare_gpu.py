"""GPU: the indexer's front end (flash_mla_index_prepare_queries, flash_mla_index_prepare_append) against rotate_mla_index_rows / fp64 torch and the two existing
quantisers.  Integer data makes every partial sum of the transform exact, so those tests compare bytes; random data is held to a bound made of format half-ulps
and the fp32 sum's worst case, which the torch reference path has to meet on the same inputs before the kernel is asked to."""
import pytest
import torch

import flash_attn_turing as F

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
B, CAP, PAGE, SENT = 4, 48, 16, 0xA5        # the append test: sequences, capacity, page size, the byte both buffers are filled with
DF = pytest.mark.parametrize("dtype,fmt", [(d, f) for d in (torch.float16, torch.bfloat16) for f in ("fp32", "ue8m0")])
HSIGN = torch.tensor([[bin(c & d).count("1") & 1 for d in range(128)] for c in range(128)], dtype=torch.uint8)      # 1 where H[c][d] = -1


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8)


def _ints(shape, seed):
    return torch.randint(-7, 8, shape, generator=torch.Generator().manual_seed(seed)).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("v", [1, 3, -2])
def test_the_sign_matrix_exactly(gpu, dtype, v):
    """row d = v e_d: every rotated entry is +-round_T(fl32(v * 128 ** -0.5)), so every code is 0x7e / 0xfe and its sign bit is H[d][c]'s: all 128 x 128 signs"""
    q, w = (v * torch.eye(128)).to(dtype).view(8, 16, 128), torch.ones(8, 16)
    codes, w8 = F.flash_mla_index_prepare_queries(q.to(gpu), w.to(gpu))
    codes = codes.cpu().view(128, 128)
    assert torch.equal(codes & 0x7F, torch.full((128, 128), 0x7E, dtype=torch.uint8))
    assert torch.equal(codes >> 7, HSIGN ^ int(v < 0))
    assert torch.equal(_bits(w8), _bits(F.quantize_mla_index_queries(F.rotate_mla_index_rows(q), w)[1]))


@DF
@pytest.mark.parametrize("tokens,heads", [(1, 1), (1, 15), (17, 1), (3, 64), (65, 16)])
def test_integer_data_byte_for_byte(gpu, tokens, heads, dtype, fmt):
    """integers in [-7, 7]: sums stay at or below 896, exact in any order.  q_idx is a token-strided view over NaN-filled gaps, weights a strided view"""
    rows = _ints((tokens * heads, 128), 100 * tokens + heads)
    if tokens * heads >= 3:
        rows[1] = 0                             # an all-zero row: scale 2^-24 / 448
        rows[2] = rows[2].clamp(-1, 1)          # a row whose amax is 1
    buf = torch.full((tokens, 2, heads, 128), float("nan"))
    buf[:, 0] = rows.view(tokens, heads, 128)
    buf = buf.to(dtype)
    wbuf = torch.randn(tokens, heads, 2, generator=torch.Generator().manual_seed(7))
    q, w = buf[:, 0], wbuf[..., 0]
    want_codes, want_w8 = F.quantize_mla_index_queries(F.rotate_mla_index_rows(q), w, fmt)
    codes, w8 = F.flash_mla_index_prepare_queries(buf.to(gpu)[:, 0], wbuf.to(gpu)[..., 0], scale_format=fmt)
    assert codes.shape == q.shape and codes.dtype == torch.uint8 and codes.is_contiguous() and w8.shape == w.shape and w8.is_contiguous()
    assert torch.equal(codes.cpu(), want_codes) and torch.equal(_bits(w8), _bits(want_w8))


@DF
def test_without_rotation_every_pattern_is_the_torch_quantiser(gpu, dtype, fmt):
    """all 65536 bit patterns as 512 rows, and the same patterns transposed so that every row mixes NaN, inf, subnormals and finite values"""
    pats = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)
    q = torch.cat([pats.view(512, 128), pats.view(128, 512).T.contiguous()]).view(64, 16, 128)
    w = torch.randn(64, 16, generator=torch.Generator().manual_seed(3))
    want_codes, want_w8 = F.quantize_mla_index_queries(q, w, fmt)
    codes, w8 = F.flash_mla_index_prepare_queries(q.to(gpu), w.to(gpu), hadamard=False, scale_format=fmt)
    assert torch.equal(codes.cpu(), want_codes) and torch.equal(_bits(w8), _bits(want_w8))


def _within_the_bound(x, codes, scale, fmt):
    """the issue's bound: every term is a format's half-ulp (e4m3: 2^-4 relative, 2^-10 scale absolute; T: u relative, twice) or the fp32 sum's worst case (2^-16 S)"""
    u = 2.0 ** -9 if x.dtype == torch.bfloat16 else 2.0 ** -11
    y64 = (x.double() @ (1.0 - 2.0 * HSIGN.double())) * 128 ** -0.5
    S = (128 ** -0.5 * x.double().abs().sum(-1, keepdim=True))
    scale = scale.double().unsqueeze(-1)
    err = (codes.view(torch.float8_e4m3fn).double() * scale - y64).abs()
    ok = bool((err <= (2.0 ** -4 + 2 * u) * y64.abs() + 2.0 ** -10 * scale + 2.0 ** -16 * S).all())
    amax = y64.abs().amax(-1, keepdim=True)
    lo = torch.clamp(amax * (1 - 2 * u) - 2.0 ** -16 * S, min=2.0 ** -24) * (1 - 2.0 ** -23)
    hi = torch.clamp(amax * (1 + 2 * u) + 2.0 ** -16 * S, min=2.0 ** -24) * (1 + 2.0 ** -23)
    if fmt == "fp32":
        return ok and bool(((448 * scale >= lo) & (448 * scale <= hi)).all())
    pow2ceil = lambda v: 2.0 ** torch.ceil(torch.log2(v))
    return ok and bool(((scale == pow2ceil(scale)) & (scale >= pow2ceil(lo / 448)) & (scale <= pow2ceil(hi / 448))).all())


@DF
def test_the_bound_on_random_finite_data(gpu, dtype, fmt):
    """16 rows each of N(0, 1), N(0, 1) x 2^12, N(0, 1) x 2^-12 and N(0, 1) with one element x 1000; weights of 1, so that w8 is the scale"""
    x = torch.randn(4, 16, 128, generator=torch.Generator().manual_seed(11))
    x[1] *= 2.0 ** 12
    x[2] *= 2.0 ** -12
    x[3, torch.arange(16), 5 * torch.arange(16)] *= 1000.0
    x, w = x.to(dtype), torch.ones(4, 16)
    assert _within_the_bound(x, *F.quantize_mla_index_queries(F.rotate_mla_index_rows(x), w, fmt), fmt), "the torch reference path misses the bound: the bound is wrong"
    codes, w8 = F.flash_mla_index_prepare_queries(x.to(gpu), w.to(gpu), scale_format=fmt)
    assert _within_the_bound(x, codes.cpu(), w8.cpu(), fmt)


@DF
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("paged", [False, True])
def test_the_append_is_the_existing_append_on_rotated_rows(gpu, paged, packed, dtype, fmt):
    """lengths 5 and 14: runs that cross the page edge at 16; -3: clamped to 0; 40: rows at or past the capacity are dropped.  Packed: an empty sequence and three
    surplus rows past cu[-1].  One table entry where a row lands is outside the pool: the clamp sends it to the pool's last page, which no other entry names"""
    lens = torch.tensor([5, -3, 40, 14], dtype=torch.int32)
    counts = [12, 0, 10, 7] if packed else [12] * B
    k_new = _ints((sum(counts) + 3, 128) if packed else (B, 12, 128), 40 + packed).to(dtype)
    if packed:
        k_new[-3:] = float("nan")
    kw = dict(scale_format=fmt)
    if packed:
        kw["cu_seqlens_new"] = torch.tensor([0, 12, 12, 22, 29], dtype=torch.int32, device=gpu)
    if paged:
        table = torch.randperm(B * CAP // PAGE, generator=torch.Generator().manual_seed(5)).view(B, CAP // PAGE).to(torch.int32)
        table[0, 1] = 1000
        kw["block_table"] = table.to(gpu)
    shape = (B * CAP // PAGE + 2, PAGE) if paged else (B, CAP)
    out = []
    for fn, rows in ((F.flash_mla_index_prepare_append, k_new), (F.flash_mla_index_cache_append, F.rotate_mla_index_rows(k_new))):
        cache, sbuf = torch.full(shape + (128,), SENT, dtype=torch.uint8, device=gpu), torch.full(shape + (8,), SENT, dtype=torch.uint8, device=gpu).view(torch.float32)
        assert fn(cache, rows.to(gpu), lens.to(gpu), k_scale=sbuf[..., 0], **kw) is None
        out.append((cache.cpu(), _bits(sbuf)))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert (out[0][0] != SENT).any(-1).sum().item() == (12 + 0 + 8 + 7 if packed else 12 + 12 + 8 + 12)         # no vacuous pass: the rows the rules name were written


@DF
def test_it_feeds_the_indexer(gpu, dtype, fmt):
    """against the torch path (rotation reference, then the two quantisers), bit for bit; a captured append + prepare + logits replays with the inputs then in memory"""
    b, h, cap, n = 2, 16, 64, 40
    q, k, w = _ints((b, 1, h, 128), 1).to(dtype), _ints((b, n, 128), 2).to(dtype), torch.randn(b, 1, h, generator=torch.Generator().manual_seed(9))
    lens = torch.full((b,), n, dtype=torch.int32, device=gpu)

    def torch_path(q, k):
        codes, w8 = F.quantize_mla_index_queries(F.rotate_mla_index_rows(q), w, fmt)
        kc, ks = torch.zeros(b, cap, 128, dtype=torch.uint8), torch.zeros(b, cap)
        kc[:, :n], ks[:, :n] = F.quantize_mla_index_keys(F.rotate_mla_index_rows(k), fmt)
        return F.flash_mla_indexer_logits(codes.to(gpu), w8.to(gpu), kc.to(gpu), lens, k_scale=ks.to(gpu))[..., :n].cpu()

    qg, kg, wg = q.to(gpu), k.to(gpu), w.to(gpu)
    cache, scales, got = torch.zeros(b, cap, 128, dtype=torch.uint8, device=gpu), torch.zeros(b, cap, device=gpu), []
    at0 = torch.zeros(b, dtype=torch.int32, device=gpu)

    def ours():
        F.flash_mla_index_prepare_append(cache, kg, at0, k_scale=scales, scale_format=fmt)
        codes, w8 = F.flash_mla_index_prepare_queries(qg, wg, scale_format=fmt)
        got[:] = [F.flash_mla_indexer_logits(codes, w8, cache, lens, k_scale=scales)]

    ours()
    assert torch.equal(_bits(got[0][..., :n]), _bits(torch_path(q, k)))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ours()
    for seed in (21, 22):                   # two replays, each after the inputs changed in place
        q2, k2 = _ints((b, 1, h, 128), seed).to(dtype), _ints((b, n, 128), seed + 10).to(dtype)
        qg.copy_(q2)
        kg.copy_(k2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[0][..., :n]), _bits(torch_path(q2, k2)))
