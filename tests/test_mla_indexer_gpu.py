"""GPU: the DeepSeek-V3.2 indexer (flash_mla_indexer_logits, flash_mla_indexer_topk, flash_mla_index_with_kvcache; fa_run_mla_indexer_logits /
fa_run_mla_indexer_topk).

Logits: on integer data fp32 math is exact in any order, so the kernel must equal the fp64 model bit for bit; on N(0, 1) data it is held to
2^-15 x the magnitude of the sum (tests/_mla_indexer_cases.py TOL; the CPU test shows that the bound bites).  Everything else is a relation that
holds to the bit.  The selection is compared for equality with the integer model.  Shapes are the smallest at which the kernels can go wrong: lengths
around the 32-key step over a capacity of 320, pages of 16 and 64, one and three tokens, 16 and 64 heads."""
import zlib

import numpy as np
import pytest
import torch

import _mla_indexer_cases as C
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
LENS2 = [(0, 257), (1, 100), (31, 33), (32, 320)]         # b = 2: every length of C.LENS, and the full capacity


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _lens_t(lens, dev):
    return torch.tensor(lens, dtype=torch.int32, device=dev)


def _run(dev, q, w, k, sc, lens, causal, page=None, gen=None):
    """the public call on the device, contiguous or over a random paging of the same logical cache"""
    if page is None:
        return F.flash_mla_indexer_logits(q.to(dev), w.to(dev), k.to(dev), _lens_t(lens, dev), k_scale=None if sc is None else sc.to(dev), causal=causal)
    pool, spool, table = C.paginate(k, sc if sc is not None else torch.ones(k.shape[:2]), page, gen)
    return F.flash_mla_indexer_logits(q.to(dev), w.to(dev), pool.to(dev), _lens_t(lens, dev), k_scale=None if sc is None else spool.to(dev),
                                      block_table=table.to(dev), causal=causal)


def _masked(x, mask, fill=0.0):
    return torch.where(mask, x.cpu(), torch.full_like(x.cpu(), fill))


# ---- logits: exact ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16, 64])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("h", [16, 64])
@pytest.mark.parametrize("sq", [1, 3])
def test_logits_equal_fp64_bit_for_bit_on_integer_data(gpu, sq, h, dt, fp8, page):
    gen = _gen("exact", sq, h, dt, fp8, page)
    q, w, k, sc = C.exact_inputs(2, sq, h, DT[dt], fp8, gen)
    ref, _ = C.logits_model(q, w, k, sc)
    for lens in LENS2:
        for causal in (True, False):
            got = _run(gpu, q, w, k, sc, lens, causal, page, gen)
            mask = C.visible_mask(lens, sq, C.CAP, causal)
            assert got.shape == (2, sq, C.CAP) and got.dtype == torch.float32
            assert torch.equal(_masked(got, mask).double(), _masked(ref, mask)), (lens, causal)


# ---- logits: tolerance on N(0, 1) data -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16, 64])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("h", [16, 64])
@pytest.mark.parametrize("sq", [1, 3])
def test_logits_within_the_rounding_bound_on_normal_data(gpu, sq, h, dt, fp8, page):
    gen = _gen("normal", sq, h, dt, fp8, page)
    q, w, k, sc = C.normal_inputs(2, sq, h, DT[dt], fp8, gen)
    ref, mag = C.logits_model(q, w, k, sc)
    worst = 0.0
    for lens in LENS2:
        for causal in (True, False):
            got = _run(gpu, q, w, k, sc, lens, causal, page, gen)
            mask = C.visible_mask(lens, sq, C.CAP, causal)
            err = _masked((got.cpu().double() - ref).abs() / mag, mask)
            worst = max(worst, float(err.max()))
    print(f"indexer logits sq={sq} h={h} {dt} fp8={fp8} page={page}: worst |err| / magnitude = {worst:.3e} (bound {C.TOL:.3e})")
    assert worst <= C.TOL, worst


# ---- logits: relations that hold to the bit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8", [False, True])
def test_logits_relations_bit_for_bit(gpu, fp8):
    """paged == contiguous; run to run; a strided weights; k_scale as a view of one buffer that holds values and scales block by block"""
    gen = _gen("relations", fp8)
    sq, h, lens = 3, 64, (257, 100)
    q, w, k, sc = C.normal_inputs(2, sq, h, torch.bfloat16, fp8, gen)
    mask = C.visible_mask(lens, sq, C.CAP, True)
    base = _run(gpu, q, w, k, sc, lens, True)
    assert torch.equal(_masked(base, mask), _masked(_run(gpu, q, w, k, sc, lens, True), mask))
    for page in (16, 64):
        assert torch.equal(_masked(base, mask), _masked(_run(gpu, q, w, k, sc, lens, True, page, gen), mask)), page
    wide = torch.full((2, sq, 2 * h + 3), float("nan"))
    wide[:, :, 1:2 * h + 1:2] = w
    ws = wide.to(gpu)[:, :, 1:2 * h + 1:2]
    assert ws.stride(2) == 2
    got = F.flash_mla_indexer_logits(q.to(gpu), ws, k.to(gpu), _lens_t(lens, gpu), k_scale=sc.to(gpu), causal=True)
    assert torch.equal(_masked(base, mask), _masked(got, mask))
    # one buffer, block by block: 64 tokens x 128 value bytes, then 64 fp32 scales (the layout of an FP8 index cache with per-token scales)
    if fp8:
        P, blocks = 64, 2 * C.CAP // 64
        buf = torch.zeros(blocks, P * 128 + P * 4, dtype=torch.uint8)
        buf[:, :P * 128] = k.view(torch.uint8).reshape(blocks, P * 128)
        buf[:, P * 128:] = sc.reshape(blocks, P).contiguous().view(torch.uint8).reshape(blocks, P * 4)
        dbuf = buf.to(gpu)
        values = dbuf[:, :P * 128].view(torch.float8_e4m3fn).unflatten(1, (P, 128))
        scales = dbuf[:, P * 128:].view(torch.float32)
        assert values.stride(0) == P * 132 and scales.stride(0) == P * 33
        table = torch.arange(blocks, dtype=torch.int32).reshape(2, C.CAP // 64).to(gpu)
        got = F.flash_mla_indexer_logits(q.to(gpu), w.to(gpu), values, _lens_t(lens, gpu), k_scale=scales, block_table=table, causal=True)
        assert torch.equal(_masked(base, mask), _masked(got, mask))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16, 64])
def test_what_is_never_read_may_hold_nan(gpu, fp8, page):
    """NaN codes / elements and NaN scales in rows at or past L_i, in unreferenced pages (C.paginate's spare pages) and in pages wholly past L_i;
    garbage table entries past the needed pages: the visible logits keep their bits"""
    gen = _gen("never_read", fp8, page)
    sq, h, lens = 3, 64, (100, 33)
    q, w, k, sc = C.normal_inputs(2, sq, h, torch.float16, fp8, gen)
    mask = C.visible_mask(lens, sq, C.CAP, True)
    base = _run(gpu, q, w, k, sc, lens, True)
    kp, scp = k.clone(), sc.clone()
    raw = kp.view(torch.uint8) if fp8 else kp
    for i, L in enumerate(lens):
        raw[i, L:] = 0x7F if fp8 else float("nan")
        scp[i, L:] = float("nan")
    if page is None:
        got = _run(gpu, q, w, kp, scp, lens, True)
    else:
        pool, spool, table = C.paginate(kp, scp, page, gen)
        garbage = torch.tensor([-1, 2 ** 31 - 1, -2 ** 31, 123456], dtype=torch.int32)
        for i, L in enumerate(lens):
            first = (L + page - 1) // page                  # the first column no visible key needs
            table[i, first:] = garbage.repeat(table.shape[1])[:table.shape[1] - first]
        got = F.flash_mla_indexer_logits(q.to(gpu), w.to(gpu), pool.to(gpu), _lens_t(lens, gpu), k_scale=spool.to(gpu), block_table=table.to(gpu), causal=True)
    assert torch.equal(_masked(base, mask), _masked(got, mask))
    assert torch.isfinite(_masked(got, mask)).all()


@pytest.mark.parametrize("causal", [True, False])
@pytest.mark.parametrize("page", [None, 16])
def test_entries_past_the_visible_length_are_never_written(gpu, page, causal):
    """through the C ABI, whose logits buffer is the caller's: every entry at j >= n_t keeps the sentinel, every visible one is written"""
    gen = _gen("sentinel", page, causal)
    sq, h = 3, 32
    q, w, k, sc = C.exact_inputs(2, sq, h, torch.bfloat16, True, gen)
    ref, _ = C.logits_model(q, w, k, sc)
    for lens in LENS2:
        logits = torch.full((2, sq, C.CAP), C.SENTINEL, dtype=torch.float32, device=gpu)
        if page is None:
            dk, dsc, table = k.to(gpu), sc.to(gpu), None
        else:
            pool, spool, table = C.paginate(k, sc, page, gen)
            dk, dsc, table = pool.to(gpu), spool.to(gpu), table.to(gpu)
        dq, dw, dl = q.to(gpu), w.to(gpu), _lens_t(lens, gpu)
        capi.run_mla_indexer_logits(capi.mla_indexer_params(dq, dw, dk, logits, dl, k_scale=dsc, block_table=table, causal=causal))
        torch.cuda.synchronize()
        mask = C.visible_mask(lens, sq, C.CAP, causal)
        want = torch.where(mask, ref, torch.full_like(ref, float(np.float32(C.SENTINEL))))
        assert torch.equal(logits.cpu().double(), want), lens


def test_logits_rows_past_two_gib(gpu):
    """b 5, sq 1, a paged cache of capacity 2^27 + 64 (a table of 8 MB a sequence over a small pool), L = 64: row 4 of logits starts at 2^31 bytes.
    The first 64 entries of every row equal those of the same call at a small capacity"""
    gen = _gen("offsets")
    b, h, P, L = 5, 64, 64, 64
    cols = (2 ** 27 + 64) // P
    q, w, k, sc = C.exact_inputs(b, 1, h, torch.bfloat16, True, gen, cap=P)
    dq, dw, dk, dsc, dl = q.to(gpu), w.to(gpu), k.to(gpu), sc.to(gpu), _lens_t([L] * b, gpu)
    small = F.flash_mla_indexer_logits(dq, dw, dk, dl, k_scale=dsc, block_table=torch.arange(b, dtype=torch.int32, device=gpu).view(b, 1), causal=True)
    table = torch.full((b, cols), 2 ** 31 - 1, dtype=torch.int32, device=gpu)
    table[:, 0] = torch.arange(b, dtype=torch.int32, device=gpu)
    big = F.flash_mla_indexer_logits(dq, dw, dk, dl, k_scale=dsc, block_table=table, causal=True)
    assert big.shape == (b, 1, cols * P) and big[4].data_ptr() - big.data_ptr() >= 2 ** 31
    assert torch.equal(big[:, :, :L], small[:, :, :L])
    ref, _ = C.logits_model(q, w, k, sc)
    assert torch.equal(small.cpu().double(), ref)
    idx = F.flash_mla_indexer_topk(big, dl, 32, causal=True)
    assert torch.equal(idx.cpu(), C.topk_model(small.cpu(), [L] * b, 32, True))


# ---- top-k -------------------------------------------------------------------------------------------------------------------------------------------

ROWS = C.topk_rows()


@pytest.mark.parametrize("name", sorted(ROWS))
def test_topk_equals_the_integer_model(gpu, name):
    row, n, topk = ROWS[name]
    x = torch.from_numpy(row.copy()).view(1, 1, -1)
    got = F.flash_mla_indexer_topk(x.to(gpu), n, topk, causal=True)
    want = torch.from_numpy(C.topk_row_model(row, n, topk)).view(1, 1, topk)
    assert got.dtype == torch.int32 and got.is_contiguous() and torch.equal(got.cpu(), want)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_topk_on_three_sequences_of_two_tokens(gpu, name):
    """every case on b 3 x sq 2: the visible entries of each row shuffled on their own, per-sequence lengths n, n - 1, n, with and without causal
    (under it token 0 sees one key less)"""
    row, n, topk = ROWS[name]
    rng = np.random.default_rng(7)
    x = np.stack([np.stack([row.copy() for _ in range(2)]) for _ in range(3)])
    for i in range(3):
        for t in range(2):
            x[i, t, :n] = rng.permutation(x[i, t, :n])
    lens = [n, max(n - 1, 0), n]
    for causal in (True, False):
        got = F.flash_mla_indexer_topk(torch.from_numpy(x).to(gpu), _lens_t(lens, gpu), topk, causal=causal)
        assert torch.equal(got.cpu(), C.topk_model(x, lens, topk, causal)), causal


def test_topk_over_a_padded_view_and_poison_past_n(gpu):
    """a logits view with a padded row stride; +inf and NaN at j >= n_t are never selected"""
    rng = np.random.default_rng(3)
    b, sq, cap, topk = 2, 2, 300, 32
    store = torch.full((b, sq, cap + 52), float("inf"))
    x = torch.from_numpy(rng.standard_normal((b, sq, cap)).astype(np.float32))
    lens = [200, 40]
    for i, L in enumerate(lens):
        x[i, :, L:] = float("nan")
        x[i, 0, L - 1] = float("inf")       # causal hides the last key from token 0
    store[:, :, 7:7 + cap] = x
    view = store.to(gpu)[:, :, 7:7 + cap]
    assert view.stride(1) == cap + 52 and not view.is_contiguous()
    got = F.flash_mla_indexer_topk(view, _lens_t(lens, gpu), topk, causal=True)
    want = C.topk_model(x, lens, topk, True)
    assert torch.equal(got.cpu(), want)
    assert int(got[0, 0].max()) < lens[0] - 1


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8_latent", [False, True])
def test_indices_feed_the_sparse_call_and_give_the_dense_causal_bits(gpu, fp8_latent):
    """L_i <= topk, sq 2, causal: the produced lists are 0 .. n_t - 1 padded with -1, and the sparse call on them equals flash_mla_with_kvcache(causal=True)
    bit for bit in out and lse (the identity-list relation), over a 16-bit and a 656-byte latent cache"""
    gen = _gen("e2e", fp8_latent)
    b, sq, h, cap, topk = 2, 2, 16, 128, 64
    lens = [64, 37]
    dl = _lens_t(lens, gpu)
    q_idx, w, k, sc = C.normal_inputs(b, sq, 64, torch.bfloat16, True, gen, cap=cap)
    idx = F.flash_mla_index_with_kvcache(q_idx.to(gpu), w.to(gpu), k.to(gpu), dl, topk, k_scale=sc.to(gpu), causal=True)
    want = torch.full((b, sq, topk), -1, dtype=torch.int32)
    for i, L in enumerate(lens):
        for t in range(sq):
            n = C.visible(L, sq, t, True, cap)
            want[i, t, :n] = torch.arange(n, dtype=torch.int32)
    assert torch.equal(idx.cpu(), want)
    q = (torch.randn(b, sq, h, 576, generator=gen) * 0.5).to(torch.bfloat16).to(gpu)
    kv = (torch.randn(b, cap, 1, 576, generator=gen) * 0.5).to(torch.bfloat16).to(gpu)
    if fp8_latent:
        kv = F.quantize_mla_kv_cache(kv)
    so, sl = F.flash_mla_sparse_with_kvcache(q, kv, dl, idx, num_splits=1, return_softmax_lse=True)
    do, dlse = F.flash_mla_with_kvcache(q, kv, dl, causal=True, num_splits=1, return_softmax_lse=True)
    assert torch.equal(so, do) and torch.equal(sl, dlse)


def test_convenience_call_equals_the_two_calls(gpu):
    gen = _gen("conv")
    b, sq, cap, topk = 2, 3, 320, 32
    lens = [257, 100]
    q, w, k, sc = C.normal_inputs(b, sq, 64, torch.float16, True, gen)
    pool, spool, table = C.paginate(k, sc, 16, gen)
    args = (q.to(gpu), w.to(gpu), pool.to(gpu), _lens_t(lens, gpu))
    kw = dict(k_scale=spool.to(gpu), block_table=table.to(gpu))
    for causal in (True, False):
        logits = F.flash_mla_indexer_logits(*args, causal=causal, **kw)
        idx = F.flash_mla_indexer_topk(logits, args[3], topk, causal=causal)
        got, lg = F.flash_mla_index_with_kvcache(*args, topk, causal=causal, return_logits=True, **kw)
        only = F.flash_mla_index_with_kvcache(*args, topk, causal=causal, **kw)
        mask = C.visible_mask(lens, sq, cap, causal)
        assert torch.equal(got, idx) and torch.equal(only, idx) and torch.equal(_masked(lg, mask), _masked(logits, mask))
        assert torch.equal(idx.cpu(), C.topk_model(logits.cpu(), lens, topk, causal))


def test_graph_replay_reads_the_lengths_then_in_memory(gpu):
    """all three calls captured in one graph; cache_seqlens changes in place; the replay equals the eager calls on the new lengths"""
    gen = _gen("graph")
    b, sq, cap, topk = 2, 2, 320, 32
    q, w, k, sc = C.normal_inputs(b, sq, 64, torch.bfloat16, True, gen)
    dq, dw, dk, dsc = q.to(gpu), w.to(gpu), k.to(gpu), sc.to(gpu)
    dl = _lens_t([100, 257], gpu)

    def calls():
        lg = F.flash_mla_indexer_logits(dq, dw, dk, dl, k_scale=dsc, causal=True)
        return lg, F.flash_mla_indexer_topk(lg, dl, topk, causal=True), F.flash_mla_index_with_kvcache(dq, dw, dk, dl, topk, k_scale=dsc, causal=True)

    calls()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_lg, g_idx, g_both = calls()
    dl.copy_(_lens_t([301, 33], gpu))
    graph.replay()
    torch.cuda.synchronize()
    e_lg, e_idx, e_both = calls()
    mask = C.visible_mask([301, 33], sq, cap, True)
    assert torch.equal(g_idx, e_idx) and torch.equal(g_both, e_both) and torch.equal(g_idx, g_both)
    assert torch.equal(_masked(g_lg, mask), _masked(e_lg, mask))
    assert torch.equal(e_idx.cpu(), C.topk_model(e_lg.cpu(), [301, 33], topk, True))


# ---- one speed relation --------------------------------------------------------------------------------------------------------------------------

def torch_indexer(q, w, k8, sc, topk):
    """the indexer in torch ops: dequantise, einsum, relu, weighted sum, * k_scale, torch.topk (full lengths, no mask)"""
    kf = k8.to(q.dtype)
    s = torch.einsum("bthd,bjd->bthj", q, kf).float()
    logits = torch.einsum("bth,bthj->btj", w, torch.relu(s)) * sc.unsqueeze(1)
    return torch.topk(logits, topk, dim=-1).indices


def test_index_call_is_no_slower_than_the_torch_formulation(gpu):
    """b 8, L 32768, h 64, FP8 keys, topk 2048, bf16: median of 5 interleaved rounds, no margin - the torch path writes and re-reads the
    (b, sq, 64, L) tensor this call exists to avoid"""
    gen = _gen("speed")
    b, L, topk = 8, 32768, 2048
    q = torch.randn(b, 1, 64, 128, generator=gen).to(torch.bfloat16).to(gpu)
    w = torch.randn(b, 1, 64, generator=gen).to(gpu)
    k8 = torch.randn(b, L, 128, generator=gen).to(gpu).to(torch.float8_e4m3fn)
    sc = (torch.rand(b, L, generator=gen) + 0.5).to(gpu)
    dl = _lens_t([L] * b, gpu)
    ours = lambda: F.flash_mla_index_with_kvcache(q, w, k8, dl, topk, k_scale=sc, causal=True)
    theirs = lambda: torch_indexer(q, w, k8, sc, topk)

    def timed(fn, reps=5):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / reps

    for fn in (ours, theirs):
        timed(fn, 2)
    t_ours, t_theirs = [], []
    for _ in range(5):
        t_ours.append(timed(ours))
        t_theirs.append(timed(theirs))
    ratio = float(np.median(t_ours) / np.median(t_theirs))
    print(f"flash_mla_index_with_kvcache {np.median(t_ours) * 1e3:.1f} us, torch formulation {np.median(t_theirs) * 1e3:.1f} us, ratio {ratio:.3f}")
    assert ratio <= 1.0, ratio
