"""GPU: the prompt-chunk index logits (flash_mla_indexer_prefill_logits, flash_mla_index_prefill_with_kvcache; fa_run_mla_indexer_prefill_logits).

The contract is one relation: for every input the decode call (flash_mla_indexer_logits) accepts, the prefill call writes exactly the entries that call
writes, with the same bits, and no others - but for a NaN key, which reaches its column as a NaN here (the decode call's fmaxf leaves 0 there).  So the logits buffers are the caller's (the C ABI), pre-filled with a sentinel, and compared WHOLE with
torch.equal.  Next to it: the fp64 model (independent of the decode call), what is never read, where a NaN key goes, views, the composite call, graph
replay, the adversarial-timing builds and one speed relation.  Shapes are those of the decode suite (capacity 320, lengths around the 32-key step) with
sq around the tile of TQ tokens a workgroup serves (capi.mla_indexer_prefill_launch)."""
import ctypes
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

import _mla_indexer_cases as C
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
B = len(C.LENS)


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _lens_t(lens, dev):
    return torch.tensor(lens, dtype=torch.int32, device=dev)


def _tile():
    """TQ: the tokens of a workgroup's tile, from the host query"""
    q, w, k = torch.zeros(1, 1, 64, 128, dtype=torch.bfloat16), torch.zeros(1, 1, 64), torch.zeros(1, 64, 128, dtype=torch.uint8)
    lg, cs = torch.zeros(1, 1, 64), torch.zeros(1, dtype=torch.int32)
    tq = capi.mla_indexer_prefill_launch(capi.mla_indexer_params(q, w, k, lg, cs))[0]
    assert tq in (4, 8)
    return tq


TQ = _tile()
SQS = [1, TQ - 1, TQ, TQ + 1, 2 * TQ + 3]


def _device_cache(dev, k, sc, page, gen):
    """(k_idx_cache, k_scale, block_table) on the device: contiguous, or a random paging of the same logical cache (C.paginate: NaN spare pages)"""
    if page is None:
        return k.to(dev), None if sc is None else sc.to(dev), None
    pool, spool, table = C.paginate(k, sc if sc is not None else torch.ones(k.shape[:2]), page, gen)
    return pool.to(dev), None if sc is None else spool.to(dev), table.to(dev)


def _both(dev, dq, dw, dk, dsc, table, dl, causal, cap, row_stride=None):
    """(decode call, prefill call) into sentinel-filled buffers of the caller through the C ABI; row_stride: a logits row stride above the capacity"""
    out = []
    for run in (capi.run_mla_indexer_logits, capi.run_mla_indexer_prefill_logits):
        store = torch.full((dq.shape[0], dq.shape[1], row_stride or cap), C.SENTINEL, dtype=torch.float32, device=dev)
        run(capi.mla_indexer_params(dq, dw, dk, store[:, :, :cap], dl, k_scale=dsc, block_table=table, causal=causal))
        out.append(store)
    torch.cuda.synchronize()
    return out


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _sentinel_outside(x, mask):
    """every entry outside `mask` still holds the sentinel"""
    s = torch.tensor(C.SENTINEL, dtype=torch.float32)
    return bool((x.cpu()[~mask] == s).all())


# ---- equals the decode call ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16, 64])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("h", [16, 32, 64])
def test_equals_the_decode_call_in_every_entry(gpu, h, dt, fp8, page):
    """b 7 (C.LENS: sq > L under causal included), every sq around the tile, causal or not: the whole buffers, sentinels included"""
    for sq in SQS:
        gen = _gen("equal", sq, h, dt, fp8, page)
        q, w, k, sc = C.normal_inputs(B, sq, h, DT[dt], fp8, gen)
        dk, dsc, table = _device_cache(gpu, k, sc if fp8 else None, page, gen)
        dq, dw, dl = q.to(gpu), w.to(gpu), _lens_t(C.LENS, gpu)
        for causal in (True, False):
            dec, pre = _both(gpu, dq, dw, dk, dsc, table, dl, causal, C.CAP)
            assert torch.equal(dec, pre) and _same_bits(dec, pre), (sq, causal, int((dec != pre).sum()))
            mask = C.visible_mask(C.LENS, sq, C.CAP, causal)
            assert _sentinel_outside(pre, mask) and torch.isfinite(pre.cpu()[mask]).all(), (sq, causal)


# ---- independent of the decode call ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
@pytest.mark.parametrize("h", [16, 64])
def test_against_the_fp64_model(gpu, h, dt, fp8, page):
    """sq = 2 TQ + 3: within TOL x magnitude on N(0, 1) data, the fp64 model's bits on integer data"""
    sq = 2 * TQ + 3
    dl = _lens_t(C.LENS, gpu)
    for kind, make in (("normal", C.normal_inputs), ("exact", C.exact_inputs)):
        gen = _gen("model", kind, h, dt, fp8, page)
        q, w, k, sc = make(B, sq, h, DT[dt], fp8, gen)
        ref, mag = C.logits_model(q, w, k, sc)
        dk, dsc, table = _device_cache(gpu, k, sc, page, gen)
        for causal in (True, False):
            got = F.flash_mla_indexer_prefill_logits(q.to(gpu), w.to(gpu), dk, dl, k_scale=dsc, block_table=table, causal=causal).cpu().double()
            mask = C.visible_mask(C.LENS, sq, C.CAP, causal)
            if kind == "exact":
                assert torch.equal(got[mask], ref[mask]), causal
            else:
                worst = float(((got - ref).abs() / mag)[mask].max())
                print(f"prefill logits h={h} {dt} fp8={fp8} page={page} causal={causal}: worst |err| / magnitude = {worst:.3e} (bound {C.TOL:.3e})")
                assert worst <= C.TOL, worst


# ---- several key ranges and the early return ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8,page", [(True, 64), (False, None)])
def test_several_key_ranges_and_the_early_return(gpu, fp8, page):
    """b 1, capacity 4160, sq = TQ + 1: a launch of two tiles is spread over at least two key ranges; with L = 33 or 0 every range but the first (or every
    range) returns before its first barrier and writes nothing"""
    cap, sq = 4160, TQ + 1
    gen = _gen("chunks", fp8, page)
    q, w, k, sc = C.normal_inputs(1, sq, 64, torch.bfloat16, fp8, gen, cap=cap)
    dk, dsc, table = _device_cache(gpu, k, sc if fp8 else None, page, gen)
    dq, dw = q.to(gpu), w.to(gpu)
    probe = torch.empty(1, sq, cap, device=gpu)
    tq, wg, nc = capi.mla_indexer_prefill_launch(capi.mla_indexer_params(dq, dw, dk, probe, _lens_t([cap], gpu), k_scale=dsc, block_table=table))
    assert tq == TQ and nc >= 2 and wg % 32 == 0 and nc * wg >= cap, (tq, wg, nc)
    for L in (cap, 33, 0):
        dec, pre = _both(gpu, dq, dw, dk, dsc, table, _lens_t([L], gpu), True, cap)
        assert torch.equal(dec, pre) and _same_bits(dec, pre), L
        mask = C.visible_mask([L], sq, cap, True)
        assert _sentinel_outside(pre, mask) and torch.isfinite(pre.cpu()[mask]).all(), L
        assert int(mask.sum()) == sum(C.visible(L, sq, t, True, cap) for t in range(sq))


# ---- what is never read ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("page", [None, 16, 64])
def test_what_is_never_read_may_hold_nan(gpu, fp8, page):
    """NaN codes / elements and NaN scales in rows at or past L_i, in unreferenced pages (C.paginate's spare pages) and in pages wholly past L_i; table
    entries of those pages -1 and INT_MAX: the result is unchanged and finite"""
    gen = _gen("never_read", fp8, page)
    sq, h, lens = 2 * TQ + 3, 64, (100, 33)
    q, w, k, sc = C.normal_inputs(2, sq, h, torch.float16, fp8, gen)
    dq, dw, dl = q.to(gpu), w.to(gpu), _lens_t(lens, gpu)
    mask = C.visible_mask(lens, sq, C.CAP, True)
    dk, dsc, table = _device_cache(gpu, k, sc, page, gen)
    _, base = _both(gpu, dq, dw, dk, dsc, table, dl, True, C.CAP)
    kp, scp = k.clone(), sc.clone()
    raw = kp.view(torch.uint8) if fp8 else kp
    for i, L in enumerate(lens):
        raw[i, L:] = 0x7F if fp8 else float("nan")
        scp[i, L:] = float("nan")
    dk, dsc, table = _device_cache(gpu, kp, scp, page, gen)
    if page is not None:
        garbage = torch.tensor([-1, 2 ** 31 - 1], dtype=torch.int32, device=gpu)
        for i, L in enumerate(lens):
            first = (L + page - 1) // page                  # the first column no visible key needs
            table[i, first:] = garbage.repeat(table.shape[1])[:table.shape[1] - first]
    dec, got = _both(gpu, dq, dw, dk, dsc, table, dl, True, C.CAP)
    assert torch.equal(base, got) and torch.equal(dec, got)
    assert torch.isfinite(got.cpu()[mask]).all() and _sentinel_outside(got, mask)


def _nan_key_case(gpu, fp8):
    """(clean prefill run, decode and prefill runs with key j = 90 all NaN, the (b, sq) mask of the tokens that see it, j): b 2, L 100 and 257, sq = 2 TQ + 3"""
    gen = _gen("nan_key", fp8)
    sq, h, lens, j = 2 * TQ + 3, 64, (100, 257), 90
    q, w, k, sc = C.normal_inputs(2, sq, h, torch.bfloat16, fp8, gen)
    dq, dw, dl = q.to(gpu), w.to(gpu), _lens_t(lens, gpu)
    _, base = _both(gpu, dq, dw, k.to(gpu), sc.to(gpu), None, dl, True, C.CAP)
    kp = k.clone()
    raw = kp.view(torch.uint8) if fp8 else kp
    raw[:, j] = 0x7F if fp8 else float("nan")
    dec, got = _both(gpu, dq, dw, kp.to(gpu), sc.to(gpu), None, dl, True, C.CAP)
    sees = C.visible_mask(lens, sq, C.CAP, True)[:, :, j]                  # tokens with n_t > j
    assert sees.any() and not sees.all()
    return base.cpu(), dec.cpu(), got.cpu(), sees, j


@pytest.mark.parametrize("fp8", [False, True])
def test_a_nan_key_stays_in_its_column(gpu, fp8):
    """one NaN key j below L gives NaN in its column for the tokens that see it; every other entry keeps its bits - those of the clean run and those of the
    decode call on the same poisoned cache.  (In column j the decode call leaves 0: its ReLU is fmaxf, which drops a NaN; the prefill kernel's keeps it.)"""
    base, dec, got, sees, j = _nan_key_case(gpu, fp8)
    col = got[:, :, j]
    print(f"NaN key {j}: {int(torch.isnan(col[sees]).sum())} NaN among the {int(sees.sum())} tokens that see it (decode call: {int(torch.isnan(dec[:, :, j][sees]).sum())})")
    assert torch.isnan(col[sees]).all()
    other = torch.ones(C.CAP, dtype=torch.bool)
    other[j] = False
    assert _same_bits(got[:, :, other], base[:, :, other]) and _same_bits(got[:, :, other], dec[:, :, other])
    assert _same_bits(col[~sees], base[:, :, j][~sees]) and _same_bits(col[~sees], dec[:, :, j][~sees])


# ---- strided views -------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp8", [False, True])
def test_strided_views_the_checks_accept(gpu, fp8):
    """a padded key row stride, k_scale as a [:, ::2] view, q_idx sliced from a wider buffer, a logits row stride above the capacity"""
    gen = _gen("views", fp8)
    sq, h = 2 * TQ + 3, 32
    q, w, k, sc = C.normal_inputs(B, sq, h, torch.float16, fp8, gen)
    dl = _lens_t(C.LENS, gpu)
    plain_dec, plain = _both(gpu, q.to(gpu), w.to(gpu), k.to(gpu), sc.to(gpu), None, dl, True, C.CAP)
    kraw = k.view(torch.uint8) if fp8 else k
    kwide = torch.full((B, C.CAP, 128 + 32), 0x7F if fp8 else float("nan"), dtype=kraw.dtype)
    kwide[:, :, :128] = kraw
    dkv = kwide.to(gpu)[:, :, :128]
    scw = torch.full((B, 2 * C.CAP), float("nan"))
    scw[:, ::2] = sc
    dscv = scw.to(gpu)[:, ::2]
    qw = torch.full((B, sq, h + 2, 128 + 16), float("nan")).to(q.dtype)
    qw[:, :, 1:h + 1, 8:136] = q
    dqv = qw.to(gpu)[:, :, 1:h + 1, 8:136]
    assert dkv.stride(1) == 160 and dscv.stride(1) == 2 and dqv.stride(2) == 144 and not dqv.is_contiguous()
    dec, pre = _both(gpu, dqv, w.to(gpu), dkv, dscv, None, dl, True, C.CAP, row_stride=C.CAP + 37)
    assert torch.equal(dec, pre) and _same_bits(dec, pre)
    assert torch.equal(pre[:, :, :C.CAP], plain) and bool((pre[:, :, C.CAP:] == torch.tensor(C.SENTINEL, dtype=torch.float32)).all())
    assert torch.equal(plain_dec, plain)
    # the public call on the same views
    got = F.flash_mla_indexer_prefill_logits(dqv, w.to(gpu), dkv, dl, k_scale=dscv, causal=True)
    mask = C.visible_mask(C.LENS, sq, C.CAP, True)
    assert torch.equal(got.cpu()[mask], plain.cpu()[mask])


# ---- the composite call ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("topk", [32, 64])
def test_composite_equals_the_decode_composite(gpu, topk):
    gen = _gen("composite", topk)
    sq = 2 * TQ + 3
    q, w, k, sc = C.normal_inputs(B, sq, 64, torch.bfloat16, True, gen)
    pool, spool, table = C.paginate(k, sc, 16, gen)
    args = (q.to(gpu), w.to(gpu), pool.to(gpu), _lens_t(C.LENS, gpu))
    kw = dict(k_scale=spool.to(gpu), block_table=table.to(gpu))
    for causal in (True, False):
        want, want_lg = F.flash_mla_index_with_kvcache(*args, topk, causal=causal, return_logits=True, **kw)
        got, got_lg = F.flash_mla_index_prefill_with_kvcache(*args, topk, causal=causal, return_logits=True, **kw)
        only = F.flash_mla_index_prefill_with_kvcache(*args, topk, causal=causal, **kw)
        mask = C.visible_mask(C.LENS, sq, C.CAP, causal)
        assert got.dtype == torch.int32 and got.shape == (B, sq, topk) and torch.equal(got, want) and torch.equal(only, want)
        assert got_lg.shape == (B, sq, C.CAP) and torch.equal(got_lg.cpu()[mask], want_lg.cpu()[mask])
        assert torch.equal(got.cpu(), C.topk_model(got_lg.cpu(), C.LENS, topk, causal))
        for i, L in enumerate(C.LENS):          # L <= topk: 0 .. n_t - 1, then -1
            if L <= topk:
                for t in range(sq):
                    n = C.visible(L, sq, t, causal, C.CAP)
                    assert got[i, t].cpu().tolist() == list(range(n)) + [-1] * (topk - n), (i, t)


# ---- graph replay ------------------------------------------------------------------------------------------------------------------------------------------

def test_graph_replay_reads_lengths_and_table_then_in_memory(gpu):
    gen = _gen("graph")
    sq, topk = 2 * TQ + 3, 32
    q, w, k, sc = C.normal_inputs(2, sq, 64, torch.bfloat16, True, gen)
    pool, spool, table = C.paginate(k, sc, 64, gen)
    dq, dw, dk, dsc, dt = q.to(gpu), w.to(gpu), pool.to(gpu), spool.to(gpu), table.to(gpu)
    dl = _lens_t([100, 257], gpu)

    def calls():
        return (F.flash_mla_indexer_prefill_logits(dq, dw, dk, dl, k_scale=dsc, block_table=dt, causal=True),
                F.flash_mla_index_prefill_with_kvcache(dq, dw, dk, dl, topk, k_scale=dsc, block_table=dt, causal=True))

    calls()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        calls()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_lg, g_idx = calls()
    dl.copy_(_lens_t([301, 33], gpu))
    dt.copy_(dt.flip(1).contiguous())           # the same pages in another order: another logical cache
    graph.replay()
    torch.cuda.synchronize()
    e_lg, e_idx = calls()
    ref = F.flash_mla_index_with_kvcache(dq, dw, dk, dl, topk, k_scale=dsc, block_table=dt, causal=True)
    mask = C.visible_mask([301, 33], sq, C.CAP, True)
    assert torch.equal(g_idx, e_idx) and torch.equal(g_idx, ref)
    assert torch.equal(g_lg.cpu()[mask], e_lg.cpu()[mask])


# ---- the stage protocol under adversarial timing ----------------------------------------------------------------------------------------------------------

TIMING = ("stage_slow_reader", "stage_slow_writer")


@pytest.fixture(scope="module")
def timing_libs(gpu):
    spec = importlib.util.spec_from_file_location("fa_build", os.path.join(ROOT, "flash-attention-turing_amd", "build.py"))
    fa_build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fa_build)
    fa_build.build_debug_variants(force=False)          # a no-op when build() has run (the .so files travel with the tree)
    out = {}
    for name in TIMING:
        L = ctypes.CDLL(fa_build.debug_library_path(name))
        L.fa_run_mla_indexer_prefill_logits.argtypes = [ctypes.POINTER(capi.MlaIndexerParams), ctypes.c_void_p]
        L.fa_run_mla_indexer_prefill_logits.restype = ctypes.c_int
        L.fa_last_error.restype = ctypes.c_char_p
        out[name] = L
    return out


@pytest.mark.parametrize("fp8,page", [(True, 16), (False, None)])
def test_slow_reader_and_slow_writer_reproduce_the_product(gpu, timing_libs, fp8, page):
    """one wave held back in every step, in front of its reads of the stage or of its writes to the next one: the product's bits.  Lengths give 0 .. 9 steps
    (one and two are the prologue's special cases; both stages are reused from step 3 on)"""
    gen = _gen("stage", fp8, page)
    sq = 2 * TQ + 3
    q, w, k, sc = C.normal_inputs(B, sq, 64, torch.bfloat16, fp8, gen)
    dk, dsc, table = _device_cache(gpu, k, sc if fp8 else None, page, gen)
    dq, dw, dl = q.to(gpu), w.to(gpu), _lens_t(C.LENS, gpu)
    _, want = _both(gpu, dq, dw, dk, dsc, table, dl, True, C.CAP)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for name in TIMING:
        for rep in range(2):
            got = torch.full((B, sq, C.CAP), C.SENTINEL, dtype=torch.float32, device=gpu)
            p = capi.mla_indexer_params(dq, dw, dk, got, dl, k_scale=dsc, block_table=table, causal=True)
            rc = timing_libs[name].fa_run_mla_indexer_prefill_logits(ctypes.byref(p), stream)
            assert rc == 0, timing_libs[name].fa_last_error().decode()
            torch.cuda.synchronize()
            assert _same_bits(want, got), f"{name} (run {rep}) does not reproduce the product's bits: {int((want != got).sum())} entries differ"


# ---- one speed relation ------------------------------------------------------------------------------------------------------------------------------------

def test_prefill_call_is_no_slower_than_the_decode_call_on_a_chunk(gpu):
    """b 1, sq 256, L = capacity 8192, h 64, bf16, FP8 keys with scales, pages of 64, causal: median of 5 interleaved rounds in one process, the decode call
    timed twice (its own scatter); the bound is 1.0 with no margin - the call exists to be faster on a chunk"""
    gen = _gen("speed")
    sq, L, P = 256, 8192, 64
    q = torch.randn(1, sq, 64, 128, generator=gen).to(torch.bfloat16).to(gpu)
    w = torch.randn(1, sq, 64, generator=gen).to(gpu)
    pool = torch.randn(L // P, P, 128, generator=gen).to(gpu).to(torch.float8_e4m3fn)
    spool = (torch.rand(L // P, P, generator=gen) + 0.5).to(gpu)
    table = torch.randperm(L // P, generator=gen).to(torch.int32).view(1, -1).to(gpu)
    dl = _lens_t([L], gpu)
    kw = dict(k_scale=spool, block_table=table, causal=True)
    new = lambda: F.flash_mla_indexer_prefill_logits(q, w, pool, dl, **kw)
    old = lambda: F.flash_mla_indexer_logits(q, w, pool, dl, **kw)
    mask = C.visible_mask([L], sq, L, True).to(gpu)
    assert torch.equal(new()[mask], old()[mask])

    def timed(fn, reps=5):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / reps

    for fn in (new, old):
        timed(fn, 2)
    t_new, t_old, t_old2 = [], [], []
    for _ in range(5):
        t_new.append(timed(new))
        t_old.append(timed(old))
        t_old2.append(timed(old))
    ratio = float(np.median(t_new) / np.median(t_old))
    print(f"flash_mla_indexer_prefill_logits {np.median(t_new) * 1e3:.1f} us, flash_mla_indexer_logits {np.median(t_old) * 1e3:.1f} us / {np.median(t_old2) * 1e3:.1f} us "
          f"(its two runs: {float(np.median(t_old2) / np.median(t_old)):.3f}), ratio {ratio:.3f}")
    assert ratio <= 1.0, ratio
