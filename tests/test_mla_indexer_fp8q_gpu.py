"""GPU: FP8 (e4m3) q_idx through flash_mla_indexer_logits, flash_mla_indexer_prefill_logits and the two *_with_kvcache composites (fa_mla_indexer_params_v2 through the *_v2 entry points).

The product runs on v_mfma_f32_16x16x128_f8f6f4 with e4m3 operands, whose A / B lane map is used only as "row / column = lane & 15": the one-hot tests at the top
are the check of that map with exact integer data - every column, every head, every code.  Below them: integer data against fp64 and against the 16-bit q_idx
calls, ordinary data against the rounding bound, prefill == decode in every entry (NaN included), what is never read, views, composites, graph replay, the
adversarial-timing builds, the C ABI and one speed relation.  Shapes are those of the existing indexer tests (capacity 320, lengths around the 32-key step)."""
import ctypes
import importlib.util
import os
import zlib

import numpy as np
import pytest
import torch

import _mla_indexer_cases as C
import _mla_indexer_fp8q_cases as Q
import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = len(C.LENS)
E4M3 = torch.float8_e4m3fn
CALLS = {"decode": F.flash_mla_indexer_logits, "prefill": F.flash_mla_indexer_prefill_logits}


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


def _lens_t(lens, dev):
    return torch.tensor(lens, dtype=torch.int32, device=dev)


def _device_cache(dev, k, sc, page, gen):
    """(k_idx_cache, k_scale, block_table) on the device: contiguous, or a random paging of the same logical cache (C.paginate: NaN spare pages)"""
    if page is None:
        return k.to(dev), None if sc is None else sc.to(dev), None
    pool, spool, table = C.paginate(k, sc if sc is not None else torch.ones(k.shape[:2]), page, gen)
    return pool.to(dev), None if sc is None else spool.to(dev), table.to(dev)


def _both(dev, dq, dw, dk, dsc, table, dl, causal, cap, row_stride=None):
    """(decode call, prefill call) into sentinel-filled buffers of the caller through the C ABI (the v2 struct)"""
    out = []
    for run in (capi.run_mla_indexer_logits, capi.run_mla_indexer_prefill_logits):
        store = torch.full((dq.shape[0], dq.shape[1], row_stride or cap), C.SENTINEL, dtype=torch.float32, device=dev)
        run(capi.mla_indexer_params_v2(dq, dw, dk, store[:, :, :cap], dl, k_scale=dsc, block_table=table, causal=causal))
        out.append(store)
    torch.cuda.synchronize()
    return out


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _sentinel_outside(x, mask):
    return bool((x.cpu()[~mask] == torch.tensor(C.SENTINEL, dtype=torch.float32)).all())


def _all_forms(gpu, q8, w, k8, gen, sc=None):
    """logits (sq, keys) of one full-length non-causal sequence through both calls, contiguous and pages of 16: {name: fp32 cpu tensor}"""
    keys = k8.shape[1]
    dl = _lens_t([keys], gpu)
    out = {}
    for page in (None, 16):
        dk, dsc, table = _device_cache(gpu, k8, sc, page, gen)
        for name, fn in CALLS.items():
            out[f"{name} page={page}"] = fn(q8.to(gpu), w.to(gpu), dk, dl, k_scale=dsc, block_table=table, causal=False)[0].cpu()
    return out


# ---- 1 - 3. the operand mapping, with exact integer data ----------------------------------------------------------------------------------------------------

def test_every_column_meets_its_column(gpu):
    """token t holds one value at column t of head t % 16, key j one value at column j: the 128 x 128 identity, then an asymmetric diagonal"""
    for tag, (qv, kv) in (("ones", (None, None)), ("asymmetric", (lambda t: 1 + t % 5, lambda j: 2 + j % 3))):
        q8, w, k8, want = Q.one_hot_columns(qv, kv)
        for name, got in _all_forms(gpu, q8, w, k8, _gen("columns", tag)).items():
            assert _same_bits(got, want), (tag, name, int((got != want).sum()), got.diagonal()[:8].tolist())
        # the same keys under the queries of another token order: want's rows move with the tokens
        perm = torch.randperm(128, generator=_gen("columns perm", tag))
        for name, got in _all_forms(gpu, q8.view(torch.uint8)[:, perm].view(E4M3), w, k8, _gen("columns", tag, 2)).items():
            assert _same_bits(got, want[perm]), (tag, name)


@pytest.mark.parametrize("h", [16, 32, 64])
def test_every_head_meets_its_weight(gpu, h):
    """token t has head t alone non-zero, weights[t, hd] = hd + 1: logits[t, j] == t + 1"""
    q8, w, k8, want = Q.one_hot_heads(h)
    for name, got in _all_forms(gpu, q8, w, k8, _gen("heads", h)).items():
        assert _same_bits(got, want), (h, name, got[:, 0].tolist())


def test_every_code(gpu):
    """token t carries code t, key j code j at every column: max(float(code_t) * float(code_j), 0) bit for bit over the 254 x 254 finite pairs, subnormal codes
    included (OCP e4m3: 0x7e is 448, 0x7f NaN; under fnuz 0x80 would be NaN and every exponent one lower)"""
    q8, w, k8, want, fin = Q.every_code()
    for name, got in _all_forms(gpu, q8, w, k8, _gen("codes")).items():
        bad = (_bits(got) != _bits(want)) & fin
        assert not bool(bad.any()), (name, int(bad.sum()), bad.nonzero()[:4].tolist())
    assert float(want[0x7E, 0x7E]) == 448.0 * 448.0 and float(want[0x01, 0x01]) == 2.0 ** -18 and float(want[0x80, 0x38]) == 0.0


# ---- 4. exact data ---------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16, 64])
@pytest.mark.parametrize("h", [16, 32, 64])
def test_exact_data_equals_fp64_and_the_16bit_query_calls(gpu, h, page):
    """integer data: the FP8-q decode call is the fp64 model bit for bit and equals the existing call on q.to(bf16) and q.to(fp16); entries at j >= n_t keep
    the sentinel"""
    sq = 9
    gen = _gen("exact", h, page)
    q8, w, k8, sc = Q.exact_inputs(B, sq, h, gen)
    ref, _ = C.logits_model(q8.float(), w, k8, sc)
    dk, dsc, table = _device_cache(gpu, k8, sc, page, gen)
    dq, dw, dl = q8.to(gpu), w.to(gpu), _lens_t(C.LENS, gpu)
    for causal in (True, False):
        mask = C.visible_mask(C.LENS, sq, C.CAP, causal)
        dec, pre = _both(gpu, dq, dw, dk, dsc, table, dl, causal, C.CAP)
        assert _same_bits(dec, pre)
        assert _sentinel_outside(dec, mask) and torch.equal(dec.cpu().double()[mask], ref[mask]), causal
        for dt in (torch.bfloat16, torch.float16):
            for name, fn in CALLS.items():
                old = fn(dq.to(dt), dw, dk, dl, k_scale=dsc, block_table=table, causal=causal).cpu()
                assert _same_bits(old[mask], dec.cpu()[mask]), (causal, dt, name)
        pub = F.flash_mla_indexer_logits(dq.view(torch.uint8), dw, dk.view(torch.uint8), dl, k_scale=dsc, block_table=table, causal=causal).cpu()
        assert _same_bits(pub[mask], dec.cpu()[mask])                    # uint8 codes are the same call


# ---- 5. ordinary data --------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16])
@pytest.mark.parametrize("h", [16, 64])
def test_ordinary_data_within_the_rounding_bound(gpu, h, page):
    """N(0, 1) data, the queries quantised by quantize_mla_index_queries: both calls within TOL x magnitude of the fp64 model on the quantised inputs"""
    sq = 19
    gen = _gen("normal", h, page)
    q, w, k8, sc = C.normal_inputs(B, sq, h, torch.bfloat16, True, gen)
    codes, w2 = F.quantize_mla_index_queries(q, w)
    q8m, w2m, _, _ = Q.normal_quantised(B, sq, h, _gen("normal", h, page))
    assert torch.equal(codes, q8m.view(torch.uint8)) and torch.equal(w2, w2m)       # the model module restates the rule
    ref, mag = C.logits_model(codes.view(E4M3).float(), w2, k8, sc)
    dk, dsc, table = _device_cache(gpu, k8, sc, page, gen)
    dl = _lens_t(C.LENS, gpu)
    for causal in (True, False):
        mask = C.visible_mask(C.LENS, sq, C.CAP, causal)
        for name, fn in CALLS.items():
            got = fn(codes.to(gpu), w2.to(gpu), dk, dl, k_scale=dsc, block_table=table, causal=causal).cpu().double()
            worst = float(((got - ref).abs() / mag)[mask].max())
            print(f"fp8q {name} logits h={h} page={page} causal={causal}: worst |err| / magnitude = {worst:.3e} (bound {C.TOL:.3e}, ratio {worst / C.TOL:.4f})")
            assert worst <= C.TOL, (name, worst)


# ---- 6. prefill == decode -------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16, 64])
@pytest.mark.parametrize("h", [16, 32, 64])
def test_prefill_equals_decode_in_every_entry(gpu, h, page):
    """sq 19 (two full tiles, a ragged one, an inactive wave), b 7, causal or not: the whole buffers, sentinels included; then one NaN key code below L: its column
    is the same in both calls, NaN for the tokens that see it, and every other column keeps the clean run's bits"""
    sq, j = 19, 90
    gen = _gen("equal", h, page)
    q8, w, k8, sc = Q.normal_quantised(B, sq, h, gen)
    dq, dw, dl = q8.to(gpu), w.to(gpu), _lens_t(C.LENS, gpu)
    kp = k8.clone()
    kp.view(torch.uint8)[:, j] = 0x7F
    for causal in (True, False):
        mask = C.visible_mask(C.LENS, sq, C.CAP, causal)
        dk, dsc, table = _device_cache(gpu, k8, sc, page, _gen("equal pages", h, page))
        dec, pre = _both(gpu, dq, dw, dk, dsc, table, dl, causal, C.CAP)
        assert _same_bits(dec, pre), (causal, int((_bits(dec) != _bits(pre)).sum()))
        assert _sentinel_outside(pre, mask) and torch.isfinite(pre.cpu()[mask]).all(), causal
        dk, dsc, table = _device_cache(gpu, kp, sc, page, _gen("equal pages", h, page))
        ndec, npre = _both(gpu, dq, dw, dk, dsc, table, dl, causal, C.CAP)
        assert _same_bits(ndec, npre), causal                           # NaN compared as NaN: the bits
        sees = mask[:, :, j]
        assert sees.any() and not sees.all() and torch.isnan(npre.cpu()[:, :, j][sees]).all()
        other = torch.ones(C.CAP, dtype=torch.bool)
        other[j] = False
        assert _same_bits(npre[:, :, other], pre[:, :, other]) and _same_bits(npre.cpu()[:, :, j][~sees], pre.cpu()[:, :, j][~sees])


@pytest.mark.parametrize("page", [None, 64])
def test_several_key_ranges_and_the_early_return(gpu, page):
    """b 1, capacity 4160, sq 9: a launch of two tiles is spread over at least two key ranges; with L = 33 or 0 every range but the first (or every range) returns
    before its first barrier and writes nothing"""
    cap, sq = 4160, 9
    gen = _gen("chunks", page)
    q8, w, k8, sc = Q.normal_quantised(1, sq, 64, gen, cap=cap)
    dk, dsc, table = _device_cache(gpu, k8, sc, page, gen)
    dq, dw = q8.to(gpu), w.to(gpu)
    probe = torch.empty(1, sq, cap, device=gpu)
    tq, wg, nc = capi.mla_indexer_prefill_launch(capi.mla_indexer_params_v2(dq, dw, dk, probe, _lens_t([cap], gpu), k_scale=dsc, block_table=table))
    assert nc >= 2 and wg % 32 == 0 and nc * wg >= cap, (tq, wg, nc)
    ref, mag = C.logits_model(q8.float(), w, k8, sc)
    for L in (cap, 33, 0):
        dec, pre = _both(gpu, dq, dw, dk, dsc, table, _lens_t([L], gpu), True, cap)
        mask = C.visible_mask([L], sq, cap, True)
        assert _same_bits(dec, pre) and _sentinel_outside(pre, mask), L
        if L:
            assert float(((pre.cpu().double() - ref).abs() / mag)[mask].max()) <= C.TOL, L


# ---- 7. what is never read ----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("page", [None, 16, 64])
def test_what_is_never_read_may_hold_nan(gpu, page):
    """0x7f codes and NaN scales in rows at or past L_i, in unreferenced pages (C.paginate's spare pages), in pages wholly past L_i (their table entries -1 and
    INT_MAX), and - causal prefill, the last tile ragged - in keys past a tile's last n_t: the bits of the clean cache"""
    gen = _gen("never_read", page)
    sq, h, lens = 19, 64, (100, 33)
    q8, w, k8, sc = Q.normal_quantised(2, sq, h, gen)
    dq, dw, dl = q8.to(gpu), w.to(gpu), _lens_t(lens, gpu)
    mask = C.visible_mask(lens, sq, C.CAP, True)
    dk, dsc, table = _device_cache(gpu, k8, sc, page, _gen("never_read pages", page))
    base_dec, base = _both(gpu, dq, dw, dk, dsc, table, dl, True, C.CAP)
    kp, scp = k8.clone(), sc.clone()
    for i, L in enumerate(lens):
        kp.view(torch.uint8)[i, L:] = 0x7F
        scp[i, L:] = float("nan")
    dk, dsc, table = _device_cache(gpu, kp, scp, page, _gen("never_read pages", page))
    if page is not None:
        garbage = torch.tensor([-1, 2 ** 31 - 1], dtype=torch.int32, device=gpu)
        for i, L in enumerate(lens):
            first = (L + page - 1) // page                  # the first column no visible key needs
            table[i, first:] = garbage.repeat(table.shape[1])[:table.shape[1] - first]
    dec, got = _both(gpu, dq, dw, dk, dsc, table, dl, True, C.CAP)
    assert _same_bits(base, got) and _same_bits(dec, got) and _same_bits(base_dec, dec)
    assert torch.isfinite(got.cpu()[mask]).all() and _sentinel_outside(got, mask)
    # a shorter query chunk over the same poisoned cache: the keys between its tiles' last n_t and L_i are below L_i and clean, those past L_i are not read
    dec2, got2 = _both(gpu, dq[:, :9], dw[:, :9], dk, dsc, table, dl, True, C.CAP)
    m2 = C.visible_mask(lens, 9, C.CAP, True)
    assert _same_bits(dec2, got2) and torch.isfinite(got2.cpu()[m2]).all() and _sentinel_outside(got2, m2)


# ---- 8. views ---------------------------------------------------------------------------------------------------------------------------------------------------------

def test_views_in_place_and_copied(gpu):
    """q_idx as a slice of a (b, sq, h, 160) buffer (16-byte aligned: used in place) and at an odd storage offset (copied once): the same bits; the padded-row
    cache view and k_scale as a view of one buffer laid out block by block (128 code bytes, then the fp32 scale, per token)"""
    gen = _gen("views")
    sq, h = 19, 32
    q8, w, k8, sc = Q.normal_quantised(B, sq, h, gen)
    dl = _lens_t(C.LENS, gpu)
    dw = w.to(gpu)
    plain_dec, plain = _both(gpu, q8.to(gpu), dw, k8.to(gpu), sc.to(gpu), None, dl, True, C.CAP)
    mask = C.visible_mask(C.LENS, sq, C.CAP, True)
    qw = torch.full((B, sq, h, 160), 0x7F, dtype=torch.uint8)
    qw[:, :, :, 16:144] = q8.view(torch.uint8)
    dqv = qw.to(gpu)[:, :, :, 16:144].view(E4M3)
    assert dqv.stride(2) == 160 and not dqv.is_contiguous() and dqv.data_ptr() % 16 == 0
    flat = torch.full((q8.numel() + 3,), 0x7F, dtype=torch.uint8)
    flat[3:] = q8.view(torch.uint8).reshape(-1)
    dqo = flat.to(gpu)[3:].view(B, sq, h, 128)
    assert dqo.is_contiguous() and dqo.data_ptr() % 16 == 3
    # one buffer, block by block: per token 128 code bytes and 4 scale bytes in a 144-byte block
    blocks = torch.full((B, C.CAP, 144), 0x7F, dtype=torch.uint8)
    blocks[:, :, :128] = k8.view(torch.uint8)
    blocks[:, :, 128:132] = sc.contiguous().view(torch.uint8).view(B, C.CAP, 4)
    dblocks = blocks.to(gpu)
    dkv = dblocks[:, :, :128]
    dscv = dblocks.view(B, C.CAP * 144)[:, 128:].view(torch.float32).view(B, -1)[:, ::36]
    assert dkv.stride(1) == 144 and dscv.shape == (B, C.CAP) and dscv.stride(1) == 36 and torch.equal(dscv.cpu(), sc)
    for dq in (dqv, dqo):
        for name, fn in CALLS.items():
            got = fn(dq, dw, dkv, dl, k_scale=dscv, causal=True).cpu()
            want = (plain_dec if name == "decode" else plain).cpu()
            assert _same_bits(got[mask], want[mask]), name
    # the in-place view through the C ABI (its strides in bytes), a logits row stride above the capacity
    dec, pre = _both(gpu, dqv, dw, dkv, dscv, None, dl, True, C.CAP, row_stride=C.CAP + 37)
    assert _same_bits(dec, pre) and _same_bits(pre[:, :, :C.CAP], plain) and bool((pre[:, :, C.CAP:] == torch.tensor(C.SENTINEL, dtype=torch.float32)).all())


# ---- 9. composites -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_composites_equal_their_two_launches(gpu):
    gen = _gen("composite")
    sq, topk = 19, 32
    q8, w, k8, sc = Q.normal_quantised(B, sq, 64, gen)
    pool, spool, table = C.paginate(k8, sc, 16, gen)
    args = (q8.to(gpu), w.to(gpu), pool.to(gpu), _lens_t(C.LENS, gpu))
    kw = dict(k_scale=spool.to(gpu), block_table=table.to(gpu))
    for causal in (True, False):
        mask = C.visible_mask(C.LENS, sq, C.CAP, causal)
        for logits_fn, index_fn in ((F.flash_mla_indexer_logits, F.flash_mla_index_with_kvcache), (F.flash_mla_indexer_prefill_logits, F.flash_mla_index_prefill_with_kvcache)):
            lg = logits_fn(*args, causal=causal, **kw)
            idx = F.flash_mla_indexer_topk(lg, args[3], topk, causal=causal)
            got, got_lg = index_fn(*args, topk, causal=causal, return_logits=True, **kw)
            only = index_fn(*args, topk, causal=causal, **kw)
            assert got.dtype == torch.int32 and got.shape == (B, sq, topk) and torch.equal(got, idx) and torch.equal(only, idx)
            assert _same_bits(got_lg.cpu()[mask], lg.cpu()[mask])
            assert torch.equal(got.cpu(), C.topk_model(lg.cpu(), C.LENS, topk, causal))


def test_lists_feed_the_sparse_call_and_give_the_dense_causal_bits(gpu):
    """L_i <= topk, causal: the lists of both composites are 0 .. n_t - 1 padded with -1, and the sparse MLA call on them equals flash_mla_with_kvcache(causal=True)"""
    gen = _gen("e2e")
    b, sq, h, cap, topk = 2, 2, 16, 128, 32
    lens = [32, 17]
    dl = _lens_t(lens, gpu)
    q8, w, k8, sc = Q.normal_quantised(b, sq, 64, gen, cap=cap)
    want = torch.full((b, sq, topk), -1, dtype=torch.int32)
    for i, L in enumerate(lens):
        for t in range(sq):
            n = C.visible(L, sq, t, True, cap)
            want[i, t, :n] = torch.arange(n, dtype=torch.int32)
    q = (torch.randn(b, sq, h, 576, generator=gen) * 0.5).to(torch.bfloat16).to(gpu)
    kv = (torch.randn(b, cap, 1, 576, generator=gen) * 0.5).to(torch.bfloat16).to(gpu)
    do, dlse = F.flash_mla_with_kvcache(q, kv, dl, causal=True, num_splits=1, return_softmax_lse=True)
    for index_fn in (F.flash_mla_index_with_kvcache, F.flash_mla_index_prefill_with_kvcache):
        idx, lg = index_fn(q8.to(gpu), w.to(gpu), k8.to(gpu), dl, topk, k_scale=sc.to(gpu), causal=True, return_logits=True)
        assert torch.equal(idx.cpu(), want) and lg.shape == (b, sq, cap)
        so, sl = F.flash_mla_sparse_with_kvcache(q, kv, dl, idx, num_splits=1, return_softmax_lse=True)
        assert torch.equal(so, do) and torch.equal(sl, dlse)


# ---- 10. graph replay ----------------------------------------------------------------------------------------------------------------------------------------------------

def test_graph_replay_reads_lengths_table_and_scales_then_in_memory(gpu):
    gen = _gen("graph")
    sq, topk = 19, 32
    q8, w, k8, sc = Q.normal_quantised(2, sq, 64, gen)
    pool, spool, table = C.paginate(k8, sc, 64, gen)
    dq, dw, dk, dsc, dt = q8.to(gpu), w.to(gpu), pool.to(gpu), spool.to(gpu), table.to(gpu)
    dl = _lens_t([100, 257], gpu)

    def calls():
        return (F.flash_mla_indexer_logits(dq, dw, dk, dl, k_scale=dsc, block_table=dt, causal=True),
                F.flash_mla_indexer_prefill_logits(dq, dw, dk, dl, k_scale=dsc, block_table=dt, causal=True),
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
        g = calls()
    dl.copy_(_lens_t([301, 33], gpu))
    dt.copy_(dt.flip(1).contiguous())           # the same pages in another order: another logical cache
    dsc.mul_(2.0)                               # (the spare pages' NaN scales stay NaN)
    graph.replay()
    torch.cuda.synchronize()
    e = calls()
    mask = C.visible_mask([301, 33], sq, C.CAP, True)
    assert _same_bits(g[0].cpu()[mask], e[0].cpu()[mask]) and _same_bits(g[1].cpu()[mask], e[1].cpu()[mask]) and _same_bits(g[0].cpu()[mask], g[1].cpu()[mask])
    assert torch.equal(g[2], e[2])


# ---- 11. the stage protocol under adversarial timing ------------------------------------------------------------------------------------------------------------------------

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
        L.fa_run_mla_indexer_prefill_logits_v2.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        L.fa_run_mla_indexer_prefill_logits_v2.restype = ctypes.c_int
        L.fa_last_error.restype = ctypes.c_char_p
        out[name] = L
    return out


@pytest.mark.parametrize("page", [None, 16])
def test_slow_reader_and_slow_writer_reproduce_the_product(gpu, timing_libs, page):
    """one wave held back in every step, in front of its reads of the stage or of its writes to the next one: the product's bits.  Lengths give 0 .. 9 steps"""
    gen = _gen("stage", page)
    sq = 19
    q8, w, k8, sc = Q.normal_quantised(B, sq, 64, gen)
    dk, dsc, table = _device_cache(gpu, k8, sc, page, gen)
    dq, dw, dl = q8.to(gpu), w.to(gpu), _lens_t(C.LENS, gpu)
    _, want = _both(gpu, dq, dw, dk, dsc, table, dl, True, C.CAP)
    stream = torch.cuda.current_stream(gpu).cuda_stream
    for name in TIMING:
        for rep in range(2):
            got = torch.full((B, sq, C.CAP), C.SENTINEL, dtype=torch.float32, device=gpu)
            p = capi.mla_indexer_params_v2(dq, dw, dk, got, dl, k_scale=dsc, block_table=table, causal=True)
            rc = timing_libs[name].fa_run_mla_indexer_prefill_logits_v2(ctypes.byref(p), stream)
            assert rc == 0, timing_libs[name].fa_last_error().decode()
            torch.cuda.synchronize()
            assert _same_bits(want, got), f"{name} (run {rep}) does not reproduce the product's bits: {int((want != got).sum())} entries differ"


# ---- 12. the C ABI --------------------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("entry", ["decode", "prefill"])
def test_c_abi_v2_struct_gives_the_python_calls_bits(gpu, entry):
    gen = _gen("capi", entry)
    sq = 9
    q8, w, k8, sc = Q.normal_quantised(B, sq, 32, gen)
    pool, spool, table = C.paginate(k8, sc, 16, gen)
    dq, dw, dk, dsc, dt, dl = q8.to(gpu), w.to(gpu), pool.to(gpu), spool.to(gpu), table.to(gpu), _lens_t(C.LENS, gpu)
    want = CALLS[entry](dq, dw, dk, dl, k_scale=dsc, block_table=dt, causal=True)
    got = torch.full((B, sq, C.CAP), C.SENTINEL, dtype=torch.float32, device=gpu)
    p = capi.mla_indexer_params_v2(dq, dw, dk, got, dl, k_scale=dsc, block_table=dt, causal=True)
    assert p.struct_size == 224 and p.q_format == capi.FA_IDX_Q_FP8_E4M3
    (capi.run_mla_indexer_logits if entry == "decode" else capi.run_mla_indexer_prefill_logits)(p)
    torch.cuda.synchronize()
    mask = C.visible_mask(C.LENS, sq, C.CAP, True)
    assert _same_bits(got.cpu()[mask], want.cpu()[mask]) and _sentinel_outside(got, mask)
    # a v2 struct with q_format = FA_IDX_Q_16BIT is the 216-byte struct's call
    q16 = q8.to(torch.bfloat16).to(gpu)
    a, b = (torch.full((B, sq, C.CAP), C.SENTINEL, dtype=torch.float32, device=gpu) for _ in range(2))
    run = capi.run_mla_indexer_logits if entry == "decode" else capi.run_mla_indexer_prefill_logits
    run(capi.mla_indexer_params_v2(q16, dw, dk, a, dl, k_scale=dsc, block_table=dt, causal=True))
    run(capi.mla_indexer_params(q16, dw, dk, b, dl, k_scale=dsc, block_table=dt, causal=True))
    torch.cuda.synchronize()
    assert _same_bits(a, b)


# ---- 13. one speed relation ---------------------------------------------------------------------------------------------------------------------------------------------------

def test_fp8q_prefill_call_is_no_slower_than_the_bf16_query_call(gpu):
    """b 1, sq 256, L = capacity 8192, h 64, FP8 keys with scales, pages of 64, causal - the point the existing prefill test pins: the FP8-q prefill call against
    flash_mla_indexer_prefill_logits on q.to(bf16) over the same cache, medians of 5 interleaved rounds in one process, the bf16-q call timed twice (its own
    scatter).  The bf16-q kernels' device code is unchanged by FP8 q_idx, so this compares with the call as it was.  The bound is 1.0 with no margin: the new
    call issues a quarter of the MFMAs, half of the fragment reads and no conversions"""
    gen = _gen("speed")
    sq, L, P = 256, 8192, 64
    q8 = torch.randn(1, sq, 64, 128, generator=gen).to(E4M3).to(gpu)
    q16 = q8.to(torch.bfloat16)
    w = torch.randn(1, sq, 64, generator=gen).to(gpu)
    pool = torch.randn(L // P, P, 128, generator=gen).to(gpu).to(E4M3)
    spool = (torch.rand(L // P, P, generator=gen) + 0.5).to(gpu)
    table = torch.randperm(L // P, generator=gen).to(torch.int32).view(1, -1).to(gpu)
    dl = _lens_t([L], gpu)
    kw = dict(k_scale=spool, block_table=table, causal=True)
    new = lambda: F.flash_mla_indexer_prefill_logits(q8, w, pool, dl, **kw)
    old = lambda: F.flash_mla_indexer_prefill_logits(q16, w, pool, dl, **kw)
    mask = C.visible_mask([L], sq, L, True).to(gpu)
    a, b = new()[mask].double(), old()[mask].double()
    assert float((a - b).abs().max()) <= 1e-3 * float(b.abs().max())      # (the same values in another summation order: a sanity check, not the contract)

    def timed(fn, reps=5):
        s, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        z.record()
        torch.cuda.synchronize()
        return s.elapsed_time(z) / reps

    for fn in (new, old):
        timed(fn, 2)
    t_new, t_old, t_old2 = [], [], []
    for _ in range(5):
        t_new.append(timed(new))
        t_old.append(timed(old))
        t_old2.append(timed(old))
    ratio = float(np.median(t_new) / np.median(t_old))
    print(f"fp8q flash_mla_indexer_prefill_logits {np.median(t_new) * 1e3:.1f} us, bf16-q {np.median(t_old) * 1e3:.1f} us / {np.median(t_old2) * 1e3:.1f} us "
          f"(its two runs: {float(np.median(t_old2) / np.median(t_old)):.3f}), ratio {ratio:.3f}")
    assert ratio <= 1.0, ratio
