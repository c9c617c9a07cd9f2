"""GPU: the register-staged LDS stages of the 64-row KV-cache bodies (fa_fwd_kvcache_prefill.hip, and the one MLA decode body of fa_kvcache_mla_attn.hpp
as fa_fwd_kvcache_mla.hip, fa_fwd_kvcache_mla_sparse.hip and fa_fwd_kvcache_mla_fp8.hip instantiate it) under ADVERSARIAL timing - the method of tests/test_dma_protocol_gpu.py for the kernels whose waves share LDS through
registers instead of LDS-DMA.

Four waves each write a quarter of a 32-key step into one of two stages that all four read, with one barrier per step.  Waves of one unit run close to
lockstep, so a barrier one statement too early almost never hands a wave the stage's previous tenant and every value test passes.  The builds
`stage_slow_reader` / `stage_slow_writer` (flash-attention-turing_amd/build.py; the step all these bodies share and its two hooks: csrc/fa_kvcache_stage.hpp) hold one wave back in every step, in
front of its reads of the stage or in front of its writes to the next one.  A correct schedule does not care, so both must reproduce the product BIT FOR
BIT: out, lse and, with an append, every byte of the cache.  `stage_racy_slow_writer` is the plausible one-line mistake (the step's barrier in front of
store_step) under the slow writer and must NOT reproduce the product: the detector has teeth.  Nothing is asserted about the racy form at normal
timing - it is a race.

Every call goes through the C ABI of the loaded library (each .so is its own process-wide state; caller-owned workspace for splits).  Inputs are N(0, 1)
from fixed CPU-generator seeds, so neighbouring steps hold different rows.  Lengths give 0, 1, 2, 3, 4, 5 and 33 steps of 32 keys in one call: one and two
steps are the prologue's special cases, both stages are reused from step 3 on."""
import ctypes
import importlib.util
import os

import pytest
import torch

import _util as U
from test_kvcache_fp8_gpu import _descale, quantise
from test_kvcache_fp8_gpu import _page as _page8
from test_kvcache_mla_fp8_gpu import page_bytes, random_rows
from test_kvcache_mla_sparse_gpu import random_lists
from test_kvcache_window_gpu import _page

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
DK, DV = 576, 512
TIMING = ("stage_slow_reader", "stage_slow_writer")
RACY = "stage_racy_slow_writer"
# keys visible to a sequence: 0, 1, 2, 3, 4, 5 and 33 steps of 32 (20 and 131: a partial last step; 128: a full one)
LENS = [0, 20, 40, 90, 128, 131, 1040]
CAP = 1120                              # 70 pages of 16: room for the longest sequence and an append of up to 65 rows
SPARSE_LENS, SPARSE_CAP = [0, 1, 31, 33, 100, 777], 1008        # the lengths and capacity of the sparse suite, whose random_lists is used


def _build_module():
    spec = importlib.util.spec_from_file_location("fa_build", os.path.join(ROOT, "flash-attention-turing_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def libs(gpu):
    from flash_attn_turing import capi

    fa_build = _build_module()
    fa_build.build_debug_variants(force=False)          # a no-op when build() has run (the .so files travel with the tree)
    out = {"product": capi.lib()}
    vp = ctypes.c_void_p
    for name in TIMING + (RACY,):
        L = ctypes.CDLL(fa_build.debug_library_path(name))
        L.fa_run_mha_fwd_kvcache_ex.argtypes = [ctypes.POINTER(capi.KvcacheParams), vp, vp]
        for fn in ("fa_run_mla_fwd_kvcache", "fa_run_mla_sparse_fwd_kvcache"):
            getattr(L, fn).argtypes = [vp, vp]
        for fn in ("fa_run_mha_fwd_kvcache_ex", "fa_run_mla_fwd_kvcache", "fa_run_mla_sparse_fwd_kvcache"):
            getattr(L, fn).restype = ctypes.c_int
        L.fa_last_error.restype = ctypes.c_char_p
        out[name] = L
    return out


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    """every tensor of two result tuples, byte for byte (NaN payloads included)"""
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(_bytes(x), _bytes(y)) for x, y in zip(a, b))


def _worst(a, b):
    """the largest |a - b| over out and lse, a NaN on either side counted as a difference"""
    w = 0.0
    for x, y in zip(a[:2], b[:2]):
        d = (x.float() - y.float()).abs()
        w = max(w, torch.nan_to_num(d, nan=float("inf"), posinf=float("inf")).max().item())
    return w


def _workspace(p, nbytes, dev):
    ws = torch.full((max(nbytes, 16) // 4,), NAN, device=dev)
    p.workspace, p.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return ws


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _ok(L, rc):
    assert rc == 0, L.fa_last_error().decode()


def _must_match(libs, run, tag):
    """run(library) -> result tuple; the product once, every timing build twice"""
    want = run(libs["product"])
    for name in TIMING:
        for rep in range(2):
            got = run(libs[name])
            assert _same(want, got), f"{tag}: {name} (run {rep}) does not reproduce the product's bits; largest difference {_worst(want, got):.3e}"
    return want


def _must_differ(libs, run, dtname, tag):
    want = run(libs["product"])
    assert all(torch.isfinite(t.float()).all().item() for t in want[:2]), f"{tag}: the product's result is not finite"
    got = run(libs[RACY])
    w = _worst(want, got)
    print(f"{tag}: racy form under the slow writer, largest difference {w:.3e}")
    assert not _same(want[:2], got[:2]) and w > U.TOL[dtname]["max_abs"], f"{tag}: the slow-writer build did not expose the racy form (largest difference {w:.3e})"


# ---- prefill=True (fa_fwd_kvcache_prefill.hip) ------------------------------------------------------------------------------------------------------

def _prefill_case(gpu, dtname, d, fp8, paged, sq, h, hk, seed, append=True, lens=LENS):
    """-> run(library, causal, num_splits) over one fixed set of inputs.  lens are the keys a sequence sees: with an append the cache holds lens - sq of
    them before the call (a sequence shorter than the chunk starts empty)"""
    from flash_attn_turing import capi

    dt = DT[dtname]
    gen = torch.Generator().manual_seed(seed)
    b = len(lens)
    q = torch.randn(b, sq, h, d, generator=gen).to(dt).to(gpu)
    k, v = (torch.randn(b, CAP, hk, d, generator=gen).to(dt) for _ in range(2))
    k_new, v_new = ((torch.randn(b, sq, hk, d, generator=gen).to(dt).to(gpu) for _ in range(2)) if append else (None, None))
    cs = torch.tensor([max(L - sq, 0) for L in lens] if append else lens, dtype=torch.int32, device=gpu)
    okw = dict(row_tile=64)
    if fp8:
        kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
        k, v = quantise(k, kds), quantise(v, vds)
        okw.update(cache_dtype=capi.FA_CACHE_FP8_E4M3, k_descale=kds, v_descale=vds)
    k, v = k.to(gpu), v.to(gpu)
    table = None
    if paged:
        k, v, table = (_page8(k, v, 16, seed) if fp8 else _page(k, v, 16, seed))[:3]

    def run(L, causal, num_splits):
        kc, vc = k.clone(), v.clone()
        o = torch.full((b, sq, h, d), NAN, dtype=dt, device=gpu)
        lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=gpu)
        p = capi.kvcache_params(q, kc, vc, o, lse, cache_seqlens=cs, k_new=k_new, v_new=v_new, causal=causal, num_splits=num_splits, block_table=table)
        opt = capi.kvcache_options(**okw)
        assert capi.kvcache_row_tile(p, opt) == 64
        ws = _workspace(p, capi.kvcache_workspace_bytes(p, opt), gpu)
        assert capi.kvcache_num_splits(p, opt) == num_splits
        _ok(L, L.fa_run_mha_fwd_kvcache_ex(ctypes.byref(p), ctypes.cast(ctypes.byref(opt), ctypes.c_void_p), _stream(gpu)))
        torch.cuda.synchronize()
        del ws
        return o, lse, kc, vc

    return run


# packed rows of a workgroup = seqlen_q x (h / h_k): 1 (one lane), 17 (two waves idle but staging), 64 (every wave full), 65 (a second workgroup of one row)
PACKED = [(1, 1, 1, 1), (17, 17, 2, 2), (64, 16, 4, 1), (65, 13, 5, 1)]


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "pages16"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
@pytest.mark.parametrize("d", [64, 128])
def test_prefill_reproduces_its_bits_with_a_slow_reader_and_a_slow_writer(gpu, libs, d, fp8, paged, causal):
    for n, (rows, sq, h, hk) in enumerate(PACKED):
        dtname = ("fp16", "bf16")[(n + d // 64) & 1]
        run = _prefill_case(gpu, dtname, d, fp8, paged, sq, h, hk, 51000 + 10 * d + n)
        for ns in (1, 3):
            _must_match(libs, lambda L: run(L, causal, ns), f"prefill {dtname} d{d} fp8={fp8} paged={paged} causal={causal} rows {rows} splits {ns}")
    # without an append a sequence may hold nothing: the loop of zero steps (one split; with three an empty split returns before the loop)
    run = _prefill_case(gpu, "fp16", d, fp8, paged, 16, 4, 1, 51900 + d, append=False)
    for ns in (1, 3):
        _must_match(libs, lambda L: run(L, causal, ns), f"prefill d{d} fp8={fp8} paged={paged} causal={causal} no append, splits {ns}")


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_ragged_prefill_reproduces_its_bits(gpu, libs, causal):
    """one ragged call: chunks of 1 .. 70 rows over the lengths of the dense test (no append), contiguous 16-bit cache"""
    from flash_attn_turing import capi

    dt, d, h, hk = torch.float16, 128, 4, 2
    gen = torch.Generator().manual_seed(52000)
    sqs = [1, 3, 17, 33, 70, 5, 64]
    cu = torch.tensor([sum(sqs[:i]) for i in range(len(sqs) + 1)], dtype=torch.int32, device=gpu)
    total = sum(sqs)
    q = torch.randn(total, h, d, generator=gen).to(dt).to(gpu)
    k, v = (torch.randn(len(LENS), CAP, hk, d, generator=gen).to(dt).to(gpu) for _ in range(2))
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)

    def run(L, ns):
        o = torch.full((total, h, d), NAN, dtype=dt, device=gpu)
        lse = torch.full((h, total), NAN, dtype=torch.float32, device=gpu)
        p = capi.kvcache_params(q, k, v, o, lse, cache_seqlens=cs, causal=causal, num_splits=ns, cu_seqlens_q=cu, max_seqlen_q=max(sqs))
        opt = capi.kvcache_options(row_tile=64, cu_seqlens_q=cu, total_q=total)
        assert capi.kvcache_row_tile(p, opt) == 64
        ws = _workspace(p, capi.kvcache_workspace_bytes(p, opt), gpu)
        _ok(L, L.fa_run_mha_fwd_kvcache_ex(ctypes.byref(p), ctypes.cast(ctypes.byref(opt), ctypes.c_void_p), _stream(gpu)))
        torch.cuda.synchronize()
        del ws
        return o, lse

    for ns in (1, 3):
        _must_match(libs, lambda L: run(L, ns), f"ragged prefill causal={causal} splits {ns}")


# ---- flash_mla_with_kvcache (the dense kernels of fa_fwd_kvcache_mla.hip and fa_fwd_kvcache_mla_fp8.hip) ---------------------------------------------------

def _mla_cache(gpu, dt, fp8, paged, b, cap, gen, seed):
    """the latent cache (16-bit rows of 576 or FP8 rows of 656 bytes), contiguous or a pool of 16-row pages + table"""
    kv = random_rows((b, cap, 1), dt, gen).to(gpu) if fp8 else torch.randn(b, cap, 1, DK, generator=gen).to(dt).to(gpu)
    if not paged:
        return kv, None
    if fp8:
        return page_bytes(kv, 16, seed)
    pool, _, table, _ = _page(kv, kv, 16, seed)
    return pool, table


def _mla_case(gpu, dtname, fp8, paged, sq, h, seed, append=True, lens=LENS):
    from flash_attn_turing import capi

    dt = DT[dtname]
    gen = torch.Generator().manual_seed(seed)
    b = len(lens)
    q = torch.randn(b, sq, h, DK, generator=gen).to(dt).to(gpu)
    kv, table = _mla_cache(gpu, dt, fp8, paged, b, CAP, gen, seed)
    kv_new = torch.randn(b, sq, 1, DK, generator=gen).to(dt).to(gpu) if append else None
    cs = torch.tensor([max(L - sq, 0) for L in lens] if append else lens, dtype=torch.int32, device=gpu)

    def run(L, causal, num_splits):
        kvc = kv.clone()
        o = torch.full((b, sq, h, DV), NAN, dtype=dt, device=gpu)
        lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=gpu)
        p = capi.mla_params(q, kvc, o, lse, cs, kv_new=kv_new, causal=causal, num_splits=num_splits, block_table=table)
        ws = _workspace(p, capi.mla_workspace_bytes(p), gpu)
        assert capi.mla_num_splits(p) == num_splits
        _ok(L, L.fa_run_mla_fwd_kvcache(ctypes.cast(ctypes.byref(p), ctypes.c_void_p), _stream(gpu)))
        torch.cuda.synchronize()
        del ws
        return o, lse, kvc

    return run


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "pages16"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_mla_reproduces_its_bits_with_a_slow_reader_and_a_slow_writer(gpu, libs, fp8, paged):
    """h = 1: one lane; 16: one wave, three idle but staging; 24: a partly filled second wave; 128: two workgroups a token"""
    n = 0
    for h in (1, 16, 24, 128):
        for sq in (1, 2):
            dtname = ("fp16", "bf16")[n & 1]
            run = _mla_case(gpu, dtname, fp8, paged, sq, h, 53000 + n)
            n += 1
            for ns in (1, 3):
                _must_match(libs, lambda L: run(L, True, ns), f"mla {dtname} fp8={fp8} paged={paged} h{h} sq{sq} causal, append, splits {ns}")
    run = _mla_case(gpu, "bf16", fp8, paged, 2, 64, 53900, append=False)       # (a sequence that holds nothing: the loop of zero steps)
    for causal in (False, True):
        _must_match(libs, lambda L: run(L, causal, 1), f"mla fp8={fp8} paged={paged} h64 sq2 causal={causal}, no append")


# ---- flash_mla_sparse_with_kvcache (the sparse kernels of fa_fwd_kvcache_mla_sparse.hip and fa_fwd_kvcache_mla_fp8.hip) --------------------------------------

def _sparse_case(gpu, dtname, fp8, paged, sq, h, topk, seed, lens=SPARSE_LENS, dead_steps=True):
    from flash_attn_turing import capi

    dt = DT[dtname]
    gen = torch.Generator().manual_seed(seed)
    b = len(lens)
    q = torch.randn(b, sq, h, DK, generator=gen).to(dt).to(gpu)
    kv, table = _mla_cache(gpu, dt, fp8, paged, b, SPARSE_CAP, gen, seed)
    idx = random_lists(lens, sq, topk, gen, cap=SPARSE_CAP, dead_steps=dead_steps).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)

    def run(L, num_splits):
        o = torch.full((b, sq, h, DV), NAN, dtype=dt, device=gpu)
        lse = torch.full((b, h, sq), NAN, dtype=torch.float32, device=gpu)
        p = capi.mla_sparse_params(q, kv, o, lse, idx, cs, num_splits=num_splits, block_table=table)
        ws = _workspace(p, capi.mla_sparse_workspace_bytes(p), gpu)
        assert capi.mla_sparse_num_splits(p) == num_splits
        _ok(L, L.fa_run_mla_sparse_fwd_kvcache(ctypes.cast(ctypes.byref(p), ctypes.c_void_p), _stream(gpu)))
        torch.cuda.synchronize()
        del ws
        return o, lse

    return run


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "pages16"])
@pytest.mark.parametrize("fp8", [False, True], ids=["16bit", "fp8"])
def test_sparse_mla_reproduces_its_bits_with_a_slow_reader_and_a_slow_writer(gpu, libs, fp8, paged):
    """lists of the sparse suite: valid positions in random order between invalid entries of every kind (-1, past the length, INT_MIN, INT_MAX); from
    three steps on the first and a middle step are all invalid.  topk 32 / 96 / 256: one, three and eight steps"""
    for n, (topk, h) in enumerate(((32, 24), (96, 128), (256, 24), (256, 128))):
        dtname = ("fp16", "bf16")[n & 1]
        run = _sparse_case(gpu, dtname, fp8, paged, 2, h, topk, 54000 + n)
        for ns in (1, 3):
            if ns > topk // 32:
                continue                # (a split is at least one step: the library would give topk = 32 one split)
            _must_match(libs, lambda L: run(L, ns), f"sparse mla {dtname} fp8={fp8} paged={paged} h{h} topk{topk} splits {ns}")


# ---- teeth ------------------------------------------------------------------------------------------------------------------------------------------

def test_slow_writer_catches_the_barrier_in_front_of_the_store(gpu, libs):
    """the detector must fire on the mistake it exists for, in every file that carries the racy form: with the step's barrier in front of store_step, the
    waves that do not sleep read a stage whose sleeping quarter (8 of a step's 32 keys; in the prefill body a quarter of the step's 64 K / V rows) still
    holds its previous tenant - an O(1) error.  Every case has three or more steps and rows in all four waves (64 packed rows a workgroup)."""
    long = [131, 1040]
    pre = _prefill_case(gpu, "fp16", 128, False, False, 16, 4, 1, 55000, lens=long)
    _must_differ(libs, lambda L: pre(L, False, 1), "fp16", "fa_fwd_kvcache_prefill.hip, 16-bit contiguous")
    pre8 = _prefill_case(gpu, "bf16", 64, True, True, 16, 4, 1, 55001, lens=long)
    _must_differ(libs, lambda L: pre8(L, True, 1), "bf16", "fa_fwd_kvcache_prefill.hip, fp8 pages")
    mla = _mla_case(gpu, "fp16", False, False, 1, 64, 55002, lens=long)
    _must_differ(libs, lambda L: mla(L, True, 1), "fp16", "fa_fwd_kvcache_mla.hip")
    mla8 = _mla_case(gpu, "bf16", True, True, 1, 64, 55003, lens=long)
    _must_differ(libs, lambda L: mla8(L, True, 1), "bf16", "fa_fwd_kvcache_mla_fp8.hip, dense body")
    sp = _sparse_case(gpu, "fp16", False, False, 1, 64, 256, 55004, lens=[100, 777], dead_steps=False)
    _must_differ(libs, lambda L: sp(L, 1), "fp16", "fa_fwd_kvcache_mla_sparse.hip")
    sp8 = _sparse_case(gpu, "bf16", True, True, 1, 64, 256, 55005, lens=[100, 777], dead_steps=False)
    _must_differ(libs, lambda L: sp8(L, 1), "bf16", "fa_fwd_kvcache_mla_fp8.hip, sparse body")
