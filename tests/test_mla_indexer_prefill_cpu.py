"""CPU: the prompt-chunk index logits (flash_mla_indexer_prefill_logits, flash_mla_index_prefill_with_kvcache; fa_run_mla_indexer_prefill_logits,
fa_mla_indexer_prefill_launch) without a GPU: signatures, the refusals of the decode calls with the same words, the C symbols, the struct size the entry
accepts, the launch shape the host reports, and the compiled kernels' resources."""
import ctypes
import re

import pytest
import torch

import flash_attn_turing as F
from flash_attn_turing import capi
from test_mla_indexer_cpu import _args, _code, _idx_params, _sig


def test_signatures_are_those_of_the_decode_calls():
    assert _sig(F.flash_mla_indexer_prefill_logits) == _sig(F.flash_mla_indexer_logits) == (
        ["q_idx", "weights", "k_idx_cache", "cache_seqlens"], {"k_scale": None, "block_table": None, "causal": True})
    assert _sig(F.flash_mla_index_prefill_with_kvcache) == _sig(F.flash_mla_index_with_kvcache) == (
        ["q_idx", "weights", "k_idx_cache", "cache_seqlens", "topk"], {"k_scale": None, "block_table": None, "causal": True, "return_logits": False})
    for n in ("flash_mla_indexer_prefill_logits", "flash_mla_index_prefill_with_kvcache"):
        assert n in F.__all__ and getattr(F, n) is getattr(F.interface, n)


def _refused_both(word, **change):
    """the row of test_mla_indexer_cpu._refused, against the decode calls and the prefill calls: the same exception with the same words"""
    said = []
    for logits, index in ((F.flash_mla_indexer_logits, F.flash_mla_index_with_kvcache), (F.flash_mla_indexer_prefill_logits, F.flash_mla_index_prefill_with_kvcache)):
        a = _args()
        ch = dict(change)
        kw = {k: ch.pop(k) for k in list(ch) if k in ("k_scale", "block_table", "causal")}
        a.update(ch)
        with pytest.raises(ValueError, match=word) as e1:
            logits(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], **kw)
        with pytest.raises(ValueError, match=word) as e2:
            index(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], 32, **kw)
        said.append((str(e1.value), str(e2.value)))
    assert said[0] == said[1], said


def test_python_refusals_are_those_of_the_decode_calls():
    z = torch.zeros
    _refused_both("q_idx", q_idx=z(2, 2, 64, 128))
    _refused_both("q_idx", q_idx=z(2, 2, 64, 64, dtype=torch.bfloat16))
    _refused_both("q_idx", q_idx=z(2, 2, 48, 128, dtype=torch.bfloat16))
    _refused_both("q_idx", q_idx=z(2, 64, 128, dtype=torch.bfloat16))
    _refused_both("q_idx", q_idx=z(2, 0, 64, 128, dtype=torch.bfloat16), weights=z(2, 0, 64))
    _refused_both("weights", weights=z(2, 2, 64, dtype=torch.bfloat16))
    _refused_both("weights", weights=z(2, 2, 32))
    _refused_both("k_idx_cache", k_idx_cache=z(2, 64, 128, dtype=torch.float16))
    _refused_both("k_idx_cache", k_idx_cache=z(2, 64, 64, dtype=torch.bfloat16))
    _refused_both("k_idx_cache", k_idx_cache=z(3, 64, 128, dtype=torch.bfloat16))
    _refused_both("k_idx_cache", k_idx_cache=z(2, 64, 1, 128, dtype=torch.bfloat16))
    _refused_both("k_idx_cache", k_idx_cache=z(2, 64, 136, dtype=torch.uint8)[:, :, :128])
    _refused_both("k_idx_cache", k_idx_cache=z(2, 64 * 128 + 8, dtype=torch.uint8)[:, :64 * 128].unflatten(1, (64, 128)))
    _refused_both("k_idx_cache", k_idx_cache=z(2 * 64 * 128 + 8, dtype=torch.uint8)[8:].view(2, 64, 128))
    _refused_both("k_idx_cache", k_idx_cache=z(2, 64, 256, dtype=torch.uint8)[:, :, ::2])
    _refused_both("k_idx_cache", k_idx_cache=z(2, 64, 132, dtype=torch.bfloat16)[:, :, :128])
    _refused_both("k_idx_cache", k_idx_cache=z(2 * 64 * 128 + 4, dtype=torch.bfloat16)[4:].view(2, 64, 128))
    _refused_both("k_scale", k_scale=z(2, 64, dtype=torch.float64))
    _refused_both("k_scale", k_scale=z(2, 63))
    _refused_both("block_table", block_table=z(2, 4, dtype=torch.int64))
    _refused_both("block_table", block_table=z(3, 4, dtype=torch.int32))
    _refused_both("page_block_size", block_table=z(2, 4, dtype=torch.int32), k_idx_cache=z(5, 24, 128, dtype=torch.uint8))
    _refused_both("cache_seqlens", cache_seqlens=z(2, dtype=torch.int64))
    _refused_both("cache_seqlens", cache_seqlens=z(3, dtype=torch.int32))
    _refused_both("cache_seqlens", cache_seqlens=1.5)
    _refused_both("causal", causal=1)
    a = _args()
    for topk in (0, 31, 48, -32, 32.0, True):
        with pytest.raises(ValueError, match="topk"):
            F.flash_mla_index_prefill_with_kvcache(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], topk)
    # views that ARE addressable pass the checks and stop at the host module, which wants a GPU
    ok = torch.zeros(2, 64, 160, dtype=torch.uint8)[:, :, :128]
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_mla_indexer_prefill_logits(a["q_idx"], a["weights"], ok, a["cache_seqlens"], k_scale=torch.zeros(2, 128)[:, ::2])
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_mla_index_prefill_with_kvcache(torch.zeros(2, 11, 64, 128, dtype=torch.bfloat16), torch.zeros(2, 11, 64), ok, 7, 32)


def test_c_symbols_are_declared_and_exported():
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define FA_HAS_MLA_INDEXER_PREFILL 1\b", text) and re.search(r"#define FA_ABI_VERSION 4\b", text)
    assert capi.lib().fa_abi_version() == 4 and ctypes.sizeof(capi.MlaIndexerParams) == 216
    names = capi.declared_functions()
    for n in ("fa_run_mla_indexer_prefill_logits", "fa_mla_indexer_prefill_launch"):
        assert n in names and hasattr(capi.lib(), n)
    assert re.search(r"int fa_run_mla_indexer_prefill_logits\(const fa_mla_indexer_params\* params, void\* stream\);", text)
    assert re.search(r"int fa_mla_indexer_prefill_launch\(const fa_mla_indexer_params\* params, int32_t\* tokens_per_wg, int32_t\* wg_keys, int32_t\* n_chunks\);", text)


def test_c_entries_share_the_validation_of_the_decode_entry():
    L = capi.lib()
    run, dec = L.fa_run_mla_indexer_prefill_logits, L.fa_run_mla_indexer_logits
    out = [ctypes.c_int32(-7) for _ in range(3)]
    shape = lambda p, stream: L.fa_mla_indexer_prefill_launch(p, *[ctypes.byref(x) for x in out])

    def bad(code, word, paged=False, **change):
        words = []
        for fn in (dec, run, shape):
            p, keep = _idx_params(paged)
            for k, v in change.items():
                setattr(p, k, v)
            _code(p, fn, code, word)
            words.append(capi.last_error())
        assert words[0] == words[1] == words[2], words
        assert [x.value for x in out] == [-7, -7, -7]       # a refused query writes nothing

    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=208)
    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=224)
    bad(capi.FA_ERR_BAD_ABI, "magic", magic=0)
    bad(capi.FA_ERR_BAD_SHAPE, "seqlen_q", seqlen_q=0)
    bad(capi.FA_ERR_BAD_HEADDIM, "h 48", h=48)
    bad(capi.FA_ERR_BAD_HEADDIM, "d 64", d=64)
    bad(capi.FA_ERR_BAD_DTYPE, "k_format", k_format=2)
    bad(capi.FA_ERR_BAD_SHAPE, "reserved_", reserved_=1)
    bad(capi.FA_ERR_NULL_POINTER, "q_idx", q_idx=None)
    bad(capi.FA_ERR_NULL_POINTER, "logits", logits=None)
    bad(capi.FA_ERR_BAD_STRIDE, "k_cache_row_stride", k_cache_row_stride=136)
    bad(capi.FA_ERR_BAD_STRIDE, "logits_row_stride", logits_row_stride=63)
    bad(capi.FA_ERR_BAD_SHAPE, "page_block_size", paged=True, page_block_size=24)
    bad(capi.FA_ERR_BAD_STRIDE, "block_table_stride", paged=True, block_table_stride=3)
    # b == 0: FA_OK without a launch, whatever the pointers
    p, keep = _idx_params()
    p.b, p.q_idx, p.weights, p.k_idx_cache, p.logits = 0, None, None, None, None
    assert run(ctypes.byref(p), None) == capi.FA_OK
    assert run(None, None) == capi.FA_ERR_NULL_POINTER


def _launch(b, sq, cap, paged=False):
    q, w = torch.zeros(b, sq, 64, 128, dtype=torch.bfloat16), torch.zeros(b, sq, 64)
    lg, cs = torch.zeros(b, sq, cap), torch.zeros(b, dtype=torch.int32)
    if paged:
        k, bt = torch.zeros(3, 64, 128, dtype=torch.uint8), torch.zeros(b, cap // 64, dtype=torch.int32)
    else:
        k, bt = torch.zeros(b, cap, 128, dtype=torch.uint8), None
    keep = (q, w, k, lg, cs, bt)
    return capi.mla_indexer_prefill_launch(capi.mla_indexer_params(q, w, k, lg, cs, block_table=bt)), keep


def test_the_launch_the_host_reports():
    seen = set()
    for b, sq, cap, paged in ((1, 1, 64, False), (7, 19, 320, False), (2, 5, 4160, True), (1, 256, 8192, True), (1, 2048, 32768, False), (8, 128, 131072, False),
                              (3, 1, 32, False), (1, 9, 4160, False)):
        (tq, wg, nc), _ = _launch(b, sq, cap, paged)
        assert tq in (4, 8) and wg % 32 == 0 and 256 <= wg <= 4096 and nc >= 1 and nc * wg >= cap and (nc - 1) * wg < cap, (b, sq, cap, tq, wg, nc)
        seen.add(tq)
    assert len(seen) == 1                       # the tile is the build's, not the call's
    (tq, wg, nc), _ = _launch(1, seen.pop() + 1, 4160)
    assert nc >= 2, (wg, nc)                    # a launch of two tiles is spread over the key ranges
    # any of the three pointers may be NULL
    p, keep = _idx_params()
    assert capi.lib().fa_mla_indexer_prefill_launch(ctypes.byref(p), None, None, None) == capi.FA_OK


def test_prefill_kernels_isa(capsys):
    """8 kernels ((fp16, bf16) x (16-bit, 8-bit cache) x (contiguous, paged)): no scratch, two 8 KB LDS stages, two workgroups a compute unit without AGPRs;
    the loop holds its MFMAs with LDS reads and barriers and without scratch traffic or accumulator moves; subnormals kept"""
    from _kernel_isa import analyse
    import build as B

    name = "fa_mla_indexer_prefill.hip"
    assert name in B.HIP_SOURCES and name in B.STAGE_SOURCES and B.HIP_SOURCES.index(name) < B.HIP_SOURCES.index("fa_capi.hip")
    assert all(name in B.DEBUG_VARIANTS[v] for v in ("stage_slow_reader", "stage_slow_writer", "stage_racy_slow_writer"))
    ks = analyse(name)
    assert len(ks) == 8, sorted(ks)
    (tq, _, _), _ = _launch(1, 1, 64)
    keys = set()
    with capsys.disabled():
        print()
        for n, k in sorted(ks.items()):
            m = re.search(r"fa_mla_indexer_prefill_logits_kernelI(DF16_|DF16b)Li(\d)ELb(\d)E", n)
            assert m, n
            keys.add(m.groups())
            print(f"  prefill logits TQ={tq} {m.group(1)} ES={m.group(2)} paged={m.group(3)}: {k['vgprs']} VGPRs, {k['agprs']} AGPRs, {k['scratch_bytes']} B scratch, "
                  f"{k['lds_bytes']} B LDS, occupancy {k['occupancy']}")
            assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
            assert k["lds_bytes"] == 2 * 32 * 256, (n, k["lds_bytes"])
            assert k["vgprs"] <= 256 and k["agprs"] == 0 and k["occupancy"] >= 2, (n, k["vgprs"], k["agprs"], k["occupancy"])
            assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
            assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
            assert k["loops"], f"{n}: no MFMA loop found"
            for lp in k["loops"]:
                assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
            main = max(k["loops"], key=lambda lp: lp["mfma"])
            # a step of a wave: eight 16-byte fragment reads, and 2 x 4 MFMAs a token and head block in one basic block for each head count (4, 2, 1 blocks);
            # the loop holds two steps
            assert main["mfma"] == 2 * 2 * 4 * (4 + 2 + 1) * (tq // 4) and main["ds_read_b128"] == 2 * 8 and main["barriers"] == 2, (n, main["label"], main["mfma"], main["ds_read_b128"], main["barriers"])
    assert keys == {(t, e, p) for t in ("DF16_", "DF16b") for e in "12" for p in "01"}
