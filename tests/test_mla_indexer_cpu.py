"""CPU: the DeepSeek-V3.2 indexer (flash_mla_indexer_logits, flash_mla_indexer_topk, flash_mla_index_with_kvcache) without a GPU: signatures, every
refusal through Python and through the C ABI, struct layouts, the two models of tests/_mla_indexer_cases.py against brute force on the inputs the GPU
tests use, the tolerance (it holds for the formula in fp32 and bites on four wrong formulas), and the compiled kernels' resources."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _mla_indexer_cases as C
import flash_attn_turing as F
from flash_attn_turing import capi


# ---- 1. signatures -----------------------------------------------------------------------------------------------------------------------------

def _sig(fn):
    ps = inspect.signature(fn).parameters
    pos = [n for n, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD]
    kw = {n: p.default for n, p in ps.items() if p.kind == p.KEYWORD_ONLY}
    assert all(ps[n].default is inspect.Parameter.empty for n in pos)
    return pos, kw


def test_signatures():
    assert _sig(F.flash_mla_indexer_logits) == (["q_idx", "weights", "k_idx_cache", "cache_seqlens"], {"k_scale": None, "block_table": None, "causal": True})
    assert _sig(F.flash_mla_indexer_topk) == (["logits", "cache_seqlens", "topk"], {"causal": True})
    assert _sig(F.flash_mla_index_with_kvcache) == (["q_idx", "weights", "k_idx_cache", "cache_seqlens", "topk"],
                                                    {"k_scale": None, "block_table": None, "causal": True, "return_logits": False})
    for n in ("flash_mla_indexer_logits", "flash_mla_indexer_topk", "flash_mla_index_with_kvcache"):
        assert n in F.__all__
    # the call it feeds is unchanged
    assert _sig(F.flash_mla_sparse_with_kvcache)[0] == ["q", "kv_cache", "cache_seqlens", "indices"]


# ---- 2. refusals through Python ----------------------------------------------------------------------------------------------------------------

def _args(b=2, sq=2, h=64, cap=64, dt=torch.bfloat16, kdt=torch.float8_e4m3fn):
    return dict(q_idx=torch.zeros(b, sq, h, 128, dtype=dt), weights=torch.zeros(b, sq, h), k_idx_cache=torch.zeros(b, cap, 128).to(kdt),
                cache_seqlens=torch.zeros(b, dtype=torch.int32))


def _refused(word, topk=None, **change):
    a = _args()
    kw = {k: change.pop(k) for k in list(change) if k in ("k_scale", "block_table", "causal")}
    a.update(change)
    with pytest.raises(ValueError, match=word):
        F.flash_mla_indexer_logits(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], **kw)
    with pytest.raises(ValueError, match=word):
        F.flash_mla_index_with_kvcache(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], 32 if topk is None else topk, **kw)


def test_python_refusals_name_the_argument():
    z = torch.zeros
    _refused("q_idx", q_idx=z(2, 2, 64, 128))                                  # fp32
    _refused("q_idx", q_idx=z(2, 2, 64, 64, dtype=torch.bfloat16))             # width
    _refused("q_idx", q_idx=z(2, 2, 48, 128, dtype=torch.bfloat16))            # head count
    _refused("q_idx", q_idx=z(2, 64, 128, dtype=torch.bfloat16))               # rank
    _refused("q_idx", q_idx=z(2, 0, 64, 128, dtype=torch.bfloat16), weights=z(2, 0, 64))
    _refused("weights", weights=z(2, 2, 64, dtype=torch.bfloat16))
    _refused("weights", weights=z(2, 2, 32))
    _refused("k_idx_cache", k_idx_cache=z(2, 64, 128, dtype=torch.float16))    # neither q_idx's dtype nor e4m3
    _refused("k_idx_cache", k_idx_cache=z(2, 64, 64, dtype=torch.bfloat16))
    _refused("k_idx_cache", k_idx_cache=z(3, 64, 128, dtype=torch.bfloat16))   # batch
    _refused("k_idx_cache", k_idx_cache=z(2, 64, 1, 128, dtype=torch.bfloat16))
    # FP8 views must keep 16-byte loads: row stride, batch stride, storage offset - a ValueError, never a copy
    _refused("k_idx_cache", k_idx_cache=z(2, 64, 136, dtype=torch.uint8)[:, :, :128])
    _refused("k_idx_cache", k_idx_cache=z(2, 64 * 128 + 8, dtype=torch.uint8)[:, :64 * 128].unflatten(1, (64, 128)))
    _refused("k_idx_cache", k_idx_cache=z(2 * 64 * 128 + 8, dtype=torch.uint8)[8:].view(2, 64, 128))
    _refused("k_idx_cache", k_idx_cache=z(2, 64, 256, dtype=torch.uint8)[:, :, ::2])
    # ... a 16-bit cache: the same rule in elements of 8
    _refused("k_idx_cache", k_idx_cache=z(2, 64, 132, dtype=torch.bfloat16)[:, :, :128])
    _refused("k_idx_cache", k_idx_cache=z(2 * 64 * 128 + 4, dtype=torch.bfloat16)[4:].view(2, 64, 128))
    _refused("k_scale", k_scale=z(2, 64, dtype=torch.float64))
    _refused("k_scale", k_scale=z(2, 63))
    _refused("block_table", block_table=z(2, 4, dtype=torch.int64))
    _refused("block_table", block_table=z(3, 4, dtype=torch.int32))
    _refused("page_block_size", block_table=z(2, 4, dtype=torch.int32), k_idx_cache=z(5, 24, 128, dtype=torch.uint8))
    _refused("cache_seqlens", cache_seqlens=z(2, dtype=torch.int64))
    _refused("cache_seqlens", cache_seqlens=z(3, dtype=torch.int32))
    _refused("cache_seqlens", cache_seqlens=1.5)
    _refused("causal", causal=1)
    a = _args()
    for topk in (0, 31, 48, -32, 32.0, True):
        with pytest.raises(ValueError, match="topk"):
            F.flash_mla_index_with_kvcache(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], topk)
        with pytest.raises(ValueError, match="topk"):
            F.flash_mla_indexer_topk(torch.zeros(2, 2, 64), a["cache_seqlens"], topk)
    with pytest.raises(ValueError, match="logits"):
        F.flash_mla_indexer_topk(torch.zeros(2, 2, 64, dtype=torch.float16), a["cache_seqlens"], 32)
    with pytest.raises(ValueError, match="logits"):
        F.flash_mla_indexer_topk(torch.zeros(2, 2, 128)[:, :, ::2], a["cache_seqlens"], 32)
    with pytest.raises(ValueError, match="logits"):
        F.flash_mla_indexer_topk(torch.zeros(2, 64), a["cache_seqlens"], 32)
    with pytest.raises(ValueError, match="cache_seqlens"):
        F.flash_mla_indexer_topk(torch.zeros(2, 2, 64), torch.zeros(3, dtype=torch.int32), 32)
    with pytest.raises(ValueError, match="causal"):
        F.flash_mla_indexer_topk(torch.zeros(2, 2, 64), a["cache_seqlens"], 32, causal=None)
    # views that ARE addressable pass the checks (and stop at the host module, which wants a GPU): a padded row stride, a page-strided pool, k_scale as a view
    ok = torch.zeros(2, 64, 160, dtype=torch.uint8)[:, :, :128]
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_mla_indexer_logits(a["q_idx"], a["weights"], ok, a["cache_seqlens"], k_scale=torch.zeros(2, 128)[:, ::2])


# ---- 3. the C ABI ------------------------------------------------------------------------------------------------------------------------------

IDX_FIELDS = ["struct_size", "magic", "q_idx", "weights", "k_idx_cache", "k_scale", "logits", "cache_seqlens", "block_table", "b", "seqlen_q", "seqlen_cache", "h", "d",
              "dtype", "k_format", "is_causal", "page_block_size", "num_blocks", "reserved_", "q_idx_stride", "weights_stride", "k_cache_batch_stride", "k_cache_row_stride",
              "k_scale_batch_stride", "k_scale_row_stride", "logits_batch_stride", "logits_row_stride", "block_table_stride"]
TOPK_FIELDS = ["struct_size", "magic", "logits", "indices", "cache_seqlens", "b", "seqlen_q", "seqlen_cache", "topk", "is_causal", "reserved_", "logits_batch_stride",
               "logits_row_stride"]


def test_struct_layouts_and_the_feature_macro(tmp_path):
    assert [f[0] for f in capi.MlaIndexerParams._fields_] == IDX_FIELDS and [f[0] for f in capi.MlaTopkParams._fields_] == TOPK_FIELDS
    src = tmp_path / "indexer_layout.c"
    body = ""
    for st, fields in (("fa_mla_indexer_params", IDX_FIELDS), ("fa_mla_topk_params", TOPK_FIELDS)):
        body += "".join(f'    printf("{st}.{f} %zu %zu\\n", offsetof({st}, {f}), sizeof((({st}*)0)->{f}));\n' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_INDEXER\n#error "no FA_HAS_MLA_INDEXER"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu\\n", sizeof(fa_mla_indexer_params), sizeof(fa_mla_topk_params));\n'
                   '    printf("abi %d %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_INDEXER, FA_IDX_K_FP8_E4M3);\n' + body +
                   "    fa_mla_indexer_params p;\n    FA_PARAMS_INIT(p);\n    fa_mla_topk_params t;\n    FA_PARAMS_INIT(t);\n"
                   "    return p.struct_size == sizeof(p) && p.magic == FA_PARAMS_MAGIC && p.k_scale == NULL && p.reserved_ == 0 && t.struct_size == sizeof(t) && t.topk == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "indexer_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"] == [ctypes.sizeof(capi.MlaIndexerParams), ctypes.sizeof(capi.MlaTopkParams)] == [216, 72]
    assert got["abi"] == [4, 1, 1] and capi.lib().fa_abi_version() == 4 and capi.FA_IDX_K_FP8_E4M3 == 1
    for st, cls, fields in (("fa_mla_indexer_params", capi.MlaIndexerParams, IDX_FIELDS), ("fa_mla_topk_params", capi.MlaTopkParams, TOPK_FIELDS)):
        end = 0
        for f in fields:
            assert got[f"{st}.{f}"] == [getattr(cls, f).offset, getattr(cls, f).size], (st, f)
            assert got[f"{st}.{f}"][0] == end, f"{st}.{f}: padding in front of it"
            end = sum(got[f"{st}.{f}"])
        assert end == ctypes.sizeof(cls)
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define FA_HAS_MLA_INDEXER 1\b", text) and re.search(r"#define FA_ABI_VERSION 4\b", text)
    names = capi.declared_functions()
    for n in ("fa_run_mla_indexer_logits", "fa_run_mla_indexer_topk"):
        assert n in names and hasattr(capi.lib(), n)


def _idx_params(paged=False):
    """a valid struct over host tensors (the library validates before it launches; no test here reaches the launch)"""
    keep = dict(q=torch.zeros(2, 2, 64, 128, dtype=torch.bfloat16), w=torch.zeros(2, 2, 64), k=torch.zeros(8 if paged else 2, 64, 128, dtype=torch.uint8),
                sc=torch.zeros(8 if paged else 2, 64), lg=torch.zeros(2, 2, 256 if paged else 64), cs=torch.zeros(2, dtype=torch.int32),
                bt=torch.zeros(2, 4, dtype=torch.int32) if paged else None)
    p = capi.mla_indexer_params(keep["q"], keep["w"], keep["k"], keep["lg"], keep["cs"], k_scale=keep["sc"], block_table=keep["bt"], causal=True)
    return p, keep


def _code(p, fn, code, word):
    rc = fn(ctypes.byref(p), None)
    assert rc == code and word in capi.last_error(), (rc, capi.last_error(), word)


def test_c_abi_refusals_name_the_field():
    L = capi.lib()
    run = L.fa_run_mla_indexer_logits

    def bad(code, word, paged=False, **change):
        p, keep = _idx_params(paged)
        for k, v in change.items():
            setattr(p, k, v)
        _code(p, run, code, word)

    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=208)
    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=224)
    bad(capi.FA_ERR_BAD_ABI, "magic", magic=0)
    bad(capi.FA_ERR_BAD_SHAPE, "seqlen_q", seqlen_q=0)
    bad(capi.FA_ERR_BAD_SHAPE, "b=", b=-1)
    bad(capi.FA_ERR_BAD_HEADDIM, "h 48", h=48)
    bad(capi.FA_ERR_BAD_HEADDIM, "d 64", d=64)
    bad(capi.FA_ERR_BAD_DTYPE, "dtype", dtype=2)
    bad(capi.FA_ERR_BAD_DTYPE, "k_format", k_format=2)
    bad(capi.FA_ERR_BAD_SHAPE, "reserved_", reserved_=1)
    bad(capi.FA_ERR_NULL_POINTER, "q_idx", q_idx=None)
    bad(capi.FA_ERR_NULL_POINTER, "weights", weights=None)
    bad(capi.FA_ERR_NULL_POINTER, "k_idx_cache", k_idx_cache=None)
    bad(capi.FA_ERR_NULL_POINTER, "logits", logits=None)
    bad(capi.FA_ERR_BAD_STRIDE, "k_cache_row_stride", k_cache_row_stride=136)
    bad(capi.FA_ERR_BAD_STRIDE, "k_cache_row_stride", k_cache_row_stride=64)
    bad(capi.FA_ERR_BAD_STRIDE, "k_cache_batch_stride", k_cache_batch_stride=64 * 128 + 8)
    bad(capi.FA_ERR_BAD_STRIDE, "k_idx_cache", k_cache_row_stride=1 << 26)                  # one sequence spans 2^31 bytes or more
    bad(capi.FA_ERR_BAD_STRIDE, "logits_row_stride", logits_row_stride=63)
    bad(capi.FA_ERR_BAD_STRIDE, "q_idx strides", q_idx_stride=capi.Strides(2 * 64 * 128, 64 * 128, 132))
    bad(capi.FA_ERR_BAD_SHAPE, "page_block_size", paged=True, page_block_size=24)
    bad(capi.FA_ERR_BAD_SHAPE, "page_block_size", paged=True, page_block_size=0)
    bad(capi.FA_ERR_BAD_SHAPE, "num_blocks", paged=True, num_blocks=0)
    bad(capi.FA_ERR_BAD_SHAPE, "seqlen_cache", paged=True, seqlen_cache=250)
    bad(capi.FA_ERR_BAD_STRIDE, "block_table_stride", paged=True, block_table_stride=3)
    bad(capi.FA_ERR_NULL_POINTER, "page_block_size", page_block_size=64)                    # without block_table
    # pointers that break the alignment rules
    p, keep = _idx_params()
    p.k_idx_cache = keep["k"].data_ptr() + 8
    _code(p, run, capi.FA_ERR_BAD_STRIDE, "k_idx_cache")
    p, keep = _idx_params()
    p.k_scale = keep["sc"].data_ptr() + 2
    _code(p, run, capi.FA_ERR_BAD_STRIDE, "k_scale")
    # a 16-bit cache: strides in elements of 8
    p, keep = _idx_params()
    p.k_format, p.k_cache_row_stride = 0, 132
    _code(p, run, capi.FA_ERR_BAD_STRIDE, "k_cache_row_stride")
    # b == 0: FA_OK without a launch, whatever the pointers
    p, keep = _idx_params()
    p.b, p.q_idx, p.weights, p.k_idx_cache, p.logits = 0, None, None, None, None
    assert run(ctypes.byref(p), None) == capi.FA_OK
    assert run(None, None) == capi.FA_ERR_NULL_POINTER

    topk = L.fa_run_mla_indexer_topk

    def tbad(code, word, **change):
        lg, idx, cs = torch.zeros(2, 2, 64), torch.zeros(2, 2, 32, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
        p = capi.mla_topk_params(lg, idx, cs)
        for k, v in change.items():
            setattr(p, k, v)
        _code(p, topk, code, word)

    tbad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=64)
    tbad(capi.FA_ERR_BAD_ABI, "magic", magic=1)
    for t in (0, 31, 48, -32):
        tbad(capi.FA_ERR_BAD_SHAPE, "topk", topk=t)
    tbad(capi.FA_ERR_BAD_SHAPE, "seqlen_q", seqlen_q=0)
    tbad(capi.FA_ERR_BAD_SHAPE, "reserved_", reserved_=7)
    tbad(capi.FA_ERR_NULL_POINTER, "indices", indices=None)
    tbad(capi.FA_ERR_NULL_POINTER, "logits", logits=None)
    tbad(capi.FA_ERR_BAD_STRIDE, "logits_row_stride", logits_row_stride=-1)
    p = capi.mla_topk_params(torch.zeros(2, 2, 64), torch.zeros(2, 2, 32, dtype=torch.int32), None)
    p.b, p.logits, p.indices = 0, None, None
    assert topk(ctypes.byref(p), None) == capi.FA_OK


# ---- 4. the two models against brute force, on the inputs of the GPU tests ------------------------------------------------------------------

@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("kind", ["exact", "normal"])
def test_logits_model_equals_brute_force(kind, fp8):
    gen = torch.Generator().manual_seed(11)
    make = C.exact_inputs if kind == "exact" else C.normal_inputs
    q, w, k, sc = make(2, 3, 16, torch.bfloat16, fp8, gen)
    ref, mag = C.logits_model(q, w, k, sc)
    rng = np.random.default_rng(5)
    for _ in range(40):
        i, t, j = int(rng.integers(2)), int(rng.integers(3)), int(rng.integers(C.CAP))
        want = C.logits_brute(q, w, k, sc, i, t, j)
        if kind == "exact":
            assert float(ref[i, t, j]) == want
        else:
            assert abs(float(ref[i, t, j]) - want) <= 1e-12 * float(mag[i, t, j])
    if kind == "exact":     # exact in fp32 as well: the formula in torch fp32 gives the same bits
        assert torch.equal(C.logits_fp32_formula(q, w, k, sc).double(), ref)


def test_visibility_is_the_dense_mla_rule():
    for L in C.LENS + [320, 500, -3]:
        for sq in (1, 3):
            for t in range(sq):
                Lc = min(max(L, 0), C.CAP)
                assert C.visible(L, sq, t, False, C.CAP) == Lc
                # key j is visible iff j < L and j <= L - sq + t
                assert C.visible(L, sq, t, True, C.CAP) == sum(1 for j in range(C.CAP) if j < Lc and j <= Lc - sq + t)
    m = C.visible_mask([33, 1], 3, C.CAP, True)
    assert m.sum(-1).tolist() == [[31, 32, 33], [0, 0, 1]]


def test_topk_model_equals_brute_force():
    u = C.order_key(C.f32([0x80000000, 0x00000000, 0x7F800000, 0x7FC00000, 0xFF800000, 0xFFC00000, 0x00000001, 0x80000001]))
    # -0 < +0; +inf < NaN with the sign clear; NaN with the sign set is below -inf; subnormals keep their order
    assert u[0] < u[1] and u[2] < u[3] and u[5] < u[4] < u[7] < u[0] and u[1] < u[6] < u[2]
    for name, (row, n, topk) in C.topk_rows().items():
        got = C.topk_row_model(row, n, topk)
        assert got.dtype == np.int32 and got.shape == (topk,)
        if n <= 3000:
            assert got.tolist() == C.topk_row_brute(row, n, topk), name
        sel = got[got >= 0]
        assert (np.diff(sel) > 0).all() and (sel < n).all() and len(sel) == min(n, topk), name
        if n > topk:        # nothing left out beats anything taken; among equals the lower position was taken
            uu = C.order_key(row[:n])
            out = np.setdiff1d(np.arange(n), sel)
            thr = uu[sel].min()
            assert uu[out].max() <= thr, name
            ties_out = out[uu[out] == thr]
            ties_in = sel[uu[sel] == thr]
            assert len(ties_out) == 0 or ties_in.max() < ties_out.min(), name
    assert C.topk_row_model(np.full(700, 1.5, np.float32), 700, 64).tolist() == list(range(64))
    stacked = C.topk_model(np.zeros((2, 2, 50), np.float32), [40, 3], 32, True)
    assert stacked[0, 0].tolist() == list(range(32)) and stacked[1, 0].tolist() == [0, 1] + [-1] * 30 and stacked[1, 1].tolist() == [0, 1, 2] + [-1] * 29


# ---- 5. the tolerance holds for the formula and bites on wrong ones ------------------------------------------------------------------------

@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("h", [16, 64])
def test_the_tolerance_bites(h, dt, fp8):
    gen = torch.Generator().manual_seed(3)
    q, w, k, sc = C.normal_inputs(2, 3, h, dt, fp8, gen)
    ref, mag = C.logits_model(q, w, k, sc)
    worst = lambda x: float(((x.double() - ref).abs() / mag).max())
    assert worst(C.logits_fp32_formula(q, w, k, sc)) <= C.TOL
    assert worst(C.logits_model(q, w, k, sc, variant="drop_head")[0]) > C.TOL
    assert worst(C.logits_model(q, w, k, sc, variant="no_relu")[0]) > C.TOL
    assert worst(C.logits_model(q, w, k, sc * (1 + 2.0 ** -10))[0]) > C.TOL
    kf = C.keys_as_float64(k).to(torch.float32)
    assert worst(C.logits_model(q, w, torch.roll(kf, 1, dims=1), sc)[0]) > C.TOL


# ---- 6. the compiled kernels -----------------------------------------------------------------------------------------------------------------

def test_indexer_kernels_isa():
    """8 logits kernels ((fp16, bf16) x (16-bit, 8-bit cache) x (contiguous, paged)) and the selection kernel: no scratch anywhere; the logits loop holds
    its MFMAs without scratch traffic or accumulator moves, needs no LDS and no barrier, and two waves fit a SIMD; subnormals kept"""
    from _kernel_isa import analyse
    import build as B

    assert "fa_mla_indexer.hip" in B.HIP_SOURCES and B.HIP_SOURCES.index("fa_mla_indexer.hip") < B.HIP_SOURCES.index("fa_capi.hip")
    assert "fa_mla_indexer.hpp" in B.HIP_HEADERS
    ks = analyse("fa_mla_indexer.hip")
    logits = {n: k for n, k in ks.items() if "fa_mla_indexer_logits_kernel" in n}
    topk = {n: k for n, k in ks.items() if "fa_mla_indexer_topk_kernel" in n}
    assert len(logits) == 8 and len(topk) == 1 and len(ks) == 9, sorted(ks)
    keys = set()
    for n, k in ks.items():
        assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
        assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
    for n, k in logits.items():
        m = re.search(r"fa_mla_indexer_logits_kernelI(DF16_|DF16b)Li(\d)ELb(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["lds_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 256 and k["occupancy"] >= 2, (n, k["lds_bytes"], k["vgprs"], k["agprs"], k["occupancy"])
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0 and lp["barriers"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        assert max(lp["mfma"] for lp in k["loops"]) == 64, n                   # two 32-key steps of 2 x 4 x 4 MFMAs
    assert keys == {(t, e, p) for t in ("DF16_", "DF16b") for e in "12" for p in "01"}
    (k,) = topk.values()
    assert k["mfma_total"] == 0 and 0 < k["lds_bytes"] <= 32768 and k["vgprs"] <= 64
