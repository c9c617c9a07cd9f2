"""CPU: the stand-alone append and gather of the MLA caches (flash_mla_cache_append, flash_mla_cache_gather, flash_mla_index_cache_append,
quantize_mla_index_keys) without a GPU: exports and signatures, every refusal through Python and through the C ABI, struct layouts, the index-key quantiser
against the independent model of tests/_mla_cache_io_cases.py and against one tile of quantize_mla_kv_cache, and the build wiring."""
import ctypes
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _mla_cache_io_cases as C
import flash_attn_turing as F
from flash_attn_turing import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
z = torch.zeros
BF, I32 = torch.bfloat16, torch.int32


# ---- 1. exports and signatures -------------------------------------------------------------------------------------------------------------------

def _sig(fn):
    ps = inspect.signature(fn).parameters
    pos = [n for n, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD and p.default is inspect.Parameter.empty]
    rest = {n: p.default for n, p in ps.items() if n not in pos}
    kinds = {p.kind for n, p in ps.items() if n not in pos}
    return pos, rest, kinds


def test_exports_and_signatures():
    kw_only = {inspect.Parameter.KEYWORD_ONLY}
    assert _sig(F.flash_mla_cache_append) == (["kv_cache", "kv_new", "cache_seqlens"], {"k_pe": None, "block_table": None, "cu_seqlens_new": None}, kw_only)
    assert _sig(F.flash_mla_cache_gather) == (["kv_cache", "cache_seqlens", "out"], {"block_table": None, "cu_seqlens_out": None, "seq_starts": None}, kw_only)
    assert _sig(F.flash_mla_index_cache_append) == (["k_idx_cache", "k_idx_new", "cache_seqlens"],
                                                    {"k_scale": None, "block_table": None, "cu_seqlens_new": None, "scale_format": "fp32"}, kw_only)
    assert _sig(F.quantize_mla_index_keys) == (["k"], {"scale_format": "fp32"}, {inspect.Parameter.POSITIONAL_OR_KEYWORD})
    for n in ("flash_mla_cache_append", "flash_mla_cache_gather", "flash_mla_index_cache_append", "quantize_mla_index_keys"):
        assert n in F.__all__ and getattr(F, n) is getattr(F.interface, n)


# ---- 2. refusals through Python ------------------------------------------------------------------------------------------------------------------

def _append(word, exc=ValueError, **change):
    a = dict(kv_cache=z(2, 32, 1, 576, dtype=BF), kv_new=z(2, 3, 1, 576, dtype=BF), cache_seqlens=z(2, dtype=I32))
    kw = {k: change.pop(k) for k in list(change) if k in ("k_pe", "block_table", "cu_seqlens_new")}
    a.update(change)
    with pytest.raises(exc, match=word):
        F.flash_mla_cache_append(a["kv_cache"], a["kv_new"], a["cache_seqlens"], **kw)


def _gather(word, exc=ValueError, **change):
    a = dict(kv_cache=z(2, 32, 1, 576, dtype=BF), cache_seqlens=z(2, dtype=I32), out=z(2, 5, 576, dtype=BF))
    kw = {k: change.pop(k) for k in list(change) if k in ("block_table", "cu_seqlens_out", "seq_starts")}
    a.update(change)
    with pytest.raises(exc, match=word):
        F.flash_mla_cache_gather(a["kv_cache"], a["cache_seqlens"], a["out"], **kw)


def _index(word, exc=ValueError, **change):
    a = dict(k_idx_cache=z(2, 32, 128, dtype=torch.uint8), k_idx_new=z(2, 3, 128, dtype=BF), cache_seqlens=z(2, dtype=I32), k_scale=z(2, 32))
    kw = {k: change.pop(k) for k in list(change) if k in ("block_table", "cu_seqlens_new", "scale_format")}
    a.update(change)
    with pytest.raises(exc, match=word):
        F.flash_mla_index_cache_append(a["k_idx_cache"], a["k_idx_new"], a["cache_seqlens"], k_scale=a["k_scale"], **kw)


def test_latent_append_refusals_name_the_argument():
    _append("kv_cache", kv_cache=z(2, 32, 576, dtype=BF))                                  # rank
    _append("kv_cache", kv_cache=z(2, 32, 1, 576))                                         # fp32
    _append("kv_cache", kv_cache=z(2, 32, 1, 512, dtype=BF))                               # width
    _append("kv_cache", kv_cache=z(2, 32, 1, 576, dtype=torch.uint8))                      # a 1-byte cache that is not 656 wide
    _append("kv_cache", kv_cache=z(2, 32, 2, 576, dtype=BF))                               # heads
    _append("kv_cache", kv_cache=z(2, 32, 1, 580, dtype=BF)[..., :576])                    # row stride no multiple of 8
    _append("kv_cache", kv_cache=z(2 * 32 * 576 + 4, dtype=BF)[4:].view(2, 32, 1, 576))    # storage offset
    _append("kv_cache", kv_cache=z(2, 32, 1, 664, dtype=torch.uint8)[..., :656])           # FP8 rows: stride no multiple of 16
    _append("kv_cache", kv_cache=z(3, 32, 1, 576, dtype=BF))                               # batch
    _append("kv_new", kv_new=z(2, 3, 1, 576))                                              # dtype
    _append("kv_new", kv_new=z(2, 3, 1, 576, dtype=torch.float16))                         # not the 16-bit cache's dtype
    _append("kv_new", kv_new=z(2, 3, 1, 500, dtype=BF))                                    # width
    _append("kv_new", kv_new=z(2, 3, 576, dtype=BF))                                       # rank of a dense call
    _append("kv_new", kv_new=z(2, 3, 2, 576, dtype=BF))                                    # heads
    _append("kv_new", kv_new=z(2, 3, 1, 580, dtype=BF)[..., :576])                         # strides
    _append("kv_new", kv_new=z(2, 3, 1, 1152, dtype=BF)[..., ::2])                         # last dimension
    _append("kv_new", kv_new=z(2 * 3 * 576 + 4, dtype=BF)[4:].view(2, 3, 1, 576))          # offset
    _append("k_pe", kv_new=z(2, 3, 1, 512, dtype=BF))                                      # 512 wide without k_pe
    _append("k_pe", k_pe=z(2, 3, 1, 64, dtype=BF))                                         # k_pe with 576 wide rows
    _append("k_pe", kv_new=z(2, 3, 1, 512, dtype=BF), k_pe=z(2, 3, 1, 32, dtype=BF))
    _append("k_pe", kv_new=z(2, 3, 1, 512, dtype=BF), k_pe=z(2, 4, 1, 64, dtype=BF))
    _append("k_pe", kv_new=z(2, 3, 1, 512, dtype=BF), k_pe=z(2, 3, 1, 64, dtype=torch.float16))
    _append("k_pe", kv_new=z(2, 3, 1, 512, dtype=BF), k_pe=z(2, 3, 1, 68, dtype=BF)[..., :64])
    _append("cu_seqlens_new", kv_new=z(6, 1, 576, dtype=BF), cu_seqlens_new=z(3, dtype=torch.int64))
    _append("cu_seqlens_new", kv_new=z(6, 1, 576, dtype=BF), cu_seqlens_new=z(3, 1, dtype=I32))
    _append("cu_seqlens_new", kv_new=z(6, 1, 576, dtype=BF), cu_seqlens_new=z(3, dtype=I32, device="meta"))
    _append("kv_new", kv_new=z(2, 3, 1, 576, dtype=BF), cu_seqlens_new=z(3, dtype=I32))    # a rank-4 kv_new belongs to the dense call
    _append("cache_seqlens", cache_seqlens=z(3, dtype=I32))
    _append("cache_seqlens", cache_seqlens=z(2, dtype=torch.int64))
    _append("cache_seqlens", kv_new=z(6, 1, 576, dtype=BF), cu_seqlens_new=z(4, dtype=I32), kv_cache=z(3, 32, 1, 576, dtype=BF))     # batch = len(cu) - 1
    _append("block_table", block_table=z(2, 2, dtype=torch.int64))
    _append("block_table", block_table=z(3, 2, dtype=I32))
    _append("page_block_size", block_table=z(2, 2, dtype=I32), kv_cache=z(5, 24, 1, 576, dtype=BF))
    # addressable views pass the checks and stop at the host module, which wants a GPU
    _append("GPU", RuntimeError)
    _append("GPU", RuntimeError, kv_cache=z(2, 32, 1, 656, dtype=torch.uint8), kv_new=z(2, 3, 1, 640, dtype=torch.float16)[..., :512],
            k_pe=z(2, 3, 1, 128, dtype=torch.float16)[..., 64:])
    _append("GPU", RuntimeError, kv_cache=z(5, 16, 1, 576, dtype=BF), block_table=z(2, 2, dtype=I32), kv_new=z(6, 1, 576, dtype=BF), cu_seqlens_new=z(3, dtype=I32))
    # nothing to write: no launch, so no GPU is asked for
    assert F.flash_mla_cache_append(z(2, 32, 1, 576, dtype=BF), z(2, 0, 1, 576, dtype=BF), 0) is None
    assert F.flash_mla_cache_append(z(0, 32, 1, 576, dtype=BF), z(0, 3, 1, 576, dtype=BF), 0) is None


def test_latent_gather_refusals_name_the_argument():
    _gather("kv_cache", kv_cache=z(2, 32, 1, 512, dtype=BF))
    _gather("kv_cache", kv_cache=z(2, 32, 1, 672, dtype=torch.uint8)[..., 8:664])          # FP8 rows at an offset of 8 bytes
    _gather("kv_cache", kv_cache=z(3, 32, 1, 576, dtype=BF))
    _gather("out", out=z(2, 5, 576))                                                       # dtype
    _gather("out", out=z(2, 5, 576, dtype=torch.float16))                                  # not the 16-bit cache's dtype
    _gather("out", out=z(2, 5, 512, dtype=BF))
    _gather("out", out=z(10, 576, dtype=BF))                                               # rank of a dense call
    _gather("out", out=z(2, 5, 580, dtype=BF)[..., :576])                                  # row stride no multiple of 8
    _gather("out", out=z(2, 5, 1152, dtype=BF)[..., ::2])
    _gather("out", out=z(2, 1, 576, dtype=BF).expand(2, 5, 576))                           # rows closer than 576
    _gather("out", out=z(2 * 5 * 576 + 4, dtype=BF)[4:].view(2, 5, 576))
    _gather("out", out=z(2, 5, 576, dtype=BF), cu_seqlens_out=z(3, dtype=I32))             # a rank-3 out belongs to the dense call
    _gather("cu_seqlens_out", out=z(10, 576, dtype=BF), cu_seqlens_out=z(3, dtype=torch.int64))
    _gather("cu_seqlens_out", out=z(10, 576, dtype=BF), cu_seqlens_out=z(3, dtype=I32, device="meta"))
    _gather("cache_seqlens", cache_seqlens=z(3, dtype=I32))
    _gather("cache_seqlens", cache_seqlens=1.5)
    _gather("seq_starts", seq_starts=z(3, dtype=I32))
    _gather("seq_starts", seq_starts=z(2, dtype=torch.int64))
    _gather("block_table", block_table=z(3, 2, dtype=I32))
    _gather("GPU", RuntimeError)
    _gather("GPU", RuntimeError, cache_seqlens=None, kv_cache=z(2, 32, 1, 656, dtype=torch.float8_e4m3fn), out=z(10, 640, dtype=torch.float16)[:, :576],
            cu_seqlens_out=z(3, dtype=I32), seq_starts=z(2, dtype=I32))
    out = z(2, 0, 576, dtype=BF)
    assert F.flash_mla_cache_gather(z(2, 32, 1, 576, dtype=BF), None, out) is out


def test_index_append_refusals_name_the_argument():
    _index("k_idx_cache", k_idx_cache=z(2, 32, 1, 128, dtype=torch.uint8))
    _index("k_idx_cache", k_idx_cache=z(2, 32, 128))
    _index("k_idx_cache", k_idx_cache=z(2, 32, 64, dtype=torch.uint8))
    _index("k_idx_cache", k_idx_cache=z(2, 32, 136, dtype=torch.uint8)[:, :, :128])
    _index("k_idx_cache", k_idx_cache=z(2 * 32 * 128 + 8, dtype=torch.uint8)[8:].view(2, 32, 128))
    _index("k_idx_cache", k_idx_cache=z(2, 32, 132, dtype=BF)[:, :, :128], k_scale=None)
    _index("k_idx_cache", k_idx_cache=z(3, 32, 128, dtype=torch.uint8), k_scale=z(3, 32))
    _index("k_idx_new", k_idx_new=z(2, 3, 128))
    _index("k_idx_new", k_idx_new=z(2, 3, 64, dtype=BF))
    _index("k_idx_new", k_idx_new=z(6, 128, dtype=BF))
    _index("k_idx_new", k_idx_new=z(2, 3, 132, dtype=BF)[..., :128])
    _index("k_idx_new", k_idx_cache=z(2, 32, 128, dtype=BF), k_idx_new=z(2, 3, 128, dtype=torch.float16), k_scale=None)
    _index("k_scale", k_idx_cache=z(2, 32, 128, dtype=BF))                                 # k_scale with a 16-bit cache
    _index("k_scale", k_scale=None)                                                        # ... missing with an FP8 one
    _index("k_scale", k_scale=z(2, 32, dtype=torch.float64))
    _index("k_scale", k_scale=z(2, 31))
    _index("scale_format", scale_format="e8m0")
    _index("scale_format", scale_format=1)
    _index("cu_seqlens_new", k_idx_new=z(6, 128, dtype=BF), cu_seqlens_new=z(3, dtype=torch.int64))
    _index("cu_seqlens_new", k_idx_new=z(6, 128, dtype=BF), cu_seqlens_new=z(3, dtype=I32, device="meta"))
    _index("cache_seqlens", cache_seqlens=z(3, dtype=I32))
    _index("block_table", block_table=z(2, 2, dtype=torch.int64))
    _index("page_block_size", block_table=z(2, 2, dtype=I32), k_idx_cache=z(5, 24, 128, dtype=torch.uint8), k_scale=z(5, 24))
    _index("GPU", RuntimeError)
    _index("GPU", RuntimeError, scale_format="ue8m0", k_idx_cache=z(2, 32, 160, dtype=torch.float8_e4m3fn)[:, :, :128], k_scale=z(2, 64)[:, ::2],
           k_idx_new=z(6, 128, dtype=torch.float16), cu_seqlens_new=z(3, dtype=I32))
    _index("GPU", RuntimeError, k_idx_cache=z(2, 32, 128, dtype=BF), k_scale=None)
    assert F.flash_mla_index_cache_append(z(2, 32, 128, dtype=BF), z(2, 0, 128, dtype=BF), 0) is None
    with pytest.raises(ValueError, match="scale_format"):
        F.quantize_mla_index_keys(z(2, 128, dtype=BF), "ue8")
    for bad in (z(2, 128), z(2, 64, dtype=BF), None):
        with pytest.raises(ValueError, match="k must be"):
            F.quantize_mla_index_keys(bad)


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------------------------------------

APPEND_FIELDS = ["struct_size", "magic", "kv_cache", "kv_new", "k_pe", "cache_seqlens", "cu_seqlens_new", "block_table", "b", "seqlen_new", "seqlen_cache", "dtype",
                 "kv_format", "page_block_size", "num_blocks", "reserved_", "total_new", "kv_cache_stride", "kv_new_stride", "k_pe_stride", "block_table_stride"]
GATHER_FIELDS = ["struct_size", "magic", "kv_cache", "out", "cache_seqlens", "cu_seqlens_out", "seq_starts", "block_table", "b", "seqlen_out", "seqlen_cache", "dtype",
                 "kv_format", "page_block_size", "num_blocks", "reserved_", "total_out", "kv_cache_stride", "out_batch_stride", "out_row_stride", "block_table_stride"]
INDEX_FIELDS = ["struct_size", "magic", "k_idx_cache", "k_scale", "k_idx_new", "cache_seqlens", "cu_seqlens_new", "block_table", "b", "seqlen_new", "seqlen_cache",
                "dtype", "k_format", "scale_format", "page_block_size", "num_blocks", "total_new", "reserved_", "k_cache_batch_stride", "k_cache_row_stride",
                "k_scale_batch_stride", "k_scale_row_stride", "k_new_batch_stride", "k_new_row_stride", "block_table_stride"]
STRUCTS = (("fa_mla_cache_append_params", "MlaCacheAppendParams", APPEND_FIELDS, 176), ("fa_mla_cache_gather_params", "MlaCacheGatherParams", GATHER_FIELDS, 144),
           ("fa_mla_index_cache_append_params", "MlaIndexCacheAppendParams", INDEX_FIELDS, 160))


def test_struct_layouts_and_the_feature_macro(tmp_path):
    body = ""
    for st, cls, fields, size in STRUCTS:
        assert [f[0] for f in getattr(capi, cls)._fields_] == fields
        body += f'    printf("{st} %zu 0\\n", sizeof({st}));\n'
        body += "".join(f'    printf("{st}.{f} %zu %zu\\n", offsetof({st}, {f}), sizeof((({st}*)0)->{f}));\n' for f in fields)
    src = tmp_path / "cache_io_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_CACHE_IO\n#error "no FA_HAS_MLA_CACHE_IO"\n#endif\n'
                   "int main(void) {\n"
                   '    printf("abi %d %d %d %d %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_CACHE_IO, FA_IDX_SCALE_FP32, FA_IDX_SCALE_UE8M0, FA_MLA_KV_FP8_ROWS656, FA_IDX_K_FP8_E4M3);\n'
                   + body +
                   "    fa_mla_cache_append_params a;\n    FA_PARAMS_INIT(a);\n    fa_mla_cache_gather_params g;\n    FA_PARAMS_INIT(g);\n"
                   "    fa_mla_index_cache_append_params x;\n    FA_PARAMS_INIT(x);\n"
                   "    return a.struct_size == sizeof(a) && a.magic == FA_PARAMS_MAGIC && a.k_pe == NULL && g.struct_size == sizeof(g) && g.seq_starts == NULL "
                   "&& x.struct_size == sizeof(x) && x.scale_format == FA_IDX_SCALE_FP32 && x.reserved_ == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "cache_io_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["abi"] == [4, 1, 0, 1, 1, 1] and capi.lib().fa_abi_version() == 4
    assert (capi.FA_IDX_SCALE_FP32, capi.FA_IDX_SCALE_UE8M0) == (0, 1)
    for st, cls, fields, size in STRUCTS:
        cls = getattr(capi, cls)
        assert got[st][0] == ctypes.sizeof(cls) == size, (st, got[st], ctypes.sizeof(cls))
        end = 0
        for f in fields:
            assert got[f"{st}.{f}"] == [getattr(cls, f).offset, getattr(cls, f).size], (st, f)
            assert got[f"{st}.{f}"][0] == end, f"{st}.{f}: padding in front of it"
            end = sum(got[f"{st}.{f}"])
        assert end == ctypes.sizeof(cls)
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define FA_HAS_MLA_CACHE_IO 1\b", text) and re.search(r"#define FA_ABI_VERSION 4\b", text)
    for n in ("fa_run_mla_cache_append", "fa_run_mla_cache_gather", "fa_run_mla_index_cache_append"):
        assert n in capi.declared_functions() and hasattr(capi.lib(), n)


def _code(p, fn, code, word):
    rc = fn(ctypes.byref(p), None)
    assert rc == code and word in capi.last_error(), (rc, capi.last_error(), word)


def _append_params(paged=False, packed=False, fp8=False, k_pe=False):
    """valid structs over host tensors (the library validates before it launches; no test here reaches a launch)"""
    w = 512 if k_pe else 576
    keep = dict(c=z(8 if paged else 2, 32, 1, 656, dtype=torch.uint8) if fp8 else z(8 if paged else 2, 32, 1, 576, dtype=BF),
                n=z(6, 1, w, dtype=BF) if packed else z(2, 3, 1, w, dtype=BF), cs=z(2, dtype=I32), bt=z(2, 4, dtype=I32) if paged else None,
                cu=z(3, dtype=I32) if packed else None)
    keep["pe"] = z(*keep["n"].shape[:-1], 64, dtype=BF) if k_pe else None
    return capi.mla_cache_append_params(keep["c"], keep["n"], keep["cs"], k_pe=keep["pe"], block_table=keep["bt"], cu_seqlens_new=keep["cu"]), keep


def _gather_params(paged=False, packed=False, fp8=False):
    keep = dict(c=z(8 if paged else 2, 32, 1, 656, dtype=torch.uint8) if fp8 else z(8 if paged else 2, 32, 1, 576, dtype=BF),
                o=z(10, 576, dtype=BF) if packed else z(2, 5, 576, dtype=BF), cs=z(2, dtype=I32), st=z(2, dtype=I32), bt=z(2, 4, dtype=I32) if paged else None,
                cu=z(3, dtype=I32) if packed else None)
    return capi.mla_cache_gather_params(keep["c"], keep["o"], keep["cs"], block_table=keep["bt"], cu_seqlens_out=keep["cu"], seq_starts=keep["st"]), keep


def _index_params(paged=False, packed=False, fp8=True):
    keep = dict(c=z(8 if paged else 2, 32, 128, dtype=torch.uint8 if fp8 else BF), sc=z(8 if paged else 2, 32) if fp8 else None,
                n=z(6, 128, dtype=BF) if packed else z(2, 3, 128, dtype=BF), cs=z(2, dtype=I32), bt=z(2, 4, dtype=I32) if paged else None,
                cu=z(3, dtype=I32) if packed else None)
    return capi.mla_index_cache_append_params(keep["c"], keep["n"], keep["cs"], k_scale=keep["sc"], block_table=keep["bt"], cu_seqlens_new=keep["cu"]), keep


def _bad(make, run, code, word, _args=(), **change):
    p, keep = make(*_args)
    for k, v in change.items():
        setattr(p, k, v)
    _code(p, run, code, word)


def test_c_abi_refusals_name_the_field():
    L = capi.lib()
    S = capi.Strides
    for make, run, rows, total, cu in ((_append_params, L.fa_run_mla_cache_append, "seqlen_new", "total_new", "cu_seqlens_new"),
                                      (_gather_params, L.fa_run_mla_cache_gather, "seqlen_out", "total_out", "cu_seqlens_out"),
                                      (_index_params, L.fa_run_mla_index_cache_append, "seqlen_new", "total_new", "cu_seqlens_new")):
        size = make()[0].struct_size
        _bad(make, run, capi.FA_ERR_BAD_ABI, "struct_size", struct_size=size - 8)
        _bad(make, run, capi.FA_ERR_BAD_ABI, "struct_size", struct_size=size + 8)
        _bad(make, run, capi.FA_ERR_BAD_ABI, "magic", magic=0)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "b=", b=-1)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, rows, **{rows: -1})
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "seqlen_cache", seqlen_cache=-1)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, total, (False, True), **{total: -1})
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "call too large", **{rows: 1 << 30})
        _bad(make, run, capi.FA_ERR_BAD_DTYPE, "dtype", dtype=2)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "reserved_", reserved_=1)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "page_block_size", (True,), page_block_size=24)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "page_block_size", (True,), page_block_size=0)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "num_blocks", (True,), num_blocks=0)
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "seqlen_cache", (True,), seqlen_cache=100)
        _bad(make, run, capi.FA_ERR_BAD_STRIDE, "block_table_stride", (True,), block_table_stride=3)
        _bad(make, run, capi.FA_ERR_NULL_POINTER, "page_block_size", page_block_size=32)              # without block_table
        p, keep = make(False, True)
        setattr(p, cu, keep["cu"].data_ptr() + 2)
        _code(p, run, capi.FA_ERR_BAD_STRIDE, cu)
        # b == 0 and no rows: FA_OK without a launch, whatever the pointers
        for field in ("b", rows):
            p, keep = make()
            setattr(p, field, 0)
            for f, t in p._fields_:
                if t is ctypes.c_void_p:
                    setattr(p, f, None)
            assert run(ctypes.byref(p), None) == capi.FA_OK, capi.last_error()
        assert run(None, None) == capi.FA_ERR_NULL_POINTER

    # the latent cache, both calls
    for make, run in ((_append_params, L.fa_run_mla_cache_append), (_gather_params, L.fa_run_mla_cache_gather)):
        _bad(make, run, capi.FA_ERR_BAD_SHAPE, "kv_format", kv_format=2)
        _bad(make, run, capi.FA_ERR_NULL_POINTER, "kv_cache", kv_cache=None)
        _bad(make, run, capi.FA_ERR_BAD_STRIDE, "kv_cache", kv_cache_stride=S(32 * 576, 580, 0))
        _bad(make, run, capi.FA_ERR_BAD_STRIDE, "kv_cache", kv_cache_stride=S(32 * 576, 512, 0))
        _bad(make, run, capi.FA_ERR_BAD_STRIDE, "kv_cache", (False, False, True), kv_cache_stride=S(32 * 656, 664, 0))      # FP8 rows: bytes, multiples of 16
        _bad(make, run, capi.FA_ERR_BAD_STRIDE, "kv_cache", (False, False, True), kv_cache_stride=S(32 * 656 + 8, 656, 0))
        p, keep = make()
        p.kv_cache = keep["c"].data_ptr() + 8
        _code(p, run, capi.FA_ERR_BAD_STRIDE, "kv_cache")
    run = L.fa_run_mla_cache_append
    _bad(_append_params, run, capi.FA_ERR_NULL_POINTER, "cache_seqlens", cache_seqlens=None)
    _bad(_append_params, run, capi.FA_ERR_NULL_POINTER, "kv_new", kv_new=None)
    _bad(_append_params, run, capi.FA_ERR_BAD_STRIDE, "kv_new", kv_new_stride=S(3 * 576, 580, 0))
    _bad(_append_params, run, capi.FA_ERR_BAD_STRIDE, "kv_new", kv_new_stride=S(3 * 576 + 4, 576, 0))
    _bad(_append_params, run, capi.FA_ERR_BAD_STRIDE, "k_pe", (False, False, False, True), k_pe_stride=S(3 * 64, 68, 0))
    p, keep = _append_params()
    p.kv_new = keep["n"].data_ptr() + 4
    _code(p, run, capi.FA_ERR_BAD_STRIDE, "kv_new")
    run = L.fa_run_mla_cache_gather
    _bad(_gather_params, run, capi.FA_ERR_NULL_POINTER, "out", out=None)
    _bad(_gather_params, run, capi.FA_ERR_BAD_STRIDE, "out", out_row_stride=580)
    _bad(_gather_params, run, capi.FA_ERR_BAD_STRIDE, "out", out_row_stride=512)
    _bad(_gather_params, run, capi.FA_ERR_BAD_STRIDE, "out", out_batch_stride=5 * 576 + 4)
    p, keep = _gather_params()
    p.seq_starts = keep["st"].data_ptr() + 2
    _code(p, run, capi.FA_ERR_BAD_STRIDE, "seq_starts")
    run = L.fa_run_mla_index_cache_append
    _bad(_index_params, run, capi.FA_ERR_BAD_DTYPE, "k_format", k_format=2)
    _bad(_index_params, run, capi.FA_ERR_BAD_DTYPE, "scale_format", scale_format=2)
    _bad(_index_params, run, capi.FA_ERR_NULL_POINTER, "cache_seqlens", cache_seqlens=None)
    _bad(_index_params, run, capi.FA_ERR_NULL_POINTER, "k_idx_cache", k_idx_cache=None)
    _bad(_index_params, run, capi.FA_ERR_NULL_POINTER, "k_scale", k_scale=None)
    _bad(_index_params, run, capi.FA_ERR_NULL_POINTER, "k_idx_new", k_idx_new=None)
    _bad(_index_params, run, capi.FA_ERR_BAD_SHAPE, "k_scale", k_format=0)                           # scales with a 16-bit cache
    _bad(_index_params, run, capi.FA_ERR_BAD_STRIDE, "k_cache_row_stride", k_cache_row_stride=136)
    _bad(_index_params, run, capi.FA_ERR_BAD_STRIDE, "k_cache_row_stride", k_cache_row_stride=64)
    _bad(_index_params, run, capi.FA_ERR_BAD_STRIDE, "k_cache_batch_stride", k_cache_batch_stride=32 * 128 + 8)
    _bad(_index_params, run, capi.FA_ERR_BAD_STRIDE, "k_cache_row_stride", (False, False, False), k_cache_row_stride=132)
    _bad(_index_params, run, capi.FA_ERR_BAD_STRIDE, "k_idx_new", k_new_row_stride=132)
    p, keep = _index_params()
    p.k_scale = keep["sc"].data_ptr() + 2
    _code(p, run, capi.FA_ERR_BAD_STRIDE, "k_scale")


# ---- 4. the quantiser ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_quantiser_equals_the_independent_model_and_one_latent_tile(dtname):
    rows = C.index_key_rows(dtname)
    assert rows.shape[0] >= 512 + 40 and torch.equal(rows[:512].view(torch.int16).flatten().int() & 0xFFFF, torch.arange(65536, dtype=torch.int32))
    amax = torch.where(torch.isfinite(rows.float()), rows.float().abs(), z(())).amax(-1)
    top = 65504.0 if dtname == "fp16" else float(torch.tensor([0x7F7F], dtype=torch.int16).view(torch.bfloat16).float())
    assert amax.max() == top and ((amax > 0) & (amax < 2.0 ** -24)).any() == (dtname == "bf16") and (amax == 0).any()
    got = {}
    for fmt in ("fp32", "ue8m0"):
        codes, scale = F.quantize_mla_index_keys(rows, fmt)
        assert codes.dtype == torch.uint8 and codes.shape == rows.shape and scale.dtype == torch.float32 and scale.shape == rows.shape[:1]
        want_c, want_s = C.np_quantize_index_keys(C.u16(rows), dtname, fmt)
        assert np.array_equal(scale.numpy().view(np.uint32), want_s.view(np.uint32)), fmt
        bad = np.argwhere(codes.numpy() != want_c)
        assert bad.size == 0, (fmt, bad[:5], codes.numpy()[tuple(bad[0])], want_c[tuple(bad[0])])
        got[fmt] = (codes, scale)
    # one 128-column tile of the latent cache's quantiser: the same rule
    lat = torch.zeros(rows.shape[0], 576, dtype=rows.dtype)
    lat[:, 128:256] = rows
    q = F.quantize_mla_kv_cache(lat)
    assert torch.equal(q[:, 128:256], got["fp32"][0]) and torch.equal(q[:, 516:520].contiguous().view(torch.float32).flatten(), got["fp32"][1])
    # UE8M0: a power of two, at least the fp32 scale and below twice it
    s32, s8 = got["fp32"][1], got["ue8m0"][1]
    assert ((s8.view(torch.int32) & 0x007FFFFF) == 0).all() and (s8 >= s32).all() and (s8 < 2 * s32).all()
    assert (s8 != s32).any() and (s8 == s32).any()
    # leading dimensions are kept
    c3, s3 = F.quantize_mla_index_keys(rows[:12].view(3, 4, 128), "ue8m0")
    assert torch.equal(c3.view(12, 128), got["ue8m0"][0][:12]) and torch.equal(s3.view(12), s8[:12])


def test_placement_model():
    """the integer model the GPU tests place rows with, on the cases they use"""
    lens, news = zip(*C.APPEND_CASES)
    assert {x for l in lens for x in l} == set(C.LENS) and {x for n in news for x in n} == set(C.NEWS)
    kept = C.placed_rows((95, 96, -3, 15), (20, 5, 3, 1))
    assert kept == [(0, 0, 95), (2, 0, 0), (2, 1, 1), (2, 2, 2), (3, 0, 15)]
    assert any(len(C.placed_rows(l, n)) < sum(n) for l, n in C.APPEND_CASES)                      # something is dropped
    assert any(p // 16 != (max(l[i], 0)) // 16 for l, n in C.APPEND_CASES for i, s, p in C.placed_rows(l, n))      # an append crosses a page
    _, starts, counts = zip(*C.GATHER_CASES)
    assert {x for s in starts for x in s} == set(C.STARTS) and {x for c in counts for x in c} == set(C.COUNTS)
    g = C.gathered_rows((17, -3), (16, -2), (3, 2))
    assert g == [(0, 0, 16), (0, 1, None), (0, 2, None), (1, 0, None), (1, 1, None)]
    assert C.gathered_rows(None, None, (2,), cap=1) == [(0, 0, 0), (0, 1, None)]
    table = [[-1, 2 ** 31 - 1, 3]]
    assert [C.physical(table, 0, p, 16, 6) for p in (5, 20, 40)] == [(5, 5), (5, 4), (3, 8)]
    assert C.cu_of((3, 0, 5)).tolist() == [0, 3, 3, 8]


# ---- 5. build wiring -------------------------------------------------------------------------------------------------------------------------------

def test_build_lists_the_new_source():
    spec = importlib.util.spec_from_file_location("fa_build_io", os.path.join(ROOT, "flash-attention-turing_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "fa_mla_cache_io.hip" in b.HIP_SOURCES and b.HIP_SOURCES.index("fa_mla_cache_io.hip") < b.HIP_SOURCES.index("fa_capi.hip")
    assert "fa_mla_cache_io.hip" in b.M0_GUARD_SOURCES and "fa_mla_cache_io.hpp" in b.HIP_HEADERS
    assert os.path.exists(os.path.join(b.CSRC, "fa_mla_cache_io.hip")) and os.path.exists(os.path.join(b.CSRC, "fa_mla_cache_io.hpp"))
    assert "fa_mla_cache_io.hip" not in b.EXTRA_FLAGS and all("fa_mla_cache_io.hip" not in v for v in b.DEBUG_VARIANTS.values())
