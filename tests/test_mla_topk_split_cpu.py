"""CPU: the split top-k selection without a GPU: the symbols and FA_HAS_MLA_TOPK_SPLIT, the layout of fa_mla_topk_params_v2, every refusal through the C ABI and
through Python, and what the host-only queries answer."""
import ctypes
import os
import subprocess

import pytest
import torch

import flash_attn_turing as F
from flash_attn_turing import capi

V2_TAIL = ["workspace", "workspace_bytes", "num_splits", "reserved2_"]


def _v2(b=2, sq=2, cap=4160, topk=32, **kw):
    keep = (torch.zeros(b, sq, cap), torch.zeros(b, sq, topk, dtype=torch.int32), torch.zeros(b, dtype=torch.int32), torch.zeros(1 << 16))
    return capi.mla_topk_params_v2(keep[0], keep[1], keep[2], causal=True, **kw), keep


def test_symbols_macro_and_struct_layout(tmp_path):
    names = capi.declared_functions()
    for n in ("fa_run_mla_indexer_topk_v2", "fa_mla_topk_workspace_bytes", "fa_mla_topk_num_splits"):
        assert n in names and hasattr(capi.lib(), n)
    fields = [f[0] for f in capi.MlaTopkParamsV2._fields_]
    assert fields == [f[0] for f in capi.MlaTopkParams._fields_] + V2_TAIL
    src = tmp_path / "topk_v2_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_TOPK_SPLIT\n#error "no FA_HAS_MLA_TOPK_SPLIT"\n#endif\n'
                   "int main(void) {\n" + "".join(f'    printf("%zu\\n", offsetof(fa_mla_topk_params_v2, {f}));\n' for f in fields) +
                   '    printf("%zu %zu %d %d\\n", sizeof(fa_mla_topk_params_v2), sizeof(fa_mla_topk_params), FA_ABI_VERSION, FA_HAS_MLA_TOPK_SPLIT);\n    return 0;\n}\n')
    exe = tmp_path / "topk_v2_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    *offsets, last = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert [int(x) for x in offsets] == [getattr(capi.MlaTopkParamsV2, f).offset for f in fields]
    assert [int(x) for x in last.split()] == [ctypes.sizeof(capi.MlaTopkParamsV2), ctypes.sizeof(capi.MlaTopkParams), capi.lib().fa_abi_version(), 1] == [96, 72, 4, 1]


def test_c_abi_refusals_name_the_field():
    L = capi.lib()
    entries = (lambda p: L.fa_run_mla_indexer_topk_v2(p, None), L.fa_mla_topk_num_splits, L.fa_mla_topk_workspace_bytes)

    def bad(code, word, fns=entries, make=None, **change):
        for fn in fns:
            p, keep = _v2(**(make or {}))
            for k, v in change.items():
                setattr(p, k, v)
            rc = fn(ctypes.byref(p))
            assert rc == code and word in capi.last_error(), (rc, capi.last_error(), word)

    bad(capi.FA_ERR_BAD_SHAPE, "num_splits", num_splits=-1)
    bad(capi.FA_ERR_BAD_SHAPE, "reserved2_", reserved2_=1)
    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=80)
    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=104)
    p, keep = _v2(num_splits=7)
    need = capi.mla_topk_workspace_bytes(p)
    assert need == 2 * 2 * 4 * (4096 + 1024 + 1024 + 7 * 1040)
    ws = torch.zeros(need // 4 + 4)
    for size, want in ((need, 7), (need - 1, capi.FA_ERR_BAD_SHAPE)):
        p.workspace, p.workspace_bytes = ws.data_ptr(), size
        assert L.fa_mla_topk_num_splits(ctypes.byref(p)) == want        # the forced count fits; one byte short it does not
    assert L.fa_run_mla_indexer_topk_v2(ctypes.byref(p), None) == capi.FA_ERR_BAD_SHAPE and "workspace_bytes" in capi.last_error()
    p, keep = _v2()
    rc = L.fa_run_mla_indexer_topk(ctypes.cast(ctypes.pointer(p), ctypes.POINTER(capi.MlaTopkParams)), None)
    assert rc == capi.FA_ERR_BAD_ABI and "struct_size 96" in capi.last_error(), (rc, capi.last_error())


def test_num_splits_query():
    ws = torch.zeros(1 << 22)

    def splits(num_splits, workspace=ws, **shape):
        p, keep = _v2(num_splits=num_splits, workspace=workspace, **shape)
        return capi.mla_topk_num_splits(p)

    for n in (0, 1, 9):
        assert splits(n, cap=2048, topk=2048) == 1          # seqlen_cache <= topk
        assert splits(n, workspace=None, b=1, sq=1, cap=131072, topk=2048) == 1
    assert splits(0, b=64, sq=64, cap=32768, topk=2048) == 1       # many rows: one workgroup per row fills the chip
    assert splits(0, b=1, sq=1, cap=4096, topk=2048) == 1          # a short row
    assert splits(9, b=1, sq=1, cap=131072, topk=2048) == 9 and splits(1, b=1, sq=1, cap=131072, topk=2048) == 1
    for cap in (33, 100, 4160, 131072):         # never more chunks than 64-entry blocks of the capacity
        for n in (0, 2, 64, 1000):
            assert 1 <= splits(n, b=1, sq=1, cap=cap, topk=32) <= (cap + 63) // 64
    p, keep = _v2(b=1, sq=1, cap=131072, topk=2048)
    p.struct_size = ctypes.sizeof(capi.MlaTopkParams)
    assert capi.mla_topk_num_splits(p) == 1 and capi.mla_topk_workspace_bytes(p) == 0


def test_python_refusals_name_the_argument():
    a = dict(q_idx=torch.zeros(2, 2, 64, 128, dtype=torch.bfloat16), weights=torch.zeros(2, 2, 64), k_idx_cache=torch.zeros(2, 64, 128, dtype=torch.uint8),
             cache_seqlens=torch.zeros(2, dtype=torch.int32))
    for badv in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match="num_splits"):
            F.flash_mla_indexer_topk(torch.zeros(2, 2, 64), a["cache_seqlens"], 32, num_splits=badv)
        for fn in (F.flash_mla_index_with_kvcache, F.flash_mla_index_prefill_with_kvcache):
            with pytest.raises(ValueError, match="topk_splits"):
                fn(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], 32, topk_splits=badv)
