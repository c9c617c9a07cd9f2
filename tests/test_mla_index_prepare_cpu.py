"""CPU: the indexer's front end without a GPU: the rotation's definition, exports, every refusal through Python and through the C ABI, the struct layout."""
import ctypes
import os
import subprocess

import pytest
import torch

import flash_attn_turing as F
from flash_attn_turing import capi

z = torch.zeros
BF, I32, U8 = torch.bfloat16, torch.int32, torch.uint8
HMAT = torch.tensor([[(-1.0) ** bin(c & d).count("1") for d in range(128)] for c in range(128)], dtype=torch.float64)


@pytest.mark.parametrize("dtype", [torch.float16, BF])
def test_rotation_is_the_sylvester_hadamard_matrix_times_two_to_the_minus_three_and_a_half(dtype):
    # H H = 128 I: rotating 16 e_d gives 16 * 128 ** -0.5 * H[d] (sqrt(2), rounded once), rotating H's rows gives 128 ** 0.5 e_d exactly where it is not zero
    s = (torch.tensor(16.0) * torch.tensor(128 ** -0.5, dtype=torch.float32)).to(dtype)
    assert torch.equal(F.rotate_mla_index_rows((16 * torch.eye(128)).to(dtype)), (HMAT.float() * s.float()).to(dtype))
    hh = F.rotate_mla_index_rows(HMAT.to(dtype)).double()
    assert torch.equal(hh != 0, torch.eye(128) != 0) and torch.equal(hh.diagonal(), torch.full((128,), float(torch.tensor(128 ** 0.5).to(dtype)), dtype=torch.float64))
    # random rows: the explicit +-1 product in fp64, one rounding to fp32, one fp32 product, one rounding to T
    x = torch.randn(3, 5, 128, generator=torch.Generator().manual_seed(1)).to(dtype)
    want = ((x.double() @ HMAT.T).float() * torch.tensor(128 ** -0.5, dtype=torch.float32)).to(dtype)
    assert torch.equal(F.rotate_mla_index_rows(x), want) and want.shape == x.shape and want.dtype == dtype


def _refuses(fn, word, *args, **kw):
    with pytest.raises(ValueError, match=word):
        fn(*args, **kw)


def test_exports_and_refusals_that_name_the_argument():
    for n in ("rotate_mla_index_rows", "flash_mla_index_prepare_queries", "flash_mla_index_prepare_append"):
        assert n in F.__all__ and getattr(F, n) is getattr(F.interface, n)
    q, w = z(2, 3, 16, 128, dtype=BF, device="meta"), z(2, 3, 16, device="meta")
    pq = F.flash_mla_index_prepare_queries
    m = lambda *shape, **kw: z(*shape, device="meta", **kw)
    for x in (z(4, 128), z(4, 64, dtype=BF), z(4, 256, dtype=BF)[:, ::2]):                          # fp32, width, last dimension strided
        _refuses(F.rotate_mla_index_rows, "x", x)
    for qq, ww in ((q.float(), w), (m(2, 16, 64, dtype=BF), m(2, 16)), (m(128, dtype=BF), m(())), (m(2, 16, 256, dtype=BF)[..., ::2], m(2, 16))):
        _refuses(pq, "q_idx", qq, ww)                                                               # dtype, width, no heads dimension, last dimension strided
    for ww in (m(2, 3, 8), w.double(), z(2, 3, 16)):                                                # shape, dtype, device
        _refuses(pq, "weights", q, ww)
    _refuses(pq, "hadamard", q, w, hadamard=1)
    _refuses(pq, "scale_format", q, w, scale_format="e8m0")
    a = dict(k_idx_cache=z(2, 32, 128, dtype=U8), k_idx_new=z(2, 3, 128, dtype=BF), cache_seqlens=z(2, dtype=I32), k_scale=z(2, 32))
    for word, change in (("rotated 16-bit rows are out of scope", dict(k_idx_cache=z(2, 32, 128, dtype=BF))), ("k_scale", dict(k_scale=None)), ("k_scale", dict(k_scale=z(2, 31))),
                         ("k_idx_new", dict(k_idx_new=z(2, 3, 128))), ("k_idx_new", dict(k_idx_new=z(2, 3, 64, dtype=BF))), ("k_idx_cache", dict(k_idx_cache=z(2, 32, 144, dtype=U8)[..., 8:136])),
                         ("scale_format", dict(scale_format="fp16")), ("cache_seqlens", dict(cache_seqlens=z(3, dtype=I32))), ("block_table", dict(block_table=z(2, 2)))):
        b = dict(a, **change)
        _refuses(F.flash_mla_index_prepare_append, word, b.pop("k_idx_cache"), b.pop("k_idx_new"), b.pop("cache_seqlens"), **b)
    assert F.flash_mla_index_prepare_append(a["k_idx_cache"], z(2, 0, 128, dtype=BF), 0, k_scale=a["k_scale"]) is None
    codes, w8 = pq(z(0, 16, 128, dtype=BF), z(0, 16))
    assert codes.shape == (0, 16, 128) and codes.dtype == U8 and w8.shape == (0, 16) and w8.dtype == torch.float32


FIELDS = ["struct_size", "magic", "q_idx", "weights", "codes", "w8", "k_idx_cache", "k_scale", "k_idx_new", "cache_seqlens", "cu_seqlens_new", "block_table", "dtype",
          "scale_format", "hadamard", "k_format", "heads", "b", "seqlen_new", "seqlen_cache", "page_block_size", "num_blocks", "tokens", "total_new", "reserved_",
          "q_token_stride", "q_head_stride", "w_token_stride", "w_head_stride", "k_cache_batch_stride", "k_cache_row_stride", "k_scale_batch_stride",
          "k_scale_row_stride", "k_new_batch_stride", "k_new_row_stride", "block_table_stride"]


def test_struct_layout_and_the_feature_macro(tmp_path):
    st, cls = "fa_mla_index_prepare_params", capi.MlaIndexPrepareParams
    assert [f[0] for f in cls._fields_] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#if FA_HAS_MLA_INDEX_PREPARE != 1 || FA_ABI_VERSION != 4\n#error "feature macro"\n#endif\n'
                   f'int main(void) {{\n    {st} x;\n    FA_PARAMS_INIT(x);\n    printf("%zu %d\\n", sizeof({st}), x.struct_size == sizeof(x) && x.hadamard == 0 && x.q_idx == NULL);\n'
                   + "".join(f'    printf("%zu %zu\\n", offsetof({st}, {f}), sizeof((({st}*)0)->{f}));\n' for f in FIELDS) + "    return 0;\n}\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(tmp_path / "layout")])
    got = [[int(v) for v in line.split()] for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert got[0] == [ctypes.sizeof(cls), 1] and got[0][0] == 240
    end = 0
    for f, (off, size) in zip(FIELDS, got[1:]):
        assert (off, size) == (getattr(cls, f).offset, getattr(cls, f).size) and off == end, f      # no padding anywhere
        end = off + size
    assert end == ctypes.sizeof(cls) and capi.lib().fa_abi_version() == 4
    for n in ("fa_run_mla_index_prepare_queries", "fa_run_mla_index_prepare_append"):
        assert n in capi.declared_functions() and hasattr(capi.lib(), n)


def _q_params():
    keep = dict(q=z(3, 16, 128, dtype=BF), w=z(3, 16), c=z(3, 16, 128, dtype=U8), o=z(3, 16))
    return capi.mla_index_prepare_queries_params(keep["q"], keep["w"], keep["c"], keep["o"]), keep


def _k_params(paged=False, packed=False):
    keep = dict(c=z(8 if paged else 2, 32, 128, dtype=U8), sc=z(8 if paged else 2, 32), n=z(6, 128, dtype=BF) if packed else z(2, 3, 128, dtype=BF), cs=z(2, dtype=I32),
                bt=z(2, 4, dtype=I32) if paged else None, cu=z(3, dtype=I32) if packed else None)
    return capi.mla_index_prepare_append_params(keep["c"], keep["n"], keep["cs"], keep["sc"], block_table=keep["bt"], cu_seqlens_new=keep["cu"]), keep


Q_BAD = [(capi.FA_ERR_BAD_ABI, "struct_size", dict(struct_size=232)), (capi.FA_ERR_BAD_ABI, "magic", dict(magic=0)), (capi.FA_ERR_BAD_DTYPE, "dtype", dict(dtype=2)),
         (capi.FA_ERR_BAD_DTYPE, "scale_format", dict(scale_format=2)), (capi.FA_ERR_BAD_SHAPE, "hadamard", dict(hadamard=2)), (capi.FA_ERR_BAD_SHAPE, "reserved_", dict(reserved_=1)),
         (capi.FA_ERR_BAD_SHAPE, "heads", dict(heads=0)), (capi.FA_ERR_BAD_SHAPE, "tokens", dict(tokens=-1)), (capi.FA_ERR_BAD_SHAPE, "call too large", dict(tokens=1 << 27)),
         (capi.FA_ERR_NULL_POINTER, "q_idx", dict(q_idx=None)), (capi.FA_ERR_BAD_STRIDE, "q_idx", dict(q_head_stride=132)), (capi.FA_ERR_BAD_STRIDE, "q_idx", dict(q_token_stride=2052)),
         (capi.FA_ERR_NULL_POINTER, "weights", dict(weights=None)), (capi.FA_ERR_NULL_POINTER, "w8", dict(w8=None)), (capi.FA_ERR_NULL_POINTER, "codes", dict(codes=None)),
         (capi.FA_OK, "", dict(tokens=0, q_idx=None))]                  # nothing to do: FA_OK without a launch, whatever the pointers
K_BAD = [(capi.FA_ERR_BAD_ABI, "struct_size", dict(struct_size=160)), (capi.FA_ERR_BAD_SHAPE, "hadamard", dict(hadamard=0)),
         (capi.FA_ERR_BAD_DTYPE, "rotated 16-bit rows are out of scope", dict(k_format=0)), (capi.FA_ERR_BAD_DTYPE, "scale_format", dict(scale_format=-1)),
         (capi.FA_ERR_BAD_SHAPE, "seqlen_new", dict(seqlen_new=-1)), (capi.FA_ERR_BAD_SHAPE, "reserved_", dict(reserved_=1)), (capi.FA_ERR_NULL_POINTER, "k_scale", dict(k_scale=None)),
         (capi.FA_ERR_NULL_POINTER, "cache_seqlens", dict(cache_seqlens=None)), (capi.FA_ERR_NULL_POINTER, "k_idx_new", dict(k_idx_new=None)),
         (capi.FA_ERR_BAD_STRIDE, "k_idx_cache", dict(k_cache_row_stride=136)), (capi.FA_ERR_BAD_STRIDE, "k_idx_new", dict(k_new_row_stride=132)),
         (capi.FA_ERR_NULL_POINTER, "page_block_size", dict(page_block_size=32)), (capi.FA_OK, "", dict(seqlen_new=0, k_idx_new=None)), (capi.FA_OK, "", dict(b=0, k_scale=None))]


@pytest.mark.parametrize("make,run,code,word,change", [(_q_params, "fa_run_mla_index_prepare_queries") + c for c in Q_BAD] + [(_k_params, "fa_run_mla_index_prepare_append") + c for c in K_BAD])
def test_c_abi_refusals_name_the_field(make, run, code, word, change):
    p, keep = make()                # (valid structs over host tensors: the library validates before it launches, and no case here reaches a launch)
    for k, v in change.items():
        setattr(p, k, v)
    rc = getattr(capi.lib(), run)(ctypes.byref(p), None)
    assert rc == code and word in capi.last_error(), (rc, capi.last_error())
