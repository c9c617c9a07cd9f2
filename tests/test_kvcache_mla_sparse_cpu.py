"""CPU: sparse MLA decode over a latent KV cache (flash_mla_sparse_with_kvcache, fa_mla_sparse_params / fa_run_mla_sparse_fwd_kvcache of the C ABI) - the
Python surface and its refusals, the struct against the header, the host-only helpers, the error codes with the argument they name, the exports,
the automatic split over topk, and the resources of the kernels of fa_fwd_kvcache_mla_sparse.hip.  No GPU involved."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi


# ---- 1. the Python surface ----------------------------------------------------------------------------------------------------------------

def test_surface_and_refusals_before_any_device_work():
    import flash_attn_turing as F

    assert "flash_mla_sparse_with_kvcache" in F.__all__ and F.flash_mla_sparse_with_kvcache is F.interface.flash_mla_sparse_with_kvcache
    sig = inspect.signature(F.flash_mla_sparse_with_kvcache)
    names = list(sig.parameters)
    assert names[:4] == ["q", "kv_cache", "cache_seqlens", "indices"]
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:4])
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[4:])
    assert names[4:] == ["head_dim_v", "block_table", "softmax_scale", "num_splits", "return_softmax_lse"]
    defaults = {n: sig.parameters[n].default for n in names[4:]}
    assert defaults == dict(head_dim_v=512, block_table=None, softmax_scale=None, num_splits=0, return_softmax_lse=False)
    for gone in ("causal", "kv_new", "window_size", "softcap", "sinks", "tree_mask", "cu_seqlens_q", "k_descale"):
        assert gone not in names

    b, sq, h, cap, topk = 2, 2, 16, 64, 64
    q = torch.zeros(b, sq, h, 576, dtype=torch.bfloat16)
    kv = torch.zeros(b, cap, 1, 576, dtype=torch.bfloat16)
    idx = torch.zeros(b, sq, topk, dtype=torch.int32)
    call = F.flash_mla_sparse_with_kvcache
    with pytest.raises(TypeError):
        call(q, kv, 8, idx, 512)
    with pytest.raises(TypeError):
        call(q, kv, 8, idx, causal=True)
    # indices
    for bad in (idx.long(), idx.float(), idx.tolist(), None):
        with pytest.raises(ValueError, match="indices must be an int32 tensor"):
            call(q, kv, 8, bad)
    for bad in (idx[0], idx[:1], idx[:, :1], idx.unsqueeze(0), torch.zeros(b, sq + 1, topk, dtype=torch.int32)):
        with pytest.raises(ValueError, match="indices must have shape"):
            call(q, kv, 8, bad)
    for bad_k in (0, 1, 31, 33, 48, 100):
        with pytest.raises(ValueError, match="indices: topk must be a positive multiple of 32"):
            call(q, kv, 8, torch.zeros(b, sq, bad_k, dtype=torch.int32))
    with pytest.raises(ValueError, match="indices: the last dimension must be contiguous"):
        call(q, kv, 8, torch.zeros(b, sq, 2 * topk, dtype=torch.int32)[..., ::2])
    with pytest.raises(ValueError, match="indices must be on q's device"):
        call(q, kv, 8, idx.to("meta"))
    # everything flash_mla_with_kvcache refuses, in its words
    with pytest.raises(ValueError, match="q must be 576 wide"):
        call(torch.zeros(b, sq, h, 512, dtype=torch.bfloat16), kv, 8, idx)
    with pytest.raises(ValueError, match="q must be fp16 or bf16"):
        call(q.float(), kv.float(), 8, idx)
    with pytest.raises(ValueError, match="kv_cache must have exactly one head"):
        call(q, torch.zeros(b, cap, 2, 576, dtype=torch.bfloat16), 8, idx)
    with pytest.raises(ValueError, match="kv_cache must be 576 wide"):
        call(q, torch.zeros(b, cap, 1, 512, dtype=torch.bfloat16), 8, idx)
    with pytest.raises(ValueError, match="kv_cache batch"):
        call(q, torch.zeros(b + 1, cap, 1, 576, dtype=torch.bfloat16), 8, idx)
    with pytest.raises(ValueError, match="must be a rank-4 tensor"):
        call(q[0], kv, 8, idx)
    with pytest.raises(ValueError, match="head_dim_v must be 512"):
        call(q, kv, 8, idx, head_dim_v=256)
    for other in (torch.float16, torch.float32, torch.float8_e4m3fn):
        with pytest.raises(ValueError, match="kv_cache must have q's dtype"):
            call(q, torch.zeros(b, cap, 1, 576, dtype=torch.float32).to(other), 8, idx)
    pool = torch.zeros(8, 16, 1, 576, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="block_table must be an int32 tensor"):
        call(q, pool, 8, idx, block_table=torch.zeros(b, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="block_table must have shape"):
        call(q, pool, 8, idx, block_table=torch.zeros(b + 1, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="page_block_size"):
        call(q, torch.zeros(8, 24, 1, 576, dtype=torch.bfloat16), 8, idx, block_table=torch.zeros(b, 4, dtype=torch.int32))
    for bad in (0, 0.0, float("nan"), float("inf"), -1.0, True, False, "1"):
        with pytest.raises(ValueError, match="softmax_scale"):
            call(q, kv, 8, idx, softmax_scale=bad)
    for bad in (torch.zeros(b, dtype=torch.int64), torch.zeros(b + 1, dtype=torch.int32), None, True, 1.5):
        with pytest.raises(ValueError, match="cache_seqlens"):
            call(q, kv, bad, idx)
    for bad in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match="num_splits"):
            call(q, kv, 8, idx, num_splits=bad)
    with pytest.raises(RuntimeError, match="forward-only"):
        call(q.clone().requires_grad_(), kv, 8, idx)
    # a CPU call that passes the checks is refused by the extension (no quiet fall-back)
    wide = torch.zeros(b, sq + 2, topk + 32, dtype=torch.int32)
    for kw in (dict(), dict(num_splits=2, softmax_scale=192 ** -0.5), dict(return_softmax_lse=True), dict(block_table=torch.zeros(b, 4, dtype=torch.int32))):
        for ix in (idx, wide[:, 1:1 + sq, :topk]):
            with pytest.raises(RuntimeError, match="GPU"):
                call(q, pool if "block_table" in kw else kv, 8, ix, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q.half(), kv.half(), torch.full((b,), 8, dtype=torch.int32), idx)
    from flash_attn_turing import _C
    with pytest.raises(RuntimeError, match="GPU"):
        _C.fwd_mla_sparse_kvcache(q, kv, idx)
    doc = call.__doc__
    assert "576" in doc and "512" in doc and "topk" in doc and "Out of scope" in doc and "multiset" in doc


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_mla_sparse_params_layout_matches_header(tmp_path):
    fields = [f[0] for f in capi.MlaSparseParams._fields_]
    for f in ("indices", "indices_batch_stride", "indices_row_stride", "topk", "reserved_"):
        assert f in fields
    for f in ("kv_new", "kv_new_stride", "seqlen_new", "is_causal"):
        assert f not in fields
    assert set(f[0] for f in capi.MlaParams._fields_) - {"kv_new", "kv_new_stride", "seqlen_new", "is_causal"} == set(fields) - {"indices", "indices_batch_stride", "indices_row_stride", "topk"}
    src = tmp_path / "mla_sparse_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_SPARSE_KVCACHE\n#error "no FA_HAS_MLA_SPARSE_KVCACHE"\n#endif\n'
                   '#ifndef FA_HAS_MLA_KVCACHE\n#error "no FA_HAS_MLA_KVCACHE"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu\\n", sizeof(fa_mla_sparse_params), sizeof(fa_mla_params));\n'
                   '    printf("abi %d %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_KVCACHE, FA_HAS_MLA_SPARSE_KVCACHE);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_mla_sparse_params, {f}), sizeof(((fa_mla_sparse_params*)0)->{f}));\n' for f in fields)
                   + "    fa_mla_sparse_params p;\n    FA_PARAMS_INIT(p);\n"
                     "    return p.struct_size == sizeof(p) && p.magic == FA_PARAMS_MAGIC && p.indices == NULL && p.topk == 0 && p.softmax_scale == 0.0f && p.reserved_ == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "mla_sparse_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"] == [ctypes.sizeof(capi.MlaSparseParams), 240] and ctypes.sizeof(capi.MlaParams) == 240
    assert got["abi"] == [4, 1, 1] and capi.lib().fa_abi_version() == 4
    end = 0
    for f in fields:
        assert got[f] == [getattr(capi.MlaSparseParams, f).offset, getattr(capi.MlaSparseParams, f).size], f
        assert got[f][0] == end, f"{f}: padding in front of it"          # no implicit padding: every byte of the struct is a named field
        end = got[f][0] + got[f][1]
    assert end == got["size"][0]


def test_plain_c_caller(tmp_path):
    """sizeof, the workspace of a forced split (n_split x rows x 512 x 4 + align16(n_split x rows x 4)), one split without a workspace, codes with the
    argument in fa_last_error, b = 0, ABI 4"""
    src = tmp_path / "use_mla_sparse.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
#ifndef FA_HAS_MLA_SPARSE_KVCACHE
#error "no FA_HAS_MLA_SPARSE_KVCACHE"
#endif
static _Alignas(16) char mem[256];
static void fill(fa_mla_sparse_params* p) {
    FA_PARAMS_INIT(*p);
    p->q = p->kv_cache = p->o = mem; p->lse = (float*)mem; p->cache_seqlens = (const int32_t*)mem; p->indices = (const int32_t*)mem;
    p->b = 8; p->seqlen_q = 2; p->seqlen_cache = 32768; p->topk = 2048; p->h = 128; p->d_qk = 576; p->d_v = 512; p->dtype = FA_BF16; p->num_splits = 4;
    p->q_stride = (fa_strides){2 * 128 * 576, 128 * 576, 576};
    p->o_stride = (fa_strides){2 * 128 * 512, 128 * 512, 512};
    p->kv_cache_stride = (fa_strides){32768LL * 576, 576, 576};
    p->indices_batch_stride = 2 * 2048; p->indices_row_stride = 2048;
}
#define CODE(field_change, code, word, ret) do { fa_mla_sparse_params t; fill(&t); field_change; \
    if (fa_mla_sparse_workspace_bytes(&t) != (code) || !strstr(fa_last_error(), word)) { fprintf(stderr, "%s\n", fa_last_error()); return ret; } \
    if (fa_run_mla_sparse_fwd_kvcache(&t, NULL) != (code) || fa_mla_sparse_num_splits(&t) != (code)) return ret; } while (0)
int main(void) {
    fa_mla_sparse_params p;
    fill(&p);
    if (sizeof(fa_mla_params) != 240) return 9;
    const long long rows = 8LL * 128 * 2;
    if (fa_mla_sparse_workspace_bytes(&p) != 4 * rows * 512 * 4 + 4 * rows * 4) return 10;
    if (fa_mla_sparse_num_splits(&p) != 1) return 11;                 /* no workspace in the params */
    p.workspace = mem; p.workspace_bytes = 1LL << 40;
    if (fa_mla_sparse_num_splits(&p) != 4) return 12;
    p.num_splits = 1;
    if (fa_mla_sparse_workspace_bytes(&p) != 0) return 13;
    p.num_splits = 3; p.b = 1; p.seqlen_q = 1; p.h = 1;              /* 3 rows of LSE: 12 bytes, aligned to 16 */
    if (fa_mla_sparse_workspace_bytes(&p) != 3 * 512 * 4 + 16) return 14;
    p.num_splits = 1000; p.topk = 96;                                 /* never more splits than 32-slot steps */
    if (fa_mla_sparse_num_splits(&p) != 3) return 15;
    CODE(t.d_qk = 512, FA_ERR_BAD_HEADDIM, "d_qk", 20);
    CODE(t.d_v = 256, FA_ERR_BAD_HEADDIM, "d_v", 21);
    CODE(t.dtype = 2, FA_ERR_BAD_DTYPE, "dtype", 22);
    CODE(t.seqlen_q = 0, FA_ERR_BAD_SHAPE, "seqlen_q", 23);
    CODE(t.h = 0, FA_ERR_BAD_SHAPE, "h=", 24);
    CODE(t.num_splits = -1, FA_ERR_BAD_SHAPE, "num_splits", 25);
    CODE(t.softmax_scale = -1.0f, FA_ERR_BAD_SHAPE, "softmax_scale", 26);
    CODE(t.softmax_scale = 0.0f / 0.0f, FA_ERR_BAD_SHAPE, "softmax_scale", 27);
    CODE((t.block_table = (const int32_t*)mem, t.page_block_size = 24, t.num_blocks = 4, t.block_table_stride = 4096), FA_ERR_BAD_SHAPE, "page_block_size", 28);
    CODE(t.page_block_size = 16, FA_ERR_NULL_POINTER, "block_table", 29);
    CODE(t.indices = NULL, FA_ERR_NULL_POINTER, "indices", 30);
    CODE(t.topk = 0, FA_ERR_BAD_SHAPE, "topk", 31);
    CODE(t.topk = 2047, FA_ERR_BAD_SHAPE, "topk", 43);
    CODE(t.topk = -32, FA_ERR_BAD_SHAPE, "topk", 44);
    CODE(t.indices_row_stride = -1, FA_ERR_BAD_STRIDE, "indices_row_stride", 45);
    CODE(t.q = NULL, FA_ERR_NULL_POINTER, "q is NULL", 32);
    CODE(t.kv_cache = NULL, FA_ERR_NULL_POINTER, "kv_cache", 33);
    CODE(t.kv_cache_stride.row = 580, FA_ERR_BAD_STRIDE, "kv_cache", 34);
    CODE(t.o_stride.row = 500, FA_ERR_BAD_STRIDE, "o strides", 35);
    CODE(t.kv_cache_stride.row = 1 << 20, FA_ERR_BAD_STRIDE, "kv_cache", 36);   /* one sequence spans 2^31 bytes or more */
    CODE(t.reserved_ = 1, FA_ERR_BAD_ABI, "reserved_", 37);
    CODE(t.struct_size -= 8, FA_ERR_BAD_ABI, "struct_size", 38);
    CODE(t.magic = 0, FA_ERR_BAD_ABI, "magic", 39);
    fill(&p);
    p.b = 0; p.q = p.kv_cache = p.o = NULL; p.lse = NULL; p.indices = NULL;
    if (fa_run_mla_sparse_fwd_kvcache(&p, NULL) != FA_OK) return 40;    /* nothing to do: no launch */
    if (fa_mla_sparse_workspace_bytes(&p) != 0 || fa_mla_sparse_num_splits(&p) != 1) return 41;
    if (fa_abi_version() != 4) return 42;
    return 0;
}
""")
    exe = tmp_path / "use_mla_sparse"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_exports_and_the_automatic_split_over_topk():
    names = capi.declared_functions()
    L = capi.lib()
    for n in ("fa_run_mla_sparse_fwd_kvcache", "fa_mla_sparse_workspace_bytes", "fa_mla_sparse_num_splits"):
        assert n in names and hasattr(L, n), n
    for n in ("MlaSparseParams", "mla_sparse_params", "mla_sparse_workspace_bytes", "mla_sparse_num_splits", "run_mla_sparse_fwd_kvcache"):
        assert hasattr(capi, n), n

    # the automatic split: the rule of the decode call with topk in the place of seqlen_cache over b x seqlen_q x ceil(h / 64) workgroups (256 compute
    # units without a device), at least 8 steps a split
    def splits(topk, b=1, h=128, sq=1, forced=0, cap=131072):
        q = torch.zeros(1, sq, h, 576, dtype=torch.bfloat16)
        o = torch.zeros(1, sq, h, 512, dtype=torch.bfloat16)
        lse = torch.zeros(1, h, sq)
        kv = torch.zeros(1, 16, 1, 576, dtype=torch.bfloat16)
        idx = torch.zeros(1, sq, topk, dtype=torch.int32)
        p = capi.mla_sparse_params(q, kv, o, lse, idx, num_splits=forced)
        p.b, p.seqlen_cache = b, cap
        p.kv_cache_stride = capi.Strides(cap * 576, 576, 576)
        ws = capi.mla_sparse_workspace_bytes(p)
        n = 1
        if ws:
            rows = b * h * sq
            n = ws // (rows * 512 * 4)
            assert ws == n * rows * 512 * 4 + (n * rows * 4 + 15) // 16 * 16
            p.workspace, p.workspace_bytes = 16, ws         # (host-only: the pointer is never followed)
            assert capi.mla_sparse_num_splits(p) == n
        return n

    assert splits(2048) == 8                    # 2 workgroups want 256; 64 steps / 8 steps per split
    assert splits(2048, cap=2048) == splits(2048, cap=1 << 20) == 8     # the capacity does not enter
    assert splits(2048, h=16) == 8
    assert splits(32) == 1                      # one step
    assert splits(224) == 1 and splits(256) == 1 and splits(512) == 2
    assert splits(2048, b=128) == 1             # a grid that already fills the chip: 256 workgroups
    assert splits(2048, b=64, sq=2) == 1        # ... counted per token: 64 x 2 x 2
    assert splits(2048, b=64, h=64, sq=2) == 4  # 128 workgroups: ceil(512 / 128)
    assert splits(2048, b=32) == 8              # 64 workgroups: ceil(512 / 64)
    for topk in (32, 96, 256, 2048):
        for forced in (1, 2, 3, 7, 64, 65, 1000):
            assert splits(topk, forced=forced) == min(forced, topk // 32), (topk, forced)


# ---- 3. ISA -----------------------------------------------------------------------------------------------------------------------------------

def test_mla_sparse_kernels_isa():
    """4 attention kernels ({fp16, bf16} x {contiguous, paged}) and 2 combines.  Every attention kernel: no scratch, an MFMA loop free of scratch
    traffic and accumulator moves that reads K as rows and V^T transposed from the same LDS images behind a barrier, 72 KB of LDS, subnormals kept,
    no MFMA result read early, M0 untouched, one wave per SIMD (one workgroup per compute unit).  The dense file keeps its 12 kernels."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    name = "fa_fwd_kvcache_mla_sparse.hip"
    assert name in B.HIP_SOURCES and name in B.M0_GUARD_SOURCES and B.EXTRA_FLAGS[name] == B.EXTRA_FLAGS["fa_fwd_kvcache_mla.hip"]
    ks = analyse(name)
    attn = {n: k for n, k in ks.items() if "fa_fwd_kvcache_mla_sparse_kernel" in n}
    assert len(attn) == 4 and len(ks) == 6, sorted(ks)
    assert sum("fa_kvcache_combine_kernelI" in n and "Li512E" in n for n in ks) == 2
    keys = set()
    for n, k in attn.items():
        m = re.search(r"fa_fwd_kvcache_mla_sparse_kernelI(DF16_|DF16b)Lb(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
        assert k["lds_bytes"] == 73728 == 2 * (32 * 1024 + 32 * 128), (n, k["lds_bytes"])
        assert k["occupancy"] == 1 and k["vgprs"] <= 256 and k["vgprs"] + k["agprs"] <= 512, (n, k["occupancy"], k["vgprs"], k["agprs"])
        assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        assert main["ds_read_b128"] > 0 and main["ds_read_tr"] > 0 and main["barriers"] > 0, (n, main["label"])
    assert keys == {(t, p) for t in ("DF16_", "DF16b") for p in "01"}
    for n, k in ks.items():
        if n not in attn:
            assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0, n
    assert len(analyse("fa_fwd_kvcache_mla.hip")) == 12
