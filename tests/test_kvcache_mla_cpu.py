"""CPU: MLA decode over a latent KV cache (flash_mla_with_kvcache, fa_mla_params / fa_run_mla_fwd_kvcache of the C ABI) - the Python surface and
its refusals, the struct against the header, the host-only helpers, the error codes with the argument they name, the exports, and the
resources of the kernels of fa_fwd_kvcache_mla.hip.  No GPU involved."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi

S, HD, DT, NUL, STR, ABI = capi.FA_ERR_BAD_SHAPE, capi.FA_ERR_BAD_HEADDIM, capi.FA_ERR_BAD_DTYPE, capi.FA_ERR_NULL_POINTER, capi.FA_ERR_BAD_STRIDE, capi.FA_ERR_BAD_ABI
MLA_WAVES_PER_SIMD = 1          # the occupancy that is shipped: one workgroup of four waves per compute unit


# ---- 1. the Python surface ----------------------------------------------------------------------------------------------------------------

def test_surface_and_refusals_before_any_device_work():
    import flash_attn_turing as F

    assert "flash_mla_with_kvcache" in F.__all__ and F.flash_mla_with_kvcache is F.interface.flash_mla_with_kvcache
    sig = inspect.signature(F.flash_mla_with_kvcache)
    names = list(sig.parameters)
    assert names[:3] == ["q", "kv_cache", "cache_seqlens"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[3:])
    assert set(names[3:]) == {"head_dim_v", "kv_new", "block_table", "softmax_scale", "causal", "num_splits", "return_softmax_lse"}
    assert sig.parameters["head_dim_v"].default == 512
    for gone in ("window_size", "softcap", "sinks", "tree_mask", "rotary_cos", "cu_seqlens_q", "k_descale"):
        assert gone not in names

    b, sq, h, cap = 2, 2, 16, 64
    q = torch.zeros(b, sq, h, 576, dtype=torch.bfloat16)
    kv = torch.zeros(b, cap, 1, 576, dtype=torch.bfloat16)
    call = F.flash_mla_with_kvcache
    with pytest.raises(TypeError):
        call(q, kv, 8, 512)
    with pytest.raises(ValueError, match="q must be 576 wide"):
        call(torch.zeros(b, sq, h, 512, dtype=torch.bfloat16), kv, 8)
    with pytest.raises(ValueError, match="kv_cache must have exactly one head"):
        call(q, torch.zeros(b, cap, 2, 576, dtype=torch.bfloat16), 8)
    with pytest.raises(ValueError, match="head_dim_v must be 512"):
        call(q, kv, 8, head_dim_v=256)
    for other in (torch.float16, torch.float32, torch.float8_e4m3fn):
        with pytest.raises(ValueError, match="kv_cache must have q's dtype"):
            call(q, torch.zeros(b, cap, 1, 576, dtype=torch.float32).to(other), 8)
    pool = torch.zeros(8, 16, 1, 576, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="block_table must be an int32 tensor"):
        call(q, pool, 8, block_table=torch.zeros(b, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="page_block_size"):
        call(q, torch.zeros(8, 24, 1, 576, dtype=torch.bfloat16), 8, block_table=torch.zeros(b, 4, dtype=torch.int32))
    for bad in (0, 0.0, float("nan"), float("inf"), -1.0, True, False, "1"):
        with pytest.raises(ValueError, match="softmax_scale"):
            call(q, kv, 8, softmax_scale=bad)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(ValueError, match="causal must be a bool"):
            call(q, kv, 8, causal=bad)
    with pytest.raises(ValueError, match="kv_new"):
        call(q, kv, 8, kv_new=torch.zeros(b, 1, 2, 576, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="cache_seqlens"):
        call(q, kv, torch.zeros(b, dtype=torch.int64))
    with pytest.raises(ValueError, match="num_splits"):
        call(q, kv, 8, num_splits=-1)
    # a CPU call that passes the checks is refused by the extension (no quiet fall-back)
    kn = torch.zeros(b, sq, 1, 576, dtype=torch.bfloat16)
    for kw in (dict(), dict(causal=True), dict(num_splits=3, softmax_scale=192 ** -0.5), dict(kv_new=kn), dict(return_softmax_lse=True),
               dict(block_table=torch.zeros(b, 4, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="GPU"):
            call(q, pool if "block_table" in kw else kv, 8, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q.half(), kv.half(), torch.full((b,), 8, dtype=torch.int32))
    from flash_attn_turing import _C
    with pytest.raises(RuntimeError, match="GPU"):
        _C.fwd_mla_kvcache(q, kv)
    doc = call.__doc__
    assert "576" in doc and "512" in doc and "Out of scope" in doc


# ---- 2. the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_mla_params_layout_matches_header(tmp_path):
    fields = [f[0] for f in capi.MlaParams._fields_]
    src = tmp_path / "mla_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_KVCACHE\n#error "no FA_HAS_MLA_KVCACHE"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu 0\\n", sizeof(fa_mla_params));\n'
                   '    printf("abi %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_KVCACHE);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_mla_params, {f}), sizeof(((fa_mla_params*)0)->{f}));\n' for f in fields)
                   + "    fa_mla_params p;\n    FA_PARAMS_INIT(p);\n"
                     "    return p.struct_size == sizeof(p) && p.magic == FA_PARAMS_MAGIC && p.kv_new == NULL && p.softmax_scale == 0.0f && p.reserved_ == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "mla_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"][0] == ctypes.sizeof(capi.MlaParams) == 240
    assert got["abi"] == [4, 1] and capi.lib().fa_abi_version() == 4
    for f in fields:
        assert got[f] == [getattr(capi.MlaParams, f).offset, getattr(capi.MlaParams, f).size], f


def test_plain_c_caller(tmp_path):
    """sizeof, the workspace of a forced split (n_split x rows x 512 x 4 + n_split x rows x 4), one split without a workspace, codes with the
    argument in fa_last_error, b = 0"""
    src = tmp_path / "use_mla.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
#ifndef FA_HAS_MLA_KVCACHE
#error "no FA_HAS_MLA_KVCACHE"
#endif
static _Alignas(16) char mem[256];
static void fill(fa_mla_params* p) {
    FA_PARAMS_INIT(*p);
    p->q = p->kv_cache = p->o = mem; p->lse = (float*)mem; p->cache_seqlens = (const int32_t*)mem;
    p->b = 8; p->seqlen_q = 2; p->seqlen_cache = 32768; p->h = 128; p->d_qk = 576; p->d_v = 512; p->dtype = FA_BF16; p->num_splits = 4; p->is_causal = 1;
    p->q_stride = (fa_strides){2 * 128 * 576, 128 * 576, 576};
    p->o_stride = (fa_strides){2 * 128 * 512, 128 * 512, 512};
    p->kv_cache_stride = (fa_strides){32768LL * 576, 576, 576};
}
#define CODE(field_change, code, word, ret) do { fa_mla_params t; fill(&t); field_change; \
    if (fa_mla_workspace_bytes(&t) != (code) || !strstr(fa_last_error(), word)) { fprintf(stderr, "%s\n", fa_last_error()); return ret; } \
    if (fa_run_mla_fwd_kvcache(&t, NULL) != (code) || fa_mla_num_splits(&t) != (code)) return ret; } while (0)
int main(void) {
    fa_mla_params p;
    fill(&p);
    if (sizeof(p) != 240) return 9;
    const long long rows = 8LL * 128 * 2;
    if (fa_mla_workspace_bytes(&p) != 4 * rows * 512 * 4 + 4 * rows * 4) return 10;
    if (fa_mla_num_splits(&p) != 1) return 11;                 /* no workspace in the params */
    p.workspace = mem; p.workspace_bytes = 1LL << 40;
    if (fa_mla_num_splits(&p) != 4) return 12;
    p.num_splits = 1;
    if (fa_mla_workspace_bytes(&p) != 0) return 13;
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
    CODE((t.kv_new = mem, t.seqlen_new = 1, t.kv_new_stride = (fa_strides){576, 576, 576}, t.cache_seqlens = NULL), FA_ERR_NULL_POINTER, "cache_seqlens", 30);
    CODE(t.seqlen_new = 2, FA_ERR_BAD_SHAPE, "kv_new", 31);
    CODE(t.q = NULL, FA_ERR_NULL_POINTER, "q is NULL", 32);
    CODE(t.kv_cache = NULL, FA_ERR_NULL_POINTER, "kv_cache", 33);
    CODE(t.kv_cache_stride.row = 580, FA_ERR_BAD_STRIDE, "kv_cache", 34);
    CODE(t.o_stride.row = 500, FA_ERR_BAD_STRIDE, "o strides", 35);
    CODE(t.kv_cache_stride.row = 1 << 20, FA_ERR_BAD_STRIDE, "kv_cache", 36);   /* one sequence spans 2^31 bytes or more */
    CODE(t.reserved_ = 1, FA_ERR_BAD_ABI, "reserved_", 37);
    CODE(t.struct_size = 232, FA_ERR_BAD_ABI, "struct_size", 38);
    CODE(t.magic = 0, FA_ERR_BAD_ABI, "magic", 39);
    fill(&p);
    p.b = 0; p.q = p.kv_cache = p.o = NULL; p.lse = NULL;
    if (fa_run_mla_fwd_kvcache(&p, NULL) != FA_OK) return 40;    /* nothing to do: no launch */
    if (fa_mla_workspace_bytes(&p) != 0 || fa_mla_num_splits(&p) != 1) return 41;
    if (fa_abi_version() != 4) return 42;
    return 0;
}
""")
    exe = tmp_path / "use_mla"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_exports_and_the_automatic_split():
    names = capi.declared_functions()
    L = capi.lib()
    for n in ("fa_run_mla_fwd_kvcache", "fa_mla_workspace_bytes", "fa_mla_num_splits"):
        assert n in names and hasattr(L, n), n
    # the automatic split: the rule of the decode call over b x ceil(sq * h / 64) workgroups (256 compute units without a device), at least 8
    # steps a split, at most 128 splits
    q = torch.zeros(1, 1, 128, 576, dtype=torch.bfloat16)
    o = torch.zeros(1, 1, 128, 512, dtype=torch.bfloat16)
    lse = torch.zeros(1, 128, 1)

    def splits(cap, b=1, h=128):
        kv = torch.zeros(1, 16, 1, 576, dtype=torch.bfloat16)
        p = capi.mla_params(q, kv, o, lse)
        p.b, p.h, p.seqlen_cache = b, h, cap
        p.kv_cache_stride = capi.Strides(cap * 576, 576, 576)
        n = capi.mla_workspace_bytes(p) // (b * h * (512 * 4 + 4)) if capi.mla_workspace_bytes(p) else 1
        return n

    assert splits(131072) == 128              # 2 tiles: ceil(512 / 2) = 256 wanted, capped at 128
    assert splits(4096) == 16                 # 128 steps / 8 steps per split
    assert splits(131072, h=16) == 128
    assert splits(32768, b=64) == 4           # 128 workgroups: ceil(512 / 128)
    assert splits(32768, b=128) == 1          # one workgroup per compute unit: no split
    assert splits(16) == 1


# ---- 3. ISA -----------------------------------------------------------------------------------------------------------------------------------

def test_mla_kernels_isa():
    """8 attention kernels ({fp16, bf16} x {plain, causal} x {contiguous, paged}), 2 appends, 2 combines.  Every attention kernel: no scratch, an
    MFMA loop free of scratch traffic and accumulator moves that reads K as rows and V^T transposed from the SAME LDS images behind a barrier,
    72 KB of LDS (<= 80 KB), subnormals kept, no MFMA result read early, M0 untouched, and the occupancy DESIGN.md states: one wave per SIMD
    (one workgroup per compute unit; built for two the kernels spill)."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_kvcache_mla.hip" in B.HIP_SOURCES and "fa_fwd_kvcache_mla.hip" in B.M0_GUARD_SOURCES
    ks = analyse("fa_fwd_kvcache_mla.hip")
    attn = {n: k for n, k in ks.items() if "fa_fwd_kvcache_mla_kernel" in n}
    assert len(attn) == 8 and len(ks) == 12, sorted(ks)
    assert sum("fa_kvcache_mla_append_kernel" in n for n in ks) == 2 and sum("fa_kvcache_combine_kernelI" in n and "Li512E" in n for n in ks) == 2
    keys = set()
    for n, k in attn.items():
        m = re.search(r"fa_fwd_kvcache_mla_kernelI(DF16_|DF16b)Lb(\d)ELb(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
        assert k["lds_bytes"] == 2 * (32 * 1024 + 32 * 128) <= 80 * 1024, (n, k["lds_bytes"])
        assert k["occupancy"] == MLA_WAVES_PER_SIMD and k["vgprs"] <= 256 and k["vgprs"] + k["agprs"] <= 512, (n, k["occupancy"], k["vgprs"], k["agprs"])
        assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        assert main["ds_read_b128"] > 0 and main["ds_read_tr"] > 0 and main["barriers"] > 0, (n, main["label"])
    assert keys == {(t, c, p) for t in ("DF16_", "DF16b") for c in "01" for p in "01"}
    for n, k in ks.items():
        if n not in attn:
            assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0, n
