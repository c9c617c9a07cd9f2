"""CPU: the paged KV cache of the C ABI (fa_kvcache_params.block_table / block_table_stride / page_block_size / num_blocks) - struct layout
against the header, the old-size compatibility, host validation codes from all three entry points, the split rule against a contiguous
cache of the same capacity - and the ISA of the paged attention and append kernels.  No GPU involved."""
import ctypes
import os
import subprocess

import pytest

from flash_attn_turing import capi

ENTRY_POINTS = ["fa_run_mha_fwd_kvcache", "fa_kvcache_workspace_bytes", "fa_kvcache_num_splits"]


def _aligned_addr(n=256):
    buf = (ctypes.c_char * (n + 16))()
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


def _params(b=1, sq=1, cache=32768, h=32, hk=8, d=128, num_splits=0, sn=0, ws_bytes=None, page=None, num_blocks=None, bt_stride=None):
    """fa_kvcache_params over dummy 16-byte aligned addresses (no launch).  page=P: a paged cache of capacity `cache`, a pool of
    num_blocks (default b * cache / P) pages with page stride P * hk * d and a table of cache / P columns"""
    buf, addr = _aligned_addr()
    p = capi.KvcacheParams()
    p.q = p.k_cache = p.v_cache = p.o = p.lse = addr
    p.cache_seqlens = addr
    if sn:
        p.k_new = p.v_new = addr
        p.seqlen_new = sn
        p.k_new_stride = p.v_new_stride = capi.Strides(sn * hk * d, hk * d, d)
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.h_k, p.d = b, sq, cache, h, hk, d
    p.dtype, p.num_splits = 0, num_splits
    p.q_stride = p.o_stride = capi.Strides(sq * h * d, h * d, d)
    p.k_cache_stride = p.v_cache_stride = capi.Strides(cache * hk * d, hk * d, d)
    if page is not None:
        p.block_table = addr
        p.page_block_size = page
        cols = cache // page if page > 0 else 1
        p.num_blocks = b * cols if num_blocks is None else num_blocks
        p.block_table_stride = cols if bt_stride is None else bt_stride
        p.k_cache_stride = p.v_cache_stride = capi.Strides(max(page, 1) * hk * d, hk * d, d)
    if ws_bytes is not None:
        p.workspace, p.workspace_bytes = addr, ws_bytes
    p._keep = buf
    return p


def _rc(p, fn):
    f = getattr(capi.lib(), fn)
    return f(ctypes.byref(p), None) if fn == "fa_run_mha_fwd_kvcache" else f(ctypes.byref(p))


def test_paged_fields_layout_matches_header(tmp_path):
    """the four appended fields sit where a C compiler puts them, after workspace_bytes; the struct grows by exactly them"""
    new = ["block_table", "block_table_stride", "page_block_size", "num_blocks"]
    names = [f[0] for f in capi.KvcacheParams._fields_]
    assert names[-4:] == new and names[-5] == "workspace_bytes"
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\nint main(void) {\n'
                   '    printf("size %zu\\n", sizeof(fa_kvcache_params));\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_params, {f}), sizeof(((fa_kvcache_params*)0)->{f}));\n'
                             for f in new + ["workspace_bytes"])
                   + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"][0] == ctypes.sizeof(capi.KvcacheParams)
    for f in new:
        assert got[f][0] == getattr(capi.KvcacheParams, f).offset, f
        assert got[f][1] == getattr(capi.KvcacheParams, f).size, f
    assert got["block_table"][0] == got["workspace_bytes"][0] + 8
    assert got["size"][0] == got["num_blocks"][0] + 4


def test_pre_paging_struct_size_runs_the_contiguous_path(tmp_path):
    """a plain-C caller built before the paged fields (struct_size = offsetof(block_table)) is accepted, and whatever lies in memory after its
    struct is not looked at: the contiguous validation and split rule apply"""
    src = tmp_path / "old_caller.c"
    src.write_text(r"""
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
static char buf[4096] __attribute__((aligned(16)));
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = buf; p.lse = (float*)buf; p.cache_seqlens = (const int32_t*)buf;
    p.b = 1; p.seqlen_q = 1; p.seqlen_cache = 32768; p.h = 32; p.h_k = 8; p.d = 128; p.dtype = FA_FP16;
    p.q_stride = p.o_stride = (fa_strides){32 * 128, 32 * 128, 128};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 128, 8 * 128, 128};
    int64_t want = fa_kvcache_workspace_bytes(&p);
    if (want <= 0) return 10;
    /* what an old caller's stack may hold past its struct: garbage where the new fields are */
    p.block_table = (const int32_t*)buf + 1; p.block_table_stride = -5; p.page_block_size = 7; p.num_blocks = -1;
    if (fa_kvcache_workspace_bytes(&p) != FA_ERR_BAD_SHAPE) return 11;       /* the full-size struct sees them */
    p.struct_size = (uint32_t)offsetof(fa_kvcache_params, block_table);
    if (fa_kvcache_workspace_bytes(&p) != want) return 12;
    if (fa_kvcache_num_splits(&p) != 1) return 13;                          /* no workspace: one split, as before */
    p.h = 3; p.h_k = 2;
    if (fa_run_mha_fwd_kvcache(&p, NULL) != FA_ERR_BAD_GQA) return 14;
    p.h = 32; p.h_k = 8;
    p.k_cache_stride.row = 8 * 128 + 4;                                      /* the contiguous stride checks, over seqlen_cache rows */
    if (fa_kvcache_workspace_bytes(&p) != FA_ERR_BAD_STRIDE) return 15;
    p.struct_size = (uint32_t)offsetof(fa_kvcache_params, block_table) - 8;  /* shorter than the pre-paging struct: an error */
    if (fa_kvcache_workspace_bytes(&p) != FA_ERR_BAD_ABI) return 16;
    p.struct_size = (uint32_t)sizeof(fa_kvcache_params) + 8;
    if (fa_kvcache_workspace_bytes(&p) != FA_ERR_BAD_ABI) return 17;
    return 0;
}
""")
    exe = tmp_path / "old_caller"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    assert capi.lib().fa_abi_version() == 4


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_paged_validation_codes(fn):
    """every paged-cache rejection, with its own message, from all three entry points"""
    for P in (16, 48, 64, 256):
        assert _rc(_params(page=P, cache=768), fn) >= 0, (P, capi.last_error())
    cases = [
        (dict(page=0), capi.FA_ERR_BAD_SHAPE, "block_table given without page_block_size"),
        (dict(page=8, cache=64), capi.FA_ERR_BAD_SHAPE, "page_block_size 8 must be a positive multiple of 16"),
        (dict(page=40, cache=80), capi.FA_ERR_BAD_SHAPE, "page_block_size 40 must be a positive multiple of 16"),
        (dict(page=-16, cache=64), capi.FA_ERR_BAD_SHAPE, "page_block_size -16 must be a positive multiple of 16"),
        (dict(page=16, num_blocks=0), capi.FA_ERR_BAD_SHAPE, "num_blocks"),
        (dict(page=16, num_blocks=-3), capi.FA_ERR_BAD_SHAPE, "num_blocks"),
        (dict(page=64, cache=1000), capi.FA_ERR_BAD_SHAPE, "seqlen_cache (1000) must be a positive multiple of page_block_size (64)"),
        (dict(page=64, cache=0, num_blocks=4), capi.FA_ERR_BAD_SHAPE, "positive multiple of page_block_size"),
        (dict(page=64, cache=4096, bt_stride=63), capi.FA_ERR_BAD_STRIDE, "block_table_stride 63"),
        (dict(page=64, cache=128, sn=129), capi.FA_ERR_BAD_SHAPE, "seqlen_new (129) exceeds"),
    ]
    for kw, code, text in cases:
        p = _params(**kw)
        assert _rc(p, fn) == code, (kw, capi.last_error())
        assert text in capi.last_error(), (kw, capi.last_error())
    # page_block_size without block_table
    p = _params()
    p.page_block_size = 16
    assert _rc(p, fn) == capi.FA_ERR_NULL_POINTER and "page_block_size = 16 given without block_table" in capi.last_error()
    # a misaligned table
    p = _params(page=16)
    p.block_table = p.block_table + 2
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "block_table must be 4-byte aligned" in capi.last_error()
    # a wider table row than the capacity needs is fine
    assert _rc(_params(page=64, cache=4096, bt_stride=1000), fn) >= 0
    # the pool checks apply per page: a page stride (batch) that is not a multiple of 8, a row stride below head_dim
    p = _params(page=64)
    p.k_cache_stride = capi.Strides(64 * 8 * 128 + 4, 8 * 128, 128)
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "k_cache" in capi.last_error()
    p = _params(page=64)
    p.v_cache_stride = capi.Strides(64 * 8 * 128, 64, 128)
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "v_cache" in capi.last_error()


@pytest.mark.parametrize("fn", ENTRY_POINTS)
def test_paged_byte_limit_is_per_page(fn):
    """the 2^31-byte limit of one descriptor applies to a page (rows = page_block_size), not to the capacity or the pool"""
    # 2^20 rows x 1024-element rows x 2 bytes = 2^31 bytes of capacity: rejected contiguous, fine paged (one page of 256 rows is 512 KiB)
    big = 1 << 20
    p = _params(cache=big, hk=8, d=128)
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "limit 2^31" in capi.last_error()
    p = _params(cache=big, hk=8, d=128, page=256, num_blocks=1 << 22)
    assert _rc(p, fn) >= 0, capi.last_error()
    # a page stride above 2^31 elements is fine (page offsets are 64-bit); a page that spans 2^31 bytes is not
    p = _params(page=256, cache=4096)
    p.k_cache_stride = capi.Strides(3 << 30, 8 * 128, 128)
    assert _rc(p, fn) >= 0, capi.last_error()
    p = _params(page=256, cache=4096)
    p.v_cache_stride = capi.Strides(1 << 32, 1 << 22, 128)
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "v_cache" in capi.last_error() and "limit 2^31" in capi.last_error()


def test_split_and_workspace_match_contiguous_capacity():
    """the split and its workspace follow the capacity: a paged cache gives what a contiguous one of the same seqlen_cache gives"""
    for b, h, hk, cache, P in ((1, 32, 8, 32768, 16), (1, 32, 8, 32768, 256), (3, 16, 4, 768, 48), (2, 32, 1, 131072, 64), (64, 32, 8, 4096, 64),
                               (1, 8, 8, 16, 16)):
        for kw in (dict(), dict(num_splits=3), dict(num_splits=1), dict(num_splits=500)):
            c = _params(b=b, h=h, hk=hk, cache=cache, **kw)
            g = _params(b=b, h=h, hk=hk, cache=cache, page=P, **kw)
            assert capi.kvcache_workspace_bytes(g) == capi.kvcache_workspace_bytes(c), (b, h, hk, cache, P, kw)
            for ws in (1 << 40, 0, 16, 3 * b * h * 128 * 4 + (3 * b * h * 4 + 15) // 16 * 16):
                cw = _params(b=b, h=h, hk=hk, cache=cache, ws_bytes=ws, **kw)
                gw = _params(b=b, h=h, hk=hk, cache=cache, page=P, ws_bytes=ws, **kw)
                assert capi.kvcache_num_splits(gw) == capi.kvcache_num_splits(cw), (b, h, hk, cache, P, kw, ws)
    # a capped workspace caps both alike
    rows = 32
    small = 3 * rows * 128 * 4 + (3 * rows * 4 + 15) // 16 * 16
    assert capi.kvcache_num_splits(_params(page=64, ws_bytes=small)) == 3
    assert capi.kvcache_num_splits(_params(page=64, ws_bytes=small - 1)) == 2
    assert capi.kvcache_num_splits(_params(page=64, num_splits=16, ws_bytes=small)) == 3


def test_paged_kernels_isa_clean():
    """the paged attention and append kernels: no scratch, no spills or accumulator moves in the MFMA loops, no MFMA hazards, M0 untouched
    by hipcc's code, two workgroups per CU; the contiguous kernels keep their count of 8"""
    from _kernel_isa import analyse

    ks = analyse("fa_fwd_kvcache.hip")
    assert len([n for n in ks if "fa_fwd_kvcache_kernel" in n]) == 8
    attn = {n: k for n, k in ks.items() if "fa_fwd_kvcache_paged_kernel" in n}
    append = {n: k for n, k in ks.items() if "fa_kvcache_append_paged_kernel" in n}
    assert len(attn) == 8                                   # fp16 / bf16 x d64 / d128 x causal / not
    assert len(append) == 2                                 # d64 / d128
    for n, k in {**attn, **append}.items():
        assert k.get("scratch_bytes") == 0, (n, k.get("scratch_bytes"))
        assert k["mfma_hazards"] == [], (n, k["mfma_hazards"][:3])
        assert k["m0_outside_asm"] == 0, n
        assert k["occupancy"] >= 2, n
    for n, k in attn.items():
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
