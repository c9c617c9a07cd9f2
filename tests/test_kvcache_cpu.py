"""CPU: the KV-cache decode entry points of the C ABI (fa_run_mha_fwd_kvcache, fa_kvcache_workspace_bytes, fa_kvcache_num_splits) - struct
layout against the header, host validation codes, the split rule - and the ISA of the new kernels.  No GPU involved."""
import ctypes
import os
import subprocess

import pytest

from flash_attn_turing import capi


def _aligned_addr(n=256):
    buf = (ctypes.c_char * (n + 16))()
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


def _params(b=1, sq=1, cache=32768, h=32, hk=8, d=128, causal=False, num_splits=0, sn=0, ws_bytes=None):
    """fa_kvcache_params over dummy 16-byte aligned addresses with contiguous strides: enough for the host-side entry points (no launch)"""
    buf, addr = _aligned_addr()
    p = capi.KvcacheParams()
    p.q = p.k_cache = p.v_cache = p.o = p.lse = addr
    p.cache_seqlens = addr
    if sn:
        p.k_new = p.v_new = addr
        p.seqlen_new = sn
        p.k_new_stride = p.v_new_stride = capi.Strides(sn * hk * d, hk * d, d)
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.h_k, p.d = b, sq, cache, h, hk, d
    p.dtype, p.is_causal, p.num_splits = 0, int(causal), num_splits
    p.q_stride = p.o_stride = capi.Strides(sq * h * d, h * d, d)
    p.k_cache_stride = p.v_cache_stride = capi.Strides(cache * hk * d, hk * d, d)
    if ws_bytes is not None:
        p.workspace, p.workspace_bytes = addr, ws_bytes
    p._keep = buf
    return p


def _cus():
    import torch

    if torch.cuda.is_available():
        return torch.cuda.get_device_properties(0).multi_processor_count
    return 256


def test_struct_layout_matches_header(tmp_path):
    """ctypes offsets and size of fa_kvcache_params agree with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheParams._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\nint main(void) {\n'
                   '    printf("size %zu\\n", sizeof(fa_kvcache_params));\n'
                   + "".join(f'    printf("{f} %zu\\n", offsetof(fa_kvcache_params, {f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(capi.KvcacheParams)
    for f in fields:
        assert int(got[f]) == getattr(capi.KvcacheParams, f).offset, f
    assert capi.KvcacheParams.struct_size.offset == 0 and capi.KvcacheParams.magic.offset == 4
    p = capi.KvcacheParams()
    assert p.struct_size == ctypes.sizeof(capi.KvcacheParams) and p.magic == capi.FA_PARAMS_MAGIC


def test_exports_and_abi_version_unchanged():
    L = capi.lib()
    for n in ("fa_run_mha_fwd_kvcache", "fa_kvcache_workspace_bytes", "fa_kvcache_num_splits"):
        assert n in capi.declared_functions() and hasattr(L, n)
    assert L.fa_abi_version() == 4


def _rc(p, fn="fa_run_mha_fwd_kvcache"):
    f = getattr(capi.lib(), fn)
    return f(ctypes.byref(p), None) if fn == "fa_run_mha_fwd_kvcache" else f(ctypes.byref(p))


@pytest.mark.parametrize("fn", ["fa_run_mha_fwd_kvcache", "fa_kvcache_workspace_bytes", "fa_kvcache_num_splits"])
def test_validation_error_codes_without_gpu(fn):
    """every host-side rejection, before anything is launched; the same codes from all three entry points"""
    L = capi.lib()
    cases = [
        (dict(h=6, hk=4), capi.FA_ERR_BAD_GQA, "divisible"),
        (dict(d=96), capi.FA_ERR_BAD_HEADDIM, "head_dim"),
        (dict(sq=0), capi.FA_ERR_BAD_SHAPE, "seqlen_q"),
        (dict(cache=64, sn=65), capi.FA_ERR_BAD_SHAPE, "seqlen_new"),
        (dict(num_splits=-1), capi.FA_ERR_BAD_SHAPE, "num_splits"),
    ]
    for kw, code, text in cases:
        p = _params(**kw)
        assert _rc(p, fn) == code, (kw, capi.last_error())
        assert text in capi.last_error(), (kw, capi.last_error())
    p = _params()
    p.dtype = 7
    assert _rc(p, fn) == capi.FA_ERR_BAD_DTYPE and "dtype" in capi.last_error()
    # only one of k_new / v_new
    p = _params(sn=1)
    p.v_new = None
    assert _rc(p, fn) == capi.FA_ERR_NULL_POINTER and "both" in capi.last_error()
    # k_new without cache_seqlens
    p = _params(sn=1)
    p.cache_seqlens = None
    assert _rc(p, fn) == capi.FA_ERR_NULL_POINTER and "cache_seqlens" in capi.last_error()
    # null tensors
    for name in ("q", "k_cache", "v_cache", "o"):
        p = _params()
        setattr(p, name, None)
        assert _rc(p, fn) == capi.FA_ERR_NULL_POINTER and name in capi.last_error(), name
    p = _params()
    p.lse = None
    assert _rc(p, fn) == capi.FA_ERR_NULL_POINTER and "lse" in capi.last_error()
    # strides and alignment
    p = _params()
    p.k_cache_stride = capi.Strides(32768 * 8 * 128, 8 * 128 + 4, 128)
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "k_cache" in capi.last_error()
    p = _params()
    p.v_cache = p.v_cache + 8
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "v_cache" in capi.last_error()
    p = _params(sn=2)
    p.k_new_stride = capi.Strides(2 * 8 * 128, 100, 128)
    assert _rc(p, fn) == capi.FA_ERR_BAD_STRIDE and "k_new" in capi.last_error()
    # params header
    assert L.fa_run_mha_fwd_kvcache(None, None) == capi.FA_ERR_NULL_POINTER
    p = _params()
    p.magic = 0
    assert _rc(p, fn) == capi.FA_ERR_BAD_ABI
    p = _params()
    p.struct_size = ctypes.sizeof(capi.KvcacheParams) + 8
    assert _rc(p, fn) == capi.FA_ERR_BAD_ABI


def test_workspace_pointer_checked_by_the_launch_only():
    """an unaligned workspace is rejected by the launch and the split query; the size query ignores the workspace fields"""
    p = _params(ws_bytes=1 << 20)
    p.workspace = p.workspace + 4
    assert _rc(p) == capi.FA_ERR_BAD_STRIDE and "workspace" in capi.last_error()
    assert _rc(p, "fa_kvcache_num_splits") == capi.FA_ERR_BAD_STRIDE
    assert capi.kvcache_workspace_bytes(p) > 0
    p = _params(ws_bytes=-1)
    assert _rc(p) == capi.FA_ERR_BAD_SHAPE
    assert capi.kvcache_workspace_bytes(p) > 0


def test_c_program_links_and_gets_validation_codes(tmp_path):
    src = tmp_path / "use_kvcache.c"
    src.write_text(r"""
#include <stdio.h>
#include "flash_attn_gfx950.h"
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.b = 1; p.seqlen_q = 1; p.seqlen_cache = 64; p.h = 3; p.h_k = 2; p.d = 128; p.dtype = FA_FP16;
    if (fa_run_mha_fwd_kvcache(&p, NULL) != FA_ERR_BAD_GQA) return 11;
    p.h = 4;
    if (fa_kvcache_workspace_bytes(&p) != FA_ERR_NULL_POINTER) return 12;
    if (fa_abi_version() != 4) return 13;
    return 0;
}
""")
    exe = tmp_path / "use_kvcache"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def _splits(**kw):
    return capi.kvcache_num_splits(_params(ws_bytes=1 << 40, **kw))


def test_split_heuristic():
    cus = _cus()
    tiles = lambda cache: (cache + 31) // 32
    # a launch that fills the chip is not split: b x h_k x row tiles >= CUs
    assert _splits(b=cus, hk=1, h=1, cache=32768) == 1
    if 32 * 32 >= cus:
        assert _splits(b=32, h=32, hk=32, cache=32768) == 1              # MHA decode at b32: 1024 workgroups
    assert capi.kvcache_workspace_bytes(_params(b=cus, hk=1, h=1)) == 0
    # b1 h32 h_k8 L32k: 8 workgroups unsplit; the split brings the launch to at least one workgroup per CU
    n = _splits(b=1, h=32, hk=8, cache=32768)
    assert n > 1 and 8 * n >= cus
    # monotone in seqlen_cache, never more splits than 32-key tiles
    prev = 0
    for cache in (1, 31, 32, 33, 64, 255, 256, 257, 1000, 4096, 8191, 32768, 131072):
        n = _splits(b=1, h=32, hk=8, cache=cache)
        assert 1 <= n <= tiles(cache), (cache, n)
        assert n >= prev, (cache, n, prev)
        prev = n
    # an explicit request overrides the rule, capped by the tiles
    assert _splits(b=1, h=32, hk=8, cache=32768, num_splits=3) == 3
    assert _splits(b=64, h=32, hk=8, cache=32768, num_splits=7) == 7
    assert _splits(b=1, h=32, hk=8, cache=100, num_splits=50) == tiles(100)


def test_workspace_rule():
    p = _params(b=1, h=32, hk=8, cache=32768)
    n = capi.kvcache_num_splits(_params(b=1, h=32, hk=8, cache=32768, ws_bytes=1 << 40))
    rows = 1 * 32 * 1
    want = n * rows * 128 * 4 + (n * rows * 4 + 15) // 16 * 16
    assert capi.kvcache_workspace_bytes(p) == want
    # no workspace: one split
    assert capi.kvcache_num_splits(p) == 1
    # a smaller workspace caps the split
    small = 3 * rows * 128 * 4 + (3 * rows * 4 + 15) // 16 * 16
    assert capi.kvcache_num_splits(_params(b=1, h=32, hk=8, cache=32768, ws_bytes=small)) == 3
    assert capi.kvcache_num_splits(_params(b=1, h=32, hk=8, cache=32768, ws_bytes=small - 1)) == 2
    assert capi.kvcache_num_splits(_params(b=1, h=32, hk=8, cache=32768, ws_bytes=16)) == 1
    # ... a forced count as well
    assert capi.kvcache_num_splits(_params(b=1, h=32, hk=8, cache=32768, num_splits=16, ws_bytes=small)) == 3
    assert capi.kvcache_workspace_bytes(_params(b=1, h=32, hk=8, cache=32768, num_splits=1)) == 0


def test_kernel_isa_clean():
    """the split-KV, combine and append kernels: no scratch, no spills or accumulator shuffles in the MFMA loops, no MFMA result touched
    before it lands, and M0 (which the LDS-DMA kernels of this library leave unsaved) never used by hipcc's own code"""
    from _kernel_isa import analyse

    ks = analyse("fa_fwd_kvcache.hip")
    attn = {n: k for n, k in ks.items() if "fa_fwd_kvcache_kernel" in n}
    assert len(attn) == 8                                   # fp16 / bf16 x d64 / d128 x causal / not
    assert any("combine" in n for n in ks) and any("append" in n for n in ks)
    for n, k in ks.items():
        assert k.get("scratch_bytes") == 0, (n, k.get("scratch_bytes"))
        assert k["mfma_hazards"] == [], (n, k["mfma_hazards"][:3])
        assert k["m0_outside_asm"] == 0, n
    for n, k in attn.items():
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        assert k["occupancy"] >= 2, n
