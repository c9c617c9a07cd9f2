"""CPU: the sliding window of the KV-cache decode path (fa_kvcache_options and the _ex entry points of the C ABI) - struct layout against the
header, the exports, validation codes from Python and from plain C, the split and workspace rule with a window - and the ISA of the new
_local attention kernels.  No GPU involved."""
import ctypes
import os
import subprocess

import pytest

from flash_attn_turing import capi

EX_ENTRY_POINTS = ["fa_run_mha_fwd_kvcache_ex", "fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"]


def _aligned_addr(n=256):
    buf = (ctypes.c_char * (n + 16))()
    addr = ctypes.addressof(buf)
    return buf, addr + (-addr) % 16


def _params(b=1, sq=1, cache=32768, h=32, hk=8, d=128, causal=False, num_splits=0, ws_bytes=None, page=None):
    """fa_kvcache_params over dummy 16-byte aligned addresses (no launch); page=P: a paged cache of capacity `cache`"""
    buf, addr = _aligned_addr()
    p = capi.KvcacheParams()
    p.q = p.k_cache = p.v_cache = p.o = p.lse = addr
    p.cache_seqlens = addr
    p.b, p.seqlen_q, p.seqlen_cache, p.h, p.h_k, p.d = b, sq, cache, h, hk, d
    p.dtype, p.is_causal, p.num_splits = 0, int(causal), num_splits
    p.q_stride = p.o_stride = capi.Strides(sq * h * d, h * d, d)
    p.k_cache_stride = p.v_cache_stride = capi.Strides(cache * hk * d, hk * d, d)
    if page is not None:
        p.block_table, p.page_block_size = addr, page
        p.num_blocks = b * (cache // page)
        p.block_table_stride = cache // page
        p.k_cache_stride = p.v_cache_stride = capi.Strides(page * hk * d, hk * d, d)
    if ws_bytes is not None:
        p.workspace, p.workspace_bytes = addr, ws_bytes
    p._keep = buf
    return p


def _win(left, right):
    return capi.kvcache_options((left, right))


def _rc(p, fn, opt):
    f = getattr(capi.lib(), fn)
    o = None if opt is None else ctypes.byref(opt)
    return f(ctypes.byref(p), o, None) if fn == "fa_run_mha_fwd_kvcache_ex" else f(ctypes.byref(p), o)


def test_options_layout_matches_header(tmp_path):
    """ctypes offsets and size of fa_kvcache_options agree with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheOptions._fields_]
    assert fields == ["struct_size", "magic", "is_local", "window_size_left", "window_size_right"]
    src = tmp_path / "opt_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\nint main(void) {\n'
                   '    printf("size %zu\\n", sizeof(fa_kvcache_options));\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options, {f}), sizeof(((fa_kvcache_options*)0)->{f}));\n' for f in fields)
                   + "    return 0;\n}\n")
    exe = tmp_path / "opt_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"][0] == ctypes.sizeof(capi.KvcacheOptions) == 20
    for f in fields:
        assert got[f][0] == getattr(capi.KvcacheOptions, f).offset, f
        assert got[f][1] == getattr(capi.KvcacheOptions, f).size, f


def test_ex_symbols_declared_and_exported():
    declared = capi.declared_functions()
    L = capi.lib()
    for n in EX_ENTRY_POINTS:
        assert n in declared, n
        assert hasattr(L, n), n
    assert L.fa_abi_version() == 4
    # a zeroed options struct is "no window"
    o = capi.kvcache_options()
    assert (o.struct_size, o.magic, o.is_local) == (20, capi.FA_PARAMS_MAGIC, 0)


@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_options_validation_codes(fn):
    """a bad options header is FA_ERR_BAD_ABI, a window side of -2 FA_ERR_BAD_SHAPE (from every _ex entry point, before any launch);
    NULL options and a zeroed struct behave like the plain entry point"""
    plain = getattr(capi.lib(), fn[:-3])
    for kw in (dict(), dict(ws_bytes=1 << 40), dict(page=64), dict(causal=True, sq=4)):
        p = _params(**kw)
        if fn == "fa_run_mha_fwd_kvcache_ex":
            p.b = 0                                     # (the addresses are dummies: b = 0 is validated and launches nothing)
            want = plain(ctypes.byref(p), None)
        else:
            want = plain(ctypes.byref(p))
        assert _rc(p, fn, None) == want, kw
        assert _rc(p, fn, capi.KvcacheOptions()) == want, kw
        o = capi.KvcacheOptions()
        o.window_size_left = o.window_size_right = -7     # not read without is_local
        assert _rc(p, fn, o) == want, kw
    for bad in ((-2, 0), (0, -2), (-2, -1), (-(2**31), 5)):
        p = _params()
        assert _rc(p, fn, _win(*bad)) == capi.FA_ERR_BAD_SHAPE, bad
        assert "window_size" in capi.last_error()
    o = _win(4095, 0)
    o.magic = 0
    assert _rc(_params(), fn, o) == capi.FA_ERR_BAD_ABI and "fa_kvcache_options" in capi.last_error()
    for size in (8, 16, 28):
        o = _win(4095, 0)
        o.struct_size = size
        assert _rc(_params(), fn, o) == capi.FA_ERR_BAD_ABI, size
    # params are validated as before, with or without options
    p = _params(h=3, hk=2)
    assert _rc(p, fn, _win(128, 0)) == capi.FA_ERR_BAD_GQA
    for ok in ((0, 0), (-1, 0), (0, -1), (5, 7), (4095, 0), (1 << 30, 1 << 30)):
        p = _params(ws_bytes=1 << 40)
        if fn == "fa_run_mha_fwd_kvcache_ex":
            p.b = 0
        assert _rc(p, fn, _win(*ok)) >= 0, (ok, capi.last_error())


def test_plain_c_caller(tmp_path):
    """the options struct and _ex calls as a plain-C caller uses them (FA_PARAMS_INIT, validation before any launch)"""
    src = tmp_path / "use_window.c"
    src.write_text(r"""
#include <stdio.h>
#include "flash_attn_gfx950.h"
static char buf[4096] __attribute__((aligned(16)));
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = buf; p.lse = (float*)buf; p.cache_seqlens = (const int32_t*)buf;
    p.b = 1; p.seqlen_q = 1; p.seqlen_cache = 131072; p.h = 32; p.h_k = 8; p.d = 128; p.dtype = FA_FP16; p.is_causal = 1;
    p.q_stride = p.o_stride = (fa_strides){32 * 128, 32 * 128, 128};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){8 * 128, 8 * 128, 128};   /* (batch stride unused at b = 1) */
    fa_kvcache_options o;
    FA_PARAMS_INIT(o);
    if (o.struct_size != sizeof(fa_kvcache_options) || o.is_local != 0) return 10;
    int64_t plain = fa_kvcache_workspace_bytes(&p);
    if (plain <= 0) return 11;
    if (fa_kvcache_workspace_bytes_ex(&p, NULL) != plain) return 12;
    if (fa_kvcache_workspace_bytes_ex(&p, &o) != plain) return 13;            /* zeroed: no window */
    o.is_local = 1; o.window_size_left = 4095; o.window_size_right = 0;
    int64_t win = fa_kvcache_workspace_bytes_ex(&p, &o);
    if (win <= 0 || win > plain) return 14;
    o.window_size_left = -2;
    if (fa_kvcache_num_splits_ex(&p, &o) != FA_ERR_BAD_SHAPE) return 15;
    if (fa_run_mha_fwd_kvcache_ex(&p, &o, NULL) != FA_ERR_BAD_SHAPE) return 16;
    o.window_size_left = 4095; o.magic = 0;
    if (fa_run_mha_fwd_kvcache_ex(&p, &o, NULL) != FA_ERR_BAD_ABI) return 17;
    o.magic = FA_PARAMS_MAGIC; o.struct_size = 12;
    if (fa_kvcache_workspace_bytes_ex(&p, &o) != FA_ERR_BAD_ABI) return 18;
    o.struct_size = sizeof(o);
    p.b = 0;
    if (fa_run_mha_fwd_kvcache_ex(&p, &o, NULL) != FA_OK) return 19;          /* nothing to do: no launch */
    if (fa_abi_version() != 4) return 20;
    printf("%lld %lld\n", (long long)plain, (long long)win);
    return 0;
}
""")
    exe = tmp_path / "use_window"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def _ns(p, opt=None):
    return capi.kvcache_num_splits(p, opt)


def _wsb(p, opt=None):
    return capi.kvcache_workspace_bytes(p, opt)


def test_unbounded_windows_are_the_plain_call():
    """(-1, -1), left >= seqlen_cache - 1 (right unbounded or causal) and right >= seqlen_q - 1 give exactly the plain split and workspace"""
    for b, sq, h, hk, cache, causal in ((1, 1, 32, 8, 131072, True), (1, 4, 32, 8, 32768, False), (3, 16, 16, 4, 768, True), (2, 33, 32, 1, 4096, False),
                                        (64, 1, 32, 8, 4096, False)):
        for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
            for page in (None, 256):
                for ws in (None, 1 << 40, 0, 3 * b * h * sq * 128 * 4 + (3 * b * h * sq * 4 + 15) // 16 * 16):
                    p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, page=page, ws_bytes=ws, **kw)
                    want_ws, want_ns = _wsb(p), _ns(p)
                    unbounded = [(-1, -1), (cache, -1), (cache - 1, -1), (1 << 30, sq - 1), (-1, sq - 1), (-1, 1 << 30), (cache + 5, sq + 3)]
                    if causal:
                        unbounded += [(cache, 0), (-1, 0), (cache, 17), (-1, 5)]
                    for win in unbounded:
                        assert _wsb(p, _win(*win)) == want_ws, (b, sq, cache, causal, page, ws, kw, win)
                        assert _ns(p, _win(*win)) == want_ns, (b, sq, cache, causal, page, ws, kw, win)


def test_windowed_split_never_above_plain():
    """a window's split and workspace never exceed those of the same call without it, over shapes, forced splits and workspace limits"""
    shapes = [(1, 1, 32, 8, 131072), (1, 4, 32, 8, 32768), (8, 1, 32, 32, 32768), (2, 33, 32, 1, 4096), (1, 16, 16, 4, 768), (3, 2, 8, 8, 100),
              (1, 255, 32, 8, 65536), (256, 1, 8, 8, 4096)]
    wins = [(0, 0), (1, 0), (31, 0), (32, 0), (33, 0), (4095, 0), (127, 3), (-1, 0), (0, -1), (1000, 1000), (65535, 0), (7, -1)]
    for b, sq, h, hk, cache in shapes:
        for causal in (False, True):
            for kw in (dict(), dict(num_splits=2), dict(num_splits=128), dict(num_splits=100000)):
                rows = b * h * sq
                for ws in (None, 1 << 40, 0, 2 * rows * 128 * 4 + (2 * rows * 4 + 15) // 16 * 16, 7 * rows * 128 * 4 + (7 * rows * 4 + 15) // 16 * 16):
                    p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, ws_bytes=ws, **kw)
                    ns, wsb = _ns(p), _wsb(p)
                    for win in wins:
                        o = _win(*win)
                        assert _ns(p, o) <= ns, (b, sq, h, hk, cache, causal, kw, ws, win)
                        assert _wsb(p, o) <= wsb, (b, sq, h, hk, cache, causal, kw, ws, win)
                        assert _ns(p, o) >= 1


def test_window_split_follows_the_span():
    """b1 h32 h_k8 sq1 over a 131072 capacity with window (4095, 0) gets the split of a capacity near the window's span (4096 keys plus
    the base's alignment), not that of 131072; a forced num_splits is capped by the window's 32-key steps"""
    big = _params(b=1, sq=1, h=32, hk=8, cache=131072, causal=True, ws_bytes=1 << 40)
    near = _params(b=1, sq=1, h=32, hk=8, cache=4096 + 32, causal=True, ws_bytes=1 << 40)
    plain_small = _params(b=1, sq=1, h=32, hk=8, cache=4096, causal=True, ws_bytes=1 << 40)
    o = _win(4095, 0)
    assert _ns(big, o) == _ns(near) == _ns(plain_small)
    assert _ns(big, o) < _ns(big)
    assert _wsb(big, o) == _wsb(near)
    # the span is left + seqlen_q + max(right, 0) (+ 31 for the alignment of the base) in 32-key steps; a right side >= seqlen_q - 1
    # cannot bind and counts as unbounded
    for left, right, sq in ((4095, 0, 1), (4095, 0, 16), (100, 50, 4), (100, 2, 4), (0, 0, 1), (31, -1, 2), (1000, 3, 33)):
        r = -1 if right >= sq - 1 else right
        steps = -(-min(131072, left + sq + max(r, 0) + 31) // 32)
        p = _params(b=1, sq=sq, h=32, hk=8, cache=131072, num_splits=100000, ws_bytes=1 << 40)
        assert _ns(p, _win(left, right)) == min(steps, 100000), (left, right, sq)
        p = _params(b=1, sq=sq, h=32, hk=8, cache=131072, num_splits=3, ws_bytes=1 << 40)
        assert _ns(p, _win(left, right)) == min(3, steps), (left, right, sq)
    # a window with no left edge reads from key 0: the capacity's split
    p = _params(b=1, sq=4, h=32, hk=8, cache=131072, ws_bytes=1 << 40)
    assert _ns(p, _win(-1, 0)) == _ns(p)
    # a one-step window: one split
    assert _ns(_params(b=1, sq=1, h=32, hk=8, cache=131072, num_splits=16, ws_bytes=1 << 40), _win(0, 0)) == 1
    # paged: the same rule
    pg = _params(b=1, sq=1, h=32, hk=8, cache=131072, causal=True, ws_bytes=1 << 40, page=256)
    assert _ns(pg, o) == _ns(big, o) and _wsb(pg, o) == _wsb(big, o)


def test_python_window_validation():
    """flash_attn_with_kvcache rejects a window_size that is not a pair of ints >= -1 before anything reaches the device"""
    import torch

    import flash_attn_turing as F

    q = torch.zeros(1, 1, 8, 64, dtype=torch.float16)
    kc = torch.zeros(1, 64, 8, 64, dtype=torch.float16)
    for bad in ((-2, 0), (0, -2), (1, 2, 3), (1,), 5, "ab", (1.5, 0), (True, 0), (0, None), None, (2**31, 0)):
        with pytest.raises(ValueError, match="window_size"):
            F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=1, window_size=bad)


def test_local_kernels_isa_clean():
    """the 8 _local attention kernels (fp16 / bf16 x d64 / d128 x contiguous / paged): no scratch, no spills or accumulator moves in the MFMA
    loops, no MFMA hazards, M0 untouched by hipcc's code, two workgroups per CU; the plain kernels keep their counts of 8 / 8 / 2"""
    from _kernel_isa import analyse

    ks = analyse("fa_fwd_kvcache.hip")
    assert len([n for n in ks if "fa_fwd_kvcache_kernel" in n]) == 8
    assert len([n for n in ks if "fa_fwd_kvcache_paged_kernel" in n]) == 8
    assert len([n for n in ks if "fa_kvcache_append_paged_kernel" in n]) == 2
    local = {n: k for n, k in ks.items() if "fa_fwd_kvcache_local_kernel" in n}
    assert len(local) == 8
    for n, k in local.items():
        assert k.get("scratch_bytes") == 0, (n, k.get("scratch_bytes"))
        assert k["mfma_hazards"] == [], (n, k["mfma_hazards"][:3])
        assert k["m0_outside_asm"] == 0, n
        assert k["occupancy"] >= 2, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
