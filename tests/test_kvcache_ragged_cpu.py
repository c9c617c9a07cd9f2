"""CPU: ragged query batches on the decode path (cu_seqlens_q / max_seqlen_q / cu_seqlens_k_new of flash_attn_with_kvcache,
fa_kvcache_options_v4 of the C ABI) - the struct layout against the header, old callers, validation codes before any device work, the
workspace and split rules of a ragged call, the Python surface's validation, and the ISA of the new kernels.  No GPU involved."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi
from test_kvcache_window_cpu import EX_ENTRY_POINTS, _aligned_addr, _params, _rc

FP8 = capi.FA_CACHE_FP8_E4M3
ROWS = 16                                                # packed query rows of a tile (kKvcRows)


def _opt4(**kw):
    o = capi.KvcacheOptionsV4()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _rag(addr, total_q=64, **kw):
    base = dict(cu_seqlens_q=addr, total_q=total_q)
    base.update(kw)
    return _opt4(**base)


def _rag_params(fn, total_q=64, sn=0, **kw):
    """dummy params of a ragged call: packed q / o (batch stride 0), seqlen_q = max_seqlen_q; sn > 0: packed k_new / v_new; b = 0 for the
    launch (the addresses are dummies: b = 0 is validated and launches nothing)"""
    p = _params(**kw)
    p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
    if sn:
        buf, addr = _aligned_addr()
        p.k_new = p.v_new = addr
        p.seqlen_new = sn
        p.k_new_stride = p.v_new_stride = capi.Strides(0, p.h_k * p.d, p.d)
        p._keep2 = buf
    if fn == "fa_run_mha_fwd_kvcache_ex":
        p.b = 0
    return p


# ---- 1. layout --------------------------------------------------------------------------------------------------------------------------

def test_options_v4_layout_matches_header(tmp_path):
    """fa_kvcache_options (20 bytes), _v2 (72) and _v3 (112) keep their layouts; v4 repeats the v3 fields at the same offsets, appends the
    ragged fields and is 144 bytes; ctypes agrees with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheOptionsV4._fields_]
    v3 = [f[0] for f in capi.KvcacheOptionsV3._fields_]
    assert fields[:len(v3)] == v3
    assert fields[len(v3):] == ["cu_seqlens_q", "cu_seqlens_k_new", "total_q", "total_k_new"]
    src = tmp_path / "opt4_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_KVCACHE_RAGGED\n#error "no FA_HAS_KVCACHE_RAGGED"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu %zu %zu\\n", sizeof(fa_kvcache_options_v4), sizeof(fa_kvcache_options_v3), sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options));\n'
                   '    printf("abi %d 0\\n", FA_ABI_VERSION);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options_v4, {f}), sizeof(((fa_kvcache_options_v4*)0)->{f}));\n' for f in fields)
                   + "".join(f'    printf("v3_{f} %zu 0\\n", offsetof(fa_kvcache_options_v3, {f}));\n' for f in v3)
                   + "    fa_kvcache_options_v4 o;\n    FA_PARAMS_INIT(o);\n"
                     "    return o.struct_size == sizeof(o) && o.cu_seqlens_q == NULL && o.cu_seqlens_k_new == NULL && o.total_q == 0 && o.total_k_new == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "opt4_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    sizes = [ctypes.sizeof(c) for c in (capi.KvcacheOptionsV4, capi.KvcacheOptionsV3, capi.KvcacheOptionsV2, capi.KvcacheOptions)]
    assert got["size"] == sizes == [144, 112, 72, 20]
    assert got["abi"][0] == 4 == capi.lib().fa_abi_version()
    for f in fields:
        assert got[f] == [getattr(capi.KvcacheOptionsV4, f).offset, getattr(capi.KvcacheOptionsV4, f).size], f
    for f in v3:
        assert got["v3_" + f][0] == got[f][0], f
    # the sizes the older tests expect to be refused
    assert 144 not in (8, 12, 16, 24, 28, 40, 64, 71, 76, 80, 96, 104, 108, 111, 113, 116, 120, 128)


SHAPES = [(1, 1, 32, 8, 131072, True), (1, 4, 32, 8, 32768, False), (3, 16, 16, 4, 768, True), (2, 33, 32, 1, 4096, False), (64, 1, 32, 8, 4096, False),
          (8, 1, 32, 32, 32768, False), (3, 2, 8, 8, 100, False)]
WINDOWS = [(-1, -1), (0, 0), (31, 0), (4095, 0), (127, 3), (7, -1)]


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_v4_with_a_zeroed_tail_is_a_v3_call(fn):
    """same split and workspace from a v3 struct and a v4 struct whose ragged fields are zero (total_q / total_k_new are not read without
    cu_seqlens_q) - 16-bit and 8-bit cache, with and without a window"""
    f = getattr(capi.lib(), fn)
    for b, sq, h, hk, cache, causal in SHAPES:
        for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
            for ws in (None, 1 << 40, 3 * b * h * sq * 128 * 4 + (3 * b * h * sq * 4 + 15) // 16 * 16):
                p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, ws_bytes=ws, **kw)
                for win in WINDOWS:
                    for fp8 in (0, FP8):
                        v3, v4 = capi.KvcacheOptionsV3(), _opt4(total_q=77, total_k_new=5)
                        assert (v3.struct_size, v4.struct_size) == (112, 144)
                        for o in (v3, v4):
                            o.is_local, o.window_size_left, o.window_size_right, o.cache_dtype = int(win != (-1, -1)), win[0], win[1], fp8
                        want = f(ctypes.byref(p), ctypes.byref(v3))
                        assert want >= 0, capi.last_error()
                        assert f(ctypes.byref(p), ctypes.byref(v4)) == want, (b, sq, cache, ws, kw, win, fp8)


# ---- 2. validation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_ragged_option_validation_codes(fn):
    buf, addr = _aligned_addr()
    S, ST, NP, ABI = capi.FA_ERR_BAD_SHAPE, capi.FA_ERR_BAD_STRIDE, capi.FA_ERR_NULL_POINTER, capi.FA_ERR_BAD_ABI
    # what is accepted: plain, with packed k_new (the same cu tensor or another), any older option beside it, total_q = 0
    for o, sn in ((_rag(addr), 0), (_rag(addr, cu_seqlens_k_new=addr, total_k_new=64), 8), (_rag(addr, cu_seqlens_k_new=addr + 64, total_k_new=3), 3),
                  (_rag(addr, cache_dtype=FP8), 0), (_rag(addr, is_local=1, window_size_left=37, window_size_right=0), 0), (_rag(addr, total_q=0), 0),
                  (_rag(addr, total_q=1 << 20), 0), (_opt4(), 0), (_opt4(cache_dtype=FP8), 0)):
        assert _rc(_rag_params(fn, sq=4, sn=sn), fn, o) >= 0, capi.last_error()
    # cu_seqlens_k_new without cu_seqlens_q, or without k_new / v_new
    assert _rc(_rag_params(fn, sn=2), fn, _opt4(cu_seqlens_k_new=addr, total_k_new=2)) == NP and "without cu_seqlens_q" in capi.last_error()
    assert _rc(_rag_params(fn), fn, _rag(addr, cu_seqlens_k_new=addr, total_k_new=2)) == NP and "without k_new" in capi.last_error()
    # k_new in a ragged call without cu_seqlens_k_new
    assert _rc(_rag_params(fn, sn=2), fn, _rag(addr, total_k_new=2)) == NP and "need cu_seqlens_k_new" in capi.last_error()
    # the packed row counts
    for kw in (dict(total_q=-1), dict(total_q=-(1 << 40))):
        assert _rc(_rag_params(fn), fn, _rag(addr, **kw)) == S and "total_q" in capi.last_error(), kw
    assert _rc(_rag_params(fn, sn=2), fn, _rag(addr, cu_seqlens_k_new=addr, total_k_new=-1)) == S and "total_k_new" in capi.last_error()
    assert _rc(_rag_params(fn), fn, _rag(addr, total_q=1 << 40)) == S and "too large" in capi.last_error()
    # alignment
    for kw in (dict(cu_seqlens_q=addr + 2), dict(cu_seqlens_q=addr + 1), dict(cu_seqlens_k_new=addr + 6, total_k_new=2)):
        assert _rc(_rag_params(fn, sn=2 if "cu_seqlens_k_new" in kw else 0), fn, _rag(addr, **kw)) == ST, kw
        assert "4-byte aligned" in capi.last_error()
    assert _rc(_rag_params(fn), fn, _rag(addr + 4)) >= 0, capi.last_error()
    # rotary together with cu_seqlens_q: out of scope, and said so - after the rotary fields' own errors
    rot = dict(rotary_cos=addr, rotary_sin=addr, rotary_row_stride=64, seqlen_ro=32768, rotary_dim=128, rotary_interleaved=1, cu_seqlens_k_new=addr, total_k_new=2)
    assert _rc(_rag_params(fn, sn=2), fn, _rag(addr, **rot)) == S and "not supported" in capi.last_error() and "cu_seqlens_q" in capi.last_error()
    assert _rc(_rag_params(fn, sn=2), fn, _rag(addr, **dict(rot, rotary_dim=24))) == S and "rotary_dim" in capi.last_error()
    rot.update(cu_seqlens_q=None, cu_seqlens_k_new=None, total_k_new=0)
    p = _rag_params(fn, sn=2)
    p.k_new_stride = p.v_new_stride = capi.Strides(2 * p.h_k * p.d, p.h_k * p.d, p.d)
    if p.workspace is None:
        p.workspace, p.workspace_bytes = addr, 1 << 40
    assert _rc(p, fn, _opt4(**rot)) >= 0, capi.last_error()       # (the same rotary fields in a v4 struct without cu_seqlens_q: a v3 call)
    # struct sizes: exactly four are accepted
    for size in (24, 28, 40, 64, 71, 76, 80, 96, 104, 108, 111, 113, 116, 120, 128, 136, 140, 143, 145, 148, 152, 160, 176, 256):
        o = _rag(addr)
        o.struct_size = size
        assert _rc(_rag_params(fn), fn, o) == ABI, size
    for size, cls in ((20, capi.KvcacheOptions), (72, capi.KvcacheOptionsV2), (112, capi.KvcacheOptionsV3), (144, capi.KvcacheOptionsV4)):
        assert cls().struct_size == size and _rc(_params(), fn, cls()) >= 0, size
    # params errors still come first, and so do the older options' errors
    assert _rc(_rag_params(fn, h=3, hk=2), fn, _rag(addr, total_q=-1)) == capi.FA_ERR_BAD_GQA
    assert _rc(_rag_params(fn, sq=0), fn, _rag(addr, total_q=-1)) == S and "seqlen_q" in capi.last_error()          # max_seqlen_q >= 1
    assert _rc(_rag_params(fn), fn, _rag(addr, total_q=-1, cache_dtype=9)) == capi.FA_ERR_BAD_DTYPE
    assert _rc(_rag_params(fn), fn, _rag(addr, total_q=-1, is_local=1, window_size_left=-2)) == S and "window_size" in capi.last_error()
    # the batch strides of the packed tensors are not read: a value that the dense call refuses passes
    p = _rag_params(fn, sn=2)
    p.q_stride = p.o_stride = capi.Strides(3, p.h * p.d, p.d)
    p.k_new_stride = p.v_new_stride = capi.Strides(5, p.h_k * p.d, p.d)
    assert _rc(p, fn, _rag(addr, cu_seqlens_k_new=addr, total_k_new=2)) >= 0, capi.last_error()
    if fn != "fa_run_mha_fwd_kvcache_ex":                # (b = 0 there: the tensors are not looked at)
        assert _rc(p, fn, _opt4()) == ST


# ---- 3. workspace and split -----------------------------------------------------------------------------------------------------------------

def _ws_formula(n, rows, d):
    return 0 if n <= 1 else n * rows * d * 4 + (n * rows * 4 + 15) // 16 * 16


def _slots(total_q, b, max_sq, ratio):
    return min(-(-total_q * ratio // ROWS) + b, b * -(-max_sq * ratio // ROWS))


def test_workspace_is_todays_formula_over_h_times_total_q_rows():
    buf, addr = _aligned_addr()
    L = capi.lib()
    for b, max_sq, h, hk, cache, causal in SHAPES:
        for d in (64, 128):
            for total_q in (b, b * max_sq, 3 * b + 7, 1000):
                for ns in (0, 1, 2, 7, 500):
                    p = _rag_params("fa_kvcache_workspace_bytes_ex", b=b, sq=max_sq, h=h, hk=hk, cache=cache, causal=causal, d=d, num_splits=ns)
                    o = _rag(addr, total_q=total_q)
                    p.workspace, p.workspace_bytes = addr, 1 << 50
                    n = L.fa_kvcache_num_splits_ex(ctypes.byref(p), ctypes.byref(o))
                    assert n >= 1, capi.last_error()
                    assert L.fa_kvcache_workspace_bytes_ex(ctypes.byref(p), ctypes.byref(o)) == _ws_formula(n, h * total_q, d), (b, max_sq, h, d, total_q, ns)
                    # a workspace one byte short of n splits caps the split below n
                    if n > 1:
                        p.workspace_bytes = _ws_formula(n, h * total_q, d) - 1
                        assert L.fa_kvcache_num_splits_ex(ctypes.byref(p), ctypes.byref(o)) == n - 1


def test_forced_split_of_a_ragged_call_is_that_of_the_dense_call():
    """no window: the forced split depends on the capacity and the request alone, so ragged and dense calls cut the keys at the same places;
    with a left-bounded window the ragged call's span is sized from max_seqlen_q, as the dense call's from seqlen_q"""
    buf, addr = _aligned_addr()
    L = capi.lib()
    big = 1 << 50
    for b, max_sq, h, hk, cache, causal in SHAPES:
        for ns in (1, 2, 3, 7, 37, 128, 500, 100000):
            for fp8 in (0, FP8):
                dense = _params(b=1, sq=1, h=h, hk=hk, cache=cache, causal=causal, num_splits=ns, ws_bytes=big)
                want = L.fa_kvcache_num_splits_ex(ctypes.byref(dense), ctypes.byref(_opt4(cache_dtype=fp8)))
                assert want == min(ns, -(-cache // 32))
                for total_q in (1, b * max_sq, 999):
                    p = _rag_params("fa_kvcache_num_splits_ex", b=b, sq=max_sq, h=h, hk=hk, cache=cache, causal=causal, num_splits=ns, ws_bytes=big)
                    assert L.fa_kvcache_num_splits_ex(ctypes.byref(p), ctypes.byref(_rag(addr, total_q=total_q, cache_dtype=fp8))) == want
            for win in ((31, 0), (127, 3)):
                dense = _params(b=1, sq=max_sq, h=h, hk=hk, cache=cache, causal=causal, num_splits=ns, ws_bytes=big)
                p = _rag_params("fa_kvcache_num_splits_ex", b=b, sq=max_sq, h=h, hk=hk, cache=cache, causal=causal, num_splits=ns, ws_bytes=big)
                w = dict(is_local=1, window_size_left=win[0], window_size_right=win[1])
                assert L.fa_kvcache_num_splits_ex(ctypes.byref(p), ctypes.byref(_rag(addr, total_q=b * max_sq, **w))) == \
                    L.fa_kvcache_num_splits_ex(ctypes.byref(dense), ctypes.byref(_opt4(**w)))


def test_automatic_split_follows_the_slot_count():
    """the dense rule - no split once one workgroup per compute unit is there, else up to two per unit, at least 8 steps per split, at most 128 -
    with h_k x slots workgroups, slots = min(ceil(total_q * h_ratio / 16) + b, b * tiles(max_seqlen_q)).  Without a device the library
    assumes 256 compute units."""
    buf, addr = _aligned_addr()
    L = capi.lib()
    cus = 256 if not torch.cuda.is_available() else torch.cuda.get_device_properties(0).multi_processor_count

    def auto(b, max_sq, h, hk, cache, total_q):
        p = _rag_params("fa_kvcache_num_splits_ex", b=b, sq=max_sq, h=h, hk=hk, cache=cache, ws_bytes=1 << 50)
        return L.fa_kvcache_num_splits_ex(ctypes.byref(p), ctypes.byref(_rag(addr, total_q=total_q)))

    def rule(b, max_sq, h, hk, cache, total_q):
        wgs = hk * _slots(total_q, b, max_sq, h // hk)
        steps = -(-cache // 32)
        if steps <= 1 or wgs >= cus:
            return 1
        return max(1, min(-(-2 * cus // wgs), steps // 8, 128))

    # hand-computed points (256 units): slots, workgroups, splits
    assert _slots(4, 4, 1, 4) == 4 and _slots(64, 64, 1, 4) == 64                    # uniform decode: the plain grid is the smaller one
    assert _slots(63 + 512, 64, 512, 4) == 144 + 64 == 208                            # one 512-token chunk beside 63 decoding sequences, not 64 x 128
    assert _slots(10, 3, 8, 3) == min(2 + 3, 3 * 2) == 5
    if cus == 256:
        assert auto(4, 1, 32, 8, 32768, 4) == 16            # 8 x 4 = 32 workgroups -> ceil(512 / 32)
        assert auto(64, 1, 32, 8, 32768, 64) == 1           # 8 x 64 = 512 workgroups: already two per unit
        assert auto(64, 512, 32, 8, 32768, 575) == 1        # 8 x 208 workgroups
        assert auto(8, 256, 32, 8, 32768, 270) == 1         # 8 x (68 + 8) = 608
        assert auto(2, 16, 32, 8, 32768, 17) == 10          # slots = min(5 + 2, 2 x 4) = 7 -> 56 workgroups -> ceil(512 / 56)
        assert auto(1, 1, 32, 8, 1024, 1) == 4              # 8 workgroups, 32 steps: at most 32 // 8 = 4 splits
    for b, max_sq, h, hk, cache, _ in SHAPES:
        for total_q in (b, b * max_sq, b + max_sq - 1, 5000):
            assert auto(b, max_sq, h, hk, cache, total_q) == rule(b, max_sq, h, hk, cache, total_q), (b, max_sq, h, hk, cache, total_q)


def test_plain_c_caller_uses_the_v4_struct(tmp_path):
    src = tmp_path / "use_ragged.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
static _Alignas(16) char mem[256];
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = mem; p.lse = (float*)mem; p.cache_seqlens = (const int32_t*)mem;
    p.b = 4; p.seqlen_q = 8; p.seqlen_cache = 32768; p.h = 32; p.h_k = 8; p.d = 128; p.dtype = FA_FP16; p.num_splits = 4;
    p.q_stride = p.o_stride = (fa_strides){0, 32 * 128, 128};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 128, 8 * 128, 128};
    fa_kvcache_options_v3 o3;
    FA_PARAMS_INIT(o3);
    fa_kvcache_options_v4 o4;
    FA_PARAMS_INIT(o4);
    long long dense = fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o3);
    if (dense != 4LL * (4 * 32 * 8) * 128 * 4 + 4LL * (4 * 32 * 8) * 4) return 10;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o4) != dense) return 11;      /* zeroed tail: the v3 call */
    o4.cu_seqlens_q = (const int32_t*)mem; o4.total_q = 11;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o4) != 4LL * (32 * 11) * 128 * 4 + 4LL * (32 * 11) * 4) return 12;
    o4.total_q = -1;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o4) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "total_q")) return 13;
    o4.total_q = 11; o4.cu_seqlens_k_new = (const int32_t*)mem;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o4) != FA_ERR_NULL_POINTER) return 14;
    o4.cu_seqlens_k_new = NULL; o4.cu_seqlens_q = (const int32_t*)(mem + 2);
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o4) != FA_ERR_BAD_STRIDE) return 15;
    o4.cu_seqlens_q = (const int32_t*)mem; p.b = 0;
    if (fa_run_mha_fwd_kvcache_ex(&p, (const fa_kvcache_options*)&o4, NULL) != FA_OK) return 16;      /* nothing to do: no launch */
    return 0;
}
""")
    exe = tmp_path / "use_ragged"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_capi_helpers_build_the_v4_struct():
    q = torch.zeros(11, 32, 128, dtype=torch.float16)
    kc = torch.zeros(4, 256, 8, 128, dtype=torch.float16)
    kn = torch.zeros(5, 8, 128, dtype=torch.float16)
    lse = torch.zeros(32, 11)
    cu = torch.tensor([0, 1, 2, 10, 11], dtype=torch.int32)
    cun = torch.tensor([0, 1, 2, 4, 5], dtype=torch.int32)
    p = capi.kvcache_params(q, kc, kc, torch.empty_like(q), lse, cache_seqlens=torch.zeros(4, dtype=torch.int32), k_new=kn, v_new=kn, causal=True,
                            cu_seqlens_q=cu, max_seqlen_q=8)
    assert (p.b, p.seqlen_q, p.seqlen_cache, p.seqlen_new, p.h, p.h_k, p.d, p.is_causal) == (4, 8, 256, 5, 32, 8, 128, 1)
    assert (p.q_stride.row, p.q_stride.head, p.k_new_stride.row, p.k_new_stride.head) == (32 * 128, 128, 8 * 128, 128)
    o = capi.kvcache_options(cu_seqlens_q=cu, cu_seqlens_k_new=cun, total_q=11, total_k_new=5)
    assert isinstance(o, capi.KvcacheOptionsV4) and o.struct_size == 144
    assert (o.cu_seqlens_q, o.cu_seqlens_k_new, o.total_q, o.total_k_new) == (cu.data_ptr(), cun.data_ptr(), 11, 5)
    assert capi.kvcache_num_splits(p, o) == 1                       # (no workspace in the params)
    assert capi.kvcache_workspace_bytes(p, o) >= 0
    assert isinstance(capi.kvcache_options((3, 0)), capi.KvcacheOptions) and isinstance(capi.kvcache_options(cache_dtype=FP8), capi.KvcacheOptionsV2)


# ---- 4. the Python surface ----------------------------------------------------------------------------------------------------------------

def test_python_surface_rejects_bad_ragged_arguments():
    import flash_attn_turing as F

    b, h, hk, d, cap = 3, 4, 2, 64, 32
    q = torch.zeros(7, h, d, dtype=torch.float16)
    kc = torch.zeros(b, cap, hk, d, dtype=torch.float16)
    kn = torch.zeros(7, hk, d, dtype=torch.float16)
    cu = torch.tensor([0, 1, 6, 7], dtype=torch.int32)
    cs = torch.zeros(b, dtype=torch.int32)

    def call(qq=q, **kw):
        args = dict(cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=5)
        args.update(kw)
        return F.flash_attn_with_kvcache(qq, kc, kc, **args)

    # rotary together with cu_seqlens_q: out of scope, and the message says so
    cos = torch.ones(cap, 16, dtype=torch.float16)
    with pytest.raises(ValueError, match="rotary_cos / rotary_sin together with cu_seqlens_q are not supported"):
        call(k=kn, v=kn, cu_seqlens_k_new=cu, rotary_cos=cos, rotary_sin=cos)
    # the cu tensors
    for bad in (cu.long(), cu.float(), [0, 1, 6, 7], 7):
        with pytest.raises(ValueError, match="cu_seqlens_q must be an int32 tensor"):
            call(cu_seqlens_q=bad)
    for bad in (cu[None], cu[:0], torch.tensor(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"cu_seqlens_q must have shape \(batch \+ 1,\)"):
            call(cu_seqlens_q=bad)
    with pytest.raises(ValueError, match="cu_seqlens_q must be on q's device"):
        call(cu_seqlens_q=cu.to("meta"))
    with pytest.raises(ValueError, match="cu_seqlens_q must be contiguous"):
        call(cu_seqlens_q=torch.zeros(8, dtype=torch.int32)[::2])
    # max_seqlen_q: a Python int >= 1, required
    for bad in (None, 0, -1, 2.0, True, torch.tensor(5), 2**31):
        with pytest.raises(ValueError, match="max_seqlen_q must be a Python int >= 1"):
            call(max_seqlen_q=bad)
    # packed q, packed k / v with their own cu
    with pytest.raises(ValueError, match=r"q must be packed \(total_q, nheads, d\)"):
        call(qq=q[None])
    with pytest.raises(ValueError, match="packed k and v need cu_seqlens_k_new"):
        call(k=kn, v=kn)
    with pytest.raises(ValueError, match="a 4-D k belongs to the dense call"):
        call(k=kn[None], v=kn[None], cu_seqlens_k_new=cu)
    with pytest.raises(ValueError, match="cu_seqlens_k_new given without k and v"):
        call(cu_seqlens_k_new=cu)
    with pytest.raises(ValueError, match="both be given or both be None"):
        call(k=kn, cu_seqlens_k_new=cu)
    with pytest.raises(ValueError, match=r"cu_seqlens_k_new must have shape \(batch \+ 1,\) = \(4,\)"):
        call(k=kn, v=kn, cu_seqlens_k_new=cu[:3])
    with pytest.raises(ValueError, match="cu_seqlens_k_new must be an int32 tensor"):
        call(k=kn, v=kn, cu_seqlens_k_new=cu.long())
    # without cu_seqlens_q the other two are refused
    with pytest.raises(ValueError, match="cu_seqlens_k_new given without cu_seqlens_q"):
        F.flash_attn_with_kvcache(q[None], kc[:1], kc[:1], cache_seqlens=4, cu_seqlens_k_new=cu)
    with pytest.raises(ValueError, match="max_seqlen_q given without cu_seqlens_q"):
        F.flash_attn_with_kvcache(q[None], kc[:1], kc[:1], cache_seqlens=4, max_seqlen_q=3)
    # the batch is len(cu_seqlens_q) - 1
    with pytest.raises(ValueError, match=r"cache_seqlens must have shape \(batch,\) = \(3,\)"):
        call(cache_seqlens=torch.zeros(7, dtype=torch.int32))
    with pytest.raises(ValueError, match="k_cache / v_cache must have batch"):
        F.flash_attn_with_kvcache(q, kc[:2], kc[:2], cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=5)
    pool = torch.zeros(8, 16, hk, d, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"block_table must have shape \(batch, max_blocks_per_seq\)"):
        F.flash_attn_with_kvcache(q, pool, pool, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=5, block_table=torch.zeros(7, 2, dtype=torch.int32))
    c8 = torch.zeros(b, cap, hk, d, dtype=torch.float8_e4m3fn)
    with pytest.raises(ValueError, match=r"k_descale must have shape \(batch, nheads_k\) = \(3, 2\)"):
        F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=5, k_descale=torch.ones(7, hk))
    with pytest.raises(RuntimeError, match="forward-only"):
        call(qq=q.clone().requires_grad_(True))
    # a CPU call that passes the checks is still refused by the extension (no quiet fall-back)
    for kw in (dict(), dict(causal=True, window_size=(7, 0)), dict(k=kn, v=kn, cu_seqlens_k_new=cu), dict(cache_seqlens=4, num_splits=3)):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=5, k_descale=torch.ones(b, hk), v_descale=torch.ones(b, hk))


def test_extension_signature_keeps_the_old_calls_and_gains_the_keywords():
    from flash_attn_turing import _C

    doc = _C.fwd_kvcache.__doc__
    # the signature as it was stays the first overload (every existing call resolves to it); the second continues it after rotary_interleaved
    first, second = doc[doc.index("1. fwd_kvcache("):doc.index("2. fwd_kvcache(")], doc[doc.index("2. fwd_kvcache("):]
    assert re.search(r"rotary_interleaved: bool = True\) ->", first) and "cu_seqlens" not in first, first
    sig = second[:second.index("->")]
    assert re.search(r"rotary_interleaved: bool = True, cu_seqlens_q: [^,]*= None, max_seqlen_q: [^,]*= 0, cu_seqlens_k_new: [^,]*= None\)", sig), sig
    assert sig.index("*, k_descale") < sig.index("cu_seqlens_q")                 # keyword-only, after rotary_interleaved


# ---- 5. ISA -------------------------------------------------------------------------------------------------------------------------------

def test_ragged_kernels_isa():
    """48 attention kernels ({fp16, bf16} x {64, 128} x {plain, causal, local} x {contiguous, paged} x {16-bit, FP8}), 4 combine, 12 append: no
    scratch, two workgroups per CU for the attention kernels with an MFMA loop free of scratch traffic and accumulator moves, no MFMA hazard, M0
    untouched, and no scalar memory write anywhere; the dense kernels are not compiled a second time"""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_kvcache_ragged.hip" in B.HIP_SOURCES and "fa_fwd_kvcache_ragged.hip" in B.M0_GUARD_SOURCES
    ks = analyse("fa_fwd_kvcache_ragged.hip")
    attn = {n: k for n, k in ks.items() if "fa_fwd_kvcache_ragged_kernel" in n}
    comb = {n: k for n, k in ks.items() if "fa_kvcache_combine_ragged_kernel" in n}
    app = {n: k for n, k in ks.items() if "fa_kvcache_append_ragged_kernel" in n}
    assert (len(attn), len(comb), len(app)) == (48, 4, 12) and len(ks) == 64, sorted(ks)
    keys = set()
    for n, k in attn.items():
        m = re.search(r"fa_fwd_kvcache_ragged_kernelI(DF16_|DF16b)Li(\d+)ELi(\d)ELb(\d)ELi(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 256, (n, k["vgprs"], k["scratch_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
    assert keys == {(t, d, m, p, e) for t in ("DF16_", "DF16b") for d in ("64", "128") for m in "012" for p in "01" for e in "12"}
    for n, k in list(comb.items()) + list(app.items()):
        assert k["scratch_bytes"] == 0 and k["m0_outside_asm"] == 0 and k["mfma_total"] == 0 and k["lds_bytes"] == 0, (n, k)
    src = os.path.join(B.CSRC, "fa_fwd_kvcache_ragged.hip")
    asm = subprocess.run([B.hipcc_path()] + B.HIPCC_FLAGS + ["-I", B.CSRC, "-I", B.INCLUDE, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    assert B.m0_uses_outside_asm(asm) == 0
    ops = set(re.findall(r"^\s+(s_[a-z0-9_]+)", asm, re.M))
    assert not [o for o in ops if "store" in o or "atomic" in o or "dcache" in o], ops              # scalar instructions only load
