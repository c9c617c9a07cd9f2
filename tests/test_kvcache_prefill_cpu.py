"""CPU: the 64-row attention kernels for prompt chunks (the `prefill` keyword of flash_attn_with_kvcache, fa_kvcache_options_v8.row_tile of the
C ABI) - the struct layout against the header, the eight accepted struct sizes, a zeroed tail as a v7 call, fa_kvcache_row_tile_ex, every
refusal with its code and the field it names, the Python surface's validation, the ragged slot formula at 64 rows as the split rule sees it,
the extension's entry point, and the resources of the new kernels.  No GPU involved."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi
from test_kvcache_softcap_cpu import SHAPES
from test_kvcache_window_cpu import EX_ENTRY_POINTS, _aligned_addr, _params, _rc

FP8 = capi.FA_CACHE_FP8_E4M3
ALL_ENTRY_POINTS = EX_ENTRY_POINTS + ["fa_kvcache_row_tile_ex"]


def _opt8(**kw):
    o = capi.KvcacheOptionsV8()
    for k, v in kw.items():
        if k in ("reserved", "reserved2", "reserved3", "reserved4"):
            for i, x in enumerate(v):
                getattr(o, k)[i] = x
        else:
            setattr(o, k, v)
    return o


# ---- 1. layout --------------------------------------------------------------------------------------------------------------------------

def test_options_v8_layout_matches_header(tmp_path):
    """fa_kvcache_options .. _v7 keep their sizes; v8 repeats the v7 fields at the same offsets, appends row_tile, reserved4_ and reserved4[5]
    and is 288 bytes; ctypes agrees with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheOptionsV8._fields_]
    v7 = [f[0] for f in capi.KvcacheOptionsV7._fields_]
    assert fields[:len(v7)] == v7
    assert fields[len(v7):] == ["row_tile", "reserved4_", "reserved4"]
    src = tmp_path / "opt8_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_KVCACHE_PREFILL\n#error "no FA_HAS_KVCACHE_PREFILL"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(fa_kvcache_options_v8), sizeof(fa_kvcache_options_v7), sizeof(fa_kvcache_options_v6), sizeof(fa_kvcache_options_v5), sizeof(fa_kvcache_options_v4), sizeof(fa_kvcache_options_v3), sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options));\n'
                   '    printf("abi %d 0\\n", FA_ABI_VERSION);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options_v8, {f}), sizeof(((fa_kvcache_options_v8*)0)->{f}));\n' for f in fields)
                   + "".join(f'    printf("v7_{f} %zu 0\\n", offsetof(fa_kvcache_options_v7, {f}));\n' for f in v7)
                   + "    fa_kvcache_options_v8 o;\n    FA_PARAMS_INIT(o);\n"
                     "    return o.struct_size == sizeof(o) && o.magic == FA_PARAMS_MAGIC && o.row_tile == 0 && o.reserved4_ == 0 && o.reserved4[0] == 0 && o.reserved4[4] == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "opt8_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    sizes = [ctypes.sizeof(c) for c in (capi.KvcacheOptionsV8, capi.KvcacheOptionsV7, capi.KvcacheOptionsV6, capi.KvcacheOptionsV5, capi.KvcacheOptionsV4,
                                        capi.KvcacheOptionsV3, capi.KvcacheOptionsV2, capi.KvcacheOptions)]
    assert got["size"] == sizes == [288, 240, 200, 168, 144, 112, 72, 20]
    assert got["abi"][0] == 4 == capi.lib().fa_abi_version()
    for f in fields:
        assert got[f] == [getattr(capi.KvcacheOptionsV8, f).offset, getattr(capi.KvcacheOptionsV8, f).size], f
    for f in v7:
        assert got["v7_" + f][0] == got[f][0], f
    assert (got["row_tile"], got["reserved4_"], got["reserved4"]) == ([240, 4], [244, 4], [248, 40])


@pytest.mark.parametrize("fn", ALL_ENTRY_POINTS)
def test_exactly_eight_struct_sizes_are_accepted(fn):
    for size in list(range(8, 20)) + [24, 64, 71, 76, 104, 111, 113, 120, 136, 143, 145, 152, 160, 167, 169, 176, 184, 192, 199, 201, 208, 216, 224, 232, 236, 239, 241, 244,
                                      248, 256, 264, 272, 280, 284, 287, 289, 292, 296, 304, 320, 336, 512, 1024]:
        o = _opt8(row_tile=64)
        o.struct_size = size
        assert _rc(_params(), fn, o) == capi.FA_ERR_BAD_ABI, size
    for size, cls in ((20, capi.KvcacheOptions), (72, capi.KvcacheOptionsV2), (112, capi.KvcacheOptionsV3), (144, capi.KvcacheOptionsV4), (168, capi.KvcacheOptionsV5),
                      (200, capi.KvcacheOptionsV6), (240, capi.KvcacheOptionsV7), (288, capi.KvcacheOptionsV8)):
        assert cls().struct_size == size and _rc(_params(), fn, cls()) >= 0, size
    # a v8 struct that states a shorter size is that shorter struct: the tail is not read
    o = _opt8(row_tile=5, reserved4_=7, reserved4=(7, 7, 7, 7, 7))
    o.struct_size = 240
    assert _rc(_params(), fn, o) >= 0, capi.last_error()


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_v8_with_a_zeroed_tail_is_a_v7_call(fn):
    """same split and workspace from a v7 struct and a v8 struct with a zeroed tail - 16-bit and 8-bit cache, dense and ragged, causal or not,
    with and without a softmax_scale, over the shapes of the tree CPU test; and both take the 16-row kernels"""
    f = getattr(capi.lib(), fn)
    tile = capi.lib().fa_kvcache_row_tile_ex
    buf, addr = _aligned_addr()
    for b, sq, h, hk, cache, causal in SHAPES:
        for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
            for ws in (None, 1 << 40, 3 * b * h * sq * 128 * 4 + (3 * b * h * sq * 4 + 15) // 16 * 16):
                for ragged in (False, True):
                    for cz in (False, True):
                        p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=cz, ws_bytes=ws, **kw)
                        if ragged:
                            p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
                        for fp8 in (0, FP8):
                            v7, v8 = capi.KvcacheOptionsV7(), _opt8()
                            assert (v7.struct_size, v8.struct_size) == (240, 288)
                            for o in (v7, v8):
                                o.cache_dtype = fp8
                                o.softmax_scale = 0.37 if cache == 768 else 0.0
                                if ragged:
                                    o.cu_seqlens_q, o.total_q = addr, b * sq - 1 + b
                            want = f(ctypes.byref(p), ctypes.byref(v7))
                            assert want >= 0, capi.last_error()
                            assert f(ctypes.byref(p), ctypes.byref(v8)) == want, (b, sq, cache, ws, kw, fp8, ragged, cz, capi.last_error())
                            assert tile(ctypes.byref(p), ctypes.byref(v8)) == tile(ctypes.byref(p), ctypes.byref(v7)) == 16


# ---- 2. which path, and the split of the wide grid ----------------------------------------------------------------------------------------

def test_row_tile_ex_says_which_kernels_a_call_takes():
    buf, addr = _aligned_addr()
    for p in (_params(), _params(sq=2048, causal=True), _params(sq=100, d=64, page=16), _params(b=0)):
        assert capi.kvcache_row_tile(p) == 16                                   # NULL options
        for o in (capi.KvcacheOptions(), capi.KvcacheOptionsV7(), _opt8(), capi.kvcache_options((5, 0)), capi.kvcache_options(softcap=30.0)):
            assert capi.kvcache_row_tile(p, o) == 16
        for o in (_opt8(row_tile=64), _opt8(row_tile=64, cache_dtype=FP8), _opt8(row_tile=64, softmax_scale=0.3), capi.kvcache_options(row_tile=64)):
            assert capi.kvcache_row_tile(p, o) == 64, capi.last_error()
    pr = _params(b=3, sq=40)
    pr.q_stride = pr.o_stride = capi.Strides(0, pr.h * pr.d, pr.d)
    assert capi.kvcache_row_tile(pr, _opt8(row_tile=64, cu_seqlens_q=addr, total_q=77)) == 64
    assert capi.kvcache_row_tile(pr, _opt8(cu_seqlens_q=addr, total_q=77)) == 16
    # the workspace fields are not looked at
    p = _params(sq=2048)
    p.workspace, p.workspace_bytes = addr + 1, -5
    assert capi.kvcache_row_tile(p, _opt8(row_tile=64)) == 64
    # errors are those of the launch
    assert capi.lib().fa_kvcache_row_tile_ex(ctypes.byref(_params(h=3, hk=2)), None) == capi.FA_ERR_BAD_GQA
    assert capi.lib().fa_kvcache_row_tile_ex(ctypes.byref(_params()), ctypes.byref(_opt8(row_tile=32))) == capi.FA_ERR_BAD_SHAPE
    assert "fa_kvcache_row_tile_ex" in capi.declared_functions()
    o = capi.kvcache_options(row_tile=64)
    assert isinstance(o, capi.KvcacheOptionsV8) and o.struct_size == 288 and o.row_tile == 64 and o.tree_mask is None
    assert type(capi.kvcache_options(tree_mask=torch.zeros(1, 1, dtype=torch.int64))) is capi.KvcacheOptionsV7 and type(capi.kvcache_options()) is capi.KvcacheOptions


def _auto_split(wgs, cache, cus):
    """the existing rule (fa_fwd_kvcache.hip kvcache_split) for a launch of `wgs` workgroups over a capacity of `cache` keys"""
    steps = (cache + 31) // 32
    if steps <= 1 or wgs >= cus:
        return 1
    return max(1, min((2 * cus + wgs - 1) // wgs, steps // 8, 128))


def test_automatic_split_counts_the_wide_grid_and_a_forced_split_is_unchanged():
    """dense: b x h_k x ceil(sq x h_ratio / 64) workgroups; ragged: h_k x min(ceil(total_q x h_ratio / 64) + b, b x tiles64(max_seqlen_q)) - the
    rule itself, the workspace formula and a forced num_splits are those of the 16-row call"""
    buf, addr = _aligned_addr()
    cus = 256                                                    # (no device here: the library's stand-in)
    big = 1 << 40
    seen = set()
    for b, sq, h, hk, cache in ((1, 1, 32, 8, 32768), (1, 64, 32, 8, 32768), (1, 100, 32, 8, 8192), (2, 300, 32, 8, 8192), (1, 2048, 32, 8, 32768), (3, 17, 6, 2, 4096),
                                (1, 1024, 32, 8, 4096), (1, 128, 16, 1, 1024), (5, 65, 8, 8, 65536)):
        ratio = h // hk
        p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, ws_bytes=big)
        for rows, o in ((16, _opt8()), (64, _opt8(row_tile=64))):
            want = _auto_split(b * hk * ((sq * ratio + rows - 1) // rows), cache, cus)
            got = capi.kvcache_num_splits(p, o)
            assert got == want, (b, sq, h, hk, cache, rows, got, want)
            seen.add((rows, got > 1))
            rowsz = b * h * sq
            assert capi.kvcache_workspace_bytes(p, o) == (0 if got == 1 else got * rowsz * 128 * 4 + (got * rowsz * 4 + 15) // 16 * 16)
        for ns in (1, 3, 7, 500):
            pf = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, ws_bytes=big, num_splits=ns)
            assert capi.kvcache_num_splits(pf, _opt8(row_tile=64)) == capi.kvcache_num_splits(pf, _opt8()) == min(ns, (cache + 31) // 32)
            assert capi.kvcache_workspace_bytes(pf, _opt8(row_tile=64)) == capi.kvcache_workspace_bytes(pf, _opt8())
        # ragged, max_seqlen_q = sq: total_q rows over b sequences
        pr = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, ws_bytes=big)
        pr.q_stride = pr.o_stride = capi.Strides(0, h * 128, 128)
        for total in (b, b * sq // 2 + 1, b * sq):
            for rows, o in ((16, _opt8(cu_seqlens_q=addr, total_q=total)), (64, _opt8(row_tile=64, cu_seqlens_q=addr, total_q=total))):
                slots = min((total * ratio + rows - 1) // rows + b, b * ((sq * ratio + rows - 1) // rows))
                want = _auto_split(hk * slots, cache, cus)
                got = capi.kvcache_num_splits(pr, o)
                assert got == want, ("ragged", b, sq, h, hk, cache, total, rows, got, want)
                assert capi.kvcache_workspace_bytes(pr, o) == (0 if got == 1 else got * h * total * 128 * 4 + (got * h * total * 4 + 15) // 16 * 16)
    assert seen == {(16, False), (16, True), (64, False), (64, True)}
    # the two grids differ where it matters: 300 rows x 4 heads per KV head are 75 x 8 = 600 workgroups of 16 rows (no split at 256 units) and
    # 19 x 8 = 152 of 64 rows (split until two per unit: ceil(512 / 152) = 4)
    p = _params(b=1, sq=300, h=32, hk=8, cache=8192, ws_bytes=big)
    assert capi.kvcache_num_splits(p, _opt8()) == 1 and capi.kvcache_num_splits(p, _opt8(row_tile=64)) == 4


# ---- 3. validation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", ALL_ENTRY_POINTS)
def test_prefill_option_validation_codes_and_their_order(fn):
    buf, addr = _aligned_addr()
    S, ABI, STRIDE = capi.FA_ERR_BAD_SHAPE, capi.FA_ERR_BAD_ABI, capi.FA_ERR_BAD_STRIDE

    def P(**kw):
        p = _params(**kw)
        if fn == "fa_run_mha_fwd_kvcache_ex":
            p.b = 0                                          # (validated, launches nothing: the addresses are dummies)
        return p

    def R(**kw):                                             # the params of a ragged call
        p = P(**kw)
        p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
        return p

    W = dict(row_tile=64)
    # what is accepted
    for o in (_opt8(), _opt8(**W), _opt8(softmax_scale=0.125, **W), _opt8(cache_dtype=FP8, k_descale=addr, v_descale=addr, **W),
              _opt8(is_local=1, window_size_left=-1, window_size_right=-1, **W), _opt8(is_local=0, window_size_left=5, **W)):
        for d in (64, 128):
            for sq in (1, 5, 64, 65, 2048):
                for causal in (False, True):
                    assert _rc(P(sq=sq, d=d, causal=causal), fn, o) >= 0, capi.last_error()
    assert _rc(R(sq=300), fn, _opt8(cu_seqlens_q=addr, total_q=1000, **W)) >= 0, capi.last_error()
    assert _rc(P(sq=400, page=16), fn, _opt8(**W)) >= 0 and _rc(P(sq=400, page=48, cache=48 * 100), fn, _opt8(**W)) >= 0, capi.last_error()
    pk = P(sq=200, ws_bytes=1 << 30)
    pk.k_new = pk.v_new = pk.cache_seqlens = addr
    pk.seqlen_new = 200
    pk.k_new_stride = pk.v_new_stride = capi.Strides(200 * pk.h_k * pk.d, pk.h_k * pk.d, pk.d)
    assert _rc(pk, fn, _opt8(**W)) >= 0, capi.last_error()
    # without row_tile everything is what it was
    assert _rc(P(d=256, sq=100, causal=True), fn, _opt8(softcap=30.0)) >= 0 and _rc(P(sq=65), fn, _opt8(sinks=addr)) >= 0, capi.last_error()
    assert _rc(P(sq=5), fn, _opt8(tree_mask=addr, tree_mask_row_stride=1)) >= 0 and _rc(P(), fn, _opt8(is_local=1, window_size_left=7)) >= 0, capi.last_error()
    # a row tile the library does not have
    for rt in (1, 16, 32, 63, 65, 128, 256, -1, -64):
        assert _rc(P(), fn, _opt8(row_tile=rt)) == S and "row_tile" in capi.last_error(), rt
    # the refusals, each with the field named
    for win in ((7, 0), (-1, 0), (3, -1), (0, 0)):
        assert _rc(P(), fn, _opt8(is_local=1, window_size_left=win[0], window_size_right=win[1], **W)) == S, win
        assert "row_tile" in capi.last_error() and "window_size" in capi.last_error(), win
    assert _rc(P(), fn, _opt8(softcap=30.0, **W)) == S and "row_tile" in capi.last_error() and "softcap" in capi.last_error()
    assert _rc(P(), fn, _opt8(sinks=addr, sinks_stride=1, **W)) == S and "row_tile" in capi.last_error() and "sinks" in capi.last_error()
    assert _rc(P(sq=5), fn, _opt8(tree_mask=addr, tree_mask_row_stride=1, **W)) == S and "row_tile" in capi.last_error() and "tree_mask" in capi.last_error()
    pr = P(sq=2, ws_bytes=1 << 30)                         # (a rotary call keeps the image of the rotated q in the workspace)
    pr.k_new = pr.v_new = pr.cache_seqlens = addr
    pr.seqlen_new = 2
    pr.k_new_stride = pr.v_new_stride = capi.Strides(2 * pr.h_k * pr.d, pr.h_k * pr.d, pr.d)
    rot = dict(rotary_cos=addr, rotary_sin=addr, rotary_row_stride=64, seqlen_ro=32768, rotary_dim=128)
    assert _rc(pr, fn, _opt8(**rot)) >= 0, capi.last_error()
    assert _rc(pr, fn, _opt8(**rot, **W)) == S and "row_tile" in capi.last_error() and "rotary" in capi.last_error()
    assert _rc(P(d=256), fn, _opt8(**W)) == S and "row_tile" in capi.last_error() and "256" in capi.last_error()
    # a non-zero reserved word is a newer caller's field
    for kw in (dict(reserved4_=1), dict(reserved4_=-1), dict(reserved4=(1, 0, 0, 0, 0)), dict(reserved4=(0, 0, 0, 0, 1 << 40)), dict(reserved4=(0, 0, -1, 0, 0))):
        assert _rc(P(), fn, _opt8(**kw)) == ABI and "reserved4" in capi.last_error(), kw
        assert _rc(P(), fn, _opt8(**kw, **W)) == ABI and "reserved4" in capi.last_error(), kw
    # the order: params first, then the older option fields (their reserved words among them), then row_tile, then reserved4
    bad8 = dict(row_tile=7, reserved4=(1, 1, 1, 1, 1))
    assert _rc(P(h=3, hk=2), fn, _opt8(**bad8)) == capi.FA_ERR_BAD_GQA
    assert _rc(P(sq=0), fn, _opt8(**bad8)) == S and "seqlen_q" in capi.last_error() and "row_tile" not in capi.last_error()
    assert _rc(P(), fn, _opt8(cache_dtype=9, **bad8)) == capi.FA_ERR_BAD_DTYPE
    assert _rc(P(), fn, _opt8(is_local=1, window_size_left=-2, **bad8)) == S and "row_tile" not in capi.last_error()
    assert _rc(P(), fn, _opt8(softmax_scale=-1.0, **bad8)) == S and "softmax_scale" in capi.last_error()
    assert _rc(P(), fn, _opt8(sinks=addr + 2, **bad8)) == STRIDE and "sinks" in capi.last_error()
    assert _rc(P(), fn, _opt8(tree_mask=addr + 4, **bad8)) == STRIDE and "tree_mask" in capi.last_error()
    assert _rc(P(), fn, _opt8(reserved3=(1, 0), **bad8)) == ABI and "fa_kvcache_options_v7" in capi.last_error()
    assert _rc(P(), fn, _opt8(**bad8)) == S and "row_tile" in capi.last_error()
    assert _rc(P(), fn, _opt8(row_tile=64, softcap=5.0, reserved4=(1, 1, 1, 1, 1))) == S and "softcap" in capi.last_error()
    assert _rc(P(), fn, _opt8(row_tile=64, reserved4=(1, 1, 1, 1, 1))) == ABI


def test_plain_c_caller_uses_the_v8_struct(tmp_path):
    src = tmp_path / "use_prefill.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
static _Alignas(16) char mem[256];
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = mem; p.lse = (float*)mem; p.cache_seqlens = (const int32_t*)mem;
    p.b = 1; p.seqlen_q = 512; p.seqlen_cache = 32768; p.h = 32; p.h_k = 8; p.d = 128; p.dtype = FA_BF16; p.num_splits = 4; p.is_causal = 1;
    p.q_stride = p.o_stride = (fa_strides){512 * 32 * 128, 32 * 128, 128};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 128, 8 * 128, 128};
    fa_kvcache_options_v7 o7;
    FA_PARAMS_INIT(o7);
    fa_kvcache_options_v8 o8;
    FA_PARAMS_INIT(o8);
    if (sizeof(o8) != 288) return 9;
    long long dense = fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o7);
    if (dense != 4LL * (32 * 512) * 128 * 4 + 4LL * (32 * 512) * 4) return 10;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o8) != dense) return 11;      /* zeroed tail: the v7 call */
    if (fa_kvcache_row_tile_ex(&p, (const fa_kvcache_options*)&o8) != 16 || fa_kvcache_row_tile_ex(&p, NULL) != 16) return 12;
    o8.row_tile = 64;
    if (fa_kvcache_row_tile_ex(&p, (const fa_kvcache_options*)&o8) != 64) return 13;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o8) != dense) return 14;      /* a forced split: the same planes */
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o8) != 1) return 15;               /* (no workspace in the params) */
    o8.softcap = 30.0f;
    if (fa_kvcache_row_tile_ex(&p, (const fa_kvcache_options*)&o8) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "softcap")) return 16;
    o8.softcap = 0.0f; o8.row_tile = 48;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o8) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "row_tile")) return 17;
    o8.row_tile = 64; o8.reserved4[3] = 1;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o8) != FA_ERR_BAD_ABI) return 18;
    o8.reserved4[3] = 0; p.b = 0;
    if (fa_run_mha_fwd_kvcache_ex(&p, (const fa_kvcache_options*)&o8, NULL) != FA_OK) return 19;      /* nothing to do: no launch */
    return 0;
}
""")
    exe = tmp_path / "use_prefill"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


# ---- 4. the Python surface and the extension --------------------------------------------------------------------------------------------

def test_python_surface_checks_prefill_before_any_device_work():
    import flash_attn_turing as F

    b, sq, h, hk, d, cap = 2, 70, 4, 2, 64, 128
    q = torch.zeros(b, sq, h, d, dtype=torch.float16)
    kc = torch.zeros(b, cap, hk, d, dtype=torch.float16)

    def call(**kw):
        return F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=8, **kw)

    for bad in (1, 0, None, "yes", 64, 1.0, torch.tensor(True), [True]):
        with pytest.raises(ValueError, match="prefill must be a bool"):
            call(prefill=bad)
    for win in ((7, 0), (-1, 0), (3, -1)):
        with pytest.raises(ValueError, match="prefill=True together with window_size"):
            call(prefill=True, window_size=win)
        with pytest.raises(ValueError, match="prefill=True together with window_size"):
            call(prefill=True, window_size=win, causal=True)
    with pytest.raises(ValueError, match="prefill=True together with softcap"):
        call(prefill=True, softcap=30.0)
    with pytest.raises(ValueError, match="prefill=True together with sinks"):
        call(prefill=True, sinks=torch.zeros(h))
    q5 = torch.zeros(b, 5, h, d, dtype=torch.float16)
    with pytest.raises(ValueError, match="prefill=True together with tree_mask"):
        F.flash_attn_with_kvcache(q5, kc, kc, cache_seqlens=8, prefill=True, tree_mask=torch.zeros(b, 5, dtype=torch.int64))
    kn = torch.zeros(b, sq, hk, d, dtype=torch.float16)
    cos = torch.zeros(cap, 16, dtype=torch.float16)
    with pytest.raises(ValueError, match="prefill=True together with rotary"):
        F.flash_attn_with_kvcache(q, kc, kc, k=kn, v=kn, cache_seqlens=8, rotary_cos=cos, rotary_sin=cos, prefill=True)
    q256, kc256 = torch.zeros(b, sq, h, 256, dtype=torch.float16), torch.zeros(b, cap, hk, 256, dtype=torch.float16)
    with pytest.raises(ValueError, match="prefill=True at head_dim 256"):
        F.flash_attn_with_kvcache(q256, kc256, kc256, cache_seqlens=8, prefill=True)
    qr = torch.zeros(7, h, d, dtype=torch.float16)
    cu = torch.tensor([0, 2, 7], dtype=torch.int32)
    with pytest.raises(ValueError, match="prefill=True together with softcap"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=8, cu_seqlens_q=cu, max_seqlen_q=5, prefill=True, softcap=2.0)
    # keyword-only
    with pytest.raises(TypeError):
        F.flash_attn_with_kvcache(q, kc, kc, None, None, 8, False, 0, False, True)
    # a CPU call that passes the checks is still refused by the extension (no quiet fall-back): dense, causal, split, scaled, appended, ragged, FP8
    for kw in (dict(prefill=True), dict(prefill=True, causal=True), dict(prefill=True, num_splits=3, softmax_scale=0.125), dict(prefill=True, k=kn, v=kn),
               dict(prefill=True, window_size=(-1, -1), softcap=0.0), dict(prefill=False), dict()):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=8, cu_seqlens_q=cu, max_seqlen_q=64, prefill=True, causal=True)
    k8 = torch.zeros(b, cap, hk, d, dtype=torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(q, k8, k8, cache_seqlens=8, prefill=True, k_descale=torch.ones(b, hk), v_descale=torch.ones(b, hk))
    doc = F.flash_attn_with_kvcache.__doc__
    assert "prefill" in doc and "NO bit relation" in doc and "64" in doc


def test_extension_takes_prefill_on_a_function_of_its_own():
    from flash_attn_turing import _C

    doc = _C.fwd_kvcache.__doc__
    assert "3. fwd_kvcache(" in doc and "4. fwd_kvcache(" not in doc and "prefill" not in doc
    assert "prefill" not in _C.fwd_kvcache_sinks.__doc__ and "prefill" not in _C.fwd_kvcache_tree.__doc__
    pdoc = _C.fwd_kvcache_prefill.__doc__
    sig = pdoc[:pdoc.index("->")]
    assert re.search(r"tree_mask: [^,]*= None, prefill: bool = False\)", sig), sig
    assert sig.index("*, k_descale") < sig.index("softmax_scale") < sig.index(", sinks:") < sig.index(", tree_mask:") < sig.index(", prefill:")        # keyword-only
    names = lambda s: re.findall(r"(\w+): ", s[s.index("("):])
    tdoc = _C.fwd_kvcache_tree.__doc__
    n7, n8 = names(tdoc[:tdoc.index("->")]), names(sig)
    assert n8[:len(n7)] == n7 and n8[len(n7):] == ["prefill"], (n7, n8)
    q = torch.zeros(2, 3, 4, 64, dtype=torch.float16)
    kc = torch.zeros(2, 32, 2, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        _C.fwd_kvcache_prefill(q, kc, kc, prefill=True)


# ---- 5. ISA -----------------------------------------------------------------------------------------------------------------------------

def test_prefill_kernels_isa():
    """64 attention kernels ({fp16, bf16} x {64, 128} x {plain, causal} x {contiguous, paged} x {16-bit, FP8} x {dense, ragged}) and nothing else -
    no append, no combine, no second copy of an existing kernel.  No scratch, two workgroups per CU as the launch bounds ask (VGPRs <= 256, no
    AGPRs, 2 x LDS <= 160 KiB; the double-buffered K / V images are 2 x 16 KiB at head_dim 128 and 2 x 8 KiB at 64), an MFMA loop free of
    scratch traffic and accumulator moves that reads K as rows and V transposed from LDS and holds a barrier, no MFMA result read early, M0
    untouched."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_kvcache_prefill.hip" in B.HIP_SOURCES and "fa_fwd_kvcache_prefill.hip" in B.M0_GUARD_SOURCES
    src = open(os.path.join(B.CSRC, "fa_fwd_kvcache_prefill.hip")).read()
    assert src.count("__launch_bounds__(kKvcThreads, 2)") == 2
    ks = analyse("fa_fwd_kvcache_prefill.hip")
    dense = {n: k for n, k in ks.items() if "fa_fwd_kvcache_prefill_kernel" in n}
    ragged = {n: k for n, k in ks.items() if "fa_fwd_kvcache_ragged_prefill_kernel" in n}
    assert (len(dense), len(ragged)) == (32, 32) and len(ks) == 64, sorted(ks)
    keys = set()
    for n, k in {**dense, **ragged}.items():
        m = re.search(r"fa_fwd_kvcache_(ragged_)?prefill_kernelI(DF16_|DF16b)Li(\d+)ELb(\d)ELb(\d)ELi(\d)E", n)
        assert m, n
        keys.add(m.groups())
        d = int(m.group(3))
        assert k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 256, (n, k["vgprs"], k["scratch_bytes"])
        assert k["lds_bytes"] == 2 * 2 * 32 * d * 2, (n, k["lds_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        assert main["ds_read_b128"] > 0 and main["ds_read_tr"] > 0 and main["barriers"] > 0, (n, main["label"])
    assert keys == {(r, t, d, c, p, e) for r in (None, "ragged_") for t in ("DF16_", "DF16b") for d in ("64", "128") for c in "01" for p in "01" for e in "12"}
