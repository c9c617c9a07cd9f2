"""CPU: tree attention masks on the decode path (the `tree_mask` keyword of flash_attn_with_kvcache, fa_kvcache_options_v7 of the C ABI) - the
struct layout against the header, the seven accepted struct sizes, a zeroed tail as a v6 call, every refusal with its code and the field it
names, the Python surface's validation, the two mask helpers against plain Python loops, the extension's entry point, and the resources of
the new kernels.  No GPU involved."""
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


def _opt7(**kw):
    o = capi.KvcacheOptionsV7()
    for k, v in kw.items():
        if k in ("reserved", "reserved2", "reserved3"):
            getattr(o, k)[0], getattr(o, k)[1] = v
        else:
            setattr(o, k, v)
    return o


# ---- 1. layout --------------------------------------------------------------------------------------------------------------------------

def test_options_v7_layout_matches_header(tmp_path):
    """fa_kvcache_options .. _v6 keep their sizes; v7 repeats the v6 fields at the same offsets, appends tree_mask, its two strides and
    reserved3[2] and is 240 bytes; ctypes agrees with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheOptionsV7._fields_]
    v6 = [f[0] for f in capi.KvcacheOptionsV6._fields_]
    assert fields[:len(v6)] == v6
    assert fields[len(v6):] == ["tree_mask", "tree_mask_batch_stride", "tree_mask_row_stride", "reserved3"]
    src = tmp_path / "opt7_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_KVCACHE_TREE_MASK\n#error "no FA_HAS_KVCACHE_TREE_MASK"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(fa_kvcache_options_v7), sizeof(fa_kvcache_options_v6), sizeof(fa_kvcache_options_v5), sizeof(fa_kvcache_options_v4), sizeof(fa_kvcache_options_v3), sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options));\n'
                   '    printf("abi %d 0\\n", FA_ABI_VERSION);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options_v7, {f}), sizeof(((fa_kvcache_options_v7*)0)->{f}));\n' for f in fields)
                   + "".join(f'    printf("v6_{f} %zu 0\\n", offsetof(fa_kvcache_options_v6, {f}));\n' for f in v6)
                   + "    fa_kvcache_options_v7 o;\n    FA_PARAMS_INIT(o);\n"
                     "    return o.struct_size == sizeof(o) && o.magic == FA_PARAMS_MAGIC && o.tree_mask == NULL && o.tree_mask_batch_stride == 0 && o.tree_mask_row_stride == 0 "
                     "&& o.reserved3[0] == 0 && o.reserved3[1] == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "opt7_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    sizes = [ctypes.sizeof(c) for c in (capi.KvcacheOptionsV7, capi.KvcacheOptionsV6, capi.KvcacheOptionsV5, capi.KvcacheOptionsV4, capi.KvcacheOptionsV3,
                                        capi.KvcacheOptionsV2, capi.KvcacheOptions)]
    assert got["size"] == sizes == [240, 200, 168, 144, 112, 72, 20]
    assert got["abi"][0] == 4 == capi.lib().fa_abi_version()
    for f in fields:
        assert got[f] == [getattr(capi.KvcacheOptionsV7, f).offset, getattr(capi.KvcacheOptionsV7, f).size], f
    for f in v6:
        assert got["v6_" + f][0] == got[f][0], f
    assert (got["tree_mask"], got["tree_mask_batch_stride"], got["tree_mask_row_stride"], got["reserved3"]) == ([200, 8], [208, 8], [216, 8], [224, 16])


@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_exactly_seven_struct_sizes_are_accepted(fn):
    _, addr = _aligned_addr()
    for size in list(range(8, 20)) + [24, 64, 71, 76, 104, 111, 113, 120, 136, 143, 145, 152, 160, 167, 169, 176, 184, 192, 199, 201, 208, 216, 224, 232, 236, 239, 241, 244,
                                      248, 256, 264, 272, 280, 1024]:
        o = _opt7(tree_mask=addr, tree_mask_row_stride=1)
        o.struct_size = size
        assert _rc(_params(), fn, o) == capi.FA_ERR_BAD_ABI, size
    for size, cls in ((20, capi.KvcacheOptions), (72, capi.KvcacheOptionsV2), (112, capi.KvcacheOptionsV3), (144, capi.KvcacheOptionsV4), (168, capi.KvcacheOptionsV5),
                      (200, capi.KvcacheOptionsV6), (240, capi.KvcacheOptionsV7)):
        assert cls().struct_size == size and _rc(_params(), fn, cls()) >= 0, size
    # a v7 struct that states a shorter size is that shorter struct: the tail is not read
    o = _opt7(tree_mask=addr + 1, reserved3=(7, 7))
    o.struct_size = 200
    assert _rc(_params(), fn, o) >= 0, capi.last_error()


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_v7_with_a_zeroed_tail_is_a_v6_call_and_the_mask_does_not_move_the_split(fn):
    """same split and workspace from a v6 struct, a v7 struct with a zeroed tail, and a v7 struct with a mask pointer - 16-bit and 8-bit cache,
    dense and ragged, with and without a softmax_scale (the shapes of the sinks CPU test; those with more than 64 query rows cannot carry a
    mask and are compared without one)"""
    f = getattr(capi.lib(), fn)
    buf, addr = _aligned_addr()
    masked = 0
    for b, sq, h, hk, cache, causal in SHAPES:
        for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
            for ws in (None, 1 << 40, 3 * b * h * sq * 128 * 4 + (3 * b * h * sq * 4 + 15) // 16 * 16):
                for ragged in (False, True):
                    p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=False, ws_bytes=ws, **kw)
                    if ragged:
                        p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
                    for fp8 in (0, FP8):
                        v6, v7 = capi.KvcacheOptionsV6(), _opt7()
                        opts = [v6, v7]
                        if sq <= 64:
                            opts.append(_opt7(tree_mask=addr, tree_mask_batch_stride=sq, tree_mask_row_stride=1))
                            masked += 1
                        assert (v6.struct_size, v7.struct_size) == (200, 240)
                        for o in opts:
                            o.cache_dtype = fp8
                            o.softmax_scale = 0.37 if cache == 768 else 0.0
                            if ragged:
                                o.cu_seqlens_q, o.total_q = addr, b * sq - 1 + b
                        want = f(ctypes.byref(p), ctypes.byref(v6))
                        assert want >= 0, capi.last_error()
                        for o in opts[1:]:
                            assert f(ctypes.byref(p), ctypes.byref(o)) == want, (b, sq, cache, ws, kw, fp8, ragged, capi.last_error())
                        # a causal v7 call with a zeroed tail is the causal v6 call as well
                        pc = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=True, ws_bytes=ws, **kw)
                        pc.q_stride, pc.o_stride = p.q_stride, p.o_stride
                        assert f(ctypes.byref(pc), ctypes.byref(v7)) == f(ctypes.byref(pc), ctypes.byref(v6)) >= 0
    assert masked > 0


# ---- 2. validation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_tree_option_validation_codes_and_their_order(fn):
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

    T = dict(tree_mask=addr, tree_mask_batch_stride=64, tree_mask_row_stride=1)
    # what is accepted: nothing, a mask under any strides, beside the options it combines with, up to 64 query rows
    for o in (_opt7(), _opt7(**T), _opt7(tree_mask=addr + 8, tree_mask_batch_stride=0, tree_mask_row_stride=0), _opt7(tree_mask=addr + 128, tree_mask_batch_stride=-3, tree_mask_row_stride=-1),
              _opt7(softmax_scale=0.125, **T), _opt7(cache_dtype=FP8, **T), _opt7(is_local=1, window_size_left=-1, window_size_right=-1, **T), _opt7(is_local=0, window_size_left=5, **T),
              _opt7(tree_mask_row_stride=5)):
        for d in (64, 128):
            for sq in (1, 5, 64):
                assert _rc(P(sq=sq, d=d), fn, o) >= 0, capi.last_error()
    assert _rc(R(sq=64), fn, _opt7(cu_seqlens_q=addr, total_q=100, **T)) >= 0, capi.last_error()
    assert _rc(P(sq=4, page=16), fn, _opt7(**T)) >= 0, capi.last_error()
    # without a mask everything is what it was
    assert _rc(P(d=256, sq=100, causal=True), fn, _opt7(softcap=30.0)) >= 0 and _rc(P(sq=65), fn, _opt7(sinks=addr)) >= 0, capi.last_error()
    # a mask pointer that is not 8-byte aligned
    for off in (1, 2, 4, 7):
        assert _rc(P(), fn, _opt7(**dict(T, tree_mask=addr + off))) == STRIDE and "tree_mask" in capi.last_error(), off
    # the refusals, each with the field named
    assert _rc(P(causal=True), fn, _opt7(**T)) == S and "tree_mask" in capi.last_error() and "is_causal" in capi.last_error()
    for win in ((7, 0), (-1, 0), (3, -1), (0, 0)):
        assert _rc(P(), fn, _opt7(is_local=1, window_size_left=win[0], window_size_right=win[1], **T)) == S, win
        assert "tree_mask" in capi.last_error() and "window_size" in capi.last_error(), win
    assert _rc(P(), fn, _opt7(softcap=30.0, **T)) == S and "tree_mask" in capi.last_error() and "softcap" in capi.last_error()
    assert _rc(P(), fn, _opt7(sinks=addr, sinks_stride=1, **T)) == S and "tree_mask" in capi.last_error() and "sinks" in capi.last_error()
    pk = P(sq=2, ws_bytes=1 << 30)                         # (a rotary call keeps the image of the rotated q in the workspace)
    pk.k_new = pk.v_new = pk.cache_seqlens = addr
    pk.seqlen_new = 2
    pk.k_new_stride = pk.v_new_stride = capi.Strides(2 * pk.h_k * pk.d, pk.h_k * pk.d, pk.d)
    rot = dict(rotary_cos=addr, rotary_sin=addr, rotary_row_stride=64, seqlen_ro=32768, rotary_dim=128)
    assert _rc(pk, fn, _opt7(**rot)) >= 0, capi.last_error()
    assert _rc(pk, fn, _opt7(**rot, **T)) == S and "tree_mask" in capi.last_error() and "rotary" in capi.last_error()
    assert _rc(P(d=256), fn, _opt7(**T)) == S and "tree_mask" in capi.last_error() and "256" in capi.last_error()
    for sq in (65, 128, 1000):
        assert _rc(P(sq=sq), fn, _opt7(**T)) == S and "tree_mask" in capi.last_error() and "seqlen_q" in capi.last_error() and "64" in capi.last_error(), sq
    assert _rc(R(sq=65), fn, _opt7(cu_seqlens_q=addr, total_q=100, **T)) == S and "max_seqlen_q" in capi.last_error()
    # a non-zero reserved word is a newer caller's field
    for r in ((1, 0), (0, 1), (-1, 0), (0, 1 << 40)):
        assert _rc(P(), fn, _opt7(reserved3=r)) == ABI and "reserved3" in capi.last_error(), r
        assert _rc(P(), fn, _opt7(reserved3=r, **T)) == ABI and "reserved3" in capi.last_error(), r
    # the order: params first, then the older option fields (their reserved words among them), then the mask, then reserved3
    bad7 = dict(tree_mask=addr + 4, reserved3=(1, 1))
    assert _rc(P(h=3, hk=2), fn, _opt7(**bad7)) == capi.FA_ERR_BAD_GQA
    assert _rc(P(sq=0), fn, _opt7(**bad7)) == S and "seqlen_q" in capi.last_error() and "tree_mask" not in capi.last_error()
    assert _rc(P(), fn, _opt7(cache_dtype=9, **bad7)) == capi.FA_ERR_BAD_DTYPE
    assert _rc(P(), fn, _opt7(is_local=1, window_size_left=-2, **bad7)) == S and "tree_mask" not in capi.last_error()
    assert _rc(P(), fn, _opt7(softmax_scale=-1.0, **bad7)) == S and "softmax_scale" in capi.last_error()
    assert _rc(P(), fn, _opt7(sinks=addr + 2, **bad7)) == STRIDE and "sinks" in capi.last_error() and "tree_mask" not in capi.last_error()
    assert _rc(P(), fn, _opt7(reserved2=(1, 0), **bad7)) == ABI and "fa_kvcache_options_v6" in capi.last_error()
    assert _rc(P(), fn, _opt7(**bad7)) == STRIDE and "tree_mask" in capi.last_error()
    assert _rc(P(causal=True), fn, _opt7(tree_mask=addr, reserved3=(1, 1))) == S and "is_causal" in capi.last_error()
    assert _rc(P(), fn, _opt7(tree_mask=addr, reserved3=(1, 1))) == ABI


def test_plain_c_caller_uses_the_v7_struct(tmp_path):
    src = tmp_path / "use_tree.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
static _Alignas(16) char mem[256];
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = mem; p.lse = (float*)mem; p.cache_seqlens = (const int32_t*)mem;
    p.b = 4; p.seqlen_q = 8; p.seqlen_cache = 32768; p.h = 64; p.h_k = 8; p.d = 64; p.dtype = FA_BF16; p.num_splits = 4;
    p.q_stride = p.o_stride = (fa_strides){8 * 64 * 64, 64 * 64, 64};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 64, 8 * 64, 64};
    fa_kvcache_options_v6 o6;
    FA_PARAMS_INIT(o6);
    fa_kvcache_options_v7 o7;
    FA_PARAMS_INIT(o7);
    if (sizeof(o7) != 240) return 9;
    long long dense = fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o6);
    if (dense != 4LL * (4 * 64 * 8) * 64 * 4 + 4LL * (4 * 64 * 8) * 4) return 10;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o7) != dense) return 11;      /* zeroed tail: the v6 call */
    o7.tree_mask = (const int64_t*)mem; o7.tree_mask_batch_stride = 8; o7.tree_mask_row_stride = 1;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o7) != dense) return 12;      /* the mask does not move the workspace */
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o7) != 1) return 13;               /* (no workspace in the params) */
    p.is_causal = 1;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o7) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "tree_mask")) return 14;
    p.is_causal = 0; o7.tree_mask = (const int64_t*)(mem + 4);
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o7) != FA_ERR_BAD_STRIDE || !strstr(fa_last_error(), "tree_mask")) return 15;
    o7.tree_mask = (const int64_t*)mem; o7.reserved3[1] = 1;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o7) != FA_ERR_BAD_ABI) return 16;
    o7.reserved3[1] = 0; p.seqlen_q = 65;
    p.q_stride = p.o_stride = (fa_strides){65 * 64 * 64, 64 * 64, 64};
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o7) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "seqlen_q")) return 17;
    p.b = 0; p.seqlen_q = 8;
    if (fa_run_mha_fwd_kvcache_ex(&p, (const fa_kvcache_options*)&o7, NULL) != FA_OK) return 18;      /* nothing to do: no launch */
    return 0;
}
""")
    exe = tmp_path / "use_tree"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_capi_helper_builds_the_v7_struct_only_when_asked():
    words = torch.arange(48, dtype=torch.int64).view(4, 12)
    o = capi.kvcache_options(tree_mask=words[:, ::2])
    assert isinstance(o, capi.KvcacheOptionsV7) and o.struct_size == 240
    assert (o.tree_mask, o.tree_mask_batch_stride, o.tree_mask_row_stride, o.reserved3[0], o.reserved3[1], o.sinks, o.softcap, o.is_local) == (words.data_ptr(), 12, 2, 0, 0, None, 0.0, 0)
    o = capi.kvcache_options(cache_dtype=FP8, softmax_scale=0.25, tree_mask=words.view(-1)[3::5])
    assert isinstance(o, capi.KvcacheOptionsV7)
    assert (o.tree_mask, o.tree_mask_batch_stride, o.tree_mask_row_stride, o.softmax_scale, o.cache_dtype) == (words.data_ptr() + 24, 0, 5, 0.25, FP8)
    # without the keyword every call keeps the struct it had
    assert type(capi.kvcache_options(sinks=torch.zeros(8))) is capi.KvcacheOptionsV6 and type(capi.kvcache_options(softcap=30.0)) is capi.KvcacheOptionsV5
    assert type(capi.kvcache_options((3, 0))) is capi.KvcacheOptions and type(capi.kvcache_options()) is capi.KvcacheOptions
    p = _params(ws_bytes=1 << 40, h=8, hk=8, sq=4)
    assert capi.kvcache_num_splits(p, capi.kvcache_options(tree_mask=words[:1, :4])) == capi.kvcache_num_splits(p, capi.kvcache_options())
    assert capi.kvcache_workspace_bytes(p, capi.kvcache_options(tree_mask=words[:1, :4])) == capi.kvcache_workspace_bytes(p, capi.kvcache_options())


# ---- 3. the Python surface and the extension --------------------------------------------------------------------------------------------

def test_python_surface_rejects_bad_tree_masks():
    import flash_attn_turing as F

    b, sq, h, hk, d, cap = 2, 5, 4, 2, 64, 32
    q = torch.zeros(b, sq, h, d, dtype=torch.float16)
    kc = torch.zeros(b, cap, hk, d, dtype=torch.float16)
    good = torch.zeros(b, sq, dtype=torch.int64)

    def call(**kw):
        return F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=8, **kw)

    # non-tensors, dtype, rank, shape, device (the meta device stands for "another device" here)
    for bad in (0, [[0] * sq] * b, "tree", True, good.numpy(), good.int(), good.float(), good.bool(), good.to(torch.uint8), torch.zeros((), dtype=torch.int64),
                torch.zeros(sq, dtype=torch.int64), torch.zeros(b * sq, dtype=torch.int64), torch.zeros(b, sq, 1, dtype=torch.int64), torch.zeros(b, sq + 1, dtype=torch.int64),
                torch.zeros(b + 1, sq, dtype=torch.int64), torch.zeros(sq, b, dtype=torch.int64), torch.zeros(b, sq, sq, dtype=torch.int64),
                torch.zeros(b, sq, dtype=torch.int64, device="meta")):
        with pytest.raises(ValueError, match="tree_mask"):
            call(tree_mask=bad)
        with pytest.raises(ValueError, match="tree_mask"):
            call(tree_mask=bad, num_splits=3, softmax_scale=0.5)
    # the refusals
    with pytest.raises(ValueError, match="tree_mask together with causal"):
        call(tree_mask=good, causal=True)
    for win in ((7, 0), (-1, 0), (3, -1)):
        with pytest.raises(ValueError, match="tree_mask together with window_size"):
            call(tree_mask=good, window_size=win)
    with pytest.raises(ValueError, match="tree_mask together with softcap"):
        call(tree_mask=good, softcap=30.0)
    with pytest.raises(ValueError, match="tree_mask together with sinks"):
        call(tree_mask=good, sinks=torch.zeros(h))
    kn = torch.zeros(b, sq, hk, d, dtype=torch.float16)
    cos = torch.zeros(cap, 16, dtype=torch.float16)
    with pytest.raises(ValueError, match="tree_mask together with rotary"):
        F.flash_attn_with_kvcache(q, kc, kc, k=kn, v=kn, cache_seqlens=8, rotary_cos=cos, rotary_sin=cos, tree_mask=good)
    q256, kc256 = torch.zeros(b, sq, h, 256, dtype=torch.float16), torch.zeros(b, cap, hk, 256, dtype=torch.float16)
    with pytest.raises(ValueError, match="tree_mask at head_dim 256"):
        F.flash_attn_with_kvcache(q256, kc256, kc256, cache_seqlens=8, tree_mask=good)
    q65, kc128 = torch.zeros(b, 65, h, d, dtype=torch.float16), torch.zeros(b, 128, hk, d, dtype=torch.float16)
    with pytest.raises(ValueError, match="at most 64"):
        F.flash_attn_with_kvcache(q65, kc128, kc128, cache_seqlens=8, tree_mask=torch.zeros(b, 65, dtype=torch.int64))
    # ragged: (total_q,), max_seqlen_q at most 64
    qr = torch.zeros(7, h, d, dtype=torch.float16)
    cu = torch.tensor([0, 2, 7], dtype=torch.int32)
    for bad in (torch.zeros(6, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), torch.zeros(2, 5, dtype=torch.int64), torch.zeros(7, dtype=torch.int32)):
        with pytest.raises(ValueError, match="tree_mask"):
            F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=8, cu_seqlens_q=cu, max_seqlen_q=5, tree_mask=bad)
    with pytest.raises(ValueError, match="at most 64"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=8, cu_seqlens_q=cu, max_seqlen_q=65, tree_mask=torch.zeros(7, dtype=torch.int64))
    # keyword-only
    with pytest.raises(TypeError):
        F.flash_attn_with_kvcache(q, kc, kc, None, None, 8, False, 0, False, good)
    # a CPU call that passes the checks is still refused by the extension (no quiet fall-back): contiguous, strided, sq = 64, ragged, and no mask at all
    for kw in (dict(tree_mask=good), dict(tree_mask=torch.zeros(sq, 2 * b, dtype=torch.int64).t()[::2]), dict(tree_mask=good, num_splits=3, softmax_scale=0.125),
               dict(tree_mask=good, window_size=(-1, -1), softcap=0.0, causal=False), dict(tree_mask=None), dict()):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**kw)
    q64 = torch.zeros(b, 64, h, d, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(q64, kc128, kc128, cache_seqlens=8, tree_mask=torch.zeros(b, 64, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=8, cu_seqlens_q=cu, max_seqlen_q=64, tree_mask=torch.zeros(9, dtype=torch.int64)[:7])
    doc = F.flash_attn_with_kvcache.__doc__
    assert "tree_mask" in doc and "BIT FOR BIT" in doc and "pack_tree_mask" in doc and "tree_mask_from_parents" in doc
    assert "pack_tree_mask" in F.__all__ and "tree_mask_from_parents" in F.__all__


def test_extension_takes_tree_mask_on_a_function_of_its_own():
    from flash_attn_turing import _C

    doc = _C.fwd_kvcache.__doc__
    assert "3. fwd_kvcache(" in doc and "4. fwd_kvcache(" not in doc and "tree_mask" not in doc
    assert "tree_mask" not in _C.fwd_kvcache_sinks.__doc__
    tdoc = _C.fwd_kvcache_tree.__doc__
    sig = tdoc[:tdoc.index("->")]
    assert re.search(r"sinks: [^,]*= None, tree_mask: [^,]*= None\)", sig), sig
    assert sig.index("*, k_descale") < sig.index("softmax_scale") < sig.index(", sinks:") < sig.index(", tree_mask:")        # keyword-only
    # it continues fwd_kvcache_sinks argument for argument
    names = lambda s: re.findall(r"(\w+): ", s[s.index("("):])
    sdoc = _C.fwd_kvcache_sinks.__doc__
    n6, n7 = names(sdoc[:sdoc.index("->")]), names(sig)
    assert n7[:len(n6)] == n6 and n7[len(n6):] == ["tree_mask"], (n6, n7)
    q = torch.zeros(2, 3, 4, 64, dtype=torch.float16)
    kc = torch.zeros(2, 32, 2, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        _C.fwd_kvcache_tree(q, kc, kc, tree_mask=torch.zeros(2, 3, dtype=torch.int64))


# ---- 4. the helpers ---------------------------------------------------------------------------------------------------------------------

def _wrap64(x):
    """a Python int of 64 bits as the int64 that holds those bits"""
    return x - (1 << 64) if x >= (1 << 63) else x


def _pack_loop(mask):
    sq = len(mask)
    return [_wrap64(sum(1 << u for u in range(sq) if mask[t][u])) for t in range(sq)]


def _parents_loop(parents):
    out = []
    for t, p in enumerate(parents):
        w, a = 1 << t, p
        while a >= 0:
            w |= 1 << a
            a = parents[a]
        out.append(_wrap64(w))
    return out


def test_pack_tree_mask_against_a_python_loop():
    import flash_attn_turing as F

    gen = torch.Generator().manual_seed(5)
    for sq in (1, 2, 5, 17, 63, 64):
        m = torch.rand(sq, sq, generator=gen) < 0.5
        m[sq - 1, sq - 1] = True                             # (sq = 64: bit 63 of the last row, the sign bit)
        got = F.pack_tree_mask(m)
        assert got.dtype == torch.int64 and got.shape == (sq,)
        assert got.tolist() == _pack_loop(m.tolist()), sq
    full = torch.ones(64, 64, dtype=torch.bool)
    assert F.pack_tree_mask(full).tolist() == [-1] * 64
    only63 = torch.zeros(64, 64, dtype=torch.bool)
    only63[63, 63] = True
    w = F.pack_tree_mask(only63)
    assert w[63].item() == -(1 << 63) and (w[:63] == 0).all().item()
    tri = torch.tril(torch.ones(64, 64, dtype=torch.bool))
    assert F.pack_tree_mask(tri).tolist() == [_wrap64((1 << (t + 1)) - 1) for t in range(64)]
    # leading dimensions, a strided view
    m = torch.rand(3, 2, 9, 9, generator=gen) < 0.5
    got = F.pack_tree_mask(m)
    assert got.shape == (3, 2, 9)
    for i in range(3):
        for j in range(2):
            assert got[i, j].tolist() == _pack_loop(m[i, j].tolist())
    assert F.pack_tree_mask(m.transpose(-1, -2))[1, 1].tolist() == _pack_loop(m[1, 1].t().tolist())
    for bad in (torch.zeros(3, 3), torch.zeros(3, 4, dtype=torch.bool), torch.zeros(65, 65, dtype=torch.bool), torch.zeros(4, dtype=torch.bool), [[True]]):
        with pytest.raises(ValueError):
            F.pack_tree_mask(bad)


def test_tree_mask_from_parents_against_a_python_loop():
    import flash_attn_turing as F

    heap = [(t - 1) // 2 if t else -1 for t in range(64)]
    chain = [t - 1 for t in range(64)]
    forest = [-1, -1, 0, 1, -1, 2, 2, 4, 3, -1, 9, 7]          # several roots, branching, a lone root
    gen = torch.Generator().manual_seed(6)
    rand = [-1] + [int(torch.randint(-1, t, (1,), generator=gen)) for t in range(1, 40)]
    for parents in (heap, chain, forest, rand, [-1], [-1] * 7, heap[:8], heap[:32]):
        for dt in (torch.int64, torch.int32):
            got = F.tree_mask_from_parents(torch.tensor(parents, dtype=dt))
            assert got.dtype == torch.int64 and got.tolist() == _parents_loop(parents), parents
    # the chain is the lower triangle; its last word at sq = 64 has every bit, the sign bit included
    assert F.tree_mask_from_parents(torch.tensor(chain)).tolist() == [_wrap64((1 << (t + 1)) - 1) for t in range(64)]
    assert F.tree_mask_from_parents(torch.tensor(chain))[63].item() == -1
    assert F.tree_mask_from_parents(torch.tensor(heap))[63].item() < 0           # node 63 sees itself: bit 63
    # it agrees with pack_tree_mask on the ancestor matrix
    for parents in (heap, forest):
        sq = len(parents)
        m = torch.zeros(sq, sq, dtype=torch.bool)
        for t in range(sq):
            a = t
            while a >= 0:
                m[t, a] = True
                a = parents[a]
        assert torch.equal(F.tree_mask_from_parents(torch.tensor(parents)), F.pack_tree_mask(m))
    # batched
    both = torch.tensor([heap[:12], forest])
    got = F.tree_mask_from_parents(both)
    assert got.shape == (2, 12) and got[0].tolist() == _parents_loop(heap[:12]) and got[1].tolist() == _parents_loop(forest)
    for bad in (torch.zeros(4), torch.zeros(65, dtype=torch.int64), torch.zeros((), dtype=torch.int64), [0, 1], torch.zeros(3, dtype=torch.bool)):
        with pytest.raises(ValueError):
            F.tree_mask_from_parents(bad)


# ---- 5. ISA -----------------------------------------------------------------------------------------------------------------------------

def _check_tree_unit(ks):
    dense = {n: k for n, k in ks.items() if "fa_fwd_kvcache_tree_kernel" in n}
    ragged = {n: k for n, k in ks.items() if "fa_fwd_kvcache_ragged_tree_kernel" in n}
    assert (len(dense), len(ragged)) == (16, 16) and len(ks) == 32, sorted(ks)
    keys = set()
    for n, k in {**dense, **ragged}.items():
        m = re.search(r"fa_fwd_kvcache_(ragged_)?tree_kernelI(DF16_|DF16b)Li(\d+)ELb(\d)ELi(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 256, (n, k["vgprs"], k["scratch_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
    assert keys == {(r, t, d, p, e) for r in (None, "ragged_") for t in ("DF16_", "DF16b") for d in ("64", "128") for p in "01" for e in "12"}


def test_tree_kernels_isa():
    """32 attention kernels ({fp16, bf16} x {64, 128} x {contiguous, paged} x {16-bit, FP8} x {dense, ragged}) and nothing else - no append, no
    combine, no second copy of an existing kernel.  No scratch, two workgroups per CU as the launch bounds ask (VGPRs <= 256, no AGPRs, 2 x LDS
    <= 160 KiB), an MFMA loop free of scratch traffic and accumulator moves, no MFMA hazard, M0 untouched."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_kvcache_tree.hip" in B.HIP_SOURCES and "fa_fwd_kvcache_tree.hip" in B.M0_GUARD_SOURCES
    src = open(os.path.join(B.CSRC, "fa_fwd_kvcache_tree.hip")).read()
    assert src.count("__launch_bounds__(kKvcThreads, 2)") == 2
    _check_tree_unit(analyse("fa_fwd_kvcache_tree.hip"))


def test_tree_uniform_branch_variant_isa():
    """-DFA_KVC_TREE_UNIFORM=1 (the A / B build of DESIGN.md 3.11): the same 32 kernels under the same limits"""
    from _kernel_isa import analyse

    _check_tree_unit(analyse("fa_fwd_kvcache_tree.hip", extra_flags=["-DFA_KVC_TREE_UNIFORM=1"]))
