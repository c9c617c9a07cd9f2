"""CPU: attention sinks on the decode path (the `sinks` keyword of flash_attn_with_kvcache, fa_kvcache_options_v6 of the C ABI) - the struct
layout against the header, a zeroed tail as a v5 call, the accepted struct sizes, validation codes and their order before any device work,
the two refusals (soft cap, head_dim 256), a plain C caller, the capi helper, the Python surface's validation, the extension's entry point,
and the ISA of the new kernels.  No GPU involved."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi
from test_kvcache_softcap_cpu import SHAPES, WINDOWS
from test_kvcache_window_cpu import EX_ENTRY_POINTS, _aligned_addr, _params, _rc

FP8 = capi.FA_CACHE_FP8_E4M3
NAN, INF = float("nan"), float("inf")


def _opt6(**kw):
    o = capi.KvcacheOptionsV6()
    for k, v in kw.items():
        if k in ("reserved", "reserved2"):
            getattr(o, k)[0], getattr(o, k)[1] = v
        else:
            setattr(o, k, v)
    return o


# ---- 1. layout --------------------------------------------------------------------------------------------------------------------------

def test_options_v6_layout_matches_header(tmp_path):
    """fa_kvcache_options .. _v5 keep their sizes (20, 72, 112, 144, 168); v6 repeats the v5 fields at the same offsets, appends sinks,
    sinks_stride and reserved2[2] and is 200 bytes; ctypes agrees with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheOptionsV6._fields_]
    v5 = [f[0] for f in capi.KvcacheOptionsV5._fields_]
    assert fields[:len(v5)] == v5
    assert fields[len(v5):] == ["sinks", "sinks_stride", "reserved2"]
    src = tmp_path / "opt6_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_KVCACHE_SINKS\n#error "no FA_HAS_KVCACHE_SINKS"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu %zu %zu %zu %zu\\n", sizeof(fa_kvcache_options_v6), sizeof(fa_kvcache_options_v5), sizeof(fa_kvcache_options_v4), sizeof(fa_kvcache_options_v3), sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options));\n'
                   '    printf("abi %d 0\\n", FA_ABI_VERSION);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options_v6, {f}), sizeof(((fa_kvcache_options_v6*)0)->{f}));\n' for f in fields)
                   + "".join(f'    printf("v5_{f} %zu 0\\n", offsetof(fa_kvcache_options_v5, {f}));\n' for f in v5)
                   + "    fa_kvcache_options_v6 o;\n    FA_PARAMS_INIT(o);\n"
                     "    return o.struct_size == sizeof(o) && o.magic == FA_PARAMS_MAGIC && o.sinks == NULL && o.sinks_stride == 0 && o.reserved2[0] == 0 && o.reserved2[1] == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "opt6_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    sizes = [ctypes.sizeof(c) for c in (capi.KvcacheOptionsV6, capi.KvcacheOptionsV5, capi.KvcacheOptionsV4, capi.KvcacheOptionsV3, capi.KvcacheOptionsV2, capi.KvcacheOptions)]
    assert got["size"] == sizes == [200, 168, 144, 112, 72, 20]
    assert got["abi"][0] == 4 == capi.lib().fa_abi_version()
    for f in fields:
        assert got[f] == [getattr(capi.KvcacheOptionsV6, f).offset, getattr(capi.KvcacheOptionsV6, f).size], f
    for f in v5:
        assert got["v5_" + f][0] == got[f][0], f
    assert (got["sinks"], got["sinks_stride"], got["reserved2"]) == ([168, 8], [176, 8], [184, 16])


@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_exactly_six_struct_sizes_are_accepted(fn):
    _, addr = _aligned_addr()
    for size in list(range(8, 20)) + [24, 28, 40, 64, 71, 76, 80, 96, 104, 108, 111, 113, 116, 120, 128, 136, 140, 143, 145, 148, 152, 160, 164, 167, 169, 172, 176, 184,
                                      192, 196, 199, 201, 204, 208, 216, 224, 232, 256, 1024]:
        o = _opt6(sinks=addr, sinks_stride=1)
        o.struct_size = size
        assert _rc(_params(), fn, o) == capi.FA_ERR_BAD_ABI, size
    for size, cls in ((20, capi.KvcacheOptions), (72, capi.KvcacheOptionsV2), (112, capi.KvcacheOptionsV3), (144, capi.KvcacheOptionsV4), (168, capi.KvcacheOptionsV5),
                      (200, capi.KvcacheOptionsV6)):
        assert cls().struct_size == size and _rc(_params(), fn, cls()) >= 0, size
    # a v6 struct that states a shorter size is that shorter struct: the tail is not read
    o = _opt6(sinks=addr + 1, reserved2=(7, 7))
    o.struct_size = 168
    assert _rc(_params(), fn, o) >= 0, capi.last_error()


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_v6_with_a_zeroed_tail_is_a_v5_call_and_sinks_do_not_move_the_split(fn):
    """same split and workspace from a v5 struct, a v6 struct with a zeroed tail, and a v6 struct with sinks - 16-bit and 8-bit cache, with and
    without a window, dense and ragged, with and without a softmax_scale"""
    f = getattr(capi.lib(), fn)
    buf, addr = _aligned_addr()
    for b, sq, h, hk, cache, causal in SHAPES:
        for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
            for ws in (None, 1 << 40, 3 * b * h * sq * 128 * 4 + (3 * b * h * sq * 4 + 15) // 16 * 16):
                for ragged in (False, True):
                    p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, ws_bytes=ws, **kw)
                    if ragged:
                        p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
                    for win in WINDOWS:
                        for fp8 in (0, FP8):
                            v5, v6, v6s = capi.KvcacheOptionsV5(), _opt6(), _opt6(sinks=addr, sinks_stride=3)
                            assert (v5.struct_size, v6.struct_size) == (168, 200)
                            for o in (v5, v6, v6s):
                                o.is_local, o.window_size_left, o.window_size_right, o.cache_dtype = int(win != (-1, -1)), win[0], win[1], fp8
                                o.softmax_scale = 0.37 if cache == 768 else 0.0
                                if ragged:
                                    o.cu_seqlens_q, o.total_q = addr, b * sq - 1 + b
                            want = f(ctypes.byref(p), ctypes.byref(v5))
                            assert want >= 0, capi.last_error()
                            assert f(ctypes.byref(p), ctypes.byref(v6)) == want, (b, sq, cache, ws, kw, win, fp8, ragged)
                            assert f(ctypes.byref(p), ctypes.byref(v6s)) == want, (b, sq, cache, ws, kw, win, fp8, ragged)


# ---- 2. validation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_sink_option_validation_codes_and_their_order(fn):
    buf, addr = _aligned_addr()
    S, ABI, STRIDE = capi.FA_ERR_BAD_SHAPE, capi.FA_ERR_BAD_ABI, capi.FA_ERR_BAD_STRIDE

    def P(**kw):
        p = _params(**kw)
        if fn == "fa_run_mha_fwd_kvcache_ex":
            p.b = 0                                          # (validated, launches nothing: the addresses are dummies)
        return p

    # what is accepted: nothing, sinks under any stride (0 broadcasts one logit, a negative one walks backwards), beside every older option
    for o in (_opt6(), _opt6(sinks=addr), _opt6(sinks=addr, sinks_stride=1), _opt6(sinks=addr + 4, sinks_stride=7), _opt6(sinks=addr + 128, sinks_stride=-1),
              _opt6(sinks=addr, sinks_stride=1, softmax_scale=0.125), _opt6(sinks=addr, sinks_stride=1, cache_dtype=FP8),
              _opt6(sinks=addr, sinks_stride=1, is_local=1, window_size_left=127, window_size_right=0), _opt6(sinks=addr, sinks_stride=1, cu_seqlens_q=addr, total_q=64),
              _opt6(sinks_stride=5)):
        for d in (64, 128):
            p = P(sq=4, d=d)
            if o.cu_seqlens_q:
                p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
            assert _rc(p, fn, o) >= 0, capi.last_error()
    # without sinks head_dim 256 and the soft cap are what they were
    assert _rc(P(d=256), fn, _opt6()) >= 0 and _rc(P(d=256), fn, _opt6(softcap=30.0)) >= 0 and _rc(P(), fn, _opt6(softcap=30.0)) >= 0, capi.last_error()
    # a sink pointer that is not 4-byte aligned
    for off in (1, 2, 3):
        assert _rc(P(), fn, _opt6(sinks=addr + off, sinks_stride=1)) == STRIDE and "sinks" in capi.last_error(), off
    # the two refusals, the field named
    assert _rc(P(), fn, _opt6(sinks=addr, sinks_stride=1, softcap=30.0)) == S and "sinks" in capi.last_error() and "softcap" in capi.last_error()
    assert _rc(P(d=256), fn, _opt6(sinks=addr, sinks_stride=1)) == S and "sinks" in capi.last_error() and "256" in capi.last_error()
    # a non-zero reserved word is a newer caller's field
    for r in ((1, 0), (0, 1), (-1, 0), (0, 1 << 40)):
        assert _rc(P(), fn, _opt6(reserved2=r)) == ABI and "reserved2" in capi.last_error(), r
        assert _rc(P(), fn, _opt6(sinks=addr, sinks_stride=1, reserved2=r)) == ABI and "reserved2" in capi.last_error(), r
    # the order: params first, then the older option fields (the v5 reserved words among them), then sinks, then reserved2
    bad6 = dict(sinks=addr + 2, reserved2=(1, 1))
    assert _rc(P(h=3, hk=2), fn, _opt6(**bad6)) == capi.FA_ERR_BAD_GQA
    assert _rc(P(sq=0), fn, _opt6(**bad6)) == S and "seqlen_q" in capi.last_error()
    assert _rc(P(), fn, _opt6(cache_dtype=9, **bad6)) == capi.FA_ERR_BAD_DTYPE
    assert _rc(P(), fn, _opt6(is_local=1, window_size_left=-2, **bad6)) == S and "window_size" in capi.last_error()
    assert _rc(P(), fn, _opt6(rotary_cos=addr, **bad6)) == S and "rotary" in capi.last_error()
    p = P()
    p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
    assert _rc(p, fn, _opt6(cu_seqlens_q=addr, total_q=-1, **bad6)) == S and "total_q" in capi.last_error()
    assert _rc(P(), fn, _opt6(softmax_scale=-1.0, **bad6)) == S and "softmax_scale" in capi.last_error()
    assert _rc(P(), fn, _opt6(softcap=NAN, **bad6)) == S and "softcap" in capi.last_error() and "sinks" not in capi.last_error()
    assert _rc(P(), fn, _opt6(reserved=(1, 0), **bad6)) == ABI and "fa_kvcache_options_v5" in capi.last_error()
    assert _rc(P(), fn, _opt6(**bad6)) == STRIDE and "sinks" in capi.last_error()
    assert _rc(P(), fn, _opt6(sinks=addr, softcap=2.0, reserved2=(1, 1))) == S and "softcap" in capi.last_error()
    assert _rc(P(d=256), fn, _opt6(sinks=addr, reserved2=(1, 1))) == S and "256" in capi.last_error()
    assert _rc(P(), fn, _opt6(sinks=addr, reserved2=(1, 1))) == ABI


def test_plain_c_caller_uses_the_v6_struct(tmp_path):
    src = tmp_path / "use_sinks.c"
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
    fa_kvcache_options_v5 o5;
    FA_PARAMS_INIT(o5);
    fa_kvcache_options_v6 o6;
    FA_PARAMS_INIT(o6);
    if (sizeof(o6) != 200) return 9;
    long long dense = fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o5);
    if (dense != 4LL * (4 * 64 * 8) * 64 * 4 + 4LL * (4 * 64 * 8) * 4) return 10;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o6) != dense) return 11;      /* zeroed tail: the v5 call */
    o6.sinks = (const float*)mem; o6.sinks_stride = 1; o6.is_local = 1; o6.window_size_left = 127; o6.window_size_right = 0;
    o5.is_local = 1; o5.window_size_left = 127; o5.window_size_right = 0;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o6) != fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o5)) return 12;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o6) != 1) return 13;               /* (no workspace in the params) */
    o6.softcap = 50.0f;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o6) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "sinks")) return 14;
    o6.softcap = 0.0f; o6.sinks = (const float*)(mem + 2);
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o6) != FA_ERR_BAD_STRIDE || !strstr(fa_last_error(), "sinks")) return 15;
    o6.sinks = (const float*)mem; o6.reserved2[1] = 1;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o6) != FA_ERR_BAD_ABI) return 16;
    o6.reserved2[1] = 0; p.d = 256;
    p.q_stride = p.o_stride = (fa_strides){8 * 64 * 256, 64 * 256, 256};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 256, 8 * 256, 256};
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o6) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "256")) return 17;
    p.b = 0; p.d = 64;
    if (fa_run_mha_fwd_kvcache_ex(&p, (const fa_kvcache_options*)&o6, NULL) != FA_OK) return 18;      /* nothing to do: no launch */
    return 0;
}
""")
    exe = tmp_path / "use_sinks"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_capi_helper_builds_the_v6_struct_only_when_asked():
    sinks = torch.arange(16, dtype=torch.float32)
    o = capi.kvcache_options(sinks=sinks[::2])
    assert isinstance(o, capi.KvcacheOptionsV6) and o.struct_size == 200
    assert (o.sinks, o.sinks_stride, o.reserved2[0], o.reserved2[1], o.softmax_scale, o.softcap, o.is_local, o.cache_dtype) == (sinks.data_ptr(), 2, 0, 0, 0.0, 0.0, 0, 0)
    o = capi.kvcache_options((127, 0), cache_dtype=FP8, softmax_scale=0.25, sinks=sinks[3:11])
    assert isinstance(o, capi.KvcacheOptionsV6)
    assert (o.sinks, o.sinks_stride, o.softmax_scale, o.is_local, o.window_size_left, o.cache_dtype) == (sinks.data_ptr() + 12, 1, 0.25, 1, 127, FP8)
    # without the keyword every call keeps the struct it had
    assert type(capi.kvcache_options(softcap=30.0)) is capi.KvcacheOptionsV5 and type(capi.kvcache_options(softmax_scale=0.1)) is capi.KvcacheOptionsV5
    cu = torch.tensor([0, 1, 2], dtype=torch.int32)
    assert type(capi.kvcache_options(cu_seqlens_q=cu, total_q=2)) is capi.KvcacheOptionsV4
    assert type(capi.kvcache_options((3, 0))) is capi.KvcacheOptions and type(capi.kvcache_options(cache_dtype=FP8)) is capi.KvcacheOptionsV2
    assert type(capi.kvcache_options()) is capi.KvcacheOptions
    p = _params(ws_bytes=1 << 40, h=8, hk=8)
    assert capi.kvcache_num_splits(p, capi.kvcache_options(sinks=sinks[:8])) == capi.kvcache_num_splits(p, capi.kvcache_options())
    assert capi.kvcache_workspace_bytes(p, capi.kvcache_options(sinks=sinks[:8])) == capi.kvcache_workspace_bytes(p, capi.kvcache_options())


# ---- 3. the Python surface and the extension --------------------------------------------------------------------------------------------

def test_python_surface_rejects_bad_sinks():
    import flash_attn_turing as F

    b, h, hk, d, cap = 2, 4, 2, 64, 32
    q = torch.zeros(b, 1, h, d, dtype=torch.float16)
    kc = torch.zeros(b, cap, hk, d, dtype=torch.float16)
    good = torch.zeros(h)

    def call(**kw):
        return F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=4, **kw)

    # rank, length, dtype, device (the meta device stands for "another device" here), non-tensors
    for bad in (torch.zeros(()), torch.zeros(h, 1), torch.zeros(1, h), torch.zeros(h + 1), torch.zeros(h - 1), torch.zeros(hk), torch.zeros(0),
                torch.zeros(h, dtype=torch.float64), torch.zeros(h, dtype=torch.bfloat16), torch.zeros(h, dtype=torch.int32), torch.zeros(h, device="meta"),
                0.0, 1, [0.0] * h, (0.0,) * h, "sinks", True, good.numpy()):
        with pytest.raises(ValueError, match="sinks"):
            call(sinks=bad)
        with pytest.raises(ValueError, match="sinks"):
            call(sinks=bad, causal=True, window_size=(7, 0), num_splits=3)
    # the two refusals
    with pytest.raises(ValueError, match="sinks together with softcap"):
        call(sinks=good, softcap=30.0)
    q256, kc256 = torch.zeros(b, 1, h, 256, dtype=torch.float16), torch.zeros(b, cap, hk, 256, dtype=torch.float16)
    with pytest.raises(ValueError, match="sinks at head_dim 256"):
        F.flash_attn_with_kvcache(q256, kc256, kc256, cache_seqlens=4, sinks=good)
    # keyword-only
    with pytest.raises(TypeError):
        F.flash_attn_with_kvcache(q, kc, kc, None, None, 4, False, 0, False, good)
    # a sinks that requires grad hits the forward-only error
    with pytest.raises(RuntimeError, match="forward-only"):
        call(sinks=torch.zeros(h, requires_grad=True))
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        call(sinks=torch.zeros(h, requires_grad=True))
    # a CPU call that passes the checks is still refused by the extension (no quiet fall-back): float32, q's dtype, a strided view, with the older keywords
    for kw in (dict(sinks=good), dict(sinks=good.half()), dict(sinks=torch.zeros(2 * h)[::2]), dict(sinks=good, softmax_scale=0.125), dict(sinks=good, softcap=0.0),
               dict(sinks=good, causal=True, window_size=(127, 0)), dict(sinks=good, num_splits=3), dict(sinks=None), dict()):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**kw)
    qr = torch.zeros(3, h, d, dtype=torch.float16)
    cu = torch.tensor([0, 1, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=4, cu_seqlens_q=cu, max_seqlen_q=2, sinks=good)
    with pytest.raises(ValueError, match="sinks"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=4, cu_seqlens_q=cu, max_seqlen_q=2, sinks=torch.zeros(h + 1))
    doc = F.flash_attn_with_kvcache.__doc__
    assert "sinks" in doc and "INCLUDES the sink" in doc


def test_extension_takes_sinks_on_a_function_of_its_own_and_fwd_kvcache_keeps_its_three_overloads():
    from flash_attn_turing import _C

    doc = _C.fwd_kvcache.__doc__
    assert "3. fwd_kvcache(" in doc and "4. fwd_kvcache(" not in doc and "sinks" not in doc
    sdoc = _C.fwd_kvcache_sinks.__doc__
    sig = sdoc[:sdoc.index("->")]
    assert re.search(r"softmax_scale: [^,]*= None, softcap: [^,]*[Ff]loat = 0\.0, sinks: [^,]*= None\)", sig), sig
    assert sig.index("*, k_descale") < sig.index("cu_seqlens_q") < sig.index("softmax_scale") < sig.index(", sinks:")        # keyword-only
    # it continues the third overload of fwd_kvcache argument for argument
    names = lambda s: re.findall(r"(\w+): ", s[s.index("("):])
    third = doc[doc.index("3. fwd_kvcache("):]
    n3, ns = names(third[:third.index("->")]), names(sig)
    assert ns[:len(n3)] == n3 and ns[len(n3):] == ["sinks"], (n3, ns)
    # the extension's own checks (the Python layer has them too)
    q = torch.zeros(2, 1, 4, 64, dtype=torch.float16)
    kc = torch.zeros(2, 32, 2, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU"):
        _C.fwd_kvcache_sinks(q, kc, kc, sinks=torch.zeros(4))


# ---- 4. ISA -----------------------------------------------------------------------------------------------------------------------------

def test_sink_kernels_isa():
    """32 attention kernels ({fp16, bf16} x {64, 128} x {contiguous, paged} x {16-bit, FP8} x {dense, ragged}; the window code serves plain
    and causal calls) and 8 combines ({dense, ragged} x {fp16, bf16} x {64, 128}), nothing else - no append, no second copy of an existing
    kernel.  Attention: no scratch, two workgroups per CU (VGPRs <= 256, no AGPRs, 2 x LDS <= 160 KiB), an MFMA loop free of scratch traffic and
    accumulator moves, no MFMA hazard, M0 untouched.  Combines: no MFMA, no LDS, no scratch."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_kvcache_sink.hip" in B.HIP_SOURCES and "fa_fwd_kvcache_sink.hip" in B.M0_GUARD_SOURCES
    ks = analyse("fa_fwd_kvcache_sink.hip")
    dense = {n: k for n, k in ks.items() if "fa_fwd_kvcache_sink_kernel" in n}
    ragged = {n: k for n, k in ks.items() if "fa_fwd_kvcache_ragged_sink_kernel" in n}
    comb = {n: k for n, k in ks.items() if "fa_kvcache_sink_combine_" in n}
    assert (len(dense), len(ragged), len(comb)) == (16, 16, 8) and len(ks) == 40, sorted(ks)
    keys = set()
    for n, k in {**dense, **ragged}.items():
        m = re.search(r"fa_fwd_kvcache_(ragged_)?sink_kernelI(DF16_|DF16b)Li(\d+)ELb(\d)ELi(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 256, (n, k["vgprs"], k["scratch_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
    assert keys == {(r, t, d, p, e) for r in (None, "ragged_") for t in ("DF16_", "DF16b") for d in ("64", "128") for p in "01" for e in "12"}
    ckeys = set()
    for n, k in comb.items():
        m = re.search(r"fa_kvcache_sink_combine_(ragged_)?kernelI(DF16_|DF16b)Li(\d+)E", n)
        assert m, n
        ckeys.add(m.groups())
        assert k["mfma_total"] == 0 and k["lds_bytes"] == 0 and k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["m0_outside_asm"] == 0, (n, k)
    assert ckeys == {(r, t, d) for r in (None, "ragged_") for t in ("DF16_", "DF16b") for d in ("64", "128")}


def test_sink_plain_variant_isa():
    """-DFA_KVC_SINK_PLAIN=1 (the A / B build of DESIGN.md 3.10): the 40 kernels above plus plain and causal attention instantiations, 2 x 32 more,
    under the same resource limits"""
    from _kernel_isa import analyse

    ks = analyse("fa_fwd_kvcache_sink.hip", extra_flags=["-DFA_KVC_SINK_PLAIN=1"])
    plain = {n: k for n, k in ks.items() if "sink_plain_kernel" in n}
    assert len(plain) == 64 and len(ks) == 104, sorted(ks)
    keys = set()
    for n, k in plain.items():
        m = re.search(r"fa_fwd_kvcache_(ragged_)?sink_plain_kernelI(DF16_|DF16b)Li(\d+)ELb(\d)ELb(\d)ELi(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 256, (n, k["vgprs"], k["scratch_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
    assert keys == {(r, t, d, c, p, e) for r in (None, "ragged_") for t in ("DF16_", "DF16b") for d in ("64", "128") for c in "01" for p in "01" for e in "12"}
