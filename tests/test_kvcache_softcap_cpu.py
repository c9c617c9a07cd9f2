"""CPU: softmax_scale and softcap on the decode path (the two keywords of flash_attn_with_kvcache, fa_kvcache_options_v5 of the C ABI) - the
struct layout against the header, a zeroed tail as a v4 call, validation codes and their order before any device work, the accepted struct
sizes, a plain C caller, the capi helper, the Python surface's validation, the extension's overloads, and the ISA of the new kernels.
No GPU involved."""
import ctypes
import math
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi
from test_kvcache_window_cpu import EX_ENTRY_POINTS, _aligned_addr, _params, _rc

FP8 = capi.FA_CACHE_FP8_E4M3
NAN, INF = float("nan"), float("inf")


def _opt5(**kw):
    o = capi.KvcacheOptionsV5()
    for k, v in kw.items():
        if k == "reserved":
            o.reserved[0], o.reserved[1] = v
        else:
            setattr(o, k, v)
    return o


# ---- 1. layout --------------------------------------------------------------------------------------------------------------------------

def test_options_v5_layout_matches_header(tmp_path):
    """fa_kvcache_options .. _v4 keep their sizes (20, 72, 112, 144); v5 repeats the v4 fields at the same offsets, appends softmax_scale,
    softcap and reserved[2] and is 168 bytes; ctypes agrees with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheOptionsV5._fields_]
    v4 = [f[0] for f in capi.KvcacheOptionsV4._fields_]
    assert fields[:len(v4)] == v4
    assert fields[len(v4):] == ["softmax_scale", "softcap", "reserved"]
    src = tmp_path / "opt5_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_KVCACHE_SOFTCAP\n#error "no FA_HAS_KVCACHE_SOFTCAP"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu %zu %zu %zu\\n", sizeof(fa_kvcache_options_v5), sizeof(fa_kvcache_options_v4), sizeof(fa_kvcache_options_v3), sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options));\n'
                   '    printf("abi %d 0\\n", FA_ABI_VERSION);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options_v5, {f}), sizeof(((fa_kvcache_options_v5*)0)->{f}));\n' for f in fields)
                   + "".join(f'    printf("v4_{f} %zu 0\\n", offsetof(fa_kvcache_options_v4, {f}));\n' for f in v4)
                   + "    fa_kvcache_options_v5 o;\n    FA_PARAMS_INIT(o);\n"
                     "    return o.struct_size == sizeof(o) && o.magic == FA_PARAMS_MAGIC && o.softmax_scale == 0.0f && o.softcap == 0.0f && o.reserved[0] == 0 && o.reserved[1] == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "opt5_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    sizes = [ctypes.sizeof(c) for c in (capi.KvcacheOptionsV5, capi.KvcacheOptionsV4, capi.KvcacheOptionsV3, capi.KvcacheOptionsV2, capi.KvcacheOptions)]
    assert got["size"] == sizes == [168, 144, 112, 72, 20]
    assert got["abi"][0] == 4 == capi.lib().fa_abi_version()
    for f in fields:
        assert got[f] == [getattr(capi.KvcacheOptionsV5, f).offset, getattr(capi.KvcacheOptionsV5, f).size], f
    for f in v4:
        assert got["v4_" + f][0] == got[f][0], f
    assert (got["softmax_scale"], got["softcap"], got["reserved"]) == ([144, 4], [148, 4], [152, 16])
    # 168 is the smallest 8-aligned size past 144 that the older tests do not pin as FA_ERR_BAD_ABI
    pinned = (145, 148, 152, 160, 176, 256)
    assert 168 not in pinned and all(s in pinned for s in (152, 160))


SHAPES = [(1, 1, 32, 8, 131072, True), (1, 4, 32, 8, 32768, False), (3, 16, 16, 4, 768, True), (2, 33, 32, 1, 4096, False), (64, 1, 32, 8, 4096, False),
          (3, 2, 8, 8, 100, False)]
WINDOWS = [(-1, -1), (0, 0), (31, 0), (127, 3), (7, -1)]


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_v5_with_a_zeroed_tail_is_a_v4_call_and_the_two_values_do_not_move_the_split(fn):
    """same split and workspace from a v4 struct, a v5 struct with a zeroed tail, and a v5 struct with a scale and a cap - 16-bit and 8-bit
    cache, with and without a window, dense and ragged"""
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
                            v4, v5, v5s = capi.KvcacheOptionsV4(), _opt5(), _opt5(softmax_scale=0.37, softcap=30.0)
                            assert (v4.struct_size, v5.struct_size) == (144, 168)
                            for o in (v4, v5, v5s):
                                o.is_local, o.window_size_left, o.window_size_right, o.cache_dtype = int(win != (-1, -1)), win[0], win[1], fp8
                                if ragged:
                                    o.cu_seqlens_q, o.total_q = addr, b * sq - 1 + b
                            want = f(ctypes.byref(p), ctypes.byref(v4))
                            assert want >= 0, capi.last_error()
                            assert f(ctypes.byref(p), ctypes.byref(v5)) == want, (b, sq, cache, ws, kw, win, fp8, ragged)
                            assert f(ctypes.byref(p), ctypes.byref(v5s)) == want, (b, sq, cache, ws, kw, win, fp8, ragged)


# ---- 2. validation ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_softcap_option_validation_codes_and_their_order(fn):
    buf, addr = _aligned_addr()
    S, ABI = capi.FA_ERR_BAD_SHAPE, capi.FA_ERR_BAD_ABI

    def P(**kw):
        p = _params(**kw)
        if fn == "fa_run_mha_fwd_kvcache_ex":
            p.b = 0                                          # (validated, launches nothing: the addresses are dummies)
        return p

    # what is accepted: nothing, either alone, both, tiny and huge finite values, beside every older option
    for o in (_opt5(), _opt5(softmax_scale=0.125), _opt5(softcap=30.0), _opt5(softmax_scale=1e-10, softcap=1e10), _opt5(softmax_scale=1e10, softcap=1e-10),
              _opt5(softmax_scale=0.5, softcap=50.0, cache_dtype=FP8), _opt5(softcap=2.0, is_local=1, window_size_left=37, window_size_right=0),
              _opt5(softcap=2.0, cu_seqlens_q=addr, total_q=64), _opt5(softmax_scale=-0.0)):
        p = P(sq=4)
        if o.cu_seqlens_q:
            p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
        assert _rc(p, fn, o) >= 0, capi.last_error()
    # softmax_scale: negative, NaN, inf - the field is named
    for bad in (-1.0, -1e-30, NAN, INF, -INF):
        assert _rc(P(), fn, _opt5(softmax_scale=bad)) == S and "softmax_scale" in capi.last_error(), bad
        assert _rc(P(), fn, _opt5(softmax_scale=bad, softcap=30.0)) == S and "softmax_scale" in capi.last_error(), bad
    # softcap likewise
    for bad in (-1.0, -1e-30, NAN, INF, -INF):
        assert _rc(P(), fn, _opt5(softcap=bad)) == S and "softcap" in capi.last_error() and "softmax_scale" not in capi.last_error(), bad
    # a pair whose ratio softmax_scale / softcap leaves the fp32 range cannot be evaluated
    for kw in (dict(softmax_scale=1e-30, softcap=1e30), dict(softmax_scale=1e30, softcap=1e-30)):
        assert _rc(P(), fn, _opt5(**kw)) == S and "fp32 range" in capi.last_error(), kw
    # a non-zero reserved word is a newer caller's field
    for r in ((1, 0), (0, 1), (-1, 0), (0, 1 << 40)):
        assert _rc(P(), fn, _opt5(reserved=r)) == ABI and "reserved" in capi.last_error(), r
    # the order: params first, then the older option fields, then the scale, the cap, the reserved words
    bad5 = dict(softmax_scale=-1.0, softcap=-1.0, reserved=(1, 1))
    assert _rc(P(h=3, hk=2), fn, _opt5(**bad5)) == capi.FA_ERR_BAD_GQA
    assert _rc(P(sq=0), fn, _opt5(**bad5)) == S and "seqlen_q" in capi.last_error()
    assert _rc(P(), fn, _opt5(cache_dtype=9, **bad5)) == capi.FA_ERR_BAD_DTYPE
    assert _rc(P(), fn, _opt5(is_local=1, window_size_left=-2, **bad5)) == S and "window_size" in capi.last_error()
    assert _rc(P(), fn, _opt5(rotary_cos=addr, **bad5)) == S and "rotary" in capi.last_error()
    p = P()
    p.q_stride = p.o_stride = capi.Strides(0, p.h * p.d, p.d)
    assert _rc(p, fn, _opt5(cu_seqlens_q=addr, total_q=-1, **bad5)) == S and "total_q" in capi.last_error()
    assert _rc(P(), fn, _opt5(**bad5)) == S and "softmax_scale" in capi.last_error()
    assert _rc(P(), fn, _opt5(softcap=-1.0, reserved=(1, 1))) == S and "softcap" in capi.last_error()
    assert _rc(P(), fn, _opt5(softmax_scale=0.5, softcap=3.0, reserved=(1, 1))) == ABI


@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_exactly_five_struct_sizes_are_accepted(fn):
    for size in list(range(8, 20)) + [24, 28, 40, 64, 71, 76, 80, 96, 104, 108, 111, 113, 116, 120, 128, 136, 140, 143, 145, 148, 152, 160, 164, 167, 169, 172, 176, 184,
                                      192, 256, 1024]:
        o = _opt5(softcap=30.0)
        o.struct_size = size
        assert _rc(_params(), fn, o) == capi.FA_ERR_BAD_ABI, size
    for size, cls in ((20, capi.KvcacheOptions), (72, capi.KvcacheOptionsV2), (112, capi.KvcacheOptionsV3), (144, capi.KvcacheOptionsV4), (168, capi.KvcacheOptionsV5)):
        assert cls().struct_size == size and _rc(_params(), fn, cls()) >= 0, size
    # a v5 struct that states a shorter size is that shorter struct: the tail is not read
    o = _opt5(softmax_scale=-1.0, softcap=NAN, reserved=(7, 7))
    o.struct_size = 144
    assert _rc(_params(), fn, o) >= 0, capi.last_error()


def test_plain_c_caller_uses_the_v5_struct(tmp_path):
    src = tmp_path / "use_softcap.c"
    src.write_text(r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
static _Alignas(16) char mem[256];
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = mem; p.lse = (float*)mem; p.cache_seqlens = (const int32_t*)mem;
    p.b = 4; p.seqlen_q = 8; p.seqlen_cache = 32768; p.h = 32; p.h_k = 8; p.d = 128; p.dtype = FA_BF16; p.num_splits = 4;
    p.q_stride = p.o_stride = (fa_strides){8 * 32 * 128, 32 * 128, 128};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 128, 8 * 128, 128};
    fa_kvcache_options_v4 o4;
    FA_PARAMS_INIT(o4);
    fa_kvcache_options_v5 o5;
    FA_PARAMS_INIT(o5);
    if (sizeof(o5) != 168) return 9;
    long long dense = fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o4);
    if (dense != 4LL * (4 * 32 * 8) * 128 * 4 + 4LL * (4 * 32 * 8) * 4) return 10;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o5) != dense) return 11;      /* zeroed tail: the v4 call */
    o5.softmax_scale = 1.0f / 16.0f; o5.softcap = 50.0f;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o5) != dense) return 12;      /* the two values do not move the split */
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o5) != 1) return 13;               /* (no workspace in the params) */
    o5.softcap = -50.0f;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o5) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "softcap")) return 14;
    o5.softcap = 50.0f; o5.softmax_scale = NAN;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o5) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "softmax_scale")) return 15;
    o5.softmax_scale = 0.0f; o5.reserved[1] = 1;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o5) != FA_ERR_BAD_ABI) return 16;
    o5.reserved[1] = 0; p.b = 0;
    if (fa_run_mha_fwd_kvcache_ex(&p, (const fa_kvcache_options*)&o5, NULL) != FA_OK) return 17;      /* nothing to do: no launch */
    return 0;
}
""")
    exe = tmp_path / "use_softcap"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_capi_helper_builds_the_v5_struct_only_when_asked():
    cu = torch.tensor([0, 1, 2, 10, 11], dtype=torch.int32)
    o = capi.kvcache_options(softcap=30.0)
    assert isinstance(o, capi.KvcacheOptionsV5) and o.struct_size == 168
    assert (o.softmax_scale, o.softcap, o.reserved[0], o.reserved[1], o.is_local, o.cache_dtype, o.cu_seqlens_q) == (0.0, 30.0, 0, 0, 0, 0, None)
    o = capi.kvcache_options((7, 0), cache_dtype=FP8, cu_seqlens_q=cu, total_q=11, softmax_scale=0.25, softcap=2.0)
    assert isinstance(o, capi.KvcacheOptionsV5)
    assert (o.softmax_scale, o.softcap, o.is_local, o.window_size_left, o.cache_dtype, o.cu_seqlens_q, o.total_q) == (0.25, 2.0, 1, 7, FP8, cu.data_ptr(), 11)
    o = capi.kvcache_options(softmax_scale=0.1)
    assert isinstance(o, capi.KvcacheOptionsV5) and o.softcap == 0.0 and o.softmax_scale == ctypes.c_float(0.1).value
    # without the two keywords every call keeps the struct it had
    o = capi.kvcache_options(cu_seqlens_q=cu, total_q=11)
    assert type(o) is capi.KvcacheOptionsV4 and o.struct_size == 144
    assert type(capi.kvcache_options((3, 0))) is capi.KvcacheOptions and type(capi.kvcache_options(cache_dtype=FP8)) is capi.KvcacheOptionsV2
    assert type(capi.kvcache_options()) is capi.KvcacheOptions
    p = _params(ws_bytes=1 << 40)
    assert capi.kvcache_num_splits(p, capi.kvcache_options(softcap=30.0, softmax_scale=0.5)) == capi.kvcache_num_splits(p, capi.kvcache_options())


# ---- 3. the Python surface and the extension --------------------------------------------------------------------------------------------

def test_python_surface_rejects_bad_scale_and_cap():
    import flash_attn_turing as F

    b, h, hk, d, cap = 2, 4, 2, 64, 32
    q = torch.zeros(b, 1, h, d, dtype=torch.float16)
    kc = torch.zeros(b, cap, hk, d, dtype=torch.float16)

    def call(**kw):
        return F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=4, **kw)

    for bad in (True, False, 0, 0.0, -0.0, -1, -0.125, NAN, INF, -INF, "0.1", [0.1], torch.tensor(0.1), 1e-60, 1e60, 1j):
        with pytest.raises(ValueError, match="softmax_scale"):
            call(softmax_scale=bad)
        with pytest.raises(ValueError, match="softmax_scale"):
            call(softmax_scale=bad, softcap=30.0)
    for bad in (True, False, -1, -1e-3, NAN, INF, -INF, "30", [30.0], torch.tensor(30.0), None, 1e60, 1e-60, 1j):
        with pytest.raises(ValueError, match="softcap"):
            call(softcap=bad)
    # both are keyword-only
    with pytest.raises(TypeError):
        F.flash_attn_with_kvcache(q, kc, kc, None, None, 4, False, 0, False, 0.125)
    # a CPU call that passes the checks is still refused by the extension (no quiet fall-back), whichever overload it resolves to
    for kw in (dict(), dict(softmax_scale=0.125), dict(softcap=30.0), dict(softmax_scale=1, softcap=2), dict(softcap=0.0), dict(softmax_scale=None),
               dict(softcap=30.0, causal=True, window_size=(7, 0)), dict(softcap=30.0, num_splits=3)):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**kw)
    qr = torch.zeros(3, h, d, dtype=torch.float16)
    cu = torch.tensor([0, 1, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=4, cu_seqlens_q=cu, max_seqlen_q=2, softcap=30.0, softmax_scale=0.2)
    with pytest.raises(ValueError, match="softcap"):
        F.flash_attn_with_kvcache(qr, kc, kc, cache_seqlens=4, cu_seqlens_q=cu, max_seqlen_q=2, softcap=-30.0)
    # rotary together with cu_seqlens_q stays refused, with the new keywords as without
    cos = torch.ones(cap, 16, dtype=torch.float16)
    kn = torch.zeros(3, hk, d, dtype=torch.float16)
    with pytest.raises(ValueError, match="rotary_cos / rotary_sin together with cu_seqlens_q are not supported"):
        F.flash_attn_with_kvcache(qr, kc, kc, k=kn, v=kn, cache_seqlens=4, cu_seqlens_q=cu, max_seqlen_q=2, cu_seqlens_k_new=cu, rotary_cos=cos, rotary_sin=cos, softcap=30.0)


def test_extension_gains_a_third_overload_and_keeps_the_first_two():
    from flash_attn_turing import _C

    doc = _C.fwd_kvcache.__doc__
    i1, i2, i3 = doc.index("1. fwd_kvcache("), doc.index("2. fwd_kvcache("), doc.index("3. fwd_kvcache(")
    assert "4. fwd_kvcache(" not in doc
    first, second, third = doc[i1:i2], doc[i2:i3], doc[i3:]
    assert re.search(r"rotary_interleaved: bool = True\) ->", first) and "cu_seqlens" not in first and "softcap" not in first, first
    sig2 = second[:second.index("->")]
    assert re.search(r"rotary_interleaved: bool = True, cu_seqlens_q: [^,]*= None, max_seqlen_q: [^,]*= 0, cu_seqlens_k_new: [^,]*= None\)", sig2), sig2
    assert "softcap" not in second and "softmax_scale" not in second
    sig3 = third[:third.index("->")]
    assert re.search(r"cu_seqlens_k_new: [^,]*= None, softmax_scale: [^,]*= None, softcap: [^,]*[Ff]loat = 0\.0\)", sig3), sig3
    assert sig3.index("*, k_descale") < sig3.index("cu_seqlens_q") < sig3.index("softmax_scale")        # keyword-only
    # the third continues the second, which continues the first: argument for argument
    names = lambda sig: re.findall(r"(\w+): ", sig[sig.index("("):])
    n1, n2, n3 = names(first[:first.index("->")]), names(sig2), names(sig3)
    assert n2[:len(n1)] == n1 and n3[:len(n2)] == n2 and n3[len(n2):] == ["softmax_scale", "softcap"], (n1, n2, n3)


# ---- 4. ISA -----------------------------------------------------------------------------------------------------------------------------

def test_softcap_kernels_isa():
    """32 attention kernels ({fp16, bf16} x {64, 128} x {contiguous, paged} x {16-bit, FP8} x {dense, ragged}; the window code serves plain
    and causal calls) and nothing else - no append, no combine, no second copy of a dense or ragged kernel: no scratch, two workgroups per
    CU with an MFMA loop free of scratch traffic and accumulator moves, no MFMA hazard, M0 untouched, no scalar memory write anywhere, and
    the tanh built from the exponential and the reciprocal inside the loop"""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_kvcache_softcap.hip" in B.HIP_SOURCES and "fa_fwd_kvcache_softcap.hip" in B.M0_GUARD_SOURCES
    ks = analyse("fa_fwd_kvcache_softcap.hip")
    dense = {n: k for n, k in ks.items() if "fa_fwd_kvcache_softcap_kernel" in n}
    ragged = {n: k for n, k in ks.items() if "fa_fwd_kvcache_ragged_softcap_kernel" in n}
    assert (len(dense), len(ragged)) == (16, 16) and len(ks) == 32, sorted(ks)
    keys = set()
    for n, k in ks.items():
        m = re.search(r"fa_fwd_kvcache_(ragged_)?softcap_kernelI(DF16_|DF16b)Li(\d+)ELb(\d)ELi(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 256, (n, k["vgprs"], k["scratch_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
            # 8 scores per lane and step, two steps per trip of the loop: the tanh costs each an exponential and a reciprocal beside the exponential of P
            n_rcp = sum(c for op, c in lp["histogram"].items() if op.startswith("v_rcp_f32"))
            n_exp = sum(c for op, c in lp["histogram"].items() if op.startswith("v_exp_f32"))
            assert n_rcp >= 16 and n_exp >= 32, (n, lp["label"], n_rcp, n_exp)
    assert keys == {(r, t, d, p, e) for r in (None, "ragged_") for t in ("DF16_", "DF16b") for d in ("64", "128") for p in "01" for e in "12"}
    src = os.path.join(B.CSRC, "fa_fwd_kvcache_softcap.hip")
    asm = subprocess.run([B.hipcc_path()] + B.HIPCC_FLAGS + ["-I", B.CSRC, "-I", B.INCLUDE, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    assert B.m0_uses_outside_asm(asm) == 0
    ops = set(re.findall(r"^\s+(s_[a-z0-9_]+)", asm, re.M))
    assert not [o for o in ops if "store" in o or "atomic" in o or "dcache" in o], ops              # scalar instructions only load
    assert len(re.findall(r"^\s*\.amdhsa_kernel ", asm, re.M)) == 32
