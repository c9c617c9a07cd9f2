"""CPU: the FP8 (e4m3fn) KV cache of the decode path - the number-format facts the design rests on, the C ABI (fa_kvcache_options_v2: layout
against the header, old callers, validation codes before any device work, the split / workspace rule), the Python surface's validation, and
the ISA of the new kernels next to the unchanged 16-bit ones.  No GPU involved."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi
from test_kvcache_window_cpu import EX_ENTRY_POINTS, _params, _rc

FP8 = capi.FA_CACHE_FP8_E4M3


def quantise(x, descale):
    """the append contract, stated with torch alone: e4m3_rne(clamp(float(x) / descale, -448, 448)); NaN stays NaN"""
    return (x.float() / descale).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


# ---- 10. e4m3 facts ------------------------------------------------------------------------------------------------------------------

def test_every_finite_e4m3_value_is_an_fp16_and_a_bf16_value():
    codes = torch.arange(256, dtype=torch.int16).to(torch.uint8)
    f8 = codes.view(torch.float8_e4m3fn)
    f32 = f8.float()
    finite = torch.isfinite(f32)
    assert int(finite.sum()) == 254 and codes[~finite].tolist() == [0x7F, 0xFF]
    assert torch.isnan(f32[~finite]).all()
    for dt in (torch.float16, torch.bfloat16):
        w = f8.to(dt)
        assert torch.equal(w[finite].float(), f32[finite]), dt                # widening loses nothing
        assert torch.equal(w[finite].to(torch.float8_e4m3fn).view(torch.uint8), codes[finite]), dt
        assert torch.isnan(w[~finite]).all(), dt
    assert f32[finite].abs().max().item() == 448.0
    assert f32[finite & (f32 != 0)].abs().min().item() == 2.0 ** -9
    assert f32[0].item() == 0.0 and codes[0].item() == 0                      # the zero-fill of out-of-range loads is +0


def test_test_side_quantiser_saturates_rounds_to_even_and_keeps_nan():
    x = torch.tensor([448.0, 449.0, 1e4, 65504.0, float("inf"), -449.0, float("-inf"), float("nan"), 0.0, 2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 2.0 ** -11,
                      17.0, 19.0, 1.0625, 1.1875])
    q = quantise(x, 1.0)
    want = [448.0, 448.0, 448.0, 448.0, 448.0, -448.0, -448.0, None, 0.0, 2.0 ** -9, 0.0, 2.0 ** -8, 0.0, 16.0, 20.0, 1.0, 1.25]
    got = q.float().tolist()
    for g, w in zip(got, want):
        assert (g != g) if w is None else g == w, (got, want)
    assert q.view(torch.uint8)[7].item() == 0x7F
    # a descale that is not a power of two: the quotient is rounded once to fp32, then once to e4m3
    y = torch.tensor([1.0, 3.0, -7.5], dtype=torch.float16)
    assert quantise(y, 3.0).float().tolist() == [0.34375, 1.0, -2.5]


# ---- 11. C ABI on the host -------------------------------------------------------------------------------------------------------------

def _opt(**kw):
    o = capi.KvcacheOptionsV2()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_options_v2_layout_matches_header(tmp_path):
    """fa_kvcache_options keeps its 20 bytes; fa_kvcache_options_v2 starts with the same five fields and ctypes agrees with a C program"""
    fields = [f[0] for f in capi.KvcacheOptionsV2._fields_]
    assert fields[:5] == [f[0] for f in capi.KvcacheOptions._fields_]
    assert fields[5:] == ["cache_dtype", "k_descale", "v_descale", "k_descale_batch_stride", "k_descale_head_stride", "v_descale_batch_stride",
                          "v_descale_head_stride"]
    src = tmp_path / "opt2_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\nint main(void) {\n'
                   '    printf("size %zu %zu\\n", sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options));\n    printf("fp8 %d 0\\n", FA_CACHE_FP8_E4M3);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options_v2, {f}), sizeof(((fa_kvcache_options_v2*)0)->{f}));\n' for f in fields)
                   + "".join(f'    printf("old_{f} %zu 0\\n", offsetof(fa_kvcache_options, {f}));\n' for f in fields[:5])
                   + "    fa_kvcache_options_v2 o;\n    FA_PARAMS_INIT(o);\n    return o.struct_size == sizeof(o) && o.cache_dtype == 0 && o.k_descale == NULL ? 0 : 1;\n}\n")
    exe = tmp_path / "opt2_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"] == [ctypes.sizeof(capi.KvcacheOptionsV2), ctypes.sizeof(capi.KvcacheOptions)] == [72, 20]
    assert got["fp8"][0] == FP8
    for f in fields:
        assert got[f] == [getattr(capi.KvcacheOptionsV2, f).offset, getattr(capi.KvcacheOptionsV2, f).size], f
    for f in fields[:5]:
        assert got["old_" + f][0] == got[f][0], f


def test_library_exports_what_the_header_declares():
    L = capi.lib()
    for n in capi.declared_functions():
        assert hasattr(L, n), n
    assert L.fa_abi_version() == 4                      # the feature is detected by struct_size, not by the ABI version
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define FA_CACHE_FP8_E4M3 1\b", text) and "fa_kvcache_options_v2" in text


SHAPES = [(1, 1, 32, 8, 131072, True), (1, 4, 32, 8, 32768, False), (3, 16, 16, 4, 768, True), (2, 33, 32, 1, 4096, False), (64, 1, 32, 8, 4096, False),
          (1, 1, 32, 8, 32768, False), (8, 1, 32, 32, 32768, False), (1, 16, 16, 4, 768, False), (3, 2, 8, 8, 100, False), (1, 255, 32, 8, 65536, True),
          (256, 1, 8, 8, 4096, False)]          # the shapes of test_kvcache_window_cpu.py
WINDOWS = [(-1, -1), (0, 0), (31, 0), (4095, 0), (127, 3), (7, -1)]


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_old_struct_size_zeroed_tail_and_fp8_give_the_same_split(fn):
    """a caller built against fa_kvcache_options (struct_size 20), a v2 struct with a zeroed tail and NULL options where there is no window
    all get the same split and workspace - and so does an 8-bit cache of the same shape (they follow the capacity, not the element size)"""
    f = getattr(capi.lib(), fn)
    plain = getattr(capi.lib(), fn[:-3])
    for b, sq, h, hk, cache, causal in SHAPES:
        for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
            for page in (None, 256) if cache % 256 == 0 else (None,):
                for ws in (None, 1 << 40, 3 * b * h * sq * 128 * 4 + (3 * b * h * sq * 4 + 15) // 16 * 16):
                    p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, page=page, ws_bytes=ws, **kw)
                    for win in WINDOWS:
                        old = capi.kvcache_options(win)
                        assert old.struct_size == 20
                        want = f(ctypes.byref(p), ctypes.byref(old))
                        assert want >= 0, capi.last_error()
                        if win == (-1, -1):
                            assert want == plain(ctypes.byref(p)) == f(ctypes.byref(p), None)
                        new = _opt(is_local=old.is_local, window_size_left=old.window_size_left, window_size_right=old.window_size_right)
                        assert new.struct_size == 72
                        assert f(ctypes.byref(p), ctypes.byref(new)) == want, (b, sq, cache, page, ws, kw, win)
                        new.cache_dtype = FP8
                        assert f(ctypes.byref(p), ctypes.byref(new)) == want, (b, sq, cache, page, ws, kw, win, "fp8")


# (num_splits, workspace bytes) the library gave before the 8-bit cache existed, with an unlimited workspace on a 256-CU device (also the count assumed
# without a device), for the windows (-1, -1), (31, 0), (4095, 0), (127, 3)
PARENT_WINDOWS = [(-1, -1), (31, 0), (4095, 0), (127, 3)]
PARENT_SPLITS = [
    ((1, 1, 32, 8, 131072, True), [(64, 1056768), (1, 0), (16, 264192), (1, 0)]),
    ((1, 4, 32, 8, 32768, False), [(64, 4227072), (1, 0), (16, 1056768), (1, 0)]),
    ((3, 16, 16, 4, 768, True), [(3, 1188864), (1, 0), (3, 1188864), (1, 0)]),
    ((2, 33, 32, 1, 4096, False), [(4, 4359168), (1, 0), (4, 4359168), (1, 0)]),
    ((64, 1, 32, 8, 4096, False), [(1, 0), (1, 0), (1, 0), (1, 0)]),
    ((1, 1, 32, 8, 32768, False), [(64, 1056768), (1, 0), (16, 264192), (1, 0)]),
    ((8, 1, 32, 32, 32768, False), [(1, 0), (1, 0), (1, 0), (1, 0)]),
    ((1, 16, 16, 4, 768, False), [(3, 396288), (1, 0), (3, 396288), (1, 0)]),
    ((3, 2, 8, 8, 100, False), [(1, 0), (1, 0), (1, 0), (1, 0)]),
    ((1, 255, 32, 8, 65536, True), [(1, 0), (1, 0), (1, 0), (1, 0)]),
    ((256, 1, 8, 8, 4096, False), [(1, 0), (1, 0), (1, 0), (1, 0)]),
]


def test_parent_values_of_split_and_workspace_are_kept():
    """the split and workspace of the library before this feature, through the old struct, the new one with a zeroed tail, and for an 8-bit cache"""
    for (b, sq, h, hk, cache, causal), rows in PARENT_SPLITS:
        for win, (ns, wsb) in zip(PARENT_WINDOWS, rows):
            p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, ws_bytes=1 << 40)
            old = capi.kvcache_options(win)
            new = _opt(is_local=old.is_local, window_size_left=old.window_size_left, window_size_right=old.window_size_right)
            fp8 = _opt(is_local=old.is_local, window_size_left=old.window_size_left, window_size_right=old.window_size_right, cache_dtype=FP8)
            for o in (old, new, fp8) + ((None,) if win == (-1, -1) else ()):
                assert capi.kvcache_num_splits(p, o) == ns, (b, sq, cache, win, type(o))
                assert capi.kvcache_workspace_bytes(p, o) == wsb, (b, sq, cache, win, type(o))


@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_fp8_option_validation_codes(fn):
    """unknown cache dtype and a descale without FP8: FA_ERR_BAD_DTYPE; struct sizes between the two layouts: FA_ERR_BAD_ABI; strides of an
    8-bit cache that are not multiples of 16 elements, or a base that is not 16-byte aligned: FA_ERR_BAD_STRIDE - all before any device work"""
    buf = (ctypes.c_float * 64)()
    addr = ctypes.addressof(buf)

    def p0(**kw):
        p = _params(**kw)
        if fn == "fa_run_mha_fwd_kvcache_ex":
            p.b = 0                                      # (the addresses are dummies: b = 0 is validated and launches nothing)
        return p

    assert _rc(p0(), fn, _opt()) >= 0 and _rc(p0(), fn, _opt(cache_dtype=FP8)) >= 0, capi.last_error()
    assert _rc(p0(), fn, _opt(cache_dtype=FP8, k_descale=addr, v_descale=addr, k_descale_batch_stride=8, k_descale_head_stride=1)) >= 0, capi.last_error()
    for bad in (2, 3, -1, 0x7F):
        assert _rc(p0(), fn, _opt(cache_dtype=bad)) == capi.FA_ERR_BAD_DTYPE, bad
        assert "cache_dtype" in capi.last_error() and "FA_CACHE_FP8_E4M3" in capi.last_error()
    for kw in (dict(k_descale=addr), dict(v_descale=addr), dict(k_descale=addr, v_descale=addr)):
        assert _rc(p0(), fn, _opt(**kw)) == capi.FA_ERR_BAD_DTYPE, kw
        assert "descale" in capi.last_error()
    for size in (24, 28, 40, 64, 71, 76):
        o = _opt(cache_dtype=FP8)
        o.struct_size = size
        assert _rc(p0(), fn, o) == capi.FA_ERR_BAD_ABI, size
    # params errors still come first
    assert _rc(p0(h=3, hk=2), fn, _opt(cache_dtype=FP8)) == capi.FA_ERR_BAD_GQA
    if fn == "fa_run_mha_fwd_kvcache_ex":
        return                                          # (b = 0 there: the tensors are not looked at)
    d, hk, cache = 128, 8, 32768
    good = capi.Strides(cache * hk * d, hk * d, d)
    for which in ("k_cache_stride", "v_cache_stride"):
        for st in (capi.Strides(cache * hk * d + 8, hk * d, d), capi.Strides(cache * hk * d, hk * d + 8, d), capi.Strides(cache * hk * d, hk * d, d + 8),
                   capi.Strides(cache * hk * d, 64, d)):
            p = _params()
            setattr(p, which, st)
            assert _rc(p, fn, _opt(cache_dtype=FP8)) == capi.FA_ERR_BAD_STRIDE, (which, st.batch, st.row, st.head)
            assert "16" in capi.last_error() and which[:7] in capi.last_error()
        # ... while 8-element multiples remain fine for a 16-bit cache
        p = _params()
        setattr(p, which, capi.Strides(cache * hk * d + 8, hk * d + 8, d + 8))
        assert _rc(p, fn, _opt()) >= 0, capi.last_error()
        setattr(p, which, good)
    p = _params()
    p.k_cache += 8
    assert _rc(p, fn, _opt(cache_dtype=FP8)) == capi.FA_ERR_BAD_STRIDE and "16-byte aligned" in capi.last_error()
    # one sequence of an 8-bit cache may span 2^31 - 1 bytes: twice the rows of a 16-bit cache
    rows = (1 << 31) // (8 * 128)
    assert _rc(_params(cache=rows - 32), fn, _opt(cache_dtype=FP8)) >= 0, capi.last_error()
    assert _rc(_params(cache=rows - 32), fn, _opt()) == capi.FA_ERR_BAD_STRIDE
    assert _rc(_params(cache=rows), fn, _opt(cache_dtype=FP8)) == capi.FA_ERR_BAD_STRIDE


def test_plain_c_caller_uses_both_option_structs(tmp_path):
    src = tmp_path / "use_fp8.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
static _Alignas(16) char mem[256];
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = mem; p.lse = (float*)mem; p.cache_seqlens = (const int32_t*)mem;
    p.b = 1; p.seqlen_q = 1; p.seqlen_cache = 32768; p.h = 32; p.h_k = 8; p.d = 128; p.dtype = FA_FP16;
    p.q_stride = p.o_stride = (fa_strides){32 * 128, 32 * 128, 128};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 128, 8 * 128, 128};
    fa_kvcache_options o1;
    FA_PARAMS_INIT(o1);
    fa_kvcache_options_v2 o2;
    FA_PARAMS_INIT(o2);
    long long plain = fa_kvcache_workspace_bytes(&p);
    if (plain <= 0) return 10;
    if (fa_kvcache_workspace_bytes_ex(&p, &o1) != plain) return 11;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o2) != plain) return 12;
    o2.cache_dtype = FA_CACHE_FP8_E4M3;
    o2.k_descale = (const float*)mem; o2.k_descale_head_stride = 1; o2.k_descale_batch_stride = 8;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o2) != plain) return 13;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o2) != fa_kvcache_num_splits(&p)) return 14;
    o2.cache_dtype = 0;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o2) != FA_ERR_BAD_DTYPE || !strstr(fa_last_error(), "descale")) return 15;
    o2.k_descale = NULL; o2.cache_dtype = 9;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o2) != FA_ERR_BAD_DTYPE || !strstr(fa_last_error(), "cache_dtype")) return 16;
    o2.cache_dtype = FA_CACHE_FP8_E4M3; p.k_cache_stride.row = 8 * 128 + 8;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o2) != FA_ERR_BAD_STRIDE) return 17;
    p.b = 0;
    if (fa_run_mha_fwd_kvcache_ex(&p, (const fa_kvcache_options*)&o2, NULL) != FA_OK) return 18;      /* nothing to do: no launch */
    return 0;
}
""")
    exe = tmp_path / "use_fp8"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


# ---- 8. validation of the Python surface that needs no device memory ---------------------------------------------------------------------

def test_python_surface_rejects_bad_cache_dtypes_and_descales():
    import flash_attn_turing as F

    b, hk, d = 2, 2, 64
    q = torch.zeros(b, 1, 4, d, dtype=torch.float16)
    c16 = torch.zeros(b, 32, hk, d, dtype=torch.float16)
    c8 = torch.zeros(b, 32, hk, d, dtype=torch.uint8).view(torch.float8_e4m3fn)
    ds = torch.ones(b, hk)
    for bad in (torch.float8_e4m3fnuz, torch.float8_e5m2, torch.float8_e5m2fnuz, torch.int8, torch.uint8):
        c = torch.zeros(b, 32, hk, d, dtype=torch.uint8).view(bad)
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            F.flash_attn_with_kvcache(q, c, c, cache_seqlens=4)
    for bad in (torch.bfloat16, torch.float32):
        with pytest.raises(ValueError, match="float8_e4m3fn"):
            F.flash_attn_with_kvcache(q, c16.to(bad), c16.to(bad), cache_seqlens=4)
    with pytest.raises(ValueError, match="same dtype"):
        F.flash_attn_with_kvcache(q, c8, c16, cache_seqlens=4)
    with pytest.raises(ValueError, match="same dtype"):
        F.flash_attn_with_kvcache(q, c16, c8, cache_seqlens=4)
    for kw in (dict(k_descale=ds), dict(v_descale=ds), dict(k_descale=ds, v_descale=ds)):
        with pytest.raises(ValueError, match="descale needs a torch.float8_e4m3fn cache"):
            F.flash_attn_with_kvcache(q, c16, c16, cache_seqlens=4, **kw)
    for name in ("k_descale", "v_descale"):
        for bad in (ds.double(), ds.half(), ds.to(torch.int32), 1.0):
            with pytest.raises(ValueError, match=name + " must be a float32 tensor"):
                F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, **{name: bad})
        for bad in (torch.ones(b), torch.ones(hk, b + 1), torch.ones(b, hk, 1), torch.ones(b, 4), torch.ones(1, hk)):
            with pytest.raises(ValueError, match=name + " must have shape"):
                F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, **{name: bad})
        with pytest.raises(ValueError, match=name + " must be on q's device"):
            F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, **{name: ds.to("meta")})
    with pytest.raises(RuntimeError, match="forward-only"):
        F.flash_attn_with_kvcache(q.clone().requires_grad_(True), c8, c8, cache_seqlens=4, k_descale=ds)
    # a CPU call that passes the dtype checks is still refused by the extension (no quiet fall-back)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, k_descale=ds, v_descale=ds)


# ---- 12. ISA ---------------------------------------------------------------------------------------------------------------------------

# VGPRs, AGPRs, LDS bytes of the 16-bit kernels before the 8-bit cache was added (same for fp16 and bf16): (kernel, head_dim, bool template argument)
PARENT_16BIT = {
    ("fa_fwd_kvcache_kernel", 64, "0"): (120, 0, 17920), ("fa_fwd_kvcache_kernel", 64, "1"): (120, 0, 17920),
    ("fa_fwd_kvcache_kernel", 128, "0"): (220, 0, 34304), ("fa_fwd_kvcache_kernel", 128, "1"): (220, 0, 34304),
    ("fa_fwd_kvcache_paged_kernel", 64, "0"): (123, 0, 17920), ("fa_fwd_kvcache_paged_kernel", 64, "1"): (123, 0, 17920),
    ("fa_fwd_kvcache_paged_kernel", 128, "0"): (238, 0, 34304), ("fa_fwd_kvcache_paged_kernel", 128, "1"): (238, 0, 34304),
    ("fa_fwd_kvcache_local_kernel", 64, "0"): (121, 0, 17920), ("fa_fwd_kvcache_local_kernel", 64, "1"): (121, 0, 17920),
    ("fa_fwd_kvcache_local_kernel", 128, "0"): (224, 0, 34304), ("fa_fwd_kvcache_local_kernel", 128, "1"): (222, 0, 34304),
    ("fa_kvcache_append_kernel", 64, None): (33, 0, 0), ("fa_kvcache_append_kernel", 128, None): (33, 0, 0),
    ("fa_kvcache_append_paged_kernel", 64, None): (24, 0, 0), ("fa_kvcache_append_paged_kernel", 128, None): (24, 0, 0),
    ("fa_kvcache_combine_kernel", 64, None): (28, 0, 0), ("fa_kvcache_combine_kernel", 128, None): (28, 0, 0),
}


@pytest.fixture(scope="module")
def kernels():
    from _kernel_isa import analyse

    return analyse("fa_fwd_kvcache.hip")


def _key(name):
    m = re.search(r"\d+(fa_\w+?_kernel)I(?:DF16_|DF16b)?Li(\d+)E(?:Lb(\d)E)?", name)
    assert m, name
    return m.group(1), int(m.group(2)), m.group(3)


def test_fp8_attention_kernels_isa(kernels):
    """every 8-bit attention instantiation: no scratch, two workgroups per CU, an MFMA loop free of scratch traffic and accumulator moves, the
    FP8 widening instruction of its dtype and no FP8 MFMA, no MFMA hazard, M0 untouched"""
    import build as B                                   # (on sys.path through _kernel_isa)

    attn = {n: k for n, k in kernels.items() if re.search(r"fa_fwd_kvcache_fp8_(paged_|local_)?kernel", n)}
    assert len(attn) == 24                                 # fp16 / bf16 x d64 / d128 x (contiguous, paged) x causal / not + local x layouts
    src = os.path.join(B.CSRC, "fa_fwd_kvcache.hip")
    asm = subprocess.run([B.hipcc_path()] + B.HIPCC_FLAGS + ["-I", B.CSRC, "-I", B.INCLUDE, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    for n, k in attn.items():
        assert k.get("scratch_bytes") == 0, (n, k.get("scratch_bytes"))
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["agprs"] == 0 and k["vgprs"] <= 256, (n, k["vgprs"], k["agprs"])
        assert k["mfma_hazards"] == [], (n, k["mfma_hazards"][:3])
        assert k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        assert any(lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0 for lp in k["loops"]), n
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
        body = asm[asm.index(n + ":"):]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
        cvt = "v_cvt_scalef32_pk_bf16_fp8" if "IDF16b" in n else "v_cvt_scalef32_pk_f16_fp8"
        d = _key(n)[1]
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        assert main["histogram"].get(cvt, 0) >= d // 2, (n, main["histogram"].get(cvt))     # K and V of one 32-key step: 64 at d 128
        assert not re.search(r"v_mfma\w*(fp8|bf8|f8f6f4)", body), n
        assert re.search(r"v_mfma_f32_16x16x32_(f16|bf16)", body), n
        assert "buffer_load_dwordx4" in main["histogram"], n


def test_fp8_append_kernels_isa(kernels):
    app = {n: k for n, k in kernels.items() if "fa_kvcache_append_fp8_kernel" in n}
    assert len(app) == 8                                   # fp16 / bf16 x d64 / d128 x contiguous / paged
    for n, k in app.items():
        assert k.get("scratch_bytes") == 0 and k["m0_outside_asm"] == 0 and k["mfma_total"] == 0, n


def test_16bit_kernels_keep_the_parents_registers(kernels):
    """element size and widening are template parameters: the 16-bit instantiations report the numbers they had before"""
    seen = set()
    for n, k in kernels.items():
        if "fp8" in n:
            continue
        key = _key(n)
        assert key in PARENT_16BIT, n
        assert (k["vgprs"], k["agprs"], k["lds_bytes"]) == PARENT_16BIT[key], (n, k["vgprs"], k["agprs"], k["lds_bytes"], PARENT_16BIT[key])
        assert k["scratch_bytes"] == 0 and k["mfma_hazards"] == [], n
        seen.add(key)
    assert seen == set(PARENT_16BIT)
    assert len([n for n in kernels if "fp8" not in n]) == 24 + 2 + 2 + 4
