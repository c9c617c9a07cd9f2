"""CPU: head_dim 256 of the KV-cache decode path - what the C ABI accepts and still rejects (before any device work), the workspace rule at
d = 256, the feature macro of the header, the Python surface's validation, and the resources of every kernel of fa_fwd_kvcache_d256.hip as the
compiler reports them.  No GPU involved."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi
from test_kvcache_window_cpu import EX_ENTRY_POINTS, _params, _rc

FP8 = capi.FA_CACHE_FP8_E4M3
PLAIN_ENTRY_POINTS = ["fa_run_mha_fwd_kvcache", "fa_kvcache_workspace_bytes", "fa_kvcache_num_splits"]


def _call(p, fn, opt=None):
    """any of the six entry points; the plain three take no options"""
    if fn.endswith("_ex"):
        return _rc(p, fn, opt)
    f = getattr(capi.lib(), fn)
    return f(ctypes.byref(p), None) if fn == "fa_run_mha_fwd_kvcache" else f(ctypes.byref(p))


def _p(fn, **kw):
    p = _params(**kw)
    if fn.startswith("fa_run_mha_fwd_kvcache"):
        p.b = 0                                          # (the addresses are dummies: b = 0 is validated and launches nothing)
    return p


# ---- 1. C ABI ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", PLAIN_ENTRY_POINTS + EX_ENTRY_POINTS)
def test_head_dim_256_is_accepted_and_other_head_dims_are_not(fn):
    """d in {64, 128, 256} passes the validation of all six kvcache entry points, with every option struct; d in {32, 96, 192, 512} is
    FA_ERR_BAD_HEADDIM with "head_dim" in the message"""
    opts = [None] if not fn.endswith("_ex") else [None, capi.KvcacheOptions(), capi.KvcacheOptionsV2(), capi.KvcacheOptionsV3(), capi.KvcacheOptionsV4(),
                                                  capi.KvcacheOptionsV5()]
    for d in (64, 128, 256):
        for o in opts:
            assert _call(_p(fn, d=d), fn, o) >= 0, (d, type(o), capi.last_error())
    if fn.endswith("_ex"):
        o = capi.KvcacheOptionsV2()
        o.cache_dtype = FP8
        assert _call(_p(fn, d=256), fn, o) >= 0, capi.last_error()
        o5 = capi.KvcacheOptionsV5()
        o5.softcap, o5.softmax_scale = 30.0, 0.0625
        assert _call(_p(fn, d=256), fn, o5) >= 0, capi.last_error()
        assert _call(_p(fn, d=256, causal=True), fn, capi.kvcache_options((127, 0))) >= 0, capi.last_error()
        assert _call(_p(fn, d=256, cache=4096, page=16), fn, None) >= 0, capi.last_error()
    for d in (32, 96, 192, 512):
        for o in opts:
            assert _call(_p(fn, d=d), fn, o) == capi.FA_ERR_BAD_HEADDIM, (d, type(o))
            assert "head_dim" in capi.last_error() and str(d) in capi.last_error(), capi.last_error()


def test_prefill_entry_points_still_reject_head_dim_256():
    """fa_run_mha_fwd / fa_run_mha_bwd keep the 64 / 128 rule and its text"""
    L = capi.lib()
    buf = (ctypes.c_char * 272)()
    addr = ctypes.addressof(buf)
    addr += (-addr) % 16
    for d in (256, 96):
        p = capi.FwdParams()
        p.q = p.k = p.v = p.o = p.lse = addr
        p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d = 1, 16, 16, 2, 2, d
        p.q_stride = p.k_stride = p.v_stride = p.o_stride = capi.Strides(16 * 2 * d, 2 * d, d)
        assert L.fa_run_mha_fwd(ctypes.byref(p), None) == capi.FA_ERR_BAD_HEADDIM, d
        assert f"head_dim {d} unsupported (64 or 128)" in capi.last_error(), capi.last_error()


def test_workspace_bytes_of_a_forced_split_at_head_dim_256():
    """n_split x rows x 256 x 4 bytes of partial O plus n_split x rows x 4 of partial LSE (rounded up to 16): the rule of 64 / 128, written in d"""
    for (b, sq, h, hk, ns) in ((1, 1, 32, 8, 5), (3, 4, 8, 2, 2), (2, 17, 8, 1, 7), (1, 1, 4, 4, 128)):
        rows = b * h * sq
        want = ns * rows * 256 * 4 + (ns * rows * 4 + 15) // 16 * 16
        assert want == ns * rows * 256 * 4 + ns * rows * 4 or (ns * rows) % 4 != 0
        p = _params(b=b, sq=sq, h=h, hk=hk, d=256, cache=32768, num_splits=ns)
        assert capi.kvcache_workspace_bytes(p) == want, (b, sq, h, hk, ns)
        assert _rc(p, "fa_kvcache_workspace_bytes_ex", capi.KvcacheOptionsV5()) == want
        assert capi.kvcache_num_splits(_params(b=b, sq=sq, h=h, hk=hk, d=256, cache=32768, num_splits=ns, ws_bytes=want)) == ns
        # twice the bytes of the same call at head_dim 128, up to the LSE planes
        p128 = _params(b=b, sq=sq, h=h, hk=hk, d=128, cache=32768, num_splits=ns)
        lse = (ns * rows * 4 + 15) // 16 * 16
        assert capi.kvcache_workspace_bytes(p) - lse == 2 * (capi.kvcache_workspace_bytes(p128) - lse)
    # the automatic split does not depend on d (it is sized from the launch and the capacity): same count as at 128
    for kw in (dict(b=1, h=32, hk=8, cache=32768), dict(b=2, h=8, hk=1, cache=4096), dict(b=1, sq=4, h=32, hk=8, cache=131072)):
        assert capi.kvcache_num_splits(_params(d=256, ws_bytes=1 << 40, **kw)) == capi.kvcache_num_splits(_params(d=128, ws_bytes=1 << 40, **kw)), kw


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_fp8_alignment_rules_are_unchanged_at_head_dim_256(fn):
    """an 8-bit d-256 cache keeps the 16-element stride rule; a 16-bit one the 8-element rule"""
    d, hk, cache = 256, 8, 4096
    o8 = capi.KvcacheOptionsV2()
    o8.cache_dtype = FP8
    for which in ("k_cache_stride", "v_cache_stride"):
        for st in (capi.Strides(cache * hk * d + 8, hk * d, d), capi.Strides(cache * hk * d, hk * d + 8, d), capi.Strides(cache * hk * d, hk * d, d + 8),
                   capi.Strides(cache * hk * d, 128, d)):
            p = _params(d=d, hk=hk, cache=cache)
            setattr(p, which, st)
            assert _rc(p, fn, o8) == capi.FA_ERR_BAD_STRIDE, (which, st.batch, st.row, st.head)
            assert "16" in capi.last_error() and which[:7] in capi.last_error()
        p = _params(d=d, hk=hk, cache=cache)
        setattr(p, which, capi.Strides(cache * hk * d + 8, hk * d + 8, d + 8))
        assert _rc(p, fn, capi.KvcacheOptionsV2()) >= 0, capi.last_error()
        setattr(p, which, capi.Strides(cache * hk * d + 16, hk * d + 16, d + 16))
        assert _rc(p, fn, o8) >= 0, capi.last_error()


def test_rotary_dim_may_reach_256_through_the_c_abi():
    buf = (ctypes.c_char * 272)()
    addr = ctypes.addressof(buf)
    addr += (-addr) % 16

    def rc(rotary_dim, d):
        p = _params(d=d, cache=64)
        p.k_new = p.v_new = addr
        p.seqlen_new = 1
        p.k_new_stride = p.v_new_stride = capi.Strides(8 * d, 8 * d, d)
        o = capi.KvcacheOptionsV3()
        o.rotary_cos = o.rotary_sin = addr
        o.rotary_dim, o.seqlen_ro, o.rotary_row_stride = rotary_dim, 64, rotary_dim // 2 // 8 * 8 + 8
        return _rc(p, "fa_kvcache_workspace_bytes_ex", o)

    for rd in (16, 64, 240, 256):
        assert rc(rd, 256) >= 0, (rd, capi.last_error())
    for rd in (272, 264, 512, 8):
        assert rc(rd, 256) == capi.FA_ERR_BAD_SHAPE and "rotary_dim" in capi.last_error(), rd
    assert rc(256, 128) == capi.FA_ERR_BAD_SHAPE
    # the rotated-q image at the head of the workspace is written in d as well: b x seqlen_q x h x 256 x 2 bytes
    assert rc(256, 256) == 1 * 1 * 32 * 256 * 2


def test_abi_version_and_feature_macro(tmp_path):
    assert capi.lib().fa_abi_version() == 4
    src = tmp_path / "has_d256.c"
    src.write_text(r"""
#include <stdio.h>
#include "flash_attn_gfx950.h"
#ifndef FA_HAS_KVCACHE_HEADDIM256
#error "no FA_HAS_KVCACHE_HEADDIM256"
#endif
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.b = 0; p.seqlen_q = 1; p.seqlen_cache = 64; p.h = 4; p.h_k = 2; p.d = 256; p.dtype = FA_BF16;
    if (FA_HAS_KVCACHE_HEADDIM256 != 1) return 10;
    if (fa_run_mha_fwd_kvcache(&p, NULL) != FA_OK) return 11;
    p.d = 192;
    if (fa_run_mha_fwd_kvcache(&p, NULL) != FA_ERR_BAD_HEADDIM) return 12;
    fa_fwd_params f;
    FA_PARAMS_INIT(f);
    f.b = 0; f.seqlen_q = 1; f.seqlen_k = 1; f.h = 4; f.h_k = 2; f.d = 256; f.dtype = FA_FP16;
    if (fa_run_mha_fwd(&f, NULL) != FA_ERR_BAD_HEADDIM) return 13;
    if (fa_abi_version() != 4 || FA_ABI_VERSION != 4) return 14;
    if (sizeof(fa_kvcache_options) != 20 || sizeof(fa_kvcache_options_v2) != 72 || sizeof(fa_kvcache_options_v3) != 112 || sizeof(fa_kvcache_options_v4) != 144 ||
        sizeof(fa_kvcache_options_v5) != 168) return 15;
    return 0;
}
""")
    exe = tmp_path / "has_d256"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


# ---- 2. Python surface ------------------------------------------------------------------------------------------------------------------

def test_python_surface_names_the_head_dims():
    """a d-192 (or 96) cache and a rotary_dim of 272 at d 256 are ValueErrors that need no device; a d-256 call that passes the checks is
    refused by the extension for its CPU tensors (no quiet fall-back), as at 64 / 128.  (The 16-element stride rule of an FP8 view is the
    C library's: test_fp8_alignment_rules_are_unchanged_at_head_dim_256 here, and through Python on the GPU in test_kvcache_d256_gpu.py.)"""
    import flash_attn_turing as F

    b, hk, h, cap = 2, 2, 4, 32
    for d in (192, 96, 32, 512):
        q = torch.zeros(b, 1, h, d, dtype=torch.float16)
        c = torch.zeros(b, cap, hk, d, dtype=torch.float16)
        with pytest.raises(ValueError, match=f"head_dim {d} unsupported.*64, 128 and 256"):
            F.flash_attn_with_kvcache(q, c, c, cache_seqlens=4)
        with pytest.raises(ValueError, match="head_dim"):
            F.flash_attn_with_kvcache(q.view(b, h, d), c, c, cache_seqlens=4, cu_seqlens_q=torch.arange(b + 1, dtype=torch.int32), max_seqlen_q=1)
    d = 256
    q = torch.zeros(b, 1, h, d, dtype=torch.float16)
    c = torch.zeros(b, cap, hk, d, dtype=torch.float16)
    kn = torch.zeros(b, 1, hk, d, dtype=torch.float16)
    for half in (136, 132, 256, 4):                         # rotary_dim 272, 264, 512: > d or no multiple of 16; 8: too small
        t = torch.zeros(cap, half, dtype=torch.float16)
        with pytest.raises(ValueError, match=r"rotary_dim .* head_dim \(256\)"):
            F.flash_attn_with_kvcache(q, c, c, k=kn, v=kn, cache_seqlens=4, rotary_cos=t, rotary_sin=t)
    for half in (128, 32):                                  # rotary_dim 256 and 64 pass the Python checks
        t = torch.zeros(cap, half, dtype=torch.float16)
        with pytest.raises(RuntimeError, match="GPU"):
            F.flash_attn_with_kvcache(q, c, c, k=kn, v=kn, cache_seqlens=4, rotary_cos=t, rotary_sin=t)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(q, c, c, cache_seqlens=4)
    c8 = torch.zeros(b, cap, hk, d, dtype=torch.uint8).view(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(q, c8, c8, cache_seqlens=4, k_descale=torch.ones(b, hk), softcap=30.0)
    assert "64 / 128 / 256" in F.flash_attn_with_kvcache.__doc__


# ---- 3. kernel resources ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def kernels():
    from _kernel_isa import analyse

    return analyse("fa_fwd_kvcache_d256.hip")


ATTN = r"fa_fwd_kvcache_d256_(ragged_)?(softcap_)?kernelI(DF16_|DF16b)(?:Li2E)?Lb(\d)ELi(\d)E"


def test_d256_file_is_built_guarded_and_holds_exactly_its_56_kernels(kernels):
    """32 attention kernels - {fp16, bf16} x {contiguous, paged} x {16-bit, FP8} x {dense, ragged} x {plain, softcap}, the window instantiation
    serving plain and causal calls - 6 + 6 append, 2 + 2 combine, 8 rotary; every one without scratch, MFMA hazards or M0 use"""
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_kvcache_d256.hip" in B.HIP_SOURCES and "fa_fwd_kvcache_d256.hip" in B.M0_GUARD_SOURCES
    count = lambda pat: len([n for n in kernels if re.search(pat, n)])
    keys = {re.search(ATTN, n).groups() for n in kernels if re.search(ATTN, n)}
    assert keys == {(r, s, t, p, e) for r in (None, "ragged_") for s in (None, "softcap_") for t in ("DF16_", "DF16b") for p in "01" for e in "12"}
    assert count(ATTN) == 32
    assert count(r"\d+fa_kvcache_append_kernelILi256E") == 1 and count(r"\d+fa_kvcache_append_paged_kernelILi256E") == 1
    assert count(r"\d+fa_kvcache_append_fp8_kernelI(DF16_|DF16b)Li256E") == 4
    assert count(r"\d+fa_kvcache_append_ragged_kernelI(DF16_|DF16b)Li256E") == 6
    assert count(r"\d+fa_kvcache_combine_kernelI(DF16_|DF16b)Li256E") == 2 and count(r"\d+fa_kvcache_combine_ragged_kernelI(DF16_|DF16b)Li256E") == 2
    assert count(r"\d+fa_kvcache_rotary_kernelI(DF16_|DF16b)Li256E") == 8
    assert len(kernels) == 56, sorted(kernels)
    assert not [n for n in kernels if re.search(r"Li(64|128)E", n)], "a head_dim 64 / 128 kernel compiled a second time"
    for n, k in kernels.items():
        assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
        assert k["mfma_hazards"] == [], (n, k["mfma_hazards"][:3])
        assert k["m0_outside_asm"] == 0, n
        if not re.search(ATTN, n):
            assert k["mfma_total"] == 0 and k["lds_bytes"] == 0 and k["agprs"] == 0, n


def test_d256_attention_kernels_run_one_workgroup_per_cu_without_spills_or_moves(kernels):
    """the shipped shape: one 4-wave workgroup per compute unit - VGPRs + AGPRs <= 512, occupancy >= 1, LDS <= 160 KiB - and an MFMA loop with
    neither scratch traffic nor accumulator-register moves; the 16x16x32 MFMA of the dtype; the FP8 kernels widen with the conversion of
    their dtype and use no FP8 MFMA"""
    import build as B

    src = os.path.join(B.CSRC, "fa_fwd_kvcache_d256.hip")
    asm = subprocess.run([B.hipcc_path()] + B.HIPCC_FLAGS + B.EXTRA_FLAGS.get("fa_fwd_kvcache_d256.hip", []) +
                         ["-I", B.CSRC, "-I", B.INCLUDE, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    assert B.m0_uses_outside_asm(asm) == 0
    assert len(re.findall(r"^\s*\.amdhsa_kernel ", asm, re.M)) == 56
    attn = {n: k for n, k in kernels.items() if re.search(ATTN, n)}
    assert len(attn) == 32
    for n, k in attn.items():
        ragged, softcap, t, paged, es = re.search(ATTN, n).groups()
        assert k["vgprs"] + k["agprs"] <= 512 and k["vgprs"] <= 256 and k["agprs"] <= 256, (n, k["vgprs"], k["agprs"])
        assert k["occupancy"] >= 1 and k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"], k["lds_bytes"])
        assert k["lds_bytes"] == 4 * 16 * (256 + 4) * 4 + 2 * 4 * 16 * 4 == 67072, (n, k["lds_bytes"])     # the merge planes (the four V images are 65536)
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        assert main["mfma"] == 64, (n, main["mfma"])            # two 32-key steps: 2 x (2 x 8 QK + 16 PV)
        assert main["ds_read_tr"] == 64 and "buffer_load_dwordx4" in main["histogram"], n
        body = asm[asm.index(n + ":"):]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
        mfma = "v_mfma_f32_16x16x32_bf16" if t == "DF16b" else "v_mfma_f32_16x16x32_f16"
        assert mfma in main["histogram"] and set(re.findall(r"v_mfma\w+", body)) == {mfma}, (n, set(re.findall(r"v_mfma\w+", body)))
        cvt = "v_cvt_scalef32_pk_bf16_fp8" if t == "DF16b" else "v_cvt_scalef32_pk_f16_fp8"
        if es == "1":
            assert main["histogram"].get(cvt, 0) >= 2 * 128, (n, main["histogram"].get(cvt))     # K and V of two 32-key steps: 2 x (32 x 256 x 2 / 64 / 2) conversions a lane
            assert not re.search(r"v_mfma\w*(fp8|bf8|f8f6f4)", body), n
        else:
            assert "v_cvt_scalef32" not in body, n
        if softcap:
            n_rcp = sum(c for op, c in main["histogram"].items() if op.startswith("v_rcp_f32"))
            n_exp = sum(c for op, c in main["histogram"].items() if op.startswith("v_exp_f32"))
            assert n_rcp >= 16 and n_exp >= 32, (n, n_rcp, n_exp)
