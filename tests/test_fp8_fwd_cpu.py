"""CPU: the surface of the FP8 (e4m3) dense attention forward - flash_attn_fp8_func, fa_run_fp8_fwd / fa_fp8_fwd_params, the build lists - and the compiled
form of its kernels (fa_fwd_fp8.hip).  No GPU: every call is refused, or returns for an empty batch, before anything is launched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import _kernel_isa
import flash_attn_turing as F
from flash_attn_turing import capi

E4M3 = torch.float8_e4m3fn


def _t(*shape, dtype=E4M3):
    return torch.zeros(*shape, dtype=torch.uint8).view(dtype) if dtype in (E4M3, torch.float8_e5m2, torch.float8_e4m3fnuz) else torch.zeros(*shape, dtype=dtype)


def test_surface_and_build_lists():
    B = _kernel_isa._build
    assert "flash_attn_fp8_func" in F.__all__ and hasattr(F._C, "fwd_fp8") and F.abi_version() == 4
    sig = inspect.signature(F.flash_attn_fp8_func)
    assert [n for n, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD] == ["q", "k", "v"]
    assert {n: p.default for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == dict(
        q_descale=None, k_descale=None, v_descale=None, cu_seqlens_q=None, cu_seqlens_k=None, softmax_scale=None, causal=False, out_dtype=torch.bfloat16,
        return_softmax_lse=False)
    assert B.HIP_SOURCES.index("fa_fwd_fp8.hip") < B.HIP_SOURCES.index("fa_capi.hip") and "fa_fwd_fp8.hip" in B.STAGE_SOURCES and "fa_fwd_fp8.hpp" in B.HIP_HEADERS
    with open(os.path.join(B.INCLUDE, "flash_attn_gfx950.h")) as f:
        header = f.read()
    assert "#define FA_HAS_FP8_FWD 1" in header and re.search(r"int fa_run_fp8_fwd\(const fa_fp8_fwd_params\* params, void\* stream\);", header)
    assert hasattr(capi.lib(), "fa_run_fp8_fwd") and ctypes.sizeof(capi.Fp8FwdParams) == 288      # (the library refuses any other struct_size: C_REFUSALS)


REFUSALS = [
    (dict(q=_t(1, 4, 2, 128, dtype=torch.float16)), "q must be torch.float8_e4m3fn"),
    (dict(k=_t(1, 4, 2, 128, dtype=torch.float8_e4m3fnuz)), "k must be torch.float8_e4m3fn"),
    (dict(v=_t(1, 4, 2, 128, dtype=torch.float8_e5m2)), "v must be torch.float8_e4m3fn"),
    (dict(q=_t(4, 2, 128)), "q must be a rank-4 tensor"),
    (dict(q=_t(1, 4, 2, 64)), "q must be 128 wide"),
    (dict(q=_t(1, 4, 3, 128)), "nheads of q (3) must be a positive multiple"),
    (dict(k=_t(2, 4, 2, 128), v=_t(2, 4, 2, 128)), "k / v batch (2) must match q's (1)"),
    (dict(k=_t(1, 5, 2, 128)), "k and v must have one shape"),
    (dict(q=_t(1, 4, 2, 136)[..., 8:]), "q: strides"),
    (dict(q=_t(1, 4, 2, 256)[..., ::2]), "q: the last dimension must be contiguous"),
    (dict(cu_seqlens_q=torch.zeros(2, dtype=torch.int32)), "got only cu_seqlens_q"),
    (dict(q_descale=torch.ones(1, 2, dtype=torch.float64)), "q_descale must be None or a float32 tensor"),
    (dict(k_descale=torch.ones(2)), "k_descale must have shape (batch, heads) = (1, 2)"),
    (dict(out_dtype=torch.float32), "out_dtype must be torch.bfloat16 or torch.float16"),
    (dict(softmax_scale=0.0), "softmax_scale must be finite and > 0"),
    (dict(softmax_scale=True), "softmax_scale must be None or a real number"),
    (dict(causal=1), "causal must be a bool"),
]


@pytest.mark.parametrize("change,words", REFUSALS, ids=[w[:40] for _, w in REFUSALS])
def test_python_refusals(change, words):
    args = dict(q=_t(1, 4, 2, 128), k=_t(1, 4, 2, 128), v=_t(1, 4, 2, 128))
    args.update(change)
    q, k, v = args.pop("q"), args.pop("k"), args.pop("v")
    with pytest.raises(ValueError, match=re.escape(words)):
        F.flash_attn_fp8_func(q, k, v, **args)


def test_cpu_tensors_and_grad_are_refused():
    q = _t(1, 4, 2, 128)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_fp8_func(q, q, q)
    g = torch.zeros(1, 4, 2, 128, requires_grad=True)
    with pytest.raises(ValueError, match="q requires grad: flash_attn_fp8_func is forward-only"):
        F.flash_attn_fp8_func(g, q, q)


def _params(**kw):
    p = capi.Fp8FwdParams()
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.out_dtype = 1, 8, 8, 4, 2, 128, capi.FA_BF16
    p.q, p.k, p.v, p.o, p.lse = (ADDR + (i << 20) for i in range(5))
    for name in ("q_stride", "k_stride", "v_stride", "o_stride"):
        setattr(p, name, capi.Strides(8 * 4 * 128, 4 * 128, 128))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


ADDR = 0x7F0000000000       # a fake device address, 16-byte aligned (never dereferenced by the host checks)
C_REFUSALS = [
    (dict(d=64), capi.FA_ERR_BAD_HEADDIM, "d 64 unsupported"),
    (dict(h=3), capi.FA_ERR_BAD_GQA, "h (3) must be divisible by h_k (2)"),
    (dict(seqlen_q=-1), capi.FA_ERR_BAD_SHAPE, "bad sizes"),
    (dict(out_dtype=2), capi.FA_ERR_BAD_DTYPE, "out_dtype 2 unsupported"),
    (dict(cu_seqlens_q=ADDR), capi.FA_ERR_NULL_POINTER, "cu_seqlens_k is NULL but cu_seqlens_q is given (both or neither)"),
    (dict(cu_seqlens_q=ADDR + 2, cu_seqlens_k=ADDR + 256), capi.FA_ERR_BAD_STRIDE, "cu_seqlens_q / cu_seqlens_k must be 4-byte aligned"),
    (dict(softmax_scale=float("inf")), capi.FA_ERR_BAD_SHAPE, "must be finite and > 0 (0 = the default 128 ** -0.5)"),
    (dict(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR + 256, total_q=-1), capi.FA_ERR_BAD_SHAPE, "total_q (-1)"),
    (dict(reserved_=1), capi.FA_ERR_BAD_SHAPE, "fa_fp8_fwd_params: reserved_ is not zero"),
    (dict(magic=0), capi.FA_ERR_BAD_ABI, "fa_fp8_fwd_params: magic is not FA_PARAMS_MAGIC"),
    (dict(struct_size=280), capi.FA_ERR_BAD_ABI, "struct_size 280 is not 288"),
    (dict(lse=0), capi.FA_ERR_NULL_POINTER, "lse is NULL"),
    (dict(q=ADDR + 8), capi.FA_ERR_BAD_STRIDE, "q base pointer must be 16-byte aligned"),
    (dict(k_stride=capi.Strides(4096, 520, 128)), capi.FA_ERR_BAD_STRIDE, "k (e4m3) strides"),
    (dict(o_stride=capi.Strides(4096, 516, 128)), capi.FA_ERR_BAD_STRIDE, "o strides"),
    (dict(v_descale=ADDR + 2), capi.FA_ERR_BAD_STRIDE, "q_descale / k_descale / v_descale must be 4-byte aligned"),
    (dict(b=0), capi.FA_OK, ""),
]


@pytest.mark.parametrize("change,code,words", C_REFUSALS, ids=[w[:40] or "empty batch" for _, _, w in C_REFUSALS])
def test_c_refusals(change, code, words):
    rc = capi.lib().fa_run_fp8_fwd(ctypes.byref(_params(**change)), None)
    assert rc == code and (code == capi.FA_OK or words in capi.last_error()), (rc, capi.last_error())


def test_kernels_as_compiled():
    """8 kernels, each with no scratch, subnormals kept, 64 KB of LDS at two workgroups a compute unit, and a key loop whose MFMAs are all the
    16x16x128 f8f6f4 one: 16 per step (8 of S^T, 8 of O^T), free of scratch traffic and accumulator moves"""
    kernels = {k: v for k, v in _kernel_isa.analyse("fa_fwd_fp8.hip").items() if "fa_fwd_fp8_kernel" in k}
    assert len(kernels) == 8
    for name, info in kernels.items():
        assert info["scratch_bytes"] == 0 and info["agprs"] == 0 and info["vgprs"] <= 256 and info["occupancy"] == 2 and info["lds_bytes"] == 65536, (name, info)
        assert info["float_denorm_mode_32"] == 3 and info["float_denorm_mode_16_64"] == 3 and not info["mfma_hazards"], (name, info)
        assert info["loops"], name
        for loop in info["loops"]:
            assert {k for k in loop["histogram"] if "mfma" in k} == {"v_mfma_f32_16x16x128_f8f6f4"}, (name, loop["histogram"])
            assert loop["mfma"] % 16 == 0 and loop["scratch_ops"] == 0 and loop["accvgpr_moves"] == 0, (name, loop["label"], loop["mfma"])
