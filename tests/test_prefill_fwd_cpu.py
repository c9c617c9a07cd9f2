"""CPU: the surface of the prompt forward with a sliding window and attention sinks (flash_attn_prefill_func, fa_run_prefill_fwd, the build lists) and the
compiled form of its kernels (fa_fwd_prefill.hip).  No GPU: every call is refused, or returns for an empty batch, before anything is launched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import _kernel_isa
import flash_attn_turing as F
from flash_attn_turing import capi


_t = lambda *shape, dtype=torch.float16: torch.zeros(*shape, dtype=dtype)  # noqa: E731


def test_surface_and_build_lists():
    B = _kernel_isa._build
    assert "flash_attn_prefill_func" in F.__all__ and hasattr(F._C, "fwd_prefill") and F.abi_version() == 4
    sig = inspect.signature(F.flash_attn_prefill_func)
    assert [n for n, p in sig.parameters.items() if p.kind is p.POSITIONAL_OR_KEYWORD] == ["q", "k", "v"]
    assert {n: p.default for n, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == dict(
        cu_seqlens_q=None, cu_seqlens_k=None, softmax_scale=None, causal=False, window_size=(-1, -1), sinks=None, return_softmax_lse=False)
    name = "fa_fwd_prefill.hip"
    assert B.HIP_SOURCES.index(name) < B.HIP_SOURCES.index("fa_capi.hip") and name in B.STAGE_SOURCES and name in B.M0_GUARD_SOURCES
    assert "fa_fwd_prefill.hpp" in B.HIP_HEADERS
    with open(os.path.join(B.INCLUDE, "flash_attn_gfx950.h")) as f:
        header = f.read()
    assert "#define FA_HAS_PREFILL_FWD 1" in header and re.search(r"int fa_run_prefill_fwd\(const fa_prefill_fwd_params\* params, void\* stream\);", header)
    assert "fa_run_prefill_fwd" in capi.declared_functions() and hasattr(capi.lib(), "fa_run_prefill_fwd")
    assert ctypes.sizeof(capi.PrefillFwdParams) == 248      # (the library refuses any other struct_size: C_REFUSALS)


REFUSALS = [
    (dict(q=_t(1, 4, 2, 128, dtype=torch.float32)), "q must be fp16 or bf16"),
    (dict(q=_t(4, 2, 128)), "q must be a rank-4 tensor"),
    (dict(q=_t(1, 4, 2, 96), k=_t(1, 4, 2, 96), v=_t(1, 4, 2, 96)), "q must be 64 or 128 wide"),
    (dict(q=_t(1, 4, 3, 128)), "nheads of q (3) must be a positive multiple"),
    (dict(cu_seqlens_k=torch.zeros(2, dtype=torch.int32)), "got only cu_seqlens_k"),
    (dict(window_size=(-2, 0)), "each side must be >= -1"),
    (dict(sinks=torch.zeros(3)), "sinks must have shape (nheads,) = (2,)"),
    (dict(sinks=torch.zeros(2, dtype=torch.float64)), "sinks must be float32 or have q's dtype"),
    (dict(softmax_scale=0.0), "softmax_scale must be finite and > 0"),
    (dict(q=_t(1, 4, 2, 128).requires_grad_()), "q requires grad: flash_attn_prefill_func is forward-only"),
]


@pytest.mark.parametrize("change,words", REFUSALS, ids=[w[:40] for _, w in REFUSALS])
def test_python_refusals(change, words):
    args = dict(q=_t(1, 4, 2, 128), k=_t(1, 4, 2, 128), v=_t(1, 4, 2, 128))
    args.update(change)
    q, k, v = args.pop("q"), args.pop("k"), args.pop("v")
    with pytest.raises(ValueError, match=re.escape(words)):
        F.flash_attn_prefill_func(q, k, v, **args)


def _params(**kw):
    p = capi.PrefillFwdParams()
    p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d, p.dtype = 1, 8, 8, 4, 2, 128, capi.FA_BF16
    p.q, p.k, p.v, p.o, p.lse = (ADDR + (i << 20) for i in range(5))
    for name in ("q_stride", "k_stride", "v_stride", "o_stride"):
        setattr(p, name, capi.Strides(8 * 4 * 128, 4 * 128, 128))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


ADDR = 0x7F0000000000       # a fake device address, 16-byte aligned (never dereferenced by the host checks)
C_REFUSALS = [
    (dict(d=96), capi.FA_ERR_BAD_HEADDIM, "head_dim 96 unsupported (64 or 128)"),
    (dict(h=3), capi.FA_ERR_BAD_GQA, "h (3) must be divisible by h_k (2)"),
    (dict(cu_seqlens_k=ADDR), capi.FA_ERR_NULL_POINTER, "cu_seqlens_q is NULL but cu_seqlens_k is given (both or neither)"),
    (dict(softmax_scale=float("nan")), capi.FA_ERR_BAD_SHAPE, "must be finite and > 0 (0 = the default d ** -0.5)"),
    (dict(cu_seqlens_q=ADDR, cu_seqlens_k=ADDR + 256, total_k=-1), capi.FA_ERR_BAD_SHAPE, "total_k (-1)"),
    (dict(reserved_=1), capi.FA_ERR_BAD_SHAPE, "fa_prefill_fwd_params: reserved_ is not zero"),
    (dict(sinks_dtype=2), capi.FA_ERR_BAD_DTYPE, "sinks_dtype 2 unsupported"),
    (dict(struct_size=240), capi.FA_ERR_BAD_ABI, "struct_size 240 is not 248"),
    (dict(lse=0), capi.FA_ERR_NULL_POINTER, "lse is NULL"),
    (dict(sinks=ADDR + 2), capi.FA_ERR_BAD_STRIDE, "sinks must be 4-byte aligned"),
    (dict(b=0), capi.FA_OK, ""),
]


@pytest.mark.parametrize("change,code,words", C_REFUSALS, ids=[w[:40] or f"empty {list(c)[0]}" for c, _, w in C_REFUSALS])
def test_c_refusals(change, code, words):
    rc = capi.lib().fa_run_prefill_fwd(ctypes.byref(_params(**change)), None)
    assert rc == code and (code == capi.FA_OK or words in capi.last_error()), (rc, capi.last_error())


def test_kernels_as_compiled():
    """8 kernels, no scratch, no AGPRs, subnormals kept; registers, occupancy and LDS as DESIGN.md 3.26 records them (d 128: 2 waves a SIMD, 32 KB; d 64: 4,
    16 KB); the key loops hold 16x16x32 MFMAs only - 2 blocks x (d / 16 of S^T + d / 16 of O^T) a step - and no scratch traffic or accumulator moves"""
    kernels = {k: v for k, v in _kernel_isa.analyse("fa_fwd_prefill.hip").items() if "fa_fwd_prefill_kernel" in k}
    assert len(kernels) == 8
    for name, info in kernels.items():
        d = 128 if "Li128E" in name else 64
        assert info["scratch_bytes"] == 0 and info["agprs"] == 0 and info["vgprs"] <= (188 if d == 128 else 128), (name, info)
        assert info["occupancy"] == (2 if d == 128 else 4) and info["lds_bytes"] == 256 * d, (name, info)
        assert info["float_denorm_mode_32"] == 3 and info["float_denorm_mode_16_64"] == 3 and not info["mfma_hazards"], (name, info)
        assert info["loops"], name
        for loop in info["loops"]:
            assert {k for k in loop["histogram"] if "mfma" in k} <= {"v_mfma_f32_16x16x32_f16", "v_mfma_f32_16x16x32_bf16"}, (name, loop["histogram"])
            assert loop["mfma"] % (4 * d // 16) == 0 and loop["scratch_ops"] == 0 and loop["accvgpr_moves"] == 0, (name, loop["label"], loop["mfma"])
