"""CPU: the MLA prefill backward (flash_mla_prefill_bwd, flash_mla_attn_func, fa_mla_prefill_bwd_params / fa_run_mla_prefill_bwd of the C ABI) - the fp64
expectation the GPU tests use against autograd through fp64 SDPA, the struct against the header, every refusal of the Python functions and of the C
entry point with the argument it names, the resources of the kernels of fa_bwd_mla_prefill.hip, and the rounding model with its mutants.  No GPU involved."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import _accuracy as A
import _mla_prefill_bwd_cases as B
import _mla_prefill_cases as C
import _util as U

LDS_DQ = 2 * (32 * 256 + 32 * 128 + 32 * 256)               # two stages of a wide K image, a narrow K image and a V image: 40 KB
LDS_DKDV = LDS_DQ + 2 * 2 * 32 * 4                          # ... of Q / dO images plus the step's 32 lse and 32 D values: 40.5 KB


# ---- 1. the expectation ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", B.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
def test_expectation_equals_autograd_through_fp64_sdpa(heads, causal):
    """every shape of the GPU tests: forward64 is _util.fp64_math bit for bit, and autograd through it gives what autograd through fp64 SDPA under the
    explicit mask gives (dead rows: dQ = 0; keys no row sees: dK = dV = 0)"""
    h, hk = heads
    shapes = list(B.SHAPES) + list(zip(B.PACKED_SQ, B.PACKED_SK))
    for n, (sq, sk) in enumerate(shapes):
        q, k, v = (t[0] for t in C.inputs(sq, sk, h, hk, "bf16" if n % 2 else "fp16", 100 + n))
        dout = B.dout_like(q, 200 + n)
        o, _ = U.fp64_math(q, k, v, causal)
        assert torch.equal(B.forward64(q.double(), k.double(), v.double(), causal), o), (sq, sk)
        got, want = B.grads64(q, k, v, dout, causal), B.sdpa_grads64(q, k, v, dout, causal)
        for name, x, w, t in zip(("dq", "dk", "dv"), got, want, (q, k, v)):
            assert x.shape == t.shape and x.dtype == torch.float64 and torch.isfinite(x).all()
            if x.numel():
                assert (x - w).abs().max().item() <= 1e-11, (name, sq, sk, (x - w).abs().max().item())
        dead = torch.tensor([causal and t < sq - sk or sk == 0 for t in range(sq)], dtype=torch.bool)
        assert (got[0][dead] == 0).all()
        unseen = torch.tensor([sq == 0 or (causal and j > sk - 1) for j in range(sk)], dtype=torch.bool)
        assert (got[1][unseen] == 0).all() and (got[2][unseen] == 0).all()


def test_packed_expectation_is_the_sequences_side_by_side():
    q, k, v, cu_q, cu_k = C.packed_inputs(B.PACKED_SQ, B.PACKED_SK, 6, 2, "bf16", 7)
    dout = B.dout_like(q, 8)
    dq, dk, dv = B.packed_grads64(q, k, v, dout, cu_q, cu_k, True)
    assert dq.shape == q.shape and dk.shape == k.shape and dv.shape == v.shape
    one = B.grads64(q[18:82], k[38:135], v[38:135], dout[18:82], True)           # sequence 3: rows 18 .. 81, keys 38 .. 134
    assert torch.equal(dq[18:82], one[0]) and torch.equal(dk[38:135], one[1]) and torch.equal(dv[38:135], one[2])
    assert (dq[0:1] == 0).all() and (dk[:33] == 0).all() and (dv[:33] == 0).all()      # sequence 0 has no row, sequence 1 no key


# ---- 2. the Python surface ------------------------------------------------------------------------------------------------------------------

def _dense(dt=torch.float16):
    q, k, v = torch.zeros(2, 5, 4, 192, dtype=dt), torch.zeros(2, 9, 2, 192, dtype=dt), torch.zeros(2, 9, 2, 128, dtype=dt)
    return q, k, v, torch.zeros(2, 5, 4, 128, dtype=dt), torch.zeros(2, 4, 5)


def test_surface_and_refusals_before_any_device_work():
    import flash_attn_turing as F

    for name in ("flash_mla_prefill_bwd", "flash_mla_attn_func", "flash_mla_prefill_func"):
        assert name in F.__all__ and getattr(F, name) is getattr(F.interface, name)
    sig = inspect.signature(F.flash_mla_prefill_bwd)
    assert list(sig.parameters) == ["dout", "q", "k", "v", "out", "lse", "cu_seqlens_q", "cu_seqlens_k", "softmax_scale", "causal"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("cu_seqlens_q", "cu_seqlens_k", "softmax_scale", "causal"))
    sig = inspect.signature(F.flash_mla_attn_func)
    assert list(sig.parameters) == ["q", "k", "v", "cu_seqlens_q", "cu_seqlens_k", "softmax_scale", "causal", "return_softmax_lse"]
    assert "Out of scope" in F.flash_mla_prefill_bwd.__doc__ and "contiguous once" in F.flash_mla_attn_func.__doc__

    q, k, v, o, lse = _dense()
    bwd = lambda *a, **kw: F.flash_mla_prefill_bwd(*a, **kw)
    cases = [
        ("dout", lambda: bwd(o[:, :4], q, k, v, o, lse)),
        ("dout", lambda: bwd(o.float(), q, k, v, o, lse)),
        ("dout", lambda: bwd(torch.zeros(2, 5, 128, 4, dtype=q.dtype).transpose(2, 3), q, k, v, o, lse)),
        ("dout", lambda: bwd(torch.zeros(2, 5, 4, 132, dtype=q.dtype)[..., 4:], q, k, v, o, lse)),
        ("dout", lambda: bwd(o[:, :1].expand(2, 5, 4, 128), q, k, v, o, lse)),              # an expanded dout (row stride 0), as autograd delivers behind out.sum(dim=1)
        ("out", lambda: bwd(o, q, k, v, o[:, :1].expand(2, 5, 4, 128), lse)),
        ("out", lambda: bwd(o, q, k, v, torch.zeros(2, 5, 4, 192, dtype=q.dtype), lse)),
        ("out", lambda: bwd(o, q, k, v, o.bfloat16(), lse)),
        ("out", lambda: bwd(o, q, k, v, None, lse)),
        ("lse", lambda: bwd(o, q, k, v, o, lse.half())),
        ("lse", lambda: bwd(o, q, k, v, o, torch.zeros(2, 5, 4).transpose(1, 2))),
        ("lse", lambda: bwd(o, q, k, v, o, torch.zeros(2, 4, 6))),
        ("q", lambda: bwd(o, q[..., :128], k, v, o, lse)),
        ("k", lambda: bwd(o, q, k[..., :128], v, o, lse)),
        ("v", lambda: bwd(o, q, k, k, o, lse)),
        ("k", lambda: bwd(o, q, k.bfloat16(), v, o, lse)),
        ("q", lambda: bwd(o, q.float(), k, v, o, lse)),
        ("q", lambda: bwd(o, q[0], k, v, o, lse)),
        ("nheads", lambda: bwd(o, q, k[:, :, :1].expand(2, 9, 3, 192), v[:, :, :1].expand(2, 9, 3, 128), o, lse)),
        ("cu_seqlens", lambda: bwd(o[0], q[0], k[0], v[0], o[0], lse[0], cu_seqlens_q=C.cu((5,)))),
        ("softmax_scale", lambda: bwd(o, q, k, v, o, lse, softmax_scale=0.0)),
        ("softmax_scale", lambda: bwd(o, q, k, v, o, lse, softmax_scale=float("nan"))),
        ("causal", lambda: bwd(o, q, k, v, o, lse, causal=1)),
        ("q", lambda: F.flash_mla_attn_func(q[..., :128], k, v)),
        ("v", lambda: F.flash_mla_attn_func(q, k, k)),
        ("causal", lambda: F.flash_mla_attn_func(q, k, v, causal="yes")),
        ("cu_seqlens", lambda: F.flash_mla_attn_func(q[0], k[0], v[0], cu_seqlens_k=C.cu((9,)))),
    ]
    for word, fn in cases:
        with pytest.raises(ValueError, match=word):
            fn()
    # the checks passed: what is left is the extension's own refusal of CPU tensors, with and without grad
    for fn in (lambda: F.flash_mla_attn_func(q, k, v), lambda: F.flash_mla_attn_func(q, k, v, causal=True, return_softmax_lse=True),
               lambda: F.flash_mla_attn_func(q.clone().requires_grad_(True), k, v), lambda: bwd(o, q, k, v, o, lse, causal=True)):
        with pytest.raises(RuntimeError, match="GPU"):
            fn()
    # the forward-only function still refuses inputs that require grad, and now names the differentiable one
    for name in ("q", "k", "v"):
        ts = {"q": q, "k": k, "v": v}
        ts[name] = ts[name].clone().requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} requires grad") as e:
            F.flash_mla_prefill_func(ts["q"], ts["k"], ts["v"])
        assert "flash_mla_attn_func" in str(e.value)
    assert "Out of scope" in F.flash_mla_prefill_func.__doc__


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------------------

FIELDS = ["struct_size", "magic", "q", "k", "v", "o", "lse", "dout", "dq", "dk", "dv", "dsoftmax_sum", "cu_seqlens_q", "cu_seqlens_k", "b", "seqlen_q", "seqlen_k", "h",
          "h_k", "d_qk", "d_v", "dtype", "is_causal", "softmax_scale", "phases", "reserved_", "q_stride", "k_stride", "v_stride", "o_stride", "dout_stride", "dq_stride",
          "dk_stride", "dv_stride", "total_q", "total_k"]


def test_params_layout_matches_header(tmp_path):
    from flash_attn_turing import capi

    assert [f[0] for f in capi.MlaPrefillBwdParams._fields_] == FIELDS
    src = tmp_path / "mlapb_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_PREFILL_BWD\n#error "no FA_HAS_MLA_PREFILL_BWD"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu\\n", sizeof(fa_mla_prefill_bwd_params), sizeof(fa_mla_prefill_params));\n'
                   '    printf("abi %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_PREFILL_BWD);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_mla_prefill_bwd_params, {f}), sizeof(((fa_mla_prefill_bwd_params*)0)->{f}));\n' for f in FIELDS)
                   + "    fa_mla_prefill_bwd_params p;\n    FA_PARAMS_INIT(p);\n"
                     "    return p.struct_size == sizeof(p) && p.magic == FA_PARAMS_MAGIC && p.cu_seqlens_q == NULL && p.softmax_scale == 0.0f && p.phases == 0 && p.total_k == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "mlapb_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"] == [ctypes.sizeof(capi.MlaPrefillBwdParams), 216] and ctypes.sizeof(capi.MlaPrefillParams) == 216
    assert got["abi"] == [4, 1] and capi.lib().fa_abi_version() == 4
    for f in FIELDS:
        assert got[f] == [getattr(capi.MlaPrefillBwdParams, f).offset, getattr(capi.MlaPrefillBwdParams, f).size], f
    assert "fa_run_mla_prefill_bwd" in capi.declared_functions() and hasattr(capi.lib(), "fa_run_mla_prefill_bwd")


def test_plain_c_caller_every_refusal_names_its_field(tmp_path):
    """codes with the argument in fa_last_error; b = 0 and no query rows are FA_OK without a launch (no device is touched: every call here ends in the
    host checks)"""
    from flash_attn_turing import capi

    src = tmp_path / "use_mlapb.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
#ifndef FA_HAS_MLA_PREFILL_BWD
#error "no FA_HAS_MLA_PREFILL_BWD"
#endif
static _Alignas(16) char mem[256];
static void fill(fa_mla_prefill_bwd_params* p) {
    FA_PARAMS_INIT(*p);
    p->q = p->k = p->v = p->o = p->dout = mem; p->dq = p->dk = p->dv = mem; p->lse = (const float*)mem; p->dsoftmax_sum = (float*)mem;
    p->b = 2; p->seqlen_q = 128; p->seqlen_k = 256; p->h = 16; p->h_k = 4; p->d_qk = 192; p->d_v = 128; p->dtype = FA_BF16; p->is_causal = 1;
    p->q_stride = p->dq_stride = (fa_strides){128 * 16 * 192, 16 * 192, 192};
    p->o_stride = p->dout_stride = (fa_strides){128 * 16 * 128, 16 * 128, 128};
    p->k_stride = p->dk_stride = (fa_strides){256 * 4 * 192, 4 * 192, 192};
    p->v_stride = p->dv_stride = (fa_strides){256 * 4 * 128, 4 * 128, 128};
}
static void pack(fa_mla_prefill_bwd_params* p) {
    p->cu_seqlens_q = p->cu_seqlens_k = (const int32_t*)mem; p->total_q = 256; p->total_k = 512;
}
#define CODE(field_change, code, word, ret) do { fa_mla_prefill_bwd_params t; fill(&t); field_change; \
    if (fa_run_mla_prefill_bwd(&t, NULL) != (code) || !strstr(fa_last_error(), word)) { fprintf(stderr, "%d: %s\n", ret, fa_last_error()); return ret; } } while (0)
int main(void) {
    fa_mla_prefill_bwd_params p;
    if (sizeof(fa_mla_prefill_params) != 216) return 9;
    CODE(t.d_qk = 128, FA_ERR_BAD_HEADDIM, "d_qk", 20);
    CODE(t.d_qk = 576, FA_ERR_BAD_HEADDIM, "d_qk", 21);
    CODE(t.d_v = 192, FA_ERR_BAD_HEADDIM, "d_v", 22);
    CODE(t.dtype = 2, FA_ERR_BAD_DTYPE, "dtype", 23);
    CODE(t.h_k = 3, FA_ERR_BAD_GQA, "h_k", 24);
    CODE(t.h = 0, FA_ERR_BAD_SHAPE, "h=", 25);
    CODE(t.seqlen_q = -1, FA_ERR_BAD_SHAPE, "seqlen_q", 26);
    CODE(t.b = -1, FA_ERR_BAD_SHAPE, "b=", 27);
    CODE(t.softmax_scale = -1.0f, FA_ERR_BAD_SHAPE, "softmax_scale", 28);
    CODE(t.softmax_scale = 0.0f / 0.0f, FA_ERR_BAD_SHAPE, "softmax_scale", 29);
    CODE(t.softmax_scale = 1.0f / 0.0f, FA_ERR_BAD_SHAPE, "softmax_scale", 30);
    CODE(t.cu_seqlens_q = (const int32_t*)mem, FA_ERR_NULL_POINTER, "cu_seqlens_k is NULL", 31);
    CODE(t.cu_seqlens_k = (const int32_t*)mem, FA_ERR_NULL_POINTER, "cu_seqlens_q is NULL", 32);
    CODE((pack(&t), t.cu_seqlens_k = (const int32_t*)(mem + 2)), FA_ERR_BAD_STRIDE, "cu_seqlens", 33);
    CODE((pack(&t), t.total_q = -1), FA_ERR_BAD_SHAPE, "total_q", 34);
    CODE((pack(&t), t.total_k = -1), FA_ERR_BAD_SHAPE, "total_k", 35);
    CODE(t.q = NULL, FA_ERR_NULL_POINTER, "q is NULL", 36);
    CODE(t.k = NULL, FA_ERR_NULL_POINTER, "k is NULL", 37);
    CODE(t.v = NULL, FA_ERR_NULL_POINTER, "v is NULL", 38);
    CODE(t.o = NULL, FA_ERR_NULL_POINTER, "o is NULL", 39);
    CODE(t.lse = NULL, FA_ERR_NULL_POINTER, "lse is NULL", 40);
    CODE(t.dout = NULL, FA_ERR_NULL_POINTER, "dout is NULL", 41);
    CODE(t.dq = NULL, FA_ERR_NULL_POINTER, "dq is NULL", 42);
    CODE(t.dk = NULL, FA_ERR_NULL_POINTER, "dk is NULL", 43);
    CODE(t.dv = NULL, FA_ERR_NULL_POINTER, "dv is NULL", 44);
    CODE(t.dsoftmax_sum = NULL, FA_ERR_NULL_POINTER, "dsoftmax_sum is NULL", 45);
    CODE(t.q = mem + 8, FA_ERR_BAD_STRIDE, "q base pointer", 46);
    CODE(t.dout = mem + 8, FA_ERR_BAD_STRIDE, "dout base pointer", 47);
    CODE(t.dk = mem + 8, FA_ERR_BAD_STRIDE, "dk base pointer", 48);
    CODE(t.q_stride.head = 196, FA_ERR_BAD_STRIDE, "q strides", 49);
    CODE(t.k_stride.row = 188, FA_ERR_BAD_STRIDE, "k strides", 50);
    CODE(t.v_stride.batch = 12, FA_ERR_BAD_STRIDE, "v strides", 51);
    CODE(t.o_stride.row = 120, FA_ERR_BAD_STRIDE, "o strides", 52);
    CODE(t.dout_stride.row = 120, FA_ERR_BAD_STRIDE, "dout strides", 53);
    CODE(t.dq_stride.head = 196, FA_ERR_BAD_STRIDE, "dq strides", 54);
    CODE(t.dk_stride.row = 188, FA_ERR_BAD_STRIDE, "dk strides", 55);
    CODE(t.dv_stride.batch = 12, FA_ERR_BAD_STRIDE, "dv strides", 56);
    CODE(t.k_stride.row = 1 << 23, FA_ERR_BAD_STRIDE, "k: one sequence spans", 57);
    CODE(t.dv_stride.row = 1 << 23, FA_ERR_BAD_STRIDE, "dv: one sequence spans", 58);
    CODE((pack(&t), t.total_k = 1 << 22), FA_ERR_BAD_STRIDE, "k: one sequence spans", 59);
    CODE((t.seqlen_q = 1 << 30, t.h = 4, t.h_k = 1), FA_ERR_BAD_SHAPE, "call too large", 60);
    CODE(t.phases = 3, FA_ERR_BAD_SHAPE, "phases", 61);
    CODE(t.phases = -1, FA_ERR_BAD_SHAPE, "phases", 66);
    CODE(t.reserved_ = 1, FA_ERR_BAD_SHAPE, "reserved_", 62);
    CODE(t.struct_size = 216, FA_ERR_BAD_ABI, "struct_size", 63);
    CODE(t.magic = 0, FA_ERR_BAD_ABI, "magic", 64);
    if (fa_run_mla_prefill_bwd(NULL, NULL) != FA_ERR_NULL_POINTER) return 65;
    /* nothing to do: FA_OK without a launch, whatever the pointers hold */
    fill(&p); p.b = 0; p.q = p.k = p.v = p.o = p.dout = NULL; p.dq = p.dk = p.dv = NULL; p.lse = NULL; p.dsoftmax_sum = NULL;
    if (fa_run_mla_prefill_bwd(&p, NULL) != FA_OK) return 70;
    fill(&p); pack(&p); p.total_q = 0; p.q = p.o = p.dout = NULL; p.dq = NULL; p.lse = NULL;
    if (fa_run_mla_prefill_bwd(&p, NULL) != FA_OK) return 71;
    fill(&p); p.seqlen_q = 0; p.q = p.o = NULL;
    if (fa_run_mla_prefill_bwd(&p, NULL) != FA_OK) return 72;
    if (fa_abi_version() != 4) return 73;
    return 0;
}
""")
    exe = tmp_path / "use_mlapb"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_ctypes_params_of_dense_and_packed_tensors():
    from flash_attn_turing import capi

    q, k, v, o, lse = _dense()
    dq, dk, dv, dsum = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v), torch.zeros_like(lse)
    p = capi.mla_prefill_bwd_params(o, q, k, v, o, lse, dq, dk, dv, dsum, causal=True)
    assert (p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d_qk, p.d_v, p.dtype, p.is_causal, p.phases) == (2, 5, 9, 4, 2, 192, 128, capi.FA_FP16, 1, 0)
    assert (p.dk_stride.batch, p.dk_stride.row, p.dk_stride.head) == (9 * 2 * 192, 2 * 192, 192) and p.softmax_scale == 0.0 and not p.cu_seqlens_q
    assert p.dout == o.data_ptr() and p.dsoftmax_sum == dsum.data_ptr() and p.dv == dv.data_ptr()
    cq, ck = C.cu((5, 5)), C.cu((9, 0))
    f = lambda t: t.flatten(0, 1)
    p = capi.mla_prefill_bwd_params(f(o), f(q), f(k), f(v), f(o), lse.permute(1, 0, 2).reshape(4, 10), f(dq), f(dk), f(dv), dsum.view(4, 10), cq, ck, softmax_scale=0.25, phases=2)
    assert (p.b, p.total_q, p.total_k, p.h, p.h_k, p.phases) == (2, 10, 18, 4, 2, 2) and p.cu_seqlens_q == cq.data_ptr() and p.cu_seqlens_k == ck.data_ptr()
    assert (p.dv_stride.row, p.dv_stride.head, p.dout_stride.row) == (2 * 128, 128, 4 * 128) and p.softmax_scale == 0.25


# ---- 4. ISA -----------------------------------------------------------------------------------------------------------------------------------

def test_mla_prefill_bwd_kernels_isa():
    """16 kernels ({dQ, dK/dV} x {fp16, bf16} x {plain, causal} x {dense, packed}) and nothing else.  Every one: no scratch, an MFMA loop free of scratch
    traffic and accumulator moves that reads rows and transposed fragments from LDS images behind a barrier, the LDS bytes and the two workgroups a compute
    unit that DESIGN.md 3.18 states, subnormals kept, no MFMA result read early, M0 untouched."""
    from _kernel_isa import analyse
    import build as B_                                   # (on sys.path through _kernel_isa)

    name = "fa_bwd_mla_prefill.hip"
    assert name in B_.HIP_SOURCES and name in B_.M0_GUARD_SOURCES and name in B_.STAGE_SOURCES
    assert B_.HIP_SOURCES.index(name) < B_.HIP_SOURCES.index("fa_capi.hip")
    ks = analyse(name)
    assert len(ks) == 16, sorted(ks)
    keys = set()
    for n, k in ks.items():
        m = re.search(r"fa_bwd_mla_prefill_(dq|dkdv)_kernelI(DF16_|DF16b)Lb(\d)ELb(\d)E", n)
        assert m, n
        keys.add(m.groups())
        dq = m.group(1) == "dq"
        assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
        assert k["lds_bytes"] == (LDS_DQ if dq else LDS_DKDV), (n, k["lds_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"])
        assert k["vgprs"] <= 256 and k["agprs"] == 0, (n, k["vgprs"], k["agprs"])
        assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        # a step of a wave: dQ 2 x (6 + 4) MFMAs of S^T and dP^T, then 12 of dQ^T; dK/dV 2 x (6 + 4) of S and dP, then 8 of dV^T and 12 of dK^T
        assert main["mfma"] % (32 if dq else 40) == 0 and main["ds_read_b128"] > 0 and main["ds_read_tr"] > 0 and main["barriers"] > 0, (n, main["label"], main["mfma"])
    assert keys == {(w, t, c, p) for w in ("dq", "dkdv") for t in ("DF16_", "DF16b") for c in "01" for p in "01"}
    assert LDS_DQ == 40960 and LDS_DKDV == 41472


# ---- 5. the rounding model and its mutants -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def budget_case():
    """the inputs of the GPU accuracy test (fp16, causal; b 2, h 8 = h_k, sq = sk = 777) with the model's own statistics.  Causal, because D only weighs
    where a row sees few keys: with all 777 keys visible D = sum_j P_tj dP_tj averages out and a factor on it moves dS by less than its rounding does."""
    q, k, v = C.inputs(777, 777, 8, 8, "fp16", 3000, b=2)
    dout = B.dout_like(q, 3001)
    model, exact = B.rounding_model(q, k, v, dout, True, "fp16")
    return (q, k, v, dout), model, exact, [A.stats(m, e) for m, e in zip(model, exact)]


def _passes(x, exact, sm, dtname="fp16"):
    s = A.stats(x, exact)
    return abs(s["gain"]) <= A.G[dtname] and s["relrms"] <= A.RMS_FACTOR * sm["relrms"]


def test_rounding_model_meets_the_bounds_on_the_gpu_tests_inputs(budget_case):
    """the model is within the bounds it sets (|gain| <= G / 4 as budget_check asks of a case, ratio 1), per output tensor"""
    _, model, exact, sms = budget_case
    for name, m, e, sm in zip(("dQ", "dK", "dV"), model, exact, sms):
        assert abs(sm["gain"]) <= A.G["fp16"] / 4, (name, sm)
        assert _passes(m, e, sm), name


@pytest.mark.parametrize("mutant", ["truncated_ds", "d_factor", "no_scale_on_dk", "scale_off", "pair_dropped", "head_dropped"])
def test_every_mutant_fails_the_bounds(budget_case, mutant):
    """each of these is caught by the two bounds on at least one output tensor: a truncating pack of dS; D times 1 + 2^-9; softmax_scale missing on dK;
    softmax_scale off by 2^-12 (dQ and dK); one (row, key) pair of 777 dropped; one head of a GQA group left out of dK"""
    (q, k, v, dout), _, exact, sms = budget_case
    if mutant == "head_dropped":                    # needs a group: the same inputs read as h 8 over h_k 4
        k, v = k[:, :, :4].contiguous(), v[:, :, :4].contiguous()
        base, exact = B.rounding_model(q, k, v, dout, True, "fp16")
        sms = [A.stats(m, e) for m, e in zip(base, exact)]
    kw = {"truncated_ds": dict(ds_rounding="truncate"), "d_factor": dict(d_factor=1 + 2.0 ** -9), "no_scale_on_dk": dict(dk_scale=1.0),
          "scale_off": dict(scale_error=2.0 ** -12), "pair_dropped": dict(drop_pair=(400, 300)), "head_dropped": dict(drop_head=5)}[mutant]
    model, _ = B.rounding_model(q, k, v, dout, True, "fp16", **kw)
    ok = [_passes(m, e, sm) for m, e, sm in zip(model, exact, sms)]
    print(mutant, ok, [A.stats(m, e) for m, e in zip(model, exact)])
    assert not all(ok), f"the mutant {mutant} passes the accuracy bounds on dQ, dK and dV"
