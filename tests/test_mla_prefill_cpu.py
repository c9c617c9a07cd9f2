"""CPU: MLA prefill attention (flash_mla_prefill_func, fa_mla_prefill_params / fa_run_mla_prefill_fwd of the C ABI) - the fp64 model the GPU tests use
against torch's fp64 SDPA, the struct against the header, every refusal of the Python function and of the C entry point with the argument it names,
and the resources of the kernels of fa_fwd_mla_prefill.hip.  No GPU involved."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import _mla_prefill_cases as C

TILE_ROWS = 128                 # the tile that ships: four waves of two 16-row query column blocks
LDS_BYTES = 2 * (32 * 256 + 32 * 128 + 32 * 256)        # two stages of a wide K image, a narrow K image and a V image: 40 KB


# ---- 1. the expectation ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("heads", C.HEADS, ids=lambda x: f"h{x[0]}_{x[1]}")
def test_model_equals_fp64_sdpa_with_an_explicit_mask(heads, causal):
    """every shape of the GPU tests, both dtypes' inputs: _util.fp64_math on (192, 128) widths is SDPA in fp64 under the bottom-right mask, and its
    dead rows are exactly the rows the mask leaves empty (O = 0, LSE = 0)"""
    h, hk = heads
    shapes = list(C.SHAPES) + list(zip(C.PACKED_SQ, C.PACKED_SK))
    for n, (sq, sk) in enumerate(shapes):
        for dtname in C.DTYPES:
            q, k, v = (t[0] for t in C.inputs(sq, sk, h, hk, dtname, 100 + n))
            o, lse = C.model(q, k, v, causal)
            want, mask = C.sdpa(q, k, v, causal)
            assert o.shape == (sq, h, C.DV) and lse.shape == (h, sq) and o.dtype == torch.float64
            assert torch.isfinite(o).all() and torch.isfinite(lse).all()
            if o.numel():
                assert (o - want).abs().max().item() <= 1e-12, (sq, sk, dtname, (o - want).abs().max().item())
            dead = ~mask.any(-1)
            assert dead.tolist() == [causal and t < sq - sk or sk == 0 for t in range(sq)]
            assert (o[dead] == 0).all() and (lse[:, dead] == 0).all()
            if sk and (~dead).any():
                s = C.scores64(q.unsqueeze(0), k.unsqueeze(0))[0].masked_fill(~mask, float("-inf"))
                assert (torch.logsumexp(s[:, ~dead], -1) - lse[:, ~dead]).abs().max().item() <= 1e-12


def test_packed_model_is_the_sequences_side_by_side():
    q, k, v, cu_q, cu_k = C.packed_inputs(C.PACKED_SQ, C.PACKED_SK, 6, 2, "bf16", 7)
    o, lse = C.packed_model(q, k, v, cu_q, cu_k, True)
    assert o.shape == (sum(C.PACKED_SQ), 6, C.DV) and lse.shape == (6, sum(C.PACKED_SQ))
    o3, l3 = C.model(q[18:82], k[38:135], v[38:135], True)           # sequence 3: rows 18 .. 81, keys 38 .. 134
    assert torch.equal(o[18:82], o3) and torch.equal(lse[:, 18:82], l3)
    assert (o[1:2] == 0).all() and (lse[:, 1:2] == 0).all()           # sequence 1 has no key


# ---- 2. the Python surface ------------------------------------------------------------------------------------------------------------------

def test_surface_and_refusals_before_any_device_work():
    import flash_attn_turing as F

    assert "flash_mla_prefill_func" in F.__all__ and F.flash_mla_prefill_func is F.interface.flash_mla_prefill_func
    sig = inspect.signature(F.flash_mla_prefill_func)
    names = list(sig.parameters)
    assert names[:3] == ["q", "k", "v"]
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[3:])
    assert set(names[3:]) == {"cu_seqlens_q", "cu_seqlens_k", "softmax_scale", "causal", "return_softmax_lse"}
    for gone in ("max_seqlen_q", "max_seqlen_k", "window_size", "softcap", "sinks", "num_splits", "block_table"):
        assert gone not in names

    call = F.flash_mla_prefill_func
    bf, hf = torch.bfloat16, torch.float16
    b, sq, sk, h, hk = 2, 5, 9, 4, 2
    q, k, v = torch.zeros(b, sq, h, 192, dtype=bf), torch.zeros(b, sk, hk, 192, dtype=bf), torch.zeros(b, sk, hk, 128, dtype=bf)
    with pytest.raises(TypeError):
        call(q, k, v, True)
    # widths
    for bad_q, bad_k, bad_v, word in ((torch.zeros(b, sq, h, 128, dtype=bf), k, v, "q must be 192 wide"), (torch.zeros(b, sq, h, 576, dtype=bf), k, v, "q must be 192 wide"),
                                      (q, torch.zeros(b, sk, hk, 128, dtype=bf), v, "k must be 192 wide"), (q, k, torch.zeros(b, sk, hk, 192, dtype=bf), "v must be 128 wide"),
                                      (q, k, torch.zeros(b, sk, hk, 64, dtype=bf), "v must be 128 wide")):
        with pytest.raises(ValueError, match=word):
            call(bad_q, bad_k, bad_v)
    # dtypes
    with pytest.raises(ValueError, match="q must be fp16 or bf16"):
        call(q.float(), k.float(), v.float())
    with pytest.raises(ValueError, match="k must have q's dtype"):
        call(q, k.to(hf), v)
    with pytest.raises(ValueError, match="v must have q's dtype"):
        call(q, k, v.to(hf))
    # heads and shapes
    with pytest.raises(ValueError, match="nheads of q"):
        call(torch.zeros(b, sq, 3, 192, dtype=bf), k, v)
    with pytest.raises(ValueError, match="k and v must agree"):
        call(q, k, torch.zeros(b, sk + 1, hk, 128, dtype=bf))
    with pytest.raises(ValueError, match="batch"):
        call(q, k[:1], v[:1])
    with pytest.raises(ValueError, match="q must be a rank-4 tensor"):
        call(q[0], k, v)
    # views: refused, never copied
    wide = torch.zeros(b, sq, h, 200, dtype=bf)
    with pytest.raises(ValueError, match="q: the last dimension must be contiguous"):
        call(torch.zeros(b, sq, 192, h, dtype=bf).transpose(2, 3), k, v)
    with pytest.raises(ValueError, match="q: strides"):
        call(torch.zeros(b, sq, h, 196, dtype=bf)[..., :192], k, v)                 # a head stride of 196 elements
    with pytest.raises(ValueError, match="q: strides .* storage offset 4"):
        call(wide[..., 4:196], k, v)
    with pytest.raises(ValueError, match="k: strides"):
        call(q, torch.zeros(b, sk, hk, 196, dtype=bf)[..., :192], v)
    with pytest.raises(ValueError, match="v: strides .* storage offset 1"):
        call(q, k, torch.zeros(b * sk * hk * 128 + 8, dtype=bf)[1:1 + b * sk * hk * 128].view(b, sk, hk, 128))
    # cu_seqlens: both or neither, int32, (b + 1,)
    q3, k3, v3 = q.flatten(0, 1), k.flatten(0, 1), v.flatten(0, 1)
    cq, ck = C.cu((sq, sq)), C.cu((sk, sk))
    with pytest.raises(ValueError, match="come both or neither, got only cu_seqlens_q"):
        call(q3, k3, v3, cu_seqlens_q=cq)
    with pytest.raises(ValueError, match="come both or neither, got only cu_seqlens_k"):
        call(q3, k3, v3, cu_seqlens_k=ck)
    with pytest.raises(ValueError, match="q must be a rank-3 tensor"):
        call(q, k, v, cu_seqlens_q=cq, cu_seqlens_k=ck)
    with pytest.raises(ValueError, match="cu_seqlens_q must be an int32 tensor"):
        call(q3, k3, v3, cu_seqlens_q=cq.long(), cu_seqlens_k=ck)
    with pytest.raises(ValueError, match="cu_seqlens_k must have shape"):
        call(q3, k3, v3, cu_seqlens_q=cq, cu_seqlens_k=ck[:2])
    # the scale: the validation of flash_mla_with_kvcache
    for bad in (0, 0.0, float("nan"), float("inf"), -1.0, True, False, "1", 1e-60):
        with pytest.raises(ValueError, match="softmax_scale"):
            call(q, k, v, softmax_scale=bad)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(ValueError, match="causal must be a bool"):
            call(q, k, v, causal=bad)
    # there is no backward
    for i, name in enumerate("qkv"):
        t = [q, k, v]
        t[i] = t[i].clone().requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} requires grad"):
            call(*t)
        with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
            call(*t)                                                                # (a disabled grad mode: the same call passes the checks)
    # a CPU call that passes the checks is refused by the extension (no quiet fall-back)
    for kw in (dict(), dict(causal=True), dict(softmax_scale=0.1, return_softmax_lse=True)):
        with pytest.raises(RuntimeError, match="GPU"):
            call(q, k, v, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q3.to(hf), k3.to(hf), v3.to(hf), cu_seqlens_q=cq, cu_seqlens_k=ck, causal=True)
    with pytest.raises(RuntimeError, match="GPU"):
        call(torch.zeros(b, sq, h, 200, dtype=bf)[..., 8:200], k, v)               # an aligned view passes
    doc = call.__doc__
    assert "192" in doc and "128" in doc and "Out of scope" in doc and "cu_seqlens_q" in doc


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------------------

def test_params_layout_matches_header(tmp_path):
    from flash_attn_turing import capi

    fields = [f[0] for f in capi.MlaPrefillParams._fields_]
    assert fields == ["struct_size", "magic", "q", "k", "v", "o", "lse", "cu_seqlens_q", "cu_seqlens_k", "b", "seqlen_q", "seqlen_k", "h", "h_k", "d_qk", "d_v", "dtype",
                      "is_causal", "softmax_scale", "q_stride", "k_stride", "v_stride", "o_stride", "total_q", "total_k"]
    src = tmp_path / "mlap_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_PREFILL\n#error "no FA_HAS_MLA_PREFILL"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu 0\\n", sizeof(fa_mla_prefill_params));\n'
                   '    printf("abi %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_PREFILL);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_mla_prefill_params, {f}), sizeof(((fa_mla_prefill_params*)0)->{f}));\n' for f in fields)
                   + "    fa_mla_prefill_params p;\n    FA_PARAMS_INIT(p);\n"
                     "    return p.struct_size == sizeof(p) && p.magic == FA_PARAMS_MAGIC && p.cu_seqlens_q == NULL && p.softmax_scale == 0.0f && p.total_k == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "mlap_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"][0] == ctypes.sizeof(capi.MlaPrefillParams) == 216
    assert got["abi"] == [4, 1] and capi.lib().fa_abi_version() == 4
    for f in fields:
        assert got[f] == [getattr(capi.MlaPrefillParams, f).offset, getattr(capi.MlaPrefillParams, f).size], f
    assert "fa_run_mla_prefill_fwd" in capi.declared_functions() and hasattr(capi.lib(), "fa_run_mla_prefill_fwd")


def test_plain_c_caller_every_refusal_names_its_field(tmp_path):
    """codes with the argument in fa_last_error; b = 0 and total_q = 0 are FA_OK without a launch (no device is touched: every call here ends in the
    host checks)"""
    from flash_attn_turing import capi

    src = tmp_path / "use_mlap.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
#ifndef FA_HAS_MLA_PREFILL
#error "no FA_HAS_MLA_PREFILL"
#endif
static _Alignas(16) char mem[256];
static void fill(fa_mla_prefill_params* p) {
    FA_PARAMS_INIT(*p);
    p->q = p->k = p->v = p->o = mem; p->lse = (float*)mem;
    p->b = 2; p->seqlen_q = 128; p->seqlen_k = 256; p->h = 16; p->h_k = 4; p->d_qk = 192; p->d_v = 128; p->dtype = FA_BF16; p->is_causal = 1;
    p->q_stride = (fa_strides){128 * 16 * 192, 16 * 192, 192};
    p->o_stride = (fa_strides){128 * 16 * 128, 16 * 128, 128};
    p->k_stride = (fa_strides){256 * 4 * 192, 4 * 192, 192};
    p->v_stride = (fa_strides){256 * 4 * 128, 4 * 128, 128};
}
static void pack(fa_mla_prefill_params* p) {
    p->cu_seqlens_q = p->cu_seqlens_k = (const int32_t*)mem; p->total_q = 256; p->total_k = 512;
}
#define CODE(field_change, code, word, ret) do { fa_mla_prefill_params t; fill(&t); field_change; \
    if (fa_run_mla_prefill_fwd(&t, NULL) != (code) || !strstr(fa_last_error(), word)) { fprintf(stderr, "%d: %s\n", ret, fa_last_error()); return ret; } } while (0)
int main(void) {
    fa_mla_prefill_params p;
    if (sizeof(p) != 216) return 9;
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
    CODE(t.q = mem + 8, FA_ERR_BAD_STRIDE, "q base pointer", 41);
    CODE(t.q_stride.head = 196, FA_ERR_BAD_STRIDE, "q strides", 42);
    CODE(t.k_stride.row = 188, FA_ERR_BAD_STRIDE, "k strides", 43);               /* a row stride below the row's width */
    CODE(t.v_stride.batch = 12, FA_ERR_BAD_STRIDE, "v strides", 44);
    CODE(t.o_stride.row = 120, FA_ERR_BAD_STRIDE, "o strides", 45);
    CODE(t.k_stride.row = 1 << 23, FA_ERR_BAD_STRIDE, "k: one sequence spans", 46);   /* 256 rows x 16 MiB: the limit of fa_run_mha_fwd */
    CODE((pack(&t), t.total_k = 1 << 22), FA_ERR_BAD_STRIDE, "k: one sequence spans", 47);      /* packed: the whole tensor */
    CODE((t.seqlen_q = 1 << 30, t.h = 4, t.h_k = 1), FA_ERR_BAD_SHAPE, "call too large", 48);
    CODE(t.struct_size = 208, FA_ERR_BAD_ABI, "struct_size", 49);
    CODE(t.magic = 0, FA_ERR_BAD_ABI, "magic", 50);
    if (fa_run_mla_prefill_fwd(NULL, NULL) != FA_ERR_NULL_POINTER) return 51;
    /* nothing to do: FA_OK without a launch, whatever the pointers hold */
    fill(&p); p.b = 0; p.q = p.k = p.v = p.o = NULL; p.lse = NULL;
    if (fa_run_mla_prefill_fwd(&p, NULL) != FA_OK) return 60;
    fill(&p); pack(&p); p.total_q = 0; p.q = p.o = NULL; p.lse = NULL;
    if (fa_run_mla_prefill_fwd(&p, NULL) != FA_OK) return 61;
    fill(&p); p.seqlen_q = 0; p.q = p.o = NULL;
    if (fa_run_mla_prefill_fwd(&p, NULL) != FA_OK) return 62;
    if (fa_abi_version() != 4) return 63;
    return 0;
}
""")
    exe = tmp_path / "use_mlap"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_ctypes_params_of_dense_and_packed_tensors():
    from flash_attn_turing import capi

    q, k, v = torch.zeros(2, 5, 4, 192, dtype=torch.float16), torch.zeros(2, 9, 2, 192, dtype=torch.float16), torch.zeros(2, 9, 2, 128, dtype=torch.float16)
    o, lse = torch.zeros(2, 5, 4, 128, dtype=torch.float16), torch.zeros(2, 4, 5)
    p = capi.mla_prefill_params(q, k, v, o, lse, causal=True)
    assert (p.b, p.seqlen_q, p.seqlen_k, p.h, p.h_k, p.d_qk, p.d_v, p.dtype, p.is_causal) == (2, 5, 9, 4, 2, 192, 128, capi.FA_FP16, 1)
    assert (p.k_stride.batch, p.k_stride.row, p.k_stride.head) == (9 * 2 * 192, 2 * 192, 192) and p.softmax_scale == 0.0 and not p.cu_seqlens_q
    cq, ck = C.cu((5, 5)), C.cu((9, 0))
    p = capi.mla_prefill_params(q.flatten(0, 1), k.flatten(0, 1), v.flatten(0, 1), o.flatten(0, 1), lse.permute(1, 0, 2).reshape(4, 10), cq, ck, softmax_scale=0.25)
    assert (p.b, p.total_q, p.total_k, p.h, p.h_k) == (2, 10, 18, 4, 2) and p.cu_seqlens_q == cq.data_ptr() and p.cu_seqlens_k == ck.data_ptr()
    assert (p.v_stride.row, p.v_stride.head) == (2 * 128, 128) and p.softmax_scale == 0.25


# ---- 4. ISA -----------------------------------------------------------------------------------------------------------------------------------

def test_mla_prefill_kernels_isa():
    """8 attention kernels ({fp16, bf16} x {plain, causal} x {dense, packed}) and nothing else.  Every one: no scratch, an MFMA loop free of scratch
    traffic and accumulator moves that reads K as rows and V^T transposed from LDS images behind a barrier, 40 KB of LDS, at least two workgroups
    (of four waves: two waves per SIMD) a compute unit by registers (243 VGPRs with two column blocks a wave) and by LDS, subnormals kept, no MFMA result read early, M0 untouched."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    assert "fa_fwd_mla_prefill.hip" in B.HIP_SOURCES and "fa_fwd_mla_prefill.hip" in B.M0_GUARD_SOURCES and "fa_fwd_mla_prefill.hip" in B.STAGE_SOURCES
    assert B.HIP_SOURCES.index("fa_fwd_mla_prefill.hip") < B.HIP_SOURCES.index("fa_capi.hip")
    ks = analyse("fa_fwd_mla_prefill.hip")
    assert len(ks) == 8, sorted(ks)
    keys = set()
    for n, k in ks.items():
        m = re.search(r"fa_fwd_mla_prefill_kernelI(DF16_|DF16b)Lb(\d)ELb(\d)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
        assert k["lds_bytes"] == LDS_BYTES == 40960, (n, k["lds_bytes"])
        assert k["occupancy"] >= 2 and 2 * k["lds_bytes"] <= 160 * 1024, (n, k["occupancy"])
        assert k["vgprs"] <= 256 and k["agprs"] == 0, (n, k["vgprs"], k["agprs"])
        assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        # a step of a wave: 2 x 6 MFMAs of S^T per column block over twelve 16-byte K row reads, 8 MFMAs of O^T per column block over sixteen transposed V reads
        assert main["mfma"] % (20 * TILE_ROWS // 64) == 0 and main["ds_read_b128"] > 0 and main["ds_read_tr"] > 0 and main["barriers"] > 0, (n, main["label"], main["mfma"])
    assert keys == {(t, c, p) for t in ("DF16_", "DF16b") for c in "01" for p in "01"}
