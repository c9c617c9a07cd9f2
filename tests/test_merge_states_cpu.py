"""CPU: merging attention states (flash_attn_merge_states, fa_merge_params / fa_run_merge_states of the C ABI) and the two calls built on it
(flash_attn_with_shared_prefix, flash_mla_chunked_prefill_func) - the fp64 model of the merge with its emptiness rule, the three signatures, every
refusal before any device work, the struct against the header, a plain C caller, and the kernels of fa_merge_states.hip.  No GPU involved."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import _merge_cases as M


# ---- 1. the model and why the emptiness rule exists -----------------------------------------------------------------------------------------

def test_model_is_attention_over_the_union_of_the_keys():
    """two halves of a key set, each with its own softmax, merged = the softmax over all keys (fp64, 1e-12)"""
    rng = np.random.default_rng(0)
    s, v = rng.standard_normal((7, 3, 40)) * 3, rng.standard_normal((40, 8))
    def part(sl):
        m = s[..., sl].max(-1, keepdims=True)
        p = np.exp(s[..., sl] - m)
        return p @ v[sl] / p.sum(-1, keepdims=True), (m + np.log(p.sum(-1, keepdims=True)))[..., 0]
    (o1, l1), (o2, l2), (o, l) = part(slice(0, 13)), part(slice(13, 40)), part(slice(0, 40))
    got_o, got_l = M.merge64([o1, o2], [l1, l2])
    assert np.abs(got_o - o).max() <= 1e-12 and np.abs(got_l - l).max() <= 1e-12
    # three parts, any order of the cut
    (oa, la), (ob, lb), (oc, lc) = part(slice(0, 5)), part(slice(5, 6)), part(slice(6, 40))
    got_o, got_l = M.merge64([oa, ob, oc], [la, lb, lc])
    assert np.abs(got_o - o).max() <= 1e-12 and np.abs(got_l - l).max() <= 1e-12


def test_emptiness_rule_and_the_former_readme_snippet():
    """the library's dead row is (O = 0, LSE = 0), not LSE = -inf: the five-op torch merge the README used to print gives a dead part the weight
    exp(0 - m) and shrinks the live part; the model leaves it out, bit for bit"""
    rng = np.random.default_rng(1)
    o_live, l_live = rng.standard_normal((4, 2, 8)), -3.0 - np.abs(rng.standard_normal((4, 2)))
    o_dead, l_dead = np.zeros((4, 2, 8)), np.zeros((4, 2))
    for outs, lses in (([o_live, o_dead], [l_live, l_dead]), ([o_dead, o_live], [l_dead, l_live]), ([o_dead, o_live, o_dead], [l_dead, l_live, -l_dead])):
        got_o, got_l = M.merge64(outs, lses)
        assert np.array_equal(got_o, o_live) and np.array_equal(got_l, l_live)
    naive_o, naive_l = M.naive_merge(torch.from_numpy(o_live), torch.from_numpy(l_live), torch.from_numpy(o_dead), torch.from_numpy(l_dead))
    assert (naive_l.numpy() > l_live + 1.0).all(), "the dead part's LSE of 0 dominates a live LSE of about -3"
    assert np.abs(naive_o.numpy()).max() < 0.5 * np.abs(o_live).max(), "and takes most of the weight away from the live rows"
    # -inf is the other empty form; all parts empty is the dead row again
    got_o, got_l = M.merge64([o_live, o_dead], [l_live, np.full((4, 2), -np.inf)])
    assert np.array_equal(got_o, o_live) and np.array_equal(got_l, l_live)
    got_o, got_l = M.merge64([o_dead, o_dead], [l_dead, np.full((4, 2), -np.inf)])
    assert (got_o == 0).all() and (got_l == 0).all()
    # the caveat: LSE = 0 with a non-zero row is a live part
    o1 = o_dead.copy(); o1[0, 0, 3] = 1.0
    got_o, got_l = M.merge64([o1, o1], [l_dead, l_dead])
    assert got_l[0, 0] == np.log(2.0) and got_l[1, 1] == 0 and got_o[0, 0, 3] == 1.0
    # NaN: that (row, head) and no other
    l_nan = l_live.copy(); l_nan[2, 1] = np.nan
    got_o, got_l = M.merge64([o_live, o_live], [l_live, l_nan])
    assert np.isnan(got_o[2, 1]).all() and np.isnan(got_l[2, 1]) and np.isfinite(np.delete(got_l.ravel(), 5)).all()
    o_nan = o_live.copy(); o_nan[1, 0, 7] = np.nan
    got_o, got_l = M.merge64([o_nan, o_live], [l_live, l_live])
    assert np.isnan(got_o[1, 0]).all() and np.isnan(got_l[1, 0]) and np.isfinite(np.delete(got_l.ravel(), 2)).all()
    got_o, got_l = M.merge64([o_nan, o_live], [np.full((4, 2), -np.inf), l_live])      # a NaN in an EMPTY part's row is never read into a result
    assert np.array_equal(got_o, o_live) and np.array_equal(got_l, l_live)


# ---- 2. the Python surface ------------------------------------------------------------------------------------------------------------------

def test_signatures_and_exports():
    import flash_attn_turing as F

    for name in ("flash_attn_merge_states", "flash_attn_with_shared_prefix", "flash_mla_chunked_prefill_func"):
        assert name in F.__all__ and getattr(F, name) is getattr(F.interface, name)
    assert list(inspect.signature(F.flash_attn_merge_states).parameters) == ["outs", "lses"]
    sig = inspect.signature(F.flash_attn_with_shared_prefix)
    names = list(sig.parameters)
    assert names[:7] == ["q", "k_cache", "v_cache", "shared_prefix_len", "k", "v", "cache_seqlens"]
    assert all(sig.parameters[n].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for n in names[:7])
    assert set(names[7:]) == {"block_table", "causal", "softmax_scale", "k_descale", "v_descale", "return_softmax_lse"}
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[7:])
    for gone in ("window_size", "rotary_cos", "sinks", "tree_mask", "cu_seqlens_q", "softcap", "num_splits", "prefill"):
        assert gone not in names
    sig = inspect.signature(F.flash_mla_chunked_prefill_func)
    names = list(sig.parameters)
    assert names[:5] == ["q", "k_ctx", "v_ctx", "k_new", "v_new"]
    assert set(names[5:]) == {"cu_seqlens_q", "cu_seqlens_k_ctx", "softmax_scale", "return_softmax_lse"}
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[5:])
    for f in (F.flash_attn_merge_states, F.flash_attn_with_shared_prefix, F.flash_mla_chunked_prefill_func):
        assert "empt" in f.__doc__ and ("Out of scope" in f.__doc__ or "out of scope" in f.__doc__)


def test_merge_refusals_before_any_device_work():
    import flash_attn_turing as F

    call = F.flash_attn_merge_states
    hf, bf = torch.float16, torch.bfloat16
    o, l = torch.zeros(2, 3, 5, 128, dtype=hf), torch.zeros(2, 5, 3)
    with pytest.raises(ValueError, match="outs must be a list or tuple"):
        call(o, [l, l])
    with pytest.raises(ValueError, match="lses must be a list or tuple"):
        call([o, o], l)
    with pytest.raises(ValueError, match="outs must be a list or tuple"):
        call([o, None], [l, l])
    for n in (0, 1, 9):
        with pytest.raises(ValueError, match="outs must hold 2 .. 8 parts"):
            call([o] * n, [l] * n)
    with pytest.raises(ValueError, match="lses must hold as many"):
        call([o, o], [l, l, l])
    with pytest.raises(ValueError, match=r"outs\[0\] must be \(batch"):
        call([o[0, 0], o[0, 0]], [l, l])
    with pytest.raises(ValueError, match=r"outs\[0\] must be fp16 or bf16"):
        call([o.float(), o.float()], [l, l])
    with pytest.raises(ValueError, match=r"outs\[0\]: d_v must be one of"):
        call([o[..., :96], o[..., :96]], [l, l])
    with pytest.raises(ValueError, match=r"outs\[1\] must have the shape"):
        call([o, o[:, :2]], [l, l])
    with pytest.raises(ValueError, match=r"outs\[2\] must have the dtype"):
        call([o, o, o.to(bf)], [l, l, l])
    with pytest.raises(ValueError, match=r"lses\[1\] must be float32"):
        call([o, o], [l, l.double()])
    with pytest.raises(ValueError, match=r"lses\[0\] must have shape \(2, 5, 3\)"):
        call([o, o], [l.transpose(1, 2), l])
    with pytest.raises(ValueError, match=r"lses\[1\] must have shape \(5, 6\)"):
        call([o.flatten(0, 1), o.flatten(0, 1)], [torch.zeros(5, 6), torch.zeros(6, 5)])
    # views: used in place or refused, never copied
    with pytest.raises(ValueError, match=r"outs\[1\]: the last dimension must be contiguous"):
        call([o, torch.zeros(2, 3, 128, 5, dtype=hf).transpose(2, 3)], [l, l])
    with pytest.raises(ValueError, match=r"outs\[0\]: strides"):
        call([torch.zeros(2, 3, 5, 132, dtype=hf)[..., :128], o], [l, l])
    with pytest.raises(ValueError, match=r"outs\[1\]: strides .* storage offset 4"):
        call([o, torch.zeros(2, 3, 5, 136, dtype=hf)[..., 4:132]], [l, l])
    g = o.clone().requires_grad_(True)
    with pytest.raises(ValueError, match=r"outs\[1\] requires grad"):
        call([o, g], [l, l])
    # a CPU call that passes the checks is refused by the extension (no quiet fall-back)
    with pytest.raises(RuntimeError, match="GPU"):
        call([o, o], [l, l])
    with pytest.raises(RuntimeError, match="GPU"):
        call((o.to(bf), torch.zeros(2, 3, 5, 136, dtype=bf)[..., 8:136]), (l, torch.zeros(1, 5, 6).as_strided((2, 5, 3), (3, 6, 1))))      # aligned view, strided LSE
    with pytest.raises(RuntimeError, match="GPU"):
        call([o.flatten(0, 1)] * 8, [torch.zeros(5, 6)] * 8)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        call([o, g], [l, l])


def test_shared_prefix_refusals_before_any_device_work():
    import flash_attn_turing as F

    call = F.flash_attn_with_shared_prefix
    hf = torch.float16
    q = torch.zeros(3, 2, 8, 64, dtype=hf)
    pool, table = torch.zeros(20, 16, 2, 64, dtype=hf), torch.zeros(3, 6, dtype=torch.int32)
    kc = torch.zeros(3, 96, 2, 64, dtype=hf)
    lens = torch.full((3,), 40, dtype=torch.int32)
    for bad in (-1, 1.0, True, None, "32", torch.tensor(32)):
        with pytest.raises(ValueError, match="shared_prefix_len must be a Python int >= 0"):
            call(q, pool, pool, bad, cache_seqlens=lens, block_table=table)
    with pytest.raises(ValueError, match=r"multiple of page_block_size \(16\)"):
        call(q, pool, pool, 24, cache_seqlens=lens, block_table=table)
    with pytest.raises(ValueError, match="multiple of 16"):
        call(q, kc, kc, 40, cache_seqlens=lens)
    with pytest.raises(ValueError, match="below the cache capacity"):
        call(q, pool, pool, 96, cache_seqlens=lens, block_table=table)
    with pytest.raises(ValueError, match="below the cache capacity"):
        call(q, kc, kc, 96, cache_seqlens=lens)
    with pytest.raises(ValueError, match=r"cache_seqlens \(31\) must be at least shared_prefix_len"):
        call(q, kc, kc, 32, cache_seqlens=31)
    with pytest.raises(ValueError, match="q: the batch stride"):
        call(torch.zeros(3, 4, 8, 64, dtype=hf)[:, :2], kc, kc, 32, cache_seqlens=lens)
    with pytest.raises(ValueError, match="q must be a rank-4 tensor"):
        call(q[0], kc, kc, 32, cache_seqlens=lens)
    with pytest.raises(ValueError, match="k and v must both be given"):
        call(q, kc, kc, 32, k=torch.zeros(3, 2, 2, 64, dtype=hf), cache_seqlens=lens)
    with pytest.raises(ValueError, match="causal must be a bool"):
        call(q, kc, kc, 32, cache_seqlens=lens, causal=1)
    with pytest.raises(TypeError):
        call(q, kc, kc, 32, None, None, lens, table)
    for kw in ("window_size", "num_splits", "softcap", "sinks", "tree_mask", "cu_seqlens_q", "rotary_cos"):
        with pytest.raises(TypeError):
            call(q, kc, kc, 32, cache_seqlens=lens, **{kw: None})
    # calls that pass the checks end in the extension, which refuses CPU tensors: paged and contiguous, Ls = 0 (the plain call) and causal with nothing left
    for args, kw in (((q, pool, pool, 32), dict(cache_seqlens=lens, block_table=table)), ((q, kc, kc, 32), dict(cache_seqlens=lens, causal=True)),
                     ((q, kc, kc, 0), dict(cache_seqlens=lens)), ((q, kc, kc, 16), dict(cache_seqlens=40, causal=True)),
                     ((q[:, :1], kc, kc, 48), dict(softmax_scale=0.2, return_softmax_lse=True))):
        with pytest.raises(RuntimeError, match="GPU"):
            call(*args, **kw)


def test_chunked_prefill_refusals_before_any_device_work():
    import flash_attn_turing as F

    call = F.flash_mla_chunked_prefill_func
    bf = torch.bfloat16
    b, sq, sc, h, hk = 2, 5, 9, 4, 2
    q, kn, vn = torch.zeros(b, sq, h, 192, dtype=bf), torch.zeros(b, sq, hk, 192, dtype=bf), torch.zeros(b, sq, hk, 128, dtype=bf)
    kc, vc = torch.zeros(b, sc, hk, 192, dtype=bf), torch.zeros(b, sc, hk, 128, dtype=bf)
    with pytest.raises(TypeError):
        call(q, kc, vc, kn, vn, None)
    with pytest.raises(ValueError, match="k_ctx must be a tensor"):
        call(q, None, vc, kn, vn)
    with pytest.raises(ValueError, match="k_ctx must be 192 wide"):
        call(q, kc[..., :128], vc, kn, vn)
    with pytest.raises(ValueError, match="v_new must be 128 wide"):
        call(q, kc, vc, kn, kn)
    with pytest.raises(ValueError, match="q must be 192 wide"):
        call(q[..., :128], kc, vc, kn, vn)
    with pytest.raises(ValueError, match="k_new / v_new must have one row per query row"):
        call(q, kc, vc, kn[:, :4], vn[:, :4])
    with pytest.raises(ValueError, match="k_ctx must have q's dtype"):
        call(q, kc.half(), vc, kn, vn)
    with pytest.raises(ValueError, match="k_new: strides"):
        call(q, kc, vc, torch.zeros(b, sq, hk, 196, dtype=bf)[..., :192], vn)
    with pytest.raises(ValueError, match="come both or neither, got only cu_seqlens_q"):
        call(q.flatten(0, 1), kc.flatten(0, 1), vc.flatten(0, 1), kn.flatten(0, 1), vn.flatten(0, 1), cu_seqlens_q=torch.tensor([0, 5, 10], dtype=torch.int32))
    with pytest.raises(ValueError, match="v_ctx must be a rank-3 tensor"):
        call(q.flatten(0, 1), kc.flatten(0, 1), vc, kn.flatten(0, 1), vn.flatten(0, 1), cu_seqlens_q=torch.tensor([0, 5, 10], dtype=torch.int32),
             cu_seqlens_k_ctx=torch.tensor([0, 9, 18], dtype=torch.int32))
    with pytest.raises(ValueError, match="cu_seqlens_k_ctx must be an int32 tensor"):
        call(q.flatten(0, 1), kc.flatten(0, 1), vc.flatten(0, 1), kn.flatten(0, 1), vn.flatten(0, 1), cu_seqlens_q=torch.tensor([0, 5, 10], dtype=torch.int32),
             cu_seqlens_k_ctx=torch.tensor([0, 9, 18]))
    for bad in (0, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="softmax_scale"):
            call(q, kc, vc, kn, vn, softmax_scale=bad)
    # forward only, in the words of flash_mla_prefill_func
    for i, name in enumerate(("q", "k_ctx", "v_ctx", "k_new", "v_new")):
        t = [q, kc, vc, kn, vn]
        t[i] = t[i].clone().requires_grad_(True)
        with pytest.raises(ValueError, match=f"{name} requires grad: flash_mla_chunked_prefill_func is forward-only .the differentiable function is flash_mla_attn_func."):
            call(*t)
    for kw in (dict(), dict(softmax_scale=0.1, return_softmax_lse=True)):
        with pytest.raises(RuntimeError, match="GPU"):
            call(q, kc, vc, kn, vn, **kw)
    with pytest.raises(RuntimeError, match="GPU"):
        call(q, kc[:, :0], vc[:, :0], kn, vn)                                      # no context at all
    with pytest.raises(RuntimeError, match="GPU"):
        call(q.flatten(0, 1), kc.flatten(0, 1), vc.flatten(0, 1), kn.flatten(0, 1), vn.flatten(0, 1), cu_seqlens_q=torch.tensor([0, 5, 10], dtype=torch.int32),
             cu_seqlens_k_ctx=torch.tensor([0, 0, 18], dtype=torch.int32))


# ---- 3. the C ABI ---------------------------------------------------------------------------------------------------------------------------

FIELDS = ["struct_size", "magic", "dtype", "n_parts", "b", "rows", "h", "d_v", "o", "o_stride", "lse", "lse_stride", "out", "out_stride", "lse_out", "lse_out_stride", "stream"]


def test_params_layout_matches_header(tmp_path):
    from flash_attn_turing import capi

    assert [f[0] for f in capi.MergeParams._fields_] == FIELDS
    src = tmp_path / "merge_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MERGE_STATES\n#error "no FA_HAS_MERGE_STATES"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu 0\\n", sizeof(fa_merge_params));\n'
                   '    printf("abi %d %d %d\\n", FA_ABI_VERSION, FA_HAS_MERGE_STATES, FA_MERGE_MAX_PARTS);\n'
                   '    printf("lse_strides %zu %zu %zu %zu\\n", sizeof(fa_lse_strides), offsetof(fa_lse_strides, batch), offsetof(fa_lse_strides, head), offsetof(fa_lse_strides, row));\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_merge_params, {f}), sizeof(((fa_merge_params*)0)->{f}));\n' for f in FIELDS)
                   + "    fa_merge_params p;\n    FA_PARAMS_INIT(p);\n"
                     "    return p.struct_size == sizeof(p) && p.magic == FA_PARAMS_MAGIC && p.o[7] == NULL && p.lse_stride[7].row == 0 && p.stream == NULL ? 0 : 1;\n}\n")
    exe = tmp_path / "merge_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"][0] == ctypes.sizeof(capi.MergeParams) == 32 + 8 * (8 + 24 + 8 + 24) + 8 + 24 + 8 + 24 + 8
    assert got["abi"] == [4, 1, 8] and capi.lib().fa_abi_version() == 4 and capi.FA_MERGE_MAX_PARTS == 8
    assert got["lse_strides"] == [24, 0, 8, 16] and ctypes.sizeof(capi.LseStrides) == 24
    assert [capi.LseStrides.batch.offset, capi.LseStrides.head.offset, capi.LseStrides.row.offset] == [0, 8, 16]
    for f in FIELDS:
        assert got[f] == [getattr(capi.MergeParams, f).offset, getattr(capi.MergeParams, f).size], f
    assert "fa_run_merge_states" in capi.declared_functions() and hasattr(capi.lib(), "fa_run_merge_states")


def test_no_existing_struct_changed_size():
    """the sizes the other *_cpu.py suites pin, in one place: the merge came as a struct and an entry point of its own"""
    from flash_attn_turing import capi

    assert ctypes.sizeof(capi.MlaPrefillParams) == 216 and ctypes.sizeof(capi.Strides) == 24
    with open(capi.HEADER_PATH) as f:
        assert re.search(r"#define FA_ABI_VERSION 4\b", f.read())


def test_plain_c_caller_every_refusal_names_its_field(tmp_path):
    """codes with the field in fa_last_error; b * rows * h = 0 is FA_OK without a launch (no device is touched: every call here ends in the host checks)"""
    from flash_attn_turing import capi

    src = tmp_path / "use_merge.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
#ifndef FA_HAS_MERGE_STATES
#error "no FA_HAS_MERGE_STATES"
#endif
static _Alignas(16) char mem[256];
static void fill(fa_merge_params* p) {
    FA_PARAMS_INIT(*p);
    p->dtype = FA_BF16; p->n_parts = 3; p->b = 2; p->rows = 7; p->h = 5; p->d_v = 128;
    for (int i = 0; i < 3; ++i) {
        p->o[i] = mem; p->lse[i] = (const float*)mem;
        p->o_stride[i] = (fa_strides){7 * 5 * 128, 5 * 128, 128};
        p->lse_stride[i] = (fa_lse_strides){5 * 7, 7, 1};
    }
    p->out = mem; p->lse_out = (float*)mem;
    p->out_stride = (fa_strides){7 * 5 * 128, 5 * 128, 128};
    p->lse_out_stride = (fa_lse_strides){5 * 7, 7, 1};
}
#define CODE(field_change, code, word, ret) do { fa_merge_params t; fill(&t); field_change; \
    if (fa_run_merge_states(&t) != (code) || !strstr(fa_last_error(), word)) { fprintf(stderr, "%d: %s\n", ret, fa_last_error()); return ret; } } while (0)
int main(void) {
    fa_merge_params p;
    CODE(t.n_parts = 1, FA_ERR_BAD_SHAPE, "n_parts", 20);
    CODE(t.n_parts = 9, FA_ERR_BAD_SHAPE, "n_parts", 21);
    CODE(t.n_parts = 0, FA_ERR_BAD_SHAPE, "n_parts", 22);
    CODE(t.d_v = 192, FA_ERR_BAD_HEADDIM, "d_v", 23);
    CODE(t.d_v = 32, FA_ERR_BAD_HEADDIM, "d_v", 24);
    CODE(t.dtype = 2, FA_ERR_BAD_DTYPE, "dtype", 25);
    CODE(t.b = -1, FA_ERR_BAD_SHAPE, "b=", 26);
    CODE(t.rows = -1, FA_ERR_BAD_SHAPE, "rows=", 27);
    CODE(t.h = -1, FA_ERR_BAD_SHAPE, "h=", 28);
    CODE((t.b = 1 << 20, t.rows = 1 << 20), FA_ERR_BAD_SHAPE, "call too large", 29);
    CODE(t.o[0] = NULL, FA_ERR_NULL_POINTER, "o[0] is NULL", 30);
    CODE(t.o[2] = NULL, FA_ERR_NULL_POINTER, "o[2] is NULL", 31);
    CODE(t.lse[1] = NULL, FA_ERR_NULL_POINTER, "lse[1] is NULL", 32);
    CODE(t.out = NULL, FA_ERR_NULL_POINTER, "out is NULL", 33);
    CODE(t.lse_out = NULL, FA_ERR_NULL_POINTER, "lse_out is NULL", 34);
    CODE(t.o[1] = mem + 8, FA_ERR_BAD_STRIDE, "o[1] base pointer", 35);
    CODE(t.out = mem + 2, FA_ERR_BAD_STRIDE, "out base pointer", 36);
    CODE(t.lse[2] = (const float*)(mem + 2), FA_ERR_BAD_STRIDE, "lse[2] must be 4-byte aligned", 37);
    CODE(t.lse_out = (float*)(mem + 1), FA_ERR_BAD_STRIDE, "lse_out must be 4-byte aligned", 38);
    CODE(t.o_stride[0].head = 132, FA_ERR_BAD_STRIDE, "o[0] strides", 39);
    CODE(t.o_stride[2].row = 5 * 128 + 4, FA_ERR_BAD_STRIDE, "o[2] strides", 40);
    CODE(t.o_stride[1].batch = 12, FA_ERR_BAD_STRIDE, "o[1] strides", 41);
    CODE(t.out_stride.row = 4, FA_ERR_BAD_STRIDE, "out strides", 42);
    CODE(t.struct_size -= 8, FA_ERR_BAD_ABI, "struct_size", 43);
    CODE(t.magic = 0, FA_ERR_BAD_ABI, "magic", 44);
    if (fa_run_merge_states(NULL) != FA_ERR_NULL_POINTER) return 45;
    /* parts at or past n_parts are not looked at */
    /* nothing to do: FA_OK without a launch, whatever the pointers hold */
    fill(&p); p.b = 0; p.o[0] = NULL; p.out = NULL; p.lse_out = NULL;
    if (fa_run_merge_states(&p) != FA_OK) return 60;
    fill(&p); p.rows = 0; p.lse[1] = NULL;
    if (fa_run_merge_states(&p) != FA_OK) return 61;
    fill(&p); p.h = 0; p.o_stride[0].row = 3;
    if (fa_run_merge_states(&p) != FA_OK) return 62;
    if (fa_abi_version() != 4) return 63;
    return 0;
}
""")
    exe = tmp_path / "use_merge"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_ctypes_params_of_dense_and_packed_tensors():
    from flash_attn_turing import capi

    o = [torch.zeros(2, 3, 5, 64, dtype=torch.float16), torch.zeros(2, 3, 5, 72, dtype=torch.float16)[..., 8:]]
    l = [torch.zeros(2, 5, 3), torch.zeros(1, 5, 6).as_strided((2, 5, 3), (3, 6, 1))]
    out, lse = torch.zeros(2, 3, 5, 64, dtype=torch.float16), torch.zeros(2, 5, 3)
    p = capi.merge_params(o, l, out, lse)
    assert (p.n_parts, p.dtype, p.b, p.rows, p.h, p.d_v) == (2, capi.FA_FP16, 2, 3, 5, 64) and not p.stream
    assert (p.o_stride[1].batch, p.o_stride[1].row, p.o_stride[1].head) == (3 * 5 * 72, 5 * 72, 72) and p.o[1] == o[1].data_ptr()
    assert (p.lse_stride[1].batch, p.lse_stride[1].head, p.lse_stride[1].row) == (3, 6, 1)
    assert (p.lse_out_stride.batch, p.lse_out_stride.head, p.lse_out_stride.row) == (15, 3, 1) and not p.o[2]
    p = capi.merge_params([t.flatten(0, 1) for t in o[:1]] * 3, [torch.zeros(5, 6)] * 3, out.flatten(0, 1), torch.zeros(5, 6), stream=0)
    assert (p.n_parts, p.b, p.rows, p.h) == (3, 1, 6, 5) and (p.lse_stride[2].batch, p.lse_stride[2].head, p.lse_stride[2].row) == (0, 6, 1)
    assert (p.out_stride.batch, p.out_stride.row, p.out_stride.head) == (0, 5 * 64, 64)


# ---- 4. ISA -----------------------------------------------------------------------------------------------------------------------------------

def test_merge_kernels_isa():
    """16 kernels ({fp16, bf16} x d_v {64, 128, 256, 512} x {two parts, up to eight}) and nothing else.  Every one: no scratch, no LDS, no MFMA, subnormals
    kept, M0 untouched, at least seven waves a SIMD by registers (a streaming kernel lives off loads in flight; the two-part kernels fit eight); one 16-byte global load per part - 2 or 8 -
    with the lse loads as many, one 16-byte global store, and not one narrower access to the parts."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    name = "fa_merge_states.hip"
    assert name in B.HIP_SOURCES and B.HIP_SOURCES.index(name) < B.HIP_SOURCES.index("fa_capi.hip") and "fa_merge_states.hpp" in B.HIP_HEADERS
    assert name not in B.STAGE_SOURCES and name not in B.M0_GUARD_SOURCES and name not in B.EXTRA_FLAGS      # no LDS shared between waves, no LDS-DMA, the plain flags
    assert not any(name in v for v in B.DEBUG_VARIANTS.values())
    ks = analyse(name)
    assert len(ks) == 16, sorted(ks)
    asm = subprocess.run(B.debug_compile_command(name, [], "-", assembly=True), capture_output=True, text=True, check=True).stdout
    keys = set()
    for n, k in ks.items():
        m = re.search(r"fa_merge_states_kernelI(DF16_|DF16b)Li(\d+)ELb(\d)E", n)
        assert m, n
        keys.add(m.groups())
        parts = 2 if m.group(3) == "1" else 8
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["agprs"] == 0 and k["mfma_total"] == 0, (n, k)
        assert k["vgprs"] <= (40 if parts == 2 else 72) and k["occupancy"] >= 7, (n, k["vgprs"], k["occupancy"])
        assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
        assert k["m0_outside_asm"] == 0, n
        body = asm[asm.index(n + ":"):]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
        assert len(re.findall(r"global_load_dwordx4", body)) == parts, (n, len(re.findall(r"global_load_dwordx4", body)))
        assert len(re.findall(r"global_load_dword\s", body)) == parts, n
        assert len(re.findall(r"global_store_dwordx4", body)) == 1 and len(re.findall(r"global_store_dword\s", body)) == 1, n
        assert not re.findall(r"global_(?:load|store)_(?:u?short|u?byte|dwordx2|dwordx3)|flat_(?:load|store)|buffer_(?:load|store)|scratch_|ds_", body), n
        assert not re.findall(r"global_atomic|buffer_atomic|flat_atomic", body), n
    assert keys == {(t, str(d), two) for t in ("DF16_", "DF16b") for d in (64, 128, 256, 512) for two in "01"}
