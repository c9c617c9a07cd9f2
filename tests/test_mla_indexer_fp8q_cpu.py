"""CPU: FP8 (e4m3) q_idx through the four logits-taking indexer calls, without a GPU: signatures, the refusals in Python and through the C ABI
(fa_mla_indexer_params_v2), the struct's layout, the models the GPU test compares with, quantize_mla_index_queries, and the compiled kernels' resources."""
import ctypes
import inspect
import os
import re
import subprocess
import zlib

import pytest
import torch

import _mla_indexer_cases as C
import _mla_indexer_fp8q_cases as Q
import flash_attn_turing as F
from flash_attn_turing import capi
from test_mla_indexer_cpu import IDX_FIELDS, _code, _sig

E4M3 = torch.float8_e4m3fn
LOGITS_CALLS = ("flash_mla_indexer_logits", "flash_mla_index_with_kvcache", "flash_mla_indexer_prefill_logits", "flash_mla_index_prefill_with_kvcache")


def _gen(*seed):
    return torch.Generator().manual_seed(zlib.crc32(repr(seed).encode()))


# ---- 1. signatures -------------------------------------------------------------------------------------------------------------------------------------

def test_signatures_are_unchanged_and_the_helper_is_public():
    for n in ("flash_mla_indexer_logits", "flash_mla_indexer_prefill_logits"):
        assert _sig(getattr(F, n)) == (["q_idx", "weights", "k_idx_cache", "cache_seqlens"], {"k_scale": None, "block_table": None, "causal": True})
    for n in ("flash_mla_index_with_kvcache", "flash_mla_index_prefill_with_kvcache"):
        assert _sig(getattr(F, n)) == (["q_idx", "weights", "k_idx_cache", "cache_seqlens", "topk"], {"k_scale": None, "block_table": None, "causal": True, "return_logits": False})
    assert _sig(F.flash_mla_indexer_topk) == (["logits", "cache_seqlens", "topk"], {"causal": True})
    assert "quantize_mla_index_queries" in F.__all__ and F.quantize_mla_index_queries is F.interface.quantize_mla_index_queries
    ps = inspect.signature(F.quantize_mla_index_queries).parameters
    assert list(ps) == ["q_idx", "weights", "scale_format"] and ps["scale_format"].default == "fp32"
    for n in LOGITS_CALLS:
        assert "FP8 q_idx," not in getattr(F, n).__doc__        # no longer listed under "Out of scope"
    names = capi.declared_functions()
    for n in ("fa_run_mla_indexer_logits_v2", "fa_run_mla_indexer_prefill_logits_v2", "fa_mla_indexer_prefill_launch_v2"):
        assert n in names and hasattr(capi.lib(), n)
    assert "quantize_mla_index_keys" in F.quantize_mla_index_queries.__doc__


# ---- 2. refusals through Python --------------------------------------------------------------------------------------------------------------------------

def _args8(b=2, sq=2, h=64, cap=64, qdt=E4M3, kdt=E4M3):
    return dict(q_idx=torch.zeros(b, sq, h, 128).to(qdt), weights=torch.zeros(b, sq, h), k_idx_cache=torch.zeros(b, cap, 128).to(kdt), cache_seqlens=torch.zeros(b, dtype=torch.int32))


def _call(name, a, **kw):
    topk = (32,) if "index_" in name and "with_kvcache" in name else ()
    return getattr(F, name)(a["q_idx"], a["weights"], a["k_idx_cache"], a["cache_seqlens"], *topk, **kw)


def _refused(word, **change):
    said = set()
    for n in LOGITS_CALLS:
        a = _args8()
        a.update(change)
        with pytest.raises(ValueError, match=word) as e:
            _call(n, a)
        said.add(str(e.value))
    assert len(said) == 1, said                 # the four calls share one set of checks
    return said.pop()


def test_python_refusals_name_the_argument():
    z = torch.zeros
    for kdt in (torch.bfloat16, torch.float16):
        msg = _refused("k_idx_cache", k_idx_cache=z(2, 64, 128, dtype=kdt))                 # FP8 q_idx over a 16-bit cache
        assert "e4m3" in msg
    _refused("k_idx_cache", q_idx=z(2, 2, 64, 128, dtype=torch.uint8), k_idx_cache=z(2, 64, 128, dtype=torch.bfloat16))
    _refused("q_idx", q_idx=z(2, 2, 64, 128).to(torch.float8_e5m2))
    _refused("q_idx", q_idx=z(2, 2, 64, 128))                                               # fp32, as before
    _refused("q_idx", q_idx=z(2, 2, 64, 64).to(E4M3))                                       # width
    _refused("q_idx", q_idx=z(2, 2, 48, 128).to(E4M3))                                      # head count
    _refused("q_idx", q_idx=z(2, 64, 128).to(E4M3))                                         # rank
    _refused("q_idx", q_idx=z(2, 0, 64, 128).to(E4M3), weights=z(2, 0, 64))
    _refused("weights", weights=z(2, 2, 32))
    _refused("k_idx_cache", k_idx_cache=z(2, 64, 136, dtype=torch.uint8)[:, :, :128])       # the cache's view rules stay
    # an FP8 q_idx sliced out of a wider buffer, e4m3 or uint8, passes the checks and stops at the host module, which wants a GPU
    for qdt in (E4M3, torch.uint8):
        a = _args8()
        a["q_idx"] = z(2, 2, 66, 160).to(qdt)[:, :, 1:65, 16:144]
        assert not a["q_idx"].is_contiguous()
        for n in LOGITS_CALLS:
            with pytest.raises(RuntimeError, match="GPU"):
                _call(n, a, k_scale=z(2, 64))


# ---- 3. the C ABI ----------------------------------------------------------------------------------------------------------------------------------------

V2_FIELDS = IDX_FIELDS + ["q_format", "reserved2_"]


def test_v2_struct_layout_and_the_feature_macro(tmp_path):
    assert [f[0] for f in capi.MlaIndexerParamsV2._fields_] == V2_FIELDS and [f[0] for f in capi.MlaIndexerParams._fields_] == IDX_FIELDS
    src = tmp_path / "indexer_v2_layout.c"
    body = "".join(f'    printf("v2.{f} %zu %zu\\n", offsetof(fa_mla_indexer_params_v2, {f}), sizeof(((fa_mla_indexer_params_v2*)0)->{f}));\n' for f in V2_FIELDS)
    body += "".join(f'    printf("v1.{f} %zu %zu\\n", offsetof(fa_mla_indexer_params, {f}), sizeof(((fa_mla_indexer_params*)0)->{f}));\n' for f in IDX_FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_INDEXER_FP8_Q\n#error "no FA_HAS_MLA_INDEXER_FP8_Q"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu\\n", sizeof(fa_mla_indexer_params_v2), sizeof(fa_mla_indexer_params));\n'
                   '    printf("abi %d %d %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_INDEXER_FP8_Q, FA_IDX_Q_16BIT, FA_IDX_Q_FP8_E4M3);\n' + body +
                   "    fa_mla_indexer_params_v2 p;\n    FA_PARAMS_INIT(p);\n"
                   "    return p.struct_size == sizeof(p) && p.magic == FA_PARAMS_MAGIC && p.q_format == FA_IDX_Q_16BIT && p.reserved2_ == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "indexer_v2_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"] == [ctypes.sizeof(capi.MlaIndexerParamsV2), ctypes.sizeof(capi.MlaIndexerParams)] == [224, 216]
    assert got["abi"] == [4, 1, 0, 1] and capi.lib().fa_abi_version() == 4 and (capi.FA_IDX_Q_16BIT, capi.FA_IDX_Q_FP8_E4M3) == (0, 1)
    end = 0
    for f in V2_FIELDS:
        assert got[f"v2.{f}"] == [getattr(capi.MlaIndexerParamsV2, f).offset, getattr(capi.MlaIndexerParamsV2, f).size], f
        assert got[f"v2.{f}"][0] == end, f"{f}: padding in front of it"
        end = sum(got[f"v2.{f}"])
        if f in IDX_FIELDS:                     # the first 216 bytes are fa_mla_indexer_params, field for field
            assert got[f"v2.{f}"] == got[f"v1.{f}"], f
    assert end == 224 and got["v2.q_format"] == [216, 4] and got["v2.reserved2_"] == [220, 4]
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"#define FA_HAS_MLA_INDEXER_FP8_Q 1\b", text) and re.search(r"#define FA_ABI_VERSION 4\b", text)


def _v2(q8=True, paged=False):
    """a valid v2 struct over host tensors (the library validates before it launches; no test here reaches the launch)"""
    keep = dict(q=torch.zeros(2, 2, 64, 128, dtype=torch.uint8 if q8 else torch.bfloat16), w=torch.zeros(2, 2, 64), k=torch.zeros(8 if paged else 2, 64, 128, dtype=torch.uint8),
                sc=torch.zeros(8 if paged else 2, 64), lg=torch.zeros(2, 2, 256 if paged else 64), cs=torch.zeros(2, dtype=torch.int32),
                bt=torch.zeros(2, 4, dtype=torch.int32) if paged else None)
    p = capi.mla_indexer_params_v2(keep["q"], keep["w"], keep["k"], keep["lg"], keep["cs"], k_scale=keep["sc"], block_table=keep["bt"], causal=True)
    return p, keep


def test_c_abi_refusals_name_the_field():
    L = capi.lib()
    out = [ctypes.c_int32(-7) for _ in range(3)]
    shape = lambda p, stream: L.fa_mla_indexer_prefill_launch_v2(p, *[ctypes.byref(x) for x in out])
    entries = (L.fa_run_mla_indexer_logits_v2, L.fa_run_mla_indexer_prefill_logits_v2, shape)
    old_shape = lambda p, stream: L.fa_mla_indexer_prefill_launch(p, *[ctypes.byref(x) for x in out])
    old_entries = (L.fa_run_mla_indexer_logits, L.fa_run_mla_indexer_prefill_logits, old_shape)

    def bad(code, word, q8=True, **change):
        words = []
        for fn in entries:
            p, keep = _v2(q8)
            for k, v in change.items():
                setattr(p, k, v)
            _code(p, fn, code, word)
            words.append(capi.last_error())
        assert words[0] == words[1] == words[2], words
        assert [x.value for x in out] == [-7, -7, -7]       # a refused query writes nothing

    p, keep = _v2()
    assert (p.struct_size, p.q_format, p.k_format, p.dtype) == (224, capi.FA_IDX_Q_FP8_E4M3, capi.FA_IDX_K_FP8_E4M3, capi.FA_BF16)
    assert (p.q_idx_stride.batch, p.q_idx_stride.row, p.q_idx_stride.head) == (2 * 64 * 128, 64 * 128, 128)        # bytes
    bad(capi.FA_ERR_BAD_DTYPE, "q_format", q_format=2)
    bad(capi.FA_ERR_BAD_DTYPE, "q_format", q_format=-1)
    bad(capi.FA_ERR_BAD_DTYPE, "q_format", q8=False, q_format=2)
    bad(capi.FA_ERR_BAD_SHAPE, "reserved2_", reserved2_=1)
    bad(capi.FA_ERR_BAD_SHAPE, "reserved2_", q8=False, reserved2_=1)
    bad(capi.FA_ERR_BAD_DTYPE, "k_format", k_format=capi.FA_MLA_KV_16BIT)                   # e4m3 queries over a 16-bit cache
    bad(capi.FA_ERR_BAD_DTYPE, "dtype", dtype=2)                                            # not used, still a valid value
    bad(capi.FA_ERR_BAD_STRIDE, "q_idx strides", q_idx_stride=capi.Strides(2 * 64 * 128, 64 * 128, 136))       # 8 bytes past a multiple of 16
    bad(capi.FA_ERR_BAD_STRIDE, "q_idx strides", q_idx_stride=capi.Strides(2 * 64 * 128, 64 * 128 + 8, 128))
    bad(capi.FA_ERR_BAD_STRIDE, "q_idx strides", q_idx_stride=capi.Strides(8, 64 * 128, 128))
    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=220)
    bad(capi.FA_ERR_BAD_ABI, "struct_size", struct_size=232)
    bad(capi.FA_ERR_BAD_SHAPE, "reserved_", reserved_=1)
    bad(capi.FA_ERR_BAD_HEADDIM, "h 48", h=48)
    p, keep = _v2()
    p.q_idx = keep["q"].data_ptr() + 8
    _code(p, entries[0], capi.FA_ERR_BAD_STRIDE, "q_idx")
    # a valid v2 struct of either q_format passes every check: the launch query answers, and answers what the 216-byte struct gets
    from test_mla_indexer_cpu import _idx_params
    p1, keep1 = _idx_params()
    want = capi.mla_indexer_prefill_launch(p1)
    for q8 in (True, False):
        p, keep = _v2(q8)
        assert capi.mla_indexer_prefill_launch(p) == want
    # the 216-byte struct behaves as before, through its own entry points and through the _v2 ones (told apart by struct_size): its words for a stride that is no
    # multiple of 8 mention elements, a stride of 136 elements is fine for it
    for fns in (old_entries, entries):
        for fn in fns:
            p1, keep1 = _idx_params()
            p1.q_idx_stride = capi.Strides(2 * 64 * 128, 64 * 128, 132)
            _code(p1, fn, capi.FA_ERR_BAD_STRIDE, "multiples of 8 elements")
            p1, keep1 = _idx_params()
            p1.q_idx_stride = capi.Strides(2 * 64 * 136, 64 * 136, 136)
            tq, wg, nc = (ctypes.c_int32(0) for _ in range(3))
            launch = L.fa_mla_indexer_prefill_launch_v2 if fns is entries else L.fa_mla_indexer_prefill_launch
            assert launch(ctypes.byref(p1), ctypes.byref(tq), ctypes.byref(wg), ctypes.byref(nc)) == capi.FA_OK and (tq.value, wg.value, nc.value) == want
    # the entry points without _v2 take the 216-byte struct alone: a 224-byte struct there is a struct_size they do not know, whatever its q_format
    for q8 in (True, False):
        for fn in old_entries:
            p, keep = _v2(q8)
            rc = fn(ctypes.cast(ctypes.pointer(p), ctypes.POINTER(capi.MlaIndexerParams)), None)
            assert rc == capi.FA_ERR_BAD_ABI and "struct_size 224" in capi.last_error(), (rc, capi.last_error())
    assert [x.value for x in out] == [-7, -7, -7]
    # b == 0: FA_OK without a launch, whatever the pointers
    p, keep = _v2()
    p.b, p.q_idx, p.weights, p.k_idx_cache, p.logits = 0, None, None, None, None
    assert entries[0](ctypes.byref(p), None) == capi.FA_OK and entries[1](ctypes.byref(p), None) == capi.FA_OK


# ---- 4. the models ---------------------------------------------------------------------------------------------------------------------------------------

def test_every_pair_of_finite_codes_has_an_exact_fp32_product():
    v = Q.code_values()
    fin = torch.isfinite(v)
    assert int(fin.sum()) == 254 and not fin[0x7F] and not fin[0xFF] and float(v[Q.ONE]) == 1.0 and float(v[0x7E]) == 448.0 and float(v[0x01]) == 2.0 ** -9
    f = v[fin]
    p32 = f.view(-1, 1) * f.view(1, -1)
    p64 = f.double().view(-1, 1) * f.double().view(1, -1)
    assert torch.equal(p32.double(), p64)
    nz = p64[p64 != 0].abs()
    print(f"e4m3 x e4m3: |product| in [2^{torch.log2(nz.min()).item():.0f}, {nz.max().item():.0f}]")
    assert float(nz.min()) == 2.0 ** -18 and float(nz.max()) == 200704.0


@pytest.mark.parametrize("h", [16, 64])
def test_the_fp32_formula_on_fp8_queries_meets_the_bound_and_the_bound_bites(h):
    gen = _gen("model", h)
    q8, w, k, sc = Q.normal_quantised(2, 9, h, gen)
    ref, mag = C.logits_model(q8.float(), w, k, sc)
    got = C.logits_fp32_formula(q8.float(), w, k, sc).double()
    worst = float(((got - ref).abs() / mag).max())
    print(f"fp32 formula on e4m3 q, h={h}: worst |err| / magnitude = {worst:.3e} ({worst / C.TOL:.4f} of TOL)")
    assert worst <= C.TOL
    for variant in ("no_relu", "drop_head"):
        wrong, _ = C.logits_model(q8.float(), w, k, sc, variant=variant)
        assert float(((wrong - ref).abs() / mag).max()) > C.TOL, variant
    # brute force at a few entries
    for (i, t, j) in ((0, 0, 0), (1, 8, 319), (0, 4, 100)):
        assert abs(C.logits_brute(q8.float(), w, k, sc, i, t, j) - float(ref[i, t, j])) <= 1e-12 * float(mag[i, t, j])
    # integer data: the fp32 formula is the fp64 model
    q8, w, k, sc = Q.exact_inputs(2, 9, h, gen)
    ref, _ = C.logits_model(q8.float(), w, k, sc)
    assert torch.equal(C.logits_fp32_formula(q8.float(), w, k, sc).double(), ref)
    for dt in (torch.bfloat16, torch.float16):      # the widened queries of relation 1 hold the same values
        assert torch.equal(q8.to(dt).float(), q8.float())


def test_the_one_hot_patterns_say_what_they_claim():
    q, w, k, want = Q.one_hot_columns()
    assert torch.equal(want, torch.eye(128)) and torch.equal(C.logits_model(q.float(), w, k, None)[0][0].float(), want)
    q, w, k, want = Q.one_hot_columns(qv=lambda t: 1 + t % 5, kv=lambda j: 2 + j % 3)
    assert len(set(want.diagonal().tolist())) > 8 and torch.equal(C.logits_model(q.float(), w, k, None)[0][0].float(), want)
    assert float(want[7, 7]) == (1 + 7 % 5) * (2 + 7 % 3)
    for h in (16, 32, 64):
        q, w, k, want = Q.one_hot_heads(h)
        assert torch.equal(C.logits_model(q.float(), w, k, None)[0][0].float(), want) and want[h - 1, 0] == h
    q, w, k, want, fin = Q.every_code()
    assert int(fin.sum()) == 254 * 254
    ref = C.logits_model(torch.nan_to_num(q.float()), w, torch.nan_to_num(k.float()).to(E4M3), None)[0][0].float()
    assert torch.equal(ref[fin], want[fin]) and bool((want[fin] >= 0).all())


# ---- 5. quantize_mla_index_queries --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["fp32", "ue8m0"])
def test_quantize_queries_is_the_key_rule_per_row(fmt):
    gen = _gen("quant", fmt)
    q = (torch.randn(2, 3, 16, 128, generator=gen) * 3).to(torch.bfloat16)
    q[0, 0, 0] = 0                              # an all-zero row: scale 2^-24 / 448
    q[1, 2, 5, 7] = float("nan")
    q[1, 1, 3, 9] = float("inf")
    w = torch.randn(2, 3, 16, generator=gen)
    codes, w2 = F.quantize_mla_index_queries(q, w, fmt)
    kc, ks = F.quantize_mla_index_keys(q.reshape(-1, 128), fmt)
    assert codes.dtype == torch.uint8 and codes.shape == q.shape and torch.equal(codes.reshape(-1, 128), kc)
    assert w2.dtype == torch.float32 and w2.shape == w.shape and torch.equal(w2, w * ks.view(2, 3, 16))
    assert int(codes[1, 2, 5, 7]) & 0x7F == 0x7F and int(codes[1, 1, 3, 9]) == 0x7E
    # what the calls take: dequantised, it is q to within half an e4m3 step of the row's amax
    deq = codes.view(E4M3).float() * ks.view(2, 3, 16, 1)
    okrow = torch.isfinite(q.float()).all(-1)
    assert float(((deq - q.float()).abs()[okrow]).max()) <= float(q.float().abs()[okrow].max()) * 2.0 ** -4
    for bad in (dict(q_idx=q.float()), dict(weights=w[:, :, :8]), dict(weights=w.double()), dict(scale_format="e8m0")):
        a = dict(q_idx=q, weights=w, scale_format=fmt)
        a.update(bad)
        with pytest.raises(ValueError):
            F.quantize_mla_index_queries(**a)


# ---- 6. the compiled kernels ---------------------------------------------------------------------------------------------------------------------------------

def test_fp8q_kernels_isa(capsys):
    """2 + 2 kernels (contiguous, paged): one 16x16x128 e4m3 MFMA per (token, 16 keys, 16 heads), no conversion from e4m3 anywhere, no scratch, no AGPRs;
    the decode kernels without LDS, the prefill kernels with two 4 KB stages; subnormals kept; at least two workgroups a compute unit"""
    from _kernel_isa import analyse
    import build as B
    from test_mla_indexer_prefill_cpu import _launch

    dec, pre = "fa_mla_indexer_fp8q.hip", "fa_mla_indexer_prefill_fp8q.hip"
    for name in (dec, pre):
        assert name in B.HIP_SOURCES and B.HIP_SOURCES.index(name) < B.HIP_SOURCES.index("fa_capi.hip")
    assert pre in B.STAGE_SOURCES and dec not in B.STAGE_SOURCES
    assert all(pre in B.DEBUG_VARIANTS[v] for v in ("stage_slow_reader", "stage_slow_writer", "stage_racy_slow_writer"))
    (tq, _, _), _ = _launch(1, 1, 64)
    nt = tq // 4                                # tokens of a wave
    from mfma_hazards import NEED
    assert NEED["16x16x128_f8f6f4"] == 12 == NEED["32x32x16"]
    with capsys.disabled():
        print()
        for name, lds, step_mfma, reads in ((dec, 0, 2 * (1 + 1 + 2), 0), (pre, 2 * 32 * 128, 2 * nt * (4 + 2 + 1), 2 * 2)):
            ks = analyse(name)
            assert len(ks) == 2, sorted(ks)
            assert {re.search(r"kernelILb(\d)E", n).group(1) for n in ks} == {"0", "1"}
            for n, k in sorted(ks.items()):
                paged = re.search(r"kernelILb(\d)E", n).group(1)
                print(f"  {name} paged={paged}: {k['vgprs']} VGPRs, {k['agprs']} AGPRs, {k['scratch_bytes']} B scratch, {k['lds_bytes']} B LDS, "
                      f"occupancy {k['occupancy']} waves a SIMD")
                assert k["scratch_bytes"] == 0 and k["agprs"] == 0 and k["lds_bytes"] == lds, (n, k)
                assert k["vgprs"] <= 256 and k["occupancy"] >= 2, (n, k["vgprs"], k["occupancy"])       # four waves a workgroup, one a SIMD: workgroups a compute unit = occupancy
                assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
                assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
                assert k["loops"], f"{n}: no MFMA loop found"
                for lp in k["loops"]:
                    assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"])
                main = max(k["loops"], key=lambda lp: lp["mfma"])
                hist = main["histogram"]
                # the loop holds two steps.  decode: 2 + 2 + 4 MFMAs a step behind the head-count branches = 8 for h = 64; prefill: a basic block per head
                # count, 2 x 4 x tokens-per-wave for h = 64 (+ the blocks of h = 32 and 16), and two fragment reads per 16-key block
                assert main["mfma"] == 2 * step_mfma and hist.get("v_mfma_f32_16x16x128_f8f6f4", 0) == main["mfma"] == k["mfma_total"], (n, main["mfma"], k["mfma_total"])
                assert main["ds_read_b128"] == 2 * reads and main["barriers"] == (2 if lds else 0), (n, main["ds_read_b128"], main["barriers"])
                assert not [op for op in hist if op.startswith("v_cvt")], (n, [op for op in hist if op.startswith("v_cvt")])
                assert hist.get("v_maximum3_f32", 0) > 0 and "v_max_f32" not in hist, n         # the ReLU that keeps a NaN
