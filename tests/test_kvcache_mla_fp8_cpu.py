"""CPU: the FP8 latent cache (656-byte rows) of the two MLA decode calls - the format's two helpers to the bit, the Python surface and its refusals,
the _v2 structs against the header, the error codes, workspace and split against format 0, and the resources of the kernels of
fa_fwd_kvcache_mla_fp8.hip.  No GPU involved."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import flash_attn_turing as F
from flash_attn_turing import capi

DTS = [torch.float16, torch.bfloat16]
F8 = torch.float8_e4m3fn


def decode_e4m3(code):
    """fp64 value of an OCP e4m3 code, from the bit fields (no torch conversion): NaN for 0x7f / 0xff"""
    s, e, m = code >> 7, (code >> 3) & 15, code & 7
    if e == 15 and m == 7:
        return float("nan")
    v = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


def bits16(t):
    return t.contiguous().view(torch.int16)


# ---- 1. the helpers ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", DTS)
def test_layout_scales_at_512_rope_copied(dt):
    gen = torch.Generator().manual_seed(1)
    kv = (torch.randn(3, 5, 1, 576, generator=gen) * 2).to(dt)
    assert "quantize_mla_kv_cache" in F.__all__ and "dequantize_mla_kv_cache" in F.__all__
    assert F.quantize_mla_kv_cache is F.interface.quantize_mla_kv_cache and F.dequantize_mla_kv_cache is F.interface.dequantize_mla_kv_cache
    q8 = F.quantize_mla_kv_cache(kv)
    assert q8.shape == (3, 5, 1, 656) and q8.dtype == torch.uint8
    # the scales: four little-endian fp32 at bytes 512 .. 527, max(amax, 2^-24) / 448 of the tile
    scale = torch.from_numpy(np.frombuffer(q8[..., 512:528].contiguous().numpy().tobytes(), dtype="<f4").copy()).view(3, 5, 1, 4)
    amax = kv[..., :512].float().abs().view(3, 5, 1, 4, 128).amax(-1)
    assert torch.equal(scale, (amax / 448.0).float()) and (amax > 2.0 ** -24).all()
    # the rope bytes are kv's, bit for bit
    assert torch.equal(q8[..., 528:].contiguous().view(torch.int16), bits16(kv[..., 512:]))
    # codes: e4m3_rne(x / scale), the amax element at +-448 (0x7e / 0xfe)
    want = (kv[..., :512].float().view(3, 5, 1, 4, 128) / scale.unsqueeze(-1)).to(F8).view(torch.uint8).view(3, 5, 1, 512)
    assert torch.equal(q8[..., :512], want)
    assert ((q8[..., :512] & 0x7F) == 0x7E).view(3, 5, 1, 4, 128).any(-1).all()
    # and back: the row formula; the rope part returns exactly, the rest within the format's step
    back = F.dequantize_mla_kv_cache(q8, dt)
    assert back.shape == kv.shape and back.dtype == dt
    assert torch.equal(bits16(back[..., 512:]), bits16(kv[..., 512:]))
    assert torch.equal(bits16(back[..., :512]), bits16((want.view(F8).float().view(3, 5, 1, 4, 128) * scale.unsqueeze(-1)).to(dt).view(3, 5, 1, 512)))
    err = (back[..., :512].float() - kv[..., :512].float()).abs().view(3, 5, 1, 4, 128)
    assert (err <= amax.unsqueeze(-1) * 2.0 ** -4 + 2.0 ** -9 * scale.unsqueeze(-1)).all()     # half a step of 3 mantissa bits at the top binade, plus the output rounding
    # float8_e4m3fn views of the same bytes are the same cache
    assert torch.equal(bits16(F.dequantize_mla_kv_cache(q8.view(F8), dt)), bits16(back))
    for bad in (kv.float(), kv[..., :512], None):
        with pytest.raises(ValueError, match="kv must be"):
            F.quantize_mla_kv_cache(bad)
    for bad in (q8[..., :576], q8.float(), None):
        with pytest.raises(ValueError, match="kv8 must be"):
            F.dequantize_mla_kv_cache(bad, dt)
    with pytest.raises(ValueError, match="dtype must be"):
        F.dequantize_mla_kv_cache(q8, torch.float32)


@pytest.mark.parametrize("dt", DTS)
def test_every_code_under_four_scales_is_the_product_rounded_once(dt):
    """all 256 codes x scales {2^-7, 0.3, 1.0, 3.7}: the expectation is computed here in fp64 from the code's bit fields and the fp32 scale - the exact
    product of an e4m3 value (4 significant bits) and an fp32 number fits fp64 - rounded once to fp32 (the contract's fp32 product) and once to dt"""
    scales = [2.0 ** -7, 0.3, 1.0, 3.7]
    row = torch.zeros(2, 656, dtype=torch.uint8)
    codes = torch.arange(256, dtype=torch.uint8)
    row[0, :256], row[0, 256:512] = codes, codes           # row 0: tiles 0 / 1 hold codes 0 .. 127 / 128 .. 255 under scales 0 / 1, tiles 2 / 3 under 2 / 3
    row[1, :256], row[1, 256:512] = codes, codes
    sc = np.array([[scales[0], scales[0], scales[1], scales[1]], [scales[2], scales[2], scales[3], scales[3]]], dtype="<f4")
    row[:, 512:528] = torch.from_numpy(np.frombuffer(sc.tobytes(), dtype=np.uint8).copy()).view(2, 16)
    got = F.dequantize_mla_kv_cache(row, dt)[:, :512]
    for r in range(2):
        for half in range(2):
            s32 = float(sc[r, 2 * half])
            for c in range(256):
                x = float(np.float32(decode_e4m3(c) * s32))             # fp64 product (exact), rounded once to fp32
                want = torch.tensor([x], dtype=torch.float32).to(dt)    # ... and once to dt (nearest-even)
                g = got[r, 256 * half + c]
                if np.isnan(x):
                    assert torch.isnan(g) and c & 0x7F == 0x7F, (r, half, c)
                else:
                    assert bits16(g.view(1)).item() == bits16(want).item(), (r, half, c, float(g), x)
    # fp16: a product beyond 65504 becomes inf by the rounding rule
    if dt == torch.float16:
        big = row[:1].clone()
        big[:, 512:528] = torch.from_numpy(np.frombuffer(np.array([1024.0] * 4, dtype="<f4").tobytes(), dtype=np.uint8).copy())
        out = F.dequantize_mla_kv_cache(big, dt)[0, :512]
        assert out[0x7E].item() == float("inf") and out[128 + 0x7E].item() == float("-inf") and out[0x60].item() == 32768.0      # 448 x 1024, 32 x 1024


@pytest.mark.parametrize("dt", DTS)
def test_quantiser_edges(dt):
    """all-zero tile, tile with NaN, tile with +-inf, tile whose amax is subnormal (in dt, and below the 2^-24 floor)"""
    tiny = 2.0 ** -24 if dt == torch.float16 else 2.0 ** -130
    kv = torch.zeros(6, 576, dtype=dt)
    kv[1, 3], kv[1, 4], kv[1, 5] = float("nan"), 2.0, -1.0
    kv[1, 6] = torch.tensor([-1], dtype=torch.int16).view(dt)[0]        # a negative NaN (all ones)
    kv[2, 130], kv[2, 131], kv[2, 132], kv[2, 133] = float("inf"), float("-inf"), 3.0, -0.75
    kv[3, 256], kv[3, 257] = tiny, -tiny / 2 if dt == torch.bfloat16 else 0.0
    kv[4, :512] = float("nan")
    kv[5, :512] = float("inf")
    q8 = F.quantize_mla_kv_cache(kv)
    sc = torch.from_numpy(np.frombuffer(q8[:, 512:528].contiguous().numpy().tobytes(), dtype="<f4").copy()).view(6, 4)
    floor = float(np.float32(2.0 ** -24) / np.float32(448.0))
    assert (sc[0] == floor).all() and (q8[0, :512] == 0).all()                                  # all zero: the floor scale, codes 0
    assert sc[1, 0].item() == float(np.float32(2.0) / np.float32(448.0))                        # NaN skipped by amax
    assert q8[1, 3].item() == 0x7F and q8[1, 6].item() == 0xFF and q8[1, 4].item() == 0x7E and q8[1, 5].item() == 0xF6   # NaN keeps its sign; 448; -224
    assert sc[2, 1].item() == float(np.float32(3.0) / np.float32(448.0))                        # +-inf skipped by amax ...
    assert q8[2, 130].item() == 0x7E and q8[2, 131].item() == 0xFE and q8[2, 132].item() == 0x7E and q8[2, 133].item() == 0xEE      # ... and saturated; -112
    want_tiny = max(float(torch.tensor(tiny, dtype=dt)), 2.0 ** -24)
    assert sc[3, 2].item() == float(np.float32(want_tiny) / np.float32(448.0))
    if dt == torch.float16:
        assert q8[3, 256].item() == 0x7E                                                        # the subnormal amax itself sits at 448
    else:
        assert q8[3, 256].item() == 0 and q8[3, 257].item() in (0x00, 0x80)                     # far below the floor's smallest code
    assert (sc[4] == floor).all() and ((q8[4, :512] & 0x7F) == 0x7F).all()                      # nothing finite: amax 0
    assert (sc[5] == floor).all() and (q8[5, :512] == 0x7E).all()
    assert torch.isnan(F.dequantize_mla_kv_cache(q8, dt)[1, 3]) and F.dequantize_mla_kv_cache(q8, dt)[1, 4].item() == 2.0


# ---- 2. the Python surface --------------------------------------------------------------------------------------------------------------------

def test_surface_accepts_the_format_and_keeps_every_refusal():
    dense, sparse = F.flash_mla_with_kvcache, F.flash_mla_sparse_with_kvcache
    assert list(inspect.signature(dense).parameters) == ["q", "kv_cache", "cache_seqlens", "head_dim_v", "kv_new", "block_table", "softmax_scale", "causal", "num_splits",
                                                         "return_softmax_lse"]
    assert list(inspect.signature(sparse).parameters) == ["q", "kv_cache", "cache_seqlens", "indices", "head_dim_v", "block_table", "softmax_scale", "num_splits",
                                                          "return_softmax_lse"]
    for fn in (dense, sparse):
        assert "656" in fn.__doc__ and "dequantize_mla_kv_cache" in fn.__doc__
    b, sq, h, cap = 2, 2, 16, 64
    q = torch.zeros(b, sq, h, 576, dtype=torch.bfloat16)
    idx = torch.zeros(b, sq, 32, dtype=torch.int32)
    table = torch.zeros(b, 4, dtype=torch.int32)
    calls = [lambda kv, **kw: dense(q, kv, 8, **kw), lambda kv, **kw: sparse(q, kv, 8, idx, **kw)]
    for call in calls:
        # accepted up to the device check: what is left to fail is the host module's "GPU tensors" (a RuntimeError, not a ValueError of the surface)
        for dt in (torch.uint8, F8):
            with pytest.raises(RuntimeError, match="GPU"):
                call(torch.zeros(b, cap, 1, 656, dtype=torch.uint8).view(dt))
            with pytest.raises(RuntimeError, match="GPU"):
                call(torch.zeros(9, 16, 1, 656, dtype=torch.uint8).view(dt), block_table=table)
            with pytest.raises(RuntimeError, match="GPU"):                     # a row stride of 672 bytes, an offset of 16
                call(torch.zeros(b, cap, 1, 672, dtype=torch.uint8).view(dt)[..., 16:])
        # misaligned views are refused by name, never copied
        wide = torch.zeros(b, cap, 1, 664, dtype=torch.uint8)
        with pytest.raises(ValueError, match="kv_cache: .*strides.*multiples of 16 bytes"):
            call(wide[..., :656])
        with pytest.raises(ValueError, match="kv_cache: .*strides.*multiples of 16 bytes"):
            call(torch.zeros(b, cap * 656 + 8, dtype=torch.uint8)[:, :cap * 656].view(b, cap, 1, 656))
        with pytest.raises(ValueError, match="kv_cache: .*start at a multiple of 16 bytes"):
            call(torch.zeros(b, cap, 1, 672, dtype=torch.uint8)[..., 8:664])
        with pytest.raises(ValueError, match="kv_cache: .*last dimension"):
            call(torch.zeros(b, cap, 1, 2 * 656, dtype=torch.uint8)[..., ::2])
        # the old refusals keep their words
        with pytest.raises(ValueError, match="kv_cache must have q's dtype"):
            call(torch.zeros(b, cap, 1, 576, dtype=torch.uint8).view(F8))
        with pytest.raises(ValueError, match="kv_cache must have q's dtype"):
            call(torch.zeros(b, cap, 1, 576, dtype=torch.uint8))
        with pytest.raises(ValueError, match="kv_cache must have q's dtype"):
            call(torch.zeros(b, cap, 1, 656, dtype=torch.float16))
        with pytest.raises(ValueError, match="kv_cache must have q's dtype"):
            call(torch.zeros(b, cap, 1, 656, dtype=torch.int8))
        with pytest.raises(ValueError, match="kv_cache must be 576 wide"):
            call(torch.zeros(b, cap, 1, 656, dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="kv_cache must be 576 wide"):
            call(torch.zeros(b, cap, 1, 512, dtype=torch.bfloat16))
        with pytest.raises(ValueError, match="exactly one head"):
            call(torch.zeros(b, cap, 2, 656, dtype=torch.uint8))
        with pytest.raises(ValueError, match="kv_cache batch"):
            call(torch.zeros(b + 1, cap, 1, 656, dtype=torch.uint8))
        with pytest.raises(ValueError, match="page_block_size"):
            call(torch.zeros(9, 24, 1, 656, dtype=torch.uint8), block_table=table)
        with pytest.raises(ValueError, match="kv_cache must be on q's device"):
            call(torch.zeros(b, cap, 1, 656, dtype=torch.uint8, device="meta"))
    # kv_new stays 16-bit and 576 wide
    kv8 = torch.zeros(b, cap, 1, 656, dtype=torch.uint8)
    with pytest.raises(ValueError, match="kv_new must have shape"):
        dense(q, kv8, 8, kv_new=torch.zeros(b, 1, 1, 656, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="kv_new must be a rank-4 tensor of q's dtype"):
        dense(q, kv8, 8, kv_new=torch.zeros(b, 1, 1, 656, dtype=torch.uint8))


# ---- 3. the C ABI -------------------------------------------------------------------------------------------------------------------------------

def test_v2_structs_match_the_header(tmp_path):
    assert ctypes.sizeof(capi.MlaParams) == 240 and ctypes.sizeof(capi.MlaParamsV2) == 248
    assert ctypes.sizeof(capi.MlaSparseParamsV2) == ctypes.sizeof(capi.MlaSparseParams) + 8
    assert capi.FA_MLA_KV_16BIT == 0 and capi.FA_MLA_KV_FP8_ROWS656 == 1
    lines = []
    for cname, cls in (("fa_mla_params_v2", capi.MlaParamsV2), ("fa_mla_sparse_params_v2", capi.MlaSparseParamsV2)):
        lines.append(f'    printf("{cname} size %zu 0\\n", sizeof({cname}));\n')
        lines += [f'    printf("{cname} {f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));\n' for f, *_ in cls._fields_]
    src = tmp_path / "mla_v2_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_MLA_FP8_KVCACHE\n#error "no FA_HAS_MLA_FP8_KVCACHE"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("macros %d %d %d %d\\n", FA_ABI_VERSION, FA_HAS_MLA_FP8_KVCACHE, FA_MLA_KV_16BIT, FA_MLA_KV_FP8_ROWS656);\n'
                   '    printf("old %zu %zu\\n", sizeof(fa_mla_params), sizeof(fa_mla_sparse_params));\n' + "".join(lines)
                   + "    fa_mla_params_v2 p;\n    FA_PARAMS_INIT(p);\n    fa_mla_sparse_params_v2 s;\n    FA_PARAMS_INIT(s);\n"
                     "    return p.struct_size == sizeof(p) && p.kv_format == 0 && p.reserved2_ == 0 && s.struct_size == sizeof(s) && s.kv_format == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "mla_v2_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        tok = line.split()
        if tok[0] == "macros":
            got["macros"] = [int(x) for x in tok[1:]]
        else:
            got[" ".join(tok[:-2])] = [int(tok[-2]), int(tok[-1])]
    assert got["macros"] == [4, 1, 0, 1] and capi.lib().fa_abi_version() == 4
    assert got["old"] == [240, ctypes.sizeof(capi.MlaSparseParams)]
    for cname, cls, old in (("fa_mla_params_v2", capi.MlaParamsV2, capi.MlaParams), ("fa_mla_sparse_params_v2", capi.MlaSparseParamsV2, capi.MlaSparseParams)):
        end = 0
        for f, *_ in cls._fields_:
            assert got[f"{cname} {f}"] == [getattr(cls, f).offset, getattr(cls, f).size], (cname, f)
            assert got[f"{cname} {f}"][0] == end, f"{cname}.{f}: padding in front of it"
            end = sum(got[f"{cname} {f}"])
            if hasattr(old, f):                 # the shared prefix: the same fields at the same offsets
                assert getattr(old, f).offset == getattr(cls, f).offset, (cname, f)
        assert end == got[f"{cname} size"][0] == ctypes.sizeof(cls)
        assert [f for f, *_ in cls._fields_][-2:] == ["kv_format", "reserved2_"] and getattr(cls, "kv_format").offset == ctypes.sizeof(old)


def test_plain_c_caller_both_sizes_and_the_new_codes(tmp_path):
    """both struct sizes through the same entry points, other sizes FA_ERR_BAD_ABI; kv_format / reserved2_ FA_ERR_BAD_SHAPE naming the field; the 16-byte
    rule of the FP8 cache FA_ERR_BAD_STRIDE; workspace and split of format 1 equal those of format 0"""
    src = tmp_path / "use_mla_fp8.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
#ifndef FA_HAS_MLA_FP8_KVCACHE
#error "no FA_HAS_MLA_FP8_KVCACHE"
#endif
static _Alignas(16) char mem[256];
static void fill(fa_mla_params_v2* p, int fmt) {
    FA_PARAMS_INIT(*p);
    p->q = p->kv_cache = p->o = mem; p->lse = (float*)mem; p->cache_seqlens = (const int32_t*)mem;
    p->b = 8; p->seqlen_q = 2; p->seqlen_cache = 32768; p->h = 128; p->d_qk = 576; p->d_v = 512; p->dtype = FA_BF16; p->num_splits = 4;
    p->q_stride = (fa_strides){2 * 128 * 576, 128 * 576, 576};
    p->o_stride = (fa_strides){2 * 128 * 512, 128 * 512, 512};
    p->kv_format = fmt;
    p->kv_cache_stride = fmt ? (fa_strides){32768LL * 656, 656, 656} : (fa_strides){32768LL * 576, 576, 576};
}
static void fills(fa_mla_sparse_params_v2* p, int fmt) {
    FA_PARAMS_INIT(*p);
    p->q = p->kv_cache = p->o = mem; p->lse = (float*)mem; p->cache_seqlens = (const int32_t*)mem; p->indices = (const int32_t*)mem;
    p->b = 8; p->seqlen_q = 2; p->seqlen_cache = 32768; p->topk = 2048; p->h = 128; p->d_qk = 576; p->d_v = 512; p->dtype = FA_BF16; p->num_splits = 4;
    p->q_stride = (fa_strides){2 * 128 * 576, 128 * 576, 576};
    p->o_stride = (fa_strides){2 * 128 * 512, 128 * 512, 512};
    p->indices_batch_stride = 2 * 2048; p->indices_row_stride = 2048;
    p->kv_format = fmt;
    p->kv_cache_stride = fmt ? (fa_strides){32768LL * 656, 656, 656} : (fa_strides){32768LL * 576, 576, 576};
}
#define D(p) ((const fa_mla_params*)(p))
#define S(p) ((const fa_mla_sparse_params*)(p))
#define CODE(change, code, word, ret) do { fa_mla_params_v2 t; fill(&t, 1); change; \
    if (fa_mla_workspace_bytes(D(&t)) != (code) || !strstr(fa_last_error(), word)) { fprintf(stderr, "dense %d: %s\n", ret, fa_last_error()); return ret; } \
    if (fa_run_mla_fwd_kvcache(D(&t), NULL) != (code) || fa_mla_num_splits(D(&t)) != (code)) return ret; } while (0)
#define SCODE(change, code, word, ret) do { fa_mla_sparse_params_v2 t; fills(&t, 1); change; \
    if (fa_mla_sparse_workspace_bytes(S(&t)) != (code) || !strstr(fa_last_error(), word)) { fprintf(stderr, "sparse %d: %s\n", ret, fa_last_error()); return ret; } \
    if (fa_run_mla_sparse_fwd_kvcache(S(&t), NULL) != (code) || fa_mla_sparse_num_splits(S(&t)) != (code)) return ret; } while (0)
int main(void) {
    if (sizeof(fa_mla_params) != 240 || sizeof(fa_mla_params_v2) != 248 || sizeof(fa_mla_sparse_params_v2) != sizeof(fa_mla_sparse_params) + 8) return 9;
    /* workspace and split: format 1 == format 0 == the first struct */
    for (int forced = 0; forced <= 4; forced += 2) {
        fa_mla_params_v2 a, b; fill(&a, 0); fill(&b, 1); a.num_splits = b.num_splits = forced;
        fa_mla_params o; memcpy(&o, &a, sizeof(o)); o.struct_size = sizeof(o);
        const long long w = fa_mla_workspace_bytes(&o);
        if (w < 0 || fa_mla_workspace_bytes(D(&a)) != w || fa_mla_workspace_bytes(D(&b)) != w) return 10;
        if (forced == 4 && w != 4 * (8LL * 128 * 2) * 512 * 4 + 4 * (8LL * 128 * 2) * 4) return 11;
        a.workspace = b.workspace = o.workspace = mem; a.workspace_bytes = b.workspace_bytes = o.workspace_bytes = 1LL << 40;
        const int n = fa_mla_num_splits(&o);
        if (n < 1 || fa_mla_num_splits(D(&a)) != n || fa_mla_num_splits(D(&b)) != n || (forced == 4 && n != 4)) return 12;
        fa_mla_sparse_params_v2 sa, sb; fills(&sa, 0); fills(&sb, 1); sa.num_splits = sb.num_splits = forced;
        fa_mla_sparse_params so; memcpy(&so, &sa, sizeof(so)); so.struct_size = sizeof(so);
        const long long sw = fa_mla_sparse_workspace_bytes(&so);
        if (sw < 0 || fa_mla_sparse_workspace_bytes(S(&sa)) != sw || fa_mla_sparse_workspace_bytes(S(&sb)) != sw) return 13;
        sa.workspace = sb.workspace = so.workspace = mem; sa.workspace_bytes = sb.workspace_bytes = so.workspace_bytes = 1LL << 40;
        const int sn = fa_mla_sparse_num_splits(&so);
        if (sn < 1 || fa_mla_sparse_num_splits(S(&sa)) != sn || fa_mla_sparse_num_splits(S(&sb)) != sn || (forced == 4 && sn != 4)) return 14;
    }
    /* sizes: exactly the two known ones */
    CODE(t.struct_size = 244, FA_ERR_BAD_ABI, "struct_size", 20);
    CODE(t.struct_size = 232, FA_ERR_BAD_ABI, "struct_size", 21);
    CODE(t.struct_size = 256, FA_ERR_BAD_ABI, "struct_size", 22);
    SCODE(t.struct_size -= 4, FA_ERR_BAD_ABI, "struct_size", 23);
    SCODE(t.struct_size -= 16, FA_ERR_BAD_ABI, "struct_size", 24);
    SCODE(t.struct_size += 8, FA_ERR_BAD_ABI, "struct_size", 25);
    /* the first struct's size through a _v2 in memory: kv_format is not read, the strides are then elements of a 16-bit cache (656 is a multiple of 8) */
    { fa_mla_params_v2 t; fill(&t, 1); t.struct_size = 240; if (fa_mla_workspace_bytes(D(&t)) < 0) return 26; }
    CODE(t.kv_format = 2, FA_ERR_BAD_SHAPE, "kv_format", 30);
    CODE(t.kv_format = -1, FA_ERR_BAD_SHAPE, "kv_format", 31);
    CODE(t.reserved2_ = 1, FA_ERR_BAD_SHAPE, "reserved2_", 32);
    CODE(t.reserved_ = 1, FA_ERR_BAD_ABI, "reserved_", 33);
    CODE(t.kv_cache_stride.row = 664, FA_ERR_BAD_STRIDE, "kv_cache", 34);
    CODE(t.kv_cache_stride.row = 640, FA_ERR_BAD_STRIDE, "kv_cache", 35);
    CODE(t.kv_cache_stride.batch += 8, FA_ERR_BAD_STRIDE, "kv_cache", 36);
    CODE(t.kv_cache = mem + 8, FA_ERR_BAD_STRIDE, "kv_cache", 37);
    CODE(t.kv_cache = NULL, FA_ERR_NULL_POINTER, "kv_cache", 38);
    CODE(t.kv_cache_stride.row = 1 << 17, FA_ERR_BAD_STRIDE, "kv_cache", 39);      /* one sequence spans 2^31 bytes or more */
    CODE((t.kv_new = mem, t.seqlen_new = 1, t.kv_new_stride = (fa_strides){568, 568, 568}), FA_ERR_BAD_STRIDE, "kv_new", 40);   /* kv_new stays 576 elements wide */
    CODE(t.d_qk = 656, FA_ERR_BAD_HEADDIM, "d_qk", 41);
    { fa_mla_params_v2 t; fill(&t, 1); t.kv_cache_stride.row = 672; t.kv_cache_stride.batch = 32768LL * 672; t.kv_new = mem; t.seqlen_new = 2;
      t.kv_new_stride = (fa_strides){2 * 576, 576, 576}; if (fa_mla_workspace_bytes(D(&t)) < 0) { fprintf(stderr, "%s\n", fa_last_error()); return 42; } }
    SCODE(t.kv_format = 2, FA_ERR_BAD_SHAPE, "kv_format", 50);
    SCODE(t.reserved2_ = -1, FA_ERR_BAD_SHAPE, "reserved2_", 51);
    SCODE(t.kv_cache_stride.row = 664, FA_ERR_BAD_STRIDE, "kv_cache", 52);
    SCODE(t.kv_cache_stride.batch += 8, FA_ERR_BAD_STRIDE, "kv_cache", 53);
    SCODE(t.kv_cache = mem + 4, FA_ERR_BAD_STRIDE, "kv_cache", 54);
    SCODE(t.topk = 33, FA_ERR_BAD_SHAPE, "topk", 55);
    { fa_mla_params_v2 t; fill(&t, 1); t.b = 0; t.q = t.kv_cache = t.o = NULL; t.lse = NULL; if (fa_run_mla_fwd_kvcache(D(&t), NULL) != FA_OK) return 60; }
    { fa_mla_sparse_params_v2 t; fills(&t, 1); t.b = 0; t.q = t.kv_cache = t.o = NULL; t.lse = NULL; t.indices = NULL; if (fa_run_mla_sparse_fwd_kvcache(S(&t), NULL) != FA_OK) return 61; }
    if (fa_abi_version() != 4) return 62;
    return 0;
}
""")
    exe = tmp_path / "use_mla_fp8"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


def test_ctypes_builders_pick_the_struct_by_the_cache():
    q = torch.zeros(2, 1, 16, 576, dtype=torch.float16)
    o = torch.zeros(2, 1, 16, 512, dtype=torch.float16)
    lse = torch.zeros(2, 16, 1)
    idx = torch.zeros(2, 1, 64, dtype=torch.int32)
    kv16 = torch.zeros(2, 128, 1, 576, dtype=torch.float16)
    for dt in (torch.uint8, F8):
        kv8 = torch.zeros(2, 128, 1, 672, dtype=torch.uint8).view(dt)[..., :656]
        p = capi.mla_params(q, kv8, o, lse, num_splits=2)
        assert isinstance(p, capi.MlaParamsV2) and p.struct_size == 248 and p.kv_format == capi.FA_MLA_KV_FP8_ROWS656 and p.reserved2_ == 0
        assert (p.kv_cache_stride.batch, p.kv_cache_stride.row) == (128 * 672, 672)            # bytes
        s = capi.mla_sparse_params(q, kv8, o, lse, idx, num_splits=2)
        assert isinstance(s, capi.MlaSparseParamsV2) and s.kv_format == capi.FA_MLA_KV_FP8_ROWS656
        p16, s16 = capi.mla_params(q, kv16, o, lse, num_splits=2), capi.mla_sparse_params(q, kv16, o, lse, idx, num_splits=2)
        assert type(p16) is capi.MlaParams and type(s16) is capi.MlaSparseParams and p16.struct_size == 240
        assert capi.mla_workspace_bytes(p) == capi.mla_workspace_bytes(p16) > 0
        assert capi.mla_sparse_workspace_bytes(s) == capi.mla_sparse_workspace_bytes(s16) > 0
        for forced in (0, 1, 3):
            p.num_splits = p16.num_splits = s.num_splits = s16.num_splits = forced
            assert capi.mla_workspace_bytes(p) == capi.mla_workspace_bytes(p16)
            assert capi.mla_sparse_workspace_bytes(s) == capi.mla_sparse_workspace_bytes(s16)
    for n in ("MlaParamsV2", "MlaSparseParamsV2", "mla_cache_is_fp8"):
        assert hasattr(capi, n), n


# ---- 4. build and ISA ---------------------------------------------------------------------------------------------------------------------------

def test_mla_fp8_kernels_isa():
    """8 dense + 4 sparse attention kernels, 4 quantising appends, 2 combines.  Every attention kernel: no scratch, an MFMA loop free of scratch traffic
    and accumulator moves that reads K as rows and V^T transposed from the same LDS images behind a barrier, 72 KB of LDS, subnormals kept, no MFMA
    result read early, M0 untouched, one workgroup per compute unit; the conversion to fp16 rounds to nearest (no v_cvt_pkrtz).  The 16-bit files keep
    their kernel counts."""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    name = "fa_fwd_kvcache_mla_fp8.hip"
    assert name in B.HIP_SOURCES and name in B.M0_GUARD_SOURCES and B.EXTRA_FLAGS[name] == B.EXTRA_FLAGS["fa_fwd_kvcache_mla.hip"]
    assert B.HIP_SOURCES.index(name) < B.HIP_SOURCES.index("fa_capi.hip")
    ks = analyse(name)
    dense = {n: k for n, k in ks.items() if "fa_fwd_kvcache_mla_fp8_kernelI" in n}
    sparse = {n: k for n, k in ks.items() if "fa_fwd_kvcache_mla_sparse_fp8_kernelI" in n}
    append = {n: k for n, k in ks.items() if "fa_kvcache_mla_append_fp8_kernelI" in n}
    assert (len(dense), len(sparse), len(append), len(ks)) == (8, 4, 4, 18), sorted(ks)
    assert sum("fa_kvcache_combine_kernelI" in n and "Li512E" in n for n in ks) == 2
    keys = set()
    for n, k in {**dense, **sparse}.items():
        m = re.search(r"fa_fwd_kvcache_mla_(sparse_)?fp8_kernelI(DF16_|DF16b)((?:Lb\dE)+)E", n)
        assert m, n
        keys.add(m.groups())
        assert k["scratch_bytes"] == 0, (n, k["scratch_bytes"])
        assert k["lds_bytes"] == 73728 == 2 * (32 * 1024 + 32 * 128), (n, k["lds_bytes"])
        assert k["occupancy"] == 1 and k["vgprs"] <= 256 and k["vgprs"] + k["agprs"] <= 512, (n, k["occupancy"], k["vgprs"], k["agprs"])
        assert (k["float_denorm_mode_32"], k["float_denorm_mode_16_64"]) == (3, 3), n
        assert k["mfma_hazards"] == [] and k["m0_outside_asm"] == 0, n
        assert k["loops"], f"{n}: no MFMA loop found"
        for lp in k["loops"]:
            assert lp["scratch_ops"] == 0 and lp["accvgpr_moves"] == 0, (n, lp["label"], lp["scratch_ops"], lp["accvgpr_moves"])
        main = max(k["loops"], key=lambda lp: lp["mfma"])
        assert main["ds_read_b128"] > 0 and main["ds_read_tr"] > 0 and main["barriers"] > 0, (n, main["label"])
        hist = main["histogram"]
        assert hist.get("v_cvt_pk_f32_fp8", 0) + hist.get("v_cvt_pk_f32_fp8_sdwa", 0) + hist.get("v_cvt_pk_f32_fp8_e32", 0) + hist.get("v_cvt_pk_f32_fp8_e64", 0) > 0, (n, sorted(hist))
        assert not any("pkrtz" in op for op in hist), n
    assert keys == ({(None, t, f"Lb{c}ELb{p}E") for t in ("DF16_", "DF16b") for c in "01" for p in "01"}
                    | {("sparse_", t, f"Lb{p}E") for t in ("DF16_", "DF16b") for p in "01"})
    for n, k in ks.items():
        if n not in dense and n not in sparse:
            assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0, n
    assert {re.search(r"append_fp8_kernelI(DF16_|DF16b)Lb(\d)E", n).groups() for n in append} == {(t, p) for t in ("DF16_", "DF16b") for p in "01"}
    assert len(analyse("fa_fwd_kvcache_mla.hip")) == 12 and len(analyse("fa_fwd_kvcache_mla_sparse.hip")) == 6
