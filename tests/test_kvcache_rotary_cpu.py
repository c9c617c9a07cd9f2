"""CPU: rotary embedding on the decode path (rotary_cos / rotary_sin / rotary_interleaved of flash_attn_with_kvcache, fa_kvcache_options_v3 of
the C ABI) - the struct layout against the header, old callers, validation codes before any device work, the workspace rule (the image of the
rotated q), the Python surface's validation, the number-format fact the bit-exact contract rests on, and the ISA of the fused kernel.  No GPU
involved.  rotate_ref below is the contract's formula in torch on the CPU; the GPU tests import it."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from flash_attn_turing import capi
from test_kvcache_window_cpu import EX_ENTRY_POINTS, _aligned_addr, _params, _rc

FP8 = capi.FA_CACHE_FP8_E4M3


def rotate_ref(x, cos, sin, positions, interleaved):
    """the contract, with torch on the CPU: x (b, s, heads, d), cos / sin (seqlen_ro, rotary_dim / 2) of x's dtype, positions (b, s) ints
    (already clamped to the tables by the caller).  Pair (a, b) = (x[i], x[i + rotary_dim / 2]) or, interleaved, (x[2 i], x[2 i + 1]);
    y_a = x_a c - x_b s, y_b = x_b c + x_a s, every operation its own fp32 torch op (no contraction), one rounding to x's dtype; elements
    at or past rotary_dim pass through."""
    x, cos, sin = x.detach().cpu(), cos.detach().cpu(), sin.detach().cpu()
    assert cos.dtype == x.dtype and sin.dtype == x.dtype and cos.shape == sin.shape
    positions = torch.as_tensor(positions, dtype=torch.long).cpu()
    rd = 2 * cos.shape[1]
    c, s = cos[positions].float()[:, :, None, :], sin[positions].float()[:, :, None, :]
    xf = x.float()
    ia, ib = (slice(0, rd, 2), slice(1, rd, 2)) if interleaved else (slice(0, rd // 2), slice(rd // 2, rd))
    xa, xb = xf[..., ia], xf[..., ib]
    y = x.clone()
    y[..., ia] = (xa * c - xb * s).to(x.dtype)
    y[..., ib] = (xb * c + xa * s).to(x.dtype)
    return y


def test_rotate_ref_is_the_textbook_rotation():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 4, 64, generator=g).half()
    ang = torch.rand(10, 16, generator=g) * 6.0
    cos, sin = ang.cos().half(), ang.sin().half()
    pos = torch.tensor([[0, 1, 2], [7, 8, 9]])
    for inter in (False, True):
        y = rotate_ref(x, cos, sin, pos, inter)
        assert torch.equal(y[..., 32:], x[..., 32:])                          # rotary_dim = 32 of 64: the rest passes through
        for bi in range(2):
            for si in range(3):
                c, s = cos[pos[bi, si]].double(), sin[pos[bi, si]].double()
                xr = x[bi, si, :, :32].double()
                a, b = (xr[:, 0::2], xr[:, 1::2]) if inter else (xr[:, :16], xr[:, 16:])
                ya, yb = a * c - b * s, b * c + a * s
                got = y[bi, si, :, :32].double()
                ga, gb = (got[:, 0::2], got[:, 1::2]) if inter else (got[:, :16], got[:, 16:])
                assert (ga - ya).abs().max() < 4e-3 and (gb - yb).abs().max() < 4e-3      # one fp16 rounding of |y| < 8
    # position 0 of a table built from angle 0 is the identity
    one, zero = torch.ones(4, 16).half(), torch.zeros(4, 16).half()
    assert torch.equal(rotate_ref(x, one, zero, torch.zeros(2, 3, dtype=torch.long), True), x)


# ---- 1. layout --------------------------------------------------------------------------------------------------------------------------

def _opt3(**kw):
    o = capi.KvcacheOptionsV3()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_options_v3_layout_matches_header(tmp_path):
    """fa_kvcache_options (20 bytes) and fa_kvcache_options_v2 (72) keep their layouts; v3 repeats the v2 fields at the same offsets, appends the
    rotary fields and is 112 bytes; ctypes agrees with a C program compiled against the header"""
    fields = [f[0] for f in capi.KvcacheOptionsV3._fields_]
    v2 = [f[0] for f in capi.KvcacheOptionsV2._fields_]
    assert fields[:len(v2)] == v2
    assert fields[len(v2):] == ["rotary_cos", "rotary_sin", "rotary_row_stride", "seqlen_ro", "rotary_dim", "rotary_interleaved", "reserved_"]
    src = tmp_path / "opt3_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flash_attn_gfx950.h"\n#ifndef FA_HAS_KVCACHE_ROTARY\n#error "no FA_HAS_KVCACHE_ROTARY"\n#endif\n'
                   'int main(void) {\n'
                   '    printf("size %zu %zu %zu\\n", sizeof(fa_kvcache_options_v3), sizeof(fa_kvcache_options_v2), sizeof(fa_kvcache_options));\n'
                   '    printf("abi %d 0\\n", FA_ABI_VERSION);\n'
                   + "".join(f'    printf("{f} %zu %zu\\n", offsetof(fa_kvcache_options_v3, {f}), sizeof(((fa_kvcache_options_v3*)0)->{f}));\n' for f in fields)
                   + "".join(f'    printf("v2_{f} %zu 0\\n", offsetof(fa_kvcache_options_v2, {f}));\n' for f in v2)
                   + "    fa_kvcache_options_v3 o;\n    FA_PARAMS_INIT(o);\n"
                     "    return o.struct_size == sizeof(o) && o.rotary_cos == NULL && o.rotary_sin == NULL && o.rotary_dim == 0 ? 0 : 1;\n}\n")
    exe = tmp_path / "opt3_layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe)])
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        k, *v = line.split()
        got[k] = [int(x) for x in v]
    assert got["size"] == [ctypes.sizeof(capi.KvcacheOptionsV3), ctypes.sizeof(capi.KvcacheOptionsV2), ctypes.sizeof(capi.KvcacheOptions)] == [112, 72, 20]
    assert got["abi"][0] == 4 == capi.lib().fa_abi_version()
    for f in fields:
        assert got[f] == [getattr(capi.KvcacheOptionsV3, f).offset, getattr(capi.KvcacheOptionsV3, f).size], f
    for f in v2:
        assert got["v2_" + f][0] == got[f][0], f
    assert 112 not in (8, 12, 16, 24, 28, 40, 64, 71, 76)                     # the sizes the older tests expect to be refused


SHAPES = [(1, 1, 32, 8, 131072, True), (1, 4, 32, 8, 32768, False), (3, 16, 16, 4, 768, True), (2, 33, 32, 1, 4096, False), (64, 1, 32, 8, 4096, False),
          (1, 1, 32, 8, 32768, False), (8, 1, 32, 32, 32768, False), (1, 16, 16, 4, 768, False), (3, 2, 8, 8, 100, False), (256, 1, 8, 8, 4096, False)]
WINDOWS = [(-1, -1), (0, 0), (31, 0), (4095, 0), (127, 3), (7, -1)]


@pytest.mark.parametrize("fn", ["fa_kvcache_workspace_bytes_ex", "fa_kvcache_num_splits_ex"])
def test_v3_with_a_zeroed_tail_is_a_v2_call(fn):
    """same split and workspace from fa_kvcache_options, fa_kvcache_options_v2 and a v3 struct whose rotary fields are zero - 16-bit and 8-bit cache"""
    f = getattr(capi.lib(), fn)
    for b, sq, h, hk, cache, causal in SHAPES:
        for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
            for page in (None, 256) if cache % 256 == 0 else (None,):
                for ws in (None, 1 << 40, 3 * b * h * sq * 128 * 4 + (3 * b * h * sq * 4 + 15) // 16 * 16):
                    p = _params(b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, page=page, ws_bytes=ws, **kw)
                    for win in WINDOWS:
                        old = capi.kvcache_options(win)
                        want = f(ctypes.byref(p), ctypes.byref(old))
                        assert want >= 0, capi.last_error()
                        for fp8 in (0, FP8):
                            v2 = capi.KvcacheOptionsV2()
                            v3 = _opt3()
                            assert (v2.struct_size, v3.struct_size) == (72, 112)
                            for o in (v2, v3):
                                o.is_local, o.window_size_left, o.window_size_right, o.cache_dtype = old.is_local, old.window_size_left, old.window_size_right, fp8
                                # the other rotary fields are not read without the tables
                            v3.seqlen_ro, v3.rotary_dim, v3.rotary_interleaved, v3.rotary_row_stride = 7, 5, 1, 3
                            assert f(ctypes.byref(p), ctypes.byref(v2)) == want == f(ctypes.byref(p), ctypes.byref(v3)), (b, sq, cache, page, ws, kw, win, fp8)


# ---- 2. validation ----------------------------------------------------------------------------------------------------------------------

def _rot_params(fn, sn=1, **kw):
    """dummy params with k_new / v_new (rotary needs them) and, for the queries, a workspace that holds any image; b = 0 for the launch"""
    p = _params(**kw)
    buf, addr = _aligned_addr()
    p.k_new = p.v_new = addr
    p.seqlen_new = sn
    p.k_new_stride = p.v_new_stride = capi.Strides(sn * p.h_k * p.d, p.h_k * p.d, p.d)
    p._keep2 = buf
    if p.workspace is None:
        p.workspace, p.workspace_bytes = addr, 1 << 40
    if fn == "fa_run_mha_fwd_kvcache_ex":
        p.b = 0                                          # (the addresses are dummies: b = 0 is validated and launches nothing)
    return p


def _rot(addr, cache=32768, dim=128, **kw):
    base = dict(rotary_cos=addr, rotary_sin=addr, rotary_row_stride=dim // 2, seqlen_ro=cache, rotary_dim=dim, rotary_interleaved=1)
    base.update(kw)
    return _opt3(**base)


@pytest.mark.parametrize("fn", EX_ENTRY_POINTS)
def test_rotary_option_validation_codes(fn):
    buf, addr = _aligned_addr()
    S, ST, ABI = capi.FA_ERR_BAD_SHAPE, capi.FA_ERR_BAD_STRIDE, capi.FA_ERR_BAD_ABI
    # what is accepted
    for o in (_rot(addr), _rot(addr, dim=16), _rot(addr, dim=64, rotary_interleaved=0), _rot(addr, seqlen_ro=32768 + 5), _rot(addr, rotary_row_stride=1024),
              _rot(addr, cache_dtype=FP8), _rot(addr, is_local=1, window_size_left=37, window_size_right=0), _opt3(), _opt3(cache_dtype=FP8)):
        assert _rc(_rot_params(fn), fn, o) >= 0, capi.last_error()
    assert _rc(_rot_params(fn, d=64), fn, _rot(addr, dim=64)) >= 0, capi.last_error()
    # one table without the other
    for kw in (dict(rotary_cos=None), dict(rotary_sin=None)):
        assert _rc(_rot_params(fn), fn, _rot(addr, **kw)) == S, kw
        assert "both" in capi.last_error()
    # rotary_dim: a multiple of 16 in [16, d]
    for dim in (0, 8, 24, 15, 17, 120, 144, 256, -16):
        assert _rc(_rot_params(fn), fn, _rot(addr, dim=dim, rotary_row_stride=128)) == S, dim
        assert "rotary_dim" in capi.last_error()
    assert _rc(_rot_params(fn, d=64), fn, _rot(addr, dim=128)) == S and "rotary_dim" in capi.last_error()
    # the tables cover the capacity
    for ro in (0, 1, 32767, -1):
        assert _rc(_rot_params(fn), fn, _rot(addr, seqlen_ro=ro)) == S, ro
        assert "seqlen_ro" in capi.last_error()
    assert _rc(_rot_params(fn, cache=4096, page=256), fn, _rot(addr, seqlen_ro=4095)) == S and "seqlen_ro" in capi.last_error()
    assert _rc(_rot_params(fn, cache=4096, page=256), fn, _rot(addr, seqlen_ro=4096)) >= 0, capi.last_error()
    # rotary without k_new / v_new
    p = _rot_params(fn)
    p.k_new = p.v_new = None
    p.seqlen_new = 0
    assert _rc(p, fn, _rot(addr)) == S and "k_new" in capi.last_error()
    # alignment
    for kw in (dict(rotary_cos=addr + 8), dict(rotary_sin=addr + 2), dict(rotary_cos=addr + 4, rotary_sin=addr + 4)):
        assert _rc(_rot_params(fn), fn, _rot(addr, **kw)) == ST, kw
        assert "16-byte aligned" in capi.last_error()
    for stride in (68, 65, 60, 56, 8, 0, -64):
        assert _rc(_rot_params(fn), fn, _rot(addr, rotary_row_stride=stride)) == ST, stride
        assert "rotary_row_stride" in capi.last_error()
    # struct sizes: exactly three are accepted
    for size in (24, 28, 40, 64, 71, 76, 80, 96, 104, 108, 111, 113, 116, 120, 128):
        o = _rot(addr)
        o.struct_size = size
        assert _rc(_rot_params(fn), fn, o) == ABI, size
    # params errors still come first, and so do the older options' errors
    assert _rc(_rot_params(fn, h=3, hk=2), fn, _rot(addr, dim=24)) == capi.FA_ERR_BAD_GQA
    assert _rc(_rot_params(fn), fn, _rot(addr, dim=24, cache_dtype=9)) == capi.FA_ERR_BAD_DTYPE
    assert _rc(_rot_params(fn), fn, _rot(addr, dim=24, is_local=1, window_size_left=-2)) == S and "window_size" in capi.last_error()


# ---- 3. workspace -----------------------------------------------------------------------------------------------------------------------

def _align16(n):
    return (n + 15) // 16 * 16


def test_workspace_is_the_image_plus_the_plain_workspace_and_the_split_is_unchanged():
    buf, addr = _aligned_addr()
    L = capi.lib()
    for b, sq, h, hk, cache, causal in SHAPES:
        for d in (64, 128):
            for kw in (dict(), dict(num_splits=3), dict(num_splits=500)):
                for win in ((-1, -1), (31, 0), (4095, 0)):
                    for fp8 in (0, FP8):
                        image = _align16(b * sq * h * d * 2)
                        plain_o = _opt3(cache_dtype=fp8)
                        rot_o = _rot(addr, cache=cache, dim=d // 2, cache_dtype=fp8)
                        if win != (-1, -1):
                            for o in (plain_o, rot_o):
                                o.is_local, o.window_size_left, o.window_size_right = 1, win[0], win[1]
                        p = _rot_params("fa_kvcache_workspace_bytes_ex", b=b, sq=sq, h=h, hk=hk, cache=cache, causal=causal, d=d, **kw)
                        plain = L.fa_kvcache_workspace_bytes_ex(ctypes.byref(p), ctypes.byref(plain_o))
                        assert plain >= 0, capi.last_error()
                        assert L.fa_kvcache_workspace_bytes_ex(ctypes.byref(p), ctypes.byref(rot_o)) == plain + image, (b, sq, h, d, cache, kw, win, fp8)
                        # the split: unlimited, exactly what the query states, and capped by what is left behind the image
                        for split_ws in (1 << 40, plain, plain // 2, 0):
                            p.workspace_bytes = split_ws
                            want = L.fa_kvcache_num_splits_ex(ctypes.byref(p), ctypes.byref(plain_o))
                            assert want >= 1, capi.last_error()
                            p.workspace_bytes = split_ws + image
                            assert L.fa_kvcache_num_splits_ex(ctypes.byref(p), ctypes.byref(rot_o)) == want, (b, sq, h, d, cache, kw, win, fp8, split_ws)
                        # a workspace that cannot hold the image: an error that names the bytes needed
                        for ws, nbytes in ((addr, image - 16), (None, 0)):
                            p.workspace, p.workspace_bytes = ws, nbytes
                            for fn in ("fa_kvcache_num_splits_ex", "fa_run_mha_fwd_kvcache_ex"):
                                assert _rc(p, fn, rot_o) == capi.FA_ERR_BAD_SHAPE, (fn, ws, nbytes)
                                assert str(image) in capi.last_error() and "workspace" in capi.last_error()
                            assert L.fa_kvcache_workspace_bytes_ex(ctypes.byref(p), ctypes.byref(rot_o)) == plain + image      # (the query ignores the fields)


def test_plain_c_caller_uses_the_v3_struct(tmp_path):
    src = tmp_path / "use_rotary.c"
    src.write_text(r"""
#include <stdio.h>
#include <string.h>
#include "flash_attn_gfx950.h"
static _Alignas(16) char mem[256];
int main(void) {
    fa_kvcache_params p;
    FA_PARAMS_INIT(p);
    p.q = p.k_cache = p.v_cache = p.o = mem; p.lse = (float*)mem; p.cache_seqlens = (const int32_t*)mem;
    p.k_new = p.v_new = mem; p.seqlen_new = 1;
    p.b = 1; p.seqlen_q = 1; p.seqlen_cache = 32768; p.h = 32; p.h_k = 8; p.d = 128; p.dtype = FA_FP16;
    p.q_stride = p.o_stride = (fa_strides){32 * 128, 32 * 128, 128};
    p.k_cache_stride = p.v_cache_stride = (fa_strides){32768LL * 8 * 128, 8 * 128, 128};
    p.k_new_stride = p.v_new_stride = (fa_strides){8 * 128, 8 * 128, 128};
    fa_kvcache_options_v2 o2;
    FA_PARAMS_INIT(o2);
    fa_kvcache_options_v3 o3;
    FA_PARAMS_INIT(o3);
    long long plain = fa_kvcache_workspace_bytes(&p);
    if (plain <= 0) return 10;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o2) != plain) return 11;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o3) != plain) return 12;
    o3.rotary_cos = o3.rotary_sin = mem; o3.rotary_row_stride = 64; o3.seqlen_ro = 32768; o3.rotary_dim = 128; o3.rotary_interleaved = 1;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o3) != plain + 32 * 128 * 2) return 13;
    p.workspace = mem; p.workspace_bytes = plain + 32 * 128 * 2;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o3) != fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o2)) return 14;
    o3.rotary_dim = 24;
    if (fa_kvcache_num_splits_ex(&p, (const fa_kvcache_options*)&o3) != FA_ERR_BAD_SHAPE || !strstr(fa_last_error(), "rotary_dim")) return 15;
    o3.rotary_dim = 128; o3.rotary_sin = NULL;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o3) != FA_ERR_BAD_SHAPE) return 16;
    o3.rotary_sin = mem + 8;
    if (fa_kvcache_workspace_bytes_ex(&p, (const fa_kvcache_options*)&o3) != FA_ERR_BAD_STRIDE) return 17;
    o3.rotary_sin = mem; p.b = 0;
    if (fa_run_mha_fwd_kvcache_ex(&p, (const fa_kvcache_options*)&o3, NULL) != FA_OK) return 18;      /* nothing to do: no launch */
    return 0;
}
""")
    exe = tmp_path / "use_rotary"
    libdir = os.path.dirname(capi.LIBRARY_PATH)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(capi.HEADER_PATH), str(src), "-o", str(exe),
                           "-L", libdir, "-l:libflash_attn_gfx950.so", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)


# ---- 4. the Python surface ----------------------------------------------------------------------------------------------------------------

def test_python_surface_rejects_bad_rotary_arguments():
    import flash_attn_turing as F

    b, hk, d, cap = 2, 2, 64, 32
    q = torch.zeros(b, 1, 4, d, dtype=torch.float16)
    kc = torch.zeros(b, cap, hk, d, dtype=torch.float16)
    kn = torch.zeros(b, 1, hk, d, dtype=torch.float16)
    cos = torch.ones(cap, 16, dtype=torch.float16)
    sin = torch.zeros(cap, 16, dtype=torch.float16)

    def call(**kw):
        args = dict(k=kn, v=kn, cache_seqlens=4, rotary_cos=cos, rotary_sin=sin)
        args.update(kw)
        return F.flash_attn_with_kvcache(q, kc, kc, **args)

    for kw in (dict(rotary_sin=None), dict(rotary_cos=None)):
        with pytest.raises(ValueError, match="both be given or both be None"):
            call(**kw)
    for bad in (cos.float(), cos.bfloat16(), cos.double()):
        with pytest.raises(ValueError, match="rotary_cos must be a tensor of q's dtype"):
            call(rotary_cos=bad)
        with pytest.raises(ValueError, match="rotary_sin must be a tensor of q's dtype"):
            call(rotary_sin=bad)
    with pytest.raises(ValueError, match="rotary_cos must be a tensor"):
        call(rotary_cos=1.0)
    for bad in (cos[0], cos[None], cos[:, :, None]):
        with pytest.raises(ValueError, match=r"rotary_cos must have shape \(seqlen_ro, rotary_dim / 2\)"):
            call(rotary_cos=bad)
    for bad in (sin[:, :8], sin[:-1], torch.zeros(cap + 1, 16, dtype=torch.float16)):
        with pytest.raises(ValueError, match="same shape"):
            call(rotary_sin=bad)
    with pytest.raises(ValueError, match="rotary_sin must be on q's device"):
        call(rotary_sin=sin.to("meta"))
    with pytest.raises(ValueError, match="last dimension must be contiguous"):
        call(rotary_cos=torch.ones(cap, 32, dtype=torch.float16)[:, ::2])
    for half in (4, 12, 20, 40, 48):                       # rotary_dim 8, 24, 40: not multiples of 16 or too small; 80, 96: > d
        t = torch.zeros(cap, half, dtype=torch.float16)
        with pytest.raises(ValueError, match="rotary_dim"):
            call(rotary_cos=t, rotary_sin=t)
    for rows in (cap - 1, 1):
        with pytest.raises(ValueError, match="seqlen_ro"):
            call(rotary_cos=cos[:rows], rotary_sin=sin[:rows])
    # paged: the capacity is max_blocks_per_seq x page_block_size
    pool = torch.zeros(8, 16, hk, d, dtype=torch.float16)
    table = torch.zeros(b, 3, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"seqlen_ro .* capacity \(48\)"):
        F.flash_attn_with_kvcache(q, pool, pool, k=kn, v=kn, cache_seqlens=4, block_table=table, rotary_cos=cos, rotary_sin=sin)
    with pytest.raises(ValueError, match="only applicable if k and v are passed in"):
        call(k=None, v=None)
    for bad in (1, 0, None, "yes", torch.tensor(True)):
        with pytest.raises(ValueError, match="rotary_interleaved must be a bool"):
            call(rotary_interleaved=bad)
        with pytest.raises(ValueError, match="rotary_interleaved must be a bool"):
            F.flash_attn_with_kvcache(q, kc, kc, cache_seqlens=4, rotary_interleaved=bad)
    with pytest.raises(RuntimeError, match="forward-only"):
        F.flash_attn_with_kvcache(q.clone().requires_grad_(True), kc, kc, k=kn, v=kn, cache_seqlens=4, rotary_cos=cos, rotary_sin=sin)
    # a CPU call that passes the checks is still refused by the extension (no quiet fall-back), positional and keyword forms alike
    for kw in (dict(), dict(rotary_interleaved=False), dict(causal=True, window_size=(7, 0))):
        with pytest.raises(RuntimeError, match="GPU"):
            call(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        F.flash_attn_with_kvcache(q, kc, kc, kn, kn, 4, False, 0, False)


def test_extension_signature_keeps_the_old_calls_and_gains_the_keywords():
    from flash_attn_turing import _C

    doc = _C.fwd_kvcache.__doc__
    sig = doc[:doc.index("->")]
    assert re.search(r"v_descale: [^,]*= None, rotary_cos: [^,]*= None, rotary_sin: [^,]*= None, rotary_interleaved: bool = True\)", sig), sig
    assert sig.index("*, k_descale") < sig.index("rotary_cos")               # keyword-only, after v_descale


# ---- 5. the number-format fact ------------------------------------------------------------------------------------------------------------

def _all_patterns(dt):
    return torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(dt)


def _sample(dt, n, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randint(-32768, 32768, (n,), generator=g, dtype=torch.int32).to(torch.int16).view(dt)
    fi = torch.finfo(dt)
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, fi.max, -fi.max, fi.tiny, fi.smallest_normal * 0.5, fi.eps, 1.0 + fi.eps, 3.0, 1.0 / 3.0, 0.1], dtype=torch.float32).to(dt)
    x = torch.cat([rnd, edge])
    return x[torch.isfinite(x.float())]


def test_fp16_products_are_exact_in_fp32():
    """EVERY fp16 c against a sample of x: the fp32 product equals the fp64 (= exact, 22 significant bits) product - no exceptions, subnormals and
    the largest values included - so y = x_a c -/+ x_b s is the correctly rounded fp32 sum of two exact terms whether or not the two steps are
    contracted into an FMA"""
    c = _all_patterns(torch.float16)
    c = c[torch.isfinite(c.float())]
    x = _sample(torch.float16, 600, 5)
    p32 = x.float()[:, None] * c.float()[None, :]
    p64 = x.double()[:, None] * c.double()[None, :]
    assert torch.isfinite(p32).all()
    assert torch.equal(p32.double(), p64)


def test_bf16_products_are_exact_in_fp32_inside_its_exponent_range():
    """EVERY bf16 c against a sample of x: the fp32 product (16 significant bits) is exact wherever it stays inside fp32's normal range -
    bf16 shares fp32's exponent range, so the product of two tiny values can leave it, which fp16 cannot; that is why the kernel switches
    contraction off instead of relying on exactness.  Inside [2^-60, 2^60] x [2^-60, 2] - any activation against any cos / sin value that
    is not an underflowed zero - nothing is excluded."""
    c = _all_patterns(torch.bfloat16)
    c = c[torch.isfinite(c.float())]
    x = _sample(torch.bfloat16, 600, 6)
    p32 = x.float()[:, None] * c.float()[None, :]
    p64 = x.double()[:, None] * c.double()[None, :]
    fi = torch.finfo(torch.float32)
    inside = (p64 == 0) | ((p64.abs() >= fi.smallest_normal) & (p64.abs() <= fi.max))
    assert torch.equal(p32.double()[inside], p64[inside])
    xin = (x.float().abs() >= 2.0 ** -60) & (x.float().abs() <= 2.0 ** 60)
    cin = (c.float().abs() >= 2.0 ** -60) & (c.float().abs() <= 2.0)
    assert inside[xin][:, cin].all() and int(xin.sum()) > 100 and int(cin.sum()) > 15000


def test_two_step_fp32_rotation_is_correctly_rounded_for_fp16():
    """2^20 random fp16 (x_a, x_b, c, s): x_a c - x_b s in two fp32 steps equals the exact value (exact products, summed exactly in fp64: two
    22-bit terms whose exponents lie within 30 of each other) rounded to fp32 - which is what an FMA would give as well"""
    g = torch.Generator().manual_seed(9)
    n = 1 << 20
    xa, xb = (torch.randn(n, generator=g) * 2).half(), (torch.randn(n, generator=g) * 2).half()
    ang = torch.rand(n, generator=g) * 6.2831853
    c, s = ang.cos().half(), ang.sin().half()
    two_step = (xa.float() * c.float() - xb.float() * s.float())
    exact = xa.double() * c.double() - xb.double() * s.double()             # both products exact; the fp64 sum of two 22-bit terms within 2^30 of each other is exact
    assert torch.equal(two_step.double(), exact.float().double())            # fp32 sum = the correctly rounded exact value
    assert torch.equal(two_step.half(), exact.float().half())


# ---- 6. ISA -------------------------------------------------------------------------------------------------------------------------------

def test_rotary_kernels_isa():
    """one fused kernel per (dtype, head_dim, paged, fp8): no scratch, no MFMA, no LDS, M0 untouched; 16-byte global loads and stores, nothing
    narrower than 8 bytes stored anywhere and nothing narrower than 16 in the 16-bit kernels; the rotation's multiplies and adds stay separate
    instructions (no contraction)"""
    from _kernel_isa import analyse
    import build as B                                   # (on sys.path through _kernel_isa)

    ks = {n: k for n, k in analyse("fa_kvcache_rotary.hip").items() if "fa_kvcache_rotary_kernel" in n}
    assert len(ks) == 16
    keys = set()
    src = os.path.join(B.CSRC, "fa_kvcache_rotary.hip")
    asm = subprocess.run([B.hipcc_path()] + B.HIPCC_FLAGS + ["-I", B.CSRC, "-I", B.INCLUDE, "-Wno-unused-command-line-argument", "--cuda-device-only", "-S", src, "-o", "-"],
                         capture_output=True, text=True, check=True).stdout
    assert B.m0_uses_outside_asm(asm) == 0
    assert "fa_kvcache_rotary.hip" in B.HIP_SOURCES and "fa_kvcache_rotary.hip" in B.M0_GUARD_SOURCES and "fa_kvcache_quant.hpp" in B.HIP_HEADERS
    for n, k in ks.items():
        m = re.search(r"fa_kvcache_rotary_kernelI(DF16_|DF16b)Li(\d+)ELb(\d)ELb(\d)E", n)
        assert m, n
        keys.add(m.groups())
        fp8 = m.group(4) == "1"
        assert k["scratch_bytes"] == 0 and k["lds_bytes"] == 0 and k["agprs"] == 0 and k["vgprs"] <= 64, (n, k)
        assert k["mfma_total"] == 0 and k["m0_outside_asm"] == 0 and k["mfma_hazards"] == [], n
        body = asm[asm.index(n + ":"):]
        body = body[:re.search(r"^\.Lfunc_end\d+:", body, re.M).start()]
        ops = set(re.findall(r"^\s+((?:global|buffer|flat|scratch)_[a-z0-9_]+)", body, re.M))
        assert "global_load_dwordx4" in ops and "global_store_dwordx4" in ops, (n, ops)
        stores = {o for o in ops if "store" in o or "atomic" in o}
        assert stores == ({"global_store_dwordx4", "global_store_dwordx2"} if fp8 else {"global_store_dwordx4"}), (n, stores)
        assert not any(o.startswith(("scratch_", "flat_")) for o in ops), (n, ops)
        cvt = "v_cvt_pk_bf16_f32" if m.group(1) == "DF16b" else "v_cvt_pk_f16_f32"
        assert len(re.findall(cvt, body)) == 4, n                          # eight results, rounded once, two at a time
        if not fp8:                                                      # (the 8-bit kernels hold the quantiser's division, which is made of FMAs)
            assert not re.search(r"\bv_(?:pk_)?(?:fma|fmac|mad|mac)_(?:f32|legacy)", body), n
    assert keys == {(t, d, p, f) for t in ("DF16_", "DF16b") for d in ("64", "128") for p in "01" for f in "01"}
