"""GPU: the LDS-DMA protocols of fa_fwd_pp16 (role-split rings, counted waits) and fa_bwd_dkdv16 (toggled Q / dO rings) under ADVERSARIAL timing.

Why this module exists.  A race of the class "a consumer reads a ring slot before the wait + barrier that publishes the producer's
pieces" is invisible to every value test as long as the DMA is usually early: round 4's first counted-wait form was WRONG and bit-identical on every
shape (profiles/r4_fwd_counted_wait_racy_form_ab.log; found by walking the two wave groups' timelines side by side).  Determinism soaks cannot see it
either.  What can: builds of the SAME kernels whose DMA requests are moved, mechanically, to the latest point the protocol itself allows - directly in
front of the wait that retires them (`dma_late`), or behind a sleep longer than a tile period in one wave group (`dma_sleepy`).  A correct protocol
does not care when the bytes land as long as its own waits and barriers are honoured, so both builds must reproduce the product BIT FOR BIT; a protocol
that reads before the publishing barrier reads the slot's previous tenant and fails.  To show the method has teeth, the documented racy form is kept
in the source behind a test-only switch (`dma_racy`: bit-identical at normal timing, as round 4 recorded) and must FAIL under late issue
(`dma_racy_late`).  The debug libraries are built by flash-attention-turing_amd/build.py (DEBUG_VARIANTS) next to the product; the product's ISA is unchanged.

The same two builds also carry the switches of the other LDS-DMA kernels: fa_bwd_dq16 (the 16x16x32 dQ, compared on the shapes above), and the 32x32x16
set - fa_fwd_pp, fa_bwd_dq, fa_bwd_dkdv - which runs under a pinned policy on small shapes of its own (SHAPES32).  The register-staged decode kernels are
in tests/test_stage_protocol_gpu.py; tests/test_debug_variants_cpu.py checks that every build differs from the product as it should."""
import ctypes
import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (name, b, sq, sk, h, hk, dtype, causal): every shape reaches the unrolled steady loop of fa_fwd_pp16 under the default policy
# (asserted through capi.kernel_name in the test body - the policy's thresholds are stated in include/flash_attn_gfx950.h only; >= 4 unmasked tiles per workgroup) and fa_bwd_dkdv16
SHAPES = [
    ("c2_b4_s4096_h32", 4, 4096, 4096, 32, 32, torch.float16, False),            # BASELINE configs[1]
    ("causal_b1_s8192_h16", 1, 8192, 8192, 16, 16, torch.float16, True),
    ("ragged_b2_sq5000_sk5100_gqa", 2, 5000, 5100, 8, 2, torch.float16, False),
    ("bf16_b2_s4096_h8", 2, 4096, 4096, 8, 8, torch.bfloat16, False),
    # head_dim 64: the round-5 instances of both kernels - 128-key forward tiles, dK/dV with one piece per wave and ring and the 2^13 ring-toggle bit - share the switches
    ("d64_fp16_b2_s4096_h8", 2, 4096, 4096, 8, 8, torch.float16, False, 64),
    ("d64_fp16_causal_b1_s8192_h8", 1, 8192, 8192, 8, 8, torch.float16, True, 64),
]


# The 32x32x16 set (fa_fwd_pp.hip, fa_bwd.hip) under a pinned policy: (name, b, sq, sk, h, hk, causal).  The smallest shapes that reach each steady loop, read
# from the sources (256-row query blocks, 64-key tiles at both head dims below 16384 keys; n_main = key tiles every row of the block sees whole):
#   fa_fwd_pp_kernel   head_dim 128: the constant-slot loop `for (; u + 3 <= n_main; u += 3)` from u = 1 needs n_main >= 4, the tail loop `for (; u < n_main; ++u)`
#                      the tiles left over; head_dim 64 (64-key tiles): the tail loop alone, n_main >= 2.  Masked tiles run `iteration`, which carries the switch too.
#   fa_bwd_dq_kernel   requests tile t + 1 while t + 1 < n_tiles; head_dim 128 walks two tiles a trip (`t + 2 <= n_tiles`) and one more if n_tiles is odd.
#   fa_bwd_dkdv_kernel requests the next 64-row Q / dO tile while `it + 1 < n_iters`, n_iters = 64-row tiles x query heads of the KV head's group.
# full: 3 query blocks (88 rows in the last), 11 key tiles (60 keys in the last), n_main = 10, n_iters = 10 x 4.  causal: sq != sk, delta = 257; block 0 has
# n_main = 4 and two diagonal tiles, block 2 (8 rows) n_main = 12 of 13.  GQA 4 / 1 and 2 / 2.
SHAPES32 = [
    ("full_b2_sq600_sk700_gqa4", 2, 600, 700, 4, 1, False),
    ("causal_b1_sq520_sk777_gqa4", 1, 520, 777, 4, 1, True),
    ("causal_b2_sq600_sk600_h2", 2, 600, 600, 2, 2, True),
]
KERNELS32 = {"fwd": "fa_fwd_pp_kernel", "dq": "fa_bwd_dq_kernel", "dkdv": "fa_bwd_dkdv_kernel"}
STAGE_CODES = {"fwd": 0, "dq": 1, "dkdv": 2}
POLICY_MFMA32 = 0


def _build_module():
    spec = importlib.util.spec_from_file_location("fa_build", os.path.join(ROOT, "flash-attention-turing_amd", "build.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def libs(gpu):
    from flash_attn_turing import capi

    fa_build = _build_module()
    fa_build.build_debug_variants(force=False)          # a no-op when build() has run (the .so files travel with the tree); hipcc is on the GPU box otherwise
    out = {"product": capi.lib()}
    for name in ("dma_late", "dma_sleepy", "dma_racy", "dma_racy_late"):
        L = ctypes.CDLL(fa_build.debug_library_path(name))
        L.fa_run_mha_fwd.argtypes = [ctypes.POINTER(capi.FwdParams), ctypes.c_void_p]
        L.fa_run_mha_bwd.argtypes = [ctypes.POINTER(capi.BwdParams), ctypes.c_void_p]
        L.fa_kernel_name_dtype.restype = ctypes.c_char_p
        L.fa_kernel_name_dtype.argtypes = [ctypes.c_int32] * 8
        L.fa_set_kernel_policy.restype = ctypes.c_int32
        L.fa_set_kernel_policy.argtypes = [ctypes.c_int32]
        out[name] = L
    return out


def _inputs(gpu, b, sq, sk, h, hk, dt, d=128):
    g = torch.Generator(device=gpu).manual_seed(20260929)
    q, do = (torch.randn(b, sq, h, d, device=gpu, dtype=dt, generator=g) for _ in range(2))
    k, v = (torch.randn(b, sk, hk, d, device=gpu, dtype=dt, generator=g) for _ in range(2))
    return q, k, v, do


def _fwd(L, q, k, v, causal):
    from flash_attn_turing import capi

    o = torch.full_like(q, float("nan"))
    lse = torch.full((q.shape[0], q.shape[2], q.shape[1]), float("nan"), device=q.device, dtype=torch.float32)
    p = capi.fwd_params(q, k, v, o, lse, causal)
    assert L.fa_run_mha_fwd(ctypes.byref(p), torch.cuda.current_stream(q.device).cuda_stream) == 0
    torch.cuda.synchronize()
    return o, lse


def _bwd(L, q, k, v, o, lse, do, causal):
    from flash_attn_turing import capi

    dq, dk, dv = (torch.full_like(t, float("nan")) for t in (q, k, v))
    dsum = torch.empty_like(lse)
    p = capi.bwd_params(q, k, v, o, lse, do, dq, dk, dv, dsum, causal)
    assert L.fa_run_mha_bwd(ctypes.byref(p), torch.cuda.current_stream(q.device).cuda_stream) == 0
    torch.cuda.synchronize()
    return dq, dk, dv


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_product_protocol_is_bit_identical_under_adversarial_dma_timing(gpu, libs, shape):
    from flash_attn_turing import capi

    _, b, sq, sk, h, hk, dt, causal = shape[:8]
    d = shape[8] if len(shape) > 8 else 128
    dtn = "fp16" if dt == torch.float16 else "bf16"
    assert capi.kernel_name("fwd", b, sq, sk, h, d, causal, dtn) == "fa_fwd_pp16_kernel"
    # (head_dim 64 under a causal mask: dK/dV stays on the 32x32x16 kernel below 2^28 pairs per head - that shape is there for the forward)
    assert capi.kernel_name("dkdv", b, sq, sk, h, d, causal, dtn) == "fa_bwd_dkdv16_kernel" or (d == 64 and causal)
    # fa_bwd_dq16.hip carries the switches too (FA_DQ16_DMA_DEBUG): the dQ compared below comes from it
    assert capi.kernel_name("dq", b, sq, sk, h, d, causal, dtn) == "fa_bwd_dq16_kernel"
    q, k, v, do = _inputs(gpu, b, sq, sk, h, hk, dt, d)
    o, lse = _fwd(libs["product"], q, k, v, causal)
    assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
    grads = _bwd(libs["product"], q, k, v, o, lse, do, causal)
    for name in ("dma_late", "dma_sleepy"):
        for rep in range(2):
            o2, lse2 = _fwd(libs[name], q, k, v, causal)
            assert torch.equal(o, o2) and torch.equal(lse, lse2), (name, rep, (o.float() - o2.float()).abs().max().item())
        g2 = _bwd(libs[name], q, k, v, o, lse, do, causal)
        for a, c, t in zip(grads, g2, ("dq", "dk", "dv")):
            assert torch.equal(a, c), (name, t, (a.float() - c.float()).abs().max().item())


@pytest.mark.parametrize("dtn", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("shape", SHAPES32, ids=[s[0] for s in SHAPES32])
def test_mfma32_set_is_bit_identical_under_adversarial_dma_timing(gpu, libs, shape, d, dtn):
    """fa_fwd_pp.hip (the schedule the round-4 race lived in; small launches, smoke() included, run it) and both kernels of fa_bwd.hip, pinned through
    fa_set_kernel_policy on EACH library (every .so has its own policy global) and asserted through that library's fa_kernel_name_dtype"""
    _, b, sq, sk, h, hk, causal = shape
    dt = torch.float16 if dtn == "fp16" else torch.bfloat16
    names = ("product", "dma_late", "dma_sleepy")
    prev = {n: libs[n].fa_set_kernel_policy(POLICY_MFMA32) for n in names}
    try:
        for n in names:
            for stage, kernel in KERNELS32.items():
                got = libs[n].fa_kernel_name_dtype(STAGE_CODES[stage], 0 if dtn == "fp16" else 1, b, sq, sk, h, d, int(causal)).decode()
                assert got == kernel, (n, stage, got)
        q, k, v, do = _inputs(gpu, b, sq, sk, h, hk, dt, d)
        o, lse = _fwd(libs["product"], q, k, v, causal)
        assert torch.isfinite(o.float()).all() and torch.isfinite(lse).all()
        grads = _bwd(libs["product"], q, k, v, o, lse, do, causal)
        for name in names[1:]:
            for rep in range(2):
                o2, lse2 = _fwd(libs[name], q, k, v, causal)
                assert torch.equal(o, o2) and torch.equal(lse, lse2), (name, rep, (o.float() - o2.float()).abs().max().item())
                g2 = _bwd(libs[name], q, k, v, o, lse, do, causal)
                for a, c, t in zip(grads, g2, ("dq", "dk", "dv")):
                    assert torch.equal(a, c), (name, rep, t, (a.float() - c.float()).abs().max().item())
    finally:
        for n in names:
            libs[n].fa_set_kernel_policy(prev[n])


def test_late_issue_catches_the_documented_racy_form(gpu, libs):
    """the detector must fire on the bug it exists for: round 4's counted-wait form (K(u+2) left in flight across the barrier, the other group's half of
    the tile retired one barrier after the first read) is bit-identical to the product at normal timing - recorded, not asserted: it is a race - and
    wrong under late issue on every shape that reaches the steady loop"""
    seen_normal_equal = 0
    for _, b, sq, sk, h, hk, dt, causal in SHAPES[:3]:
        q, k, v, _ = _inputs(gpu, b, sq, sk, h, hk, dt)
        o, lse = _fwd(libs["product"], q, k, v, causal)
        o_r, _ = _fwd(libs["dma_racy"], q, k, v, causal)
        seen_normal_equal += int(torch.equal(o, o_r))
        o_rl, _ = _fwd(libs["dma_racy_late"], q, k, v, causal)
        diff = (o.float() - o_rl.float()).abs()
        assert not torch.equal(o, o_rl) and torch.nan_to_num(diff, nan=1.0).max().item() > 1e-2, "the late-issue build did not expose the racy form"
    print(f"racy form at normal timing: bit-identical to the product on {seen_normal_equal} of 3 shapes (the race is invisible to value tests)")
