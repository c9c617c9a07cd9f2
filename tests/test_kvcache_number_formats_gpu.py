"""GPU: flash_attn_with_kvcache at every e4m3 code, every 16-bit value and across the range of V and of the descales.

Every other value test of the KV-cache kernels draws q, K and V from N(0, 1) with descales in [0.25, 4] and checks against the suite's absolute
bounds, so a conversion that is wrong for ONE exponent value, a kernel that loses small or large magnitudes, or a descale folded at the wrong
place would pass.  What the gfx950 conversion instructions (e4m3 -> fp16 / bf16 in `widen8`, fp32 -> e4m3 in `quant8_e4m3`) do with the
subnormal codes, the top binade, the NaN codes, saturation and ties cannot be learned on a CPU; it is walked here, exhaustively.  "Every path"
below is the list PATHS (base / causal, paged, window, split + combine, ragged, soft cap, sinks, tree, 64-row prefill, head_dim 256, fused
rotary append), each over a 16-bit and over an FP8 cache, minus what the interface refuses.  Fixed CPU-generator seeds throughout.

  A. One visible key copies V exactly.  A row that sees one key has P = 1, l = 1, O = v in fp32 math.  With q = 0 by construction; with q from
     N(0, 1) the kernel's l is exp2 of a rounding residue of at most |s c| 2^-24, a relative perturbation of about 1e-6: far below half an ulp
     of fp16 (2^-12) or bf16 (2^-9) and below half a step of the subnormal grid, so O is still v BIT FOR BIT.  16-bit cache: V holds all finite
     bit patterns of the dtype (63488 in fp16, 65280 in bf16; subnormals and the largest finite value among them), out must equal V's bits;
     where V is +-0 a zero of either sign is required (the accumulator starts at +0, and +0 + 1 x -0 = +0).  FP8 cache: V holds the 254 finite
     codes (NaN codes fill every row past L and must never show), one sequence per v_descale in {1, 2^-3, 2^5, 0.37, 2.9}: out equals the fp32
     product float(code) x v_descale rounded once to the dtype (inv = v_descale / l with l = 1; for the powers of two the product is exact).
     Geometry per path: L = 1, sq = 1 (capacity 96, so num_splits = 3 runs the combine); window: sq 16, L 40, window (0, 0), row t sees key
     24 + t alone, rows 0 .. 23 hold other finite patterns; tree: sq 64, L 64, mask word t = 1 << t; rotary: the row is appended by the call.
     At nheads = nheads_k and at nheads / nheads_k = 4 (the four heads of a token give identical rows).
  B. Every e4m3 code on the K side, every 16-bit q.  L = 1, num_splits = 1, softmax_scale = 1, a one-hot q row (1.0 at element j): the row's
     LSE is K[j] x k_descale.  sq 16 and nheads = nheads_k, so the 16 rows of a tile read 16 different elements; 36 (sequence, head) pairs read
     all 254 finite codes twice at different elements, and four pairs hold a NaN code (0x7f, 0xff): all rows of those pairs are NaN in O and
     LSE, every other row is finite.  Bound, derived: |lse - x| <= 2^-20 max(|x|, 1) with x = float(code) x k_descale in float64 - lse =
     fl(m sc) + logf(l) carries a few fp32 roundings (relative 2^-23 each) and l = exp2(residue), |residue| <= |x log2 e| 2^-24, so log l is
     within 2^-24 |x| + 1.2e-7; neighbouring e4m3 values differ by 2^-4 relative (2^-9 absolute in the subnormals), so a mis-widened code
     misses by orders of magnitude.  Under softcap = 30 the expectation is 30 tanh(x / 30) and the bound adds 30 x 2^-22: the tanh is 1 - 2 /
     (2^y + 1) with the hardware exponential and reciprocal (fa_fwd_kvcache.hip: "absolute error about 1e-7") - 2^y + 1 carries 2^-23 from the
     exponential and 2^-23 from the addition near 2, its reciprocal a quarter of that plus its own 2^-24, doubled: 2^-22 = 2.4e-7.  16-bit q:
     K is one-hot and q holds all finite patterns, LSE = q[j]; the same bound.  THE CONTRACT ENDS at |score| x log2 e = 2^31, which only bf16
     can reach: the kernels take p = exp2(fma(s, c, -fl(m c))), whose argument is the rounding residue of m c, at most |m c| 2^-24 - up to
     2^31 that is at most 64 and costs the LSE a relative 2^-24, from 2^32 on exp2 of it overflows (O and LSE not finite; first seen at q =
     3.09e9) or underflows to a dead row.  So the bf16 patterns go up to |q| < 2^30; the precondition is stated in README.md and interface.py.
  C. Every 16-bit input through every append kernel.  k_new / v_new hold all 65536 bit patterns (NaNs of both signs and +-inf included),
     appended at lengths that cross page boundaries.  FP8 cache: every cache byte after the call equals the contract formula evaluated by torch
     on the CPU (test_kvcache_fp8_gpu.quantise; NaN -> 0x7f / 0xff by sign), under the descales 1, 3, 1/3, 0.013, 7.3, 2^-6, 53.248, 448 /
     65504, 1e-3, 1e3, one per (sequence, head), each meeting all 65536 inputs.  This pins the conversion, the clamp, the NaN rule and the
     rounding into the subnormals; it does NOT separate a correctly rounded fp32 division from a reciprocal-multiply (with 16-bit inputs the
     two differ on 2 of these 1.3 million cases).  16-bit cache: the appended rows are a copy of the input bits, NaN payloads included.  No
     other byte changes.  Kernels: dense and ragged (packed k / v under cu_seqlens_k_new) appends, contiguous and paged, at d 64 / 128 / 256,
     and the fused rotary append (rotary_dim 16: the patterns sit in the unrotated tail, the rotated head against rotate_ref).
  D. V across its range against the C oracle (fp16).  Lengths 1, 2, 31, 33, 100, 777, sq 3, h 8 / h_k 2, causal, V = fp16(N(0, 1) x 2^e), e in
     {-14, +12} (two thirds of V subnormal at -14, max |O| 1.4e4 at +12).  Kernel, oracle (ROUND_FP16) and float64 math x 2^-e (exact), then
     U.assert_close at the plain tolerances: one step of the subnormal output grid is 9.8e-4 after rescaling, inside the bound, and the ulp
     slack covers outputs near 1e4.  LSE unscaled within LSE_TOL; everything finite.  FP8 counterpart: codes quantised from N(0, 1) under a
     descale in [0.25, 4], v_descale x 2^e, the oracle on the dequantised cache.
  E. Exact power-of-two relations, out and lse bit for bit, on the problem of D at unit scale, num_splits 1 and 3: V x 2^e (bf16) and
     v_descale x 2^e (bf16, FP8 cache) scale out by exactly 2^e and leave lse, e in {-24, -8, +8, +24}; k_descale x 2^e with softmax_scale x
     2^-e changes no bit (e in {-8, -3, +3, +8}; with sinks present as well: sinks are in units of the final scores); q x 2^e with k_descale x
     2^-e changes no bit (e in {-3, +3}, |q| below 2^-6 lifted to 2^-6 first).  On the soft-cap path only the last two (the descale multiplies
     the score inside the tanh).  A kernel that breaks one has an intermediate the algorithm does not have, or a conversion that is not
     round-to-nearest.

Measured on the MI355X (150 cases, 10 s; also in DESIGN.md section 3.5a).  A, C, E: every case bit for bit.  B, worst |lse - x|: e4m3 codes 3.1e-5 at
|x| = 448 (0.07 of the bound; 7.6e-6 under k_descale 0.37), soft cap 3.7e-6 (0.43 of its bound: the tanh is 1.2e-7 off), fp16 q 3.9e-3 at |x| =
4.6e4 (0.09 of the bound), bf16 q below 2^30 64 at |x| = 7.5e8 (0.09 of the bound); bf16 q from 3.09e9 on: non-finite LSE (see B).  D, worst raw metrics after rescaling
over the 36 cases: max_abs 9.8e-4 (one step of the subnormal output grid), mean_abs 2.5e-5, mean_rel 3.0e-3, LSE 9.5e-7."""
import math

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from oracle import attn_oracle as A
from test_kvcache_fp8_gpu import _bits, _descale, deq, quantise
from test_kvcache_rotary_cpu import rotate_ref
from test_kvcache_rotary_gpu import positions, tables
from test_kvcache_window_gpu import _bounds
from test_kvcache_window_gpu import _exact as window_exact

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
F8 = torch.float8_e4m3fn
NAN8, NAN16 = 0x7F, 0x7FC1                                   # 0x7fc1: a NaN in fp16 and in bf16
FINITE8 = torch.tensor([c for c in range(256) if c & 0x7F != 0x7F], dtype=torch.uint8)
VDS = (1.0, 2.0 ** -3, 2.0 ** 5, 0.37, 2.9)                  # A: one sequence per v_descale
APPEND_DESCALES = (1.0, 3.0, 1.0 / 3.0, 0.013, 7.3, 2.0 ** -6, 53.248, 448.0 / 65504.0, 1e-3, 1e3)
SOFTCAP = 30.0
TANH_ERR = 2.0 ** -22                                        # see B in the docstring
SCORE_LIMIT_EXP = 30                                         # bf16 q patterns: |q| < 2^30 (the contract ends at |score| x log2 e = 2^31)

# what a path adds to the plain call (num_splits = 1 unless the path or the caller says otherwise)
PATHS = {
    "base": dict(), "causal": dict(causal=True), "paged": dict(paged=True), "window": dict(causal=True, window=(0, 0)),
    "window40": dict(causal=True, window=(40, 0)), "split": dict(num_splits=3), "ragged": dict(ragged=True), "ragged_paged": dict(ragged=True, paged=True),
    "softcap": dict(softcap=True), "sinks": dict(sinks=True), "sinks_split": dict(sinks=True, num_splits=3), "prefill": dict(prefill=True),
    "prefill_ragged": dict(prefill=True, ragged=True),
}
NOT_AT_256 = ("sinks", "sinks_split", "prefill", "prefill_ragged")


def _i16(a):
    """int32 bit patterns 0 .. 65535 -> int16"""
    return torch.where(a >= 32768, a - 65536, a).to(torch.int16)


def finite_patterns(dt, below_exp=None):
    """every finite bit pattern of dt as int16 (63488 in fp16, 65280 in bf16); below_exp: only |x| < 2^below_exp"""
    a = torch.arange(65536, dtype=torch.int32)
    em = 0x7C00 if dt == torch.float16 else 0x7F80
    a = a[(a & em) != em]
    p = _i16(a)
    if below_exp is not None:
        p = p[p.view(dt).float().abs() < 2.0 ** below_exp]
    return p


def _spread(pats, b, rows, hk, d, per_sequence, shift=0, cover=True):
    """(b, rows, hk, d) of `pats` (1-D), cycled from `shift`: over the whole tensor, or over every sequence on its own"""
    n = rows * hk * d * (1 if per_sequence else b)
    assert n >= pats.numel() or not cover, "every pattern must appear"
    t = pats[(torch.arange(n) + shift) % pats.numel()].view(-1, rows, hk, d)
    return t.expand(b, -1, -1, -1).contiguous() if per_sequence else t


def _paged(kc, vc, seed=5, P=16):
    """pool + shuffled block table (pages of 16) holding the logical caches (b, cap, hk, d) of either width; unreferenced pages hold NaN"""
    b, cap, hk, d = kc.shape
    cols = cap // P
    nb = b * cols + 2
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))
    table = perm[: b * cols].view(b, cols).to(torch.int32).to(kc.device)
    pools = []
    for c in (kc, vc):
        bits = _bits(c)
        pool = torch.full((nb, P, hk, d), NAN8 if bits.dtype == torch.uint8 else NAN16, dtype=bits.dtype, device=kc.device)
        pool[table.long()] = bits.reshape(b, cols, P, hk, d)
        pools.append(pool.view(c.dtype))
    return pools[0], pools[1], table


def call(path, q, kc, vc, lens, *, kds=None, vds=None, num_splits=None, scale=None, sinks=None, tree=None, causal=None):
    """one call down `path`: q (b, sq, h, d), the LOGICAL caches (b, cap, hk, d), all on the GPU -> out (b, sq, h, d), lse (b, h, sq)"""
    spec = PATHS[path]
    b, sq, h, d = q.shape
    kw = dict(cache_seqlens=torch.tensor(lens, dtype=torch.int32, device=q.device), return_softmax_lse=True,
              causal=spec.get("causal", False) if causal is None else causal, num_splits=spec.get("num_splits", 1) if num_splits is None else num_splits)
    if "window" in spec:
        kw["window_size"] = spec["window"]
    if spec.get("softcap"):
        kw["softcap"] = SOFTCAP
    if spec.get("sinks"):
        kw["sinks"] = torch.full((h,), float("-inf"), device=q.device) if sinks is None else sinks
    if spec.get("prefill"):
        kw["prefill"] = True
    if scale is not None:
        kw["softmax_scale"] = scale
    if kds is not None or vds is not None:
        kw.update(k_descale=kds, v_descale=vds)
    if spec.get("paged"):
        kc, vc, kw["block_table"] = _paged(kc, vc)
    if spec.get("ragged"):
        cu = (torch.arange(b + 1, dtype=torch.int32) * sq).to(q.device)
        if tree is not None:
            kw["tree_mask"] = tree.reshape(-1)
        out, lse = F.flash_attn_with_kvcache(q.reshape(b * sq, h, d), kc, vc, cu_seqlens_q=cu, max_seqlen_q=sq, **kw)
        return out.view(b, sq, h, d), lse.view(h, b, sq).permute(1, 0, 2)
    if tree is not None:
        kw["tree_mask"] = tree
    return F.flash_attn_with_kvcache(q, kc, vc, **kw)


def _fail_summary(fails):
    return f"{len(fails)} failing cases:\n" + "\n".join(fails[:40])


# ---- A. one visible key copies V exactly -----------------------------------------------------------------------------------------------

GEOMS = {"one": dict(sq=1, L=1, cap=96, first=0), "window": dict(sq=16, L=40, cap=48, first=24), "tree": dict(sq=64, L=64, cap=64, first=0)}


def _a_paths(d):
    """(geometry, path) of family A at head_dim d; "rotary" and "tree" are handled by the caller"""
    if d == 256:
        return [("one", "base"), ("one", "causal"), ("one", "paged"), ("window", "window")]
    one = ["base", "causal", "paged", "split", "ragged", "ragged_paged", "softcap", "sinks", "sinks_split", "prefill", "prefill_ragged", "rotary"]
    return [("one", p) for p in one] + [("window", "window"), ("tree", "tree")]


def _copy_mismatch(out, want_bits):
    """None if out has the bits `want_bits` (int16; where the pattern is +-0: a zero of either sign), else a description"""
    got, want = _bits(out).cpu(), want_bits.cpu()
    zero = (want & 0x7FFF) == 0
    ok = torch.where(zero, (got & 0x7FFF) == 0, got == want)
    if ok.all():
        return None
    bad = (~ok).nonzero()
    ex = ", ".join(f"{(got[tuple(i)].item() & 0xFFFF):#06x} for {(want[tuple(i)].item() & 0xFFFF):#06x}" for i in bad[:4])
    return f"{bad.shape[0]} of {ok.numel()} elements differ (got for want: {ex})"


def _single_key_sweep(gpu, dt, d, ratio, hk, b_of, pats, per_sequence, cache_dt, expect, kds_vds=None):
    """family A over every path: V rows made of `pats` (int16 or uint8 bit patterns) where exactly one is visible per query row; expect(seen, i)
    -> the int16 bits out must hold for the visible V elements `seen` (b, sq, hk, d) in cache bits.  Returns the list of failures."""
    fails = []
    h = hk * ratio
    bitdt = pats.dtype
    nan = NAN8 if bitdt == torch.uint8 else NAN16
    gen = torch.Generator().manual_seed(7000 + d + ratio)
    for geom, path in _a_paths(d):
        g = GEOMS[geom]
        sq, L, cap, first = g["sq"], g["L"], g["cap"], g["first"]
        b = b_of(sq)
        seen = _spread(pats, b, sq, hk, d, per_sequence)
        vbits = torch.full((b, cap, hk, d), nan, dtype=bitdt)
        vbits[:, :L] = _spread(pats, b, L, hk, d, True, shift=pats.numel() // 3, cover=False)       # rows other query rows see: other finite patterns
        vbits[:, first:first + sq] = seen
        kf = torch.randn(b, cap, hk, d, generator=gen)
        kc = (kf.to(dt) if cache_dt != F8 else quantise(kf, None)).to(gpu)
        kds, vds = (None, None) if kds_vds is None else (t.to(gpu) for t in kds_vds(b))
        want = expect(seen, vds).repeat_interleave(ratio, dim=2)
        for qkind in ("zero", "randn"):
            q = (torch.zeros(b, sq, h, d) if qkind == "zero" else torch.randn(b, sq, h, d, generator=gen)).to(dt).to(gpu)
            tag = f"{path} q={qkind}"
            if path == "rotary":
                # the row is appended by the call (rotary needs k / v): an empty cache, v_new = the row every query must copy
                if cache_dt == F8:
                    v_new = (seen.view(F8).float() * vds.cpu()[:, None, :, None]).to(dt)
                    codes = quantise(v_new, vds)
                    want_r = expect(codes.view(torch.uint8), vds).repeat_interleave(ratio, dim=2)
                else:
                    v_new, want_r = seen.view(dt), want
                vc = torch.full((b, cap, hk, d), nan, dtype=bitdt).view(cache_dt).to(gpu)
                cos, sin = tables(cap, 16, dt)
                out, lse = F.flash_attn_with_kvcache(q, kc.clone(), vc, k=torch.randn(b, 1, hk, d, generator=gen).to(dt).to(gpu), v=v_new.to(gpu), cache_seqlens=0,
                                                     num_splits=1, return_softmax_lse=True, rotary_cos=cos.to(gpu), rotary_sin=sin.to(gpu), k_descale=kds, v_descale=vds)
                bad = _copy_mismatch(out, want_r)
            else:
                vc = vbits.view(cache_dt).to(gpu)
                tree = None
                if path == "tree":
                    tree = (torch.ones((), dtype=torch.int64) << torch.arange(64, dtype=torch.int64)).expand(b, 64).contiguous().to(gpu)
                out, lse = call("base" if path == "tree" else path, q, kc, vc, [L] * b, kds=kds, vds=vds, tree=tree)
                bad = _copy_mismatch(out, want)
            if bad is not None:
                fails.append(f"{tag}: {bad}")
            if not torch.isfinite(lse).all():
                fails.append(f"{tag}: non-finite LSE")
    return fails


@pytest.mark.parametrize("ratio", [1, 4])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_a_one_visible_key_copies_every_finite_16bit_value_of_v(gpu, dtname, d, ratio):
    """16-bit cache: all finite bit patterns of the dtype as V, every path: out has V's bits (a zero of either sign for +-0)"""
    dt, hk = DT[dtname], 8
    pats = finite_patterns(dt)
    assert pats.numel() == (63488 if dtname == "fp16" else 65280)
    b_of = lambda sq: -(-pats.numel() // (sq * hk * d))
    fails = _single_key_sweep(gpu, dt, d, ratio, hk, b_of, pats, False, dt, lambda seen, vds: seen)
    assert not fails, f"{dtname} d{d} h/hk={ratio}: " + _fail_summary(fails)


@pytest.mark.parametrize("ratio", [1, 4])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_a_one_visible_key_copies_every_finite_e4m3_code_of_v_times_v_descale(gpu, dtname, d, ratio):
    """FP8 cache: the 254 finite codes as V in every sequence, sequence i under v_descale VDS[i]: out is the fp32 product float(code) x
    v_descale rounded once to the dtype, bit for bit (exact for the powers of two); NaN codes past L never show"""
    dt, hk = DT[dtname], 4
    gen = torch.Generator().manual_seed(7100 + d)
    kds_vds = lambda b: (_descale(b, hk, gen, "cpu"), torch.tensor(VDS, dtype=torch.float32)[:, None].expand(b, hk).contiguous())
    expect = lambda seen, vds: _bits((seen.view(F8).float() * vds.cpu()[:, None, :, None]).to(dt))
    # the expectation formula itself: code 0x7e is 448, 0x01 is 2^-9, and a power-of-two descale is exact
    probe = expect(torch.tensor([0x7E, 0x01, 0x08, 0xFE], dtype=torch.uint8).view(1, 1, 1, 4), torch.tensor([[2.0 ** -3]]))
    assert probe.view(dt).float().flatten().tolist() == [56.0, 2.0 ** -12, 2.0 ** -9, -56.0]
    fails = _single_key_sweep(gpu, dt, d, ratio, hk, lambda sq: len(VDS), FINITE8, True, F8, expect, kds_vds)
    assert not fails, f"fp8 {dtname} d{d} h/hk={ratio}: " + _fail_summary(fails)


# ---- B. every e4m3 code on the K side, every 16-bit q ---------------------------------------------------------------------------------------

def _lse_bound(x):
    return 2.0 ** -20 * np.maximum(np.abs(x), 1.0)


def _k_code_case(d):
    """K codes (b 10, cap 16, hk 4, d) with row 0 set, one-hot q (b, 16, 4, d) as float, the code each (b, head, row) reads, and the pairs that hold
    a NaN code.  Pairs 0 .. 15 and 16 .. 31 each read the 254 finite codes (plus two repeats) at different elements, pairs 32 .. 35 hold 0x7f /
    0xff at one element, pairs 36 .. 39 are finite neighbours."""
    b, hk, sq = 10, 4, 16
    fin = torch.cat([FINITE8, FINITE8[:2]])
    k = FINITE8[(torch.arange(b * 16 * hk * d) * 37 + 11) % 254].view(b, 16, hk, d).clone()
    q = torch.zeros(b, sq, hk, d)
    read = torch.zeros(b, hk, sq, dtype=torch.uint8)
    nan_pair = torch.zeros(b, hk, dtype=torch.bool)
    for r in range(b * hk):
        i, g = divmod(r, hk)
        for t in range(sq):
            j = (t * (d // 16) + r) % d
            q[i, t, g, j] = 1.0
            if r < 32:
                src = fin if r < 16 else fin.flip(0)
                k[i, 0, g, j] = src[(r % 16) * 16 + t]
            read[i, g, t] = k[i, 0, g, j]
        if 32 <= r < 36:
            k[i, 0, g, (5 * (d // 16) + r) % d] = 0x7F if r % 2 == 0 else 0xFF
            nan_pair[i, g] = True
    assert set(read[~nan_pair].flatten().tolist()) >= set(FINITE8.tolist())
    return k, q, read, nan_pair


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_b_every_e4m3_code_of_k_reaches_the_lse(gpu, dtname, d):
    dt = DT[dtname]
    k8, q, read, nan_pair = _k_code_case(d)
    b, _, hk, _ = k8.shape
    gen = torch.Generator().manual_seed(7200 + d)
    v8 = quantise(torch.randn(b, 16, hk, d, generator=gen), None).to(gpu)
    kc, qg = k8.view(F8).to(gpu), q.to(dt).to(gpu)
    codes = read.view(F8).double().numpy()
    live = ~nan_pair.numpy()
    fails, worst = [], {}
    paths = ["base", "paged", "ragged", "softcap"] + ([] if d == 256 else ["prefill"])
    for kd in (1.0, 0.37):
        kds = torch.full((b, hk), kd, dtype=torch.float32, device=gpu)
        x = codes * float(np.float32(kd))
        for path in paths:
            out, lse = call(path, qg, kc, v8, [1] * b, kds=kds, vds=None, scale=1.0)
            lse, onan = lse.double().cpu().numpy(), torch.isnan(out).all(-1).permute(0, 2, 1).cpu().numpy()
            want, bound = x, _lse_bound(x)
            if path == "softcap":
                want = SOFTCAP * np.tanh(x / SOFTCAP)
                bound = _lse_bound(want) + SOFTCAP * TANH_ERR
            tag = f"{path} k_descale={kd}"
            if not (np.isnan(lse[~live]).all() and onan[~live].all()):
                fails.append(f"{tag}: a pair with a NaN code must be NaN in O and LSE")
            if not (np.isfinite(lse[live]).all() and torch.isfinite(out).all(-1).permute(0, 2, 1).cpu().numpy()[live].all()):
                fails.append(f"{tag}: non-finite rows beside the NaN codes")
                continue
            ratio = (np.abs(lse - want) / bound)[live]
            worst[tag] = (float(np.abs(lse - want)[live].max()), float(ratio.max()))
            if ratio.max() > 1.0:
                at = np.argwhere((np.abs(lse - want) / bound > 1.0) & live[:, :, None])[0]
                fails.append(f"{tag}: |lse - x| exceeds the bound on {int((ratio > 1).sum())} rows, worst {ratio.max():.2f} x the bound; first at {at.tolist()}: code "
                             f"{int(read[tuple(at)]):#04x} lse {lse[tuple(at)]!r} want {want[tuple(at)]!r}")
    print(f"MARGIN B codes {dtname} d{d}: worst |lse - x| and worst ratio to the bound per path: {worst}")
    assert not fails, f"{dtname} d{d}: " + _fail_summary(fails)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_b_every_finite_16bit_q_reaches_the_lse(gpu, dtname, d):
    """K one-hot at element j, q[j] every finite pattern (bf16: |q| < 2^30, see the docstring): LSE = q[j] within the bound of B; on the rotary path the
    patterns sit in the unrotated tail of q and travel through the q image in the workspace"""
    dt, sq, h = DT[dtname], 16, 8
    pats = finite_patterns(dt, SCORE_LIMIT_EXP if dtname == "bf16" else None)
    b = -(-pats.numel() // (sq * h))
    gen = torch.Generator().manual_seed(7300 + d)
    vals = _spread(pats, b, sq, h, 1, False).view(dt)                                      # (b, sq, h, 1)
    x = vals.double().squeeze(-1).permute(0, 2, 1).numpy()                                 # (b, h, sq)
    fails, worst = [], {}
    for path in ["base", "rotary"] + ([] if d == 256 else ["prefill"]):
        i, g = torch.meshgrid(torch.arange(b), torch.arange(h), indexing="ij")
        j = (7 * i + 5 * g) % d if path != "rotary" else 16 + (7 * i + 5 * g) % (d - 16)
        q = torch.randn(b, sq, h, d, generator=gen).to(dt)
        q.scatter_(3, j[:, None, :, None].expand(b, sq, h, 1), vals)
        krow = torch.zeros(b, 1, h, d, dtype=dt).scatter_(3, j[:, None, :, None], torch.ones(b, 1, h, 1, dtype=dt))
        kc, vc = torch.zeros(b, 16, h, d, dtype=dt, device=gpu), torch.zeros(b, 16, h, d, dtype=dt, device=gpu)
        if path == "rotary":
            cos, sin = tables(16, 16, dt)
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), kc, vc, k=krow.to(gpu), v=torch.zeros(b, 1, h, d, dtype=dt, device=gpu), cache_seqlens=0, num_splits=1,
                                                 return_softmax_lse=True, softmax_scale=1.0, rotary_cos=cos.to(gpu), rotary_sin=sin.to(gpu))
        else:
            kc[:, :1] = krow.to(gpu)
            out, lse = call(path, q.to(gpu), kc, vc, [1] * b, scale=1.0)
        lse = lse.double().cpu().numpy()
        if not np.isfinite(lse).all():
            fails.append(f"{path}: {int((~np.isfinite(lse)).sum())} non-finite LSE entries, first for q = {x[~np.isfinite(lse)][0]!r}")
            continue
        ratio = np.abs(lse - x) / _lse_bound(x)
        worst[path] = (float(np.abs(lse - x).max()), float(ratio.max()))
        if ratio.max() > 1.0:
            at = tuple(np.argwhere(ratio > 1.0)[0])
            fails.append(f"{path}: |lse - q[j]| exceeds the bound on {int((ratio > 1).sum())} rows, worst {ratio.max():.2f} x the bound; first: q {x[at]!r} lse {lse[at]!r}")
    print(f"MARGIN B q {dtname} d{d}: worst |lse - x| and worst ratio to the bound per path: {worst}")
    assert not fails, f"{dtname} d{d}: " + _fail_summary(fails)


# ---- C. every 16-bit input through every append kernel ----------------------------------------------------------------------------------------

C_LENS = [5, 0, 30, 9, 17]


def _append_case(dt, d, rotary, gen):
    """k_new, v_new (b 5, sn, hk 2, d) holding all 65536 patterns per (sequence, head) in two different orders (rotary: K's patterns in elements 16 ..
    d - 1, finite values in the rotated head)"""
    b, hk = len(C_LENS), 2
    allp = _i16(torch.arange(65536, dtype=torch.int32))
    width = d - 16 if rotary else d
    sn = -(-65536 // width)
    per_head = lambda pats, w, shift: torch.stack([torch.stack([pats[(torch.arange(sn * w) + shift * (1 + g + hk * i)) % 65536].view(sn, w) for g in range(hk)], 1)
                                                   for i in range(b)])
    k_new = torch.randn(b, sn, hk, d, generator=gen).to(dt)
    _bits(k_new)[..., d - width:] = per_head(allp, width, 4099)
    v_new = per_head(allp.flip(0), d, 12345).view(dt)
    for t in (k_new, v_new):
        assert all(torch.unique(_bits(t)[i, :, g, d - width if t is k_new else 0:]).numel() == 65536 for i in range(b) for g in range(hk))
    return k_new, v_new, sn


def _expected_after_append(cache, rows, lens):
    e = cache.clone()
    for i, L in enumerate(lens):
        _bits(e)[i, L:L + rows.shape[1]] = _bits(rows)[i]
    return e


def _bytes_mismatch(got, want, what):
    g, w = _bits(got).cpu(), _bits(want).cpu()
    if torch.equal(g, w):
        return None
    bad = (g != w).nonzero()
    mask = (1 << (8 * g.element_size())) - 1
    ex = ", ".join(f"{i.tolist()}: {(g[tuple(i)].item() & mask):#x} for {(w[tuple(i)].item() & mask):#x}" for i in bad[:4])
    return f"{what}: {bad.shape[0]} elements differ ({ex})"


@pytest.mark.parametrize("variant", ["contiguous", "paged", "ragged", "ragged_paged", "rotary"])
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_c_every_16bit_input_through_the_append(gpu, dtname, d, fp8, variant):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(7400 + d)
    rotary, paged, ragged = variant == "rotary", variant.endswith("paged"), variant.startswith("ragged")
    k_new, v_new, sn = _append_case(dt, d, rotary, gen)
    b, hk, h = len(C_LENS), 2, 4
    cap = (max(C_LENS) + sn + 15) // 16 * 16 + 16
    ds = torch.tensor(APPEND_DESCALES, dtype=torch.float32).view(b, hk)
    kds, vds = (ds, ds.flatten().roll(3).view(b, hk).contiguous()) if fp8 else (None, None)
    init = torch.randn(b, cap, hk, d, generator=gen)
    k0, v0 = (quantise(init, None), quantise(init * 0.5, None)) if fp8 else (init.to(dt), (init * 0.5).to(dt))
    k_rows = k_new
    kw = {}
    if rotary:
        cos, sin = tables(cap, 16, dt)
        k_rows = rotate_ref(k_new, cos, sin, positions(C_LENS, sn, True, cap), True)
        assert torch.equal(_bits(k_rows)[..., 16:], _bits(k_new)[..., 16:])
        kw.update(rotary_cos=cos.to(gpu), rotary_sin=sin.to(gpu), rotary_interleaved=True)
    k_exp = _expected_after_append(k0, quantise(k_rows, kds) if fp8 else k_rows, C_LENS)
    v_exp = _expected_after_append(v0, quantise(v_new, vds) if fp8 else v_new, C_LENS)
    if fp8:
        # NaN inputs become 0x7f / 0xff by sign, +-inf saturate: the reference formula does what the contract says
        kq = _bits(quantise(k_rows, kds))
        src = k_rows.float()
        assert torch.equal(kq[torch.isnan(src)] & 0x7F, torch.full_like(kq[torch.isnan(src)], NAN8)) and set(kq[torch.isinf(src)].tolist()) == {0x7E, 0xFE}
        assert torch.equal(kq[torch.isnan(src)] >> 7, (_bits(k_rows)[torch.isnan(src)] < 0).to(torch.uint8))
        kw.update(k_descale=kds.to(gpu), v_descale=vds.to(gpu))
    kc, vc = k0.to(gpu), v0.to(gpu)
    if paged:
        kc, vc, kw["block_table"] = _paged(kc, vc)
    cs = torch.tensor(C_LENS, dtype=torch.int32, device=gpu)
    q = torch.randn(b, 1, h, d, generator=gen).to(dt).to(gpu)
    if ragged:
        cu_q = torch.arange(b + 1, dtype=torch.int32, device=gpu)
        cu_k = (torch.arange(b + 1, dtype=torch.int32) * sn).to(gpu)
        F.flash_attn_with_kvcache(q.view(b, h, d), kc, vc, k=k_new.reshape(b * sn, hk, d).to(gpu), v=v_new.reshape(b * sn, hk, d).to(gpu), cache_seqlens=cs,
                                  cu_seqlens_q=cu_q, max_seqlen_q=1, cu_seqlens_k_new=cu_k, **kw)
    else:
        F.flash_attn_with_kvcache(q, kc, vc, k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=cs, **kw)
    torch.cuda.synchronize()
    if paged:
        k_exp, v_exp, _ = _paged(k_exp.to(gpu), v_exp.to(gpu))
    fails = [m for m in (_bytes_mismatch(kc, k_exp, "k_cache"), _bytes_mismatch(vc, v_exp, "v_cache")) if m]
    assert not fails, f"{variant} {'fp8' if fp8 else '16-bit'} {dtname} d{d}: " + "; ".join(fails)
    assert cs.tolist() == C_LENS


# ---- D. V across its range against the oracle (fp16) ----------------------------------------------------------------------------------------

D_LENS, D_CAP, D_SQ, D_H, D_HK = [1, 2, 31, 33, 100, 777], 784, 3, 8, 2
_D_REF = {}


def _d_problem(d, e, fp8, dt=torch.float16):
    """q, the logical caches as they go to the kernels, the descales, and the fp32 caches the expectation is computed on"""
    gen = torch.Generator().manual_seed(7500 + d + (1000 if fp8 else 0))
    b = len(D_LENS)
    q = torch.randn(b, D_SQ, D_H, d, generator=gen).to(dt)
    kf, vf = torch.randn(b, D_CAP, D_HK, d, generator=gen), torch.randn(b, D_CAP, D_HK, d, generator=gen)
    if not fp8:
        k, v = kf.to(dt), (vf * 2.0 ** e).to(dt)
        return q, k, v, None, None, k.float(), v.float()
    kds, vds0 = _descale(b, D_HK, gen, "cpu"), _descale(b, D_HK, gen, "cpu")
    k8, v8 = quantise(kf, kds), quantise(vf, vds0)
    vds = vds0 * 2.0 ** e
    return q, k8, v8, kds, vds, deq(k8, kds), deq(v8, vds)


def _d_reference(key, q, k, v, window):
    """per live (sequence, row): the C oracle (ROUND_FP16) on the row's visible slice and float64 math; computed once per problem and visibility"""
    if key not in _D_REF:
        qn, kn, vn = (t.float().numpy() for t in (q, k, v))
        rows, qs, ks, vs, cu = [], [], [], [], [0]
        for i, L in enumerate(D_LENS):
            for t in range(D_SQ):
                lo, hi = _bounds(L, D_SQ, t, window, True)
                if hi > lo:
                    rows.append((i, t))
                    qs.append(qn[i, t]), ks.append(kn[i, lo:hi]), vs.append(vn[i, lo:hi])
                    cu.append(cu[-1] + hi - lo)
        o_ref, lse_ref = A.attn_fwd(np.stack(qs), np.concatenate(ks), np.concatenate(vs), causal=False, round_mode=A.ROUND_FP16,
                                    cu_seqlens_q=np.arange(len(rows) + 1, dtype=np.int32), cu_seqlens_k=np.asarray(cu, dtype=np.int32), max_seqlen_q=1,
                                    max_seqlen_k=int(np.diff(cu).max()))
        xo, _ = window_exact(q, k, v, D_LENS, window, True)
        assert np.isfinite(o_ref).all() and np.isfinite(lse_ref).all(), "the oracle itself must stay finite"
        _D_REF[key] = (rows, o_ref, lse_ref[:, :, 0], xo.numpy())
    return _D_REF[key]


def _d_check(out, lse, ref, e, tag):
    rows, o_ref, lse_ref, xo = ref
    assert torch.isfinite(out.float()).all().item() and torch.isfinite(lse).all().item(), f"{tag}: non-finite values"
    got, got_lse = out.double().cpu().numpy(), lse.cpu().numpy()
    live = np.zeros(got.shape[:2], dtype=bool)
    f = 2.0 ** -e
    worst = dict(max_abs=0.0, mean_abs=0.0, mean_rel=0.0, lse=0.0)
    for i, L in enumerate(D_LENS):
        idx = [n for n, (bi, _) in enumerate(rows) if bi == i]
        ts = [rows[n][1] for n in idx]
        live[i, ts] = True
        orc = o_ref[idx].astype(np.float64) * f
        raw = U.assert_close(got[i, ts] * f, orc, "fp16", f"kvcache O {tag} b{i} L{L}", sk=L, oracle=orc, exact=xo[i, ts] * f)
        for m in raw:
            worst[m] = max(worst[m], raw[m])
        err = float(np.abs(got_lse[i][:, ts].T - lse_ref[idx]).max())
        worst["lse"] = max(worst["lse"], err)
        assert err <= U.LSE_TOL, f"{tag}: LSE b{i} L{L} err {err}"
    assert (got[~live] == 0).all() and (got_lse.transpose(0, 2, 1)[~live] == 0).all(), f"{tag}: rows that see no key must be O = 0, LSE = 0"
    print(f"MARGIN D {tag}: worst raw metrics after rescaling {worst}")


@pytest.mark.parametrize("e", [-14, 12])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("path", ["causal", "paged", "window40", "split", "ragged", "prefill"])
def test_d_fp16_v_across_its_range_follows_the_oracle(gpu, path, d, e):
    q, k, v, _, _, kx, vx = _d_problem(d, e, False)
    if e == -14:
        share = (v.float().abs() < 2.0 ** -14).float().mean().item()
        assert 0.55 <= share <= 0.8, f"about two thirds of V must be subnormal, got {share:.2f}"
    window = PATHS[path].get("window", (-1, -1))
    ref = _d_reference(("16", d, e, window), q, kx, vx, window)
    out, lse = call(path, q.to(gpu), k.to(gpu), v.to(gpu), D_LENS, causal=True)
    _d_check(out, lse, ref, e, f"V x 2^{e} {path} fp16 d{d}")


@pytest.mark.parametrize("e", [-14, 12])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("path", ["causal", "paged", "prefill"])
def test_d_fp8_v_descale_across_its_range_follows_the_oracle(gpu, path, d, e):
    q, k8, v8, kds, vds, kx, vx = _d_problem(d, e, True)
    ref = _d_reference(("8", d, e), q, kx, vx, (-1, -1))
    out, lse = call(path, q.to(gpu), k8.to(gpu), v8.to(gpu), D_LENS, kds=kds.to(gpu), vds=vds.to(gpu), causal=True)
    _d_check(out, lse, ref, e, f"v_descale x 2^{e} {path} fp8 fp16 d{d}")


# ---- E. exact power-of-two relations ---------------------------------------------------------------------------------------------------------

def _e_paths(d, softcap=False, sinks=False):
    if d == 256:
        return ["causal", "paged", "window40"]
    return ["causal", "paged", "window40", "ragged", "prefill"] + (["softcap"] if softcap else []) + (["sinks", "sinks_split"] if sinks else [])


def _scaled_out_mismatch(unit, got, f):
    """None if out is the unit-scale out x f and lse keeps its bits"""
    (o1, l1), (o2, l2) = unit, got
    if not torch.equal(_bits(l1.contiguous()), _bits(l2.contiguous())):
        return f"lse changed ({int((l1 != l2).sum())} entries)"
    want = o1.float() * f
    if not torch.equal(o2.float(), want):
        bad = o2.float() != want
        return f"out is not the unit-scale out x {f}: {int(bad.sum())} of {bad.numel()} elements"
    return None


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("fp8", [False, True])
def test_e_bf16_scaling_v_or_v_descale_by_a_power_of_two_scales_out_exactly(gpu, fp8, d):
    """bf16 keeps fp32's exponent range: V x 2^e (16-bit cache) or v_descale x 2^e (FP8 cache) scales out by exactly 2^e and leaves lse"""
    dt = torch.bfloat16
    q, k, v, kds, vds, _, _ = _d_problem(d, 0, fp8, dt)
    qg, kg, vg = q.to(gpu), k.to(gpu), v.to(gpu)
    dsk = dict(kds=kds.to(gpu)) if fp8 else {}
    fails = []
    for path in _e_paths(d):
        for ns in (1, 3):
            unit = call(path, qg, kg, vg, D_LENS, causal=True, num_splits=ns, vds=vds.to(gpu) if fp8 else None, **dsk)
            for e in (-24, -8, 8, 24):
                if fp8:
                    got = call(path, qg, kg, vg, D_LENS, causal=True, num_splits=ns, vds=(vds * 2.0 ** e).to(gpu), **dsk)
                else:
                    vs = (v.float() * 2.0 ** e).to(dt)
                    assert torch.equal(vs.float(), v.float() * 2.0 ** e)
                    got = call(path, qg, kg, vs.to(gpu), D_LENS, causal=True, num_splits=ns)
                bad = _scaled_out_mismatch(unit, got, 2.0 ** e)
                if bad:
                    fails.append(f"{path} num_splits={ns} e={e}: {bad}")
    assert not fails, f"{'v_descale' if fp8 else 'V'} bf16 d{d}: " + _fail_summary(fails)


def _same_bits_mismatch(a, b):
    bad = [n for n, x, y in (("out", a[0], b[0]), ("lse", a[1], b[1])) if not torch.equal(_bits(x.contiguous()), _bits(y.contiguous()))]
    return f"{' and '.join(bad)} changed" if bad else None


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_e_a_power_of_two_moves_between_k_descale_and_softmax_scale(gpu, dtname, d):
    """FP8 cache: k_descale x 2^e with softmax_scale x 2^-e changes no bit of out or lse - with finite sinks too, which are in units of the final scores"""
    dt = DT[dtname]
    q, k8, v8, kds, vds, _, _ = _d_problem(d, 0, True, dt)
    qg, kg, vg, vdg = q.to(gpu), k8.to(gpu), v8.to(gpu), vds.to(gpu)
    sinks = torch.linspace(-2.0, 2.0, D_H).to(gpu)
    scale = 1.0 / math.sqrt(d)
    fails = []
    for path in _e_paths(d, softcap=True, sinks=True):
        for ns in (1, 3):
            kw = dict(causal=True, num_splits=ns, vds=vdg, sinks=sinks if path.startswith("sinks") else None)
            unit = call(path, qg, kg, vg, D_LENS, kds=kds.to(gpu), scale=scale, **kw)
            for e in (-8, -3, 3, 8):
                got = call(path, qg, kg, vg, D_LENS, kds=(kds * 2.0 ** e).to(gpu), scale=scale * 2.0 ** -e, **kw)
                bad = _same_bits_mismatch(unit, got)
                if bad:
                    fails.append(f"{path} num_splits={ns} e={e}: {bad}")
    assert not fails, f"k_descale / softmax_scale {dtname} d{d}: " + _fail_summary(fails)


@pytest.mark.parametrize("d", [64, 128, 256])
@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
def test_e_a_power_of_two_moves_between_q_and_k_descale(gpu, dtname, d):
    """FP8 cache: q x 2^e with k_descale x 2^-e changes no bit of out or lse (|q| below 2^-6 lifted to 2^-6 first: the scaling is exact in fp16)"""
    dt = DT[dtname]
    q, k8, v8, kds, vds, _, _ = _d_problem(d, 0, True, dt)
    qf = q.float()
    q = torch.where(qf.abs() < 2.0 ** -6, torch.where(qf < 0, -torch.ones_like(qf), torch.ones_like(qf)) * 2.0 ** -6, qf).to(dt)
    kg, vg, vdg = k8.to(gpu), v8.to(gpu), vds.to(gpu)
    fails = []
    for path in _e_paths(d, softcap=True):
        for ns in (1, 3):
            unit = call(path, q.to(gpu), kg, vg, D_LENS, kds=kds.to(gpu), vds=vdg, causal=True, num_splits=ns)
            for e in (-3, 3):
                qs = (q.float() * 2.0 ** e).to(dt)
                assert torch.equal(qs.float(), q.float() * 2.0 ** e), "the scaled q must be exact"
                got = call(path, qs.to(gpu), kg, vg, D_LENS, kds=(kds * 2.0 ** -e).to(gpu), vds=vdg, causal=True, num_splits=ns)
                bad = _same_bits_mismatch(unit, got)
                if bad:
                    fails.append(f"{path} num_splits={ns} e={e}: {bad}")
    assert not fails, f"q / k_descale {dtname} d{d}: " + _fail_summary(fails)
