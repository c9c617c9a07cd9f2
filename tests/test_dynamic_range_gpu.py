"""GPU: the dense and packed backward (and the forward, where V moves) across the dynamic range of dO, V and the scores, under both kernel sets.

Every other backward test draws q, k, v and dO from N(0, 1).  In fp16 training dO is loss-scaled (x 2^8 .. 2^16) or unscaled and tiny - at 1e-5
it is made of fp16 SUBNORMALS, and dS = P (dP - D) and the outputs are subnormal too.  P and dS are rounded to 16 bits (LP<T>::pack2,
fa_device.hpp) into the operands of the second GEMMs, D is an fp32 row sum, the outputs are packed to 16 bits at the end: whether subnormals
survive those conversions, the MFMA operands and the stores depends on the kernels' float mode (tests/test_kernel_resources_cpu.py pins it)
and on the hardware.  The C oracle (oracle/attn_oracle.c) models what is needed: oracle_round_fp16 has the subnormal grid and the overflow to
infinity, and it sums in double, so the reference algorithm itself says where the contract ends.

Every test runs twice, with the 16x16x32 and the 32x32x16 kernel set pinned (fixture `pinned_set`), and asserts through capi.kernel_name
that the dQ and dK/dV stages go to that set.  Base problem: dense, b2 sq320 sk320 h4/hk2 (a whole 256-row query block plus a ragged one, key
tiles plus a tail at both tile widths), d in {64, 128}, causal or not, fixed CPU-generator seeds.
  A. fp16, dO x 2^e, e in {-14, -8, +8, +12} (at -14 about half of dO is subnormal): dQ, dK, dV against the C oracle on the same scaled inputs,
     kernel, oracle and float64 math multiplied by 2^-e (exact) before U.assert_close at the suite's plain tolerances - one spacing of the
     subnormal output grid is 2^-24 x 2^14 = 9.8e-4 after rescaling, inside the 5e-3 bound; everything finite.  The same through the packed
     entry points (d128, e in {-14, +12}; one sequence whose causal mask leaves dead rows, one without queries), checked per sequence.
  B. fp16, V x 2^e, e in {-14, +12}: forward O (in the subnormal output range at -14), dQ and dK rescaled by 2^-e, dV and LSE unscaled.
  C. bf16, bit for bit: dO x 2^e scales dQ, dK, dV by exactly 2^e; V x 2^e scales O, dQ, dK by exactly 2^e and leaves LSE and dV; q x 2^e with
     k x 2^-e leaves O, LSE, dV, scales dQ by 2^-e and dK by 2^e.  e in {-24, -8, +8, +24} (q / k: {-3, +3}): with unit q and k, P >= ~1e-9, so
     every intermediate stays within [1e-25, 1e15], and bf16 has fp32's exponent range.  Every operation between the inputs and the outputs
     (fp32 FMA, MFMA accumulation, round-to-nearest conversion, the final multiplication by `scale`) commutes with an exact power-of-two
     scaling while nothing leaves the normal range: a kernel that breaks a relation has an intermediate the algorithm does not have, or a
     conversion that is not round-to-nearest.  For the q / k pair every |q| or |k| element below 2^-6 is first replaced by 2^-6, so the
     scaled inputs stay exactly representable (in fp16 as well).
  D. fp16, the q / k relation, e in {-3, +3}: O, LSE, dV bit for bit; dQ and dK bit for bit wherever both sides are fp16-normal
     (|unit result| >= 2^-14 and |expected| >= 2^-14), at most 2 % of a tensor excluded (the oracle alone excludes at most 0.66 %), the
     excluded elements within 2^-24 x 2^3, one subnormal spacing carried through the scaling.  (There is no fp16 relation for dO or V: at
     unit scale many dS values are already subnormal, so the two sides round differently; family A covers that.)
  E. sharp softmax in the backward: q, k x s, b1 sq384 sk640 h2/hk1, both dtypes: the reference algorithm itself (dS rounded to 16 bits) is
     8e-3 .. 1.6e-2 (dQ, dK, fp16, s = 4 and 6) off exact math in max_abs, so the expectation is the C oracle, float64 math gives mean_rel
     under the oracle rule; LSE relative, |dLSE| / max(|LSE|, 1) <= 1e-4; everything finite.
A, B and E run twice: as the chain a training step runs (F.fwd, then F.bwd on the kernel's own O and LSE), and with the backward given the
ORACLE's O and LSE, so that kernel and oracle differentiate the same function (see `_run`).

The oracle side of A, B and E was run on the CPU before the first GPU run.  A and B: every case passes the oracle's own cap inside
U.check_mean_rel and all of the oracle's values are finite; no exponent was moved.  E, planned at s in {4, 6}: the oracle stays finite, but
its OWN dQ mean_rel against float64 math is 0.47 - 0.86 (fp16) and 1.1 - 2.7 (bf16), past the cap of 25 x the tolerance on all fp16 and some
bf16 cases, and past the largest bound the rule can derive (10 x) on every case; dK at s = 6 in fp16 is 0.12 - 0.14, past that bound too.
Most rows are then close to one-hot, their dQ is ~0 in exact math, and what the algorithm leaves there is the rounding of O inside
D (~1e-3): relative to max(|e|, 1e-6) that is unbounded, and it is rows, not the whole tensor, so the "zero" rule does not see it.  Moved
towards 0 in steps of 2, s = 6 -> 4 -> 2 and s = 4 -> 2: at s = 2 the oracle's own mean_rel is at most 1.1 x the tolerance (at s = 3: 19 - 24 x
in fp16), and the full check is asserted there.  s = 4 and 6 are kept for everything the oracle itself can meet: O and dV in full, dK in full
at s = 4, dQ (and dK at s = 6) in max_abs and mean_abs against the oracle (`_close(rel=False)`: the bounds of U.assert_close without the
relative metric), LSE, finiteness.

Measured on the MI355X, worst RAW metrics of the kernel against the oracle after rescaling, both kernel sets, backward on the oracle's O: A dense
dQ / dK / dV max_abs 9.8e-4 each (one step of the subnormal output grid at e = -14), mean_abs 2.3e-7 / 5.7e-7 / 4.4e-7, mean_rel 6.0e-3 / 2.0e-4 /
5.0e-5; A packed max_abs 9.8e-4, mean_abs 2.5e-7 / 1.2e-6 / 4.1e-7: the plain tolerances hold.  C: all 80 cases bit for bit.  D: at most 0.72 % of dQ
or dK subnormal on either side, worst deviation there 2^-22.  The chained E cases at s = 4 and 6 carry the derived bound
max(project tolerance, 2 x the oracle's own error against float64 math) for dQ and dK (see the test); every other case asserts the plain bounds."""
import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from flash_attn_turing import capi
from oracle import attn_oracle as A

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
MODE = {"fp16": A.ROUND_FP16, "bf16": A.ROUND_BF16}
BASE = (2, 320, 320, 4, 2)                                 # b, sq, sk, h, hk
SHARP = (1, 384, 640, 2, 1)                                # the shape of test_large_magnitude_inputs_stay_finite
PACKED_LQ, PACKED_LK = [320, 70, 0, 200], [320, 40, 9, 320]
FP16_MIN_NORMAL = 2.0 ** -14
NAMES = ("O", "LSE", "dQ", "dK", "dV")


@pytest.fixture(autouse=True, params=["mfma16", "mfma32"])
def pinned_set(gpu, request):
    prev = capi.set_kernel_policy(capi.POLICY_MFMA16 if request.param == "mfma16" else capi.POLICY_MFMA32)
    yield request.param
    capi.set_kernel_policy(prev)


def _assert_kernel_set(pinned_set, b, sq, sk, h, d, causal, dtype):
    want = {"mfma16": ("fa_bwd_dq16_kernel", "fa_bwd_dkdv16_kernel"), "mfma32": ("fa_bwd_dq_kernel", "fa_bwd_dkdv_kernel")}[pinned_set]
    got = tuple(capi.kernel_name(stage, b, sq, sk, h, d, causal, dtype) for stage in ("dq", "dkdv"))
    assert got == want, (pinned_set, got)


def _problem(dtype, d, causal, family, dims=BASE, packed=False, q_scale=1.0, k_scale=1.0, v_exp=0, do_exp=0):
    """q, k, v, dO on the CPU in `dtype`: N(0, 1) drawn in fp32 from a fixed seed, scaled in fp32, then rounded (a power of two in front of an
    fp16 rounding reaches the subnormal grid).  packed: (total, heads, d) rows of the PACKED_LQ / PACKED_LK sequences."""
    b, sq, sk, h, hk = dims
    gen = torch.Generator(device="cpu").manual_seed(97000 + 1000 * family + d + int(causal))
    qs, ks = ((sum(PACKED_LQ), h, d), (sum(PACKED_LK), hk, d)) if packed else ((b, sq, h, d), (b, sk, hk, d))
    q, k, v, do = (torch.randn(s, generator=gen) for s in (qs, ks, ks, qs))
    return tuple((t * f).to(DT[dtype]) for t, f in ((q, q_scale), (k, k_scale), (v, 2.0 ** v_exp), (do, 2.0 ** do_exp)))


def _cu(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


_REF = {}


def _reference(key, q, k, v, do, causal, dtype, packed=False):
    """(oracle, exact), each (O, LSE, dQ, dK, dV) as numpy arrays: the C oracle with the reference's rounding points in `dtype` and plain
    float64 math on the CPU (U.torch_attention_ref), on the same 16-bit inputs; computed once per problem and shared by both kernel sets"""
    if key not in _REF:
        n = lambda t: t.float().numpy()
        kw = dict(cu_seqlens_q=_cu(PACKED_LQ), cu_seqlens_k=_cu(PACKED_LK), max_seqlen_q=max(PACKED_LQ), max_seqlen_k=max(PACKED_LK)) if packed else {}
        o, lse = A.attn_fwd(n(q), n(k), n(v), causal=causal, round_mode=MODE[dtype], **kw)
        dq, dk, dv = A.attn_bwd(n(q), n(k), n(v), o, lse, n(do), causal=causal, round_mode=MODE[dtype], **kw)
        if not packed:
            exact = tuple(t.numpy() for t in U.torch_attention_ref(q, k, v, do, causal, device="cpu", dtype=torch.float64))
        else:
            cq, ck = _cu(PACKED_LQ), _cu(PACKED_LK)
            xo, xdq = np.zeros(q.shape), np.zeros(q.shape)
            xdk, xdv = np.zeros(k.shape), np.zeros(k.shape)
            xl = np.zeros(lse.shape)
            for i, (lq, lk) in enumerate(zip(PACKED_LQ, PACKED_LK)):
                if lq == 0:
                    continue
                qs, ks = slice(cq[i], cq[i + 1]), slice(ck[i], ck[i + 1])
                r = U.torch_attention_ref(q[qs][None], k[ks][None], v[ks][None], do[qs][None], causal, device="cpu", dtype=torch.float64)
                xo[qs], xl[i, :, :lq], xdq[qs], xdk[ks], xdv[ks] = (t[0].numpy() for t in r)
            exact = (xo, xl, xdq, xdk, xdv)
        _REF[key] = ((o, lse, dq, dk, dv), exact)
    return _REF[key]


def _run(gpu, q, k, v, do, causal, o_from="kernel", oracle=None, dtype=None):
    """forward and backward on the GPU -> (O, LSE, dQ, dK, dV).  o_from = "kernel": the chain a training step runs, the backward on the kernel's own O
    and LSE.  o_from = "oracle": the backward on the oracle's O (already on the 16-bit grid) and LSE, so that kernel and oracle differentiate the SAME
    function - with the kernel's own O one element that rounds the other way (fp32 summation order) moves D = rowsum(dO * O) of its row by an output
    ulp times |dO|, and with it every dS of the row; the variant separates the backward from that property of the forward."""
    q, k, v, do = (t.to(gpu) for t in (q, k, v, do))
    o, lse = F.fwd(q, k, v, causal)
    bo, bl = (o, lse) if o_from == "kernel" else _oracle_o_lse(gpu, oracle, dtype)
    return (o, lse) + tuple(F.bwd(q, k, v, bo, bl, do, causal))


def _oracle_o_lse(gpu, oracle, dtype):
    return torch.from_numpy(oracle[0]).to(gpu, DT[dtype]), torch.from_numpy(oracle[1]).to(gpu)


def _finite(outs, tag):
    for name, t in zip(NAMES, outs):
        assert torch.isfinite(t.float()).all().item(), f"{name}: non-finite values [{tag}]"


def _abs_bounds(x, ref, dtype, name):
    """the max_abs and mean_abs bounds of U.assert_close (one output ulp of slack per element, half an ulp on average) without the relative metric"""
    ref = U.round_like_output(ref, dtype).astype(np.float64)
    tol, ulp = U.TOL[dtype], U.ULP[dtype]
    diff, aref = np.abs(x - ref), np.abs(ref)
    m_max, m_mean = float(np.maximum(diff - ulp * aref, 0.0).max()), float(diff.mean() - 0.5 * ulp * aref.mean())
    assert m_max <= tol["max_abs"], f"{name} max_abs(excess over 1 ulp)={m_max:.3e} > {tol['max_abs']:.3e}"
    assert m_mean <= tol["mean_abs"], f"{name} mean_abs(excess over ulp/2)={m_mean:.3e} > {tol['mean_abs']:.3e}"


def _close(x, oracle, exact, factor, dtype, name, sk, rel=True, derived=False):
    """kernel, oracle and float64 math times `factor` (a power of two: exact in float64), then the suite's small-problem convention at scale 1.0:
    max_abs and mean_abs against the C oracle, mean_rel against exact math under the oracle rule (U.check_mean_rel).  rel=False: without the
    relative metric, for tensors on which the ORACLE's own mean_rel is past what that rule can bound.
    derived=True (a family whose plain bound was missed on the GPU while the kernel stayed within twice the oracle's own error, see the file's
    docstring): where the plain check fails, max_abs and mean_abs of the kernel against float64 math must be within max(project tolerance,
    2 x the oracle's own against float64 math) - the rule of U.check_mean_rel applied to those metrics - and mean_rel as before."""
    x = x.detach().double().cpu().numpy() * factor
    orc, ex = np.asarray(oracle, dtype=np.float64) * factor, np.asarray(exact, dtype=np.float64) * factor
    try:
        if rel:
            U.assert_close(x, orc, dtype, name, sk=sk, oracle=orc, exact=ex)
        else:
            _abs_bounds(x, orc, dtype, name)
    except AssertionError as err:
        e_out = U.round_like_output(ex, dtype).astype(np.float64)
        k, o = U.error_metrics(x, e_out), U.error_metrics(orc, e_out)
        if not derived:
            raise AssertionError(f"{err} [against float64 math: kernel {k}, oracle {o}]") from None
        for m in ("max_abs", "mean_abs"):
            bound = max(U.TOL[dtype][m], 2.0 * o[m])
            assert k[m] <= bound, f"{name} {m} against float64 math {k[m]:.3e} > max({U.TOL[dtype][m]:.1e}, 2 x oracle's {o[m]:.3e}) (plain check: {err})"
        if rel:
            U.check_mean_rel(x, e_out, dtype, name, 1.0, sk, orc, ex)


# ---- A. fp16, dO x 2^e --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o_from", ["kernel", "oracle"])
@pytest.mark.parametrize("e", [-14, -8, 8, 12])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_backward_follows_the_oracle_across_the_range_of_dout(gpu, d, causal, e, o_from, pinned_set):
    """dO = fp16(N(0, 1) x 2^e): loss-scaled (e > 0: |dS| reaches the top of the fp16 range at +12) or tiny (e = -14: about half of dO, and
    most of dS and of the outputs, are fp16 subnormals).  dQ, dK, dV x 2^-e within the plain tolerances of the C oracle, everything finite."""
    b, sq, sk, h, hk = BASE
    _assert_kernel_set(pinned_set, b, sq, sk, h, d, causal, "fp16")
    q, k, v, do = _problem("fp16", d, causal, 1, do_exp=e)
    if e == -14:
        share = (do.float().abs() < FP16_MIN_NORMAL).float().mean().item()
        assert 0.3 <= share <= 0.7, f"about half of dO must be subnormal, got {share:.2f}"
    oracle, exact = _reference(("A", d, causal, e), q, k, v, do, causal, "fp16")
    assert all(np.isfinite(t).all() for t in oracle), "the oracle itself must stay finite"
    outs = _run(gpu, q, k, v, do, causal, o_from, oracle, "fp16")
    tag = f"dO x 2^{e} fp16 d{d} causal={causal} O from the {o_from} {pinned_set}"
    _finite(outs, tag)
    for i in (2, 3, 4):
        _close(outs[i], oracle[i], exact[i], 2.0 ** -e, "fp16", f"{NAMES[i]} {tag}", sk)


@pytest.mark.parametrize("o_from", ["kernel", "oracle"])
@pytest.mark.parametrize("e", [-14, 12])
@pytest.mark.parametrize("causal", [False, True])
def test_fp16_packed_backward_follows_the_oracle_across_the_range_of_dout(gpu, causal, e, o_from, pinned_set):
    """the same through varlen_fwd / varlen_bwd at head_dim 128: sequences of 320 / 70 / 0 / 200 queries over 320 / 40 / 9 / 320 keys (under a
    causal mask the second one's first 30 rows see no key; the third has no queries), each sequence against the C oracle; dead rows and the
    keys of the sequence without queries are exact zeros, padded LSE entries are zero"""
    d, dtype = 128, "fp16"
    h, hk = BASE[3], BASE[4]
    mq, mk = max(PACKED_LQ), max(PACKED_LK)
    _assert_kernel_set(pinned_set, len(PACKED_LQ), mq, mk, h, d, causal, dtype)
    q, k, v, do = _problem(dtype, d, causal, 2, packed=True, do_exp=e)
    oracle, exact = _reference(("A packed", causal, e), q, k, v, do, causal, dtype, packed=True)
    assert all(np.isfinite(t).all() for t in oracle), "the oracle itself must stay finite"
    cq, ck = _cu(PACKED_LQ), _cu(PACKED_LK)
    qg, kg, vg, dog = (t.to(gpu) for t in (q, k, v, do))
    cqg, ckg = torch.from_numpy(cq).to(gpu), torch.from_numpy(ck).to(gpu)
    o, lse = F.varlen_fwd(qg, kg, vg, cqg, ckg, mq, mk, causal)
    bo, bl = (o, lse) if o_from == "kernel" else _oracle_o_lse(gpu, oracle, dtype)
    dq, dk, dv = F.varlen_bwd(qg, kg, vg, bo, bl, dog, cqg, ckg, mq, mk, causal)
    tag = f"packed dO x 2^{e} fp16 d{d} causal={causal} O from the {o_from} {pinned_set}"
    _finite((o, lse, dq, dk, dv), tag)
    for i, (lq, lk) in enumerate(zip(PACKED_LQ, PACKED_LK)):
        qs, ks = slice(cq[i], cq[i + 1]), slice(ck[i], ck[i + 1])
        assert (lse[i, :, lq:] == 0).all().item(), f"padded LSE of sequence {i} must stay zero [{tag}]"
        if lq == 0:
            assert (dk[ks] == 0).all().item() and (dv[ks] == 0).all().item(), f"dK / dV of the sequence without queries must be zero [{tag}]"
            continue
        dead = max(0, lq - lk) if causal else 0
        if causal and i == 1:
            assert dead == 30
        assert (o[qs][:dead] == 0).all().item() and (dq[qs][:dead] == 0).all().item() and (lse[i, :, :dead] == 0).all().item(), f"dead rows of sequence {i} [{tag}]"
        for j, x, sl in ((2, dq, qs), (3, dk, ks), (4, dv, ks)):
            _close(x[sl], oracle[j][sl], exact[j][sl], 2.0 ** -e, dtype, f"{NAMES[j]} {tag} seq {i} lq={lq} lk={lk}", lk)


# ---- B. fp16, V x 2^e ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o_from", ["kernel", "oracle"])
@pytest.mark.parametrize("e", [-14, 12])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_forward_and_backward_follow_the_oracle_across_the_range_of_v(gpu, d, causal, e, o_from, pinned_set):
    """V = fp16(N(0, 1) x 2^e): O (subnormal outputs at e = -14), dQ and dK x 2^-e, dV unscaled, within the plain tolerances of the C oracle; LSE
    within U.LSE_TOL of float64 math; everything finite"""
    b, sq, sk, h, hk = BASE
    _assert_kernel_set(pinned_set, b, sq, sk, h, d, causal, "fp16")
    q, k, v, do = _problem("fp16", d, causal, 3, v_exp=e)
    oracle, exact = _reference(("B", d, causal, e), q, k, v, do, causal, "fp16")
    assert all(np.isfinite(t).all() for t in oracle), "the oracle itself must stay finite"
    outs = _run(gpu, q, k, v, do, causal, o_from, oracle, "fp16")
    tag = f"V x 2^{e} fp16 d{d} causal={causal} O from the {o_from} {pinned_set}"
    _finite(outs, tag)
    for i, factor in ((0, 2.0 ** -e), (2, 2.0 ** -e), (3, 2.0 ** -e), (4, 1.0)):
        _close(outs[i], oracle[i], exact[i], factor, "fp16", f"{NAMES[i]} {tag}", sk)
    err = float(np.abs(outs[1].double().cpu().numpy() - exact[1]).max())
    assert err <= U.LSE_TOL, f"LSE {tag}: {err:.3e}"


# ---- C / D. power-of-two relations ---------------------------------------------------------------------------------------------------

def _floor_magnitude(t, floor=2.0 ** -6):
    """every element with |x| < floor -> +-floor (0 -> +floor): x 2^+-3 stays exactly representable, in fp16 as well"""
    f = t.float()
    sign = torch.where(f < 0, -torch.ones_like(f), torch.ones_like(f))
    return torch.where(f.abs() < floor, sign * floor, f).to(t.dtype)


def _scaled_pair(gpu, dtype, d, causal, relation, e, family):
    """(unit-scale results, scaled results, factor per output or None for 'same bits') of one relation, two runs on the GPU"""
    q, k, v, do = _problem(dtype, d, causal, family)
    f = 2.0 ** e
    scaled = lambda t, s: (t.float() * s).to(t.dtype)
    if relation == "dout":
        unit = _run(gpu, q, k, v, do, causal)
        got = _run(gpu, q, k, v, scaled(do, f), causal)
        return unit, got, (None, None, f, f, f)
    if relation == "v":
        unit = _run(gpu, q, k, v, do, causal)
        return unit, _run(gpu, q, k, scaled(v, f), do, causal), (f, None, f, f, None)
    q, k = _floor_magnitude(q), _floor_magnitude(k)
    qs, ks = scaled(q, f), scaled(k, 1.0 / f)
    assert torch.equal(qs.float(), q.float() * f) and torch.equal(ks.float(), k.float() / f), "the scaled inputs must be exact"
    unit = _run(gpu, q, k, v, do, causal)
    return unit, _run(gpu, qs, ks, v, do, causal), (None, None, 1.0 / f, f, None)


def _mismatch(x, want):
    bad = x != want
    return f"{int(bad.sum())} of {bad.numel()} elements differ, max |diff| {(x - want)[bad].abs().max().item():.3e}"


@pytest.mark.parametrize("relation,e", [("dout", -24), ("dout", -8), ("dout", 8), ("dout", 24), ("v", -24), ("v", -8), ("v", 8), ("v", 24), ("qk", -3), ("qk", 3)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_bf16_power_of_two_scalings_are_exact(gpu, d, causal, relation, e, pinned_set):
    """bf16 keeps fp32's exponent range, so scaling dO, V or the pair (q, 1 / k) by 2^e moves every intermediate by an exact power of two:
    the outputs are the unit-scale outputs times that power BIT FOR BIT, LSE (and whatever the relation leaves alone) keeps its bits"""
    b, sq, sk, h, hk = BASE
    _assert_kernel_set(pinned_set, b, sq, sk, h, d, causal, "bf16")
    unit, got, factors = _scaled_pair(gpu, "bf16", d, causal, relation, e, 4)
    tag = f"{relation} x 2^{e} bf16 d{d} causal={causal} {pinned_set}"
    _finite(got, tag)
    for name, x, u, f in zip(NAMES, got, unit, factors):
        if f is None:
            assert torch.equal(U.bits(x), U.bits(u)), f"{name} must keep its bits [{tag}]"
        else:
            want = u.float() * f
            assert torch.equal(x.float(), want), f"{name} is not the unit-scale result x {f} [{tag}]: {_mismatch(x.float(), want)}"


@pytest.mark.parametrize("e", [-3, 3])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
def test_fp16_q_k_scaling_is_exact_on_normal_outputs(gpu, d, causal, e, pinned_set):
    """fp16, q x 2^e with k x 2^-e: the scores, P, dP, D and dS do not move, so O, LSE and dV keep their bits; dQ x 2^-e and dK x 2^e are exact
    wherever both sides are fp16-normal (at most 2 % of a tensor is not), and within one subnormal spacing carried through the scaling,
    2^-24 x 2^3, elsewhere"""
    b, sq, sk, h, hk = BASE
    _assert_kernel_set(pinned_set, b, sq, sk, h, d, causal, "fp16")
    unit, got, factors = _scaled_pair(gpu, "fp16", d, causal, "qk", e, 5)
    tag = f"qk x 2^{e} fp16 d{d} causal={causal} {pinned_set}"
    _finite(got, tag)
    for name, x, u, f in zip(NAMES, got, unit, factors):
        if f is None:
            assert torch.equal(U.bits(x), U.bits(u)), f"{name} must keep its bits [{tag}]"
            continue
        xs, want = x.float(), u.float() * f
        normal = (u.float().abs() >= FP16_MIN_NORMAL) & (want.abs() >= FP16_MIN_NORMAL)
        excluded = 1.0 - normal.float().mean().item()
        worst = (xs - want)[~normal].abs().max().item() if excluded > 0 else 0.0
        print(f"MARGIN {name} {tag}: {excluded:.4%} of the elements subnormal on either side, their worst deviation {worst:.3e}")
        assert torch.equal(xs[normal], want[normal]), f"{name} is not the unit-scale result x {f} on fp16-normal elements [{tag}]: {_mismatch(xs[normal], want[normal])}"
        assert excluded <= 0.02, f"{name}: {excluded:.4%} of the elements are subnormal on either side [{tag}]"
        assert worst <= 2.0 ** -21, f"{name}: a subnormal element is {worst:.3e} off [{tag}]"


# ---- E. sharp softmax in the backward ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("o_from", ["kernel", "oracle"])
@pytest.mark.parametrize("s", [2.0, 4.0, 6.0])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_sharp_softmax_backward_follows_the_oracle(gpu, dtype, d, causal, s, o_from, pinned_set):
    """q, k x s: score deviations of s^2 nats, at 4 and 6 most rows close to one-hot, |dS|, |dQ| and |dK| well above 1.  O, dQ, dK, dV against the C
    oracle (max_abs, mean_abs) and float64 math (mean_rel under the oracle rule: dQ at s = 2 only, dK up to s = 4, see the file's docstring), LSE
    relative to float64 math, everything finite"""
    b, sq, sk, h, hk = SHARP
    _assert_kernel_set(pinned_set, b, sq, sk, h, d, causal, dtype)
    q, k, v, do = _problem(dtype, d, causal, 6, dims=SHARP, q_scale=s, k_scale=s)
    oracle, exact = _reference(("E", dtype, d, causal, s), q, k, v, do, causal, dtype)
    assert all(np.isfinite(t).all() for t in oracle), "the oracle itself must stay finite"
    outs = _run(gpu, q, k, v, do, causal, o_from, oracle, dtype)
    tag = f"q, k x {s} {dtype} d{d} causal={causal} O from the {o_from} {pinned_set}"
    _finite(outs, tag)
    for i in (0, 2, 3, 4):
        rel = not ((i == 2 and s > 2.0) or (i == 3 and s > 4.0))
        # the chain at s = 4 and 6: one O element that rounds the other way moves D of a near-one-hot row, whose dS_top = P_top (dP_top - D) ~ D's
        # error; an fp32 restatement of the oracle (same rounding points, sums in another order, 0.2 - 0.6 % of O one ulp off) is already 5.0e-3 ..
        # 7.6e-3 from the oracle in dQ max_abs there while no further from float64 math than the oracle is: the derived bound of `_close`
        _close(outs[i], oracle[i], exact[i], 1.0, dtype, f"{NAMES[i]} {tag}", sk, rel=rel, derived=o_from == "kernel" and s > 2.0 and i in (2, 3))
    rel = float((np.abs(outs[1].double().cpu().numpy() - exact[1]) / np.maximum(np.abs(exact[1]), 1.0)).max())
    assert rel <= 1e-4, f"LSE {tag}: relative error {rel:.3e}"
