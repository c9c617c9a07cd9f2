"""GPU: softmax_scale and softcap on the decode path (flash_attn_with_kvcache(..., softmax_scale=, softcap=), fa_kvcache_options_v5).

Expectations: the C oracle has a fixed scale and no cap, so the value tests compare with fp64 math written here - the masked softmax of
test_kvcache_window_gpu._exact with the scale and cap * tanh(s / cap) added - through _util.assert_close without an oracle (its "plain" rule
from 64 keys on, its "floor" rule below) and _util.LSE_TOL: the project's numbers, no new tolerance.  The rows of one call are asserted
together, in the two groups those rules make (rows that see at least _util.PLAIN_SK_MIN keys, rows that see fewer), as the window suites do.
Every value case also asserts that its own expectation is far (4 x the dtype's mean_abs tolerance) from the expectation with the default scale
and no cap, so a kernel that ignored the new arguments could not pass.  Everything else is a relation that must hold to the bit."""
import math

import numpy as np
import pytest
import torch

import _util as U
import flash_attn_turing as F
from test_kvcache_fp8_gpu import _descale, deq, quantise
from test_kvcache_fp8_gpu import _page as _page8
from test_kvcache_rotary_cpu import rotate_ref
from test_kvcache_rotary_gpu import positions, tables
from test_kvcache_window_gpu import _bounds, _page

pytestmark = pytest.mark.gpu

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
F8 = torch.float8_e4m3fn
NAN = float("nan")


def default_scale(d):
    """1.0f / sqrtf((float)d) as a Python float"""
    return float(np.float32(1.0) / np.sqrt(np.float32(d)))


def _f32(x):
    return float(np.float32(x))


def _rand(shape, dt, gen, mult=1.0):
    return (torch.randn(*shape, dtype=torch.float32, generator=gen) * mult).to(dt)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def exact(q, k, v, lens, scale=None, cap=0.0, window=(-1, -1), causal=False):
    """fp64: scores (q . k) * scale, capped to cap * tanh(s / cap) when cap > 0, THEN masked (length, causal, window), softmax over what is left.
    q (b, sq, h, d), k / v the logical caches (b, capacity, hk, d) (any float dtype: a dequantised 8-bit cache comes as fp32).  Returns O
    (b, sq, h, d), LSE (b, h, sq) - rows without a visible key 0, 0 - and the visible keys per row (b, sq)."""
    b, sq, h, d = q.shape
    capacity, hk = k.shape[1], k.shape[2]
    qd, kd, vd = (t.detach().cpu().double() for t in (q, k, v))
    kd, vd = kd.repeat_interleave(h // hk, dim=2), vd.repeat_interleave(h // hk, dim=2)
    s = torch.einsum("bthd,bjhd->bhtj", qd, kd) * (default_scale(d) if scale is None else _f32(scale))
    if cap > 0:
        s = _f32(cap) * torch.tanh(s / _f32(cap))
    mask = torch.zeros(b, 1, sq, capacity, dtype=torch.bool)
    nvis = torch.zeros(b, sq, dtype=torch.long)
    for i, L in enumerate(lens):
        for t in range(sq):
            lo, hi = _bounds(L, sq, t, window, causal)
            mask[i, 0, t, lo:hi] = True
            nvis[i, t] = hi - lo
    s = s.masked_fill(~mask, float("-inf"))
    m = s.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(s - m)
    den = p.sum(-1, keepdim=True)
    live = mask.any(-1, keepdim=True).expand_as(den)
    w = torch.where(live, p / torch.where(live, den, torch.ones_like(den)), torch.zeros_like(p))
    # (a masked key has weight exactly 0: keep a non-finite V row it holds out of the product)
    o = torch.einsum("bhtj,bjhd->bthd", w, torch.where(mask.any(2)[:, 0, :, None, None], vd, torch.zeros_like(vd)))
    lse = torch.where(live, m + torch.log(den), torch.zeros_like(den)).squeeze(-1)
    return o, lse, nvis


def split_rows(out, lse, xo, xl, nvis, tag):
    """out (b, sq, h, d) / lse (b, h, sq) of one call against the fp64 expectation, the part that is asserted row by row: dead rows exactly 0
    and LSE under LSE_TOL.  Returns the live rows in the two groups of _util.check_mean_rel's rules, {"long" / "short": (got (n, d), expected
    (n, d), the fewest keys a row of the group sees)}, for assert_groups."""
    out_c, lse_c = out.detach().float().cpu(), lse.detach().cpu()
    dead = nvis == 0
    if dead.any():
        assert (out_c[dead] == 0).all().item() and (lse_c.permute(0, 2, 1)[dead] == 0).all().item(), f"{tag}: a row without a visible key must be O = 0, LSE = 0"
    live = ~dead
    if live.any():
        err = float((lse_c.permute(0, 2, 1)[live].double() - xl.permute(0, 2, 1)[live]).abs().max())
        print(f"{tag}: LSE err {err:.3e}")
        assert err <= U.LSE_TOL, f"{tag}: LSE err {err}"
    d = out_c.shape[-1]
    parts = {}
    for name, sel in (("long", nvis >= U.PLAIN_SK_MIN), ("short", (nvis > 0) & (nvis < U.PLAIN_SK_MIN))):
        if sel.any():
            parts[name] = (out_c[sel].reshape(-1, d).numpy(), xo[sel].reshape(-1, d).numpy(), int(nvis[sel].min()))
    return parts


def assert_groups(parts_list, dtname, tag):
    """assert_close over the rows of one or several calls, per group, with sk = the fewest keys any row of the group sees"""
    for name in ("long", "short"):
        parts = [p[name] for p in parts_list if name in p]
        if not parts:
            continue
        got, want = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        raw = U.assert_close(got, want, dtname, f"softcap O {tag} {name} rows", sk=min(p[2] for p in parts))
        print(f"{tag} {name} rows ({got.shape[0]} x {got.shape[1]}): {raw}")


def check(out, lse, xo, xl, nvis, dtname, tag):
    """one call: dead rows exactly 0, LSE under LSE_TOL, and the live rows in their two groups under assert_close"""
    assert_groups([split_rows(out, lse, xo, xl, nvis, tag)], dtname, tag)


def assert_far_from_default(xo, q, k, v, lens, dtname, tag, **kw):
    """the expectation of this case against the expectation with the default scale and no cap: mean |difference| >= 4 x the mean_abs tolerance"""
    x0, _, _ = exact(q, k, v, lens, **kw)
    gap = float((xo - x0).abs().mean())
    print(f"{tag}: mean |expectation - default expectation| = {gap:.3e} ({gap / U.TOL[dtname]['mean_abs']:.1f} x mean_abs tol)")
    assert gap >= 4 * U.TOL[dtname]["mean_abs"], f"{tag}: the case does not tell the new arguments from the defaults (gap {gap:.3e})"


# (softcap, q multiplier, softmax_scale as a multiple of 1 / sqrt(d); None = default)
SETTINGS = [(2.0, 1.0, None), (30.0, 4.0, None), (50.0, 8.0, None), (5.0, 1.0, 0.37), (0.0, 1.0, 2.0), (0.0, 1.0, 0.37)]
COMBOS = [(1, 8, 8), (3, 32, 8), (17, 16, 2), (3, 16, 1), (1, 32, 1)]        # (seqlen_q, h, h_k): ratios 1, 4, 8, MQA with 3 rows, MQA decode
LENS = [0, 1, 31, 33, 64, 100, 777, 1000]
CAP = 1024


def _scale_of(mult, d):
    return None if mult is None else mult / math.sqrt(d)


# ---- 1. values --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_scale_and_cap_against_fp64(gpu, dtname, d, causal):
    """Every call of the grid - the five head / seqlen_q combinations x the six settings x three split counts - has its dead rows and its LSE
    asserted on its own.  For O the rows of the five calls of one (setting, split count) are asserted TOGETHER, per group.  Why not per call:
    the relative metric is mean(|x - e| / max(|e|, 1e-6)), a decode call here has four rows of 8 heads x 64 elements in its "long" group, and
    under the flat softmaxes of the settings with scale 0.37 / sqrt(d) the outputs are averages of hundreds of V rows, about 0.03 in size: an
    element whose exact value lies within 1e-5 of zero carries the ordinary error of a rounded P as a relative error of 1 to 10 and alone puts
    the mean of 2048 elements near the bound, whatever computed it.  The reference algorithm itself (fp32 scores, the exp2 / reciprocal tanh, P
    rounded to the dtype, fp32 accumulation), emulated with torch on exactly this data, gives 1.34e-2 > 1e-2 on the fp16, d 64, sq 1, h 8 / 8,
    cap 5, scale 0.37 call alone and passes on the five calls together.  Bound, reference and cases are unchanged; every row is asserted."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(1000 + d + int(causal))
    b = len(LENS)
    cs = torch.tensor(LENS, dtype=torch.int32, device=gpu)
    data = []
    for sq, h, hk in COMBOS:
        k, v = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen)
        data.append((sq, h, hk, k, v, k.to(gpu), v.to(gpu), _rand((b, sq, h, d), dt, gen)))
    for cap, mult, smult in SETTINGS:
        scale = _scale_of(smult, d)
        parts = {ns: [] for ns in (1, 0, 5)}
        for sq, h, hk, k, v, kg, vg, q1 in data:
            q = (q1.float() * mult).to(dt)
            tag = f"{dtname} d{d} sq{sq} h{h}/{hk} causal={causal} cap={cap} q x{mult} scale={smult}"
            xo, xl, nvis = exact(q, k, v, LENS, scale=scale, cap=cap, causal=causal)
            assert_far_from_default(xo, q, k, v, LENS, dtname, tag, causal=causal)
            for ns in parts:
                out, lse = F.flash_attn_with_kvcache(q.to(gpu), kg, vg, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, softmax_scale=scale,
                                                     softcap=cap)
                assert out.shape == q.shape and out.dtype == dt and lse.shape == (b, h, sq) and lse.dtype == torch.float32
                assert torch.isfinite(out).all().item(), tag
                parts[ns].append(split_rows(out, lse, xo, xl, nvis, f"{tag} splits={ns}"))
        for ns, pl in parts.items():
            assert_groups(pl, dtname, f"{dtname} d{d} causal={causal} cap={cap} q x{mult} scale={smult} splits={ns}, the five calls")


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_fp8_cache_with_cap_and_scale_against_fp64_on_the_dequantised_cache(gpu, dtname, d):
    """read side: an 8-bit cache under per-(batch, head) descales; append side: k / v rows quantised by the call, attention over the quantised
    rows - both against fp64 math on the dequantised cache, k_descale inside the tanh"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(2000 + d)
    lens, sn, sq, h, hk = [0, 1, 31, 64, 333, 1000], 3, 3, 32, 8
    b = len(lens)
    cap, mult, scale = 30.0, 4.0, 0.37 / math.sqrt(d)
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8 = quantise(torch.randn(b, CAP, hk, d, generator=gen), kds).to(gpu)
    v8 = quantise(torch.randn(b, CAP, hk, d, generator=gen), vds).to(gpu)
    q = _rand((b, sq, h, d), dt, gen, mult / 0.37)                                # (so that the scores are those of the q x 4 setting)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for causal in (False, True):
        xo, xl, nvis = exact(q, deq(k8, kds), deq(v8, vds), lens, scale=scale, cap=cap, causal=causal)
        assert_far_from_default(xo, q, deq(k8, kds), deq(v8, vds), lens, dtname, f"fp8 read {dtname} d{d}", causal=causal)
        for ns in (1, 0, 5):
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k8, v8, cache_seqlens=cs, causal=causal, num_splits=ns, return_softmax_lse=True, k_descale=kds, v_descale=vds,
                                                 softmax_scale=scale, softcap=cap)
            check(out, lse, xo, xl, nvis, dtname, f"fp8 read {dtname} d{d} causal={causal} splits={ns}")
    # the append
    k_new, v_new = _rand((b, sn, hk, d), dt, gen), _rand((b, sn, hk, d), dt, gen)
    ka, va = k8.clone(), v8.clone()
    ke, ve = k8.clone(), v8.clone()
    kq, vq = quantise(k_new, kds).to(gpu), quantise(v_new, vds).to(gpu)
    for i, L in enumerate(lens):
        _bits(ke)[i, L:L + sn] = _bits(kq)[i]
        _bits(ve)[i, L:L + sn] = _bits(vq)[i]
    out, lse = F.flash_attn_with_kvcache(q.to(gpu), ka, va, k=k_new.to(gpu), v=v_new.to(gpu), cache_seqlens=cs, causal=True, return_softmax_lse=True, k_descale=kds,
                                         v_descale=vds, softmax_scale=scale, softcap=cap)
    assert _same(ka, ke) and _same(va, ve), "the append of a soft-capped call must write the bytes of the plain append"
    after = [L + sn for L in lens]
    xo, xl, nvis = exact(q, deq(ke, kds), deq(ve, vds), after, scale=scale, cap=cap, causal=True)
    check(out, lse, xo, xl, nvis, dtname, f"fp8 append {dtname} d{d}")


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_window_with_cap_against_fp64(gpu, dtname, d):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(3000 + d)
    lens, sq, h, hk = [0, 1, 31, 33, 100, 777, 1000], 5, 16, 4
    b = len(lens)
    k, v = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen)
    q = _rand((b, sq, h, d), dt, gen, 4.0)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for window, causal in (((31, 0), True), ((100, 0), True), ((45, -1), False), ((-1, 3), False), ((200, 2), False), ((0, 0), False)):
        xo, xl, nvis = exact(q, k, v, lens, cap=30.0, window=window, causal=causal)
        if window != (0, 0):           # (one key per row: the softmax is 1 whatever the score)
            assert_far_from_default(xo, q, k, v, lens, dtname, f"window {window} {dtname} d{d}", window=window, causal=causal)
        for ns in (1, 0, 3):
            out, lse = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns,
                                                 return_softmax_lse=True, softcap=30.0)
            check(out, lse, xo, xl, nvis, dtname, f"window {window} causal={causal} {dtname} d{d} splits={ns}")


# ---- 2. relations that hold to the bit -----------------------------------------------------------------------------------------------------

def _dense_case(gpu, dt, d, gen, sq=3, h=32, hk=8, lens=(0, 1, 31, 33, 100, 777, 1000), mult=4.0):
    b = len(lens)
    k, v = _rand((b, CAP, hk, d), dt, gen).to(gpu), _rand((b, CAP, hk, d), dt, gen).to(gpu)
    q = _rand((b, sq, h, d), dt, gen, mult).to(gpu)
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device=gpu)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_defaults_are_todays_call(gpu, dtname, d):
    """softmax_scale=None, the explicit fp32 default, softcap=0.0 and no keyword at all: the same out, lse and cache bytes - dense, windowed,
    paged, 8-bit, with an append, ragged"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(4000 + d)
    q, k, v, cs = _dense_case(gpu, dt, d, gen)
    b, sq, h, _ = q.shape
    hk = k.shape[2]
    s0 = default_scale(d)
    assert s0 == (0.125 if d == 64 else _f32(1.0 / math.sqrt(128.0)))
    variants = (dict(softmax_scale=None), dict(softmax_scale=s0), dict(softcap=0.0), dict(softmax_scale=s0, softcap=0.0), dict(softmax_scale=None, softcap=0.0),
                dict(softcap=0), dict(softmax_scale=np.float32(1.0) / np.sqrt(np.float32(d))))
    kp, vp, table, _ = _page(k, v, 64, 5)
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
    k_new, v_new = _rand((b, 2, hk, d), dt, gen).to(gpu), _rand((b, 2, hk, d), dt, gen).to(gpu)
    sqs = [1, 0, 5, 3, 16, 1, 2]
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    qr = _rand((sum(sqs), h, d), dt, gen).to(gpu)
    calls = [("dense", q, k, v, dict()), ("causal split", q, k, v, dict(causal=True, num_splits=5)), ("window", q, k, v, dict(causal=True, window_size=(40, 0))),
             ("paged", q, kp, vp, dict(block_table=table, num_splits=3)), ("fp8", q, k8, v8, dict(k_descale=kds, v_descale=vds, causal=True)),
             ("append", q, k, v, dict(k=k_new, v=v_new, causal=True)), ("fp8 append", q, k8, v8, dict(k=k_new, v=v_new, k_descale=kds, v_descale=vds)),
             ("ragged", qr, k, v, dict(cu_seqlens_q=cu, max_seqlen_q=16, causal=True, num_splits=2))]
    for name, qq, kk, vv, kw in calls:
        ka, va = kk.clone(), vv.clone()
        want = F.flash_attn_with_kvcache(qq, ka, va, cache_seqlens=cs, return_softmax_lse=True, **kw)
        for extra in variants:
            kb, vb = kk.clone(), vv.clone()
            got = F.flash_attn_with_kvcache(qq, kb, vb, cache_seqlens=cs, return_softmax_lse=True, **kw, **extra)
            assert _same(got[0], want[0]) and _same(got[1], want[1]), (name, extra)
            assert _same(kb, ka) and _same(vb, va), (name, extra)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("fp8", [False, True])
def test_a_power_of_two_moves_between_the_scale_and_q(gpu, dtname, d, fp8):
    """softmax_scale = s * 2^k on q equals softmax_scale = s on q * 2^k, bit for bit: the raw scores, the multiplier in front of the exponential
    and the LSE factor all scale by exact powers of two.  q is kept where q * 2^k is exact in its dtype (away from fp16's subnormals and its
    overflow).  With and without a cap, over 16-bit and 8-bit caches: this pins the scale path without an oracle."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(5000 + d + int(fp8))
    q, k, v, cs = _dense_case(gpu, dt, d, gen, mult=2.0)
    qf = q.float()
    q = torch.where(qf.abs() < 2.0 ** -6, torch.copysign(torch.full_like(qf, 2.0 ** -6), qf), qf).clamp(-64.0, 64.0).to(dt)
    kw = dict(cache_seqlens=cs, return_softmax_lse=True)
    if fp8:
        kds, vds = _descale(q.shape[0], k.shape[2], gen, gpu), _descale(q.shape[0], k.shape[2], gen, gpu)
        k, v = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
        kw.update(k_descale=kds, v_descale=vds)
    for s in (default_scale(d), 0.37 / math.sqrt(d), 0.11):
        for cap in (0.0, 30.0, 2.0):
            for causal, ns in ((False, 1), (True, 5), (False, 0)):
                base = F.flash_attn_with_kvcache(q, k, v, causal=causal, num_splits=ns, softmax_scale=s, softcap=cap, **kw)
                for e in (-2, -1, 1, 2):
                    q2 = (q.float() * 2.0 ** e).to(dt)
                    assert torch.equal(q2.float(), q.float() * 2.0 ** e)
                    got = F.flash_attn_with_kvcache(q2, k, v, causal=causal, num_splits=ns, softmax_scale=_f32(s) * 2.0 ** -e, softcap=cap, **kw)
                    assert _same(got[0], base[0]) and _same(got[1], base[1]), (s, cap, causal, ns, e)
        # ... and the scale does something: another value gives other bits
        other = F.flash_attn_with_kvcache(q, k, v, softmax_scale=_f32(s) * 1.5, **kw)
        assert not _same(other[0], F.flash_attn_with_kvcache(q, k, v, softmax_scale=s, **kw)[0])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_capped_paged_call_gives_the_bits_of_the_contiguous_one_and_runs_are_identical(gpu, dtname, d):
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(6000 + d)
    q, k, v, cs = _dense_case(gpu, dt, d, gen)
    b, hk = q.shape[0], k.shape[2]
    kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
    k8, v8 = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
    for P in (16, 256):
        kp, vp, table, _ = _page(k, v, P, 11 + P)
        kp8, vp8, table8 = _page8(k8, v8, P, 13 + P)
        for causal, window in ((False, (-1, -1)), (True, (-1, -1)), (True, (77, 0))):
            for ns in (1, 0, 5):
                kw = dict(cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, softcap=30.0, softmax_scale=0.11)
                a = F.flash_attn_with_kvcache(q, k, v, **kw)
                a2 = F.flash_attn_with_kvcache(q, k, v, **kw)
                p = F.flash_attn_with_kvcache(q, kp, vp, block_table=table, **kw)
                assert _same(a[0], a2[0]) and _same(a[1], a2[1]), ("not deterministic", P, causal, window, ns)
                assert _same(a[0], p[0]) and _same(a[1], p[1]), ("paged", P, causal, window, ns)
                a8 = F.flash_attn_with_kvcache(q, k8, v8, k_descale=kds, v_descale=vds, **kw)
                a82 = F.flash_attn_with_kvcache(q, k8, v8, k_descale=kds, v_descale=vds, **kw)
                p8 = F.flash_attn_with_kvcache(q, kp8, vp8, block_table=table8, k_descale=kds, v_descale=vds, **kw)
                assert _same(a8[0], a82[0]) and _same(a8[1], a82[1]), ("fp8 not deterministic", P, causal, window, ns)
                assert _same(a8[0], p8[0]) and _same(a8[1], p8[1]), ("fp8 paged", P, causal, window, ns)
                assert not _same(a[0], F.flash_attn_with_kvcache(q, k, v, **dict(kw, softcap=0.0))[0])


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_sequence_of_a_capped_ragged_call_is_the_capped_dense_call_on_it_alone(gpu, dtname, d):
    """num_splits = 1 always, and a forced split without a left-bounded window; both layouts, 16-bit and 8-bit, with an append"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(7000 + d)
    sqs = [1, 1, 5, 0, 16, 3, 40, 1]
    lens = [1, 0, 63, 64, 65, 777, 900, 300]
    b, total = len(sqs), sum(sqs)
    sns = [1, 0, 2, 0, 16, 3, 40, 1]
    cu = torch.tensor([0] + list(np.cumsum(sqs)), dtype=torch.int32, device=gpu)
    cun = torch.tensor([0] + list(np.cumsum(sns)), dtype=torch.int32, device=gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for h, hk in ((32, 8), (12, 4), (16, 1)):
        k, v = _rand((b, CAP, hk, d), dt, gen).to(gpu), _rand((b, CAP, hk, d), dt, gen).to(gpu)
        q = _rand((total, h, d), dt, gen, 4.0).to(gpu)
        k_new, v_new = _rand((sum(sns), hk, d), dt, gen).to(gpu), _rand((sum(sns), hk, d), dt, gen).to(gpu)
        kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
        k8, v8 = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
        kp, vp, table, _ = _page(k, v, 64, 3)
        layouts = [("contiguous", k, v, dict()), ("paged", kp, vp, dict(block_table=table)), ("fp8", k8, v8, dict(k_descale=kds, v_descale=vds))]
        for name, kk, vv, lkw in layouts:
            for causal, window, ns, append in ((False, (-1, -1), 1, False), (True, (-1, -1), 1, True), (True, (-1, -1), 7, False), (False, (-1, 2), 3, True),
                                               (True, (50, 0), 1, False)):
                kw = dict(causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, softcap=30.0, softmax_scale=0.5 / math.sqrt(d))
                kr, vr = kk.clone(), vv.clone()
                rag = dict(k=k_new, v=v_new, cu_seqlens_k_new=cun) if append else dict()
                out, lse = F.flash_attn_with_kvcache(q, kr, vr, cache_seqlens=cs, cu_seqlens_q=cu, max_seqlen_q=max(sqs), **rag, **lkw, **kw)
                assert out.shape == q.shape and lse.shape == (h, total)
                kd, vd = kk.clone(), vv.clone()
                paged = "block_table" in lkw
                for i, s in enumerate(sqs):
                    c0, n0 = sum(sqs[:i]), sum(sns[:i])
                    one = {key: val[i:i + 1] for key, val in lkw.items()}
                    if append and sns[i]:
                        one.update(k=k_new[n0:n0 + sns[i]][None], v=v_new[n0:n0 + sns[i]][None])
                    if s == 0:
                        continue
                    od, ld = F.flash_attn_with_kvcache(q[c0:c0 + s][None], kd if paged else kd[i:i + 1], vd if paged else vd[i:i + 1], cache_seqlens=cs[i:i + 1], **one, **kw)
                    assert _same(out[c0:c0 + s], od[0]) and _same(lse[:, c0:c0 + s], ld[0]), (name, h, hk, causal, window, ns, append, i)
                if append:          # (sequences without query rows append nothing in this case: sns follows sqs there)
                    assert _same(kr, kd) and _same(vr, vd), (name, "cache bytes", causal, window, ns)


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("fp8", [False, True])
def test_rotary_with_cap_is_the_capped_call_on_rotated_inputs(gpu, dtname, fp8):
    dt = DT[dtname]
    d, h, hk, sn, lens = 128, 16, 4, 3, [0, 5, 100, 700]
    b = len(lens)
    gen = torch.Generator().manual_seed(8000 + int(fp8))
    cos, sin = tables(CAP, 64, dt)
    k0, v0 = _rand((b, CAP, hk, d), dt, gen), _rand((b, CAP, hk, d), dt, gen)
    q, k_new, v_new = _rand((b, sn, h, d), dt, gen, 4.0), _rand((b, sn, hk, d), dt, gen), _rand((b, sn, hk, d), dt, gen)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, return_softmax_lse=True, softcap=2.0, softmax_scale=0.06)
    if fp8:
        kds, vds = _descale(b, hk, gen, gpu), _descale(b, hk, gen, gpu)
        k0, v0 = quantise(k0, kds), quantise(v0, vds)
        kw.update(k_descale=kds, v_descale=vds)
    for causal, inter, ns in ((True, False, 1), (False, True, 4), (True, True, 0)):
        q_rot = rotate_ref(q, cos, sin, positions(lens, sn, causal, CAP), inter)
        k_rot = rotate_ref(k_new, cos, sin, positions(lens, sn, True, CAP), inter)
        ka, va, kb, vb = k0.to(gpu), v0.to(gpu), k0.to(gpu), v0.to(gpu)
        r = F.flash_attn_with_kvcache(q.to(gpu), ka, va, k=k_new.to(gpu), v=v_new.to(gpu), causal=causal, num_splits=ns, rotary_cos=cos.to(gpu), rotary_sin=sin.to(gpu),
                                      rotary_interleaved=inter, **kw)
        p = F.flash_attn_with_kvcache(q_rot.to(gpu), kb, vb, k=k_rot.to(gpu), v=v_new.to(gpu), causal=causal, num_splits=ns, **kw)
        assert _same(r[0], p[0]) and _same(r[1], p[1]) and _same(ka, kb) and _same(va, vb), (causal, inter, ns)
        assert not _same(r[0], F.flash_attn_with_kvcache(q_rot.to(gpu), kb, vb, causal=causal, num_splits=ns, **dict(kw, softcap=0.0))[0])


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("num_splits", [1, 4])
def test_non_finite_scores_follow_fp32_math_on_the_capped_scores(gpu, dtname, num_splits):
    """a NaN query row: that row's O and LSE are NaN, the others keep their bits.  A K row with an inf element: its raw score is +inf for the
    query heads whose element there is positive and -inf for the others, and caps to +softcap / -softcap - every row stays finite and meets the
    fp64 expectation, in which the key takes part with that score"""
    dt = DT[dtname]
    d, h, hk, sq, lens, cap = 64, 8, 2, 2, [200, 70, 33], 5.0
    b = len(lens)
    gen = torch.Generator().manual_seed(9000)
    k, v = _rand((b, 256, hk, d), dt, gen), _rand((b, 256, hk, d), dt, gen)
    q = _rand((b, sq, h, d), dt, gen)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, num_splits=num_splits, return_softmax_lse=True, softcap=cap)
    clean = F.flash_attn_with_kvcache(q.to(gpu), k.to(gpu), v.to(gpu), **kw)
    qn = q.clone()
    qn[1, 0, 3, 7] = NAN
    out, lse = F.flash_attn_with_kvcache(qn.to(gpu), k.to(gpu), v.to(gpu), **kw)
    assert torch.isnan(out[1, 0, 3]).all().item() and torch.isnan(lse[1, 3, 0]).item()
    keep = torch.ones(b, sq, h, dtype=torch.bool)
    keep[1, 0, 3] = False
    assert _same(out[keep.to(gpu)], clean[0][keep.to(gpu)]) and _same(lse.permute(0, 2, 1)[keep.to(gpu)], clean[1].permute(0, 2, 1)[keep.to(gpu)])
    # an inf element in visible K rows; q's element there is made clearly positive for the even query heads and clearly negative for the odd ones
    ki = k.clone()
    ki[0, 150, :, 5] = float("inf")
    ki[1, 3, :, 5] = float("inf")
    ki[2, 32, 1, 5] = float("-inf")
    qi = q.clone()
    qi[..., 5] = torch.where(torch.arange(h) % 2 == 0, 1.0, -1.0)[None, None, :].to(dt) * (qi[..., 5].float().abs() + 0.5).to(dt)
    xo, xl, nvis = exact(qi, ki, v, lens, cap=cap)
    assert torch.isfinite(xo).all() and torch.isfinite(xl).all()
    out, lse = F.flash_attn_with_kvcache(qi.to(gpu), ki.to(gpu), v.to(gpu), **kw)
    assert torch.isfinite(out).all().item() and torch.isfinite(lse).all().item()
    check(out, lse, xo, xl, nvis, dtname, f"inf K element {dtname} splits={num_splits}")
    # the key is there: without it the expectation is another one (one key of 33 at the cap's full weight)
    x_wo, _, _ = exact(qi, torch.where(torch.isinf(ki), torch.zeros_like(ki), ki), v, lens, cap=cap)
    assert float((xo[2] - x_wo[2]).abs().mean()) >= 4 * U.TOL[dtname]["mean_abs"]
    # without the cap the same call is NaN in the rows whose score is +inf (today's contract)
    out0, _ = F.flash_attn_with_kvcache(qi.to(gpu), ki.to(gpu), v.to(gpu), cache_seqlens=cs, num_splits=num_splits, return_softmax_lse=True)
    assert torch.isnan(out0[0, :, 0]).all().item()


@pytest.mark.parametrize("dtname", ["fp16", "bf16"])
@pytest.mark.parametrize("d", [64, 128])
def test_rows_and_pages_out_of_sight_are_never_read(gpu, dtname, d):
    """rows at or past L, rows before a window and unreferenced pages hold NaN: the result is finite and the bits of the clean call"""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(10000 + d)
    lens, sq, h, hk = [0, 1, 31, 33, 100, 777, 1000], 3, 16, 4
    b = len(lens)
    k, v = _rand((b, CAP, hk, d), dt, gen).to(gpu), _rand((b, CAP, hk, d), dt, gen).to(gpu)
    q = _rand((b, sq, h, d), dt, gen, 4.0).to(gpu)
    cs = torch.tensor(lens, dtype=torch.int32, device=gpu)
    for window, causal in (((-1, -1), False), ((-1, -1), True), ((40, 0), True), ((100, 1), False)):
        kn, vn = k.clone(), v.clone()
        for i, L in enumerate(lens):
            lo, _ = _bounds(L, sq, 0, window, causal)
            for t in (kn, vn):
                t[i, :lo] = NAN
                t[i, L:] = NAN
        kp, vp, table, _ = _page(kn, vn, 16, 17)            # (unreferenced pages: NaN)
        for ns in (1, 0, 5):
            kw = dict(cache_seqlens=cs, causal=causal, window_size=window, num_splits=ns, return_softmax_lse=True, softcap=30.0)
            want = F.flash_attn_with_kvcache(q, k, v, **kw)
            assert torch.isfinite(want[0]).all().item() and torch.isfinite(want[1]).all().item()
            assert (want[0][0] == 0).all().item() and (want[1][0] == 0).all().item()            # the empty sequence: a dead row
            for got in (F.flash_attn_with_kvcache(q, kn, vn, **kw), F.flash_attn_with_kvcache(q, kp, vp, block_table=table, **kw)):
                assert _same(got[0], want[0]) and _same(got[1], want[1]), (window, causal, ns)


def test_captured_call_with_a_cap_replays_with_new_lengths(gpu):
    dt, d, h, hk, b = torch.float16, 128, 32, 8, 2
    gen = torch.Generator().manual_seed(11000)
    k, v = _rand((b, 4096, hk, d), dt, gen).to(gpu), _rand((b, 4096, hk, d), dt, gen).to(gpu)
    q = _rand((b, 1, h, d), dt, gen, 4.0).to(gpu)
    cs = torch.tensor([100, 4000], dtype=torch.int32, device=gpu)
    kw = dict(cache_seqlens=cs, causal=True, return_softmax_lse=True, softcap=30.0, softmax_scale=0.05)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.flash_attn_with_kvcache(q, k, v, **kw)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_g, lse_g = F.flash_attn_with_kvcache(q, k, v, **kw)
    lens = [2500, 1]
    cs.copy_(torch.tensor(lens, dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    out_e, lse_e = F.flash_attn_with_kvcache(q, k, v, **kw)
    assert _same(out_g, out_e) and _same(lse_g, lse_e)
    xo, xl, nvis = exact(q, k, v, lens, scale=0.05, cap=30.0, causal=True)
    check(out_g, lse_g, xo, xl, nvis, "fp16", "graph replay")
