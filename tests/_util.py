"""Shared test helpers: golden-vector loading, error metrics, torch fp32 reference.

The metric set and the tolerances restate the reference's test contract
(reference test_flash_attn.py:51-71 `_error_metrics`, :407-414 tolerances):
    max_abs <= 5e-3, mean_abs <= 2e-4, mean_rel <= 1e-2  for O, dQ, dK, dV (fp16).
bf16 is an extension (the reference is fp16-only); its 8-bit mantissa makes P/dS/outputs ~8x
coarser, so bf16 tolerances are 8x the fp16 ones and stated here explicitly.
LSE is not pinned by any reference test; we require |dLSE| <= 1e-3 vs fp32 math.
"""
import glob
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

TOL = {
    "fp16": dict(max_abs=5e-3, mean_abs=2e-4, mean_rel=1e-2),
    "bf16": dict(max_abs=4e-2, mean_abs=1.6e-3, mean_rel=8e-2),
}
LSE_TOL = 1e-3
ORACLE_OWN_CAP = 25      # check_mean_rel: the C oracle's own mean_rel may be at most this many times the plain tolerance (an oracle beyond it fails the test: drift)
ORACLE_BOUND_CAP = 10    # ... and a bound derived from it at most this many times the plain tolerance,
ORACLE_TINY_SK = 4       # except on problems of at most this many keys: there the reference algorithm itself reaches 0.18-0.23 (dQ at sk = 2), the derived bound may go as far
                         # as the oracle's own cap (25 x; round 5: 50 x), and BOTH sides are measured against max(|e|, 1 % of the tensor's RMS) instead of max(|e|, 1e-6)
ZERO_ABS_TOL = 1e-4      # rule "zero": |kernel value| where the expectation vanishes identically (fp32 summation-order noise of dP - D, ~1e-6 per dS element, summed over the
                         # query rows and the GQA group of a key; the output format does not enter).  Worst seen on the whole suite: 3.7e-5 (1502 cases, profiles/r6_mean_rel_table.json)
REL_EPS = 1e-6


ULP = {"fp16": 2.0 ** -10, "bf16": 2.0 ** -7}   # one unit in the last place of the OUTPUT format, relative


def error_metrics(x, ref):
    """Raw metrics exactly as the reference defines them (reference test_flash_attn.py:51-71)."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    if x.size == 0:
        return dict(max_abs=0.0, mean_abs=0.0, mean_rel=0.0)
    diff = np.abs(x - ref)
    rel = diff / np.maximum(np.abs(ref), REL_EPS)
    return dict(max_abs=float(diff.max()), mean_abs=float(diff.mean()), mean_rel=float(rel.mean()))


def round_like_output(ref, dtype):
    """fp32 expectation -> nearest fp16 / bf16 value (as fp32).  The kernels (and the reference's
    kernels) emit fp16/bf16; the reference's own tests compare against an oracle that ALSO emits
    fp16 (reference test_flash_attn.py:352-367), so representation error of the output format is
    not part of the tolerance budget: an |x| ~ 2 entry carries up to 1e-3 of pure fp16 rounding."""
    ref = np.asarray(ref, dtype=np.float32)
    if dtype == "fp16":
        with np.errstate(over="ignore"):
            return ref.astype(np.float16).astype(np.float32)
    u = ref.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32)


MARGINS = {}     # test family -> tensor -> worst RAW metrics seen (reference-style, no slack); flushed by conftest at session end
PLAIN_SK_MIN = 64


def _record_margin(name, raw, dtype, plain):
    fam = os.environ.get("PYTEST_CURRENT_TEST", "unknown").split("::")[-1].split("[")[0].split(" ")[0]
    tensor = name.split(" ")[0]
    slot = MARGINS.setdefault(fam, {}).setdefault(f"{tensor}/{dtype}", dict(max_abs=0.0, mean_abs=0.0, mean_rel=0.0, cases=0, plain_bound_cases=0))
    for k in ("max_abs", "mean_abs", "mean_rel"):
        slot[k] = max(slot[k], raw[k])
    slot["cases"] += 1
    slot["plain_bound_cases"] += int(plain)


REL_TABLE = []   # one row per mean_rel decision (family, case, tensor, dtype, kernel / oracle raw mean_rel, bound, rule) -> gpurun_out/mean_rel_table_<stamp>.json (tests/conftest.py)


def raw_mean_rel(x, e):
    """The reference's plain metric (test_flash_attn.py:51-71): mean(|x - e| / max(|e|, 1e-6))."""
    x, e = np.asarray(x, dtype=np.float64), np.asarray(e, dtype=np.float64)
    return float((np.abs(x - e) / np.maximum(np.abs(e), REL_EPS)).mean()) if x.size else 0.0


def check_mean_rel(xa, e, dtype, name, scale, sk, oracle, e_unrounded=None):
    """mean_rel, the reference's third bound (test_flash_attn.py:117,412: plain mean(|d| / max(|ref|, 1e-6)) <= 1e-2).  FOUR rules, every one an assertion:
      "oracle": the caller supplied the C oracle's result (the reference ALGORITHM in contract mode: P / dS / outputs rounded where the reference rounds
                them, everything else exact) for the same tensor.  Bound = max(1e-2, 2 x the oracle's own mean_rel against the same expectation): where the
                reference algorithm itself meets 1e-2 the kernel must meet the plain bound, where it provably cannot (a handful of keys: nothing averages
                the rounding of P / dS out; tools/mean_rel_oracle_table.py prints the oracle's side on the dev container) the kernel may be at most twice as
                far off as the algorithm is - never more than ORACLE_BOUND_CAP (10) x the plain bound, or ORACLE_OWN_CAP (25) x on problems of at most
                ORACLE_TINY_SK (4) keys.  On those tiny problems kernel and oracle are both measured against max(|e|, 1 % of the tensor's RMS): one query
                over two keys has dS_0 = -dS_1, so dQ = dS_0 (K_0 - K_1) is ~1e-6 wherever two fp16 key components nearly agree while the rounding of dS
                leaves ~1e-4 there, and ONE such element puts the raw relative mean of the reference algorithm itself at 0.4 .. 1.7 (round 5, the packed
                grid; that was a rule of its own then).  The oracle must pass its own sanity cap in the same metric.
                Elements where expectation AND oracle are exactly 0 (dead rows, the single-key row 0 of a causal square problem) are left out of both
                relative means (max_abs / mean_abs still cover them).
      "plain":  no oracle result (large problems) and sk >= 64: the reference's plain bound.
      "zero":   the expectation is identically ~0 (max |e| < 1e-4): a single visible key makes dS = P (dP - D) vanish analytically, the oracle returns exact
                zeros, and ANY fp32 implementation that forms D = rowsum(dO * O) and dP = dO . V in different summation orders (the reference's own dot_do_o +
                tensor-core dP included) leaves ~1e-7 .. 1e-5 of noise whose RELATIVE error against 0 is unbounded.  Asserted instead: max |kernel value| <=
                ZERO_ABS_TOL (round 6; recorded without an assertion until then).
      "floor":  neither (sk < 64 without an oracle result): elements below 1 % of the tensor's RMS are measured against 1 % of the RMS instead of against
                (nearly) zero.
    Every decision is appended to REL_TABLE with the asserted quantity (`asserted`) and its bound."""
    tol = TOL[dtype]["mean_rel"] * scale
    fam = os.environ.get("PYTEST_CURRENT_TEST", "unknown").split("::")[-1].split(" ")[0]
    row = dict(family=fam, case=name, dtype=dtype, kernel=raw_mean_rel(xa, e), oracle=None, bound=None, rule=None, asserted=None)
    REL_TABLE.append(row)
    if float(np.abs(e).max(initial=0.0)) < 1e-4:
        zmax = float(np.abs(xa).max(initial=0.0))
        row.update(rule="zero", bound=ZERO_ABS_TOL * scale, asserted=zmax)
        assert zmax <= ZERO_ABS_TOL * scale, f"{name}: expectation vanishes identically, kernel max |x| = {zmax:.3e} > {ZERO_ABS_TOL * scale:.1e}"
        return
    if oracle is not None:
        # Elements where BOTH the exact expectation and the oracle are exactly zero - dead rows; rows with a single visible key, where dS = 0
        # analytically (causal row 0 of every square problem); cancellations such as dS_0 K_0 + dS_1 K_1 with two equal fp16 key components
        # that survive the oracle's exact sums but not fp32 ones - carry no relative information: |x - 0| / 1e-6.  They are left out of
        # the relative mean of kernel and oracle alike and stay under the max_abs / mean_abs bounds of assert_close.
        oa = np.asarray(oracle, dtype=np.float64)
        eu = e if e_unrounded is None else np.asarray(e_unrounded, dtype=np.float64)
        nz = ~((eu == 0.0) & (oa == 0.0))
        if not nz.all():
            row.update(zero_elements=int((~nz).sum()), max_abs_on_zero_elements=float(np.abs(xa[~nz]).max()))       # (bounded by assert_close's max_abs check)
        tiny = sk is not None and sk <= ORACLE_TINY_SK
        floor = max(REL_EPS, 0.01 * float(np.sqrt(np.mean(e * e)))) if tiny else REL_EPS
        rel = lambda t: float((np.abs(t[nz] - e[nz]) / np.maximum(np.abs(e[nz]), floor)).mean()) if nz.any() else 0.0
        o_v, k_v = rel(oa), rel(xa)
        # the oracle may widen the bound only so far: an oracle that drifts past ORACLE_OWN_CAP x the plain tolerance fails here instead of silently
        # loosening every bound derived from it
        assert o_v <= ORACLE_OWN_CAP * tol, f"{name}: the ORACLE's own mean_rel {o_v:.3e} exceeds {ORACLE_OWN_CAP} x {tol:.1e} - oracle drift?"
        bound = min(max(tol, 2.0 * o_v), float(ORACLE_OWN_CAP if tiny else ORACLE_BOUND_CAP) * tol)
        row.update(rule="oracle", oracle=raw_mean_rel(oa[nz], e[nz]), oracle_asserted=o_v, asserted=k_v, bound=bound, floored_denominator=bool(tiny))
        assert k_v <= bound, f"{name} mean_rel={k_v:.3e} > max({tol:.1e}, 2 x oracle's {o_v:.3e}) (sk={sk}{', denominators floored at %.1e' % floor if tiny else ''})"
    elif sk is not None and sk >= PLAIN_SK_MIN:
        k_raw = row["kernel"]
        row.update(rule="plain", bound=tol, asserted=k_raw)
        assert k_raw <= tol, f"{name} PLAIN mean_rel={k_raw:.3e} > {tol:.1e} (sk={sk})"
    else:
        floor = max(REL_EPS, 0.01 * float(np.sqrt(np.mean(e * e))))
        m_rel = float((np.abs(xa - e) / np.maximum(np.abs(e), floor)).mean())
        row.update(rule="floor", bound=tol, asserted=m_rel)
        assert m_rel <= tol, f"{name} mean_rel(floor {floor:.1e})={m_rel:.3e} > {tol:.1e} raw={row['kernel']:.3e}"


def assert_close(x, ref, dtype, name, scale=1.0, sk=None, oracle=None, exact=None):
    """THE stated tolerance of this repo (DESIGN.md "Parity"): the reference's three bounds
    (max_abs 5e-3, mean_abs 2e-4, mean_rel 1e-2 for fp16; x8 for bf16), made magnitude-aware so they stay
    meaningful on the reference grid's degenerate shapes (e.g. sk = 1: dV sums 1024 N(0,1) terms,
    |dV| ~ 30, where ONE fp16 ulp is already 3e-2):
      * the expectation is rounded to the output format first (round_like_output);
      * max_abs:  max(|d| - ulp_out * |ref|)        <= 5e-3   (one output ulp of slack per element)
      * mean_abs: mean|d| - ulp_out/2 * mean|ref|   <= 2e-4   (half an ulp on average)
      * mean_rel: the reference's RAW metric, see check_mean_rel (`oracle` = the C oracle's contract-mode result for this
        tensor when the caller has it; `exact` = exact-arithmetic expectation for the relative metric when `ref` itself is the
        oracle's result - small problems, where max_abs / mean_abs are measured against the reference algorithm with its
        rounding points and mean_rel against exact math for kernel and oracle alike).
    For |values| <~ 1 (every non-degenerate case) these reduce to the reference's plain bounds.
    `sk` (keys per query, when the caller knows it): every case with sk >= 64 must ALSO meet the reference's PLAIN bounds
    (reference test_flash_attn.py:407-414: no ulp slack, no floor) against the expectation in the output format, wherever the
    output FORMAT itself leaves room for them: max_abs <= 5e-3 when max|ref| <= 4 (one fp16 ulp is 3.9e-3 in [4, 8): a single
    rounding flip there already spends the bound) and mean_abs <= 2e-4 when mean|ref| <= 0.25 (the mean half-ulp of a tensor with
    mean |x| = 0.8 is 2e-4 by itself).  First GPU run with the unconditional form (profiles/r2_parity_margins_first_run.json):
    O and dQ met the plain bounds on every one of ~2400 cases; dK / dV exceeded them on 6 cases, all sq >> sk with GQA
    (e.g. lq = 1002, lk = 99, 6 q-heads per kv-head: |dV| ~ 0.8-16), by exactly one output ulp.
    The worst raw metrics per test family go to MARGINS (-> gpurun_out/parity_margins_<stamp>.json).
    Returns the raw reference-style metrics for logging."""
    xa = np.asarray(x, dtype=np.float64)
    assert np.isfinite(xa).all(), f"{name}: non-finite values"
    ref_unrounded = ref
    ref = round_like_output(ref, dtype).astype(np.float64)
    raw = error_metrics(xa, ref)
    if xa.size == 0:
        return raw
    tol, ulp = TOL[dtype], ULP[dtype]
    aref0 = np.abs(ref)
    plain_max = sk is not None and sk >= PLAIN_SK_MIN and float(aref0.max()) <= 4.0
    plain_mean = sk is not None and sk >= PLAIN_SK_MIN and float(aref0.mean()) <= 0.25
    _record_margin(name, raw, dtype, plain_max and plain_mean)
    if plain_max:
        assert raw["max_abs"] <= tol["max_abs"] * scale, f"{name} PLAIN max_abs={raw['max_abs']:.3e} > {tol['max_abs'] * scale:.3e} (sk={sk})"
    if plain_mean:
        assert raw["mean_abs"] <= tol["mean_abs"] * scale, f"{name} PLAIN mean_abs={raw['mean_abs']:.3e} > {tol['mean_abs'] * scale:.3e} (sk={sk})"
    diff, aref = np.abs(xa - ref), np.abs(ref)
    m_max = float(np.maximum(diff - ulp * aref, 0.0).max())
    m_mean = float(diff.mean() - 0.5 * ulp * aref.mean())
    assert m_max <= tol["max_abs"] * scale, f"{name} max_abs(excess over 1 ulp)={m_max:.3e} > {tol['max_abs'] * scale:.3e} raw={raw}"
    assert m_mean <= tol["mean_abs"] * scale, f"{name} mean_abs(excess over ulp/2)={m_mean:.3e} > {tol['mean_abs'] * scale:.3e} raw={raw}"
    e = ref if exact is None else round_like_output(exact, dtype).astype(np.float64)
    check_mean_rel(xa, e, dtype, name, scale, sk, oracle, ref_unrounded if exact is None else exact)
    return raw



def check_kvcache_rows(out, lse, q, k_cache, v_cache, lens, causal, dtname, tag, scale=1.0):
    """decode over a KV cache: every batch entry against the C oracle (the reference's rounding points) on its valid prefix k_cache[i, :L_i];
    the relative metric against exact fp64 math for kernel and oracle alike (assert_close).  An empty entry must be exactly O = 0, LSE = 0."""
    import torch
    from oracle import attn_oracle as A

    mode = A.ROUND_FP16 if dtname == "fp16" else A.ROUND_BF16
    for i, L in enumerate(lens):
        if L == 0:
            assert (out[i] == 0).all().item() and (lse[i] == 0).all().item(), f"{tag}: empty sequence {i} must give O = 0, LSE = 0"
            continue
        qi, ki, vi = (t.detach().double().cpu().numpy() for t in (q[i:i + 1], k_cache[i:i + 1, :L], v_cache[i:i + 1, :L]))
        o_ref, lse_ref = A.attn_fwd(qi, ki, vi, causal=causal, round_mode=mode)
        xo, _ = torch_attention_ref(q[i:i + 1], k_cache[i:i + 1, :L], v_cache[i:i + 1, :L], causal=causal, device="cpu", dtype=torch.float64)
        assert_close(out[i:i + 1].float().cpu().numpy(), o_ref, dtname, f"kvcache O {tag} b{i} L{L}", scale=scale, sk=L, oracle=o_ref, exact=xo.numpy())
        err = float(np.abs(lse[i:i + 1].cpu().numpy() - lse_ref).max())
        assert err <= LSE_TOL, f"{tag}: LSE b{i} L{L} err {err}"


# ---- edge-case helpers shared by the edges suites (tests/test_kvcache_edges_gpu.py, tests/test_attention_edges_gpu.py) ------------------

POISON = (float("nan"), float("inf"), float("-inf"), 65504.0)
SENT16 = 0x7E5A          # an fp16 / bf16 NaN payload nobody computes


def bits(t):
    """the bit pattern of a 16- or 32-bit tensor, for exact comparisons (NaN payloads included)"""
    return t.view(torch_int(t.element_size()))


def torch_int(nbytes):
    import torch

    return {2: torch.int16, 4: torch.int32}[nbytes]


def poison_(t):
    """fill t (any view) with NaN, +inf, -inf and 65504, cycling along the last dim"""
    import torch

    vals = torch.tensor(POISON, dtype=torch.float32, device=t.device).to(t.dtype)
    idx = torch.arange(t.shape[-1], device=t.device) % len(POISON)
    t.copy_(vals[idx].expand(t.shape))
    return t


def guarded(shape, dt, dev, pad, fill=SENT16):
    """a buffer filled with the 16-bit pattern `fill` (fill=None: the POISON cycle) with `pad` extra elements on every dim, and the view
    of `shape` into it (offset by pad // 2 on every dim but the last, 8 elements on the last: rows stay 16-byte aligned); returns
    (buffer, view, index of the view)"""
    import torch

    full = [s + p for s, p in zip(shape, pad)]
    if fill is None:
        buf = poison_(torch.empty(full, dtype=dt, device=dev))
    else:
        buf = torch.full(full, fill, dtype=torch.int16, device=dev).view(dt)
    sl = tuple(slice(p // 2, p // 2 + s) for s, p in zip(shape[:-1], pad[:-1])) + (slice(8, 8 + shape[-1]),)
    return buf, buf[sl], sl


def fp64_math(q, k, v, causal, device="cpu"):
    """plain fp64 attention of ONE batch entry, no special cases beyond the contract's dead rows: q (sq, h, d), k / v (L, hk, d) ->
    O (sq, h, d), LSE (h, sq), on `device`.  NaN / inf propagate as IEEE arithmetic makes them (max and exp included).  The causal mask
    is bottom-right aligned: key j is hidden from query t when j > L - sq + t."""
    import math

    import torch

    q, k, v = (t.detach().to(device=device, dtype=torch.float64) for t in (q, k, v))
    sq, h, d = q.shape
    L, hk = k.shape[0], k.shape[1]
    kt, vt = k.repeat_interleave(h // hk, dim=1), v.repeat_interleave(h // hk, dim=1)
    s = torch.einsum("thd,jhd->htj", q, kt) / math.sqrt(d)
    if causal:
        t = torch.arange(sq, device=device).view(-1, 1)
        j = torch.arange(L, device=device).view(1, -1)
        s = s.masked_fill((j > L - sq + t).unsqueeze(0), float("-inf"))
    m = s.amax(dim=-1) if L > 0 else torch.full((h, sq), float("-inf"), dtype=torch.float64, device=device)
    dead = m == float("-inf")
    p = torch.exp(s - torch.where(dead, torch.zeros_like(m), m).unsqueeze(-1))
    l = p.sum(dim=-1)
    lse = torch.where(dead, torch.zeros_like(m), m + torch.log(l))
    o = torch.einsum("htj,jhd->thd", p, vt) / l.t().unsqueeze(-1)
    o = torch.where(dead.t().unsqueeze(-1), torch.zeros_like(o), o)
    return o, lse


def golden_names(varlen=None):
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
    if varlen is True:
        return [n for n in names if n.startswith("varlen")]
    if varlen is False:
        return [n for n in names if not n.startswith("varlen")]
    return names


def _decode(a, is_bf16):
    """stored inputs: float16 arrays, or int16 bit patterns for bf16 -> float32 values"""
    if is_bf16:
        return (a.astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
    return a.astype(np.float32)


def load_golden(name):
    z = dict(np.load(os.path.join(GOLDEN_DIR, name + ".npz")))
    if "q" not in z:  # c1_causal shares its inputs with c1_noncausal
        src = np.load(os.path.join(GOLDEN_DIR, "c1_noncausal.npz"))
        for k in ("q", "k", "v", "dout"):
            z[k] = src[k]
    b, sq, sk, h, hk, d, causal, is_bf16, sub = (int(x) for x in z["meta"])
    g = dict(name=name, b=b, sq=sq, sk=sk, h=h, hk=hk, d=d, causal=bool(causal),
             dtype="bf16" if is_bf16 else "fp16", sub=sub, varlen="cu_seqlens_q" in z)
    for k in ("q", "k", "v", "dout"):
        g[k] = _decode(z[k], is_bf16)
    for k in ("o", "dq", "dk", "dv", "lse"):
        g[k] = z[k]
    if g["varlen"]:
        g["cu_seqlens_q"], g["cu_seqlens_k"] = z["cu_seqlens_q"], z["cu_seqlens_k"]
    return g


def subsample(g, o=None, dq=None, dk=None, dv=None, lse=None):
    """apply the golden file's row subsampling to full results"""
    s = g["sub"]
    out = []
    for t, is_lse in ((o, False), (dq, False), (dk, False), (dv, False), (lse, True)):
        if t is None:
            out.append(None)
        elif g["varlen"]:
            out.append(t)
        else:
            out.append(t[:, :, ::s] if is_lse else t[:, ::s])
    return out


def torch_dtype(name):
    import torch

    return torch.float16 if name == "fp16" else torch.bfloat16


def to_device(arr, dtype_name, device):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(device=device, dtype=torch_dtype(dtype_name))


def torch_attention_ref(q, k, v, dout=None, causal=False, device=None, dtype=None):
    """Plain PyTorch fp32 statement of the attention contract on the
    tensors' own device (or on `device`, in `dtype`: the small-problem exact expectation runs on the CPU in float64).
    q (b,sq,h,d), k/v (b,sk,hk,d) any float dtype -> fp32 O, LSE (dead rows: O = 0, LSE = 0) and, if dout is given, dQ, dK, dV."""
    import torch

    dtype = dtype or torch.float32
    mv = (lambda t: t.detach().to(device=device, dtype=dtype)) if device is not None else (lambda t: t.detach().to(dtype))
    if dout is not None:
        dout = mv(dout)
    qf = mv(q).requires_grad_(dout is not None)
    kf = mv(k).requires_grad_(dout is not None)
    vf = mv(v).requires_grad_(dout is not None)
    b, sq, h, d = qf.shape
    sk, hk = kf.shape[1], kf.shape[2]
    ratio = h // hk
    qt = qf.permute(0, 2, 1, 3)
    kt = kf.permute(0, 2, 1, 3).repeat_interleave(ratio, dim=1)
    vt = vf.permute(0, 2, 1, 3).repeat_interleave(ratio, dim=1)
    s = torch.matmul(qt, kt.transpose(-1, -2)) * (1.0 / d ** 0.5)
    if causal:
        i = torch.arange(sq, device=qf.device).view(-1, 1)
        j = torch.arange(sk, device=qf.device).view(1, -1)
        s = s.masked_fill(j - i > sk - sq, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    dead = torch.isinf(lse)
    p = torch.exp(s - torch.where(dead, torch.zeros_like(lse), lse).unsqueeze(-1))
    p = torch.where(dead.unsqueeze(-1), torch.zeros_like(p), p)
    o = torch.matmul(p, vt).permute(0, 2, 1, 3)
    lse = torch.where(dead, torch.zeros_like(lse), lse)
    if dout is None:
        return o.detach(), lse.detach()
    dq, dk, dv = torch.autograd.grad(o, (qf, kf, vf), dout)
    return o.detach(), lse.detach(), dq, dk, dv
