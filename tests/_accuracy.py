"""The accuracy budget: every kernel family's error on ordinary random data against the error of the rounding model.

_util.assert_close restates the reference's tolerances, which are absolute; with N(0, 1) inputs over n keys |O| is about n^-1/2 and a mean
tolerance of 2e-4 is 20 .. 100 times the error the algorithm has.  A factor 1 + 2^-9 on O, a truncating pack or a low-precision constant
on the output side passes it.  Two statistics of e = x - ref64 over a whole tensor (ref64 the fp64 expectation, NOT rounded to the output
type) separate those cases:
    gain   = <e, ref64> / <ref64, ref64>      the multiplicative bias
    relrms = rms(e) / rms(ref64)
and both are compared with the same statistics of THE ROUNDING MODEL on the same inputs: fp64 attention that rounds P to the dtype (nearest
even, fp16 subnormals included) in front of P.V and rounds O once - the rounding points of oracle/attn_oracle.c and of every forward
kernel here.  The bounds (`budget_check`):
    |gain_kernel| <= G, G = 2^-13 (fp16) / 2^-10 (bf16): an eighth of the output format's worst-case relative ulp (_util.ULP); the case
                  itself must have |gain_model| <= G / 4, asserted first (a case that cannot is enlarged, G never moves);
    relrms_kernel <= 1.25 relrms_model: what a correct kernel does differently (fp32 accumulation, 1-ulp exp2 / rcp, online rescaling,
                  an fp32 split merge) is orders of magnitude below the two roundings that make up relrms_model, the model's seed scatter is
                  <= 1.09, and the smallest defect to catch (P truncated) starts at 1.37;
    LSE (fp32):   max |lse - lse64| <= max(4 x lse_yardstick, 2^-20 max(|lse64|, 1)), |mean(lse - lse64)| <= 2^-20.  The yardstick is the same
                  logsumexp evaluated in numpy float32; 4 covers two 1-ulp transcendental instructions and sequential sums.

Every bound is asserted on the whole tensor of a call and on every length class of its batch that has 4096 live elements of its own
(`budget_entries`), and every decode case runs with its appended rows at 3 x scale and again at N(0, 1) (`kvcache_case` says why).

The masks are the integer model of tests/_visibility.py (`visible`) and the FP8 latent rows go through dequantize_mla_kv_cache; the fp64 scores
are formed here and not taken from the `scores64` / `exact` builders of the tree, prefill and softcap suites, because those live in GPU test
modules and this one has to load without a device.
This module is CPU only (numpy / torch fp64; the library is imported for nothing but the two plain-torch FP8 latent-row helpers): the
statistics, the model, its mutants' switches and the case builders that tests/test_accuracy_budget_gpu.py runs and
tests/test_accuracy_budget_cpu.py checks without a GPU."""
import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

import _util as U
import _visibility as V

DT = {"fp16": torch.float16, "bf16": torch.bfloat16}
G = {dt: U.ULP[dt] / 8 for dt in ("fp16", "bf16")}          # 2^-13, 2^-10
RMS_FACTOR = 1.25
MIN_N = 4096
LSE_REL = 2.0 ** -20
LSE_YARD = 4.0
INF = float("inf")
DKL, DVL = 576, 512                                          # a latent row (MLA): key width, value width


# ---- rounding to the 16-bit types, from fp64 in one step -------------------------------------------------------------------------------------

def round16(x, dtname, mode="nearest"):
    """float64 array -> the values of fp16 / bf16 as float64, rounded once from fp64 (no fp32 step in between).  mode "nearest": to nearest
    even, into fp16's subnormals too; "truncate": towards zero, what v_cvt_pkrtz would do.  No inf / NaN inputs."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if dtname == "fp16" and mode == "nearest":
        with np.errstate(over="ignore"):
            return x.astype(np.float16).astype(np.float64)              # (numpy converts double -> half directly, correctly rounded)
    a = np.abs(x)
    drop, emin, sub = (42, -14, 2.0 ** 24) if dtname == "fp16" else (45, -126, 2.0 ** 133)      # dropped mantissa bits; smallest normal; 1 / subnormal step
    u = a.view(np.uint64)
    one = np.uint64(1)
    if mode == "nearest":
        r = (u + ((one << np.uint64(drop - 1)) - one) + ((u >> np.uint64(drop)) & one)) & ~((one << np.uint64(drop)) - one)
        small = np.rint(a * sub) / sub
    else:
        assert mode == "truncate", mode
        r = u & ~((one << np.uint64(drop)) - one)
        small = np.floor(a * sub) / sub
    out = np.where(a < 2.0 ** emin, small, r.view(np.float64))
    return np.copysign(out, x)


# ---- the statistics ----------------------------------------------------------------------------------------------------------------------------

def _np64(t):
    return t.detach().double().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)


def _t64(t):
    return t.detach().double().cpu() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))


def stats(x, ref64, live=None):
    """gain, relrms and n of x against the fp64 expectation, over the elements that are finite in both and live (`live`: a bool mask over the
    leading dims of x, True = the element's row sees a key; None = all).  Fewer than 4096 such elements is an AssertionError: the statistic
    means nothing below that."""
    x, r = _t64(x), _t64(ref64)
    assert x.shape == r.shape, (x.shape, r.shape)
    m = torch.isfinite(x) & torch.isfinite(r)
    if live is not None:
        lv = torch.as_tensor(np.asarray(live) if not isinstance(live, torch.Tensor) else live, dtype=torch.bool)
        m &= lv.reshape(lv.shape + (1,) * (x.dim() - lv.dim()))
    n = int(m.sum())
    assert n >= MIN_N, f"stats: {n} finite live elements, the statistics need {MIN_N}"
    xv, rv = (x.reshape(-1), r.reshape(-1)) if n == x.numel() else (x[m], r[m])
    e = xv - rv
    rr = float(torch.dot(rv, rv))
    return dict(gain=float(torch.dot(e, rv)) / rr, relrms=math.sqrt(float(torch.dot(e, e)) / rr), n=n)


# ---- the rounding model ------------------------------------------------------------------------------------------------------------------------

def rounding_model(scores64, visible, v64, dtype, *, sink=None, rowsum="exact", rounded_keys=None, p_rounding="nearest", o_factor=1.0):
    """The forward with the kernels' rounding points and nothing else.  scores64 (..., rows, keys) fp64, ALREADY scaled, capped, descaled (the
    caller does that, so one model serves every family); visible bool, broadcastable to it; v64 (..., keys, dv) fp64, broadcastable over
    the leading dims; dtype "fp16" / "bf16"; sink: None or fp64 broadcastable to (..., rows), one logit that joins the denominator.
    Softmax over the visible keys in fp64; P = exp(s - M) (M the row maximum, the sink included) rounded to dtype; P.V in fp64; O = P.V / l
    rounded once.  rowsum "exact": l is the sum of the unrounded P (and the sink's term) - every decode family (fa_kvcache_attn.hpp, the
    prefill, MLA, sparse MLA and FP8 MLA kernels add the fp32 exponentials before they pack them), the backward's forward recomputation, the
    32x32x16 forward and the bf16 16x16x32 forward.  rowsum "rounded": l is the sum of the ROUNDED P over the keys `rounded_keys` (a slice;
    None = all) and of the unrounded P elsewhere - the fp16 16x16x32 forward with FA_PP16_MFMA_ROWSUM (fa_fwd_pp16.hip), which takes the row
    sums of its steady tiles from the packed P through the matrix pipe but keeps VALU sums of the unrounded P for the first 16 tiles of 64
    keys and for every tail tile: the only family that sums packed P.  p_rounding "truncate" and o_factor (O times a constant in front of its rounding) are the
    mutants of tests/test_accuracy_budget_cpu.py.
    Returns (o_model, lse64, o64): (..., rows, dv), (..., rows), (..., rows, dv) fp64 tensors; rows without a visible key are 0 in all three."""
    assert rowsum in ("exact", "rounded")
    s = torch.as_tensor(scores64, dtype=torch.float64)
    vis = torch.as_tensor(visible, dtype=torch.bool).expand(s.shape)
    sm = s.masked_fill(~vis, -INF)
    m = sm.amax(-1, keepdim=True)
    live = vis.any(-1, keepdim=True)
    snk = None
    if sink is not None:
        snk = torch.as_tensor(sink, dtype=torch.float64).expand(s.shape[:-1]).unsqueeze(-1)
        m = torch.maximum(m, snk)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    p = torch.exp(sm - m)
    extra = torch.exp(snk - m) if snk is not None else torch.zeros_like(m)
    den = p.sum(-1, keepdim=True) + extra
    one = torch.ones_like(den)
    pr = torch.from_numpy(round16(p.numpy(), dtype, p_rounding))
    den_model = den
    if rowsum == "rounded":
        sel = torch.zeros(s.shape[-1], dtype=torch.bool)
        sel[rounded_keys if rounded_keys is not None else slice(None)] = True
        den_model = torch.where(sel, pr, p).sum(-1, keepdim=True) + extra
    v = torch.as_tensor(v64, dtype=torch.float64)
    o64 = torch.where(live, torch.matmul(p, v) / torch.where(live, den, one), torch.zeros(()).double())
    om = torch.where(live, torch.matmul(pr, v) / torch.where(live, den_model, one), torch.zeros(()).double())
    om = torch.from_numpy(round16(om.numpy() * o_factor, dtype))
    lse = torch.where(live, m + torch.log(torch.where(live, den, one)), torch.zeros_like(m)).squeeze(-1)
    return om, lse, o64


def merged_model(scores64, visible, v64, dtype, bounds, *, sink=None, weight_dtype=None):
    """The model over a key split: the keys are cut at `bounds` (0 = b_0 < b_1 < .. = keys), every part is the rounding model WITHOUT the final
    rounding of O (the kernels' partials are fp32), and the parts are merged with the weights exp(lse_part - lse) - rounded to `weight_dtype`
    if given: the mutant "split-merge weights formed in low precision".  With exact weights this is rounding_model (the sink joins the merge)."""
    s = torch.as_tensor(scores64, dtype=torch.float64)
    vis = torch.as_tensor(visible, dtype=torch.bool).expand(s.shape)
    _, lse, _ = rounding_model(s, vis, v64, dtype, sink=sink)
    acc = None
    v = torch.as_tensor(v64, dtype=torch.float64)
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        sp, vp = s[..., lo:hi], vis[..., lo:hi]
        sm = sp.masked_fill(~vp, -INF)
        m = sm.amax(-1, keepdim=True)
        live = vp.any(-1, keepdim=True)
        m = torch.where(live, m, torch.zeros_like(m))
        p = torch.exp(sm - m)
        l = p.sum(-1, keepdim=True)
        pr = torch.from_numpy(round16(p.numpy(), dtype))
        part = torch.matmul(pr, v[..., lo:hi, :]) / torch.where(live, l, torch.ones_like(l))
        w = torch.where(live, torch.exp(m + torch.log(torch.where(live, l, torch.ones_like(l))) - lse.unsqueeze(-1)), torch.zeros_like(l))
        if weight_dtype is not None:
            w = torch.from_numpy(round16(w.numpy(), weight_dtype))
        acc = w * part if acc is None else acc + w * part
    acc = torch.where(vis.any(-1, keepdim=True), acc, torch.zeros(()).double())
    return torch.from_numpy(round16(acc.numpy(), dtype))


def lse_yardstick(scores64, visible, lse64=None, sink=None, rowsum="exact", rounded_keys=None, dtype=None):
    """The same logsumexp in numpy float32: the scores rounded to fp32, max, exp, sum and log in fp32.  Returns its largest error against fp64
    over the rows that see a key (0.0 if none does).  rowsum "rounded" (with dtype and rounded_keys as in rounding_model) is the logsumexp of
    the one family whose LSE is the logarithm of a sum of PACKED P: the fp32 exponentials of those keys are rounded to dtype before they are
    added.  That yardstick is no longer fp32-sized: it carries the rounding noise of P, about 2^-11 sqrt(sum p^2) / sum p per row."""
    assert rowsum in ("exact", "rounded")
    s = torch.as_tensor(scores64, dtype=torch.float64)
    vis = torch.as_tensor(visible, dtype=torch.bool).expand(s.shape)
    if lse64 is None:
        _, lse64, _ = rounding_model(s, vis, torch.zeros(s.shape[-1], 1, dtype=torch.float64), "fp16", sink=sink)
    s32 = s.numpy().astype(np.float32)
    s32[~vis.numpy()] = -np.inf
    sel = np.zeros(s.shape[-1] + (sink is not None), dtype=bool)
    if rowsum == "rounded":
        sel[rounded_keys if rounded_keys is not None else slice(0, s.shape[-1])] = True
    if sink is not None:
        snk = torch.as_tensor(sink, dtype=torch.float64).expand(s.shape[:-1]).numpy().astype(np.float32)
        s32 = np.concatenate([s32, snk[..., None]], axis=-1)
    live = vis.any(-1).numpy()
    if not live.any():
        return 0.0
    rows = s32[live]
    m = rows.max(-1, keepdims=True)
    e = np.exp(rows - m, dtype=np.float32)
    if sel.any():
        e[:, sel] = round16(e[:, sel].astype(np.float64), dtype).astype(np.float32)
    l = e.sum(-1, dtype=np.float32)
    y = (m[:, 0] + np.log(l, dtype=np.float32)).astype(np.float32)
    return float(np.abs(y.astype(np.float64) - _np64(lse64)[live]).max())


# ---- the assertions ----------------------------------------------------------------------------------------------------------------------------

def budget_check(tag, dtname, x, o_model, o64, live=None, lse=None, lse64=None, yard=None, model_stats=None):
    """The three bounds on one tensor (and its LSE, if given) of one call; prints and returns the line of profiles/accuracy_budget.log.  The
    condition on the case (|gain_model| <= G / 4) is asserted before the kernel's values are looked at."""
    g = G[dtname]
    sm = model_stats if model_stats is not None else stats(o_model, o64, live)
    assert abs(sm["gain"]) <= g / 4, f"{tag}: the CASE is too small: |gain_model| = {abs(sm['gain']):.3e} > G / 4 = {g / 4:.3e}"
    xa = _np64(x)
    assert np.isfinite(xa).all(), f"{tag}: non-finite values"
    sk = stats(xa, o64, live)
    ratio = sk["relrms"] / sm["relrms"]
    line = (f"{tag} [{dtname}] n={sk['n']} gain={sk['gain']:+.3e} (model {sm['gain']:+.3e}, G {g:.3e}) relrms={sk['relrms']:.4e} "
            f"relrms_model={sm['relrms']:.4e} ratio={ratio:.4f}")
    checks = [(abs(sk["gain"]) <= g, f"|gain| = {abs(sk['gain']):.3e} > G = {g:.3e}"),
              (ratio <= RMS_FACTOR, f"relrms = {sk['relrms']:.4e} > {RMS_FACTOR} x the model's {sm['relrms']:.4e} (ratio {ratio:.4f})")]
    if lse is not None:
        la, l64 = _np64(lse), _np64(lse64)
        lv = np.ones(l64.shape, dtype=bool) if live is None else np.asarray(live.numpy() if isinstance(live, torch.Tensor) else live, dtype=bool)
        assert np.isfinite(la[lv]).all(), f"{tag}: non-finite LSE"
        err = (la - l64)[lv]
        emax, emean = float(np.abs(err).max()), float(err.mean())
        bound = max(LSE_YARD * yard, LSE_REL * max(float(np.abs(l64[lv]).max()), 1.0))
        line += f" lse_max={emax:.3e} lse_mean={emean:+.3e} yardstick={yard:.3e} lse_bound={bound:.3e}"
        checks += [(emax <= bound, f"max |dLSE| = {emax:.3e} > max(4 x yardstick {yard:.3e}, 2^-20 max(|lse|, 1)) = {bound:.3e}"),
                   (abs(emean) <= LSE_REL, f"|mean dLSE| = {abs(emean):.3e} > 2^-20")]
    print(line)
    failed = [msg for ok, msg in checks if not ok]
    assert not failed, f"{tag} [{dtname}]: " + "; ".join(failed)
    return line


def budget_entries(tag, dtname, base, x, lse=None):
    """budget_check on the whole tensor of a call (the batch entries pooled) AND on every batch entry that has 4096 live elements of its own.
    The pooled statistic weighs an element by its magnitude, so the entry with the fewest keys (|O| ~ n^-1/2) decides it; a defect that shows
    where the softmax is spread (a truncating pack: the 777-key entry) or where the key split cuts through the weight does not move it.  `base`
    is the dict of model_of / attn_forward_model; x (R, dv) and lse (R,) in its row order.  Every statistic is printed; the failures of all of
    them are raised together.  Returns the lines."""
    lines, fails = [], []
    dv = base["o64"].shape[-1]
    for e in [None] + list(range(len(base["yard"]))):
        sel = slice(None) if e is None else base["entry"] == e
        live = base["live"][sel]
        if e is not None and int(live.sum()) * dv < MIN_N:
            continue
        yard = max(base["yard"]) if e is None else base["yard"][e]
        memo = base.setdefault("_model_stats", {})              # (the model's own statistics: once per case, not once per call)
        if e not in memo:
            memo[e] = stats(base["om"][sel], base["o64"][sel], live)
        try:
            lines.append(budget_check(f"{tag} {'pooled' if e is None else 'entry%d' % e}", dtname, x[sel], base["om"][sel], base["o64"][sel], live,
                                      None if lse is None else lse[sel], base["lse"][sel], yard, memo[e]))
        except AssertionError as err:
            fails.append(str(err))
    assert not fails, "\n".join(fails)
    return lines


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------

def _rand(shape, dt, gen, mult=1.0):
    return (torch.randn(*shape, dtype=torch.float32, generator=gen) * mult).to(dt)


def f32(x):
    return float(np.float32(x))


def default_scale(d):
    """1.0f / sqrtf((float)d) as a Python float"""
    return float(np.float32(1.0) / np.sqrt(np.float32(d)))


def heap_words(sq):
    """the binary-heap draft tree (parent (t - 1) // 2): word t has the bits of t's ancestors and of t itself, as unsigned Python integers"""
    words = []
    for t in range(sq):
        w, a = 0, t
        while a >= 0:
            w |= 1 << a
            a = (a - 1) // 2 if a else -1
        words.append(w)
    return words


def visible_mask(lens, sqs, cap, causal=False, window=(-1, -1), words=None):
    """bool per sequence (sq_i, cap) from the integer model of tests/_visibility.py (README's formulas)"""
    out = []
    for L, sq in zip(lens, sqs):
        vis = torch.zeros(sq, cap, dtype=torch.bool)
        for t in range(sq):
            r, extras = V.visible(L, sq, t, causal=causal, window=window, tree_word=None if words is None else words[t])
            vis[t, r.start:r.stop] = True
            if extras:
                vis[t, list(extras)] = True
        out.append(vis)
    return out


@dataclass
class Group:
    """the rows of a call that share one score matrix: scores (hk, ratio, sq, keys) fp64 already scaled / capped / descaled, vis (sq, keys),
    v (hk, 1, keys, dv) fp64, sink None or (hk, ratio, 1); take(out, lse) -> the kernel's values in the model's layout, (hk, ratio, sq, dv) and
    (hk, ratio, sq)"""
    scores: torch.Tensor
    vis: torch.Tensor
    v: torch.Tensor
    sink: torch.Tensor = None
    take: object = None
    L: int = 0
    entry: int = 0                 # the batch entry the rows belong to
    raw: torch.Tensor = None       # the scores in front of the soft cap (None: not capped) and the cap, for the mutant that changes the scale
    cap: float = 0.0


@dataclass
class Built:
    kind: str                          # "kvcache", "mla", "mla_sparse"
    dtname: str
    args: dict                         # CPU tensors and keywords of the call (tests/test_accuracy_budget_gpu.py moves them to the device)
    groups: list
    rowsum: str = "exact"
    rounded_keys: slice = None
    v_descale: torch.Tensor = None     # fp8 kvcache: (b, hk) fp32, already inside Group.v; `v_codes` the undescaled values, for the mutant
    v_codes: list = None
    model: dict = None                 # filled by `model_of`


def _cat_model(parts, yards, entries):
    """per-group (o_model, lse64, o64, live) -> the dict every check takes: om / o64 (R, dv), lse / live / entry (R,), the rows of the groups
    concatenated, and yard = the LSE yardstick per batch entry"""
    flat = lambda i: torch.cat([p[i].reshape(-1, p[i].shape[-1]) if i in (0, 2) else p[i].reshape(-1) for p in parts])
    n = max(entries) + 1
    return dict(om=flat(0), lse=flat(1), o64=flat(2), live=flat(3), entry=torch.cat([torch.full((p[1].numel(),), e, dtype=torch.long) for p, e in zip(parts, entries)]),
                yard=[max([y for y, e in zip(yards, entries) if e == k], default=0.0) for k in range(n)])


def model_of(built, **mutation):
    """The rounding model of a case, per group, rows concatenated (_cat_model).  The plain model is computed once per case and kept; keywords go
    to rounding_model (the mutants; they get no yardstick of their own)."""
    if not mutation and built.model is not None:
        return built.model
    parts, yards = [], []
    for g in built.groups:
        om, lse, o64 = rounding_model(g.scores, g.vis, g.v, built.dtname, sink=g.sink, rowsum=built.rowsum, rounded_keys=built.rounded_keys, **mutation)
        parts.append((om, lse, o64, g.vis.any(-1).expand(lse.shape)))
        yards.append(0.0 if mutation else lse_yardstick(g.scores, g.vis, lse, sink=g.sink))
    res = _cat_model(parts, yards, [g.entry for g in built.groups])
    if not mutation:
        built.model = res
    return res


def flatten_kernel(built, out, lse):
    """the kernel's out / lse (CPU tensors) in the row order of model_of"""
    xs, ls = zip(*(g.take(out, lse) for g in built.groups))
    return torch.cat([x.reshape(-1, x.shape[-1]) for x in xs]).double(), torch.cat([l.reshape(-1) for l in ls]).double()


KEYS = (33, 100, 777)      # a step tail, a few steps, many steps (the split merge) - in one batch,
LENS = KEYS * 3            # three sequences of each: a length class has 3 x sq x h rows, so that its own statistic is quiet enough for |gain_model| <= G / 4
CAP = 800                  # 50 pages of 16
N_HOT = 5                  # rows at 3 x scale in front of L when they are not this call's appended rows


def _quantise(x, descale):
    """the FP8 append contract with torch on the CPU: e4m3_rne(clamp(float(x) / descale, -448, 448)); x (b, s, hk, d), descale (b, hk)"""
    return (x.float() / descale[:, None, :, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)


def _descales(b, hk, gen):
    """(b, hk) fp32 in [0.3, 3], none a power of two"""
    ds = (0.3 * 10.0 ** torch.rand(b, hk, generator=gen)).float()
    return torch.where(torch.log2(ds) == torch.log2(ds).round(), ds * 1.1, ds)


def _paged(k, v, P, seed):
    """pool + table of the logical caches (b, cap, hk, d) under a random page permutation, two spare pages of zeros"""
    b, cap = k.shape[:2]
    cols = cap // P
    nb = b * cols + 2
    perm = torch.randperm(nb, generator=torch.Generator().manual_seed(seed))
    table = perm[:b * cols].view(b, cols).to(torch.int32)
    pools = []
    for t in (k, v):
        raw = t.view(torch.uint8) if t.dtype == torch.float8_e4m3fn else t
        pool = torch.zeros((nb, P) + tuple(t.shape[2:]), dtype=raw.dtype)
        pool[table.long()] = raw.reshape((b, cols, P) + tuple(t.shape[2:]))
        pools.append(pool.view(t.dtype))
    return pools[0], pools[1], table


@lru_cache(maxsize=None)
def kvcache_case(dtname, name, hot=True, d=128, h=16, hk=2, sqs=(5,) * 9, lens=LENS, causal=False, page=0, fp8=False, window=(-1, -1), softcap=0.0, qk_mult=1.0,
                 sinks=False, tree=False, prefill=False, ragged=False, scale_mult=None, append=True, seed=0):
    """One flash_attn_with_kvcache call over a batch with lens[i] keys AFTER the append of sq_i rows.  hot=True: K of the new rows at 3 x the
    scale, as tests/test_kvcache_tree_gpu.py::tree_case and mla_case do, so that the new keys carry weight against a long prefix (append=False:
    the last N_HOT rows of every sequence hold such keys already).  hot=False: the new rows are N(0, 1) like the rest.  Every case runs both ways,
    because they see different defects: a few keys at 3 x scale take most of a row's weight, their P is 1 or close to it, and the rounding of P
    all but leaves the error - a truncating pack is invisible there and plain in the flat variant; rounded split-merge weights add at most the
    error of one more rounding, a factor sqrt(3 / 2) = 1.22 where P's rounding is in the budget and up to sqrt(2) where it is not.  N(0, 1) q / k / v x
    qk_mult (q, k), rounded to the dtype; an FP8 cache holds N(0, 1) data quantised under non-power-of-two descales in [0.3, 3].  The Groups hold
    the fp64 scores as the kernels define them: (q . k) x fp32(softmax_scale) x k_descale, through softcap x tanh(. / softcap) if capped."""
    dt, b, ratio = DT[dtname], len(lens), h // hk
    gen = torch.Generator().manual_seed(7700 + seed)
    assert ragged or len(set(sqs)) == 1
    tq = sum(sqs)
    cu = [sum(sqs[:i]) for i in range(b + 1)]
    q = _rand((tq, h, d), dt, gen, qk_mult)
    kf, vf = torch.randn(b, CAP, hk, d, generator=gen) * qk_mult, torch.randn(b, CAP, hk, d, generator=gen)
    kn, vn = torch.randn(tq, hk, d, generator=gen) * qk_mult * (3.0 if hot else 1.0), torch.randn(tq, hk, d, generator=gen)
    if hot and not append:
        for i, L in enumerate(lens):
            kf[i, L - N_HOT:L] *= 3.0
    kds = vds = None
    if fp8:
        kds, vds = _descales(b, hk, gen), _descales(b, hk, gen)
        kc, vc = _quantise(kf, kds), _quantise(vf, vds)
        knd, vnd = kn.to(dt), vn.to(dt)                       # what the call is given; the kernel quantises it into the cache
    else:
        kc, vc = kf.to(dt), vf.to(dt)
        knd, vnd = kn.to(dt), vn.to(dt)
    kl, vl = kc.clone(), vc.clone()                            # the logical caches after the append
    if append:
        for i in range(b):
            pre = lens[i] - sqs[i]
            assert pre >= 0
            rows = slice(cu[i], cu[i + 1])
            if fp8:
                kl[i, pre:lens[i]] = _quantise(knd[None, rows], kds[i:i + 1])[0]
                vl[i, pre:lens[i]] = _quantise(vnd[None, rows], vds[i:i + 1])[0]
            else:
                kl[i, pre:lens[i]], vl[i, pre:lens[i]] = knd[rows], vnd[rows]
    scale = default_scale(d) if scale_mult is None else f32(default_scale(d) * scale_mult)
    words = heap_words(sqs[0]) if tree else None
    vis = visible_mask(lens, sqs, CAP, causal=causal, window=window, words=words)
    snk = (1.0 + torch.randn(h, generator=gen)).float() if sinks else None
    groups = []
    for i in range(b):
        sq = sqs[i]
        if sq == 0:
            continue
        L = lens[i]                                                                             # (rows at or past L are never visible: left out)
        qi = q[cu[i]:cu[i + 1]].double().view(sq, hk, ratio, d).permute(1, 2, 0, 3)             # (hk, ratio, sq, d)
        ki = kl[i, :L].double().permute(1, 2, 0)[:, None]                                       # (hk, 1, d, L)
        s = torch.matmul(qi, ki) * scale
        vcodes = vl[i, :L].double().permute(1, 0, 2)[:, None]                                   # (hk, 1, L, d)
        vi = vcodes
        if fp8:
            s = s * kds[i].double().view(hk, 1, 1, 1)
            vi = vcodes * vds[i].double().view(hk, 1, 1, 1)
        raw = None
        if softcap > 0:
            raw, s = s, f32(softcap) * torch.tanh(s / f32(softcap))
        if ragged:
            take = (lambda o, l, a=cu[i], n=sq: (o[a:a + n].view(n, hk, ratio, d).permute(1, 2, 0, 3), l[:, a:a + n].view(hk, ratio, n)))
        else:
            take = (lambda o, l, i=i, n=sq: (o[i].view(n, hk, ratio, d).permute(1, 2, 0, 3), l[i].view(hk, ratio, n)))
        groups.append(Group(s, vis[i][:, :L], vi, None if snk is None else snk.double().view(hk, ratio, 1), take, lens[i], KEYS.index(lens[i]), raw, f32(softcap)))
    prefix = torch.tensor([L - n if append else L for L, n in zip(lens, sqs)], dtype=torch.int32)
    kw = dict(cache_seqlens=prefix, causal=causal, return_softmax_lse=True)
    if append:
        kw.update(k=knd if ragged else knd.view(b, sqs[0], hk, d), v=vnd if ragged else vnd.view(b, sqs[0], hk, d))
    if page:
        kc, vc, table = _paged(kc, vc, page, seed)
        kw.update(block_table=table)
    if fp8:
        kw.update(k_descale=kds, v_descale=vds)
    if window != (-1, -1):
        kw.update(window_size=window)
    if softcap > 0:
        kw.update(softcap=softcap)
    if scale_mult is not None:
        kw.update(softmax_scale=scale)
    if sinks:
        kw.update(sinks=snk)
    if tree:
        kw.update(tree_mask=torch.tensor([[w - (1 << 64) if w >= (1 << 63) else w for w in words]] * b, dtype=torch.int64))
    if prefill:
        kw.update(prefill=True)
    if ragged:
        kw.update(cu_seqlens_q=torch.tensor(cu, dtype=torch.int32), max_seqlen_q=max(sqs))
        if append:
            kw.update(cu_seqlens_k_new=torch.tensor(cu, dtype=torch.int32))
    built = Built("kvcache", dtname, dict(q=q if ragged else q.view(b, sqs[0], h, d), k_cache=kc, v_cache=vc, kw=kw), groups)
    if fp8:
        built.v_descale, built.v_codes = vds, [vl[i, :lens[i]].double().permute(1, 0, 2)[:, None] for i in range(b) if sqs[i]]
    return built


# name -> keywords of kvcache_case: one case per attention family (every one runs with num_splits 0, 1 and 3)
KVCACHE_CASES = {
    "plain":     dict(seed=1),
    "causal":    dict(causal=True, d=64, h=12, hk=4, seed=2),
    "paged":     dict(page=16, causal=True, h=12, hk=4, seed=3),
    "fp8":       dict(fp8=True, causal=True, seed=4),
    "fp8_paged": dict(fp8=True, page=16, d=64, h=12, hk=4, seed=5),
    "window":    dict(window=(300, 2), seed=6),
    "softcap":   dict(softcap=5.0, qk_mult=4.0, causal=True, seed=7),
    "sinks":     dict(sinks=True, causal=True, seed=8),
    "sinks_d64": dict(sinks=True, d=64, h=12, hk=4, seed=9),
    "tree":      dict(tree=True, seed=10),
    "prefill":   dict(prefill=True, causal=True, sqs=(65,) * 9, h=12, hk=4, append=False, seed=11),
    "prefill_d64": dict(prefill=True, sqs=(65,) * 9, d=64, h=4, hk=2, append=False, seed=12),
    "d256":      dict(d=256, causal=True, seed=13),
    "ragged":    dict(ragged=True, sqs=(1, 5, 17) * 3, causal=True, seed=14),
    "scale":     dict(scale_mult=0.83, causal=True, d=64, seed=15),
}
SPLITS = (0, 1, 3)


@lru_cache(maxsize=None)
def mla_case(dtname, name, hot=True, h=16, sq=1, causal=True, fp8=False, sparse=0, reps=3, seed=0):
    """flash_mla_with_kvcache (sparse = 0): lens 33 / 100 / 777, three sequences of each, after the append of sq rows - at 3 x scale if hot
    (mla_case of tests/test_kvcache_mla_gpu.py), N(0, 1) if not; see kvcache_case for why both.
    flash_mla_sparse_with_kvcache (sparse = topk): a cache of 4096 rows, lengths 4096 / 3000 / 777, and per token an unsorted list of topk
    entries: distinct valid positions, then duplicates of some of them (a position listed twice counts twice), -1 padding and positions at or
    past the length (invalid: they contribute nothing), shuffled.  hot: the last two rows of every sequence are at 3 x scale (there is no append:
    the engine wrote them) and every list names them.  fp8: the cache as 656-byte rows (quantize_mla_kv_cache); the model runs on
    dequantize_mla_kv_cache, which the call equals bit for bit."""
    dt = DT[dtname]
    gen = torch.Generator().manual_seed(8800 + seed)
    scale = f32(np.float32(1.0) / np.sqrt(np.float32(DKL)))
    if sparse:
        cap, lens, b = 4096, (4096, 3000, 777), 3
        classes = lens
        q = _rand((b, sq, h, DKL), dt, gen)
        kvf = torch.randn(b, cap, 1, DKL, generator=gen)
        if hot:
            for i, L in enumerate(lens):
                kvf[i, L - 2:L] *= 3.0
        kv = kvf.to(dt)
        idx = torch.full((b, sq, sparse), -1, dtype=torch.int32)
        for i, L in enumerate(lens):
            for t in range(sq):
                n_valid = min(L, sparse) * 3 // 4
                keys = torch.randperm(L - 2, generator=gen)[:n_valid]
                if hot:
                    keys[:2] = torch.tensor([L - 2, L - 1])
                n_dup = sparse // 16
                dup = keys[torch.randint(0, n_valid, (n_dup,), generator=gen)]
                n_bad = sparse // 16
                bad = torch.randint(L, cap + 100, (n_bad,), generator=gen)
                lst = torch.cat([keys, dup, bad]).to(torch.int32)[:sparse]
                row = torch.full((sparse,), -1, dtype=torch.int32)
                row[:lst.numel()] = lst
                idx[i, t] = row[torch.randperm(sparse, generator=gen)]
        kv_new = None
        kvl = kv
    else:
        cap, lens, b = CAP, KEYS * reps, len(KEYS) * reps
        classes = KEYS
        q = _rand((b, sq, h, DKL), dt, gen)
        kv = _rand((b, cap, 1, DKL), dt, gen)
        kv_new = _rand((b, sq, 1, DKL), dt, gen, 3.0 if hot else 1.0)
        kvl = kv.clone()
        for i, L in enumerate(lens):
            kvl[i, L - sq:L] = kv_new[i]
    cache = kv
    if fp8:
        from flash_attn_turing.interface import dequantize_mla_kv_cache, quantize_mla_kv_cache

        cache = quantize_mla_kv_cache(kv)
        kvl = dequantize_mla_kv_cache(quantize_mla_kv_cache(kvl), dt)          # (the append quantises whole rows by the same rule)
    groups = []
    for i, L in enumerate(lens):
        if sparse:
            for t in range(sq):
                lst = idx[i, t].long()
                lst = lst[(lst >= 0) & (lst < L)]                              # the valid slots, a multiset
                rows = kvl[i, lst, 0].double()
                s = torch.matmul(q[i, t].double(), rows.t())[None, :, None, :] * scale          # (1, h, 1, slots)
                take = (lambda o, l, i=i, t=t: (o[i, t].view(1, h, 1, DVL), l[i, :, t].view(1, h, 1)))
                groups.append(Group(s, torch.ones(1, lst.numel(), dtype=torch.bool), rows[None, None, :, :DVL], None, take, int(lst.numel()), classes.index(L)))
        else:
            qi = q[i].double().permute(1, 0, 2)[None]                          # (1, h, sq, 576)
            s = torch.matmul(qi, kvl[i, :L, 0].double().t()[None, None]) * scale
            vis = visible_mask([L], [sq], L, causal=causal)[0]
            take = (lambda o, l, i=i: (o[i].permute(1, 0, 2)[None], l[i][None]))
            groups.append(Group(s, vis, kvl[i, :L, 0, :DVL].double()[None, None], None, take, L, classes.index(L)))
    if sparse:
        args = dict(q=q, kv_cache=cache, cache_seqlens=torch.tensor(lens, dtype=torch.int32), indices=idx, kw=dict(return_softmax_lse=True))
    else:
        args = dict(q=q, kv_cache=cache, cache_seqlens=torch.tensor([L - sq for L in lens], dtype=torch.int32),
                    kw=dict(kv_new=kv_new, causal=causal, return_softmax_lse=True))
    built = Built("mla_sparse" if sparse else "mla", dtname, args, groups)
    return built


MLA_CASES = {
    "mla_h16_sq1":     dict(h=16, sq=1, seed=1),
    "mla_h16_sq2":     dict(h=16, sq=2, seed=2),
    "mla_h128_sq1":    dict(h=128, sq=1, seed=3),
    "mla_h128_sq2":    dict(h=128, sq=2, seed=4),
    # (six sequences of each length: with three, one sequence whose token sits on a single key decided a length class and |gain_model| came to
    # 4.3e-4 in bf16, above G / 4)
    "mla_fp8":         dict(h=16, sq=2, fp8=True, reps=6, seed=5),
    "sparse_topk64":   dict(h=16, sq=2, sparse=64, seed=6),
    "sparse_topk2048": dict(h=16, sq=2, sparse=2048, seed=7),
    "sparse_fp8":      dict(h=128, sq=1, sparse=2048, fp8=True, seed=8),
}


def decode_case(dtname, name, hot=True):
    return kvcache_case(dtname, name, hot, **KVCACHE_CASES[name]) if name in KVCACHE_CASES else mla_case(dtname, name, hot, **MLA_CASES[name])


VARIANTS = (True, False)       # hot: the appended rows at 3 x scale; flat: N(0, 1) like the rest


DECODE_NAMES = list(KVCACHE_CASES) + list(MLA_CASES)


# ---- dense and packed forward / backward ---------------------------------------------------------------------------------------------------------

ATTN_SQ = 320              # one 256-row workgroup plus a tail
ATTN_H, ATTN_HK = 4, 2
# packed: (sq_i, sk_i); one sequence is empty on both sides
PACKED = ((320, 320), (0, 0), (100, 777), (33, 100))
# (name, d, causal, sk): sk 320 everywhere, and one long case in which the fp16 16x16x32 forward leaves its exactly summed prefix (1024 keys)
ATTN_CASES = [(f"d{d}_{'causal' if c else 'full'}", d, c, ATTN_SQ) for d in (64, 128) for c in (False, True)] + [("d128_full_sk1664", 128, False, 1664)]
PP16_EXACT_KEYS = 1024


def pp16_rounded_keys(nk):
    """the keys whose row sums the fp16 16x16x32 forward takes from the packed P, for an unmasked head_dim-128 problem of nk keys (fa_fwd_pp16.hip,
    64-key tiles): the steady loop runs trips of three tiles over the n_main = nk // 64 whole tiles, tile 0 apart; the first FA_PP16_EXACT_TILES = 16
    tiles keep VALU sums of the unrounded P, the trips from tile 16 on sum through the matrix pipe, the one or two tiles left over and the tail do not"""
    n_main = nk // 64
    trips = max(0, (n_main - 16) // 3)
    return slice(PP16_EXACT_KEYS, PP16_EXACT_KEYS + 3 * 64 * trips)


@lru_cache(maxsize=None)
def attn_case(dtname, d, causal, sk=ATTN_SQ, packed=False, b=2, seed=0):
    """fwd / bwd (packed: varlen_fwd / varlen_bwd): N(0, 1) q, k, v, dO rounded to the dtype.  Returns a dict with the inputs (numpy float32,
    and cu_seqlens for the packed case) and the shapes; `attn_forward_model` / `attn_backward_model` hold the expectations."""
    from oracle import attn_oracle as A

    mode = A.ROUND_FP16 if dtname == "fp16" else A.ROUND_BF16
    rng = np.random.default_rng(9900 + seed + d + int(causal) + sk + 7 * int(packed))
    h, hk = ATTN_H, ATTN_HK
    if packed:
        lq, lk = [a for a, _ in PACKED], [c for _, c in PACKED]
        shq, shk = (sum(lq), h, d), (sum(lk), hk, d)
        cu_q = np.concatenate([[0], np.cumsum(lq)]).astype(np.int32)
        cu_k = np.concatenate([[0], np.cumsum(lk)]).astype(np.int32)
    else:
        lq, lk, shq, shk, cu_q, cu_k = [ATTN_SQ] * b, [sk] * b, (b, ATTN_SQ, h, d), (b, sk, hk, d), None, None
    c = {n: A.round_lp(rng.standard_normal(s), mode) for n, s in (("q", shq), ("k", shk), ("v", shk), ("do", shq))}
    c.update(dtname=dtname, d=d, causal=causal, packed=packed, lq=lq, lk=lk, cu_q=cu_q, cu_k=cu_k, mode=mode, h=h, hk=hk)
    return c


def _seqs(c):
    """per sequence: (q, k, v, do) as torch fp64 (1, s, h, d) views of the case"""
    out = []
    for i, (nq, nk) in enumerate(zip(c["lq"], c["lk"])):
        if c["packed"]:
            a, e = int(c["cu_q"][i]), int(c["cu_k"][i])
            parts = [c["q"][a:a + nq], c["k"][e:e + nk], c["v"][e:e + nk], c["do"][a:a + nq]]
        else:
            parts = [c[n][i] for n in ("q", "k", "v", "do")]
        out.append(tuple(torch.from_numpy(np.ascontiguousarray(p)).double()[None] for p in parts))
    return out


def attn_forward_model(c, rowsum="exact", **mutation):
    """-> the dict of _cat_model, rows in the order (sequence, kv head, ratio, row); entry = the sequence"""
    key = ("fwd", rowsum) + tuple(sorted(mutation.items()))
    if key in c:
        return c[key]
    h, hk, d = c["h"], c["hk"], c["d"]
    parts, yards, entries = [], [], []
    for i, (q, k, v, _) in enumerate(_seqs(c)):
        nq, nk = q.shape[1], k.shape[1]
        if nq == 0:
            continue
        qi = q[0].view(nq, hk, h // hk, d).permute(1, 2, 0, 3)
        s = torch.matmul(qi, k[0].permute(1, 2, 0)[:, None]) * default_scale(d)
        vis = visible_mask([nk], [nq], nk, causal=c["causal"])[0]
        rk = pp16_rounded_keys(nk) if rowsum == "rounded" else None
        om, lse, o64 = rounding_model(s, vis, v[0].permute(1, 0, 2)[:, None], c["dtname"], rowsum=rowsum, rounded_keys=rk, **mutation)
        parts.append((om, lse, o64, vis.any(-1).expand(lse.shape)))
        yards.append(0.0 if mutation else lse_yardstick(s, vis, lse, rowsum=rowsum, rounded_keys=rk, dtype=c["dtname"]))
        entries.append(i if c["packed"] else 0)           # (the sequences of a dense batch are alike: one statistic)
    c[key] = _cat_model(parts, yards, entries)
    return c[key]


def attn_flatten(c, t, is_lse=False):
    """a kernel output of the q side (O / dQ (.., h, d), or LSE (b, h, max_q)) as CPU tensor -> the row order of attn_forward_model"""
    h, hk, d = c["h"], c["hk"], c["d"]
    out = []
    for i, nq in enumerate(c["lq"]):
        if nq == 0:
            continue
        if is_lse:
            out.append(t[i, :, :nq].reshape(-1))
        else:
            rows = t[int(c["cu_q"][i]):int(c["cu_q"][i]) + nq] if c["packed"] else t[i]
            out.append(rows.view(nq, hk, h // hk, d).permute(1, 2, 0, 3).reshape(-1, d))
    return torch.cat(out).double()


def attn_backward_model(c):
    """The backward's model is the C oracle in ROUND_FP16 / ROUND_BF16 mode (P and dS rounded in front of their products, dQ / dK / dV rounded
    once; its forward supplies O and LSE), and ref64 is torch autograd in fp64 on the same inputs - no rounding anywhere.  -> {"dq" / "dk" /
    "dv": (model, ref64)} as numpy arrays in the layout of the inputs, and the oracle's (o, lse) for the C-ABI call's saved tensors."""
    if "bwd" in c:
        return c["bwd"]
    from oracle import attn_oracle as A

    kw = dict(causal=c["causal"], round_mode=c["mode"])
    if c["packed"]:
        kw.update(cu_seqlens_q=c["cu_q"], cu_seqlens_k=c["cu_k"], max_seqlen_q=max(c["lq"]), max_seqlen_k=max(c["lk"]))
    o, lse = A.attn_fwd(c["q"], c["k"], c["v"], **kw)
    dq, dk, dv = A.attn_bwd(c["q"], c["k"], c["v"], o, lse, c["do"], **kw)
    r = {n: [] for n in ("dq", "dk", "dv")}
    for q, k, v, do in _seqs(c):
        if q.shape[1] == 0 or k.shape[1] == 0:
            g = (torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v))
        else:
            g = U.torch_attention_ref(q, k, v, do, causal=c["causal"], device="cpu", dtype=torch.float64)[2:]
        for n, t in zip(("dq", "dk", "dv"), g):
            r[n].append(t[0].numpy() if c["packed"] else t.numpy())
    ref = {n: np.concatenate(r[n]) for n in r}
    c["bwd"] = dict(dq=(dq, ref["dq"]), dk=(dk, ref["dk"]), dv=(dv, ref["dv"]), o=o, lse=lse)
    return c["bwd"]


def attn_grad_rows(c, name, t):
    """a gradient in the layout of its input (numpy or CPU tensor) -> (R, d) fp64 rows, and the sequence each row belongs to"""
    d, lens = c["d"], c["lq"] if name == "dq" else c["lk"]
    t = torch.as_tensor(np.asarray(t, dtype=np.float64) if not isinstance(t, torch.Tensor) else t.double())
    heads = t.shape[-2]
    if c["packed"]:
        entry = torch.cat([torch.full((n * heads,), i, dtype=torch.long) for i, n in enumerate(lens)])
        return t[:sum(lens)].reshape(-1, d), entry
    return t.reshape(-1, d), torch.zeros(t.numel() // d, dtype=torch.long)


def attn_grad_base(c, name):
    """the dict budget_entries takes for dQ / dK / dV of a case: the oracle in rounding mode as the model, torch fp64 as ref64"""
    model, ref = attn_backward_model(c)[name]
    om, entry = attn_grad_rows(c, name, model)
    o64, _ = attn_grad_rows(c, name, ref)
    return dict(om=om, o64=o64, lse=torch.zeros(om.shape[0], dtype=torch.float64), live=torch.ones(om.shape[0], dtype=torch.bool), entry=entry,
                yard=[0.0] * (int(entry.max()) + 1))
