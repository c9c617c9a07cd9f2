"""The visibility probe: decode the exact SET of keys every query row of an attention call sees.

Every mask of this library is integer arithmetic on key indices, and a tolerance on floating-point values cannot see one key among
hundreds.  The probe turns the question into integers:

  * K = 0 everywhere (cache, appended k, fp8 code 0), q random and finite: every score is exactly 0 - also under softcap, whose
    1 - 2 / (exp(0) + 1) is exactly 0, and under any k_descale.  Every visible key then has the unnormalised P = 1 exactly, so a live
    row's LSE is log(n) (log(n + 1) with a sink of 0.0), n = the number of keys it sees: n_hat = round(exp(lse)).
  * V[j, :] is a two-digit one-hot code of the key index j in base B = min(d / 2, 64): column j % B is 1 and column B + (j // B) % B
    is 1, everything else 0 (d = 256: base 64 on the first 128 columns).  1 and 0 are exact in fp16, bf16 and as e4m3 codes (0x38, 0).
    Then out[c] = m_c / n with m_c = the visible keys whose digit is c, and round(out[c] * n_hat) = m_c.
  * Outside the keys a sequence owns (rows at or past L before an append, spare pages, other sequences' pages) V holds the BAD CODE, 1
    in every column, and K stays 0: an extra key from there changes the count and every column.

CONDITIONS, derived and asserted on the inputs (`check_conditions`), never used to drop a case:
  * n <= 4096: |lse - log n| < 1 / (2 n + 1) decodes n; at 4096 that is 1.2e-4, a hundred times fp32's error on this sum;
  * every expected m_c <= 64: bf16's half ulp (2^-9 relative) then puts at most 0.125 on out[c] * n, the reciprocal's ulp and the
    LSE's error another 64 * (2^-23 + 4096 * 3e-7 / 4096) << 0.25;
  * capacity <= B * B keys, so that the second digit is unique: 1024 keys at d = 64, 4096 at d = 128 and 256.

WHAT IT DOES NOT SEE: two key sets with the same count and the same digit histogram (remove (a, b) and (c, e), add (a, e) and (c, b), in
digits) - a swap invisible to both digits; the value path (V is 0 / 1).  The backward has a probe of its own, below (THE BACKWARD PROBE).

The expectation is `visible`, a pure integer model written from the README's formulas (no float in it, nothing taken from the kernels).
This module holds the encoding, the model, the decoder, the condition asserts, the cache builders and the parameter tables of the GPU
tests (tests/test_kvcache_visibility_gpu.py, tests/test_attention_visibility_gpu.py, tests/test_attention_backward_visibility_gpu.py), which tests/test_visibility_cpu.py enumerates
without a GPU, and the route table of tests/test_kvcache_routes_gpu.py (one case per leaf of the launch dispatch; tests/test_kvcache_routes_cpu.py)."""
import itertools
from dataclasses import dataclass, replace
from functools import lru_cache

import numpy as np

MAX_DIGIT = 64          # largest expected count per code column
MAX_N = 4096            # largest count of visible keys
BAD = 1                 # the bad code: this value in every column
FP8_ONE = 0x38          # e4m3 code of 1.0
K_DESCALE = 0.37        # multiplies a score of 0


def base_of(d):
    return min(d // 2, 64)


def capacity_of(d):
    return base_of(d) ** 2


@lru_cache(maxsize=None)
def codes(d, cap):
    """int64 (cap, d): row j = the code of key j"""
    B = base_of(d)
    assert cap <= B * B, f"capacity {cap} > {B * B}: the second digit would repeat at d = {d}"
    c = np.zeros((cap, d), dtype=np.int64)
    j = np.arange(cap)
    c[j, j % B] = 1
    c[j, B + (j // B) % B] = 1
    c.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def _prefix(d, cap):
    p = np.zeros((cap + 1, d), dtype=np.int64)
    np.cumsum(codes(d, cap), axis=0, out=p[1:])
    return p


# ---- the model --------------------------------------------------------------------------------------------------------------------------

def visible(L, sq, t, causal=False, window=(-1, -1), tree_word=None):
    """The keys query row t of a sequence with L keys and sq query rows sees, as (range, extras): the set is the range plus the tuple.
    README: j < L; causal: j <= L - sq + t; window: L - sq + t - left <= j <= L - sq + t + right, -1 = unbounded, causal sets right = 0;
    tree: j < L - sq, or bit j - (L - sq) of the row's word (an unsigned 64-bit int) with 0 <= j - (L - sq) < sq and j >= 0."""
    L = max(int(L), 0)
    base = L - sq
    if tree_word is not None:
        assert not causal and tuple(window) == (-1, -1) and 0 <= tree_word < 1 << 64
        extras = tuple(base + u for u in range(min(sq, 64)) if (tree_word >> u) & 1 and 0 <= base + u < L)
        return range(0, max(0, min(base, L))), extras
    left, right = window
    if causal:
        right = 0
    lo = 0 if left < 0 else max(0, base + t - left)
    hi = L if right < 0 else min(L, base + t + right + 1)
    return range(lo, max(lo, hi)), ()


def visible_set(*a, **kw):
    r, extras = visible(*a, **kw)
    return set(r) | set(extras)


def signature(d, cap, vis):
    """(n, histogram int64 (d,)) of a (range, extras) pair"""
    r, extras = vis
    assert len(r) == 0 or (r.step == 1 and 0 <= r.start <= r.stop <= cap)
    p = _prefix(d, cap)
    h = p[r.stop] - p[r.start] if len(r) else np.zeros(d, dtype=np.int64)
    if extras:
        h = h + codes(d, cap)[list(extras)].sum(axis=0)
    return len(r) + len(extras), h


# ---- cases ------------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Case:
    """One flash_attn_with_kvcache call.  lens = L_i AFTER the append; sq = the query rows per sequence (dense calls: all equal); tree =
    per sequence a tuple of sq_i unsigned 64-bit words; sink: None, "zero" (0.0 on every head), "ninf" (-inf on every head) or "mixed"
    (0.0 on even heads, -inf on odd ones)."""
    family: str
    name: str
    lens: tuple
    sq: tuple
    d: int = 64
    dtype: str = "fp16"
    fp8: bool = False
    page: int = 0
    h: int = 4
    hk: int = 1
    append: bool = False
    causal: bool = False
    window: tuple = (-1, -1)
    splits: int = 1
    softcap: float = 0.0
    sink: str = None
    tree: tuple = None
    prefill: bool = False
    ragged: bool = False
    cap: int = 1024
    v_scale: float = 1.0

    @property
    def ratio(self):
        return self.h // self.hk

    def sink_extra(self):
        """per query head: 1 where a sink of 0.0 joins the denominator"""
        return [0 if self.sink in (None, "ninf") or (self.sink == "mixed" and g % 2) else 1 for g in range(self.h)]


def check_conditions(c):
    """the derived conditions and the preconditions of the call, on the inputs"""
    assert c.cap <= capacity_of(c.d) and c.cap <= MAX_N and c.cap % 16 == 0
    assert len(c.lens) == len(c.sq) and len(c.lens) >= 1
    assert c.ragged or len(set(c.sq)) == 1 and c.sq[0] >= 1, "a dense call has one seqlen_q"
    assert all(0 <= L <= c.cap for L in c.lens)
    assert not c.append or all(L >= s for L, s in zip(c.lens, c.sq)), "an append of sq rows leaves L >= sq"
    assert c.page == 0 or (c.page % 16 == 0 and c.cap % c.page == 0)
    assert c.h % c.hk == 0 and c.splits >= 0
    assert c.v_scale == 1.0 or (c.fp8 and c.v_scale in (0.25, 0.5, 2.0, 4.0)), "v_descale: 1 or a power of two, over an FP8 cache"
    if c.tree is not None:
        assert max(c.sq) <= 64 and not c.causal and c.window == (-1, -1) and all(len(w) == s for w, s in zip(c.tree, c.sq))
        assert all(0 <= x < 1 << 64 for w in c.tree for x in w)


def expected(c):
    """-> n int64 (R,), hist int64 (R, d), rows [(i, t)]: the model's signature of every (sequence, query row) in packed order"""
    check_conditions(c)
    rows = [(i, t) for i, s in enumerate(c.sq) for t in range(s)]
    n = np.zeros(len(rows), dtype=np.int64)
    hist = np.zeros((len(rows), c.d), dtype=np.int64)
    for r, (i, t) in enumerate(rows):
        vis = visible(c.lens[i], c.sq[i], t, c.causal, c.window, None if c.tree is None else c.tree[i][t])
        n[r], hist[r] = signature(c.d, c.cap, vis)
    assert n.max(initial=0) <= MAX_N and hist.max(initial=0) <= MAX_DIGIT, f"{c.name}: a count leaves the decodable range"
    return n, hist, rows


def row_sets(c):
    return [visible_set(c.lens[i], c.sq[i], t, c.causal, c.window, None if c.tree is None else c.tree[i][t])
            for i, s in enumerate(c.sq) for t in range(s)]


# ---- the decoder (torch, on the tensors' own device; the CPU tests feed it emulated kernel outputs) ---------------------------------------

def decode(out, lse, extra, v_scale=1.0):
    """out (R, h, d) fp16 / bf16, lse (R, h) fp32, extra (h,) int = 1 where a sink of 0.0 sits in the denominator
    -> n (R, h) int64 = the visible keys, hist (R, h, d) int64.  A dead row (O = 0, LSE = 0 exactly) decodes to n = 0; a row that sees one
    key has LSE = 0 too and is told apart by its two ones."""
    import torch

    assert torch.isfinite(out.float()).all().item() and torch.isfinite(lse).all().item(), "non-finite output"
    n_tot = torch.round(torch.exp(lse.double())).long()
    hist = torch.round(out.double() / v_scale * n_tot.unsqueeze(-1).double()).long()
    n = n_tot - extra.to(n_tot.device).long().unsqueeze(0)
    dead = (out == 0).all(dim=-1) & (lse == 0)
    n = torch.where(dead, torch.zeros_like(n), n)
    return n, hist


def assert_signature(c, n_dec, hist_dec, n_exp, hist_exp, rows):
    """integer equality of the decoded and the expected signature on every (sequence, head, row).  The message names the first rows that differ with the digit columns that differ: which key was lost or gained."""
    import torch

    ne = torch.from_numpy(n_exp).to(n_dec.device).unsqueeze(1)
    he = torch.from_numpy(hist_exp).to(n_dec.device).unsqueeze(1)
    bad = (n_dec != ne) | (hist_dec != he).any(dim=-1)
    if not bad.any().item():
        return
    B, msgs = base_of(c.d), []
    for r, g in bad.nonzero()[:6].tolist():
        i, t = rows[r]
        diff = (hist_dec[r, g] - he[r, 0]).cpu().numpy()
        cols = {(f"lo{k}" if k < B else f"hi{k - B}" if k < 2 * B else f"pad{k}"): (int(hist_exp[r, k]), int(hist_exp[r, k] + diff[k])) for k in np.flatnonzero(diff)[:12]}
        msgs.append(f"seq {i} (L={c.lens[i]}, sq={c.sq[i]}) head {g} row {t}: expected n={int(n_exp[r])}, decoded n={int(n_dec[r, g])}; "
                    f"digit counts (expected, decoded) that differ: {cols}")
    raise AssertionError(f"{c.name}: {int(bad.sum())} (row, head) signatures differ from the model [{c}]\n  " + "\n  ".join(msgs))


# ---- builders and the call --------------------------------------------------------------------------------------------------------------

def torch_dtype(name):
    import torch

    return torch.float16 if name == "fp16" else torch.bfloat16


def code_tensor(d, cap, dev):
    import torch

    return torch.from_numpy(codes(d, cap).copy()).to(dev).to(torch.uint8)


def build_cache(c, dev, gen):
    """K (all 0) and V of the call: good codes on the rows a sequence owns BEFORE the append, the bad code everywhere else (rows at or past
    that length, spare pages).  Contiguous (b, cap, hk, d), or a pool under a random page permutation with spare pages.
    -> k_cache, v_cache, block_table or None"""
    import torch

    b, cap, hk, d = len(c.lens), c.cap, c.hk, c.d
    before = torch.tensor([L - s if c.append else L for L, s in zip(c.lens, c.sq)], device=dev)
    good = torch.arange(cap, device=dev).unsqueeze(0) < before.unsqueeze(1)
    v = torch.where(good.unsqueeze(-1), code_tensor(d, cap, dev).unsqueeze(0), torch.full((), BAD, dtype=torch.uint8, device=dev))
    v = v.unsqueeze(2).expand(b, cap, hk, d).contiguous()
    table = None
    if c.page:
        nblk, spare = cap // c.page, 5
        perm = torch.randperm(b * nblk + spare, generator=gen)
        table = perm[: b * nblk].view(b, nblk).to(device=dev, dtype=torch.int32)
        pool = torch.full((b * nblk + spare, c.page, hk, d), BAD, dtype=torch.uint8, device=dev)
        pool[table.flatten().long()] = v.view(b * nblk, c.page, hk, d)
        v = pool
    if c.fp8:
        v = (v * FP8_ONE).view(torch.float8_e4m3fn)
        k = torch.zeros(v.shape, dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
    else:
        v = v.to(torch_dtype(c.dtype))
        k = torch.zeros_like(v)
    return k, v, table


def run_kvcache(c, dev):
    """build the probe's inputs for the case, call flash_attn_with_kvcache, -> out (R, h, d), lse (R, h) in packed (sequence, row) order"""
    import torch

    from flash_attn_turing import flash_attn_with_kvcache

    check_conditions(c)
    dt = torch_dtype(c.dtype)
    gen = torch.Generator(device="cpu").manual_seed(len(c.name) * 7919 + sum(c.lens))
    b, total = len(c.lens), sum(c.sq)
    q = torch.randn(total, c.h, c.d, generator=gen).to(dev, dt)
    k_cache, v_cache, table = build_cache(c, dev, gen)
    kw = dict(cache_seqlens=torch.tensor([L - s if c.append else L for L, s in zip(c.lens, c.sq)], dtype=torch.int32, device=dev), causal=c.causal,
              num_splits=c.splits, return_softmax_lse=True, block_table=table, window_size=c.window)
    cu = torch.tensor([0] + list(itertools.accumulate(c.sq)), dtype=torch.int32, device=dev)
    if c.append:
        pos = torch.tensor([L - s + t for L, s in zip(c.lens, c.sq) for t in range(s)], dtype=torch.long, device=dev)
        # (the logical V is v_scale x code: over an FP8 cache the appended 0 / v_scale quantise to the codes 0 / 0x38, exactly, v_scale a power of two)
        v_new = (code_tensor(c.d, c.cap, dev)[pos].to(dt) * c.v_scale).unsqueeze(1).expand(total, c.hk, c.d).contiguous()
        k_new = torch.zeros_like(v_new)
        if not c.ragged:
            k_new, v_new = (x.view(b, c.sq[0], c.hk, c.d) for x in (k_new, v_new))
        else:
            kw.update(cu_seqlens_k_new=cu)
        kw.update(k=k_new, v=v_new)
    if c.fp8:
        kw.update(k_descale=torch.full((b, c.hk), K_DESCALE, dtype=torch.float32, device=dev),
                  v_descale=torch.full((b, c.hk), c.v_scale, dtype=torch.float32, device=dev))
    if c.ragged:
        kw.update(cu_seqlens_q=cu, max_seqlen_q=max(max(c.sq), 1))
    else:
        q = q.view(b, c.sq[0], c.h, c.d)
    if c.softcap:
        kw.update(softcap=c.softcap)
    if c.sink is not None:
        kw.update(sinks=torch.tensor([0.0 if e else float("-inf") for e in c.sink_extra()], dtype=torch.float32, device=dev))
    if c.tree is not None:
        words = [x - (1 << 64) if x >= 1 << 63 else x for w in c.tree for x in w]
        tm = torch.tensor(words, dtype=torch.int64, device=dev)
        kw.update(tree_mask=tm if c.ragged else tm.view(b, c.sq[0]))
    if c.prefill:
        kw.update(prefill=True)
    out, lse = flash_attn_with_kvcache(q, k_cache, v_cache, **kw)
    if c.ragged:
        assert out.shape == (total, c.h, c.d) and lse.shape == (c.h, total)
        return out, lse.t()
    assert out.shape == (b, c.sq[0], c.h, c.d) and lse.shape == (b, c.h, c.sq[0])
    return out.reshape(total, c.h, c.d), lse.permute(0, 2, 1).reshape(total, c.h)


def probe_kvcache(c, dev):
    """run the case and assert that the decoded signature equals the model's -> n, hist decoded"""
    import torch

    out, lse = run_kvcache(c, dev)
    n_dec, hist_dec = decode(out, lse, torch.tensor(c.sink_extra()), c.v_scale)
    assert_signature(c, n_dec, hist_dec, *expected(c))
    return n_dec, hist_dec


# ---- parameter tables of tests/test_kvcache_visibility_gpu.py ----------------------------------------------------------------------------

DTYPES = ("fp16", "bf16")
PAGES = (0, 16, 48, 256)
SPLITS = (1, 2, 3, 5, "steps", 0)
RATIOS = (1, 3, 4, 5, 12, 16)
SQS = (1, 2, 3, 5, 16, 17, 33)
LEFTS = (0, 1, 15, 16, 31, 32, 33, 63, 64, 65, 100, 500, -1)
RIGHTS = (-1, 0, 1, 2, 31, 32, 40)
TREE_SQS = (1, 2, 17, 33, 63, 64)
PREFILL_SQS = (1, 15, 16, 17, 63, 64, 65, 127, 129, 200)
PREFILL_RATIOS = (1, 4, 5, 64)
SOFTCAP = 30.0


def _axes(i, ratios=RATIOS, d=None):
    """the common axes, rotated through the cases of a family (not a cross-product): every value of every axis occurs within any six
    consecutive i, which tests/test_visibility_cpu.py asserts per family"""
    page = PAGES[(i + i // 4) % 4]
    ratio = ratios[(5 * i + i // len(ratios)) % len(ratios)]
    hk = 2 if ratio <= 5 else 1
    cap = 1008 if page == 48 else 1024       # 21 pages of 48 rows: the largest paged capacity within 32 x 32 keys
    splits = SPLITS[(i + i // 6) % 6]
    return dict(dtype=DTYPES[i % 2], fp8=bool((i // 2) % 2), page=page, h=ratio * hk, hk=hk, cap=cap, splits=cap // 32 if splits == "steps" else splits,
                append=bool((i // 3) % 2), d=d or (64, 64, 128)[i % 3])


def band_lens(cap, sq=0, append=False):
    """every L from 0 to 130, 250..262, 505..519 and the last 15 up to the capacity (1010..1024); an append of sq rows leaves L >= sq"""
    lens = list(range(0, 131)) + list(range(250, 263)) + list(range(505, 520)) + list(range(cap - 14, cap + 1))
    return tuple(L for L in lens if not append or L >= sq)


def window_lens(cap, sq=0, append=False):
    """three runs of more than 64 consecutive lengths - lo and lim of every row take every residue mod 32 at the start of the cache, around
    key 512 (where a forced split of the capacity cuts) and at its end"""
    lens = list(range(0, 71)) + list(range(480, 561)) + list(range(cap - 70, cap + 1))
    return tuple(L for L in lens if not append or L >= sq)


def _dense(family, name, lens, sq, **kw):
    return Case(family=family, name=f"{family}/{name}", lens=tuple(lens), sq=(sq,) * len(lens), **kw)


def _plain_cases(family="plain", thin=1, **extra):
    out = []
    for i, (sq, causal) in enumerate(itertools.product(SQS, (False, True))):
        ax = _axes(i)
        v_scale = 0.25 if ax["fp8"] and i % 4 == 2 else 1.0
        out.append(_dense(family, f"sq{sq}-{'causal' if causal else 'full'}", band_lens(ax["cap"], sq, ax["append"])[::thin], sq, causal=causal, v_scale=v_scale, **ax, **extra))
    return out


def _window_cases(family="window", thin=1, **extra):
    out = []
    for i in range(16):
        ax = _axes(i + 1)
        left, right, causal, sq = LEFTS[i % 13], RIGHTS[i % 7], i % 4 == 3, SQS[(3 * i) % 7]
        out.append(_dense(family, f"w{left}_{right}-{'causal-' if causal else ''}sq{sq}", window_lens(ax["cap"], sq, ax["append"])[::thin], sq, causal=causal,
                          window=(left, right), **ax, **extra))
    return out


def _sink_cases():
    out = []
    for i, (mode, split, kind) in enumerate(itertools.product(("zero", "ninf", "mixed"), (False, True), ("causal", "window"))):
        ax = _axes(i)
        ax["splits"] = (2, 3, 5, ax["cap"] // 32, 0, 7)[(i // 4) * 2 + i % 2] if split else 1     # 0: the library's choice may be 1 at these sizes
        sq = SQS[(2 * i) % 7]
        if kind == "causal":
            kw, lens = dict(causal=True), band_lens(ax["cap"], sq, ax["append"])
        else:
            kw, lens = dict(window=(LEFTS[(5 * i + 2) % 12], RIGHTS[i % 7]), causal=i % 3 == 0), window_lens(ax["cap"], sq, ax["append"])
        out.append(_dense("sinks", f"{mode}-{'split' if split else 'unsplit'}-{kind}-sq{sq}", lens, sq, sink=mode, **kw, **ax))
    return out


def heap_words(sq):
    """the words of tree_mask_from_parents for the binary-heap tree parents[t] = (t - 1) // 2: ancestors plus self"""
    words = []
    for t in range(sq):
        w, u = 0, t
        while u >= 0:
            w |= 1 << u
            u = (u - 1) // 2 if u > 0 else -1
        words.append(w)
    return tuple(words)


def tree_entries(sq, cap, append, seed):
    """(L, words) per sequence of one tree call: every mask kind at lengths below, at and above sq; the single-bit masks (row t sees draft
    token (t + p) % sq only) at every shift p, two lengths each"""
    rng = np.random.default_rng(seed)
    full64 = (1 << 64) - 1
    kinds = {
        "empty": (0,) * sq,
        "full": ((1 << sq) - 1,) * sq,
        "full64": (full64,) * sq,                                                  # bits at or above sq are ignored
        "tril": tuple((1 << (t + 1)) - 1 for t in range(sq)),
        "bit63": (1 << 63,) * sq,                                                  # the sign bit: a key only at sq = 64
        "heap": heap_words(sq),
        "random": tuple(int(x) for x in rng.integers(0, 1 << 64, size=sq, dtype=np.uint64)),
    }
    lens = sorted({L for L in (0, sq // 2, sq - 1, sq, sq + 1, sq + 31, sq + 32, sq + 33, 200, 517, cap - 1, cap) if 0 <= L <= cap and (not append or L >= sq)})
    entries = [(L, w) for w in kinds.values() for L in lens]
    for p in range(sq):
        for L in (lens[p % len(lens)], lens[-1 - p % 2]):
            entries.append((L, tuple(1 << ((t + p) % sq) for t in range(sq))))
    return entries


def _tree_cases():
    out = []
    for i, sq in enumerate(TREE_SQS):
        ax = _axes(i)
        ent = tree_entries(sq, ax["cap"], ax["append"], 100 + sq)
        out.append(_dense("tree", f"sq{sq}", [e[0] for e in ent], sq, tree=tuple(e[1] for e in ent), **ax))
    for i, append in ((6, False), (7, True)):                                      # ragged: every sq of the table (and 0) in one call
        ax = dict(_axes(i), append=append)
        ent = [(s, e) for s in (0,) + TREE_SQS for e in (tree_entries(s, ax["cap"], append, 200 + s)[:: 5] if s else [(0, ()), (33, ()), (ax["cap"], ())])]
        out.append(Case(family="tree", name=f"tree/ragged-{'append' if append else 'read'}", lens=tuple(e[0] for _, e in ent), sq=tuple(s for s, _ in ent),
                        tree=tuple(e[1] for _, e in ent), ragged=True, **ax))
    return out


def prefill_lens(sq, cap, append, ratio):
    lens = sorted({L for L in [0, 1, 2, sq // 2, sq - 1, sq, sq + 1, 2 * sq - 1, 2 * sq, 2 * sq + 1, cap - sq, cap - 1, cap] + list(range(30, 35)) + list(range(62, 67))
                   + list(range(126, 131)) + list(range(250, 263, 2)) + list(range(505, 520)) + list(range(cap - 14, cap - 1, 3)) if 0 <= L <= cap and (not append or L >= sq)})
    return tuple(lens[:: 3 if sq * ratio > 2048 else 1])


def _prefill_cases():
    out = []
    for i, (sq, causal) in enumerate(itertools.product(PREFILL_SQS, (True, False))):
        ax = _axes(i, ratios=PREFILL_RATIOS)
        out.append(_dense("prefill", f"sq{sq}-{'causal' if causal else 'full'}", prefill_lens(sq, ax["cap"], ax["append"], ax["h"] // ax["hk"]), sq, causal=causal, prefill=True, **ax))
    return out


def _d256_cases():
    out = []
    kinds = (("full", {}), ("causal", dict(causal=True)), ("w33_2", dict(window=(33, 2))), ("w100-causal", dict(window=(100, 0), causal=True)))
    for i, ((name, kw), fp8) in enumerate(itertools.product(kinds, (False, True))):
        ax = dict(_axes(i, d=256), fp8=fp8)
        sq = SQS[(i + 2) % 7]
        lens = (window_lens if "window" in kw else band_lens)(ax["cap"], sq, ax["append"])[::2]
        out.append(_dense("d256", f"{name}-{'fp8' if fp8 else '16bit'}-sq{sq}", lens, sq, **kw, **ax))
    return out


RAGGED_SQS = (0, 1, 2, 5, 16, 17, 40)


def ragged_entries(cap, append, sqs=RAGGED_SQS):
    """(sq_i, L_i): every sq_i with lengths on both sides of it"""
    ent = []
    for s in sqs:
        for L in sorted({0, max(s - 1, 0), s, s + 1, s // 2, 31, 32, 33, 100, 517, cap - 1, cap}):
            if not append or L >= s:
                ent.append((s, L))
    return ent


def _ragged_cases():
    kinds = (("mixed-causal", dict(causal=True), RAGGED_SQS), ("mixed-window", dict(window=(33, 1)), RAGGED_SQS), ("mixed-full", {}, RAGGED_SQS),
             ("mixed-causal-prefill", dict(causal=True, prefill=True), RAGGED_SQS), ("mixed-full-prefill", dict(prefill=True), RAGGED_SQS),
             ("uniform1-causal", dict(causal=True), (1,) * 7), ("uniform2-window", dict(window=(15, 0), causal=True), (2,) * 7),
             ("uniform5-causal-prefill", dict(causal=True, prefill=True), (5,) * 7), ("mixed-window-causal", dict(window=(64, 0), causal=True), RAGGED_SQS))
    out = []
    for i, (name, kw, sqs) in enumerate(kinds):
        ax = _axes(i)
        ent = ragged_entries(ax["cap"], ax["append"], sqs)
        out.append(Case(family="ragged", name=f"ragged/{name}", lens=tuple(e[1] for e in ent), sq=tuple(e[0] for e in ent), ragged=True, **kw, **ax))
    # more than 512 sequences: the second round of the slot lookup's prefix sum
    sqs = tuple((0, 1, 2, 5, 1, 17, 1, 3)[i % 8] for i in range(520))
    lens = tuple(min(64, (7 * i) % 66 + (s if i % 3 else 0)) for i, s in enumerate(sqs))
    lens = tuple(max(L, s) for L, s in zip(lens, sqs))
    out.append(Case(family="ragged", name="ragged/520-sequences", lens=lens, sq=sqs, ragged=True, causal=True, append=True, cap=64, h=6, hk=2, dtype="bf16", splits=1))
    return out


@lru_cache(maxsize=None)
def kv_families():
    fams = {
        "plain": _plain_cases(),
        "window": _window_cases(),
        "softcap": _plain_cases("softcap", thin=3, softcap=SOFTCAP) + _window_cases("softcap", thin=3, softcap=SOFTCAP),
        "sinks": _sink_cases(),
        "tree": _tree_cases(),
        "prefill": _prefill_cases(),
        "d256": _d256_cases(),
        "ragged": _ragged_cases(),
    }
    names = [c.name for cs in fams.values() for c in cs]
    assert len(names) == len(set(names))
    return fams


def kv_cases(family):
    return kv_families()[family]


# ---- parameter tables of tests/test_kvcache_routes_gpu.py: one case per leaf of the launch dispatch --------------------------------------

ROUTE_CAP = 96                          # three 32-key steps: a forced split of 2 is real
ROUTE_LENS = (0, 31, 33, 70, 96)
ROUTE_FAMILIES = ("plain", "causal", "window", "softcap", "sinks", "tree", "prefill", "prefill_causal", "d256_causal", "d256_window", "d256_softcap", "append")
_ROUTE_KW = {
    "plain": {}, "causal": dict(causal=True), "window": dict(window=(5, 0)), "softcap": dict(causal=True, softcap=SOFTCAP), "sinks": dict(causal=True, sink="zero"),
    "tree": {}, "prefill": dict(prefill=True), "prefill_causal": dict(prefill=True, causal=True),
    "d256_causal": dict(causal=True), "d256_window": dict(window=(5, 0)), "d256_softcap": dict(causal=True, softcap=SOFTCAP), "append": dict(causal=True, append=True),
}


@lru_cache(maxsize=None)
def route_cases(family):
    """The common axes CROSSED, where the families above rotate them: dense / ragged x dtype x head_dim x layout x cache width x num_splits, at
    the smallest shapes at which a wrong leaf still shows - h / h_k = 2 / 1 (rows packed across heads), sq = 3 (ragged: 1 and 3; the 64-row
    kernels: 63 and 65), every length of ROUTE_LENS in one call.  `append` is not a kernel family: the causal call with its rows appended,
    for the leaves of the append launch."""
    kw = _ROUTE_KW[family]
    wide = "prefill" in family
    out = []
    for ragged, dtype, d, page, fp8, splits in itertools.product((False, True), DTYPES, (256,) if family.startswith("d256") else (64, 128), (0, 16), (False, True), (1, 2)):
        # a ragged call carries both sq in its batch, a dense call has one
        for sqs in ([(63, 65) if wide else (1, 3)] if ragged else [(63,), (65,)] if wide else [(3,)]):
            pairs = [(L, s) for L in ROUTE_LENS for s in sqs]
            if kw.get("append"):
                pairs = [(max(L, s), s) for L, s in pairs]
            tree = tuple(heap_words(s) for _, s in pairs) if family == "tree" else None
            name = f"route-{family}/{'ragged' if ragged else 'dense'}-{dtype}-d{d}-{'paged' if page else 'contig'}-{'fp8' if fp8 else '16bit'}-splits{splits}" + ("" if ragged else f"-sq{sqs[0]}")
            out.append(Case(family="route-" + family, name=name, lens=tuple(p[0] for p in pairs), sq=tuple(p[1] for p in pairs), d=d, dtype=dtype, fp8=fp8, page=page,
                            h=2, hk=1, splits=splits, tree=tree, ragged=ragged, cap=ROUTE_CAP, **kw))
    return out


def route_leaf(c):
    """the attention kernel a route case must run, as the launch layer keys it: (file, dense / ragged, dtype, head_dim, layout, cache width[, mode]).
    mode is there only where the file has an instantiation per mask; a split call with sinks runs the causal kernel of the call without them."""
    if c.d == 256:
        file, mode = "d256", "softcap" if c.softcap else "window"
    elif c.prefill:
        file, mode = "prefill", c.causal
    elif c.softcap:
        file, mode = "softcap", None
    elif c.sink is not None and c.splits == 1:
        file, mode = "sinks", None
    elif c.tree is not None:
        file, mode = "tree", None
    else:
        file, mode = "ragged" if c.ragged else "dense", "window" if c.window != (-1, -1) else "causal" if c.causal else "plain"
    return (file, c.ragged, c.dtype, c.d, bool(c.page), c.fp8, mode)


# ---- sensitivity: one parameter moved by one, at the largest length of each family -------------------------------------------------------

def sensitivity_pairs():
    """(name, base case, moved case): the moved call must decode to the model of the MOVED parameters, and differ from the model of the base
    exactly on the rows whose visible sets differ"""
    cap = 1024
    L = (cap - 1, cap - 2, 517, cap - 1)
    pairs = []

    def add(name, base, **moved):
        pairs.append((name, base, replace(base, name=base.name + "+moved", **moved)))

    def longer(c, i=0):
        return dict(lens=tuple(x + (j == i) for j, x in enumerate(c.lens)))

    def flip(c, i, t, bit):
        return dict(tree=tuple(tuple(x ^ (1 << bit) if (j, u) == (i, t) else x for u, x in enumerate(w)) for j, w in enumerate(c.tree)))

    base = _dense("sens", "plain", L, 5, h=4, hk=1, splits=3)
    add("plain: one length + 1", base, **longer(base))
    base = _dense("sens", "causal", L, 17, causal=True, h=3, hk=1, dtype="bf16", splits=0)
    add("causal: one length + 1", base, **longer(base, 1))
    base = _dense("sens", "window", L, 5, window=(500, 2), h=4, hk=2, splits=2)
    add("window: left + 1", base, window=(501, 2))
    add("window: right + 1", base, window=(500, 3))
    base = _dense("sens", "window-causal", L, 3, window=(100, 0), causal=True, h=5, hk=1, dtype="bf16", fp8=True, page=16, splits=5)
    add("causal window: left + 1", base, window=(101, 0))
    base = _dense("sens", "softcap", L, 5, window=(500, 1), softcap=SOFTCAP, h=4, hk=1)
    add("softcap: left + 1", base, window=(501, 1))
    add("softcap: right + 1", base, window=(500, 2))
    base = _dense("sens", "sinks-unsplit", L, 2, window=(500, 0), causal=True, sink="zero", h=4, hk=1)
    add("sinks, unsplit: left + 1", base, window=(501, 0))
    base = _dense("sens", "sinks-split", L, 2, causal=True, sink="zero", h=4, hk=1, splits=3, page=256)
    add("sinks, split: one length + 1", base, **longer(base, 3))
    base = _dense("sens", "tree", L, 33, tree=(heap_words(33),) * 4, h=4, hk=1, splits=2)
    add("tree: one bit flipped", base, **flip(base, 0, 20, 7))
    add("tree: one length + 1", base, **longer(base, 2))
    base = _dense("sens", "prefill", L, 65, causal=True, prefill=True, h=4, hk=1, splits=3)
    add("prefill: one length + 1", base, **longer(base))
    base = _dense("sens", "d256", L, 5, d=256, window=(500, 2), h=4, hk=1, fp8=True)
    add("d256: left + 1", base, window=(501, 2))
    add("d256: right + 1", base, window=(500, 3))
    base = Case(family="sens", name="sens/ragged", lens=L + (40, 1023), sq=(1, 5, 17, 0, 40, 2), ragged=True, window=(500, 1), h=4, hk=1)
    add("ragged: left + 1", base, window=(501, 1))
    add("ragged: one length + 1", base, **longer(base, 5))
    return pairs


# ---- parameter tables of tests/test_attention_visibility_gpu.py ---------------------------------------------------------------------------

ATTN_SK = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1023, 1024)
ATTN_SQ = (1, 2, 63, 64, 65, 255, 256, 257, 300, 513)
ATTN_HEADS = ((2, 2), (4, 1), (6, 1))           # h / h_k = 1, 4 and 6 / 1


def attn_pairs(causal):
    """causal: every (sq, sk) pair of the table, sq > sk included (its first rows are dead); non-causal: the table's diagonal, which visits
    every sk and every sq"""
    if causal:
        return list(itertools.product(ATTN_SQ, ATTN_SK))
    return [(ATTN_SQ[i % len(ATTN_SQ)], sk) for i, sk in enumerate(ATTN_SK)]


def attn_case(sq, sk, causal, d, dtype, heads):
    """fwd / varlen_fwd as a Case: L = sk for every sequence, no window, capacity = the code's"""
    h, hk = heads
    return Case(family="attn", name=f"attn/sq{sq}-sk{sk}-{'causal' if causal else 'full'}-d{d}-{dtype}-h{h}_{hk}", lens=(sk,), sq=(sq,), d=d, dtype=dtype,
                h=h, hk=hk, causal=causal, cap=1024)


def attn_packed(causal, d, dtype, heads, equal):
    """one varlen_fwd call: the lengths of the tables as sequences, empty ones among them (skewed: the compact grid), or eight sequences of
    64 x 64 (equal lengths: the plain grid)"""
    h, hk = heads
    if equal:
        pairs = [(64, 64)] * 8
    else:
        pairs = attn_pairs(False) + [(0, 64), (65, 0), (0, 0), (513, 1), (300, 255), (2, 1024), (257, 256), (64, 65)]
    return Case(family="attn", name=f"attn/packed-{'equal' if equal else 'skewed'}-{'causal' if causal else 'full'}-d{d}-{dtype}-h{h}_{hk}", lens=tuple(p[1] for p in pairs),
                sq=tuple(p[0] for p in pairs), d=d, dtype=dtype, h=h, hk=hk, causal=causal, cap=1024, ragged=True)


def all_gpu_cases():
    """every Case the two GPU modules run, for the CPU tests"""
    cases = [c for cs in kv_families().values() for c in cs]
    for _, base, moved in sensitivity_pairs():
        cases += [base, moved]
    for i, (d, dtype) in enumerate(itertools.product((64, 128), DTYPES)):
        for causal in (True, False):
            cases += [attn_case(sq, sk, causal, d, dtype, ATTN_HEADS[(j + i) % 3]) for j, (sq, sk) in enumerate(attn_pairs(causal))]
            cases += [attn_packed(causal, d, dtype, ATTN_HEADS[(i + causal + e) % 3], bool(e)) for e in (0, 1)]
    return cases


# ---- THE BACKWARD PROBE (tests/test_attention_backward_visibility_gpu.py) ---------------------------------------------
#
# bwd / varlen_bwd take O and LSE as ARGUMENTS, and the kernels use them in two places only: P = exp2(s * c - lse * log2e) and
# D = rowsum(dO * O).  With lse = 0, O = 0 and every score exactly 0 (Q = 0 or K = 0), P is exactly 1 on every (row, key) pair a kernel
# treats as visible and 0 elsewhere, D = 0 and dS = P * dP.  V = 1 in every column and dO_t = code(t), the two-digit one-hot code of the
# query row's index in its sequence, make dP = dO_t . V_j = 2 exactly.  Two calls per case:
#   A: Q = 0, K_j = code(j):  dQ_t = scale * 2 * hist_keys(t),  dV_j = sum over the group's hot query heads of hist_rows(j),  dK = 0
#   B: K = 0, Q_t = code(t):  dK_j = scale * 2 * sum over the hot heads of hist_rows(j),  dV as in A,  dQ = 0
# hist_keys(t) = the digit histogram of the keys row t sees (`visible`), hist_rows(j) = that of the rows that see key j (`rows_seeing`,
# the transpose in closed form).  Every gradient is a small integer (times scale), held exactly by the fp32 accumulators.
#
# HOT HEADS.  hot = None: every query head carries dO (and Q in call B), every KV head K / V: a group's dK / dV is ratio x hist, which
# pins that every head is counted once in total.  hot = g: query head g alone carries dO (and Q), its KV head alone K / V; every other
# head holds zeros and must come back exactly 0, the hot ones exactly 1 x hist: which head, not only how many.
#
# The code is `codes(64, 1024)`, base 32, on the first 64 columns at EVERY head_dim (the other columns of d = 128 are 0 and must come
# back 0): up to 1024 rows or keys, at most 32 of them share a digit, which keeps the integers small enough for bf16.
#
# CONDITIONS, derived and asserted on the inputs (`bwd_check_conditions`), never used to drop a case:
#   * every expected integer (dQ: 2 m, dK: 2 x hot heads of the group x m, dV: hot heads x m; m <= 32 the largest digit count) is at most
#     256 in bf16 and 2048 in fp16: every integer up to there is exact in the type, so a count one off cannot round back;
#   * d = 64: scale = 1 / 8, a power of two - everything is exact and the outputs are compared as bits;
#   * d = 128: scale = fp32(1 / sqrt(128)) is not a power of two.  A kernel returns x = round16(fp32(N * scale)) (one fp32 product, one
#     rounding to 16 bits: the epilogues and fa_bwd_sum_splits_kernel), so |x / scale - N| <= (2^(e - p) + 2^(e - 24)) / scale with
#     e = floor(log2(N * scale)) and p = 11 (fp16), 8 (bf16) significant bits; required below 0.25: N <= 724 in fp16, N <= 90 in bf16.
# The tables choose hot = None where 2 x ratio x 32 meets these and rotate the single hot head through the group's positions where it
# does not (bf16: ratio 6 at d = 64, ratios 4 and 6 at d = 128), so every (sq, sk) runs at every ratio in both types.
#
# WHAT IT DOES NOT SEE: swaps invisible to both digits (as in the forward); the value path (operands are 0 / 1 / 2); a use of O or LSE
# other than the two above that cancels at O = 0, LSE = 0.

BWD_BASE = 32
BWD_CAP = 1024
BWD_INT_EXACT = {"fp16": 2048, "bf16": 256}          # every integer up to here is exact in the type
BWD_SIG_BITS = {"fp16": 11, "bf16": 8}
BWD_GQA_HEADS = ((4, 1), (6, 1), (8, 2))             # the group split needs a group
BWD_BATCH = 2


def bwd_scale(d):
    """the kernels' softmax scale, 1.0f / sqrtf((float)d), as a Python float"""
    return float(np.float32(1.0) / np.sqrt(np.float32(d)))


def bwd_decode_error(n, dtype, d):
    """upper bound of |x / scale - n| for x = round16(fp32(n * scale)): 0 where scale is a power of two"""
    import math

    s = bwd_scale(d)
    if n == 0 or math.frexp(s)[0] == 0.5:
        return 0.0
    e = math.floor(math.log2(n * s))
    return (2.0 ** (e - BWD_SIG_BITS[dtype]) + 2.0 ** (e - 24)) / s


@lru_cache(maxsize=None)
def bwd_int_limit(dtype, d):
    """the largest N such that every integer up to N is exact in the type and decodes with an error below 0.25"""
    n = 0
    while n < BWD_INT_EXACT[dtype] and bwd_decode_error(n + 1, dtype, d) < 0.25:
        n += 1
    return n


@lru_cache(maxsize=None)
def bwd_code(d):
    """int64 (1024, d): row i = the code of query row or key i of its sequence"""
    c = np.zeros((BWD_CAP, d), dtype=np.int64)
    c[:, : 2 * BWD_BASE] = codes(2 * BWD_BASE, BWD_CAP)
    c.setflags(write=False)
    return c


@lru_cache(maxsize=None)
def _bwd_prefix(d):
    p = np.zeros((BWD_CAP + 1, d), dtype=np.int64)
    np.cumsum(bwd_code(d), axis=0, out=p[1:])
    return p


def rows_seeing(L, sq, j, causal=False):
    """The transpose of `visible` without window or tree: the query rows of a sequence with L keys and sq rows that see key j, a range.
    j < L, and under the bottom-right causal mask j <= L - sq + t, i.e. t >= j - (L - sq)."""
    L = max(int(L), 0)
    if not 0 <= j < L:
        return range(0)
    lo = max(0, j - (L - sq)) if causal else 0
    return range(lo, max(lo, sq))


@lru_cache(maxsize=32)
def _seq_hists(L, sq, causal, d):
    """hist_keys int64 (sq, d) and hist_rows int64 (L, d) of one sequence"""
    p = _bwd_prefix(d)
    vis = [visible(L, sq, t, causal)[0] for t in range(sq)]
    seen = [rows_seeing(L, sq, j, causal) for j in range(L)]
    hk = p[[r.stop for r in vis]] - p[[r.start for r in vis]] if sq else np.zeros((0, d), dtype=np.int64)
    hr = p[[r.stop for r in seen]] - p[[r.start for r in seen]] if L else np.zeros((0, d), dtype=np.int64)
    return hk, hr


def bwd_head_weights(c, hot):
    """wq int64 (h,): 1 on the hot query heads; cnt int64 (hk,): the hot query heads of each KV head's group"""
    wq = np.ones(c.h, dtype=np.int64) if hot is None else np.eye(c.h, dtype=np.int64)[hot]
    return wq, wq.reshape(c.hk, c.ratio).sum(axis=1)


def bwd_check_conditions(c, hot, n_max):
    """the preconditions of the probe and its derived conditions, on the inputs; n_max = (dQ, dK, dV) largest expected integers"""
    assert c.d in (64, 128) and c.dtype in DTYPES and c.window == (-1, -1) and c.tree is None and not c.fp8 and c.cap == BWD_CAP
    assert len(c.lens) == len(c.sq) and all(0 <= L <= BWD_CAP for L in c.lens) and all(0 <= s <= BWD_CAP for s in c.sq)
    assert c.h % c.hk == 0 and (hot is None or 0 <= hot < c.h)
    assert max(n_max) <= BWD_INT_EXACT[c.dtype], f"{c.name}: an expected integer {max(n_max)} is not exact in {c.dtype}"
    err = bwd_decode_error(max(n_max[:2]), c.dtype, c.d)
    assert err < 0.25, f"{c.name}: {max(n_max[:2])} x scale decodes with an error up to {err:.3f} in {c.dtype} at d = {c.d}"


def expected_bwd(c, hot, call):
    """-> (dQ int64 (Rq, h, d), dK int64 (Rk, hk, d), dV int64 (Rk, hk, d)), rows [(i, t)], keys [(i, j)]: the model's integers of call
    "A" or "B" in packed (sequence, row) and (sequence, key) order; dQ and dK are in units of scale"""
    hists = [_seq_hists(L, s, c.causal, c.d) for L, s in zip(c.lens, c.sq)]
    hk = np.concatenate([x[0] for x in hists])
    hr = np.concatenate([x[1] for x in hists])
    wq, cnt = bwd_head_weights(c, hot)
    dq = 2 * hk[:, None, :] * wq[None, :, None]
    dk = 2 * hr[:, None, :] * cnt[None, :, None]
    dv = hr[:, None, :] * cnt[None, :, None]
    bwd_check_conditions(c, hot, (int(dq.max(initial=0)), int(dk.max(initial=0)), int(dv.max(initial=0))))
    if call == "A":
        dk = np.zeros_like(dk)
    else:
        assert call == "B"
        dq = np.zeros_like(dq)
    rows = [(i, t) for i, s in enumerate(c.sq) for t in range(s)]
    keys = [(i, j) for i, L in enumerate(c.lens) for j in range(L)]
    return (dq, dk, dv), rows, keys


def decode_bwd(c, grads):
    """(dQ, dK, dV) fp16 / bf16 -> int64 tensors: dQ and dK in units of scale"""
    import torch

    s = bwd_scale(c.d)
    for name, x in zip(("dQ", "dK", "dV"), grads):
        assert torch.isfinite(x.float()).all().item(), f"{c.name}: non-finite {name} (a read of NaN LSE padding or of memory outside the views)"
    return tuple(torch.round(x.double() / m).long() for x, m in zip(grads, (s, s, 1.0)))


def bwd_mismatch(c, grads, exp):
    """per tensor a bool (R, heads): where the decoded integers differ from the model, an expected 0 is not an exact 0, or - where the
    scale is a power of two - the bits differ"""
    import math

    import torch

    s = bwd_scale(c.d)
    out = []
    for x, dec, e, m in zip(grads, decode_bwd(c, grads), exp, (s, s, 1.0)):
        e = torch.from_numpy(e).to(x.device)
        bad = ((dec != e) | ((e == 0) & (x != 0))).any(dim=-1)                  # (an expected 0 is an exact 0 at every scale)
        if math.frexp(m)[0] == 0.5:
            bad |= (x != (e.double() * m).to(x.dtype)).any(dim=-1)
        out.append(bad)
    return out


def assert_bwd_signature(c, hot, call, grads, exp, rows, keys):
    """integer (and, at a power-of-two scale, bit) equality of every gradient with the model on every (sequence, head, row or key).  The
    message names the first rows / keys that differ with the digit columns that differ."""
    bads = bwd_mismatch(c, grads, exp)
    if not any(b.any().item() for b in bads):
        return
    dec = decode_bwd(c, grads)
    msgs, total = [], 0
    for name, what, index, lens, bad, x, d_int, e in zip(("dQ", "dK", "dV"), ("row", "key", "key"), (rows, keys, keys), (c.sq, c.lens, c.lens), bads, grads, dec, exp):
        total += int(bad.sum())
        for r, g in bad.nonzero()[:4].tolist():
            i, t = index[r]
            diff = np.flatnonzero(d_int[r, g].cpu().numpy() != e[r, g])[:12]
            cols = {(f"lo{k}" if k < BWD_BASE else f"hi{k - BWD_BASE}" if k < 2 * BWD_BASE else f"pad{k}"): (int(e[r, g, k]), int(d_int[r, g, k])) for k in diff}
            msgs.append(f"{name} seq {i} (L={c.lens[i]}, sq={c.sq[i]}) head {g} {what} {t}: digit counts (expected, decoded) that differ: {cols or 'none (the bits differ)'}")
    raise AssertionError(f"{c.name} call {call} hot={hot}: {total} (row or key, head) signatures differ from the model [{c}]\n  " + "\n  ".join(msgs))


def bwd_inputs(c, hot, call, dev):
    """The probe's operands in packed order with three rows of the bad code behind each: q, do (Rq + 3, h, d) and k, v (Rk + 3, hk, d) in the
    case's dtype.  Cold heads are 0.  (A dense call repeats the one sequence over its batch and slices the tail off per entry.)"""
    import torch

    dt = torch_dtype(c.dtype)
    code = torch.from_numpy(bwd_code(c.d).copy()).to(dev).to(dt)
    wq, cnt = bwd_head_weights(c, hot)
    wq = torch.from_numpy(wq).to(dev).to(dt).view(1, c.h, 1)
    wk = torch.from_numpy((cnt > 0).astype(np.int64)).to(dev).to(dt).view(1, c.hk, 1)
    rq = torch.cat([torch.arange(s, device=dev) for s in c.sq] + [torch.zeros(0, dtype=torch.long, device=dev)])
    rk = torch.cat([torch.arange(L, device=dev) for L in c.lens] + [torch.zeros(0, dtype=torch.long, device=dev)])

    def behind(x):
        return torch.cat([x, torch.full((3,) + tuple(x.shape[1:]), BAD, dtype=dt, device=dev)])

    do = code[rq].unsqueeze(1) * wq
    v = torch.ones(len(rk), 1, c.d, dtype=dt, device=dev) * wk
    if call == "A":
        q, k = torch.zeros_like(do), code[rk].unsqueeze(1) * wk
    else:
        q, k = do.clone(), torch.zeros_like(v)
    return behind(q), behind(k), behind(v), behind(do)


# ---- parameter tables of tests/test_attention_backward_visibility_gpu.py ------------------------------------------------------------------

def bwd_hot(heads, dtype, d, j):
    """None (every head hot) where the group sum 2 x ratio x 32 meets the derived conditions, else the single hot head, rotated by j"""
    h, hk = heads
    return None if 2 * (h // hk) * BWD_BASE <= bwd_int_limit(dtype, d) else j % h


def _cfg(d, dtype):
    return (d == 128) * 2 + DTYPES.index(dtype)


def bwd_dense_cases(d, dtype, causal, gqa=False):
    """[(Case, hot)].  gqa = False (bwd of the host module): every (sq, sk) of attn_pairs, h / h_k rotating through ATTN_HEADS.  gqa = True
    (the C ABI with and without a workspace): every third pair, the phase rotated over (d, dtype, causal), h / h_k through BWD_GQA_HEADS."""
    i = _cfg(d, dtype)
    pairs = attn_pairs(causal)
    if gqa:
        pairs = pairs[(i + causal) % 3:: 3]
    table = BWD_GQA_HEADS if gqa else ATTN_HEADS
    out = []
    for n, (sq, sk) in enumerate(pairs):
        heads = table[(n + i) % 3]
        out.append((attn_case(sq, sk, causal, d, dtype, heads), bwd_hot(heads, dtype, d, n // 3)))       # (n // 3: a shape recurs every third case)
    return out


def bwd_packed_case(d, dtype, causal, equal, gqa=False):
    i = _cfg(d, dtype)
    heads = (BWD_GQA_HEADS if gqa else ATTN_HEADS)[(i + causal + equal) % 3]
    return attn_packed(causal, d, dtype, heads, equal), bwd_hot(heads, dtype, d, i + 2 * causal + equal)


HEAD_SHAPES = ((2, 2), (4, 1), (6, 1), (8, 2))         # h / h_k = 1, 4, 6, and 4 over two KV heads


def bwd_head_cases(d, dtype, causal, split):
    """[(Case, hot)]: every head position of every shape hot once, on a dense call (three 128-key blocks, five 64-row tiles, a 44-key offset
    of the diagonal) and on a packed one with an empty sequence on either side.  The group split needs a group: no h / h_k = 1 then."""
    out = []
    for heads in HEAD_SHAPES[1:] if split else HEAD_SHAPES:
        for g in range(heads[0]):
            out.append((attn_case(257, 301, causal, d, dtype, heads), g))
            pairs = ((64, 65), (0, 64), (130, 257), (65, 0), (129, 70))
            out.append((Case(family="attn", name=f"attn/head-packed-{'causal' if causal else 'full'}-d{d}-{dtype}-h{heads[0]}_{heads[1]}", lens=tuple(p[1] for p in pairs),
                             sq=tuple(p[0] for p in pairs), d=d, dtype=dtype, h=heads[0], hk=heads[1], causal=causal, cap=1024, ragged=True), g))
    return out


def bwd_sensitivity_pairs():
    """(name, base, moved, hot): one length moved by one at the largest shapes of the tables, packed with a second sequence"""
    def mk(name, sqs, lens, causal, d, dtype, heads):
        return Case(family="attn", name=f"attn/bwd-sens-{name}", lens=tuple(lens), sq=tuple(sqs), d=d, dtype=dtype, h=heads[0], hk=heads[1], causal=causal, cap=1024, ragged=True)

    out = []
    for k, (name, sqs, lens, moved_sq, moved_len, causal) in enumerate((
            ("causal-key+1", (513, 300), (1023, 257), (513, 300), (1024, 257), True),
            ("causal-key-1", (513, 300), (1023, 257), (513, 300), (1023, 256), True),
            ("causal-row+1", (512, 257), (1024, 300), (513, 257), (1024, 300), True),
            ("causal-row+1-dead", (512, 257), (1024, 256), (512, 258), (1024, 256), True),
            ("full-key+1", (513, 64), (1023, 129), (513, 64), (1024, 129), False),
            ("full-row+1", (512, 64), (1024, 129), (513, 64), (1024, 129), False))):
        d, dtype = ((64, "fp16"), (128, "bf16"), (128, "fp16"), (64, "bf16"))[k % 4]
        heads = ATTN_HEADS[k % 3]
        out.append((name, mk(name, sqs, lens, causal, d, dtype, heads), mk(name + "-moved", moved_sq, moved_len, causal, d, dtype, heads), bwd_hot(heads, dtype, d, k)))
    return out


def all_bwd_gpu_cases():
    """every (Case, hot) tests/test_attention_backward_visibility_gpu.py runs, for the CPU tests"""
    cases = []
    for d, dtype, causal in itertools.product((64, 128), DTYPES, (True, False)):
        cases += bwd_dense_cases(d, dtype, causal) + bwd_dense_cases(d, dtype, causal, gqa=True)
        for equal in (False, True):
            cases += [bwd_packed_case(d, dtype, causal, equal), bwd_packed_case(d, dtype, causal, equal, gqa=True)]
        for split in (False, True):
            cases += bwd_head_cases(d, dtype, causal, split)
    for _, base, moved, hot in bwd_sensitivity_pairs():
        cases += [(base, hot), (moved, hot)]
    return cases
