"""GPU: the top-k selection with one logits row spread over several workgroups (flash_mla_indexer_topk(num_splits = n), fa_run_mla_indexer_topk_v2).  The work is
integer, so every check is equality of the WHOLE int32 buffer: with a five-line numpy reference and with the num_splits = 1 call."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import flash_attn_turing as F
from flash_attn_turing import capi

pytestmark = pytest.mark.gpu

CAP, PAD = 4160, 32                             # capacity: a multiple of 64 but of no chunk size; the logits are a view of rows CAP + PAD apart
NAN = 0x7FC00000                                # a NaN with the sign bit clear: the largest key
# (b, sq) -> cache_seqlens(topk).  (2, 3) causal: n_t = topk - 1, topk, topk + 1 and CAP - 2, CAP - 1 (odd), CAP; (1, 1): 64 chunks over 2101 entries leaves 31 empty
SHAPES = {(1, 1): lambda topk: [2101], (2, 3): lambda topk: [topk + 1, CAP]}


def _bits(family, rng):
    """fp32 bit patterns of one row of CAP logits"""
    j = np.arange(CAP)
    if family == "normal":
        return rng.standard_normal(CAP).astype(np.float32).view(np.uint32)
    if family == "equal":                       # the answer is 0 .. topk - 1
        return np.full(CAP, 1.5, np.float32).view(np.uint32)
    if family == "three":                       # a third of each value, interleaved: the threshold ties lie in every chunk and r ends inside one
        return np.choose(j % 3, [-1.0, 0.25, 7.0]).astype(np.float32).view(np.uint32)
    if family == "ulps":                        # 1 + k 2^-23: all share the first 12 key bits, half of them the first 22 as well
        k = np.where(j % 2 == 0, rng.integers(0, 1 << 20, CAP), rng.integers(0, 1 << 10, CAP))
        return (0x3F800000 + k).astype(np.uint32)
    v = -np.abs(rng.standard_normal(CAP)).astype(np.float32)            # "specials": negatives, both zeros, both infinities and a NaN among the first entries
    v[j % 11 == 3], v[j % 11 == 7] = -0.0, 0.0
    v[5], v[17], v[18] = np.inf, -np.inf, np.inf
    b = v.view(np.uint32).copy()
    b[9] = NAN
    return b


@functools.lru_cache(maxsize=None)
def _case(family, shape, topk):
    """(logits bits (b, sq, CAP + PAD), lengths, reference (b, sq, topk)): every entry at j >= n_t holds NAN, so any read past n_t changes the answer"""
    b, sq = shape
    rng = np.random.default_rng([sorted(SHAPES).index(shape), topk, len(family)])
    lens = SHAPES[shape](topk)
    buf = np.full((b, sq, CAP + PAD), NAN, np.uint32)
    ref = np.full((b, sq, topk), -1, np.int32)
    for i in range(b):
        for t in range(sq):
            n = min(lens[i], max(lens[i] - sq + t + 1, 0))
            x = _bits(family, rng)[:n]
            buf[i, t, :n] = x
            u = x ^ np.where(x >> 31 != 0, 0xFFFFFFFF, 0x80000000).astype(np.uint32)
            order = np.lexsort((np.arange(n), -u.astype(np.int64)))
            sel = np.sort(order[:topk]) if n > topk else np.arange(n)
            ref[i, t, :len(sel)] = sel
    return buf, lens, ref


@pytest.mark.parametrize("family", ["normal", "equal", "three", "ulps", "specials"])
@pytest.mark.parametrize("num_splits", [2, 3, 7, 16, 64])
def test_every_split_count_gives_the_reference_in_every_word(gpu, num_splits, family):
    for shape in SHAPES:
        for topk in (32, 2048):
            buf, lens, ref = _case(family, shape, topk)
            logits = torch.from_numpy(buf.view(np.float32)).to(gpu)[:, :, :CAP]
            dl = torch.tensor(lens, dtype=torch.int32, device=gpu)
            got = F.flash_mla_indexer_topk(logits, dl, topk, causal=True, num_splits=num_splits)
            again = F.flash_mla_indexer_topk(logits, dl, topk, causal=True, num_splits=num_splits)
            one = F.flash_mla_indexer_topk(logits, dl, topk, causal=True, num_splits=1)
            assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), ref), (shape, topk)
            assert torch.equal(got, one) and torch.equal(got, again), (shape, topk)


def test_a_callers_workspace_may_hold_anything_and_be_reused(gpu):
    topk, shape = 2048, (2, 3)
    ws, idx = None, torch.empty(2, 3, topk, dtype=torch.int32, device=gpu)
    for family in ("normal", "three"):          # the second call finds what the first left
        buf, lens, ref = _case(family, shape, topk)
        logits = torch.from_numpy(buf.view(np.float32)).to(gpu)[:, :, :CAP]
        dl = torch.tensor(lens, dtype=torch.int32, device=gpu)
        p = capi.mla_topk_params_v2(logits, idx, dl, causal=True, num_splits=7)
        need = capi.mla_topk_workspace_bytes(p)
        if ws is None:
            ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=gpu)
        p.workspace, p.workspace_bytes = ws.data_ptr(), need
        assert need == ws.numel() and capi.mla_topk_num_splits(p) == 7
        idx.fill_(-7)
        capi.run_mla_indexer_topk(p)
        assert np.array_equal(idx.cpu().numpy(), ref), family
        p.workspace_bytes = need - 1            # a forced count the workspace cannot hold
        rc = capi.lib().fa_run_mla_indexer_topk_v2(ctypes.byref(p), None)
        assert rc == capi.FA_ERR_BAD_SHAPE and "workspace_bytes" in capi.last_error(), (rc, capi.last_error())


def test_a_captured_split_call_replays_with_the_data_then_in_memory(gpu):
    topk, shape = 2048, (2, 3)
    cases = [_case(f, shape, topk) for f in ("normal", "three", "specials")]
    logits = torch.from_numpy(cases[0][0].view(np.float32)).to(gpu)[:, :, :CAP]
    dl = torch.tensor(cases[0][1], dtype=torch.int32, device=gpu)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        F.flash_mla_indexer_topk(logits, dl, topk, num_splits=7)       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = F.flash_mla_indexer_topk(logits, dl, topk, num_splits=7)
    for buf, lens, ref in cases + cases[:1]:    # several replays, each on other data
        logits.copy_(torch.from_numpy(buf.view(np.float32))[:, :, :CAP])
        g.replay()
        assert np.array_equal(got.cpu().numpy(), ref)


def test_the_library_rule_beats_one_workgroup_per_row_at_b1_128k(gpu):
    """b 1, L 131072, topk 2048: num_splits = 0 against num_splits = 1 timed twice (A1, A2), medians of 5 interleaved rounds.  The auto call must be faster than
    min(A1, A2) by more than |A1 - A2|: it beats the one-workgroup kernel by more than that kernel differs from itself.  Measured: 27.7 us against 85.2 / 85.2 us,
    ratio 0.33 (profiles/mla_topk_split_bench.log)."""
    L, topk = 131072, 2048
    logits = torch.randn(1, 1, L, generator=torch.Generator().manual_seed(7)).to(gpu)
    dl = torch.tensor([L], dtype=torch.int32, device=gpu)
    calls = [lambda n=n: F.flash_mla_indexer_topk(logits, dl, topk, num_splits=n) for n in (0, 1, 1)]
    assert torch.equal(calls[0](), calls[1]())

    def timed(fn, reps=20):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / reps

    for fn in calls:
        timed(fn, 3)
    ts = [[], [], []]
    for _ in range(5):
        for i, fn in enumerate(calls):
            ts[i].append(timed(fn))
    auto, a1, a2 = (float(np.median(t)) * 1e3 for t in ts)
    print(f"num_splits=0 {auto:.1f} us, num_splits=1 {a1:.1f} / {a2:.1f} us, ratio {auto / min(a1, a2):.3f}")
    assert min(a1, a2) - auto > abs(a1 - a2), (auto, a1, a2)
