"""CPU: the visibility probe of tests/_visibility.py decodes what it claims to, on the very inputs the GPU tests use.

  * an emulation of the kernels' arithmetic - an fp32 sum of ones, times an fp32 reciprocal 1 ulp off, one rounding to fp16 / bf16, an
    LSE of float32(log n) 3e-7 (relative) off - goes through the decoder of the GPU tests and must return the model's integers for every
    case of every parameter table of tests/test_kvcache_visibility_gpu.py and tests/test_attention_visibility_gpu.py (so the derived
    conditions - n <= 4096, digit counts <= 64, capacity <= B x B - are checked on the real inputs);
  * every mutation of a visible set a mask bug can make changes the decoded signature, at the largest count used per head_dim;
  * the model agrees with a brute force over (t, j) of the README's inequalities, written a second way;
  * every value of every common axis occurs in every family that supports it."""
import itertools

import numpy as np
import pytest
import torch

import _visibility as V


def emulate(n, hist, extra, dtype, v_scale, sign):
    """n (R,), hist (R, d) int64, extra 0 / 1 -> out (R, 1, d) in the output dtype, lse (R, 1) fp32, as a kernel with the worst allowed
    arithmetic would return them; sign = +1 / -1: the direction of both perturbations"""
    n_tot = torch.from_numpy(n).float() + extra
    live = n_tot > 0
    rcp = torch.where(live, 1.0 / n_tot.clamp(min=1), torch.zeros_like(n_tot))
    rcp = torch.nextafter(rcp, torch.full_like(rcp, float(sign) * 4.0))
    acc = torch.from_numpy(hist).float()                                        # the fp32 sum of P = 1 times V = 0 / 1: exact
    out = (acc * rcp.unsqueeze(1) * np.float32(v_scale)).to(V.torch_dtype(dtype))
    lse = torch.log(n_tot.clamp(min=1).double()).float() * np.float32(1.0 + sign * 3e-7)
    return out.unsqueeze(1), lse.unsqueeze(1)


def roundtrip(c, n, hist, sign=1):
    """the signatures after emulation and decoding, per distinct sink state of the case's heads"""
    res = []
    for extra in sorted(set(c.sink_extra())):
        out, lse = emulate(n, hist, extra, c.dtype, c.v_scale, sign)
        n_dec, hist_dec = V.decode(out, lse, torch.tensor([extra]), c.v_scale)
        res.append((n_dec[:, 0].numpy(), hist_dec[:, 0].numpy()))
    return res


def test_decoder_returns_the_model_on_every_gpu_case():
    cases = V.all_gpu_cases()
    assert len(cases) > 500
    rows = 0
    for k, c in enumerate(cases):
        n, hist, r = V.expected(c)                                              # asserts the derived conditions on the inputs
        rows += len(r)
        for n_dec, hist_dec in roundtrip(c, n, hist, sign=1 if k % 2 else -1):
            assert np.array_equal(n_dec, n) and np.array_equal(hist_dec, hist), c.name
    assert rows > 100000


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("d,cap", [(64, 1024), (128, 4096), (256, 4096)])
def test_decoder_on_every_range_of_the_largest_capacities(d, cap, dtype, extra):
    """every [lo, hi) on a grid of edges that holds every residue mod 32 at both ends of the cache, both perturbation signs"""
    edges = sorted(set(range(0, 70)) | set(range(cap // 2 - 35, cap // 2 + 35)) | set(range(cap - 70, cap + 1)))
    pairs = [(lo, hi) for lo in edges[::3] for hi in edges if hi >= lo]
    n = np.array([hi - lo for lo, hi in pairs], dtype=np.int64)
    hist = np.stack([V.signature(d, cap, (range(lo, hi), ()))[1] for lo, hi in pairs])
    assert hist.max() <= V.MAX_DIGIT and n.max() <= V.MAX_N
    for sign in (1, -1):
        out, lse = emulate(n, hist, extra, dtype, 1.0, sign)
        n_dec, hist_dec = V.decode(out, lse, torch.tensor([extra]))
        assert np.array_equal(n_dec[:, 0].numpy(), n) and np.array_equal(hist_dec[:, 0].numpy(), hist)


def _mutations(lo, hi, cap):
    """name -> (range, extras) or an explicit key LIST (a key may repeat) of a mutated visible set [lo, hi)"""
    keys = list(range(lo, hi))
    step = [j for j in keys if j // 32 == (lo + 40) // 32]                       # one whole 32-key step inside the set
    page = [j for j in keys if j // 16 == (lo + 40) // 16]                       # one whole 16-row page inside the set
    assert len(step) == 32 and len(page) == 16 and lo >= 32 and hi < cap
    return {
        "drop the first key": keys[1:],
        "drop the last key": keys[:-1],
        "add the key below lo": [lo - 1] + keys,
        "add the key at hi": keys + [hi],
        "shift the range by one": [j + 1 for j in keys],
        "count one key twice": keys + [keys[len(keys) // 2]],
        "exchange a 32-key step for one outside": [j for j in keys if j not in step] + list(range(0, 32)),
        "exchange a 32-key step for the one past hi": [j for j in keys if j not in step] + [j - step[0] + (hi + 31) // 32 * 32 for j in step if (hi + 31) // 32 * 32 + 32 <= cap],
        "exchange a 16-row page for one outside": [j for j in keys if j not in page] + list(range(16, 32)),
    }


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("d", [64, 128, 256])
def test_every_mutation_changes_the_decoded_signature(d, dtype, extra):
    """at the largest n the GPU tests use per head_dim (their capacity is 1024 at every head_dim), and at the code's own capacity"""
    for cap in sorted({1024, V.capacity_of(d)}):
        lo, hi = 32, cap - 33
        code = V.codes(d, cap)
        n0, h0 = V.signature(d, cap, (range(lo, hi), ()))
        muts = _mutations(lo, hi, cap)
        for name, keys in muts.items():
            if len(keys) < hi - lo - 1:
                continue                                                        # (the step past hi does not exist at this capacity)
            n = np.array([n0, len(keys)], dtype=np.int64)
            hist = np.stack([h0, code[keys].sum(axis=0)])
            for sign in (1, -1):
                out, lse = emulate(n, hist, extra, dtype, 1.0, sign)
                n_dec, hist_dec = V.decode(out, lse, torch.tensor([extra]))
                assert int(n_dec[0, 0]) == n0 and np.array_equal(hist_dec[0, 0].numpy(), h0)
                assert int(n_dec[1, 0]) != n0 or not np.array_equal(hist_dec[1, 0].numpy(), h0), f"{name} is invisible at d={d} cap={cap}"
        assert sum(len(k) >= hi - lo - 1 for k in muts.values()) >= 8


@pytest.mark.parametrize("d", [64, 128])
def test_one_tree_bit_flipped_changes_the_decoded_signature(d):
    cap, sq, L = 1024, 64, 1024
    words = V.heap_words(sq)
    for t, bit in itertools.product((0, 31, 63), (0, 1, 31, 32, 62, 63)):
        sigs = []
        for w in (words[t], words[t] ^ (1 << bit)):
            n, h = V.signature(d, cap, V.visible(L, sq, t, tree_word=w))
            out, lse = emulate(np.array([n]), h[None], 0, "bf16", 1.0, 1)
            n_dec, hist_dec = V.decode(out, lse, torch.tensor([0]))
            assert int(n_dec[0, 0]) == n and np.array_equal(hist_dec[0, 0].numpy(), h)
            sigs.append((n, tuple(h)))
        assert sigs[0] != sigs[1]


def test_dead_rows_and_one_key_rows_are_told_apart():
    d, cap = 64, 1024
    n = np.array([0, 1, 1], dtype=np.int64)
    hist = np.stack([np.zeros(d, dtype=np.int64), V.codes(d, cap)[0], V.codes(d, cap)[777]])
    out, lse = emulate(n, hist, 0, "fp16", 1.0, 1)
    assert (lse == 0).all()
    n_dec, hist_dec = V.decode(out, lse, torch.tensor([0]))
    assert n_dec[:, 0].tolist() == [0, 1, 1] and np.array_equal(hist_dec[:, 0].numpy(), hist)
    out, lse = emulate(n, hist, 1, "fp16", 1.0, 1)                              # with a sink of 0.0 a dead row is O = 0, LSE = sink = 0
    n_dec, hist_dec = V.decode(out, lse, torch.tensor([1]))
    assert n_dec[:, 0].tolist() == [0, 1, 1] and np.array_equal(hist_dec[:, 0].numpy(), hist)


def _brute(L, sq, t, causal, left, right, word):
    """the README's inequalities over every j, written on the offset of the key from the row's diagonal"""
    keys = set()
    for j in range(L):
        off = j - (L - sq + t)                                                  # 0 = the row's own position, bottom-right aligned
        if word is not None:
            u = j - (L - sq)
            if u < 0 or (u < sq and word & (1 << u)):
                keys.add(j)
            continue
        if causal and off > 0:
            continue
        if left != -1 and -off > left:
            continue
        if not causal and right != -1 and off > right:
            continue
        keys.add(j)
    return keys


def test_model_against_brute_force():
    rng = np.random.default_rng(5)
    checked = 0
    for L, sq, causal, left, right in itertools.product((0, 1, 2, 5, 9, 33, 40), (1, 2, 5, 9, 17), (False, True), (-1, 0, 1, 3, 8, 40), (-1, 0, 2, 7)):
        for t in range(sq):
            assert V.visible_set(L, sq, t, causal, (left, right)) == _brute(L, sq, t, causal, left, right, None), (L, sq, t, causal, left, right)
        checked += 1
    for L, sq in itertools.product((0, 1, 5, 33, 63, 64, 65, 100), (1, 2, 17, 33, 63, 64)):
        masks = [0, (1 << 64) - 1, 1 << 63, 1 << (sq - 1)] + [int(x) for x in rng.integers(0, 1 << 64, size=3, dtype=np.uint64)]
        for t, w in itertools.product((0, sq // 2, sq - 1), masks):
            assert V.visible_set(L, sq, t, tree_word=w) == _brute(L, sq, t, False, -1, -1, w), (L, sq, t, hex(w))
        checked += 1
    assert checked > 300


def test_heap_words_are_tree_mask_from_parents():
    from flash_attn_turing import tree_mask_from_parents

    for sq in V.TREE_SQS:
        parents = torch.tensor([[(t - 1) // 2 if t else -1 for t in range(sq)]])
        words = [int(x) & ((1 << 64) - 1) for x in tree_mask_from_parents(parents)[0].tolist()]
        assert tuple(words) == V.heap_words(sq)


def test_every_axis_value_occurs_in_every_family():
    fams = V.kv_families()
    for name, cases in fams.items():
        seen = lambda f: {f(c) for c in cases}
        assert seen(lambda c: c.dtype) == set(V.DTYPES), name
        assert seen(lambda c: c.fp8) == {False, True}, name
        assert seen(lambda c: c.page) == set(V.PAGES), name
        assert seen(lambda c: c.append) == {False, True}, name
        steps = {c.cap // 32 for c in cases}
        assert {1, 2, 3, 5, 0} <= seen(lambda c: c.splits) and seen(lambda c: c.splits) & steps, name
        if name == "prefill":
            assert seen(lambda c: c.ratio) == set(V.PREFILL_RATIOS), name
        else:
            assert set(V.RATIOS) <= seen(lambda c: c.ratio), name
        if name != "d256":
            assert seen(lambda c: c.d) == {64, 128}, name
    sq_of = lambda name: {c.sq[0] for c in fams[name] if not c.ragged}
    assert sq_of("plain") == set(V.SQS) and sq_of("tree") == set(V.TREE_SQS) and sq_of("prefill") == set(V.PREFILL_SQS)
    win = [c for c in fams["window"]]
    assert {c.window[0] for c in win} == set(V.LEFTS) and {c.window[1] for c in win if not c.causal} == set(V.RIGHTS)
    assert any(c.causal for c in win) and any(not c.causal and c.window[0] >= 0 and c.window[1] >= 0 for c in win)
    assert {L for c in fams["plain"] if c.cap == 1024 and not c.append for L in c.lens} >= set(range(131)) | set(range(250, 263)) | set(range(505, 520)) | set(range(1010, 1025))
    assert any(L < c.sq[0] for c in fams["plain"] for L in c.lens) and any(L < c.sq[0] for c in fams["prefill"] for L in c.lens)
    assert {c.sink for c in fams["sinks"]} == {"zero", "ninf", "mixed"} and {c.splits == 1 for c in fams["sinks"]} == {False, True}
    assert any(len(c.lens) > 512 for c in fams["ragged"]) and {c.prefill for c in fams["ragged"]} == {False, True}
    assert {s for c in fams["ragged"] for s in c.sq} >= {0, 1, 2, 5, 16, 17, 40}
    assert any(c.v_scale != 1.0 for c in fams["plain"])
    for _, base, moved in V.sensitivity_pairs():
        assert [a != b for a, b in zip(V.row_sets(base), V.row_sets(moved))].count(True) >= 1


# ---- the backward probe ------------------------------------------------------------------------------------------------------------------

def pair_matrix(L, sq, causal):
    """int64 (sq, L): 1 where the model's row t sees key j, from `visible` row by row"""
    m = np.zeros((sq, max(L, 0)), dtype=np.int64)
    for t in range(sq):
        r, extras = V.visible(L, sq, t, causal)
        assert not extras
        m[t, r.start:r.stop] = 1
    return m


def pair_hists(m, d):
    """fp32 sums over one sequence's pair weights m int64 (sq, L): (sq, d) = sum over the keys row t sees of code(j), (L, d) = sum over
    the rows that see key j of code(t).  The integers stay far below 2^24: the sums are exact."""
    code = torch.from_numpy(V.bwd_code(d).copy()).float()
    w = torch.from_numpy(m).float()
    hk, hr = w @ code[: m.shape[1]], w.t() @ code[: m.shape[0]]
    assert max(float(x.max()) if x.numel() else 0.0 for x in (hk, hr)) < 2 ** 22
    return hk, hr


def emulate_bwd(c, wq, mats, call, hists=None):
    """The backward's arithmetic on pair weights: mats[i] int64 (sq_i, L_i) = how often the kernels count pair (t, j) of sequence i (the
    model: 0 / 1), wq int64 (h,) = how often each query head is counted.  fp32 sums of the integers dS = P x dP = 2 and P = 1 times the
    0 / 1 codes, one fp32 product with scale, one rounding to the output type.  -> (dQ (Rq, h, d), dK, dV (Rk, hk, d)) in the output type"""
    dt = V.torch_dtype(c.dtype)
    scale = np.float32(V.bwd_scale(c.d))
    hists = hists or [pair_hists(m, c.d) for m in mats]
    hk, hr = torch.cat([x[0] for x in hists]), torch.cat([x[1] for x in hists])
    wq = torch.from_numpy(np.asarray(wq)).float()
    cnt = wq.view(c.hk, c.ratio).sum(dim=1)
    dq = 2 * hk.unsqueeze(1) * wq.view(1, -1, 1)
    dk = 2 * hr.unsqueeze(1) * cnt.view(1, -1, 1)
    dv = hr.unsqueeze(1) * cnt.view(1, -1, 1)
    if call == "A":
        dk = torch.zeros_like(dk)
    else:
        dq = torch.zeros_like(dq)
    return (dq * scale).to(dt), (dk * scale).to(dt), dv.to(dt)


def test_rows_seeing_is_the_transpose_of_visible():
    checked = 0
    for L, sq, causal in itertools.product((0, 1, 2, 5, 9, 33, 40, 64, 65), (0, 1, 2, 5, 9, 17, 64, 70), (False, True)):
        pairs = {(t, j) for t in range(sq) for j in V.visible_set(L, sq, t, causal)}
        for j in range(-1, L + 2):
            assert set(V.rows_seeing(L, sq, j, causal)) == {t for t, jj in pairs if jj == j}, (L, sq, j, causal)
        checked += 1
    assert checked == 144


def test_backward_decoder_returns_the_model_on_every_gpu_case():
    """the emulated kernel outputs of both calls of every case, built from the brute-force pair matrix, decode to the closed forms'
    integers (which asserts the derived conditions on the real inputs), with no mismatch in integers or - at d = 64 - bits"""
    cases = V.all_bwd_gpu_cases()
    assert len(cases) > 1400
    seen, pairs, hists = set(), 0, {}
    for c, hot in cases:
        key = (c.lens, c.sq, c.causal, c.d, c.dtype, c.h, c.hk, hot)
        if key in seen:
            continue                                                            # (the same call by another route: host module, C ABI with and without a workspace)
        seen.add(key)
        for L, s in zip(c.lens, c.sq):
            if (L, s, c.causal, c.d) not in hists:
                m = pair_matrix(L, s, c.causal)
                hists[L, s, c.causal, c.d] = pair_hists(m, c.d) + (int(m.sum()),)
        mats = [hists[L, s, c.causal, c.d] for L, s in zip(c.lens, c.sq)]
        pairs += sum(x[2] for x in mats)
        wq, _ = V.bwd_head_weights(c, hot)
        for call in "AB":
            exp, rows, keys = V.expected_bwd(c, hot, call)
            grads = emulate_bwd(c, wq, None, call, hists=mats)
            assert [g.shape for g in grads] == [(len(rows), c.h, c.d), (len(keys), c.hk, c.d), (len(keys), c.hk, c.d)]
            V.assert_bwd_signature(c, hot, call, grads, exp, rows, keys)
    assert len(seen) > 700 and pairs > 10 ** 7


def test_backward_tables_cover_what_they_claim():
    cases = V.all_bwd_gpu_cases()
    for d, dtype, causal in itertools.product((64, 128), V.DTYPES, (True, False)):
        dense = V.bwd_dense_cases(d, dtype, causal)
        assert [(c.sq[0], c.lens[0]) for c, _ in dense] == V.attn_pairs(causal)
        assert {c.ratio for c, _ in dense} == {1, 4, 6} and {c.ratio for c, _ in V.bwd_dense_cases(d, dtype, causal, gqa=True)} == {4, 6}
        assert {c.hk for c, _ in V.bwd_dense_cases(d, dtype, causal, gqa=True)} == {1, 2}
        for split in (False, True):
            head = V.bwd_head_cases(d, dtype, causal, split)
            for heads in V.HEAD_SHAPES[1:] if split else V.HEAD_SHAPES:         # every head position hot, dense and packed
                for ragged in (False, True):
                    assert sorted(g for c, g in head if (c.h, c.hk) == heads and c.ragged == ragged) == list(range(heads[0]))
    # a single hot head only where the group sum would leave the decodable range; every position of the group hot where it does
    for c, hot in cases:
        if hot is None:
            assert 2 * c.ratio * V.BWD_BASE <= V.bwd_int_limit(c.dtype, c.d)
    assert [V.bwd_int_limit(t, d) for t, d in (("fp16", 64), ("bf16", 64), ("fp16", 128), ("bf16", 128))] == [2048, 256, 724, 90]
    rotated = [(c, hot) for c, hot in V.bwd_dense_cases(128, "bf16", True) if c.ratio == 6]
    assert {hot for _, hot in rotated} == set(range(6))
    assert any(s > L for c, _ in cases for L, s in zip(c.lens, c.sq)) and any(s == 0 for c, _ in cases for s in c.sq) and any(L == 0 for c, _ in cases for L in c.lens)
    for _, base, moved, _ in V.bwd_sensitivity_pairs():
        assert sum(a != b for a, b in zip(base.lens + base.sq, moved.lens + moved.sq)) == 1


def _bwd_signature(c, wq, mats):
    sig = []
    for call in "AB":
        grads = emulate_bwd(c, wq, mats, call)
        sig += [x.numpy() for x in V.decode_bwd(c, grads)]
    return sig


def _differs(a, b):
    return any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", V.DTYPES)
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("heads", V.HEAD_SHAPES)
def test_every_backward_mutation_changes_the_decoded_signature(d, dtype, heads):
    """at the largest shape of the tables, 513 x 1024 under the causal mask: what a mask, tile or head-index bug can do to the pair
    weights or to the head counts changes the decoded integers of call A or B"""
    sq, L = 513, 1024
    hot = V.bwd_hot(heads, dtype, d, 3)
    c = V.attn_case(sq, L, True, d, dtype, heads)
    wq, _ = V.bwd_head_weights(c, hot)
    m0 = pair_matrix(L, sq, True)
    base = _bwd_signature(c, wq, [m0])
    exp = [V.expected_bwd(c, hot, call)[0] for call in "AB"]
    assert not _differs(base, [x for e in exp for x in e])
    t, lim = 300, L - sq + 300                                                  # row 300 sees keys 0 .. lim
    jt = np.arange(sq)[:, None], np.arange(L)[None, :]
    muts = {}

    def mut(name, f):
        m = m0.copy()
        f(m)
        muts[name] = ([m], wq)

    mut("one pair dropped at the diagonal", lambda m: m.__setitem__((t, lim), 0))
    mut("one pair dropped at a tile seam", lambda m: m.__setitem__((256, 128), 0))
    mut("one pair added just outside the mask", lambda m: m.__setitem__((t, lim + 1), 1))
    muts["the diagonal shifted by + 1"] = ([(jt[1] <= L - sq + jt[0] + 1).astype(np.int64)], wq)
    muts["the diagonal shifted by - 1"] = ([(jt[1] <= L - sq + jt[0] - 1).astype(np.int64)], wq)
    mut("a 64-row Q tile of one 128-key block skipped", lambda m: m.__setitem__((slice(64, 128), slice(128, 256)), 0))
    mut("a 64-row Q tile of one 128-key block doubled", lambda m: m.__setitem__((slice(64, 128), slice(128, 256)), 2))
    mut("the first Q tile of a diagonal key block skipped", lambda m: m.__setitem__((slice(128, 192), slice(640, 768)), 0))     # keys 640 .. 767 are seen from row 129 on
    mut("a 128-key block skipped", lambda m: m.__setitem__((slice(None), slice(256, 384)), 0))
    mut("a 128-key block doubled", lambda m: m.__setitem__((slice(None), slice(256, 384)), 2 * m0[:, 256:384]))
    mut("a 64-key tile of one 256-row block skipped", lambda m: m.__setitem__((slice(256, 512), slice(64, 128)), 0))
    hot_heads = np.flatnonzero(wq)
    muts["a head counted twice"] = ([m0], wq + np.eye(c.h, dtype=np.int64)[hot_heads[0]])
    muts["a head omitted"] = ([m0], wq - np.eye(c.h, dtype=np.int64)[hot_heads[-1]])
    if hot is not None:
        for other in sorted({(hot + 1) % c.h, (hot + c.ratio) % c.h} - {hot}):  # a neighbour in the group, the same position of the next group
            muts[f"heads {hot} and {other} exchanged"] = ([m0], np.eye(c.h, dtype=np.int64)[other])
    for name, (mats, w) in muts.items():
        assert _differs(_bwd_signature(c, w, mats), base), f"{name} is invisible at d={d} {dtype} h={heads}"
    assert len(muts) >= 13
