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
