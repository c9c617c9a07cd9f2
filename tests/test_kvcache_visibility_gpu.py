"""GPU: the exact set of keys every query row of flash_attn_with_kvcache sees, in every attention kernel family.

The probe of tests/_visibility.py: K = 0 makes every score exactly 0, so a row's LSE is log(number of visible keys), and V carries a
two-digit one-hot code of the key index, so out x count is the histogram of the visible keys' digits.  Both decode to integers, and every
assertion here is an integer equality with `_visibility.visible`, a model written from the README's formulas: length, causal, window_size,
tree_mask, the per-sequence sq_i of ragged calls, L_i after an append.  Memory a sequence does not own - rows at or past its length before
the append, spare pages - holds the bad code (1 in every column, K = 0): a key read from there changes the count and every column, and
an append has to overwrite exactly its rows.

One call carries a sweep of lengths in its batch dimension; the common axes (dtype, cache width, page size, num_splits, h / h_k, append)
are rotated through the cases of a family, not crossed (tests/test_visibility_cpu.py asserts every value occurs in every family).  The
tolerance tests cannot see one key in hundreds; `test_one_parameter_moved_by_one_is_seen` shows on the real kernels that this probe does.

Not covered: the backward (with uniform P, dK / dV are sums of dO / n_i over rows and do not decode to integers with this coding), the
value path (V is 0 / 1 here; tests/test_kvcache_number_formats_gpu.py), key sets that differ by a swap invisible to both digits, and
rotary, which selects no attention kernel of its own."""
import numpy as np
import pytest
import torch

import _visibility as V

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [c.name.split("/", 1)[1] for c in cases]


def _run(c, gpu):
    """dead rows need no assertion of their own: decode() maps a row to n = 0 only where O = 0 and LSE = 0 exactly"""
    n_dec, _ = V.probe_kvcache(c, gpu)
    assert n_dec.shape == (sum(c.sq), c.h)


@pytest.mark.parametrize("c", V.kv_cases("plain"), ids=_ids(V.kv_cases("plain")))
def test_plain_and_causal(gpu, c):
    """the 16-row kernels of fa_fwd_kvcache.hip: every L in 0..130, 250..262, 505..519, 1010..1024, L < sq included"""
    _run(c, gpu)


@pytest.mark.parametrize("c", V.kv_cases("window"), ids=_ids(V.kv_cases("window")))
def test_windows(gpu, c):
    """window_size: k_begin aligned down from the first row's window, the split sized from the span; lo and lim of every row take every
    residue mod 32"""
    _run(c, gpu)


@pytest.mark.parametrize("c", V.kv_cases("softcap"), ids=_ids(V.kv_cases("softcap")))
def test_softcap(gpu, c):
    """fa_fwd_kvcache_softcap.hip: the window instantiation serves plain, causal and windowed calls; the capped score stays exactly 0"""
    _run(c, gpu)


@pytest.mark.parametrize("c", V.kv_cases("sinks"), ids=_ids(V.kv_cases("sinks")))
def test_sinks(gpu, c):
    """a sink of 0.0 adds exactly one to the count, -inf nothing; unsplit calls run the sink attention kernels, split ones the plain
    kernels and the sink combine"""
    _run(c, gpu)
    if c.sink == "ninf":
        without = V.replace(c, sink=None, name=c.name + "-without")
        a, b = V.run_kvcache(c, gpu), V.run_kvcache(without, gpu)
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("c", V.kv_cases("tree"), ids=_ids(V.kv_cases("tree")))
def test_tree_masks(gpu, c):
    """fa_fwd_kvcache_tree.hip: empty, full, all 64 bits, lower triangle, bit 63 alone, the binary-heap tree, random words and a single bit
    per row at every position, at L below, at and above sq; dense and ragged"""
    _run(c, gpu)


@pytest.mark.parametrize("c", V.kv_cases("prefill"), ids=_ids(V.kv_cases("prefill")))
def test_prefill(gpu, c):
    """fa_fwd_kvcache_prefill.hip, 64-row workgroups: under causal a tile reads no key past the one its last row sees and loses none"""
    _run(c, gpu)


@pytest.mark.parametrize("c", V.kv_cases("d256"), ids=_ids(V.kv_cases("d256")))
def test_head_dim_256(gpu, c):
    """fa_fwd_kvcache_d256.hip: base 64 on the first 128 columns; the other 128 stay 0 unless a bad code is read"""
    _run(c, gpu)


@pytest.mark.parametrize("c", V.kv_cases("ragged"), ids=_ids(V.kv_cases("ragged")))
def test_ragged(gpu, c):
    """fa_fwd_kvcache_ragged.hip: sq_i in 0, 1, 2, 5, 16, 17, 40 with lengths on both sides of sq_i in one call (the compact grid), uniform
    batches (the plain grid), prefill both ways, and 520 sequences (the second round of the slot lookup's prefix sum)"""
    _run(c, gpu)


def test_tree_heap_words_match_the_library(gpu):
    from flash_attn_turing import tree_mask_from_parents

    for sq in V.TREE_SQS:
        parents = torch.tensor([[(t - 1) // 2 if t else -1 for t in range(sq)]], device=gpu)
        words = [int(x) & ((1 << 64) - 1) for x in tree_mask_from_parents(parents)[0].tolist()]
        assert tuple(words) == V.heap_words(sq)


_PAIRS = V.sensitivity_pairs()


@pytest.mark.parametrize("name,base,moved", _PAIRS, ids=[p[0].replace(" ", "_") for p in _PAIRS])
def test_one_parameter_moved_by_one_is_seen(gpu, name, base, moved):
    """At the largest lengths used, where one key moves the LSE by 1e-3 / n and no tolerance test can see it: the call with left + 1,
    right + 1, one length + 1 or one tree bit flipped decodes to the model of the MOVED parameters, and differs from the model of the
    unmoved ones on exactly the rows whose visible sets differ."""
    V.probe_kvcache(base, gpu)
    out, lse = V.run_kvcache(moved, gpu)
    n_dec, hist_dec = V.decode(out, lse, torch.tensor(moved.sink_extra()), moved.v_scale)
    n_mov, hist_mov, rows = V.expected(moved)
    V.assert_signature(moved, n_dec, hist_dec, n_mov, hist_mov, rows)
    n_base, hist_base, rows_base = V.expected(base)
    assert rows_base == rows
    differ = np.array([a != b for a, b in zip(V.row_sets(base), V.row_sets(moved))])
    assert differ.any()
    seen = (n_dec != torch.from_numpy(n_base).to(gpu).unsqueeze(1)) | (hist_dec != torch.from_numpy(hist_base).to(gpu).unsqueeze(1)).any(dim=-1)
    want = torch.from_numpy(differ).to(gpu).unsqueeze(1).expand_as(seen)
    assert torch.equal(seen, want), f"{name}: the decoded signature differs from the unmoved model on rows {seen.any(dim=1).nonzero().flatten().tolist()}, " \
                                    f"the visible sets differ on rows {np.flatnonzero(differ).tolist()}"
