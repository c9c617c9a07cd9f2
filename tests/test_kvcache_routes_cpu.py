"""CPU: the route table of tests/test_kvcache_routes_gpu.py (tests/_visibility.py route_cases) is decodable and complete.

  * every case meets the probe's derived conditions, and the decoder returns the model on it (the emulation of tests/test_visibility_cpu.py);
  * the table holds one case per leaf of the launch dispatch: per file, the distinct (dense / ragged, dtype, head_dim, layout, cache width[, mode])
    keys of the cases that must run its kernels number what that file's ISA test counts as its attention kernels - so a leaf dropped from the
    table fails here.  The counts are those tests' literals, not taken from the launch code."""
import collections

import numpy as np

import _visibility as V
from test_visibility_cpu import roundtrip

# attention kernels per file, as asserted by: test_kvcache_cpu.py / _paged_cpu.py / _window_cpu.py (8 + 8 + 8) + test_kvcache_fp8_cpu.py (24);
# test_kvcache_ragged_cpu.py (48); test_kvcache_softcap_cpu.py, _sinks_cpu.py, _tree_cpu.py (16 dense + 16 ragged each); test_kvcache_prefill_cpu.py
# (32 + 32); test_kvcache_d256_cpu.py (32)
ATTENTION_KERNELS = {"dense": 48, "ragged": 48, "softcap": 32, "sinks": 32, "tree": 32, "prefill": 64, "d256": 32}


def _all():
    return [c for f in V.ROUTE_FAMILIES for c in V.route_cases(f)]


def test_decoder_returns_the_model_on_every_route_case():
    cases = _all()
    assert len({c.name for c in cases}) == len(cases) > 600
    for k, c in enumerate(cases):
        n, hist, _ = V.expected(c)                                              # asserts check_conditions on the inputs
        for n_dec, hist_dec in roundtrip(c, n, hist, sign=1 if k % 2 else -1):
            assert np.array_equal(n_dec, n) and np.array_equal(hist_dec, hist), c.name


def test_the_shapes_are_the_ones_a_wrong_leaf_shows_at():
    for c in _all():
        assert c.cap == 96 and (c.h, c.hk) == (2, 1) and c.page in (0, 16) and c.splits in (1, 2), c.name
        assert c.append or set(c.lens) == set(V.ROUTE_LENS), c.name              # (an append of sq rows leaves L >= sq)
        want = {63, 65} if c.prefill else {1, 3} if c.ragged else {3}
        assert set(c.sq) == want if c.ragged else len(set(c.sq)) == 1 and set(c.sq) <= want, c.name
        sets = V.row_sets(c)
        assert any(sets) and (c.append or not all(sets)), c.name                # live rows, and the dead rows of L = 0


def test_one_case_per_leaf_of_every_file():
    leaves = collections.defaultdict(set)
    for c in _all():
        leaves[V.route_leaf(c)[0]].add(V.route_leaf(c))
    assert {f: len(v) for f, v in leaves.items()} == ATTENTION_KERNELS
    # ... and every leaf is run unsplit and split, where the split changes nothing about the kernel (sinks: the split call runs the kernels without them)
    for f in V.ROUTE_FAMILIES:
        by_leaf = collections.defaultdict(set)
        for c in V.route_cases(f):
            by_leaf[V.route_leaf(V.replace(c, splits=1))].add(c.splits)
        assert all(v == {1, 2} for v in by_leaf.values()), f
