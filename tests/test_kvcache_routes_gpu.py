"""GPU: every leaf of the decode launch dispatch runs the kernel it names (fa_kvcache_launch.hpp: kvc_dispatch, kvc_route_attn).

tests/test_kvcache_visibility_gpu.py rotates the common axes through the cases of a family; a dispatcher goes wrong in ONE leaf - the bf16 /
paged / FP8 / ragged corner of one family - so here the axes are crossed: family x dense / ragged x dtype x head_dim x layout x cache width
x num_splits, one tiny call each (tests/_visibility.py route_cases: 96 keys = three 32-key steps, h / h_k = 2 / 1, sq = 3, or 63 and 65 for
the 64-row kernels, lengths 0, 31, 33, 70, 96 in one batch).  The assertion is the probe's: the decoded set of visible keys equals the
integer model, exactly.  A leaf that lands on the kernel of another dtype, head_dim, layout or cache width reads or writes other bytes and
decodes to other integers; one that lands on another mask decodes to another set.

The probe sets K = 0, which a soft cap maps to 0: it cannot tell a soft-capped leaf from an uncapped one.  The softcap leaves therefore also
run a random-valued call whose scores lie far beyond the cap (q, k = 4 x N(0, 1), softcap 5) against the fp64 reference and the tolerances
of tests/test_kvcache_softcap_gpu.py, and the test shows that the uncapped output of any one of these calls fails that check."""
import copy

import pytest
import torch

import _util as U
import _visibility as V
from test_kvcache_d256_gpu import _page
from test_kvcache_fp8_gpu import _descale, deq, quantise
from test_kvcache_softcap_gpu import DT, assert_groups, exact, split_rows

pytestmark = pytest.mark.gpu

CAP_SOFT = 5.0


def softcap_run(c, gpu):
    """the route case c with random values: the capped and the uncapped call -> q, the logical caches as the kernels read them (CPU), out, lse of
    the capped call, out of the uncapped one"""
    import flash_attn_turing as F

    dt, b, d, cap = DT[c.dtype], len(c.lens), c.d, c.cap
    gen = torch.Generator().manual_seed(len(c.name) * 7919 + d)
    k = torch.randn(b, cap, c.hk, d, generator=gen) * 4.0
    v = torch.randn(b, cap, c.hk, d, generator=gen)
    q = (torch.randn(sum(c.sq), c.h, d, generator=gen) * 4.0).to(dt)
    kw = dict(cache_seqlens=torch.tensor(c.lens, dtype=torch.int32, device=gpu), causal=c.causal, num_splits=c.splits, return_softmax_lse=True)
    if c.fp8:
        kds, vds = _descale(b, c.hk, gen, gpu), _descale(b, c.hk, gen, gpu)
        kc, vc = quantise(k, kds).to(gpu), quantise(v, vds).to(gpu)
        k_ref, v_ref = deq(kc, kds), deq(vc, vds)
        kw.update(k_descale=kds, v_descale=vds)
    else:
        kc, vc = k.to(dt).to(gpu), v.to(dt).to(gpu)
        k_ref, v_ref = kc.cpu(), vc.cpu()
    if c.page:
        kc, vc, table = _page(kc, vc, c.page, seed=len(c.name))
        kw.update(block_table=table)
    if c.ragged:
        kw.update(cu_seqlens_q=torch.tensor([sum(c.sq[:i]) for i in range(b + 1)], dtype=torch.int32, device=gpu), max_seqlen_q=max(c.sq))
        qg = q.to(gpu)
    else:
        qg = q.view(b, c.sq[0], c.h, d).to(gpu)
    out, lse = F.flash_attn_with_kvcache(qg, kc, vc, softcap=CAP_SOFT, **kw)
    out0, _ = F.flash_attn_with_kvcache(qg, kc, vc, softcap=0.0, **kw)
    assert torch.isfinite(out).all().item() and torch.isfinite(out0).all().item(), c.name
    return q, k_ref, v_ref, out, lse, out0


def _softcap_call(c, gpu):
    """-> the parts (split_rows) of the capped call against the fp64 reference, and the same with the uncapped call's O in the place of its O"""
    q, k_ref, v_ref, out, lse, out0 = softcap_run(c, gpu)
    b, d = len(c.lens), c.d
    cu = [sum(c.sq[:i]) for i in range(b + 1)]
    parts, parts0 = [], []
    for s in sorted(set(c.sq)):                     # the sequences of one sq together: the reference takes one seqlen_q
        idx = [i for i, x in enumerate(c.sq) if x == s]
        if c.ragged:
            rows = torch.tensor([cu[i] + t for i in idx for t in range(s)])
            pick = lambda o: o[rows.to(o.device)].view(len(idx), s, c.h, d)
            q_s, o_s, o0_s, l_s = pick(q), pick(out), pick(out0), lse[:, rows.to(gpu)].view(c.h, len(idx), s).permute(1, 0, 2)
        else:
            q_s, o_s, o0_s, l_s = q.view(b, s, c.h, d), out, out0, lse
        lens = [c.lens[i] for i in idx]
        xo, xl, nvis = exact(q_s, k_ref[idx], v_ref[idx], lens, cap=CAP_SOFT, causal=c.causal)
        parts.append(split_rows(o_s, l_s, xo, xl, nvis, f"{c.name} sq{s}"))
        parts0.append(split_rows(o0_s, l_s, xo, xl, nvis, f"{c.name} sq{s} (uncapped O)"))
    return parts, parts0


def _softcap_values(cases, gpu):
    """Dead rows and the LSE are asserted per call (split_rows).  O is asserted over the calls of one (dense / ragged, dtype, head_dim) together,
    per group of rows, as tests/test_kvcache_softcap_gpu.py::test_scale_and_cap_against_fp64 asserts its five calls and for its reason: a call
    here has a few hundred elements in a group, and one element whose exact value lies within 1e-5 of zero would decide the relative mean.
    Then, call by call, the uncapped O takes the place of that call's O in its group and the same check must fail: one uncapped leaf among
    the eight is seen."""
    groups = {}
    for c in cases:
        groups.setdefault((c.ragged, c.dtype, c.d), []).append((c,) + _softcap_call(c, gpu))
    assert len(groups) * 8 == len(cases)
    for (ragged, dtype, d), items in groups.items():
        tag = f"route softcap {'ragged' if ragged else 'dense'} {dtype} d{d}"
        assert_groups([p for _, ps, _ in items for p in ps], dtype, tag)
        saved = copy.deepcopy(U.MARGINS), len(U.REL_TABLE)        # (the checks that must fail stay out of the recorded margins)
        for i, (c, _, _) in enumerate(items):
            swapped = [p for j, (_, ps, ps0) in enumerate(items) for p in (ps0 if j == i else ps)]
            with pytest.raises(AssertionError):
                assert_groups(swapped, dtype, f"{tag}, the uncapped O of {c.name}")
        U.MARGINS.clear()
        U.MARGINS.update(saved[0])
        del U.REL_TABLE[saved[1]:]


@pytest.mark.parametrize("family", V.ROUTE_FAMILIES)
def test_every_leaf_of_the_dispatch(gpu, family):
    cases = V.route_cases(family)
    for c in cases:
        n_dec, _ = V.probe_kvcache(c, gpu)
        assert n_dec.shape == (sum(c.sq), c.h)
    if "softcap" in family:
        _softcap_values(cases, gpu)
