"""CPU: the accuracy-budget check of tests/test_accuracy_budget_gpu.py would fail on a kernel that is subtly wrong (as tests/test_visibility_cpu.py
shows it for the visibility probe).  On the very inputs the GPU cases generate (tests/_accuracy.py builds them for both files):
  * the rounding model, taken as the "kernel", passes all three assertions - and with them the condition on the case, |gain_model| <= G / 4;
  * each mutant of the model fails at least one assertion, in both dtypes, on every case it applies to:
      P truncated instead of rounded to nearest-even; O x (1 + 2^-12) in fp16, O x (1 + 2^-9) in bf16; the softmax scale x (1 + 2^-12) (seen by
      the LSE); v_descale rounded to the 16-bit type (FP8 caches); split-merge weights rounded to the 16-bit type; the sink logit added twice
      (sink cases); one visible key of the 777-key sequence dropped.
The statistics and the model themselves are checked first, on values worked out by hand."""
import math

import numpy as np
import pytest
import torch

import _accuracy as A

DTS = ["fp16", "bf16"]
O_FACTOR = {"fp16": 2.0 ** -12, "bf16": 2.0 ** -9}
SCALE_FACTOR = 2.0 ** -12


# ---- the helper --------------------------------------------------------------------------------------------------------------------------------

def test_round16_against_torch_and_by_hand():
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(20000, generator=gen, dtype=torch.float64) * torch.exp(torch.randn(20000, generator=gen, dtype=torch.float64) * 3 - 6)       # fp16: normal and subnormal, none overflows
    for dtname, dt in A.DT.items():
        r = A.round16(x.numpy(), dtname)
        # torch rounds fp32 -> 16 bit to nearest even: on fp32 inputs (no double rounding) the two must agree to the bit
        x32 = x.float()
        assert np.array_equal(A.round16(x32.double().numpy(), dtname), x32.to(dt).double().numpy()), dtname
        t = A.round16(x.numpy(), dtname, "truncate")
        assert (np.abs(t) <= np.abs(x.numpy())).all() and (np.abs(r - x.numpy()) <= np.abs(t - x.numpy())).all(), dtname
        assert np.array_equal(A.round16(t, dtname), t), f"{dtname}: a truncated value is not a value of the type"
    # ties go to even; the subnormal grid of fp16 has step 2^-24
    assert A.round16(np.array([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -24 * 2.5, 2.0 ** -24 * 3.5]), "fp16").tolist() == [1.0, 1 + 2.0 ** -9, 2.0 ** -23, 2.0 ** -22]
    assert A.round16(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8 + 2.0 ** -30)]), "bf16").tolist() == [1.0, 1 + 2.0 ** -6, -(1 + 2.0 ** -7)]
    assert A.round16(np.array([1 + 2.0 ** -10 - 2.0 ** -30, -2.0 ** -24 * 2.9]), "fp16", "truncate").tolist() == [1.0, -2.0 ** -23]
    assert A.round16(np.array([1 + 2.0 ** -7 - 2.0 ** -30]), "bf16", "truncate").tolist() == [1.0]


def test_stats_by_hand_and_refusal():
    gen = torch.Generator().manual_seed(2)
    ref = torch.randn(64, 128, generator=gen, dtype=torch.float64)
    noise = torch.randn(64, 128, generator=gen, dtype=torch.float64)
    noise -= (noise * ref).sum() / (ref * ref).sum() * ref                   # orthogonal to ref: it adds to relrms and not to gain
    s = A.stats(ref * (1 + 2.0 ** -9) + 1e-3 * noise, ref)
    assert s["n"] == 8192 and abs(s["gain"] - 2.0 ** -9) < 1e-12
    want = math.sqrt(2.0 ** -18 + 1e-6 * float((noise * noise).sum() / (ref * ref).sum()))
    assert abs(s["relrms"] - want) < 1e-12
    live = torch.zeros(64, dtype=torch.bool)
    live[:32] = True
    x = ref.clone()
    x[32:] = 7.0                                                              # dead rows are left out
    assert A.stats(x, ref, live)["relrms"] == 0.0 and A.stats(x, ref, live)["n"] == 4096
    with pytest.raises(AssertionError):
        A.stats(ref[:31], ref[:31])
    live[0] = False
    with pytest.raises(AssertionError):
        A.stats(x, ref, live)


def test_stats_counts_only_finite_elements():
    ref = torch.ones(33, 128, dtype=torch.float64)
    x = ref.clone()
    x[0, :] = float("inf")
    assert A.stats(x, ref)["n"] == 4096
    x[1, 0] = float("nan")
    with pytest.raises(AssertionError):
        A.stats(x, ref)


def test_model_by_hand():
    """two keys, scores 0 and log(3) - M = log 3, P = (1/3, 1), l = 4/3 - and V = (1, 0), (0, 1)"""
    s = torch.tensor([[0.0, math.log(3.0)]], dtype=torch.float64)
    v = torch.eye(2, dtype=torch.float64)
    for dtname in DTS:
        om, lse, o64 = A.rounding_model(s, torch.ones(1, 2, dtype=torch.bool), v, dtname)
        p0 = float(A.round16(np.array([math.exp(-math.log(3.0))]), dtname)[0])
        assert torch.allclose(o64, torch.tensor([[0.25, 0.75]], dtype=torch.float64), atol=1e-15) and abs(float(lse) - math.log(4.0)) < 1e-15
        assert om.numpy().tolist() == [A.round16(np.array([p0 / (4.0 / 3.0), 1.0 / (4.0 / 3.0)]), dtname).tolist()]
        # the row sum of the rounded P instead
        om_r, _, _ = A.rounding_model(s, torch.ones(1, 2, dtype=torch.bool), v, dtname, rowsum="rounded")
        assert om_r.numpy().tolist() == [A.round16(np.array([p0 / (p0 + 1.0), 1.0 / (p0 + 1.0)]), dtname).tolist()]
        # a sink of log 4 doubles the denominator; a row that sees nothing is 0, 0
        om_s, lse_s, o64_s = A.rounding_model(s, torch.ones(1, 2, dtype=torch.bool), v, dtname, sink=torch.tensor([math.log(4.0)], dtype=torch.float64))
        assert torch.allclose(o64_s, torch.tensor([[0.125, 0.375]], dtype=torch.float64), atol=1e-15) and abs(float(lse_s) - math.log(8.0)) < 1e-15
        om_d, lse_d, o64_d = A.rounding_model(s, torch.zeros(1, 2, dtype=torch.bool), v, dtname)
        assert float(om_d.abs().sum()) == 0 and float(lse_d) == 0 and float(o64_d.abs().sum()) == 0
        # the merge over a key split with exact weights is the model
        gen = torch.Generator().manual_seed(3)
        s2, v2 = torch.randn(4, 7, 90, generator=gen, dtype=torch.float64), torch.randn(4, 1, 90, 16, generator=gen, dtype=torch.float64)[:, 0]
        vis2 = torch.rand(7, 90, generator=gen) < 0.8
        om2, _, _ = A.rounding_model(s2, vis2, v2, dtname)
        mm = A.merged_model(s2, vis2, v2, dtname, (0, 30, 60, 90))
        # (P is rounded against the part's own maximum there: the same values except where a part's maximum is not the row's, to rounding)
        assert float((mm - om2).abs().max()) <= 2 * A.U.ULP[dtname] * float(om2.abs().max())


def test_lse_yardstick_is_fp32_sized():
    gen = torch.Generator().manual_seed(4)
    s = torch.randn(8, 5, 777, generator=gen, dtype=torch.float64)
    y = A.lse_yardstick(s, torch.ones(5, 777, dtype=torch.bool))
    assert 0 < y < 16 * 2.0 ** -24 * math.log(777 * math.e)
    assert A.lse_yardstick(s, torch.zeros(5, 777, dtype=torch.bool)) == 0.0


# ---- the model passes, every mutant fails --------------------------------------------------------------------------------------------------------

def _as_kernel(om, lse64):
    return om, torch.from_numpy(lse64.numpy().astype(np.float32)).double()


def _check(tag, dtname, base, x, lse):
    return A.budget_entries(tag, dtname, base, x, lse)


def _rejected(tag, dtname, base, x, lse):
    with pytest.raises(AssertionError) as info:
        _check(tag, dtname, base, x, lse)
    assert "CASE is too small" not in str(info.value) and "non-finite" not in str(info.value), str(info.value)
    print("rejected:", str(info.value))


def _decode_mutants(name):
    kw = A.KVCACHE_CASES.get(name)
    muts = ["p_truncated", "o_scaled", "scale", "merge_weights"]
    if kw is not None:
        muts.append("key_dropped")
        if kw.get("fp8"):
            muts.append("v_descale")
        if kw.get("sinks"):
            muts.append("sink_twice")
    elif not A.MLA_CASES[name].get("sparse"):
        muts.append("key_dropped")
    return muts


def _mutate_groups(built, fn):
    """the model over groups changed by fn(index, group) -> keywords that replace fields of the group (the plain model of the case stays cached)"""
    import copy
    import dataclasses

    b2 = copy.copy(built)
    b2.model = None
    b2.groups = [dataclasses.replace(g, **fn(i, g)) for i, g in enumerate(built.groups)]
    m = A.model_of(b2, p_rounding="nearest")
    return m["om"], m["lse"]


@pytest.mark.parametrize("hot", A.VARIANTS, ids=["hot", "flat"])
@pytest.mark.parametrize("name", A.DECODE_NAMES)
@pytest.mark.parametrize("dtname", DTS)
def test_decode_model_passes_as_kernel(dtname, name, hot):
    built = A.decode_case(dtname, name, hot)
    base = A.model_of(built)
    assert all(g.vis.any(-1).sum() > 0 for g in built.groups)
    _check(f"{name} {'hot' if hot else 'flat'} model-as-kernel", dtname, base, *_as_kernel(base["om"], base["lse"]))


@pytest.mark.parametrize("name,mutant", [(n, m) for n in A.DECODE_NAMES for m in _decode_mutants(n)])
@pytest.mark.parametrize("dtname", DTS)
def test_decode_mutant_is_rejected(dtname, name, mutant):
    """a case is its two calls (tests/_accuracy.py kvcache_case: the appended rows at 3 x scale, and N(0, 1) like the rest): the mutant must fail
    an assertion on at least one of them, and may not owe that to the condition on the case"""
    said = []
    for hot in A.VARIANTS:
        try:
            _mutant_call(dtname, name, mutant, hot)
        except AssertionError as err:
            said.append(str(err))
    assert said, f"{name} {mutant} [{dtname}]: passes on both calls of the case"
    assert all("CASE is too small" not in m and "non-finite" not in m for m in said), said
    print("rejected:", " | ".join(said))


def _mutant_call(dtname, name, mutant, hot):
    built = A.decode_case(dtname, name, hot)
    base = A.model_of(built)
    tag = f"{name} {'hot' if hot else 'flat'} {mutant}"
    if mutant == "p_truncated":
        m = A.model_of(built, p_rounding="truncate")
        om, lse = m["om"], m["lse"]
    elif mutant == "o_scaled":
        m = A.model_of(built, o_factor=1 + O_FACTOR[dtname])
        om, lse = m["om"], m["lse"]
    elif mutant == "scale":
        f = 1 + SCALE_FACTOR
        om, lse = _mutate_groups(built, lambda i, g: dict(scores=g.scores * f if g.raw is None else g.cap * torch.tanh(g.raw * f / g.cap)))
    elif mutant == "merge_weights":
        # the keys of every sequence cut in three where its own keys are (thirds of its length; the last part takes the rest of the capacity)
        parts = []
        for g in built.groups:
            n = g.scores.shape[-1]
            parts.append(A.merged_model(g.scores, g.vis, g.v, dtname, (0, g.L // 3, 2 * g.L // 3, n), sink=g.sink, weight_dtype=dtname))
        om, lse = torch.cat([p.reshape(-1, p.shape[-1]) for p in parts]), base["lse"]
    elif mutant == "v_descale":
        vds = torch.from_numpy(A.round16(built.v_descale.double().numpy(), dtname))
        assert not torch.equal(vds, built.v_descale.double())
        om, lse = _mutate_groups(built, lambda i, g: dict(v=built.v_codes[i] * vds[i].view(-1, 1, 1, 1)))
    elif mutant == "sink_twice":
        om, lse = _mutate_groups(built, lambda i, g: dict(sink=g.sink + math.log(2.0)))
    else:
        assert mutant == "key_dropped"
        def drop(i, g):
            if g.L != 777:
                return {}
            vis = g.vis.clone()
            assert vis[:, 777 - 80].all()
            vis[:, 777 - 80] = False
            return dict(vis=vis)
        om, lse = _mutate_groups(built, drop)
    _check(tag, dtname, base, *_as_kernel(om, lse))


ATTN_IDS = [c[0] for c in A.ATTN_CASES]


# (the long case exists for the dense call: the packed batch has its own lengths)
FWD_PARAMS = [pytest.param(c, p, id=f"{c[0]}-{'packed' if p else 'dense'}") for c in A.ATTN_CASES for p in (False, True) if not (p and c[3] != A.ATTN_SQ)]


@pytest.mark.parametrize("case,packed", FWD_PARAMS)
@pytest.mark.parametrize("dtname", DTS)
def test_forward_model_and_its_mutants(dtname, case, packed):
    name, d, causal, sk = case
    c = A.attn_case(dtname, d, causal, sk, packed)
    rowsum = "rounded" if (sk > A.PP16_EXACT_KEYS and dtname == "fp16") else "exact"
    base = A.attn_forward_model(c, rowsum)
    tag = f"fwd {name} {'packed' if packed else 'dense'}"
    _check(tag + " model-as-kernel", dtname, base, *_as_kernel(base["om"], base["lse"]))
    if rowsum == "rounded":
        # O: either row sum passes against the other, the difference is far below the budget.  LSE: the yardstick of this family carries the
        # rounding noise of the packed P it sums (keys 1024 .. 1599 of 1664) - several times the fp32-sized one, and far below 2^-12
        other = A.attn_forward_model(c, "exact")
        _check(tag + " exact row sums against the rounded-sum model", dtname, base, *_as_kernel(other["om"], other["lse"]))
        assert A.pp16_rounded_keys(sk) == slice(1024, 1600) and A.pp16_rounded_keys(1024 + 2 * 64) == slice(1024, 1024)
        assert 4 * other["yard"][0] < base["yard"][0] < 2.0 ** -14, (other["yard"], base["yard"])
    trunc = A.attn_forward_model(c, rowsum, p_rounding="truncate")
    _rejected(tag + " p_truncated", dtname, base, *_as_kernel(trunc["om"], trunc["lse"]))
    scaled = A.attn_forward_model(c, rowsum, o_factor=1 + O_FACTOR[dtname])
    _rejected(tag + " o_scaled", dtname, base, *_as_kernel(scaled["om"], scaled["lse"]))


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("case", [c for c in A.ATTN_CASES if c[3] == A.ATTN_SQ], ids=ATTN_IDS[:4])
@pytest.mark.parametrize("dtname", DTS)
def test_backward_model_and_a_scaled_gradient(dtname, case, packed):
    """the C oracle in rounding mode against torch fp64 autograd: the condition on the case holds for dQ, dK and dV, the oracle passes as the
    kernel, and each exact gradient x (1 + 2^-12) / (1 + 2^-9), rounded once - a backward with no other error than that factor - is rejected"""
    name, d, causal, sk = case
    c = A.attn_case(dtname, d, causal, sk, packed)
    for t in ("dq", "dk", "dv"):
        base = A.attn_grad_base(c, t)
        tag = f"bwd {name} {'packed' if packed else 'dense'} {t}"
        A.budget_entries(tag + " model-as-kernel", dtname, base, base["om"])
        with pytest.raises(AssertionError) as info:
            A.budget_entries(tag + " scaled", dtname, base, torch.from_numpy(A.round16(base["o64"].numpy() * (1 + O_FACTOR[dtname]), dtname)))
        assert "CASE is too small" not in str(info.value)
