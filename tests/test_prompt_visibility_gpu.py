"""GPU: the exact set of keys every query row of flash_attn_prefill_func (fa_fwd_prefill.hip) and flash_attn_fp8_func (fa_fwd_fp8.hip) sees.

The probe of tests/_visibility.py (THE PROMPT AND FP8 FORWARDS) on the two kernel families whose visibility logic is integer code of their
own: the prompt forward's w0 / k_lo / k_hi per 128-row tile, its descriptors that start at w0 and end at k_hi, and its wave-uniform choice
of the steps that skip the per-row compare; the FP8 forward's lim_lo and tile_key_end at 64 rows a tile and 128-key steps.  K = 0, V = the
two-digit code of the key index, the bad code behind every K / V extent.  Every assertion is the integer equality of
`_visibility.assert_signature` with the model `_visibility.visible`; there is no tolerance anywhere.  Rows without a key are exactly
O = 0, LSE = 0, under a sink of 0.0 too.

h / h_k takes 3, 5, 6 and 12 (a token's heads straddle waves, 16-row column blocks and tiles), 64 and 160 (more than a tile); packed calls
sweep L through every residue mod 32 (mod 128 for FP8) below sq, around it and up to the capacity; the dense instantiations run the
(sq, sk) pairs of the forward probe.  tests/test_visibility_cpu.py enumerates the same tables without a GPU.

Not covered: key sets that differ by a swap invisible to both digits, and the value path (V and P are 0 / 1 here;
tests/test_prefill_fwd_gpu.py and tests/test_fp8_fwd_gpu.py compare values)."""
import numpy as np
import pytest
import torch

import _visibility as V

pytestmark = pytest.mark.gpu


def _run_all(cases, gpu, tag):
    calls = sigs = 0
    for c in cases:
        n_dec, _, k = V.probe_prompt(c, gpu)
        assert n_dec.shape == (sum(c.sq) * (1 if c.ragged else V.PROMPT_BATCH), c.h)
        calls, sigs = calls + 1, sigs + k
    print(f"{tag}: {calls} calls, {sigs} (row, head) signatures")


@pytest.mark.parametrize("d,dtype", V.PROMPT_CONFIGS)
def test_prompt_forward_packed(gpu, d, dtype):
    """one packed call per case: sequences of one sq over three runs of consecutive L, an empty query and an empty key sequence among them;
    sq, h / h_k, window_size, causal and sinks rotate"""
    _run_all(V.prompt_cases(d, dtype), gpu, f"prompt packed d{d} {dtype}")


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("d,dtype", V.PROMPT_CONFIGS)
def test_prompt_forward_dense(gpu, d, dtype, half):
    """the dense instantiation: every (sq, sk) pair of the forward probe's causal table, sq > sk included, batch 2"""
    _run_all(V.prompt_dense_cases(d, dtype)[half::2], gpu, f"prompt dense d{d} {dtype} half {half}")


@pytest.mark.parametrize("part", [0, 1, 2])
@pytest.mark.parametrize("dtype,causal", V.FP8FWD_CONFIGS)
def test_fp8_forward_packed(gpu, dtype, causal, part):
    """one packed call per case: L over 0..260, 380..390, 505..519 and 1010..1024, every residue mod 128 at a step seam"""
    _run_all(V.fp8fwd_cases(dtype, causal)[part::3], gpu, f"fp8 packed {dtype} causal={causal} part {part}")


@pytest.mark.parametrize("dtype,causal", V.FP8FWD_CONFIGS)
def test_fp8_forward_dense(gpu, dtype, causal):
    """the dense instantiation over the (sq, sk) pairs of the forward probe, batch 2"""
    _run_all(V.fp8fwd_dense_cases(dtype, causal), gpu, f"fp8 dense {dtype} causal={causal}")


def test_sinks_of_minus_infinity_are_no_sinks(gpu):
    """the bits of a probe call with sinks = -inf on every head are those of the call without sinks"""
    c = next(c for c in V.prompt_cases(128, "bf16") if c.sink == "ninf")
    a, b = V.run_prompt(c, gpu), V.run_prompt(V.replace(c, sink=None), gpu)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].contiguous().view(torch.int32), b[1].contiguous().view(torch.int32))


_PAIRS = V.prompt_sensitivity_pairs()


@pytest.mark.parametrize("name,base,moved", _PAIRS, ids=[p[0].replace(" ", "_").replace(":", "") for p in _PAIRS])
def test_one_parameter_moved_by_one_is_seen(gpu, name, base, moved):
    """At the largest shapes, where one key moves the LSE by 1e-3 / n: the call with left + 1, right + 1, one L + 1 or one sq + 1 decodes
    to the model of the MOVED parameters, and differs from the model of the unmoved ones on exactly the rows whose visible sets differ
    (a row that only the moved call has is compared with nothing)."""
    V.probe_prompt(base, gpu)
    n_dec, hist_dec, _ = V.probe_prompt(moved, gpu)
    n_base, hist_base, rows_base = V.expected(base)
    rows = V.expected(moved)[2]
    at = {r: k for k, r in enumerate(rows_base)}
    both = [k for k, r in enumerate(rows) if r in at]                               # rows of the moved call that the base has too
    twin = [at[rows[k]] for k in both]
    assert len(both) == len(rows_base) and len(rows) - len(both) <= 1
    sets_base, sets_moved = V.row_sets(base), V.row_sets(moved)
    differ = np.array([sets_base[j] != sets_moved[k] for k, j in zip(both, twin)])
    assert differ.any()
    n_b, h_b = (torch.from_numpy(x[twin]).to(gpu).unsqueeze(1) for x in (n_base, hist_base))
    sel = torch.tensor(both, device=gpu)
    seen = (n_dec[sel] != n_b) | (hist_dec[sel] != h_b).any(dim=-1)
    want = torch.from_numpy(differ).to(gpu).unsqueeze(1).expand_as(seen)
    assert torch.equal(seen, want), f"{name}: the decoded signature differs from the unmoved model on rows {seen.any(dim=1).nonzero().flatten().tolist()[:20]}, " \
                                    f"the visible sets differ on rows {np.flatnonzero(differ).tolist()[:20]}"
