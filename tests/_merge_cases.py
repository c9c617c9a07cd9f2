"""The model of flash_attn_merge_states, shared by tests/test_merge_states_cpu.py and the GPU suites of the merge and of the calls built on it: the fp64
merge with the library's emptiness rule, the torch formulation the README printed before the call existed, and the error bounds."""
import numpy as np

P_BITS = {"fp16": 11, "bf16": 8}            # significand bits of the output formats: half an ulp is 2^-p relative
LSE_REL = 2.0 ** -20
WIDTHS = (64, 128, 256, 512)


def merge64(outs, lses):
    """outs[i] (..., d_v), lses[i] (...) as float64 arrays (the 16-bit / fp32 inputs widened) -> out (..., d_v), lse (...), float64.
    Part i is EMPTY for a row iff lse_i is -inf, or lse_i is +-0 and every element of that outs[i] row is +-0; an empty part contributes nothing; all parts
    empty gives out = 0, lse = 0; a NaN lse_i, or a NaN in a non-empty part's row, makes that row NaN, out and lse."""
    outs = [np.asarray(o, dtype=np.float64) for o in outs]
    lses = [np.asarray(l, dtype=np.float64) for l in lses]
    empty = [(l == -np.inf) | ((l == 0) & (o == 0).all(-1)) for o, l in zip(outs, lses)]
    with np.errstate(all="ignore"):
        live_lse = [np.where(e, -np.inf, np.where(np.isnan(l), -np.inf, l)) for e, l in zip(empty, lses)]
        m = np.max(live_lse, axis=0)
        any_live = m > -np.inf
        m0 = np.where(any_live, m, 0.0)
        w = [np.where(e, 0.0, np.exp(l - m0)) for e, l in zip(empty, lses)]
        acc = sum(np.where(e[..., None], 0.0, wi[..., None] * o) for e, wi, o in zip(empty, w, outs))
        tot = sum(w)
        out = np.where(any_live[..., None], acc / np.where(tot == 0, 1.0, tot)[..., None], 0.0)
        lse = np.where(any_live, m0 + np.log(np.where(tot == 0, 1.0, tot)), 0.0)
    nan = np.zeros(lse.shape, dtype=bool)
    for e, o, l in zip(empty, outs, lses):
        nan |= np.isnan(l) | (~e & np.isnan(o).any(-1))
    out = np.where(nan[..., None], np.nan, out)
    lse = np.where(nan, np.nan, lse)
    return out, lse


def naive_merge(o_a, lse_a, o_b, lse_b):
    """the five torch ops README.md printed for chunked prefill before flash_attn_merge_states existed, on (..., d_v) / (...) tensors: it knows no empty part"""
    import torch

    lse = torch.logaddexp(lse_a, lse_b)
    w_a, w_b = (torch.exp(l - lse).unsqueeze(-1) for l in (lse_a, lse_b))
    return w_a * o_a.double() + w_b * o_b.double(), lse


def out_bound(ref, outs, dtname):
    """|out - ref| <= 2^-p |ref| + 2^-20 max_i |o_i| (+ 2^-25 for fp16's subnormals): half an output ulp plus the fp32 evaluation"""
    big = np.max([np.abs(o) for o in outs], axis=0)
    return 2.0 ** -P_BITS[dtname] * np.abs(ref) + 2.0 ** -20 * big + (2.0 ** -25 if dtname == "fp16" else 0.0)


def lse_bound(ref):
    return LSE_REL * np.maximum(np.abs(ref), 1.0)
